"""The body-mounted actuators of a batch (mgf_batch_set_actuators, mgf_batch_actuator_count, mgf_batch_actuate, mgf_batch_actuate_dev)
without a GPU: the numpy restatement of an actuator's wrench that the GPU tests hold the kernel to is built from a rotate that equals
the oracle's mgfo_rotate_vector bit for bit, with its TORQUE and WORLD_DIR branches, and gives the fixed cases written out below; the
header, the library, the binding and the documents carry the calls; what can be refused before a device is looked at is refused there;
every refusal of mgf_batch_set_actuators precedes the first change of the rig; mgf_batch_actuate_dev looks both pointers up before it
enqueues anything; the binding turns a wrong tensor down before it calls C; the new kernel uses no scratch and spills nothing."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mgf_amd
from mgf_amd import _capi
from tests import batch_actuator_cases as AC
from tests import batch_sensor_cases as SC
from tests.util import ROOT, kernel_resources, read

CALLS = ("mgf_batch_set_actuators", "mgf_batch_actuator_count", "mgf_batch_actuate", "mgf_batch_actuate_dev")
RIG_FILE = "host_batch_actuator.inc"
f32 = np.float32


def _rig(rows):
    """ACTUATOR_DTYPE rows from (flags, gain, p, lo, d, hi)"""
    rig = np.zeros(len(rows), _capi.ACTUATOR_DTYPE)
    for i, (flags, gain, p, lo, d, hi) in enumerate(rows):
        rig[i] = (0, i, flags, gain, p, lo, d, hi)
    return rig


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_fixed_cases_of_a_wrench():
    """q = (0, 0, 0, 1), half a turn about z: rotate(q, (a, b, c)) = (-a, -b, c) exactly, so every figure below is exact in f32.
    p = (1, 0, 0) turns to r = (-1, 0, 0); d = (0, 1, 0) turns to e = (0, -1, 0)."""
    inf = np.inf
    p, d = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)
    rows = [
        # flags, gain, p, lo, d, hi                  u        L              A
        ((0, 2.0, p, -1.0, d, 1.0),                  5.0,     (0, -2, 0),    (0, 0, 2)),      # the clamp hit from above: c = 1, s = 2
        ((0, 2.0, p, -1.0, d, 1.0),                  -5.0,    (0, 2, 0),     (0, 0, -2)),     # ... from below: c = -1, s = -2
        ((0, 2.0, p, -1.0, d, 1.0),                  -inf,    (0, 2, 0),     (0, 0, -2)),     # an infinite control under a clamp is the clamp
        ((0, 2.0, p, -1.0, d, 1.0),                  0.25,    (0, -0.5, 0),  (0, 0, 0.5)),    # inside the clamp
        ((AC.WORLD_DIR, 2.0, p, -1.0, d, 1.0),       0.5,     (0, 1, 0),     (0, 0, -1)),     # d as it stands, the arm still turned
        ((AC.TORQUE, -3.0, p, -1.0, d, 1.0),         0.5,     (0, 0, 0),     (0, 1.5, 0)),    # a couple about the turned d; p not read
        ((AC.TORQUE | AC.WORLD_DIR, -3.0, p, -1.0, d, 1.0), 0.5, (0, 0, 0),  (0, -1.5, 0)),   # a couple about d as it stands
        ((0, 3.0e38, p, -inf, d, inf),               2.0,     (0, 0, 0),     (0, 0, 0)),      # gain * c overflows to infinity: skipped
        ((0, 2.0, p, -1.0, d, 1.0),                  np.nan,  (0, 0, 0),     (0, 0, 0)),      # a NaN control stays a NaN: skipped
        ((AC.TORQUE, 2.0, p, -inf, d, inf),          inf,     (0, 0, 0),     (0, 0, 0)),      # no clamp: gain * inf, skipped
        ((0, 0.0, p, -1.0, d, 1.0),                  0.5,     (0, 0, 0),     (0, 0, 0)),      # a zero gain is a zero wrench, not skipped
    ]
    rig = _rig([r[0] for r in rows])
    u = f32([r[1] for r in rows])
    q = np.tile(f32([0, 0, 0, 1]), (len(rows), 1))
    assert SC.rotate(q[:1], [p]).tolist() == [[-1.0, 0.0, 0.0]] and SC.rotate(q[:1], [d]).tolist() == [[0.0, -1.0, 0.0]]
    W, skipped = AC.wrenches(rig, u, q)
    for i, r in enumerate(rows):
        assert np.array_equal(W[i], f32(r[2] + r[3])), (i, W[i].tolist(), r[2], r[3])          # (-0.0 == 0.0: the signs of zeros are case 2's)
    assert skipped.tolist() == [False] * 7 + [True, True, True, False]
    assert np.all(np.isfinite(W))


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_restatement_of_a_wrench_is_the_oracles_rotate_vector_and_plain_f32_operations():
    """a few hundred seeded (q, d, p) through the oracle's mgfo_rotate_vector; AC.wrenches must give, bit for bit, what the header's
    lines give when written out here scalar by scalar around the ORACLE's rotated vectors: the GPU tests' reference is anchored to the
    oracle, not to itself"""
    from oracle import oracle as O
    rng = np.random.default_rng(29)
    n = 320
    q = rng.normal(0, 1, (n, 4))
    q[: n // 2] /= np.linalg.norm(q[: n // 2], axis=1, keepdims=True)
    q = q.astype(f32)
    rig = np.zeros(n, _capi.ACTUATOR_DTYPE)
    rig["body"] = np.arange(n)
    rig["flags"] = np.arange(n) % 4
    rig["gain"] = rng.uniform(-3, 3, n)
    rig["p"], rig["d"] = rng.normal(0, 1, (n, 3)), rng.normal(0, 1, (n, 3)) * rng.choice([1.0, 1e-3, 30.0], (n, 1))
    rig["d"][3::11, 1] = 1e-41                         # a denormal component
    rig["lo"], rig["hi"] = -rng.uniform(0.0, 1.0, n), rng.uniform(0.0, 1.0, n)
    rig["lo"][::5], rig["hi"][::7] = -np.inf, np.inf
    u = rng.uniform(-2, 2, n).astype(f32)
    u[::13], u[4::17] = 0.0, np.nan
    rig["gain"][6::19], rig["lo"][6::19], rig["hi"][6::19], u[6::19] = 3.0e38, -np.inf, np.inf, 1.75
    lib = O.lib()

    def oracle_rotate(v):
        want = np.empty_like(v)
        for i in range(n):
            out = O.Vec3()
            lib.mgfo_rotate_vector(C.byref(O.Quat(*q[i].tolist())), C.byref(O.Vec3(*v[i].tolist())), C.byref(out))
            want[i] = (out.x, out.y, out.z)
        return want
    rd, rp = oracle_rotate(rig["d"]), oracle_rotate(rig["p"])
    assert SC.rotate(q, rig["d"]).tobytes() == rd.tobytes() and SC.rotate(q, rig["p"]).tobytes() == rp.tobytes()
    want, want_skipped = np.zeros((n, 6), f32), np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for i in range(n):
            c = u[i]
            if c < rig["lo"][i]:
                c = rig["lo"][i]
            if c > rig["hi"][i]:
                c = rig["hi"][i]
            s = f32(rig["gain"][i] * c)
            e = rig["d"][i] if rig["flags"][i] & AC.WORLD_DIR else rd[i]
            if rig["flags"][i] & AC.TORQUE:
                L, A = f32([0, 0, 0]), f32([e[0] * s, e[1] * s, e[2] * s])
            else:
                L, r = f32([e[0] * s, e[1] * s, e[2] * s]), rp[i]
                A = f32([f32(r[1] * L[2]) - f32(r[2] * L[1]), f32(r[2] * L[0]) - f32(r[0] * L[2]), f32(r[0] * L[1]) - f32(r[1] * L[0])])
            if not np.isfinite(s):
                L, A, want_skipped[i] = f32([0, 0, 0]), f32([0, 0, 0]), True
            want[i, 0:3], want[i, 3:6] = L, A
    W, skipped = AC.wrenches(rig, u, q)
    assert skipped.tolist() == want_skipped.tolist() and 30 <= int(skipped.sum()) <= 60
    assert W.tobytes() == want.tobytes(), [i for i in range(n) if W[i].tobytes() != want[i].tobytes()][:8]
    live = ~skipped
    for fl in range(4):
        assert np.any(W[live & (rig["flags"] == fl)] != 0), fl
    assert np.any(u[live] < rig["lo"][live]) and np.any(u[live] > rig["hi"][live])               # both clamps bite
    # the force mode's restated adds: a body's records in array order, one rounded add each
    world, body = np.zeros(6, np.int32), np.int32([2, 0, 2, 1, 2, 0])
    before = dict(force=np.tile(f32([0.0, -9.8, 0.0]), (6, 1)), torque=np.zeros((6, 3), f32))
    uw, ub, F, T = AC.forces_expected(before, world, body, W[:6])
    assert ub.tolist() == [2, 0, 1] and uw.tolist() == [0, 0, 0]
    assert F[0].tobytes() == (((before["force"][0] + W[0, :3]) + W[2, :3]) + W[4, :3]).astype(f32).tobytes()
    assert T[1].tobytes() == ((before["torque"][1] + W[1, 3:]) + W[5, 3:]).astype(f32).tobytes()


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_header_library_binding_and_documents_carry_the_calls():
    h = read("include", "mgf_hip.h")
    for sig in (r"mgf_status mgf_batch_set_actuators\(mgf_batch\* b, const mgf_batch_actuator\* a, int64_t n\);",
                r"int64_t\s+mgf_batch_actuator_count\(const mgf_batch\* b\);",
                r"mgf_status mgf_batch_actuate\(mgf_batch\* b, const float\* u, int64_t n, int32_t mode, float\* wrench_out\);",
                r"mgf_status mgf_batch_actuate_dev\(mgf_batch\* b, const float\* u_dev, int64_t n, int32_t mode, float\* wrench_out_dev\);"):
        assert re.search(r"MGF_API " + sig, h), sig
    assert h.index("mgf_batch_cast_feelers_dev(") < h.index("typedef struct mgf_batch_actuator") < h.index("mgf_batch_counter(")   # behind the feelers
    for name, value in (("MGF_ACTUATOR_TORQUE", _capi.ACTUATOR_TORQUE), ("MGF_ACTUATOR_WORLD_DIR", _capi.ACTUATOR_WORLD_DIR),
                        ("MGF_ACTUATE_IMPULSE", _capi.ACTUATE_IMPULSE), ("MGF_ACTUATE_FORCE", _capi.ACTUATE_FORCE),
                        ("MGF_BATCH_ACTUATOR_LAUNCHES", _capi.BATCH_ACTUATOR_LAUNCHES)):
        m = re.search(r"#define %s\s+(\d+)" % name, h)
        assert m and int(m.group(1)) == value, name
    assert (_capi.ACTUATOR_TORQUE, _capi.ACTUATOR_WORLD_DIR, _capi.ACTUATE_IMPULSE, _capi.ACTUATE_FORCE) == (1, 2, 0, 1) == (AC.TORQUE, AC.WORLD_DIR, AC.IMPULSE, AC.FORCE)
    assert _capi.BATCH_ACTUATOR_LAUNCHES == 1
    section = h[h.index("body-mounted actuators"):]
    for word in ("c = u[i];  if (c < lo) c = lo;  if (c > hi) c = hi;", "a NaN stays a NaN", "s = gain * c", "e = WORLD_DIR ? d : rotate(q, d)",
                 "A = cross(r, L)", "a.y*b.z - a.z*b.y", "actuators_skipped", "bit for bit", "ACCUMULATE", "mgf_batch_set_forces_dev",
                 "v = v + L * inv_mass", "omega = omega + I * A", "force = force + L", "torque = torque + A", "untouched to the bit",
                 "several components", "drive_launches", "the rig was not changed", "nothing enqueued", "mgf_batch_add_bodies",
                 "not a prefix", "no float atomic", "AT ONCE"):
        assert word in section, word
    # what the header said before stands: the drive section still lists impulses at a point as out of its scope
    drive = h[:h.index("body-mounted actuators")]
    assert "impulses at a point" in drive
    # the record: 48 bytes, the same fields at the same offsets in the ctypes struct and the numpy dtype
    assert C.sizeof(_capi.BatchActuator) == 48 == _capi.ACTUATOR_DTYPE.itemsize
    names = ["world", "body", "flags", "gain", "p", "lo", "d", "hi"]
    assert [f[0] for f in _capi.BatchActuator._fields_] == list(_capi.ACTUATOR_DTYPE.names) == names
    want_off = [0, 4, 8, 12, 16, 28, 32, 44]
    assert [_capi.ACTUATOR_DTYPE.fields[k][1] for k in names] == want_off == [getattr(_capi.BatchActuator, k).offset for k in names]
    assert re.search(r"typedef struct mgf_batch_actuator \{\s*int32_t world, body; uint32_t flags; float gain;\s*mgf_vec3 p; float lo;\s*mgf_vec3 d; float hi;\s*\} mgf_batch_actuator;", h)
    lib = mgf_amd.load_library()
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    want = {"mgf_batch_set_actuators": (i32, [vp, vp, i64]), "mgf_batch_actuator_count": (i64, [vp]),
            "mgf_batch_actuate": (i32, [vp, vp, i64, i32, vp]), "mgf_batch_actuate_dev": (i32, [vp, vp, i64, i32, vp])}
    for name in CALLS:
        assert name in _capi.SYMBOLS, name
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == want[name], name
    for method in ("set_actuators", "actuator_count", "actuate", "actuate_dev"):
        assert callable(getattr(mgf_amd.WorldBatch, method)), method
    for name in ("ACTUATOR_DTYPE", "ACTUATOR_TORQUE", "ACTUATOR_WORLD_DIR", "ACTUATE_IMPULSE", "ACTUATE_FORCE", "BATCH_ACTUATOR_LAUNCHES"):
        assert getattr(mgf_amd, name) is getattr(_capi, name), name
    flat = re.sub(r"\s+", " ", read("INTEGRATION.md"))
    for sig in ("pub fn mgf_batch_set_actuators(b: *mut mgf_batch, a: *const mgf_batch_actuator, n: i64) -> mgf_status;",
                "pub fn mgf_batch_actuator_count(b: *const mgf_batch) -> i64;",
                "pub fn mgf_batch_actuate(b: *mut mgf_batch, u: *const f32, n: i64, mode: i32, wrench_out: *mut f32) -> mgf_status;",
                "pub fn mgf_batch_actuate_dev(b: *mut mgf_batch, u_dev: *const f32, n: i64, mode: i32, wrench_out_dev: *mut f32) -> mgf_status;",
                "pub struct mgf_batch_actuator { pub world: i32, pub body: i32, pub flags: u32, pub gain: f32, pub p: mgf_vec3, pub lo: f32, pub d: mgf_vec3, pub hi: f32 }",
                "pub const MGF_ACTUATOR_TORQUE: u32 = 1;", "pub const MGF_ACTUATOR_WORLD_DIR: u32 = 2;", "pub const MGF_ACTUATE_IMPULSE: i32 = 0;",
                "pub const MGF_ACTUATE_FORCE: i32 = 1;", "pub fn set_actuators(", "pub fn actuator_count(", "pub fn actuate(", "pub unsafe fn actuate_dev("):
        assert sig in flat, sig
    kernels = read("mgf_amd", "csrc", "kernels.h")
    assert kernels.index('#include "k_batch_feeler.h"') < kernels.index('#include "k_batch_actuator.h"') and "k_batch_actuate<MODE, OUT> (k_batch_actuator.h)" in kernels
    hip = read("mgf_amd", "csrc", "mgf_hip.hip")
    assert hip.index('#include "host_batch_feeler.inc"') < hip.index('#include "host_batch_actuator.inc"')
    design = read("DESIGN.md")
    assert design.index("Body-mounted feelers") < design.index("Body-mounted actuators")
    sub = design[design.index("Body-mounted actuators"):]
    for word in ("k_batch_actuate", "A = cross(r, L)", "Out of scope", "batch_actuator_bench.py", "Compiler output", "MGF_BATCH_ACTUATOR_LAUNCHES", "__any"):
        assert word in sub, word
    readme = read("README.md")
    assert "set_actuators" in readme and "actuate_dev" in readme
    assert os.path.exists(os.path.join(ROOT, "tools", "batch_actuator_bench.py"))


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def test_what_needs_no_device_is_refused_before_the_handle_is_dereferenced():
    lib = mgf_amd.load_library()
    INV = _capi.ERR_INVALID

    def err():
        return lib.mgf_last_error().decode()
    fake = C.c_void_p(16)   # a handle that is never dereferenced; addresses that are never looked up
    rig = np.zeros(4, _capi.ACTUATOR_DTYPE)
    u, out = C.c_void_p(1 << 20), C.c_void_p(1 << 21)
    assert lib.mgf_batch_actuator_count(None) == -1
    assert lib.mgf_batch_set_actuators(None, rig.ctypes.data, 4) == INV and "NULL" in err()
    assert lib.mgf_batch_set_actuators(None, None, 0) == INV and "NULL" in err()
    assert lib.mgf_batch_set_actuators(fake, None, 4) == INV and "NULL" in err()
    assert lib.mgf_batch_set_actuators(fake, rig.ctypes.data, -1) == INV and "negative" in err()
    assert lib.mgf_batch_set_actuators(fake, rig.ctypes.data, -(1 << 40)) == INV and "negative" in err()
    assert lib.mgf_batch_set_actuators(fake, rig.ctypes.data, 1 << 31) == INV and "too many" in err()
    for fn in (lib.mgf_batch_actuate, lib.mgf_batch_actuate_dev):
        for mode in (0, 1, 2):
            assert fn(None, u, 4, mode, out) == INV and "NULL" in err()                      # the handle first, whatever the rest
            assert fn(None, None, -1, mode, None) == INV and "NULL" in err()
        assert fn(fake, u, -1, 0, out) == INV and "negative" in err()
        assert fn(fake, u, -1, 7, out) == INV and "negative" in err()                        # n ahead of the mode
        assert fn(fake, None, -(1 << 40), 1, None) == INV and "negative" in err()
        for mode in (2, -1, 1 << 20):
            assert fn(fake, u, 4, mode, out) == INV and "mode" in err(), mode
            assert fn(fake, None, 0, mode, None) == INV and "mode" in err(), mode
    # what needs the handle is refused on the host too, every record ahead of any change of the rig and of any device work (read
    # here; run in tests/test_gpu_world_batch_actuators.py, where a handle exists)
    src = read("mgf_amd", "csrc", RIG_FILE)
    body = src[src.index('extern "C" mgf_status mgf_batch_set_actuators('):src.index('extern "C" int64_t mgf_batch_actuator_count(')]
    plan_call = "batch_actuator_plan(b->actuators, a, n);"
    assert not re.search(r"b->actuators\.|\bR\.", body.replace(plan_call, ""))               # the rig changes in the plan step alone
    plan = src[src.index("static void batch_actuator_plan("):src.index('extern "C" mgf_status mgf_batch_set_actuators(')]
    body = body[:body.index(plan_call)] + plan + body[body.index(plan_call) + len(plan_call):]
    first_change = min(body.index(s) for s in ("R.recs.assign(", "R.items.swap(", "R.order.swap(", "R.stale = true;"))
    assert first_change == body.index("R.recs.assign(")
    order = [body.index(s) for s in ("batch_rig_set_args(b, a, n_in)", 'batch_rig_ref_check(b, a[i].world, a[i].body, 0, "actuator")',
                                     "an actuator's flags hold a bit beyond MGF_ACTUATOR_WORLD_DIR: the rig was not changed",
                                     "an actuator's p, d or gain is not finite: the rig was not changed",
                                     "an actuator's lo or hi is a NaN, or lo > hi: the rig was not changed")]
    assert order == sorted(order) and max(order) < first_change, order
    assert body.count("the rig was not changed") == 3
    assert "std::stable_sort(" in plan and plan.index("std::stable_sort(") < plan.index("R.recs.assign(")    # a body's actuators keep the caller's order
    assert not re.search(r"<<<|Async|hipMalloc|\.ensure\(|h2d\(", body)                      # no device work at all
    args = src[src.index("static mgf_status batch_actuator_args("):src.index('extern "C" mgf_status mgf_batch_actuate(')]
    order = [args.index(s) for s in ("batch_rig_handle(b)", '"n is negative"', "mode != MGF_ACTUATE_IMPULSE && mode != MGF_ACTUATE_FORCE",
                                     "(uint64_t)n != (uint64_t)*count", "*count && !u")]
    assert order == sorted(order), order
    assert "ctx_bind" not in args and "<<<" not in args


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_both_pointers_are_looked_up_before_the_first_enqueue_and_the_kernel_has_one_exit():
    src = read("mgf_amd", "csrc", RIG_FILE)
    run = src[src.index('extern "C" mgf_status mgf_batch_actuate_dev('):]
    enqueue = r"batch_actuator_run\(|batch_rig_up\(|batch_rig_upload\(|batch_push\(|hipMemsetAsync|hipMemcpyAsync|<<<|\.ensure\(|h2d\("
    first_enqueue = min(m.start() for m in re.finditer(enqueue, run))
    checks = [m.start() for m in re.finditer(r"dev_span\(", run)]
    assert len(checks) == 2 and max(checks) < first_enqueue
    for name in ("u_dev, 4 \\* n", "wrench_out_dev, 24 \\* n"):
        assert re.search(r"dev_span\(b->ctx, " + name, run), name
    assert run.index('arrays[2] = {{wrench_out_dev, 24 * n, "wrench_out_dev"}, {u_dev, 4 * n, "u_dev"}};') < run.index("dev_outputs_overlap(arrays, 2, 1)")
    assert max(checks) < run.index("dev_outputs_overlap(") < first_enqueue
    assert run.index("batch_actuator_args(") < run.index("ctx_bind(") < min(checks)
    assert run.index("if (n == 0) return MGF_OK;") < first_enqueue                            # an empty rig enqueues nothing
    assert "hipStreamSynchronize" not in run and "hipMemcpy" not in run                      # it waits for nothing
    host_form = src[src.index('extern "C" mgf_status mgf_batch_actuate('):src.index('extern "C" mgf_status mgf_batch_actuate_dev(')]
    assert host_form.count("hipStreamSynchronize") == 1 and host_form.count("hipMemcpyHostToDevice") == 1 and host_form.count("hipMemcpyDeviceToHost") == 1
    assert host_form.index("if (n == 0) return MGF_OK;") < host_form.index(".ensure(")
    # everything that launches is batch_actuator_run: ONE launch whatever the mode, counted among the drive calls'; the rig through the
    # shared upload; no part check - actuators read no shapes
    helper = src[src.index("static mgf_status batch_actuator_run("):src.index("static mgf_status batch_actuator_args(")]
    assert helper.count("<<<") == 4 and len(re.findall(r"k_batch_actuate<ACTUATE_(?:IMPULSE|FORCE), (?:true|false)><<<", helper)) == 4
    assert helper.count("LAUNCH_CHECK();") == 1 and "b->d_launches += MGF_BATCH_ACTUATOR_LAUNCHES;" in helper
    assert "hipStreamSynchronize" not in helper and "hipMemcpy" not in helper
    assert helper.index("batch_push(") < helper.index('batch_rig_up(b, R, "actuator", 3)') < helper.index("k_batch_actuate<")
    assert "batch_single_parts(" not in src
    # what tests/test_world_batch_rigs_host.py asks of a rig file
    assert src.count("batch_rig_set_args(b, ") == 1 and src.count("batch_rig_up(b, R, ") == 1
    for gone in ("BatchQueryPlan plan(", "batch_rig_upload(", "names a body its world does not hold", '"batch is NULL"'):
        assert gone not in src, gone
    for fn in ("batch_rig_set_args", "batch_rig_ref_check", "batch_rig_plan", "batch_rig_upload", "batch_rig_up", "batch_rig_handle", "batch_rig_cap", "batch_rig_fits"):
        assert not re.search(r"^static \w+ " + fn + r"\(", src, re.M), fn
    host = read("mgf_amd", "csrc", "host_batch.inc")
    stale = host[host.index("static void batch_rigs_stale("):host.index('extern "C" mgf_status mgf_batch_add_bodies(')]
    assert host.count("BatchRig<mgf_batch_actuator> actuators;") == 1 and "b->actuators.stale = true;" in stale
    for add in ('extern "C" mgf_status mgf_batch_add_bodies(', 'extern "C" mgf_status mgf_batch_add_compound_bodies('):
        text = host[host.index(add):]
        assert "batch_rigs_stale(b);" in text[:text.index("\n}\n")], add
    assert '"actuators_skipped"' in host[host.index('extern "C" mgf_status mgf_batch_counter('):]
    # the kernel: one lane a run; the walk is a loop the whole wave leaves together, and nothing leaves the kernel ahead of it; no
    # float atomic (the one atomic is the 64-bit counter of skipped actuators); its name is off the query prefix
    k = read("mgf_amd", "csrc", "k_batch_actuator.h")
    body = k[k.index("void k_batch_actuate("):]
    body = body[:body.index("\n}\n")]
    assert body.count("return;") == 1 and body.index("__any(j < cnt)") < body.index("if (j < cnt)") < body.index("if (!live) return;")
    assert "__syncthreads" not in body and "break" not in body and "continue" not in body
    assert re.findall(r"atomic\w*\(", body) == ["atomicAdd("] and "atomicAdd(A.skipped, (unsigned long long)n_skip)" in body
    assert "lin + L * inv_mass" in body and "ang + I * T" in body and "lin + L;" in body and "ang + T;" in body
    assert len(re.findall(r"__global__ __launch_bounds__\(kBatchBlock\)", k)) == len(re.findall(r"__global__", k)) == 1
    assert not re.search(r"void k_batch_query_\w+\(", k)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_binding_turns_a_wrong_tensor_down_before_it_calls_c():
    import torch

    class Handle(mgf_amd.WorldBatch):   # no context, no C handle: a call that got as far as C would fail differently
        def __init__(self):
            self._h, self.n_worlds = None, 2

        def actuator_count(self):
            return 4

    b, n = Handle(), 4
    wrong_u = [torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.int32), torch.zeros(2 * n, dtype=torch.float32)[::2],
               torch.zeros(n - 1, dtype=torch.float32), torch.zeros((n, 2), dtype=torch.float32)]
    wrong_out = [torch.zeros((n, 6), dtype=torch.float64), torch.zeros((n, 6), dtype=torch.int32), torch.zeros((6, n), dtype=torch.float32).t(),
                 torch.zeros((n - 1, 6), dtype=torch.float32), torch.zeros((n, 5), dtype=torch.float32)]
    for t in wrong_u:
        with pytest.raises(ValueError) as e:
            b.actuate_dev(t, wrenches_out=1 << 21)
        assert "on cpu" not in str(e.value), str(e.value)              # turned down for what it is, not for where it is
    for t in wrong_out:
        with pytest.raises(ValueError) as e:
            b.actuate_dev(1 << 20, wrenches_out=t)
        assert "on cpu" not in str(e.value), str(e.value)
    with pytest.raises(ValueError, match="on cpu"):                     # everything right but the device
        b.actuate_dev(torch.zeros(n, dtype=torch.float32))
    with pytest.raises(ValueError, match="on cpu"):
        b.actuate_dev(1 << 20, wrenches_out=torch.zeros((n, 6), dtype=torch.float32))
    with pytest.raises(ValueError, match="required"):
        b.actuate_dev(None)
    with pytest.raises(ValueError, match="not ndarray"):
        b.actuate_dev(np.zeros(n, np.float32))
    with pytest.raises(mgf_amd.MgfError):                               # and a call whose arguments are all in order does reach C
        b.actuate_dev(1 << 20, _capi.ACTUATE_FORCE, wrenches_out=1 << 21)
    with pytest.raises(mgf_amd.MgfError):
        b.actuate(np.zeros(n, np.float32), _capi.ACTUATE_IMPULSE, wrenches=True)
    with pytest.raises(ValueError):
        b.actuate(np.zeros(n - 1, np.float32))                          # neither one nor n
    # set_actuators broadcasts scalars and single rows; what reaches C is ACTUATOR_DTYPE rows (no handle: C refuses, after the marshalling)
    with pytest.raises(mgf_amd.MgfError):
        b.set_actuators([0, 1, 1], 0, p=(0, 0, 0.5), d=[(0, 0, 1), (0, 1, 0), (1, 0, 0)], gain=2.0, lo=-1.0, hi=[1.0, 2.0, 3.0], world_dir=[True, False, True])
    with pytest.raises(mgf_amd.MgfError):
        b.set_actuators([0, 1], [0, 0], d=(0, 1, 0), torque=True)
    with pytest.raises(ValueError):
        b.set_actuators([0, 1, 1], [0, 1], d=(0, 0, 1))                 # neither one nor n


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_new_kernel_uses_no_scratch_and_spills_nothing():
    if not os.path.exists(os.path.join(ROOT, "mgf_amd", "libmgf_hip.so")) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    rows = kernel_resources("k_batch_actuate")
    assert set(rows) == {"k_batch_actuate<0, false>", "k_batch_actuate<0, true>", "k_batch_actuate<1, false>", "k_batch_actuate<1, true>"}, sorted(rows)
    design = re.sub(r"\s+", " ", read("DESIGN.md"))
    for name, v in sorted(rows.items()):
        print(name, ": vgpr, sgpr, scratch, static lds, sgpr spills, vgpr spills =", v)
        assert v[2] == "0" and v[4] == "0" and v[5] == "0", (name, v)    # no scratch, no spills
        assert "`%s` %s / %s / 0 / 0 / 0" % (name, v[0], v[1]) in design, (name, v)


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_rig_holds_what_the_gpu_tests_ask_of_it():
    """from the scenes alone: worlds of 8 to 64 bodies; worlds with 257, 0 and 1 actuators; four actuators on one body with other
    bodies' between them; every flag word; a zero control, gains of both signs, both clamps biting, three planted skips; the added
    bodies carry actuators"""
    scs = AC.actuator_scenes()
    lens = [len(sc["comps"]) for sc in scs]
    assert lens == [48, 8, 18, 64, 8]
    assert scs[AC.FIELD_WORLD]["terrain"] is not None and set(scs[AC.FIELD_WORLD]["comps"]["tag"].tolist()) == {1}
    lens[AC.LATE_WORLD] += AC.LATE_BODIES
    rig, u, planted = AC.main_rig(lens)
    n = len(rig)
    assert 400 <= n <= 500 and np.any(np.diff(rig["world"]) < 0)
    assert np.bincount(rig["world"], minlength=5)[:3].tolist() == list(AC.COUNTS)
    assert np.all(rig["body"] >= 0) and np.all(rig["body"] < np.int64(lens)[rig["world"]])
    four = np.flatnonzero((rig["world"] == AC.FOUR_ON[0]) & (rig["body"] == AC.FOUR_ON[1]))
    assert len(four) == 4 and np.all(np.diff(four) > 50) and rig["flags"][four].tolist() == [0, 1, 2, 3]
    late = rig["body"][rig["world"] == AC.LATE_WORLD]
    assert {lens[AC.LATE_WORLD] - 1, lens[AC.LATE_WORLD] - 2} <= set(late.tolist())
    assert set(rig["flags"].tolist()) == {0, 1, 2, 3} and np.any(rig["gain"] < 0) and np.any(rig["gain"] > 0)
    assert np.any(u == 0) and np.any(u < rig["lo"]) and np.any(u > rig["hi"]) and np.any(np.isinf(rig["lo"])) and np.any(np.isfinite(rig["lo"]))
    assert np.all(np.isfinite(rig["p"])) and np.all(np.isfinite(rig["d"])) and np.all(np.isfinite(rig["gain"])) and np.all(rig["lo"] <= rig["hi"])
    q = np.tile(f32([0.5, 0.5, -0.5, 0.5]), (n, 1))
    W, skipped = AC.wrenches(rig, u, q)
    assert sorted(np.flatnonzero(skipped).tolist()) == sorted(planted) and len(set(planted)) == 3
    assert np.all(W[skipped] == 0) and np.all(np.isfinite(W))
    drig, du = AC.dumbbell_rig(22)
    assert len(drig) == len(du) == 40 and set(drig["flags"].tolist()) == {0, 1, 2, 3} and np.all(drig["body"] < 22)
