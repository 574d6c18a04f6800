"""The box zones of a batch (mgf_batch_set_zones, mgf_batch_zone_count, mgf_batch_read_zones, mgf_batch_read_zones_dev,
mgf_batch_overlap_first_dev) without a GPU: the numpy restatement the GPU tests hold the kernel to equals float64 where every operation
is exact, and hand-checked corners; the header, the library, the binding and the documents carry the calls and the struct; what can be
refused before a device is looked at is refused there; both device forms look every pointer up before they enqueue anything; the binding
turns a wrong tensor down before it calls C; the new kernel uses no scratch and no static LDS and keeps the figures DESIGN.md records
(the plan of a rig and the query kernels' figures: tests/test_world_batch_rigs_host.py); and, by the oracle's box test, the scenes of the GPU
tests hold the cases those tests are for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mgf_amd
from mgf_amd import _capi
from tests import batch_query_device_cases as QD
from tests import batch_rig_cases as RC
from tests import batch_zone_cases as ZC
from tests.util import ROOT, kernel_resources, read

CALLS = ("mgf_batch_set_zones", "mgf_batch_zone_count", "mgf_batch_read_zones", "mgf_batch_read_zones_dev", "mgf_batch_overlap_first_dev")
f32 = np.float32


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
def _rig(rows):
    return np.array([(w, b, p, r, fl, 0) for w, b, p, r, fl in rows], _capi.ZONE_DTYPE)


def test_the_restated_centre_equals_float64_where_every_operation_is_exact_and_hand_checked_corners():
    # quaternions whose every product with a small dyadic vector is exact in f32: the identity, the half turns about the axes, the
    # third of a turn about (1, 1, 1) - (x, y, z) -> (z, x, y) - and a quaternion of length 2 (taken as given, not normalised)
    quats = {"identity": (1, 0, 0, 0), "half turn x": (0, 1, 0, 0), "half turn y": (0, 0, 1, 0), "half turn z": (0, 0, 0, 1),
             "third turn": (0.5, 0.5, 0.5, 0.5), "length two": (2, 0, 0, 0)}
    want = {"identity": (1, 2, 3), "half turn x": (1, -2, -3), "half turn y": (-1, 2, -3), "half turn z": (-1, -2, 3), "third turn": (3, 1, 2),
            "length two": (1, 2, 3)}
    # (length two: tmp = r * 2, v x tmp = 0: the result is r - the formula is not a sandwich product, and the restatement keeps it so)
    x = f32([[10.0, 20.0, 30.0]])
    state = dict(x=np.repeat(x, len(quats), axis=0), q=f32(list(quats.values())))
    rig = _rig([(0, i, (1.0, 2.0, 3.0), (0.5, 0.25, 4.0), 0) for i in range(len(quats))])
    got = ZC.boxes(rig, state, [len(quats)])
    for i, name in enumerate(quats):
        assert got[i, :3].tolist() == (np.float64(x[0]) + np.float64(want[name])).tolist(), (name, got[i])
        assert got[i, 3:].tolist() == [0.5, 0.25, 4.0]
    # against the same formula in float64, over dyadic inputs for which neither precision rounds
    rng = np.random.default_rng(3)
    n = 64
    q = rng.choice([0.0, 0.5, -0.5, 1.0, -1.0], (n, 4))
    p = rng.integers(-8, 9, (n, 3)) / 4.0
    xs = rng.integers(-64, 65, (n, 3)) / 2.0
    s, v = q[:, 0:1], q[:, 1:4]
    ref = xs + np.cross(v, np.cross(v, p) + p * s) * 2.0 + p
    rig = _rig([(0, i, tuple(p[i]), (1.0, 1.0, 1.0), 0) for i in range(n)])
    got = ZC.boxes(rig, dict(x=xs.astype(f32), q=q.astype(f32)), [n])
    assert got.dtype == f32 and np.array_equal(got[:, :3].astype(np.float64), ref)
    # in a batch of several worlds the body is found behind its world's offset; a zone fixed in the world is p as given, to the bit
    lengths = [2, 0, 3]
    state = dict(x=f32(np.arange(15).reshape(5, 3)), q=np.tile(f32([0, 1, 0, 0]), (5, 1)))
    nan = np.float32(np.nan)
    rig = _rig([(2, 1, (1.0, 1.0, 1.0), (1, 1, 1), 1), (0, 1, (1.0, 1.0, 1.0), (1, 1, 1), 0), (1, -1, (7.0, nan, -0.0), (-1.0, nan, 2.0), 0),
                (2, -1, (0.5, 0.25, 0.125), (3, 3, 3), 0)])
    got = ZC.boxes(rig, state, lengths)
    assert got[0, :3].tolist() == [9 + 1, 10 - 1, 11 - 1] and got[1, :3].tolist() == [3 + 1, 4 - 1, 5 - 1]
    assert got[2].tobytes() == f32([7.0, nan, -0.0, -1.0, nan, 2.0]).tobytes() and got[3].tolist() == [0.5, 0.25, 0.125, 3, 3, 3]
    assert ZC.ignore_of(rig).tolist() == [1, -1, -1, -1]
    # the record: the full count, the first k ascending, -1 behind them
    assert ZC.record([2, 5, 9], 0).tolist() == [3] and ZC.record([2, 5, 9], 2).tolist() == [3, 2, 5]
    assert ZC.record([2, 5, 9], 3).tolist() == [3, 2, 5, 9] and ZC.record([2, 5, 9], 5).tolist() == [3, 2, 5, 9, -1, -1]
    assert ZC.record([], 2).tolist() == [0, -1, -1]
    recs = ZC.records([0, 3, 3, 5], [1, 2, 4, 0, 7], [2, -1, 9], 2)
    assert recs.tolist() == [[2, 1, 4], [0, -1, -1], [2, 0, 7]] and recs.dtype == np.int32


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def test_header_library_binding_and_documents_carry_the_calls_and_the_struct():
    h = read("include", "mgf_hip.h")
    for sig in (r"mgf_status mgf_batch_set_zones\(mgf_batch\* b, const mgf_batch_zone\* z, int64_t n\);",
                r"int64_t mgf_batch_zone_count\(const mgf_batch\* b\);",
                r"mgf_status mgf_batch_read_zones\(mgf_batch\* b, int32_t k, int32_t\* out, mgf_aabb\* boxes_out, int64_t cap\);",
                r"mgf_status mgf_batch_read_zones_dev\(mgf_batch\* b, int32_t k, int32_t\* out_dev, mgf_aabb\* boxes_out_dev, int64_t cap\);",
                r"mgf_status mgf_batch_overlap_first_dev\(mgf_batch\* b, const mgf_aabb\* boxes_dev, int64_t n, const int32_t\* ignore_body_dev, int32_t k,\s+"
                r"int32_t\* out_dev\);"):
        assert re.search(r"MGF_API " + sig, h), sig
    assert h.index("mgf_batch_cast_cameras_dev(") < h.index("typedef struct mgf_batch_zone")             # behind the cameras
    assert re.search(r"typedef struct mgf_batch_zone \{ int32_t world, body; mgf_vec3 p, r; int32_t flags, reserved; \} mgf_batch_zone;", h)
    m = re.search(r"#define MGF_BATCH_ZONE_LAUNCHES (\d+)", h)
    assert m and int(m.group(1)) == _capi.BATCH_ZONE_LAUNCHES == 1
    section = h[h.index("---- box zones"):]
    for word in ("c = x + rotate(q, p)", "body = -1: c = p", "WITHOUT delta", "AT ONCE", "the colliders move at the next tick", "NOT truncated",
                 "the rest are -1", "MGF_ERR_CAPACITY", "nothing enqueued", "mgf_batch_add_bodies", "MGF_BATCH_MAX_BODIES", "4 (1 + k)",
                 "multiple of n_worlds", "OUT OF SCOPE"):
        assert word in section, word
    assert C.sizeof(_capi.BatchZone) == 40 == _capi.ZONE_DTYPE.itemsize
    assert [f[0] for f in _capi.BatchZone._fields_] == list(_capi.ZONE_DTYPE.names) == ["world", "body", "p", "r", "flags", "reserved"]
    assert [_capi.ZONE_DTYPE.fields[k][1] for k in _capi.ZONE_DTYPE.names] == [0, 4, 8, 20, 32, 36]
    assert ZC.IGNORE_SELF == _capi.SENSOR_IGNORE_SELF and max(ZC.KS) == _capi.BATCH_MAX_BODIES
    lib = mgf_amd.load_library()
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    want = {"mgf_batch_set_zones": (i32, [vp, vp, i64]), "mgf_batch_zone_count": (i64, [vp]), "mgf_batch_read_zones": (i32, [vp, i32, vp, vp, i64]),
            "mgf_batch_read_zones_dev": (i32, [vp, i32, vp, vp, i64]), "mgf_batch_overlap_first_dev": (i32, [vp, vp, i64, vp, i32, vp])}
    for name in CALLS:
        assert name in _capi.SYMBOLS, name
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == want[name], name
    for method in ("set_zones", "zone_count", "read_zones", "read_zones_dev", "overlap_first_dev"):
        assert callable(getattr(mgf_amd.WorldBatch, method)), method
    flat = re.sub(r"\s+", " ", read("INTEGRATION.md"))
    for sig in ("pub fn mgf_batch_set_zones(b: *mut mgf_batch, z: *const mgf_batch_zone, n: i64) -> mgf_status;",
                "pub fn mgf_batch_zone_count(b: *const mgf_batch) -> i64;",
                "pub fn mgf_batch_read_zones(b: *mut mgf_batch, k: i32, out: *mut i32, boxes_out: *mut mgf_aabb, cap: i64) -> mgf_status;",
                "pub fn mgf_batch_read_zones_dev(b: *mut mgf_batch, k: i32, out_dev: *mut i32, boxes_out_dev: *mut mgf_aabb, cap: i64) -> mgf_status;",
                "pub fn mgf_batch_overlap_first_dev(b: *mut mgf_batch, boxes_dev: *const mgf_aabb, n: i64, ignore_body_dev: *const i32, k: i32, "
                "out_dev: *mut i32) -> mgf_status;",
                "pub struct mgf_batch_zone"):
        assert sig in flat, sig
    kernels = read("mgf_amd", "csrc", "kernels.h")
    assert kernels.index('#include "k_batch_camera.h"') < kernels.index('#include "k_batch_zone.h"') and "k_batch_zone_first" in kernels
    hip = read("mgf_amd", "csrc", "mgf_hip.hip")
    assert hip.index('#include "host_batch_camera.inc"') < hip.index('#include "host_batch_zone.inc"')
    design = read("DESIGN.md")
    sub = design[design.index("Box zones"):]
    for word in ("k_batch_zone_first", "c = x + rotate(q, p)", "Out of scope", "batch_zone_bench.py", "Compiler output", "Not measured"):
        assert word in sub, word
    # the remarks that left device-pointer box queries out - two in DESIGN.md, one in the header - point here
    assert design.count("(since: \"Box zones\"") == 2 and "mgf_batch_read_zones_dev / mgf_batch_overlap_first_dev, below" in h
    readme = read("README.md")
    assert "set_zones" in readme and "read_zones_dev" in readme and "overlap_first_dev" in readme
    assert os.path.exists(os.path.join(ROOT, "tools", "batch_zone_bench.py"))


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_what_needs_no_device_is_refused_before_the_handle_is_dereferenced():
    lib = mgf_amd.load_library()
    INV = _capi.ERR_INVALID

    def err():
        return lib.mgf_last_error().decode()
    fake = C.c_void_p(16)   # a handle that is never dereferenced; addresses that are never looked up
    rig = np.zeros(4, _capi.ZONE_DTYPE)
    out, boxes, ign = C.c_void_p(1 << 20), C.c_void_p(1 << 21), C.c_void_p(1 << 22)
    assert lib.mgf_batch_zone_count(None) == -1
    assert lib.mgf_batch_set_zones(None, rig.ctypes.data, 4) == INV and "NULL" in err()
    assert lib.mgf_batch_set_zones(None, None, 0) == INV and "NULL" in err()
    assert lib.mgf_batch_set_zones(fake, None, 4) == INV and "NULL" in err()
    assert lib.mgf_batch_set_zones(fake, rig.ctypes.data, -1) == INV and "negative" in err()
    assert lib.mgf_batch_set_zones(fake, rig.ctypes.data, 1 << 31) == INV and "too many" in err()
    for fn in (lib.mgf_batch_read_zones, lib.mgf_batch_read_zones_dev):
        assert fn(None, 8, out, boxes, 4) == INV and "NULL" in err()
        for k in (-1, _capi.BATCH_MAX_BODIES + 1, -(1 << 31), (1 << 31) - 1):
            assert fn(fake, k, out, boxes, 4) == INV and "k is outside" in err(), k
            assert fn(fake, k, None, None, 0) == INV and "k is outside" in err(), k
        assert fn(fake, 8, out, None, -1) == INV and "negative" in err()
        assert fn(fake, 0, out, None, -(1 << 40)) == INV and "negative" in err()
    fn = lib.mgf_batch_overlap_first_dev
    assert fn(None, boxes, 4, ign, 8, out) == INV and "NULL" in err()
    assert fn(fake, boxes, -1, ign, 8, out) == INV and "negative" in err()
    assert fn(fake, boxes, 1 << 31, ign, 8, out) == INV and "too many" in err()
    assert fn(fake, None, 4, ign, 8, out) == INV and "NULL" in err()
    assert fn(fake, boxes, 4, None, 8, None) == INV and "NULL" in err()
    for k in (-1, _capi.BATCH_MAX_BODIES + 1):
        assert fn(fake, boxes, 4, ign, k, out) == INV and "k is outside" in err(), k
        assert fn(fake, None, 0, None, k, None) == INV and "k is outside" in err(), k
    # what needs the handle - a world or a body out of range, a flag bit beyond the one defined, body = -1 with the flag, a reserved word,
    # cap below the count - is refused on the host too, ahead of any change of the rig and of any device work (read here; run in
    # tests/test_gpu_world_batch_zones.py, where a handle exists)
    src = read("mgf_amd", "csrc", "host_batch_zone.inc")
    body = src[src.index('extern "C" mgf_status mgf_batch_set_zones('):src.index('extern "C" int64_t mgf_batch_zone_count(')]
    assert not re.search(r"b->zones\.|\bR\.", body.replace("batch_rig_plan(b, b->zones, z, n);", ""))   # the rig changes in the plan step alone
    body = RC.set_call_with_plan(body, "batch_rig_plan(b, b->zones, z, n);")    # the set call together with the shared plan step
    first_change = body.index("R.recs.assign(")
    for refusal in ("batch_rig_set_args(b, z, n_in)", 'batch_rig_ref_check(b, z[i].world, z[i].body, z[i].flags, "zone", true)', "has no body of its own to ignore", "reserved word is not 0"):
        assert body.index(refusal) < first_change, refusal
    assert not re.search(r"<<<|Async|hipMalloc|\.ensure\(|h2d\(", body)            # no device work at all
    # the sensor and camera rigs are not touched from here: it names b->zones and neither b->sensors nor b->cameras
    assert not re.search(r"b->[sc]_\w+", src) and "b->zones" in src and "b->sensors" not in src and "b->cameras" not in src
    # the helper is the rigs' one: one copy of it, and it lets -1 through only where it is asked to
    sens = read("mgf_amd", "csrc", "host_batch_sensor.inc")
    assert "batch_rig_ref_check(" not in src.replace("MGF_TRY(batch_rig_ref_check(", "") and RC.rig_source().count("static mgf_status batch_rig_ref_check(") == 1
    assert "static mgf_status batch_rig_ref_check(" not in sens
    check = RC.ref_check_step()
    assert "bool or_world = false" in check and "!(or_world && body == -1) && (body < 0 ||" in check
    args = src[src.index("static mgf_status batch_zone_read_args("):src.index('extern "C" mgf_status mgf_batch_read_zones(')]
    RC.assert_the_read_and_cast_refusals(args, ["zone_k_check(k)", "batch_rig_cap(cap)"])          # k ahead of a negative cap
    host = read("mgf_amd", "csrc", "host_batch.inc")
    add = host[host.index('extern "C" mgf_status mgf_batch_add_bodies('):]
    add = add[:add.index("\n}\n")]
    stale = RC.stale_step()
    assert "batch_rigs_stale(b);" in add and "b->zones.stale = true;" in stale and "b->sensors.stale = true;" in stale and "b->cameras.stale = true;" in stale
    assert "b->zones" not in sens and "b->zones" not in read("mgf_amd", "csrc", "host_batch_camera.inc")


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
ENQUEUE = (r"batch_zone_run\(|batch_rig_up\(|batch_rig_upload\(|batch_push\(|batch_dev_begin\(|batch_env_sync\(|batch_cols_refresh\(|hipMemsetAsync|"
           r"hipMemcpyAsync|<<<|prim_exclusive_scan_u32|\.ensure\(|h2d\(")


def test_both_device_forms_look_every_pointer_up_before_the_first_enqueue():
    src = read("mgf_amd", "csrc", "host_batch_zone.inc")
    # mgf_batch_read_zones_dev: args | bind | two look-ups | the overlap of the outputs | an empty rig leaves | the run
    run = src[src.index('extern "C" mgf_status mgf_batch_read_zones_dev('):src.index("// The same kernel over boxes the caller computed")]
    first_enqueue = min(m.start() for m in re.finditer(ENQUEUE, run))
    checks = [m.start() for m in re.finditer(r"dev_span\(", run)]
    assert len(checks) == 2 and max(checks) < first_enqueue
    assert "const size_t out_bytes = 4 * ((size_t)k + 1) * n;" in run
    for name in ("out_dev, out_bytes", "boxes_out_dev, 24 \\* n"):
        assert re.search(r"dev_span\(b->ctx, " + name, run), name
    assert run.index('arrays[2] = {{out_dev, out_bytes, "out_dev"}, {boxes_out_dev, 24 * n, "boxes_out_dev"}};') < run.index("dev_outputs_overlap(arrays, 2, 2)")
    assert run.index("batch_zone_read_args(") < run.index("ctx_bind(") < min(checks) and max(checks) < run.index("dev_outputs_overlap(") < first_enqueue
    assert run.index("if (n == 0) return MGF_OK;") < first_enqueue                   # an empty rig enqueues nothing
    # mgf_batch_overlap_first_dev: the order of mgf_batch_raycast_many_dev with world_dev == NULL
    run = src[src.index('extern "C" mgf_status mgf_batch_overlap_first_dev('):]
    first_enqueue = min(m.start() for m in re.finditer(ENQUEUE, run))
    checks = [m.start() for m in re.finditer(r"dev_span\(", run)]
    assert len(checks) == 3 and max(checks) < first_enqueue
    for name in ("boxes_dev, 24 \\* n", "ignore_body_dev, 4 \\* n", "out_dev, out_bytes"):
        assert re.search(r"dev_span\(b->ctx, " + name, run), name
    assert (run.index("batch_dev_args(") < run.index('"NULL argument"') < run.index("zone_k_check(") < run.index("ctx_bind(") < run.index("n % b->K")
            < min(checks))
    assert max(checks) < run.index('dev_outputs_overlap(arrays, 3, 1, "an input array")') < first_enqueue
    assert run.index("if (n == 0) return MGF_OK;") < first_enqueue
    assert "hipStreamSynchronize" not in run and "hipMemcpy" not in run
    q = read("mgf_amd", "csrc", "host_batch_query_dev.inc")
    helper = q[q.index("static mgf_status dev_outputs_overlap("):q.index("// Q = ParticleIn")]
    assert "dev_bytes_overlap(a[i].p, a[i].bytes, a[j].p, a[j].bytes)" in helper and not re.search(ENQUEUE, helper) and "b->" not in helper
    # everything a rig read enqueues is in batch_zone_run and batch_rig_up: one launch, counted; no wait, no copy but the rig's
    helper = src[src.index("static mgf_status batch_zone_run("):src.index("static mgf_status zone_k_check(")]
    assert helper.count("<<<") == 1 and "k_batch_zone_first<kItemTable><<<" in helper and "hipStreamSynchronize" not in helper and "hipMemcpy" not in helper
    assert helper.index("LAUNCH_CHECK();") < helper.index("b->q_launches += MGF_BATCH_ZONE_LAUNCHES;")
    assert helper.index("batch_push(") < helper.index('batch_rig_up(b, R, "zone", 3, true)') < helper.index("k_batch_zone_first<kItemTable><<<")
    up = RC.up_step()
    assert up.index("if (!R.stale) return MGF_OK;") < up.index("internal error") < up.index("batch_rig_upload(") and up.count("batch_rig_upload(") == 1 and "h2d(" not in up
    # the host form: one download, one wait
    host = src[src.index('extern "C" mgf_status mgf_batch_read_zones('):src.index('extern "C" mgf_status mgf_batch_read_zones_dev(')]
    assert host.count("hipMemcpyAsync(") == 2 and host.count("hipStreamSynchronize(") == 2 and host.index("if (!boxes_out) {") < host.index("hipMemcpyAsync(")
    # the kernel: no exit at all, no atomic, one barrier ahead of the split; every lane makes every trip
    # (read in the front the kernel shares with k_batch_observe_overlap - bo_front, k_batch_observe.h - followed by the kernel itself,
    # which brings the loaders, the store behind a hit and the epilogue: the loaders and the kernel's body - bz_first - are written once
    # for this kernel and its part-aware form, and the kernel is the one call of that body with the plain bodies)
    k, o = read("mgf_amd", "csrc", "k_batch_zone.h"), read("mgf_amd", "csrc", "k_batch_observe.h")
    shared = o[o.index("uint32_t bo_front("):o.index("// k_batch_observe_overlap<FILL> and its part-aware form")]
    body = k[k.index("BatchBox bz_fixed("):]
    assert body.count("bz_first<SRC>(A, PlainBodies(A), S, s_dyn);") == 1 and body.index("void bz_first(") < body.index("void k_batch_zone_first(")
    front = shared + body
    # (the only returns: the front's count at its end and the values of the kernel's hooks - a loader's box, the record's address)
    assert "return;" not in front and not re.search(r"return (?!m;|b;|BatchBox\{|A\.out \+|bz_fixed\(A, qi\);|bz_mounted\(A, qi, g0\);)", front)
    assert shared.rstrip().endswith("return m;\n}")
    assert "atomic" not in front and front.count("__syncthreads()") == 1
    assert (front.index("__syncthreads()") < front.index("W.template split<IDENTITY>(A, min(W.shift(), 6u))") < front.index("load(W.qi, g0)")
            < front.index("for (uint32_t i0 = 0; i0 < n; i0 += L)") < front.index("(int32_t)i != ign") < front.index("__ballot(hit)")
            < front.index("put(hit, i, m + (uint32_t)__popcll(g & ((1ull << sub) - 1ull)));") < len(shared)
            < front.index("if (hit && rank < k) record()[1u + rank] = (int32_t)i") < front.index("o[0] = (int32_t)m") < front.index("o[1u + s] = -1"))
    # the fixed layout splits with the identity for an order, and both layouts drop the ignored body
    assert ("SRC == kItemFixed ? bo_front<true, true>(A, bodies, W, s_dyn, z, fixed, store) : bo_front<false, true>(A, bodies, W, s_dyn, z, mounted, store)"
            in body)
    assert "template <bool IDENTITY, bool IGNORE, class Bodies, class Load, class Put>" in o and "(!IGNORE || (int32_t)i != ign)" in shared
    # the staged box is the bodies' policy's: the plain one is the tight bounds of the collider row
    q = read("mgf_amd", "csrc", "k_batch_query.h")
    plain = q[q.index("struct PlainBodies {"):q.index("void bq_ray_front(")]
    assert "bodies.box((size_t)g0 + i)" in shared and plain.count("comp_bounds(to_comp(A.col0[g], A.col1[g]))") == 1 and "isnan" not in plain
    assert "isnan" not in k and "isnan" not in o
    assert not re.search(r"return;|__syncthreads|atomic|__shared__ (?!float4 s_dyn)", body.replace("extern __shared__ float4 s_dyn[];", ""))


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_binding_turns_a_wrong_tensor_down_before_it_calls_c():
    import torch

    class Handle(mgf_amd.WorldBatch):   # no context, no C handle: a call that got as far as C would fail differently
        def __init__(self):
            self._h, self.n_worlds = None, 2

        def zone_count(self):
            return 4

    b, n, k = Handle(), 4, 8
    wrong_out = [torch.zeros((n, 1 + k), dtype=torch.float32), torch.zeros((n, 1 + k), dtype=torch.int64), torch.zeros((1 + k, n), dtype=torch.int32).t(),
                 torch.zeros((n - 1, 1 + k), dtype=torch.int32), torch.zeros(n * (1 + k), dtype=torch.int32), torch.zeros((n, 0), dtype=torch.int32)]
    wrong_boxes = [torch.zeros((n, 6), dtype=torch.float64), torch.zeros((n, 6), dtype=torch.int32), torch.zeros((6, n), dtype=torch.float32).t(),
                   torch.zeros((n - 1, 6), dtype=torch.float32), torch.zeros((n, 7), dtype=torch.float32)]
    good_out = torch.zeros((n, 1 + k), dtype=torch.int32)
    for t in wrong_out:
        with pytest.raises(ValueError) as e:
            b.read_zones_dev(t, boxes=1 << 21)
        assert "on cpu" not in str(e.value), str(e.value)              # turned down for what it is, not for where it is
        with pytest.raises(ValueError) as e:
            b.overlap_first_dev(1 << 21, t, n=n)
        assert "on cpu" not in str(e.value), str(e.value)
    for t in wrong_boxes:
        with pytest.raises(ValueError) as e:
            b.read_zones_dev(1 << 20, boxes=t, k=k)
        assert "on cpu" not in str(e.value), str(e.value)
        with pytest.raises(ValueError) as e:
            b.overlap_first_dev(t, 1 << 20, n=n, k=k)
        assert "on cpu" not in str(e.value), str(e.value)
    for t in (torch.zeros(n, dtype=torch.int64), torch.zeros(n - 1, dtype=torch.int32), torch.zeros((n, 2), dtype=torch.int32)[:, 0]):
        with pytest.raises(ValueError) as e:
            b.overlap_first_dev(1 << 21, 1 << 20, ignore=t, n=n, k=k)
        assert "on cpu" not in str(e.value), str(e.value)
    with pytest.raises(ValueError, match="on cpu"):                     # everything right but the device
        b.read_zones_dev(good_out)
    with pytest.raises(ValueError, match="on cpu"):
        b.read_zones_dev(1 << 20, boxes=torch.zeros((n, 6), dtype=torch.float32), k=k)
    with pytest.raises(ValueError, match="on cpu"):
        b.overlap_first_dev(torch.zeros((n, 6), dtype=torch.float32), 1 << 20, k=k)
    with pytest.raises(ValueError, match="on cpu"):
        b.overlap_first_dev(1 << 21, good_out, n=n)
    with pytest.raises(ValueError, match="required"):
        b.read_zones_dev(None)
    with pytest.raises(ValueError, match="required"):
        b.overlap_first_dev(None, 1 << 20, n=n, k=k)
    with pytest.raises(ValueError, match="k given"):
        b.read_zones_dev(1 << 20)                                       # a raw address says nothing of k
    with pytest.raises(ValueError, match="multiple"):
        b.overlap_first_dev(1 << 21, 1 << 20, n=3, k=k)
    with pytest.raises(ValueError, match="not ndarray"):
        b.read_zones_dev(np.zeros((n, 1 + k), np.int32), k=k)
    with pytest.raises(mgf_amd.MgfError):                               # and a call whose arguments are all in order does reach C
        b.read_zones_dev(1 << 20, boxes=1 << 21, k=k)
    with pytest.raises(mgf_amd.MgfError):
        b.overlap_first_dev(1 << 21, 1 << 20, ignore=1 << 22, n=n, k=k)
    # set_zones broadcasts scalars and single rows; what reaches C is ZONE_DTYPE rows (no handle: C refuses, after the marshalling)
    with pytest.raises(mgf_amd.MgfError):
        b.set_zones([0, 1, 1], 0, (0, 0, 0), [(1, 1, 1), (1, 2, 1), (2, 1, 1)])
    with pytest.raises(mgf_amd.MgfError):
        b.set_zones([0, 1], p=[(0, 0, 0), (1, 1, 1)], r=(1, 1, 1))     # fixed in the world
    with pytest.raises(ValueError):
        b.set_zones([0, 1, 1], [0, 1], (0, 0, 0), (1, 1, 1))           # neither one nor n


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_new_kernel_uses_no_scratch_and_the_query_kernels_keep_their_figures():
    if not os.path.exists(os.path.join(ROOT, "mgf_amd", "libmgf_hip.so")) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    rows = kernel_resources("k_batch_zone_")
    assert set(rows) == {"k_batch_zone_first<0>", "k_batch_zone_first<2>"}, sorted(rows)
    design = re.sub(r"\s+", " ", read("DESIGN.md"))
    for name, v in rows.items():
        assert (v[2], v[3], v[4], v[5]) == ("0", "0", "0", "0"), (name, v)       # no scratch, no static LDS, no spills
        assert int(v[0]) <= 64, (name, v)                                         # eight waves a SIMD at 64 VGPRs
        assert f"`{name}` {v[0]} / {v[1]} / 0 / 0 / 0" in design, (name, v)       # the line DESIGN.md records
    k = read("mgf_amd", "csrc", "k_batch_zone.h")
    assert len(re.findall(r"__global__ __launch_bounds__\(kBatchBlock\)", k)) == len(re.findall(r"__global__", k)) == 1
    assert "__shared__" not in k.replace("extern __shared__ float4 s_dyn[];", "")


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------------
def _oracle_lists(scs, bx, world):
    """per box the bodies of its world whose BoundedBy<AABB> box Overlaps<AABB> it, by the oracle's own two functions, ascending"""
    from oracle import oracle as O
    L = O.lib()
    zero = O.vec3((0.0, 0.0, 0.0))
    tight = []
    for sc in scs:
        row = []
        for c in sc["comps"]:
            b = O.Aabb()
            L.mgfo_component_bounds(C.byref(O.Component(int(c["tag"]), O.vec3(c["p"]), O.vec3(c["d"]), float(c["r"]))), C.byref(zero), C.byref(b))
            row.append(b)
        tight.append(row)
    out = []
    for q, w in zip(bx, world):
        qb = O.Aabb(O.vec3(q[:3]), O.vec3(q[3:]))
        out.append([i for i, b in enumerate(tight[int(w)]) if L.mgfo_aabb_overlaps(C.byref(b), C.byref(qb))])
    return out


def test_the_scenes_hold_the_cases_the_gpu_tests_are_for():
    scs = ZC.zone_scenes()
    lengths = ZC.lengths_of(scs)
    assert lengths == [5, 0, 1, 300] and all({0, 1} <= set(scs[w]["comps"]["tag"].tolist()) for w in (ZC.W5, ZC.W300))
    rig, role = ZC.zone_rig(scs)
    assert np.bincount(rig["world"], minlength=4).tolist() == [3, 2, 20, 257] and np.any(np.diff(rig["world"]) < 0)
    assert np.all(rig["body"] >= -1) and np.all(rig["body"] < np.int64(lengths)[rig["world"]]) and np.all(rig["reserved"] == 0)
    assert not np.any((rig["body"] < 0) & (rig["flags"] != 0))
    bx = ZC.boxes(rig, ZC.initial_state(scs), lengths)
    lists = _oracle_lists(scs, bx, rig["world"])
    ign = ZC.ignore_of(rig)
    own = [rig["body"][i] in lists[i] for i in range(len(rig))]
    lists = [[j for j in lst if j != ign[i]] for i, lst in enumerate(lists)]
    count = np.int64([len(lst) for lst in lists])
    ks = [k for k in ZC.KS if 0 < k < 1024]
    assert np.any(count == 0) and all(np.any((count > 0) & (count < k)) for k in ks[1:])
    assert all(np.any(count == k) for k in (1,)) and all(np.any(count > k) for k in ks)
    print("zones by count:", {int(c): int(n) for c, n in zip(*np.unique(count, return_counts=True))})
    # by role: a zone that holds its own body, with and without the flag; the NaN boxes and the far one hold nothing; -0.1 still holds
    # its body and -2 nothing; two zones on one body; the cover is the last zone of its world and lists every body
    seen, ignored = np.flatnonzero(role == ZC.OWN_SEEN), np.flatnonzero(role == ZC.OWN_IGNORED)
    assert len(seen) >= 3 and all(own[i] and lists[i] == [rig["body"][i]] for i in seen)
    assert len(ignored) >= 2 and all(own[i] and lists[i] == [] for i in ignored)
    assert {int(scs[rig["world"][i]]["comps"]["tag"][rig["body"][i]]) for i in seen} == {0, 1}
    for r in (ZC.NAN_P, ZC.NAN_R, ZC.FAR):
        assert np.sum(role == r) >= 1 and np.all(count[role == r] == 0), r
    assert np.sum(role == ZC.NAN_P) == 2 and set(rig["body"][role == ZC.NAN_P] >= 0) == {True, False}
    neg = np.flatnonzero(role == ZC.NEGATIVE)
    assert sorted(count[neg].tolist()) == [0, 1, 1] and np.all(rig["r"][neg] < 0)
    twin = np.flatnonzero(role == ZC.TWIN)
    assert len(twin) == 2 and rig["body"][twin[0]] == rig["body"][twin[1]] and rig["flags"][twin[0]] != rig["flags"][twin[1]]
    cover = int(np.flatnonzero((rig["world"] == ZC.W300) & (role == ZC.COVER))[0])
    assert cover == int(np.flatnonzero(rig["world"] == ZC.W300)[-1]) and lists[cover] == list(range(300))
    # ... so the second work item of that world is this one zone: 64 lanes, five trips over 300 bodies, hits on both sides of every cut
    items, order, _ = QD.plan_model(rig["world"], 4)
    assert items[:, 2].tolist() == [3, 2, 20, 256, 1] and order[items[-1][1]] == cover
    # and with one lane a zone (the item of 256) a list of several bodies whose indices lie on both sides of a multiple of 64
    first = set(order[items[3][1]:items[3][1] + 256].tolist())
    assert any(i in first and len(lists[i]) >= 2 and lists[i][0] // 64 != lists[i][-1] // 64 for i in range(len(rig)))
    # the fixed layouts: per = 1, 3 and 257 boxes a world, the cover of every world first
    for per in ZC.PERS:
        fb, fi = ZC.fixed_boxes(scs, per)
        assert fb.shape == (4 * per, 6) and fi.shape == (4 * per,) and fb.dtype == f32 and fi.dtype == np.int32
        fl = _oracle_lists(scs, fb, np.repeat(np.arange(4), per))
        for w in range(4):
            assert fl[w * per] == list(range(lengths[w])), (per, w)
        if per >= 3:
            assert all(fl[w * per + 2] == [] and np.isnan(fb[w * per + 2, 1]) for w in range(4))
        if per == 257:
            none = (fi < 0) | (fi >= np.repeat(lengths, per))
            hit = np.array([fi[i] in fl[i] for i in range(len(fi))])
            assert np.sum(none & (fi != -1)) >= 50 and np.sum(hit) >= 20, (int(np.sum(none & (fi != -1))), int(np.sum(hit)))
