"""The body-mounted feelers of a batch (mgf_batch_set_feelers, mgf_batch_feeler_count, mgf_batch_cast_feelers,
mgf_batch_cast_feelers_dev) without a GPU: the numpy restatement of a feeler's cast that the GPU tests hold the kernel to is built
from a rotate that equals the oracle's mgfo_rotate_vector bit for bit, with its WORLD_DELTA and OWN_SHAPE branches; the header, the
library, the binding and the documents carry the calls; what can be refused before a device is looked at is refused there;
mgf_batch_cast_feelers_dev looks both pointers up and holds the outputs against each other before it enqueues anything; the rig file
writes nothing a second time that the shared rig steps write; the binding turns a wrong tensor down before it calls C; the new kernel
uses no scratch and spills nothing."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mgf_amd
from mgf_amd import _capi
from tests import batch_feeler_cases as FC
from tests import batch_rig_cases as RC
from tests import batch_sensor_cases as SC
from tests.util import ROOT, kernel_resources, read

CALLS = ("mgf_batch_set_feelers", "mgf_batch_feeler_count", "mgf_batch_cast_feelers", "mgf_batch_cast_feelers_dev")
RIG_FILE = "host_batch_feeler.inc"


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_restatement_of_a_cast_is_the_oracles_rotate_vector_and_plain_f32_adds():
    """a few hundred seeded (q, v) through the oracle's mgfo_rotate_vector; FC.casts over a made-up state and made-up colliders must
    give exactly x + that, that, and - by flag - the record's delta or that, or the collider as it stands: equal bits, so that the GPU
    tests' reference is anchored to the oracle, not to itself"""
    from oracle import oracle as O
    rng = np.random.default_rng(23)
    n = 300
    q = rng.normal(0, 1, (n, 4))
    q[: n // 2] /= np.linalg.norm(q[: n // 2], axis=1, keepdims=True)
    vs = [rng.normal(0, 1, (n, 3)) * rng.choice([1.0, 1e-3, 30.0], (n, 1)) for _ in range(3)]
    vs[0][::7] *= 1e4
    vs[2][3::11, 1] = 1e-41                            # a denormal component
    q, vs = q.astype(np.float32), [v.astype(np.float32) for v in vs]
    lib = O.lib()

    def oracle_rotate(v):
        want = np.empty_like(v)
        for i in range(n):
            out = O.Vec3()
            lib.mgfo_rotate_vector(C.byref(O.Quat(*q[i].tolist())), C.byref(O.Vec3(*v[i].tolist())), C.byref(out))
            want[i] = (out.x, out.y, out.z)
        return want
    rp, rd, rdelta = (oracle_rotate(v) for v in vs)
    for v, r in zip(vs, (rp, rd, rdelta)):
        assert SC.rotate(q, v).tobytes() == r.tobytes()
    # one body a feeler, in one world; every allowed flag word in turn
    state = dict(x=rng.normal(0, 5, (n, 3)).astype(np.float32), q=q)
    col = np.zeros(n, _capi.MOVING_DTYPE)
    col["tag"], col["r"] = rng.integers(0, 2, n), rng.uniform(0.1, 1, n)
    col["p"], col["d"], col["delta"] = rng.normal(0, 5, (n, 3)), rng.normal(0, 1, (n, 3)), rng.normal(0, 1, (n, 3))
    rig = np.zeros(n, _capi.FEELER_DTYPE)
    rig["body"] = np.arange(n)
    rig["tag"], rig["r"] = rng.integers(0, 2, n), rng.uniform(0.1, 1, n)
    rig["p"], rig["d"], rig["delta"] = vs
    rig["flags"] = np.resize(FC.ALLOWED_FLAGS, n)
    c = FC.casts(rig, state, col, [n])
    own, wd = (rig["flags"] & FC.OWN_SHAPE) != 0, (rig["flags"] & FC.WORLD_DELTA) != 0
    assert own.any() and (~own).any() and wd.any() and (~wd).any() and (own & wd).any() and (own & ~wd).any()
    assert c["p"][~own].tobytes() == (state["x"] + rp)[~own].tobytes() and c["d"][~own].tobytes() == rd[~own].tobytes()
    assert c["tag"][~own].tobytes() == rig["tag"][~own].tobytes() and c["r"][~own].tobytes() == rig["r"][~own].tobytes()
    for k in ("tag", "p", "d", "r"):
        assert c[k][own].tobytes() == col[k][own].tobytes(), k
    assert c["delta"][wd].tobytes() == rig["delta"][wd].tobytes() and c["delta"][~wd].tobytes() == rdelta[~wd].tobytes()
    assert FC.ignore_of(rig).tolist() == [b if f & 1 else -1 for b, f in zip(rig["body"].tolist(), rig["flags"].tolist())]


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def test_header_library_binding_and_documents_carry_the_calls():
    h = read("include", "mgf_hip.h")
    for sig in (r"mgf_status mgf_batch_set_feelers\(mgf_batch\* b, const mgf_batch_feeler\* f, int64_t n\);",
                r"int64_t\s+mgf_batch_feeler_count\(const mgf_batch\* b\);",
                r"mgf_status mgf_batch_cast_feelers\(mgf_batch\* b, int32_t kinds_mask, mgf_sweep_hit\* out, mgf_moving_component\* casts_out, int64_t cap\);",
                r"mgf_status mgf_batch_cast_feelers_dev\(mgf_batch\* b, int32_t kinds_mask, mgf_sweep_hit\* out_dev, mgf_moving_component\* casts_out_dev,\s*int64_t cap\);"):
        assert re.search(r"MGF_API " + sig, h), sig
    assert h.index("mgf_batch_read_touches_dev(") < h.index("typedef struct mgf_batch_feeler") < h.index("mgf_batch_counter(")   # behind the contact sensors
    for name, value in (("MGF_FEELER_IGNORE_SELF", _capi.FEELER_IGNORE_SELF), ("MGF_FEELER_WORLD_DELTA", _capi.FEELER_WORLD_DELTA),
                        ("MGF_FEELER_OWN_SHAPE", _capi.FEELER_OWN_SHAPE), ("MGF_BATCH_FEELER_LAUNCHES", _capi.BATCH_FEELER_LAUNCHES)):
        m = re.search(r"#define %s\s+(\d+)" % name, h)
        assert m and int(m.group(1)) == value, name
    assert (_capi.FEELER_IGNORE_SELF, _capi.FEELER_WORLD_DELTA, _capi.FEELER_OWN_SHAPE) == (1, 2, 4) == (FC.IGNORE_SELF, FC.WORLD_DELTA, FC.OWN_SHAPE)
    assert _capi.FEELER_IGNORE_SELF == _capi.SENSOR_IGNORE_SELF and _capi.BATCH_FEELER_LAUNCHES == 1
    section = h[h.index("body-mounted feelers"):]
    for word in ("P = x + rotate(q, p)", "D = rotate(q, d)", "WITHOUT delta", "move a feeler AT ONCE", "move at the next tick", "bit for bit",
                 "MGF_ERR_CAPACITY", "nothing enqueued", "mgf_batch_add_bodies", "the rig was not changed", "several components"):
        assert word in section, word
    limits = h[h.index("LIMITS: bodies of one to four components"):h.index("canonical constraint order only")]
    assert "_cast_feelers(_dev)" in limits
    # the record: 64 bytes, the same fields at the same offsets in the ctypes struct and the numpy dtype
    assert C.sizeof(_capi.BatchFeeler) == 64 == _capi.FEELER_DTYPE.itemsize
    names = ["world", "body", "tag", "flags", "p", "d", "r", "delta", "reserved"]
    assert [f[0] for f in _capi.BatchFeeler._fields_] == list(_capi.FEELER_DTYPE.names) == names
    want_off = [0, 4, 8, 12, 16, 28, 40, 44, 56]
    assert [_capi.FEELER_DTYPE.fields[k][1] for k in names] == want_off == [getattr(_capi.BatchFeeler, k).offset for k in names]
    assert re.search(r"typedef struct mgf_batch_feeler \{\s*int32_t world, body, tag, flags;\s*mgf_vec3 p, d;\s*float r;\s*mgf_vec3 delta;\s*int32_t reserved\[2\];", h)
    lib = mgf_amd.load_library()
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    want = {"mgf_batch_set_feelers": (i32, [vp, vp, i64]), "mgf_batch_feeler_count": (i64, [vp]),
            "mgf_batch_cast_feelers": (i32, [vp, i32, vp, vp, i64]), "mgf_batch_cast_feelers_dev": (i32, [vp, i32, vp, vp, i64])}
    for name in CALLS:
        assert name in _capi.SYMBOLS, name
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == want[name], name
    for method in ("set_feelers", "feeler_count", "cast_feelers", "cast_feelers_dev"):
        assert callable(getattr(mgf_amd.WorldBatch, method)), method
    flat = re.sub(r"\s+", " ", read("INTEGRATION.md"))
    for sig in ("pub fn mgf_batch_set_feelers(b: *mut mgf_batch, f: *const mgf_batch_feeler, n: i64) -> mgf_status;",
                "pub fn mgf_batch_feeler_count(b: *const mgf_batch) -> i64;",
                "pub fn mgf_batch_cast_feelers(b: *mut mgf_batch, kinds_mask: i32, out: *mut mgf_sweep_hit, casts_out: *mut mgf_moving_component, cap: i64) -> mgf_status;",
                "pub fn mgf_batch_cast_feelers_dev(b: *mut mgf_batch, kinds_mask: i32, out_dev: *mut mgf_sweep_hit, casts_out_dev: *mut mgf_moving_component, cap: i64) -> mgf_status;",
                "pub struct mgf_batch_feeler"):
        assert sig in flat, sig
    kernels = read("mgf_amd", "csrc", "kernels.h")
    assert kernels.index('#include "k_batch_touch.h"') < kernels.index('#include "k_batch_feeler.h"') and "k_batch_feeler_bodies (k_batch_feeler.h)" in kernels
    hip = read("mgf_amd", "csrc", "mgf_hip.hip")
    assert hip.index('#include "host_batch_touch.inc"') < hip.index('#include "host_batch_feeler.inc"')
    design = read("DESIGN.md")
    assert design.index("Contact sensors") < design.index("Body-mounted feelers")
    sub = design[design.index("Body-mounted feelers"):]
    for word in ("k_batch_feeler_bodies", "P = x + rotate(q, p)", "Out of scope", "batch_feeler_bench.py", "Compiler output", "MGF_BATCH_FEELER_LAUNCHES"):
        assert word in sub, word
    readme = read("README.md")
    assert "set_feelers" in readme and "cast_feelers_dev" in readme
    assert os.path.exists(os.path.join(ROOT, "tools", "batch_feeler_bench.py"))


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_what_needs_no_device_is_refused_before_the_handle_is_dereferenced():
    lib = mgf_amd.load_library()
    INV = _capi.ERR_INVALID

    def err():
        return lib.mgf_last_error().decode()
    fake = C.c_void_p(16)   # a handle that is never dereferenced; addresses that are never looked up
    rig = np.zeros(4, _capi.FEELER_DTYPE)
    out, casts = C.c_void_p(1 << 20), C.c_void_p(1 << 21)
    assert lib.mgf_batch_feeler_count(None) == -1
    assert lib.mgf_batch_set_feelers(None, rig.ctypes.data, 4) == INV and "NULL" in err()
    assert lib.mgf_batch_set_feelers(None, None, 0) == INV and "NULL" in err()
    assert lib.mgf_batch_set_feelers(fake, None, 4) == INV and "NULL" in err()
    assert lib.mgf_batch_set_feelers(fake, rig.ctypes.data, -1) == INV and "negative" in err()
    assert lib.mgf_batch_set_feelers(fake, rig.ctypes.data, -(1 << 40)) == INV and "negative" in err()
    assert lib.mgf_batch_set_feelers(fake, rig.ctypes.data, 1 << 31) == INV and "too many" in err()
    for fn in (lib.mgf_batch_cast_feelers, lib.mgf_batch_cast_feelers_dev):
        assert fn(None, 7, out, casts, 4) == INV and "NULL" in err()
        assert fn(fake, 7, out, None, -1) == INV and "negative" in err()
        for mask in (0, 8, 16, -1):
            assert fn(fake, mask, out, casts, 4) == INV and "kinds_mask" in err(), mask
            assert fn(fake, mask, out, None, 0) == INV and "kinds_mask" in err(), mask
    # what needs the handle is refused on the host too, every record ahead of any change of the rig and of any device work (read
    # here; run in tests/test_gpu_world_batch_feelers.py, where a handle exists)
    src = read("mgf_amd", "csrc", RIG_FILE)
    body = src[src.index('extern "C" mgf_status mgf_batch_set_feelers('):src.index('extern "C" int64_t mgf_batch_feeler_count(')]
    plan_call = "batch_rig_plan(b, b->feelers, f, n);"
    assert not re.search(r"b->feelers\.|\bR\.", body.replace(plan_call, ""))                  # the rig changes in the plan step alone
    body = RC.set_call_with_plan(body, plan_call)
    first_change = body.index("R.recs.assign(")
    order = [body.index(s) for s in ("batch_rig_set_args(b, f, n_in)", 'batch_rig_ref_check(b, f[i].world, f[i].body, 0, "feeler")',
                                     "a feeler's flags hold a bit beyond MGF_FEELER_OWN_SHAPE: the rig was not changed",
                                     "without MGF_FEELER_OWN_SHAPE: the rig was not changed",
                                     "MGF_FEELER_OWN_SHAPE without MGF_FEELER_IGNORE_SELF",
                                     "a feeler's reserved words must be 0: the rig was not changed")]
    assert order == sorted(order) and max(order) < first_change, order
    assert body.count("the rig was not changed") == 4
    assert not re.search(r"<<<|Async|hipMalloc|\.ensure\(|h2d\(", body)                       # no device work at all
    args = src[src.index("static mgf_status batch_feeler_args("):src.index('extern "C" mgf_status mgf_batch_cast_feelers(')]
    RC.assert_the_read_and_cast_refusals(args, ["batch_rig_cap(cap)", "query_mask_check(kinds_mask)"])


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def test_both_pointers_are_looked_up_before_the_first_enqueue_and_the_rig_file_repeats_nothing():
    src = read("mgf_amd", "csrc", RIG_FILE)
    run = src[src.index('extern "C" mgf_status mgf_batch_cast_feelers_dev('):]
    enqueue = (r"batch_feeler_run\(|batch_rig_up\(|batch_rig_upload\(|batch_ray_obstacles\(|batch_sweep_tail\(|batch_push\(|batch_dev_begin\(|batch_env_sync\(|"
               r"batch_cols_refresh\(|hipMemsetAsync|hipMemcpyAsync|<<<|prim_exclusive_scan_u32|\.ensure\(|h2d\(")
    first_enqueue = min(m.start() for m in re.finditer(enqueue, run))
    checks = [m.start() for m in re.finditer(r"dev_span\(", run)]
    assert len(checks) == 2 and max(checks) < first_enqueue
    for name in ("out_dev, 52 \\* n", "casts_out_dev, 44 \\* n"):
        assert re.search(r"dev_span\(b->ctx, " + name, run), name
    assert run.index('arrays[2] = {{out_dev, 52 * n, "out_dev"}, {casts_out_dev, 44 * n, "casts_out_dev"}};') < run.index("dev_outputs_overlap(arrays, 2, 2)")
    assert max(checks) < run.index("dev_outputs_overlap(") < first_enqueue
    assert run.index("batch_feeler_args(") < run.index("batch_single_parts(b, \"mgf_batch_cast_feelers_dev\")") < run.index("ctx_bind(") < min(checks)
    assert run.index("if (n == 0) return MGF_OK;") < first_enqueue                            # an empty rig enqueues nothing
    assert "hipStreamSynchronize" not in run and "hipMemcpy" not in run                      # it waits for nothing
    host_form = src[src.index('extern "C" mgf_status mgf_batch_cast_feelers('):src.index('extern "C" mgf_status mgf_batch_cast_feelers_dev(')]
    assert host_form.count("hipStreamSynchronize") == 1 and 'batch_single_parts(b, "mgf_batch_cast_feelers")' in host_form
    # everything that launches is batch_feeler_run: its own kernel, then the shared passes over faces and obstacles, unchanged
    helper = src[src.index("static mgf_status batch_feeler_run("):src.index("static mgf_status batch_feeler_args(")]
    assert helper.count("<<<") == 1 and helper.index("k_batch_feeler_bodies<<<") < helper.index("batch_sweep_tail(")
    assert "hipStreamSynchronize" not in helper and "hipMemcpy" not in helper
    assert helper.index("batch_push(") < helper.index('batch_rig_up(b, R, "feeler", 4)') < helper.index("batch_cols_refresh(") < helper.index("k_batch_feeler_bodies<<<")
    assert "b->q_launches += MGF_BATCH_FEELER_LAUNCHES;" in helper
    assert src.count("k_batch_query_sweep_faces") == 0 and src.count("k_batch_query_sweep_obstacles") == 0
    # what tests/test_world_batch_rigs_host.py asks of a rig file
    assert src.count("batch_rig_set_args(b, ") == 1 and src.count("batch_rig_up(b, R, ") == 1
    for gone in ("BatchQueryPlan plan(", "batch_rig_upload(", "names a body its world does not hold", '"batch is NULL"', '"cap is negative"',
                 '"buffer too small"'):
        assert gone not in src, gone
    for fn in ("batch_rig_set_args", "batch_rig_ref_check", "batch_rig_plan", "batch_rig_upload", "batch_rig_up", "batch_rig_handle", "batch_rig_cap", "batch_rig_fits"):
        assert not re.search(r"^static \w+ " + fn + r"\(", src, re.M), fn
    host = read("mgf_amd", "csrc", "host_batch.inc")
    assert host.count("BatchRig<mgf_batch_feeler> feelers;") == 1 and "b->feelers.stale = true;" in RC.stale_step()
    for add in ('extern "C" mgf_status mgf_batch_add_bodies(', 'extern "C" mgf_status mgf_batch_add_compound_bodies('):
        text = host[host.index(add):]
        assert "batch_rigs_stale(b);" in text[:text.index("\n}\n")], add
    # the kernel: every exit and every barrier is the front's; the loader and the store hold neither; its name is off the query prefix
    # (the front is the one k_batch_query_sweep_bodies has - bq_sweep_front, k_batch_query.h - whose other exit is the device plan's,
    # a whole workgroup ahead of the staging, and whose only atomic is the fixed layout's count of skipped casts; the walk over the
    # bodies is the bodies' policy's)
    k, q = read("mgf_amd", "csrc", "k_batch_feeler.h"), read("mgf_amd", "csrc", "k_batch_query.h")
    front = q[q.index("void bq_sweep_front("):]
    front = front[:front.index("\n}\n")]
    assert front.count("return;") == 2 and front.index("return;") < front.index("bodies.stage(") and "__syncthreads" not in front    # (the barriers are bq_stage's and bq_reduce's)
    assert "if (SRC == kItemPlan && blockIdx.x >= *S.n_items) return;" in front and re.findall(r"atomic\w*\([^;]*", front) == ["atomicAdd(S.skipped, 1ull)"]
    assert (front.index("bodies.stage(") < front.index("load(qi, W.g0);") < front.index("bodies.sweep_walk(")
            < front.index("bq_reduce(") < front.index("if (W.sub != 0u || !W.live) return;") < front.index("q_sweep_store(") < front.index("done("))
    plain = q[q.index("struct PlainBodies {"):q.index("void bq_ray_front(")]
    assert "bq_stage(A, g0, n, s_dyn, s_dyn + n);" in plain
    walk = plain[plain.index("SweepBest sweep_walk("):plain.index("Box box(")]
    assert walk.index("q_sweep_far(") < walk.index("comp_mcomp(") < walk.index("best.offer(") and not re.search(r"return;|__syncthreads|atomic", walk)
    body = k[k.index("void bf_casts("):]
    assert "bq_sweep_front<kItemTable>(" in body and not re.search(r"return;|__syncthreads|atomic|bq_stage|bq_reduce", body)
    assert body.count("bf_casts(A, PlainBodies(A), s_dyn);") == 1 and body.index("bq_sweep_front<kItemTable>(") < body.index("void k_batch_feeler_bodies(")
    assert "const float4 a = A.col0[g], b = A.col1[g];" in body              # a body's own shape: the collider rows themselves, whatever was staged
    assert len(re.findall(r"__global__ __launch_bounds__\(kBatchBlock\)", k)) == len(re.findall(r"__global__", k)) == 1
    assert not re.search(r"void k_batch_query_\w+\(", k)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_binding_turns_a_wrong_tensor_down_before_it_calls_c():
    import torch

    class Handle(mgf_amd.WorldBatch):   # no context, no C handle: a call that got as far as C would fail differently
        def __init__(self):
            self._h, self.n_worlds = None, 2

        def feeler_count(self):
            return 4

    b, n = Handle(), 4
    wrong_out = [torch.zeros((n, 13), dtype=torch.float32), torch.zeros((n, 13), dtype=torch.int64), torch.zeros((13, n), dtype=torch.int32).t(),
                 torch.zeros((n - 1, 13), dtype=torch.int32), torch.zeros((n, 12), dtype=torch.int32)]
    wrong_casts = [torch.zeros((n, 11), dtype=torch.float64), torch.zeros((n, 11), dtype=torch.int64), torch.zeros((11, n), dtype=torch.float32).t(),
                   torch.zeros((n - 1, 11), dtype=torch.float32), torch.zeros((n, 10), dtype=torch.float32), torch.zeros((n, 13), dtype=torch.int32)]
    for t in wrong_out:
        with pytest.raises(ValueError) as e:
            b.cast_feelers_dev(t, casts=1 << 21)
        assert "on cpu" not in str(e.value), str(e.value)              # turned down for what it is, not for where it is
    for t in wrong_casts:
        with pytest.raises(ValueError) as e:
            b.cast_feelers_dev(1 << 20, casts=t)
        assert "on cpu" not in str(e.value), str(e.value)
    with pytest.raises(ValueError, match="on cpu"):                     # everything right but the device
        b.cast_feelers_dev(torch.zeros((n, 13), dtype=torch.int32))
    for dtype in (torch.float32, torch.int32):
        with pytest.raises(ValueError, match="on cpu"):
            b.cast_feelers_dev(1 << 20, casts=torch.zeros((n, 11), dtype=dtype))
    with pytest.raises(ValueError, match="required"):
        b.cast_feelers_dev(None)
    with pytest.raises(ValueError, match="not ndarray"):
        b.cast_feelers_dev(np.zeros((n, 13), np.int32))
    with pytest.raises(mgf_amd.MgfError):                               # and a call whose arguments are all in order does reach C
        b.cast_feelers_dev(1 << 20, casts=1 << 21)
    # set_feelers broadcasts scalars and single rows; what reaches C is FEELER_DTYPE rows (no handle: C refuses, after the marshalling)
    with pytest.raises(mgf_amd.MgfError):
        b.set_feelers([0, 1, 1], 0, tag=1, p=(0, 0, 0), d=[(0, 0, 1), (0, 1, 0), (1, 0, 0)], r=0.1, delta=(0, -1, 0), world_delta=[True, False, True])
    with pytest.raises(mgf_amd.MgfError):
        b.set_feelers([0, 1], [0, 0], delta=(0, -1, 0), own_shape=True)
    with pytest.raises(ValueError):
        b.set_feelers([0, 1, 1], [0, 1], delta=(0, 0, 1))              # neither one nor n


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_new_kernel_uses_no_scratch_and_spills_nothing():
    if not os.path.exists(os.path.join(ROOT, "mgf_amd", "libmgf_hip.so")) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    rows = kernel_resources("k_batch_feeler")
    assert set(rows) == {"k_batch_feeler_bodies"}, sorted(rows)
    v = rows["k_batch_feeler_bodies"]
    print("k_batch_feeler_bodies: vgpr, sgpr, scratch, static lds, sgpr spills, vgpr spills =", v)
    assert v[2] == "0" and v[4] == "0" and v[5] == "0", v                # no scratch, no spills
    design = re.sub(r"\s+", " ", read("DESIGN.md"))
    assert "`k_batch_feeler_bodies` %s / %s / 0 / 0 / 0" % (v[0], v[1]) in design, v


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_layouts_hold_what_the_gpu_tests_ask_of_them():
    """from the scenes alone: a world with terrain, one of a single body, one with the ring, one bare; capsules among the bodies; about
    a thousand feelers in shuffled world order, several on one body, every role; the plan's worlds of 0, 1, 256, 257 and 600"""
    scs = FC.feeler_scenes()
    n = [len(sc["comps"]) for sc in scs]
    assert n == [5, 1, 300, 48, 18]
    assert scs[FC.TERRAIN_WORLD]["terrain"] is not None and not scs[FC.TERRAIN_WORLD].get("obstacles")
    assert scs[FC.PILE_WORLD].get("obstacles") and scs[FC.RING_WORLD].get("obstacles") and scs[FC.RING_WORLD]["terrain"] is None
    assert scs[FC.BARE_WORLD]["terrain"] is None and not scs[FC.BARE_WORLD].get("obstacles")
    assert all({0, 1} <= set(sc["comps"]["tag"].tolist()) for k, sc in enumerate(scs) if k != FC.ONE_BODY_WORLD)
    lay = FC.main_layout(scs)
    assert 900 <= len(lay["world"]) <= 1100 and np.any(np.diff(lay["world"]) < 0)
    assert np.all(lay["body"] >= 0) and np.all(lay["body"] < np.int64(n)[lay["world"]])
    for r, least in ((FC.DOWN, 60), (FC.UP, 60), (FC.RING, 40), (FC.ZERO, 20), (FC.OWN, 60), (FC.RANDOM, 400)):
        assert np.sum(lay["role"] == r) >= least, r
    key = lay["world"].astype(np.int64) * 4096 + lay["body"]
    assert np.bincount(np.unique(key, return_inverse=True)[1]).max() >= 4
    for i in np.flatnonzero(lay["role"] == FC.RING):
        assert scs[lay["world"][i]].get("obstacles"), i
    plan = FC.plan_layout(scs)
    assert np.bincount(plan["world"], minlength=5).tolist() == list(SC.PLAN_COUNTS) and np.any(np.diff(plan["world"]) < 0)
    assert np.all(plan["body"] < np.int64(n)[plan["world"]])
    # aimed from the scenes' own poses (q the identity): every flag word the set call allows, both tags, a zero delta
    state = dict(x=np.concatenate([SC.centres(sc) for sc in scs]).astype(np.float32), q=np.tile(np.float32([1, 0, 0, 0]), (sum(n), 1)))
    rig = FC.aimed_rig(lay, scs, state, n)
    assert set(rig["flags"].tolist()) == set(FC.ALLOWED_FLAGS)
    plain = (rig["flags"] & FC.OWN_SHAPE) == 0
    assert set(rig["tag"][plain].tolist()) == {0, 1} and np.all(rig["reserved"] == 0)
    assert np.any(np.all(rig["delta"] == 0, axis=1))
