"""The zones of a batch read nearest first (mgf_batch_read_zones_nearest, mgf_batch_read_zones_nearest_dev, mgf_batch_overlap_nearest_dev)
without a GPU: the header, the library, the binding and the documents carry the three calls with matching arities; what can be refused
before a device is looked at is refused there, before the handle is dereferenced; both device forms look every pointer up before they
enqueue anything; the binding turns a wrong tensor down before it calls C; the numpy restatement the GPU tests hold the kernel to
(tests/batch_nearest_cases.py) agrees with a brute-force sort, on the tie scene and on the zones' scenes; those scenes hold the cases
the GPU tests rely on; and the new kernel uses no scratch and no static LDS."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mgf_amd
from mgf_amd import _capi
from tests import batch_nearest_cases as NC
from tests import batch_zone_cases as ZC
from tests.util import ROOT, kernel_resources, read

CALLS = ("mgf_batch_read_zones_nearest", "mgf_batch_read_zones_nearest_dev", "mgf_batch_overlap_nearest_dev")
f32 = np.float32


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
def test_header_library_binding_and_documents_carry_the_calls():
    h = read("include", "mgf_hip.h")
    for sig in (r"mgf_status mgf_batch_read_zones_nearest\(mgf_batch\* b, int32_t k, int32_t\* out, float\* dist2_out, mgf_aabb\* boxes_out, int64_t cap\);",
                r"mgf_status mgf_batch_read_zones_nearest_dev\(mgf_batch\* b, int32_t k, int32_t\* out_dev, float\* dist2_out_dev, mgf_aabb\* boxes_out_dev,\s*"
                r"int64_t cap\);",
                r"mgf_status mgf_batch_overlap_nearest_dev\(mgf_batch\* b, const mgf_aabb\* boxes_dev, int64_t n, const int32_t\* ignore_body_dev, int32_t k,\s+"
                r"int32_t\* out_dev, float\* dist2_out_dev\);"):
        assert re.search(r"MGF_API " + sig, h), sig
    m = re.search(r"#define MGF_BATCH_ZONE_NEAREST_MAX_K (\d+)", h)
    assert m and int(m.group(1)) == _capi.BATCH_ZONE_NEAREST_MAX_K == NC.MAX_K == 32 == max(NC.KS)
    m = re.search(r"#define MGF_BATCH_NEAREST_LAUNCHES (\d+)", h)
    assert m and int(m.group(1)) == _capi.BATCH_NEAREST_LAUNCHES == 1
    # directly behind the zones section, which now points here where it left nearest-first ordering out
    assert h.index("mgf_batch_overlap_first_dev(") < h.index("---- box zones, nearest first") < h.index("mgf_batch_read_zones_nearest(") < h.index("MGF_API mgf_status mgf_batch_counter(")
    zones = h[h.index("---- box zones:"):h.index("---- box zones, nearest first")]
    assert "nearest-first ordering" not in zones and '"box zones, nearest first"' in zones[zones.index("OUT OF SCOPE"):]
    section = h[h.index("---- box zones, nearest first"):h.index("MGF_API mgf_status mgf_batch_counter(")]
    for word in ("c = x + rotate(q, p)", "c = p for body = -1", "MGF_SENSOR_IGNORE_SELF", "bounds.rs:170-188", "a + d * 0.5", "e = m_i - c",
                 "d2_i = (e.x * e.x + e.y * e.y) + e.z * e.z", "no fused multiply-add", "never NaN", "[+0, +inf]", "total order", "the full count",
                 "ascending (d2, body index)", "the rest are -1", "+INFINITY (0x7F800000)", "defined to the bit", "MGF_BATCH_ZONE_NEAREST_MAX_K = 32",
                 "several components", "MGF_ERR_CAPACITY", "nothing enqueued", "4 (1 + k)", "4 k", "multiple of n_worlds", "OUT OF SCOPE",
                 "k is outside [0, MGF_BATCH_ZONE_NEAREST_MAX_K]"):
        assert word in re.sub(r"\s*\n \* ", " ", section), word
    lib = mgf_amd.load_library()
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    want = {"mgf_batch_read_zones_nearest": (i32, [vp, i32, vp, vp, vp, i64]), "mgf_batch_read_zones_nearest_dev": (i32, [vp, i32, vp, vp, vp, i64]),
            "mgf_batch_overlap_nearest_dev": (i32, [vp, vp, i64, vp, i32, vp, vp])}
    for name in CALLS:
        assert name in _capi.SYMBOLS, name
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == want[name], name
    for method in ("read_zones_nearest", "read_zones_nearest_dev", "overlap_nearest_dev"):
        assert callable(getattr(mgf_amd.WorldBatch, method)), method
    flat = re.sub(r"\s+", " ", read("INTEGRATION.md"))
    for sig in ("pub fn mgf_batch_read_zones_nearest(b: *mut mgf_batch, k: i32, out: *mut i32, dist2_out: *mut f32, boxes_out: *mut mgf_aabb, cap: i64) -> mgf_status;",
                "pub fn mgf_batch_read_zones_nearest_dev(b: *mut mgf_batch, k: i32, out_dev: *mut i32, dist2_out_dev: *mut f32, boxes_out_dev: *mut mgf_aabb, "
                "cap: i64) -> mgf_status;",
                "pub fn mgf_batch_overlap_nearest_dev(b: *mut mgf_batch, boxes_dev: *const mgf_aabb, n: i64, ignore_body_dev: *const i32, k: i32, "
                "out_dev: *mut i32, dist2_out_dev: *mut f32) -> mgf_status;"):
        assert sig in flat, sig
    kernels = read("mgf_amd", "csrc", "kernels.h")
    assert kernels.index('#include "k_batch_zone.h"') < kernels.index('#include "k_batch_nearest.h"') and "k_batch_nearest<SRC> (k_batch_nearest.h)" in kernels
    hip = read("mgf_amd", "csrc", "mgf_hip.hip")
    assert hip.index('#include "host_batch_zone.inc"') < hip.index('#include "host_batch_nearest.inc"')
    design = read("DESIGN.md")
    sub = design[design.index("Box zones, nearest first"):]
    for word in ("k_batch_nearest", "d2 = (e.x * e.x + e.y * e.y) + e.z * e.z", "Out of scope", "batch_nearest_bench.py", "Compiler output"):
        assert word in sub, word
    readme = read("README.md")
    assert "read_zones_nearest" in readme and "read_zones_nearest_dev" in readme and "overlap_nearest_dev" in readme
    assert os.path.exists(os.path.join(ROOT, "tools", "batch_nearest_bench.py"))


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def test_what_needs_no_device_is_refused_before_the_handle_is_dereferenced():
    lib = mgf_amd.load_library()
    INV = _capi.ERR_INVALID

    def err():
        return lib.mgf_last_error().decode()
    fake = C.c_void_p(16)   # a handle that is never dereferenced; addresses that are never looked up
    out, d2, boxes, ign = C.c_void_p(1 << 20), C.c_void_p(1 << 23), C.c_void_p(1 << 21), C.c_void_p(1 << 22)
    bad_k = (-1, _capi.BATCH_ZONE_NEAREST_MAX_K + 1, 64, _capi.BATCH_MAX_BODIES, -(1 << 31), (1 << 31) - 1)
    for fn in (lib.mgf_batch_read_zones_nearest, lib.mgf_batch_read_zones_nearest_dev):
        assert fn(None, 8, out, d2, boxes, 4) == INV and "NULL" in err()
        for k in bad_k:
            assert fn(fake, k, out, d2, boxes, 4) == INV and "k is outside [0, MGF_BATCH_ZONE_NEAREST_MAX_K]" in err(), k
            assert fn(fake, k, None, None, None, 0) == INV and "k is outside" in err(), k
            assert fn(fake, k, out, None, None, -1) == INV and "k is outside" in err(), k        # the k check comes ahead of a negative cap
        for k in (0, 8, 32):
            assert fn(fake, k, out, None, None, -1) == INV and "negative" in err(), k
            assert fn(fake, k, out, d2, boxes, -(1 << 40)) == INV and "negative" in err(), k
    fn = lib.mgf_batch_overlap_nearest_dev
    assert fn(None, boxes, 4, ign, 8, out, d2) == INV and "NULL" in err()
    assert fn(fake, boxes, -1, ign, 8, out, d2) == INV and "negative" in err()
    assert fn(fake, boxes, 1 << 31, ign, 8, out, d2) == INV and "too many" in err()
    assert fn(fake, None, 4, ign, 8, out, d2) == INV and "NULL" in err()
    assert fn(fake, boxes, 4, None, 8, None, d2) == INV and "NULL" in err()             # a NULL out with n > 0
    assert fn(fake, boxes, 4, None, 33, None, None) == INV and "NULL" in err()          # ... ahead of k, as in mgf_batch_overlap_first_dev
    for k in bad_k:
        assert fn(fake, boxes, 4, ign, k, out, d2) == INV and "k is outside [0, MGF_BATCH_ZONE_NEAREST_MAX_K]" in err(), k
        assert fn(fake, None, 0, None, k, None, None) == INV and "k is outside" in err(), k
    # what needs the handle - cap below the count, NULL out with a rig that is not empty, several components - comes behind these and
    # ahead of any device work (read here; run in tests/test_gpu_world_batch_nearest.py, where a handle exists)
    src = read("mgf_amd", "csrc", "host_batch_nearest.inc")
    args = src[src.index("static mgf_status batch_nearest_read_args("):src.index('extern "C" mgf_status mgf_batch_read_zones_nearest(')]
    assert (args.index("batch_rig_handle(b)") < args.index("nearest_k_check(k)") < args.index("batch_rig_cap(cap)") < args.index("b->zones.recs.size()")
            < args.index("batch_rig_fits(*n, cap, out != nullptr)"))
    assert args.index("b->") > args.index("batch_rig_cap(cap)")                           # nothing of the handle is read before them
    for name in CALLS:
        body = src[src.index('extern "C" mgf_status %s(' % name):]
        body = body[:body.index("\n}\n")]
        assert f'batch_single_parts(b, "{name}")' in body and body.index("batch_single_parts(") < body.index("ctx_bind(") < body.index("batch_call_begin(b)"), name
    # the rig is the zones' and is only read: no set call here, no member of the handle beside it and the zones' download buffer
    assert "b->zones" in src and "b->sensors" not in src and "b->cameras" not in src and "R.recs.assign(" not in src and "batch_rig_plan(" not in src
    assert set(re.findall(r"b->(\w+)", src)) <= {"zones", "ctx", "dm", "q_launches", "z_out", "K"}
    # and neither the zones' host file nor their kernel file names anything of this
    for f in ("host_batch_zone.inc", "k_batch_zone.h", "k_batch_observe.h"):
        assert "nearest" not in read("mgf_amd", "csrc", f).lower(), f


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
ENQUEUE = (r"batch_nearest_run\(|batch_rig_up\(|batch_rig_upload\(|batch_push\(|batch_dev_begin\(|batch_env_sync\(|batch_cols_refresh\(|hipMemsetAsync|"
           r"hipMemcpyAsync|<<<|prim_exclusive_scan_u32|\.ensure\(|h2d\(")


def test_both_device_forms_look_every_pointer_up_before_the_first_enqueue():
    src = read("mgf_amd", "csrc", "host_batch_nearest.inc")
    run = src[src.index('extern "C" mgf_status mgf_batch_read_zones_nearest_dev('):src.index("// The same kernel over boxes the caller computed")]
    first_enqueue = min(m.start() for m in re.finditer(ENQUEUE, run))
    checks = [m.start() for m in re.finditer(r"dev_span\(", run)]
    assert len(checks) == 3 and max(checks) < first_enqueue
    assert "out_bytes = 4 * ((size_t)k + 1) * n, dist2_bytes = 4 * (size_t)k * n;" in run
    for name in ("out_dev, out_bytes", "dist2_out_dev, dist2_bytes", "boxes_out_dev, 24 \\* n"):
        assert re.search(r"dev_span\(b->ctx, " + name, run), name
    assert run.index("batch_nearest_read_args(") < run.index("ctx_bind(") < min(checks) and max(checks) < run.index("dev_outputs_overlap(arrays, 3, 3)") < first_enqueue
    assert run.index("if (n == 0) return MGF_OK;") < first_enqueue                   # an empty rig enqueues nothing
    assert "hipStreamSynchronize" not in run and "hipMemcpy" not in run
    run = src[src.index('extern "C" mgf_status mgf_batch_overlap_nearest_dev('):]
    first_enqueue = min(m.start() for m in re.finditer(ENQUEUE, run))
    checks = [m.start() for m in re.finditer(r"dev_span\(", run)]
    assert len(checks) == 4 and max(checks) < first_enqueue
    for name in ("boxes_dev, 24 \\* n", "ignore_body_dev, 4 \\* n", "out_dev, out_bytes", "dist2_out_dev, dist2_bytes"):
        assert re.search(r"dev_span\(b->ctx, " + name, run), name
    assert (run.index("batch_dev_args(") < run.index('"NULL argument"') < run.index("nearest_k_check(") < run.index("ctx_bind(") < run.index("n % b->K")
            < min(checks))
    assert max(checks) < run.index('dev_outputs_overlap(arrays, 4, 2, "an input array")') < first_enqueue
    assert run.index("if (n == 0) return MGF_OK;") < first_enqueue
    assert "hipStreamSynchronize" not in run and "hipMemcpy" not in run
    # everything a rig read enqueues is in batch_nearest_run and batch_rig_up: one launch, counted; no wait, no copy but the rig's
    helper = src[src.index("static mgf_status batch_nearest_run("):src.index("// the refusals of both rig reads")]
    assert helper.count("<<<") == 1 and "k_batch_nearest<kItemTable><<<" in helper and "hipStreamSynchronize" not in helper and "hipMemcpy" not in helper
    assert helper.index("LAUNCH_CHECK();") < helper.index("b->q_launches += MGF_BATCH_NEAREST_LAUNCHES;")
    assert helper.index("batch_push(") < helper.index('batch_rig_up(b, R, "zone", 3, true)') < helper.index("k_batch_nearest<kItemTable><<<")
    assert src.count("<<<") == 2 and src.count("b->q_launches += MGF_BATCH_NEAREST_LAUNCHES;") == 2
    # the host form: one download, one wait
    host = src[src.index('extern "C" mgf_status mgf_batch_read_zones_nearest('):src.index('extern "C" mgf_status mgf_batch_read_zones_nearest_dev(')]
    assert host.count("hipMemcpyAsync(") == 2 and host.count("hipStreamSynchronize(") == 2 and host.index("if (!dwords && !bwords) {") < host.index("hipMemcpyAsync(")
    assert host.index("return MGF_OK;\n  }\n  std::vector<int32_t> h(") > host.index("hipStreamSynchronize(")      # each path: one of each
    # the kernel: no exit, no atomic, no barrier of its own; every loop's bounds are the work item's or the call's
    k = read("mgf_amd", "csrc", "k_batch_nearest.h")
    # (the kernel's body is bn_nearest, written once for this kernel and its part-aware form; the kernel is the one call of it with the
    # plain bodies; the two box loaders and the box store are k_batch_zone.h's)
    body = k[k.index("struct NearestPick {"):]          # the selection's registers, the shared body and the kernel
    assert not re.search(r"return;|break;|continue;|__syncthreads|atomic|__shared__ (?!float4 s_dyn)", body.replace("extern __shared__ float4 s_dyn[];", ""))
    assert not re.search(r"return (?!b;|o;|BatchBox\{|bz_fixed\(A, qi\);|bz_mounted\(A, qi, g0\);)", body)
    zone = read("mgf_amd", "csrc", "k_batch_zone.h")
    loaders = zone[zone.index("BatchBox bz_fixed("):zone.index("void bz_first(")]
    assert not re.search(r"return;|break;|continue;|__syncthreads|atomic|__shared__", loaders) and not re.search(r"return (?!b;|BatchBox\{)", loaders)
    assert body.count("bn_nearest<SRC>(A, PlainBodies(A), S, s_dyn);") == 1 and body.index("void bn_nearest(") < body.index("void k_batch_nearest(")
    assert (body.index("__shfl_xor(") < body.index("void bn_nearest(") < body.index("bo_front<true, true>(") < body.index("for (uint32_t r0 = 0; r0 < k; r0 += 4u)")
            < body.index("for (uint32_t i0 = 0; i0 < n; i0 += L)") < body.index("min(i, n - 1u)") < body.index("live & (i < n) & ((int32_t)i != ign) & hit & (key >= lo)")
            < body.index("best.put(ok ? key : kNearestNone)") < body.index("for (uint32_t off = L >> 1; off > 0u; off >>= 1) best.merge(best.shfl((int)off));")
            < body.index("put(r0, best.t0);") < body.index("if (r0 + 3u < k) put(r0 + 3u, best.t3);") < body.index("o[0] = (int32_t)m"))
    kernel = body[body.index("void bn_nearest("):]
    assert not re.search(r"\bif \((?!first|r0 \+ \du < k|od|A\.boxes_out)", kernel)                    # a trip of the selection has no branch of its own
    assert not re.search(r"\bif \((?!s\.body >= 0)", loaders)
    assert "dot(e, e)" in body and not re.search(r"\bfmaf?\(|__fm", body)
    assert "[" not in re.sub(r"//[^\n]*", "", body[:body.index("// k_batch_nearest<SRC> and its part-aware form")])                  # the four registers by name, never by index
    assert len(re.findall(r"__global__ __launch_bounds__\(kBatchBlock\)", k)) == len(re.findall(r"__global__", k)) == 1


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
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
    wrong_d2 = [torch.zeros((n, k), dtype=torch.float64), torch.zeros((n, k), dtype=torch.int32), torch.zeros((k, n), dtype=torch.float32).t(),
                torch.zeros((n - 1, k), dtype=torch.float32), torch.zeros((n, k + 1), dtype=torch.float32)]
    wrong_boxes = [torch.zeros((n, 6), dtype=torch.float64), torch.zeros((n - 1, 6), dtype=torch.float32), torch.zeros((n, 7), dtype=torch.float32)]
    for t in wrong_out:
        with pytest.raises(ValueError) as e:
            b.read_zones_nearest_dev(t, dist2=1 << 23)
        assert "on cpu" not in str(e.value), str(e.value)              # turned down for what it is, not for where it is
        with pytest.raises(ValueError) as e:
            b.overlap_nearest_dev(1 << 21, t, n=n)
        assert "on cpu" not in str(e.value), str(e.value)
    for t in wrong_d2:
        with pytest.raises(ValueError) as e:
            b.read_zones_nearest_dev(1 << 20, dist2=t, k=k)
        assert "on cpu" not in str(e.value), str(e.value)
        with pytest.raises(ValueError) as e:
            b.overlap_nearest_dev(1 << 21, 1 << 20, dist2=t, n=n, k=k)
        assert "on cpu" not in str(e.value), str(e.value)
    for t in wrong_boxes:
        with pytest.raises(ValueError) as e:
            b.read_zones_nearest_dev(1 << 20, boxes=t, k=k)
        assert "on cpu" not in str(e.value), str(e.value)
        with pytest.raises(ValueError) as e:
            b.overlap_nearest_dev(t, 1 << 20, n=n, k=k)
        assert "on cpu" not in str(e.value), str(e.value)
    with pytest.raises(ValueError, match="on cpu"):                     # everything right but the device
        b.read_zones_nearest_dev(torch.zeros((n, 1 + k), dtype=torch.int32))
    with pytest.raises(ValueError, match="on cpu"):
        b.read_zones_nearest_dev(1 << 20, dist2=torch.zeros((n, k), dtype=torch.float32), k=k)
    with pytest.raises(ValueError, match="on cpu"):
        b.overlap_nearest_dev(1 << 21, 1 << 20, dist2=torch.zeros((n, k), dtype=torch.float32), n=n, k=k)
    with pytest.raises(ValueError, match="required"):
        b.read_zones_nearest_dev(None)
    with pytest.raises(ValueError, match="required"):
        b.overlap_nearest_dev(None, 1 << 20, n=n, k=k)
    with pytest.raises(ValueError, match="k given"):
        b.read_zones_nearest_dev(1 << 20)                               # a raw address says nothing of k
    with pytest.raises(ValueError, match="multiple"):
        b.overlap_nearest_dev(1 << 21, 1 << 20, n=3, k=k)
    with pytest.raises(mgf_amd.MgfError):                               # and a call whose arguments are all in order does reach C
        b.read_zones_nearest_dev(1 << 20, dist2=1 << 23, boxes=1 << 21, k=k)
    with pytest.raises(mgf_amd.MgfError):
        b.overlap_nearest_dev(1 << 21, 1 << 20, dist2=1 << 23, ignore=1 << 22, n=n, k=k)
    with pytest.raises(mgf_amd.MgfError):
        b.read_zones_nearest(k, dist2=True, boxes=True)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def _oracle_tight(scs):
    """per world the BoundedBy<AABB> box of every collider by the oracle's own function"""
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
    return tight


def _oracle_lists(tight, bx, world):
    """per box the bodies of its world whose tight box Overlaps<AABB> it, by the oracle's own function, ascending"""
    from oracle import oracle as O
    L = O.lib()
    out = []
    for q, w in zip(bx, world):
        qb = O.Aabb(O.vec3(q[:3]), O.vec3(q[3:]))
        out.append([i for i, b in enumerate(tight[int(w)]) if L.mgfo_aabb_overlaps(C.byref(b), C.byref(qb))])
    return out


@pytest.fixture(scope="module")
def defined():
    """the scenes, the rig, its boxes before any tick and - by the oracle's two functions - every zone's list; the restated centres"""
    scs, rig, role, tie = NC.scenes_and_rig()
    lengths = ZC.lengths_of(scs)
    bx = ZC.boxes(rig, ZC.initial_state(scs), lengths)
    tight = _oracle_tight(scs)
    ign = ZC.ignore_of(rig)
    lists = [[j for j in lst if j != ign[i]] for i, lst in enumerate(_oracle_lists(tight, bx, rig["world"]))]
    centres = NC.tight_centres(np.concatenate([sc["comps"] for sc in scs]))
    return dict(scs=scs, rig=rig, role=role, tie=tie, lengths=lengths, bx=bx, tight=tight, lists=lists, centres=centres)


def test_the_restated_centre_is_the_tight_boxs_centre_and_d2_is_the_three_step_sum(defined):
    flat = [b for row in defined["tight"] for b in row]
    got = defined["centres"]
    assert got.dtype == f32 and len(flat) == len(got) == sum(defined["lengths"])
    want = f32([(b.c.x, b.c.y, b.c.z) for b in flat])
    comps = np.concatenate([sc["comps"] for sc in defined["scs"]])
    sph = comps["tag"] == 0
    # a sphere's c as given; a capsule's a + d * 0.5, each operation an f32 one
    assert np.any(sph) and np.any(~sph) and got[sph].tobytes() == comps["p"][sph].tobytes()
    assert got[~sph].tobytes() == (comps["p"][~sph] + comps["d"][~sph] * f32(0.5)).astype(f32).tobytes() and got[~sph].tobytes() != comps["p"][~sph].tobytes()
    # The oracle's entry point answers with the bounds of the collider swept by zero - combine(s, s + 0), which forms the centre again
    # from the corners c - r and c + r (r < 1) - so it holds the restatement to a few units in the last place of the corners only
    assert np.all(np.abs(got.astype(np.float64) - want) <= 4 * np.spacing(np.abs(want) + f32(1.0)))
    # d2: the order of the sum matters - (x2 + y2) + z2, not x2 + (y2 + z2) - and no product is fused into it
    e = f32([[1.0, 2.0 ** -12, 2.0 ** -12], [2.0 ** -12, 2.0 ** -12, 1.0], [1.0 + 2.0 ** -12, 2.0 ** -12, 0.0]])
    d = NC.dist2(e, (0.0, 0.0, 0.0))
    assert float(d[0]) == 1.0 and float(d[1]) == 1.0 + 2.0 ** -23                     # 2^-24 is lost against 1 on its own; two of them summed first are not
    assert float(d[2]) == 1.0 + 2.0 ** -11                                            # the square of 1 + 2^-12 rounds before the add: its 2^-24 is gone ...
    assert float(f32((1.0 + 2.0 ** -12) ** 2 + 2.0 ** -24)) == 1.0 + 2.0 ** -11 + 2.0 ** -23     # ... which a fused product would have kept
    assert NC.dist2(f32([[3.0, 4.0, 12.0]]), (0.0, 0.0, 0.0))[0] == 169.0 and NC.dist2(f32([[1.0, 1.0, 1.0]]), f32([1.0, 1.0, 1.0]))[0].tobytes() == f32(0.0).tobytes()
    with np.errstate(over="ignore"):
        assert np.isinf(NC.dist2(f32([[3e19, 0.0, 0.0]]), (-3e19, 0.0, 0.0))[0])
    # the record: count, the nearest first, ties by index, -1 and +inf behind them
    rec, dd = NC.record([2, 5, 9, 11], f32([4.0, 1.0, 4.0, 0.0]), 3)
    assert rec.tolist() == [4, 11, 5, 2] and dd.tolist() == [0.0, 1.0, 4.0] and rec.dtype == np.int32 and dd.dtype == f32
    rec, dd = NC.record([2, 5, 9, 11], f32([4.0, 1.0, 4.0, 0.0]), 6)
    assert rec.tolist() == [4, 11, 5, 2, 9, -1, -1] and dd.view(np.uint32).tolist() == [0, 0x3F800000, 0x40800000, 0x40800000, NC.INF_BITS, NC.INF_BITS]
    rec, dd = NC.record([], f32([]), 2)
    assert rec.tolist() == [0, -1, -1] and dd.view(np.uint32).tolist() == [NC.INF_BITS] * 2
    rec, dd = NC.record([7, 8], f32([np.inf, 1.0]), 0)
    assert rec.tolist() == [2] and dd.shape == (0,)
    rec, dd = NC.record([7, 8, 9], f32([np.inf, 1.0, np.inf]), 3)
    assert rec.tolist() == [3, 8, 7, 9] and dd.tolist() == [1.0, np.inf, np.inf]    # an overflowed d2 reads +inf too: the count says which are real


def test_the_definition_agrees_with_a_brute_force_sort_on_the_tie_scene_and_the_zone_scenes(defined):
    rig, lists, lengths, bx = defined["rig"], defined["lists"], defined["lengths"], defined["bx"]
    off = np.concatenate([[0], np.cumsum([len(lst) for lst in lists])])
    bodies = np.concatenate([np.int64(lst) for lst in lists])
    first = np.concatenate([[0], np.cumsum(lengths)])
    for k in NC.KS:
        rec, dd = NC.records(off, bodies, np.full(len(rig), -1), rig["world"], bx, defined["centres"], lengths, k)   # (the lists have the ignored body out already)
        assert rec.shape == (len(rig), 1 + k) and dd.shape == (len(rig), k) and rec.dtype == np.int32 and dd.dtype == f32
        for i, lst in enumerate(lists):
            d2 = NC.dist2(defined["centres"][first[rig["world"][i]] + np.int64(lst)], bx[i, :3]) if lst else f32([])
            want, want_d = NC.brute_record(lst, d2, k)
            assert rec[i].tolist() == want and dd[i].tolist() == want_d, (k, i)
    # and with the ignored bodies still in the lists, taken out by `records` itself
    full = _oracle_lists(defined["tight"], bx, rig["world"])
    off2 = np.concatenate([[0], np.cumsum([len(lst) for lst in full])])
    rec2, dd2 = NC.records(off2, np.concatenate([np.int64(lst) for lst in full]), ZC.ignore_of(rig), rig["world"], bx, defined["centres"], lengths, 8)
    rec, dd = NC.records(off, bodies, np.full(len(rig), -1), rig["world"], bx, defined["centres"], lengths, 8)
    assert rec2.tobytes() == rec.tobytes() and dd2.tobytes() == dd.tobytes() and any(len(a) != len(b) for a, b in zip(full, lists))


def test_the_scenes_hold_the_cases_the_gpu_tests_rely_on(defined):
    scs, rig, lists, lengths, bx = defined["scs"], defined["rig"], defined["lists"], defined["lengths"], defined["bx"]
    w_tie, nodes, centre, at = defined["tie"]
    assert lengths == [5, 0, 1, 300, 27] and w_tie == 4 and np.bincount(rig["world"]).tolist() == list(ZC.COUNTS) + [3]
    count = np.int64([len(lst) for lst in lists])
    first = np.concatenate([[0], np.cumsum(lengths)])
    d2 = [NC.dist2(defined["centres"][first[rig["world"][i]] + np.int64(lst)], bx[i, :3]) if lst else f32([]) for i, lst in enumerate(lists)]
    assert np.any(count == 0) and count.max() == 300
    for k in (1, 8, 32):
        assert np.any((count > 0) & (count < k)) or k == 1, k
        assert np.any(count > k) and np.any(count == 1), k
    assert np.sum(count > 32) >= 3 and np.any((count > 8) & (count < 32))
    # a zone whose nearest-first order is not its index order within the first k: what the first-k record cannot give
    reordered = [i for i, lst in enumerate(lists) if len(lst) > 8 and np.argsort(d2[i], kind="stable")[:8].tolist() != list(range(8))]
    assert len(reordered) >= 20, len(reordered)
    # a d2 of exactly +0: a zone at its own body's centre that lists the body
    zero = [i for i in range(len(rig)) if len(d2[i]) and d2[i].min() == 0.0]
    assert len(zero) >= 3 and all(d2[i].view(np.uint32).min() == 0 for i in zero)
    # the tie world: every coordinate exact, the capsules' tight centres at their nodes, the four shells
    tie = scs[w_tie]["comps"]
    assert np.sum(tie["tag"] == 1) == 2 and NC.tight_centres(tie).tobytes() == nodes.tobytes()
    caps = np.flatnonzero(tie["tag"] == 1)
    assert (nodes[caps[0]] + nodes[caps[1]]).tolist() == (2 * f32(NC.TIE_CENTRE)).tolist()          # mirrored about the centre
    assert nodes[centre].tolist() == list(NC.TIE_CENTRE) and tie["tag"][centre] == 0
    assert np.any(np.diff(np.lexsort(nodes.T[::-1])) != 1)                                            # the body order is not the lattice's
    fixed, seen, ignored = (int(i) for i in at)
    assert rig["body"][fixed] == -1 and rig["body"][seen] == rig["body"][ignored] == centre and rig["flags"][ignored] == ZC.IGNORE_SELF
    assert bx[fixed].tobytes() == bx[seen].tobytes() == bx[ignored].tobytes()
    assert lists[fixed] == lists[seen] == list(range(27)) and lists[ignored] == [j for j in range(27) if j != centre]
    vals, mult = np.unique(d2[fixed], return_counts=True)
    assert vals.tolist() == list(NC.TIE_D2) and mult.tolist() == list(NC.TIE_SHELLS)
    rec, dd = NC.record(lists[fixed], d2[fixed], 32)
    assert rec[0] == 27 and rec[1] == centre and dd[:27].tolist() == sum(([v] * m for v, m in zip(NC.TIE_D2, NC.TIE_SHELLS)), [])
    for lo, hi in ((2, 8), (8, 20), (20, 28)):                                                       # within a shell: ascending index, nothing else
        shell = rec[lo:hi]
        assert np.all(np.diff(shell) > 0) and len(set(d2[fixed][shell].tolist())) == 1, (lo, hi)
    assert np.any(np.diff(rec[1:28]) < 0)                                                             # ... and across shells it is not
    rec_i, dd_i = NC.record(lists[ignored], d2[ignored], 32)
    assert rec_i[0] == 26 and rec_i[1:27].tolist() == rec[2:28].tolist() and dd_i[:26].tolist() == dd[1:27].tolist() and np.isinf(dd_i[26:]).all()
    # k = 8 cuts the shell of 12 in two: the tie at the cut is decided by index
    assert NC.record(lists[fixed], d2[fixed], 8)[0][1:].tolist() == rec[1:9].tolist() and dd[7] == dd[8]
    # the fixed layouts cover the tie world too
    for per in ZC.PERS:
        fb, fi = ZC.fixed_boxes(scs, per)
        assert fb.shape == (5 * per, 6) and fi.shape == (5 * per,)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_new_kernel_uses_no_scratch_and_no_static_lds_and_keeps_the_figures_the_design_records():
    if not os.path.exists(os.path.join(ROOT, "mgf_amd", "libmgf_hip.so")) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    rows = kernel_resources("k_batch_nearest")
    assert set(rows) == {"k_batch_nearest<0>", "k_batch_nearest<2>"}, sorted(rows)
    design = re.sub(r"\s+", " ", read("DESIGN.md"))
    for name, v in rows.items():
        assert (v[2], v[3], v[4], v[5]) == ("0", "0", "0", "0"), (name, v)       # no scratch, no static LDS, no spills
        assert int(v[0]) <= 64, (name, v)                                         # eight waves a SIMD at 64 VGPRs
        assert f"`{name}` {v[0]} / {v[1]} / 0 / 0 / 0" in design, (name, v)       # the line DESIGN.md records
    k = read("mgf_amd", "csrc", "k_batch_nearest.h")
    assert "__shared__" not in k.replace("extern __shared__ float4 s_dyn[];", "")
