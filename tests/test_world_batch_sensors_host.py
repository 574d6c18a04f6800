"""The body-mounted ray sensors of a batch (mgf_batch_set_sensors, mgf_batch_sensor_count, mgf_batch_cast_sensors,
mgf_batch_cast_sensors_dev) without a GPU: the numpy restatement of the definition the GPU tests hold the kernel to equals the oracle's
mgfo_rotate_vector bit for bit; the header, the library, the binding and INTEGRATION.md carry the calls; what can be refused before a
device is looked at is refused there; mgf_batch_cast_sensors_dev looks both pointers up before it enqueues anything; the binding turns
a wrong tensor down before it calls C; the new kernel uses no scratch and spills nothing and DESIGN.md records the query kernels'
figures (held to the build, as the plan of a rig is, in tests/test_world_batch_rigs_host.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mgf_amd
from mgf_amd import _capi
from tests import batch_query_device_cases as QD
from tests import batch_rig_cases as RC
from tests import batch_sensor_cases as SC
from tests.util import RESOURCES, ROOT, kernel_resources, read

CALLS = ("mgf_batch_set_sensors", "mgf_batch_sensor_count", "mgf_batch_cast_sensors", "mgf_batch_cast_sensors_dev")


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_restatement_is_the_oracles_rotate_vector_bit_for_bit():
    """a few hundred seeded quaternions and vectors - unit and not, with denormal-sized and 1e4-sized components among them - through
    SC.rotate and through mgfo_rotate_vector: equal bits, so that the GPU tests' reference is anchored to the oracle, not to itself"""
    from oracle import oracle as O
    rng = np.random.default_rng(17)
    n = 400
    q = rng.normal(0, 1, (n, 4))
    q[: n // 2] /= np.linalg.norm(q[: n // 2], axis=1, keepdims=True)
    v = rng.normal(0, 1, (n, 3)) * rng.choice([1.0, 1e-3, 30.0], (n, 1))
    v[::7] *= 1e4                                    # 1e4-sized
    v[3::11, rng.integers(0, 3)] = 1e-41             # a denormal component
    q[5::13, 1 + rng.integers(0, 3)] = 3e-42
    v[10], q[11] = 0.0, (1.0, 0.0, 0.0, 0.0)
    q, v = q.astype(np.float32), v.astype(np.float32)
    assert np.any((np.abs(v) > 0) & (np.abs(v) < 1.1754944e-38)) and np.any(np.abs(v) > 1e4)
    got = SC.rotate(q, v)
    want = np.empty_like(got)
    lib = O.lib()
    for i in range(n):
        out = O.Vec3()
        lib.mgfo_rotate_vector(C.byref(O.Quat(*q[i].tolist())), C.byref(O.Vec3(*v[i].tolist())), C.byref(out))
        want[i] = (out.x, out.y, out.z)
    assert got.tobytes() == want.tobytes(), np.flatnonzero(np.any(got.view(np.uint32) != want.view(np.uint32), axis=1))
    # and the sum is a plain f32 add
    x = rng.normal(0, 5, (n, 3)).astype(np.float32)
    P, D = SC.particles(x, q, v, v)
    assert P.tobytes() == (x + want).tobytes() and D.tobytes() == want.tobytes() and P.dtype == np.float32


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def test_header_library_binding_and_documents_carry_the_calls():
    h = read("include", "mgf_hip.h")
    for sig in (r"mgf_status mgf_batch_set_sensors\(mgf_batch\* b, const mgf_batch_sensor\* s, int64_t n\);",
                r"int64_t mgf_batch_sensor_count\(const mgf_batch\* b\);",
                r"mgf_status mgf_batch_cast_sensors\(mgf_batch\* b, int32_t kinds_mask, mgf_ray_hit\* out, mgf_particle\* parts_out, int64_t cap\);",
                r"mgf_status mgf_batch_cast_sensors_dev\(mgf_batch\* b, int32_t kinds_mask, mgf_ray_hit\* out_dev, mgf_particle\* parts_out_dev, int64_t cap\);"):
        assert re.search(r"MGF_API " + sig, h), sig
    assert h.index("mgf_batch_sweep_many_dev(") < h.index("typedef struct mgf_batch_sensor")      # behind the device-pointer queries
    assert re.search(r"typedef struct mgf_batch_sensor \{ int32_t world, body; mgf_vec3 p, d; float dt; int32_t flags; \} mgf_batch_sensor;", h)
    m = re.search(r"#define MGF_SENSOR_IGNORE_SELF (\d+)", h)
    assert m and int(m.group(1)) == _capi.SENSOR_IGNORE_SELF == 1 == SC.IGNORE_SELF
    m = re.search(r"#define MGF_BATCH_SENSOR_LAUNCHES (\d+)", h)
    assert m and int(m.group(1)) == _capi.BATCH_SENSOR_LAUNCHES == 1
    section = h[h.index("body-mounted ray sensors"):]
    for word in ("P = x + rotate(q, p)", "D = rotate(q, d)", "WITHOUT delta", "AT ONCE", "the colliders move at the next tick", "bit for bit",
                 "MGF_ERR_CAPACITY", "nothing enqueued", "mgf_batch_add_bodies"):
        assert word in section, word
    assert C.sizeof(_capi.BatchSensor) == 40 == _capi.SENSOR_DTYPE.itemsize
    assert [f[0] for f in _capi.BatchSensor._fields_] == list(_capi.SENSOR_DTYPE.names) == ["world", "body", "p", "d", "dt", "flags"]
    assert [_capi.SENSOR_DTYPE.fields[k][1] for k in _capi.SENSOR_DTYPE.names] == [0, 4, 8, 20, 32, 36]
    lib = mgf_amd.load_library()
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    want = {"mgf_batch_set_sensors": (i32, [vp, vp, i64]), "mgf_batch_sensor_count": (i64, [vp]),
            "mgf_batch_cast_sensors": (i32, [vp, i32, vp, vp, i64]), "mgf_batch_cast_sensors_dev": (i32, [vp, i32, vp, vp, i64])}
    for name in CALLS:
        assert name in _capi.SYMBOLS, name
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == want[name], name
    for method in ("set_sensors", "sensor_count", "cast_sensors", "cast_sensors_dev"):
        assert callable(getattr(mgf_amd.WorldBatch, method)), method
    flat = re.sub(r"\s+", " ", read("INTEGRATION.md"))
    for sig in ("pub fn mgf_batch_set_sensors(b: *mut mgf_batch, s: *const mgf_batch_sensor, n: i64) -> mgf_status;",
                "pub fn mgf_batch_sensor_count(b: *const mgf_batch) -> i64;",
                "pub fn mgf_batch_cast_sensors(b: *mut mgf_batch, kinds_mask: i32, out: *mut mgf_ray_hit, parts_out: *mut mgf_particle, cap: i64) -> mgf_status;",
                "pub fn mgf_batch_cast_sensors_dev(b: *mut mgf_batch, kinds_mask: i32, out_dev: *mut mgf_ray_hit, parts_out_dev: *mut mgf_particle, cap: i64) -> mgf_status;",
                "pub struct mgf_batch_sensor"):
        assert sig in flat, sig
    kernels = read("mgf_amd", "csrc", "kernels.h")
    assert kernels.index('#include "k_batch_query_dev.h"') < kernels.index('#include "k_batch_sensor.h"') and "k_batch_sensor_ray" in kernels
    hip = read("mgf_amd", "csrc", "mgf_hip.hip")
    assert hip.index('#include "host_batch_query_dev.inc"') < hip.index('#include "host_batch_sensor.inc"')
    design = read("DESIGN.md")
    sub = design[design.index("Body-mounted sensors"):]
    for word in ("k_batch_sensor_ray", "P = x + rotate(q, p)", "Out of scope", "batch_sensor_bench.py", "Compiler output"):
        assert word in sub, word
    readme = read("README.md")
    assert "set_sensors" in readme and "cast_sensors_dev" in readme
    assert os.path.exists(os.path.join(ROOT, "tools", "batch_sensor_bench.py"))


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_what_needs_no_device_is_refused_before_the_handle_is_dereferenced():
    lib = mgf_amd.load_library()
    INV = _capi.ERR_INVALID

    def err():
        return lib.mgf_last_error().decode()
    fake = C.c_void_p(16)   # a handle that is never dereferenced; addresses that are never looked up
    rig = np.zeros(4, _capi.SENSOR_DTYPE)
    out, parts = C.c_void_p(1 << 20), C.c_void_p(1 << 21)
    assert lib.mgf_batch_sensor_count(None) == -1
    assert lib.mgf_batch_set_sensors(None, rig.ctypes.data, 4) == INV and "NULL" in err()
    assert lib.mgf_batch_set_sensors(None, None, 0) == INV and "NULL" in err()
    assert lib.mgf_batch_set_sensors(fake, None, 4) == INV and "NULL" in err()
    assert lib.mgf_batch_set_sensors(fake, rig.ctypes.data, -1) == INV and "negative" in err()
    assert lib.mgf_batch_set_sensors(fake, rig.ctypes.data, -(1 << 40)) == INV and "negative" in err()
    assert lib.mgf_batch_set_sensors(fake, rig.ctypes.data, 1 << 31) == INV and "too many" in err()
    for fn in (lib.mgf_batch_cast_sensors, lib.mgf_batch_cast_sensors_dev):
        assert fn(None, 7, out, parts, 4) == INV and "NULL" in err()
        assert fn(fake, 7, out, None, -1) == INV and "negative" in err()
        for mask in (0, 8, -1, 16):
            assert fn(fake, mask, out, parts, 4) == INV and "kinds_mask" in err(), mask
            assert fn(fake, mask, out, None, 0) == INV and "kinds_mask" in err(), mask
    assert lib.mgf_batch_sensor_count(None) == -1
    # what needs the handle - a world or a body out of range, a flag bit beyond the one defined, cap below the count - is refused on the
    # host too, ahead of any device work (read here; run in tests/test_gpu_world_batch_sensors.py, where a handle exists)
    src = read("mgf_amd", "csrc", "host_batch_sensor.inc")
    body = src[src.index('extern "C" mgf_status mgf_batch_set_sensors('):src.index('extern "C" int64_t mgf_batch_sensor_count(')]
    assert not re.search(r"b->sensors\.|\bR\.", body.replace("batch_rig_plan(b, b->sensors, s, n);", ""))   # the rig changes in the plan step alone
    body = RC.set_call_with_plan(body, "batch_rig_plan(b, b->sensors, s, n);")  # the set call together with the shared plan step
    first_change = body.index("R.recs.assign(")
    assert body.index("batch_rig_set_args(b, s, n_in)") < first_change
    assert body.index("batch_rig_ref_check(b, s[i].world, s[i].body, s[i].flags, \"sensor\")") < first_change   # every record, ahead of any change
    check = RC.ref_check_step()
    assert (check.index("world index out of range: the rig was not changed") < check.index("body index out of range: the rig was not changed")
            < check.index("a %s's flags hold a bit beyond MGF_SENSOR_IGNORE_SELF: the rig was not changed") < check.index("return MGF_OK;"))
    assert not re.search(r"<<<|Async|hipMalloc|\.ensure\(|h2d\(|b->\w+ =[^=]", check)    # it refuses; it changes nothing
    assert not re.search(r"<<<|Async|hipMalloc|\.ensure\(|h2d\(", body)            # no device work at all
    args = src[src.index("static mgf_status batch_sensor_args("):src.index('extern "C" mgf_status mgf_batch_cast_sensors(')]
    RC.assert_the_read_and_cast_refusals(args, ["batch_rig_cap(cap)", "query_mask_check(kinds_mask)"])


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def _the_overlap_helper_compares_and_enqueues_nothing(enqueue):
    """dev_outputs_overlap (host_batch_query_dev.inc), which every device-pointer cast calls between its last dev_span and its first
    enqueue: dev_bytes_overlap over the pairs of its list, an error message, nothing else"""
    src = read("mgf_amd", "csrc", "host_batch_query_dev.inc")
    helper = src[src.index("static mgf_status dev_outputs_overlap("):src.index("// Q = ParticleIn")]
    assert "dev_bytes_overlap(a[i].p, a[i].bytes, a[j].p, a[j].bytes)" in helper and '"%s overlaps %s"' in helper
    assert not re.search(enqueue, helper) and "b->" not in helper


def _the_shared_obstacle_pass():
    """batch_ray_obstacles (host_batch_query.inc): the one launch of k_batch_query_ray_obstacles, counted"""
    src = read("mgf_amd", "csrc", "host_batch_query.inc")
    helper = src[src.index("static mgf_status batch_ray_obstacles("):src.index("static mgf_status batch_sweep_tail(")]
    assert helper.count("<<<") == 1 and "k_batch_query_ray_obstacles<<<" in helper and helper.index("LAUNCH_CHECK();") < helper.index("++b->q_launches;")
    for f in ("host_batch_query.inc", "host_batch_query_dev.inc", "host_batch_sensor.inc", "host_batch_camera.inc"):
        text = read("mgf_amd", "csrc", f)
        assert text.count("k_batch_query_ray_obstacles<<<") == (f == "host_batch_query.inc") and "batch_ray_obstacles(" in text, f
    return helper


def test_both_pointers_are_looked_up_before_the_first_enqueue():
    """the order "check, then enqueue" of mgf_batch_cast_sensors_dev, read in the source as tests/test_world_batch_query_device_host.py
    reads batch_query_dev_run: the last dev_span and the overlap check come before the first thing that enqueues - here all of that
    is batch_sensor_run - and the refusals that need no device before the context is bound"""
    src = read("mgf_amd", "csrc", "host_batch_sensor.inc")
    run = src[src.index('extern "C" mgf_status mgf_batch_cast_sensors_dev('):]
    enqueue = (r"batch_sensor_run\(|batch_rig_up\(|batch_rig_upload\(|batch_ray_obstacles\(|batch_sweep_tail\(|batch_push\(|batch_dev_begin\(|batch_env_sync\(|"
               r"batch_cols_refresh\(|hipMemsetAsync|hipMemcpyAsync|<<<|prim_exclusive_scan_u32|\.ensure\(|h2d\(")
    first_enqueue = min(m.start() for m in re.finditer(enqueue, run))
    checks = [m.start() for m in re.finditer(r"dev_span\(", run)]
    assert len(checks) == 2 and max(checks) < first_enqueue
    for name in ("out_dev, 28 \\* n", "parts_out_dev, 28 \\* n"):
        assert re.search(r"dev_span\(b->ctx, " + name, run), name
    # the two outputs, both written, held against each other by the one helper of host_batch_query_dev.inc
    assert run.index('arrays[2] = {{out_dev, 28 * n, "out_dev"}, {parts_out_dev, 28 * n, "parts_out_dev"}};') < run.index("dev_outputs_overlap(arrays, 2, 2)")
    overlap = run.index("dev_outputs_overlap(")
    assert max(checks) < overlap < first_enqueue
    _the_overlap_helper_compares_and_enqueues_nothing(enqueue)
    assert run.index("batch_sensor_args(") < run.index("ctx_bind(") < min(checks)
    assert run.index("if (n == 0) return MGF_OK;") < first_enqueue                   # an empty rig enqueues nothing
    # everything that enqueues is in batch_sensor_run and batch_rig_up, and those are reached from the two cast calls only
    helper = src[src.index("static mgf_status batch_sensor_run("):src.index("static mgf_status batch_sensor_args(")]
    # its own kernel's launch and the shared obstacle pass; neither it nor that pass waits or copies
    assert helper.count("<<<") == 1 and "k_batch_sensor_ray<<<" in helper and helper.index("k_batch_sensor_ray<<<") < helper.index("batch_ray_obstacles(")
    assert "hipStreamSynchronize" not in helper and "hipMemcpy" not in helper
    obstacles = _the_shared_obstacle_pass()
    assert "hipStreamSynchronize" not in obstacles and "hipMemcpy" not in obstacles
    assert helper.index("batch_push(") < helper.index('batch_rig_up(b, R, "sensor", 4)') < helper.index("k_batch_sensor_ray<<<")
    up = RC.up_step()
    assert up.index("if (!R.stale) return MGF_OK;") < up.index("internal error") < up.index("batch_rig_upload(") and "h2d(" not in up
    upload = RC.upload_step()
    assert upload.count("h2d(") == 1 and upload.count(".ensure(") == 1 and "<<<" not in upload          # the steady state uploads nothing; ONE copy
    # no exit ahead of a barrier, no atomic: the front the kernel shares with k_batch_query_ray (k_batch_query.h) holds every exit and
    # every barrier, and what the kernel itself brings - the loader and the store behind the hit - holds neither
    q = read("mgf_amd", "csrc", "k_batch_query.h")
    front = q[q.index("void bq_ray_front("):]
    front = front[:front.index("\n}\n")]
    assert front.count("return;") == 2 and "atomic" not in front
    assert (front.index("blockIdx.x >= *S.n_items) return;") < front.index("bodies.stage(") < front.index("load(qi, W.g0);") < front.index("bodies.ray_walk(")
            < front.index("bq_reduce(") < front.index("if (W.sub != 0u || !W.live) return;") < front.index("q_ray_store(") < front.index("done("))
    assert "__syncthreads" not in front                                   # (the barriers are the staging's - bq_stage's - and bq_reduce's)
    plain = q[q.index("struct PlainBodies {"):q.index("void bq_ray_front(")]
    assert "bq_stage(A, g0, n, s_dyn, s_dyn + n);" in plain
    walk = plain[plain.index("QueryBest ray_walk("):plain.index("SweepBest sweep_walk(")]
    assert walk.index("bq_ray_far(") < walk.index("q_ray_comp(") < walk.index("best.offer(") and not re.search(r"return;|__syncthreads|atomic", walk)
    # (the loader and the store are bs_rays, written once for this kernel and its part-aware form; the kernel is the one call of it)
    k = read("mgf_amd", "csrc", "k_batch_sensor.h")
    body = k[k.index("void bs_rays("):]
    assert "bq_ray_front<kItemTable>(" in body and not re.search(r"return;|__syncthreads|atomic|bq_stage|bq_reduce", body)
    assert body.count("bs_rays(A, PlainBodies(A), s_dyn);") == 1 and body.index("bq_ray_front<kItemTable>(") < body.index("void k_batch_sensor_ray(")


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_binding_turns_a_wrong_tensor_down_before_it_calls_c():
    import torch

    class Handle(mgf_amd.WorldBatch):   # no context, no C handle: a call that got as far as C would fail differently
        def __init__(self):
            self._h, self.n_worlds = None, 2

        def sensor_count(self):
            return 4

    b, n = Handle(), 4
    wrong_out = [torch.zeros((n, 7), dtype=torch.float32), torch.zeros((n, 7), dtype=torch.int64), torch.zeros((7, n), dtype=torch.int32).t(),
                 torch.zeros((n - 1, 7), dtype=torch.int32), torch.zeros((n, 6), dtype=torch.int32)]
    wrong_parts = [torch.zeros((n, 7), dtype=torch.float64), torch.zeros((n, 7), dtype=torch.int32), torch.zeros((7, n), dtype=torch.float32).t(),
                   torch.zeros((n - 1, 7), dtype=torch.float32), torch.zeros((n, 6), dtype=torch.float32)]
    for t in wrong_out:
        with pytest.raises(ValueError) as e:
            b.cast_sensors_dev(t, parts=1 << 21)
        assert "on cpu" not in str(e.value), str(e.value)              # turned down for what it is, not for where it is
    for t in wrong_parts:
        with pytest.raises(ValueError) as e:
            b.cast_sensors_dev(1 << 20, parts=t)
        assert "on cpu" not in str(e.value), str(e.value)
    with pytest.raises(ValueError, match="on cpu"):                     # everything right but the device
        b.cast_sensors_dev(torch.zeros((n, 7), dtype=torch.int32))
    with pytest.raises(ValueError, match="on cpu"):
        b.cast_sensors_dev(1 << 20, parts=torch.zeros((n, 7), dtype=torch.float32))
    with pytest.raises(ValueError, match="required"):
        b.cast_sensors_dev(None)
    with pytest.raises(ValueError, match="not ndarray"):
        b.cast_sensors_dev(np.zeros((n, 7), np.int32))
    with pytest.raises(mgf_amd.MgfError):                               # and a call whose arguments are all in order does reach C
        b.cast_sensors_dev(1 << 20, parts=1 << 21)
    # set_sensors broadcasts scalars and single rows; what reaches C is SENSOR_DTYPE rows (no handle: C refuses, after the marshalling)
    with pytest.raises(mgf_amd.MgfError):
        b.set_sensors([0, 1, 1], 0, (0, 0, 0), [(0, 0, 1), (0, 1, 0), (1, 0, 0)])
    with pytest.raises(ValueError):
        b.set_sensors([0, 1, 1], [0, 1], (0, 0, 0), (0, 0, 1))         # neither one nor n


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_new_kernel_uses_no_scratch_and_the_query_kernels_keep_their_figures():
    if not os.path.exists(os.path.join(ROOT, "mgf_amd", "libmgf_hip.so")) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    rows = kernel_resources("k_batch_sensor_")
    assert set(rows) == {"k_batch_sensor_ray"}, sorted(rows)
    v = rows["k_batch_sensor_ray"]
    assert (v[2], v[3], v[4], v[5]) == ("0", "0", "0", "0"), v               # no scratch, no static LDS, no spills
    # (RESOURCES is held to the build in tests/test_world_batch_rigs_host.py)
    assert int(v[0]) <= int(RESOURCES["k_batch_query_ray"][0]) + 8, (v, RESOURCES["k_batch_query_ray"])   # one piece of work, about the same registers
    design = re.sub(r"\s+", " ", read("DESIGN.md"))
    for text in ("`k_batch_query_ray` 45 / 66 / 0 / 0 / 0", "`k_batch_query_sweep_faces` 133 / 69 / 9216 / 0 / 0", "`_ray_obstacles` 68 / 64 / 0 / 0 / 0",
                 "`k_batch_query_sweep_bodies` 108 / 90 / 0 / 0 / 0", "`k_batch_query_plan_fill` 10 / 20", "`_sweep_obstacles` 115 / 87 / 0 / 0 / 0"):
        assert text in design, text
    k = read("mgf_amd", "csrc", "k_batch_sensor.h")
    assert len(re.findall(r"__global__ __launch_bounds__\(kBatchBlock\)", k)) == len(re.findall(r"__global__", k)) == 1


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_layouts_hold_what_the_gpu_tests_ask_of_them():
    """from the scenes alone: 257 sensors on the world of 300, none on one world, one on the world of one body, four on one body, the
    d = 0 and the too-short sensor, the pair at one sphere's centre, and sensors for the floor, the ring and the sky"""
    twin = SC.twin_scenes()
    assert [len(sc["comps"]) for sc in twin] == [5, 1, 300] and all({0, 1} <= set(sc["comps"]["tag"].tolist()) for sc in twin[::2])
    for scs, lay in ((twin, SC.twin_layout(twin)), (QD.pile_scenes(), SC.pile_layout(QD.pile_scenes()))):
        n = [len(sc["comps"]) for sc in scs]
        assert np.all(lay["body"] >= 0) and np.all(lay["body"] < np.int64(n)[lay["world"]])
        role = lay["role"]
        for r, least in ((SC.DOWN, 10), (SC.UP, 10), (SC.RING, 12), (SC.ZERO, 1), (SC.SHORT, 1), (SC.SELF_IGNORED, 1), (SC.SELF_SEEN, 1), (SC.RANDOM, 100)):
            assert np.sum(role == r) >= least, r
        pair = np.flatnonzero((role == SC.SELF_IGNORED) | (role == SC.SELF_SEEN))
        assert len(pair) == 2 and lay["body"][pair[0]] == lay["body"][pair[1]] and lay["world"][pair[0]] == lay["world"][pair[1]]
        assert scs[lay["world"][pair[0]]]["comps"]["tag"][lay["body"][pair[0]]] == 0
        key = lay["world"].astype(np.int64) * 4096 + lay["body"]
        assert np.bincount(np.unique(key, return_inverse=True)[1]).max() >= 4          # four on one body
        for i in np.flatnonzero(role == SC.RING):
            assert scs[lay["world"][i]].get("obstacles"), i
