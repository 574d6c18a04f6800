"""The body-mounted depth cameras of a batch (mgf_batch_set_cameras, mgf_batch_camera_count, mgf_batch_camera_pixels,
mgf_batch_cast_cameras, mgf_batch_cast_cameras_dev) without a GPU: the numpy restatement of the pixel rays the GPU tests hold the kernel
to equals values worked out in float64 wherever every single operation is exact; the header, the library, the binding and the documents
carry the calls; what can be refused before a device is looked at is refused there; mgf_batch_cast_cameras_dev looks all three pointers
up and checks their overlap before it enqueues anything; the binding turns a wrong tensor down before it calls C; the tile table of a
rig partitions every camera's pixels exactly once; the new kernels use no scratch, spill nothing and hold no static LDS, and the sensor
kernel keeps the figures DESIGN.md records (the query kernels': tests/test_world_batch_rigs_host.py); and the scenes of the GPU tests hold what those tests claim of them, by the
oracle's ray tests."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mgf_amd
from mgf_amd import _capi
from tests import batch_camera_cases as CC
from tests import batch_rig_cases as RC
from tests import batch_sensor_cases as SC
from tests.util import ROOT, kernel_resources, read

CALLS = ("mgf_batch_set_cameras", "mgf_batch_camera_count", "mgf_batch_camera_pixels", "mgf_batch_cast_cameras", "mgf_batch_cast_cameras_dev")


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,height,tan_x,tan_y", [(1, 1, 1.0, 1.0), (4, 2, 1.0, 0.5), (8, 16, 2.0, 0.25), (64, 64, 1.0, 1.0), (3, 5, 4.0, 0.0),
                                                     (4096, 1, 0.5, 1.0)])
def test_the_restatement_equals_float64_where_every_operation_is_exact(width, height, tan_x, tan_y):
    """widths and heights that are powers of two and tangents that are: (2 ix + 1) / width is a dyadic fraction of a few bits, so the
    quotient, the difference and the product are exactly representable in f32 and rounding cannot hide a wrong formula; 3 x 5 has
    quotients that round, with tangents - 4 and 0 - whose product adds no rounding of its own: compared with the f64 value rounded
    ONCE per operation"""
    d = CC.pixel_dirs(width, height, tan_x, tan_y).reshape(height, width, 3)
    assert d.dtype == np.float32 and np.all(d[..., 2] == 1.0)
    ix, iy = np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64)
    qx, qy = ((2 * ix + 1) / width).astype(np.float32).astype(np.float64), ((2 * iy + 1) / height).astype(np.float32).astype(np.float64)
    u = ((qx - 1.0).astype(np.float32).astype(np.float64) * tan_x).astype(np.float32)
    v = ((1.0 - qy).astype(np.float32).astype(np.float64) * tan_y).astype(np.float32)
    if width & (width - 1) == 0 and height & (height - 1) == 0:
        assert np.array_equal(u.astype(np.float64), ((2 * ix + 1) / width - 1.0) * tan_x)       # nothing was rounded at all
        assert np.array_equal(v.astype(np.float64), (1.0 - (2 * iy + 1) / height) * tan_y)
    assert d[..., 0].tobytes() == np.broadcast_to(u[None, :], (height, width)).astype(np.float32).tobytes()
    assert d[..., 1].tobytes() == np.broadcast_to(v[:, None], (height, width)).astype(np.float32).tobytes()
    # +x to the right, +y up, row 0 at the top
    if width > 1 and tan_x > 0:
        assert np.all(np.diff(d[0, :, 0]) > 0) and d[0, 0, 0] < 0 < d[0, -1, 0]
    if height > 1 and tan_y > 0:
        assert np.all(np.diff(d[:, 0, 1]) < 0) and d[0, 0, 1] > 0 > d[-1, 0, 1]


def test_hand_checked_corners_of_the_restatement():
    d = CC.pixel_dirs(5, 3, 0.7, 1.9).reshape(3, 5, 3)
    assert d[1, 2].tolist() == [0.0, 0.0, 1.0]                       # the centre pixel of an odd image: u = v = 0 exactly
    d = CC.pixel_dirs(17, 9, 50.0, 50.0).reshape(9, 17, 3)
    assert d[4, 8].tolist() == [0.0, 0.0, 1.0]
    d = CC.pixel_dirs(2, 2, 1.0, 1.0).reshape(2, 2, 3)             # pixel centres at a quarter and three quarters of the image
    assert d.tolist() == [[[-0.5, 0.5, 1.0], [0.5, 0.5, 1.0]], [[-0.5, -0.5, 1.0], [0.5, -0.5, 1.0]]]
    d = CC.pixel_dirs(1, 1, 3.0, 4.0)
    assert d.tolist() == [[0.0, 0.0, 1.0]]
    d = CC.pixel_dirs(4, 1, 2.0, 1.0)
    assert d[:, 0].tolist() == [-1.5, -0.5, 0.5, 1.5]
    # the particles: the identity leaves d_cam as it is; a quarter turn about y takes +z to +x; P is x + rotate(q, p)
    rig = np.zeros(1, _capi.CAMERA_DTYPE)
    rig["r"], rig["p"], rig["tan_x"], rig["tan_y"], rig["far"], rig["width"], rig["height"] = (1, 0, 0, 0), (0, 2, 0), 1.0, 1.0, 7.0, 2, 2
    rig["flags"] = 1
    st = dict(x=np.float32([[1, 1, 1]]), q=np.float32([[1, 0, 0, 0]]))
    W, P, D, T, I = CC.rig_particles(rig, st, [1])
    assert D.tolist() == CC.pixel_dirs(2, 2, 1.0, 1.0).tolist() and np.all(P == np.float32([1, 3, 1])) and np.all(T == 7.0) and I.tolist() == [0] * 4
    rig["r"], rig["width"], rig["height"], rig["flags"] = CC.LOOK_X, 1, 1, 0
    W, P, D, T, I = CC.rig_particles(rig, st, [1])
    assert np.allclose(D, [[1, 0, 0]], atol=1e-6) and I.tolist() == [-1]
    rig["r"] = CC.LOOK_DOWN
    assert np.allclose(CC.rig_particles(rig, st, [1])[2], [[0, -1, 0]], atol=1e-6)
    # the sensor rig of the same rays
    s = CC.sensor_rig(rig)
    assert len(s) == 1 and np.allclose(s["d"], [[0, -1, 0]], atol=1e-6) and s["dt"][0] == 7.0 and s["p"].tolist() == [[0, 2, 0]]


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def test_header_library_binding_and_documents_carry_the_calls():
    h = read("include", "mgf_hip.h")
    for sig in (r"mgf_status mgf_batch_set_cameras\(mgf_batch\* b, const mgf_batch_camera\* cams, int64_t n\);",
                r"int64_t mgf_batch_camera_count\(const mgf_batch\* b\);", r"int64_t mgf_batch_camera_pixels\(const mgf_batch\* b\);",
                r"mgf_status mgf_batch_cast_cameras\(mgf_batch\* b, int32_t kinds_mask, float\* depth, mgf_ray_hit\* hits, mgf_particle\* parts_out, int64_t cap\);",
                r"mgf_status mgf_batch_cast_cameras_dev\(mgf_batch\* b, int32_t kinds_mask, float\* depth_dev, mgf_ray_hit\* hits_dev, mgf_particle\* parts_out_dev,\s+int64_t cap\);"):
        assert re.search(r"MGF_API " + sig, h), sig
    assert h.index("mgf_batch_cast_sensors_dev(") < h.index("typedef struct mgf_batch_camera")      # behind the sensors section
    m = re.search(r"#define MGF_BATCH_CAMERA_LAUNCHES (\d+)", h)
    assert m and int(m.group(1)) == _capi.BATCH_CAMERA_LAUNCHES == 1
    m = re.search(r"#define MGF_CAMERA_MAX_SIDE (\d+)", h)
    assert m and int(m.group(1)) == _capi.CAMERA_MAX_SIDE == 4096
    section = h[h.index("body-mounted depth cameras"):]
    for word in ("u = ((float)(2*ix + 1) / (float)width  - 1.0f) * tan_x", "v = (1.0f - (float)(2*iy + 1) / (float)height) * tan_y", "d_cam = (u, v, 1.0f)",
                 "D = rotate(q, rotate(r, d_cam))", "WITHOUT delta", "AT ONCE", "bit for bit", "depth along the optical axis", "first(c) + iy * width + ix",
                 "MGF_ERR_CAPACITY", "nothing enqueued", "mgf_batch_add_bodies", "a near plane", "colour", "sharing one workgroup", "a tile cull of the terrain walk",
                 "lone mgf_world", "independent of the sensor rig"):
        assert word in section, word
    assert C.sizeof(_capi.BatchCamera) == 64 == _capi.CAMERA_DTYPE.itemsize
    names = ["world", "body", "p", "r", "tan_x", "tan_y", "far", "width", "height", "flags", "reserved"]
    assert [f[0] for f in _capi.BatchCamera._fields_] == list(_capi.CAMERA_DTYPE.names) == names
    assert [_capi.CAMERA_DTYPE.fields[k][1] for k in names] == [0, 4, 8, 20, 36, 40, 44, 48, 52, 56, 60]
    assert [getattr(_capi.BatchCamera, k).offset for k in names] == [0, 4, 8, 20, 36, 40, 44, 48, 52, 56, 60]
    lib = mgf_amd.load_library()
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    want = {"mgf_batch_set_cameras": (i32, [vp, vp, i64]), "mgf_batch_camera_count": (i64, [vp]), "mgf_batch_camera_pixels": (i64, [vp]),
            "mgf_batch_cast_cameras": (i32, [vp, i32, vp, vp, vp, i64]), "mgf_batch_cast_cameras_dev": (i32, [vp, i32, vp, vp, vp, i64])}
    for name in CALLS:
        assert name in _capi.SYMBOLS, name
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == want[name], name
    for method in ("set_cameras", "camera_count", "camera_pixels", "cast_cameras", "cast_cameras_dev"):
        assert callable(getattr(mgf_amd.WorldBatch, method)), method
    flat = re.sub(r"\s+", " ", read("INTEGRATION.md"))
    for sig in ("pub fn mgf_batch_set_cameras(b: *mut mgf_batch, cams: *const mgf_batch_camera, n: i64) -> mgf_status;",
                "pub fn mgf_batch_camera_count(b: *const mgf_batch) -> i64;", "pub fn mgf_batch_camera_pixels(b: *const mgf_batch) -> i64;",
                "pub fn mgf_batch_cast_cameras(b: *mut mgf_batch, kinds_mask: i32, depth: *mut f32, hits: *mut mgf_ray_hit, parts_out: *mut mgf_particle, cap: i64) -> mgf_status;",
                "pub fn mgf_batch_cast_cameras_dev(b: *mut mgf_batch, kinds_mask: i32, depth_dev: *mut f32, hits_dev: *mut mgf_ray_hit, parts_out_dev: *mut mgf_particle, cap: i64) -> mgf_status;",
                "pub struct mgf_batch_camera"):
        assert sig in flat, sig
    kernels = read("mgf_amd", "csrc", "kernels.h")
    assert kernels.index('#include "k_batch_sensor.h"') < kernels.index('#include "k_batch_camera.h"') and "k_batch_camera_tile" in kernels
    hip = read("mgf_amd", "csrc", "mgf_hip.hip")
    assert hip.index('#include "host_batch_sensor.inc"') < hip.index('#include "host_batch_camera.inc"')
    design = read("DESIGN.md")
    sub = design[design.index("Body-mounted depth cameras"):]
    for word in ("k_batch_camera_tile", "k_batch_camera_depth", "D = rotate(q, rotate(r, d_cam))", "conservative", "Out of scope", "batch_camera_bench.py",
                 "Compiler output"):
        assert word in sub, word
    readme = read("README.md")
    assert "set_cameras" in readme and "cast_cameras_dev" in readme
    assert os.path.exists(os.path.join(ROOT, "tools", "batch_camera_bench.py"))


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_what_needs_no_device_is_refused_before_the_handle_is_dereferenced():
    lib = mgf_amd.load_library()
    INV = _capi.ERR_INVALID

    def err():
        return lib.mgf_last_error().decode()
    fake = C.c_void_p(16)   # a handle that is never dereferenced; addresses that are never looked up
    rig = np.zeros(4, _capi.CAMERA_DTYPE)
    depth, out, parts = C.c_void_p(1 << 20), C.c_void_p(1 << 21), C.c_void_p(1 << 22)
    assert lib.mgf_batch_camera_count(None) == -1 and lib.mgf_batch_camera_pixels(None) == -1
    assert lib.mgf_batch_set_cameras(None, rig.ctypes.data, 4) == INV and "NULL" in err()
    assert lib.mgf_batch_set_cameras(None, None, 0) == INV and "NULL" in err()
    assert lib.mgf_batch_set_cameras(fake, None, 4) == INV and "NULL" in err()
    assert lib.mgf_batch_set_cameras(fake, rig.ctypes.data, -1) == INV and "negative" in err()
    assert lib.mgf_batch_set_cameras(fake, rig.ctypes.data, 1 << 31) == INV and "too many" in err()
    for fn in (lib.mgf_batch_cast_cameras, lib.mgf_batch_cast_cameras_dev):
        assert fn(None, 7, depth, out, parts, 4) == INV and "NULL" in err()
        assert fn(fake, 7, depth, out, None, -1) == INV and "negative" in err()
        for mask in (0, 8, -1, 16):
            assert fn(fake, mask, depth, out, parts, 4) == INV and "kinds_mask" in err(), mask
            assert fn(fake, mask, None, None, None, 0) == INV and "kinds_mask" in err(), mask
    # what needs the handle is refused on the host too, ahead of any change of the rig and of any device work (read here; run in
    # tests/test_gpu_world_batch_cameras.py, where a handle exists)
    src = read("mgf_amd", "csrc", "host_batch_camera.inc")
    body = src[src.index('extern "C" mgf_status mgf_batch_set_cameras('):src.index('extern "C" int64_t mgf_batch_camera_count(')]
    first_change = body.index("b->cameras.recs.assign(")
    assert not re.search(r"b->cameras\.|b->c_pixels", body[:first_change])       # (the tiles are its own work items: no shared plan step)
    for refusal in ("batch_rig_set_args(b, cams, n_in)", "batch_rig_ref_check(b, c.world, c.body, c.flags, \"camera\")", "reserved word is not 0",
                    "outside [1, 4096]", "is not finite", "far is NaN or not above 0", "more than INT32_MAX pixels"):
        assert body.index(refusal) < first_change, refusal
    # the world, the body and the flags: the rigs' one check (host_batch_rig.inc), which names the rig it is asked about
    check = RC.ref_check_step()
    for refusal in ("world index out of range: the rig was not changed", "body index out of range: the rig was not changed",
                    "a %s's flags hold a bit beyond MGF_SENSOR_IGNORE_SELF: the rig was not changed"):
        assert refusal in check, refusal
    assert not re.search(r"<<<|Async|hipMalloc|\.ensure\(|h2d\(|b->\w+ =[^=]", check)    # it refuses; it changes nothing
    assert not re.search(r"<<<|Async|hipMalloc|\.ensure\(|h2d\(", body)            # no device work at all
    # the sensor rig and the zone rig are not touched from here, nor this one from the sensors' file
    assert not re.search(r"b->s_\w+", src) and "b->cameras" in src and "b->sensors" not in src and "b->zones" not in src
    assert "b->cameras" not in read("mgf_amd", "csrc", "host_batch_sensor.inc")
    args = src[src.index("static mgf_status batch_camera_args("):src.index('extern "C" mgf_status mgf_batch_cast_cameras(')]
    RC.assert_the_read_and_cast_refusals(args, ["batch_rig_cap(cap)", "query_mask_check(kinds_mask)"], "depth and hits are both NULL")
    host = read("mgf_amd", "csrc", "host_batch.inc")
    add = host[host.index('extern "C" mgf_status mgf_batch_add_bodies('):]
    assert "batch_rigs_stale(b);" in add[:add.index("\n}\n")] and "b->cameras.stale = true;" in RC.stale_step()


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def test_all_pointers_are_looked_up_and_compared_before_the_first_enqueue():
    src = read("mgf_amd", "csrc", "host_batch_camera.inc")
    run = src[src.index('extern "C" mgf_status mgf_batch_cast_cameras_dev('):]
    enqueue = (r"batch_camera_run\(|batch_rig_up\(|batch_rig_upload\(|batch_ray_obstacles\(|batch_sweep_tail\(|batch_push\(|batch_dev_begin\(|batch_env_sync\(|"
               r"batch_cols_refresh\(|hipMemsetAsync|hipMemcpyAsync|<<<|prim_exclusive_scan_u32|\.ensure\(|h2d\(")
    first_enqueue = min(m.start() for m in re.finditer(enqueue, run))
    checks = [m.start() for m in re.finditer(r"dev_span\(", run)]
    assert len(checks) == 3 and max(checks) < first_enqueue
    for name in ("depth_dev, 4 \\* n", "hits_dev, 28 \\* n", "parts_out_dev, 28 \\* n"):
        assert re.search(r"dev_span\(b->ctx, " + name, run), name
    # all three are written, so the one helper holds every pair against each other, in list order: depth with hits, depth with
    # particles, hits with particles
    listed = run.index('arrays[3] = {{depth_dev, 4 * n, "depth_dev"}, {hits_dev, 28 * n, "hits_dev"}, {parts_out_dev, 28 * n, "parts_out_dev"}};')
    assert max(checks) < listed < run.index("dev_outputs_overlap(arrays, 3, 3)") < first_enqueue
    from tests.test_world_batch_sensors_host import _the_overlap_helper_compares_and_enqueues_nothing, _the_shared_obstacle_pass
    _the_overlap_helper_compares_and_enqueues_nothing(enqueue)
    dev = read("mgf_amd", "csrc", "host_batch_query_dev.inc")
    loops = dev[dev.index("static mgf_status dev_outputs_overlap("):dev.index("// Q = ParticleIn")]
    assert "for (size_t i = 0; i < n_out; ++i)" in loops and "for (size_t j = i + 1; j < n; ++j)" in loops
    assert run.index("batch_camera_args(") < run.index("ctx_bind(") < min(checks)
    assert run.index("if (n == 0) return MGF_OK;") < first_enqueue                   # an empty rig enqueues nothing
    helper = src[src.index("static mgf_status batch_camera_run("):src.index("static mgf_status batch_camera_args(")]
    # its own two kernels' launches with the shared obstacle pass between them; neither it nor that pass waits or copies
    assert helper.index("k_batch_camera_tile<<<") < helper.index("batch_ray_obstacles(") < helper.index("k_batch_camera_depth<<<") and helper.count("<<<") == 2
    assert "hipStreamSynchronize" not in helper and "hipMemcpy" not in helper
    obstacles = _the_shared_obstacle_pass()
    assert "hipStreamSynchronize" not in obstacles and "hipMemcpy" not in obstacles
    assert helper.index("batch_push(") < helper.index('batch_rig_up(b, R, "camera", 2)') < helper.index("k_batch_camera_tile<<<")
    assert "k_batch_camera_tile<<<(unsigned)R.items.size(), kBatchBlock, batch_camera_lds(b), s>>>(A);" in helper
    up = RC.up_step()
    assert up.index("if (!R.stale) return MGF_OK;") < up.index("internal error") < up.index("batch_rig_upload(") and up.count("batch_rig_upload(") == 1
    assert "h2d(" not in up
    upload = RC.upload_step()
    assert upload.count("h2d(") == 1 and upload.count(".ensure(") == 1 and "<<<" not in upload          # the steady state uploads nothing; one copy
    k = read("mgf_amd", "csrc", "k_batch_camera.h")
    body = k[k.index("void k_batch_camera_tile("):k.index("void k_batch_camera_depth(")]
    assert "return" not in body[:body.rindex("}\n\n")] and body.count("__syncthreads()") == 3         # no exit ahead of a barrier: no exit at all
    assert "atomicAdd(&s_ctl[0]" in body and not re.search(r"atomic\w*\([^)]*float", body) and "__shared__ float4 s_dyn[]" in body
    assert len(re.findall(r"__shared__", k)) == 1                                                     # dynamic LDS only


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_binding_turns_a_wrong_tensor_down_before_it_calls_c():
    import torch

    class Handle(mgf_amd.WorldBatch):   # no context, no C handle: a call that got as far as C would fail differently
        def __init__(self):
            self._h, self.n_worlds = None, 2

        def camera_pixels(self):
            return 4

    b, n = Handle(), 4
    wrong_depth = [torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.int32), torch.zeros((n, 2), dtype=torch.float32)[:, 0],
                   torch.zeros(n - 1, dtype=torch.float32), torch.zeros((n, 2), dtype=torch.float32)]
    wrong_hits = [torch.zeros((n, 7), dtype=torch.float32), torch.zeros((n, 7), dtype=torch.int64), torch.zeros((7, n), dtype=torch.int32).t(),
                  torch.zeros((n - 1, 7), dtype=torch.int32), torch.zeros((n, 6), dtype=torch.int32)]
    wrong_parts = [torch.zeros((n, 7), dtype=torch.float64), torch.zeros((n, 7), dtype=torch.int32), torch.zeros((7, n), dtype=torch.float32).t(),
                   torch.zeros((n - 1, 7), dtype=torch.float32), torch.zeros((n, 6), dtype=torch.float32)]
    for t in wrong_depth:
        with pytest.raises(ValueError) as e:
            b.cast_cameras_dev(depth=t, hits=1 << 21)
        assert "on cpu" not in str(e.value), str(e.value)              # turned down for what it is, not for where it is
    for t in wrong_hits:
        with pytest.raises(ValueError) as e:
            b.cast_cameras_dev(depth=1 << 20, hits=t)
        assert "on cpu" not in str(e.value), str(e.value)
    for t in wrong_parts:
        with pytest.raises(ValueError) as e:
            b.cast_cameras_dev(depth=1 << 20, parts=t)
        assert "on cpu" not in str(e.value), str(e.value)
    with pytest.raises(ValueError, match="on cpu"):                     # everything right but the device
        b.cast_cameras_dev(depth=torch.zeros(n, dtype=torch.float32))
    with pytest.raises(ValueError, match="on cpu"):
        b.cast_cameras_dev(hits=torch.zeros((n, 7), dtype=torch.int32))
    with pytest.raises(ValueError, match="on cpu"):
        b.cast_cameras_dev(depth=1 << 20, parts=torch.zeros((n, 7), dtype=torch.float32))
    with pytest.raises(ValueError, match="required"):
        b.cast_cameras_dev()
    with pytest.raises(ValueError, match="required"):
        b.cast_cameras_dev(parts=1 << 22)
    with pytest.raises(ValueError, match="not ndarray"):
        b.cast_cameras_dev(depth=np.zeros(n, np.float32))
    with pytest.raises(mgf_amd.MgfError):                               # and a call whose arguments are all in order does reach C
        b.cast_cameras_dev(depth=1 << 20, hits=1 << 21, parts=1 << 22)
    with pytest.raises(mgf_amd.MgfError):                               # set_cameras marshals dicts into CAMERA_DTYPE rows (no handle: C refuses)
        b.set_cameras([dict(world=0, body=0, p=(0, 0, 0), tan_x=1.0, tan_y=1.0, width=4, height=4)])
    with pytest.raises(ValueError, match="no such field"):
        b.set_cameras([dict(world=0, body=0, fov=1.0)])
    with pytest.raises(ValueError, match="CAMERA_DTYPE"):
        b.set_cameras(np.zeros(2, _capi.SENSOR_DTYPE))


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_tile_shape_of_the_model_is_the_kernels():
    k = read("mgf_amd", "csrc", "k_batch_camera.h")
    m = re.search(r"constexpr uint32_t kCamTileW = (\d+), kCamTileH = (\d+);", k)
    assert m and (int(m.group(1)), int(m.group(2))) == (CC.TILE_W, CC.TILE_H) and CC.TILE_W * CC.TILE_H == 256
    assert "x0 + (threadIdx.x % kCamTileW)" in k and "y0 + (threadIdx.x / kCamTileW)" in k
    assert "(size_t)it.y + (size_t)iy * (uint32_t)c.width + ix" in k
    src = read("mgf_amd", "csrc", "host_batch_camera.inc")
    assert re.search(r"for \(uint32_t y0 = 0; y0 < \(uint32_t\)cams\[i\]\.height; y0 \+= kCamTileH\)\s+for \(uint32_t x0 = 0; x0 < \(uint32_t\)cams\[i\]\.width; x0 \+= kCamTileW\) "
                     r"tiles\.push_back\(make_uint4\(\(uint32_t\)i, first, x0 \| \(y0 << 16\), 0u\)\);", src)


@pytest.mark.parametrize("shapes", [[(1, 1)], [(17, 9)], [(16, 16)], [(40, 33)], [(4096, 1)], [(1, 1), (17, 9), (16, 16), (40, 33), (4096, 1), (64, 64)]])
def test_the_tile_table_partitions_every_cameras_pixels_exactly_once(shapes):
    widths, heights = [s[0] for s in shapes], [s[1] for s in shapes]
    table = CC.tile_table(widths, heights)
    total = sum(w * h for w, h in shapes)
    seen = np.zeros(total, np.int64)
    first = np.concatenate([[0], np.cumsum([w * h for w, h in shapes])])
    for row in table:
        c = int(row[0])
        assert row[1] == first[c] and row[2] % CC.TILE_W == 0 and row[3] % CC.TILE_H == 0 and row[2] < 65536 and row[3] < 65536
        pix = CC.tile_pixels(row, widths[c], heights[c])
        assert 1 <= len(pix) <= 256 and pix.min() >= first[c] and pix.max() < first[c + 1]      # a tile stays inside its camera; none is empty
        seen[pix] += 1
    assert np.all(seen == 1)
    assert len(table) == sum(-(-w // CC.TILE_W) * -(-h // CC.TILE_H) for w, h in shapes)
    assert np.all(np.diff(table[:, 0]) >= 0)
    if shapes == [(40, 33)]:
        assert len(table) == 9 and len(CC.tile_pixels(table[-1], 40, 33)) == 8 * 1           # partial in both directions
    if shapes == [(4096, 1)]:
        assert len(table) == 256 and all(len(CC.tile_pixels(r, 4096, 1)) == 16 for r in table)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_new_kernels_use_no_scratch_and_the_sensor_and_query_kernels_keep_their_figures():
    if not os.path.exists(os.path.join(ROOT, "mgf_amd", "libmgf_hip.so")) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    rows = kernel_resources("k_batch_camera_")
    assert set(rows) == {"k_batch_camera_tile", "k_batch_camera_depth"}, sorted(rows)
    for name, v in rows.items():
        assert (v[2], v[3], v[4], v[5]) == ("0", "0", "0", "0"), (name, v)         # no scratch, no static LDS, no spills
    assert int(rows["k_batch_camera_tile"][0]) <= 64, rows                         # eight waves a SIMD stay possible
    sensor = kernel_resources("k_batch_sensor_")
    assert sensor == {"k_batch_sensor_ray": ("45", "68", "0", "0", "0", "0")}, sensor
    design = re.sub(r"\s+", " ", read("DESIGN.md"))
    t, d = rows["k_batch_camera_tile"], rows["k_batch_camera_depth"]
    for text in (f"`k_batch_camera_tile` {t[0]} / {t[1]} / 0 / 0 / 0", f"`k_batch_camera_depth` {d[0]} / {d[1]} / 0 / 0 / 0"):
        assert text in design, text
    k = read("mgf_amd", "csrc", "k_batch_camera.h")
    assert len(re.findall(r"__global__ __launch_bounds__\(kBatchBlock\)", k)) == len(re.findall(r"__global__", k)) == 2


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_hits():
    scs, long_body = CC.camera_scenes()
    rig = CC.camera_rig(scs)
    kind, index, t = CC.oracle_hits(scs, rig)
    return scs, long_body, rig, kind, index, t


SEES = CC.SEES


def test_the_scenes_hold_what_the_gpu_tests_claim_camera_by_camera(scene_hits):
    scs, long_body, rig, kind, index, t = scene_hits
    assert [len(sc["comps"]) for sc in scs] == [5, 1, 300] and not np.any(rig["world"] == CC.BARE_WORLD)
    assert sorted(zip(rig["width"].tolist(), rig["height"].tolist())) == sorted([(64, 64), (40, 33), (17, 9), (17, 9), (1, 1), (1, 1), (17, 9)])
    assert np.all(scs[CC.CAMERA_WORLD]["comps"]["tag"][rig["body"][rig["world"] == CC.CAMERA_WORLD]] == 0)     # every camera sits on a sphere
    fs = CC.firsts(rig)
    per = {}
    for c, name in enumerate(CC.NAMES):
        n = int(rig["width"][c]) * int(rig["height"][c])
        per[name] = (kind[fs[c]:fs[c] + n], index[fs[c]:fs[c] + n], t[fs[c]:fs[c] + n])
        assert set(per[name][0].tolist()) == SEES[name], (name, sorted(set(per[name][0].tolist())))
    # pixels that hit a body, the terrain, an obstacle and nothing - at least eight of each
    assert all(int(np.sum(kind == k)) >= 8 for k in (-1, 0, 1, 2)), {k: int(np.sum(kind == k)) for k in (-1, 0, 1, 2)}
    # the long capsule crosses many tiles of the camera above it
    k0, i0, _ = per["above"]
    on_long = np.flatnonzero((k0 == 0) & (i0 == long_body))
    tiles_hit = {(int(p % 64) // CC.TILE_W, int(p // 64) // CC.TILE_H) for p in on_long}
    assert len(tiles_hit) >= 6, sorted(tiles_hit)
    # a tile in which some body is outside the tile's cone while another tile of the same image hits that body
    cen, rad = CC.bounds(scs[CC.CAMERA_WORLD])
    cam = rig[0]
    eye = scs[CC.CAMERA_WORLD]["comps"]["p"][cam["body"]].astype(np.float64) + cam["p"].astype(np.float64)
    found = 0
    for j in np.unique(i0[k0 == 0]):
        hit_tiles = {(int(p % 64) // CC.TILE_W, int(p // 64) // CC.TILE_H) for p in np.flatnonzero((k0 == 0) & (i0 == j))}
        for ty in range(4):
            for tx in range(4):
                ax, cs = CC.tile_cone(cam, tx * CC.TILE_W, ty * CC.TILE_H)
                if (tx, ty) not in hit_tiles and CC.sphere_outside_cone(eye, ax, cs, cen[j], 1.5 * rad[j] + 0.1):
                    found += 1
    assert found >= 100, found                              # (most bodies are outside most tiles: what the cull is for)
    # a body whose sphere contains the eye: the camera at the centre of its own sphere, ignored and not
    for name in ("inside_row", "lone_seen", "lone_ignored"):
        c = CC.NAMES.index(name)
        assert np.all(rig["p"][c] == 0) and scs[rig["world"][c]]["comps"]["r"][rig["body"][c]] == 0.5
    ks, js, ts = per["lone_seen"]
    assert ks[0] == 0 and js[0] == 0 and ts[0] == 0.0
    ki, ji, _ = per["inside_row"]
    assert not np.any((ki == 0) & (ji == rig["body"][1])) and np.any(ki == 0)
    # a body beyond far on the optical axis of inside_row, which looks along +x for 4 * |D|: bodies of its row stand beyond that
    c = rig[1]
    eye = scs[CC.CAMERA_WORLD]["comps"]["p"][c["body"]].astype(np.float64)
    axis = CC._rot64(c["r"], (0.0, 0.0, 1.0))
    reach = float(c["far"]) * np.linalg.norm(axis)
    w = cen - eye
    along = w @ axis / np.linalg.norm(axis)
    off = np.linalg.norm(w - np.outer(along, axis / np.linalg.norm(axis)), axis=1)
    beyond = (off < rad) & (along - rad > reach)
    assert np.sum(beyond) >= 2, int(np.sum(beyond))
    assert not np.any(np.isin(ji[ki == 0], np.flatnonzero(beyond)))                   # and none of them is seen
    assert np.all(per["inside_row"][2][ki >= 0] <= 4.0)
    # the fan: tan_x = 0, every pixel of a row has the same direction; the r that is not of unit length
    assert rig["tan_x"][3] == 0.0 and abs(np.linalg.norm(rig["r"][1]) - 1.3) < 1e-6 and abs(np.linalg.norm(rig["r"][3]) - 1.0) > 0.01
    assert rig["body"][0] == rig["body"][6] and rig["body"][2] == rig["body"][3]       # two cameras on one body
    assert np.isinf(rig["far"][0]) and np.isfinite(rig["far"][1]) and rig["tan_x"][2] == 50.0
