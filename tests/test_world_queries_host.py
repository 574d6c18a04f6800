"""The world queries' C-ABI without a GPU: the header declares mgf_world_raycast_many, mgf_world_overlap_aabb_many and
mgf_ray_hit (with the layout the Python binding reads), and the entry points refuse bad arguments before they need a device."""
import ctypes as C
import os
import re

import numpy as np

import mgf_amd
from mgf_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "mgf_hip.h")).read()


def test_header_declares_the_queries_and_the_hit_record():
    h = _header()
    assert re.search(r"MGF_API mgf_status mgf_world_raycast_many\(mgf_world\* w, const mgf_particle\* parts, int64_t n,\s*"
                     r"const int32_t\* ignore_body,\s*int32_t kinds_mask, mgf_ray_hit\* out\);", h)
    assert re.search(r"MGF_API mgf_status mgf_world_overlap_aabb_many\(mgf_world\* w, const mgf_aabb\* boxes, int64_t n, "
                     r"uint64_t\* out_offsets[^,]*,\s*uint32_t\* out_bodies, int64_t cap, int64_t\* total\);", h)
    assert re.search(r"typedef struct mgf_ray_hit \{ int32_t kind; int32_t index; int32_t part; mgf_intersection inter; \} mgf_ray_hit;", h)
    consts = dict(re.findall(r"#define\s+(MGF_(?:HIT|QUERY)_\w+)\s+\(?(-?\d+)\)?", h))
    assert consts == {"MGF_HIT_NONE": "-1", "MGF_HIT_BODY": "0", "MGF_HIT_TERRAIN": "1", "MGF_HIT_OBSTACLE": "2",
                      "MGF_QUERY_BODIES": "1", "MGF_QUERY_TERRAIN": "2", "MGF_QUERY_OBSTACLES": "4", "MGF_QUERY_ALL": "7"}
    assert (_capi.HIT_NONE, _capi.HIT_BODY, _capi.HIT_TERRAIN, _capi.HIT_OBSTACLE) == (-1, 0, 1, 2)
    assert (_capi.QUERY_BODIES, _capi.QUERY_TERRAIN, _capi.QUERY_OBSTACLES, _capi.QUERY_ALL) == (1, 2, 4, 7)


def test_ray_hit_layout():
    assert _capi.RAY_HIT_DTYPE.itemsize == 28
    assert [_capi.RAY_HIT_DTYPE.fields[k][1] for k in ("kind", "index", "part", "p", "t")] == [0, 4, 8, 12, 24]


def test_library_exports_the_queries():
    lib = mgf_amd.load_library()
    assert hasattr(lib, "mgf_world_raycast_many") and hasattr(lib, "mgf_world_overlap_aabb_many")
    assert "mgf_world_raycast_many" in _capi.SYMBOLS and "mgf_world_overlap_aabb_many" in _capi.SYMBOLS


def test_bad_arguments_are_refused_without_a_device():
    lib = mgf_amd.load_library()
    parts = np.zeros((1, 7), np.float32)
    out = np.zeros(1, _capi.RAY_HIT_DTYPE)
    # no world
    assert lib.mgf_world_raycast_many(None, parts.ctypes.data, 1, None, 7, out.ctypes.data) == _capi.ERR_INVALID
    assert "NULL" in lib.mgf_last_error().decode()
    boxes = np.zeros((1, 6), np.float32)
    off = np.zeros(2, np.uint64)
    vals = np.zeros(4, np.uint32)
    total = C.c_int64(-1)
    assert lib.mgf_world_overlap_aabb_many(None, boxes.ctypes.data, 1, off.ctypes.data, vals.ctypes.data, 4, C.byref(total)) == _capi.ERR_INVALID
    # a world handle that is never dereferenced: every check below comes before the device is touched
    fake = C.c_void_p(16)
    assert lib.mgf_world_raycast_many(fake, None, 1, None, 7, out.ctypes.data) == _capi.ERR_INVALID
    assert lib.mgf_world_raycast_many(fake, parts.ctypes.data, -1, None, 7, out.ctypes.data) == _capi.ERR_INVALID
    for mask in (0, 8, -1, 15):
        assert lib.mgf_world_raycast_many(fake, parts.ctypes.data, 1, None, mask, out.ctypes.data) == _capi.ERR_INVALID
        assert "kinds_mask" in lib.mgf_last_error().decode()
    assert lib.mgf_world_overlap_aabb_many(fake, boxes.ctypes.data, 1, None, vals.ctypes.data, 4, C.byref(total)) == _capi.ERR_INVALID
    assert lib.mgf_world_overlap_aabb_many(fake, boxes.ctypes.data, 1, off.ctypes.data, None, 4, C.byref(total)) == _capi.ERR_INVALID
    assert lib.mgf_world_overlap_aabb_many(fake, None, 1, off.ctypes.data, vals.ctypes.data, 4, C.byref(total)) == _capi.ERR_INVALID
    assert lib.mgf_world_overlap_aabb_many(fake, boxes.ctypes.data, 1, off.ctypes.data, vals.ctypes.data, -1, C.byref(total)) == _capi.ERR_INVALID


def test_integration_md_sketches_both_queries():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "pub fn mgf_world_raycast_many(" in text and "pub fn mgf_world_overlap_aabb_many(" in text
    assert "pub struct mgf_ray_hit { pub kind: i32, pub index: i32, pub part: i32, pub inter: mgf_intersection }" in text
