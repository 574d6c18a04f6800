"""The sweep query's C-ABI without a GPU: the header declares mgf_world_sweep_many and mgf_sweep_hit (with the layout the Python
binding reads), the library exports it, INTEGRATION.md carries its Rust twin, and the entry point refuses bad arguments before it
needs a device."""
import ctypes as C
import os
import re

import numpy as np

import mgf_amd
from mgf_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_header_declares_the_sweep_and_its_hit_record():
    h = _read("include", "mgf_hip.h")
    assert re.search(r"MGF_API mgf_status mgf_world_sweep_many\(mgf_world\* w, const mgf_moving_component\* casts, int64_t n,\s*"
                     r"const int32_t\* ignore_body,\s*int32_t kinds_mask, mgf_sweep_hit\* out\);", h)
    assert re.search(r"typedef struct mgf_sweep_hit \{ int32_t kind; int32_t index; int32_t part; mgf_contact contact; \} mgf_sweep_hit;", h)
    # the definition cites the reference's tests it rests on
    for cite in ("collision.rs:1089-1356", "collision.rs:610-1000", "compound.rs:334-351", "collision.rs:1097-1100"):
        assert cite in h, cite


def test_sweep_hit_layout():
    dt = _capi.SWEEP_HIT_DTYPE
    assert dt.itemsize == 52
    assert [dt.fields[k][1] for k in ("kind", "index", "part", "a", "b", "n", "t")] == [0, 4, 8, 12, 24, 36, 48]
    assert mgf_amd.SWEEP_HIT_DTYPE is dt


def test_library_exports_the_sweep():
    lib = mgf_amd.load_library()
    assert hasattr(lib, "mgf_world_sweep_many")
    assert "mgf_world_sweep_many" in _capi.SYMBOLS


def _casts(tags):
    c = np.zeros(len(tags), _capi.MOVING_DTYPE)
    c["tag"] = tags
    c["r"] = 0.5
    c["delta"] = (1.0, 0.0, 0.0)
    return c


def test_bad_arguments_are_refused_without_a_device():
    lib = mgf_amd.load_library()
    casts = _casts([0, 1])
    out = np.zeros(2, _capi.SWEEP_HIT_DTYPE)

    def err():
        return lib.mgf_last_error().decode()
    # no world
    assert lib.mgf_world_sweep_many(None, casts.ctypes.data, 2, None, 7, out.ctypes.data) == _capi.ERR_INVALID
    assert "NULL" in err()
    # a world handle that is never dereferenced: every check below comes before the device is touched
    fake = C.c_void_p(16)
    assert lib.mgf_world_sweep_many(fake, None, 2, None, 7, out.ctypes.data) == _capi.ERR_INVALID
    assert lib.mgf_world_sweep_many(fake, casts.ctypes.data, 2, None, 7, None) == _capi.ERR_INVALID
    assert lib.mgf_world_sweep_many(fake, casts.ctypes.data, -1, None, 7, out.ctypes.data) == _capi.ERR_INVALID
    assert "NULL" in err() or "negative" in err()
    for mask in (0, 8, -1, 15, 16):
        assert lib.mgf_world_sweep_many(fake, casts.ctypes.data, 2, None, mask, out.ctypes.data) == _capi.ERR_INVALID
        assert "kinds_mask" in err()
    for tag in (2, 3, -1, 7):
        bad = _casts([0, tag])
        assert lib.mgf_world_sweep_many(fake, bad.ctypes.data, 2, None, 7, out.ctypes.data) == _capi.ERR_INVALID
        assert "tag" in err()


def test_integration_md_sketches_the_sweep():
    text = _read("INTEGRATION.md")
    assert "pub fn mgf_world_sweep_many(w: *mut mgf_world, casts: *const mgf_moving_component, n: i64, ignore_body: *const i32," in text
    assert "pub struct mgf_sweep_hit { pub kind: i32, pub index: i32, pub part: i32, pub contact: mgf_contact }" in text
    assert "mgf_world_sweep_many(w, &cast, 1, &me" in text  # the safe wrapper's call
