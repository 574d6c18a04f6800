"""The batch of small worlds' C-ABI without a GPU: the header declares the section and its entry points, the library exports them, the
Python binding and INTEGRATION.md carry them, bad arguments are refused before a device is touched, nothing computes without a device -
and the batch tick's kernels use no scratch memory and spill no register."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mgf_amd
from mgf_amd import _capi
from tests.util import ROOT, kernel_resources, read

ENTRY_POINTS = {
    "mgf_batch_new": r"mgf_status mgf_batch_new\(mgf_ctx\* ctx, const mgf_params\* params, int64_t n_worlds, mgf_batch\*\* out\);",
    "mgf_batch_free": r"void mgf_batch_free\(mgf_batch\* b\);",
    "mgf_batch_set_terrain": r"mgf_status mgf_batch_set_terrain\(mgf_batch\* b, const mgf_mesh\* mesh\);",
    "mgf_batch_add_bodies": r"mgf_status mgf_batch_add_bodies\(mgf_batch\* b, int64_t world, const mgf_component\* comps, int64_t n, const float\* mass,\s*"
                            r"const float\* restitution, const float\* friction, const mgf_vec3\* world_force, uint64_t\* first_id\);",
    "mgf_batch_len": r"int64_t mgf_batch_len\(const mgf_batch\* b, int64_t world\);",
    "mgf_batch_step": r"mgf_status mgf_batch_step\(mgf_batch\* b, float dt, int32_t iters, int64_t n_ticks, mgf_step_stats\* stats\);",
    "mgf_batch_read_state": r"mgf_status mgf_batch_read_state\(mgf_batch\* b, int64_t world, mgf_vec3\* x, mgf_quat\* q, mgf_vec3\* v, mgf_vec3\* omega, "
                            r"mgf_vec3\* delta, int64_t cap\);",
    "mgf_batch_write_state": r"mgf_status mgf_batch_write_state\(mgf_batch\* b, int64_t world, const mgf_vec3\* x, const mgf_quat\* q, const mgf_vec3\* v, "
                             r"const mgf_vec3\* omega,\s*const mgf_vec3\* delta, int64_t n\);",
    "mgf_batch_read_constraints": r"mgf_status mgf_batch_read_constraints\(mgf_batch\* b, int64_t world, mgf_constraint\* out, int64_t cap, int64_t\* count\);",
    "mgf_batch_counter": r"mgf_status mgf_batch_counter\(const mgf_batch\* b, const char\* name, int64_t\* out\);",
    "mgf_batch_set_option": r"mgf_status mgf_batch_set_option\(mgf_batch\* b, const char\* key, int64_t value\);",
}


def test_header_declares_the_section_and_its_entry_points():
    h = read("include", "mgf_hip.h")
    assert "typedef struct mgf_batch mgf_batch;" in h
    assert re.search(r"#define MGF_BATCH_MAX_BODIES 1024\b", h)
    assert "many small worlds" in h
    for name, sig in ENTRY_POINTS.items():
        assert re.search(r"MGF_API " + sig, h), name
    # the definition cites the reference, and the limits are stated
    for cite in ("world.rs:227-294", "world.rs:235-238", "physics.rs:200-218", "solver.rs:72-78"):
        assert cite in h[h.index("many small worlds"):], cite
    assert "LIMITS" in h[h.index("many small worlds"):]


def test_library_and_binding_export_them():
    lib = mgf_amd.load_library()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in _capi.SYMBOLS, name
    assert mgf_amd.WorldBatch is _capi.WorldBatch and mgf_amd.BATCH_MAX_BODIES == 1024
    for method in ("from_scenes", "step", "state", "write_state", "constraints", "counter", "__len__"):
        assert hasattr(mgf_amd.WorldBatch, method), method


def test_integration_md_has_the_rust_twins():
    text = read("INTEGRATION.md")
    assert re.search(r"pub enum mgf_batch \{\}", text)
    assert "pub const MGF_BATCH_MAX_BODIES: usize = 1024;" in text
    for name in ENTRY_POINTS:
        assert re.search(r"pub fn %s\(" % name, text), name
    assert "pub fn mgf_batch_step(b: *mut mgf_batch, dt: f32, iters: i32, n_ticks: i64, stats: *mut mgf_step_stats) -> mgf_status;" in text
    assert "pub struct WorldBatch" in text and "mgf_batch_step(self.raw" in text   # the safe wrapper


def _comps(tags):
    c = np.zeros(len(tags), _capi.COMPONENT_DTYPE)
    c["tag"] = tags
    c["r"] = 0.5
    c["d"] = (0.0, 1.0, 0.0)
    return c


def test_bad_arguments_are_refused_before_a_device_is_touched():
    lib = mgf_amd.load_library()
    INV = _capi.ERR_INVALID

    def err():
        return lib.mgf_last_error().decode()
    ones = np.ones(2048, np.float32)
    force = np.zeros((2048, 3), np.float32)
    out = C.c_void_p()
    first = C.c_uint64()
    cnt = C.c_int64()
    x = np.zeros((4, 3), np.float32)

    def add(h, world, comps, n):
        return lib.mgf_batch_add_bodies(h, world, comps.ctypes.data, n, ones.ctypes.data, ones.ctypes.data, ones.ctypes.data, force.ctypes.data, C.byref(first))
    # a NULL handle
    two = _comps([0, 1])
    assert add(None, 0, two, 2) == INV and "NULL" in err()
    assert lib.mgf_batch_step(None, 1.0 / 60.0, 4, 1, None) == INV and "NULL" in err()
    assert lib.mgf_batch_set_terrain(None, None) == INV and "NULL" in err()
    assert lib.mgf_batch_read_state(None, 0, x.ctypes.data, None, None, None, None, 4) == INV and "NULL" in err()
    assert lib.mgf_batch_write_state(None, 0, x.ctypes.data, None, None, None, None, 4) == INV and "NULL" in err()
    assert lib.mgf_batch_read_constraints(None, 0, None, 0, C.byref(cnt)) == INV and "NULL" in err()
    assert lib.mgf_batch_counter(None, b"capacity_retries", C.byref(cnt)) == INV and "NULL" in err()
    assert lib.mgf_batch_set_option(None, b"cons_per_body", 4) == INV and "NULL" in err()
    assert lib.mgf_batch_len(None, 0) == -1
    lib.mgf_batch_free(None)
    # n_worlds <= 0, whatever the context
    for n_worlds in (0, -1, -(1 << 40)):
        assert lib.mgf_batch_new(None, None, n_worlds, C.byref(out)) == INV and "n_worlds" in err()
        assert not out.value
    assert lib.mgf_batch_new(None, None, 4, None) == INV
    # a handle that is never dereferenced: every check below comes before the batch or a device is looked at
    fake = C.c_void_p(16)
    for world in (-1, -2, -(1 << 40)):
        assert add(fake, world, two, 2) == INV and "world index" in err()
        assert lib.mgf_batch_read_constraints(fake, world, None, 0, C.byref(cnt)) == INV and "world index" in err()
    for world in (-2, -(1 << 40)):   # (-1 is the whole batch there)
        assert lib.mgf_batch_read_state(fake, world, x.ctypes.data, None, None, None, None, 4) == INV and "world index" in err()
        assert lib.mgf_batch_write_state(fake, world, x.ctypes.data, None, None, None, None, 4) == INV and "world index" in err()
    assert add(fake, 0, two, -1) == INV and "negative" in err()
    assert lib.mgf_batch_write_state(fake, 0, x.ctypes.data, None, None, None, None, -4) == INV and "negative" in err()
    assert lib.mgf_batch_step(fake, 1.0 / 60.0, 4, -1, None) == INV and "n_ticks" in err()
    assert lib.mgf_batch_step(fake, 1.0 / 60.0, -1, 1, None) == INV and "iters" in err()
    for tag in (2, 3, -1, 7):
        assert add(fake, 0, _comps([0, tag]), 2) == INV and "tag" in err()
    many = _comps([0] * 1025)
    assert add(fake, 0, many, 1025) == INV and "MGF_BATCH_MAX_BODIES" in err()


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except Exception:
        return True


@pytest.mark.skipif(not _no_gpu(), reason="needs a machine without a GPU")
def test_no_batch_without_a_device():
    lib = mgf_amd.load_library()
    out = C.c_void_p()
    assert lib.mgf_batch_new(None, None, 4, C.byref(out)) == _capi.ERR_HIP   # no context, no batch: there is no CPU fallback
    assert "no CPU fallback" in lib.mgf_last_error().decode() and not out.value
    with pytest.raises(mgf_amd.MgfError) as e:
        mgf_amd.Context(0)
    assert e.value.status == _capi.ERR_HIP


def test_the_batch_kernels_use_no_scratch_and_spill_nothing():
    if not os.path.exists(os.path.join(ROOT, "mgf_amd", "libmgf_hip.so")) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    rows = kernel_resources("k_batch_")
    tick = {"k_batch_front", "k_batch_faces", "k_batch_pairs", "k_batch_pack", "k_batch_setup", "k_batch_solve"}
    assert tick <= set(rows), rows
    bad = {k: v for k, v in rows.items() if (v[2], v[4], v[5]) != ("0", "0", "0")}
    assert not bad, bad
