"""The batch's queries (mgf_batch_read_colliders, mgf_batch_raycast_many, mgf_batch_sweep_many) without a GPU: the header declares and
defines them, the library, the Python binding and INTEGRATION.md carry them, bad arguments are refused before the handle or a device is
touched - and the query kernels use no scratch memory and spill no register."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mgf_amd
from mgf_amd import _capi
from tests.util import ROOT, kernel_resources, read

ENTRY_POINTS = {
    "mgf_batch_read_colliders": r"mgf_status mgf_batch_read_colliders\(mgf_batch\* b, int64_t world, mgf_moving_component\* out, int64_t cap\);",
    "mgf_batch_raycast_many": r"mgf_status mgf_batch_raycast_many\(mgf_batch\* b, const int32_t\* world, const mgf_particle\* parts, int64_t n,\s*"
                              r"const int32_t\* ignore_body, int32_t kinds_mask, mgf_ray_hit\* out\);",
    "mgf_batch_sweep_many": r"mgf_status mgf_batch_sweep_many\(mgf_batch\* b, const int32_t\* world, const mgf_moving_component\* casts, int64_t n,\s*"
                            r"const int32_t\* ignore_body, int32_t kinds_mask, mgf_sweep_hit\* out\);",
}


def test_header_declares_and_defines_the_queries():
    h = read("include", "mgf_hip.h")
    section = h[h.index("many small worlds"):]
    for name, sig in ENTRY_POINTS.items():
        assert re.search(r"MGF_API " + sig, section), name
    # the definition cites what the world's queries cite
    for cite in ("collision.rs:169-373", "compound.rs:150", "collision.rs:1089-1356", "collision.rs:610-1000", "physics.rs:243-251", ":1097-1100",
                 ":901-1060", ":698-719"):
        assert cite in section, cite
    for word in ("MGF_QUERY_OBSTACLES", "ignore_body", "query_launches", "query_run_ns", "mgf_batch_write_state does not move it"):
        assert word in section, word
    for text in (h, read("README.md"), read("DESIGN.md")):
        assert "no queries" not in text
    readme = read("README.md")
    for name in ("read_colliders", "raycast_many", "sweep_many"):
        assert name in readme[readme.index("mgf_batch_new"):], name


def test_library_and_binding_export_them():
    lib = mgf_amd.load_library()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in _capi.SYMBOLS, name
    for method in ("colliders", "raycast", "sweep"):
        assert callable(getattr(mgf_amd.WorldBatch, method)), method


def test_integration_md_has_the_rust_twins():
    text = read("INTEGRATION.md")
    assert "pub fn mgf_batch_read_colliders(b: *mut mgf_batch, world: i64, out: *mut mgf_moving_component, cap: i64) -> mgf_status;" in text
    assert re.search(r"pub fn mgf_batch_raycast_many\(b: \*mut mgf_batch, world: \*const i32, parts: \*const mgf_particle, n: i64, ignore_body: \*const i32,\s*"
                     r"kinds_mask: i32, out: \*mut mgf_ray_hit\) -> mgf_status;", text)
    assert re.search(r"pub fn mgf_batch_sweep_many\(b: \*mut mgf_batch, world: \*const i32, casts: \*const mgf_moving_component, n: i64, ignore_body: \*const i32,\s*"
                     r"kinds_mask: i32, out: \*mut mgf_sweep_hit\) -> mgf_status;", text)
    wrapper = text[text.index("pub struct WorldBatch"):]
    for call in ("mgf_batch_raycast_many(self.raw", "mgf_batch_sweep_many(self.raw", "mgf_batch_read_colliders(self.raw"):
        assert call in wrapper, call


def test_bad_arguments_are_refused_before_the_handle_or_a_device_is_touched():
    lib = mgf_amd.load_library()
    INV = _capi.ERR_INVALID

    def err():
        return lib.mgf_last_error().decode()
    n = 4
    world = np.zeros(n, np.int32)
    parts = np.zeros((n, 7), np.float32)
    parts[:, 3] = 1.0
    casts = np.zeros(n, _capi.MOVING_DTYPE)
    casts["r"] = 0.5
    rays_out = np.zeros(n, _capi.RAY_HIT_DTYPE)
    sweeps_out = np.zeros(n, _capi.SWEEP_HIT_DTYPE)
    cols = np.zeros(n, _capi.MOVING_DTYPE)

    def ray(h, w=world, q=parts, count=n, mask=7, out=rays_out):
        return lib.mgf_batch_raycast_many(h, w.ctypes.data if w is not None else None, q.ctypes.data if q is not None else None, count, None, mask,
                                          out.ctypes.data if out is not None else None)

    def sweep(h, w=world, q=casts, count=n, mask=7, out=sweeps_out):
        return lib.mgf_batch_sweep_many(h, w.ctypes.data if w is not None else None, q.ctypes.data if q is not None else None, count, None, mask,
                                        out.ctypes.data if out is not None else None)
    # a NULL handle
    assert ray(None) == INV and "NULL" in err()
    assert sweep(None) == INV and "NULL" in err()
    assert lib.mgf_batch_read_colliders(None, 0, cols.ctypes.data, n) == INV and "NULL" in err()
    # each refusal, with a NULL handle and with one that is never dereferenced
    bad_tag = []
    for tag in (2, 3, -1, 7):
        c = casts.copy()
        c["tag"][1] = tag
        bad_tag.append(c)
    neg = world.copy()
    neg[2] = -1
    for h in (None, C.c_void_p(16)):
        for call in (ray, sweep):
            for kw in (dict(w=None), dict(q=None), dict(out=None)):
                assert call(h, **kw) == INV and "NULL" in err(), kw
            assert call(h, count=-1) == INV and ("negative" in err() or h is None)
            for mask in (0, 8, -1, 16):
                assert call(h, mask=mask) == INV and ("kinds_mask" in err() or h is None), mask
            assert call(h, w=neg) == INV and ("world index" in err() or h is None)
        for c in bad_tag:
            assert sweep(h, q=c) == INV and ("tag" in err() or h is None)
        for w in (-2, -(1 << 40)):   # (-1 is the whole batch)
            assert lib.mgf_batch_read_colliders(h, w, cols.ctypes.data, n) == INV and ("world index" in err() or h is None)
        assert lib.mgf_batch_read_colliders(h, 0, None, n) == INV and "NULL" in err()
    assert lib.mgf_batch_counter(None, b"query_launches", C.byref(C.c_int64())) == INV


def test_the_query_kernels_use_no_scratch_and_spill_nothing():
    if not os.path.exists(os.path.join(ROOT, "mgf_amd", "libmgf_hip.so")) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    rows = kernel_resources("k_batch_query_")
    assert any("ray" in k for k in rows) and any("sweep" in k for k in rows) and "k_batch_query_gather" in rows, rows
    bad = {k: v for k, v in rows.items() if (v[2], v[4], v[5]) != ("0", "0", "0")}
    assert not bad, bad


@pytest.mark.parametrize("ticks", [0, 30])
def test_the_pile_rays_meet_bodies_terrain_and_nothing_in_every_world(ticks):
    """the conditions of the GPU test's ray set, from the oracle composition alone: its answers hold body, terrain and no hit in every
    non-empty world, and more than half of the rays hit a body - so the GPU test cannot pass on nothing"""
    from tests import batch_query_cases as BQ
    from tests.test_gpu_world_queries import Targets
    from tests.util import oracle_world
    scs = BQ.pile_scenes()
    centres = []
    for sc in scs:
        x = sc["comps"]["p"]
        if ticks and len(x):
            ow = oracle_world(sc)
            for _ in range(ticks):
                ow.step(float(sc["dt"]), sc["iters"])
            x = ow.state()["x"]     # a sphere's collider is its position (construct, compound.rs:54-66)
        centres.append(np.asarray(x, np.float32))
    rays = BQ.pile_rays(centres, BQ.COUNTS_T30 if ticks else BQ.COUNTS_T0)
    t = scs[0]["terrain"]
    v = np.asarray(t["verts"], np.float32).reshape(-1, 3) + np.asarray(t["pos"], np.float32)
    faces = v[np.asarray(t["faces"], np.int64).reshape(-1, 3)]
    body = 0
    for k, sc in enumerate(scs):
        comps = sc["comps"].copy()
        comps["p"] = centres[k]
        T = Targets([[c] for c in comps], faces)
        sel = np.nonzero(rays["world"] == k)[0]
        kinds = []
        for i in sel:
            w = T.raycast(rays["p"][i], rays["d"][i], float(rays["dt"][i]), int(rays["ignore"][i]), 7)
            kinds.append(-1 if w is None else w[1])
        if len(comps):
            assert set(kinds) == {-1, 0, 1}, (k, set(kinds))
        body += kinds.count(0)
    assert 2 * body > len(rays["world"]), (body, len(rays["world"]))
