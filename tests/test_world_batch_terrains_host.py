"""A terrain mesh and a mesh position per world of a batch (mgf_batch_add_terrain, mgf_batch_set_world_terrain, mgf_batch_terrain_count)
without a GPU: the header, the library and the binding carry them, bad arguments are refused before the handle or a device is touched,
the table WorldBatch.from_scenes(own_terrain=True) builds - and, from the oracle alone, the conditions on the inputs of
tests/test_gpu_world_batch_terrains.py, so that the GPU tests cannot pass on nothing."""
import ctypes as C
import re

import numpy as np
import pytest

import mgf_amd
from mgf_amd import _capi
from tests import batch_terrain_cases as TC
from tests.util import read

ENTRY_POINTS = {
    "mgf_batch_add_terrain": r"mgf_status mgf_batch_add_terrain\(mgf_batch\* b, const mgf_mesh\* mesh, int32_t\* id\);",
    "mgf_batch_set_world_terrain": r"mgf_status mgf_batch_set_world_terrain\(mgf_batch\* b, const int32_t\* world, const int32_t\* terrain, "
                                   r"const mgf_vec3\* pos, int64_t n\);",
    "mgf_batch_terrain_count": r"int64_t mgf_batch_terrain_count\(const mgf_batch\* b\);",
}


# ---- a ------------------------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_carry_the_entry_points():
    h = read("include", "mgf_hip.h")
    section = h[h.index("many small worlds"):]
    lib = mgf_amd.load_library()
    for name, sig in ENTRY_POINTS.items():
        assert re.search(r"MGF_API " + sig, section), name
        assert hasattr(lib, name), name
        assert name in _capi.SYMBOLS, name
    assert re.search(r"MGF_API mgf_status mgf_batch_set_terrain\(mgf_batch\* b, const mgf_mesh\* mesh\);", section)
    assert "one terrain mesh shared by every world" not in h and "the batch's terrain and" not in h
    for word in ("terrain table", "mgf_mesh_set_pos", "a world named twice keeps the last", "empty tree"):
        assert word in section, word
    assert lib.mgf_batch_add_terrain.restype is C.c_int32 and lib.mgf_batch_set_world_terrain.restype is C.c_int32
    assert lib.mgf_batch_terrain_count.restype is C.c_int64
    assert len(lib.mgf_batch_add_terrain.argtypes) == 3 and len(lib.mgf_batch_set_world_terrain.argtypes) == 5
    for method in ("add_terrain", "set_world_terrain", "terrain_count", "set_terrain"):
        assert callable(getattr(mgf_amd.WorldBatch, method)), method
    for text in (read("README.md"), read("DESIGN.md")):
        assert "mgf_batch_set_world_terrain" in text
    rust = read("INTEGRATION.md")
    assert "pub fn mgf_batch_add_terrain(b: *mut mgf_batch, mesh: *const mgf_mesh, id: *mut i32) -> mgf_status;" in rust
    assert "pub fn mgf_batch_terrain_count(b: *const mgf_batch) -> i64;" in rust
    assert re.search(r"pub fn mgf_batch_set_world_terrain\(b: \*mut mgf_batch, world: \*const i32, terrain: \*const i32, pos: \*const mgf_vec3,\s*n: i64\) -> mgf_status;", rust)


def test_bad_arguments_are_refused_before_the_handle_or_a_device_is_touched():
    lib = mgf_amd.load_library()
    INV = _capi.ERR_INVALID

    def err():
        return lib.mgf_last_error().decode()
    world = np.zeros(4, np.int32)
    terrain = np.zeros(4, np.int32)
    pos = np.zeros((4, 3), np.float32)
    tid = C.c_int32(-7)
    mesh = mgf_amd.Mesh(None)   # a host-only mesh: no device is needed to hold one

    def assign(h, w=world, t=terrain, p=pos, n=4):
        return lib.mgf_batch_set_world_terrain(h, w.ctypes.data if w is not None else None, t.ctypes.data if t is not None else None,
                                               p.ctypes.data if p is not None else None, n)
    # a NULL batch
    assert lib.mgf_batch_add_terrain(None, mesh._h, C.byref(tid)) == INV and "batch is NULL" in err()
    assert assign(None) == INV and "batch is NULL" in err()
    assert assign(None, n=0) == INV and "batch is NULL" in err()
    assert lib.mgf_batch_terrain_count(None) == -1
    # a handle that is never dereferenced: every check below comes before the batch or a device is looked at
    fake = C.c_void_p(16)
    assert lib.mgf_batch_add_terrain(fake, None, C.byref(tid)) == INV and "NULL argument" in err()
    assert lib.mgf_batch_add_terrain(fake, mesh._h, None) == INV and "NULL argument" in err()
    assert tid.value == -7
    for n in (-1, -(1 << 40)):
        assert assign(fake, n=n) == INV and "negative" in err()
    assert assign(fake, w=None) == INV and "NULL argument" in err()
    assert assign(fake, t=None) == INV and "NULL argument" in err()
    assert assign(fake, w=None, t=None, p=None) == INV and "NULL argument" in err()
    neg = world.copy()
    neg[2] = -1
    assert assign(fake, w=neg) == INV and "world index" in err()
    low = terrain.copy()
    low[3] = -2
    assert assign(fake, t=low) == INV and "terrain id" in err()
    assert assign(fake, t=low, p=None) == INV and "terrain id" in err()


# ---- b ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracles():
    scs = TC.mixed_scenes()
    ows, stats = TC.run_oracles(scs, TC.TICKS)
    return scs, ows, stats


def test_the_mixed_scenes_meet_their_terrains_and_differ(oracles):
    scs, ows, stats = oracles
    assert [len(sc["comps"]) for sc in scs] == [48, 48, 96, 48, 27, 0]
    for k, sc in enumerate(scs):
        most = max(s[1] for s in stats[k])
        if sc["terrain"] is not None and len(sc["comps"]):
            assert most > 0, k
            assert max(s[1] for t, s in enumerate(stats[k]) if t + 1 in TC.LIST_TICKS) > 0, k   # in a list that is compared
        else:
            assert most == 0, k
    fell = scs[TC.BARE]["comps"]["p"][:, 1] - ows[TC.BARE].state()["x"][:, 1]
    assert np.all(fell > 1.0), "the bodies without terrain fall freely: about g t^2 / 2 = 2.2 in 40 ticks"
    a, b = (ows[k].state() for k in TC.HEIGHTFIELDS)
    assert not np.array_equal(a["x"], b["x"]) and not np.array_equal(a["v"], b["v"])
    t0, t1 = (ows[k].state() for k in TC.TWINS)
    assert np.array_equal(scs[TC.TWINS[0]]["comps"], scs[TC.TWINS[1]]["comps"])
    assert not np.array_equal(t0["x"], t1["x"]), "the raised terrain changes nothing"
    # the terrains: two heightfields that differ, one of them twice (its position apart), a box twice
    ta, tb = scs[0]["terrain"], scs[1]["terrain"]
    assert ta["verts"].shape == tb["verts"].shape and not np.array_equal(ta["verts"], tb["verts"])
    assert float(np.float32(TC.RAISE)) != TC.RAISE


def test_the_mixed_rays_meet_faces_bodies_and_nothing_in_every_world(oracles):
    from tests.test_gpu_world_queries import Targets
    scs, ows, _ = oracles
    cols = [ow.colliders()[0] for ow in ows]
    rays = TC.mixed_rays([TC.centres_of(c) for c in cols])
    answers = {}
    for k, sc in enumerate(scs):
        T = Targets([[c] for c in cols[k]], TC.world_faces(sc))
        sel = np.nonzero(rays["world"] == k)[0]
        assert len(sel) == TC.RAY_COUNTS[k] + TC.PROBES ** 2
        got = [T.raycast(rays["p"][i], rays["d"][i], float(rays["dt"][i]), int(rays["ignore"][i]), 7) for i in sel]
        kinds = {-1 if w is None else w[1] for w in got}
        if sc["terrain"] is not None and len(sc["comps"]):
            assert kinds == {-1, 0, 1}, (k, kinds)
        elif sc["terrain"] is not None:
            assert kinds == {-1, 1}, (k, kinds)
        else:
            assert kinds == {-1, 0}, (k, kinds)
            assert all(T.raycast(rays["p"][i], rays["d"][i], float(rays["dt"][i]), -1, 2) is None for i in sel)
        answers[k] = {int(rays["probe"][i]): w for i, w in zip(sel, got) if rays["probe"][i] >= 0}
    # the same probe over the two heightfields - and over the twin's raised one - answers with another face or another t
    for x, y in (TC.HEIGHTFIELDS, TC.TWINS):
        differ = [g for g in answers[x] if answers[x][g] is not None and answers[y][g] is not None and answers[x][g][1] == answers[y][g][1] == 1
                  and answers[x][g][:3] != answers[y][g][:3]]
        assert differ, (x, y)


# ---- c ------------------------------------------------------------------------------------------------------------------------------------
def test_terrain_table_shares_equal_geometry():
    scs = TC.mixed_scenes()
    entries, assign = _capi.terrain_table([sc["terrain"] for sc in scs])
    assert len(entries) == 3
    assert [e for e, _ in assign] == [0, 1, 2, 0, -1, 2]
    assert entries[0] is scs[0]["terrain"] and entries[1] is scs[1]["terrain"] and entries[2] is scs[2]["terrain"]
    for k, sc in enumerate(scs):
        if sc["terrain"] is not None:
            assert np.array_equal(np.float32(assign[k][1]), sc["terrain"]["pos"]), k
    assert assign[3][1] != assign[0][1] and assign[3][1][1] == float(np.float32(TC.RAISE))
    # the order of the scenes is the order of the table; a copy of the arrays is the same geometry, one vertex moved is not
    entries, assign = _capi.terrain_table([sc["terrain"] for sc in scs[::-1]])
    assert [e for e, _ in assign] == [0, -1, 1, 0, 2, 1]
    t = scs[0]["terrain"]
    moved = dict(t, verts=t["verts"].copy())
    moved["verts"][5, 1] = np.nextafter(moved["verts"][5, 1], np.float32(1.0))
    entries, assign = _capi.terrain_table([t, dict(t, verts=t["verts"].copy(), faces=t["faces"].copy()), moved, None])
    assert len(entries) == 2 and [e for e, _ in assign] == [0, 0, 1, -1]
    assert _capi.terrain_table([]) == ([], []) and _capi.terrain_table([None])[0] == []
