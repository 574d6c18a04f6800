"""Static Compound obstacles per world of a batch (mgf_batch_add_obstacle, mgf_batch_set_world_obstacles, mgf_batch_obstacle_count,
mgf_batch_world_obstacle_count) without a GPU: the header, the library, the binding and the documents carry them, bad arguments are
refused before the handle or a device is touched, the batch kernels use no scratch and spill nothing - and, from the oracle alone, the
conditions on the inputs of tests/test_gpu_world_batch_obstacles.py, so that the GPU tests cannot pass on nothing.  (The scenes of
tests/batch_obstacle_cases.py were adjusted until these conditions held: the ring under the world without terrain was lowered and the
pile over it widened to one layer of 6 x 6 - spheres that overlap a ring sphere from the start report nothing, and the reference's
Compound queries its tree with a box that is right only near the compound's own frame, so the obstacles sit within half a unit of
theirs - and three in five particles aim at a component.)"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mgf_amd
from mgf_amd import _capi
from tests import batch_obstacle_cases as BC
from tests.util import ROOT, kernel_resources, read

ENTRY_POINTS = {
    "mgf_batch_add_obstacle": r"mgf_status mgf_batch_add_obstacle\(mgf_batch\* b, const mgf_compound\* c, int32_t\* id\);",
    "mgf_batch_set_world_obstacles": r"mgf_status mgf_batch_set_world_obstacles\(mgf_batch\* b, const int32_t\* world, const int32_t\* obstacle, "
                                     r"const mgf_vec3\* disp,\s*const mgf_quat\* rot, int64_t n\);",
    "mgf_batch_obstacle_count": r"int64_t mgf_batch_obstacle_count\(const mgf_batch\* b\);",
    "mgf_batch_world_obstacle_count": r"int64_t mgf_batch_world_obstacle_count\(const mgf_batch\* b, int64_t world\);",
}


# ---- a ------------------------------------------------------------------------------------------------------------------------------------
def test_header_library_binding_and_documents_carry_the_entry_points():
    h = read("include", "mgf_hip.h")
    section = h[h.index("many small worlds"):]
    lib = mgf_amd.load_library()
    for name, sig in ENTRY_POINTS.items():
        assert re.search(r"MGF_API " + sig, section), name
        assert hasattr(lib, name), name
        assert name in _capi.SYMBOLS, name
    assert re.search(r"#define MGF_BATCH_MAX_WORLD_OBSTACLES 64\b", section) and _capi.BATCH_MAX_WORLD_OBSTACLES == 64
    # the two sentences that said a batch has none are gone, in the header and in the design document
    flat = " ".join(h.split())
    assert "no obstacles" not in flat and "matches nothing" not in flat and "a batch has no obstacles" not in flat
    design = " ".join(read("DESIGN.md").split())
    assert "no obstacles, no ghosts" not in design and "is accepted and matches nothing" not in design
    for word in ("the obstacle table", "mgf_compound_set_pose", "MGF_HIT_OBSTACLE", "keeps its place in a world's list", "n_terrain like every other record"):
        assert word in " ".join(section.split()), word
    assert "obstacle list" in section[section.index("RigidBodyVec: Clone"):section.index("MGF_API mgf_status mgf_batch_copy_worlds")]
    assert lib.mgf_batch_add_obstacle.restype is C.c_int32 and lib.mgf_batch_set_world_obstacles.restype is C.c_int32
    assert lib.mgf_batch_obstacle_count.restype is C.c_int64 and lib.mgf_batch_world_obstacle_count.restype is C.c_int64
    assert len(lib.mgf_batch_add_obstacle.argtypes) == 3 and len(lib.mgf_batch_set_world_obstacles.argtypes) == 6
    for method in ("add_obstacle", "set_world_obstacles", "obstacle_count", "world_obstacle_count"):
        assert callable(getattr(mgf_amd.WorldBatch, method)), method
    for text in (read("README.md"), read("DESIGN.md")):
        assert "Obstacles per world" in text and "mgf_batch_set_world_obstacles" in text
    rust = read("INTEGRATION.md")
    assert "pub fn mgf_batch_add_obstacle(b: *mut mgf_batch, c: *const mgf_compound, id: *mut i32) -> mgf_status;" in rust
    assert "pub fn mgf_batch_obstacle_count(b: *const mgf_batch) -> i64;" in rust
    assert "pub fn mgf_batch_world_obstacle_count(b: *const mgf_batch, world: i64) -> i64;" in rust
    assert re.search(r"pub fn mgf_batch_set_world_obstacles\(b: \*mut mgf_batch, world: \*const i32, obstacle: \*const i32, disp: \*const mgf_vec3,\s*"
                     r"rot: \*const mgf_quat,\s*n: i64\) -> mgf_status;", rust)
    assert os.path.exists(os.path.join(ROOT, "tools", "batch_obstacle_bench.py"))


def test_bad_arguments_are_refused_before_the_handle_or_a_device_is_touched():
    lib = mgf_amd.load_library()
    INV = _capi.ERR_INVALID

    def err():
        return lib.mgf_last_error().decode()
    world = np.zeros(4, np.int32)
    obstacle = np.zeros(4, np.int32)
    disp = np.zeros((4, 3), np.float32)
    rot = np.tile(np.float32([1, 0, 0, 0]), (4, 1))
    oid = C.c_int32(-7)
    comp = mgf_amd.Compound(None, BC.compounds()["single"])   # a host-only compound: no device is needed to hold one

    def assign(h, w=world, o=obstacle, d=disp, r=rot, n=4):
        p = [a.ctypes.data if a is not None else None for a in (w, o, d, r)]
        return lib.mgf_batch_set_world_obstacles(h, p[0], p[1], p[2], p[3], n)
    # a NULL batch
    assert lib.mgf_batch_add_obstacle(None, comp._h, C.byref(oid)) == INV and "batch is NULL" in err()
    assert assign(None) == INV and "batch is NULL" in err()
    assert assign(None, n=0) == INV and "batch is NULL" in err()
    assert lib.mgf_batch_obstacle_count(None) == -1 and lib.mgf_batch_world_obstacle_count(None, 0) == -1
    # a handle that is never dereferenced: every check below comes before the batch or a device is looked at
    fake = C.c_void_p(16)
    assert lib.mgf_batch_add_obstacle(fake, None, C.byref(oid)) == INV and "NULL argument" in err()
    assert lib.mgf_batch_add_obstacle(fake, comp._h, None) == INV and "NULL argument" in err()
    assert oid.value == -7
    for n in (-1, -(1 << 40)):
        assert assign(fake, n=n) == INV and "negative" in err()
    assert assign(fake, w=None) == INV and "NULL argument" in err()
    assert assign(fake, o=None) == INV and "NULL argument" in err()
    assert assign(fake, w=None, o=None, d=None, r=None) == INV and "NULL argument" in err()
    neg = world.copy()
    neg[2] = -1
    assert assign(fake, w=neg) == INV and "world index" in err()
    low = obstacle.copy()
    low[3] = -2
    assert assign(fake, o=low) == INV and "obstacle id" in err()
    assert assign(fake, o=low, d=None, r=None) == INV and "obstacle id" in err()
    assert lib.mgf_batch_world_obstacle_count(fake, -1) == -1


def test_the_batch_kernels_use_no_scratch_spill_nothing_and_keep_their_lane_masks():
    if not os.path.exists(os.path.join(ROOT, "mgf_amd", "libmgf_hip.so")) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    rows = kernel_resources("k_batch_")
    for name in ("k_batch_front", "k_batch_faces", "k_batch_pairs", "k_batch_pack", "k_batch_setup", "k_batch_solve", "k_batch_query_ray",
                 "k_batch_query_sweep_bodies", "k_batch_query_sweep_faces", "k_batch_query_ray_obstacles", "k_batch_query_sweep_obstacles"):
        assert name in rows, (name, sorted(rows))
    bad = {k: v for k, v in rows.items() if (v[2], v[4], v[5]) != ("0", "0", "0")}
    assert not bad, bad
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_lane_masks.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 lane masks" in r.stdout, r.stdout


# ---- the GPU tests' inputs are not trivial: by the oracle alone ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run():
    scs = BC.obstacle_scenes()
    ows = [BC.oracle_with_obstacles(sc) for sc in scs]
    cps = [BC.oracle_compounds(sc["obstacles"]) for sc in scs]
    K = len(scs)
    ticks_with, per_entry, triple, static = [0] * K, [0] * K, [0] * K, [0] * K
    for _ in range(BC.TICKS):
        for k, (sc, ow) in enumerate(zip(scs, ows)):
            st = ow.step(float(sc["dt"]), sc["iters"])
            static[k] = max(static[k], int(st.n_terrain_constraints))
            if not len(sc["comps"]) or not cps[k]:
                continue
            oc = BC.obstacle_contacts(ow, cps[k])
            per_entry[k] = per_entry[k] + oc.sum(axis=0)
            ticks_with[k] += bool(oc.sum())
            cons = ow.constraints()
            for i in np.nonzero(oc.sum(axis=1))[0]:
                n_static = int(((cons["a"] == i) & (cons["b"] < 0)).sum())
                n_pair = int((((cons["a"] == i) | (cons["b"] == i)) & (cons["b"] >= 0)).sum())
                triple[k] += n_static > oc[i].sum() and n_pair > 0   # more static records than obstacle contacts: the rest are faces
    return dict(scs=scs, ows=ows, ticks_with=ticks_with, per_entry=per_entry, triple=triple, static=static)


def test_the_worlds_meet_their_obstacles(run):
    """measured: ticks with an obstacle contact 40, 40, 34, 40 of 40 in worlds 1-4 (counting from 1); contacts per list entry
    (1183, 433), (442, 517), (476,), (990, 221); world 7: (0, 162)"""
    scs, ows = run["scs"], run["ows"]
    assert [len(sc["comps"]) for sc in scs] == [48, 18, 36, 48, 48, 0, 8]
    assert [len(sc["obstacles"]) for sc in scs] == [2, 2, 1, 2, 0, 3, 2]
    print("ticks with an obstacle contact:", run["ticks_with"], "contacts per list entry:", run["per_entry"])
    for k in (BC.BOX, BC.FIELD, BC.BARE, BC.POSED):
        assert run["ticks_with"][k] >= 10, (k, run["ticks_with"])
        assert np.all(run["per_entry"][k] > 0), (k, run["per_entry"][k])   # every entry of the list is met
    # the world without terrain has static constraints: its obstacle's
    assert scs[BC.BARE]["terrain"] is None and run["static"][BC.BARE] > 0
    # a body with a face, a component of an obstacle and a partner in one tick, over the heightfield
    assert run["triple"][BC.FIELD] > 0, run["triple"]
    # the pose matters, and so do the obstacles
    a, b, c = (ows[k].state() for k in (BC.BOX, BC.POSED, BC.PLAIN))
    assert np.array_equal(scs[BC.BOX]["comps"], scs[BC.POSED]["comps"]) and np.array_equal(scs[BC.BOX]["comps"], scs[BC.PLAIN]["comps"])
    assert scs[BC.BOX]["obstacles"][0][0] is scs[BC.POSED]["obstacles"][0][0] and scs[BC.BOX]["obstacles"][1][0] is scs[BC.POSED]["obstacles"][1][0]
    assert not np.array_equal(a["x"], b["x"]) and not np.array_equal(a["x"], c["x"]) and not np.array_equal(b["x"], c["x"])
    # the list (empty compound, single sphere): every contact comes from list index 1
    assert len(scs[BC.HOLE]["obstacles"][0][0]) == 0 and run["per_entry"][BC.HOLE][0] == 0 and run["per_entry"][BC.HOLE][1] > 0
    assert run["static"][BC.EMPTY] == 0 and run["static"][BC.PLAIN] > 0


def test_the_rays_and_casts_meet_obstacles_bodies_terrain_and_ties(run):
    """measured: of 199 particles 52 meet an obstacle first, 43 a body (11 of them in front of an obstacle), 47 a face (30); of 129 casts
    34, 68 (36) and 15 (8); the particles and casts onto the doubled ring are ties between list entries 1 and 2, bit for bit"""
    from tests.test_gpu_world_queries import Targets
    from tests.test_gpu_world_sweeps import Sweeper, _shape
    scs, ows = run["scs"], run["ows"]
    cols = [ow.colliders()[0] for ow in ows]
    rays, casts = BC.rays_and_casts(scs, [BC.centres_of(c) for c in cols])
    assert np.any(np.diff(rays["world"]) < 0) and np.any(np.diff(casts["world"]) < 0)   # one shuffled call
    first = {-1: 0, 0: 0, 1: 0, 2: 0}
    in_front = {0: 0, 1: 0}
    ties = 0
    for k, sc in enumerate(scs):
        T = Targets([[c] for c in cols[k]], BC.world_faces(sc), sc["obstacles"])
        S = Sweeper(T, sc["obstacles"])
        for i in np.nonzero(rays["world"] == k)[0]:
            q = (rays["p"][i], rays["d"][i], float(rays["dt"][i]), int(rays["ignore"][i]))
            a = T.raycast(*q, 7)
            first[-1 if a is None else a[1]] += 1
            if a is not None and a[1] != 2 and T.raycast(*q, 4) is not None:
                in_front[a[1]] += 1
            if rays["tie"][i]:
                hits = [c.intersection(*q[:3]) for c in T.obstacles]
                if a is not None and a[1] == 2 and a[2] == 1:
                    assert hits[1] is not None and hits[1] == hits[2], hits   # the same point and t from both entries: the first wins
                    ties += 1
        for i in np.nonzero(casts["world"] == k)[0]:
            c = casts["casts"][i]
            a = S.answer(c, -1, 7)
            first[-1 if a is None else a[1]] += 1
            if a is not None and a[1] != 2 and S.answer(c, -1, 4) is not None:
                in_front[a[1]] += 1
            if casts["tie"][i]:
                sh = _shape(c["tag"], c["p"], c["d"], c["r"])
                ts = [[x["t"] for x in comp.contacts(sh, c["delta"])] for comp in T.obstacles]
                if a is not None and a[1] == 2 and a[2] == 1:
                    assert ts[1] and ts[1] == ts[2] and a[0] == min(ts[1]), ts
                    ties += 1
    n = len(rays["world"]) + len(casts["world"])
    print("first met:", first, "in front of an obstacle:", in_front, "ties:", ties, "of", n)
    assert 5 * first[2] >= n, (first, n)
    assert in_front[0] >= 1 and in_front[1] >= 1, in_front
    assert ties >= 2, ties
    assert first[-1] > 0 and first[0] > 0 and first[1] > 0


def test_from_scenes_shares_equal_compounds():
    scs = BC.obstacle_scenes()
    keys = {}
    for sc in scs:
        for comps, _, _ in sc["obstacles"]:
            keys.setdefault((len(comps), np.ascontiguousarray(comps).tobytes()), len(keys))
    assert len(keys) == 4   # ramp, ring, empty, single: every world's list draws on these
