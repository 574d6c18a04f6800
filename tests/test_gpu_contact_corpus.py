"""Every contact branch through every front end of the tick: the corpus of tests/contact_corpus.py (whose reach tests/test_contact_corpus.py
measures on the CPU) single-shot through the C-ABI, then planted in worlds and run under each front end that can take it - constraint list and
state after one solve against the oracle's, bit for bit (+0 == -0, NaN == NaN in the same place), and the world's counters have to say that
the intended path is the one that ran."""

import numpy as np
import pytest

from oracle import oracle as O
from tests import contact_corpus as CC
from tests.util import CONSTRAINT_FIELDS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import mgf_amd
    c = mgf_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def corpus():
    cases = CC.corpus()
    want, counts = CC.oracle_answers(cases)
    return cases, want, counts


def _where(cases, idx):
    return [(CC.TYPES[CC.case_type(cases[i:i + 1])[0]], CC.FAMILIES[cases["family"][i]], CC.LADDER[cases["rung"][i]]) for i in idx[:5]]


def _comp(s):
    k = int(s["kind"])
    return (k, s["v"][:3], s["v"][3:6] if k == CC.CAPSULE else np.zeros(3, np.float32), float(s["v"][6] if k == CC.CAPSULE else s["v"][3]))


# ---- a. single-shot -------------------------------------------------------------------------------------------------------------------
def test_contacts_batch_is_the_oracle_on_the_whole_corpus(ctx, corpus):
    """count, order, a, b, n, t of every case at every rung of the ladder"""
    import mgf_amd
    cases, want, wcnt = corpus
    n = len(cases)
    got, gcnt = np.zeros((n, 2), O.CONTACT_DTYPE), np.zeros(n, np.int32)
    arrs = [np.ascontiguousarray(cases[f]) for f in ("a", "va", "b", "vb", "hv")]
    mgf_amd._capi._check(mgf_amd._capi.load_library().mgf_contacts_batch(ctx._h, n, *[a.ctypes.data for a in arrs], got.ctypes.data, gcnt.ctypes.data))
    bad = np.nonzero(gcnt != wcnt)[0]
    assert len(bad) == 0, (len(bad), _where(cases, bad))
    for k in range(2):
        live = wcnt > k
        for f in ("a", "b", "n", "t"):
            g, w = got[f][live, k].reshape(live.sum(), -1), want[f][live, k].reshape(live.sum(), -1)
            bad = np.nonzero(live)[0][~np.all((g == w) | (np.isnan(g) & np.isnan(w)), axis=1)]
            assert len(bad) == 0, (f, k, len(bad), _where(cases, bad))
    cl = CC.classes(cases, want, wcnt)
    print("cases per type and class:", cl)
    assert all(v >= 20 for t in CC.TYPES for key, v in cl[t].items() if key != "two")


def test_the_triangle_reject_drops_no_contact_of_the_corpus(ctx, corpus):
    """comp_tri_far beside the body-triangle tests (mgf_tri_reject_batch) on every triangle case: the count is the oracle's, and no case with a
    contact is dropped - small bodies 1e5 from the origin included"""
    import mgf_amd
    cases, want, wcnt = corpus
    tri = cases["a"]["kind"] == CC.TRIANGLE
    tc, wc = cases[tri], wcnt[tri]
    cap = tc["b"]["kind"] == CC.CAPSULE
    far, cnt = mgf_amd._capi.tri_reject_batch(ctx, tc["b"]["kind"], tc["b"]["v"][:, :3], tc["b"]["v"][:, 3:6] * cap[:, None],
                                              np.where(cap, tc["b"]["v"][:, 6], tc["b"]["v"][:, 3]), tc["vb"], tc["a"]["v"][:, :9])
    bad = np.nonzero(cnt != wc)[0]
    assert len(bad) == 0, (len(bad), _where(tc, bad))
    lost = np.nonzero((far == 1) & (wc > 0))[0]
    assert len(lost) == 0, (len(lost), _where(tc, lost))
    print(f"comp_tri_far dropped {int(far.sum())} of {len(far)} triangle cases, none of the {int((wc > 0).sum())} with a contact")
    assert far.sum() > 0.05 * len(far)


def test_local_contacts_pair_is_the_oracle_behind_its_reject(ctx, corpus):
    """mgf_local_contacts_pair runs comp_pair_far ahead of the tests (contacts_batch does not): every pair case of the corpus (but the family of
    zero radii, which is no body)"""
    import mgf_amd
    cases, want, wcnt = corpus
    fam = np.array(CC.FAMILIES)[cases["family"]]
    pair = np.nonzero((cases["a"]["kind"] != CC.TRIANGLE) & (fam != "cc_zero_radii"))[0]
    sel = pair
    lw, lcnt = O.local_contacts_pair_batch(CC._comp(cases["a"][sel]), cases["va"][sel], CC._comp(cases["b"][sel]), cases["vb"][sel])
    assert np.array_equal(lcnt, wcnt[sel])
    lost, n_hit = [], 0
    for k, i in enumerate(sel):
        c = cases[i]
        g = mgf_amd.local_contacts_pair(ctx, _comp(c["a"]) + (c["va"],), _comp(c["b"]) + (c["vb"],))
        if len(g) != lcnt[k]:
            lost.append(i)
            continue
        if len(g):
            n_hit += 1
            for f in ("local_a", "local_b", "a", "b", "n", "t"):
                assert CC.same_f32(g[0][f], lw[f][k, 0]), (f, _where(cases, [i]))
    assert not lost, (len(lost), _where(cases, lost))
    assert n_hit > 40000
    print(f"{len(sel)} pairs through mgf_local_contacts_pair, {n_hit} with a contact")


def test_local_contacts_mesh_is_the_oracle_on_triangle_cases(ctx, corpus):
    """a mesh of one face per case: LocalContacts<Mesh> (count, order, every field) on every triangle case of the corpus"""
    import mgf_amd
    cases, want, wcnt = corpus
    tri = np.nonzero(cases["a"]["kind"] == CC.TRIANGLE)[0]
    face = np.array([[0, 1, 2]], np.uint32)
    n_hit = n_two = 0
    for i in tri:
        c = cases[i]
        verts = c["a"]["v"][:9].reshape(3, 3)
        m = mgf_amd.Mesh(ctx)
        m.build(verts, face)
        g = mgf_amd.local_contacts_mesh(ctx, _comp(c["b"]) + (c["vb"],), m)
        ow = O.World()
        ow.set_terrain(verts, face, (0.0, 0.0, 0.0))
        ow.add_bodies(CC._comp(cases["b"][i:i + 1]), 1.0, 0.3, 0.6, (0.0, 0.0, 0.0))
        ow.set_state(delta=c["vb"])
        w = ow.terrain_contacts(0)
        assert len(g) == len(w), _where(cases, [i])
        for gg, ww in zip(g, w):
            for f in ("local_a", "local_b", "a", "b", "n", "t"):
                assert CC.same_f32(gg[f], ww[f]), (f, _where(cases, [i]))
        n_hit += len(w) > 0
        n_two += len(w) == 2
    assert n_hit > 40000 and n_two > 5000, (n_hit, n_two)   # (fewer than single-shot: a mesh looks at a face only where the boxes overlap)


# ---- b. through the tick ----------------------------------------------------------------------------------------------------------------
COUNTERS = ("pair_brick_ticks", "fused_contacts_ticks", "front_rows_ticks", "front_rows", "terrain_grid", "wide_ticks", "wide_bodies",
            "early_cells_ticks", "grid_too_wide", "row_overflows", "capacity_retries", "two_pass_ticks", "tree_ticks", "big_parts_ticks", "max_parts")


def _gpu_world(ctx, scene, options):
    import mgf_amd
    keep = []

    def mesh(w, m):
        me = mgf_amd.Mesh(ctx)
        me.build(m["verts"], m["faces"])
        me.set_pos(m["pos"])
        w.set_terrain(me)
        keep.append(me)

    def obstacle(w, ob):
        c = mgf_amd.Compound(ctx, ob)
        w.add_obstacle(c)
        keep.append(c)
    w = CC.build_world(scene, lambda: mgf_amd.World(ctx), mesh, obstacle)
    w._keep = keep
    for k, v in options.items():
        w.set_option(k, v)
    return w


def _same_constraints(got, want, what, check_impulse=False):
    if len(got) != len(want):
        pg, pw = set(zip(got["a"].tolist(), got["b"].tolist())), set(zip(want["a"].tolist(), want["b"].tolist()))
        raise AssertionError(f"{what}: {len(got)} constraints, the oracle has {len(want)}; body pairs only here {sorted(pg - pw)[:4]}, only there {sorted(pw - pg)[:4]}")
    assert np.array_equal(got["a"], want["a"]) and np.array_equal(got["b"], want["b"]), f"{what}: the order of the bodies differs"
    for f in CONSTRAINT_FIELDS + (["normal_impulse"] if check_impulse else []):
        g, w = got[f].reshape(len(got), -1), want[f].reshape(len(want), -1)
        bad = np.nonzero(~np.all((g == w) | (np.isnan(g) & np.isnan(w)), axis=1))[0]
        assert len(bad) == 0, f"{what}: constraint field {f} differs in {len(bad)} rows, first {bad[0]} (bodies {got['a'][bad[0]]}, {got['b'][bad[0]]}): {g[bad[0]]} vs {w[bad[0]]}"


def _same_state(gw, ow, what):
    g, o = gw.state(), ow.state()
    for k in ("x", "q", "v", "omega", "delta"):
        assert CC.same_f32(g[k], o[k]), f"{what}: {k} differs"


def run_front_end(ctx, scene, options, ticks=2):
    """the scene in both worlds: constraint list, then the state after one solve, `ticks` times over; returns the GPU world's counters"""
    ow = CC.oracle_world(scene)
    gw = _gpu_world(ctx, scene, options)
    seen = {}
    recount = CC.LeafRecount(ow) if scene["compound"] is None else None
    for tick in range(ticks):
        what = f"{options} tick {tick}"
        so = CC.constrain(ow, scene, lambda w, **kw: w.set_state(**kw)) if tick == 0 else ow.build_constraints(1.0)
        sg = CC.constrain(gw, scene, lambda w, **kw: w.write_state(**kw)) if tick == 0 else gw.build_constraints(1.0)
        _same_constraints(gw.constraints(), ow.constraints(), what)
        assert (sg.n_constraints, sg.n_terrain_constraints) == (so.n_constraints, so.n_terrain_constraints), what
        leaves = recount.count(ow) if recount is not None else None
        if sg.n_pair_candidates != so.n_pair_candidates:
            # The one stated limit (include/mgf_hip.h at mgf_step_stats): 1e5 from the origin the reference's tree can lose a pair whose
            # boxes touch within an ulp to the rounding of an ancestor's box; the HIP path counts by the leaf boxes.  Nowhere else, and then exactly so.
            assert scene["offset"] >= 1e5 and leaves is not None, f"{what}: {sg.n_pair_candidates} pair candidates, the oracle has {so.n_pair_candidates}"
            assert sg.n_pair_candidates == leaves > so.n_pair_candidates, f"{what}: {sg.n_pair_candidates} pair candidates, {leaves} by the leaf boxes, the oracle has {so.n_pair_candidates}"
            seen["tree_lost_candidates"] = seen.get("tree_lost_candidates", 0) + leaves - int(so.n_pair_candidates)
        elif leaves is not None:
            assert leaves == sg.n_pair_candidates, f"{what}: {sg.n_pair_candidates} pair candidates, {leaves} by the leaf boxes"
        ow.solve(CC.ITERS)
        gw.solve(CC.ITERS)
        _same_constraints(gw.constraints(), ow.constraints(), what, check_impulse=True)
        _same_state(gw, ow, what)
        for k in COUNTERS:
            seen[k] = max(seen.get(k, 0), gw.counter(k))
        seen[f"n_constraints_{tick}"] = int(so.n_constraints)
        seen[f"n_terrain_constraints_{tick}"] = int(so.n_terrain_constraints)
        seen["n_pair_candidates"] = int(sg.n_pair_candidates)
    return seen


# world -> [(options, what the counters must say after the two ticks)]: a silent fall-back to another path must not pass for coverage
_FR = {"front_rows": 1, "front_rows_check": 1}
FRONT_ENDS = {
    # spheres over a mesh too small for a face grid: k_pair_brick or k_pair_grid<true>, then k_contacts_spheres with tri_msphere_x4
    "spheres": [({}, [("pair_brick_ticks", ">=", 1), ("fused_contacts_ticks", "==", 2), ("terrain_grid", "==", 0), ("front_rows_ticks", "==", 0)]),
                ({"pair_brick": 0}, [("pair_brick_ticks", "==", 0), ("fused_contacts_ticks", "==", 2)]),
                ({"fused_contacts": 0}, [("fused_contacts_ticks", "==", 0), ("pair_brick_ticks", ">=", 1)]),
                ({"no_fused_narrowphase": 1}, [("fused_contacts_ticks", "==", 0), ("pair_brick_ticks", "==", 0), ("front_rows_ticks", "==", 2)]),
                ({"broadphase_tree": 1}, [("tree_ticks", "==", 2), ("two_pass_ticks", "==", 0), ("pair_brick_ticks", "==", 0), ("front_rows_ticks", "==", 0)]),
                ({"two_pass_candidates": 1}, [("two_pass_ticks", "==", 2), ("tree_ticks", "==", 0), ("pair_brick_ticks", "==", 0), ("front_rows_ticks", "==", 0)])],
    "spheres_face_grid": [({}, [("terrain_grid", "==", 1), ("fused_contacts_ticks", "==", 0), ("pair_brick_ticks", ">=", 1)]),
                          ({"terrain_tree": 1}, [("terrain_grid", "==", 0), ("fused_contacts_ticks", "==", 2)])],
    # capsules and spheres over a small mesh: the list-free front end on the rows of k_integrate's tail, or the candidate lists
    "mixed_0": [(_FR, [("front_rows_ticks", "==", 2), ("front_rows", "==", 1), ("terrain_grid", "==", 0)]),
                ({"front_rows": 0}, [("front_rows_ticks", "==", 0), ("pair_brick_ticks", ">=", 1)]),
                ({"terrain_tree": 1}, [("front_rows_ticks", "==", 2), ("terrain_grid", "==", 0)]),
                ({"side_stream": 0}, [("front_rows_ticks", "==", 2)]),
                ({"fused_contacts": 0}, [("front_rows_ticks", "==", 0), ("pair_brick_ticks", ">=", 1)])],
    "mixed_1": [(_FR, [("front_rows_ticks", "==", 2)]), ({"front_rows": 0}, [("front_rows_ticks", "==", 0), ("pair_brick_ticks", ">=", 1)])],
    "mixed_2": [(_FR, [("front_rows_ticks", "==", 2)]), ({"front_rows": 0}, [("front_rows_ticks", "==", 0), ("pair_brick_ticks", ">=", 1)])],
    # ... over a mesh with a face grid: k_near_list + k_terrain_near beside the pair search, or k_terrain_grid and the lists
    "mixed_face_grid": [(_FR, [("front_rows_ticks", "==", 2), ("front_rows", "==", 1), ("terrain_grid", "==", 1)]),
                        ({"front_rows": 0}, [("front_rows_ticks", "==", 0), ("terrain_grid", "==", 1), ("pair_brick_ticks", ">=", 1)]),
                        ({"terrain_tree": 1}, [("front_rows_ticks", "==", 2), ("terrain_grid", "==", 0)]),
                        ({"side_stream": 0}, [("front_rows_ticks", "==", 2), ("terrain_grid", "==", 1)])],
    # the static receivers as one obstacle Compound: an obstacle keeps a world on the candidate lists
    "obstacle": [({}, [("front_rows_ticks", "==", 0), ("n_terrain_constraints_0", ">=", 1000)])],
    # bodies of two parts over a small mesh: k_pair_grid_n<true> and k_terrain_contacts<2> on the rows of k_integrate's tail; over a face grid the lists
    "two_parts": [({}, [("front_rows_ticks", ">=", 1), ("front_rows", "==", 1), ("max_parts", "==", 2), ("n_terrain_constraints_0", ">=", 10)]),
                  ({"front_rows": 0}, [("front_rows_ticks", "==", 0), ("pair_brick_ticks", ">=", 1), ("n_terrain_constraints_0", ">=", 10)])],
    "two_parts_face_grid": [({}, [("terrain_grid", "==", 1), ("front_rows_ticks", "==", 0), ("pair_brick_ticks", ">=", 1), ("n_terrain_constraints_0", ">=", 100)]),
                            ({"terrain_tree": 1}, [("terrain_grid", "==", 0), ("front_rows_ticks", "==", 2), ("n_terrain_constraints_0", ">=", 100)])],
    # four parts: k_narrow_pairs_parts<kMaxParts> / k_narrow_terrain_parts<kMaxParts>
    "four_parts": [({}, [("max_parts", "==", 4), ("big_parts_ticks", "==", 0), ("front_rows_ticks", "==", 0), ("n_terrain_constraints_0", ">=", 10)])],
    "four_parts_face_grid": [({}, [("max_parts", "==", 4), ("terrain_grid", "==", 1), ("big_parts_ticks", "==", 0), ("n_terrain_constraints_0", ">=", 100)]),
                             ({"terrain_tree": 1}, [("max_parts", "==", 4), ("terrain_grid", "==", 0), ("n_terrain_constraints_0", ">=", 100)])],
    "three_parts_obstacle": [({}, [("max_parts", "==", 3), ("front_rows_ticks", "==", 0), ("n_terrain_constraints_0", ">=", 100)])],
    # 7 and 32 parts: k_narrow_pairs_big / k_narrow_terrain_big (a lane per part)
    "seven_parts": [({}, [("big_parts_ticks", "==", 2), ("max_parts", "==", 7), ("terrain_grid", "==", 1), ("n_terrain_constraints_0", ">=", 100)]),
                    ({"terrain_tree": 1}, [("big_parts_ticks", "==", 2), ("terrain_grid", "==", 0), ("n_terrain_constraints_0", ">=", 100)])],
    "seven_parts_small_mesh": [({}, [("big_parts_ticks", "==", 2), ("max_parts", "==", 7), ("terrain_grid", "==", 0), ("n_terrain_constraints_0", ">=", 10)])],
    "thirty_two_parts": [({}, [("big_parts_ticks", "==", 2), ("max_parts", "==", 32), ("n_terrain_constraints_0", ">=", 1000)])],
    "wide": [({}, [("wide_ticks", ">=", 1), ("wide_bodies", ">=", 4)]), ({"wide_list": 0}, [("wide_ticks", "==", 0), ("wide_bodies", "==", 0), ("tree_ticks", "==", 0)])],
}
_scenes = {}


def _scene(rung, name):
    if rung not in _scenes:
        _scenes.clear()          # (one rung's worlds at a time)
        _scenes[rung] = CC.world_scenes(rung)
    return _scenes[rung][name]


@pytest.mark.parametrize("rung", CC.WORLD_RUNGS, ids=[f"rung{r}" for r in CC.WORLD_RUNGS])
@pytest.mark.parametrize("name,k", [(n, k) for n, fe in FRONT_ENDS.items() for k in range(len(fe))])
def test_planted_cases_through_the_tick(ctx, rung, name, k):
    """two ticks (k_pair_wide engages from the second) of a world of planted cases under one front end"""
    options, path = FRONT_ENDS[name][k]
    scene = _scene(rung, name)
    seen = run_front_end(ctx, scene, options)
    print(f"rung {CC.LADDER[rung]} {name} {options}: " + ", ".join(f"{key} = {v}" for key, v in seen.items() if v))
    assert seen["n_constraints_0"] > 100 and seen["n_constraints_1"] > 100
    if scene["obstacle"] is None:
        assert seen["n_pair_candidates"] > 100
    for key, op, v in path:
        assert (seen[key] == v) if op == "==" else (seen[key] >= v), f"{name} {options}: {key} = {seen[key]}, expected {op} {v} - another path ran"
