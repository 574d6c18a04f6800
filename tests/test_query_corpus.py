"""The query corpus (tests/query_corpus.py) proves its own reach on the CPU, as tests/test_contact_corpus.py does for the contacts: the
oracle, instrumented with gcov, runs the corpus in a child process and every executable line of the ray tests has to have run; the
unfiltered reference (every target of a world through the oracle's single test) is compared with the filtered one the older query
tests use, family by family; and every planted world keeps the share of its queries that hit something between 20 % and 80 %.  Run it
alone with

    pytest -m "not gpu" -s tests/test_query_corpus.py

(-s shows the coverage list and the per-family counts).  The GPU side (tests/test_gpu_query_corpus.py) then holds the single-shot
entry, the lone world and the batch to the unfiltered oracle on these very inputs."""
import collections

import numpy as np
import pytest

from tests import contact_corpus as CC
from tests import oracle_coverage
from tests import query_corpus as QC

needs_gcov = pytest.mark.skipif(not oracle_coverage.available(), reason="gcov (or g++) is not on this machine: the coverage of the corpus cannot be measured")

# contains(Triangle), ray_sphere, ray_capsule, ray_plane, ray_polygon, ray_aabb of mgf_collision.hpp; Intersects<Compound> of mgf_compound.hpp
# and BVH::raytrace of mgf_bvh.hpp (the compound intersection walk)
RAY_LINES = {"mgf_collision.hpp": [(35, 42), (51, 149)], "mgf_compound.hpp": [(88, 106)], "mgf_bvh.hpp": [(192, 209)]}
# ---- lines the corpus need not reach: one reason per line ------------------------------------------------------------------------------
ALLOWED = {}      # {file: {line: reason}} - empty: the corpus reaches them all


def _in(ranges, line):
    return any(lo <= line <= hi for lo, hi in ranges)


# ---- the targets of a corpus world without a GPU ---------------------------------------------------------------------------------------
IDENTITY = ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0))


def corpus_obstacles(w):
    return [(ob, IDENTITY[0], IDENTITY[1]) for ob in (w["obstacle"] or [])]


def corpus_parts(w):
    """{body index: its world-space parts} of the bodies of several components (behind the ordinary ones)"""
    if w["compound"] is None:
        return {}
    off, n0 = w["compound"]["offsets"], len(w["comps"])
    return {n0 + b: w["compound"]["comps"][off[b]:off[b + 1]] for b in range(len(off) - 1)}


def corpus_targets(w):
    """the world as the unstepped GPU world shows it: tests.test_gpu_world_queries.Targets over the planted components, faces and obstacles"""
    from tests.test_gpu_world_queries import Targets
    bodies = [[c] for c in w["comps"]] + [list(p) for _, p in sorted(corpus_parts(w).items())]
    faces = None
    if w["mesh"] is not None:
        faces = (w["mesh"]["verts"] + w["mesh"]["pos"])[w["mesh"]["faces"].astype(np.int64)]
    return Targets(bodies, faces, corpus_obstacles(w))


def _key(ans):
    """an answer of Targets.raycast / Sweeper.answer as something comparable: None, or (kind, index, part, the floats' bits)"""
    if ans is None:
        return None
    if len(ans) == 5:
        t, kind, index, part, ip = ans
        return (kind, index, part, np.float32(t).tobytes(), np.asarray(ip, np.float32).tobytes())
    t, kind, index, part, j, c = ans
    return (kind, index, part, j) + tuple(np.asarray(c[k], np.float32).tobytes() for k in ("a", "b", "n", "t"))


def ray_differences(T, p, d, dt, banded=True):
    """indices of the particles whose filtered and unfiltered answers differ.  banded=False: without the direction band of
    include/mgf_hip.h (only d = 0 hits nothing), the definition as it stood before the band"""
    band = None if banded else (0.0, np.inf)
    full = T.raycast_all(p, d, dt, band=band)
    dts = np.broadcast_to(dt, (len(p),))
    return [i for i in range(len(p)) if _key(T.raycast(p[i], d[i], float(dts[i]), band=band)) != _key(full[i])], full


# ---- coverage ------------------------------------------------------------------------------------------------------------------------------
def run_ray_corpus():
    """the load the coverage is measured under: the pair-level corpus and every planted world's particles through the unfiltered reference"""
    QC.oracle_answers(QC.ray_families())
    for rung in (0, 13):
        for name in QC.WORLDS:
            w = QC.ray_world(name, rung)
            corpus_targets(w).raycast_all(*QC.world_particles(w))


@needs_gcov
def test_the_ray_corpus_reaches_every_line_of_the_ray_tests():
    with oracle_coverage.Coverage() as cov:
        cov.run("from tests.test_query_corpus import run_ray_corpus; run_ray_corpus()")
        lines = cov.lines()
    print("\nlines of the ray tests the corpus need not reach:")
    for f, allowed in ALLOWED.items():
        for line, why in sorted(allowed.items()):
            print(f"  {f}:{line}  {why}")
    if not any(ALLOWED.values()):
        print("  (none)")
    for f, ranges in RAY_LINES.items():
        assert any(c > 0 for l, c in lines[f].items() if _in(ranges, l)), f
        miss = sorted(l for l, c in lines[f].items() if c == 0 and _in(ranges, l))
        allowed = ALLOWED.get(f, {})
        unexpected = [l for l in miss if l not in allowed]
        assert not unexpected, f"{f}: the ray corpus never runs lines {unexpected}"
        stale = [l for l in allowed if lines[f].get(l, 0) > 0]
        assert not stale, f"{f}: lines {stale} are allowed to be missed but ran - drop them from the list"


# ---- families ------------------------------------------------------------------------------------------------------------------------------
def test_every_family_is_there_at_every_rung_it_is_laid_over():
    c = QC.ray_families()
    names = QC.family_names(c)
    ladder = [f for f in QC.FAMILIES if f.startswith("direction_ladder")]
    assert len(ladder) == 6
    for f in QC.FAMILIES:
        rungs = [0] if f in ladder else range(len(CC.LADDER))
        for r in rungs:
            if f.startswith("dt_"):
                assert np.sum((names == f) & (c["rung"] == r)) >= 10, (f, r)
            else:
                assert np.sum((names == f) & (c["rung"] == r)) >= 6, (f, r)
    for f in ladder:        # every decade, three directions
        m = names == f
        assert set(QC.decade_of(c[m]).tolist()) == set(QC.DECADES)
    hit, _, t = QC.oracle_answers(c)
    for kind in ("sphere", "capsule", "triangle"):      # the hit's own t as dt: just below misses, at and just above hit
        assert not np.any(hit[names == f"dt_below_hit:{kind}"] == 1)
        assert np.all(hit[names == f"dt_at_hit:{kind}"] == 1) and np.all(hit[names == f"dt_above_hit:{kind}"] == 1)
    a, b = QC.ray_families(), QC.ray_families()
    assert a.tobytes() == b.tobytes()
    s = QC.sweep_base()
    fam = np.array(CC.FAMILIES)[s["family"]]
    for f in ("sweep_sphere_equal_centres", "sweep_delta_zero_overlapping", "sweep_delta_tiny", "sweep_starts_overlapping", "sweep_capsule_at_rest_parallel",
              "reject_head_on", "reject_tri_reach", "tc_level_both_ends_t0_rot0", "cc_parallel_rest_overlapping", "ts_edge0_front_impact"):
        assert np.any(fam == f), f


def test_the_evidence_of_the_direction_ladder():
    """what the issue reports of the single tests, as the oracle answers today: hits nowhere near the line for tiny and for huge directions"""
    from oracle import oracle as O
    S, K = O.shape(O.SPHERE, (50, 30, -20), 0.5), O.shape(O.CAPSULE, (50, 30, -20), (0, 1, 0), 0.5)
    inf = float("inf")
    for sh in (S, K):
        ip, t = O.intersection((0, 0, 0), (1e-23, 0, 0), inf, sh)
        assert t == inf and ip[0] == inf
        ip, t = O.intersection((0, 0, 0), tuple(np.float32([0.7, 0.5, -0.3]) * np.float32(1e-23)), inf, sh)
        assert t == 0 and ip == (0, 0, 0)
    assert O.intersection((0, 0, 0), (1e18, 0, 0), inf, S)[1] == 0
    assert np.isnan(O.intersection((0, 0, 0), (1e18, 0, 0), inf, K)[1])
    import tests.test_gpu_world_queries as WQ
    assert WQ.RAY_DMIN == np.float32(1e-20) and WQ.RAY_DMAX == np.float32(1e12)      # the measured band (EXPERIMENTS.md) is the header's
    assert not WQ.ray_castable((1e-23, 0, 0)) and not WQ.ray_castable((1e18, 0, 0)) and not WQ.ray_castable((0, 0, 0)) and not WQ.ray_castable((1, np.nan, 0))
    assert WQ.ray_castable((1e-20, 0, 0)) and WQ.ray_castable((0, -1e12, 1.0))


# ---- the planted worlds ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def worlds():
    out = {}
    for rung in CC.WORLD_RUNGS:
        for name in QC.WORLDS:
            w = QC.ray_world(name, rung)
            out[(name, rung)] = (w, corpus_targets(w))
    return out


def test_the_restated_grid_is_the_one_the_walk_families_were_built_for(worlds):
    for (name, rung), (w, _) in worlds.items():
        if name == "parts":
            continue        # (its bodies of several parts are beside the lattice: the walk families are laid over the ordinary bodies' grid)
        G = QC.world_grid(w)
        assert G["n_large"] == (2 if name == "wide" else 0), (name, rung, G)
        assert np.all(G["dims"] >= 2) and G["dims"].prod() <= 4096 + 4096, (name, rung, G)
        if name != "wide":
            assert G["dims"].max() >= 4, (name, rung, G)      # a walk worth the name


# Families the unfiltered comparison exposed as non-local besides the direction ladder: particles that start far from the bodies they pass.
# ray_sphere decides by the sign of b^2 - a c, which cancels for an origin far away - a body 50 off the line answers from 1e5 away
# (EXPERIMENTS.md, "rays from far away").  The answers stand as the definition's; test_far_hits_stay_within_the_tube bounds them.
NON_LOCAL = {"walk_far_origin", "walk_far_origin_unit_d", "walk_grazes_a_face_from_afar", "walk_far_origin_beside_the_grid", "walk_far_segment_ends_short_of_the_grid", "walk_enters_through_face", "walk_enters_through_edge", "walk_enters_through_corner",
             "walk_hit_in_last_cell", "walk_corner_diagonal"}


def test_filtered_and_unfiltered_references_agree_but_for_the_direction_ladder(worlds):
    """per family, the particles whose filtered answer (Targets._near in front of the oracle) differs from the unfiltered one.  Without the
    direction band the direction ladder differs; with the band of include/mgf_hip.h it no longer does.  The only other families that
    differ are NON_LOCAL's, with or without the band."""
    raw, banded, total, share = collections.Counter(), collections.Counter(), collections.Counter(), {}
    for (name, rung), (w, T) in worlds.items():
        p, d, dt = QC.world_particles(w)
        fam = w["families"]
        bad, full = ray_differences(T, p, d, dt, banded=False)
        for i in bad:
            raw[fam[i].split(":")[0]] += 1
        bad, full = ray_differences(T, p, d, dt, banded=True)
        for i in bad:
            banded[fam[i].split(":")[0]] += 1
        for f in fam:
            total[f.split(":")[0]] += 1
        share[(name, rung)] = np.mean([a is not None for a in full])
    print("\nfiltered vs unfiltered reference, particles that differ per family (without the band / with it / of):")
    for f in sorted(total):
        print(f"  {f:44s} {raw[f]:6d} {banded[f]:6d} {total[f]:7d}")
    print("share of particles that hit something, per world and rung:")
    for k, v in sorted(share.items()):
        print(f"  {k[0]:18s} rung {k[1]:2d}  {v:.2f}")
    assert raw["direction_ladder"] > 0 and banded["direction_ladder"] == 0
    assert {f for f, n in raw.items() if n} <= {"direction_ladder"} | NON_LOCAL, dict(raw)
    assert {f for f, n in banded.items() if n} <= NON_LOCAL, dict(banded)
    for k, v in share.items():
        assert 0.2 <= v <= 0.8, (k, v)


def test_the_families_aimed_at_the_walk_are_what_they_say(worlds):
    """equal t: two targets at the least t, bit for bit, for every particle of the family; beside the grid and short of it: the path misses
    the restated grid's box, and some of those particles hit a body all the same"""
    from oracle import oracle as O
    n_tie = n_beside = 0
    grazes = {}
    for (name, rung), (w, T) in worlds.items():
        p, d, dt = QC.world_particles(w)
        fam = w["families"]
        if "ties" in w:
            m = fam == "equal_t_at_two_bodies"
            hit, _, t = O.intersection_batch(p[m], d[m], dt[m], T._all_shapes(), every=True)
            t = np.where(hit == 1, t, np.inf)
            least = t.min(axis=1)
            assert m.sum() == 2 * QC.TIES and np.all(np.isfinite(least)) and np.all((t == least[:, None]).sum(axis=1) == 2), (name, rung)
            a, b = w["ties"]
            assert np.all((b - a) % 256 != 0) and (name != "mixed" or np.all(b // 64 != a // 64))      # other lanes; in `mixed` another wave
            n_tie += int(m.sum())
        if name == "parts":
            continue
        G = QC.world_grid(w)
        lo = G["lo"].astype(np.float64)
        hi = lo + G["dims"] * float(G["h"])
        for f in ("walk_far_origin_beside_the_grid", "walk_far_segment_ends_short_of_the_grid"):
            m = np.nonzero(fam == f)[0]
            assert len(m) >= 12, (name, rung, f)
            for i in m:     # the slab clip of the walk, in float64: no t in [0, dt] inside the box
                pp, dd = p[i].astype(np.float64), d[i].astype(np.float64)
                t0, t1 = 0.0, float(dt[i])
                for k in range(3):
                    if dd[k] == 0:
                        if not lo[k] <= pp[k] <= hi[k]:
                            t1 = -1.0
                    else:
                        ta, tb = sorted(((lo[k] - pp[k]) / dd[k], (hi[k] - pp[k]) / dd[k]))
                        t0, t1 = max(t0, ta), min(t1, tb)
                assert t0 > t1, (name, rung, f, i)
            n_beside += sum(a is not None and a[1] == 0 for a in T.raycast_all(p[m], d[m], dt[m], kinds=1))
        # grazing a face from afar: hits at points of the line outside the restated box, in every world at every rung
        m = np.nonzero(fam == "walk_grazes_a_face_from_afar")[0]
        hits = [a for a in T.raycast_all(p[m], d[m], dt[m], kinds=1) if a is not None]
        outside = [a for a in hits if np.any(np.asarray(a[4]) < lo) or np.any(np.asarray(a[4]) > hi)]
        grazes[(name, rung)] = (len(m), len(hits), len(outside))
        assert len(hits) >= 5, (name, rung, grazes[(name, rung)])
        # (a cell of the wide world is 400 wide: its grid's box dwarfs the lattice, no body lies at a face; and where the box's own pad,
        # twice the margin, is half a size or more - 1e5 from the origin - it exceeds what the tube allows from this far: no hit outside it)
        if name != "wide" and 2.0 * float(G["margin"]) < 0.5 * w["size"]:
            assert len(outside) >= 1, (name, rung, grazes[(name, rung)])
    print("\nwalk_grazes_a_face_from_afar (particles, hit a body, at a point outside the grid's box):", grazes)
    assert n_tie == 2 * 2 * QC.TIES * len(CC.WORLD_RUNGS) and n_beside > 50, (n_tie, n_beside)
    assert sum(v[2] for v in grazes.values()) > 100, grazes


def test_every_sweep_family_is_planted_at_some_rung():
    base = QC.sweep_base()
    want = set(np.array(CC.FAMILIES)[base["family"]].tolist())
    seen = set()
    for rung in CC.WORLD_RUNGS:
        seen |= set(QC.sweep_world(rung)["families"].tolist())
    assert want <= seen, sorted(want - seen)


def test_far_hits_stay_within_the_tube(worlds):
    """What bounds the non-local answers (mgf_amd/csrc/k_query.h, q_ray_tube): b^2 and a c each carry at most 8 roundings of 2^-24 relative
    to a |m|^2, so a sphere of radius r answers only if the particle's path passes its centre within sqrt(r^2 + 1e-6 |m|^2), m from the
    origin to the centre.  Held here for every sphere the unfiltered reference reports, in every world at every rung."""
    worst = 0.0
    for (name, rung), (w, T) in worlds.items():
        p, d, dt = QC.world_particles(w)
        for i, a in enumerate(T.raycast_all(p, d, dt)):
            if a is None or a[1] != 0:
                continue
            e = int(np.nonzero((T.owner == a[2]) & (T.part == a[3]))[0][0])
            if T.comps["tag"][e] != 0:
                continue
            c, r = T.comps["p"][e].astype(np.float64), float(T.comps["r"][e])
            pp, dd = p[i].astype(np.float64), d[i].astype(np.float64)
            m = c - pp
            s = np.clip((m @ dd) / (dd @ dd), 0.0, float(dt[i]))
            e2 = float(np.sum((m - s * dd) ** 2))
            if e2 > r * r:
                worst = max(worst, (e2 - r * r) / float(m @ m))
    print(f"\nlargest (e^2 - r^2) / |m|^2 of a reported sphere: {worst:.3g}")
    assert worst <= 1e-6


def test_filtered_and_unfiltered_sweeps_agree(worlds):
    from tests.test_gpu_world_sweeps import Sweeper, answer_all
    import mgf_amd
    diff, share = collections.Counter(), {}
    for rung in CC.WORLD_RUNGS:
        w = QC.sweep_world(rung)
        T = corpus_targets(w)
        casts = QC.world_casts(w, mgf_amd.MOVING_DTYPE)
        S = Sweeper(T)
        full = answer_all(T, casts)
        fam = w["families"]
        for i in range(len(casts)):
            if _key(S.answer(casts[i], kinds=3)) != _key(full[i]):
                diff[fam[i]] += 1
        share[rung] = np.mean([a is not None for a in full])
    print("\nfiltered vs unfiltered sweep reference, casts that differ per family:", dict(diff))
    print("share of casts that meet something, per rung:", {k: round(float(v), 2) for k, v in share.items()})
    assert not diff, dict(diff)
    for k, v in share.items():
        assert 0.2 <= v <= 0.8, (k, v)


def test_the_older_tests_reference_was_right_for_what_they_asked():
    """the generators of tests/test_gpu_world_queries.py and tests/test_gpu_world_sweeps.py (rays_at, the grazing and floor rays, casts_at) over
    their scenes as added: the filtered reference they use and the unfiltered one agree on every query"""
    import mgf_amd
    from mgf_amd import scenes
    from tests.test_gpu_world_queries import Targets, rays_at
    from tests.test_gpu_world_sweeps import Sweeper, answer_all, casts_at
    n_bad = 0
    for sc, seed in ((scenes.balls_demo(8), 1), (scenes.capsule_field(8, 2, 8, quads=12), 2)):
        comps = np.zeros(len(sc["comps"]), scenes.COMPONENT_DTYPE)
        for k in ("tag", "p", "d", "r"):
            comps[k] = sc["comps"][k]
        t = sc["terrain"]
        v = np.asarray(t["verts"], np.float32).reshape(-1, 3) + np.asarray(t["pos"], np.float32)
        T = Targets([[c] for c in comps], v[np.asarray(t["faces"], np.int64).reshape(-1, 3)])
        cen = (comps["p"] + 0.5 * comps["d"] * (comps["tag"] == 1)[:, None]).astype(np.float32)
        rng = np.random.default_rng(seed)
        p, d = rays_at(rng, cen, 96, 0.4)
        top = cen[rng.integers(0, len(cen), 48)] + np.array([0.0, 0.5, 0.0], np.float32)
        pg = (top + np.array([-15.0, 0.0, 0.0], np.float32)).astype(np.float32)
        dg = np.tile(np.array([1.0, 0.0, 0.0], np.float32), (48, 1))
        pf = np.stack([rng.uniform(-9, 9, 64), np.full(64, 30.0), rng.uniform(-9, 9, 64)], axis=1).astype(np.float32)
        df = np.tile(np.array([0.0, -1.0, 0.0], np.float32), (64, 1))
        P, D = np.concatenate([p, pg, pf]), np.concatenate([d, dg, df])
        bad, full = ray_differences(T, P, D, np.float32(np.inf))
        n_bad += len(bad)
        assert sum(a is not None for a in full) > 100
        casts = np.concatenate([casts_at(rng, cen, 48, 0.4, (0.05, 0.9)), casts_at(rng, cen, 48, 0.4, (4.0, 20.0)), casts_at(rng, cen, 24, 0.4, (0.0, 0.0))])
        S = Sweeper(T)
        full = answer_all(T, casts)
        n_bad += sum(_key(S.answer(casts[i], kinds=3)) != _key(full[i]) for i in range(len(casts)))
    assert n_bad == 0
