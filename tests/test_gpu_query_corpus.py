"""The query corpus (tests/query_corpus.py) through every query front, bit for bit against the UNFILTERED oracle: every target of a world
put through the oracle's single test and ranked by the definition (Targets.raycast_all, answer_all) - not the bounding-sphere filter of
the older query tests, which drops what the kernels' rejects drop.

  the pair-level ray corpus through the single-shot intersection entry (mgf_intersections_batch);
  at each rung of WORLD_RUNGS the corpus's worlds - spheres, mixed over a small mesh and over a face grid, with obstacles, with bodies of 2
  and 4 parts, with bodies on the grid's large list - through mgf_world_raycast_many, before a tick and after two, under the kinds masks
  1, 2, 4 and 7 and with `ignore` set to the body that would answer; the sweep world through mgf_world_sweep_many;
  the same worlds as one batch (own_terrain) through mgf_batch_raycast_many / mgf_batch_sweep_many, with part_queries off and on, the
  _dev form once, at every number of lanes a query can get: the oracle's answers, and the lone world's records byte for byte.

tests/test_query_corpus.py measures on the CPU what this corpus reaches."""
import numpy as np
import pytest

import mgf_amd
from tests import contact_corpus as CC
from tests import query_corpus as QC
from tests.test_gpu_world_queries import world_targets
from tests.test_gpu_world_sweeps import answer_all
from tests.test_query_corpus import corpus_obstacles, corpus_parts

pytestmark = pytest.mark.gpu
DT, ITERS = 1.0 / 60.0, 4


@pytest.fixture(scope="module")
def ctx():
    c = mgf_amd.Context(0)
    yield c
    c.close()


# ---- the single-shot entry ---------------------------------------------------------------------------------------------------------------
def _shape_dicts(sh):
    out = []
    for k, v in zip(sh["kind"], sh["v"]):
        if k == QC.SPHERE:
            out.append(dict(kind="sphere", c=v[:3], r=v[3]))
        elif k == QC.CAPSULE:
            out.append(dict(kind="capsule", a=v[:3], d=v[3:6], r=v[6]))
        else:
            out.append(dict(kind="triangle", a=v[:3], b=v[3:6], c=v[6:9]))
    return out


def test_the_pair_level_ray_corpus_through_the_single_shot_entry(ctx):
    """the whole corpus, 119 000 particles: every family, every rung, the direction ladder (the single test has no band: whatever the oracle
    answers, NaN and inf included, is the expectation)"""
    c = QC.ray_families()
    names = QC.family_names(c)
    hit, ip, t = QC.oracle_answers(c)
    parts = np.zeros(len(c), mgf_amd.PARTICLE_DTYPE)
    parts["p"], parts["d"], parts["dt"] = QC.origin(c), c["vb"], c["dt"]
    got = mgf_amd.intersections(ctx, parts, shapes=_shape_dicts(c["a"]))
    ghit = np.array([g is not None for g in got])
    names = QC.family_names(c)
    bad = np.nonzero(ghit != (hit == 1))[0]
    assert len(bad) == 0, (len(bad), names[bad[0]], c[bad[0]], got[bad[0]], (ip[bad[0]], t[bad[0]]))
    gp = np.array([g[0] if g is not None else (0, 0, 0) for g in got], np.float32)
    gt = np.array([g[1] if g is not None else 0 for g in got], np.float32)
    same = ((gt == t) | (np.isnan(gt) & np.isnan(t))) & np.all((gp == ip) | (np.isnan(gp) & np.isnan(ip)), axis=1)
    bad = np.nonzero(~same)[0]
    assert len(bad) == 0, (len(bad), names[bad[0]], c[bad[0]], got[bad[0]], (ip[bad[0]], t[bad[0]]))
    assert ghit.sum() > len(c) // 5


# ---- the worlds ------------------------------------------------------------------------------------------------------------------------------
def as_scene(w):
    """a corpus world as mgf_amd.scenes makes scenes (World.from_scene, WorldBatch.from_scenes): bodies at rest, no force"""
    sc = dict(comps=w["comps"], mass=1.0, restitution=0.3, friction=0.6, force=(0.0, 0.0, 0.0), terrain=w["mesh"], dt=DT, iters=ITERS,
              obstacles=corpus_obstacles(w), compound=None)
    if w["compound"] is not None:
        sc["compound"] = dict(comps=w["compound"]["comps"], comp_mass=1.0, offsets=w["compound"]["offsets"], restitution=0.3, friction=0.6, force=(0.0, 0.0, 0.0))
    return sc


def lone_world(ctx, w):
    sc = as_scene(w)
    gw = mgf_amd.World.from_scene(ctx, sc)
    gw._keep = []
    for comps, disp, rot in sc["obstacles"]:
        k = mgf_amd.Compound(ctx, comps)
        k.set_pose(disp, rot)
        gw.add_obstacle(k)
        gw._keep.append(k)
    return gw, sc


def ray_records(want):
    """the definition's answers as RAY_HIT_DTYPE records (a miss: all zero but kind -1); an obstacle's component is not the oracle's to say"""
    out = np.zeros(len(want), mgf_amd.RAY_HIT_DTYPE)
    out["kind"] = -1
    for i, a in enumerate(want):
        if a is not None:
            t, kind, index, part, ip = a
            out[i]["kind"], out[i]["index"], out[i]["part"], out[i]["p"], out[i]["t"] = kind, index, 0 if part is None else part, ip, t
    return out


def same_rays(got, want, what, fam):
    want = ray_records(want)
    g = got.copy()
    g["part"][g["kind"] == 2] = 0
    bad = np.nonzero([a.tobytes() != b.tobytes() for a, b in zip(g, want)])[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} particles differ from the unfiltered oracle, by family {sorted(set(fam[bad]))}; first {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"


def sweep_records(want):
    out = np.zeros(len(want), mgf_amd.SWEEP_HIT_DTYPE)
    out["kind"] = -1
    for i, a in enumerate(want):
        if a is not None:
            t, kind, index, part, _, c = a
            out[i]["kind"], out[i]["index"], out[i]["part"] = kind, index, part
            for k in ("a", "b", "n", "t"):
                out[i][k] = c[k]
    return out


def same_sweeps(got, want, what, fam):
    want = sweep_records(want)
    bad = np.nonzero([a.tobytes() != b.tobytes() for a, b in zip(got, want)])[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} casts differ from the unfiltered oracle, by family {sorted(set(fam[bad]))}; first {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"


def would_answer(want):
    """per particle the body that answers (-1: none does): what `ignore` is set to"""
    return np.array([a[2] if a is not None and a[1] == 0 else -1 for a in want], np.int32)


_worlds = {}


def corpus_world(name, rung):
    if (name, rung) not in _worlds:
        if len(_worlds) > 8:
            _worlds.clear()
        _worlds[(name, rung)] = QC.sweep_world(rung) if name == "sweeps" else QC.ray_world(name, rung)
    return _worlds[(name, rung)]


@pytest.mark.parametrize("rung", CC.WORLD_RUNGS)
@pytest.mark.parametrize("name", QC.WORLDS)
def test_the_corpus_through_the_lone_world(ctx, name, rung):
    w = corpus_world(name, rung)
    gw, sc = lone_world(ctx, w)
    p, d, dt = QC.world_particles(w)
    fam = w["families"]
    parts = corpus_parts(w) or None
    for ticks in (0, 2):
        if ticks:
            gw.step_many(DT, ITERS, ticks)
            if parts:
                break       # (the world-space parts of a stepped body are not read back: the batch test holds the stepped world to the lone one)
        T = world_targets(gw, sc, parts=parts, obstacles=sc["obstacles"])
        what = f"{name} rung {rung} after {ticks} ticks"
        want = T.raycast_all(p, d, dt)
        same_rays(gw.raycast(p, d, dt), want, what, fam)
        if ticks == 0 and name != "parts":
            G = QC.world_grid(w)
            assert gw.counter("query_large_bodies") == G["n_large"] and gw.counter("query_cells") == int(G["dims"].prod()), (what, G)
        for kinds in (1, 2, 4):
            same_rays(gw.raycast(p, d, dt, kinds=kinds), T.raycast_all(p, d, dt, kinds=kinds), f"{what}, kinds {kinds}", fam)
        ign = would_answer(want)
        assert np.sum(ign >= 0) > len(ign) // 10
        same_rays(gw.raycast(p, d, dt, ignore=ign), T.raycast_all(p, d, dt, ignore=ign), f"{what}, ignoring the body that answers", fam)
        if ticks == 0 and "ties" in w:      # equal t at two bodies: the lower index, whichever cell, lane or wave finds the other first
            g = gw.raycast(p, d, dt)[fam == "equal_t_at_two_bodies"]
            assert np.all(g["kind"] == 0) and np.array_equal(g["index"], np.tile(w["ties"][0], 2)), g
        # the world's casts: every mask, and the body that would answer ignored
        casts, cfam = QC.world_casts(w, mgf_amd.MOVING_DTYPE), w["cast_families"]
        cwant = answer_all(T, casts, kinds=7, obstacles=sc["obstacles"])
        same_sweeps(gw.sweep(casts), cwant, what, cfam)
        for kinds in (1, 2, 4):
            same_sweeps(gw.sweep(casts, kinds=kinds), answer_all(T, casts, kinds=kinds, obstacles=sc["obstacles"]), f"{what}, kinds {kinds}", cfam)
        cign = would_answer(cwant)
        same_sweeps(gw.sweep(casts, ignore=cign), answer_all(T, casts, ignore=cign, kinds=7, obstacles=sc["obstacles"]), f"{what}, ignoring the body that answers", cfam)
        if ticks == 0:
            met = np.mean([a is not None for a in cwant])
            assert 0.2 <= met <= 0.8, (name, rung, met)
            if name == "wide":
                assert any(a is not None and a[1] == 0 and a[2] == len(w["comps"]) - 2 for a in cwant)      # a body of the large list answers
            if name == "obstacle":
                assert any(a is not None and a[1] == 2 for a in cwant)
            if parts:
                assert any(a is not None and a[1] == 0 and a[3] > 0 for a in cwant)
    hits = np.mean([a is not None for a in want])
    assert 0.2 <= hits <= 0.8, (name, rung, hits)


@pytest.mark.parametrize("rung", CC.WORLD_RUNGS)
def test_the_sweep_corpus_through_the_lone_world(ctx, rung):
    w = corpus_world("sweeps", rung)
    gw, sc = lone_world(ctx, w)
    casts = QC.world_casts(w, mgf_amd.MOVING_DTYPE)
    fam = w["families"]
    for ticks in (0, 2):
        if ticks:
            gw.step_many(DT, ITERS, ticks)
        T = world_targets(gw, sc)
        what = f"sweeps rung {rung} after {ticks} ticks"
        want = answer_all(T, casts)
        same_sweeps(gw.sweep(casts), want, what, fam)
        for kinds in (1, 2, 7):
            same_sweeps(gw.sweep(casts, kinds=kinds), answer_all(T, casts, kinds=kinds), f"{what}, kinds {kinds}", fam)
        ign = would_answer(want)
        same_sweeps(gw.sweep(casts, ignore=ign), answer_all(T, casts, ignore=ign), f"{what}, ignoring the body that answers", fam)
    hits = np.mean([a is not None for a in want])
    assert 0.2 <= hits <= 0.8, (rung, hits)


# ---- the same worlds as one batch -------------------------------------------------------------------------------------------------------------
def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


LANE_COUNTS = (1, 2, 3, 6, 12, 24, 48, 100, 200)      # particles of one world in a call: 256, 128, 64, .. 1 lanes each (test_gpu_world_batch_queries.py)


@pytest.mark.parametrize("rung", CC.WORLD_RUNGS)
def test_the_corpus_through_the_batch(ctx, rung):
    """the worlds without bodies of several parts as one batch with a terrain of its own per world: every particle and cast of the corpus in
    one call, the worlds mixed - the unfiltered oracle's answers and the lone world's bytes; then after two ticks; the _dev form once"""
    names = [n for n in QC.WORLDS if n != "parts"] + ["sweeps"]
    ws = [corpus_world(n, rung) for n in names]
    scs = [as_scene(w) for w in ws]
    b = mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True)
    lone = [lone_world(ctx, w)[0] for w in ws]
    rays = [QC.world_particles(w) for w in ws[:-1]]
    world = np.concatenate([np.full(len(r[0]), k, np.int32) for k, r in enumerate(rays)])
    p, d, dt = (np.concatenate([r[j] for r in rays]) for j in range(3))
    casts = QC.world_casts(ws[-1], mgf_amd.MOVING_DTYPE)
    mix = np.random.default_rng(rung).permutation(len(world))      # the worlds mixed within the call
    world, p, d, dt = world[mix], p[mix], d[mix], dt[mix]
    for ticks in (0, 2):
        if ticks:
            b.step(DT, ITERS, ticks)
            for gw in lone:
                gw.step_many(DT, ITERS, ticks)
        got = b.raycast(world, p, d, dt)
        for k, (w, sc) in enumerate(zip(ws[:-1], scs)):
            sel = np.nonzero(world == k)[0]
            assert same_bytes(b.colliders(k), lone[k].colliders()), (names[k], rung, ticks)
            assert same_bytes(got[sel], lone[k].raycast(p[sel], d[sel], dt[sel])), f"{names[k]} rung {rung} after {ticks} ticks: the lone world answers otherwise"
            T = world_targets(lone[k], sc, obstacles=sc["obstacles"])
            same_rays(got[sel], T.raycast_all(p[sel], d[sel], dt[sel]), f"batch, {names[k]} rung {rung} after {ticks} ticks", w["families"][mix[sel] - sum(len(r[0]) for r in rays[:k])])
            # under a mask and with the body that answers ignored; the world's casts under every mask
            ign = np.where(got[sel]["kind"] == 0, got[sel]["index"], -1).astype(np.int32)
            for kinds in (1, 6):
                assert same_bytes(b.raycast(k, p[sel], d[sel], dt[sel], ignore=ign, kinds=kinds), lone[k].raycast(p[sel], d[sel], dt[sel], ignore=ign, kinds=kinds)), (names[k], rung, ticks, kinds)
            same_rays(b.raycast(k, p[sel], d[sel], dt[sel], ignore=ign), T.raycast_all(p[sel], d[sel], dt[sel], ignore=ign), f"batch, {names[k]} rung {rung} after {ticks} ticks, ignoring", w["families"][mix[sel] - sum(len(r[0]) for r in rays[:k])])
            wc = QC.world_casts(w, mgf_amd.MOVING_DTYPE)
            for kinds in (7, 1, 2, 4):
                gc = b.sweep(k, wc, kinds=kinds)
                assert same_bytes(gc, lone[k].sweep(wc, kinds=kinds)), (names[k], rung, ticks, kinds)
                if kinds == 7:
                    same_sweeps(gc, answer_all(T, wc, kinds=7, obstacles=sc["obstacles"]), f"batch, {names[k]} rung {rung} after {ticks} ticks", w["cast_families"])
        ks = len(ws) - 1
        gs = b.sweep(ks, casts)
        assert same_bytes(gs, lone[ks].sweep(casts)), f"sweeps rung {rung} after {ticks} ticks: the lone world answers otherwise"
        same_sweeps(gs, answer_all(world_targets(lone[ks], scs[ks]), casts), f"batch, sweeps rung {rung} after {ticks} ticks", ws[-1]["families"])
    # the device-pointer forms once: the same records
    from tests.test_gpu_world_batch_query_device import _casts_dev, _parts, _rays_dev
    assert same_bytes(_rays_dev(b, world, _parts(dict(p=p, d=d, dt=dt))), got)
    assert same_bytes(_casts_dev(b, np.full(len(casts), ks, np.int32), casts), gs)
    # every number of lanes a query can get, over the families in order (a slice of each world's particles), against the lone world
    for k in range(len(rays)):
        pk, dk, tk = rays[k]
        tie = np.nonzero(ws[k]["families"] == "equal_t_at_two_bodies")[0]      # (the first particle of every count is one with a tie, where the world has them)
        at = int(tie[0]) if len(tie) else 0
        for count in LANE_COUNTS:
            sl = (np.arange(count) * 7 + at) % len(pk)
            at += 1 if len(tie) else 13
            assert same_bytes(b.raycast(k, pk[sl], dk[sl], tk[sl]), lone[k].raycast(pk[sl], dk[sl], tk[sl])), (names[k], rung, count)
            cs = casts[(np.arange(count) * 3 + at) % len(casts)]
            assert same_bytes(b.sweep(ks, cs), lone[ks].sweep(cs)), (rung, count)


@pytest.mark.parametrize("rung", CC.WORLD_RUNGS)
def test_bodies_of_several_parts_in_a_batch(ctx, rung):
    """the world with bodies of 2 and 4 parts beside a world without, part_queries on: the oracle before a tick, the lone world's bytes before
    and after two ticks; the ordinary world answers the same with part_queries off and on"""
    ws = [corpus_world("parts", rung), corpus_world("mixed", rung)]
    scs = [as_scene(w) for w in ws]
    b = mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True)
    plain = mgf_amd.WorldBatch.from_scenes(ctx, scs[1:], own_terrain=True)
    lone = [lone_world(ctx, w)[0] for w in ws]
    b.set_option("part_queries", 1)
    for ticks in (0, 2):
        if ticks:
            b.step(DT, ITERS, ticks)
            plain.step(DT, ITERS, ticks)
            for gw in lone:
                gw.step_many(DT, ITERS, ticks)
        for k, w in enumerate(ws):
            p, d, dt = QC.world_particles(w)
            got = b.raycast(k, p, d, dt)
            assert same_bytes(got, lone[k].raycast(p, d, dt)), f"{w['name']} rung {rung} after {ticks} ticks: the lone world answers otherwise"
            if ticks == 0:
                T = world_targets(lone[k], scs[k], parts=corpus_parts(w) or None, obstacles=scs[k]["obstacles"])
                same_rays(got, T.raycast_all(p, d, dt), f"batch with part queries, {w['name']} rung {rung}", w["families"])
                if k == 0:
                    assert np.any((got["kind"] == 0) & (got["part"] > 0))
            wc = QC.world_casts(w, mgf_amd.MOVING_DTYPE)
            gc = b.sweep(k, wc)
            assert same_bytes(gc, lone[k].sweep(wc)), f"{w['name']} rung {rung} after {ticks} ticks: the lone world sweeps otherwise"
            if ticks == 0:
                same_sweeps(gc, answer_all(T, wc, kinds=7, obstacles=scs[k]["obstacles"]), f"batch with part queries, {w['name']} rung {rung}", w["cast_families"])
                if k == 0:
                    assert np.any((gc["kind"] == 0) & (gc["part"] > 0))
            if k == 1:
                assert same_bytes(got, plain.raycast(0, p, d, dt)), f"rung {rung} after {ticks} ticks: part_queries changes an ordinary world's answers"
                assert same_bytes(gc, plain.sweep(0, wc)), f"rung {rung} after {ticks} ticks: part_queries changes an ordinary world's sweeps"
