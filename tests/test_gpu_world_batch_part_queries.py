"""Rays, sweeps and box queries of a batch that see the parts of bodies of several components (mgf_batch_set_option "part_queries"):
every answer bit for bit against the lone mgf_world that has been through the same add calls and ticks, at tick 0 also against the
definition composed from the oracle's single-shape tests (Targets / Sweeper with parts=), whatever the mix of worlds in a call and the
lanes a query gets.  Counts a test requires are asserted on the reference's answers."""
import numpy as np
import pytest

import mgf_amd
from mgf_amd import _capi, scenes
from tests import batch_part_query_cases as QC
from tests import batch_parts_cases as PC
from tests.test_gpu_world_batch_query_device import _casts_dev, _cuda, _parts, _rays_dev, _sync
from tests.test_gpu_world_queries import compare_overlaps, compare_rays, rays_at, some_boxes, world_targets
from tests.test_gpu_world_sweeps import Sweeper, _cast, casts_at, compare_sweeps

pytestmark = pytest.mark.gpu
INF = float("inf")
f32 = np.float32
SEVERAL = (PC.DUMBBELLS, PC.JACKS, PC.MIXED, PC.ONE_JACK)


@pytest.fixture(scope="module")
def ctx():
    c = mgf_amd.Context(0)
    yield c
    c.close()


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _lone(ctx, sc):
    w = mgf_amd.World.from_scene(ctx, dict(sc, obstacles=None))
    for comps, disp, rot in (sc.get("obstacles") or ()):
        c = _capi.Compound(ctx, np.ascontiguousarray(comps, scenes.COMPONENT_DTYPE))
        c.set_pose(disp, rot)
        w.add_obstacle(c)
    return w


def _pair(ctx, scs, ticks, option=1):
    """the batch (option set), one lone world per scene stepped alike, and every world's x at tick 0"""
    b = mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True)
    if option is not None:
        b.set_option(QC.OPTION, option)
    lone = [_lone(ctx, sc) for sc in scs]
    x0 = [w.state()["x"].copy() if len(w) else np.zeros((0, 3), f32) for w in lone]
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    if ticks:
        b.step(dt, iters, ticks)
        for w in lone:
            if len(w):
                w.step_many(dt, iters, ticks)
    return b, lone, x0


def _points(scs, lone, x0):
    """per world the points to aim at (QC.aim_points); a world without bodies: one point above the floor"""
    return [QC.aim_points(sc, x0[k], lone[k].state()) if len(lone[k]) else np.array([[0.0, 2.0, 0.0]]) for k, sc in enumerate(scs)]


class Asked:
    """what compare_rays / compare_sweeps / compare_overlaps take for a world: world k's share of a call of the batch, already answered"""

    def __init__(self, b, k, answers=None):
        self.b, self.k, self.answers = b, k, answers

    def colliders(self):
        return self.b.colliders(self.k)

    def raycast(self, p, d, dt=INF, ignore=None, kinds=7):
        return self.answers if self.answers is not None else self.b.raycast(self.k, p, d, dt, ignore=ignore, kinds=kinds)

    def sweep(self, casts, delta=None, ignore=None, kinds=7):
        return self.answers if self.answers is not None else self.b.sweep(self.k, casts, delta, ignore=ignore, kinds=kinds)

    def overlap_aabb(self, lo, hi):
        return self.b.overlap_aabb(self.k, lo, hi)


def _targets(b, k, sc, obstacles=()):
    return world_targets(Asked(b, k), sc, parts=QC.compound_parts(sc) or None, obstacles=obstacles)


def _on_several(hits, sc):
    """the hits of a reference answer that lie on bodies of several components"""
    return hits[(hits["kind"] == 0) & np.isin(hits["index"], list(QC.compound_parts(sc)))]


@pytest.fixture(scope="module")
def six(ctx):
    """the six worlds at tick 0 and after 30 ticks: batch, lone worlds, aim points (tests 2, 6, 7, 9 and 10 share them)"""
    scs = PC.six_scenes()
    out = {}
    for ticks in (0, 30):
        b, lone, x0 = _pair(ctx, scs, ticks)
        out[ticks] = dict(scs=scs, b=b, lone=lone, pts=_points(scs, lone, x0))
    return out


# ---- 1: the option ----------------------------------------------------------------------------------------------------------------------
def test_option_values_and_default(ctx):
    scs = PC.six_scenes()
    plain = mgf_amd.WorldBatch.from_scenes(ctx, [scs[PC.PILE], scs[PC.PILE]])
    parts = mgf_amd.WorldBatch.from_scenes(ctx, [scs[PC.JACKS], scs[PC.PILE]], own_terrain=True)
    for bad in (2, -1):
        with pytest.raises(mgf_amd.MgfError) as e:
            plain.set_option(QC.OPTION, bad)
        assert e.value.status == _capi.ERR_INVALID
    rng = np.random.default_rng(31)
    cen = plain.colliders(0)["p"]
    p, d = rays_at(rng, cen, 40, 0.4)
    casts = casts_at(rng, cen, 40, 0.4, (0.0, 6.0))
    lo, hi = some_boxes(rng, cen, 20, 1.5)

    def answers(b):
        off, vals = b.overlap_aabb(1, lo, hi)
        return b.raycast(1, p, d).tobytes(), b.sweep(1, casts).tobytes(), off.tobytes(), vals.tobytes()
    before = answers(plain)
    plain.set_option(QC.OPTION, 1)
    assert answers(plain) == before          # no part storage: the option changes no launch
    plain.set_option(QC.OPTION, 0)
    # the default and an explicit 0: refused as before
    for setting in (None, 0):
        if setting is not None:
            parts.set_option(QC.OPTION, setting)
        for call in (lambda: parts.raycast(0, p, d), lambda: parts.sweep(1, casts), lambda: parts.overlap_aabb(0, lo, hi)):
            with pytest.raises(mgf_amd.MgfError) as e:
                call()
            assert e.value.status == _capi.ERR_INVALID and "several components" in str(e.value)
    parts.set_option(QC.OPTION, 1)
    assert len(parts.raycast(0, p, d)) == 40


# ---- 2: rays ----------------------------------------------------------------------------------------------------------------------------
def _six_rays(c, seed):
    rng = np.random.default_rng(seed)
    ws, ps, ds, igs = [], [], [], []
    for k, n in QC.COUNTS.items():
        p, d = rays_at(rng, c["pts"][k], n, 0.3)
        ws.append(np.full(n, k, np.int32)); ps.append(p); ds.append(d)
        nb = len(c["lone"][k])
        igs.append(np.where(np.arange(n) % 5 == 0, rng.integers(0, max(nb, 1), n) if nb else -1, -1).astype(np.int32))
    return QC.shuffled(rng, np.concatenate(ws), np.concatenate(ps), np.concatenate(ds), np.concatenate(igs))


@pytest.mark.parametrize("ticks", [0, 30])
def test_rays_all_six_worlds_in_one_call(six, ticks):
    c = six[ticks]
    b, lone, scs = c["b"], c["lone"], c["scs"]
    world, p, d, ign = _six_rays(c, 41 + ticks)
    got = b.raycast(world, p, d, INF, ignore=ign, kinds=7)
    for k, sc in enumerate(scs):
        sel = np.nonzero(world == k)[0]
        assert len(sel) == QC.COUNTS[k]
        want = lone[k].raycast(p[sel], d[sel], INF, ignore=ign[sel], kinds=7)
        assert same_bytes(got[sel], want), f"world {k} tick {ticks}: the lone world answers otherwise"
        if k in SEVERAL:
            on = _on_several(want, sc)
            assert len(on) > 32 and on["part"].max() > 0, (k, len(on))
        if ticks == 0:
            compare_rays(Asked(b, k, got[sel]), _targets(b, k, sc), p[sel], d[sel], INF, ignore=ign[sel], kinds=7)
    # 256 and 64 lanes a query over bodies of several components: one ray and three rays of every such world in calls of their own, the
    # rays those whose reference hit lies on a later part of such a body
    for k in SEVERAL:
        sel = np.nonzero(world == k)[0]
        want = lone[k].raycast(p[sel], d[sel], INF, ignore=ign[sel], kinds=7)
        q = sel[(want["kind"] == 0) & np.isin(want["index"], list(QC.compound_parts(scs[k]))) & (want["part"] > 0)][:3]
        assert len(q) == 3, (k, len(q))
        for m in (1, 3):
            assert same_bytes(b.raycast(k, p[q[:m]], d[q[:m]], INF, ignore=ign[q[:m]]), lone[k].raycast(p[q[:m]], d[q[:m]], INF, ignore=ign[q[:m]])), (k, m)
    # the other masks, every fourth ray, the worlds still mixed
    sub = np.arange(0, len(world), 4)
    for kinds in (1, 2, 3):
        g = b.raycast(world[sub], p[sub], d[sub], INF, ignore=ign[sub], kinds=kinds)
        for k in range(len(scs)):
            sel = np.nonzero(world[sub] == k)[0]
            q = sub[sel]
            if len(q):
                assert same_bytes(g[sel], lone[k].raycast(p[q], d[q], INF, ignore=ign[q], kinds=kinds)), (k, kinds)


# ---- 3: `part` across waves -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_plain", [80, 200])
def test_part_travels_across_waves(ctx, n_plain):
    """the dumbbells at body indices above 64 (above 192): with one query in a call - 256 lanes - their lanes sit in the second (the
    fourth) wave, and the hit crosses bq_reduce's exchange through LDS"""
    sc = scenes.dumbbell_field(3, 2, 3, n_plain=n_plain)
    b, (lone,), _ = _pair(ctx, [sc], 0)
    parts = QC.compound_parts(sc)
    assert min(parts) == n_plain and len(lone) == n_plain + 18 <= 218
    ray_second = cast_second = 0
    for i, rows in parts.items():
        c = QC.centres(rows)
        u = (c[1] - c[0]) / np.linalg.norm(c[1] - c[0])
        reach = float(rows["r"][1]) + 0.5 * float(np.linalg.norm(rows["d"][1])) * int(rows["tag"][1] == 1)
        p = (c[1] + u * (reach + 0.3)).astype(f32)[None]
        d = (-u).astype(f32)[None]
        want = lone.raycast(p, d)
        got = b.raycast(0, p, d)
        assert (got[0]["kind"], got[0]["index"], got[0]["part"]) == (want[0]["kind"], want[0]["index"], want[0]["part"]), (i, got, want)
        assert same_bytes(got, want)
        ray_second += int(want[0]["kind"] == 0 and want[0]["index"] == i and want[0]["part"] == 1)
        cast = _cast(0, (c[1] + u * (reach + 0.4)).astype(f32), (0, 0, 0), 0.1, (-u).astype(f32))
        want = lone.sweep(cast)
        got = b.sweep(0, cast)
        assert (got[0]["kind"], got[0]["index"], got[0]["part"]) == (want[0]["kind"], want[0]["index"], want[0]["part"]), (i, got, want)
        assert same_bytes(got, want)
        cast_second += int(want[0]["kind"] == 0 and want[0]["index"] == i and want[0]["part"] == 1)
    assert ray_second >= 9 and cast_second >= 9, (ray_second, cast_second)   # (the reference: the second part answers)


# ---- 4: ties ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 256])
def test_ties_between_parts_and_bodies(ctx, n):
    sc = QC.tie_scene()
    b = mgf_amd.WorldBatch.from_scenes(ctx, [sc])
    b.set_option(QC.OPTION, 1)
    lone = mgf_amd.World.from_scene(ctx, sc)
    p = np.tile(np.array([0, 5, 0], f32), (n, 1))
    d = np.tile(np.array([0, -1, 0], f32), (n, 1))
    cast = np.tile(_cast(0, (0, 4, 0), (0, 0, 0), 0.2, (0, -3, 0)), n)
    # all four parts report one t, to the bit: each alone in a lone world of its own answers the same
    single = []
    for k in range(4):
        one = np.zeros(1, scenes.COMPONENT_DTYPE)
        one[0] = sc["compound"]["comps"][k]
        w = mgf_amd.World(ctx)
        w.add_bodies(one, np.ones(1, f32), np.zeros(1, f32), np.full(1, 0.5, f32), np.zeros((1, 3), f32))
        single.append((w.raycast(p[:1], d[:1])[0]["t"].tobytes(), w.sweep(cast[:1])[0]["t"].tobytes()))
    assert len(set(single)) == 1
    for ignore, body in ((None, 0), (np.zeros(n, np.int32), 1)):
        for got, want in ((b.raycast(0, p, d, ignore=ignore), lone.raycast(p, d, ignore=ignore)), (b.sweep(0, cast, ignore=ignore), lone.sweep(cast, ignore=ignore))):
            assert same_bytes(got, want)
            assert np.all(want["kind"] == 0) and np.all(want["index"] == body) and np.all(want["part"] == 0), (ignore is None, want[0])


# ---- 5: ignore --------------------------------------------------------------------------------------------------------------------------
def test_an_ignored_body_is_skipped_with_every_part(six):
    c = six[0]
    b, lone, sc = c["b"], c["lone"][PC.JACKS], c["scs"][PC.JACKS]
    parts = QC.compound_parts(sc)
    idx = np.array(sorted(parts), np.int32)
    p = np.array([parts[i]["p"][0] for i in idx], f32)                        # inside the hub ...
    d = np.array([parts[i]["d"][1] for i in idx], f32)                        # ... and out along the first capsule
    assert np.all(np.array([parts[i]["tag"][1] for i in idx]) == 1)
    seen = lone.raycast(p, d, kinds=1)
    assert np.all((seen["kind"] == 0) & (seen["index"] == idx) & (seen["t"] == 0))   # not ignored: itself, at once
    want = lone.raycast(p, d, ignore=idx, kinds=7)
    got = b.raycast(np.full(len(idx), PC.JACKS, np.int32), p, d, ignore=idx, kinds=7)
    assert same_bytes(got, want)
    assert not np.any((want["kind"] == 0) & (want["index"] == idx))
    casts = np.concatenate([_cast(0, p[j], (0, 0, 0), 0.1, d[j]) for j in range(len(idx))])
    want = lone.sweep(casts, ignore=idx)
    assert same_bytes(b.sweep(np.full(len(idx), PC.JACKS, np.int32), casts, ignore=idx), want)
    assert not np.any((want["kind"] == 0) & (want["index"] == idx))


# ---- 6: sweeps --------------------------------------------------------------------------------------------------------------------------
def _six_casts(c, seed):
    rng = np.random.default_rng(seed)
    ws, cs = [], []
    for k, n in QC.COUNTS.items():
        cs.append(casts_at(rng, c["pts"][k], n, 0.3, (0.0, 5.0)))
        ws.append(np.full(n, k, np.int32))
    world, casts = np.concatenate(ws), np.concatenate(cs)
    perm = rng.permutation(len(world))
    return world[perm], casts[perm]


@pytest.mark.parametrize("ticks", [0, 30])
def test_sweeps_all_six_worlds_in_one_call(six, ticks):
    c = six[ticks]
    b, lone, scs = c["b"], c["lone"], c["scs"]
    world, casts = _six_casts(c, 51 + ticks)
    ign = np.where(np.arange(len(world)) % 7 == 0, 0, -1).astype(np.int32)
    got = b.sweep(world, casts, ignore=ign, kinds=7)
    for k, sc in enumerate(scs):
        sel = np.nonzero(world == k)[0]
        want = lone[k].sweep(casts[sel], ignore=ign[sel], kinds=7)
        assert same_bytes(got[sel], want), f"world {k} tick {ticks}: the lone world answers otherwise"
        if k in SEVERAL:
            on = _on_several(want, sc)
            assert len(on) > 32 and on["part"].max() > 0, (k, len(on))
        if ticks == 0:
            compare_sweeps(Asked(b, k, got[sel]), Sweeper(_targets(b, k, sc)), casts[sel], ignore=ign[sel], kinds=7)
    # 256 and 64 lanes a cast over bodies of several components (as for the rays)
    for k in SEVERAL:
        sel = np.nonzero(world == k)[0]
        want = lone[k].sweep(casts[sel], ignore=ign[sel], kinds=7)
        q = sel[(want["kind"] == 0) & np.isin(want["index"], list(QC.compound_parts(scs[k]))) & (want["part"] > 0)][:3]
        assert len(q) == 3, (k, len(q))
        for m in (1, 3):
            assert same_bytes(b.sweep(k, casts[q[:m]], ignore=ign[q[:m]]), lone[k].sweep(casts[q[:m]], ignore=ign[q[:m]])), (k, m)
    g = b.sweep(world[::4], casts[::4], kinds=1)
    for k in range(len(scs)):
        sel = np.nonzero(world[::4] == k)[0]
        if len(sel):
            assert same_bytes(g[sel], lone[k].sweep(casts[::4][sel], kinds=1)), k


@pytest.mark.parametrize("ticks", [0, 20])
def test_obstacle_worlds_rays_and_sweeps(ctx, ticks):
    """the face and obstacle passes behind the new body pass"""
    scs = PC.obstacle_scenes()
    b, lone, x0 = _pair(ctx, scs, ticks)
    pts = _points(scs, lone, x0)
    rng = np.random.default_rng(61 + ticks)
    ws, ps, ds, cs = [], [], [], []
    for k in range(len(scs)):
        p, d = rays_at(rng, pts[k], 60, 0.4)
        ws.append(np.full(60, k, np.int32)); ps.append(p); ds.append(d); cs.append(casts_at(rng, pts[k], 60, 0.4, (0.0, 6.0)))
    world, p, d, casts = QC.shuffled(rng, np.concatenate(ws), np.concatenate(ps), np.concatenate(ds), np.concatenate(cs))
    for kinds in (7, 5, 4):
        gr, gs = b.raycast(world, p, d, kinds=kinds), b.sweep(world, casts, kinds=kinds)
        seen = set()
        for k, sc in enumerate(scs):
            sel = np.nonzero(world == k)[0]
            wr, ws_ = lone[k].raycast(p[sel], d[sel], kinds=kinds), lone[k].sweep(casts[sel], kinds=kinds)
            assert same_bytes(gr[sel], wr) and same_bytes(gs[sel], ws_), (k, kinds)
            seen |= set(wr["kind"].tolist()) | set(ws_["kind"].tolist())
            if ticks == 0 and kinds == 7 and k == 2:
                T = _targets(b, k, sc, obstacles=sc["obstacles"])
                compare_rays(Asked(b, k, gr[sel]), T, p[sel], d[sel], INF, kinds=7)
                compare_sweeps(Asked(b, k, gs[sel]), Sweeper(T, sc["obstacles"]), casts[sel], kinds=7)
        if kinds == 7:
            assert {0, 2} <= seen, seen   # (the reference: bodies and obstacles both answer)


# ---- 7: the device forms ----------------------------------------------------------------------------------------------------------------
def test_device_forms_give_the_host_forms_bytes(six):
    c = six[30]
    b, scs = c["b"], c["scs"]
    world, p, d, ign = _six_rays(c, 71)
    parts = _parts(dict(p=p, d=d, dt=np.full(len(p), INF, f32)))
    assert same_bytes(_rays_dev(b, world, parts, ignore=ign), b.raycast(world, p, d, INF, ignore=ign))
    cw, casts = _six_casts(c, 72)
    assert same_bytes(_casts_dev(b, cw, casts), b.sweep(cw, casts))
    # the fixed layout: 70 queries a world, world by world
    rng = np.random.default_rng(73)
    per, K = 70, len(scs)
    fp, fd = (np.concatenate(a) for a in zip(*[rays_at(rng, c["pts"][k], per, 0.3) for k in range(K)]))
    fw = np.repeat(np.arange(K, dtype=np.int32), per)
    fparts = _parts(dict(p=fp, d=fd, dt=np.full(len(fp), INF, f32)))
    assert same_bytes(_rays_dev(b, None, fparts), b.raycast(fw, fp, fd))
    fc = np.concatenate([casts_at(rng, c["pts"][k], per, 0.3, (0.0, 5.0)) for k in range(K)])
    assert same_bytes(_casts_dev(b, None, fc), b.sweep(fw, fc))
    # a world index out of range: the no-hit record, counted
    skipped = b.counter("device_skipped")
    bad = world.copy()
    bad[:3] = (len(scs), -1, 1 << 20)
    got = _rays_dev(b, bad, parts, ignore=ign)
    none = np.zeros(3, got.dtype)
    none["kind"] = -1
    assert same_bytes(got[:3], none)
    assert same_bytes(got[3:], b.raycast(world[3:], p[3:], d[3:], INF, ignore=ign[3:]))
    assert b.counter("device_skipped") == skipped + 3


# ---- 8: the rigs ------------------------------------------------------------------------------------------------------------------------
def _rig_bodies(c):
    """(world, body) of six jacks, six dumbbells and two plain spheres of the dumbbell world"""
    jacks = sorted(QC.compound_parts(c["scs"][PC.JACKS]))[:6]
    bells = sorted(QC.compound_parts(c["scs"][PC.DUMBBELLS]))[:6]
    world = np.array([PC.JACKS] * 6 + [PC.DUMBBELLS] * 8, np.int32)
    body = np.array(jacks + bells + [0, 1], np.int32)
    return world, body


def test_sensors_answer_raycast_of_their_particles(six):
    import torch
    c = six[30]
    b = c["b"]
    world, body = _rig_bodies(c)
    rng = np.random.default_rng(81)
    n = 2 * len(world)
    w2, b2 = np.tile(world, 2), np.tile(body, 2)
    own = np.arange(n) < len(world)                       # every mount once with the self-ignore flag and once without
    p = rng.normal(0, 0.1, (n, 3)).astype(f32)            # from inside the body: without the flag it meets itself
    d = rng.normal(0, 1, (n, 3)).astype(f32)
    b.set_sensors(w2, b2, p, d, INF, ignore_self=own)
    try:
        hits, pt = b.cast_sensors(parts=True)
        ign = np.where(own, b2, -1).astype(np.int32)
        want = b.raycast(w2, pt["p"], pt["d"], pt["dt"], ignore=ign)
        assert same_bytes(hits, want)
        hub = ~own & (w2 == PC.JACKS)                      # (a jack's centre of mass lies in its hub)
        assert np.all((want[hub]["kind"] == 0) & (want[hub]["index"] == b2[hub]) & (want[hub]["t"] == 0))
        assert not np.any((want[own]["kind"] == 0) & (want[own]["index"] == b2[own]))
        out = torch.full((n, 7), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        pd = torch.zeros((n, 7), dtype=torch.float32, device="cuda")
        _sync()
        b.cast_sensors_dev(out, parts=pd)
        _sync()
        assert out.cpu().numpy().tobytes() == hits.tobytes() and pd.cpu().numpy().tobytes() == pt.tobytes()
    finally:
        b.set_sensors(np.zeros(0, _capi.SENSOR_DTYPE))


def test_feelers_answer_sweep_of_their_casts(six):
    import torch
    c = six[30]
    b = c["b"]
    world, body = _rig_bodies(c)
    rng = np.random.default_rng(82)
    m = len(world)
    n = 2 * m + 1
    w2, b2 = np.concatenate([world, world, [PC.JACKS]]).astype(np.int32), np.concatenate([body, body, body[:1]]).astype(np.int32)
    own = np.arange(n) != -1
    own[m:2 * m] = False                                  # every mount once with the self-ignore flag and once without
    shape = np.zeros(n, bool)
    shape[-1] = True                                      # the last: the first jack's own shape
    tag = (np.arange(n) % 2).astype(np.int32)
    p = rng.normal(0, 0.1, (n, 3)).astype(f32)
    d = np.where((tag == 1)[:, None], rng.normal(0, 0.4, (n, 3)), 0.0).astype(f32)
    delta = rng.normal(0, 1.5, (n, 3)).astype(f32)
    b.set_feelers(w2, b2, tag, p, d, np.full(n, 0.15, f32), delta, ignore_self=own, world_delta=np.arange(n) % 3 == 0, own_shape=shape)
    try:
        hits, casts = b.cast_feelers(casts=True)
        ign = np.where(own, b2, -1).astype(np.int32)
        want = b.sweep(w2, casts, ignore=ign)
        assert same_bytes(hits, want)
        hub = ~own & (w2 == PC.JACKS)                      # (a jack's centre of mass lies in its hub)
        assert np.all((want[hub]["kind"] == 0) & (want[hub]["index"] == b2[hub]) & (want[hub]["t"] == 0))
        assert not np.any((want[own]["kind"] == 0) & (want[own]["index"] == b2[own]))
        row = b.colliders(PC.JACKS)[body[0]]              # OWN_SHAPE on a jack: the collider row - a radius-0 sphere at the centre of mass
        assert (casts[-1]["tag"], casts[-1]["r"]) == (0, 0.0) == (row["tag"], row["r"]) and casts[-1]["p"].tobytes() == row["p"].tobytes()
        out = torch.full((n, 13), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        cd = torch.zeros((n, 11), dtype=torch.int32, device="cuda")
        _sync()
        b.cast_feelers_dev(out, casts=cd)
        _sync()
        assert out.cpu().numpy().tobytes() == hits.tobytes() and cd.cpu().numpy().tobytes() == casts.tobytes()
    finally:
        b.set_feelers(np.zeros(0, _capi.FEELER_DTYPE))


def test_feelers_of_own_shape_with_and_without_bodies_in_the_mask(six):
    """One world, a dumbbell and two plain spheres of it; each carries a feeler of its own shape and an ordinary one.  Under a mask of
    terrain only - no body is staged then - and under bodies and terrain, the hits are the lone world's sweep of the casts byte for
    byte, and an own shape is the collider row whatever the mask."""
    c = six[30]
    b, lone, k = c["b"], c["lone"][PC.DUMBBELLS], PC.DUMBBELLS
    bodies = np.array(sorted(QC.compound_parts(c["scs"][k]))[:1] + [0, 1], np.int32)
    n = 6
    body = np.repeat(bodies, 2)
    own = np.arange(n) % 2 == 0
    p = np.tile(f32([0.0, 1.6, 0.0]), (n, 1))
    delta = np.where(own[:, None], f32([0.6, -0.8, 0.3]), f32([0.0, -4.0, 0.0])).astype(f32)
    b.set_feelers(np.full(n, k, np.int32), body, np.zeros(n, np.int32), p, np.zeros((n, 3), f32), np.full(n, 0.1, f32), delta, ignore_self=own, world_delta=True,
                  own_shape=own)
    try:
        ign = np.where(own, body, -1).astype(np.int32)
        seen = {}
        for kinds in (2, 1 | 2):                                          # terrain; bodies and terrain
            hits, casts = b.cast_feelers(kinds, casts=True)
            assert same_bytes(hits, lone.sweep(casts, ignore=ign, kinds=kinds)), kinds
            seen[kinds] = (hits, casts)
        assert seen[2][1].tobytes() == seen[3][1].tobytes()               # the casts do not depend on the mask
        rows = b.colliders(k)[body[own]]
        for key in ("tag", "p", "d", "r"):
            assert seen[2][1][key][own].tobytes() == rows[key].tobytes(), key
        assert seen[2][1]["r"][0] == 0.0 and np.all(seen[2][1]["r"][own][1:] > 0)      # the dumbbell's row: a radius-0 sphere; the plain bodies' own
        assert set(seen[2][0]["kind"].tolist()) <= {-1, 1}
    finally:
        b.set_feelers(np.zeros(0, _capi.FEELER_DTYPE))


# ---- 9: boxes ---------------------------------------------------------------------------------------------------------------------------
def _end_boxes(sc):
    """boxes that meet only the outer half of a dumbbell's end sphere - not its centre of mass, not its collider row"""
    rows = []
    for i, ps in sorted(QC.compound_parts(sc).items())[:8]:
        cen = QC.centres(ps)
        u = (cen[0] - cen[1]) / np.linalg.norm(cen[0] - cen[1])      # from the capsule towards the sphere (part 0)
        rows.append(np.concatenate([cen[0] + u * float(ps["r"][0]) * 0.8, np.full(3, 0.05)]))
    return np.array(rows, f32)


def test_box_overlaps_use_the_union_of_the_part_bounds(six):
    for ticks in (0, 30):
        c = six[ticks]
        b, lone, scs = c["b"], c["lone"], c["scs"]
        rng = np.random.default_rng(91 + ticks)
        for k in (PC.DUMBBELLS, PC.JACKS, PC.MIXED, PC.PILE, PC.ONE_JACK):
            lo, hi = some_boxes(rng, c["pts"][k], 40, 1.5)
            off, vals = b.overlap_aabb(k, lo, hi)
            woff, wvals = lone[k].overlap_aabb(lo, hi)
            assert np.array_equal(off, woff) and np.array_equal(vals, wvals), (k, ticks)
            if ticks == 0:
                assert compare_overlaps(Asked(b, k), _targets(b, k, scs[k]), lo, hi) == len(wvals)
    c = six[0]
    b, sc = c["b"], c["scs"][PC.DUMBBELLS]
    boxes = _end_boxes(sc)
    woff, wvals = c["lone"][PC.DUMBBELLS].overlap_boxes(boxes)
    off, vals = b.overlap_boxes(PC.DUMBBELLS, boxes)
    assert np.array_equal(off, woff) and np.array_equal(vals, wvals)
    own = np.array(sorted(QC.compound_parts(sc))[:8])
    col = b.colliders(PC.DUMBBELLS)[own]["p"]
    assert np.all(np.any(np.abs(col - boxes[:, :3]) > boxes[:, 3:], axis=1))            # the collider row lies outside every box ...
    assert all(own[j] in wvals[woff[j]:woff[j + 1]] for j in range(len(own)))            # ... and the reference lists the body


def _lists(lone, boxes, ignore):
    """per box the lone world's list without the ignored body"""
    off, vals = lone.overlap_boxes(boxes)
    return [np.array([v for v in vals[off[i]:off[i + 1]] if v != ignore[i]], np.int64) for i in range(len(boxes))]


def _first(lists, k):
    out = np.full((len(lists), 1 + k), -1, np.int32)
    for i, li in enumerate(lists):
        out[i, 0] = len(li)
        out[i, 1:1 + min(k, len(li))] = li[:k]
    return out


def _nearest(lists, boxes, bx, k):
    """the zones' nearest-first record and distances from the lists: d2 = (e.x e.x + e.y e.y) + e.z e.z in f32, e from the body's box's centre"""
    out, d2 = np.full((len(lists), 1 + k), -1, np.int32), np.full((len(lists), k), np.inf, f32)
    for i, li in enumerate(lists):
        e = (bx[li, :3] - boxes[i, :3]).astype(f32)
        dd = ((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]).astype(f32) + e[:, 2] * e[:, 2]).astype(f32)
        order = sorted(range(len(li)), key=lambda j: (int(dd[j].view(np.uint32)), int(li[j])))[:k]
        out[i, 0] = len(li)
        out[i, 1:1 + len(order)] = li[order]
        d2[i, :len(order)] = dd[order]
    return out, d2


def test_zones_and_nearest_over_part_boxes(six):
    import torch
    c = six[0]
    b, scs, lone = c["b"], c["scs"], c["lone"]
    K, k = len(scs), 5
    world, body = _rig_bodies(c)
    n = len(world) + 2
    zw = np.concatenate([world, [PC.JACKS, PC.DUMBBELLS]]).astype(np.int32)
    zb = np.concatenate([body, [-1, -1]]).astype(np.int32)
    zp = np.zeros((n, 3), f32)
    zp[-2:] = (c["pts"][PC.JACKS][0], c["pts"][PC.DUMBBELLS][0])
    zr = np.full((n, 3), 2.4, f32)
    b.set_zones(zw, zb, zp, zr)
    try:
        cnt, first, boxes = b.read_zones(k, boxes=True)
        ign = np.where(zb >= 0, zb, -1)
        lists = [_lists(lone[w], boxes[i:i + 1], ign[i:i + 1])[0] for i, w in enumerate(zw)]
        bx = {w: _targets(b, w, scs[w]).boxes() for w in set(zw.tolist())}
        rec = np.concatenate([cnt[:, None], first], axis=1)
        assert np.array_equal(rec, _first(lists, k))
        want = _first(lists, k)                           # (the reference: lists longer than k, bodies of several components in them)
        assert want[:, 0].max() > k and sum(len(np.intersect1d(li, list(QC.compound_parts(scs[w])))) for li, w in zip(lists, zw)) > n
        out = torch.full((n, 1 + k), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        bd = torch.zeros((n, 6), dtype=torch.float32, device="cuda")
        _sync()
        b.read_zones_dev(out, boxes=bd)
        _sync()
        assert np.array_equal(out.cpu().numpy(), rec) and bd.cpu().numpy().tobytes() == boxes.tobytes()
        ncnt, near, d2 = b.read_zones_nearest(k, dist2=True)
        wrec = [_nearest([lists[i]], boxes[i:i + 1], bx[int(zw[i])], k) for i in range(n)]
        wn, wd = np.concatenate([r[0] for r in wrec]), np.concatenate([r[1] for r in wrec])
        assert np.array_equal(np.concatenate([ncnt[:, None], near], axis=1), wn) and d2.tobytes() == wd.tobytes()
        dd = torch.zeros((n, k), dtype=torch.float32, device="cuda")
        _sync()
        b.read_zones_nearest_dev(out, dist2=dd)
        _sync()
        assert np.array_equal(out.cpu().numpy(), wn) and dd.cpu().numpy().tobytes() == wd.tobytes()
    finally:
        b.set_zones(np.zeros(0, _capi.ZONE_DTYPE))
    # the caller's own boxes, the fixed layout: 12 a world, the dumbbell world's first eight the end boxes
    rng = np.random.default_rng(93)
    per = 12
    fb = np.zeros((K * per, 6), f32)
    for w in range(K):
        lo, hi = some_boxes(rng, c["pts"][w], per, 2.0)
        fb[w * per:(w + 1) * per] = np.concatenate([(hi + lo) / f32(2), (hi - lo) / f32(2)], axis=1)
    fb[PC.DUMBBELLS * per:PC.DUMBBELLS * per + 8] = _end_boxes(scs[PC.DUMBBELLS])
    fw = np.repeat(np.arange(K), per)
    fig = np.where(np.arange(K * per) % 3 == 0, 0, -1).astype(np.int32)
    lists = [_lists(lone[w], fb[i:i + 1], fig[i:i + 1])[0] if len(lone[w]) else np.zeros(0, np.int64) for i, w in enumerate(fw)]
    out = torch.full((K * per, 1 + k), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    dd = torch.zeros((K * per, k), dtype=torch.float32, device="cuda")
    boxes_d, ign_d = _cuda(fb), _cuda(fig)
    _sync()
    b.overlap_first_dev(boxes_d, out, ignore=ign_d)
    _sync()
    assert np.array_equal(out.cpu().numpy(), _first(lists, k))
    b.overlap_nearest_dev(boxes_d, out, dist2=dd, ignore=ign_d)
    _sync()
    bxs = [_targets(b, w, scs[w]).boxes() if len(lone[w]) else np.zeros((0, 6), f32) for w in range(K)]
    wrec = [_nearest([lists[i]], fb[i:i + 1], bxs[int(fw[i])], k) for i in range(K * per)]
    assert np.array_equal(out.cpu().numpy(), np.concatenate([r[0] for r in wrec]))
    assert dd.cpu().numpy().tobytes() == np.concatenate([r[1] for r in wrec]).tobytes()


# ---- 10: ordinary worlds in a parts batch -----------------------------------------------------------------------------------------------
def test_an_ordinary_world_answers_as_in_a_batch_without_parts(ctx, six):
    c = six[30]
    b, sc = c["b"], c["scs"][PC.PILE]
    plain = mgf_amd.WorldBatch.from_scenes(ctx, [sc], own_terrain=True)
    plain.step(float(sc["dt"]), sc["iters"], 30)
    rng = np.random.default_rng(101)
    cen = c["pts"][PC.PILE]
    p, d = rays_at(rng, cen, 120, 0.4)
    casts = casts_at(rng, cen, 120, 0.4, (0.0, 6.0))
    lo, hi = some_boxes(rng, cen, 40, 1.5)
    assert same_bytes(b.colliders(PC.PILE), plain.colliders(0))
    assert same_bytes(b.raycast(PC.PILE, p, d), plain.raycast(0, p, d)) and same_bytes(b.sweep(PC.PILE, casts), plain.sweep(0, casts))
    (o1, v1), (o2, v2) = b.overlap_aabb(PC.PILE, lo, hi), plain.overlap_aabb(0, lo, hi)
    assert np.array_equal(o1, o2) and np.array_equal(v1, v2) and len(v1) > 0


# ---- 11: layout changes -----------------------------------------------------------------------------------------------------------------
def test_copied_worlds_and_bodies_added_behind_ticks(ctx):
    import torch
    scs = PC.six_scenes()
    sc = scs[PC.JACKS]
    dt, iters, n = float(sc["dt"]), sc["iters"], PC.n_bodies(sc)
    pile = dict(scenes.sphere_pile(3, 2, 3, seed=4), terrain=sc["terrain"])
    assert len(pile["comps"]) == n
    b = mgf_amd.WorldBatch.from_scenes(ctx, [sc, pile, pile, pile], own_terrain=True)
    b.set_option(QC.OPTION, 1)
    lone = _lone(ctx, sc)
    x0 = lone.state()["x"].copy()
    b.step(dt, iters, 20)
    lone.step_many(dt, iters, 20)
    b.copy_worlds([1], None, [0])
    b.copy_worlds_where([2, 3], b, [0, 1], torch.tensor([1, 0], dtype=torch.int32, device="cuda"))   # world 3 stays the pile
    pts = QC.aim_points(sc, x0, lone.state())
    rng = np.random.default_rng(111)
    p, d = rays_at(rng, pts, 100, 0.3)
    casts = casts_at(rng, pts, 100, 0.3, (0.0, 5.0))
    lo, hi = some_boxes(rng, pts, 30, 1.5)
    wr, ws, (wo, wv) = lone.raycast(p, d), lone.sweep(casts), lone.overlap_aabb(lo, hi)
    assert len(_on_several(wr, sc)) > 32 and wr["part"].max() > 0
    for k in (0, 1, 2):
        assert same_bytes(b.raycast(k, p, d), wr) and same_bytes(b.sweep(k, casts), ws), k
        off, vals = b.overlap_aabb(k, lo, hi)
        assert np.array_equal(off, wo) and np.array_equal(vals, wv), k
    # dumbbells added behind the ticks, to the batch's world 1 and to the lone world alike: seen where they were added
    add = scenes.dumbbell_field(2, 1, 2)["compound"]
    add["comps"]["p"][:, 1] += f32(9.0)
    b.add_compound_bodies(1, add["comps"], add["comp_mass"], add["offsets"], add["restitution"], add["friction"], add["force"])
    lone.add_compound_bodies(add["comps"], add["comp_mass"], add["offsets"], add["restitution"], add["friction"], add["force"])
    tp = QC.centres(add["comps"])
    p2, d2 = rays_at(rng, tp, 60, 0.3)
    c2 = casts_at(rng, tp, 60, 0.3, (0.0, 4.0))
    for ticks in (0, 3):
        if ticks:
            b.step(dt, iters, ticks)
            lone.step_many(dt, iters, ticks)
        wr = lone.raycast(np.concatenate([p, p2]), np.concatenate([d, d2]))
        assert same_bytes(b.raycast(1, np.concatenate([p, p2]), np.concatenate([d, d2])), wr), ticks
        assert same_bytes(b.sweep(1, np.concatenate([casts, c2])), lone.sweep(np.concatenate([casts, c2]))), ticks
        if not ticks:
            assert np.sum((wr["kind"] == 0) & (wr["index"] >= n)) > 10


# ---- 12: neutrality ---------------------------------------------------------------------------------------------------------------------
def test_queries_change_nothing_and_cameras_stay_refused(ctx):
    scs = PC.six_scenes()[:2]
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    b, twin = (mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True) for _ in range(2))
    b.set_option(QC.OPTION, 1)
    rng = np.random.default_rng(121)
    for _ in range(3):
        b.step(dt, iters, 5)
        twin.step(dt, iters, 5)
        for k in range(2):
            cen = b.colliders(k)["p"]
            p, d = rays_at(rng, cen, 50, 0.5)
            b.raycast(k, p, d)
            b.sweep(k, casts_at(rng, cen, 50, 0.5, (0.0, 5.0)))
            b.overlap_aabb(k, *some_boxes(rng, cen, 20, 1.5))
    for k in range(2):
        PC.same_state(b.state(k), twin.state(k), f"world {k} behind the queries")
    b.set_cameras([dict(world=0, body=0, p=(0, 0, 0), tan_x=0.5, tan_y=0.5, width=2, height=2)])
    with pytest.raises(mgf_amd.MgfError) as e:
        b.cast_cameras()
    assert e.value.status == _capi.ERR_INVALID and "several components" in str(e.value)
