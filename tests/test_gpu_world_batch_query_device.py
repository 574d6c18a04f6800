"""The device-pointer ray casts and sweeps of a batch (mgf_batch_raycast_many_dev, mgf_batch_sweep_many_dev; WorldBatch.raycast_dev /
.sweep_dev) against the host-memory calls on the SAME batch at the same moment: every hit record equal byte for byte, by the caller's
index - whatever order the device's plan puts a world's queries in - the records the call must skip answered with the no-hit record and
counted, the launch counts as the header states them, and nothing of the tick's state touched.  No test hands these calls a host
pointer, a short buffer or overlapping arrays: those refusals are read in the source (tests/test_world_batch_query_device_host.py)."""
import os
import re

import numpy as np
import pytest

from tests import batch_query_cases as BQ
from tests import batch_query_device_cases as QD

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TICKS = QD.TICKS


@pytest.fixture(scope="module")
def ctx():
    import mgf_amd
    c = mgf_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def plan_launches():
    """the constant the header states"""
    import mgf_amd
    m = re.search(r"#define MGF_BATCH_DEV_QUERY_PLAN_LAUNCHES (\d+)", open(os.path.join(ROOT, "include", "mgf_hip.h")).read())
    assert m and int(m.group(1)) == mgf_amd._capi.BATCH_DEV_QUERY_PLAN_LAUNCHES
    return int(m.group(1))


def _scenes():
    return QD.pile_scenes()


def _pile_batch(ctx):
    import mgf_amd
    scs = _scenes()
    b = mgf_amd.WorldBatch.from_scenes(ctx, scs)
    b.step(float(scs[0]["dt"]), scs[0]["iters"], TICKS)
    return b


@pytest.fixture(scope="module")
def pile(ctx):
    """the five piles after 30 ticks, their rays (BQ.pile_rays) and casts, and the host-memory calls' answers under every mask used"""
    b = _pile_batch(ctx)
    K = b.n_worlds
    assert [len(b.colliders(k)) for k in range(K)] == list(QD.PILE_BODIES)
    cen = [b.colliders(k)["p"] for k in range(K)]
    rays = BQ.pile_rays(cen, BQ.COUNTS_T30)
    assert np.array_equal(rays["world"], QD.pile_world_array())      # (what the CPU model of the plan is run over)
    casts = _pile_casts(cen)
    want_r = {(m, ig): b.raycast(rays["world"], rays["p"], rays["d"], rays["dt"], ignore=rays["ignore"] if ig else None, kinds=m)
              for m in (7, 1, 2, 3) for ig in (True, False)}
    want_s = {(m, ig): b.sweep(casts["world"], casts["casts"], ignore=casts["ignore"] if ig else None, kinds=m) for m in (7, 4) for ig in (True, False)}
    # the inputs are not trivial: bodies, terrain, obstacles and nothing are all met
    assert set(want_r[7, True]["kind"].tolist()) == {-1, 0, 1, 2} and set(want_s[7, False]["kind"].tolist()) >= {0, 1, 2}
    assert set(want_s[4, False]["kind"].tolist()) == {-1, 2}
    return dict(b=b, K=K, rays=rays, casts=casts, want_r=want_r, want_s=want_s)


def _pile_casts(cen):
    """casts a world: none for world 2, two for the world without bodies, 257 across the cut of 256; every seventh does not move (a
    capsule among them: every face); those of the world without bodies come straight down onto its ring and onto the floor"""
    from tests.test_gpu_world_sweeps import casts_at
    rng = np.random.default_rng(41)
    cw, cc = [], []
    for k, c in enumerate((3, 64, 0, 4, 257)):
        if not c:
            continue
        cs = casts_at(rng, cen[k] if len(cen[k]) else cen[1], c, 0.5, (0.0, 6.0))
        cs["delta"][::7] = 0.0
        if k == QD.EMPTY_WORLD:
            cs = QD.empty_world_casts()
        cw.append(np.full(c, k, np.int32))
        cc.append(cs)
    cw, cc = np.concatenate(cw), np.concatenate(cc)
    perm = rng.permutation(len(cw))
    casts = dict(world=cw[perm], casts=cc[perm], ignore=np.where(np.arange(len(cw)) % 3 == 0, 0, -1).astype(np.int32))
    assert {0, 1} == set(casts["casts"]["tag"].tolist()) and np.any(np.all(casts["casts"]["delta"] == 0, axis=1) & (casts["casts"]["tag"] == 1))
    return casts


def _cuda(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _sync():
    import torch
    torch.cuda.synchronize()


def _parts(r):
    from mgf_amd._capi import _particle_rows
    return _particle_rows(r["p"], r["d"], r["dt"])


def _words(casts):
    """MOVING_DTYPE rows as 11 int32 words a row (word 0 the tag)"""
    return np.ascontiguousarray(casts).view(np.int32).reshape(len(casts), 11)


def _rays_dev(b, world, parts, ignore=None, kinds=7, fill=0x5A):
    """raycast_dev between two waits for the whole device (the tensors come from torch's stream, the library has its own); the hits as a
    RAY_HIT_DTYPE array.  `out` starts as 0x5A bytes: a record the call does not write shows."""
    import torch
    from mgf_amd._capi import RAY_HIT_DTYPE
    n = len(parts)
    out = torch.full((n, 7), fill * 0x01010101, dtype=torch.int32, device="cuda")
    w = None if world is None else _cuda(np.asarray(world, np.int32))
    ig = None if ignore is None else _cuda(np.asarray(ignore, np.int32))
    p = _cuda(parts) if n else torch.zeros((0, 7), dtype=torch.float32, device="cuda")
    _sync()
    b.raycast_dev(w, p, out, ignore=ig, kinds=kinds)
    _sync()
    return out.cpu().numpy().view(RAY_HIT_DTYPE).reshape(n)


def _casts_dev(b, world, casts, ignore=None, kinds=7, as_float=False):
    import torch
    from mgf_amd._capi import SWEEP_HIT_DTYPE
    n = len(casts)
    out = torch.full((n, 13), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    w = None if world is None else _cuda(np.asarray(world, np.int32))
    ig = None if ignore is None else _cuda(np.asarray(ignore, np.int32))
    c = _cuda(_words(casts))
    if as_float:
        c = c.view(torch.float32)       # the same bits as a float32 tensor: the binding takes either
    _sync()
    b.sweep_dev(w, c, out, ignore=ig, kinds=kinds)
    _sync()
    return out.cpu().numpy().view(SWEEP_HIT_DTYPE).reshape(n)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _passes(b, kinds, rays):
    """the passes of the host-memory call, as the header lists them for this batch (terrain under every world, obstacles in one)"""
    return 1 + (0 if rays or not kinds & 2 else 1) + (1 if kinds & 4 else 0)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
def test_rays_equal_raycast_with_the_worlds_interleaved(pile, plan_launches):
    b, rays = pile["b"], pile["rays"]
    parts = _parts(rays)
    assert len(parts) == sum(BQ.COUNTS_T30) and np.any(np.diff(rays["world"]) < 0)
    skipped = b.counter("device_skipped")
    for kinds in (7, 1, 2, 3):
        for ig in (True, False):
            got = _rays_dev(b, rays["world"], parts, rays["ignore"] if ig else None, kinds)
            assert b.counter("query_launches") == plan_launches + _passes(b, kinds, True), (kinds, ig)
            assert b.counter("query_run_ns") == 0
            assert _same(got, pile["want_r"][kinds, ig]), (kinds, ig, int(np.sum(got != pile["want_r"][kinds, ig])))
    assert b.counter("device_skipped") == skipped


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_order_within_a_world_is_free(pile):
    """the plan's order of a world's queries is whatever order the lanes' atomics came in: three runs of one call and one with the
    queries reversed give the same bytes by caller index (and world 2's 300 rays, world 4's 257 are cut into two work items each)"""
    b, rays, want = pile["b"], pile["rays"], pile["want_r"][7, True]
    parts = _parts(rays)
    for _ in range(3):
        assert _same(_rays_dev(b, rays["world"], parts, rays["ignore"]), want)
    r = slice(None, None, -1)
    assert _same(_rays_dev(b, rays["world"][r], parts[r], rays["ignore"][r])[r], want)
    c = pile["casts"]
    for _ in range(2):
        assert _same(_casts_dev(b, c["world"], c["casts"], c["ignore"]), pile["want_s"][7, True])
    assert _same(_casts_dev(b, c["world"][r], c["casts"][r], c["ignore"][r])[r], pile["want_s"][7, True])


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_sweeps_equal_sweep_through_bodies_faces_and_obstacles(pile, plan_launches):
    b, c = pile["b"], pile["casts"]
    assert [b.world_obstacle_count(k) for k in range(pile["K"])] == [0, 1, 0, 1, 0]
    for kinds in (7, 4):
        for ig in (True, False):
            got = _casts_dev(b, c["world"], c["casts"], c["ignore"] if ig else None, kinds, as_float=ig)
            assert b.counter("query_launches") == plan_launches + _passes(b, kinds, False), (kinds, ig)
            assert _same(got, pile["want_s"][kinds, ig]), (kinds, ig, int(np.sum(got != pile["want_s"][kinds, ig])))
    still = np.all(c["casts"]["delta"] == 0, axis=1)
    got = pile["want_s"][7, False]
    assert np.any(got["kind"][still] >= 0) and np.any(got["kind"][~still] >= 0)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def test_skipped_records(ctx, pile):
    from mgf_amd._capi import RAY_HIT_DTYPE, SWEEP_HIT_DTYPE
    K, rays, c = pile["K"], pile["rays"], pile["casts"]
    b, twin = _pile_batch(ctx), _pile_batch(ctx)     # (the twin makes no query; b is stepped on below, so it is not the shared batch)
    want_r = b.raycast(rays["world"], rays["p"], rays["d"], rays["dt"], ignore=rays["ignore"])
    want_s = b.sweep(c["world"], c["casts"], ignore=c["ignore"])
    assert _same(want_r, pile["want_r"][7, True]) and _same(want_s, pile["want_s"][7, True])
    bad = QD.bad_worlds(K)
    assert bad.tolist() == [-1, K, -(1 << 31), (1 << 31) - 1]
    # rays: the four bad worlds among the valid records, each with an origin and an ignore entry that would otherwise hit
    parts = _parts(rays)
    at = QD.skip_positions(len(parts), len(bad))
    mixed, keep = QD.spread(dict(world=rays["world"], parts=parts, ignore=rays["ignore"]), dict(world=bad, parts=parts[:1], ignore=np.int32([0])), at)
    assert not keep[0] and not keep[-1] and np.array_equal(mixed["world"][~keep], bad)
    before = b.counter("device_skipped")
    got = _rays_dev(b, mixed["world"], mixed["parts"], mixed["ignore"])
    none_r = np.zeros(len(bad), RAY_HIT_DTYPE)
    none_r["kind"] = -1
    assert _same(got[~keep], none_r)
    assert _same(got[keep], want_r)
    assert b.counter("device_skipped") == before + len(bad)
    # casts: the same four, and tags 2 and -1 in valid worlds
    tagged = c["casts"][:2].copy()
    tagged["tag"] = [2, -1]
    fill = dict(world=np.concatenate([bad, np.int32([1, 4])]), casts=np.concatenate([c["casts"][:4], tagged]), ignore=np.full(6, -1, np.int32))
    at = QD.skip_positions(len(c["world"]), 6, seed=78)
    mixed, keep = QD.spread(dict(world=c["world"], casts=c["casts"], ignore=c["ignore"]), fill, at)
    assert sorted(mixed["casts"]["tag"][~keep].tolist())[0] == -1 and 2 in mixed["casts"]["tag"][~keep]
    got = _casts_dev(b, mixed["world"], mixed["casts"], mixed["ignore"])
    none_s = np.zeros(6, SWEEP_HIT_DTYPE)
    none_s["kind"] = -1
    assert _same(got[~keep], none_s)
    assert _same(got[keep], want_s)
    assert b.counter("device_skipped") == before + len(bad) + 6
    # the fixed layout has no plan to look at the tags: the body pass skips them itself
    per = 3
    fixed = c["casts"][:per * K].copy()
    fixed["tag"][[1, per * K - 1]] = [2, -1]
    valid = np.ones(per * K, bool)
    valid[[1, per * K - 1]] = False
    world = np.repeat(np.arange(K, dtype=np.int32), per)
    got = _casts_dev(b, None, fixed)
    assert _same(got[~valid], none_s[:2]) and _same(got[valid], b.sweep(world[valid], fixed[valid]))
    assert b.counter("device_skipped") == before + len(bad) + 6 + 2
    # nothing of the tick's state was written: the batch steps on like a twin that made no query
    scs = _scenes()
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    b.step(dt, iters, 3)
    twin.step(dt, iters, 3)
    sa, sb = b.state(), twin.state()
    for f in sa:
        assert sa[f].tobytes() == sb[f].tobytes(), f
    for k in range(K):
        assert b.constraints(k).tobytes() == twin.constraints(k).tobytes(), k
    assert b.colliders().tobytes() == twin.colliders().tobytes()


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_fixed_layout_needs_no_plan(ctx):
    import mgf_amd
    from tests.test_gpu_world_sweeps import casts_at
    b = _pile_batch(ctx)
    K = b.n_worlds
    cen = np.concatenate([b.colliders(k)["p"] for k in range(K)])
    rng = np.random.default_rng(51)
    for r in (1, 64, 257):
        n = K * r
        world = np.repeat(np.arange(K, dtype=np.int32), r)
        tgt = cen[rng.integers(0, len(cen), n)] + rng.normal(0, 0.3, (n, 3))
        p = (tgt + rng.normal(0, 2.0, (n, 3)) + (0.0, 22.0, 0.0)).astype(np.float32)
        parts = _parts(dict(p=p, d=(tgt - p).astype(np.float32), dt=np.float32(np.inf)))
        ign = rng.integers(-1, 3, n).astype(np.int32)
        want = b.raycast(world, parts[:, 0:3], parts[:, 3:6], parts[:, 6], ignore=ign)
        host_launches = b.counter("query_launches")
        got = _rays_dev(b, None, parts, ign)
        assert _same(got, want), r
        assert set(want["kind"].tolist()) >= {0, 1}
        assert b.counter("query_launches") == host_launches == _passes(b, 7, True)      # the passes alone: no plan launches
    casts = casts_at(rng, cen, K * 64, 0.5, (0.0, 6.0))
    world = np.repeat(np.arange(K, dtype=np.int32), 64)
    want = b.sweep(world, casts)
    host_launches = b.counter("query_launches")
    assert _same(_casts_dev(b, None, casts), want) and np.any(want["kind"] >= 0)
    assert b.counter("query_launches") == host_launches == _passes(b, 7, False)
    # n that is no multiple of n_worlds: the binding says so, and so does the library (asked directly: nothing is enqueued)
    import torch
    lib, INV = mgf_amd.load_library(), mgf_amd._capi.ERR_INVALID
    for fn, call, cols, words in ((lib.mgf_batch_raycast_many_dev, b.raycast_dev, 7, 7), (lib.mgf_batch_sweep_many_dev, b.sweep_dev, 11, 13)):
        q = torch.zeros((K + 1, cols), dtype=torch.float32, device="cuda")
        out = torch.zeros((K + 1, words), dtype=torch.int32, device="cuda")
        _sync()
        with pytest.raises(ValueError, match="multiple"):
            call(None, q, out)
        assert fn(b._h, None, q.data_ptr(), K + 1, None, 7, out.data_ptr()) == INV and "multiple" in lib.mgf_last_error().decode()
        assert fn(b._h, None, q.data_ptr(), K, None, 7, out.data_ptr()) == 0
        _sync()


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_more_worlds_than_a_block_of_plan_lanes(ctx, plan_launches):
    import mgf_amd
    from mgf_amd import scenes
    sc = dict(scenes.sphere_pile(1, 1, 1), terrain=None)
    b = mgf_amd.WorldBatch.from_scenes(ctx, [sc] * QD.MANY)
    one_each, all_last = QD.many_world_arrays()
    c = b.colliders(0)["p"][0]
    rng = np.random.default_rng(61)
    p = (c + rng.normal(0, 0.2, (QD.MANY, 3)) + (0.0, 5.0, 0.0)).astype(np.float32)
    d = np.tile(np.float32([0.0, -1.0, 0.0]), (QD.MANY, 1))
    parts = _parts(dict(p=p, d=d, dt=np.float32(np.inf)))
    for world in (one_each, all_last):
        want = b.raycast(world, p, d, kinds=1)
        got = _rays_dev(b, world, parts, kinds=1)
        assert _same(got, want)
        assert {-1, 0} == set(want["kind"].tolist())
        # test 1's number under this mask: neither n nor the number of worlds changes it
        assert b.counter("query_launches") == plan_launches + _passes(b, 1, True)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------
def test_edges(ctx, plan_launches):
    import torch
    import mgf_amd
    from mgf_amd import scenes
    sc = scenes.sphere_pile(2, 2, 2)
    b = mgf_amd.WorldBatch.from_scenes(ctx, [sc, sc])
    dt, iters = float(sc["dt"]), sc["iters"]
    # n = 0: OK, nothing launched - before any tick, with the batch still in its host mirror
    assert len(_rays_dev(b, np.zeros(0, np.int32), np.zeros((0, 7), np.float32))) == 0 and b.counter("query_launches") == 0
    empty = torch.zeros((0, 13), dtype=torch.int32, device="cuda")
    b.sweep_dev(None, torch.zeros((0, 11), dtype=torch.float32, device="cuda"), empty)
    assert b.counter("query_launches") == 0
    # n = 1, before any tick: the collider a query sees is the component the body was added as; nothing to gather
    c = sc["comps"]["p"]
    one = _parts(dict(p=(c[3] + np.float32([0, 5, 0]))[None], d=np.float32([[0, -1, 0]]), dt=np.float32(np.inf)))
    got = _rays_dev(b, np.int32([1]), one)
    assert _same(got, b.raycast(1, one[:, 0:3], one[:, 3:6])) and got["kind"][0] == 0
    assert _same(_rays_dev(b, np.int32([1]), one, kinds=1), got)
    assert b.counter("query_launches") == plan_launches + 1
    # straight behind set_velocities_dev and a step, nothing waited for in between: the library's stream orders them
    total = len(b)
    lin = _cuda(np.tile(np.float32([0.5, 2.0, -0.25]), (total, 1)))
    ang = _cuda(np.zeros((total, 3), np.float32))
    n = 2 * len(c)
    world = np.repeat(np.arange(2, dtype=np.int32), len(c))
    parts = _parts(dict(p=np.concatenate([c, c]) + np.float32([0.05, 6.0, 0.0]), d=np.tile(np.float32([0, -1, 0]), (n, 1)), dt=np.float32(np.inf)))
    d_world, d_parts = _cuda(world), _cuda(parts)
    out1, out2 = (torch.full((n, 7), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for _ in range(2))
    _sync()
    b.set_velocities_dev(None, lin, ang)
    b.step(dt, iters, 2)
    b.raycast_dev(d_world, d_parts, out1, kinds=1)
    first = b.counter("query_launches")
    b.raycast_dev(d_world, d_parts, out2, kinds=1)
    second = b.counter("query_launches")
    ctx.synchronize()
    _sync()
    assert (first, second) == (1 + plan_launches + 1, plan_launches + 1)      # the collider gather once, behind the step
    want = b.raycast(world, parts[:, 0:3], parts[:, 3:6], kinds=1)
    from mgf_amd._capi import RAY_HIT_DTYPE
    for o in (out1, out2):
        assert _same(o.cpu().numpy().view(RAY_HIT_DTYPE).reshape(n), want)
    assert np.all(want["kind"] == 0) and not np.array_equal(b.colliders(0)["p"], c)   # the bodies have moved: these are the tick's colliders
    assert b.counter("device_skipped") == 0
