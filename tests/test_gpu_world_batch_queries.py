"""Ray casts and sweeps against the worlds of a batch (mgf_batch_raycast_many, mgf_batch_sweep_many, mgf_batch_read_colliders): every answer
against the definition composed from the oracle's single-shape tests (Targets / Sweeper of the lone world's query tests) and, bit for bit,
against the lone mgf_world that holds the same bodies and has been through the same calls - whatever the mix of worlds in a call, the
order of the queries and the number of lanes a query gets."""
import numpy as np
import pytest

import mgf_amd
from mgf_amd import scenes
from oracle import oracle as O
from tests import batch_query_cases as BQ
from tests.test_gpu_world_queries import Targets, compare_rays, world_targets
from tests.test_gpu_world_sweeps import Sweeper, _cast, _shape, casts_at, compare_sweeps
from tests.util import bits_equal, compare_constraints

pytestmark = pytest.mark.gpu
INF = float("inf")
STATE = ("x", "q", "v", "omega", "delta")


@pytest.fixture(scope="module")
def ctx():
    c = mgf_amd.Context(0)
    yield c
    c.close()


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class Asked:
    """what compare_rays / compare_sweeps take for a world: one world of a batch, answering with its share of a call that mixed the worlds"""

    def __init__(self, b, k, answers=None):
        self.b, self.k, self.answers = b, k, answers

    def colliders(self):
        return self.b.colliders(self.k)

    def raycast(self, p, d, dt=INF, ignore=None, kinds=7):
        if self.answers is not None:
            assert len(self.answers) == len(p)
            return self.answers
        return self.b.raycast(self.k, p, d, dt, ignore=ignore, kinds=kinds)

    def sweep(self, casts, delta=None, ignore=None, kinds=7):
        if self.answers is not None:
            assert len(self.answers) == len(casts)
            return self.answers
        return self.b.sweep(self.k, casts, delta, ignore=ignore, kinds=kinds)


def _pair(ctx, scs, ticks):
    """the batch and one lone world per scene, stepped alike"""
    b = mgf_amd.WorldBatch.from_scenes(ctx, scs)
    lone = [mgf_amd.World.from_scene(ctx, sc) for sc in scs]
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    if ticks:
        b.step(dt, iters, ticks)
        for w in lone:
            if len(w):
                w.step_many(dt, iters, ticks)
    return b, lone


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def piles(ctx):
    """test 1's batches, lone worlds, rays and answers at tick 0 and after 30 ticks (tests 1 and 5 share them)"""
    scs = BQ.pile_scenes()
    out = {}
    for ticks, counts in ((0, BQ.COUNTS_T0), (30, BQ.COUNTS_T30)):
        b, lone = _pair(ctx, scs, ticks)
        rays = BQ.pile_rays([b.colliders(k)["p"] for k in range(len(scs))], counts)
        got = b.raycast(rays["world"], rays["p"], rays["d"], rays["dt"], ignore=rays["ignore"], kinds=7)
        out[ticks] = dict(scs=scs, b=b, lone=lone, rays=rays, got=got)
    return out


@pytest.mark.parametrize("ticks", [0, 30])
def test_piles_rays_every_split(piles, ticks):
    c = piles[ticks]
    scs, b, lone, rays, got = c["scs"], c["b"], c["lone"], c["rays"], c["got"]
    assert len(got) == sum(BQ.COUNTS_T30 if ticks else BQ.COUNTS_T0)
    aimed = body = 0
    for k, sc in enumerate(scs):
        sel = np.nonzero(rays["world"] == k)[0]
        if len(sel) == 0:
            continue
        assert same_bytes(b.colliders(k), lone[k].colliders()), f"world {k}: colliders"
        T = world_targets(Asked(b, k), sc)
        p, d, dt, ign = rays["p"][sel], rays["d"][sel], rays["dt"][sel], rays["ignore"][sel]
        compare_rays(Asked(b, k, got[sel]), T, p, d, dt, ignore=ign, kinds=7)
        assert same_bytes(got[sel], lone[k].raycast(p, d, dt, ignore=ign, kinds=7)), f"world {k}: the lone world answers otherwise"
        kinds = set(got[sel]["kind"].tolist())
        if len(sc["comps"]):
            assert kinds == {-1, 0, 1}, (k, kinds)
        aimed += len(sel)
        body += int(np.sum(got[sel]["kind"] == 0))
        # every fourth ray again under each of the other masks, the worlds still mixed
    assert 2 * body > aimed, (body, aimed)
    sub = np.arange(0, len(got), 4)
    for kinds in (1, 2, 3):
        g = b.raycast(rays["world"][sub], rays["p"][sub], rays["d"][sub], rays["dt"][sub], ignore=rays["ignore"][sub], kinds=kinds)
        for k, sc in enumerate(scs):
            sel = np.nonzero(rays["world"][sub] == k)[0]
            if len(sel) == 0:
                continue
            q = sub[sel]
            compare_rays(Asked(b, k, g[sel]), world_targets(Asked(b, k), sc), rays["p"][q], rays["d"][q], rays["dt"][q], ignore=rays["ignore"][q], kinds=kinds)
            assert same_bytes(g[sel], lone[k].raycast(rays["p"][q], rays["d"][q], rays["dt"][q], ignore=rays["ignore"][q], kinds=kinds))


def test_every_number_of_lanes_a_query_can_get(piles):
    """1, 2, 3, 6, 12, 24, 48, 100 and 200 particles for one world: 256, 128, 64, .. 1 lanes each - against the lone world"""
    c = piles[30]
    b, lone = c["b"], c["lone"]
    rng = np.random.default_rng(4)
    for k in (1, 4):
        cen = b.colliders(k)["p"]
        for count in (1, 2, 3, 6, 12, 24, 48, 100, 200):
            tgt = cen[rng.integers(0, len(cen), count)] + rng.normal(0, 0.2, (count, 3))
            p = (tgt + rng.normal(0, 2.0, (count, 3)) + (0.0, 24.0, 0.0)).astype(np.float32)
            d = (tgt - p).astype(np.float32)
            got = b.raycast(k, p, d)
            assert same_bytes(got, lone[k].raycast(p, d)), (k, count)
            assert np.sum(got["kind"] == 0) * 2 >= count
            casts = casts_at(rng, cen, count, 0.4, (0.0, 6.0))
            assert same_bytes(b.sweep(k, casts), lone[k].sweep(casts)), (k, count)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def test_capsules_over_a_heightfield_rays_and_sweeps(ctx):
    a, c = scenes.capsule_field(4, 3, 4), scenes.capsule_field(8, 4, 8, sphere_fraction=0.5)
    assert (len(a["comps"]), len(c["comps"])) == (48, 256)
    scs = [a, dict(c, terrain=a["terrain"])]
    b, lone = _pair(ctx, scs, 40)
    rng = np.random.default_rng(21)
    T = [world_targets(Asked(b, k), scs[k]) for k in range(2)]
    S = [Sweeper(t) for t in T]
    cen = []
    for k in range(2):
        col = b.colliders(k)
        assert same_bytes(col, lone[k].colliders())
        cen.append(col["p"] + 0.5 * col["d"] * (col["tag"] == 1)[:, None])
    # rays, the worlds interleaved
    n = 96
    world = rng.integers(0, 2, n).astype(np.int32)
    tgt = np.array([cen[w][rng.integers(0, len(cen[w]))] for w in world]) + rng.normal(0, 0.5, (n, 3))
    p = (tgt + rng.normal(0, 1.0, (n, 3)) + (0.0, 8.0, 0.0)).astype(np.float32)
    d = (tgt - p).astype(np.float32)
    got = b.raycast(world, p, d)
    for k in range(2):
        sel = world == k
        compare_rays(Asked(b, k, got[sel]), T[k], p[sel], d[sel], INF)
        assert same_bytes(got[sel], lone[k].raycast(p[sel], d[sel]))
    assert {0, 1} <= set(got["kind"].tolist())
    # the three cases with a branch of their own, in both worlds: a capsule that does not move (every face), a sphere that does not move
    # and starts inside a body, a capsule laid parallel to a face and swept down onto it (two contacts)
    tri = T[0].faces

    def parallel(f):
        fa, fb, fc = tri[f].astype(np.float64)
        nrm = np.cross(fb - fa, fc - fa)
        nrm /= np.linalg.norm(nrm)
        nrm *= np.sign(nrm[1])
        edge = (fb - fa) * 0.3
        return _cast(1, (fa + fb + fc) / 3.0 - 0.5 * edge + nrm * 1.0, edge, 0.25, -nrm * 2.0)

    def special(k, n_par):
        return np.concatenate([_cast(1, cen[k][0] + (0.0, 3.0, 0.0), (0.4, 0.1, 0.0), 0.3, (0, 0, 0)),
                               _cast(0, cen[k][1] + (0.05, 0.02, 0.0), (0, 0, 0), 0.3, (0, 0, 0))]
                              + [parallel(f) for f in np.linspace(0, len(tri) - 1, n_par).astype(int)])
    seen_two = False
    kinds_seen, t_zero, t_pos = set(), False, False
    for count in (1, 5, 257):
        lead = {1: 0, 5: 2, 257: 10}[count]   # the constructed casts in front of the random ones
        casts = [np.concatenate(([special(k, lead - 2)] if lead else []) + [casts_at(rng, cen[k], count - lead, 0.6, (0.0, 6.0))]) for k in range(2)]
        world = np.repeat(np.arange(2, dtype=np.int32), count)
        allc = np.concatenate(casts)
        perm = rng.permutation(len(allc))
        got = b.sweep(world[perm], allc[perm])
        back = np.empty_like(got)
        back[perm] = got
        for k in range(2):
            g = back[k * count:(k + 1) * count]
            _, _, wants = compare_sweeps(Asked(b, k, g), S[k], casts[k])
            assert same_bytes(g, lone[k].sweep(casts[k])), (k, count)
            kinds_seen |= set(g["kind"].tolist())
            hit = g["kind"] >= 0
            t_zero |= bool(np.any(hit & (g["t"] == 0)))
            t_pos |= bool(np.any(hit & (g["t"] > 0) & (g["t"] <= 1)))
            if lead:
                assert np.all(casts[k][0]["delta"] == 0) and casts[k][0]["tag"] == 1   # the capsule that does not move: every face
                assert g[1]["kind"] == 0 and g[1]["t"] == 0.0                            # the sphere that starts inside a body
            for i in range(2, lead):
                w = wants[i]
                if w is not None and w[1] == 1:
                    res = O.contacts(O.shape(O.TRIANGLE, *T[k].faces[w[2]]), None, _shape(1, casts[k][i]["p"], casts[k][i]["d"], casts[k][i]["r"]), casts[k][i]["delta"])
                    seen_two |= len(res) == 2
    assert seen_two and {0, 1} <= kinds_seen and t_zero and t_pos, (seen_two, kinds_seen, t_zero, t_pos)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_collider_a_query_sees(ctx):
    sc = scenes.capsule_field(3, 2, 3)
    scs = [sc, dict(scenes.capsule_field(2, 2, 2, seed=9), terrain=sc["terrain"])]
    b, lone = _pair(ctx, scs, 0)
    dt, iters = float(sc["dt"]), sc["iters"]
    rng = np.random.default_rng(31)
    cen0 = sc["comps"]["p"] + 0.5 * sc["comps"]["d"]
    tgt = cen0[rng.integers(0, len(cen0), 24)] + rng.normal(0, 0.3, (24, 3))
    p = (tgt + (0.0, 6.0, 0.0) + rng.normal(0, 1.0, (24, 3))).astype(np.float32)
    d = (tgt - p).astype(np.float32)
    casts = casts_at(rng, cen0, 16, 0.5, (0.0, 5.0))

    def agree(what):
        for k in range(2):
            assert same_bytes(b.colliders(k), lone[k].colliders()), f"{what}: colliders of world {k}"
            assert same_bytes(b.raycast(k, p, d), lone[k].raycast(p, d)), f"{what}: rays in world {k}"
            assert same_bytes(b.sweep(k, casts), lone[k].sweep(casts)), f"{what}: casts in world {k}"
        whole = b.colliders()
        assert same_bytes(whole, np.concatenate([b.colliders(0), b.colliders(1)])), what

    def step(n):
        b.step(dt, iters, n)
        for w in lone:
            w.step_many(dt, iters, n)
    agree("before any tick")
    given = b.colliders(0)
    assert all(np.array_equal(given[f], sc["comps"][f]) for f in ("tag", "p", "d", "r")) and not np.any(given["delta"])
    step(3)
    agree("after 3 ticks")
    ticked = b.colliders(0).copy()
    assert not np.array_equal(ticked["p"], sc["comps"]["p"])
    # bodies added behind a tick: the mirror comes down and goes up again
    extra = scenes.capsule_field(2, 1, 2, seed=3)
    new = extra["comps"].copy()
    new["p"] += np.float32([0.0, 6.0, 0.0])
    b.add_bodies(0, new, extra["mass"], extra["restitution"], extra["friction"], extra["force"])
    lone[0].add_bodies(new, extra["mass"], extra["restitution"], extra["friction"], extra["force"])
    agree("after add_bodies")
    col = b.colliders(0)
    assert same_bytes(col[:len(ticked)], ticked) and np.array_equal(col["p"][len(ticked):], new["p"]) and np.array_equal(col["d"][len(ticked):], new["d"])
    # write_state does not move a collider ...
    st = b.state(0)
    x2 = (st["x"] + np.float32([0.25, 0.5, 0.0])).astype(np.float32)
    b.write_state(0, x=x2)
    lone[0].write_state(x=x2)
    agree("after write_state")
    assert same_bytes(b.colliders(0), col)
    # ... the next tick does
    step(1)
    agree("after the next tick")
    assert not np.array_equal(b.colliders(0)["p"][:len(ticked)], ticked["p"])


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def test_ties_across_lanes_and_waves(ctx):
    """300 spheres in a row, never stepped; bodies 7 and 200 identical and coincident.  One query: 256 lanes over the bodies, body 7 on
    lane 7 of wave 0 and body 200 on lane 8 of wave 3 - the two answers meet in the reduction across waves."""
    sc = scenes.sphere_pile(5, 12, 5)
    assert len(sc["comps"]) == 300
    comps = sc["comps"].copy()
    comps["p"] = np.stack([3.0 * np.arange(300), np.full(300, 5.0), np.zeros(300)], axis=1).astype(np.float32)
    comps[200] = comps[7]
    b = mgf_amd.WorldBatch.from_scenes(ctx, [dict(sc, comps=comps, v0=None, terrain=None)])
    c = comps[7]["p"]
    for sign in (1.0, -1.0):
        p = np.float32([c + np.float32([0.0, 0.0, 10.0 * sign])])
        d = np.float32([[0.0, 0.0, -sign]])
        g = b.raycast(0, p, d)[0]
        assert (g["kind"], g["index"], g["t"]) == (0, 7, np.float32(9.5)), g
        g2 = b.raycast(0, p, d, ignore=7)[0]
        assert (g2["kind"], g2["index"]) == (0, 200) and g2["t"] == g["t"] and np.array_equal(g2["p"], g["p"]), g2
        assert b.raycast(0, p, d, ignore=200)[0]["index"] == 7
        cast = _cast(0, p[0], (0, 0, 0), 0.25, 20.0 * d[0])
        s = b.sweep(0, cast)[0]
        assert (s["kind"], s["index"]) == (0, 7) and 0 < s["t"] < 1, s
        s2 = b.sweep(0, cast, ignore=7)[0]
        assert (s2["kind"], s2["index"]) == (0, 200) and s2["t"] == s["t"] and np.array_equal(s2["a"], s["a"]), s2


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_an_answer_depends_on_its_query_and_its_world_only(ctx, piles):
    c = piles[30]
    scs, b, rays, got = c["scs"], c["b"], c["rays"], c["got"]
    pick = np.arange(0, len(got), 9)
    for i in pick:   # alone
        one = b.raycast(rays["world"][i:i + 1], rays["p"][i:i + 1], rays["d"][i:i + 1], rays["dt"][i:i + 1], ignore=rays["ignore"][i:i + 1])
        assert same_bytes(one[0:1], got[i:i + 1]), i
    r = slice(None, None, -1)   # the whole set in reversed order
    assert same_bytes(b.raycast(rays["world"][r], rays["p"][r], rays["d"][r], rays["dt"][r], ignore=rays["ignore"][r])[r], got)
    # the same worlds in a batch built in reverse order
    K = len(scs)
    rb = mgf_amd.WorldBatch.from_scenes(ctx, scs[::-1])
    rb.step(float(scs[0]["dt"]), scs[0]["iters"], 30)
    assert same_bytes(rb.raycast(K - 1 - rays["world"], rays["p"], rays["d"], rays["dt"], ignore=rays["ignore"]), got)
    casts = np.concatenate([casts_at(np.random.default_rng(5), b.colliders(k)["p"], 20, 0.4, (0.0, 5.0)) for k in (1, 2, 4)])
    world = np.repeat(np.int32([1, 2, 4]), 20)
    want = b.sweep(world, casts)
    assert np.any(want["kind"] == 0)
    assert same_bytes(rb.sweep(K - 1 - world, casts), want)
    assert same_bytes(b.sweep(world[r], casts[r])[r], want)
    for i in range(0, 60, 7):
        assert same_bytes(b.sweep(world[i:i + 1], casts[i:i + 1]), want[i:i + 1])


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_tick_is_untouched(ctx):
    scs = [scenes.sphere_pile(4, 6, 4, seed=5), scenes.capsule_field(3, 2, 3)]
    scs[1] = dict(scs[1], terrain=scs[0]["terrain"])
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    a, b = mgf_amd.WorldBatch.from_scenes(ctx, scs), mgf_amd.WorldBatch.from_scenes(ctx, scs)
    rng = np.random.default_rng(6)
    p = rng.uniform(-3, 3, (40, 3)).astype(np.float32) + np.float32([0, 8, 0])
    d = np.tile(np.float32([0.1, -1.0, 0.05]), (40, 1))
    world = rng.integers(0, 2, 40).astype(np.int32)
    casts = casts_at(rng, scs[0]["comps"]["p"], 40, 0.5, (0.0, 4.0))
    hits = 0
    for _ in range(20):
        a.step(dt, iters)
        b.step(dt, iters)
        hits += int(np.sum(b.raycast(world, p, d)["kind"] >= 0)) + int(np.sum(b.sweep(world, casts)["kind"] >= 0))
        b.colliders()
    assert hits > 0
    assert a.counter("launches_per_tick") == b.counter("launches_per_tick") == 6
    for k in range(2):
        sa, sb = a.state(k), b.state(k)
        for f in STATE:
            assert bits_equal(sa[f], sb[f]), (k, f)
        compare_constraints(a.constraints(k), b.constraints(k), check_impulse=True)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------
def test_edges(ctx):
    sc = scenes.sphere_pile(2, 2, 2)
    bare = dict(sc, terrain=None)
    b = mgf_amd.WorldBatch.from_scenes(ctx, [bare, BQ.empty_scene(None)])
    assert len(b.raycast(np.zeros(0, np.int32), np.zeros((0, 3)), np.zeros((0, 3)))) == 0
    assert len(b.sweep(np.zeros(0, np.int32), np.zeros(0, mgf_amd.MOVING_DTYPE))) == 0
    assert len(b.colliders(1)) == 0 and len(b.colliders()) == 8
    p = (sc["comps"]["p"] + np.float32([0, 5, 0])).astype(np.float32)
    d = np.tile(np.float32([0, -1, 0]), (len(p), 1))
    casts = np.concatenate([_cast(k % 2, p[k], (0.3, 0, 0), 0.2, (0, -6, 0)) for k in range(len(p))])
    world = np.int32([0, 1] * 4)
    zero_r, zero_s = np.zeros(len(p), mgf_amd._capi.RAY_HIT_DTYPE), np.zeros(len(p), mgf_amd._capi.SWEEP_HIT_DTYPE)
    zero_r["kind"] = zero_s["kind"] = -1
    for kinds in (mgf_amd._capi.QUERY_TERRAIN, mgf_amd._capi.QUERY_OBSTACLES):   # no terrain in this batch; a batch never has obstacles
        assert same_bytes(b.raycast(world, p, d, kinds=kinds), zero_r)
        assert same_bytes(b.sweep(world, casts, kinds=kinds), zero_s)
    got = b.raycast(world, p, d)
    assert np.all(got["kind"][world == 0] == 0) and np.all(got["kind"][world == 1] == -1)     # the empty world
    got = b.sweep(world, casts)
    assert np.all(got["kind"][world == 0] == 0) and same_bytes(got[world == 1], zero_s[world == 1])
    for bad in (2, 5):
        with pytest.raises(mgf_amd.MgfError) as e:
            b.raycast(np.int32([0, bad]), p[:2], d[:2])
        assert e.value.status == mgf_amd._capi.ERR_INVALID and "world index" in str(e.value)
        with pytest.raises(mgf_amd.MgfError):
            b.sweep(np.int32([bad, 0]), casts[:2])
    with pytest.raises(mgf_amd.MgfError):
        b.colliders(2)


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_launch_count_does_not_grow_with_the_batch(ctx):
    sc = scenes.sphere_pile(2, 2, 2)
    one, many = mgf_amd.WorldBatch.from_scenes(ctx, [sc]), mgf_amd.WorldBatch.from_scenes(ctx, [sc] * 64)
    p = np.tile(np.float32([0.1, 6.0, 0.2]), (640, 1))
    d = np.tile(np.float32([0, -1, 0]), (640, 1))
    casts = np.concatenate([_cast(0, (0.1, 6.0, 0.2), (0, 0, 0), 0.2, (0, -8, 0))] * 640)
    counts = []
    for b, world, n in ((one, np.zeros(3, np.int32), 3), (many, (np.arange(640) % 64).astype(np.int32), 640)):
        b.step(float(sc["dt"]), 4)
        b.colliders(0)
        r = b.raycast(world, p[:n], d[:n])
        lr = b.counter("query_launches")
        s = b.sweep(world, casts[:n])
        ls = b.counter("query_launches")
        assert np.all(r["kind"] >= 0) and np.all(s["kind"] >= 0) and b.counter("query_run_ns") > 0
        counts.append((lr, ls))
    assert counts[0] == counts[1] and 1 <= counts[0][0] <= 2 and 1 <= counts[0][1] <= 3, counts
