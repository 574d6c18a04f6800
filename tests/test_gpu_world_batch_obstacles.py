"""Static Compound obstacles per world of a batch (mgf_batch_add_obstacle, mgf_batch_set_world_obstacles): world k of the batch against
the oracle world that has had add_obstacle called once per entry of world k's list, and against the lone mgf_world given the same
compounds through mgf_compound_set_pose + mgf_world_add_obstacle, bit for bit - the tick's state, the constraint list with impulses,
the statistics, rays and sweeps - wherever the world sits, in whatever order the table was built and whichever worlds share an entry.
The conditions on these inputs (every list entry is met, the rays and casts meet obstacles, bodies, faces and ties) are checked from the
oracle alone in tests/test_world_batch_obstacles_host.py."""
import numpy as np
import pytest

import mgf_amd
from tests import batch_observe_cases as OC
from tests import batch_obstacle_cases as BC
from tests.util import bits_equal, compare_constraints

pytestmark = pytest.mark.gpu

STATE = ("x", "q", "v", "omega", "delta")
COUNTS = ("n_constraints", "n_terrain_constraints", "n_pair_candidates", "n_refits")
INV = mgf_amd._capi.ERR_INVALID
BODIES, TERRAIN, OBSTACLES, ALL = mgf_amd._capi.QUERY_BODIES, mgf_amd._capi.QUERY_TERRAIN, mgf_amd._capi.QUERY_OBSTACLES, mgf_amd._capi.QUERY_ALL


@pytest.fixture(scope="module")
def ctx():
    c = mgf_amd.Context(0)
    yield c
    c.close()


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _same_state(got, want, what):
    for f in STATE:
        assert bits_equal(got[f], want[f]), f"{what}: {f} differs"


def _same_world(a, ka, b, kb, what):
    _same_state(a.state(ka), b.state(kb), what)
    assert same_bytes(a.constraints(ka), b.constraints(kb)), f"{what}: the constraint lists differ"


def _batch(ctx, scs):
    return mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True)


def _lone(ctx, sc, obstacles=None):
    w = mgf_amd.World.from_scene(ctx, sc)
    for comps, disp, rot in (sc["obstacles"] if obstacles is None else obstacles):
        c = mgf_amd.Compound(ctx, comps)
        c.set_pose(disp, rot)
        w.add_obstacle(c)
    return w


def _step_lone(lone, dt, iters, n=1):
    for w in lone:
        if len(w):
            w.step_many(dt, iters, n)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run(ctx):
    """the seven worlds of BC.obstacle_scenes in one batch, free running beside one oracle world each: every tick the four counts, at
    BC.LIST_TICKS the lists with impulses and the state bits; then the lone worlds brought to the same tick (tests 1, 2, 5 and 6 share
    all this)"""
    scs = BC.obstacle_scenes()
    b = _batch(ctx, scs)
    assert b.obstacle_count() == 4 and [b.world_obstacle_count(k) for k in range(len(scs))] == [2, 2, 1, 2, 0, 3, 2]
    ows = [BC.oracle_with_obstacles(sc) for sc in scs]
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    seen = [0] * len(scs)
    for tick in range(1, BC.TICKS + 1):
        st = b.step(dt, iters)
        for k, ow in enumerate(ows):
            ost = ow.step(dt, iters)
            what = f"world {k} tick {tick}"
            assert st[k].n_bodies == len(scs[k]["comps"]) and st[k].iters == iters
            for f in COUNTS:
                assert getattr(st[k], f) == getattr(ost, f), f"{what}: {f} = {getattr(st[k], f)}, the oracle has {getattr(ost, f)}"
            if tick in BC.LIST_TICKS:
                compare_constraints(b.constraints(k), ow.constraints(), check_impulse=True)
                _same_state(b.state(k), ow.state(), what)
            seen[k] = max(seen[k], int(ost.n_terrain_constraints))
    lone = [_lone(ctx, sc) for sc in scs]
    _step_lone(lone, dt, iters, BC.TICKS)
    return dict(scs=scs, b=b, ows=ows, lone=lone, seen=seen, dt=dt, iters=iters)


def test_the_seven_worlds_against_the_oracle_wherever_they_sit(ctx, run):
    scs, b, dt, iters = run["scs"], run["b"], run["dt"], run["iters"]
    K = len(scs)
    print("most static constraints per world:", run["seen"])
    assert run["seen"][BC.BARE] > 0 and run["seen"][BC.EMPTY] == 0
    assert b.counter("launches_per_tick") <= 7
    # the worlds in reverse order, the table built by hand in another order (single, an entry nobody uses, ring, empty, ramp), one call a
    # world and the poses given per record
    C = BC.compounds()
    rb = _batch(ctx, [dict(sc, obstacles=[]) for sc in scs[::-1]])
    ids = {}
    for name in ("single", "unused", "ring", "empty", "ramp"):
        ids[name] = rb.add_obstacle(mgf_amd.Compound(ctx, C["single"] if name == "unused" else C[name]))
    assert list(ids.values()) == [0, 1, 2, 3, 4] and rb.obstacle_count() == 5
    key = {len(C[n]): n for n in ("single", "ring", "empty", "ramp")}
    for k, sc in enumerate(scs):
        if sc["obstacles"]:
            rb.set_world_obstacles(K - 1 - k, [ids[key[len(o[0])]] for o in sc["obstacles"]], [o[1] for o in sc["obstacles"]], [o[2] for o in sc["obstacles"]])
    rb.step(dt, iters, BC.TICKS)
    for k in range(K):
        _same_world(rb, K - 1 - k, b, k, f"world {k} in the batch built in reverse")
    assert rb.counter("launches_per_tick") == b.counter("launches_per_tick")


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def test_every_world_against_the_lone_world(run):
    scs, b, lone = run["scs"], run["b"], run["lone"]
    whole = b.body_contacts()
    at = 0
    for k, sc in enumerate(scs):
        n = len(sc["comps"])
        if n:
            _same_state(b.state(k), lone[k].state(), f"world {k} against the lone world")
            cons = lone[k].constraints()
            assert same_bytes(b.constraints(k), cons), f"world {k}: the constraint list differs from the lone world's"
            want = OC.fold(b.constraints(k), n)
            assert same_bytes(b.body_contacts(k), want) and same_bytes(whole[at:at + n], want), f"world {k}: contact summaries"
            if sc["obstacles"] or sc["terrain"] is not None:
                assert want["n_terrain"].sum() > 0, k
        at += n


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_capacity_reruns_with_obstacles(ctx, run):
    scs, dt, iters = run["scs"], run["dt"], run["iters"]
    b = _batch(ctx, scs)
    b.set_option("cons_per_body", 1)
    b.step(dt, iters, BC.TICKS)
    assert b.counter("capacity_retries") > 0
    for k in range(len(scs)):
        _same_world(b, k, run["b"], k, f"world {k}")


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def _forced_tick(b, k, sc, obstacles, dt, iters, what):
    """one tick of world k held to an oracle world rebuilt with `obstacles` and teacher-forced from the batch's state"""
    ow = BC.oracle_with_obstacles(sc, obstacles)
    s = b.state(k)
    ow.set_state(**s)
    st = b.step(dt, iters)
    ost = ow.step(dt, iters)
    assert (st[k].n_constraints, st[k].n_terrain_constraints) == (ost.n_constraints, ost.n_terrain_constraints), what
    compare_constraints(b.constraints(k), ow.constraints(), check_impulse=True)
    _same_state(b.state(k), ow.state(), what)
    return int(ost.n_terrain_constraints)


def test_reassignment_between_steps(ctx):
    scs = BC.obstacle_scenes()
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    C = BC.compounds()
    b, ref = _batch(ctx, scs), _batch(ctx, scs)
    ring, ramp = (next(i for i, n in enumerate(("ramp", "ring", "empty", "single")) if n == w) for w in ("ring", "ramp"))   # from_scenes' ids: first use
    assert b.obstacle_count() == 4
    b.step(dt, iters, 15)
    ref.step(dt, iters, 15)
    moved = (C["ring"], (0.2, 0.15, -0.1), BC._quat((0, 1, 0), 0.6))
    old = {k: scs[k]["obstacles"] for k in range(len(scs))}
    # world 0's list replaced by the ring alone at a new pose; world 1's emptied by -1 records; world 3 named by several records, one of
    # them a -1: (ring, ramp) at the table's poses; world 2 (and the rest) not named
    b.set_world_obstacles([0, 1, 3, 1, 3, 3], [ring, -1, ring, -1, -1, ramp],
                          [moved[1]] + [(0.0, 0.0, 0.0)] * 5, [moved[2]] + [BC.IDENT] * 5)
    assert [b.world_obstacle_count(k) for k in range(4)] == [1, 0, 1, 2]
    new = {0: [moved], 1: [], 3: [(C["ring"], (0.0, 0.0, 0.0), BC.IDENT), (C["ramp"], (0.0, 0.0, 0.0), BC.IDENT)]}
    seen = {0: 0, 1: 0, 3: 0}
    for t in range(6):
        for k in new:
            seen[k] = max(seen[k], _forced_tick(b, k, scs[k], new[k], dt, iters, f"world {k}, tick {t} behind the reassignment"))
    ref.step(dt, iters, 6 * len(new))
    _same_world(b, 2, ref, 2, "the world no record named")
    _same_world(b, 6, ref, 6, "another world no record named")
    assert not bits_equal(b.state(0)["x"], ref.state(0)["x"]) and not bits_equal(b.state(1)["x"], ref.state(1)["x"])
    assert seen[0] > 0 and seen[3] > 0
    # with disp and rot NULL the poses are the ones the compounds had when they were added: from_scenes adds them at the identity
    b.set_world_obstacles([3, 3], [ring, ramp])
    _forced_tick(b, 3, scs[3], new[3], dt, iters, "world 3 at the poses of the table")
    # restored: the lists the worlds began with
    for k in (0, 1, 3):
        key = {len(C[n]): i for i, n in enumerate(("ramp", "ring", "empty", "single"))}
        b.set_world_obstacles(k, [key[len(o[0])] for o in old[k]], [o[1] for o in old[k]], [o[2] for o in old[k]])
    for t in range(3):
        for k in (0, 1, 3):
            _forced_tick(b, k, scs[k], old[k], dt, iters, f"world {k}, tick {t} behind the restoring")
    # refusals that need a real handle change nothing
    n = b.obstacle_count()
    for world, obstacle, word in (([0, 7], [-1, -1], "world index"), ([0, 1], [-1, n], "obstacle id"), ([0, 1 << 20], [-1, 0], "world index"),
                                  ([5] + [2] * 65, [-1] + [ring] * 65, "MGF_BATCH_MAX_WORLD_OBSTACLES")):
        with pytest.raises(mgf_amd.MgfError) as e:
            b.set_world_obstacles(world, obstacle)   # (the first record of each call is a valid one: it must not be applied)
        assert e.value.status == INV and word in str(e.value), (world[:3], str(e.value))
    assert [b.world_obstacle_count(k) for k in range(7)] == [2, 2, 1, 2, 0, 3, 2]
    b.set_world_obstacles([2] * 64, ring)   # (the limit itself is a valid list)
    assert b.world_obstacle_count(2) == 64


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_queries_see_the_obstacles_of_their_world(ctx, run):
    scs, b, lone, ows = run["scs"], run["b"], run["lone"], run["ows"]
    K = len(scs)
    cols = [ow.colliders()[0] for ow in ows]
    for k in range(K):
        got = b.colliders(k)
        assert all(np.array_equal(got[f], cols[k][f]) for f in ("tag", "p", "d", "r")), f"world {k}: colliders"   # so the queries are the host check's
    rays, casts = BC.rays_and_casts(scs, [BC.centres_of(c) for c in cols])
    world, p, d, dt = rays["world"], rays["p"], rays["d"], rays["dt"]
    cw, cc = casts["world"], casts["casts"]
    launches = {}
    for kinds in (BODIES, TERRAIN, OBSTACLES, ALL):
        for ign in (None, rays["ignore"]):
            got = b.raycast(world, p, d, dt, ignore=ign, kinds=kinds)
            launches["ray", kinds] = b.counter("query_launches")
            for k in range(K):
                sel = world == k
                want = lone[k].raycast(p[sel], d[sel], dt[sel], ignore=None if ign is None else ign[sel], kinds=kinds)
                assert same_bytes(got[sel], want), f"world {k} kinds {kinds}: rays"
            if kinds == OBSTACLES:
                assert set(got["kind"].tolist()) == {-1, 2} and np.all(got[world == BC.PLAIN]["kind"] == -1)
                tie = got[rays["tie"] & (got["kind"] == 2) & (got["index"] > 0)]
                assert len(tie) >= 1 and np.all(tie["index"] == 1)   # the doubled ring: the first of the two entries answers
                assert np.all(got[(world == BC.HOLE) & (got["kind"] == 2)]["index"] == 1)   # behind the empty compound
            if kinds == ALL:
                assert set(got["kind"].tolist()) == {-1, 0, 1, 2}
        for ign in (None, np.where(np.arange(len(cw)) % 3 == 0, 0, -1).astype(np.int32)):
            got = b.sweep(cw, cc, ignore=ign, kinds=kinds)
            launches["sweep", kinds] = b.counter("query_launches")
            for k in range(K):
                sel = cw == k
                lign = None if ign is None else np.where(len(scs[k]["comps"]) > 0, ign[sel], -1).astype(np.int32)
                if ign is not None and not len(scs[k]["comps"]):
                    continue   # (a world without bodies has no body 0 to ignore: the lone world refuses the index)
                assert same_bytes(got[sel], lone[k].sweep(cc[sel], ignore=lign, kinds=kinds)), f"world {k} kinds {kinds}: sweeps"
            if kinds == OBSTACLES and ign is None:
                assert set(got["kind"].tolist()) == {-1, 2}
                tie = got[casts["tie"] & (got["kind"] == 2)]
                assert len(tie) >= 2 and np.all(tie["index"] == 1)
    print("query launches:", launches)
    assert launches["ray", OBSTACLES] == launches["ray", BODIES] + 1 and launches["ray", ALL] == launches["ray", OBSTACLES]
    assert launches["sweep", ALL] == launches["sweep", BODIES] + 2 and launches["sweep", OBSTACLES] == launches["sweep", BODIES] + 1
    # the launches of a call do not grow with the batch: 70 worlds
    many = _batch(ctx, [scs[k % K] for k in range(10 * K)])
    got = many.raycast(world + K * (np.arange(len(world)) % 10).astype(np.int32), p, d, dt)
    assert many.counter("query_launches") == launches["ray", ALL]
    many.sweep(cw + K * (np.arange(len(cw)) % 10).astype(np.int32), cc)
    assert many.counter("query_launches") == launches["sweep", ALL]
    assert many.counter("launches_per_tick") == b.counter("launches_per_tick") <= 7
    # a query touches nothing of the tick: the worlds go on as the oracle's and the lone worlds do
    st = b.step(run["dt"], run["iters"])
    _step_lone(lone, run["dt"], run["iters"])
    for k, ow in enumerate(ows):
        ow.step(run["dt"], run["iters"])
        _same_state(b.state(k), ow.state(), f"world {k} a tick behind the queries")
        if len(scs[k]["comps"]):
            _same_state(b.state(k), lone[k].state(), f"world {k} a tick behind the queries, the lone world")


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_a_table_nobody_uses_changes_nothing(ctx):
    scs = [dict(sc, obstacles=[]) for sc in BC.obstacle_scenes()]
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    C = BC.compounds()
    plain, tabled = _batch(ctx, scs), _batch(ctx, scs)
    for name in ("ramp", "ring", "empty"):
        tabled.add_obstacle(mgf_amd.Compound(ctx, C[name]))
    tabled.set_world_obstacles([0, 3], -1)   # (named, by records that contribute nothing)
    assert tabled.obstacle_count() == 3 and plain.obstacle_count() == 0 and all(tabled.world_obstacle_count(k) == 0 for k in range(len(scs)))
    sp, stt = plain.step(dt, iters, 20), tabled.step(dt, iters, 20)
    assert [s.as_dict() for s in sp] == [s.as_dict() for s in stt]
    for k in range(len(scs)):
        _same_world(tabled, k, plain, k, f"world {k}")
    assert plain.counter("launches_per_tick") == tabled.counter("launches_per_tick") == 6
    cols = [plain.colliders(k) for k in range(len(scs))]
    tabled.colliders(0)   # (the colliders gathered behind the step: not a launch of the calls counted below)
    rays, casts = BC.rays_and_casts(BC.obstacle_scenes(), [BC.centres_of(c) for c in cols])
    for kinds in (ALL, OBSTACLES):
        a = plain.raycast(rays["world"], rays["p"], rays["d"], rays["dt"], kinds=kinds)
        la = plain.counter("query_launches")
        t = tabled.raycast(rays["world"], rays["p"], rays["d"], rays["dt"], kinds=kinds)
        assert same_bytes(a, t) and la == tabled.counter("query_launches") == 1
        a = plain.sweep(casts["world"], casts["casts"], kinds=kinds)
        la = plain.counter("query_launches")
        t = tabled.sweep(casts["world"], casts["casts"], kinds=kinds)
        assert same_bytes(a, t) and la == tabled.counter("query_launches") == (2 if kinds == ALL else 1)
        if kinds == OBSTACLES:
            assert np.all(a["kind"] == -1)


def test_copy_worlds_leaves_the_destinations_list_alone(ctx, run):
    scs, src, dt, iters = run["scs"], run["b"], run["dt"], run["iters"]
    # the destination: the box scene three times, world 0 with a list of its own, world 1 with the source's, world 2 with none
    own = scs[BC.POSED]["obstacles"]
    dst = _batch(ctx, [dict(scs[BC.BOX], obstacles=own), scs[BC.BOX], dict(scs[BC.BOX], obstacles=[])])
    ref = _batch(ctx, [dict(scs[BC.BOX], obstacles=own), scs[BC.BOX], dict(scs[BC.BOX], obstacles=[])])
    dst.step(dt, iters, 3)
    ref.step(dt, iters, 3)
    s0 = src.state(BC.BOX)
    dst.copy_worlds([0, 1, 2], src, BC.BOX)
    assert [dst.world_obstacle_count(k) for k in range(3)] == [2, 2, 0]
    for k in range(3):
        _same_world(dst, k, src, BC.BOX, f"copy {k}")
    # a probe of the same tick on the oracle's side: the source's state under each destination's list
    want = {}
    for k, obs in ((0, own), (1, scs[BC.BOX]["obstacles"]), (2, [])):
        ow = BC.oracle_with_obstacles(scs[BC.BOX], obs)
        ow.set_state(**s0)
        ow.step(dt, iters)
        want[k] = ow
    dst.step(dt, iters)
    for k, ow in want.items():
        _same_state(dst.state(k), ow.state(), f"copy {k} a tick on, under the destination's list")
        compare_constraints(dst.constraints(k), ow.constraints(), check_impulse=True)
    assert not bits_equal(dst.state(0)["v"], dst.state(1)["v"]) and not bits_equal(dst.state(2)["v"], dst.state(1)["v"])
