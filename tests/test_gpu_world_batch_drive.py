"""Driving a batch on the device (mgf_batch_get_many, _set_many, _set_forces, _apply_impulses, _copy_worlds): forces, torques, velocity
commands, impulses and world-to-world copies against the oracle (free running, or teacher-forced through set_state where the oracle has
no setter), against np_restatement.Bodies for torque, against the lone mgf_world for get - and nothing else of the batch moves."""
import numpy as np
import pytest

from mgf_amd import scenes
from tests import batch_drive_cases as DC
from tests.util import bits_equal, compare_constraints, oracle_world, values_equal

pytestmark = pytest.mark.gpu

STATE = DC.STATE
COUNTS = ("n_constraints", "n_terrain_constraints", "n_pair_candidates", "n_refits")
LIST_TICKS = (1, 10, 40, 50, 75)
BYSTANDER = 6   # a seventh world, with its scene's own force, that no per-body call of these tests names


@pytest.fixture(scope="module")
def ctx():
    import mgf_amd
    c = mgf_amd.Context(0)
    yield c
    c.close()


def _scenes7():
    return DC.drive_scenes() + [scenes.sphere_pile(4, 4, 4, seed=100)]


def _forced7():
    """the scenes as the oracle builds them: world k < 6 under WORLD_FORCES[k], the bystander under its own"""
    scs = _scenes7()
    return [DC.with_force(sc, DC.WORLD_FORCES[k]) for k, sc in enumerate(scs[:6])] + scs[6:]


@pytest.fixture(scope="module")
def oracle75():
    """the seven oracle worlds free running for 75 ticks: per world and tick (counts, state), the lists at LIST_TICKS"""
    scs = _forced7()
    _, hist, lists = DC.run_oracles(scs, 75, LIST_TICKS)
    return scs, hist, lists


def _forced_batch(ctx):
    """test 1's batch: built with every scene's default force, then - before the first tick - one set_forces call for all worlds"""
    import mgf_amd
    scs = _scenes7()
    b = mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True)
    world, body = DC.all_bodies(scs[:6], 3)
    mass = np.concatenate([sc["mass"] for sc in scs[:6]])[0]
    b.set_forces(world, body, force=DC.WORLD_FORCES[world] * mass)
    return b, scs


def _same_state(got, want, what, equal=bits_equal):
    for f in STATE:
        assert equal(got[f], want[f]), f"{what}: {f} differs"


def _same_counts(st, want, what, n=4):
    got = tuple(int(getattr(st, f)) for f in COUNTS)
    assert got[:n] == tuple(want)[:n], f"{what}: counts {got}, the oracle has {want}"


def _same_world(a, ka, b, kb, what):
    _same_state(a.state(ka), b.state(kb), what)
    assert a.constraints(ka).tobytes() == b.constraints(kb).tobytes(), f"{what}: constraint lists differ"


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
def test_forces_from_tick_0_against_the_oracle(ctx, oracle75):
    import mgf_amd
    scs, hist, lists = oracle75
    b, _ = _forced_batch(ctx)
    ref = mgf_amd.WorldBatch.from_scenes(ctx, _scenes7(), own_terrain=True)   # receives no call
    got = b.get(*DC.all_bodies(scs[:6], 5))
    w5, _ = DC.all_bodies(scs[:6], 5)
    assert bits_equal(got["force"], DC.WORLD_FORCES[w5]) and not np.any(got["torque"])
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    most = [0] * 7
    for tick in range(1, 41):
        st = b.step(dt, iters)
        for k in range(7):
            what = f"world {k} tick {tick}"
            _same_counts(st[k], hist[k][tick - 1][0], what)
            _same_state(b.state(k), hist[k][tick - 1][1], what)
            if tick in (1, 10, 40):
                compare_constraints(b.constraints(k), lists[k][tick], check_impulse=True)
            most[k] = max(most[k], int(st[k].n_constraints))
    print("most constraints per world:", most)
    assert all(m >= 30 for m in most), most
    ref.step(dt, iters, 40)
    _same_world(b, BYSTANDER, ref, BYSTANDER, "the world no record names")
    assert not bits_equal(b.state(1)["x"], ref.state(1)["x"])   # (the forces did something)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def test_a_switch_of_forces_in_mid_run(ctx, oracle75):
    scs, hist, _ = oracle75
    b, _ = _forced_batch(ctx)
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    b.step(dt, iters, DC.SWITCH_TICK)
    world, body = DC.switched(scs[:6])
    mass = scs[0]["mass"][0]
    b.set_forces(world, body, force=DC.SWITCH_FORCE * mass)
    ows = []
    for k, sc in enumerate(scs[:6]):
        ow = oracle_world(DC.with_force(sc, DC.switched_force(sc, k)))
        ow.set_state(**hist[k][DC.SWITCH_TICK - 1][1])
        ows.append(ow)
    seen = [[0, 0] for _ in ows]
    for tick in range(1, DC.SWITCH_RUN + 1):
        st = b.step(dt, iters)
        for k, ow in enumerate(ows):
            ost = ow.step(dt, iters)
            what = f"world {k}, tick {tick} behind the switch"
            _same_counts(st[k], (int(ost.n_constraints), int(ost.n_terrain_constraints)), what, n=2)
            _same_state(b.state(k), ow.state(), what, equal=values_equal)
            compare_constraints(b.constraints(k), ow.constraints(), check_impulse=True)
            seen[k][0] = max(seen[k][0], int(ost.n_terrain_constraints))
            seen[k][1] = max(seen[k][1], int(ost.n_constraints - ost.n_terrain_constraints))
    assert all(t > 0 and p > 0 for t, p in seen), seen
    # the untouched bodies kept their force, the switched ones hold the new one
    for k, sc in enumerate(scs[:6]):
        got = b.get(k, np.arange(len(sc["comps"])))
        assert bits_equal(got["force"], DC.switched_force(sc, k) * mass), k
    _same_state(b.state(BYSTANDER), hist[BYSTANDER][DC.SWITCH_TICK + DC.SWITCH_RUN - 1][1], "the bystander")
    # forces are rows of the body: they survive bodies added behind a tick (the pull and push of the mirror), and so does the state
    at60 = b.state(1)
    b.add_bodies(BYSTANDER, scs[BYSTANDER]["comps"][:1], 1.0, 0.3, 0.6, (0.0, -9.8, 0.0))
    assert b.world_len(BYSTANDER) == 65 and len(b.constraints(1)) == 0
    b.set_forces(BYSTANDER, 64, torque=(0.0, 0.5, 0.0))   # a body no tick has touched, in a batch that is back in its mirror
    got = b.get(1, np.arange(len(scs[1]["comps"])))
    assert bits_equal(got["force"], DC.switched_force(scs[1], 1) * mass) and bits_equal(got["linear"], at60["v"])
    new = b.get(BYSTANDER, 64)
    assert bits_equal(new["torque"], np.float32([[0.0, 0.5, 0.0]])) and bits_equal(new["force"], np.float32([[0.0, -9.8, 0.0]]))


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_torque_in_free_flight(ctx):
    import mgf_amd
    scs = DC.torque_scenes()
    b = mgf_amd.WorldBatch(ctx, len(scs))
    for k, sc in enumerate(scs):
        b.add_bodies(k, sc["comps"], 2.0, 0.3, 0.6, sc["force"])
        b.write_state(k, v=sc["v0"], omega=sc["omega0"])
    sched = [DC.torque_schedule(k) for k in range(len(scs))]
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]

    def set_torques(t):
        world = np.concatenate([np.full(len(s[t][0]), k, np.int32) for k, s in enumerate(sched)])
        body = np.concatenate([s[t][0] for s in sched])
        order = np.random.default_rng(t).permutation(len(world))
        b.set_forces(world[order], body[order], torque=np.concatenate([s[t][1] for s in sched])[order])
    set_torques(0)
    state0 = [b.state(k) for k in range(len(scs))]
    got0 = [b.get(k, np.arange(8)) for k in range(len(scs))]
    for k in range(len(scs)):   # before a tick: inv_moment is the body inertia, the torque row holds what was set, the force world_force * mass
        assert bits_equal(got0[k]["force"], scs[k]["force"] * np.float32(2.0)) and bits_equal(got0[k]["inv_mass"], np.full(8, 0.5, np.float32))
        assert bits_equal(got0[k]["torque"][sched[k][0][0]], sched[k][0][1])
    want = [DC.torque_restatement(state0[k], got0[k], sched[k], dt) for k in range(len(scs))]
    first = None
    for t in range(DC.TORQUE_TICKS):
        if t in (10, 20):
            set_torques(t)
        st = b.step(dt, iters)
        for k in range(len(scs)):
            assert st[k].n_constraints == 0, "the bodies were to fly free"
            _same_state(b.state(k), want[k][t], f"world {k} tick {t + 1}")
        if t == 0:
            first = [b.state(k)["omega"] for k in range(len(scs))]
    # the anisotropic inertia is in play: a capsule's omega does not follow its torque's direction - neither its first increment
    # I * torque * dt nor where it ends
    skew_first, skew_end = 0, 0
    for k, sc in enumerate(scs):
        end = b.state(k)["omega"]
        for i, tq0, tq1 in zip(sched[k][0][0], sched[k][0][1], sched[k][10][1]):
            if sc["comps"]["tag"][i] != 1:
                continue
            dw = (first[k][i] - state0[k]["omega"][i]).astype(np.float64)
            skew_first += np.linalg.norm(np.cross(dw, tq0)) > 1e-3 * np.linalg.norm(dw) * np.linalg.norm(tq0)
            skew_end += np.linalg.norm(np.cross(end[i].astype(np.float64), tq1)) > 1e-3 * np.linalg.norm(end[i]) * np.linalg.norm(tq1)
    assert skew_first >= 1 and skew_end >= 1, (skew_first, skew_end)
    assert all(not np.any(b.get(k, np.arange(8))["torque"]) for k in range(len(scs)))   # zeroed at tick 20


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def _get_matches(b, lone, ows, world, body, what):
    got = b.get(world, body)
    for r, (k, i) in enumerate(zip(world.tolist(), body.tolist())):
        vel, info = lone[k].get(i)
        o = ows[k].get(i)
        mine = {f: got[f][r] for f in ("linear", "angular", "x", "restitution", "friction", "inv_mass", "inv_moment")}
        theirs = dict(linear=vel.linear.tup(), angular=vel.angular.tup(), x=info.x.tup(), restitution=info.restitution, friction=info.friction,
                      inv_mass=info.inv_mass, inv_moment=list(info.inv_moment))
        for f in mine:
            assert bits_equal(mine[f], np.float32(theirs[f])), f"{what}: {f} of body {i} of world {k} differs from mgf_world_get"
            assert bits_equal(mine[f], np.float32(o[f])), f"{what}: {f} of body {i} of world {k} differs from the oracle's get"
    return got


def test_get_and_set(ctx, oracle75):
    import mgf_amd
    scs, _, _ = oracle75
    b, _ = _forced_batch(ctx)
    lone = [mgf_amd.World.from_scene(ctx, sc) for sc in scs]
    ows = [oracle_world(sc) for sc in scs]
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    world, body = DC.random_pairs(scs, 200, 31)
    got = _get_matches(b, lone, ows, world, body, "before any tick")
    assert bits_equal(got["force"], np.array([scs[k]["force"][i] for k, i in zip(world, body)])) and not np.any(got["torque"])
    b.step(dt, iters, 20)
    for k in range(7):
        lone[k].step_many(dt, iters, 20)
        for _ in range(20):
            ows[k].step(dt, iters)
    _get_matches(b, lone, ows, world, body, "after 20 ticks")
    before = b.body_contacts()
    world, body, lin, ang = DC.velocity_commands(scs[:6])
    b.set_velocities(world, body, lin, ang)
    for k, i, lv, av in zip(world.tolist(), body.tolist(), lin, ang):
        ows[k].set_velocity(i, lv, av)
    assert b.body_contacts().tobytes() == before.tobytes()   # the list still describes the last tick
    last = {(k, i): r for r, (k, i) in enumerate(zip(world.tolist(), body.tolist()))}
    got = b.get(world, body)
    for r, key in enumerate(zip(world.tolist(), body.tolist())):
        assert bits_equal(got["linear"][r], lin[last[key]]) and bits_equal(got["angular"][r], ang[last[key]]), "the last record of a body wins"
    for tick in range(1, 11):
        st = b.step(dt, iters)
        for k, ow in enumerate(ows):
            ost = ow.step(dt, iters)
            what = f"world {k}, tick {tick} behind set_many"
            _same_counts(st[k], tuple(int(getattr(ost, f)) for f in COUNTS), what)
            _same_state(b.state(k), ow.state(), what)
            if tick in (1, 10):
                compare_constraints(b.constraints(k), ow.constraints(), check_impulse=True)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_impulses(ctx, oracle75):
    scs, hist, _ = oracle75
    b, _ = _forced_batch(ctx)
    ref, _ = _forced_batch(ctx)
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    b.step(dt, iters, 20)
    ref.step(dt, iters, 20)
    world, body, lin, ang = DC.impulse_records(scs[:6])
    before = b.get(world, body)
    want_v, want_w = DC.impulses_expected(before, world, body, lin, ang)
    b.apply_impulses(world, body, lin, ang)
    after = b.get(world, body)
    assert bits_equal(after["linear"], want_v) and bits_equal(after["angular"], want_w)
    assert not bits_equal(after["linear"], before["linear"])
    for f in ("x", "restitution", "friction", "inv_mass", "inv_moment", "force", "torque"):
        assert bits_equal(after[f], before[f]), f
    _same_world(b, BYSTANDER, ref, BYSTANDER, "the world no record names")
    named = set(zip(world.tolist(), body.tolist()))
    for k in range(6):   # of a named world, the bodies no record names and everything but the velocities
        sa, sr = b.state(k), ref.state(k)
        keep = np.array([(k, i) not in named for i in range(len(scs[k]["comps"]))])
        for f in STATE:
            rows = keep if f in ("v", "omega") else slice(None)
            assert bits_equal(sa[f][rows], sr[f][rows]), (k, f)
        assert b.constraints(k).tobytes() == ref.constraints(k).tobytes() and b.colliders(k).tobytes() == ref.colliders(k).tobytes()
    # one linear-only and one angular-only call: NULL = zero for all records of that array
    b.apply_impulses(world[:5], body[:5], linear=lin[:5])
    b.apply_impulses(world[:5], body[:5], angular=ang[:5])
    ows = []
    for k, sc in enumerate(scs[:6]):
        ow = oracle_world(sc)
        for _ in range(20):
            ow.step(dt, iters)
        ows.append(ow)
    final = b.get(world, body)
    for r, (k, i) in enumerate(zip(world.tolist(), body.tolist())):
        ows[k].set_velocity(i, final["linear"][r], final["angular"][r])
    st = b.step(dt, iters, 10)
    ref.step(dt, iters, 10)
    for k, ow in enumerate(ows):
        for t in range(10):
            ost = ow.step(dt, iters)
            _same_counts(st[t * 7 + k], tuple(int(getattr(ost, f)) for f in COUNTS), f"world {k}, tick {t + 1} behind the impulses")
        _same_state(b.state(k), ow.state(), f"world {k} ten ticks behind the impulses")
        compare_constraints(b.constraints(k), ow.constraints(), check_impulse=True)
    _same_world(b, BYSTANDER, ref, BYSTANDER, "the world no record names, ten ticks on")
    _same_state(b.state(BYSTANDER), hist[BYSTANDER][29][1], "the bystander at tick 30")


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def _answers_alike(a, b, scs, what):
    """constraints, body_contacts, colliders, 16 rays and 4 boxes per world"""
    rng = np.random.default_rng(8)
    for k, sc in enumerate(scs):
        n = len(sc["comps"])
        assert a.constraints(k).tobytes() == b.constraints(k).tobytes(), f"{what}: constraints of world {k}"
        assert a.body_contacts(k).tobytes() == b.body_contacts(k).tobytes(), f"{what}: body_contacts of world {k}"
        assert a.colliders(k).tobytes() == b.colliders(k).tobytes(), f"{what}: colliders of world {k}"
    centres = [b.colliders(k)["p"] for k in range(len(scs))]
    world = np.repeat(np.arange(len(scs), dtype=np.int32), 16)
    p = np.array([centres[k][rng.integers(0, len(centres[k]))] for k in world], np.float32) + np.float32([0.0, 4.0, 0.0]) + rng.uniform(-0.3, 0.3, (len(world), 3)).astype(np.float32)
    d = np.float32([0.0, -1.0, 0.0]) + rng.uniform(-0.2, 0.2, (len(world), 3)).astype(np.float32)
    ra, rb = a.raycast(world, p, d), b.raycast(world, p, d)
    assert ra.tobytes() == rb.tobytes(), f"{what}: rays"
    bw = np.repeat(np.arange(len(scs), dtype=np.int32), 4)
    boxes = np.empty((len(bw), 6), np.float32)
    boxes[:, :3] = [centres[k][rng.integers(0, len(centres[k]))] for k in bw]
    boxes[:, 3:] = rng.uniform(0.3, 1.5, (len(bw), 1))
    oa, va = a.overlap_boxes(bw, boxes)
    ob, vb = b.overlap_boxes(bw, boxes)
    assert np.array_equal(oa, ob) and np.array_equal(va, vb), f"{what}: boxes"
    return int(np.sum(ra["kind"] >= 0)), len(va)


@pytest.mark.parametrize("cons_per_body", [4, 1])
def test_copies(ctx, oracle75, cons_per_body):
    scs, hist, lists = oracle75
    B, _ = _forced_batch(ctx)
    S, _ = _forced_batch(ctx)
    R, _ = _forced_batch(ctx)   # receives no copy
    S.set_option("cons_per_body", cons_per_body)
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    B.step(dt, iters, 30)
    every = np.arange(7, dtype=np.int32)
    S.copy_worlds(every, B, every)
    assert S.counter("drive_launches") == (1 if cons_per_body == 4 else 2)   # (with one record a body the shares had to grow first)
    hits, inside = _answers_alike(S, B, scs, "S <- B at tick 30")
    assert hits > 30 and inside >= 28, (hits, inside)
    assert sum(hist[k][29][0][0] for k in range(7)) > 400
    for k in range(7):
        _same_state(S.state(k), B.state(k), f"S <- B, world {k}")
        assert len(S.constraints(k)) == hist[k][29][0][0]
        assert bits_equal(S.get(k, np.arange(5))["force"], B.get(k, np.arange(5))["force"])
    B.step(dt, iters, 25)
    R.step(dt, iters, 55)
    back = np.int32([0, 2, 5])
    B.copy_worlds(back, S, back)
    assert B.counter("drive_launches") == 1
    for k in (1, 3, 4, 6):
        _same_world(B, k, R, k, f"world {k} beside the copied ones")
    for k in back:
        _same_world(B, int(k), S, int(k), f"B <- S, world {k}")
    st = B.step(dt, iters, 20)
    R.step(dt, iters, 20)
    for k in range(7):
        tick = 50 if k in (0, 2, 5) else 75
        what = f"world {k} at tick {tick}"
        _same_counts(st[19 * 7 + k], hist[k][tick - 1][0], what)
        _same_state(B.state(k), hist[k][tick - 1][1], what)
        compare_constraints(B.constraints(k), lists[k][tick], check_impulse=True)
    for k in (1, 3, 4, 6):
        _same_world(B, k, R, k, f"world {k} beside the copied ones, 20 ticks on")
    # the snapshot steps on as its source did: S at tick 30 + 20
    st = S.step(dt, iters, 20)
    for k in range(7):
        what = f"the snapshot's world {k} at tick 50"
        _same_counts(st[19 * 7 + k], hist[k][49][0], what)
        _same_state(S.state(k), hist[k][49][1], what)
        compare_constraints(S.constraints(k), lists[k][50], check_impulse=True)
    # a copy within one batch: world 3 of B becomes its world 1 (both piles of 64)
    B.copy_worlds(3, None, 1)
    _same_world(B, 3, B, 1, "B[3] <- B[1]")
    assert B.body_contacts(3).tobytes() == B.body_contacts(1).tobytes() and B.colliders(3).tobytes() == B.colliders(1).tobytes()


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------
def test_fan_out_on_more_worlds_than_compute_units(ctx):
    import mgf_amd
    K, sc = DC.FAN_K, DC.fan_scene()
    n = len(sc["comps"])
    dt, iters = float(sc["dt"]), sc["iters"]
    b = mgf_amd.WorldBatch.from_scenes(ctx, [sc] * K)
    rng = np.random.default_rng(9)
    for k in range(1, K, 7):   # the other worlds are not world 0 when the copy comes
        b.write_state(k, v=rng.uniform(-1, 1, (n, 3)).astype(np.float32))
    b.step(dt, iters, DC.FAN_TICKS)
    assert len(b.constraints(0)) > 0 and not bits_equal(b.state(1)["x"], b.state(0)["x"])
    b.copy_worlds(np.arange(1, K), None, 0)
    assert b.counter("drive_launches") == 1
    whole = b.state()
    for k in (1, 150, 299):
        _same_world(b, k, b, 0, f"copy {k}")
        assert bits_equal(whole["x"][k * n:(k + 1) * n], whole["x"][:n])
    body, lin, ang = DC.fan_impulses()
    every = np.arange(K, dtype=np.int32)
    order = np.random.default_rng(10).permutation(K)
    b.apply_impulses(every[order], body[order], lin[order], ang[order])
    b.step(dt, iters, DC.FAN_RUN)
    whole = b.state()
    lists = {k: b.constraints(k) for k in range(K)}
    # ten worlds spread over the batch against oracle worlds teacher-forced the same way
    src = oracle_world(sc)
    for _ in range(DC.FAN_TICKS):
        src.step(dt, iters)
    at20 = src.state()
    for k in np.linspace(0, K - 1, 10).astype(int):
        ow = oracle_world(sc)
        ow.set_state(**at20)
        g = src.get(int(body[k]))
        v = g["linear"] + lin[k] * g["inv_mass"]
        I = g["inv_moment"].reshape(3, 3)
        w = g["angular"] + ((I[0] * ang[k][0] + I[1] * ang[k][1]) + I[2] * ang[k][2])
        ow.set_velocity(int(body[k]), v, w)
        for _ in range(DC.FAN_RUN):
            ow.step(dt, iters)
        _same_state({f: whole[f][k * n:(k + 1) * n] for f in STATE}, ow.state(), f"world {k} against the oracle", equal=values_equal)
        compare_constraints(lists[k], ow.constraints(), check_impulse=True)
    # every world against the same run in a batch of size 1: the snapshot copied in from another batch, the world's own kick, 15 ticks
    snap = mgf_amd.WorldBatch.from_scenes(ctx, [sc])
    snap.step(dt, iters, DC.FAN_TICKS)
    one = mgf_amd.WorldBatch.from_scenes(ctx, [sc])
    for k in range(K):
        one.copy_worlds(0, snap, 0)
        one.apply_impulses(0, body[k], lin[k], ang[k])
        one.step(dt, iters, DC.FAN_RUN)
        _same_state({f: whole[f][k * n:(k + 1) * n] for f in STATE}, one.state(0), f"world {k} against a batch of its own")
        assert lists[k].tobytes() == one.constraints(0).tobytes(), k
    assert len({whole["x"][k * n:(k + 1) * n].tobytes() for k in range(K)}) > K // 2   # (the kicks made the worlds differ)


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------------
def test_launches_do_not_grow_with_the_call_or_the_batch(ctx):
    import mgf_amd
    sc = DC.fan_scene()
    n = len(sc["comps"])
    dt, iters = float(sc["dt"]), sc["iters"]
    # (n = 1, one world) against (n = 4096, 300 worlds); a copy needs two worlds, and holds at most n_worlds pairs: 1 pair against 150
    one, two, big = (mgf_amd.WorldBatch.from_scenes(ctx, [sc] * k) for k in (1, 2, DC.FAN_K))
    plain = mgf_amd.WorldBatch.from_scenes(ctx, [sc] * DC.FAN_K)   # receives none of the five calls
    per_tick = plain.counter("launches_per_tick")
    rng = np.random.default_rng(12)
    N = 4096
    world, body = rng.integers(0, DC.FAN_K, N).astype(np.int32), rng.integers(0, n, N).astype(np.int32)
    a3, b3 = rng.uniform(-1, 1, (N, 3)).astype(np.float32), rng.uniform(-1, 1, (N, 3)).astype(np.float32)
    rays = (np.float32([[0.0, 30.0, 0.0]]), np.float32([[0.0, -1.0, 0.0]]))
    for stepped in (False, True):
        if stepped:
            for bt in (one, two, big, plain):
                bt.step(dt, iters, 3)
        seen = {}
        for name, bt, w, bd, x, y in (("one", one, world[:1] * 0, body[:1], a3[:1], b3[:1]), ("many", big, world, body, a3, b3)):
            counts = []
            bt.get(w, bd)
            counts.append(bt.counter("drive_launches"))
            bt.set_velocities(w, bd, x, y)
            counts.append(bt.counter("drive_launches"))
            bt.set_forces(w, bd, x, y)
            counts.append(bt.counter("drive_launches"))
            bt.apply_impulses(w, bd, x, y)
            counts.append(bt.counter("drive_launches"))
            if name == "one":
                two.copy_worlds(1, None, 0)
                counts.append(two.counter("drive_launches"))
            else:
                bt.copy_worlds(np.arange(150, 300), None, np.arange(150))
                counts.append(bt.counter("drive_launches"))
            seen[name] = counts
        assert seen["one"] == seen["many"] == [1, 1, 1, 1, 1], seen
        # "query_launches" keeps its meaning: a ray call behind the five calls counts what it counts on a batch that received none
        # (behind a step: the collider gather and the rays), and leaves "drive_launches" alone
        big.raycast(0, *rays)
        plain.raycast(0, *rays)
        assert big.counter("query_launches") == plain.counter("query_launches") == (2 if stepped else 1)
        assert big.counter("drive_launches") == 1
    assert one.counter("launches_per_tick") == two.counter("launches_per_tick") == big.counter("launches_per_tick") == per_tick


# ---- 9 ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_a_live_batch(ctx):
    import mgf_amd
    INV = mgf_amd._capi.ERR_INVALID
    scs = _scenes7()
    b, _ = _forced_batch(ctx)
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    b.step(dt, iters, 5)
    other_ctx = mgf_amd.Context(0)
    foreign = mgf_amd.WorldBatch.from_scenes(other_ctx, scs[:1])
    z = np.zeros((1, 3), np.float32)

    def snapshot():
        every = DC.all_bodies(scs, 1)
        return b.state(), b.get(*every), [b.constraints(k).tobytes() for k in range(7)]

    def refused(call, *args, **kw):
        before = snapshot()
        with pytest.raises(mgf_amd.MgfError) as e:
            call(*args, **kw)
        assert e.value.status == INV, str(e.value)
        after = snapshot()
        for f in STATE:
            assert bits_equal(after[0][f], before[0][f]), f
        assert after[1].tobytes() == before[1].tobytes() and after[2] == before[2]
    refused(b.copy_worlds, 0, None, 5)                       # 64 bodies and 48
    refused(b.copy_worlds, [2, 0], None, [1, 5])             # ... behind a pair that would have been fine: nothing is copied
    refused(b.copy_worlds, [1, 1], None, [2, 3])             # a destination named twice
    refused(b.copy_worlds, [1, 2], None, [2, 3])             # world 2: a source and a destination
    refused(b.copy_worlds, 7, None, 0)
    refused(b.copy_worlds, 0, None, 7)
    refused(b.copy_worlds, 0, foreign, 0)                    # another context
    for bad_world, bad_body in ((5, 48), (0, 64), (7, 0), (6, 1 << 20)):
        w, bd = np.int32([1, bad_world]), np.int32([3, bad_body])   # (behind a good record: nothing changes)
        refused(b.get, w, bd)
        refused(b.set_velocities, w, bd, z, z)
        refused(b.set_forces, w, bd, z, z)
        refused(b.apply_impulses, w, bd, z, z)
    b.copy_worlds(0, None, 1)   # (and the batch still takes a good call)
    _same_world(b, 0, b, 1, "a good copy behind the refusals")
    foreign = None
    other_ctx.close()
