"""Bodies of up to four components in the worlds of a batch (mgf_batch_add_compound_bodies): every world against its own oracle world
(World(ORDER_CANONICAL), the definition) and against the lone mgf_world given the same calls, bit for bit - state, constraint list with
impulses, counts - wherever the world sits, over terrain and obstacles, through a tick that outgrows its storage, through adding,
driving, observing and copying; and the calls that do not see parts yet refuse.  Every test asserts from the oracle's own lists that its
scene reached the branch it is there for."""
import numpy as np
import pytest

from mgf_amd import scenes
from tests import batch_observe_cases as OC
from tests import batch_obstacle_cases as BO
from tests import batch_parts_cases as PC
from tests.util import bits_equal, compare_constraints, oracle_world

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def ctx():
    import mgf_amd
    c = mgf_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def six():
    return PC.six_scenes()


def _batch(ctx, scs):
    import mgf_amd
    return mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True)


def _lone(ctx, sc):
    import mgf_amd
    from mgf_amd import _capi
    w = mgf_amd.World.from_scene(ctx, dict(sc, obstacles=None))
    for comps, disp, rot in (sc.get("obstacles") or ()):
        c = _capi.Compound(ctx, np.ascontiguousarray(comps, scenes.COMPONENT_DTYPE))
        c.set_pose(disp, rot)
        w.add_obstacle(c)
    return w


def _same_world(a, ka, b, kb, what):
    PC.same_state(a.state(ka), b.state(kb), what)
    compare_constraints(a.constraints(ka), b.constraints(kb), check_impulse=True)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
def test_six_worlds_against_the_oracle_free_running(ctx, six):
    b = _batch(ctx, six)
    assert [b.world_len(k) for k in range(6)] == [PC.n_bodies(sc) for sc in six] == [22, 18, 96, 35, 0, 1]
    assert b.counter("launches_per_tick") == 7
    seen = PC.run_against_oracle(b, PC.oracles(six), six, PC.TICKS, PC.LIST_TICKS)
    print("per world (most constraints, most terrain contacts, terrain contacts summed, largest manifold):", seen, "capacity_retries:",
          b.counter("capacity_retries"))
    for k in (PC.DUMBBELLS, PC.JACKS, PC.MIXED):  # terrain contacts on parts, pairs of bodies with a manifold of three records or more
        assert seen[k][1] > len(six[k]["compound"]["offsets"]) - 1, (k, seen[k])  # more terrain contacts than such bodies: several parts of one body
        assert seen[k][3] >= 3, (k, seen[k])
    assert seen[PC.JACKS][3] >= 4 and seen[PC.PILE][0] > 100 and seen[PC.ONE_JACK][1] >= 2 and seen[PC.EMPTY] == [0, 0, 0, 0], seen


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def test_six_worlds_against_the_lone_world(ctx, six):
    b = _batch(ctx, six)
    lone = [None if PC.n_bodies(sc) == 0 else _lone(ctx, sc) for sc in six]
    dt, iters = float(six[0]["dt"]), six[0]["iters"]
    multi = 0
    for tick in range(1, PC.TICKS + 1):
        st = b.step(dt, iters)
        for k, w in enumerate(lone):
            if w is None:
                assert st[k].n_bodies == 0 and st[k].n_constraints == 0
                continue
            lst = w.step(dt, iters)
            what = f"world {k} tick {tick}"
            PC.same_counts(st[k], lst, what)
            PC.same_state(b.state(k), w.state(), what)
            if tick in PC.LIST_TICKS:
                lc = w.constraints()
                compare_constraints(b.constraints(k), lc, check_impulse=True)
                multi = max(multi, PC.largest_manifold(lc))
                got, want = b.colliders(k), w.colliders()
                assert got.tobytes() == want.tobytes(), f"{what}: read_colliders differs"
    assert multi >= 3
    rows = b.colliders(PC.JACKS)   # the lone world's row for such a body: a radius-0 sphere at the centre of mass
    assert np.all(rows["tag"] == 0) and np.all(rows["r"] == 0.0)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_obstacle_worlds_against_the_oracle_and_the_lone_world(ctx):
    scs = PC.obstacle_scenes()
    plain = PC.run_against_oracle(_batch(ctx, [dict(sc, obstacles=[]) for sc in scs[:2]]), [oracle_world(sc) for sc in scs[:2]], scs[:2], 150, ())
    b = _batch(ctx, scs)
    seen = PC.run_against_oracle(b, PC.oracles(scs), scs, 150, PC.LIST_TICKS)
    print("terrain + obstacle contacts summed over 150 ticks, without and with the obstacles:", [p[2] for p in plain], [s[2] for s in seen])
    assert seen[0][2] > plain[0][2] + 500 and seen[1][2] > plain[1][2] + 500, (plain, seen)   # obstacle contacts on parts
    assert seen[2][2] > 100, seen   # no terrain there: every one of them is an obstacle's
    lb, lone = _batch(ctx, scs), [_lone(ctx, sc) for sc in scs]
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    for tick in range(1, 61):
        st = lb.step(dt, iters)
        for k, w in enumerate(lone):
            PC.same_counts(st[k], w.step(dt, iters), f"world {k} tick {tick}")
            PC.same_state(lb.state(k), w.state(), f"world {k} tick {tick}")
    for k, w in enumerate(lone):
        compare_constraints(lb.constraints(k), w.constraints(), check_impulse=True)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def test_a_world_computes_the_same_wherever_it_sits(ctx, six):
    import mgf_amd
    dt, iters, n = float(six[0]["dt"]), six[0]["iters"], 80
    base = _batch(ctx, six)
    st = base.step(dt, iters, n)
    assert max(st[t * 6 + PC.JACKS].n_constraints for t in range(n)) > 20
    rev = _batch(ctx, six[::-1])
    rev.step(dt, iters, n)
    for k in range(6):
        _same_world(rev, 5 - k, base, k, f"world {k} of the reversed batch")
    alone = _batch(ctx, [six[PC.JACKS]])
    alone.step(dt, iters, n)
    _same_world(alone, 0, base, PC.JACKS, "the jacks alone")
    many = _batch(ctx, [six[PC.JACKS]] * 64)
    many.step(dt, iters, n)
    whole, one = many.state(), base.state(PC.JACKS)
    for f in PC.STATE:
        assert bits_equal(whole[f], np.tile(one[f], (64, 1))), f
    assert many.counter("launches_per_tick") == alone.counter("launches_per_tick") == 7
    # single-part worlds through the new binding: today's batch, today's six kernels
    piles = [six[PC.PILE], scenes.sphere_pile(3, 3, 3, seed=9)]
    old = mgf_amd.WorldBatch.from_scenes(ctx, piles)
    new = mgf_amd.WorldBatch.from_scenes(ctx, [dict(sc, comps=sc["comps"][:0]) for sc in piles])
    for k, sc in enumerate(piles):
        m = len(sc["comps"])
        assert new.add_compound_bodies(k, sc["comps"], sc["mass"], np.arange(m + 1), sc["restitution"], sc["friction"], sc["force"]) == 0
        if sc.get("v0") is not None:
            new.write_state(k, v=sc["v0"])
    so, sn = old.step(dt, iters, 60), new.step(dt, iters, 60)
    assert new.counter("launches_per_tick") == 6
    for k in range(2):
        assert so[59 * 2 + k].n_constraints == sn[59 * 2 + k].n_constraints > 0
        _same_world(new, k, old, k, f"pile {k} through add_compound_bodies")
    assert len(new.raycast(0, [[0.0, 9.0, 0.0]], [[0.0, -1.0, 0.0]])) == 1   # (no body of several components: nothing is refused)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_a_tick_that_outgrows_its_share_is_run_again(ctx):
    import mgf_amd
    sc = scenes.dumbbell_field(4, 3, 4, n_plain=16)
    assert PC.n_bodies(sc) == 64
    b = mgf_amd.WorldBatch.from_scenes(ctx, [dict(sc, comps=sc["comps"][:0], compound=None, v0=None)], own_terrain=True)
    b.set_option("cons_per_body", 1)
    PC.fill_world(b, 0, sc)
    seen = PC.run_against_oracle(b, [oracle_world(sc)], [sc], 60, (1, 30, 60))
    print("most constraints:", seen[0][0], "capacity_retries:", b.counter("capacity_retries"))
    assert seen[0][0] > 64 and b.counter("capacity_retries") > 0


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_many_ticks_in_one_call_and_adding_behind_ticks(ctx, six):
    import mgf_amd
    dt, iters = float(six[0]["dt"]), six[0]["iters"]
    once, thirty = _batch(ctx, six), _batch(ctx, six)
    st = once.step(dt, iters, 30)
    for t in range(30):
        s1 = thirty.step(dt, iters)
        for k in range(6):
            PC.same_counts(st[t * 6 + k], s1[k], f"tick {t} world {k}")
    for k in range(6):
        _same_world(once, k, thirty, k, f"world {k}: one call of thirty ticks")
    # bodies added behind tick 20 into the middle world, interleaved with ordinary ones: the lone world given the same calls
    d, j = six[PC.DUMBBELLS], scenes.jack_field(2, 1, 2)
    trio = [six[PC.PILE], d, six[PC.ONE_JACK]]
    b, w = _batch(ctx, trio), _lone(ctx, d)
    for _ in range(20):
        b.step(dt, iters)
        w.step(dt, iters)
    cj = j["compound"]
    cj["comps"]["p"][:, 1] += f32(9.0)
    ball = scenes.sphere_pile(2, 1, 2)
    ball["comps"]["p"][:, 1] += f32(12.0)
    for target, add in ((b, lambda *a: b.add_compound_bodies(1, *a)), (w, w.add_compound_bodies)):
        assert add(cj["comps"][:8], cj["comp_mass"][:8], [0, 4, 8], 0.3, 0.6, [0, -9.8, 0]) == 22
    assert b.add_bodies(1, ball["comps"], 1.0, 0.3, 0.6, [0, -9.8, 0]) == w.add_bodies(ball["comps"], 1.0, 0.3, 0.6, [0, -9.8, 0]) == 24
    for target, add in ((b, lambda *a: b.add_compound_bodies(1, *a)), (w, w.add_compound_bodies)):
        assert add(cj["comps"][8:], cj["comp_mass"][8:], [0, 4, 8], 0.3, 0.6, [0, -9.8, 0]) == 28
    assert b.world_len(1) == len(w) == 30
    PC.same_state(b.state(1), w.state(), "behind the adds")
    most = 0
    for tick in range(100):
        st, lst = b.step(dt, iters), w.step(dt, iters)
        PC.same_counts(st[1], lst, f"tick {tick} behind the adds")
        PC.same_state(b.state(1), w.state(), f"tick {tick} behind the adds")
        most = max(most, int(lst.n_constraints))
    compare_constraints(b.constraints(1), w.constraints(), check_impulse=True)
    assert most > 30 and np.any(w.constraints()["a"] >= 22)   # the new bodies have landed on something


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------
def test_driving_and_observing(ctx, six):
    sc = six[PC.JACKS]
    dt, iters, n = float(sc["dt"]), sc["iters"], PC.n_bodies(sc)
    b, ow = _batch(ctx, [six[PC.PILE], sc]), oracle_world(sc)
    for _ in range(40):
        b.step(dt, iters)
        ow.step(dt, iters)
    # written poses move the parts from the next tick on
    s = ow.state()
    x = (s["x"] + f32([0.05, 0.3, -0.02])).astype(f32)
    q = s["q"][::-1].copy()
    b.write_state(1, x=x, q=q)
    ow.set_state(x=x, q=q)
    for tick in range(20):
        st, ost = b.step(dt, iters), ow.step(dt, iters)
        PC.same_counts(st[1], ost, f"tick {tick} behind write_state")
        PC.same_state(b.state(1), ow.state(), f"tick {tick} behind write_state")
    compare_constraints(b.constraints(1), ow.constraints(), check_impulse=True)
    assert PC.largest_manifold(ow.constraints()) >= 2 and ost.n_terrain_constraints > 0
    # body_contacts: the host fold of the list
    got, want = b.body_contacts(1), OC.fold(b.constraints(1), n)
    assert got.tobytes() == want.tobytes()
    # get / set_velocities against the oracle
    g, s = b.get(1, np.arange(n)), ow.state()
    assert bits_equal(g["linear"], s["v"]) and bits_equal(g["angular"], s["omega"]) and bits_equal(g["x"], (s["x"] + s["delta"]).astype(f32))
    assert np.allclose(1.0 / g["inv_mass"], 2.2, rtol=1e-6)   # a jack's mass is the sum of its components'
    bodies = [0, 5, 17]
    b.set_velocities(1, bodies, [0.5, 2.0, -0.25], [0.0, 1.5, 0.0])
    for i in bodies:
        ow.set_velocity(i, [0.5, 2.0, -0.25], [0.0, 1.5, 0.0])
    # apply_impulses: v += linear * inv_mass, omega += inv_moment * angular, in f32
    before = b.get(1, [3])
    b.apply_impulses(1, [3], [[0.0, 4.4, 0.0]], None)
    after = b.get(1, [3])
    want_v = (before["linear"][0] + f32([0.0, 4.4, 0.0]) * before["inv_mass"][0]).astype(f32)
    assert bits_equal(after["linear"][0], want_v) and bits_equal(after["angular"], before["angular"])
    ow.set_velocity(3, want_v, before["angular"][0])
    PC.same_state(b.state(1), ow.state(), "behind set_velocities and apply_impulses")
    for tick in range(10):   # ... and the ticks behind them
        st, ost = b.step(dt, iters), ow.step(dt, iters)
        what = f"tick {tick} behind set_velocities and apply_impulses"
        PC.same_counts(st[1], ost, what)
        PC.same_state(b.state(1), ow.state(), what)
        compare_constraints(b.constraints(1), ow.constraints(), check_impulse=True)
    # set_forces: from here on the world is the oracle's whose bodies were created under the new world force, its state set at the switch
    # (RigidBodyVec.force is world_force * mass, the mass of a jack the f32 sum of its components' in order)
    cb, wf = sc["compound"], f32([1.5, -9.8, 0.75])
    total = np.zeros(n, f32)
    for c in range(4):
        total = (total + cb["comp_mass"][c::4]).astype(f32)
    force = (wf[None, :] * total[:, None]).astype(f32)
    b.set_forces(1, np.arange(n), force=force)
    assert bits_equal(b.get(1, np.arange(n))["force"], force)
    ow2 = oracle_world(dict(sc, compound=dict(cb, force=np.tile(wf, (n, 1)))))
    ow2.set_state(**ow.state())
    most_t = most_m = 0
    for tick in range(30):
        st, ost = b.step(dt, iters), ow2.step(dt, iters)
        what = f"tick {tick} behind set_forces"
        # (the fresh oracle's fat boxes are those of its creation: the candidates and refits may differ, nothing else does)
        assert (st[1].n_constraints, st[1].n_terrain_constraints) == (ost.n_constraints, ost.n_terrain_constraints), what
        PC.same_state(b.state(1), ow2.state(), what)
        oc = ow2.constraints()
        compare_constraints(b.constraints(1), oc, check_impulse=True)
        most_t, most_m = max(most_t, int(ost.n_terrain_constraints)), max(most_m, PC.largest_manifold(oc))
    assert most_t > n and most_m >= 3, (most_t, most_m)   # terrain contacts on several parts of a body, a manifold of three records
    assert not bits_equal(ow2.state()["v"][:, 0], np.zeros(n, f32))   # (the sideways force did something)


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------------
def test_copying_a_world_of_jacks(ctx, six):
    import torch
    import mgf_amd
    sc = six[PC.JACKS]
    dt, iters, n = float(sc["dt"]), sc["iters"], PC.n_bodies(sc)
    pile18 = scenes.sphere_pile(3, 2, 3, seed=4)
    assert len(pile18["comps"]) == n
    src = _batch(ctx, [sc, dict(pile18, terrain=sc["terrain"]), dict(pile18, terrain=sc["terrain"]), sc])
    other = mgf_amd.WorldBatch.from_scenes(ctx, [dict(pile18, terrain=sc["terrain"]), dict(pile18, terrain=sc["terrain"])])
    st = src.step(dt, iters, 50)
    other.step(dt, iters, 50)
    assert st[49 * 4].n_constraints > 10 and other.counter("launches_per_tick") == 6
    src.copy_worlds([1], None, [0])                      # onto another world of the batch
    other.copy_worlds([1], src, [0])                     # into a batch that held single-part bodies only: it gets part storage
    assert other.counter("launches_per_tick") == 7
    mask = torch.tensor([1, 0], dtype=torch.int32, device="cuda")
    src.copy_worlds_where([2, 3], src, [0, 1], mask)     # under a device mask: world 2 becomes the jacks, world 3 stays what it is
    for what, bb, k in (("same batch", src, 1), ("second batch", other, 1), ("masked", src, 2)):
        _same_world(bb, k, src, 0, what)
        assert bb.colliders(k).tobytes() == src.colliders(0).tobytes(), what
    multi = 0
    for tick in range(30):
        s1, s2 = src.step(dt, iters), other.step(dt, iters)
        for what, ss, bb, k in (("same batch", s1, src, 1), ("second batch", s2, other, 1), ("masked", s1, src, 2), ("unmasked", s1, src, 3)):
            PC.same_counts(ss[k], s1[0], f"{what} tick {tick}")
            PC.same_state(bb.state(k), src.state(0), f"{what} tick {tick}")
        multi = max(multi, PC.largest_manifold(src.constraints(0)))
    for bb, k in ((src, 1), (other, 1), (src, 2)):
        compare_constraints(bb.constraints(k), src.constraints(0), check_impulse=True)
    assert multi >= 2 and s1[0].n_terrain_constraints > 0
    # a world of ordinary bodies copied over a clone of the jacks is ordinary again
    src.copy_worlds([2], other, [0])
    src.step(dt, iters)
    other.step(dt, iters)
    PC.same_state(src.state(2), other.state(0), "a pile copied over the jacks")


# ---- 9 ------------------------------------------------------------------------------------------------------------------------------------
def test_calls_that_read_shapes_are_refused(ctx, six):
    import torch
    import mgf_amd
    from mgf_amd import _capi
    sc = six[PC.JACKS]
    dt, iters = float(sc["dt"]), sc["iters"]
    parts, plain = _batch(ctx, [sc, six[PC.PILE]]), _batch(ctx, [six[PC.PILE], six[PC.PILE]])
    twin = _batch(ctx, [sc, six[PC.PILE]])
    dev = dict(device="cuda")
    i7, f7, f11, i13 = (torch.zeros((2, 7), dtype=torch.int32, **dev), torch.zeros((2, 7), dtype=torch.float32, **dev),
                        torch.zeros((2, 11), dtype=torch.float32, **dev), torch.zeros((2, 13), dtype=torch.int32, **dev))
    f7[:, 4], f11[:, 7] = -1.0, 0.3
    boxes, i3 = torch.ones((2, 6), dtype=torch.float32, **dev), torch.zeros((2, 3), dtype=torch.int32, **dev)
    depth = torch.zeros(4, dtype=torch.float32, **dev)
    for b in (parts, plain):   # the set_* calls of the rigs stay as they are
        b.step(dt, iters, 3)
        b.set_sensors([0, 1], [0, 0], [[0.0, 0.0, 0.0]], [[0.0, -1.0, 0.0]])
        b.set_cameras([dict(world=0, body=0, p=(0, 0, 0), tan_x=0.5, tan_y=0.5, width=2, height=2)])
        b.set_zones([0, 1], [0, 0], r=(1.0, 1.0, 1.0))
    sphere = np.zeros(1, scenes.COMPONENT_DTYPE)
    sphere["p"], sphere["r"] = (0.0, 5.0, 0.0), 0.3
    calls = {
        "raycast": lambda b: b.raycast(0, [[0.0, 9.0, 0.0]], [[0.0, -1.0, 0.0]]),
        "sweep": lambda b: b.sweep(0, sphere, [[0.0, -1.0, 0.0]]),
        "raycast_dev": lambda b: b.raycast_dev(None, f7, i7),
        "sweep_dev": lambda b: b.sweep_dev(None, f11, i13),
        "overlap_aabb": lambda b: b.overlap_aabb(0, [[-1.0, 0.0, -1.0]], [[1.0, 2.0, 1.0]]),
        "overlap_first_dev": lambda b: b.overlap_first_dev(boxes, i3),
        "cast_sensors": lambda b: b.cast_sensors(),
        "cast_sensors_dev": lambda b: b.cast_sensors_dev(i7),
        "cast_cameras": lambda b: b.cast_cameras(),
        "cast_cameras_dev": lambda b: b.cast_cameras_dev(depth=depth),
        "read_zones": lambda b: b.read_zones(2),
        "read_zones_dev": lambda b: b.read_zones_dev(i3),
    }
    for name, call in calls.items():
        with pytest.raises(mgf_amd.MgfError) as e:
            call(parts)
        assert e.value.status == _capi.ERR_INVALID and "several components" in str(e.value), name
        call(plain)   # the same call on a batch without such bodies
    torch.cuda.synchronize()
    twin.step(dt, iters, 3)
    parts.step(dt, iters)
    twin.step(dt, iters)
    for k in range(2):
        _same_world(parts, k, twin, k, f"world {k} behind the refused calls")


# ---- 10 -----------------------------------------------------------------------------------------------------------------------------------
def test_bodies_the_batch_does_not_take_add_nothing(ctx, six):
    import mgf_amd
    from mgf_amd import _capi
    sc = six[PC.JACKS]
    cb = sc["compound"]
    b, twin = _batch(ctx, [sc, six[PC.ONE_JACK]]), _batch(ctx, [sc, six[PC.ONE_JACK]])
    dt, iters = float(sc["dt"]), sc["iters"]
    b.step(dt, iters, 5)
    twin.step(dt, iters, 5)
    five = np.concatenate([cb["comps"][:4], cb["comps"][4:5]])
    one = np.zeros(1025, scenes.COMPONENT_DTYPE)
    one["p"][:, 0], one["r"] = 3.0 * np.arange(1025), 0.4
    bad = (("five components", lambda: b.add_compound_bodies(1, five, 1.0, [0, 5], 0.3, 0.6, [0, -9.8, 0]), "the batch takes four, the lone world 32"),
           ("no components", lambda: b.add_compound_bodies(1, cb["comps"][:4], 1.0, [0, 4, 4], 0.3, 0.6, [0, -9.8, 0]), "the batch takes four"),
           ("1025 bodies at once", lambda: b.add_compound_bodies(1, one, 1.0, np.arange(1026), 0.3, 0.6, [0, -9.8, 0]), "MGF_BATCH_MAX_BODIES"),
           ("1024 more bodies", lambda: b.add_compound_bodies(1, one[:1024], 1.0, np.arange(1025), 0.3, 0.6, [0, -9.8, 0]), "nothing was added"),
           ("a world out of range", lambda: b.add_compound_bodies(2, cb["comps"][:4], 1.0, [0, 4], 0.3, 0.6, [0, -9.8, 0]), "world index"))
    for what, call, msg in bad:
        with pytest.raises(mgf_amd.MgfError) as e:
            call()
        assert e.value.status == _capi.ERR_INVALID and msg in str(e.value), what
        assert [b.world_len(k) for k in range(2)] == [18, 1], what
    b.step(dt, iters, 5)
    twin.step(dt, iters, 5)
    for k in range(2):
        _same_world(b, k, twin, k, f"world {k} behind the refused adds")
