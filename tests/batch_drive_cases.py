"""Shared inputs of the tests of driving a batch (mgf_batch_get_many / _set_many / _set_forces / _apply_impulses / _copy_worlds):
test_world_batch_drive_host.py checks on the oracle alone that they are not trivial, test_gpu_world_batch_drive.py runs them."""
import numpy as np

from mgf_amd import scenes
from tests import np_restatement as NP
from tests.util import oracle_world

STATE = ("x", "q", "v", "omega", "delta")
# a world force per world of drive_scenes(); the bundled scenes have mass 1, so force = world_force * mass is exact
WORLD_FORCES = np.float32([[0.0, -9.8, 0.0], [1.5, -9.8, 0.0], [-1.0, -12.0, 0.5], [0.0, -6.5, -2.0], [2.0, -9.0, 1.0], [0.5, -11.0, -0.75]])
SWITCH_FORCE = np.float32([3.0, -9.81, 1.5])   # what every third body gets at tick 40
SWITCH_TICK, SWITCH_RUN = 40, 20
FAN_K, FAN_TICKS, FAN_RUN = 300, 20, 15


def drive_scenes():
    """five piles of 64 spheres (different seeds) and a field of 48 capsules over a heightfield, each with its scene's default force"""
    return [scenes.sphere_pile(4, 4, 4, seed=100 + k) for k in range(5)] + [scenes.capsule_field(4, 3, 4)]


def with_force(sc, force):
    """the scene with the given world force: one vector for all bodies, or a row a body"""
    n = len(sc["comps"])
    return dict(sc, force=np.ascontiguousarray(np.broadcast_to(np.asarray(force, np.float32), (n, 3))))


def all_bodies(scs, seed):
    """one record per body of every world, shuffled: (world, body)"""
    world = np.concatenate([np.full(len(sc["comps"]), k, np.int32) for k, sc in enumerate(scs)])
    body = np.concatenate([np.arange(len(sc["comps"]), dtype=np.int32) for sc in scs])
    order = np.random.default_rng(seed).permutation(len(world))
    return world[order], body[order]


def switched(scs):
    """the switch of test 2: every third body of every world, shuffled"""
    world, body = all_bodies(scs, 7)
    keep = body % 3 == 0
    return world[keep], body[keep]


def switched_force(sc, k):
    """world k's per-body world force after the switch"""
    f = np.tile(WORLD_FORCES[k], (len(sc["comps"]), 1))
    f[::3] = SWITCH_FORCE
    return f


def random_pairs(scs, count, seed):
    rng = np.random.default_rng(seed)
    world = rng.integers(0, len(scs), count).astype(np.int32)
    body = np.array([rng.integers(0, len(scs[k]["comps"])) for k in world], np.int32)
    return world, body


def velocity_commands(scs, seed=19):
    """the set_many of test 4: 150 records over all worlds, 30 of them naming a body again with another velocity"""
    rng = np.random.default_rng(seed)
    world, body = random_pairs(scs, 120, seed)
    again = rng.integers(0, 120, 30)
    world, body = np.concatenate([world, world[again]]), np.concatenate([body, body[again]])
    order = rng.permutation(len(world))
    world, body = world[order], body[order]
    lin = rng.uniform(-2.0, 2.0, (len(world), 3)).astype(np.float32)
    ang = rng.uniform(-3.0, 3.0, (len(world), 3)).astype(np.float32)
    return world, body, lin, ang


def impulse_records(scs, seed=23):
    """the apply_impulses of test 5: records of different worlds interleaved, body 5 of world 2 named three times"""
    rng = np.random.default_rng(seed)
    world, body = random_pairs(scs, 90, seed)
    world, body = np.concatenate([world, np.int32([2, 2, 2])]), np.concatenate([body, np.int32([5, 5, 5])])
    order = rng.permutation(len(world))
    world, body = world[order], body[order]
    lin = rng.uniform(-1.5, 1.5, (len(world), 3)).astype(np.float32)
    ang = rng.uniform(-2.0, 2.0, (len(world), 3)).astype(np.float32)
    return world, body, lin, ang


def impulses_expected(before, world, body, lin, ang):
    """the header's definition in numpy f32 on `before` = get() of the same records taken just before the call: per body, its records
    in array order, v = v + linear * inv_mass, omega = omega + I * angular with I * a = (c0 * a.x + c1 * a.y) + c2 * a.z.  Returns
    (linear, angular) per record: what get() of the same records returns after the call."""
    cur = {}
    for k in range(len(world)):
        key = (int(world[k]), int(body[k]))
        if key not in cur:
            cur[key] = (before["linear"][k].copy(), before["angular"][k].copy())
        v, w = cur[key]
        im, I = before["inv_mass"][k], before["inv_moment"][k].reshape(3, 3)   # (rows of the reshape = columns c0, c1, c2)
        v = v + lin[k] * im
        w = w + ((I[0] * ang[k][0] + I[1] * ang[k][1]) + I[2] * ang[k][2])
        cur[key] = (v.astype(np.float32), w.astype(np.float32))
    out_v = np.array([cur[(int(world[k]), int(body[k]))][0] for k in range(len(world))], np.float32)
    out_w = np.array([cur[(int(world[k]), int(body[k]))][1] for k in range(len(world))], np.float32)
    return out_v, out_w


# ---- test 3: torque in free flight ----------------------------------------------------------------------------------------------------------
TORQUE_TICKS = 30


def torque_scenes():
    """4 worlds of 8 bodies far apart and without terrain: spheres and capsules alternating, capsule axes off the coordinate axes"""
    out = []
    for k in range(4):
        rng = np.random.default_rng(300 + k)
        comps = np.zeros(8, scenes.sphere_pile(1, 1, 1)["comps"].dtype)
        comps["tag"] = np.arange(8) % 2
        comps["p"] = (np.arange(8)[:, None] * np.float32([25.0, 0.0, 0.0]) + rng.uniform(-1, 1, (8, 3))).astype(np.float32)
        d = rng.normal(0, 1, (8, 3))
        d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.8, 1.6, (8, 1))
        comps["d"] = np.where(comps["tag"][:, None] == 1, d, 0.0).astype(np.float32)
        comps["r"] = rng.uniform(0.3, 0.6, 8).astype(np.float32)
        sc = scenes.sphere_pile(2, 2, 2)
        omega0 = rng.uniform(-2.0, 2.0, (8, 3)).astype(np.float32)
        out.append(dict(sc, name="torque", comps=comps, terrain=None, v0=rng.uniform(-1, 1, (8, 3)).astype(np.float32), omega0=omega0,
                        force=np.tile(np.float32([0.0, -1.0, 0.25]), (8, 1))))
    return out


def torque_schedule(k):
    """world k: {tick before which the call is made: (bodies, torques)} - half the bodies at 0, other values at 10, zero at 20"""
    rng = np.random.default_rng(400 + k)
    bodies = np.int32([1, 2, 5, 7]) if k % 2 == 0 else np.int32([0, 3, 4, 5])
    return {0: (bodies, rng.uniform(-4.0, 4.0, (4, 3)).astype(np.float32)),
            10: (bodies, rng.uniform(-4.0, 4.0, (4, 3)).astype(np.float32)),
            20: (bodies, np.zeros((4, 3), np.float32))}


def torque_restatement(state0, got0, schedule, dt, ticks=TORQUE_TICKS):
    """np_restatement.Bodies seeded from the batch's tick-0 state and get()'s inv_moment (= the body inertia before a tick) and force,
    stepped `ticks` times free (complete_motion + integrate, physics.rs:222-269) under the torque schedule; returns the state per tick"""
    B = NP.Bodies(state0["x"], state0["q"], state0["v"], state0["omega"], state0["delta"], got0["force"], got0["inv_mass"], got0["inv_moment"],
                  got0["restitution"], got0["friction"])
    B.torque = list(B.torque)
    out = []
    for t in range(ticks):
        if t in schedule:
            for i, tq in zip(*schedule[t]):
                B.torque[int(i)] = NP.vec(tq)
        B.complete_motion()
        B.integrate(dt)
        out.append({f: np.array(getattr(B, f), np.float32) for f in STATE})
    return out


# ---- test 7: fan-out ------------------------------------------------------------------------------------------------------------------------
def fan_scene():
    return scenes.sphere_pile(2, 3, 2)


def fan_impulses(K=FAN_K):
    """world k's own kick: (body, linear, angular)"""
    rng = np.random.default_rng(55)
    n = len(fan_scene()["comps"])
    return rng.integers(0, n, K).astype(np.int32), rng.uniform(-3, 3, (K, 3)).astype(np.float32), rng.uniform(-3, 3, (K, 3)).astype(np.float32)


# ---- oracle runs shared by the tests ----------------------------------------------------------------------------------------------------------
def run_oracles(scs, ticks, list_ticks=()):
    """one oracle world per scene stepped `ticks` times: the worlds, and per world and tick (counts, state), the lists at list_ticks"""
    ows = [oracle_world(sc) for sc in scs]
    hist = [[] for _ in scs]
    lists = [{} for _ in scs]
    for t in range(1, ticks + 1):
        for k, (sc, ow) in enumerate(zip(scs, ows)):
            st = ow.step(float(sc["dt"]), sc["iters"])
            hist[k].append(((int(st.n_constraints), int(st.n_terrain_constraints), int(st.n_pair_candidates), int(st.n_refits)), ow.state()))
            if t in list_ticks:
                lists[k][t] = ow.constraints()
    return ows, hist, lists
