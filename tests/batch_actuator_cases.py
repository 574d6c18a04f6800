"""Shared by the tests of a batch's body-mounted actuators (mgf_batch_set_actuators / _actuate / _actuate_dev), without a GPU: a numpy
restatement of the header's definition of an actuator's wrench, f32 operation by operation -
    c = u; if (c < lo) c = lo; if (c > hi) c = hi;   s = gain * c;   e = WORLD_DIR ? d : rotate(q, d)
    TORQUE: L = 0, A = e * s;   otherwise: L = e * s, r = rotate(q, p), A = cross(r, L);   s not finite: L = A = 0, skipped
(tests/test_world_batch_actuators_host.py holds it to the oracle's mgfo_rotate_vector bit for bit; rotate and cross are
tests/batch_sensor_cases.py's) - the restated sequential adds of the force mode, and the scenes, the rig and the controls of
tests/test_gpu_world_batch_actuators.py, from the scenes alone."""
import numpy as np

from mgf_amd import _capi, scenes
from tests import batch_sensor_cases as SC

f32 = np.float32
TORQUE, WORLD_DIR = 1, 2
IMPULSE, FORCE = 0, 1
TICKS = SC.TICKS
INF = f32(np.inf)


# ---- the definition -----------------------------------------------------------------------------------------------------------------------
def wrenches(rig, u, q):
    """(W, skipped): W[i] = (L, A) of actuator i of `rig` (ACTUATOR_DTYPE rows) under the control u[i] on a body turned by q[i] - rows of
    f32, every operation a rounded f32 operation of its own, in the header's order; skipped[i]: gain * clamp(u) was not finite"""
    n = len(rig)
    u, q = np.ascontiguousarray(u, f32).reshape(n), np.ascontiguousarray(q, f32).reshape(n, 4)
    lo, hi, gain = rig["lo"].astype(f32), rig["hi"].astype(f32), rig["gain"].astype(f32)
    with np.errstate(all="ignore"):
        c = u.copy()
        c = np.where(c < lo, lo, c)                     # (a NaN compares false: it stays)
        c = np.where(c > hi, hi, c)
        s = (gain * c).astype(f32)
        world_dir, torque = (rig["flags"] & WORLD_DIR) != 0, (rig["flags"] & TORQUE) != 0
        e = np.where(world_dir[:, None], rig["d"].astype(f32), SC.rotate(q, rig["d"]))
        es = (e * s[:, None]).astype(f32)
        r = SC.rotate(q, rig["p"])
        L = np.where(torque[:, None], f32(0.0), es)
        A = np.where(torque[:, None], es, SC._cross(r, es))
    skipped = ~np.isfinite(s)
    W = np.concatenate([L, A], axis=1).astype(f32)
    W[skipped] = 0.0
    assert W.dtype == f32 and W.shape == (n, 6)
    return W, skipped


def rig_wrenches(rig, u, state, lengths):
    """wrenches of a rig from state(None) of a batch whose worlds hold `lengths` bodies"""
    g = SC.offsets(lengths)[rig["world"]] + rig["body"]
    return wrenches(rig, u, state["q"][g])


def forces_expected(before, world, body, W):
    """the force mode's definition on `before` = get() of the same records taken just before the call: per body, its records in array
    order, force = force + L, torque = torque + A.  Returns the UNIQUE (world, body) in order of first appearance and their rows:
    what set_forces of them writes."""
    cur, keys = {}, []
    for k in range(len(world)):
        key = (int(world[k]), int(body[k]))
        if key not in cur:
            cur[key] = (before["force"][k].astype(f32), before["torque"][k].astype(f32))
            keys.append(key)
        f, t = cur[key]
        cur[key] = ((f + W[k, 0:3]).astype(f32), (t + W[k, 3:6]).astype(f32))
    uw, ub = np.int32([k[0] for k in keys]), np.int32([k[1] for k in keys])
    return uw, ub, np.array([cur[k][0] for k in keys], f32).reshape(-1, 3), np.array([cur[k][1] for k in keys], f32).reshape(-1, 3)


# ---- the scenes ---------------------------------------------------------------------------------------------------------------------------
FIELD_WORLD, BARE_WORLD, ONE_WORLD, PILE_WORLD, LATE_WORLD = range(5)
COUNTS = (257, 0, 1)                # the actuators of FIELD_WORLD, BARE_WORLD, ONE_WORLD
LATE_BODIES = 2                     # bodies added to LATE_WORLD behind the ticks
FOUR_ON = (PILE_WORLD, 7)           # the body that carries four actuators, far apart in the caller's array


def actuator_scenes():
    """48 capsules over a heightfield (they tumble: q leaves the identity), 8 spheres no actuator names, 18 capsules with one
    actuator, a pile of 64 spheres, and 8 spheres that get two more bodies behind the ticks"""
    return [scenes.capsule_field(4, 3, 4), scenes.sphere_pile(2, 2, 2, seed=41), scenes.capsule_field(3, 2, 3, seed=42),
            scenes.sphere_pile(4, 4, 4, seed=43), scenes.sphere_pile(2, 2, 2, seed=44)]


def late_bodies(sc):
    """what is added to LATE_WORLD behind the ticks: two copies of its first body, above the pile"""
    comps = sc["comps"][:1].repeat(LATE_BODIES)
    comps["p"] += f32([[0.0, 4.0, 0.0], [0.0, 5.5, 0.0]])
    return comps, 1.0, float(sc["restitution"][0]), float(sc["friction"][0]), sc["force"][:1].repeat(LATE_BODIES, axis=0)


def main_rig(lengths, seed=131):
    """(rig, u, planted): about 450 actuators in one seeded shuffle of all worlds - COUNTS, 120 on the pile and four more on FOUR_ON,
    70 on LATE_WORLD with both added bodies among them - every flag word, gains of both signs, clamps that bite from both sides, controls
    of zero, and `planted` actuators whose gain * clamp(u) is not finite: an overflow, a NaN control, an infinite one without a clamp"""
    rng = np.random.default_rng(seed)
    world, body = [], []
    for k, cnt in ((FIELD_WORLD, COUNTS[0]), (ONE_WORLD, COUNTS[2]), (PILE_WORLD, 120), (LATE_WORLD, 70)):
        world.append(np.full(cnt, k, np.int32))
        body.append(rng.integers(0, lengths[k], cnt).astype(np.int32))
    body[-1][:2 * LATE_BODIES] = np.repeat(np.arange(lengths[LATE_WORLD] - LATE_BODIES, lengths[LATE_WORLD]), 2)
    body[2][body[2] == FOUR_ON[1]] = FOUR_ON[1] + 1
    world, body = np.concatenate(world), np.concatenate(body)
    order = rng.permutation(len(world))
    world, body = world[order], body[order]
    at = np.int64([3, len(world) // 3, 2 * len(world) // 3, len(world)])       # the four on one body, other bodies' between them
    world, body = np.insert(world, at, FOUR_ON[0]).astype(np.int32), np.insert(body, at, FOUR_ON[1]).astype(np.int32)
    n = len(world)
    rig = np.zeros(n, _capi.ACTUATOR_DTYPE)
    rig["world"], rig["body"] = world, body
    rig["flags"] = rng.integers(0, 4, n)
    rig["flags"][np.flatnonzero((world == FOUR_ON[0]) & (body == FOUR_ON[1]))] = [0, 1, 2, 3]
    rig["gain"] = rng.uniform(0.2, 3.0, n) * rng.choice([1.0, -1.0], n)
    rig["p"] = rng.uniform(-0.6, 0.6, (n, 3))
    d = rng.normal(0, 1, (n, 3))
    rig["d"] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rig["lo"], rig["hi"] = -np.inf, np.inf
    clamp = rng.random(n) < 0.5
    rig["lo"][clamp], rig["hi"][clamp] = -rng.uniform(0.1, 0.8, int(clamp.sum())), rng.uniform(0.1, 0.8, int(clamp.sum()))
    u = rng.uniform(-1.5, 1.5, n).astype(f32)
    u[rng.random(n) < 0.08] = 0.0
    free = np.flatnonzero(~clamp)
    over, nan, inf = free[5], np.flatnonzero(clamp)[5], free[9]
    rig["gain"][over], u[over] = 3.0e38, 2.0             # gain * c overflows
    u[nan] = np.nan                                       # a NaN goes through the clamp as a NaN
    u[inf] = -np.inf                                      # no clamp: gain * -inf
    return rig, u, [int(over), int(nan), int(inf)]


def dumbbell_rig(n_bodies, seed=137):
    """40 actuators on a world of plain spheres and dumbbells, every flag word"""
    rng = np.random.default_rng(seed)
    n = 40
    rig = np.zeros(n, _capi.ACTUATOR_DTYPE)
    rig["body"] = rng.integers(0, n_bodies, n)
    rig["body"][:2] = n_bodies - 1                        # a dumbbell (the bodies of two parts come last), twice
    rig["flags"] = np.arange(n) % 4
    rig["gain"] = rng.uniform(-2.0, 2.0, n)
    rig["p"], rig["d"] = rng.uniform(-0.6, 0.6, (n, 3)), rng.normal(0, 1, (n, 3))
    rig["lo"], rig["hi"] = -1.0, 1.0
    return rig, rng.uniform(-1.5, 1.5, n).astype(f32)
