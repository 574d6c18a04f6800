"""Shared by the tests of a batch's body-mounted feelers (mgf_batch_set_feelers / _cast_feelers / _cast_feelers_dev), without a GPU: a
numpy restatement of the definition of a feeler's cast C, f32 operation by operation -
    shape   OWN_SHAPE: colliders(world)[body] as it stands;  else tag, r the record's, P = x + rotate(q, p), D = rotate(q, d)
    delta   WORLD_DELTA: the record's;  else rotate(q, delta)
with rotate tests/batch_sensor_cases.py's (tests/test_world_batch_feelers_host.py holds it to the oracle's mgfo_rotate_vector bit for
bit) - and the rigs of tests/test_gpu_world_batch_feelers.py: the worlds, which body of which world carries which kind of feeler (a
layout, from the scenes alone), and the records aimed from a stepped state."""
import numpy as np

from mgf_amd import scenes
from tests import batch_obstacle_cases as BC
from tests import batch_sensor_cases as SC

f32 = np.float32
IGNORE_SELF, WORLD_DELTA, OWN_SHAPE = 1, 2, 4
ALLOWED_FLAGS = (0, 1, 2, 3, 5, 7)      # OWN_SHAPE needs IGNORE_SELF
TICKS = SC.TICKS
offsets = SC.offsets

# what a feeler of a layout is for
RANDOM, DOWN, UP, RING, ZERO, OWN = range(6)


# ---- the definition -----------------------------------------------------------------------------------------------------------------------
def casts(rig, state, colliders, lengths):
    """the casts C of a rig (FEELER_DTYPE rows) from state(None) and colliders(None) of a batch whose worlds hold `lengths` bodies:
    MOVING_DTYPE rows"""
    from mgf_amd._capi import MOVING_DTYPE
    g = offsets(lengths)[rig["world"]] + rig["body"]
    x, q = np.ascontiguousarray(state["x"][g], f32), np.ascontiguousarray(state["q"][g], f32)
    own = (rig["flags"] & OWN_SHAPE) != 0
    world_delta = (rig["flags"] & WORLD_DELTA) != 0
    col = colliders[g]
    P, D = SC.particles(x, q, rig["p"], rig["d"])       # P = x + rotate(q, p), D = rotate(q, d): plain f32 operations
    c = np.zeros(len(rig), MOVING_DTYPE)
    c["tag"] = np.where(own, col["tag"], rig["tag"])
    c["r"] = np.where(own, col["r"], rig["r"])
    c["p"] = np.where(own[:, None], col["p"], P)
    c["d"] = np.where(own[:, None], col["d"], D)
    c["delta"] = np.where(world_delta[:, None], rig["delta"], SC.rotate(q, rig["delta"]))
    return c


def ignore_of(rig):
    return np.where(rig["flags"] & IGNORE_SELF, rig["body"], -1).astype(np.int32)


# ---- the worlds ---------------------------------------------------------------------------------------------------------------------------
TERRAIN_WORLD, ONE_BODY_WORLD, PILE_WORLD, BARE_WORLD, RING_WORLD = range(5)
FREE_RING = (BC.compounds()["ring"], (0.0, -1.5, 0.0), BC.IDENT)      # under the bodies of RING_WORLD, which fall: no tick meets it yet


def _capsuled(sc, k):
    """SC.twin_scenes' change of a pile: every third body a short capsule about the sphere's centre"""
    comps = sc["comps"].copy()
    cap = np.arange(len(comps)) % 3 == 1
    d = np.tile(f32([0.3, 0.2, -0.1]), (len(comps), 1)) * f32(1.0 + 0.1 * k)
    comps["tag"][cap] = 1
    comps["d"][cap] = d[cap]
    comps["p"][cap] -= f32(0.5) * d[cap]
    comps["r"][cap] = 0.4
    return dict(sc, comps=comps)


def feeler_scenes():
    """SC.twin_scenes() - 5 bodies over a box, one body over a box, 300 over a box and under the ring, capsules among them - then 48
    bodies with neither terrain nor obstacle, and 18 with no terrain and a ring below them"""
    scs = SC.twin_scenes()
    scs.append(dict(_capsuled(scenes.sphere_pile(4, 3, 4, seed=204), 3), terrain=None))
    scs.append(dict(_capsuled(scenes.sphere_pile(3, 2, 3, seed=205), 4), terrain=None, obstacles=[FREE_RING]))
    return scs


# ---- layouts: (world, body, role) from the scenes alone -----------------------------------------------------------------------------------
def _world_layout(rng, sc, n_random=0, n_down=0, n_up=0, n_ring=0, n_zero=0, n_own=0, four_on_one=False):
    nb = len(sc["comps"])
    y = SC.centres(sc)[:, 1]
    bottom, top = np.flatnonzero(y < 1.0), np.flatnonzero(y > y.max() - 0.5)
    body, role = [], []
    for pool, count, r in ((bottom, n_down, DOWN), (top, n_up, UP), (top, n_ring, RING), (np.arange(nb), n_zero, ZERO), (np.arange(nb), n_own, OWN)):
        body += rng.choice(pool, count, replace=count > len(pool)).tolist(); role += [r] * count
    if four_on_one:
        body += [int(rng.integers(0, nb))] * 4; role += [RANDOM] * 4
    rest = n_random - (4 if four_on_one else 0)
    body += rng.integers(0, nb, rest).tolist(); role += [RANDOM] * rest
    return np.int32(body), np.int32(role)


def main_layout(scs, seed=95):
    """about a thousand feelers over all five worlds in one shuffled order: 704 on the pile of 300 (three work items), 24 on the lone
    body"""
    per_world = [dict(n_random=40, n_down=20, n_up=10, n_zero=6, n_own=20),
                 dict(n_random=8, n_down=8, n_zero=2, n_own=6),
                 dict(n_random=500, n_down=60, n_up=40, n_ring=30, n_zero=14, n_own=60, four_on_one=True),
                 dict(n_random=60, n_up=20, n_zero=6, n_own=14),
                 dict(n_random=30, n_ring=30, n_zero=4, n_own=12)]
    rng = np.random.default_rng(seed)
    W, B, R = [], [], []
    for k, args in enumerate(per_world):
        b, r = _world_layout(rng, scs[k], **args)
        W.append(np.full(len(b), k, np.int32)); B.append(b); R.append(r)
    W, B, R = np.concatenate(W), np.concatenate(B), np.concatenate(R)
    perm = rng.permutation(len(W))
    lay = dict(world=W[perm], body=B[perm], role=R[perm])
    assert np.bincount(lay["world"], minlength=5).tolist() == [96, 24, 704, 100, 76]
    return lay


def plan_layout(scs, seed=96):
    """SC.PLAN_COUNTS feelers a world - 0, 1, 256, 257, 600 - in one shuffled order, any body, any role but RING"""
    rng = np.random.default_rng(seed)
    world = SC.plan_worlds(seed)
    n = [len(sc["comps"]) for sc in scs]
    body = np.int32([rng.integers(0, n[w]) for w in world])
    role = rng.choice([RANDOM, RANDOM, ZERO, OWN], len(world)).astype(np.int32)
    return dict(world=world, body=body, role=role)


# ---- records aimed from a state -----------------------------------------------------------------------------------------------------------
def aimed_rig(layout, scs, state, lengths, seed=97):
    """FEELER_DTYPE rows for the layout, aimed as SC.aimed_rig aims rays.  i counts the feelers; tags alternate with i.
    DOWN leaves the body's centre straight down by 1.5, a thin shape that ignores its own body (flags 1, or 3 with the delta given in
    world coordinates); UP goes half a unit up from a body of the top layer; RING comes down by 3 from 3 above a sphere of the world's
    ring (the pile's ring hangs under the box's ceiling: there a sphere from 0.85 above, by 1); ZERO has no delta, at the body's centre, with and
    without the flag; OWN is the body's own collider moved by up to one unit (flags 5 or 7), tag, p, d and r garbage that is not read;
    RANDOM starts near the body and goes any way, every combination of IGNORE_SELF and WORLD_DELTA"""
    from mgf_amd._capi import FEELER_DTYPE
    rng = np.random.default_rng(seed)
    off = offsets(lengths)
    n = len(layout["world"])
    rig = np.zeros(n, FEELER_DTYPE)
    rig["world"], rig["body"] = layout["world"], layout["body"]
    for i, (w, bd, role) in enumerate(zip(layout["world"], layout["body"], layout["role"])):
        g = off[w] + bd
        x, q = state["x"][g].astype(np.float64), state["q"][g]
        local = lambda v: SC._unrotate(q, v)            # the local vector whose image is v
        tag, p, d, r, delta, flags = i % 2, np.zeros(3), local(rng.normal(0, 1, 3)) * 0.1, 0.1, np.zeros(3), IGNORE_SELF
        if role == DOWN:
            flags = IGNORE_SELF | (WORLD_DELTA if i % 4 < 2 else 0)
            delta = np.array([0.0, -1.5, 0.0]) if flags & WORLD_DELTA else local((0.0, -1.5, 0.0))
            d = local((0.1, 0.0, 0.05))
        elif role == UP:
            flags = IGNORE_SELF | WORLD_DELTA
            p, delta = local((0.0, 0.7, 0.0)), np.array([0.0, 0.5, 0.0])
        elif role == RING:
            ring = SC.ring_of(scs[w])
            tgt = ring[int(rng.integers(0, len(ring)))]
            boxed = scs[w]["terrain"] is not None
            high, far = (0.85, 1.0) if boxed else (3.0, 3.0)
            if boxed:
                tag = 0                                 # (a capsule within a unit of a face meets it at t = 0: q_sweep_terrain's `reach`)
            start = tgt + np.array([rng.uniform(-0.1, 0.1), high, rng.uniform(-0.1, 0.1)])
            p, d = local(start - x), local((0.05, 0.0, 0.05))
            flags = IGNORE_SELF | (WORLD_DELTA if i % 4 < 2 else 0)
            delta = np.array([0.0, -far, 0.0]) if flags & WORLD_DELTA else local((0.0, -far, 0.0))
        elif role == ZERO:
            r, flags = 0.3, (IGNORE_SELF if i % 4 < 2 else 0)
        elif role == OWN:
            flags = OWN_SHAPE | IGNORE_SELF | (WORLD_DELTA if i % 4 < 2 else 0)
            tag, p, d, r = 77, rng.normal(0, 9, 3), rng.normal(0, 9, 3), -3.0
            delta = rng.normal(0, 1, 3)
            delta *= rng.uniform(0.2, 1.0) / np.linalg.norm(delta)
        elif role == RANDOM:
            p = rng.uniform(-0.3, 0.3, 3)
            d = rng.normal(0, 1, 3) * 0.15
            r = rng.uniform(0.05, 0.3)
            delta = rng.normal(0, 1, 3)
            delta *= rng.uniform(0.5, 3.0) / np.linalg.norm(delta)
            flags = (i // 2) % 4                        # 0, 1, 2, 3 under both tags
        rig["tag"][i], rig["p"][i], rig["d"][i], rig["r"][i], rig["delta"][i], rig["flags"][i] = tag, p, d, r, delta, flags
    return rig
