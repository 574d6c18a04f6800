"""Shared by the tests of a batch's body-mounted ray sensors (mgf_batch_set_sensors / _cast_sensors / _cast_sensors_dev), without a GPU:
a numpy restatement of the definition, f32 operation by operation -
    P = x + rotate(q, p)      D = rotate(q, d)      rotate(q, r): tmp = v x r + r * s; (v x tmp) * 2 + r
(tests/test_world_batch_sensors_host.py holds it to the oracle's mgfo_rotate_vector bit for bit) - and the rigs of
tests/test_gpu_world_batch_sensors.py: which body of which world carries which kind of sensor (a layout, from the scenes alone), and
the records aimed from a state."""
import numpy as np

from tests import batch_device_cases as DV
from tests import batch_obstacle_cases as BC
from tests import batch_query_device_cases as QD

f32 = np.float32
IGNORE_SELF = 1
TICKS = 3

# what a sensor of a layout is for
RANDOM, DOWN, UP, RING, ZERO, SHORT, SELF_IGNORED, SELF_SEEN = range(8)


# ---- the definition -----------------------------------------------------------------------------------------------------------------------
def _cross(a, b):
    """cgmath Vector3::cross, rows of f32: every product and every difference a rounded f32 operation of its own"""
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def rotate(q, r):
    """Rotation::rotate_vector for rows q = (s, x, y, z) and r, in f32: tmp = v x r + r * s; (v x tmp) * 2 + r"""
    q, r = np.ascontiguousarray(q, f32).reshape(-1, 4), np.ascontiguousarray(r, f32).reshape(-1, 3)
    s, v = q[:, 0:1], q[:, 1:4]
    tmp = _cross(v, r) + r * s
    out = _cross(v, tmp) * f32(2.0) + r
    assert out.dtype == f32
    return out


def particles(x, q, p, d):
    """(P, D) of sensors with local p, d on bodies at x, q: P = x + rotate(q, p), D = rotate(q, d), rows of f32"""
    x = np.ascontiguousarray(x, f32).reshape(-1, 3)
    return x + rotate(q, p), rotate(q, d)


def offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def rig_particles(rig, state, lengths):
    """the particles of a rig (SENSOR_DTYPE rows) from state(None) of a batch whose worlds hold `lengths` bodies: (P, D, dt)"""
    g = offsets(lengths)[rig["world"]] + rig["body"]
    P, D = particles(state["x"][g], state["q"][g], rig["p"], rig["d"])
    return P, D, rig["dt"].astype(f32)


def ignore_of(rig):
    return np.where(rig["flags"] & IGNORE_SELF, rig["body"], -1).astype(np.int32)


# ---- the scenes ---------------------------------------------------------------------------------------------------------------------------
TWIN_RING = (BC.compounds()["ring"], (0.0, 3.5, 0.0), BC.IDENT)   # over the pile of 10 x 3 x 10, whose top ends near y = 3.3
TWIN_RING_WORLD = 2


def twin_scenes():
    """DV.device_scenes() - worlds of 5, 1 and 300 bodies (300: the smallest count that crosses the 256-lane cut of the staging loop) -
    with every third body a short capsule about the sphere's centre (its q is not the identity even before a tick), and a ring of
    obstacle spheres above the largest pile"""
    scs = []
    for k, sc in enumerate(DV.device_scenes()):
        comps = sc["comps"].copy()
        cap = np.arange(len(comps)) % 3 == 1
        d = np.tile(f32([0.3, 0.2, -0.1]), (len(comps), 1)) * f32(1.0 + 0.1 * k)
        comps["tag"][cap] = 1
        comps["d"][cap] = d[cap]
        comps["p"][cap] -= f32(0.5) * d[cap]
        comps["r"][cap] = 0.4
        scs.append(dict(sc, comps=comps))
    scs[TWIN_RING_WORLD] = dict(scs[TWIN_RING_WORLD], obstacles=[TWIN_RING])
    return scs


def centres(sc):
    c = sc["comps"]
    return c["p"].astype(np.float64) + 0.5 * c["d"].astype(np.float64) * (c["tag"] == 1)[:, None]


def ring_of(sc):
    """the centres of the components of the scene's first obstacle (to aim at), or None"""
    return BC.component_centres(sc["obstacles"][:1]) if sc.get("obstacles") else None


# ---- layouts: (world, body, role) from the scenes alone -----------------------------------------------------------------------------------
def _layers(sc):
    """bodies of the bottom and of the top layer of a pile, by where they were added"""
    y = centres(sc)[:, 1]
    return np.flatnonzero(y < 1.0), np.flatnonzero(y > y.max() - 0.5)


def _world_layout(rng, sc, n_random, n_down=0, n_up=0, n_ring=0, special=False):
    nb = len(sc["comps"])
    bottom, top = _layers(sc)
    spheres = np.flatnonzero(sc["comps"]["tag"] == 0)
    body, role = [], []
    body += rng.choice(bottom, n_down, replace=False).tolist(); role += [DOWN] * n_down
    body += rng.choice(top, n_up, replace=False).tolist(); role += [UP] * n_up
    body += rng.choice(top, n_ring, replace=n_ring > len(top)).tolist(); role += [RING] * n_ring
    if special:
        one = int(rng.integers(0, nb))
        body += [one] * 4; role += [RANDOM] * 4                      # four on one body
        s = int(rng.choice(spheres))                                   # (a ray that starts inside a sphere meets it at t = 0)
        body += [int(rng.integers(0, nb)), int(rng.integers(0, nb)), s, s]
        role += [ZERO, SHORT, SELF_IGNORED, SELF_SEEN]
    rest = n_random - (6 + 2 if special else 0)
    body += rng.integers(0, nb, rest).tolist(); role += [RANDOM] * rest
    return np.int32(body), np.int32(role)


def _layout(scs, per_world, seed):
    """per_world[k]: None (no sensor) or the arguments of _world_layout; the sensors of all worlds in one shuffled order"""
    rng = np.random.default_rng(seed)
    W, B, R = [], [], []
    for k, args in enumerate(per_world):
        if args is None:
            continue
        b, r = _world_layout(rng, scs[k], **args)
        W.append(np.full(len(b), k, np.int32)); B.append(b); R.append(r)
    W, B, R = np.concatenate(W), np.concatenate(B), np.concatenate(R)
    perm = rng.permutation(len(W))
    return dict(world=W[perm], body=B[perm], role=R[perm])


def twin_layout(scs):
    """none on world 0, one on the world of one body, 257 on the world of 300 - the cut between two work items: 12 at the ring, 10 down,
    10 up, four on one body, one with d = 0, one too short, the pair at their own body's centre, the rest any way"""
    lay = _layout(scs, [None, dict(n_random=1), dict(n_random=257 - 32, n_down=10, n_up=10, n_ring=12, special=True)], seed=91)
    assert np.bincount(lay["world"], minlength=3).tolist() == [0, 1, 257]
    return lay


def pile_layout(scs):
    """QD.pile_scenes(): 1, 96 (under the obstacle ring), 512, 0 and 1024 spheres.  Two sensors on the lone body, 42 under the ring (12 at
    it), 60 on the 512, none on the world without bodies, 320 on the 1024 (two work items)"""
    lay = _layout(scs, [dict(n_random=2), dict(n_random=20, n_down=10, n_ring=12), dict(n_random=40, n_down=10, n_up=10), None,
                        dict(n_random=300, n_down=10, n_up=10, special=True)], seed=92)
    assert np.bincount(lay["world"], minlength=5).tolist() == [2, 42, 60, 0, 320]
    return lay


# ---- records aimed from a state -----------------------------------------------------------------------------------------------------------
def _unrotate(q, v):
    """rotate(conjugate(q), v) in f64: about the local vector whose image is v (an input of the test, not a reference)"""
    q, v = np.asarray(q, np.float64), np.asarray(v, np.float64)
    s, u = q[0], -q[1:4]
    tmp = np.cross(u, v) + v * s
    return np.cross(u, tmp) * 2.0 + v


def aimed_rig(layout, scs, state, lengths, seed=93):
    """SENSOR_DTYPE rows for the layout: DOWN / UP leave the body's centre straight down / up, RING leaves a point three above a sphere of the
    ring, almost straight down at it - all three ignore their own body; ZERO has d = 0, SHORT ends a centimetre from its
    body's centre, the SELF pair starts at the centre with and without the flag; RANDOM starts near the body and goes any way, every
    other one a segment, a third seeing their own body"""
    from mgf_amd._capi import SENSOR_DTYPE
    rng = np.random.default_rng(seed)
    off = offsets(lengths)
    n = len(layout["world"])
    rig = np.zeros(n, SENSOR_DTYPE)
    rig["world"], rig["body"] = layout["world"], layout["body"]
    rig["dt"] = np.inf
    for i, (w, bd, role) in enumerate(zip(layout["world"], layout["body"], layout["role"])):
        g = off[w] + bd
        x, q = state["x"][g].astype(np.float64), state["q"][g]
        p, d, flags = np.zeros(3), np.zeros(3), IGNORE_SELF
        if role == DOWN:
            d = _unrotate(q, (0.0, -1.0, 0.0))
        elif role == UP:
            d = _unrotate(q, (0.0, 1.0, 0.0))
        elif role == RING:
            ring = ring_of(scs[w])
            tgt = ring[int(rng.integers(0, len(ring)))]
            # (from almost straight above: Intersects<Compound> traces its tree in a frame of its own, and of slanted rays it loses most)
            start = tgt + np.array([rng.uniform(-0.25, 0.25), 3.0, rng.uniform(-0.25, 0.25)])
            p, d = _unrotate(q, start - x), _unrotate(q, tgt - start)
        elif role == SHORT:
            d = _unrotate(q, rng.normal(0, 1, 3))
            d /= np.linalg.norm(d)
            rig["dt"][i] = 0.01
        elif role in (SELF_IGNORED, SELF_SEEN):
            d = np.array([0.0, 0.0, 1.0])
            flags = IGNORE_SELF if role == SELF_IGNORED else 0
        elif role == RANDOM:
            p = rng.uniform(-0.3, 0.3, 3)
            d = rng.normal(0, 1, 3)
            d *= rng.uniform(0.5, 3.0) / np.linalg.norm(d)
            if i % 2:
                rig["dt"][i] = 1.0
            flags = 0 if i % 3 == 0 else IGNORE_SELF
        rig["p"][i], rig["d"][i], rig["flags"][i] = p, d, flags
    return rig


# ---- rigs for the plan alone --------------------------------------------------------------------------------------------------------------
PLAN_COUNTS = (0, 1, 256, 257, 600)


def plan_worlds(seed=94):
    """a world array with worlds of 0, 1, 256, 257 and 600 sensors in one shuffled order"""
    w = np.concatenate([np.full(c, k, np.int32) for k, c in enumerate(PLAN_COUNTS)])
    return w[np.random.default_rng(seed).permutation(len(w))]
