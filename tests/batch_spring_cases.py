"""Shared by the tests of a batch's springs (mgf_batch_set_springs / _apply_springs / _apply_springs_dev, and the springs of a rollout),
without a GPU: a numpy restatement of the header's definition of a spring's wrench, f32 operation by operation -
    ra = rotate(q_a, pa);  Pa = x_a + ra;  Va = v_a + cross(omega_a, ra)
    other >= 0: rb = rotate(q_b, pb);  Pb = x_b + rb;  Vb = v_b + cross(omega_b, rb)      other == -1: Pb = pb;  Vb = 0
    d = Pb - Pa;  len = sqrt(dot(d, d));  n = d / len;  rate = dot(Vb - Va, n)
    f = k * (len - rest) + c * rate;  clamp to [lo, hi];  s = f * h
    L = n * s;  A = cross(ra, L);  Lb = -L;  Ab = cross(rb, Lb);   len == 0, or len or s not finite: zeros, skipped
(rotate and cross are tests/batch_sensor_cases.py's, which tests/test_world_batch_actuators_host.py holds to the oracle) - the record
list a call is defined by, the plan of the ends restated, and the scenes and rigs of tests/test_gpu_world_batch_springs.py, seeded."""
import numpy as np

from mgf_amd import _capi, scenes
from tests import batch_query_cases as BQ
from tests import batch_sensor_cases as SC

f32 = np.float32
STATE = ("x", "q", "v", "omega", "delta")


# ---- the definition -----------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    """cgmath InnerSpace::dot, rows of f32: (x*x' + y*y') + z*z'"""
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def wrenches(rig, h, x, q, v, om, lengths):
    """(W, skipped): W[i] = (L, A, Lb, Ab) of spring i of `rig` (SPRING_DTYPE rows) over the time step h, from the rows x (= x + delta),
    q, v, omega of every body of a batch whose worlds hold `lengths` bodies - rows of f32, every operation a rounded f32 operation of
    its own, in the header's order; skipped[i]: len == 0, or len or f * h not finite"""
    n = len(rig)
    x, q, v, om = (np.ascontiguousarray(a, f32) for a in (x, q, v, om))
    h = f32(h)
    off = SC.offsets(lengths)[rig["world"]]
    ga = off + rig["body"]
    far = rig["other"] >= 0
    gb = np.where(far, off + rig["other"], ga)            # (a world anchor: any row that exists; what comes of it is not used)
    pa, pb = rig["pa"].astype(f32).reshape(n, 3), rig["pb"].astype(f32).reshape(n, 3)
    with np.errstate(all="ignore"):
        ra = SC.rotate(q[ga], pa)
        Pa = x[ga] + ra
        Va = v[ga] + SC._cross(om[ga], ra)
        rb = np.where(far[:, None], SC.rotate(q[gb], pb), f32(0.0))
        Pb = np.where(far[:, None], x[gb] + rb, pb)
        Vb = np.where(far[:, None], v[gb] + SC._cross(om[gb], rb), f32(0.0))
        d = Pb - Pa
        ln = np.sqrt(_dot(d, d))
        nn = d / ln[:, None]
        rate = _dot(Vb - Va, nn)
        f = rig["k"].astype(f32) * (ln - rig["rest"].astype(f32)) + rig["c"].astype(f32) * rate
        lo, hi = rig["lo"].astype(f32), rig["hi"].astype(f32)
        f = np.where(f < lo, lo, f)                         # (a NaN compares false: it stays)
        f = np.where(f > hi, hi, f)
        s = f * h
        L = nn * s[:, None]
        A = SC._cross(ra, L)
        Lb = -L
        Ab = SC._cross(rb, Lb)
    Lb, Ab = np.where(far[:, None], Lb, f32(0.0)), np.where(far[:, None], Ab, f32(0.0))
    skipped = (ln == 0) | ~np.isfinite(ln) | ~np.isfinite(s)
    W = np.concatenate([L, A, Lb, Ab], axis=1)
    assert W.dtype == f32 and W.shape == (n, 12) and ln.dtype == f32 and s.dtype == f32
    W[skipped] = 0.0
    return W, skipped


def rig_wrenches(rig, h, state, lengths):
    """wrenches of a rig from state(None) of a batch: x is x + delta, as gather_state returns it"""
    x = (state["x"] + state["delta"]).astype(f32)
    return wrenches(rig, h, x, state["q"], state["v"], state["omega"], lengths)


def records(rig, W):
    """the record list a call is defined by: for i in rig order (world, body, L, A), then, where other >= 0, (world, other, Lb, Ab).
    Returns (world, body, linear, angular) - what apply_impulses takes."""
    world, body, lin, ang = [], [], [], []
    for i in range(len(rig)):
        world.append(rig["world"][i]); body.append(rig["body"][i]); lin.append(W[i, 0:3]); ang.append(W[i, 3:6])
        if rig["other"][i] >= 0:
            world.append(rig["world"][i]); body.append(rig["other"][i]); lin.append(W[i, 6:9]); ang.append(W[i, 9:12])
    return (np.int32(world), np.int32(body), np.array(lin, f32).reshape(-1, 3), np.array(ang, f32).reshape(-1, 3))


def end_plan(rig):
    """the plan of the ends restated: end e = 2 i + side (a world anchor has no far end), sorted by (world, body) - stable - and cut
    into runs of one body.  Returns (runs [(world, body, first, count)], order)"""
    ends = [2 * i + s for i in range(len(rig)) for s in ((0, 1) if rig["other"][i] >= 0 else (0,))]

    def key(e):
        r = rig[e >> 1]
        return (int(r["world"]), int(r["other"] if e & 1 else r["body"]))
    order = sorted(ends, key=key)                           # (Python's sort is stable)
    runs = []
    for p, e in enumerate(order):
        if p == 0 or key(e) != key(order[p - 1]):
            runs.append([key(e)[0], key(e)[1], p, 0])
        runs[-1][3] += 1
    return np.int64(runs).reshape(-1, 4), np.int64(order)


def spring(world, body, other=-1, pa=(0, 0, 0), pb=(0, 0, 0), rest=0.0, k=0.0, c=0.0, lo=-np.inf, hi=np.inf):
    r = np.zeros(1, _capi.SPRING_DTYPE)
    r["world"], r["body"], r["other"], r["pa"], r["pb"], r["rest"], r["k"], r["c"], r["lo"], r["hi"] = world, body, other, pa, pb, rest, k, c, lo, hi
    return r


# ---- the scenes ---------------------------------------------------------------------------------------------------------------------------
LENGTHS = (24, 24, 20, 16, 8, 0)   # the worlds of spring_scenes(): runs 48 .. 67 of the plan are world 2's - it straddles a wave of 64 lanes
BARE_WORLD, EMPTY_WORLD = 4, 5      # a world no spring names; a world without bodies
HUB = (1, 3)                        # the body 70 ends name
HUB_ENDS = 70
SETTLE_TICKS = 2                    # ticks before the state is written: delta leaves zero


def _mixed(n, seed):
    """n bodies r = 0.4 on a lattice of pitch 1.5 over the floor of a box, every third a short capsule"""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(n ** (1.0 / 3.0)))
    i, j, k = np.meshgrid(np.arange(side), np.arange(side), np.arange(side), indexing="ij")
    c = np.stack([(i.ravel() - (side - 1) / 2.0) * 1.5, 0.6 + j.ravel() * 1.5, (k.ravel() - (side - 1) / 2.0) * 1.5], axis=1)[:n].astype(f32)
    c += rng.uniform(-0.05, 0.05, c.shape).astype(f32)
    comps = scenes._spheres(c, 0.4)
    cap = np.arange(n) % 3 == 1
    d = rng.normal(0, 1, (n, 3))
    comps["tag"][cap] = 1
    comps["d"][cap] = (0.5 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)[cap]
    return scenes._scene("mixed_%d" % n, comps, scenes.box_terrain(side * 1.5 + 2.0, side * 1.5 + 4.0, (0.0, 0.0, 0.0)), v0=rng.uniform(-1, 1, (n, 3)).astype(f32))


def spring_scenes():
    scs = [_mixed(n, 300 + k) for k, n in enumerate(LENGTHS) if n]
    return scs + [BQ.empty_scene(scs[0]["terrain"])]


def written_state(total, seed=311):
    """(q, v, omega) written into every body: unit quaternions far from the identity, velocities of a few units"""
    rng = np.random.default_rng(seed)
    q = rng.normal(0, 1, (total, 4)).astype(f32)
    q = (q / np.sqrt((q.astype(np.float64) ** 2).sum(axis=1, keepdims=True))).astype(f32)
    return q, rng.uniform(-3, 3, (total, 3)).astype(f32), rng.uniform(-6, 6, (total, 3)).astype(f32)


def main_rig(lengths, x, v, seed=313):
    """(rig, planted): about 210 springs over worlds 0 .. 3 in one seeded shuffle - a chain through every body of each (every body
    carries an end: 84 runs, more than a wave), HUB_ENDS ends on HUB, random pairs, world anchors, ropes and struts whose clamp bites -
    and `planted` springs that are skipped: an anchor at the body's own point (len == 0; x: the bodies' x + delta), a stiffness that
    overflows, and a damping that gives inf - inf (v: the bodies' velocities - the damped body moves along x faster than 1.5)"""
    rng = np.random.default_rng(seed)
    rows = []
    for w in range(4):
        n = lengths[w]
        for i in range(n - 1):                                                     # the chain
            rows.append((w, i, i + 1))
        for _ in range(10):                                                        # random pairs
            a, b = rng.choice(n, 2, replace=False)
            rows.append((w, int(a), int(b)))
        for _ in range(5):                                                         # world anchors
            rows.append((w, int(rng.integers(0, n)), -1))
    others = [b for b in range(lengths[HUB[0]]) if b != HUB[1]]
    for j in range(HUB_ENDS):                                                      # the hub: as `body` and as `other` in turn
        o = others[j % len(others)]
        rows.append((HUB[0], HUB[1], o) if j % 2 == 0 else (HUB[0], o, HUB[1]))
    rows = [rows[i] for i in rng.permutation(len(rows))]
    n = len(rows)
    rig = np.zeros(n, _capi.SPRING_DTYPE)
    rig["world"], rig["body"], rig["other"] = np.int32(rows).T
    rig["pa"], rig["pb"] = rng.uniform(-0.4, 0.4, (n, 3)), rng.uniform(-0.4, 0.4, (n, 3))
    anchor = rig["other"] < 0
    off = SC.offsets(lengths)
    rig["pb"][anchor] = x[off[rig["world"][anchor]] + rig["body"][anchor]] + rng.uniform(-2, 2, (int(anchor.sum()), 3)).astype(f32)
    rig["rest"], rig["k"], rig["c"] = rng.uniform(0.0, 2.0, n), rng.uniform(5.0, 60.0, n), rng.uniform(0.0, 4.0, n)
    rig["lo"], rig["hi"] = -np.inf, np.inf
    kind = rng.integers(0, 4, n)
    rig["lo"][kind == 1] = 0.0                                                     # a rope
    rig["hi"][kind == 2] = 0.0                                                     # a strut that only pushes
    rig["lo"][kind == 3], rig["hi"][kind == 3] = -1.5, 1.5                         # a saturating element
    at = np.flatnonzero(anchor)
    g = off[rig["world"]] + rig["body"]
    zero, over = (int(i) for i in at[:2])
    nan = next(int(i) for i in at[2:] if abs(v[g[i], 0]) > 1.5)
    rig["pa"][zero], rig["pb"][zero] = 0.0, x[g[zero]]                             # Pa = x + rotate(q, 0) = x: d = 0
    rig["lo"][[zero, over, nan]], rig["hi"][[zero, over, nan]] = -np.inf, np.inf
    rig["pb"][over], rig["rest"][over], rig["k"][over], rig["c"][over] = x[g[over]] + f32([10, 0, 0]), 0.0, 3.0e38, 0.0
    # n = (1, 0, 0) and pa = 0: rate = -v.x, so k * len = +inf beside c * rate = -inf
    rig["pb"][nan], rig["rest"][nan], rig["k"][nan], rig["c"][nan] = x[g[nan]] + f32([10, 0, 0]), 0.0, 3.0e38, (3.0e38 if v[g[nan], 0] > 0 else -3.0e38)
    rig["pa"][nan] = 0.0
    return rig, [zero, over, nan]


def sized_rig(lengths, count, seed=331):
    """`count` springs over worlds 0 .. 3, pairs and anchors, no skips"""
    rng = np.random.default_rng(seed + count)
    rig = np.zeros(count, _capi.SPRING_DTYPE)
    rig["world"] = rng.integers(0, 4, count)
    n = np.int64(lengths)[rig["world"]]
    rig["body"] = rng.integers(0, n)
    rig["other"] = (rig["body"] + 1 + rng.integers(0, n - 1)) % n
    rig["other"][rng.random(count) < 0.2] = -1
    rig["pa"], rig["pb"] = rng.uniform(-0.4, 0.4, (count, 3)), rng.uniform(-0.4, 0.4, (count, 3))
    rig["pb"][rig["other"] < 0] += f32([0.0, 40.0, 0.0])                           # an anchor far above: len is never 0
    rig["rest"], rig["k"], rig["c"] = rng.uniform(0.0, 2.0, count), rng.uniform(5.0, 60.0, count), rng.uniform(0.0, 4.0, count)
    rig["lo"], rig["hi"] = -np.inf, np.inf
    return rig


def late_springs(lengths, seed=337):
    """(rig, planted): 45 weak springs over the three worlds of tests/batch_rollout_cases.py's late-contact scenes - weak enough to
    leave the ticks of first contact where they are - with one stiffness that overflows in every tick"""
    rng = np.random.default_rng(seed)
    n = 45
    rig = np.zeros(n, _capi.SPRING_DTYPE)
    rig["world"] = np.arange(n) % 3
    nb = np.int64(lengths)[rig["world"]]
    rig["body"] = rng.integers(0, nb)
    rig["other"] = (rig["body"] + 1 + rng.integers(0, nb - 1)) % nb
    rig["other"][::7] = -1
    rig["pa"], rig["pb"] = rng.uniform(-0.3, 0.3, (n, 3)), rng.uniform(-0.3, 0.3, (n, 3))
    rig["pb"][rig["other"] < 0] += f32([0.0, 30.0, 0.0])
    rig["rest"], rig["k"], rig["c"] = 1.3, rng.uniform(0.05, 0.3, n), rng.uniform(0.01, 0.05, n)
    rig["lo"], rig["hi"] = -np.inf, np.inf
    rig["lo"][1::5] = 0.0
    over = 7                                                                      # (7 % 7 == 0: an anchor 30 above)
    assert rig["other"][over] == -1
    rig["k"][over], rig["c"][over], rig["rest"][over], rig["lo"][over] = 3.0e38, 0.0, 0.0, -np.inf
    return rig, [over]


def free_pair():
    """two free unit-mass spheres 2 apart with no world force, far from every face of their box"""
    c = f32([[-1.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    return scenes._scene("free_pair", scenes._spheres(c, 0.25), scenes.box_terrain(50.0, 100.0, (0.0, -50.0, 0.0)), v0=np.zeros((2, 3), f32), gravity=(0.0, 0.0, 0.0))
