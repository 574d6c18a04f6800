"""Shared by the tests of a batch's hinge encoders (mgf_batch_read_hinges / _read_hinges_dev, mgf_batch_set_hinge_trace and the readings
table of a rollout), without a GPU: a numpy restatement of the header's reading, f32 operation by f32 operation -
    ra, rb, Pa, Pb, C, A, T1, T2, B, U1: the hinge's SETUP lines (other == -1: B = bx, U1 = ub, Pb = pb, omega_b = 0)
    c = dot(U1, T1);  sn = dot(U1, T2);  rate = dot(omega_b - omega_a, A)
    cphi = c * cm + sn * sm;  sphi = sn * cm - c * sm;  LIMIT and cphi <= ch:  sphi >= 0: side = +1;  else side = -1;  otherwise side = 0
    gap = C;  e1 = dot(B, T1);  e2 = dot(B, T2);  tilt2 = e1 * e1 + e2 * e2
- with tests/batch_hinge_cases.py's rotate, cross and dot, in float32 or in float64; the bounds of the f32 reading against the f64 one,
derived below from the count of rounded operations; and the small rigs of tests/test_gpu_world_batch_hinge_read.py."""
import numpy as np

from mgf_amd import _capi
from tests import batch_hinge_cases as HC
from tests import batch_sensor_cases as SC

f32 = np.float32
EPS = float(np.finfo(np.float32).eps)      # 2^-23; the unit roundoff u of one rounded f32 operation is EPS / 2
WORDS = ("c", "sn", "rate", "side", "gap.x", "gap.y", "gap.z", "tilt2")

# The f32 reading against the float64 one, to first order in u = EPS / 2, from the rounded operations between the quaternions and c, sn
# (every vector of the record is of unit length to 1e-3 and |q| = 1 to rounding, so every intermediate below is at most 1 in length):
#   rotate(q, p) = cross(v, cross(v, p) + p * s) * 2 + p
#     w = cross(v, p)     a component is two products and a difference, 3 rounded operations: at most 2u (|v_j p_k| + |v_k p_j| <= |v||p|)
#     m = w + p * s       one product (u), one sum (u), the 2u of w: at most 4u a component, |m| <= 1
#     z = cross(v, m)     carries 4u (|v_j| + |v_k|) <= 4 sqrt(2) u, adds 2u of its own: at most 7.66u
#     r = z * 2 + p       the doubling is exact, the sum adds u: at most 2 * 7.66u + u = 16.3u, say rho = 17.3u with the second-order slack
#   T2 = cross(A, T1)     carries rho (|A_j| + |T1_k| + |A_k| + |T1_j|) <= 2 sqrt(2) rho, adds 2u: at most 50.9u a component
#   c = dot(U1, T1)       carries rho (sum |U1_i| + sum |T1_i|) <= 2 sqrt(3) rho = 59.9u, three products and two sums add 3u: at most 63u
#   sn = dot(U1, T2)      carries sqrt(3) (50.9u + rho) = 118u, adds 3u: at most 121u
# So 14 rounded operations stand in the cone of one component of a rotated vector (two components of m at 5 each, 3 of z, 1 of r), 3
# more a component of the cross product, 5 in a dot product, and the worst case of sn is 121u = 60.5 EPS: C_SN_BOUND = 64 EPS.  The angle: d theta <= sqrt(63^2 + 121^2) u / r with
# r^2 = c^2 + sn^2 = 1 - dot(U1, A)^2 >= 0.99 for axes tilted by 0.1 rad or less, as the seeded rigs' and the arm's are:
# 138.5u = 69.3 EPS: THETA_BOUND = 72 EPS, 8.6e-6 rad.  The rate: wd = omega_b - omega_a is one rounded difference a component,
# dot(wd, A) carries sqrt(3) rho |wd| and adds 3u |wd|: at most 34u |wd|, RATE_BOUND = 20 EPS times (|omega_a| + |omega_b|).
# These are worst cases of every rounding pulling the same way; what the seeded rig shows on the CPU is printed by
# tests/test_world_batch_hinge_read_host.py and stands in DESIGN.md.
C_SN_BOUND = 64 * EPS
THETA_BOUND = 72 * EPS
RATE_BOUND = 20 * EPS


def readings(rig, state, lengths, ft=f32):
    """[n, 8] of `ft`: (c, sn, rate, side, gap.x, gap.y, gap.z, tilt2) of every hinge from `state` - rows over every body of the batch:
    x, delta, q, omega - every line a separately rounded operation of `ft`"""
    off = SC.offsets(lengths)
    x = (state["x"].astype(f32) + state["delta"].astype(f32)).astype(ft)       # x + delta is the state's own f32 sum, as gather_state returns it
    q, om = state["q"].astype(ft), state["omega"].astype(ft)
    zero = np.zeros(3, ft)
    out = np.zeros((len(rig), 8), ft)
    with np.errstate(all="ignore"):
        for i, r in enumerate(rig):
            ga = int(off[r["world"]] + r["body"])
            gb = int(off[r["world"]] + r["other"]) if r["other"] >= 0 else -1
            ra = HC._rotate(q[ga], r["pa"].astype(ft), ft)
            Pa = x[ga] + ra
            A = HC._rotate(q[ga], r["ax"].astype(ft), ft)
            T1 = HC._rotate(q[ga], r["ua"].astype(ft), ft)
            T2 = HC._cross(A, T1)
            if gb >= 0:
                rb = HC._rotate(q[gb], r["pb"].astype(ft), ft)
                Pb = x[gb] + rb
                B = HC._rotate(q[gb], r["bx"].astype(ft), ft)
                U1 = HC._rotate(q[gb], r["ub"].astype(ft), ft)
                om_b = om[gb]
            else:
                Pb, B, U1, om_b = r["pb"].astype(ft), r["bx"].astype(ft), r["ub"].astype(ft), zero
            C = Pb - Pa
            c = HC._dot(U1, T1)
            sn = HC._dot(U1, T2)
            rate = HC._dot(om_b - om[ga], A)
            cm, sm, ch = ft(r["cm"]), ft(r["sm"]), ft(r["ch"])
            cphi = c * cm + sn * sm
            sphi = sn * cm - c * sm
            side = ft(0.0)
            if int(r["flags"]) & HC.LIMIT and cphi <= ch:
                side = ft(1.0) if sphi >= 0 else ft(-1.0)
            e1 = HC._dot(B, T1)
            e2 = HC._dot(B, T2)
            tilt2 = e1 * e1 + e2 * e2
            for a in (c, sn, rate, tilt2, C, cphi, sphi):
                assert a.dtype == ft, a.dtype
            out[i] = (c, sn, rate, side, C[0], C[1], C[2], tilt2)
    return out


def as_readings(words):
    """[..., 8] float32 words as a HINGE_READING_DTYPE array [...]"""
    w = np.ascontiguousarray(words, f32)
    return w.view(_capi.HINGE_READING_DTYPE).reshape(w.shape[:-1])


def words(readings_):
    """a HINGE_READING_DTYPE or HINGE_TRACE_FULL_DTYPE array [...] as float32 words [..., 8 | 16]"""
    r = np.ascontiguousarray(readings_)
    return r.view(f32).reshape(r.shape + (r.dtype.itemsize // 4,))


def where(got, want):
    """the first rows of two [n, w] word arrays that differ by bytes, with the words that do"""
    got, want = got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1])
    bad = [i for i in range(len(want)) if got[i].tobytes() != want[i].tobytes()][:6]
    return [(i, [WORDS[k] if k < 8 else "impulse %d" % (k - 8) for k in range(want.shape[-1]) if got[i, k:k + 1].tobytes() != want[i, k:k + 1].tobytes()]) for i in bad]


# ---- the rigs of the GPU tests ------------------------------------------------------------------------------------------------------------
LIMIT_CASES = ("off", "inside", "past_lo", "past_hi")


def small_rig(lengths, state, n, worlds=(0, 2), seed=631):
    """n hinges over the worlds `worlds` of a batch (at most HC.MAX a world, the worlds interleaved in the caller's array), hinge i between
    two seeded bodies of its world or - every third - one body and the world; seeded anchors, axes and references on both ends with every
    hinge angle and a tilt of 0.1 rad or less (HC._far_frames); the limit off, on and inside, on and past lo, on and past hi, dealt round;
    every other hinge motorised as well.  Returns (rig, case of every hinge)"""
    rng = np.random.default_rng(seed)
    rig = np.zeros(n, _capi.HINGE_DTYPE)
    if n == 0:
        return rig, np.zeros(0, np.int64)
    assert n <= HC.MAX * len(worlds) and all(lengths[w] >= 2 for w in worlds)
    rig["world"] = np.asarray(worlds)[np.arange(n) % len(worlds)]
    for i in range(n):
        nb = lengths[rig["world"][i]]
        a, b = rng.choice(nb, 2, replace=False)
        rig["body"][i], rig["other"][i] = a, (-1 if i % 3 == 2 else b)
    rig["pa"] = rng.uniform(-0.5, 0.5, (n, 3))
    rig["pb"] = rng.uniform(-0.5, 0.5, (n, 3))
    rig["beta"] = 0.2
    rig["ax"], rig["ua"] = HC._perpendicular_pairs(rng, n)
    HC._far_frames(rig, state, lengths, rng)
    th = HC.thetas(rig, state, lengths)
    case = np.arange(n) % len(LIMIT_CASES)
    lo_hi = {"off": (-0.3, 0.4), "inside": (-0.3, 0.4), "past_lo": (0.2, 0.9), "past_hi": (-0.9, -0.2)}
    for c, name in enumerate(LIMIT_CASES):
        at = np.flatnonzero(case == c)
        HC.set_limits(rig, th[at] + lo_hi[name][0], th[at] + lo_hi[name][1], at)
        rig["flags"][at] = 0 if name == "off" else HC.LIMIT
    rig["flags"][1::2] |= HC.MOTOR
    rig["tmax"][1::2] = np.inf
    return rig, case


SIDE_OF = {"off": 0.0, "inside": 0.0, "past_lo": -1.0, "past_hi": 1.0}
