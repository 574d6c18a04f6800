"""Shared by the tests of a batch's slider encoders (mgf_batch_read_sliders / _read_sliders_dev, mgf_batch_set_slider_trace and the readings
table of a rollout), without a GPU: a numpy restatement of the header's reading, f32 operation by f32 operation -
    ra, rb, Pa, Pb, C, A, T1, T2, B, U1: the slider's SETUP lines (other == -1: B = bx, U1 = ub, Pb = pb, rb = 0, v_b = 0, omega_b = 0)
    U2 = cross(B, U1);  ca = ra + C;  sA = cross(ca, A);  sB = cross(rb, A)
    d = dot(C, A);  rate = (dot(v_b - v_a, A) + dot(omega_b, sB)) - dot(omega_a, sA)
    LOCK: side = 2;  LIMIT and d < lo: side = -1;  LIMIT and d > hi: side = +1;  otherwise side = 0
    off1 = dot(C, T1);  off2 = dot(C, T2);  e = ((cross(A, B) + cross(T1, U1)) + cross(T2, U2)) * 0.5
- with tests/batch_slider_cases.py's rotate, cross and dot, in float32 or in float64; the bounds of the f32 reading against the f64 one,
derived below from the rounded operations between the state and each word; and the small rigs of
tests/test_gpu_world_batch_slider_read.py."""
import numpy as np

from mgf_amd import _capi
from tests import batch_sensor_cases as SC
from tests import batch_slider_cases as LC

f32 = np.float32
EPS = float(np.finfo(np.float32).eps)      # 2^-23; the unit roundoff u of one rounded f32 operation is EPS / 2
WORDS = ("d", "rate", "side", "off1", "off2", "e.x", "e.y", "e.z")

# The f32 reading against the float64 one, to first order in u = EPS / 2, from the rounded operations between the state and each word.
# Both restatements start from the same f32 state (x + delta is the state's own f32 sum), so only the operations below round.  Lengths:
#   arms = |pa| + |pb|   the record's two anchors, each in its body's frame
#   P = |Pa| + |Pb|      the two anchors in the world: C = Pb - Pa cancels against them, which is why no bound here is absolute
#   V = |v_a| + |v_b|,  W = |omega_a| + |omega_b|
# From tests/batch_hinge_read_cases.py, whose steps are homogeneous in the length of the rotated vector:
#   r = rotate(q, p)      a component is off by at most rho |p|, rho = 17.3u; A, T1, B, U1 (unit vectors) by rho
#   cross(X, Y)           a component carries sqrt(2) (dX |Y| + dY |X|) and adds 2u |X| |Y|: T2 = cross(A, T1), U2 = cross(B, U1) are off by
#                         tau = 2 sqrt(2) rho + 2u = 50.9u
#   dot(X, Y)             carries sqrt(3) (dX |Y| + dY |X|) for componentwise errors dX, dY and adds 3u |X| |Y|
# The gap:
#   Pa = x_a + ra         rho |pa| + u |Pa| a component;  Pb likewise (other == -1: Pb = pb, exact)
#   C = Pb - Pa           rho arms + u P, and u |C_i| <= u P of its own: dC = rho arms + 2u P a component;  |C| <= P
# d and off1 (dot of C with A or T1, each off by rho):
#   sqrt(3) dC + sqrt(3) rho |C| + 3u |C| <= sqrt(3) rho arms + (2 sqrt(3) + sqrt(3) rho / u + 3) u P = 30.0u arms + 36.4u P
#   = 15.0 EPS arms + 18.2 EPS P:                                 D_BOUND = 16 EPS arms + 20 EPS P
# off2 (dot of C with T2, off by tau):
#   sqrt(3) dC + sqrt(3) tau |C| + 3u |C| <= 30.0u arms + (3.5 + 88.2 + 3) u P = 15.0 EPS arms + 47.4 EPS P:
#                                                                 OFF_BOUND = 16 EPS arms + 50 EPS P   (held for off1 too)
# e reads unit vectors alone, so its bound depends on neither length:
#   cross(A, B), cross(T1, U1)    sqrt(2) 2 rho + 2u = 50.9u each;  cross(T2, U2): sqrt(2) 2 tau + 2u = 146u
#   the two sums add u |partial sum| <= 2u and 3u;  * 0.5 is exact: (50.9 + 50.9 + 146 + 5) u / 2 = 126.4u = 63.2 EPS a component:
#                                                                 E_BOUND = 64 EPS
# The rate:
#   ca = ra + C           rho |pa| + dC + u |ca_i| with |ca| <= arms + P: dca <= (2 rho + u) arms + 3u P = 35.6u arms + 3u P
#   sA = cross(ca, A)     sqrt(2) dca + sqrt(2) rho |ca| + 2u |ca| <= 76.8u arms + 30.7u P;  |sA| <= arms + P
#   sB = cross(rb, A)     sqrt(2) rho |pb| twice, + 2u |pb|: 50.9u |pb|;  |sB| <= |pb|
#   dot(v_b - v_a, A)     the difference is off by u |wd_i|, A by rho: (1 + sqrt(3) rho / u + 3) u V = 34.0u V
#   dot(omega_b, sB)      omega is exact: sqrt(3) 50.9u |pb| |omega_b| + 3u |pb| |omega_b| = 91.2u |pb| |omega_b|
#   dot(omega_a, sA)      sqrt(3) (76.8 arms + 30.7 P) u |omega_a| + 3u (arms + P) |omega_a| = (136.0 arms + 56.2 P) u |omega_a|
#   the sum and the difference add u of each partial result: u V + u |pb| |omega_b| twice, u (arms + P) |omega_a| once
#   together 36u V + (137 arms + 57.2 P) u W = 18 EPS V + (68.5 arms + 28.6 P) EPS W:
#                                                                 RATE_BOUND = 20 EPS V + (72 arms + 32 P) EPS W
# These are worst cases of every rounding pulling the same way; what the seeded rig shows on the CPU is printed by
# tests/test_world_batch_slider_read_host.py and stands in DESIGN.md.
D_ARMS, D_P = 16 * EPS, 20 * EPS
OFF_ARMS, OFF_P = 16 * EPS, 50 * EPS
E_BOUND = 64 * EPS
RATE_V, RATE_W_ARMS, RATE_W_P = 20 * EPS, 72 * EPS, 32 * EPS


def readings(rig, state, lengths, ft=f32, parts=False):
    """[n, 8] of `ft`: (d, rate, side, off1, off2, e.x, e.y, e.z) of every slider from `state` - rows over every body of the batch: x,
    delta, q, v, omega - every line a separately rounded operation of `ft`.  parts=True: also a dict of the lines between - sA, sB, C,
    T1, T2 [n, 3] - for the tests that hold them against tests/batch_slider_cases.py's setup"""
    off = SC.offsets(lengths)
    x = (state["x"].astype(f32) + state["delta"].astype(f32)).astype(ft)       # x + delta is the state's own f32 sum, as gather_state returns it
    q, v, om = state["q"].astype(ft), state["v"].astype(ft), state["omega"].astype(ft)
    zero = np.zeros(3, ft)
    out = np.zeros((len(rig), 8), ft)
    mid = {k: np.zeros((len(rig), 3), ft) for k in ("sA", "sB", "C", "T1", "T2")}
    with np.errstate(all="ignore"):
        for i, r in enumerate(rig):
            ga = int(off[r["world"]] + r["body"])
            gb = int(off[r["world"]] + r["other"]) if r["other"] >= 0 else -1
            flags = int(r["flags"])
            ra = LC._rotate(q[ga], r["pa"].astype(ft), ft)
            Pa = x[ga] + ra
            A = LC._rotate(q[ga], r["ax"].astype(ft), ft)
            T1 = LC._rotate(q[ga], r["ua"].astype(ft), ft)
            T2 = LC._cross(A, T1)
            if gb >= 0:
                rb = LC._rotate(q[gb], r["pb"].astype(ft), ft)
                Pb = x[gb] + rb
                B = LC._rotate(q[gb], r["bx"].astype(ft), ft)
                U1 = LC._rotate(q[gb], r["ub"].astype(ft), ft)
                v_b, om_b = v[gb], om[gb]
            else:
                rb, Pb, B, U1, v_b, om_b = zero, r["pb"].astype(ft), r["bx"].astype(ft), r["ub"].astype(ft), zero, zero
            C = Pb - Pa
            U2 = LC._cross(B, U1)
            ca = ra + C
            sA = LC._cross(ca, A)
            sB = LC._cross(rb, A)
            d = LC._dot(C, A)
            rate = (LC._dot(v_b - v[ga], A) + LC._dot(om_b, sB)) - LC._dot(om[ga], sA)
            lo, hi = ft(r["lo"]), ft(r["hi"])
            side = ft(0.0)
            if flags & LC.LOCK:
                side = ft(2.0)
            elif flags & LC.LIMIT and d < lo:
                side = ft(-1.0)
            elif flags & LC.LIMIT and d > hi:
                side = ft(1.0)
            off1 = LC._dot(C, T1)
            off2 = LC._dot(C, T2)
            e = ((LC._cross(A, B) + LC._cross(T1, U1)) + LC._cross(T2, U2)) * ft(0.5)
            for a in (d, rate, off1, off2, e, sA, sB, C):
                assert a.dtype == ft, a.dtype
            out[i] = (d, rate, side, off1, off2, e[0], e[1], e[2])
            mid["sA"][i], mid["sB"][i], mid["C"][i], mid["T1"][i], mid["T2"][i] = sA, sB, C, T1, T2
    return (out, mid) if parts else out


def scales(rig, state, lengths):
    """(arms, P, V, W) of every slider, float64: |pa| + |pb|, |Pa| + |Pb|, |v_a| + |v_b| and |omega_a| + |omega_b| - the lengths the
    bounds above are in (other == -1: v_b = omega_b = 0, Pb = pb)"""
    d = np.float64
    off = SC.offsets(lengths)
    ga = off[rig["world"]] + rig["body"]
    far = rig["other"] >= 0
    gb = np.where(far, off[rig["world"]] + rig["other"], ga)
    x = (state["x"].astype(f32) + state["delta"].astype(f32)).astype(d)
    q = state["q"].astype(d)
    Pa = x[ga] + LC._rot64(q[ga], rig["pa"].astype(d))
    Pb = np.where(far[:, None], x[gb] + LC._rot64(q[gb], rig["pb"].astype(d)), rig["pb"].astype(d))
    n = np.linalg.norm
    arms = n(rig["pa"].astype(d), axis=1) + n(rig["pb"].astype(d), axis=1)
    V = n(state["v"].astype(d)[ga], axis=1) + np.where(far, n(state["v"].astype(d)[gb], axis=1), 0.0)
    W = n(state["omega"].astype(d)[ga], axis=1) + np.where(far, n(state["omega"].astype(d)[gb], axis=1), 0.0)
    return arms, n(Pa, axis=1) + n(Pb, axis=1), V, W


def bounds(rig, state, lengths):
    """(d, off, e, rate) bounds of every slider's f32 reading against the float64 one, from the derivation above"""
    arms, P, V, W = scales(rig, state, lengths)
    return D_ARMS * arms + D_P * P, OFF_ARMS * arms + OFF_P * P, np.full(len(rig), E_BOUND), RATE_V * V + (RATE_W_ARMS * arms + RATE_W_P * P) * W


def as_readings(words_):
    """[..., 8] float32 words as a SLIDER_READING_DTYPE array [...]"""
    w = np.ascontiguousarray(words_, f32)
    return w.view(_capi.SLIDER_READING_DTYPE).reshape(w.shape[:-1])


def words(readings_):
    """a SLIDER_READING_DTYPE or SLIDER_TRACE_FULL_DTYPE array [...] as float32 words [..., 8 | 16]"""
    r = np.ascontiguousarray(readings_)
    return r.view(f32).reshape(r.shape + (r.dtype.itemsize // 4,))


def where(got, want):
    """the first rows of two [n, w] word arrays that differ by bytes, with the words that do"""
    got, want = got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1])
    bad = [i for i in range(len(want)) if got[i].tobytes() != want[i].tobytes()][:6]
    return [(i, [WORDS[k] if k < 8 else "impulse %d" % (k - 8) for k in range(want.shape[-1]) if got[i, k:k + 1].tobytes() != want[i, k:k + 1].tobytes()]) for i in bad]


# ---- the rigs of the GPU tests ------------------------------------------------------------------------------------------------------------
CASES = ("none", "limit_inside", "limit_below", "limit_above", "limit_point", "lock", "both_above")
SIDE_OF = {"none": 0.0, "limit_inside": 0.0, "limit_below": -1.0, "limit_above": 1.0, "limit_point": 0.0, "lock": 2.0, "both_above": 1.0}


def small_rig(lengths, state, n, worlds=(0, 2), seed=641):
    """n sliders over the worlds `worlds` of a batch (at most LC.MAX a world, the worlds interleaved in the caller's array), slider i
    between two seeded bodies of its world or - every third - one body and the world; placed about the midpoints with seeded axes, other's
    frame up to LC.TILT radians and LC.SHIFT length units off (LC.place), so that d, the off-axis gap and the frames' error are all live;
    then, about each slider's PRESENT d - the f32 reading's own, so that lo == hi == d is met exactly - the cases dealt round: no flag;
    LIMIT inside; LIMIT below lo; LIMIT above hi; LIMIT with lo == hi == d (side 0); LOCK; LIMIT | MOTOR above hi.
    Returns (rig, case of every slider)"""
    rng = np.random.default_rng(seed)
    rig = np.zeros(n, _capi.SLIDER_DTYPE)
    if n == 0:
        return rig, np.zeros(0, np.int64)
    assert n <= LC.MAX * len(worlds) and all(lengths[w] >= 2 for w in worlds)
    rig["world"] = np.asarray(worlds)[np.arange(n) % len(worlds)]
    for i in range(n):
        nb = lengths[rig["world"][i]]
        a, b = rng.choice(nb, 2, replace=False)
        rig["body"][i], rig["other"][i] = a, (-1 if i % 3 == 2 else b)
    rig["beta"] = 0.2
    LC.place(rig, state, lengths, seed + 1, LC.TILT, LC.SHIFT)
    d = readings(rig, state, lengths)[:, 0]
    assert d.dtype == f32
    case = np.arange(n) % len(CASES)
    lo_hi = {"none": (0.0, 0.0), "limit_inside": (-0.3, 0.4), "limit_below": (0.2, 0.9), "limit_above": (-0.9, -0.2), "limit_point": (0.0, 0.0), "lock": (0.05, 0.05),
             "both_above": (-0.6, -0.25)}
    for c, name in enumerate(CASES):
        at = np.flatnonzero(case == c)
        lo, hi = lo_hi[name]
        rig["lo"][at], rig["hi"][at] = (d[at].astype(np.float64) + lo).astype(f32), (d[at].astype(np.float64) + hi).astype(f32)
        rig["flags"][at] = {"none": 0, "lock": LC.LOCK, "both_above": LC.LIMIT | LC.MOTOR}.get(name, LC.LIMIT)
        rig["fmax"][at] = np.inf if name == "both_above" else 0.0
    assert np.all(rig["lo"] <= rig["hi"]) and np.array_equal(rig["lo"][case == 4], d[case == 4])
    return rig, case
