"""Shared by the tests of a batch's sliders (mgf_batch_set_sliders / _set_slider_targets / _solve_sliders / _solve_sliders_dev, and the
sliders of a rollout), without a GPU: a numpy restatement of the header's definition, f32 operation by f32 operation - the ball joint's
ra, rb, Pa, Pb, C and s, then
    A = rotate(q_a, ax);  T1 = rotate(q_a, ua);  T2 = cross(A, T1);  B = rotate(q_b, bx);  U1 = rotate(q_b, ub)   (other == -1: B = bx, U1 = ub)
    U2 = cross(B, U1);  ca = ra + C;  d = dot(C, A);  ims = im_a + im_b
    sA = cross(ca, A);  sB = cross(rb, A);  Km = (ims + dot(sA, I_a * sA)) + dot(sB, I_b * sB)
    pAi = cross(ca, Ti);  pBi = cross(rb, Ti);  gi = dot(C, Ti) * s;  k_ij, d2, m** over (pA, pB)
    e = ((cross(A, B) + cross(T1, U1)) + cross(T2, U2)) * 0.5;  gw = e * s;  Kwinv = invert(I_a + I_b)
    LOCK: side = 2, lb = (lo - d) * s;  LIMIT and d < lo: side = -1, lb = (lo - d) * s;  LIMIT and d > hi: side = +1, lb = -((d - hi) * s)
    MOTOR:  mmax = fmax * h;  w = the row's entry
and per sweep the motor, axis, angular and off-axis rows in that order (_solve_one) - with tests/batch_joint_cases.py's rotate, cross,
M * v, invert and plan, and its dataflow under a random schedule; and the scenes and rigs of tests/test_gpu_world_batch_sliders.py,
seeded."""
import numpy as np

from mgf_amd import _capi
from tests import batch_hinge_cases as HC
from tests import batch_joint_cases as JC
from tests import batch_sensor_cases as SC

f32 = np.float32
LIMIT, MOTOR, LOCK = _capi.SLIDER_LIMIT, _capi.SLIDER_MOTOR, _capi.SLIDER_LOCK
_cross, _rotate, _mv, _invert, plan = JC._cross, JC._rotate, JC._mv, JC._invert, JC.plan
_dot, _finite, _rot64 = HC._dot, HC._finite, HC._rot64


# ---- the definition -----------------------------------------------------------------------------------------------------------------------
def setup(rig, h, w_row, state, lengths, ft=f32):
    """per slider a dict of the header's setup words from `state` - rows over every body of the batch: x, delta, q, inv_mass, inv_moment
    (column-major, as get() returns it); w_row: the target table's row, a float a slider"""
    off = SC.offsets(lengths)
    x = (state["x"].astype(f32) + state["delta"].astype(f32)).astype(ft)       # x + delta is the state's own f32 sum, as gather_state returns it
    q, im, I = state["q"].astype(ft), state["inv_mass"].astype(ft), state["inv_moment"].astype(ft).reshape(-1, 3, 3)
    h = ft(h)
    out = []
    with np.errstate(all="ignore"):
        for i, r in enumerate(rig):
            ga = int(off[r["world"]] + r["body"])
            gb = int(off[r["world"]] + r["other"]) if r["other"] >= 0 else -1
            flags = int(r["flags"])
            pa, pb = r["pa"].astype(ft), r["pb"].astype(ft)
            im_a, I_a = im[ga], I[ga]
            ra = _rotate(q[ga], pa, ft)
            Pa = x[ga] + ra
            A = _rotate(q[ga], r["ax"].astype(ft), ft)
            T1 = _rotate(q[ga], r["ua"].astype(ft), ft)
            T2 = _cross(A, T1)
            if gb >= 0:
                rb = _rotate(q[gb], pb, ft)
                Pb = x[gb] + rb
                im_b, I_b = im[gb], I[gb]
                B = _rotate(q[gb], r["bx"].astype(ft), ft)
                U1 = _rotate(q[gb], r["ub"].astype(ft), ft)
            else:
                rb, Pb, im_b, I_b = np.zeros(3, ft), pb, ft(0.0), np.zeros((3, 3), ft)
                B, U1 = r["bx"].astype(ft), r["ub"].astype(ft)
            U2 = _cross(B, U1)
            C = Pb - Pa
            s = ft(r["beta"]) / h
            ca = ra + C
            d = _dot(C, A)
            ims = im_a + im_b
            sA = _cross(ca, A)
            sB = _cross(rb, A)
            Km = (ims + _dot(sA, _mv(I_a, sA))) + _dot(sB, _mv(I_b, sB))
            pA1 = _cross(ca, T1)
            pB1 = _cross(rb, T1)
            g1 = _dot(C, T1) * s
            pA2 = _cross(ca, T2)
            pB2 = _cross(rb, T2)
            g2 = _dot(C, T2) * s
            ja1, ja2, jb1, jb2 = _mv(I_a, pA1), _mv(I_a, pA2), _mv(I_b, pB1), _mv(I_b, pB2)
            k11 = (ims + _dot(pA1, ja1)) + _dot(pB1, jb1)
            k22 = (ims + _dot(pA2, ja2)) + _dot(pB2, jb2)
            k12 = _dot(pA1, ja2) + _dot(pB1, jb2)
            k21 = _dot(pA2, ja1) + _dot(pB2, jb1)
            d2 = k11 * k22 - k12 * k21
            m11 = k22 / d2
            m12 = -k12 / d2
            m21 = -k21 / d2
            m22 = k11 / d2
            e = ((_cross(A, B) + _cross(T1, U1)) + _cross(T2, U2)) * ft(0.5)
            gw = e * s
            Kw = I_a + I_b
            ok, Kwinv = _invert(Kw)
            lo, hi = ft(r["lo"]), ft(r["hi"])
            side, lb = 0, ft(0.0)
            if flags & LOCK:
                side, lb = 2, (lo - d) * s
            elif flags & LIMIT and d < lo:
                side, lb = -1, (lo - d) * s
            elif flags & LIMIT and d > hi:
                side, lb = 1, -((d - hi) * s)
            motor = bool(flags & MOTOR)
            mmax, w = ft(0.0), ft(0.0)
            if motor:
                mmax = ft(r["fmax"]) * h
                w = ft(w_row[i])
            skip = (not ok or d2 == 0 or (flags != 0 and Km == 0) or not _finite(ra, rb, sA, sB, pA1, pA2, pB1, pB2, g1, g2, gw, m11, m12, m21, m22, Km, Kwinv, lb) or
                    (motor and (np.isnan(mmax) or not np.isfinite(w))))
            for a in (ra, rb, sA, sB, pA1, pB2, g1, g2, gw, m11, Km, lb, mmax, w, d, e) + ((Kwinv,) if ok else ()):
                assert a.dtype == ft, a.dtype
            out.append(dict(ga=ga, gb=gb, skip=bool(skip), im_a=im_a, I_a=I_a, im_b=im_b, I_b=I_b, A=A, T1=T1, T2=T2, sA=sA, sB=sB, pA1=pA1, pA2=pA2, pB1=pB1, pB2=pB2,
                            g1=g1, g2=g2, gw=gw, m=(m11, m12, m21, m22), Km=Km, Kwinv=Kwinv, side=side, lb=lb, motor=motor, mmax=mmax, w=w, C=C, d=d, e=e))
    return out


def _solve_one(S, v, om, acc, i, ft):
    """one turn of slider i: the motor, the axis row, the three angular rows and the two off-axis rows; acc row i: (p1, p2, al, am, aw.xyz, 0)"""
    if S["skip"]:
        return
    ga, gb, A, I_a, I_b, im_a, im_b, Km = S["ga"], S["gb"], S["A"], S["I_a"], S["I_b"], S["im_a"], S["im_b"], S["Km"]
    zero = np.zeros(3, ft)

    def rate(n, a, b):
        vb, ob = (v[gb], om[gb]) if gb >= 0 else (zero, zero)
        return (_dot(vb - v[ga], n) + _dot(ob, b)) - _dot(om[ga], a)

    def apply(n, a, b, lam):
        v[ga] = v[ga] - n * (lam * im_a)
        om[ga] = om[ga] - _mv(I_a, a * lam)
        if gb >= 0:
            v[gb] = v[gb] + n * (lam * im_b)
            om[gb] = om[gb] + _mv(I_b, b * lam)
    with np.errstate(all="ignore"):
        if S["motor"]:
            am, mmax = acc[i, 3], S["mmax"]
            lam = (S["w"] - rate(A, S["sA"], S["sB"])) / Km
            t = am + lam
            if t < -mmax:
                t = -mmax
            if t > mmax:
                t = mmax
            lam = t - am
            acc[i, 3] = t
            apply(A, S["sA"], S["sB"], lam)
        if S["side"] != 0:
            al = acc[i, 2]
            lam = (S["lb"] - rate(A, S["sA"], S["sB"])) / Km
            t = al + lam
            if S["side"] == -1:
                if t < 0:
                    t = ft(0.0)
            if S["side"] == 1:
                if t > 0:
                    t = ft(0.0)
            lam = t - al
            acc[i, 2] = t
            apply(A, S["sA"], S["sB"], lam)
        ob = om[gb] if gb >= 0 else zero
        L = -_mv(S["Kwinv"], (ob - om[ga]) + S["gw"])
        om[ga] = om[ga] - _mv(I_a, L)
        if gb >= 0:
            om[gb] = om[gb] + _mv(I_b, L)
        acc[i, 4:7] = acc[i, 4:7] + L
        m11, m12, m21, m22 = S["m"]
        r1 = rate(S["T1"], S["pA1"], S["pB1"]) + S["g1"]
        r2 = rate(S["T2"], S["pA2"], S["pB2"]) + S["g2"]
        l1 = -(m11 * r1 + m12 * r2)
        l2 = -(m21 * r1 + m22 * r2)
        n = S["T1"] * l1 + S["T2"] * l2
        v[ga] = v[ga] - n * im_a
        om[ga] = om[ga] - _mv(I_a, S["pA1"] * l1 + S["pA2"] * l2)
        if gb >= 0:
            v[gb] = v[gb] + n * im_b
            om[gb] = om[gb] + _mv(I_b, S["pB1"] * l1 + S["pB2"] * l2)
        acc[i, 0] = acc[i, 0] + l1
        acc[i, 1] = acc[i, 1] + l2
        assert L.dtype == ft and l1.dtype == ft and n.dtype == ft


def solve(rig, h, iters, w_row, state, lengths, ft=f32, schedule=None):
    """(v, omega, impulses [n, 8], skipped) after one call: `iters` sweeps over the sliders of every world in the rig's order.
    w_row: the target table's row (None: zeros).  schedule: a numpy Generator - the sweeps run by the PLAN's dataflow instead (a slider
    of sweep `it` is solved once prog[slot] == it * deg + rank on both its slots), the ready slider picked at random"""
    w_row = np.zeros(len(rig), f32) if w_row is None else w_row
    S = setup(rig, h, w_row, state, lengths, ft)
    v, om = state["v"].astype(ft).copy(), state["omega"].astype(ft).copy()
    acc = np.zeros((len(rig), 8), ft)
    if schedule is None:
        for w in sorted(set(rig["world"].tolist())):
            mine = np.flatnonzero(rig["world"] == w)
            for _ in range(iters):
                for i in mine:
                    _solve_one(S[i], v, om, acc, i, ft)
    else:
        items, joints, slots = plan(rig)
        for world, first, count, n_slots, first_slot in items:
            prog = [0] * n_slots
            it = [0] * count
            left = count * iters
            while left:
                ready = [p for p in range(count) if it[p] < iters and all(
                    prog[s] == it[p] * slots[first_slot + s][1] + r for s, r in zip(joints[first + p][1:3], joints[first + p][3:5]) if s >= 0)]
                assert ready, "the earliest unsolved slider is always ready"
                p = int(schedule.choice(ready))
                i = joints[first + p][0]
                _solve_one(S[i], v, om, acc, i, ft)
                for s in joints[first + p][1:3]:
                    if s >= 0:
                        prog[s] += 1
                it[p] += 1
                left -= 1
    return v, om, acc, np.array([s["skip"] for s in S], bool)


def residuals(S, v, om):
    """the rows of one slider's setup `S` under the velocities v, omega, in float64: (|(omega_b - omega_a) + gw|, |rate(T1) + g1|,
    |rate(T2) + g2|, rate(A))"""
    d = np.float64
    ga, gb = S["ga"], S["gb"]
    ob = om[gb].astype(d) if gb >= 0 else np.zeros(3)
    vb = v[gb].astype(d) if gb >= 0 else np.zeros(3)
    dv, oa = vb - v[ga].astype(d), om[ga].astype(d)

    def rate(n, a, b):
        return float(dv @ S[n].astype(d) + ob @ S[b].astype(d) - oa @ S[a].astype(d))
    return (float(np.linalg.norm((ob - oa) + S["gw"].astype(d))), abs(rate("T1", "pA1", "pB1") + d(S["g1"])), abs(rate("T2", "pA2", "pB2") + d(S["g2"])),
            rate("A", "sA", "sB"))


def frames_world(rig, state, lengths):
    """(A, T1, T2, B, U1, U2, C) of every slider in the world's frame from state rows, float64; C the gap Pb - Pa"""
    off = SC.offsets(lengths)
    d = np.float64
    q = state["q"].astype(d)
    x = state["x"].astype(d) + (state["delta"].astype(d) if "delta" in (state.dtype.names if isinstance(state, np.ndarray) else state) else 0.0)
    ga = off[rig["world"]] + rig["body"]
    gb = np.where(rig["other"] >= 0, off[rig["world"]] + rig["other"], ga)
    far = (rig["other"] >= 0)[:, None]
    A, T1 = _rot64(q[ga], rig["ax"].astype(d)), _rot64(q[ga], rig["ua"].astype(d))
    B = np.where(far, _rot64(q[gb], rig["bx"].astype(d)), rig["bx"].astype(d))
    U1 = np.where(far, _rot64(q[gb], rig["ub"].astype(d)), rig["ub"].astype(d))
    Pa = x[ga] + _rot64(q[ga], rig["pa"].astype(d))
    Pb = np.where(far, x[gb] + _rot64(q[gb], rig["pb"].astype(d)), rig["pb"].astype(d))
    return A, T1, np.cross(A, T1), B, U1, np.cross(B, U1), Pb - Pa


def travel(rig, state, lengths):
    """(d, off-axis gap, |e|) of every slider from state rows, float64: the travel dot(C, A), the length of C's part across the axis, and
    the length of the frames' error e"""
    A, T1, T2, B, U1, U2, C = frames_world(rig, state, lengths)
    d = np.sum(C * A, axis=1)
    e = (np.cross(A, B) + np.cross(T1, U1) + np.cross(T2, U2)) * 0.5
    return d, np.hypot(np.sum(C * T1, axis=1), np.sum(C * T2, axis=1)), np.linalg.norm(e, axis=1)


def slider(world, body, other=-1, pa=(0, 0, 0), pb=(0, 0, 0), ax=(0, 0, 1), ua=(1, 0, 0), bx=(0, 0, 1), ub=(1, 0, 0), beta=0.0, lo=0.0, hi=0.0, fmax=0.0,
           flags=0):
    r = np.zeros(1, _capi.SLIDER_DTYPE)
    r["world"], r["body"], r["other"], r["flags"], r["pa"], r["pb"], r["beta"], r["fmax"] = world, body, other, flags, pa, pb, beta, fmax
    r["ax"], r["ua"], r["bx"], r["ub"], r["lo"], r["hi"] = ax, ua, bx, ub, lo, hi
    return r


def place(rig, state, lengths, seed, tilt=0.0, shift=0.0):
    """pa, pb, ax, ua, bx, ub of `rig`: the anchor at the midpoint of the two bodies' centres (a slider to the world: at its body's
    centre), a seeded axis, by slider_frames - no gap, aligned frames and d = 0 in `state`; then, with tilt and shift, other's frame
    turned by a seeded rotation of up to `tilt` radians and its anchor moved by a seeded vector of up to `shift` (float64, rounded once)"""
    rng = np.random.default_rng(seed)
    n = len(rig)
    off = SC.offsets(lengths)
    ga = off[rig["world"]] + rig["body"]
    gb = np.where(rig["other"] >= 0, off[rig["world"]] + rig["other"], ga)
    x = (state["x"].astype(f32) + state["delta"].astype(f32)).astype(np.float64)
    q = state["q"].astype(np.float64)
    far = (rig["other"] >= 0)[:, None]
    qb = np.where(far, q[gb], 0.0)
    anchor = (x[ga] + x[gb]) / 2
    axis = rng.normal(0, 1, (n, 3))
    fr = _capi.slider_frames({"x": x[ga], "q": q[ga]}, {"x": x[gb], "q": qb}, anchor, axis)
    for k, a in fr.items():
        rig[k] = a
    if tilt or shift:
        A, T1, T2, B, U1, U2, C = frames_world(rig, state, lengths)
        w = rng.normal(0, 1, (n, 3))
        w *= (rng.uniform(0.3, 1.0, (n, 1)) * tilt) / np.linalg.norm(w, axis=1, keepdims=True)
        ang = np.linalg.norm(w, axis=1, keepdims=True)
        k = w / ang

        def turn(p):   # Rodrigues
            return p * np.cos(ang) + np.cross(k, p) * np.sin(ang) + k * np.sum(k * p, axis=1, keepdims=True) * (1 - np.cos(ang))
        t = rng.normal(0, 1, (n, 3))
        t *= (rng.uniform(0.3, 1.0, (n, 1)) * shift) / np.linalg.norm(t, axis=1, keepdims=True)
        conj = q[gb] * np.array([1.0, -1.0, -1.0, -1.0])
        Bn, Un, Pn = turn(B), turn(U1), anchor + t
        rig["bx"], rig["ub"] = np.where(far, _rot64(conj, Bn), Bn), np.where(far, _rot64(conj, Un), Un)
        rig["pb"] = np.where(far, _rot64(conj, Pn - x[gb]), Pn)
    return rig


# ---- the scenes ---------------------------------------------------------------------------------------------------------------------------
BIG, MAX, LENGTHS = JC.BIG, _capi.BATCH_MAX_WORLD_SLIDERS, JC.LENGTHS
BARE, ANCHOR, CHAIN, CHAIN_REV, STAR, PAIR, RING, FULL, EMPTY = range(9)
SETTLE_TICKS = JC.SETTLE_TICKS
slider_scenes, written_state, synthetic_state = JC.joint_scenes, JC.written_state, JC.synthetic_state
ROWS = 3                                   # rows of the seeded target table
TILT, SHIFT = 0.1, 0.05                    # how far the seeded rig's frames are off: radians, length units
# the flag cases, dealt round the sliders of every rig in this order
CASES = ("none", "limit_inside", "limit_below", "limit_above", "limit_point", "motor_free", "motor_capped", "motor_zero", "both", "lock")
CAPPED_FMAX = 1.0e-3                       # a cap the first sweep's impulse exceeds: mmax = fmax * h = 1.7e-5 beside |w - rate| / Km of 1e-2 and more


def deal_cases(rig, state, lengths, first=0):
    """the flag cases spread over the sliders of `rig`, case (first + i) % 10 on slider i, the ranges placed about each slider's PRESENT
    travel d (float64): inside - the row is off; below lo; above hi; lo == hi; a motor without a cap, with a cap the first sweep's
    impulse exceeds, with fmax = 0; LIMIT | MOTOR above hi; LOCK 0.05 off.  Returns the case of every slider"""
    d = travel(rig, state, lengths)[0]
    case = (first + np.arange(len(rig))) % len(CASES)
    lo_hi = {"none": (0.0, 0.0), "limit_inside": (-0.3, 0.4), "limit_below": (0.2, 0.9), "limit_above": (-0.9, -0.2), "limit_point": (0.1, 0.1),
             "motor_free": (0.0, 0.0), "motor_capped": (0.0, 0.0), "motor_zero": (0.0, 0.0), "both": (-0.6, -0.25), "lock": (0.05, 0.05)}
    for c, name in enumerate(CASES):
        at = np.flatnonzero(case == c)
        lo, hi = lo_hi[name]
        rig["lo"][at], rig["hi"][at] = d[at] + lo, d[at] + hi
        rig["flags"][at] = LOCK if name == "lock" else ((LIMIT if name.startswith("limit") or name == "both" else 0) | (MOTOR if name.startswith("motor") or name == "both" else 0))
        rig["fmax"][at] = {"motor_free": np.inf, "motor_capped": CAPPED_FMAX, "both": np.inf}.get(name, 0.0)
    assert np.all(rig["lo"] <= rig["hi"])
    return case


def main_rig(lengths, state, beta=0.2, seed=709):
    """(rig, planted, W): tests/batch_joint_cases.py's main_rig for who is tied to whom - ANCHOR one slider to the world, CHAIN a chain of
    five listed in order, CHAIN_REV the same in reverse, STAR six on one body, PAIR two on one pair, RING a ring of four, FULL MAX
    shuffled sliders over BIG bodies with bare bodies in between, the worlds interleaved in the caller's array - placed about the
    midpoints with seeded axes (place), other's frame up to TILT radians and SHIFT length units off, the flag cases dealt round
    (deal_cases), and W the seeded target table of ROWS rows.  planted: the sliders that are skipped - an arm of 3e38, and a MOTOR
    slider whose target is NaN in every row.
    state: rows with x, delta and q of every body."""
    rng = np.random.default_rng(seed)
    x = (state["x"] + state["delta"]).astype(f32)
    jr, planted = JC.main_rig(lengths, x, beta=beta)
    n = len(jr)
    rig = np.zeros(n, _capi.SLIDER_DTYPE)
    for k in ("world", "body", "other", "beta"):
        rig[k] = jr[k]
    place(rig, state, lengths, seed + 1, TILT, SHIFT)
    deal_cases(rig, state, lengths)
    for p in planted:                      # (on other's side: ra + C cancels an arm of body's, I_b * cross(rb, A) overflows whatever beta is)
        assert rig["other"][p] >= 0
        rig["pb"][p] = (3.0e38, 0.0, 0.0)
    W = rng.uniform(-2.0, 2.0, (ROWS, n)).astype(f32)
    nan_at = int(np.flatnonzero((rig["world"] == FULL) & ((rig["flags"] & MOTOR) != 0))[5])
    assert nan_at not in planted
    W[:, nan_at] = np.nan
    return rig, sorted(planted + [nan_at]), W


def late_sliders(lengths, state, seed=719):
    """(rig, W6): 24 sliders over the three worlds of tests/batch_rollout_cases.py's late-contact scenes - tests/batch_joint_cases.py's
    late_joints for who is tied to whom - placed in their rest pose (place), the flag cases dealt round about d = 0 with the ranges
    near enough for the motors to reach them, and a seeded target table of 6 rows"""
    jr = JC.late_joints(lengths)
    rig = np.zeros(len(jr), _capi.SLIDER_DTYPE)
    for k in ("world", "body", "other", "beta"):
        rig[k] = jr[k]
    place(rig, state, lengths, seed)
    deal_cases(rig, state, lengths, first=3)
    W = np.random.default_rng(seed + 1).uniform(-3.0, 3.0, (6, len(rig))).astype(f32)
    return rig, W


def chains_rig(n_worlds, n_bodies, chains=16, links=4):
    """tools/batch_slider_bench.py's rig: per world `chains` chains of links + 1 consecutive bodies, every other slider limited to
    [-0.3, 0.4], the others motorised without a cap; frames are the caller's to set (place)"""
    jr = JC.chains_rig(n_worlds, n_bodies, chains, links)
    rig = np.zeros(len(jr), _capi.SLIDER_DTYPE)
    for k in ("world", "body", "other", "beta"):
        rig[k] = jr[k]
    rig["lo"], rig["hi"] = -0.3, 0.4
    rig["flags"] = np.where(np.arange(len(rig)) % 2 == 0, LIMIT, MOTOR)
    rig["fmax"] = np.inf
    return rig


# ---- the behaviour check: a body on a vertical slider under gravity, a second one welded to it ----------------------------------------------
LIFT_LIMIT = (-0.3, 0.4)
LIFT_TICKS = 64
LIFT_ITERS = 4
LIFT_BETA = 0.2


def lift_scene():
    """two spheres r = 0.5 high above the floor of a wide box, 1.5 apart along x, at rest: they never meet and touch nothing; gravity is
    the scene's force rows"""
    from mgf_amd import scenes
    c = f32([[0.0, 12.0, 0.0], [1.5, 12.0, 0.0]])
    return scenes._scene("lift", scenes._spheres(c, 0.5), scenes.box_terrain(30.0, 40.0, (0.0, 0.0, 0.0)), v0=np.zeros((2, 3), f32))


def lift_rig(state, limit=True):
    """body 0 on a slider to the world along the vertical through its centre - the axis points up and the far anchor is the world's, so d grows as the body falls -, limited
    to LIFT_LIMIT; body 1 welded to body 0 by LOCK at the midpoint, lo = 0 - both placed by slider_frames in `state`"""
    x = (state["x"].astype(f32) + state["delta"].astype(f32)).astype(np.float64)
    q = state["q"].astype(np.float64)
    fr = _capi.slider_frames({"x": x[[0, 1]], "q": q[[0, 1]]}, {"x": x[[0, 0]], "q": np.stack([np.zeros(4), q[0]])}, [x[0], (x[0] + x[1]) / 2], [[0.0, 1.0, 0.0], [1.0, 0.0, 0.0]])
    rig = np.concatenate([slider(0, 0, -1, beta=LIFT_BETA, lo=LIFT_LIMIT[0], hi=LIFT_LIMIT[1], flags=LIMIT if limit else 0), slider(0, 1, 0, beta=LIFT_BETA, flags=LOCK)])
    for k, a in fr.items():
        rig[k] = a
    return rig


def lift_trace(rig, x_rows, q_rows, v_rows, omega_rows):
    """(d, rate) of the lift - slider 0 of lift_rig - and (gap, |e|) of the weld - slider 1 - from traced x [T, 2, 3], q, v and omega,
    float64.  gap: the whole of C, the weld holds d = 0 too"""
    d, rate, gap, tilt = [], [], [], []
    for x, q, v, om in zip(x_rows, q_rows, v_rows, omega_rows):
        st = {"x": x, "q": q}
        A, T1, T2, B, U1, U2, C = frames_world(rig, st, [2])
        d.append(C[0] @ A[0])
        ca = C[0] + _rot64(q[0].astype(np.float64), rig["pa"][0].astype(np.float64))
        rate.append(-(v[0].astype(np.float64) @ A[0]) - om[0].astype(np.float64) @ np.cross(ca, A[0]))
        dd, off_axis, e = travel(rig, st, [2])
        gap.append(np.linalg.norm(C[1]))
        tilt.append(e[1])
    return np.array(d), np.array(rate), np.array(gap), np.array(tilt)


def lift_verdict(d, rate, dt):
    """(inside, excursion, margin): does d stay within LIFT_LIMIT widened by twice the largest |rate| * dt of the trace - a limit acts
    from the call after the travel passed it, so one tick's travel is the definition's own overshoot -, how far it leaves LIFT_LIMIT at
    most, and that margin"""
    margin = 2.0 * float(np.abs(rate).max()) * float(dt)
    out = max(float((LIFT_LIMIT[0] - d).max()), float((d - LIFT_LIMIT[1]).max()), 0.0)
    return out <= margin, out, margin


def lift_sim(limit, ticks=LIFT_TICKS, iters=LIFT_ITERS):
    """the lift on the CPU: the float64 restatement of the sliders ahead of every tick, and for the tick a stand-in - v += g dt,
    x += v dt, q += dt / 2 (0, omega) q, normalised: free flight, the lift touches nothing.  Returns lift_trace's four rows"""
    sc = lift_scene()
    d = np.float64
    dt = d(sc["dt"])
    n = 2
    st = {"x": sc["comps"]["p"].astype(d), "delta": np.zeros((n, 3)), "q": np.tile([1.0, 0, 0, 0], (n, 1)), "v": sc["v0"].astype(d), "omega": np.zeros((n, 3)),
          "inv_mass": 1.0 / sc["mass"].astype(d), "inv_moment": np.tile((np.eye(3) / (0.4 * 0.25)).reshape(9), (n, 1)) / sc["mass"].astype(d)[:, None]}
    rig = lift_rig({k: st[k].astype(f32) for k in ("x", "delta", "q")}, limit)
    xs, qs, vs, oms = [], [], [], []
    for _ in range(ticks):
        v, om, _, sk = solve(rig, dt, iters, None, st, [n], ft=d)
        assert not sk.any()
        v = v + sc["force"].astype(d) * dt
        st["x"] = st["x"] + v * dt
        w, q = om, st["q"]
        dq = np.stack([-(w * q[:, 1:4]).sum(1), w[:, 0] * q[:, 0] + w[:, 1] * q[:, 3] - w[:, 2] * q[:, 2], w[:, 1] * q[:, 0] + w[:, 2] * q[:, 1] - w[:, 0] * q[:, 3],
                       w[:, 2] * q[:, 0] + w[:, 0] * q[:, 2] - w[:, 1] * q[:, 1]], axis=1)
        q = q + dq * (dt / 2)
        st["q"], st["v"], st["omega"] = q / np.linalg.norm(q, axis=1, keepdims=True), v, om
        xs.append(st["x"].copy())
        qs.append(st["q"].copy())
        vs.append(v.copy())
        oms.append(om.copy())
    return lift_trace(rig, np.array(xs), np.array(qs), np.array(vs), np.array(oms))
