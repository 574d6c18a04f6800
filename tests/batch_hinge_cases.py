"""Shared by the tests of a batch's hinges (mgf_batch_set_hinges / _set_hinge_targets / _solve_hinges / _solve_hinges_dev, and the hinges
of a rollout), without a GPU: a numpy restatement of the header's definition, f32 operation by f32 operation - the ball joint's setup
lines, then
    A = rotate(q_a, ax);  T1 = rotate(q_a, ua);  T2 = cross(A, T1);  B = rotate(q_b, bx);  U1 = rotate(q_b, ub)   (other == -1: B = bx, U1 = ub)
    n1 = cross(B, T1);  n2 = cross(B, T2);  g1 = dot(B, T1) * s;  g2 = dot(B, T2) * s;  J(n) = I_a * n + I_b * n
    k_ij = dot(n_i, J(n_j));  d2 = k11 * k22 - k12 * k21;  m11 = k22 / d2;  m12 = -k12 / d2;  m21 = -k21 / d2;  m22 = k11 / d2;  Km = dot(A, J(A))
    c = dot(U1, T1);  sn = dot(U1, T2);  cphi = c * cm + sn * sm;  sphi = sn * cm - c * sm
    LIMIT and cphi <= ch:  err = fabs(sphi) * ch - cphi * sh;  sphi >= 0: side = +1, lb = -(err * s);  else side = -1, lb = err * s
    MOTOR:  mmax = tmax * h;  w = the row's entry
and per sweep the motor, limit, angular and point rows in that order (_solve_one) - with tests/batch_joint_cases.py's rotate, cross,
M * v, invert and plan, and its dataflow under a random schedule; and the scenes and rigs of tests/test_gpu_world_batch_hinges.py,
seeded."""
import numpy as np

from mgf_amd import _capi
from tests import batch_joint_cases as JC
from tests import batch_sensor_cases as SC

f32 = np.float32
LIMIT, MOTOR = _capi.HINGE_LIMIT, _capi.HINGE_MOTOR
_cross, _rotate, _mv, _invert, _k_col, plan = JC._cross, JC._rotate, JC._mv, JC._invert, JC._k_col, JC.plan


# ---- the definition -----------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _finite(*words):
    return all(bool(np.all(np.isfinite(w))) for w in words)


def setup(rig, h, w_row, state, lengths, ft=f32):
    """per hinge a dict of the header's setup words from `state` - rows over every body of the batch: x, delta, q, inv_mass, inv_moment
    (column-major, as get() returns it); w_row: the target table's row, a float a hinge"""
    off = SC.offsets(lengths)
    x = (state["x"].astype(f32) + state["delta"].astype(f32)).astype(ft)       # x + delta is the state's own f32 sum, as gather_state returns it
    q, im, I = state["q"].astype(ft), state["inv_mass"].astype(ft), state["inv_moment"].astype(ft).reshape(-1, 3, 3)
    h = ft(h)
    E = np.eye(3, dtype=ft)
    out = []
    with np.errstate(all="ignore"):
        for i, r in enumerate(rig):
            ga = int(off[r["world"]] + r["body"])
            gb = int(off[r["world"]] + r["other"]) if r["other"] >= 0 else -1
            flags = int(r["flags"])
            pa, pb = r["pa"].astype(ft), r["pb"].astype(ft)
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
            C = Pb - Pa
            s = ft(r["beta"]) / h
            bias = C * s
            K = [_k_col(E[k], im[ga], I[ga], ra) + _k_col(E[k], im_b, I_b, rb) for k in range(3)]
            ok, Kinv = _invert(K)
            n1 = _cross(B, T1)
            n2 = _cross(B, T2)
            g1 = _dot(B, T1) * s
            g2 = _dot(B, T2) * s
            I_a = I[ga]

            def J(n):
                return _mv(I_a, n) + _mv(I_b, n)
            j1, j2 = J(n1), J(n2)
            k11, k12, k21, k22 = _dot(n1, j1), _dot(n1, j2), _dot(n2, j1), _dot(n2, j2)
            d2 = k11 * k22 - k12 * k21
            m11 = k22 / d2
            m12 = -k12 / d2
            m21 = -k21 / d2
            m22 = k11 / d2
            Km = _dot(A, J(A))
            cm, sm, ch, sh = ft(r["cm"]), ft(r["sm"]), ft(r["ch"]), ft(r["sh"])
            c = _dot(U1, T1)
            sn = _dot(U1, T2)
            cphi = c * cm + sn * sm
            sphi = sn * cm - c * sm
            side, lb = 0, ft(0.0)
            if flags & LIMIT and cphi <= ch:
                err = np.abs(sphi) * ch - cphi * sh
                if sphi >= 0:
                    side, lb = 1, -(err * s)
                else:
                    side, lb = -1, err * s
            motor = bool(flags & MOTOR)
            mmax, w = ft(0.0), ft(0.0)
            if motor:
                mmax = ft(r["tmax"]) * h
                w = ft(w_row[i])
            skip = (not ok or not _finite(ra, rb, bias, Kinv) or d2 == 0 or (flags & (LIMIT | MOTOR) and Km == 0) or
                    not _finite(n1, n2, g1, g2, m11, m12, m21, m22, Km, lb) or (motor and (np.isnan(mmax) or not np.isfinite(w))))
            for a in (ra, rb, bias, n1, n2, g1, g2, m11, Km, lb, mmax, w, cphi, sphi) + ((Kinv,) if ok else ()):
                assert a.dtype == ft, a.dtype
            out.append(dict(ga=ga, gb=gb, ra=ra, rb=rb, bias=bias, Kinv=Kinv, skip=bool(skip), im_a=im[ga], I_a=I_a, im_b=im_b, I_b=I_b, A=A, n1=n1, n2=n2,
                            g1=g1, g2=g2, m=(m11, m12, m21, m22), Km=Km, side=side, lb=lb, motor=motor, mmax=mmax, w=w, C=C, cphi=cphi, sphi=sphi, c=c, sn=sn))
    return out


def _solve_one(H, v, om, acc, i, ft):
    """one turn of hinge i: the motor, the limit, the two angular rows and the point; acc row i: (acc.xyz, a1, a2, al, am, 0)"""
    if H["skip"]:
        return
    ga, gb, A, I_a, I_b, Km = H["ga"], H["gb"], H["A"], H["I_a"], H["I_b"], H["Km"]
    zero = np.zeros(3, ft)

    def wd():
        return (om[gb] if gb >= 0 else zero) - om[ga]

    def turn(imp):
        om[ga] = om[ga] - _mv(I_a, imp)
        if gb >= 0:
            om[gb] = om[gb] + _mv(I_b, imp)
    with np.errstate(all="ignore"):
        if H["motor"]:
            am, mmax = acc[i, 6], H["mmax"]
            lam = (H["w"] - _dot(wd(), A)) / Km
            t = am + lam
            if t < -mmax:
                t = -mmax
            if t > mmax:
                t = mmax
            lam = t - am
            acc[i, 6] = t
            turn(A * lam)
        if H["side"] != 0:
            al = acc[i, 5]
            lam = (H["lb"] - _dot(wd(), A)) / Km
            t = al + lam
            if H["side"] < 0:
                if t < 0:
                    t = ft(0.0)
            elif t > 0:
                t = ft(0.0)
            lam = t - al
            acc[i, 5] = t
            turn(A * lam)
        m11, m12, m21, m22 = H["m"]
        d = wd()
        r1 = _dot(d, H["n1"]) + H["g1"]
        r2 = _dot(d, H["n2"]) + H["g2"]
        l1 = -(m11 * r1 + m12 * r2)
        l2 = -(m21 * r1 + m22 * r2)
        turn(H["n1"] * l1 + H["n2"] * l2)
        acc[i, 3] = acc[i, 3] + l1
        acc[i, 4] = acc[i, 4] + l2
        ra, rb = H["ra"], H["rb"]
        Va = v[ga] + _cross(om[ga], ra)
        Vb = v[gb] + _cross(om[gb], rb) if gb >= 0 else zero
        P = _mv(H["Kinv"], (Vb - Va) + H["bias"])
        v[ga] = v[ga] + P * H["im_a"]
        om[ga] = om[ga] + _mv(I_a, _cross(ra, P))
        if gb >= 0:
            Pn = -P
            v[gb] = v[gb] + Pn * H["im_b"]
            om[gb] = om[gb] + _mv(I_b, _cross(rb, Pn))
        acc[i, 0:3] = acc[i, 0:3] + P
        assert P.dtype == ft and l1.dtype == ft


def solve(rig, h, iters, w_row, state, lengths, ft=f32, schedule=None):
    """(v, omega, impulses [n, 8], skipped) after one call: `iters` sweeps over the hinges of every world in the rig's order.
    w_row: the target table's row (None: zeros).  schedule: a numpy Generator - the sweeps run by the PLAN's dataflow instead (a hinge
    of sweep `it` is solved once prog[slot] == it * deg + rank on both its slots), the ready hinge picked at random"""
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
                assert ready, "the earliest unsolved hinge is always ready"
                p = int(schedule.choice(ready))
                i = joints[first + p][0]
                _solve_one(S[i], v, om, acc, i, ft)
                for s in joints[first + p][1:3]:
                    if s >= 0:
                        prog[s] += 1
                it[p] += 1
                left -= 1
    return v, om, acc, np.array([s["skip"] for s in S], bool)


def residuals(H, v, om):
    """the rows of one hinge's setup `H` under the velocities v, omega, in float64: (|(Vb - Va) + bias|, |wd . n1 + g1|, |wd . n2 + g2|,
    wd . A)"""
    d = np.float64
    ga, gb = H["ga"], H["gb"]
    ob = om[gb].astype(d) if gb >= 0 else np.zeros(3)
    Va = v[ga].astype(d) + np.cross(om[ga].astype(d), H["ra"].astype(d))
    Vb = v[gb].astype(d) + np.cross(ob, H["rb"].astype(d)) if gb >= 0 else np.zeros(3)
    wd = ob - om[ga].astype(d)
    return (float(np.linalg.norm((Vb - Va) + H["bias"].astype(d))), abs(float(wd @ H["n1"].astype(d) + d(H["g1"]))),
            abs(float(wd @ H["n2"].astype(d) + d(H["g2"]))), float(wd @ H["A"].astype(d)))


def _rot64(q, p):
    s, v = q[..., 0:1], q[..., 1:4]
    return np.cross(v, np.cross(v, p) + p * s) * 2.0 + p


def frames_world(rig, state, lengths):
    """(A, T1, T2, B, U1) of every hinge in the world's frame from state rows, float64"""
    off = SC.offsets(lengths)
    q = state["q"].astype(np.float64)
    ga = off[rig["world"]] + rig["body"]
    gb = np.where(rig["other"] >= 0, off[rig["world"]] + rig["other"], ga)
    far = (rig["other"] >= 0)[:, None]
    d = np.float64
    A, T1 = _rot64(q[ga], rig["ax"].astype(d)), _rot64(q[ga], rig["ua"].astype(d))
    B = np.where(far, _rot64(q[gb], rig["bx"].astype(d)), rig["bx"].astype(d))
    U1 = np.where(far, _rot64(q[gb], rig["ub"].astype(d)), rig["ub"].astype(d))
    return A, T1, np.cross(A, T1), B, U1


def thetas(rig, state, lengths):
    """the hinge angle atan2(dot(U1, T2), dot(U1, T1)) of every hinge from state rows, float64 (the tests' own: the library evaluates none)"""
    A, T1, T2, B, U1 = frames_world(rig, state, lengths)
    return np.arctan2(np.sum(U1 * T2, axis=1), np.sum(U1 * T1, axis=1))


def misalignment(rig, state, lengths):
    """|cross(A, B)| of every hinge, float64"""
    A, T1, T2, B, U1 = frames_world(rig, state, lengths)
    return np.linalg.norm(np.cross(A, B), axis=1)


gaps = JC.gaps


def set_limits(rig, lo, hi, at=None):
    """cm, sm, ch, sh of the hinges `at` (all) from lo and hi in radians: float64, rounded once - as WorldBatch.set_hinges forms them"""
    at = slice(None) if at is None else at
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    rig["cm"][at], rig["sm"][at], rig["ch"][at], rig["sh"][at] = np.cos(mid), np.sin(mid), np.cos(half), np.sin(half)
    return rig


def hinge(world, body, other=-1, pa=(0, 0, 0), pb=(0, 0, 0), ax=(0, 0, 1), ua=(1, 0, 0), bx=(0, 0, 1), ub=(1, 0, 0), beta=0.0, lo=0.0, hi=0.0, tmax=0.0,
          flags=0):
    r = np.zeros(1, _capi.HINGE_DTYPE)
    r["world"], r["body"], r["other"], r["flags"], r["pa"], r["pb"], r["beta"], r["tmax"] = world, body, other, flags, pa, pb, beta, tmax
    r["ax"], r["ua"], r["bx"], r["ub"] = ax, ua, bx, ub
    return set_limits(r, lo, hi)


def _perpendicular_pairs(rng, n):
    """n seeded pairs (unit axis, unit reference perpendicular to it), float32 - unit and perpendicular to rounding"""
    a = rng.normal(0, 1, (n, 3))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    u = np.cross(a, rng.normal(0, 1, (n, 3)))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return a.astype(f32), u.astype(f32)


def _far_frames(rig, state, lengths, rng, tilt=0.1):
    """bx, ub of `rig` from its ax, ua and `state` (float64, rounded once): other's axis `tilt` radians or less off body's as they lie, its
    reference turned about the axis by a seeded angle in (-pi, pi) - every hinge angle, and an axis error for the angular rows to remove"""
    n = len(rig)
    off = SC.offsets(lengths)
    q = state["q"].astype(np.float64)
    ga = off[rig["world"]] + rig["body"]
    gb = np.where(rig["other"] >= 0, off[rig["world"]] + rig["other"], ga)
    A, T1 = _rot64(q[ga], rig["ax"].astype(np.float64)), _rot64(q[ga], rig["ua"].astype(np.float64))
    T2 = np.cross(A, T1)
    B = A + (T1 * rng.uniform(-1, 1, (n, 1)) + T2 * rng.uniform(-1, 1, (n, 1))) * (tilt / np.sqrt(2.0))
    B /= np.linalg.norm(B, axis=1, keepdims=True)
    th = rng.uniform(-np.pi, np.pi, (n, 1))
    U = T1 * np.cos(th) + T2 * np.sin(th)
    U -= B * np.sum(U * B, axis=1, keepdims=True)
    U /= np.linalg.norm(U, axis=1, keepdims=True)
    conj = q[gb] * np.array([1.0, -1.0, -1.0, -1.0])
    far = (rig["other"] >= 0)[:, None]
    rig["bx"], rig["ub"] = np.where(far, _rot64(conj, B), B), np.where(far, _rot64(conj, U), U)


# ---- the scenes ---------------------------------------------------------------------------------------------------------------------------
BIG, MAX, LENGTHS = JC.BIG, _capi.BATCH_MAX_WORLD_HINGES, JC.LENGTHS
BARE, ANCHOR, CHAIN, CHAIN_REV, STAR, PAIR, RING, FULL, EMPTY = range(9)
SETTLE_TICKS = JC.SETTLE_TICKS
hinge_scenes, written_state, synthetic_state = JC.joint_scenes, JC.written_state, JC.synthetic_state
ROWS = 3                                   # rows of the seeded target table
# the flag cases, dealt round the hinges of every rig in this order
CASES = ("none", "limit_inside", "limit_below", "limit_above", "limit_wide", "limit_point", "motor_free", "motor_capped", "motor_zero", "both")
CAPPED_TMAX = 1.0e-3                       # a cap the first sweep's impulse exceeds: mmax = tmax * h = 1.7e-5 beside |w - rate| / Km of 1e-2 and more


def deal_cases(rig, state, lengths, first=0):
    """the flag cases spread over the hinges of `rig`, case (first + i) % 10 on hinge i, the limits placed about each hinge's PRESENT angle
    (float64): inside - the row is off; below lo; above hi; a range wider than pi with the angle beyond pi from lo (a test on one sine
    of theta - lo takes it for inside or for below); lo == hi; a motor without a cap, with a cap the first sweep's impulse exceeds, with
    tmax = 0; both flags.  Returns the case of every hinge"""
    th = thetas(rig, state, lengths)
    case = (first + np.arange(len(rig))) % len(CASES)
    lo_hi = {"none": (0.0, 0.0), "limit_inside": (-0.3, 0.4), "limit_below": (0.2, 0.9), "limit_above": (-0.9, -0.2), "limit_wide": (-3.3, -0.1),
             "limit_point": (0.1, 0.1), "motor_free": (0.0, 0.0), "motor_capped": (0.0, 0.0), "motor_zero": (0.0, 0.0), "both": (-0.6, -0.25)}
    for c, name in enumerate(CASES):
        at = np.flatnonzero(case == c)
        lo, hi = lo_hi[name]
        set_limits(rig, th[at] + lo, th[at] + hi, at)
        rig["flags"][at] = (LIMIT if name.startswith("limit") or name == "both" else 0) | (MOTOR if name.startswith("motor") or name == "both" else 0)
        rig["tmax"][at] = {"motor_free": np.inf, "motor_capped": CAPPED_TMAX, "both": np.inf}.get(name, 0.0)
    return case


def main_rig(lengths, state, beta=0.2, seed=509):
    """(rig, planted, W): tests/batch_joint_cases.py's main_rig for who is tied to whom and where - ANCHOR one hinge to the world, CHAIN a
    chain of five listed in order, CHAIN_REV the same in reverse, STAR six on one body, PAIR two on one pair, RING a ring of four, FULL
    MAX shuffled hinges over BIG bodies with bare bodies in between, the worlds interleaved in the caller's array - with seeded axes and
    references on both ends, the flag cases dealt round (deal_cases), and W the seeded target table of ROWS rows.  planted: the hinges
    that are skipped - the joints' arm of 3e38, and a MOTOR hinge whose target is NaN in every row.
    state: rows with x, delta and q of every body."""
    rng = np.random.default_rng(seed)
    x = (state["x"] + state["delta"]).astype(f32)
    jr, planted = JC.main_rig(lengths, x, beta=beta)
    n = len(jr)
    rig = np.zeros(n, _capi.HINGE_DTYPE)
    for k in ("world", "body", "other", "pa", "pb", "beta"):
        rig[k] = jr[k]
    rig["ax"], rig["ua"] = _perpendicular_pairs(rng, n)
    _far_frames(rig, state, lengths, rng)
    deal_cases(rig, state, lengths)       # (CHAIN_REV ties CHAIN's pairs at CHAIN's anchors in the opposite order; its frames and cases are its own, as its state is)
    W = rng.uniform(-2.0, 2.0, (ROWS, n)).astype(f32)
    nan_at = int(np.flatnonzero((rig["world"] == FULL) & ((rig["flags"] & MOTOR) != 0))[5])
    assert nan_at not in planted
    W[:, nan_at] = np.nan
    return rig, sorted(planted + [nan_at]), W


def place(rig, state, lengths, seed):
    """pa, pb, ax, ua, bx, ub of `rig` by hinge_frames: the anchor at the midpoint of the two bodies' centres (a hinge to the world: at its
    body's centre), a seeded axis - no gap, parallel axes and theta = 0 in `state`"""
    rng = np.random.default_rng(seed)
    off = SC.offsets(lengths)
    ga = off[rig["world"]] + rig["body"]
    gb = np.where(rig["other"] >= 0, off[rig["world"]] + rig["other"], ga)
    x = (state["x"].astype(f32) + state["delta"].astype(f32)).astype(np.float64)
    q = state["q"].astype(np.float64)
    qb = np.where((rig["other"] >= 0)[:, None], q[gb], 0.0)
    fr = _capi.hinge_frames({"x": x[ga], "q": q[ga]}, {"x": x[gb], "q": qb}, (x[ga] + x[gb]) / 2, rng.normal(0, 1, (len(rig), 3)))
    for k, a in fr.items():
        rig[k] = a
    return rig


def late_hinges(lengths, state, seed=519):
    """(rig, W6): 24 hinges over the three worlds of tests/batch_rollout_cases.py's late-contact scenes - tests/batch_joint_cases.py's
    late_joints for who is tied to whom - placed in their rest pose (place), the flag cases dealt round about theta = 0 with the limits
    near enough for the motors to reach them, and a seeded target table of 6 rows"""
    jr = JC.late_joints(lengths)
    rig = np.zeros(len(jr), _capi.HINGE_DTYPE)
    for k in ("world", "body", "other", "beta"):
        rig[k] = jr[k]
    place(rig, state, lengths, seed)
    deal_cases(rig, state, lengths, first=3)
    W = np.random.default_rng(seed + 1).uniform(-3.0, 3.0, (6, len(rig))).astype(f32)
    return rig, W


def chains_rig(n_worlds, n_bodies, chains=16, links=4):
    """tools/batch_hinge_bench.py's rig: per world `chains` chains of links + 1 consecutive bodies, every other hinge limited to
    [-0.5, 0.7], the others motorised without a cap; frames are the caller's to set (place)"""
    jr = JC.chains_rig(n_worlds, n_bodies, chains, links)
    rig = np.zeros(len(jr), _capi.HINGE_DTYPE)
    for k in ("world", "body", "other", "beta"):
        rig[k] = jr[k]
    set_limits(rig, -0.5, 0.7)
    rig["flags"] = np.where(np.arange(len(rig)) % 2 == 0, LIMIT, MOTOR)
    rig["tmax"] = np.inf
    return rig


# ---- the behaviour check: a two-body arm pinned to the world -------------------------------------------------------------------------------
ARM_LIMIT = (-0.5, 0.7)
ARM_TICKS = 64
ARM_SPIN = 6.0                             # the outer body's initial turn about the elbow, rad/s: the elbow passes lo within a few ticks (arm_sim: it
                                           # stays within 0.085 of the range with the limit, margin 0.205, and leaves it by 6.0 without)
ARM_ITERS = 4


def arm_scene():
    """two spheres r = 0.5 high above the floor of a wide box, 1.5 apart along x and 1.2 apart along z - the hinge axis - so that they
    never meet; gravity is the scene's force rows"""
    from mgf_amd import scenes
    c = f32([[0.75, 12.0, 0.0], [2.25, 12.0, 1.2]])
    sc = scenes._scene("arm", scenes._spheres(c, 0.5), scenes.box_terrain(30.0, 40.0, (0.0, 0.0, 0.0)), v0=f32([[0.0, 0.0, 0.0], [0.0, 0.75 * ARM_SPIN, 0.0]]))
    sc["omega0"] = f32([[0.0, 0.0, 0.0], [0.0, 0.0, ARM_SPIN]])    # (the outer body turns about the elbow, 0.75 from its centre in x: v = omega x r)
    return sc


def arm_rig(state, limit=True):
    """body 0 hinged to the world at (0, 12, 0), body 1 to body 0 at the elbow (1.5, 12, 0.6), both about z, placed by hinge_frames in
    `state`; the elbow limited to ARM_LIMIT"""
    x = (state["x"].astype(f32) + state["delta"].astype(f32)).astype(np.float64)
    q = state["q"].astype(np.float64)
    fr = _capi.hinge_frames({"x": x[[0, 1]], "q": q[[0, 1]]}, {"x": x[[0, 0]], "q": np.stack([np.zeros(4), q[0]])}, [[0.0, 12.0, 0.0], [1.5, 12.0, 0.6]], [[0.0, 0.0, 1.0]])
    rig = np.concatenate([hinge(0, 0, -1, beta=0.2), hinge(0, 1, 0, beta=0.2, lo=ARM_LIMIT[0], hi=ARM_LIMIT[1], flags=LIMIT if limit else 0)])
    for k, a in fr.items():
        rig[k] = a
    return rig


def arm_trace_angles(rig, q_rows, omega_rows):
    """(theta, rate) of the elbow - hinge 1 of arm_rig - from traced q [T, 2, 4] and omega [T, 2, 3], float64; theta unwrapped"""
    th, rate = [], []
    for q, om in zip(q_rows, omega_rows):
        A, T1, T2, B, U1 = frames_world(rig, {"q": q}, [2])
        th.append(np.arctan2(U1[1] @ T2[1], U1[1] @ T1[1]))
        rate.append((om[0].astype(np.float64) - om[1].astype(np.float64)) @ A[1])
    return np.unwrap(np.array(th)), np.array(rate)


def arm_verdict(theta, rate, dt):
    """(inside, excursion, margin): does theta stay within ARM_LIMIT widened by twice the largest |rate| * dt of the trace - a limit acts
    from the call after the angle passed it, so one tick's travel is the definition's own overshoot -, how far it leaves ARM_LIMIT at
    most, and that margin"""
    margin = 2.0 * float(np.abs(rate).max()) * float(dt)
    out = max(float((ARM_LIMIT[0] - theta).max()), float((theta - ARM_LIMIT[1]).max()), 0.0)
    return out <= margin, out, margin


def arm_sim(limit, ticks=ARM_TICKS, iters=ARM_ITERS):
    """the arm on the CPU: the float64 restatement of the hinges ahead of every tick, and for the tick a stand-in - v += g dt,
    x += v dt, q += dt / 2 (0, omega) q, normalised: free flight, the arm touches nothing.  Returns (theta, rate) behind every tick"""
    sc = arm_scene()
    d = np.float64
    dt = d(sc["dt"])
    n = 2
    st = {"x": sc["comps"]["p"].astype(d), "delta": np.zeros((n, 3)), "q": np.tile([1.0, 0, 0, 0], (n, 1)), "v": sc["v0"].astype(d), "omega": sc["omega0"].astype(d),
          "inv_mass": 1.0 / sc["mass"].astype(d), "inv_moment": np.tile((np.eye(3) / (0.4 * 0.25)).reshape(9), (n, 1)) / sc["mass"].astype(d)[:, None]}
    rig = arm_rig({k: st[k].astype(f32) for k in ("x", "delta", "q")}, limit)
    qs, oms = [], []
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
        qs.append(st["q"].copy())
        oms.append(om.copy())
    return arm_trace_angles(rig, np.array(qs), np.array(oms))
