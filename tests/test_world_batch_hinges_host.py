"""The hinges of a batch (mgf_batch_set_hinges, mgf_batch_hinge_count, mgf_batch_set_hinge_targets, mgf_batch_set_hinge_targets_dev,
mgf_batch_solve_hinges, mgf_batch_solve_hinges_dev) without a GPU: the header, the library, the binding and the documents carry the
calls, the record of 112 bytes and the constants; the numpy restatement (tests/batch_hinge_cases.py) holds against itself in float64,
row by row; the plan's dataflow gives the sequential order's bits whatever the schedule; the float64 restatement holds a violated
limit, reaches a motor's target and stops at a motor's cap; hinge_frames places a hinge without gap, tilt or angle; what needs no device
is refused, in the header's order, with the rig unchanged; the launch sits behind the ball joints' and ahead of the tick; and the
kernel has k_batch_joint_solve's loop shape, no scratch and no spills."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mgf_amd
from mgf_amd import _capi
from tests import batch_hinge_cases as HC
from tests.util import ROOT, kernel_resources, read

f32 = np.float32
CALLS = ("mgf_batch_set_hinges", "mgf_batch_hinge_count", "mgf_batch_set_hinge_targets", "mgf_batch_set_hinge_targets_dev", "mgf_batch_solve_hinges",
         "mgf_batch_solve_hinges_dev")
RIG_FILE = "host_batch_hinge.inc"
H = f32(1.0 / 60.0)
NAMES = ["world", "body", "other", "flags", "pa", "beta", "pb", "tmax", "ax", "cm", "ua", "sm", "bx", "ch", "ub", "sh"]


def _seeded(beta=0.2):
    lens = list(HC.LENGTHS)
    st = HC.synthetic_state(lens)
    rig, planted, W = HC.main_rig(lens, st, beta=beta)
    return lens, st, rig, planted, W


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
def test_header_library_binding_and_documents_carry_the_calls_the_record_and_the_constants():
    h = read("include", "mgf_hip.h")
    flat_h = re.sub(r"\s+", " ", h)
    for sig in ("MGF_API mgf_status mgf_batch_set_hinges(mgf_batch* b, const mgf_batch_hinge* j, int64_t n);",
                "MGF_API int64_t mgf_batch_hinge_count(const mgf_batch* b);",
                "MGF_API mgf_status mgf_batch_set_hinge_targets(mgf_batch* b, const float* w, int64_t rows);",
                "MGF_API mgf_status mgf_batch_set_hinge_targets_dev(mgf_batch* b, const float* w_dev, int64_t rows);",
                "MGF_API mgf_status mgf_batch_solve_hinges(mgf_batch* b, float h, int32_t iters, int64_t row, float* impulse_out);",
                "MGF_API mgf_status mgf_batch_solve_hinges_dev(mgf_batch* b, float h, int32_t iters, int64_t row, float* impulse_out_dev);"):
        assert sig in flat_h, sig
    assert h.index("MGF_API mgf_status mgf_batch_solve_joints_dev(") < h.index("/* ---- hinge joints between bodies") < h.index("/* name in {")
    consts = (("MGF_HINGE_LIMIT", _capi.HINGE_LIMIT, 1), ("MGF_HINGE_MOTOR", _capi.HINGE_MOTOR, 2), ("MGF_BATCH_HINGE_LAUNCHES", _capi.BATCH_HINGE_LAUNCHES, 1),
              ("MGF_BATCH_ROLLOUT_HINGE_LAUNCHES_PER_TICK", _capi.BATCH_ROLLOUT_HINGE_LAUNCHES_PER_TICK, 1), ("MGF_BATCH_MAX_WORLD_HINGES", _capi.BATCH_MAX_WORLD_HINGES, 256))
    flat = re.sub(r"\s+", " ", read("INTEGRATION.md"))
    for name, value, want in consts:
        m = re.search(r"#define %s\s+(\d+)" % name, h)
        assert m and int(m.group(1)) == value == want, name
        assert re.search(r"pub const %s: (i64|u32) = %d;" % (name, want), flat), name
        assert getattr(mgf_amd, name[4:]) is getattr(_capi, name[4:]), name
    section = h[h.index("/* ---- hinge joints between bodies"):h.index("MGF_API mgf_status mgf_batch_solve_hinges_dev(")]
    for word in ("A = rotate(q_a, ax);  T1 = rotate(q_a, ua);  T2 = cross(A, T1)", "other == -1: B = bx;  U1 = ub;  omega_b = 0;  I_b = 0",
                 "n1 = cross(B, T1);  n2 = cross(B, T2);  g1 = dot(B, T1) * s;  g2 = dot(B, T2) * s", "J(n) = I_a * n + I_b * n", "d2 = k11 * k22 - k12 * k21",
                 "m11 = k22 / d2;  m12 = -k12 / d2;  m21 = -k21 / d2;  m22 = k11 / d2", "Km = dot(A, J(A))",
                 "c = dot(U1, T1);  sn = dot(U1, T2);  cphi = c * cm + sn * sm;  sphi = sn * cm - c * sm",
                 "LIMIT and cphi <= ch:  err = fabs(sphi) * ch - cphi * sh;  sphi >= 0: side = +1, lb = -(err * s);  else side = -1, lb = err * s",
                 "MOTOR:  mmax = tmax * h", "lam = (w - dot(wd, A)) / Km;  t = am + lam;  if (t < -mmax) t = -mmax;  if (t > mmax) t = mmax;  lam = t - am;  am = t",
                 "imp = A * lam;  omega_a = omega_a - I_a * imp;  omega_b = omega_b + I_b * imp",
                 "lam = (lb - dot(wd, A)) / Km;  t = al + lam;  side < 0: if (t < 0) t = 0;  side > 0: if (t > 0) t = 0;  lam = t - al;  al = t",
                 "r1 = dot(wd, n1) + g1;  r2 = dot(wd, n2) + g2;  l1 = -(m11 * r1 + m12 * r2);  l2 = -(m21 * r1 + m22 * r2)", "imp = n1 * l1 + n2 * l2",
                 "P = Kinv * ((Vb - Va) + bias)", "(acc.x, acc.y, acc.z, a1, a2, al, am, 0)", "hinges_skipped", "still takes its place in the order",
                 "untouched to the bit", "no warm start", "several components", "drive_launches", "rollout_launches", "the rig was not changed",
                 "nothing enqueued", "mgf_batch_add_bodies", "no float atomic", "NO arctangent", "min(t, rows - 1)", "one row of zeros", "is a brake", "ONCE",
                 "mgf_batch_step itself stays World::step, launch for launch", "OUT OF SCOPE", "interleaved sweep", "servo", "prismatic", "warm starting",
                 "speculatively", "lone mgf_world", "inside mgf_batch_step", "impulses per tick", "traced observation"):
        assert word in section, word
    assert '"hinges_skipped"' in h[h.index("/* name in {"):]
    # the record: 112 bytes, the same fields at the same offsets in the ctypes struct and the numpy dtype
    assert C.sizeof(_capi.BatchHinge) == 112 == _capi.HINGE_DTYPE.itemsize
    assert [f[0] for f in _capi.BatchHinge._fields_] == list(_capi.HINGE_DTYPE.names) == NAMES
    want_off = [0, 4, 8, 12] + [16 * w + o for w in range(1, 7) for o in (0, 12)]
    assert [_capi.HINGE_DTYPE.fields[k][1] for k in NAMES] == want_off == [getattr(_capi.BatchHinge, k).offset for k in NAMES]
    assert re.search(r"typedef struct mgf_batch_hinge \{\s*int32_t world, body, other; uint32_t flags;[^\n]*\n\s*mgf_vec3 pa; float beta;[^\n]*\n\s*mgf_vec3 pb; float tmax;[^\n]*\n"
                     r"\s*mgf_vec3 ax; float cm;[^\n]*\n\s*mgf_vec3 ua; float sm;[^\n]*\n\s*mgf_vec3 bx; float ch;[^\n]*\n\s*mgf_vec3 ub; float sh;[^\n]*\n\} mgf_batch_hinge;", h)
    lib = mgf_amd.load_library()
    vp, i64, i32, fl = C.c_void_p, C.c_int64, C.c_int32, C.c_float
    want = {"mgf_batch_set_hinges": (i32, [vp, vp, i64]), "mgf_batch_hinge_count": (i64, [vp]), "mgf_batch_set_hinge_targets": (i32, [vp, vp, i64]),
            "mgf_batch_set_hinge_targets_dev": (i32, [vp, vp, i64]), "mgf_batch_solve_hinges": (i32, [vp, fl, i32, i64, vp]),
            "mgf_batch_solve_hinges_dev": (i32, [vp, fl, i32, i64, vp])}
    for name in CALLS:
        assert name in _capi.SYMBOLS, name
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == want[name], name
    for method in ("set_hinges", "hinge_count", "set_hinge_targets", "set_hinge_targets_dev", "solve_hinges", "solve_hinges_dev"):
        assert callable(getattr(mgf_amd.WorldBatch, method)), method
    assert mgf_amd.HINGE_DTYPE is _capi.HINGE_DTYPE and mgf_amd.hinge_frames is _capi.hinge_frames
    for sig in ("pub fn mgf_batch_set_hinges(b: *mut mgf_batch, j: *const mgf_batch_hinge, n: i64) -> mgf_status;",
                "pub fn mgf_batch_hinge_count(b: *const mgf_batch) -> i64;",
                "pub fn mgf_batch_set_hinge_targets(b: *mut mgf_batch, w: *const f32, rows: i64) -> mgf_status;",
                "pub fn mgf_batch_set_hinge_targets_dev(b: *mut mgf_batch, w_dev: *const f32, rows: i64) -> mgf_status;",
                "pub fn mgf_batch_solve_hinges(b: *mut mgf_batch, h: f32, iters: i32, row: i64, impulse_out: *mut f32) -> mgf_status;",
                "pub fn mgf_batch_solve_hinges_dev(b: *mut mgf_batch, h: f32, iters: i32, row: i64, impulse_out_dev: *mut f32) -> mgf_status;",
                "pub struct mgf_batch_hinge { pub world: i32, pub body: i32, pub other: i32, pub flags: u32, pub pa: mgf_vec3, pub beta: f32, pub pb: mgf_vec3, pub tmax: f32, "
                "pub ax: mgf_vec3, pub cm: f32, pub ua: mgf_vec3, pub sm: f32, pub bx: mgf_vec3, pub ch: f32, pub ub: mgf_vec3, pub sh: f32 }",
                "pub fn set_hinges(", "pub fn hinge_count(", "pub fn set_hinge_targets(", "pub unsafe fn set_hinge_targets_dev(", "pub fn solve_hinges(",
                "pub unsafe fn solve_hinges_dev("):
        assert sig in flat, sig
    kernels = read("mgf_amd", "csrc", "kernels.h")
    assert kernels.index('#include "k_batch_joint.h"') < kernels.index('#include "k_batch_hinge.h"')
    assert "k_batch_hinge_solve<GATED> (k_batch_hinge.h)" in kernels
    hip = read("mgf_amd", "csrc", "mgf_hip.hip")
    assert hip.index('#include "host_batch_joint.inc"') < hip.index('#include "%s"' % RIG_FILE)
    design = read("DESIGN.md")
    assert design.index("### Joints between bodies") < design.index("### Hinges between bodies") < design.index("### Rollout touch traces")
    sub = design[design.index("### Hinges between bodies"):design.index("### Rollout touch traces")]
    for word in ("k_batch_hinge_solve", "done[k] == t && act[k] == t", "Compiler output", "Out of scope", "batch_hinge_bench.py", "MGF_BATCH_HINGE_LAUNCHES",
                 "MGF_BATCH_ROLLOUT_HINGE_LAUNCHES_PER_TICK", "MGF_BATCH_MAX_WORLD_HINGES", "__any", "kBatchSpinLimit", "bench.py", "Measured", "Not measured",
                 "min(t, rows - 1)"):
        assert word in sub, word
    readme = read("README.md")
    assert "set_hinges" in readme and "solve_hinges_dev" in readme and "set_hinge_targets" in readme
    assert os.path.exists(os.path.join(ROOT, "tools", "batch_hinge_bench.py"))
    for text in (h, design):   # the earlier sections that listed limits and motors as out of scope point here
        assert text.count("since: Hinge") >= 3, text.count("since: Hinge")


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
WORST_RESIDUAL = 3.47e-5   # measured: see the test below
RESIDUAL_BOUND = 8 * WORST_RESIDUAL


def test_the_definition_holds_against_itself_in_float64_row_by_row():
    """Every hinge of the seeded rig (tests/batch_hinge_cases.py: main_rig on synthetic_state, h = 1/60, beta = 0.2 and beta = 0, row 0 of
    the target table) solved ALONE for one sweep in f32 and in float64: the four residuals of the hinge's rows - |(Vb - Va) + bias|,
    |wd . n1 + g1|, |wd . n2 + g2| and the rate wd . A - are evaluated in float64 with the float64 run's own setup words, once under the
    f32 run's velocities and once under the float64 run's, and may differ by no more than a bound.  The reference is the float64
    restatement, never the library.
    Measured here on the CPU over the 2 x 275 hinges that are not skipped: the largest difference of any row is 3.47e-5, in the point
    row of a hinge whose bias is 167 (2.1e-7 of it) - WORST_RESIDUAL.  The bound allows 8 x that, 2.78e-4, for other seeds' rounding -
    RESIDUAL_BOUND."""
    worst, where = 0.0, None
    for beta in (0.2, 0.0):
        lens, st, rig, planted, W = _seeded(beta)
        S64 = HC.setup(rig, H, W[0], st, lens, np.float64)
        for i in range(len(rig)):
            one, w = rig[i:i + 1], W[0, i:i + 1]
            v, om, acc, sk = HC.solve(one, H, 1, w, st, lens)
            v64, om64, acc64, sk64 = HC.solve(one, H, 1, w, st, lens, ft=np.float64)
            assert sk.tolist() == [i in planted], i
            if sk[0]:
                assert not acc.any() and v.tobytes() == st["v"].tobytes() and om.tobytes() == st["omega"].tobytes()
                continue
            assert not sk64[0]
            r32, r64 = HC.residuals(S64[i], v, om), HC.residuals(S64[i], v64, om64)
            for row, (a, b) in enumerate(zip(r32, r64)):
                if abs(a - b) > worst:
                    worst, where = abs(a - b), (i, beta, row, float(np.linalg.norm(S64[i]["bias"])))
                assert abs(a - b) <= RESIDUAL_BOUND, (i, beta, row, a, b)
    print("worst difference of a row's residual, f32 against f64:", worst, "at (hinge, beta, row, |bias|)", where, "; bound", RESIDUAL_BOUND)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_seeded_rig_holds_every_case_and_its_dataflow_gives_the_sequential_orders_bits():
    lens, st, rig, planted, W = _seeded()
    n = len(rig)
    assert n == 1 + 4 + 4 + 6 + 2 + 4 + HC.MAX and np.any(np.diff(rig["world"]) < 0)        # interleaved in the caller's array
    items, joints, slots = HC.plan(rig)
    assert [it[0] for it in items] == [HC.ANCHOR, HC.CHAIN, HC.CHAIN_REV, HC.STAR, HC.PAIR, HC.RING, HC.FULL]     # no item for BARE and EMPTY
    assert [it[2] for it in items] == [1, 4, 4, 6, 2, 4, HC.MAX]
    # every flag case, in the state the rig was dealt for: the limit rows off, on from below, on from above; motors with every cap
    S = HC.setup(rig, H, W[0], st, lens)
    case = np.arange(n) % 10
    c, r = np.flatnonzero(rig["world"] == HC.CHAIN), np.flatnonzero(rig["world"] == HC.CHAIN_REV)
    for name, flags, side in (("none", 0, 0), ("limit_inside", 1, 0), ("limit_below", 1, -1), ("limit_above", 1, 1), ("limit_wide", 1, 1), ("limit_point", 1, -1),
                              ("motor_free", 2, 0), ("motor_capped", 2, 0), ("motor_zero", 2, 0), ("both", 3, 1)):
        at = np.flatnonzero(case == HC.CASES.index(name))
        assert len(at) >= 20 and all(rig["flags"][i] == flags and S[i]["side"] == side for i in at), name
    wide = np.flatnonzero(case == HC.CASES.index("limit_wide"))
    th = HC.thetas(rig, st, lens)
    for i in wide:   # the range is wider than pi and the angle lies beyond pi from lo: sin(theta - lo) < 0, as if theta were below lo
        half = np.arctan2(np.float64(rig["sh"][i]), np.float64(rig["ch"][i]))
        mid = np.arctan2(np.float64(rig["sm"][i]), np.float64(rig["cm"][i]))
        assert 2 * half > np.pi and np.sin(th[i] - (mid - half)) < 0 and S[i]["lb"] < 0
    assert np.isinf(rig["tmax"][case == 6]).all() and np.all(rig["tmax"][case == 8] == 0) and np.all(rig["tmax"][case == 7] == f32(HC.CAPPED_TMAX))
    # CHAIN_REV ties CHAIN's pairs at CHAIN's anchors in the opposite order: every dependency against the lane order
    for k in ("body", "other", "pa", "pb"):
        assert rig[k][r].tobytes() == rig[k][c][::-1].tobytes(), k
    assert rig["body"][r].tolist() == [3, 2, 1, 0]
    # the dataflow over ranks and degrees gives the sequential order's bits, whatever the schedule - and never stalls
    want = HC.solve(rig, H, 4, W[2], st, lens)
    for seed in (1, 2):
        got = HC.solve(rig, H, 4, W[2], st, lens, schedule=np.random.default_rng(seed))
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
    assert np.flatnonzero(want[3]).tolist() == planted and len(planted) == 2 and not want[2][planted].any() and np.all(np.isfinite(want[0]))
    assert np.all(want[2][:, 7] == 0)
    acc = want[2]
    live = np.array([i not in planted for i in range(n)])
    assert np.all(np.any(acc[live, 0:3] != 0, axis=1)) and np.all(acc[live, 3] != 0)
    assert np.all(acc[live & (case == 0), 5:7] == 0) and np.all(acc[live & (case == 1), 5] == 0) and np.all(acc[case == 8, 6] == 0)
    assert np.all(acc[live & (case == 2), 5] >= 0) and np.all(acc[live & (case == 3), 5] <= 0) and np.any(acc[live & (case == 2), 5] > 0) and np.any(acc[live & (case == 3), 5] < 0)
    mm = f32(HC.CAPPED_TMAX) * H
    assert np.all(np.abs(acc[live & (case == 7), 6]) <= mm) and np.mean(np.abs(acc[live & (case == 7), 6]) == mm) > 0.5   # the cap is reached
    assert np.all(acc[live & (case == 6), 6] != 0)
    # the rows of the table matter, and only to the motors
    other = HC.solve(rig, H, 4, W[0], st, lens)
    assert other[1].tobytes() != want[1].tobytes()
    # the host's plan is the ball joints': one template, both record types
    src = read("mgf_amd", "csrc", "host_batch_joint.inc")
    assert "template <class Rec>\nstatic void batch_joint_plan(BatchJointRig<Rec>& R, const Rec* recs, size_t n) {" in src
    assert "batch_joint_plan(b->hinges, j, n);" in read("mgf_amd", "csrc", RIG_FILE)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def _pair(seed):
    """an isolated pair of bodies of the synthetic state and a hinge between them in its rest pose (hinge_frames): theta = 0"""
    st = HC.synthetic_state([2], seed=seed)
    rig = HC.place(HC.hinge(0, 0, 1, beta=0.2), st, [2], seed)
    return st, rig


def test_the_float64_restatement_holds_a_limit_reaches_a_target_and_stops_at_a_cap():
    """Invariants of the definition, in float64, on an isolated pair with the hinge in its rest pose, beta = 0.2, 16 sweeps.  One hinge
    alone: the point row is the last of every sweep and leaves the relative angular velocity as the three rows ahead of it made it up to
    the share its arms carry, so the sweeps converge geometrically; what is asked is the side of the bound, the target and the cap."""
    d = np.float64
    for seed in (601, 602, 603):
        st, rig = _pair(seed)
        # a violated limit: theta = 0 lies below [0.2, 0.9] - the rate ends at or above lb > 0; above [-0.9, -0.2] - at or below lb < 0
        for lo, hi, side in ((0.2, 0.9, -1), (-0.9, -0.2, 1)):
            r = HC.set_limits(rig.copy(), lo, hi)
            r["flags"] = HC.LIMIT
            S = HC.setup(r, H, [0.0], st, [2], d)[0]
            assert S["side"] == side and not S["skip"] and np.sign(S["lb"]) == -side
            assert abs(abs(S["lb"]) - np.sin(0.2) * 0.2 * 60) < 1e-5                # err = sin of the violation (f32 words), s = beta / h
            v, om, acc, sk = HC.solve(r, H, 16, None, st, [2], ft=d)
            rate = HC.residuals(S, v, om)[3]
            print("limit", (lo, hi), "lb", float(S["lb"]), "rate", rate, "al", acc[0, 5])
            assert side * (rate - S["lb"]) <= 1e-9 * max(1.0, abs(S["lb"]))           # on the permitted side, to rounding
            assert side * acc[0, 5] <= 0
        # a motor whose cap is not reached: the rate ends at the target
        r = rig.copy()
        r["flags"], r["tmax"] = HC.MOTOR, np.inf
        S = HC.setup(r, H, [1.5], st, [2], d)[0]
        v, om, acc, sk = HC.solve(r, H, 16, f32([1.5]), st, [2], ft=d)
        rate = HC.residuals(S, v, om)[3]
        print("motor: target 1.5, rate", rate, "am", acc[0, 6])
        assert abs(rate - 1.5) <= RESIDUAL_BOUND and acc[0, 6] != 0
        # a capped motor stops at its cap, exactly
        r["tmax"] = 1.0e-3
        S = HC.setup(r, H, [1.5], st, [2], d)[0]
        v, om, acc, sk = HC.solve(r, H, 16, f32([1.5]), st, [2], ft=d)
        assert abs(acc[0, 6]) == S["mmax"] == d(f32(1.0e-3)) * d(H) and abs(HC.residuals(S, v, om)[3] - 1.5) > 0.1
        # the same in f32
        acc32 = HC.solve(r, H, 16, f32([1.5]), st, [2])[2]
        assert abs(acc32[0, 6]) == f32(1.0e-3) * H


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_hinge_frames_places_a_hinge_without_gap_tilt_or_angle():
    lens = list(HC.LENGTHS)
    st = HC.synthetic_state(lens)
    jr = HC.JC.main_rig(lens, (st["x"] + st["delta"]).astype(f32))[0]
    rig = np.zeros(len(jr), _capi.HINGE_DTYPE)
    for k in ("world", "body", "other"):
        rig[k] = jr[k]
    # the hinges whose ends lie within 3.2 of each other: an arm of 1.6 at most, rounded to f32 once - 6e-8 a component and end - where the
    # 1e-6 asked of the gap leaves no room for the arm of 5 and more that a pair from opposite corners of the lattice has
    x = (st["x"] + st["delta"]).astype(np.float64)
    off = HC.SC.offsets(lens)
    ga = off[rig["world"]] + rig["body"]
    gb = np.where(rig["other"] >= 0, off[rig["world"]] + rig["other"], ga)
    rig = rig[np.linalg.norm(x[ga] - x[gb], axis=1) < 3.2]
    assert len(rig) > 100 and set(rig["world"].tolist()) == {HC.ANCHOR, HC.CHAIN, HC.CHAIN_REV, HC.STAR, HC.RING, HC.FULL}
    rig["beta"] = H                          # s = beta / h = 1: g1 and g2 are the axis errors dot(B, T1) and dot(B, T2) themselves
    HC.set_limits(rig, 0.0, 0.0)
    HC.place(rig, st, lens, seed=77)
    assert np.any(rig["other"] < 0) and rig["pa"].dtype == f32
    S = HC.setup(rig, H, np.zeros(len(rig), f32), st, lens, np.float64)
    worst = [max(float(np.abs(x[k]).max()) for x in S) for k in ("C", "g1", "g2", "sphi")]
    print("hinge_frames, float64 setup of the f32 frames: largest |C|, |g1|, |g2|, |sphi|:", worst)
    assert max(worst) < 1e-6
    assert all(abs(x["c"] - 1) < 1e-6 and not x["skip"] for x in S)
    assert HC.gaps(rig, st, lens).max() < 1e-6 and HC.misalignment(rig, st, lens).max() < 1e-6 and np.abs(HC.thetas(rig, st, lens)).max() < 1e-6
    # unit and perpendicular: what mgf_batch_set_hinges asks of a record
    for a, u in (("ax", "ua"), ("bx", "ub")):
        A, U = rig[a].astype(np.float64), rig[u].astype(np.float64)
        assert np.abs(np.sum(A * A, axis=1) - 1).max() < 1e-6 and np.abs(np.sum(U * U, axis=1) - 1).max() < 1e-6 and np.abs(np.sum(A * U, axis=1)).max() < 1e-6
    # the far end the world: pb is the anchor, bx the axis, as given
    fr = mgf_amd.hinge_frames({"x": [[1, 2, 3]], "q": [[1, 0, 0, 0]]}, None, [[1, 2.5, 3]], [[0, 0, 2]])
    assert fr["pb"].tolist() == [[1, 2.5, 3]] and fr["bx"].tolist() == [[0, 0, 1]] and fr["pa"].tolist() == [[0, 0.5, 0]] and fr["ax"].tolist() == [[0, 0, 1]]
    assert fr["ua"].tobytes() == fr["ub"].tobytes() and set(fr) == {"pa", "pb", "ax", "ua", "bx", "ub"}


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_what_needs_no_device_is_refused_in_the_headers_order_with_the_rig_unchanged():
    lib = mgf_amd.load_library()
    INV = _capi.ERR_INVALID

    def err():
        return lib.mgf_last_error().decode()
    fake = C.c_void_p(16)   # a handle that is never dereferenced
    rig = np.zeros(4, _capi.HINGE_DTYPE)
    out = C.c_void_p(1 << 21)
    h = C.c_float(1.0 / 60.0)
    assert lib.mgf_batch_hinge_count(None) == -1
    assert lib.mgf_batch_set_hinges(None, rig.ctypes.data, 4) == INV and "NULL" in err()
    assert lib.mgf_batch_set_hinges(None, None, 0) == INV and "NULL" in err()
    assert lib.mgf_batch_set_hinges(fake, None, 4) == INV and "NULL" in err()
    assert lib.mgf_batch_set_hinges(fake, rig.ctypes.data, -1) == INV and "negative" in err()
    assert lib.mgf_batch_set_hinges(fake, rig.ctypes.data, 1 << 31) == INV and "too many" in err()
    for fn in (lib.mgf_batch_set_hinge_targets, lib.mgf_batch_set_hinge_targets_dev):
        assert fn(None, out, 1) == INV and "NULL" in err()
        assert fn(None, None, 0) == INV and "NULL" in err()                                   # the handle first
        for rows in (0, -1, (1 << 20) + 1):
            assert fn(fake, out, rows) == INV and "rows must be in [1, 2^20]" in err(), rows
    for fn in (lib.mgf_batch_solve_hinges, lib.mgf_batch_solve_hinges_dev):
        assert fn(None, h, 4, 0, out) == INV and "NULL" in err()
        assert fn(None, C.c_float(np.nan), -1, -1, None) == INV and "NULL" in err()           # the handle first
        for bad in (np.nan, np.inf, -np.inf):
            assert fn(fake, C.c_float(bad), -1, -1, out) == INV and "h is not finite" in err(), bad   # h ahead of iters
        assert fn(fake, h, -1, -1, out) == INV and "iters is negative" in err()               # iters ahead of row
    src = read("mgf_amd", "csrc", RIG_FILE)
    body = src[src.index('extern "C" mgf_status mgf_batch_set_hinges('):src.index('extern "C" int64_t mgf_batch_hinge_count(')]
    plan_call = "batch_joint_plan(b->hinges, j, n);"
    # (the two checks of `other`, with their two refusals, are the joint rigs' shared step; the plan step makes the table one row of zeros:
    # tests/test_world_batch_joint_family_host.py)
    marks = ["batch_rig_set_args(b, j, n_in)", 'batch_rig_ref_check(b, r.world, r.body, 0, "hinge")', "batch_joint_other_check<HingeKind>(b, r)",
             "r.flags & ~(uint32_t)(MGF_HINGE_LIMIT | MGF_HINGE_MOTOR)", "a word of a hinge is not finite (tmax may be +inf): the rig was not changed",
             "a hinge's beta is not in [0, 1]: the rig was not changed", "a hinge's tmax is negative: the rig was not changed", "is not of unit length: the rig was not changed",
             "is not perpendicular to its axis: the rig was not changed", "a hinge's sh is negative: the rig was not changed",
             "++per_world[(size_t)r.world] > MGF_BATCH_MAX_WORLD_HINGES", plan_call]
    order = [body.index(s) for s in marks]
    assert order == sorted(order), order
    assert body.count("the rig was not changed") == 10 - 2
    assert not re.search(r"b->hinges\.|\bR\.", body.replace(plan_call, ""))                  # the rig changes in the plan step alone
    assert not re.search(r"<<<|Async|hipMalloc|\.ensure\(|h2d\(", body)                      # no device work at all
    shared = read("mgf_amd", "csrc", "host_batch_joint.inc")
    assert "joint_unit(joint_dot(r.ax, r.ax))" in body and "static double joint_dot(const mgf_vec3& a, const mgf_vec3& b) { return (double)a.x * b.x" in shared   # in double on the host
    # what tests/test_world_batch_rigs_host.py asks of a rig file: the shared steps used, not copied
    assert src.count("batch_rig_set_args(b, ") == 1 and src.count("batch_rig_up(") == 0 and "batch_rig_up(b, R, T::word, 3)" in shared and 'word = "hinge";' in src
    for gone in ("BatchQueryPlan plan(", "batch_rig_upload(", "names a body its world does not hold", '"batch is NULL"', "std::stable_sort("):
        assert gone not in src, gone
    host = read("mgf_amd", "csrc", "host_batch.inc")
    stale = host[host.index("static void batch_rigs_stale("):host.index('extern "C" mgf_status mgf_batch_add_bodies(')]
    assert host.count("BatchJointRig<mgf_batch_hinge> hinges;") == 1 and "b->hinges.stale = true;" in stale
    assert '"hinges_skipped"' in host[host.index('extern "C" mgf_status mgf_batch_counter('):]
    # the target and the solve calls are one-line forwards to the joint rigs' shared steps, whose order - the refusals (the ball joints',
    # the row behind them), the context, (device form) the pointer looked up, and only then the copy or the first thing enqueued; no
    # wait in the device forms, one in the host form of the solve with the give-up reported behind it; one launch behind batch_push and
    # ready, of the named row, counted once - tests/test_world_batch_joint_family_host.py holds
    for line in ('extern "C" mgf_status mgf_batch_set_hinge_targets(mgf_batch* b, const float* w, int64_t rows) { return batch_joint_targets<HingeKind>(b, w, rows, hipMemcpyHostToDevice); }',
                 "  return batch_joint_targets<HingeKind>(b, w_dev, rows, hipMemcpyDeviceToDevice);\n}", "  return batch_joint_solve<HingeKind>(b, h, iters, row, impulse_out);\n}",
                 "  return batch_joint_solve_dev<HingeKind>(b, h, iters, row, impulse_out_dev);\n}"):
        assert src.count(line) == 1, line
    entries = src[src.index('extern "C" int64_t mgf_batch_hinge_count('):]
    assert entries.count('extern "C"') == 5 and entries.count(";") == 5 and entries.count("return ") == 5      # nothing but the forwards
    kind = src[src.index("struct HingeKind {"):src.index('extern "C" mgf_status mgf_batch_set_hinges(')]
    assert "launches = MGF_BATCH_HINGE_LAUNCHES," in kind and "launch = k_batch_hinge_solve<GATED>;" in kind and "table = true;" in kind and "using Rows = HingeRows;" in kind
    assert "static constexpr uint32_t kWords = 7, kFloats = 8;" in read("mgf_amd", "csrc", "k_batch_hinge.h")   # 32 bytes a hinge of impulse
    assert "batch_single_parts(" not in src                                                   # hinges read no shapes


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_launch_sits_behind_the_ball_joints_and_ahead_of_the_tick_and_is_counted_once():
    host = read("mgf_amd", "csrc", "host_batch.inc")
    roll = read("mgf_amd", "csrc", "host_batch_rollout.inc")
    core = roll[roll.index("static mgf_status batch_rollout_run("):roll.index('extern "C" mgf_status mgf_batch_rollout_dev(')]
    assert "!b->hinges.recs.empty()" in core and "!joints && !hinges &&" in core              # the early return to the plain step sees the hinge rig
    assert (core.index("batch_push(") < core.index("batch_joint_hook<JointKind>(") < core.index("batch_joint_hook<HingeKind>(b, dt, iters, &H.hinges)")
            < core.index("batch_step_run(b, dt, iters, n_ticks, stats, &H)"))
    train = host[host.index("static mgf_status batch_step_run("):host.index('extern "C" mgf_status mgf_batch_step(')]
    shared = read("mgf_amd", "csrc", "host_batch_joint.inc")   # (a kind's part of the train: tests/test_world_batch_joint_family_host.py holds its steps)
    tick = "batch_joint_tick<HingeKind>(b, hook->hinges, t, &hook->launches)"
    assert train.index("k_batch_rollout_act<") < train.index("batch_joint_tick<JointKind>(") < train.index(tick) < train.index("batch_collide(")
    assert train.count("batch_joint_tick<HingeKind>") == 1 and "per_tick = MGF_BATCH_ROLLOUT_HINGE_LAUNCHES_PER_TICK;" in read("mgf_amd", "csrc", RIG_FILE)
    assert "if (T::table) H.A.w = R.w.p + (size_t)std::min<int64_t>((int64_t)t, R.rows - 1) * R.recs.size();" in shared    # tick t reads row min(t, rows - 1)
    # what the kernel reads of the handle is looked up again for every pass: inside the loop over the passes, ahead of the loop over the ticks
    assert train.index("for (uint32_t first = 0, pass = 0;") < train.index("batch_joint_pass<HingeKind>(b, hook->hinges);") < train.index("for (uint32_t t = first; t < NT; ++t)")
    assert "H.A.done = b->d_done.p; H.A.act = b->d_act.p;" in shared
    assert "d2h(ctx, err, b->d_err.p, 2)" in train                                              # the read-back is as it was: both solvers' give-up word
    step = host[host.index('extern "C" mgf_status mgf_batch_step('):host.index('extern "C" mgf_status mgf_batch_read_constraints(')]
    assert "batch_step_run(b, dt, iters, n_ticks, stats, nullptr)" in step and "hinge" not in step   # mgf_batch_step applies no hinge


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_kernel_has_the_joint_solvers_loop_shape_a_bounded_spin_and_no_float_atomic():
    k = read("mgf_amd", "csrc", "k_batch_hinge.h")
    entry = k[k.index("void k_batch_hinge_solve("):]
    assert entry[:entry.index("\n}\n")] == "void k_batch_hinge_solve(BatchJointArgs A) {\n  batch_joint_loop<HingeRows, GATED>(A);"
    # the kernel is one call of the joint solvers' skeleton: the loop shape is asserted of the skeleton, the rows of HingeRows::sweep,
    # which the loop calls once a turn between its one unpack and its one re-pack of the velocities
    loop_file = read("mgf_amd", "csrc", "k_batch_joint_loop.h")
    body = loop_file[loop_file.index("void batch_joint_loop("):]
    body = body[:body.index("\n}\n")]
    sweep = k[k.index("void sweep(V3& va, V3& oa, V3& vb, V3& ob, bool has_b) {"):k.index("void store(float* p) const {")]
    gate = "if (GATED && !(A.done[k] == A.tick && A.act[k] == A.tick)) return;"
    assert gate in body and body.index(gate) < body.index("__syncthreads()")                 # the workgroup's early return ahead of the first barrier
    assert body.count("__syncthreads()") == 2 and re.findall(r"atomic\w*\(", body.replace("__hip_atomic_load(", "").replace("__hip_atomic_store(", "")) == ["atomicAdd("]
    assert "atomicAdd(A.skipped, 1ull)" in body                                               # an integer count: no float atomic
    loop = body[body.index("while (open)"):body.index("if (s_fail != 0u) return;")]
    assert loop.count("__ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP") == 2 and loop.count("__ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP") == 2   # both counters released once
    assert loop.index("if (!__any(ready)) __builtin_amdgcn_s_sleep(1);") < loop.index("if (ready) {") < loop.index("s_dyn[2 * sa] = ") < loop.index("__ATOMIC_RELEASE")
    rows = [sweep.index("// hinge row: " + w) for w in ("the motor", "the limit", "the two angular rows", "the point")]
    assert rows == sorted(rows) and loop.count("s_dyn[2 * sa] = ") == 1 and loop.count("= s_dyn[2 * sa]") == 1   # four rows in one turn, the velocities in registers between them
    assert loop.index("= s_dyn[2 * sa]") < loop.index("R.sweep(va, oa, vb, ob, has_b);") < loop.index("s_dyn[2 * sa] = ") and "s_dyn" not in sweep and "P.sweep(va, oa, vb, ob, has_b);" in sweep
    assert "++spins > kBatchSpinLimit" in loop and "A.err[1] = 1u;" in loop and "A.err[0]" not in k
    assert "GATED" not in loop and "A.done" not in loop and "break" not in loop and "continue" not in loop and "return" not in loop
    back = body[body.index("if (s_fail != 0u) return;"):]
    assert "srec[4 * (size_t)body] = s_dyn[2 * s];" in back and "srec[4 * (size_t)body + 1] = s_dyn[2 * s + 1];" in back and "+ 2]" not in back   # words 0 and 1 alone
    assert len(re.findall(r"__global__ __launch_bounds__\(kBatchBlock\)", k)) == len(re.findall(r"__global__", k)) == 1
    assert not re.search(r"A\.act\[[^\]]+\] =[^=]", k) and not re.search(r"A\.done\[[^\]]+\] =[^=]", k)
    assert "atan" not in k and "sinf" not in k and "cosf" not in k                            # no arctangent, no sine: + - * / and comparisons


# ---- 9 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_new_kernel_uses_no_scratch_and_spills_nothing():
    if not os.path.exists(os.path.join(ROOT, "mgf_amd", "libmgf_hip.so")) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    rows = kernel_resources("k_batch_hinge")
    assert set(rows) == {"k_batch_hinge_solve<false>", "k_batch_hinge_solve<true>"}, sorted(rows)
    design = re.sub(r"\s+", " ", read("DESIGN.md"))
    for name, v in sorted(rows.items()):
        print(name, ": vgpr, sgpr, scratch, static lds, sgpr spills, vgpr spills =", v)
        assert v[2] == "0" and v[4] == "0" and v[5] == "0", (name, v)    # no scratch, no spills
        assert int(v[3]) <= 16, (name, v)                                 # static LDS: the give-up flag alone
        assert "`%s` %s / %s / %s / 0 / 0" % (name, v[0], v[1], v[3]) in design, (name, v)
    old = kernel_resources("k_batch_joint")                              # the ball joints' kernel: 80 / 60 until the three solvers became one skeleton
    assert old == {"k_batch_joint_solve<false>": ("78", "51", "0", "16", "0", "0"), "k_batch_joint_solve<true>": ("78", "51", "0", "16", "0", "0")}, old


# ---- 10 -----------------------------------------------------------------------------------------------------------------------------------
def test_the_binding_marshals_a_rig_and_turns_a_wrong_tensor_down_before_it_calls_c():
    import torch

    class Handle(mgf_amd.WorldBatch):   # no context, no C handle: a call that got as far as C would fail differently
        def __init__(self):
            self._h, self.n_worlds = None, 2

        def hinge_count(self):
            return 4

    b, n = Handle(), 4
    for t in (torch.zeros((n, 8), dtype=torch.float64), torch.zeros((8, n), dtype=torch.float32).t(), torch.zeros((n - 1, 8), dtype=torch.float32),
              torch.zeros((n, 3), dtype=torch.float32)):
        with pytest.raises(ValueError) as e:
            b.solve_hinges_dev(0.01, 4, impulses_dev=t)
        assert "on cpu" not in str(e.value), str(e.value)
    with pytest.raises(ValueError, match="on cpu"):
        b.solve_hinges_dev(0.01, 4, impulses_dev=torch.zeros((n, 8), dtype=torch.float32))
    with pytest.raises(ValueError, match="on cpu"):
        b.set_hinge_targets_dev(torch.zeros((3, n), dtype=torch.float32))
    with pytest.raises(ValueError):
        b.set_hinge_targets_dev(torch.zeros((3, n + 1), dtype=torch.float32))
    with pytest.raises(ValueError):
        b.set_hinge_targets(np.zeros((3, n + 1), np.float32))
    with pytest.raises(mgf_amd.MgfError):                               # and a call whose arguments are all in order does reach C
        b.solve_hinges_dev(0.01, 4, row=1, impulses_dev=1 << 21)
    with pytest.raises(mgf_amd.MgfError):
        b.solve_hinges(0.01, 4, impulses=True)
    with pytest.raises(mgf_amd.MgfError):
        b.set_hinge_targets(np.zeros(n, np.float32))                    # one row
    with pytest.raises(mgf_amd.MgfError):
        b.set_hinges([0, 1, 1], [0, 1, 2], other=[1, -1, 0], ax=(0, 0, 1), ua=(1, 0, 0), bx=(0, 0, 1), ub=(1, 0, 0), beta=0.2, lo=-0.5, hi=0.7, limit=True)
    with pytest.raises(ValueError):
        b.set_hinges([0, 1, 1], [0, 1])                                 # neither one nor n
    # lo and hi become four words in float64, rounded once; the flags are the keywords'
    seen = {}

    class Lib:
        def mgf_batch_set_hinges(self, h, p, n):
            seen["rig"] = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (n * 112,)).view(_capi.HINGE_DTYPE).copy()
            return 0
    real = _capi.load_library
    _capi.load_library = lambda: Lib()
    try:
        b.set_hinges([0, 1], [0, 1], other=[1, -1], ax=(0, 0, 1), ua=(1, 0, 0), bx=(0, 0, 1), ub=(1, 0, 0), beta=0.2, lo=[-0.5, 0.1], hi=0.7, tmax=[np.inf, 2.0],
                     limit=[True, False], motor=[False, True])
    finally:
        _capi.load_library = real
    rig = seen["rig"]
    assert rig["flags"].tolist() == [1, 2] and rig["other"].tolist() == [1, -1] and np.isinf(rig["tmax"][0]) and rig["tmax"][1] == 2
    want = HC.set_limits(np.zeros(2, _capi.HINGE_DTYPE), [-0.5, 0.1], [0.7, 0.7])
    for k in ("cm", "sm", "ch", "sh"):
        assert rig[k].tobytes() == want[k].tobytes(), k
    assert rig["cm"][0] == f32(np.cos(0.1)) and rig["sh"][0] == f32(np.sin(0.6))
