"""The sliders of a batch (mgf_batch_set_sliders, mgf_batch_slider_count, mgf_batch_set_slider_targets, mgf_batch_set_slider_targets_dev,
mgf_batch_solve_sliders, mgf_batch_solve_sliders_dev) without a GPU: the header, the library, the binding and the documents carry the
calls, the record of 112 bytes and the constants; the numpy restatement (tests/batch_slider_cases.py) holds against itself in float64,
row by row; the plan's dataflow gives the sequential order's bits whatever the schedule; the float64 restatement holds a violated
limit, reaches a motor's target, stops at a motor's cap and holds a lock; slider_frames places a slider without gap, tilt or travel;
what needs no device is refused, in the header's order, with the rig unchanged; the launch sits behind the hinges' and ahead of the
tick; and the kernel has k_batch_hinge_solve's loop shape, no scratch and no spills."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mgf_amd
from mgf_amd import _capi
from tests import batch_slider_cases as LC
from tests.util import ROOT, kernel_resources, read

f32 = np.float32
CALLS = ("mgf_batch_set_sliders", "mgf_batch_slider_count", "mgf_batch_set_slider_targets", "mgf_batch_set_slider_targets_dev", "mgf_batch_solve_sliders",
         "mgf_batch_solve_sliders_dev")
RIG_FILE = "host_batch_slider.inc"
H = f32(1.0 / 60.0)
NAMES = ["world", "body", "other", "flags", "pa", "beta", "pb", "fmax", "ax", "lo", "ua", "hi", "bx", "pad0", "ub", "pad1"]


def _seeded(beta=0.2):
    lens = list(LC.LENGTHS)
    st = LC.synthetic_state(lens)
    rig, planted, W = LC.main_rig(lens, st, beta=beta)
    return lens, st, rig, planted, W


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
def test_header_library_binding_and_documents_carry_the_calls_the_record_and_the_constants():
    h = read("include", "mgf_hip.h")
    flat_h = re.sub(r"\s+", " ", h)
    for sig in ("MGF_API mgf_status mgf_batch_set_sliders(mgf_batch* b, const mgf_batch_slider* j, int64_t n);",
                "MGF_API int64_t mgf_batch_slider_count(const mgf_batch* b);",
                "MGF_API mgf_status mgf_batch_set_slider_targets(mgf_batch* b, const float* w, int64_t rows);",
                "MGF_API mgf_status mgf_batch_set_slider_targets_dev(mgf_batch* b, const float* w_dev, int64_t rows);",
                "MGF_API mgf_status mgf_batch_solve_sliders(mgf_batch* b, float h, int32_t iters, int64_t row, float* impulse_out);",
                "MGF_API mgf_status mgf_batch_solve_sliders_dev(mgf_batch* b, float h, int32_t iters, int64_t row, float* impulse_out_dev);"):
        assert sig in flat_h, sig
    assert h.index("MGF_API mgf_status mgf_batch_solve_hinges_dev(") < h.index("/* ---- slider joints between bodies") < h.index("/* name in {")
    consts = (("MGF_SLIDER_LIMIT", _capi.SLIDER_LIMIT, 1), ("MGF_SLIDER_MOTOR", _capi.SLIDER_MOTOR, 2), ("MGF_SLIDER_LOCK", _capi.SLIDER_LOCK, 4),
              ("MGF_BATCH_SLIDER_LAUNCHES", _capi.BATCH_SLIDER_LAUNCHES, 1), ("MGF_BATCH_ROLLOUT_SLIDER_LAUNCHES_PER_TICK", _capi.BATCH_ROLLOUT_SLIDER_LAUNCHES_PER_TICK, 1),
              ("MGF_BATCH_MAX_WORLD_SLIDERS", _capi.BATCH_MAX_WORLD_SLIDERS, 256))
    flat = re.sub(r"\s+", " ", read("INTEGRATION.md"))
    for name, value, want in consts:
        m = re.search(r"#define %s\s+(\d+)" % name, h)
        assert m and int(m.group(1)) == value == want, name
        assert re.search(r"pub const %s: (i64|u32) = %d;" % (name, want), flat), name
        assert getattr(mgf_amd, name[4:]) is getattr(_capi, name[4:]), name
    section = h[h.index("/* ---- slider joints between bodies"):h.index("MGF_API mgf_status mgf_batch_solve_sliders_dev(")]
    section = re.sub(r"\n \* ?(?! )", " ", section)                          # (a sentence may run over the end of a line of the comment)
    for word in ("A = rotate(q_a, ax);  T1 = rotate(q_a, ua);  T2 = cross(A, T1)", "other == -1: B = bx;  U1 = ub",
                 "U2 = cross(B, U1);  ca = ra + C;  d = dot(C, A);  ims = im_a + im_b",
                 "sA = cross(ca, A);  sB = cross(rb, A);  Km = (ims + dot(sA, I_a * sA)) + dot(sB, I_b * sB)",
                 "pA1 = cross(ca, T1);  pB1 = cross(rb, T1);  g1 = dot(C, T1) * s", "k11 = (ims + dot(pA1, I_a * pA1)) + dot(pB1, I_b * pB1)",
                 "k12 = dot(pA1, I_a * pA2) + dot(pB1, I_b * pB2);  k21 = dot(pA2, I_a * pA1) + dot(pB2, I_b * pB1)",
                 "d2 = k11 * k22 - k12 * k21;  m11 = k22 / d2;  m12 = -k12 / d2;  m21 = -k21 / d2;  m22 = k11 / d2",
                 "e = ((cross(A, B) + cross(T1, U1)) + cross(T2, U2)) * 0.5;  gw = e * s;  Kw = I_a + I_b (word by word);  Kwinv = invert(Kw)",
                 "LOCK:                side = 2,  lb = (lo - d) * s", "LIMIT and d < lo:    side = -1, lb = (lo - d) * s", "LIMIT and d > hi:    side = +1, lb = -((d - hi) * s)",
                 "MOTOR:  mmax = fmax * h", "rate(n, a, b) = (dot(v_b - v_a, n) + dot(omega_b, b)) - dot(omega_a, a)",
                 "v_a = v_a - n * (lam * im_a);  omega_a = omega_a - I_a * (a * lam)", "v_b = v_b + n * (lam * im_b);  omega_b = omega_b + I_b * (b * lam)",
                 "lam = (w - rate(A, sA, sB)) / Km;  t = am + lam;  if (t < -mmax) t = -mmax;  if (t > mmax) t = mmax;  lam = t - am;  am = t",
                 "lam = (lb - rate(A, sA, sB)) / Km;  t = al + lam;  side == -1: if (t < 0) t = 0;  side == +1: if (t > 0) t = 0;  lam = t - al;  al = t",
                 "L = -(Kwinv * ((omega_b - omega_a) + gw));  omega_a = omega_a - I_a * L;  omega_b = omega_b + I_b * L;  aw = aw + L",
                 "r1 = rate(T1, pA1, pB1) + g1;  r2 = rate(T2, pA2, pB2) + g2;  l1 = -(m11 * r1 + m12 * r2);  l2 = -(m21 * r1 + m22 * r2)",
                 "n = T1 * l1 + T2 * l2;  v_a = v_a - n * im_a;  omega_a = omega_a - I_a * (pA1 * l1 + pA2 * l2)",
                 "(p1, p2, al, am, aw.x, aw.y, aw.z, 0)", "sliders_skipped", "still takes its place in the order",
                 "untouched to the bit", "no warm start", "several components", "drive_launches", "rollout_launches", "the rig was not changed",
                 "nothing enqueued", "mgf_batch_add_bodies", "no float atomic", "min(t, rows - 1)", "one row of zeros", "is a brake", "ONCE",
                 "mgf_batch_step itself stays World::step, launch for launch", "OUT OF SCOPE", "slider encoders", "servo", "warm starting",
                 "interleaved", "lone mgf_world", "inside mgf_batch_step", "mgf_batch_gather_state", "LOCK excludes the other two flags"):
        assert word in section, word
    assert '"sliders_skipped"' in h[h.index("/* name in {"):]
    # the record: 112 bytes, the same fields at the same offsets in the ctypes struct and the numpy dtype
    assert C.sizeof(_capi.BatchSlider) == 112 == _capi.SLIDER_DTYPE.itemsize
    assert [f[0] for f in _capi.BatchSlider._fields_] == list(_capi.SLIDER_DTYPE.names) == NAMES
    want_off = [0, 4, 8, 12] + [16 * w + o for w in range(1, 7) for o in (0, 12)]
    assert [_capi.SLIDER_DTYPE.fields[k][1] for k in NAMES] == want_off == [getattr(_capi.BatchSlider, k).offset for k in NAMES]
    assert re.search(r"typedef struct mgf_batch_slider \{\s*int32_t world, body, other; uint32_t flags;[^\n]*\n\s*mgf_vec3 pa; float beta;[^\n]*\n\s*mgf_vec3 pb; float fmax;[^\n]*\n"
                     r"\s*mgf_vec3 ax; float lo;[^\n]*\n\s*mgf_vec3 ua; float hi;[^\n]*\n\s*mgf_vec3 bx; float pad0;[^\n]*\n\s*mgf_vec3 ub; float pad1;[^\n]*\n\} mgf_batch_slider;", h)
    lib = mgf_amd.load_library()
    vp, i64, i32, fl = C.c_void_p, C.c_int64, C.c_int32, C.c_float
    want = {"mgf_batch_set_sliders": (i32, [vp, vp, i64]), "mgf_batch_slider_count": (i64, [vp]), "mgf_batch_set_slider_targets": (i32, [vp, vp, i64]),
            "mgf_batch_set_slider_targets_dev": (i32, [vp, vp, i64]), "mgf_batch_solve_sliders": (i32, [vp, fl, i32, i64, vp]),
            "mgf_batch_solve_sliders_dev": (i32, [vp, fl, i32, i64, vp])}
    for name in CALLS:
        assert name in _capi.SYMBOLS, name
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == want[name], name
    for method in ("set_sliders", "slider_count", "set_slider_targets", "set_slider_targets_dev", "solve_sliders", "solve_sliders_dev"):
        assert callable(getattr(mgf_amd.WorldBatch, method)), method
    assert mgf_amd.SLIDER_DTYPE is _capi.SLIDER_DTYPE and mgf_amd.slider_frames is _capi.slider_frames and mgf_amd.BatchSlider is _capi.BatchSlider
    for sig in ("pub fn mgf_batch_set_sliders(b: *mut mgf_batch, j: *const mgf_batch_slider, n: i64) -> mgf_status;",
                "pub fn mgf_batch_slider_count(b: *const mgf_batch) -> i64;",
                "pub fn mgf_batch_set_slider_targets(b: *mut mgf_batch, w: *const f32, rows: i64) -> mgf_status;",
                "pub fn mgf_batch_set_slider_targets_dev(b: *mut mgf_batch, w_dev: *const f32, rows: i64) -> mgf_status;",
                "pub fn mgf_batch_solve_sliders(b: *mut mgf_batch, h: f32, iters: i32, row: i64, impulse_out: *mut f32) -> mgf_status;",
                "pub fn mgf_batch_solve_sliders_dev(b: *mut mgf_batch, h: f32, iters: i32, row: i64, impulse_out_dev: *mut f32) -> mgf_status;",
                "pub struct mgf_batch_slider { pub world: i32, pub body: i32, pub other: i32, pub flags: u32, pub pa: mgf_vec3, pub beta: f32, pub pb: mgf_vec3, pub fmax: f32, "
                "pub ax: mgf_vec3, pub lo: f32, pub ua: mgf_vec3, pub hi: f32, pub bx: mgf_vec3, pub pad0: f32, pub ub: mgf_vec3, pub pad1: f32 }",
                "pub fn set_sliders(", "pub fn slider_count(", "pub fn set_slider_targets(", "pub unsafe fn set_slider_targets_dev(", "pub fn solve_sliders(",
                "pub unsafe fn solve_sliders_dev("):
        assert sig in flat, sig
    kernels = read("mgf_amd", "csrc", "kernels.h")
    assert kernels.index('#include "k_batch_hinge.h"') < kernels.index('#include "k_batch_slider.h"') < kernels.index('#include "k_batch_joint_read.h"')
    assert "k_batch_slider_solve<GATED> (k_batch_slider.h)" in kernels
    hip = read("mgf_amd", "csrc", "mgf_hip.hip")
    assert hip.index('#include "host_batch_hinge.inc"') < hip.index('#include "%s"' % RIG_FILE) < hip.index('#include "host_batch_joint_read.inc"')
    design = read("DESIGN.md")
    assert design.index("### Hinge encoders") < design.index("### Sliders between bodies") < design.index("### Rollout touch traces")
    sub = design[design.index("### Sliders between bodies"):design.index("### Rollout touch traces")]
    for word in ("k_batch_slider_solve", "done[k] == t && act[k] == t", "Definition", "One launch", "In a rollout", "Checks", "Compiler output", "Tests", "Out of scope",
                 "batch_slider_bench.py", "MGF_BATCH_SLIDER_LAUNCHES", "MGF_BATCH_ROLLOUT_SLIDER_LAUNCHES_PER_TICK", "MGF_BATCH_MAX_WORLD_SLIDERS", "__any", "kBatchSpinLimit",
                 "bench.py", "Measured", "Not measured", "min(t, rows - 1)", "encoders"):
        assert word in sub, word
    readme = read("README.md")
    assert "set_sliders" in readme and "solve_sliders_dev" in readme and "set_slider_targets" in readme and "slider_frames" in readme
    assert os.path.exists(os.path.join(ROOT, "tools", "batch_slider_bench.py"))
    for text in (h, design):   # the hinge sections that listed prismatic and fixed joints as out of scope point here
        assert "since: Sliders between bodies" in text
    assert "prismatic and fixed joints" in h and "prismatic and fixed joints" in design


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
WORST_RESIDUAL = 4.13e-4   # measured: see the test below
RESIDUAL_BOUND = 8 * WORST_RESIDUAL


def test_the_definition_holds_against_itself_in_float64_row_by_row():
    """Every slider of the seeded rig (tests/batch_slider_cases.py: main_rig on synthetic_state, h = 1/60, beta = 0.2 and beta = 0, row 0
    of the target table) solved ALONE for one sweep in f32 and in float64: the four residuals of the slider's rows -
    |(omega_b - omega_a) + gw|, |rate(T1) + g1|, |rate(T2) + g2| and the axis rate rate(A) - are evaluated in float64 with the float64
    run's own setup words, once under the f32 run's velocities and once under the float64 run's, and may differ by no more than a bound.
    The reference is the float64 restatement, never the library.
    Measured here on the CPU over the 2 x 275 sliders that are not skipped: the largest difference of any row is 4.13e-4, in an off-axis
    row of a slider of the 256-slider world whose ends lie far apart - an arm |pA1| of 3.8 beside inverse inertias of up to 20, so k11
    and k22 are of the order of 300 and the 2 x 2 solve loses what a ball joint's point row loses at a bias of 167 - WORST_RESIDUAL.
    The bound allows 8 x that, 3.3e-3, for other seeds' rounding - RESIDUAL_BOUND."""
    worst, where = 0.0, None
    for beta in (0.2, 0.0):
        lens, st, rig, planted, W = _seeded(beta)
        S64 = LC.setup(rig, H, W[0], st, lens, np.float64)
        for i in range(len(rig)):
            one, w = rig[i:i + 1], W[0, i:i + 1]
            v, om, acc, sk = LC.solve(one, H, 1, w, st, lens)
            v64, om64, acc64, sk64 = LC.solve(one, H, 1, w, st, lens, ft=np.float64)
            assert sk.tolist() == [i in planted], i
            if sk[0]:
                assert not acc.any() and v.tobytes() == st["v"].tobytes() and om.tobytes() == st["omega"].tobytes()
                continue
            assert not sk64[0]
            r32, r64 = LC.residuals(S64[i], v, om), LC.residuals(S64[i], v64, om64)
            for row, (a, b) in enumerate(zip(r32, r64)):
                if abs(a - b) > worst:
                    worst, where = abs(a - b), (i, beta, row)
                assert abs(a - b) <= RESIDUAL_BOUND, (i, beta, row, a, b)
    print("worst difference of a row's residual, f32 against f64:", worst, "at (slider, beta, row)", where, "; bound", RESIDUAL_BOUND)
    assert worst >= WORST_RESIDUAL / 8     # (the named constant is the measured figure, not a loose guess)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_seeded_rig_holds_every_case_and_its_dataflow_gives_the_sequential_orders_bits():
    lens, st, rig, planted, W = _seeded()
    n = len(rig)
    assert n == 1 + 4 + 4 + 6 + 2 + 4 + LC.MAX and np.any(np.diff(rig["world"]) < 0)        # interleaved in the caller's array
    items, joints, slots = LC.plan(rig)
    assert [it[0] for it in items] == [LC.ANCHOR, LC.CHAIN, LC.CHAIN_REV, LC.STAR, LC.PAIR, LC.RING, LC.FULL]     # no item for BARE and EMPTY
    assert [it[2] for it in items] == [1, 4, 4, 6, 2, 4, LC.MAX]
    full = items[-1]
    assert full[3] <= LC.BIG and max(s[1] for s in slots[full[4]:full[4] + full[3]]) > 1                         # degrees above one
    live = np.array([i not in planted for i in range(n)])
    # the frames are off, within what the issue of this rig states
    d, off_axis, e = LC.travel(rig, st, lens)
    assert 0.02 < off_axis[live].max() <= LC.SHIFT and 0.05 < e[live].max() <= LC.TILT and np.abs(d[live]).max() <= LC.SHIFT
    # every flag case, in the state the rig was dealt for
    S = LC.setup(rig, H, W[0], st, lens)
    case = np.arange(n) % 10
    for name, flags, side in (("none", 0, 0), ("limit_inside", 1, 0), ("limit_below", 1, -1), ("limit_above", 1, 1), ("limit_point", 1, -1),
                              ("motor_free", 2, 0), ("motor_capped", 2, 0), ("motor_zero", 2, 0), ("both", 3, 1), ("lock", 4, 2)):
        at = np.flatnonzero((case == LC.CASES.index(name)) & live)
        assert len(at) >= 20 and all(rig["flags"][i] == flags and S[i]["side"] == side for i in at), name
    point = np.flatnonzero(case == LC.CASES.index("limit_point"))
    assert np.all(rig["lo"][point] == rig["hi"][point])
    assert np.isinf(rig["fmax"][case == 5]).all() and np.all(rig["fmax"][case == 7] == 0) and np.all(rig["fmax"][case == 6] == f32(LC.CAPPED_FMAX))
    c, r = np.flatnonzero(rig["world"] == LC.CHAIN), np.flatnonzero(rig["world"] == LC.CHAIN_REV)
    for k in ("body", "other"):   # CHAIN_REV ties CHAIN's pairs in the opposite order: every dependency against the lane order
        assert rig[k][r].tobytes() == rig[k][c][::-1].tobytes(), k
    assert rig["body"][r].tolist() == [3, 2, 1, 0]
    # the dataflow over ranks and degrees gives the sequential order's bits, whatever the schedule - and never stalls
    want = LC.solve(rig, H, 4, W[2], st, lens)
    for seed in (1, 2):
        got = LC.solve(rig, H, 4, W[2], st, lens, schedule=np.random.default_rng(seed))
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
    assert np.flatnonzero(want[3]).tolist() == planted and len(planted) == 2 and not want[2][planted].any() and np.all(np.isfinite(want[0]))
    assert rig["pb"][planted[0]][0] == f32(3.0e38) or rig["pb"][planted[1]][0] == f32(3.0e38)                    # the arm of 3e38
    assert np.all(want[2][:, 7] == 0)
    acc = want[2]
    assert np.all(np.any(acc[live, 4:7] != 0, axis=1)) and np.all(acc[live, 0] != 0) and np.all(acc[live, 1] != 0)
    assert np.all(acc[live & (case == 0), 2:4] == 0) and np.all(acc[live & (case == 1), 2] == 0) and np.all(acc[case == 7, 3] == 0)
    assert np.all(acc[live & (case == 2), 2] >= 0) and np.all(acc[live & (case == 3), 2] <= 0) and np.any(acc[live & (case == 2), 2] > 0) and np.any(acc[live & (case == 3), 2] < 0)
    assert np.any(acc[live & (case == 9), 2] > 0) and np.any(acc[live & (case == 9), 2] < 0)                     # a lock pulls both ways
    mm = f32(LC.CAPPED_FMAX) * H
    assert np.all(np.abs(acc[live & (case == 6), 3]) <= mm) and np.mean(np.abs(acc[live & (case == 6), 3]) == mm) > 0.5   # the cap is reached
    assert np.all(acc[live & (case == 5), 3] != 0)
    # the rows of the table matter, and only to the motors
    other = LC.solve(rig, H, 4, W[0], st, lens)
    assert other[1].tobytes() != want[1].tobytes()
    # the host's plan is the ball joints': one template, every record type
    src = read("mgf_amd", "csrc", "host_batch_joint.inc")
    assert "template <class Rec>\nstatic void batch_joint_plan(BatchJointRig<Rec>& R, const Rec* recs, size_t n) {" in src
    assert "batch_joint_plan(b->sliders, j, n);" in read("mgf_amd", "csrc", RIG_FILE)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def _pair(seed):
    """an isolated pair of bodies of the synthetic state and a slider between them in its rest pose (slider_frames): d = 0"""
    st = LC.synthetic_state([2], seed=seed)
    rig = LC.place(LC.slider(0, 0, 1, beta=0.2), st, [2], seed)
    return st, rig


def test_the_float64_restatement_holds_a_limit_reaches_a_target_stops_at_a_cap_and_holds_a_lock():
    """Invariants of the definition, in float64, on an isolated pair with the slider in its rest pose, beta = 0.2, 32 sweeps.  One slider
    alone: the rows of a sweep disturb each other only through the arms, so the sweeps converge geometrically; what is asked is the side
    of the bound, the target, the cap and the lock."""
    d = np.float64
    for seed in (801, 802, 803):
        st, rig = _pair(seed)
        # a violated limit: d = 0 lies below [0.2, 0.9] - the rate ends at or above lb > 0; above [-0.9, -0.2] - at or below lb < 0
        for lo, hi, side in ((0.2, 0.9, -1), (-0.9, -0.2, 1)):
            r = rig.copy()
            r["lo"], r["hi"], r["flags"] = lo, hi, LC.LIMIT
            S = LC.setup(r, H, [0.0], st, [2], d)[0]
            assert S["side"] == side and not S["skip"] and np.sign(S["lb"]) == -side
            assert abs(abs(S["lb"]) - 0.2 * 0.2 * 60) < 1e-4                         # the violation is 0.2, s = beta / h
            v, om, acc, sk = LC.solve(r, H, 32, None, st, [2], ft=d)
            rate = LC.residuals(S, v, om)[3]
            print("limit", (lo, hi), "lb", float(S["lb"]), "rate", rate, "al", acc[0, 2])
            assert side * (rate - S["lb"]) <= RESIDUAL_BOUND                         # on the permitted side, to the residual bound
            assert side * acc[0, 2] <= 0
        # a motor whose cap is not reached: the rate ends at the target
        r = rig.copy()
        r["flags"], r["fmax"] = LC.MOTOR, np.inf
        S = LC.setup(r, H, [1.5], st, [2], d)[0]
        v, om, acc, sk = LC.solve(r, H, 32, f32([1.5]), st, [2], ft=d)
        rate = LC.residuals(S, v, om)[3]
        print("motor: target 1.5, rate", rate, "am", acc[0, 3])
        assert abs(rate - 1.5) <= RESIDUAL_BOUND and acc[0, 3] != 0
        # a capped motor stops at its cap, exactly
        r["fmax"] = 1.0e-3
        S = LC.setup(r, H, [1.5], st, [2], d)[0]
        v, om, acc, sk = LC.solve(r, H, 32, f32([1.5]), st, [2], ft=d)
        assert abs(acc[0, 3]) == S["mmax"] == d(f32(1.0e-3)) * d(H) and abs(LC.residuals(S, v, om)[3] - 1.5) > 0.1
        acc32 = LC.solve(r, H, 32, f32([1.5]), st, [2])[2]                           # the same in f32
        assert abs(acc32[0, 3]) == f32(1.0e-3) * H
        # a lock: the axis row is bilateral and leaves rate == lb, from either side
        for lo in (0.1, -0.1):
            r = rig.copy()
            r["lo"], r["hi"], r["flags"] = lo, lo, LC.LOCK
            S = LC.setup(r, H, [0.0], st, [2], d)[0]
            assert S["side"] == 2 and abs(S["lb"] - lo * 0.2 * 60) < 1e-4
            v, om, acc, sk = LC.solve(r, H, 32, None, st, [2], ft=d)
            res = LC.residuals(S, v, om)
            print("lock at", lo, ": rate - lb", res[3] - S["lb"], "angular", res[0], "off-axis", res[1], res[2])
            assert abs(res[3] - S["lb"]) <= RESIDUAL_BOUND and max(res[:3]) <= RESIDUAL_BOUND


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_slider_frames_places_a_slider_without_gap_tilt_or_travel():
    lens = list(LC.LENGTHS)
    st = LC.synthetic_state(lens)
    jr = LC.JC.main_rig(lens, (st["x"] + st["delta"]).astype(f32))[0]
    rig = np.zeros(len(jr), _capi.SLIDER_DTYPE)
    for k in ("world", "body", "other"):
        rig[k] = jr[k]
    # the sliders whose ends lie within 3.2 of each other: an arm of 1.6 at most, rounded to f32 once - 6e-8 a component and end - where the
    # 1e-6 asked of the gap leaves no room for the arm of 5 and more that a pair from opposite corners of the lattice has
    x = (st["x"] + st["delta"]).astype(np.float64)
    off = LC.SC.offsets(lens)
    ga = off[rig["world"]] + rig["body"]
    gb = np.where(rig["other"] >= 0, off[rig["world"]] + rig["other"], ga)
    rig = rig[np.linalg.norm(x[ga] - x[gb], axis=1) < 3.2]
    assert len(rig) > 100 and set(rig["world"].tolist()) == {LC.ANCHOR, LC.CHAIN, LC.CHAIN_REV, LC.STAR, LC.RING, LC.FULL}
    rig["beta"] = H                          # s = beta / h = 1: g1, g2 and gw are the errors themselves
    LC.place(rig, st, lens, seed=77)
    assert np.any(rig["other"] < 0) and rig["pa"].dtype == f32
    S = LC.setup(rig, H, np.zeros(len(rig), f32), st, lens, np.float64)
    worst = [max(float(np.abs(x[k]).max()) for x in S) for k in ("C", "g1", "g2", "gw", "d", "e")]
    print("slider_frames, float64 setup of the f32 frames: largest |C|, |g1|, |g2|, |gw|, |d|, |e|:", worst)
    assert max(worst) < 1e-6 and not any(x["skip"] for x in S)
    d, off_axis, e = LC.travel(rig, st, lens)
    assert np.abs(d).max() < 1e-6 and off_axis.max() < 1e-6 and e.max() < 1e-6
    # unit and perpendicular: what mgf_batch_set_sliders asks of a record
    for a, u in (("ax", "ua"), ("bx", "ub")):
        A, U = rig[a].astype(np.float64), rig[u].astype(np.float64)
        assert np.abs(np.sum(A * A, axis=1) - 1).max() < 1e-6 and np.abs(np.sum(U * U, axis=1) - 1).max() < 1e-6 and np.abs(np.sum(A * U, axis=1)).max() < 1e-6
    # the far end the world: pb is the anchor, bx the axis, as given
    fr = mgf_amd.slider_frames({"x": [[1, 2, 3]], "q": [[1, 0, 0, 0]]}, None, [[1, 2.5, 3]], [[0, 0, 2]])
    assert fr["pb"].tolist() == [[1, 2.5, 3]] and fr["bx"].tolist() == [[0, 0, 1]] and fr["pa"].tolist() == [[0, 0.5, 0]] and fr["ax"].tolist() == [[0, 0, 1]]
    assert fr["ua"].tobytes() == fr["ub"].tobytes() and set(fr) == {"pa", "pb", "ax", "ua", "bx", "ub"}


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_what_needs_no_device_is_refused_in_the_headers_order_with_the_rig_unchanged():
    lib = mgf_amd.load_library()
    INV = _capi.ERR_INVALID

    def err():
        return lib.mgf_last_error().decode()
    fake = C.c_void_p(16)   # a handle that is never dereferenced
    rig = np.zeros(4, _capi.SLIDER_DTYPE)
    out = C.c_void_p(1 << 21)
    h = C.c_float(1.0 / 60.0)
    assert lib.mgf_batch_slider_count(None) == -1
    assert lib.mgf_batch_set_sliders(None, rig.ctypes.data, 4) == INV and "NULL" in err()
    assert lib.mgf_batch_set_sliders(None, None, 0) == INV and "NULL" in err()
    assert lib.mgf_batch_set_sliders(fake, None, 4) == INV and "NULL" in err()
    assert lib.mgf_batch_set_sliders(fake, rig.ctypes.data, -1) == INV and "negative" in err()
    assert lib.mgf_batch_set_sliders(fake, rig.ctypes.data, 1 << 31) == INV and "too many" in err()
    for fn in (lib.mgf_batch_set_slider_targets, lib.mgf_batch_set_slider_targets_dev):
        assert fn(None, out, 1) == INV and "NULL" in err()
        assert fn(None, None, 0) == INV and "NULL" in err()                                   # the handle first
        for rows in (0, -1, (1 << 20) + 1):
            assert fn(fake, out, rows) == INV and "rows must be in [1, 2^20]" in err(), rows
    for fn in (lib.mgf_batch_solve_sliders, lib.mgf_batch_solve_sliders_dev):
        assert fn(None, h, 4, 0, out) == INV and "NULL" in err()
        assert fn(None, C.c_float(np.nan), -1, -1, None) == INV and "NULL" in err()           # the handle first
        for bad in (np.nan, np.inf, -np.inf):
            assert fn(fake, C.c_float(bad), -1, -1, out) == INV and "h is not finite" in err(), bad   # h ahead of iters
        assert fn(fake, h, -1, -1, out) == INV and "iters is negative" in err()               # iters ahead of row
    src = read("mgf_amd", "csrc", RIG_FILE)
    body = src[src.index('extern "C" mgf_status mgf_batch_set_sliders('):src.index('extern "C" int64_t mgf_batch_slider_count(')]
    plan_call = "batch_joint_plan(b->sliders, j, n);"
    # (the two checks of `other`, with their two refusals, are the joint rigs' shared step; the plan step makes the table one row of zeros:
    # tests/test_world_batch_joint_family_host.py)
    marks = ["batch_rig_set_args(b, j, n_in)", 'batch_rig_ref_check(b, r.world, r.body, 0, "slider")', "batch_joint_other_check<SliderKind>(b, r)",
             "r.flags & ~(uint32_t)(MGF_SLIDER_LIMIT | MGF_SLIDER_MOTOR | MGF_SLIDER_LOCK)", "(r.flags & MGF_SLIDER_LOCK) && (r.flags & (MGF_SLIDER_LIMIT | MGF_SLIDER_MOTOR))",
             "a word of a slider is not finite (fmax may be +inf): the rig was not changed", "a slider's pad0 or pad1 is not 0: the rig was not changed",
             "a slider's beta is not in [0, 1]: the rig was not changed", "a slider's fmax is negative: the rig was not changed", "a slider's lo is above its hi: the rig was not changed",
             "is not of unit length: the rig was not changed", "is not perpendicular to its axis: the rig was not changed",
             "++per_world[(size_t)r.world] > MGF_BATCH_MAX_WORLD_SLIDERS", plan_call]
    order = [body.index(s) for s in marks]
    assert order == sorted(order), order
    assert body.count("the rig was not changed") == 12 - 2
    assert not re.search(r"b->sliders\.|\bR\.", body.replace(plan_call, ""))                 # the rig changes in the plan step alone
    assert not re.search(r"<<<|Async|hipMalloc|\.ensure\(|h2d\(", body)                      # no device work at all
    shared = read("mgf_amd", "csrc", "host_batch_joint.inc")
    assert "joint_unit(joint_dot(r.ax, r.ax))" in body and "static double joint_dot(const mgf_vec3& a, const mgf_vec3& b) { return (double)a.x * b.x" in shared   # in double on the host
    assert "static bool joint_unit(double a) { return std::fabs(a - 1.0) <= 1e-3; }" in shared and "> 1e-3" in body   # the hinges' 1e-3, and their helpers
    # what tests/test_world_batch_rigs_host.py asks of a rig file: the shared steps used, not copied
    assert src.count("batch_rig_set_args(b, ") == 1 and src.count("batch_rig_up(") == 0 and "batch_rig_up(b, R, T::word, 3)" in shared and 'word = "slider";' in src
    for gone in ("BatchQueryPlan plan(", "batch_rig_upload(", "names a body its world does not hold", '"batch is NULL"', "std::stable_sort("):
        assert gone not in src, gone
    host = read("mgf_amd", "csrc", "host_batch.inc")
    stale = host[host.index("static void batch_rigs_stale("):host.index('extern "C" mgf_status mgf_batch_add_bodies(')]
    assert host.count("BatchJointRig<mgf_batch_slider> sliders;") == 1 and "b->sliders.stale = true;" in stale
    assert '"sliders_skipped"' in host[host.index('extern "C" mgf_status mgf_batch_counter('):]
    # the target and the solve calls are one-line forwards to the joint rigs' shared steps, whose order - the refusals (the ball joints',
    # the row behind them), the context, (device form) the pointer looked up, and only then the copy or the first thing enqueued; no
    # wait in the device forms, one in the host form of the solve with the give-up reported behind it; one launch behind batch_push and
    # ready, of the named row, counted once - tests/test_world_batch_joint_family_host.py holds
    for line in ('extern "C" mgf_status mgf_batch_set_slider_targets(mgf_batch* b, const float* w, int64_t rows) { return batch_joint_targets<SliderKind>(b, w, rows, hipMemcpyHostToDevice); }',
                 "  return batch_joint_targets<SliderKind>(b, w_dev, rows, hipMemcpyDeviceToDevice);\n}", "  return batch_joint_solve<SliderKind>(b, h, iters, row, impulse_out);\n}",
                 "  return batch_joint_solve_dev<SliderKind>(b, h, iters, row, impulse_out_dev);\n}"):
        assert src.count(line) == 1, line
    entries = src[src.index('extern "C" int64_t mgf_batch_slider_count('):]
    assert entries.count('extern "C"') == 5 and entries.count(";") == 5 and entries.count("return ") == 5      # nothing but the forwards
    kind = src[src.index("struct SliderKind {"):src.index('extern "C" mgf_status mgf_batch_set_sliders(')]
    assert "launches = MGF_BATCH_SLIDER_LAUNCHES," in kind and "launch = k_batch_slider_solve<GATED>;" in kind and "table = true;" in kind and "using Rows = SliderRows;" in kind
    assert "static constexpr uint32_t kWords = 7, kFloats = 8;" in read("mgf_amd", "csrc", "k_batch_slider.h")   # 32 bytes a slider of impulse
    assert "batch_single_parts(" not in src                                                   # sliders read no shapes


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_launch_sits_behind_the_hinges_and_ahead_of_the_tick_and_is_counted_once():
    host = read("mgf_amd", "csrc", "host_batch.inc")
    roll = read("mgf_amd", "csrc", "host_batch_rollout.inc")
    core = roll[roll.index("static mgf_status batch_rollout_run("):roll.index('extern "C" mgf_status mgf_batch_rollout_dev(')]
    assert "!b->sliders.recs.empty()" in core and "!joints && !hinges && !sliders &&" in core      # the early return to the plain step sees the slider rig
    assert (core.index("batch_push(") < core.index("batch_joint_hook<HingeKind>(") < core.index("batch_joint_hook<SliderKind>(b, dt, iters, &H.sliders)")
            < core.index("batch_step_run(b, dt, iters, n_ticks, stats, &H)"))
    train = host[host.index("static mgf_status batch_step_run("):host.index('extern "C" mgf_status mgf_batch_step(')]
    shared = read("mgf_amd", "csrc", "host_batch_joint.inc")   # (a kind's part of the train: tests/test_world_batch_joint_family_host.py holds its steps)
    tick = "batch_joint_tick<SliderKind>(b, hook->sliders, t, &hook->launches)"
    assert (train.index("k_batch_rollout_act<") < train.index("batch_joint_tick<JointKind>(") < train.index("batch_joint_tick<HingeKind>(")
            < train.index(tick) < train.index("batch_collide("))
    assert train.count("batch_joint_tick<SliderKind>") == 1 and "per_tick = MGF_BATCH_ROLLOUT_SLIDER_LAUNCHES_PER_TICK;" in read("mgf_amd", "csrc", RIG_FILE)
    assert "if (T::table) H.A.w = R.w.p + (size_t)std::min<int64_t>((int64_t)t, R.rows - 1) * R.recs.size();" in shared    # tick t reads row min(t, rows - 1)
    # what the kernel reads of the handle is looked up again for every pass: inside the loop over the passes, ahead of the loop over the ticks
    assert train.index("for (uint32_t first = 0, pass = 0;") < train.index("batch_joint_pass<SliderKind>(b, hook->sliders);") < train.index("for (uint32_t t = first; t < NT; ++t)")
    assert "H.A.done = b->d_done.p; H.A.act = b->d_act.p;" in shared
    assert "d2h(ctx, err, b->d_err.p, 2)" in train                                              # the read-back is as it was: the solvers' give-up word
    step = host[host.index('extern "C" mgf_status mgf_batch_step('):host.index('extern "C" mgf_status mgf_batch_read_constraints(')]
    assert "batch_step_run(b, dt, iters, n_ticks, stats, nullptr)" in step and "slider" not in step   # mgf_batch_step applies no slider


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_kernel_has_the_hinge_solvers_loop_shape_a_bounded_spin_and_no_float_atomic():
    k = read("mgf_amd", "csrc", "k_batch_slider.h")
    entry = k[k.index("void k_batch_slider_solve("):]
    assert entry[:entry.index("\n}\n")] == "void k_batch_slider_solve(BatchJointArgs A) {\n  batch_joint_loop<SliderRows, GATED>(A);"
    # the kernel is one call of the joint solvers' skeleton: the loop shape is asserted of the skeleton, the rows of SliderRows::sweep,
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
    assert loop.count("s_sleep") == 1
    rows = [sweep.index("// slider row: " + w) for w in ("the motor", "the axis", "the three angular rows", "the two off-axis rows")]
    assert rows == sorted(rows) and loop.count("s_dyn[2 * sa] = ") == 1 and loop.count("= s_dyn[2 * sa]") == 1   # all rows in one turn, the velocities in registers between them
    assert loop.index("= s_dyn[2 * sa]") < loop.index("R.sweep(va, oa, vb, ob, has_b);") < loop.index("s_dyn[2 * sa] = ") and "s_dyn" not in sweep
    assert "++spins > kBatchSpinLimit" in loop and "A.err[1] = 1u;" in loop and "A.err[0]" not in k
    assert "GATED" not in loop and "A.done" not in loop and "break" not in loop and "continue" not in loop and "return" not in loop
    back = body[body.index("if (s_fail != 0u) return;"):]
    assert "srec[4 * (size_t)body] = s_dyn[2 * s];" in back and "srec[4 * (size_t)body + 1] = s_dyn[2 * s + 1];" in back and "+ 2]" not in back   # words 0 and 1 alone
    assert len(re.findall(r"__global__ __launch_bounds__\(kBatchBlock\)", k)) == len(re.findall(r"__global__", k)) == 1
    assert not re.search(r"A\.act\[[^\]]+\] =[^=]", k) and not re.search(r"A\.done\[[^\]]+\] =[^=]", k)
    assert not re.search(r"k_batch_(hinge|joint)\w*<", k.replace("k_batch_hinge_solve's", ""))     # (the kernels of the other rigs are selected by those prefixes)
    assert "atan" not in k and "sinf" not in k and "cosf" not in k and "sqrt" not in k        # + - * / and comparisons


# ---- 9 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_new_kernel_uses_no_scratch_and_spills_nothing():
    if not os.path.exists(os.path.join(ROOT, "mgf_amd", "libmgf_hip.so")) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    rows = kernel_resources("k_batch_slider")
    assert set(rows) == {"k_batch_slider_solve<false>", "k_batch_slider_solve<true>"}, sorted(rows)
    design = re.sub(r"\s+", " ", read("DESIGN.md"))
    for name, v in sorted(rows.items()):
        print(name, ": vgpr, sgpr, scratch, static lds, sgpr spills, vgpr spills =", v)
        assert v[2] == "0" and v[4] == "0" and v[5] == "0", (name, v)    # no scratch, no spills
        assert int(v[3]) <= 16, (name, v)                                 # static LDS: the give-up flag alone
        assert "`%s` %s / %s / %s / 0 / 0" % (name, v[0], v[1], v[3]) in design, (name, v)
    old = kernel_resources("k_batch_joint")                              # the ball joints' and the hinges' kernels: 80 / 60 and 105 / 67 until the three solvers became one skeleton
    assert old == {"k_batch_joint_solve<false>": ("78", "51", "0", "16", "0", "0"), "k_batch_joint_solve<true>": ("78", "51", "0", "16", "0", "0")}, old
    old = kernel_resources("k_batch_hinge")
    assert old == {"k_batch_hinge_solve<false>": ("103", "55", "0", "16", "0", "0"), "k_batch_hinge_solve<true>": ("103", "55", "0", "16", "0", "0")}, old


# ---- 10 -----------------------------------------------------------------------------------------------------------------------------------
def test_the_binding_marshals_a_rig_and_turns_a_wrong_tensor_down_before_it_calls_c():
    import torch

    class Handle(mgf_amd.WorldBatch):   # no context, no C handle: a call that got as far as C would fail differently
        def __init__(self):
            self._h, self.n_worlds = None, 2

        def slider_count(self):
            return 4

    b, n = Handle(), 4
    for t in (torch.zeros((n, 8), dtype=torch.float64), torch.zeros((8, n), dtype=torch.float32).t(), torch.zeros((n - 1, 8), dtype=torch.float32),
              torch.zeros((n, 3), dtype=torch.float32)):
        with pytest.raises(ValueError) as e:
            b.solve_sliders_dev(0.01, 4, impulses_dev=t)
        assert "on cpu" not in str(e.value), str(e.value)
    with pytest.raises(ValueError, match="on cpu"):
        b.solve_sliders_dev(0.01, 4, impulses_dev=torch.zeros((n, 8), dtype=torch.float32))
    with pytest.raises(ValueError, match="on cpu"):
        b.set_slider_targets_dev(torch.zeros((3, n), dtype=torch.float32))
    with pytest.raises(ValueError):
        b.set_slider_targets_dev(torch.zeros((3, n + 1), dtype=torch.float32))
    with pytest.raises(ValueError):
        b.set_slider_targets(np.zeros((3, n + 1), np.float32))
    with pytest.raises(mgf_amd.MgfError):                               # and a call whose arguments are all in order does reach C
        b.solve_sliders_dev(0.01, 4, row=1, impulses_dev=1 << 21)
    with pytest.raises(mgf_amd.MgfError):
        b.solve_sliders(0.01, 4, impulses=True)
    with pytest.raises(mgf_amd.MgfError):
        b.set_slider_targets(np.zeros(n, np.float32))                   # one row
    with pytest.raises(mgf_amd.MgfError):
        b.set_sliders([0, 1, 1], [0, 1, 2], other=[1, -1, 0], ax=(0, 0, 1), ua=(1, 0, 0), bx=(0, 0, 1), ub=(1, 0, 0), beta=0.2, lo=-0.5, hi=0.7, limit=True)
    with pytest.raises(ValueError):
        b.set_sliders([0, 1, 1], [0, 1])                                # neither one nor n
    seen = {}

    class Lib:
        def mgf_batch_set_sliders(self, h, p, n):
            seen["rig"] = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (n * 112,)).view(_capi.SLIDER_DTYPE).copy()
            return 0
    real = _capi.load_library
    _capi.load_library = lambda: Lib()
    try:
        b.set_sliders([0, 1, 1], [0, 1, 2], other=[1, -1, 0], ax=(0, 0, 1), ua=(1, 0, 0), bx=(0, 0, 1), ub=(1, 0, 0), beta=0.2, lo=[-0.5, 0.1, 0.25], hi=[0.7, 0.7, 0.25],
                      fmax=[np.inf, 2.0, 0.0], limit=[True, False, False], motor=[False, True, False], lock=[False, False, True])
        rig = seen["rig"]
        b.set_sliders(rig)                                              # a SLIDER_DTYPE array goes through as it is
        assert seen["rig"].tobytes() == rig.tobytes()
    finally:
        _capi.load_library = real
    assert rig["flags"].tolist() == [1, 2, 4] and rig["other"].tolist() == [1, -1, 0] and np.isinf(rig["fmax"][0]) and rig["fmax"][1] == 2
    assert rig["lo"].tolist() == [f32(-0.5), f32(0.1), f32(0.25)] and rig["hi"].tolist() == [f32(0.7), f32(0.7), f32(0.25)]
    assert not rig["pad0"].any() and not rig["pad1"].any() and rig["ax"].tolist() == [[0, 0, 1]] * 3
