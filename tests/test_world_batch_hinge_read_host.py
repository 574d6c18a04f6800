"""The hinge encoders of a batch (mgf_batch_read_hinges, mgf_batch_read_hinges_dev, mgf_batch_set_hinge_trace, mgf_batch_hinge_trace_rows,
mgf_batch_get_hinge_trace, mgf_batch_get_hinge_trace_dev) without a GPU: the header, the library, the binding and the documents carry
the calls, the record of 32 bytes and the constants; what needs no device is refused in the header's order; the f32 restatement of the
reading (tests/batch_hinge_read_cases.py) holds against the float64 one within bounds derived from the count of rounded operations, its
angle against tests/batch_hinge_cases.py's thetas, its side against that file's setup; the arm's angle stays clear of its limits; the
kernel's reading holds the hinge's own lines, the kernel uses no scratch and spills nothing, and the solvers' kernels are as they were.
What the hinge encoders share with the sliders' - the kernel's skeleton, the host steps, the train's site - is asserted once, in
tests/test_world_batch_encoder_family_host.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mgf_amd
from mgf_amd import _capi
from tests import batch_hinge_cases as HC
from tests import batch_hinge_read_cases as HR
from tests.util import ROOT, kernel_resources, read

f32 = np.float32
CALLS = ("mgf_batch_read_hinges", "mgf_batch_read_hinges_dev", "mgf_batch_set_hinge_trace", "mgf_batch_hinge_trace_rows", "mgf_batch_get_hinge_trace",
         "mgf_batch_get_hinge_trace_dev")
READ_FILE = "host_batch_joint_read.inc"
NAMES = ["c", "sn", "rate", "side", "gap", "tilt2"]


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
def test_header_library_binding_and_documents_carry_the_calls_the_record_and_the_constants():
    h = read("include", "mgf_hip.h")
    flat_h = re.sub(r"\s+", " ", h)
    for sig in ("MGF_API mgf_status mgf_batch_read_hinges(mgf_batch* b, mgf_hinge_reading* out);",
                "MGF_API mgf_status mgf_batch_read_hinges_dev(mgf_batch* b, mgf_hinge_reading* out_dev);",
                "MGF_API mgf_status mgf_batch_set_hinge_trace(mgf_batch* b, int64_t rows, int32_t format);",
                "MGF_API int64_t mgf_batch_hinge_trace_rows(const mgf_batch* b);",
                "MGF_API mgf_status mgf_batch_get_hinge_trace(mgf_batch* b, void* out, int64_t row0, int64_t n_rows);",
                "MGF_API mgf_status mgf_batch_get_hinge_trace_dev(mgf_batch* b, void* out_dev, int64_t row0, int64_t n_rows);"):
        assert sig in flat_h, sig
    assert h.index("MGF_API mgf_status mgf_batch_solve_hinges_dev(") < h.index("/* ---- hinge encoders:") < h.index("/* ---- rollout touch traces")
    consts = (("MGF_BATCH_HINGE_READ_LAUNCHES", _capi.BATCH_HINGE_READ_LAUNCHES, 1),
              ("MGF_BATCH_ROLLOUT_HINGE_READ_LAUNCHES_PER_TICK", _capi.BATCH_ROLLOUT_HINGE_READ_LAUNCHES_PER_TICK, 1),
              ("MGF_HINGE_TRACE_READING", _capi.HINGE_TRACE_READING, 0), ("MGF_HINGE_TRACE_FULL", _capi.HINGE_TRACE_FULL, 1))
    flat = re.sub(r"\s+", " ", read("INTEGRATION.md"))
    for name, value, want in consts:
        m = re.search(r"#define %s\s+(\d+)" % name, h)
        assert m and int(m.group(1)) == value == want, name
        assert re.search(r"pub const %s: (i64|i32) = %d;" % (name, want), flat), name
        assert getattr(mgf_amd, name[4:]) is getattr(_capi, name[4:]), name
    section = h[h.index("/* ---- hinge encoders:"):h.index("MGF_API mgf_status mgf_batch_get_hinge_trace_dev(")]
    section = re.sub(r"\n \* ?(?! )", " ", section)                          # (a sentence may run over the end of a line of the comment)
    for word in ("(c, sn, rate, side, gap.x, gap.y, gap.z, tilt2)", "c = dot(U1, T1);  sn = dot(U1, T2)", "rate = dot(omega_b - omega_a, A)",
                 "cphi = c * cm + sn * sm;  sphi = sn * cm - c * sm", "LIMIT and cphi <= ch:  sphi >= 0: side = +1.0f;  else side = -1.0f;  otherwise side = 0.0f",
                 "gap = C", "e1 = dot(B, T1);  e2 = dot(B, T2);  tilt2 = e1 * e1 + e2 * e2", "other == -1: B = bx, U1 = ub, Pb = pb, omega_b = 0",
                 "NO arctangent", "no division", "no hinge is skipped", "non-finite words", "several components", "untouched to the bit", "drive_launches",
                 "rollout_launches", "mgf_batch_read_hinges_dev(b, row t)", "bit for bit", "zeros with iters == 0", "NO clamp", "stay as they were",
                 "am / dt", "mgf_batch_set_hinges sets it back to 0 rows", "launch for launch", "in the pass in which it completes t", "OUT OF SCOPE",
                 "servo", "ball joints", "mgf_rollout_traces", "ring-buffer", "lone mgf_world", "hipGraph", "nothing enqueued", "the table as it was",
                 "aligned to 16 bytes"):
        assert word in section, word
    # the hinge section's out-of-scope sentence stays and points here
    hinge = h[h.index("/* ---- hinge joints between bodies"):h.index("#define MGF_HINGE_LIMIT")]
    assert "the impulses per tick of a rollout; joint angle and rate as a traced observation." in hinge and "since: Hinge encoders, below" in hinge
    # the record: 32 bytes, two words of 16; the full entry 64
    assert _capi.HINGE_READING_DTYPE.itemsize == 32 and _capi.HINGE_TRACE_FULL_DTYPE.itemsize == 64
    assert list(_capi.HINGE_READING_DTYPE.names) == NAMES and [_capi.HINGE_READING_DTYPE.fields[k][1] for k in NAMES] == [0, 4, 8, 12, 16, 28]
    full = _capi.HINGE_TRACE_FULL_DTYPE
    assert list(full.names) == NAMES + ["acc", "a1", "a2", "al", "am", "pad"] and [full.fields[k][1] for k in full.names[6:]] == [32, 44, 48, 52, 56, 60]
    assert [full.fields[k][1] for k in NAMES] == [0, 4, 8, 12, 16, 28]
    assert re.search(r"typedef struct mgf_hinge_reading \{\s*float c, sn;[^\n]*\n\s*float rate;[^\n]*\n\s*float side;[^\n]*\n\s*mgf_vec3 gap;[^\n]*\n\s*float tilt2;[^\n]*\n\} mgf_hinge_reading;", h)
    lib = mgf_amd.load_library()
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    want = {"mgf_batch_read_hinges": (i32, [vp, vp]), "mgf_batch_read_hinges_dev": (i32, [vp, vp]), "mgf_batch_set_hinge_trace": (i32, [vp, i64, i32]),
            "mgf_batch_hinge_trace_rows": (i64, [vp]), "mgf_batch_get_hinge_trace": (i32, [vp, vp, i64, i64]),
            "mgf_batch_get_hinge_trace_dev": (i32, [vp, vp, i64, i64])}
    for name in CALLS:
        assert name in _capi.SYMBOLS, name
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == want[name], name
    for method in ("read_hinges", "read_hinges_dev", "set_hinge_trace", "hinge_trace_rows", "hinge_trace", "hinge_trace_dev"):
        assert callable(getattr(mgf_amd.WorldBatch, method)), method
    assert mgf_amd.HINGE_READING_DTYPE is _capi.HINGE_READING_DTYPE and mgf_amd.HINGE_TRACE_FULL_DTYPE is _capi.HINGE_TRACE_FULL_DTYPE
    assert mgf_amd.hinge_angles is _capi.hinge_angles
    for sig in ("pub fn mgf_batch_read_hinges(b: *mut mgf_batch, out: *mut mgf_hinge_reading) -> mgf_status;",
                "pub fn mgf_batch_read_hinges_dev(b: *mut mgf_batch, out_dev: *mut mgf_hinge_reading) -> mgf_status;",
                "pub fn mgf_batch_set_hinge_trace(b: *mut mgf_batch, rows: i64, format: i32) -> mgf_status;",
                "pub fn mgf_batch_hinge_trace_rows(b: *const mgf_batch) -> i64;",
                "pub fn mgf_batch_get_hinge_trace(b: *mut mgf_batch, out: *mut c_void, row0: i64, n_rows: i64) -> mgf_status;",
                "pub fn mgf_batch_get_hinge_trace_dev(b: *mut mgf_batch, out_dev: *mut c_void, row0: i64, n_rows: i64) -> mgf_status;",
                "pub struct mgf_hinge_reading { pub c: f32, pub sn: f32, pub rate: f32, pub side: f32, pub gap: mgf_vec3, pub tilt2: f32 }",
                "pub fn read_hinges(", "pub unsafe fn read_hinges_dev(", "pub fn set_hinge_trace(", "pub fn hinge_trace_rows(", "pub fn hinge_trace(",
                "pub unsafe fn hinge_trace_dev("):
        assert sig in flat, sig
    kernels = read("mgf_amd", "csrc", "kernels.h")
    assert kernels.index('#include "k_batch_hinge.h"') < kernels.index('#include "k_batch_hinge_read.h"')
    assert "k_batch_read_hinges<GATED, FORMAT> (k_batch_hinge_read.h" in kernels
    hip = read("mgf_amd", "csrc", "mgf_hip.hip")
    assert hip.index('#include "host_batch_hinge.inc"') < hip.index('#include "%s"' % READ_FILE)
    design = read("DESIGN.md")
    assert design.index("### Hinges between bodies") < design.index("### Hinge encoders") < design.index("### Rollout touch traces")
    sub = design[design.index("### Hinge encoders"):design.index("### Rollout touch traces")]
    for word in ("k_batch_read_hinges", "done[k] == t + 1 && act[k] <= t + 1", "Compiler output", "Out of scope", "batch_hinge_read_bench.py",
                 "MGF_BATCH_HINGE_READ_LAUNCHES", "MGF_BATCH_ROLLOUT_HINGE_READ_LAUNCHES_PER_TICK", "bench.py", "Measured", "72 EPS", "64 EPS"):
        assert word in sub, word
    assert "since: Hinge encoders" in design[design.index("### Hinges between bodies"):design.index("### Hinge encoders")]
    readme = read("README.md")
    assert "read_hinges" in readme and "set_hinge_trace" in readme and "hinge_angles" in readme
    assert os.path.exists(os.path.join(ROOT, "tools", "batch_hinge_read_bench.py"))


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def test_what_needs_no_device_is_refused_in_the_headers_order():
    lib = mgf_amd.load_library()
    INV = _capi.ERR_INVALID

    def err():
        return lib.mgf_last_error().decode()
    fake = C.c_void_p(16)   # a handle that is never dereferenced
    out = C.c_void_p(1 << 21)
    assert lib.mgf_batch_hinge_trace_rows(None) == -1
    for fn in (lib.mgf_batch_read_hinges, lib.mgf_batch_read_hinges_dev):
        assert fn(None, out) == INV and "NULL" in err()
        assert fn(None, None) == INV and "batch is NULL" in err()                            # the handle first
    assert lib.mgf_batch_set_hinge_trace(None, 4, 0) == INV and "batch is NULL" in err()
    assert lib.mgf_batch_set_hinge_trace(None, -1, 7) == INV and "batch is NULL" in err()     # the handle first
    for rows in (-1, (1 << 20) + 1, -(1 << 40)):
        assert lib.mgf_batch_set_hinge_trace(fake, rows, 7) == INV and "rows must be in [0, 2^20]" in err(), rows   # rows ahead of the format
    for fmt in (-1, 2, 7):
        assert lib.mgf_batch_set_hinge_trace(fake, 4, fmt) == INV and "format is neither" in err(), fmt
    for fn in (lib.mgf_batch_get_hinge_trace, lib.mgf_batch_get_hinge_trace_dev):
        assert fn(None, out, 0, 1) == INV and "batch is NULL" in err()
        assert fn(None, None, -1, -1) == INV and "batch is NULL" in err()                     # the handle first
        assert fn(fake, out, -1, -1) == INV and "row0 is negative" in err()                   # row0 ahead of n_rows
        assert fn(fake, out, 0, -1) == INV and "n_rows is negative" in err()
    # (the order of refusals, context, pointer look-up and first enqueue inside every call: tests/test_world_batch_encoder_family_host.py)
    # mgf_batch_set_hinges turns the trace off, with no device work
    rig = read("mgf_amd", "csrc", "host_batch_hinge.inc")
    body = rig[rig.index('extern "C" mgf_status mgf_batch_set_hinges('):rig.index('extern "C" int64_t mgf_batch_hinge_count(')]
    assert body.index("batch_joint_plan(b->hinges, j, n);") < body.index("b->hinge_trace.rows = 0;") and not re.search(r"<<<|Async|hipMalloc|hipFree|\.ensure\(", body)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def _seeded():
    lens = list(HC.LENGTHS)
    st = HC.synthetic_state(lens)
    rig, planted, W = HC.main_rig(lens, st)
    return lens, st, rig, planted


def test_the_f32_reading_holds_against_the_float64_one_within_the_bounds_of_its_rounded_operations():
    """Every hinge of the seeded rig (tests/batch_hinge_cases.py: main_rig on synthetic_state, 277 hinges, every hinge angle in (-pi, pi),
    axes tilted by 0.1 rad or less) read in f32 and in float64.  The bounds are tests/batch_hinge_read_cases.py's, derived there from the
    count of rounded operations between the quaternions and c, sn: 64 EPS on c and sn (worst case 121 u = 60.5 EPS on sn), 72 EPS on
    atan2(sn, c) in radians, 20 EPS (|omega_a| + |omega_b|) on the rate.  Measured here on the CPU: the largest difference of c is 1.80e-7 = 1.51 EPS, of sn
    2.67e-7 = 2.24 EPS, of the angle 2.07e-7 rad = 1.73 EPS against the float64 reading and the same against
    batch_hinge_cases.thetas, of the rate 1.78e-7 of |omega_a| + |omega_b| = 1.50 EPS - the roundings never all pull the same way."""
    lens, st, rig, planted = _seeded()
    r32 = HR.readings(rig, st, lens, f32)
    r64 = HR.readings(rig, st, lens, np.float64)
    assert r32.dtype == f32 and r64.dtype == np.float64 and len(rig) == 21 + HC.MAX
    d_c, d_sn = np.abs(r32[:, 0] - r64[:, 0]), np.abs(r32[:, 1] - r64[:, 1])
    th32, rate32 = mgf_amd.hinge_angles(HR.as_readings(r32))
    assert th32.dtype == np.float64 and th32.tobytes() == np.arctan2(r32[:, 1].astype(np.float64), r32[:, 0].astype(np.float64)).tobytes()
    assert rate32.tobytes() == r32[:, 2].astype(np.float64).tobytes()
    th64 = np.arctan2(r64[:, 1], r64[:, 0])
    want = HC.thetas(rig, st, lens)

    def turn(a):                                                                 # the difference of two angles, through the cut at pi
        return np.abs((a + np.pi) % (2 * np.pi) - np.pi)
    d_th, d_want = turn(th32 - th64), turn(th32 - want)
    off = np.concatenate([[0], np.cumsum(lens)])
    ga = off[rig["world"]] + rig["body"]
    gb = np.where(rig["other"] >= 0, off[rig["world"]] + rig["other"], ga)
    om = st["omega"].astype(np.float64)
    scale = np.linalg.norm(om[ga], axis=1) + np.where(rig["other"] >= 0, np.linalg.norm(om[gb], axis=1), 0.0)
    d_rate = np.abs(r32[:, 2] - r64[:, 2]) / scale
    print("f32 against f64 over", len(rig), "hinges: largest |dc| %.3g (%.2f EPS), |dsn| %.3g (%.2f EPS), |dtheta| %.3g rad (%.2f EPS), against thetas %.3g rad, "
          "|drate| / (|omega_a| + |omega_b|) %.3g (%.2f EPS); bounds %d, %d, %d EPS"
          % (d_c.max(), d_c.max() / HR.EPS, d_sn.max(), d_sn.max() / HR.EPS, d_th.max(), d_th.max() / HR.EPS, d_want.max(), d_rate.max(), d_rate.max() / HR.EPS,
             round(HR.C_SN_BOUND / HR.EPS), round(HR.THETA_BOUND / HR.EPS), round(HR.RATE_BOUND / HR.EPS)))
    assert HR.C_SN_BOUND == 64 * HR.EPS and HR.THETA_BOUND == 72 * HR.EPS and HR.RATE_BOUND == 20 * HR.EPS
    assert d_c.max() <= HR.C_SN_BOUND and d_sn.max() <= HR.C_SN_BOUND
    assert d_th.max() <= HR.THETA_BOUND and d_want.max() <= HR.THETA_BOUND
    assert d_rate.max() <= HR.RATE_BOUND
    assert np.ptp(want) > 6.0 and np.all(r64[:, 0] ** 2 + r64[:, 1] ** 2 >= 0.99)         # every angle; the radius the angle's bound assumes
    # gap and tilt2: the anchors' gap is the ball joints' C, tilt2 the squared sine of the angle between the axes
    live = [i for i in range(len(rig)) if i not in planted or rig["flags"][i] & HC.MOTOR]      # (the planted arm of 3e38 overflows its gap in f32)
    assert np.allclose(r32[live, 4:7], r64[live, 4:7], rtol=1e-5, atol=1e-5)
    A, T1, T2, B, U1 = HC.frames_world(rig, st, lens)
    assert np.allclose(r64[:, 7], np.sum(np.cross(A, B) ** 2, axis=1), rtol=0, atol=1e-7)   # (frames rounded to f32 are orthonormal to EPS)
    assert np.allclose(r32[:, 7], r64[:, 7], rtol=0, atol=32 * HR.EPS)
    assert r64[:, 7].max() <= np.sin(0.1) ** 2 * 1.001 and r64[:, 7].max() > 1e-4


def test_side_is_the_setups_side_and_says_which_limit_row_the_next_solve_turns_on():
    lens, st, rig, planted = _seeded()
    for ft in (f32, np.float64):
        r = HR.readings(rig, st, lens, ft)
        S = HC.setup(rig, f32(1.0 / 60.0), np.zeros(len(rig), f32), st, lens, ft)
        assert [float(x) for x in r[:, 3]] == [float(s["side"]) for s in S]
        assert all(r[i, 0] == S[i]["c"] and r[i, 1] == S[i]["sn"] for i in range(len(rig)))       # the same lines, the same bits
        assert all(np.array_equal(r[i, 4:7], S[i]["C"]) or i in planted for i in range(len(rig)))
    case = np.arange(len(rig)) % len(HC.CASES)
    side = HR.readings(rig, st, lens)[:, 3]
    names = np.array(HC.CASES)[case]
    assert set(side[names == "limit_below"]) == {-1.0} and set(side[names == "limit_above"]) == {1.0} and set(side[names == "limit_inside"]) == {0.0}
    assert set(side[names == "none"]) == {0.0} and set(side[names == "motor_free"]) == {0.0} and set(np.abs(side[names == "limit_wide"])) == {1.0}
    # the small rig of the GPU tests: every case where it should be
    small, cases = HR.small_rig(lens, st, 257, worlds=(HC.CHAIN, HC.FULL))
    s = HR.readings(small, st, lens)[:, 3]
    assert [float(x) for x in s] == [HR.SIDE_OF[HR.LIMIT_CASES[c]] for c in cases]
    assert np.bincount(small["world"], minlength=len(lens)).max() <= HC.MAX and np.any(small["other"] == -1) and np.any(small["other"] >= 0)
    # non-finite state gives non-finite words, and no side
    bad = {k: v.copy() for k, v in st.items()}
    ga = int(np.concatenate([[0], np.cumsum(lens)])[small["world"][0]] + small["body"][0])
    bad["q"][ga] = np.nan
    r = HR.readings(small[:1], bad, lens)
    assert np.isnan(r[0, [0, 1, 2, 4, 5, 6, 7]]).all() and r[0, 3] == 0.0


def test_the_arms_angle_stays_clear_of_its_limits_but_for_two_ticks_at_most():
    """The use case of the GPU test leaves a tick out of its `side` check where the elbow's angle is within THETA_BOUND of a limit: at most
    2 of HC.ARM_TICKS ticks.  The float64 restatement of the arm on the CPU stays within that cap - by a wide margin: the nearest tick
    is printed."""
    theta, rate = HC.arm_sim(True)
    near = np.minimum(np.abs(theta - HC.ARM_LIMIT[0]), np.abs(theta - HC.ARM_LIMIT[1]))
    print("the arm on the CPU: the tick nearest a limit is", float(near.min()), "rad from it; bound", HR.THETA_BOUND)
    assert int((near <= HR.THETA_BOUND).sum()) <= 2 and len(theta) == HC.ARM_TICKS
    assert np.any(theta < HC.ARM_LIMIT[0]) and np.any((theta > HC.ARM_LIMIT[0]) & (theta < HC.ARM_LIMIT[1]))    # both sides of lo are met


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_hinges_reading_holds_the_hinges_own_lines_and_loads_nothing_of_its_own():
    """The lane's walk, its gate ahead of every load and the stores are the skeleton's (k_batch_joint_read.h), asserted in
    tests/test_world_batch_encoder_family_host.py; here: what HingeReading forms of the ends and the frames."""
    k = read("mgf_amd", "csrc", "k_batch_hinge_read.h")
    body = k[k.index("struct HingeReading {"):k.index("template <bool GATED, int FORMAT>")]
    for line in ("const float c = dot(F.U1, F.T1), sn = dot(F.U1, F.T2);", "const float rate = dot(b.om - a.om, F.A);",
                 "const float side = hinge_side(f2u(w0.w), c, sn, w3.w, w4.w, w5.w);", "const float e1 = dot(F.B, F.T1), e2 = dot(F.B, F.T2);",
                 "const float tilt2 = e1 * e1 + e2 * e2;", "return {make_float4(c, sn, rate, side), make_float4(F.C.x, F.C.y, F.C.z, tilt2)};"):
        assert line in body, line
    assert "template <bool GATED, int FORMAT>" in k and "void k_batch_read_hinges(" in k
    assert not re.search(r"atomic|__shared__|__syncthreads|s_dyn|A\.plan|A\.slots|A\.items| / ", body)       # no plan, no LDS, no atomic, no division
    assert not re.search(r"A\.B\.\w+\[[^\]]*\] =[^=]|srec\[[^\]]*\] =[^=]", k)
    code = k[k.index("#pragma once"):] + read("mgf_amd", "csrc", "k_batch_joint_read.h").split("#pragma once")[1] + read("mgf_amd", "csrc", "k_batch_hinge_frame.h").split("#pragma once")[1]
    assert "atan" not in code and "sinf" not in code and "cosf" not in code               # no arctangent is evaluated on the device
    # the frame lines are lifted, not pasted: written once in a header of their own, which the hinges' solver uses too (and through it
    # the sliders'); an end is loaded by the joint solvers' joint_end
    assert '#include "k_batch_joint_read.h"' in k and '#include "k_batch_hinge_frame.h"' in read("mgf_amd", "csrc", "k_batch_joint_read.h")
    assert "rotate(" not in body and "cross(" not in body and "srec[" not in body
    solver = re.sub(r"//[^\n]*", "", read("mgf_amd", "csrc", "k_batch_hinge.h"))
    assert '#include "k_batch_hinge_frame.h"' in solver and "hinge_frame(a, b, has_b, w1, w2, w3, w4, w5, w6)" in solver and "rotate(" not in solver   # no second copy


def test_the_new_kernel_uses_no_scratch_and_spills_nothing_and_the_solvers_are_as_they_were():
    if not os.path.exists(os.path.join(ROOT, "mgf_amd", "libmgf_hip.so")) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    rows = kernel_resources("k_batch_read_hinges")
    assert set(rows) == {"k_batch_read_hinges<false, 0>", "k_batch_read_hinges<true, 0>", "k_batch_read_hinges<true, 1>", "k_batch_read_hinges<true, 2>"}, sorted(rows)
    design = re.sub(r"\s+", " ", read("DESIGN.md"))
    for name, v in sorted(rows.items()):
        print(name, ": vgpr, sgpr, scratch, static lds, sgpr spills, vgpr spills =", v)
        assert v[2] == "0" and v[3] == "0" and v[4] == "0" and v[5] == "0", (name, v)    # no scratch, no LDS, no spills
        assert int(v[0]) < 105, (name, v)                                                  # far fewer than the solve's
        assert "`%s` %s / %s / 0 / 0 / 0" % (name, v[0], v[1]) in design, (name, v)
    # the solvers' kernels are what tests/test_world_batch_hinges_host.py expects of them: untouched
    old = kernel_resources("k_batch_hinge_solve")                                         # (105 / 67 and 80 / 60 until the three solvers became one skeleton)
    assert old == {"k_batch_hinge_solve<false>": ("103", "55", "0", "16", "0", "0"), "k_batch_hinge_solve<true>": ("103", "55", "0", "16", "0", "0")}, old
    assert set(kernel_resources("k_batch_hinge")) == set(old)                             # (that test selects them by this substring)
    old = kernel_resources("k_batch_joint")
    assert old == {"k_batch_joint_solve<false>": ("78", "51", "0", "16", "0", "0"), "k_batch_joint_solve<true>": ("78", "51", "0", "16", "0", "0")}, old


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_binding_shapes_its_arrays_and_turns_a_wrong_tensor_down_before_it_calls_c():
    import torch

    class Handle(mgf_amd.WorldBatch):   # no context, no C handle: a call that got as far as C would fail differently
        def __init__(self, n, rows):
            self._h, self._n, self._rows = None, n, rows

        def hinge_count(self):
            return self._n

        def hinge_trace_rows(self):
            return self._rows

        def close(self):
            pass
    b = Handle(5, 4)
    with pytest.raises(ValueError, match="on cpu"):
        b.read_hinges_dev(torch.zeros((5, 8), dtype=torch.float32))
    with pytest.raises(ValueError, match="5 rows of 8"):
        b.read_hinges_dev(torch.zeros((5, 7), dtype=torch.float32))
    with pytest.raises(ValueError, match="dtype"):
        b.read_hinges_dev(torch.zeros((5, 8), dtype=torch.float64))
    with pytest.raises(ValueError, match="rows of a table of 4"):
        b.hinge_trace(2, 3)
    with pytest.raises(ValueError, match="rows of a table of 4"):
        b.hinge_trace(-1)
    with pytest.raises(ValueError, match="10 rows of 8"):
        b.hinge_trace_dev(torch.zeros((15, 8), dtype=torch.float32), 1, 2)
    b._hinge_trace_full = True
    with pytest.raises(ValueError, match="10 rows of 16"):
        b.hinge_trace_dev(torch.zeros((10, 8), dtype=torch.float32), 1, 2)
    # hinge_angles: theta in float64 of any shape, of either dtype
    r = np.zeros((2, 3), _capi.HINGE_TRACE_FULL_DTYPE)
    r["c"], r["sn"], r["rate"] = -1.0, f32(1e-7), 2.5
    th, rate = mgf_amd.hinge_angles(r)
    assert th.shape == (2, 3) and th.dtype == np.float64 and np.all(th == np.arctan2(np.float64(f32(1e-7)), -1.0)) and np.all(rate == 2.5)
