"""The slider encoders of a batch (mgf_batch_read_sliders, mgf_batch_read_sliders_dev, mgf_batch_set_slider_trace,
mgf_batch_slider_trace_rows, mgf_batch_get_slider_trace, mgf_batch_get_slider_trace_dev) without a GPU: the header, the library, the
binding and the documents carry the calls, the record of 32 bytes and the constants; what needs no device is refused in the header's
order; the f32 restatement of the reading (tests/batch_slider_read_cases.py) holds against the float64 one within bounds derived from
the rounded operations, and its words are tests/batch_slider_cases.py's setup words and its solve's first motor-row rate by bytes; the
lift's travel stays clear of its limits; the kernel's reading holds the slider's own lines, the kernel uses no scratch and spills nothing,
and the solvers' and the hinge encoders' kernels are as they were.  What the slider encoders share with the hinges' - the kernel's
skeleton, the host steps, the train's site - is asserted once, in tests/test_world_batch_encoder_family_host.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mgf_amd
from mgf_amd import _capi
from tests import batch_slider_cases as LC
from tests import batch_slider_read_cases as SR
from tests.util import ROOT, kernel_resources, read

f32 = np.float32
CALLS = ("mgf_batch_read_sliders", "mgf_batch_read_sliders_dev", "mgf_batch_set_slider_trace", "mgf_batch_slider_trace_rows", "mgf_batch_get_slider_trace",
         "mgf_batch_get_slider_trace_dev")
READ_FILE = "host_batch_joint_read.inc"
NAMES = ["d", "rate", "side", "off", "e"]


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
def test_header_library_binding_and_documents_carry_the_calls_the_record_and_the_constants():
    h = read("include", "mgf_hip.h")
    flat_h = re.sub(r"\s+", " ", h)
    for sig in ("MGF_API mgf_status mgf_batch_read_sliders(mgf_batch* b, mgf_slider_reading* out);",
                "MGF_API mgf_status mgf_batch_read_sliders_dev(mgf_batch* b, mgf_slider_reading* out_dev);",
                "MGF_API mgf_status mgf_batch_set_slider_trace(mgf_batch* b, int64_t rows, int32_t format);",
                "MGF_API int64_t mgf_batch_slider_trace_rows(const mgf_batch* b);",
                "MGF_API mgf_status mgf_batch_get_slider_trace(mgf_batch* b, void* out, int64_t row0, int64_t n_rows);",
                "MGF_API mgf_status mgf_batch_get_slider_trace_dev(mgf_batch* b, void* out_dev, int64_t row0, int64_t n_rows);"):
        assert sig in flat_h, sig
    assert h.index("MGF_API mgf_status mgf_batch_solve_sliders_dev(") < h.index("/* ---- slider encoders:") < h.index("/* name in {")
    consts = (("MGF_BATCH_SLIDER_READ_LAUNCHES", _capi.BATCH_SLIDER_READ_LAUNCHES, 1),
              ("MGF_BATCH_ROLLOUT_SLIDER_READ_LAUNCHES_PER_TICK", _capi.BATCH_ROLLOUT_SLIDER_READ_LAUNCHES_PER_TICK, 1),
              ("MGF_SLIDER_TRACE_READING", _capi.SLIDER_TRACE_READING, 0), ("MGF_SLIDER_TRACE_FULL", _capi.SLIDER_TRACE_FULL, 1))
    flat = re.sub(r"\s+", " ", read("INTEGRATION.md"))
    for name, value, want in consts:
        m = re.search(r"#define %s\s+(\d+)" % name, h)
        assert m and int(m.group(1)) == value == want, name
        assert re.search(r"pub const %s: (i64|i32) = %d;" % (name, want), flat), name
        assert getattr(mgf_amd, name[4:]) is getattr(_capi, name[4:]), name
    section = h[h.index("/* ---- slider encoders:"):h.index("MGF_API mgf_status mgf_batch_get_slider_trace_dev(")]
    lines = section.split("\n")
    section = re.sub(r"\n \* ?(?! )", " ", section)                          # (a sentence may run over the end of a line of the comment)
    for word in ("(d, rate, side, off1, off2, e.x, e.y, e.z)", "other == -1: B = bx, U1 = ub, Pb = pb, rb = 0, v_b = 0, omega_b = 0",
                 "rate = (dot(v_b - v_a, A) + dot(omega_b, sB)) - dot(omega_a, sA)",
                 "LOCK: side = 2.0f;  LIMIT and d < lo: side = -1.0f;  LIMIT and d > hi: side = +1.0f;  otherwise side = 0.0f",
                 "e = ((cross(A, B) + cross(T1, U1)) + cross(T2, U2)) * 0.5", "no division, no h and no beta", "no slider is skipped", "non-finite words",
                 "several components", "untouched to the bit", "drive_launches", "rollout_launches", "mgf_batch_read_sliders_dev(b, row t)", "bit for bit",
                 "zeros with iters == 0", "NO clamp", "stay as they were", "am / dt", "mgf_batch_set_sliders sets it back to 0 rows", "launch for launch",
                 "in the pass in which it completes t", "(p1, p2, al, am, aw.x, aw.y, aw.z, 0)", "mgf_batch_step traces nothing", "OUT OF SCOPE", "servo",
                 "ball joints", "mgf_rollout_traces", "ring-buffer", "lone mgf_world", "hipGraph", "nothing enqueued", "the table as it was", "aligned to 16 bytes"):
        assert word in section, word
    for line in ("U2 = cross(B, U1)", "ca = ra + C", "sA = cross(ca, A)", "sB = cross(rb, A)", "off1 = dot(C, T1)"):      # one f32 operation a line
        assert any(ln.strip(" *") == line for ln in lines), line
    assert any(ln.strip(" *").startswith("d = dot(C, A) ") for ln in lines) and any(ln.strip(" *").startswith("off2 = dot(C, T2) ") for ln in lines)
    # the slider section's out-of-scope sentence stays and points here
    slider = h[h.index("/* ---- slider joints between bodies"):h.index("#define MGF_SLIDER_LIMIT")]
    assert "slider encoders - d, rate and side as a call and as a traced row" in slider and "since: Slider encoders, below" in slider
    # the record: 32 bytes, two words of 16; the full entry 64
    assert _capi.SLIDER_READING_DTYPE.itemsize == 32 and _capi.SLIDER_TRACE_FULL_DTYPE.itemsize == 64
    assert list(_capi.SLIDER_READING_DTYPE.names) == NAMES and [_capi.SLIDER_READING_DTYPE.fields[k][1] for k in NAMES] == [0, 4, 8, 12, 20]
    assert _capi.SLIDER_READING_DTYPE["off"].shape == (2,) and _capi.SLIDER_READING_DTYPE["e"].shape == (3,)
    full = _capi.SLIDER_TRACE_FULL_DTYPE
    assert list(full.names) == NAMES + ["p1", "p2", "al", "am", "aw", "pad"] and [full.fields[k][1] for k in full.names[5:]] == [32, 36, 40, 44, 48, 60]
    assert [full.fields[k][1] for k in NAMES] == [0, 4, 8, 12, 20]
    assert re.search(r"typedef struct mgf_slider_reading \{\s*float d;[^\n]*\n\s*float rate;[^\n]*\n\s*float side;[^\n]*\n\s*float off1, off2;[^\n]*\n\s*mgf_vec3 e;[^\n]*\n\} mgf_slider_reading;", h)
    lib = mgf_amd.load_library()
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    want = {"mgf_batch_read_sliders": (i32, [vp, vp]), "mgf_batch_read_sliders_dev": (i32, [vp, vp]), "mgf_batch_set_slider_trace": (i32, [vp, i64, i32]),
            "mgf_batch_slider_trace_rows": (i64, [vp]), "mgf_batch_get_slider_trace": (i32, [vp, vp, i64, i64]),
            "mgf_batch_get_slider_trace_dev": (i32, [vp, vp, i64, i64])}
    for name in CALLS:
        assert name in _capi.SYMBOLS, name
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == want[name], name
    for method in ("read_sliders", "read_sliders_dev", "set_slider_trace", "slider_trace_rows", "slider_trace", "slider_trace_dev"):
        assert callable(getattr(mgf_amd.WorldBatch, method)), method
    assert mgf_amd.SLIDER_READING_DTYPE is _capi.SLIDER_READING_DTYPE and mgf_amd.SLIDER_TRACE_FULL_DTYPE is _capi.SLIDER_TRACE_FULL_DTYPE
    for sig in ("pub fn mgf_batch_read_sliders(b: *mut mgf_batch, out: *mut mgf_slider_reading) -> mgf_status;",
                "pub fn mgf_batch_read_sliders_dev(b: *mut mgf_batch, out_dev: *mut mgf_slider_reading) -> mgf_status;",
                "pub fn mgf_batch_set_slider_trace(b: *mut mgf_batch, rows: i64, format: i32) -> mgf_status;",
                "pub fn mgf_batch_slider_trace_rows(b: *const mgf_batch) -> i64;",
                "pub fn mgf_batch_get_slider_trace(b: *mut mgf_batch, out: *mut c_void, row0: i64, n_rows: i64) -> mgf_status;",
                "pub fn mgf_batch_get_slider_trace_dev(b: *mut mgf_batch, out_dev: *mut c_void, row0: i64, n_rows: i64) -> mgf_status;",
                "pub struct mgf_slider_reading { pub d: f32, pub rate: f32, pub side: f32, pub off1: f32, pub off2: f32, pub e: mgf_vec3 }",
                "pub fn read_sliders(", "pub unsafe fn read_sliders_dev(", "pub fn set_slider_trace(", "pub fn slider_trace_rows(", "pub fn slider_trace(",
                "pub unsafe fn slider_trace_dev("):
        assert sig in flat, sig
    kernels = read("mgf_amd", "csrc", "kernels.h")
    assert kernels.index('#include "k_batch_slider.h"') < kernels.index('#include "k_batch_slider_read.h"')
    assert "k_batch_read_sliders<GATED, FORMAT> (k_batch_slider_read.h" in kernels
    hip = read("mgf_amd", "csrc", "mgf_hip.hip")
    assert hip.index('#include "host_batch_slider.inc"') < hip.index('#include "%s"' % READ_FILE)
    design = read("DESIGN.md")
    assert design.index("### Sliders between bodies") < design.index("### Slider encoders") < design.index("### Rollout touch traces")
    sub = design[design.index("### Slider encoders"):design.index("### Rollout touch traces")]
    for word in ("k_batch_read_sliders", "done[k] == t + 1 && act[k] <= t + 1", "The reading", "One launch", "The readings table", "The gate", "Checks", "Compiler output",
                 "Tests", "Measured", "Not measured", "Out of scope", "batch_slider_read_bench.py", "MGF_BATCH_SLIDER_READ_LAUNCHES",
                 "MGF_BATCH_ROLLOUT_SLIDER_READ_LAUNCHES_PER_TICK", "bench.py", "sliders.acc", "check_lane_masks.py", "16 EPS arms + 20 EPS P", "16 EPS arms + 50 EPS P", "64 EPS", "20 EPS V + (72 arms + 32 P) EPS W"):
        assert word in sub, word
    assert "since: Slider encoders, below" in design[design.index("### Sliders between bodies"):design.index("### Slider encoders")]
    readme = read("README.md")
    assert "read_sliders" in readme and "set_slider_trace" in readme
    assert os.path.exists(os.path.join(ROOT, "tools", "batch_slider_read_bench.py"))


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def test_what_needs_no_device_is_refused_in_the_headers_order():
    lib = mgf_amd.load_library()
    INV = _capi.ERR_INVALID

    def err():
        return lib.mgf_last_error().decode()
    fake = C.c_void_p(16)   # a handle that is never dereferenced
    out = C.c_void_p(1 << 21)
    assert lib.mgf_batch_slider_trace_rows(None) == -1
    for fn in (lib.mgf_batch_read_sliders, lib.mgf_batch_read_sliders_dev):
        assert fn(None, out) == INV and "NULL" in err()
        assert fn(None, None) == INV and "batch is NULL" in err()                            # the handle first
    assert lib.mgf_batch_set_slider_trace(None, 4, 0) == INV and "batch is NULL" in err()
    assert lib.mgf_batch_set_slider_trace(None, -1, 7) == INV and "batch is NULL" in err()     # the handle first
    for rows in (-1, (1 << 20) + 1, -(1 << 40)):
        assert lib.mgf_batch_set_slider_trace(fake, rows, 7) == INV and "rows must be in [0, 2^20]" in err(), rows   # rows ahead of the format
    for fmt in (-1, 2, 7):
        assert lib.mgf_batch_set_slider_trace(fake, 4, fmt) == INV and "format is neither" in err(), fmt
    for fn in (lib.mgf_batch_get_slider_trace, lib.mgf_batch_get_slider_trace_dev):
        assert fn(None, out, 0, 1) == INV and "batch is NULL" in err()
        assert fn(None, None, -1, -1) == INV and "batch is NULL" in err()                     # the handle first
        assert fn(fake, out, -1, -1) == INV and "row0 is negative" in err()                   # row0 ahead of n_rows
        assert fn(fake, out, 0, -1) == INV and "n_rows is negative" in err()
    # (the order of refusals, context, pointer look-up and first enqueue inside every call: tests/test_world_batch_encoder_family_host.py)
    # mgf_batch_set_sliders turns the trace off, with no device work
    rig = read("mgf_amd", "csrc", "host_batch_slider.inc")
    body = rig[rig.index('extern "C" mgf_status mgf_batch_set_sliders('):rig.index('extern "C" int64_t mgf_batch_slider_count(')]
    assert body.index("batch_joint_plan(b->sliders, j, n);") < body.index("b->slider_trace.rows = 0;") and not re.search(r"<<<|Async|hipMalloc|hipFree|\.ensure\(", body)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def _seeded():
    lens = list(LC.LENGTHS)
    st = LC.synthetic_state(lens)
    rig, planted, W = LC.main_rig(lens, st)
    return lens, st, rig, planted, W


def _live(rig):
    """the sliders of the seeded rig whose arm is not the planted 3e38, which overflows every word in f32"""
    return np.flatnonzero(np.abs(rig["pb"]).max(axis=1) < 1.0e30)


def test_the_f32_reading_holds_against_the_float64_one_within_the_bounds_of_its_rounded_operations():
    """Every slider of the seeded rig (tests/batch_slider_cases.py: main_rig on synthetic_state, 277 sliders, other's frame up to 0.1 rad
    and 0.05 length units off; the one whose arm is 3e38 left out) and of small_rig(257) read in f32 and in float64.  The bounds are
    tests/batch_slider_read_cases.py's, derived there from the rounded operations between the state and each word, in the lengths
    arms = |pa| + |pb|, P = |Pa| + |Pb|, V = |v_a| + |v_b| and W = |omega_a| + |omega_b|: 16 EPS arms + 20 EPS P on d, 16 EPS arms +
    50 EPS P on off1 and off2, 64 EPS on a component of e, 20 EPS V + (72 arms + 32 P) EPS W on the rate.  Measured here on the CPU, the
    largest difference as a share of its bound: d 0.019 (9.4e-7), off 0.015 (1.3e-6), e 0.023 (1.7e-7 = 1.44 EPS), rate 0.0055
    (9.3e-6) - the roundings never all pull the same way."""
    lens, st, rig, planted, W = _seeded()
    assert len(rig) == 21 + LC.MAX
    main = rig[_live(rig)]
    small, cases = SR.small_rig(lens, st, 257, worlds=(LC.CHAIN, LC.FULL))
    assert len(main) == len(rig) - 1
    assert SR.D_ARMS == 16 * SR.EPS and SR.D_P == 20 * SR.EPS and SR.OFF_ARMS == 16 * SR.EPS and SR.OFF_P == 50 * SR.EPS and SR.E_BOUND == 64 * SR.EPS
    assert SR.RATE_V == 20 * SR.EPS and SR.RATE_W_ARMS == 72 * SR.EPS and SR.RATE_W_P == 32 * SR.EPS
    for name, R in (("main_rig", main), ("small_rig", small)):
        r32 = SR.readings(R, st, lens, f32)
        r64 = SR.readings(R, st, lens, np.float64)
        assert r32.dtype == f32 and r64.dtype == np.float64 and np.all(np.isfinite(r32))
        bd, bo, be, br = SR.bounds(R, st, lens)
        diff = np.abs(r32 - r64)
        d_e = diff[:, 5:8].max(axis=1)
        d_off = diff[:, 3:5].max(axis=1)
        print("%s, f32 against f64 over %d sliders: largest |dd| %.3g (%.3g of its bound), |doff| %.3g (%.3g), |de| %.3g = %.2f EPS (%.3g), |drate| %.3g (%.3g)"
              % (name, len(R), diff[:, 0].max(), (diff[:, 0] / bd).max(), d_off.max(), (d_off / bo).max(), d_e.max(), d_e.max() / SR.EPS, (d_e / be).max(),
                 diff[:, 1].max(), (diff[:, 1] / br).max()))
        assert np.all(diff[:, 0] <= bd) and np.all(d_off <= bo) and np.all(d_e <= be) and np.all(diff[:, 1] <= br)
        assert np.all(bd < 1e-3) and np.all(br < 0.05)                                  # the bounds say something at these lengths
        # the float64 reading is the geometry: tests/batch_slider_cases.py's travel, written independently - it adds x + delta in float64
        # where the state's own sum is f32: half an ulp of a coordinate below 16, 4.8e-7, on both anchors, through a dot product with a
        # unit vector: 2 sqrt(3) 4.8e-7 = 1.7e-6
        d64, off64, e64 = LC.travel(R, st, lens)
        assert np.abs(st["x"]).max() < 16.0
        assert np.allclose(r64[:, 0], d64, rtol=0, atol=1.7e-6) and np.allclose(np.hypot(r64[:, 3], r64[:, 4]), off64, rtol=0, atol=2 * 1.7e-6)
        assert np.allclose(np.linalg.norm(r64[:, 5:8], axis=1), e64, rtol=0, atol=1e-9)
        assert off64.max() > 0.01 and e64.max() > 0.01 and np.ptp(r64[:, 1]) > 1.0       # every word is live


def test_the_words_are_the_setups_by_bytes_and_the_rate_is_the_solves_first_motor_row_rate():
    lens, st, rig, planted, W = _seeded()
    h = f32(1.0 / 60.0)
    for ft in (f32, np.float64):
        r, mid = SR.readings(rig, st, lens, ft, parts=True)
        S = LC.setup(rig, h, W[0], st, lens, ft)
        live = _live(rig) if ft == f32 else range(len(rig))
        for i in live:
            s = S[i]
            assert r[i, 0].tobytes() == s["d"].tobytes() and float(r[i, 2]) == float(s["side"]), i
            assert r[i, 5:8].tobytes() == s["e"].tobytes(), i
            assert r[i, 3].tobytes() == LC._dot(s["C"], s["T1"]).tobytes() and r[i, 4].tobytes() == LC._dot(s["C"], s["T2"]).tobytes(), i
            assert mid["sA"][i].tobytes() == s["sA"].tobytes() and mid["sB"][i].tobytes() == s["sB"].tobytes() and mid["C"][i].tobytes() == s["C"].tobytes(), i
        # the rate: what the first motor row of a solve of that slider, from that state, hands to its division - taken from the solve
        # itself, whose rate() is three dot products and two sums: the first three calls of _dot behind the setup
        motors = [i for i in live if S[i]["motor"] and not S[i]["skip"]]
        assert len(motors) > 50
        seen = []
        real = LC._dot

        def spy(a, b):
            out = real(a, b)
            seen.append(out)
            return out
        LC._dot = spy
        try:
            for i in motors:
                del seen[:]
                v, om = st["v"].astype(ft).copy(), st["omega"].astype(ft).copy()
                LC._solve_one(S[i], v, om, np.zeros((len(rig), 8), ft), i, ft)
                first = (seen[0] + seen[1]) - seen[2]
                assert first.dtype == ft and r[i, 1].tobytes() == first.tobytes(), i
        finally:
            LC._dot = real
        # ... and of every other slider the same expression over the setup's words
        zero = np.zeros(3, ft)
        v, om = st["v"].astype(ft), st["omega"].astype(ft)
        for i in live:
            s = S[i]
            vb, ob = (v[s["gb"]], om[s["gb"]]) if s["gb"] >= 0 else (zero, zero)
            want = (LC._dot(vb - v[s["ga"]], s["A"]) + LC._dot(ob, s["sB"])) - LC._dot(om[s["ga"]], s["sA"])
            assert r[i, 1].tobytes() == want.tobytes(), i


def test_every_case_and_both_far_ends_are_present_and_side_says_which_axis_row_the_next_solve_turns_on():
    lens, st, rig, planted, W = _seeded()
    small, cases = SR.small_rig(lens, st, 257, worlds=(LC.CHAIN, LC.FULL))
    assert set(cases) == set(range(len(SR.CASES))) and len(SR.CASES) == 7
    assert np.bincount(small["world"], minlength=len(lens)).max() <= LC.MAX and np.any(small["other"] == -1) and np.any(small["other"] >= 0)
    for c in range(len(SR.CASES)):                                                   # every case on both kinds of far end
        assert {bool(o >= 0) for o in small["other"][cases == c]} == {True, False}, SR.CASES[c]
    s = SR.readings(small, st, lens)[:, 2]
    assert [float(x) for x in s] == [SR.SIDE_OF[SR.CASES[c]] for c in cases]
    point = cases == SR.CASES.index("limit_point")
    assert np.all(small["flags"][point] == LC.LIMIT) and np.array_equal(small["lo"][point], small["hi"][point])
    assert np.array_equal(small["lo"][point], SR.readings(small, st, lens)[point, 0])          # lo == hi == d to the bit: neither comparison holds
    assert np.all(small["flags"][cases == SR.CASES.index("both_above")] == (LC.LIMIT | LC.MOTOR)) and np.all(small["flags"][cases == SR.CASES.index("lock")] == LC.LOCK)
    # the main rig's own cases
    names = np.array(LC.CASES)[np.arange(len(rig)) % len(LC.CASES)]
    side = SR.readings(rig, st, lens)[:, 2]
    live = np.zeros(len(rig), bool)
    live[_live(rig)] = True
    for name, want in (("none", 0.0), ("limit_inside", 0.0), ("limit_below", -1.0), ("limit_above", 1.0), ("motor_free", 0.0), ("both", 1.0), ("lock", 2.0)):
        assert set(side[(names == name) & live]) == {want}, name
    # non-finite state gives non-finite words; the comparisons fail, so a limit says 0 and a lock still says 2
    bad = {k: a.copy() for k, a in st.items()}
    off = np.concatenate([[0], np.cumsum(lens)])
    for i in (int(np.flatnonzero(cases == 2)[0]), int(np.flatnonzero(cases == 5)[0])):
        bad["q"][int(off[small["world"][i]] + small["body"][i])] = np.nan
        r = SR.readings(small[i:i + 1], bad, lens)
        assert np.isnan(r[0, [0, 1, 3, 4, 5, 6, 7]]).all() and r[0, 2] == (2.0 if cases[i] == 5 else 0.0)


def test_the_lifts_travel_stays_clear_of_its_limits():
    """The use case of the GPU test leaves a tick out of its `side` check where the lift's float64 d is within the d bound of a limit: at
    most 2 of LC.LIFT_TICKS ticks.  The float64 restatement of the lift on the CPU leaves none out - the nearest tick is 0.0157 from hi
    - with 48 ticks above hi, 16 inside and none below lo."""
    d, rate, gap, tilt = LC.lift_sim(True)
    lo, hi = LC.LIFT_LIMIT
    near = np.minimum(np.abs(d - lo), np.abs(d - hi))
    bound = SR.D_ARMS * 1.0 + SR.D_P * 30.0                                           # arms below 1, the anchors 12 above the origin each
    print("the lift on the CPU: the tick nearest a limit is", float(near.min()), "from it; bound", bound, "; above hi", int((d > hi).sum()), "inside",
          int(((d >= lo) & (d <= hi)).sum()), "below lo", int((d < lo).sum()))
    assert len(d) == LC.LIFT_TICKS == 64 and int((near <= bound).sum()) == 0 and 0.015 < near.min() < 0.016
    assert int((d > hi).sum()) == 48 and int(((d >= lo) & (d <= hi)).sum()) == 16 and not np.any(d < lo)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_sliders_reading_holds_the_sliders_own_lines_and_its_two_loads_of_v():
    """The lane's walk, its gate ahead of every load and the stores are the skeleton's (k_batch_joint_read.h), asserted in
    tests/test_world_batch_encoder_family_host.py; here: what SliderReading forms of the ends and the frames, one f32 operation a line."""
    k = read("mgf_amd", "csrc", "k_batch_slider_read.h")
    body = k[k.index("struct SliderReading {"):k.index("template <bool GATED, int FORMAT>")]
    assert "template <bool GATED, int FORMAT>" in k and "void k_batch_read_sliders(" in k
    assert not re.search(r"atomic|__shared__|__syncthreads|s_dyn|A\.plan|A\.slots|A\.items| / |A\.h\b", body)    # no plan, no LDS, no atomic, no barrier, no division, no h
    assert not re.search(r"A\.B\.\w+\[[^\]]*\] =[^=]|srec\[[^\]]*\] =[^=]", k)                                   # nothing written but the output
    assert "rotate(" not in body and "slider_rate(own.va, a.om, own.vb, b.om, F.A, sA, sB)" in body and "srec[" not in body
    assert "__device__ __forceinline__ V3 slider_read_v(const Bodies& B, size_t g) { return xyz(B.srec[4 * g]); }" in k        # v: srec word 0's xyz
    for line in ("const uint32_t flags = f2u(w0.w);", "o.va = slider_read_v(B, g0 + f2u(w0.y));", "o.vb = mk3(0.0f, 0.0f, 0.0f);", "if (has_b) o.vb = slider_read_v(B, g0 + f2u(w0.z));",
                 "const V3 U2 = cross(F.B, F.U1);", "const V3 ca = F.ra + F.C;", "const V3 sA = cross(ca, F.A);", "const V3 sB = cross(F.rb, F.A);", "const float d = dot(F.C, F.A);",
                 "const float off1 = dot(F.C, F.T1), off2 = dot(F.C, F.T2);", "const V3 e = ((cross(F.A, F.B) + cross(F.T1, F.U1)) + cross(F.T2, U2)) * 0.5f;",
                 "if ((flags & kSliderLock) != 0u) side = 2.0f;", "else if ((flags & kSliderLimit) != 0u && d < w3.w) side = -1.0f;",
                 "else if ((flags & kSliderLimit) != 0u && d > w4.w) side = 1.0f;", "return {make_float4(d, rate, side, off1), make_float4(off2, e.x, e.y, e.z)};"):
        assert line in body, line
    code = k[k.index("#pragma once"):]
    assert not re.search(r"k_batch_slider\w*<|k_batch_joint\w*<|void k_batch_slider|void k_batch_joint", code)      # (the solvers' kernels are selected by those substrings)
    assert '#include "k_batch_slider.h"' in k and "struct JointEnd {\n  Quat q;\n  V3 x, om;\n  float im;\n  M3 I;\n};" in read("mgf_amd", "csrc", "k_batch_joint_loop.h")


def test_the_new_kernel_uses_no_scratch_and_spills_nothing_and_the_other_kernels_are_as_they_were():
    if not os.path.exists(os.path.join(ROOT, "mgf_amd", "libmgf_hip.so")) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    rows = kernel_resources("k_batch_read_sliders")
    assert set(rows) == {"k_batch_read_sliders<false, 0>", "k_batch_read_sliders<true, 0>", "k_batch_read_sliders<true, 1>", "k_batch_read_sliders<true, 2>"}, sorted(rows)
    solve = kernel_resources("k_batch_slider")
    assert set(solve) == {"k_batch_slider_solve<false>", "k_batch_slider_solve<true>"}, sorted(solve)      # (tests/test_world_batch_sliders_host.py selects them by this substring)
    design = re.sub(r"\s+", " ", read("DESIGN.md"))
    for name, v in sorted(rows.items()):
        print(name, ": vgpr, sgpr, scratch, static lds, sgpr spills, vgpr spills =", v)
        assert v[2] == "0" and v[3] == "0" and v[4] == "0" and v[5] == "0", (name, v)    # no scratch, no LDS, no spills
        assert int(v[0]) < min(int(s[0]) for s in solve.values()), (name, v)              # fewer than the solve's
        assert "`%s` %s / %s / 0 / 0 / 0" % (name, v[0], v[1]) in design, (name, v)
    # the solvers' and the hinge encoders' kernels are what their own tests expect of them: untouched
    assert solve == {"k_batch_slider_solve<false>": ("118", "69", "0", "16", "0", "0"), "k_batch_slider_solve<true>": ("118", "69", "0", "16", "0", "0")}, solve
    old = kernel_resources("k_batch_hinge")
    assert old == {"k_batch_hinge_solve<false>": ("103", "55", "0", "16", "0", "0"), "k_batch_hinge_solve<true>": ("103", "55", "0", "16", "0", "0")}, old
    old = kernel_resources("k_batch_joint")
    assert old == {"k_batch_joint_solve<false>": ("78", "51", "0", "16", "0", "0"), "k_batch_joint_solve<true>": ("78", "51", "0", "16", "0", "0")}, old
    old = kernel_resources("k_batch_read_hinges")
    assert len(old) == 4
    for name, v in old.items():
        assert "`%s` %s / %s / 0 / 0 / 0" % (name, v[0], v[1]) in design, (name, v)        # the line the hinge encoders' section carries


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_binding_shapes_its_arrays_and_turns_a_wrong_tensor_down_before_it_calls_c():
    import torch

    class Handle(mgf_amd.WorldBatch):   # no context, no C handle: a call that got as far as C would fail differently
        def __init__(self, n, rows):
            self._h, self._n, self._rows = None, n, rows

        def slider_count(self):
            return self._n

        def slider_trace_rows(self):
            return self._rows

        def close(self):
            pass
    b = Handle(5, 4)
    with pytest.raises(ValueError, match="on cpu"):
        b.read_sliders_dev(torch.zeros((5, 8), dtype=torch.float32))
    with pytest.raises(ValueError, match="5 rows of 8"):
        b.read_sliders_dev(torch.zeros((5, 7), dtype=torch.float32))
    with pytest.raises(ValueError, match="5 rows of 8"):
        b.read_sliders_dev(torch.zeros((4, 8), dtype=torch.float32))
    with pytest.raises(ValueError, match="dtype"):
        b.read_sliders_dev(torch.zeros((5, 8), dtype=torch.float64))
    with pytest.raises(ValueError):
        b.read_sliders_dev(torch.zeros((8, 5), dtype=torch.float32).t())               # not contiguous
    with pytest.raises(ValueError, match="rows of a table of 4"):
        b.slider_trace(2, 3)
    with pytest.raises(ValueError, match="rows of a table of 4"):
        b.slider_trace(-1)
    with pytest.raises(ValueError, match="10 rows of 8"):
        b.slider_trace_dev(torch.zeros((15, 8), dtype=torch.float32), 1, 2)
    b._slider_trace_full = True
    with pytest.raises(ValueError, match="10 rows of 16"):
        b.slider_trace_dev(torch.zeros((10, 8), dtype=torch.float32), 1, 2)
    with pytest.raises(mgf_amd.MgfError):                                              # and a call whose arguments are all in order does reach C
        b.read_sliders_dev(1 << 21)
    r = np.zeros((2, 3), _capi.SLIDER_TRACE_FULL_DTYPE)
    assert SR.words(r).shape == (2, 3, 16) and SR.as_readings(np.zeros((4, 8), f32)).dtype == _capi.SLIDER_READING_DTYPE
