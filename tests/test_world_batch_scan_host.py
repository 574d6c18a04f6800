"""The sensor trace of a rollout (mgf_batch_rollout_observe, mgf_batch_rollout_observe_dev) without a GPU: the header, the library, the
binding and the documents carry the calls, the struct and the constants; what needs no handle is refused on a handle that is never
dereferenced, in the header's order; the device form looks every pointer up and holds the outputs against each other and the inputs
before it enqueues anything; the binding turns a wrong tensor down before it calls C; the kernels are the two the header names, the ray
front is not restated and the parents' kernels are still exactly theirs; and the late-contact rig of tests/batch_scan_cases.py does, by
the oracle, what tests/test_gpu_world_batch_scan.py needs of it."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mgf_amd
from mgf_amd import _capi
from tests import batch_rollout_cases as RC
from tests import batch_scan_cases as YC
from tests.test_world_batch_trace_host import _Fake
from tests.util import ROOT, kernel_resources, read

CALLS = ("mgf_batch_rollout_observe", "mgf_batch_rollout_observe_dev")
HOST_FILE = "host_batch_scan.inc"


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
def test_header_library_binding_and_documents_carry_the_calls():
    h = read("include", "mgf_hip.h")
    flat_h = re.sub(r"\s+", " ", h)
    for sig in ("MGF_API mgf_status mgf_batch_rollout_observe(mgf_batch* b, float dt, int32_t iters, int64_t n_ticks, const float* u, int64_t n_act, int32_t mode, "
                "const int32_t* body, int64_t m, float* x, float* q, float* v, float* omega, const mgf_rollout_traces* traces, mgf_step_stats* stats);",
                "MGF_API mgf_status mgf_batch_rollout_observe_dev(mgf_batch* b, float dt, int32_t iters, int64_t n_ticks, const float* u_dev, int64_t n_act, "
                "int32_t mode, const int32_t* body_dev, int64_t m, float* x_dev, float* q_dev, float* v_dev, float* omega_dev, const mgf_rollout_traces* traces, "
                "mgf_step_stats* stats);",
                "typedef void* mgf_trace_rows;", "typedef struct mgf_rollout_traces { /* 64 bytes */ mgf_trace_rows touch; int64_t n_touch;", "mgf_trace_rows sensor; int64_t n_sensor;",
                "int32_t touch_format, sensor_format, sensor_mask;", "int32_t reserved[5]; /* must be 0 */ } mgf_rollout_traces;"):
        assert sig in flat_h, sig
    # a section of its own, behind the touch traces' and ahead of the counters' comment
    assert (h.index("/* ---- rollout touch traces") < h.index("mgf_batch_rollout_touches_dev(mgf_batch*") < h.index("/* ---- rollout sensor traces")
            < h.index("#define MGF_ROLLOUT_SENSOR_HIT") < h.index("MGF_API mgf_status mgf_batch_rollout_observe(") < h.index("/* name in {") < h.index("mgf_batch_counter(const"))
    for name, value in (("MGF_ROLLOUT_SENSOR_HIT", _capi.ROLLOUT_SENSOR_HIT), ("MGF_ROLLOUT_SENSOR_DEPTH", _capi.ROLLOUT_SENSOR_DEPTH),
                        ("MGF_BATCH_ROLLOUT_SENSOR_LAUNCHES_PER_TICK", _capi.BATCH_ROLLOUT_SENSOR_LAUNCHES_PER_TICK)):
        m = re.search(r"#define %s\s+(\d+)" % name, h)
        assert m and int(m.group(1)) == value, name
        assert getattr(mgf_amd, name[4:]) == value, name
    assert (_capi.ROLLOUT_SENSOR_HIT, _capi.ROLLOUT_SENSOR_DEPTH, _capi.BATCH_ROLLOUT_SENSOR_LAUNCHES_PER_TICK) == (0, 1, 2)
    S = _capi.ROLLOUT_TRACES
    assert mgf_amd.ROLLOUT_TRACES is S and C.sizeof(S) == 64
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("touch", 0), ("n_touch", 8), ("sensor", 16), ("n_sensor", 24), ("touch_format", 32),
                                                                   ("sensor_format", 36), ("sensor_mask", 40), ("reserved", 44)]
    section = re.sub(r"\s*\n \* ", " ", h[h.index("/* ---- rollout sensor traces"):h.index("/* name in {")])
    for word in ("bit for bit", "mgf_batch_apply_springs_dev(b, dt, NULL)", "mgf_batch_actuate_dev(b, u[t], n_act, mode, NULL)",
                 "mgf_batch_step(b, dt, iters, 1, stats + t * n_worlds)", "mgf_batch_gather_state_dev(b, body, m, x[t], q[t], v[t], omega[t], NULL, NULL)",
                 "mgf_batch_read_touches_dev(b, touch + t * n_touch, n_touch)", "mgf_batch_cast_sensors_dev(b, sensor_mask, hits_row_t, NULL, n_sensor)",
                 "EVERY entry of every row is written", "the sensor's dt where nothing is hit", "several components", "launch for launch", "byte for byte",
                 "ONE HOST WAIT", "NO COLLIDER GATHER", "rollout_launches", "query_launches", "nothing enqueued", "overflows int64_t", "OUT OF SCOPE",
                 "feelers, zones and cameras per tick", "the particles per tick", "a kinds mask per sensor", "lone mgf_world", "hipGraph"):
        assert word in section, word
    # the note of the parent: the old words stand, with a "since"
    touch = flat_h[flat_h.index("/* ---- rollout touch traces"):flat_h.index("#define MGF_ROLLOUT_TOUCH_FULL")]
    assert re.search(r"ray sensors, feelers, zones or cameras per tick \(they need the collider gather in the train\) \(since: Rollout sensor traces", touch)
    counters = flat_h[flat_h.index("/* name in {"):]
    assert re.search(r'"rollout_launches" \(.*_rollout_observe.*sensor trace', counters)
    lib = mgf_amd.load_library()
    vp, i64, i32, f32 = C.c_void_p, C.c_int64, C.c_int32, C.c_float
    for name in CALLS:
        assert name in _capi.SYMBOLS, name
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (i32, [vp, f32, i32, i64, vp, i64, i32, vp, i64, vp, vp, vp, vp, C.POINTER(S), vp]), name
    for method in ("rollout_observe", "rollout_observe_dev"):
        assert callable(getattr(mgf_amd.WorldBatch, method)), method
    flat = re.sub(r"\s+", " ", read("INTEGRATION.md"))
    for sig in ("pub fn mgf_batch_rollout_observe(b: *mut mgf_batch, dt: f32, iters: i32, n_ticks: i64, u: *const f32, n_act: i64, mode: i32, body: *const i32, "
                "m: i64, x: *mut f32, q: *mut f32, v: *mut f32, omega: *mut f32, traces: *const mgf_rollout_traces, stats: *mut mgf_step_stats) -> mgf_status;",
                "pub fn mgf_batch_rollout_observe_dev(b: *mut mgf_batch, dt: f32, iters: i32, n_ticks: i64, u_dev: *const f32, n_act: i64, mode: i32, "
                "body_dev: *const i32, m: i64, x_dev: *mut f32, q_dev: *mut f32, v_dev: *mut f32, omega_dev: *mut f32, traces: *const mgf_rollout_traces, "
                "stats: *mut mgf_step_stats) -> mgf_status;",
                "pub const MGF_ROLLOUT_SENSOR_HIT: i32 = 0;", "pub const MGF_ROLLOUT_SENSOR_DEPTH: i32 = 1;",
                "pub const MGF_BATCH_ROLLOUT_SENSOR_LAUNCHES_PER_TICK: i64 = 2;",
                "pub type mgf_trace_rows = *mut c_void;",
                "pub struct mgf_rollout_traces { pub touch: mgf_trace_rows, pub n_touch: i64, pub sensor: mgf_trace_rows, pub n_sensor: i64, pub touch_format: i32, "
                "pub sensor_format: i32, pub sensor_mask: i32, pub reserved: [i32; 5] }",
                "pub fn rollout_observe(", "pub unsafe fn rollout_observe_dev("):
        assert sig in flat, sig
    kernels = read("mgf_amd", "csrc", "kernels.h")
    assert kernels.index('#include "k_batch_trace.h"') < kernels.index('#include "k_batch_scan.h"') and "k_batch_scan_rays / k_batch_scan_rows<FORMAT> (k_batch_scan.h)" in kernels
    hip = read("mgf_amd", "csrc", "mgf_hip.hip")
    assert hip.index('#include "host_batch_trace.inc"') < hip.index('#include "%s"' % HOST_FILE)
    design = read("DESIGN.md")
    assert design.index("## Rollout touch traces") < design.index("## Rollout sensor traces") < design.index("## 9.")
    between = design[design.index("## Rollout touch traces"):design.index("## Rollout sensor traces")]
    assert between.count("\n##") == 0                                                                    # directly behind it
    sub = design[design.index("## Rollout sensor traces"):design.index("## 9.")]
    for word in ("k_batch_scan_rays", "k_batch_scan_rows", "Definition", "Why no gather", "bpk", "TickUndo", "The gate", "done[k] == t + 1 && act[k] <= t + 1",
                 "Why the front is ungated", "Launches", "Checks", "Compiler output", "Tests", "Measured", "Out of scope", "batch_rollout_sensor_bench.py",
                 "MGF_BATCH_ROLLOUT_SENSOR_LAUNCHES_PER_TICK", "MGF_SCAN_GATE", "hipGraph"):
        assert word in sub, word
    readme = read("README.md")
    assert "rollout_observe(" in readme and "rollout_observe_dev" in readme and "batch_rollout_sensor_bench.py" in readme
    assert os.path.exists(os.path.join(ROOT, "tools", "batch_rollout_sensor_bench.py"))


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def test_what_needs_no_handle_is_refused_before_the_handle_is_dereferenced_in_the_headers_order():
    lib = mgf_amd.load_library()
    INV = _capi.ERR_INVALID

    def err():
        return lib.mgf_last_error().decode()
    fake = C.c_void_p(16)   # a handle that is never dereferenced; addresses that are never looked up
    p = [C.c_void_p((k + 1) << 20) for k in range(9)]
    u, body, x, q, v, om, st, touch, sensor = p
    dt = C.c_float(1.0 / 60.0)
    big = 1 << 62
    for fn in (lib.mgf_batch_rollout_observe, lib.mgf_batch_rollout_observe_dev):
        def call(h, iters=4, n_ticks=3, n_act=5, mode=0, m=6, n_touch=7, tfmt=0, n_sensor=8, sfmt=0, mask=7, reserved=0, word=0, traces=True):
            tr = _capi.ROLLOUT_TRACES()
            tr.touch, tr.n_touch, tr.touch_format = touch, n_touch, tfmt
            tr.sensor, tr.n_sensor, tr.sensor_format, tr.sensor_mask = sensor, n_sensor, sfmt, mask
            tr.reserved[word] = reserved
            return fn(h, dt, iters, n_ticks, u, n_act, mode, body, m, x, q, v, om, C.byref(tr) if traces else None, st)
        bad = dict(tfmt=9, sfmt=9, mask=8, reserved=1)
        assert call(None) == INV and "NULL" in err()
        assert call(None, iters=-1, n_ticks=-1, n_act=-1, mode=9, m=-1, n_touch=-1, n_sensor=-1, **bad) == INV and "NULL" in err()   # the handle first, whatever the rest
        assert call(fake, n_ticks=-1, iters=-1, n_act=-1, m=-1, n_touch=-1, n_sensor=-1, mode=9, **bad) == INV and "n_ticks is negative" in err()
        assert call(fake, iters=-1, n_act=-1, m=-1, n_touch=-1, n_sensor=-1, mode=9, **bad) == INV and "iters is negative" in err()
        assert call(fake, n_act=-1, m=-1, n_touch=-1, n_sensor=-1, mode=9, n_ticks=1 << 30, **bad) == INV and "n_act is negative" in err()
        assert call(fake, m=-(1 << 40), n_touch=-1, n_sensor=-1, mode=9, n_ticks=1 << 30, **bad) == INV and "m is negative" in err()
        assert call(fake, n_touch=-(1 << 40), n_sensor=-1, mode=9, n_ticks=1 << 30, **bad) == INV and "n_touch is negative" in err()
        assert call(fake, n_sensor=-(1 << 40), mode=9, n_ticks=1 << 30, **bad) == INV and "n_sensor is negative" in err()
        assert call(fake, n_ticks=(1 << 20) + 1, mode=9, m=1 << 31, **bad) == INV and "2^20" in err()
        for mode in (2, -1, 1 << 20):
            assert call(fake, mode=mode, m=1 << 31, **bad) == INV and "mode" in err(), mode
        assert call(fake, m=1 << 31, **bad) == INV and "touch_format" in err()
        for sfmt in (2, -1, 64, 1 << 20):
            assert call(fake, sfmt=sfmt, mask=8, reserved=1, m=1 << 31, n_sensor=big) == INV and "sensor_format" in err(), sfmt
            assert call(fake, sfmt=sfmt, n_ticks=0, n_act=0, m=0, n_touch=0, n_sensor=0) == INV and "sensor_format" in err(), sfmt
        for mask in (0, 8, -1, 1 << 20):
            assert call(fake, mask=mask, reserved=1, m=1 << 31) == INV and "kinds_mask" in err(), mask
        for word in range(5):
            assert call(fake, reserved=1 << (6 * word), word=word, m=1 << 31) == INV and "reserved word" in err(), word
        assert call(fake, reserved=-1, n_sensor=0, n_touch=0, n_ticks=0, n_act=0, m=0) == INV and "reserved word" in err()   # with no trace named too
        assert call(fake, m=1 << 31, n_act=big, n_touch=big, n_sensor=big) == INV and "too many traced" in err()
        assert call(fake, n_ticks=1 << 20, n_act=big, n_touch=big, n_sensor=big) == INV and "4 * n_ticks * n_act overflows int64_t" in err()
        assert call(fake, n_ticks=1 << 20, n_act=0, n_touch=big, n_sensor=big) == INV and "64 * n_ticks * n_touch overflows int64_t" in err()
        for sfmt in (0, 1):                                                      # the bound is the full record's, whatever the format
            assert call(fake, n_ticks=1 << 20, n_act=0, n_touch=0, n_sensor=big, sfmt=sfmt) == INV and "28 * n_ticks * n_sensor overflows int64_t" in err()
            assert call(fake, n_ticks=2, n_act=0, n_touch=0, n_sensor=1 << 58, sfmt=sfmt) == INV and "28 * n_ticks * n_sensor overflows int64_t" in err()
        # traces == NULL: mgf_batch_rollout's refusals
        assert call(fake, traces=False, mode=9) == INV and "mode" in err()
        assert call(fake, traces=False, n_ticks=1 << 20, n_act=big) == INV and "overflows int64_t" in err()
    # the order is the one the header states, and nothing of it touches a device
    src = read("mgf_amd", "csrc", HOST_FILE)
    mine = src[src.index("static mgf_status batch_scan_args("):src.index('extern "C" mgf_status mgf_batch_rollout_observe_dev(')]
    assert mine.index("batch_rollout_args(b, iters, n_ticks, u, n_act, mode, body, m, bytes, touch, scan)") < mine.index('batch_single_parts(b, "mgf_batch_rollout_observe')
    assert re.search(r"batch_single_parts\(b, [^;]*, false\)", mine)                # whatever "part_queries" says
    shared = read("mgf_amd", "csrc", "host_batch_rollout.inc")
    args = shared[shared.index("static mgf_status batch_rollout_args("):shared.index("static mgf_status batch_rollout_run(")]
    marks = ["batch_rig_handle(b)", '"n_ticks is negative"', '"iters is negative"', '"n_act is negative"', '"m is negative"', '"n_touch is negative"',
             '"n_sensor is negative"', '"n_ticks must be at most 2^20"', "mode != MGF_ACTUATE_IMPULSE && mode != MGF_ACTUATE_FORCE",
             "tt->format != MGF_ROLLOUT_TOUCH_FULL && tt->format != MGF_ROLLOUT_TOUCH_SHORT", "ts->format != MGF_ROLLOUT_SENSOR_HIT && ts->format != MGF_ROLLOUT_SENSOR_DEPTH",
             "query_mask_check(ts->mask)", "ts->reserved)", "m > (int64_t)INT32_MAX", '"4 * n_ticks * n_act overflows int64_t"',
             '"64 * n_ticks * n_touch overflows int64_t"', '"28 * n_ticks * n_sensor overflows int64_t"', "b->actuators.recs.size()", "b->touches.recs.size()",
             "b->sensors.recs.size()", "n_act > 0 && n_ticks > 0 && !u", "tt->n > 0 && n_ticks > 0 && !tt->out", "!body && m > mgf_batch_len(b, -1)"]
    order = [args.index(s) for s in marks]
    assert order == sorted(order), order
    assert args.index("n_sensor overflows int64_t") < args.index("b->")             # the handle's contents come last
    for text in (mine, args):
        assert not re.search(r"ctx_bind|<<<|Async|\.ensure\(|h2d\(|d2h\(", text)
    sec = re.sub(r"\s+", " ", re.sub(r"\s*\n \* ", " ", read("include", "mgf_hip.h")))
    sec = sec[sec.index("/* ---- rollout sensor traces"):]
    words = ["a NULL batch", "negative n_ticks, iters, n_act, m, n_touch or n_sensor", "n_ticks > 2^20", "a mode other than", "a touch_format other than",
             "a sensor_format other than", "a sensor_mask that a cast refuses", "a reserved word that is not 0", "m > INT32_MAX",
             "4 * n_ticks * n_act, then 64 * n_ticks * n_touch, then 28 * n_ticks * n_sensor", "n_act != mgf_batch_actuator_count(b)", "n_touch != mgf_batch_touch_count(b)",
             "n_sensor != mgf_batch_sensor_count(b)", "NULL u with n_act > 0 and n_ticks > 0", "body == NULL with m > mgf_batch_len(b, -1)",
             "a batch that holds bodies of several components"]
    at = [sec.index(w) for w in words]
    assert at == sorted(at), at
    for name in CALLS:
        f = src[src.index('extern "C" mgf_status %s(' % name):]
        assert f.index("batch_scan_args(") < f.index("ctx_bind(")


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_device_form_looks_every_pointer_up_before_the_first_enqueue():
    src = read("mgf_amd", "csrc", HOST_FILE)
    run = src[src.index('extern "C" mgf_status mgf_batch_rollout_observe_dev('):src.index('extern "C" mgf_status mgf_batch_rollout_observe(')]
    run = run[:run.index("\n}\n")]
    enqueue = r"batch_rollout_run\(|batch_step_run\(|batch_rig_up\(|batch_push\(|hipMemsetAsync|hipMemcpyAsync|<<<|\.ensure\(|h2d\(|d2h\("
    first_enqueue = min(m.start() for m in re.finditer(enqueue, run))
    checks = [m.start() for m in re.finditer(r"dev_span\(", run)]
    assert len(checks) == 8 and max(checks) < first_enqueue
    for name in ("u_dev, n.u", "body_dev, n.body", r"x_dev, n.out\[0\]", r"q_dev, n.out\[1\]", r"v_dev, n.out\[2\]", r"omega_dev, n.out\[3\]", "touch_dev, n.touch",
                 "sensor_dev, n.sensor"):
        assert re.search(r"dev_span\(b->ctx, " + name, run), name
    assert max(checks) < run.index("dev_outputs_overlap(arrays, 8, 6)") < first_enqueue               # six outputs, against each other and the two inputs
    assert run.index("batch_scan_args(") < run.index("ctx_bind(") < min(checks)
    assert "hipStreamSynchronize" not in run and "hipMemcpy" not in run                              # no copy of its own
    shared = read("mgf_amd", "csrc", "host_batch_rollout.inc")
    assert "bytes->sensor = ts && !ts->off() ? (ts->format == MGF_ROLLOUT_SENSOR_DEPTH ? 4u : 28u) * T * (size_t)ts->n : 0;" in shared
    # the host form: one upload, the device core, one download
    host_form = src[src.index('extern "C" mgf_status mgf_batch_rollout_observe('):]
    assert host_form.count("h2d(") == 1 and host_form.count("d2h(") == 1 and host_form.count("batch_rollout_run(") == 1
    assert host_form.index("h2d(") < host_form.index("batch_rollout_run(") < host_form.index("d2h(")
    for f in (HOST_FILE, "host_batch_rollout.inc", "host_batch_trace.inc"):
        text = read("mgf_amd", "csrc", f)
        assert "<<<" not in text and "d_launches" not in text and "q_launches" not in text and "cols_stale" not in text.replace("and cols_stale are not touched", ""), f
    # the core is the rollout's: the rig up and the scratch ahead of the train; the train launches the trace behind the touch trace's
    core = shared[shared.index("static mgf_status batch_rollout_run("):shared.index('extern "C" mgf_status mgf_batch_rollout_dev(')]
    assert (core.index("batch_push(") < core.index('batch_rig_up(b, b->sensors, "sensor", 4)') < core.index("b->q_out.ensure(7 * (size_t)ts->n, s)")
            < core.index("b->s_parts.ensure(7 * (size_t)ts->n, s)") < core.index("batch_step_run(b, dt, iters, n_ticks, stats, &H)"))
    host = read("mgf_amd", "csrc", "host_batch.inc")
    train = host[host.index("static mgf_status batch_step_run("):host.index('extern "C" mgf_status mgf_batch_step(')]
    assert train.count("k_batch_scan_rays<<<") == 1 and train.count("k_batch_scan_rows<") == 2
    assert train.index("k_batch_rollout_record<<<") < train.index("k_batch_trace_touch<") < train.index("k_batch_scan_rays<<<") < train.index("k_batch_scan_rows<")
    assert train.index("hook->launches += MGF_BATCH_ROLLOUT_SENSOR_LAUNCHES_PER_TICK;") > train.index("k_batch_scan_rows<kScanHit>")
    assert "batch_ray_lds(b), s>>>(hook->R, b->bpk.p)" in train and "k_batch_query_gather" not in train and "batch_cols_refresh" not in train
    scan = train[train.index("if (hook && hook->scan >= 0) {  // (behind the record"):]
    scan = scan[:scan.index("\n      }\n")]
    assert "q_launches" not in scan and "d_launches" not in scan and "cols_stale" not in scan
    passes = train[train.index("for (uint32_t first = 0"):]
    per_tick = passes.index("for (uint32_t t = first;")
    for word in ("V.rig = reinterpret_cast<const SensorIn*>", "V.x = b->dm[mgf_batch::AX].p;", "W.worlds = reinterpret_cast<const int32_t*>(R.dev.p + R.off[3]);",
                 "W.O = batch_obstacles(b);", "W.obstacles = batch_has_obstacles(b, V.mask)", "W.done = b->d_done.p;"):
        assert 0 < passes.index(word) < per_tick, word                                                 # inside the loop of passes, ahead of its ticks
    assert "static uint32_t batch_ray_lds(const mgf_batch* b);" in host[:host.index("static mgf_status batch_step_run(")]
    step = host[host.index('extern "C" mgf_status mgf_batch_step('):]
    assert "batch_step_run(b, dt, iters, n_ticks, stats, nullptr)" in step[:step.index("\n}\n")]


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_binding_turns_a_wrong_tensor_down_before_it_calls_c():
    import torch

    class Handle(mgf_amd.WorldBatch):   # no context, no C handle: a call that got as far as C would fail differently
        def __init__(self):
            self._h, self.n_worlds = None, 2

        def actuator_count(self):
            return 4

        def touch_count(self):
            return 6

        def sensor_count(self):
            return 5

        def __len__(self):
            return 10

    b, n, T, ns = Handle(), 4, 3, 5
    u = _Fake(torch.zeros((T, n), dtype=torch.float32))
    wrong = [torch.zeros((T, ns, 7), dtype=torch.float64), torch.zeros((T, ns, 7), dtype=torch.int64), torch.zeros((T, ns, 7), dtype=torch.int16),
             torch.zeros((T, ns, 8), dtype=torch.int32), torch.zeros((T, ns), dtype=torch.float32), torch.zeros((T + 1, ns, 7), dtype=torch.int32),
             torch.zeros((T, ns - 1, 7), dtype=torch.float32), torch.zeros((T * ns, 7), dtype=torch.int32), torch.zeros(T * ns * 7, dtype=torch.int32),
             torch.zeros((T, 7, ns), dtype=torch.int32).transpose(1, 2), torch.zeros((T, ns, 14), dtype=torch.float32)[:, :, ::2]]
    for t in wrong:
        with pytest.raises(ValueError) as e:
            b.rollout_observe_dev(u, 0.01, 4, sensors=t)
        assert "on cpu" not in str(e.value), str(e.value)              # turned down for what it is, not for where it is
    wrong = [torch.zeros((T, ns), dtype=torch.int32), torch.zeros((T, ns), dtype=torch.float64), torch.zeros((T, ns, 7), dtype=torch.float32),
             torch.zeros((T, ns, 1), dtype=torch.float32), torch.zeros((T + 1, ns), dtype=torch.float32), torch.zeros((ns, T), dtype=torch.float32).t(),
             torch.zeros(T * ns, dtype=torch.float32)]
    for t in wrong:
        with pytest.raises(ValueError) as e:
            b.rollout_observe_dev(u, 0.01, 4, sensors=t, depth=True)
        assert "on cpu" not in str(e.value), str(e.value)
    for t, depth in ((torch.zeros((T, ns, 7), dtype=torch.int32), False), (torch.zeros((T, ns, 7), dtype=torch.float32), False), (torch.zeros((T, ns), dtype=torch.float32), True)):
        with pytest.raises(ValueError, match="on cpu"):                 # everything right but the device
            b.rollout_observe_dev(u, 0.01, 4, sensors=t, depth=depth)
        with pytest.raises(mgf_amd.MgfError):                           # and a call whose arguments are all in order does reach C
            b.rollout_observe_dev(u, 0.01, 4, sensors=_Fake(t), depth=depth)
    with pytest.raises(ValueError, match="not ndarray"):
        b.rollout_observe_dev(u, 0.01, 4, sensors=np.zeros((T, ns, 7), np.int32))
    # the touch rows are rollout_touches_dev's, and rollout_dev's own checks stand ahead of both
    with pytest.raises(ValueError, match=r"touches: .* is not \[3, 6, 4\]"):
        b.rollout_observe_dev(u, 0.01, 4, touches=torch.zeros((T, 6, 16), dtype=torch.int32), short=True)
    with pytest.raises(ValueError, match="required"):
        b.rollout_observe_dev(None, 0.01, 4)
    with pytest.raises(ValueError, match=r"is not \[3, 10, 3\]"):
        b.rollout_observe_dev(u, 0.01, 4, x=torch.zeros((T, 9, 3), dtype=torch.float32))
    # the host form
    with pytest.raises(ValueError, match=r"is not \[T, 4\]"):
        b.rollout_observe(np.zeros((T, n + 1), np.float32), 0.01, 4)
    with pytest.raises(ValueError, match="sensors"):
        b.rollout_observe(np.zeros((T, n), np.float32), 0.01, 4, sensors="hits")
    with pytest.raises(ValueError, match="trace"):
        b.rollout_observe(np.zeros((T, n), np.float32), 0.01, 4, trace=("x", "sensors"))
    with pytest.raises(mgf_amd.MgfError):
        b.rollout_observe(np.zeros((T, n), np.float32), 0.01, 4, body=[1, 2, 3], sensors="depth")


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_kernels_are_the_two_the_header_names_and_the_ray_front_is_not_restated():
    k = read("mgf_amd", "csrc", "k_batch_scan.h")
    code = re.sub(r"//[^\n]*", "", k[k.index("#pragma once"):])
    assert '#include "k_batch_sensor.h"' in code
    assert code.count("bs_rays(A, TickBodies(") == 1 and "bs_rays(A, TickBodies(A, bpk), s_dyn);" in code
    assert "struct TickBodies : PlainBodies {" in code and "bpk[4 * ((size_t)g0 + i)]" in code and "bpk[4 * ((size_t)g0 + i) + 3]" in code
    assert "col0" not in code and "col1" not in code and not re.search(r"atomic|asm|__shfl|__ballot|\bfmaf?\(|__fm|bq_ray_front|bq_reduce|q_ray_terrain", code)
    assert code.count("__syncthreads()") == 1 and "__shared__" not in code.replace("extern __shared__ float4 s_dyn[];", "")
    assert len(re.findall(r"__global__ __launch_bounds__\(kBatchBlock\)", k)) == len(re.findall(r"__global__", k)) == 2
    rows = code[code.index("void k_batch_scan_rows("):]
    assert "__syncthreads" not in rows and "s_dyn" not in rows and "return;" not in rows
    assert "const bool on = in && (!MGF_SCAN_GATE || (A.done[k] == t + 1u && A.act[k] <= t + 1u));" in rows and "#define MGF_SCAN_GATE 1" in code
    assert rows.index("if (on) {") < rows.index("q_ray_load(") < rows.index("q_ray_obstacle(") < rows.index("const size_t at = (size_t)t * A.n_sensor + i;")
    assert "if (q_ray_castable(ld3(q.d)))" in rows      # the one predicate of k_query.h: no direction, or one outside the band, hits nothing
    stores = re.findall(r"(static_cast<float\*>\(A\.out\)\[at\] = |q_ray_store\(static_cast<int32_t\*>\(A\.out\) \+ 7 \* at, best\))", rows)
    assert len(stores) == 2 and rows.count("A.out") == 2                                               # the only global stores
    assert not re.findall(r"\bA\.\w+(?:\[[^\]]*\])? = ", rows)                                         # nothing of the arguments is written
    for word in ("UNGATED", "not measured", "TickUndo", "NOT bpk"):
        assert word in k, word
    # the fronts stay written once (tests/test_world_batch_rigs_host.py holds all of them): the lines this file could have restated
    batch = [f for f in sorted(os.listdir(os.path.join(ROOT, "mgf_amd", "csrc"))) if re.fullmatch(r"k_batch\w*\.h", f)]
    text = "".join(read("mgf_amd", "csrc", f) for f in batch)
    for line in ("void bq_ray_front(", "void bs_rays(", "const SensorIn s = A.rig[qi];", "q_ray_store(A.out + 7 * (size_t)qi, best);", "bs_rays(A, TickBodies("):
        assert text.count(line) == 1, line
    if not os.path.exists(os.path.join(ROOT, "mgf_amd", "libmgf_hip.so")) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    res = kernel_resources("k_batch_scan_")
    assert set(res) == {"k_batch_scan_rays", "k_batch_scan_rows<0>", "k_batch_scan_rows<1>"}, sorted(res)
    design = re.sub(r"\s+", " ", read("DESIGN.md"))
    for name, v in sorted(res.items()):
        print(name, ": vgpr, sgpr, scratch, static lds, sgpr spills, vgpr spills =", v)
        assert (v[2], v[3], v[4], v[5]) == ("0", "0", "0", "0"), (name, v)       # no scratch, no static LDS, no spills
        assert f"`{name}` {v[0]} / {v[1]} / 0 / 0 / 0" in design, (name, v)       # the line DESIGN.md records
    sensor = kernel_resources("k_batch_sensor_")
    assert set(sensor) == {"k_batch_sensor_ray"}
    v = sensor["k_batch_sensor_ray"]
    assert f"`k_batch_sensor_ray` {v[0]} / {v[1]} / 0 / 0 / 0" in design[design.index("## Rollout sensor traces"):design.index("## 9.")]
    assert int(res["k_batch_scan_rays"][0]) <= int(v[0])                           # the same front over another staging: no more vector registers
    # the pinned sets of the other prefixes are unchanged
    assert set(kernel_resources("k_batch_trace")) == {"k_batch_trace_touch<0>", "k_batch_trace_touch<1>"}
    assert set(kernel_resources("k_batch_rollout")) == {"k_batch_rollout_act<0>", "k_batch_rollout_act<1>", "k_batch_rollout_record"}
    assert set(kernel_resources("k_batch_touch")) == {"k_batch_touch"} and len(kernel_resources("k_batch_actuate")) == 4
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_lane_masks.py")], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 lane masks" in r.stdout, r.stdout[-400:]


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_late_contact_rig_shows_a_row_written_from_the_wrong_tick_by_the_oracle():
    """no actuator acts in the oracle's worlds; the GPU test's are weak enough to leave the ticks of first contact where they are
    (tests/test_world_batch_rollout_host.py), and it holds its own rows to its own loop.  What is checked here is what the bodies
    alone show (YC.sphere_hits: the oracle's Intersects<Sphere> over the oracle's poses, the definition's particles): the floor only
    adds hits."""
    rig = YC.late_sensor_rig()
    counts, seen = YC.late_oracle_view()
    scs = RC.late_contact_scenes()
    lengths = np.int64([len(sc["comps"]) for sc in scs])
    assert YC.T == len(counts) == RC.T + 2 and lengths.tolist() == [27, 18, 8]
    assert np.all(rig["body"] < lengths[rig["world"]]) and set(rig["world"].tolist()) == {0, 1, 2} and np.any(np.diff(rig["world"]) < 0)   # every world, in mixed order
    assert int(np.sum(rig["world"] == RC.LATE_A)) > 256                                                  # one world, two work items
    assert set(rig["flags"].tolist()) == {0, 1} and np.any(np.isinf(rig["dt"])) and np.any(np.isfinite(rig["dt"]))
    for k in (RC.LATE_A, RC.LATE_B):
        mine = rig["world"] == k
        rerun = next(t for t in range(YC.T) if counts[t, k] > RC.share(int(lengths[k]), 1))             # the tick that outgrows its share
        assert RC.FIRST_CONTACT <= rerun < YC.T - 1 and counts[:, k].max() <= RC.share(int(lengths[k]), 4), (k, counts[:, k].tolist())
        assert np.any(seen[rerun]["kind"][mine] == YC.HIT_BODY) and np.any(seen[rerun]["kind"][mine] == YC.HIT_NONE)
        for t in range(rerun - 1, YC.T - 1):                                                             # around it and behind it: another hit every tick
            assert seen[t][mine].tobytes() != seen[t + 1][mine].tobytes(), (k, t)
            assert np.any(seen[t]["t"][mine] != seen[t + 1]["t"][mine]), (k, t)                          # ... also in the one word of the depth format
    assert RC.share(27, 1) < counts[:, RC.LATE_A].max() and counts[:, RC.SPARSE].max() <= RC.share(8, 1)  # A re-runs, SPARSE never does
