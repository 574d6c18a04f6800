"""The touch trace of a rollout (mgf_batch_rollout_touches, mgf_batch_rollout_touches_dev) without a GPU: the header, the library, the
binding and the documents carry the calls and the constants; what needs no handle is refused on a handle that is never dereferenced, in
the header's order; the device form looks every pointer up and holds the outputs against each other and the inputs before it enqueues
anything; the binding turns a wrong tensor down before it calls C; the kernel keeps k_batch_touch's shape and bounds and the parents'
kernels are still exactly theirs; and the late-contact rig of tests/batch_trace_cases.py does, by the oracle, what
tests/test_gpu_world_batch_trace.py needs of it."""
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
from tests import batch_touch_cases as TC
from tests import batch_trace_cases as XC
from tests.util import ROOT, kernel_resources, read

CALLS = ("mgf_batch_rollout_touches", "mgf_batch_rollout_touches_dev")
HOST_FILE = "host_batch_trace.inc"


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
def test_header_library_binding_and_documents_carry_the_calls():
    h = read("include", "mgf_hip.h")
    flat_h = re.sub(r"\s+", " ", h)
    for sig in ("MGF_API mgf_status mgf_batch_rollout_touches(mgf_batch* b, float dt, int32_t iters, int64_t n_ticks, const float* u, int64_t n_act, int32_t mode, "
                "const int32_t* body, int64_t m, float* x, float* q, float* v, float* omega, void* touch, int64_t n_touch, int32_t touch_format, "
                "mgf_step_stats* stats);",
                "MGF_API mgf_status mgf_batch_rollout_touches_dev(mgf_batch* b, float dt, int32_t iters, int64_t n_ticks, const float* u_dev, int64_t n_act, "
                "int32_t mode, const int32_t* body_dev, int64_t m, float* x_dev, float* q_dev, float* v_dev, float* omega_dev, void* touch_dev, "
                "int64_t n_touch, int32_t touch_format, mgf_step_stats* stats);"):
        assert sig in flat_h, sig
    # a section of its own, behind the springs' and ahead of the counters' comment
    assert (h.index("mgf_batch_apply_springs_dev(mgf_batch*") < h.index("/* ---- rollout touch traces") < h.index("#define MGF_ROLLOUT_TOUCH_FULL")
            < h.index("MGF_API mgf_status mgf_batch_rollout_touches(") < h.index("/* name in {") < h.index("mgf_batch_counter(const"))
    for name, value in (("MGF_ROLLOUT_TOUCH_FULL", _capi.ROLLOUT_TOUCH_FULL), ("MGF_ROLLOUT_TOUCH_SHORT", _capi.ROLLOUT_TOUCH_SHORT),
                        ("MGF_BATCH_ROLLOUT_TOUCH_LAUNCHES_PER_TICK", _capi.BATCH_ROLLOUT_TOUCH_LAUNCHES_PER_TICK)):
        m = re.search(r"#define %s\s+(\d+)" % name, h)
        assert m and int(m.group(1)) == value, name
        assert getattr(mgf_amd, name[4:]) == value, name
    assert (_capi.ROLLOUT_TOUCH_FULL, _capi.ROLLOUT_TOUCH_SHORT, _capi.BATCH_ROLLOUT_TOUCH_LAUNCHES_PER_TICK) == (0, 1, 1)
    assert mgf_amd.TOUCH_SHORT_DTYPE is _capi.TOUCH_SHORT_DTYPE and _capi.TOUCH_SHORT_DTYPE.itemsize == 16
    assert _capi.TOUCH_SHORT_DTYPE.names == XC.SHORT_FIELDS == ("n_contacts", "partner", "normal_impulse", "strongest_impulse")
    assert [_capi.TOUCH_SHORT_DTYPE.fields[f][0] for f in XC.SHORT_FIELDS] == [_capi.TOUCH_REPORT_DTYPE.fields[f][0] for f in XC.SHORT_FIELDS]
    section = re.sub(r"\s*\n \* ", " ", h[h.index("/* ---- rollout touch traces"):h.index("/* name in {")])
    for word in ("bit for bit", "mgf_batch_apply_springs_dev(b, dt, NULL)", "mgf_batch_actuate_dev(b, u[t], n_act, mode, NULL)",
                 "mgf_batch_step(b, dt, iters, 1, stats + t * n_worlds)", "mgf_batch_gather_state_dev(b, body, m, x[t], q[t], v[t], omega[t], NULL, NULL)",
                 "mgf_batch_read_touches_dev(b, touch + t * n_touch, n_touch)", "n_contacts, partner, normal_impulse, strongest_impulse",
                 "EVERY entry is written", "MGF_TOUCH_BODY_FRAME", "several components", "launch for launch", "ONE HOST WAIT", "rollout_launches",
                 "query_launches", "nothing enqueued", "overflows int64_t", "OUT OF SCOPE", "collider gather", "lone mgf_world", "hipGraph"):
        assert word in section, word
    # the two notes of the parents: the old words stand, with a "since"
    rollouts = flat_h[flat_h.index("/* ---- rollouts"):flat_h.index("#define MGF_BATCH_ROLLOUT_LAUNCHES_PER_TICK")]
    assert re.search(r"contact or touch sums per tick \([^)]*since: Rollout touch traces", rollouts)
    sensors = flat_h[flat_h.index("---- contact sensors:"):flat_h.index("#define MGF_TOUCH_STATIC")]
    assert re.search(r"sums over the ticks of a multi-tick mgf_batch_step call \([^)]*\) \(since: Rollout touch traces", sensors)
    counters = flat_h[flat_h.index("/* name in {"):]
    assert re.search(r'"rollout_launches" \([^)]*_rollout_touches[^)]*touch trace', counters)
    lib = mgf_amd.load_library()
    vp, i64, i32, f32 = C.c_void_p, C.c_int64, C.c_int32, C.c_float
    for name in CALLS:
        assert name in _capi.SYMBOLS, name
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (i32, [vp, f32, i32, i64, vp, i64, i32, vp, i64, vp, vp, vp, vp, vp, i64, i32, vp]), name
    for method in ("rollout_touches", "rollout_touches_dev"):
        assert callable(getattr(mgf_amd.WorldBatch, method)), method
    flat = re.sub(r"\s+", " ", read("INTEGRATION.md"))
    for sig in ("pub fn mgf_batch_rollout_touches(b: *mut mgf_batch, dt: f32, iters: i32, n_ticks: i64, u: *const f32, n_act: i64, mode: i32, body: *const i32, "
                "m: i64, x: *mut f32, q: *mut f32, v: *mut f32, omega: *mut f32, touch: *mut c_void, n_touch: i64, touch_format: i32, "
                "stats: *mut mgf_step_stats) -> mgf_status;",
                "pub fn mgf_batch_rollout_touches_dev(b: *mut mgf_batch, dt: f32, iters: i32, n_ticks: i64, u_dev: *const f32, n_act: i64, mode: i32, "
                "body_dev: *const i32, m: i64, x_dev: *mut f32, q_dev: *mut f32, v_dev: *mut f32, omega_dev: *mut f32, touch_dev: *mut c_void, n_touch: i64, "
                "touch_format: i32, stats: *mut mgf_step_stats) -> mgf_status;",
                "pub const MGF_ROLLOUT_TOUCH_FULL: i32 = 0;", "pub const MGF_ROLLOUT_TOUCH_SHORT: i32 = 1;",
                "pub const MGF_BATCH_ROLLOUT_TOUCH_LAUNCHES_PER_TICK: i64 = 1;",
                "pub struct mgf_touch_short { pub n_contacts: i32, pub partner: i32, pub normal_impulse: f32, pub strongest_impulse: f32 }",
                "pub fn rollout_touches(", "pub unsafe fn rollout_touches_dev("):
        assert sig in flat, sig
    kernels = read("mgf_amd", "csrc", "kernels.h")
    assert kernels.index('#include "k_batch_rollout.h"') < kernels.index('#include "k_batch_trace.h"') and "k_batch_trace_touch<FORMAT> (k_batch_trace.h)" in kernels
    hip = read("mgf_amd", "csrc", "mgf_hip.hip")
    assert hip.index('#include "host_batch_spring.inc"') < hip.index('#include "%s"' % HOST_FILE)
    design = read("DESIGN.md")
    assert design.index("## Springs") < design.index("## Rollout touch traces") < design.index("## 9.")
    sub = design[design.index("## Rollout touch traces"):design.index("## 9.")]
    for word in ("k_batch_trace_touch", "Definition", "done[k] == t + 1 && act[k] <= t + 1", "batch_allot", "Launches", "Checks", "Compiler output", "Tests",
                 "Measured", "Out of scope", "batch_rollout_touch_bench.py", "MGF_BATCH_ROLLOUT_TOUCH_LAUNCHES_PER_TICK", "hipGraph"):
        assert word in sub, word
    readme = read("README.md")
    assert "rollout_touches(" in readme and "rollout_touches_dev" in readme
    assert os.path.exists(os.path.join(ROOT, "tools", "batch_rollout_touch_bench.py"))


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def test_what_needs_no_handle_is_refused_before_the_handle_is_dereferenced_in_the_headers_order():
    lib = mgf_amd.load_library()
    INV = _capi.ERR_INVALID

    def err():
        return lib.mgf_last_error().decode()
    fake = C.c_void_p(16)   # a handle that is never dereferenced; addresses that are never looked up
    p = [C.c_void_p((k + 1) << 20) for k in range(8)]
    u, body, x, q, v, om, st, touch = p
    dt = C.c_float(1.0 / 60.0)
    big = 1 << 62
    for fn in (lib.mgf_batch_rollout_touches, lib.mgf_batch_rollout_touches_dev):
        def call(h, iters=4, n_ticks=3, n_act=5, mode=0, m=6, n_touch=7, fmt=0):
            return fn(h, dt, iters, n_ticks, u, n_act, mode, body, m, x, q, v, om, touch, n_touch, fmt, st)
        assert call(None) == INV and "NULL" in err()
        assert call(None, iters=-1, n_ticks=-1, n_act=-1, mode=9, m=-1, n_touch=-1, fmt=9) == INV and "NULL" in err()   # the handle first, whatever the rest
        assert call(fake, n_ticks=-1, iters=-1, n_act=-1, m=-1, n_touch=-1, mode=9, fmt=9) == INV and "n_ticks is negative" in err()
        assert call(fake, iters=-1, n_act=-1, m=-1, n_touch=-1, mode=9, fmt=9) == INV and "iters is negative" in err()
        assert call(fake, n_act=-1, m=-1, n_touch=-1, mode=9, fmt=9, n_ticks=1 << 30) == INV and "n_act is negative" in err()
        assert call(fake, m=-(1 << 40), n_touch=-1, mode=9, fmt=9, n_ticks=1 << 30) == INV and "m is negative" in err()
        assert call(fake, n_touch=-(1 << 40), mode=9, fmt=9, n_ticks=1 << 30) == INV and "n_touch is negative" in err()
        assert call(fake, n_ticks=(1 << 20) + 1, mode=9, fmt=9, m=1 << 31) == INV and "2^20" in err()
        for mode in (2, -1, 1 << 20):
            assert call(fake, mode=mode, fmt=9, m=1 << 31) == INV and "mode" in err(), mode
        for fmt in (2, -1, 64, 1 << 20):
            assert call(fake, fmt=fmt, m=1 << 31, n_touch=big) == INV and "touch_format" in err(), fmt
            assert call(fake, fmt=fmt, n_ticks=0, n_act=0, m=0, n_touch=0) == INV and "touch_format" in err(), fmt
        assert call(fake, m=1 << 31, n_act=big, n_touch=big) == INV and "too many traced" in err()
        assert call(fake, n_ticks=1 << 20, n_act=big, n_touch=big) == INV and "4 * n_ticks * n_act overflows int64_t" in err()
        for fmt in (0, 1):                                                       # the bound is the full report's, whatever the format
            assert call(fake, n_ticks=1 << 20, n_act=0, n_touch=big, fmt=fmt) == INV and "64 * n_ticks * n_touch overflows int64_t" in err()
            assert call(fake, n_ticks=2, n_act=0, n_touch=1 << 57, fmt=fmt) == INV and "64 * n_ticks * n_touch overflows int64_t" in err()
    # the order is the one the header states, and nothing of it touches a device
    src = read("mgf_amd", "csrc", HOST_FILE)
    mine = src[src.index("static mgf_status batch_trace_args("):src.index('extern "C" mgf_status mgf_batch_rollout_touches_dev(')]
    assert "batch_rollout_args(b, iters, n_ticks, u, n_act, mode, body, m, bytes, tt)" in mine
    shared = read("mgf_amd", "csrc", "host_batch_rollout.inc")
    args = shared[shared.index("static mgf_status batch_rollout_args("):shared.index("static mgf_status batch_rollout_run(")]
    marks = ["batch_rig_handle(b)", '"n_ticks is negative"', '"iters is negative"', '"n_act is negative"', '"m is negative"', '"n_touch is negative"',
             '"n_ticks must be at most 2^20"', "mode != MGF_ACTUATE_IMPULSE && mode != MGF_ACTUATE_FORCE",
             "tt->format != MGF_ROLLOUT_TOUCH_FULL && tt->format != MGF_ROLLOUT_TOUCH_SHORT", "m > (int64_t)INT32_MAX", '"4 * n_ticks * n_act overflows int64_t"',
             '"64 * n_ticks * n_touch overflows int64_t"', "b->actuators.recs.size()", "b->touches.recs.size()", "n_act > 0 && n_ticks > 0 && !u",
             "tt->n > 0 && n_ticks > 0 && !tt->out", "!body && m > mgf_batch_len(b, -1)"]
    order = [args.index(s) for s in marks]
    assert order == sorted(order), order
    assert args.index("n_touch overflows int64_t") < args.index("b->")              # the handle's contents come last
    for text in (mine, args):
        assert not re.search(r"ctx_bind|<<<|Async|\.ensure\(|h2d\(|d2h\(", text)
    sec = re.sub(r"\s+", " ", read("include", "mgf_hip.h"))
    sec = sec[sec.index("/* ---- rollout touch traces"):]
    words = ["a NULL batch", "negative n_ticks, iters, n_act, m or n_touch", "n_ticks > 2^20", "a mode other than", "a touch_format other than", "m > INT32_MAX",
             "4 * n_ticks * n_act, then 64 * n_ticks * n_touch", "n_act != mgf_batch_actuator_count(b)", "n_touch != mgf_batch_touch_count(b)",
             "NULL u with n_act > 0 and n_ticks > 0", "NULL touch with n_touch > 0 and n_ticks > 0", "body == NULL with m > mgf_batch_len(b, -1)"]
    at = [sec.index(w) for w in words]
    assert at == sorted(at), at
    for name in CALLS:
        f = src[src.index('extern "C" mgf_status %s(' % name):]
        assert f.index("batch_trace_args(") < f.index("ctx_bind(")


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_device_form_looks_every_pointer_up_before_the_first_enqueue():
    src = read("mgf_amd", "csrc", HOST_FILE)
    run = src[src.index('extern "C" mgf_status mgf_batch_rollout_touches_dev('):src.index('extern "C" mgf_status mgf_batch_rollout_touches(')]
    enqueue = r"batch_rollout_run\(|batch_step_run\(|batch_rig_up\(|batch_push\(|hipMemsetAsync|hipMemcpyAsync|<<<|\.ensure\(|h2d\(|d2h\("
    first_enqueue = min(m.start() for m in re.finditer(enqueue, run))
    checks = [m.start() for m in re.finditer(r"dev_span\(", run)]
    assert len(checks) == 7 and max(checks) < first_enqueue
    for name in ("u_dev, n.u", "body_dev, n.body", r"x_dev, n.out\[0\]", r"q_dev, n.out\[1\]", r"v_dev, n.out\[2\]", r"omega_dev, n.out\[3\]", "touch_dev, n.touch"):
        assert re.search(r"dev_span\(b->ctx, " + name, run), name
    assert max(checks) < run.index("dev_outputs_overlap(arrays, 7, 5)") < first_enqueue               # five outputs, against each other and the two inputs
    assert run.index("batch_trace_args(") < run.index("ctx_bind(") < min(checks)
    assert "hipStreamSynchronize" not in run and "hipMemcpy" not in run                              # no copy of its own
    shared = read("mgf_amd", "csrc", "host_batch_rollout.inc")
    assert "bytes->touch = tt ? (tt->format == MGF_ROLLOUT_TOUCH_SHORT ? 16u : 64u) * T * (size_t)tt->n : 0;" in shared
    # the host form: one upload, the device core, one download
    host_form = src[src.index('extern "C" mgf_status mgf_batch_rollout_touches('):]
    assert host_form.count("h2d(") == 1 and host_form.count("d2h(") == 1 and host_form.count("batch_rollout_run(") == 1
    assert host_form.index("h2d(") < host_form.index("batch_rollout_run(") < host_form.index("d2h(")
    assert "<<<" not in src and "d_launches" not in src and "q_launches" not in src and "batch_single_parts(" not in src
    # the core is the rollout's, the rig up ahead of the train; the train launches the trace behind the record, its view rebuilt per pass
    core = shared[shared.index("static mgf_status batch_rollout_run("):shared.index('extern "C" mgf_status mgf_batch_rollout_dev(')]
    assert core.index("batch_push(") < core.index('batch_rig_up(b, b->touches, "contact sensor", 3)') < core.index("batch_step_run(b, dt, iters, n_ticks, stats, &H)")
    host = read("mgf_amd", "csrc", "host_batch.inc")
    train = host[host.index("static mgf_status batch_step_run("):host.index('extern "C" mgf_status mgf_batch_step(')]
    assert train.count("k_batch_trace_touch<") == 2
    assert train.index("k_batch_solve<<<") < train.index("k_batch_rollout_record<<<") < train.index("k_batch_trace_touch<")
    assert train.index("hook->launches += MGF_BATCH_ROLLOUT_TOUCH_LAUNCHES_PER_TICK;") > train.index("k_batch_trace_touch<")
    passes = train[train.index("for (uint32_t first = 0"):]
    per_tick = passes.index("for (uint32_t t = first;")
    for word in ("V.cons = b->cons.p;", "V.c_off = b->d_coff.p;", "V.c_count = b->d_ccount.p;", "V.tile = batch_touch_tile(b);"):
        assert 0 < passes.index(word) < per_tick, word                                                 # inside the loop of passes, ahead of its ticks
    assert passes.index("batch_allot(b, true)") > per_tick
    assert "4u * hook->T.V.tile" in train
    step = host[host.index('extern "C" mgf_status mgf_batch_step('):]
    assert "batch_step_run(b, dt, iters, n_ticks, stats, nullptr)" in step[:step.index("\n}\n")]


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
class _Fake:
    """stands for a CUDA tensor in the binding's checks: what _dev_arg reads of one"""

    def __init__(self, t):
        import torch
        self._t = t
        self.dtype, self.shape, self.device = t.dtype, t.shape, torch.device("cuda", 0)

    def data_ptr(self):
        return 1 << 22

    def is_contiguous(self):
        return self._t.is_contiguous()

    def numel(self):
        return self._t.numel()

    def dim(self):
        return self._t.dim()


def test_the_binding_turns_a_wrong_tensor_down_before_it_calls_c():
    import torch

    class Handle(mgf_amd.WorldBatch):   # no context, no C handle: a call that got as far as C would fail differently
        def __init__(self):
            self._h, self.n_worlds = None, 2

        def actuator_count(self):
            return 4

        def touch_count(self):
            return 6

        def __len__(self):
            return 10

    b, n, T, nt = Handle(), 4, 3, 6
    u = _Fake(torch.zeros((T, n), dtype=torch.float32))
    for short, words in ((False, 16), (True, 4)):
        wrong = [torch.zeros((T, nt, words), dtype=torch.float64), torch.zeros((T, nt, words), dtype=torch.int64), torch.zeros((T, nt, words), dtype=torch.int16),
                 torch.zeros((T, nt, 20 - words), dtype=torch.int32), torch.zeros((T + 1, nt, words), dtype=torch.int32),
                 torch.zeros((T, nt - 1, words), dtype=torch.float32), torch.zeros((T * nt, words), dtype=torch.int32), torch.zeros(T * nt * words, dtype=torch.int32),
                 torch.zeros((T, words, nt), dtype=torch.int32).transpose(1, 2), torch.zeros((T, nt, 2 * words), dtype=torch.float32)[:, :, ::2]]
        for t in wrong:
            with pytest.raises(ValueError) as e:
                b.rollout_touches_dev(u, 0.01, 4, touches=t, short=short)
            assert "on cpu" not in str(e.value), str(e.value)          # turned down for what it is, not for where it is
        for dtype in (torch.int32, torch.float32):
            with pytest.raises(ValueError, match="on cpu"):             # everything right but the device
                b.rollout_touches_dev(u, 0.01, 4, touches=torch.zeros((T, nt, words), dtype=dtype), short=short)
        with pytest.raises(mgf_amd.MgfError):                           # and a call whose arguments are all in order does reach C
            b.rollout_touches_dev(u, 0.01, 4, touches=_Fake(torch.zeros((T, nt, words), dtype=torch.int32)), short=short)
    with pytest.raises(ValueError, match="not ndarray"):
        b.rollout_touches_dev(u, 0.01, 4, touches=np.zeros((T, nt, 16), np.int32))
    # rollout_dev's own checks stand ahead of it
    with pytest.raises(ValueError, match="required"):
        b.rollout_touches_dev(None, 0.01, 4)
    with pytest.raises(ValueError, match="on cpu"):
        b.rollout_touches_dev(torch.zeros((T, n), dtype=torch.float32), 0.01, 4)
    with pytest.raises(ValueError, match=r"is not \[3, 10, 3\]"):
        b.rollout_touches_dev(u, 0.01, 4, x=torch.zeros((T, 9, 3), dtype=torch.float32))
    # the host form: u is [T, n]; a trace is one of the four
    with pytest.raises(ValueError, match=r"is not \[T, 4\]"):
        b.rollout_touches(np.zeros((T, n + 1), np.float32), 0.01, 4)
    with pytest.raises(ValueError, match="trace"):
        b.rollout_touches(np.zeros((T, n), np.float32), 0.01, 4, trace=("x", "touches"))
    with pytest.raises(mgf_amd.MgfError):
        b.rollout_touches(np.zeros((T, n), np.float32), 0.01, 4, body=[1, 2, 3], short=True)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_kernel_keeps_the_parents_shape_and_bounds_and_the_parents_kernels_are_theirs():
    k = read("mgf_amd", "csrc", "k_batch_trace.h")
    code = re.sub(r"//[^\n]*", "", k[k.index("#pragma once"):])
    assert '#include "k_batch_touch.h"' in code
    assert not re.search(r"atomic|\brows\b|return;|break;|continue;|asm|__shfl|__ballot|__any|\bfmaf?\(|__fm", code)
    assert code.count("__syncthreads()") == 2 and "__shared__" not in code.replace("extern __shared__ float4 s_dyn[];", "")
    assert len(re.findall(r"__global__ __launch_bounds__\(kBatchBlock\)", k)) == len(re.findall(r"__global__", k)) == 1
    assert not re.search(r"struct (TouchIn|TouchWord|TouchFold)\b|uint32_t touch_lower\(", code)        # the parent's, not restated
    # the gate: the record's condition, the workgroup's, folded into the item's count and the list's length
    assert "const bool on = T.done[k] == t + 1u && T.act[k] <= t + 1u;" in code
    assert "const uint32_t C = on ? A.c_count[k] : 0u, count = on ? it.z : 0u;" in code and "const bool live = tid < count;" in code
    loop = code[code.index("for (uint32_t c0 = 0; c0 < C; c0 += tile)"):]
    assert code.index("__syncthreads()") > code.index("for (uint32_t c0 = 0; c0 < C; c0 += tile)") and loop.count("__syncthreads()") == 2
    # the only global stores: a report's four words, or the short one
    stores = re.findall(r"\b(o\[\d\]|A\.out\[at\]) = TouchWord\{", code)
    assert stores == ["A.out[at]", "o[0]", "o[1]", "o[2]", "o[3]"], stores
    assert "A.out" not in code.replace("A.out[at] = TouchWord{", "").replace("TouchWord* o = A.out + 4 * at;", "")
    assert "const size_t at = (size_t)t * T.n_touch + qi;" in code
    assert not re.findall(r"\b(?:T|A)\.\w+(?:\[[^\]]*\])? = ", code.replace("A.out[at] = ", ""))            # nothing else of the arguments is written
    # the restated body is the parent's, line for line, where the gate and the target do not enter
    parent = read("mgf_amd", "csrc", "k_batch_touch.h")
    fold = parent[parent.index("  TouchIn s;\n"):parent.index("  const bool scan = live")]
    assert fold in k
    tile = parent[parent.index("      for (uint32_t i = tid; i < tile; i += kBatchBlock)"):parent.index("  if (live) {\n    V3 imp = F.imp")]
    assert tile in k
    tail = parent[parent.index("      const CRec* r = &cons[F.best_c];"):parent.index("    TouchWord* o = A.out")]
    assert tail.replace("\n    ", "\n      ").replace("      const CRec* r", "        const CRec* r", 1) in k
    for line in ("o[0] = TouchWord{F.n, (uint32_t)F.best_partner, (uint32_t)record, 0u};", "o[1] = TouchWord{f2u(imp.x), f2u(imp.y), f2u(imp.z), f2u(F.sum)};",
                 "o[2] = TouchWord{f2u(push.x), f2u(push.y), f2u(push.z), f2u(F.best_ni)};", "o[3] = TouchWord{f2u(arm.x), f2u(arm.y), f2u(arm.z), 0u};"):
        assert line in parent and line in k, line
    assert "A.out[at] = TouchWord{F.n, (uint32_t)F.best_partner, f2u(F.sum), f2u(F.best_ni)};" in k
    if not os.path.exists(os.path.join(ROOT, "mgf_amd", "libmgf_hip.so")) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    rows = kernel_resources("k_batch_trace")
    assert set(rows) == {"k_batch_trace_touch<0>", "k_batch_trace_touch<1>"}, sorted(rows)
    design = re.sub(r"\s+", " ", read("DESIGN.md"))
    for name, v in sorted(rows.items()):
        print(name, ": vgpr, sgpr, scratch, static lds, sgpr spills, vgpr spills =", v)
        assert (v[2], v[3], v[4], v[5]) == ("0", "0", "0", "0"), (name, v)       # no scratch, no static LDS, no spills
        assert int(v[0]) <= 64, (name, v)                                         # the parent's bound: eight waves a SIMD
        assert f"`{name}` {v[0]} / {v[1]} / 0 / 0 / 0" in design, (name, v)       # the line DESIGN.md records
    assert set(kernel_resources("k_batch_touch")) == {"k_batch_touch"}
    assert set(kernel_resources("k_batch_rollout")) == {"k_batch_rollout_act<0>", "k_batch_rollout_act<1>", "k_batch_rollout_record"}
    assert len(kernel_resources("k_batch_actuate")) == 4
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_lane_masks.py")], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 lane masks" in r.stdout, r.stdout[-400:]


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_late_contact_rig_shows_a_row_written_from_the_wrong_tick_by_the_oracle():
    """no actuator acts in the oracle's worlds; the GPU test's are weak enough to leave the ticks of first contact where they are
    (tests/test_world_batch_rollout_host.py), and it holds its own rows to its own lists"""
    scs, lists, qs = XC.late_oracle()
    rig = XC.late_touch_rig()
    assert XC.T == len(lists) == RC.T + 2 and [len(sc["comps"]) for sc in scs] == [27, 18, 8]
    lengths = np.int64([len(sc["comps"]) for sc in scs])
    assert np.all(rig["body"] < lengths[rig["world"]]) and np.all(rig["other"] < lengths[rig["world"]]) and np.all(rig["other"] != rig["body"])
    assert set(rig["world"].tolist()) == {0, 1, 2} and np.any(np.diff(rig["world"]) < 0)                # every world, in mixed order
    assert int(np.sum(rig["world"] == RC.LATE_A)) > 256                                                  # one world, two work items
    assert set(rig["flags"].tolist()) == {0, _capi.TOUCH_BODY_FRAME}
    reports = XC.fold_ticks(rig, lists, qs)
    kinds = np.array([str(XC.kind(s)) for s in rig])
    for k in (RC.LATE_A, RC.LATE_B):
        mine = rig["world"] == k
        counts = [len(lists[t][k]) for t in range(XC.T)]
        first = next(t for t in range(XC.T) if counts[t])
        assert first >= RC.FIRST_CONTACT and not reports["n_contacts"][:first, mine].any(), (k, counts)
        assert max(counts) > RC.share(int(lengths[k]), 1) and max(counts) <= RC.share(int(lengths[k]), 4), (k, counts)   # A re-runs, B never does
        for kd in TC.KINDS:
            sel = mine & (kinds == str(kd))
            assert np.any(reports["n_contacts"][first:, sel] > 0), (k, kd)
            for frame in (0, _capi.TOUCH_BODY_FRAME):
                assert np.any(sel & (rig["flags"] == frame)), (k, kd, frame)
        # a report differs between two consecutive ticks behind first contact
        changing = [t for t in range(first, XC.T - 1) if reports[t][mine].tobytes() != reports[t + 1][mine].tobytes()]
        assert changing, k
        # ... also in the four words of the short format
        short = XC.short_of(reports)
        assert any(short[t][mine].tobytes() != short[t + 1][mine].tobytes() for t in changing), k
    # the body frame turns something: a framed sensor's vectors differ from the same sensor's in the world frame
    plain = rig.copy()
    plain["flags"] = 0
    unframed = XC.fold_ticks(plain, lists, qs)
    framed = (rig["flags"] != 0)
    assert any(reports["impulse"][t, i].tobytes() != unframed["impulse"][t, i].tobytes() for t in range(XC.T) for i in np.flatnonzero(framed & (reports["n_contacts"][t] > 0)))
    # the actuator scenes' rig: every world but the one no actuator names has sensors of every kind
    arig = XC.actuator_touch_rig()
    akinds = np.array([str(XC.kind(s)) for s in arig])
    assert set(arig["world"].tolist()) == {0, 1, 2, 3, 4} and all(np.any(akinds == str(kd)) for kd in TC.KINDS) and set(arig["flags"].tolist()) == {0, 1}
