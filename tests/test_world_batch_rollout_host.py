"""The rollouts of a batch (mgf_batch_rollout, mgf_batch_rollout_dev) without a GPU: the header, the library, the binding and the
documents carry the calls; what needs no handle is refused on a handle that is never dereferenced, in the header's order; the device form
looks every pointer up and holds the outputs against each other and the inputs before it enqueues anything; the binding turns a wrong
tensor down before it calls C; the two kernels use no scratch and spill nothing; the actuators' kernel and host file are as they were;
and the scenes of tests/test_gpu_world_batch_rollout.py's re-run test do, by the oracle, what that test needs of them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mgf_amd
from mgf_amd import _capi
from tests import batch_rollout_cases as RC
from tests.util import ROOT, kernel_resources, oracle_world, read

CALLS = ("mgf_batch_rollout", "mgf_batch_rollout_dev")
HOST_FILE = "host_batch_rollout.inc"


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
def test_header_library_binding_and_documents_carry_the_calls():
    h = read("include", "mgf_hip.h")
    flat_h = re.sub(r"\s+", " ", h)
    for sig in ("MGF_API mgf_status mgf_batch_rollout(mgf_batch* b, float dt, int32_t iters, int64_t n_ticks, const float* u, int64_t n_act, int32_t mode, "
                "const int32_t* body, int64_t m, float* x, float* q, float* v, float* omega, mgf_step_stats* stats);",
                "MGF_API mgf_status mgf_batch_rollout_dev(mgf_batch* b, float dt, int32_t iters, int64_t n_ticks, const float* u_dev, int64_t n_act, int32_t mode, "
                "const int32_t* body_dev, int64_t m, float* x_dev, float* q_dev, float* v_dev, float* omega_dev, mgf_step_stats* stats);"):
        assert sig in flat_h, sig
    # a section of its own, behind the actuators' and ahead of the counters
    assert h.index("mgf_batch_actuate_dev(mgf_batch*") < h.index("/* ---- rollouts") < h.index("MGF_API mgf_status mgf_batch_rollout(") < h.index("mgf_batch_counter(const")
    m = re.search(r"#define MGF_BATCH_ROLLOUT_LAUNCHES_PER_TICK\s+(\d+)", h)
    assert m and int(m.group(1)) == _capi.BATCH_ROLLOUT_LAUNCHES_PER_TICK <= 2
    assert mgf_amd.BATCH_ROLLOUT_LAUNCHES_PER_TICK is _capi.BATCH_ROLLOUT_LAUNCHES_PER_TICK
    section = h[h.index("/* ---- rollouts"):h.index("mgf_batch_counter(const")]
    for word in ("bit for bit", "mgf_batch_actuate_dev(b, u[t], n_act, mode, NULL)", "mgf_batch_step(b, dt, iters, 1, stats + t * n_worlds)",
                 "mgf_batch_gather_state_dev(b, body, m, x[t], q[t], v[t], omega[t], NULL, NULL)", "ONE HOST WAIT", "capacity_retries", "ONCE",
                 "actuators_skipped", "device_skipped", "rollout_launches", "drive_launches", "launches_per_tick", "several components",
                 "nothing enqueued", "2^20", "INT32_MAX", "overflows int64_t", "OUT OF SCOPE", "closed-loop", "no host wait at all", "world mask",
                 "lone mgf_world", "hipGraph"):
        assert word in section, word
    assert "(since: Rollouts" in h[h.index("body-mounted actuators"):h.index("/* ---- rollouts")]
    assert "re-evaluation of a wrench per tick inside a multi-tick mgf_batch_step" in h             # the old words stand
    assert '"rollout_launches"' in h[h.index("/* name in {"):]
    lib = mgf_amd.load_library()
    vp, i64, i32, f32 = C.c_void_p, C.c_int64, C.c_int32, C.c_float
    for name in CALLS:
        assert name in _capi.SYMBOLS, name
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (i32, [vp, f32, i32, i64, vp, i64, i32, vp, i64, vp, vp, vp, vp, vp]), name
    for method in ("rollout", "rollout_dev"):
        assert callable(getattr(mgf_amd.WorldBatch, method)), method
    flat = re.sub(r"\s+", " ", read("INTEGRATION.md"))
    for sig in ("pub fn mgf_batch_rollout(b: *mut mgf_batch, dt: f32, iters: i32, n_ticks: i64, u: *const f32, n_act: i64, mode: i32, body: *const i32, m: i64, "
                "x: *mut f32, q: *mut f32, v: *mut f32, omega: *mut f32, stats: *mut mgf_step_stats) -> mgf_status;",
                "pub fn mgf_batch_rollout_dev(b: *mut mgf_batch, dt: f32, iters: i32, n_ticks: i64, u_dev: *const f32, n_act: i64, mode: i32, body_dev: *const i32, m: i64, "
                "x_dev: *mut f32, q_dev: *mut f32, v_dev: *mut f32, omega_dev: *mut f32, stats: *mut mgf_step_stats) -> mgf_status;",
                "pub const MGF_BATCH_ROLLOUT_LAUNCHES_PER_TICK: i64 = 2;", "pub fn rollout(", "pub unsafe fn rollout_dev("):
        assert sig in flat, sig
    kernels = read("mgf_amd", "csrc", "kernels.h")
    assert kernels.index('#include "k_batch_actuator.h"') < kernels.index('#include "k_batch_rollout.h"')
    assert "k_batch_rollout_act<MODE> / k_batch_rollout_record (k_batch_rollout.h)" in kernels
    hip = read("mgf_amd", "csrc", "mgf_hip.hip")
    assert hip.index('#include "host_batch_actuator.inc"') < hip.index('#include "%s"' % HOST_FILE)
    design = read("DESIGN.md")
    assert design.index("Body-mounted actuators") < design.index("## Rollouts") < design.index("## 9.")
    sub = design[design.index("## Rollouts"):design.index("## 9.")]
    for word in ("k_batch_rollout_act", "k_batch_rollout_record", "done[k] == t && act[k] == t", "undo", "Launches", "Checks", "Compiler output", "Tests",
                 "Measured", "Out of scope", "batch_rollout_bench.py", "MGF_BATCH_ROLLOUT_LAUNCHES_PER_TICK", "__any", "hipGraph"):
        assert word in sub, word
    assert "(since: Rollouts)" in design[design.index("Body-mounted actuators"):design.index("## Rollouts")]
    readme = read("README.md")
    assert "rollout_dev" in readme and "rollout(" in readme
    assert os.path.exists(os.path.join(ROOT, "tools", "batch_rollout_bench.py"))


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def test_what_needs_no_handle_is_refused_before_the_handle_is_dereferenced_in_the_headers_order():
    lib = mgf_amd.load_library()
    INV = _capi.ERR_INVALID

    def err():
        return lib.mgf_last_error().decode()
    fake = C.c_void_p(16)   # a handle that is never dereferenced; addresses that are never looked up
    p = [C.c_void_p((k + 1) << 20) for k in range(7)]
    u, body, x, q, v, om, st = p
    dt = C.c_float(1.0 / 60.0)
    big = 1 << 62
    for fn in (lib.mgf_batch_rollout, lib.mgf_batch_rollout_dev):
        def call(h, iters=4, n_ticks=3, n_act=5, mode=0, m=6):
            return fn(h, dt, iters, n_ticks, u, n_act, mode, body, m, x, q, v, om, st)
        assert call(None) == INV and "NULL" in err()
        assert call(None, iters=-1, n_ticks=-1, n_act=-1, mode=9, m=-1) == INV and "NULL" in err()           # the handle first, whatever the rest
        assert call(fake, n_ticks=-1, iters=-1, n_act=-1, m=-1, mode=9) == INV and "n_ticks is negative" in err()
        assert call(fake, iters=-1, n_act=-1, m=-1, mode=9) == INV and "iters is negative" in err()
        assert call(fake, n_act=-1, m=-1, mode=9, n_ticks=1 << 30) == INV and "n_act is negative" in err()
        assert call(fake, m=-(1 << 40), mode=9, n_ticks=1 << 30) == INV and "m is negative" in err()
        assert call(fake, n_ticks=(1 << 20) + 1, mode=9, m=1 << 31) == INV and "2^20" in err()
        for mode in (2, -1, 1 << 20):
            assert call(fake, mode=mode, m=1 << 31) == INV and "mode" in err(), mode
            assert call(fake, mode=mode, n_ticks=0, n_act=0, m=0) == INV and "mode" in err(), mode
        assert call(fake, m=1 << 31, n_act=big) == INV and "too many traced" in err()
        assert call(fake, n_ticks=1 << 20, n_act=big) == INV and "overflows int64_t" in err()
        assert call(fake, n_ticks=2, n_act=(1 << 61)) == INV and "overflows int64_t" in err()
    # the order is the one the header states, and nothing of it touches a device
    src = read("mgf_amd", "csrc", HOST_FILE)
    args = src[src.index("static mgf_status batch_rollout_args("):src.index("static mgf_status batch_rollout_run(")]
    marks = ["batch_rig_handle(b)", '"n_ticks is negative"', '"iters is negative"', '"n_act is negative"', '"m is negative"', '"n_ticks must be at most 2^20"',
             "mode != MGF_ACTUATE_IMPULSE && mode != MGF_ACTUATE_FORCE", "m > (int64_t)INT32_MAX", "overflows int64_t", "b->actuators.recs.size()",
             "n_act > 0 && n_ticks > 0 && !u", "!body && m > mgf_batch_len(b, -1)"]
    order = [args.index(s) for s in marks]
    assert order == sorted(order), order
    assert args.index("overflows int64_t") < args.index("b->")                                       # the handle's contents come last
    assert not re.search(r"ctx_bind|<<<|Async|\.ensure\(|h2d\(|d2h\(", args)
    h = re.sub(r"\s+", " ", read("include", "mgf_hip.h"))
    sec = h[h.index("/* ---- rollouts"):]
    words = ["a NULL batch", "negative n_ticks, iters, n_act or m", "n_ticks > 2^20", "a mode other than", "m > INT32_MAX", "overflows int64_t",
             "n_act != mgf_batch_actuator_count(b)", "NULL u with n_act > 0 and n_ticks > 0", "body == NULL with m > mgf_batch_len(b, -1)"]
    at = [sec.index(w) for w in words]
    assert at == sorted(at), at
    for name in CALLS:
        f = src[src.index('extern "C" mgf_status %s(' % name):]
        assert f.index("batch_rollout_args(") < f.index("ctx_bind(")


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_device_form_looks_every_pointer_up_before_the_first_enqueue():
    src = read("mgf_amd", "csrc", HOST_FILE)
    run = src[src.index('extern "C" mgf_status mgf_batch_rollout_dev('):src.index('extern "C" mgf_status mgf_batch_rollout(')]
    enqueue = r"batch_rollout_run\(|batch_step_run\(|batch_rig_up\(|batch_push\(|hipMemsetAsync|hipMemcpyAsync|<<<|\.ensure\(|h2d\(|d2h\("
    first_enqueue = min(m.start() for m in re.finditer(enqueue, run))
    checks = [m.start() for m in re.finditer(r"dev_span\(", run)]
    assert len(checks) == 6 and max(checks) < first_enqueue
    for name in ("u_dev, n.u", "body_dev, n.body", r"x_dev, n.out\[0\]", r"q_dev, n.out\[1\]", r"v_dev, n.out\[2\]", r"omega_dev, n.out\[3\]"):
        assert re.search(r"dev_span\(b->ctx, " + name, run), name
    assert max(checks) < run.index("dev_outputs_overlap(arrays, 6, 4)") < first_enqueue               # four outputs, against each other and the two inputs
    assert run.index("batch_rollout_args(") < run.index("ctx_bind(") < min(checks)
    assert "hipStreamSynchronize" not in run and "hipMemcpy" not in run                              # no copy of its own
    # the extents are the full n_ticks-fold ones
    args = src[src.index("static mgf_status batch_rollout_args("):src.index("static mgf_status batch_rollout_run(")]
    for line in ("bytes->u = 4 * T * (size_t)n_act;", "bytes->body = 4 * M;", "bytes->out[0] = 12 * T * M;", "bytes->out[1] = 16 * T * M;",
                 "bytes->out[2] = 12 * T * M;", "bytes->out[3] = 12 * T * M;"):
        assert line in args, line
    # the host form: one upload, the device core, one download
    host_form = src[src.index('extern "C" mgf_status mgf_batch_rollout('):]
    assert host_form.count("h2d(") == 1 and host_form.count("d2h(") == 1 and host_form.count("batch_rollout_run(") == 1
    assert host_form.index("h2d(") < host_form.index("batch_rollout_run(") < host_form.index("d2h(")
    # the core: the step's own launch train with a hook, the actuators' rig through the shared upload, "drive_launches" left alone
    core = src[src.index("static mgf_status batch_rollout_run("):src.index('extern "C" mgf_status mgf_batch_rollout_dev(')]
    assert core.index("batch_push(") < core.index('batch_rig_up(b, R, "actuator", 3)') < core.index("batch_step_run(b, dt, iters, n_ticks, stats, &H)")
    assert "d_launches" not in src and "<<<" not in src and "batch_single_parts(" not in src
    host = read("mgf_amd", "csrc", "host_batch.inc")
    train = host[host.index("static mgf_status batch_step_run("):host.index('extern "C" mgf_status mgf_batch_step(')]
    assert train.count("k_batch_rollout_act<") == 2 and train.count("k_batch_rollout_record<<<") == 1
    assert train.index("k_batch_rollout_act<") < train.index("batch_collide(") < train.index("k_batch_solve<<<") < train.index("k_batch_rollout_record<<<")
    assert train.index("hipMemsetAsync(b->d_done.p") < train.index("hipMemsetAsync(b->d_act.p") < train.index("for (uint32_t first = 0")
    step = host[host.index('extern "C" mgf_status mgf_batch_step('):]
    assert "batch_step_run(b, dt, iters, n_ticks, stats, nullptr)" in step[:step.index("\n}\n")]
    assert '"rollout_launches"' in host[host.index('extern "C" mgf_status mgf_batch_counter('):]
    # the kernels: the gate folded into the run length, one exit behind the loop; the record's world lane is the only writer of `act`
    k = read("mgf_amd", "csrc", "k_batch_rollout.h")
    body = k[k.index("void k_batch_rollout_act("):]
    body = body[:body.index("\n}\n")]
    assert "A.done[run.x] == A.tick && A.act[run.x] == A.tick" in body and "const uint32_t cnt = live ? run.w : 0u;" in body
    assert body.count("return;") == 1 and body.index("__any(j < cnt)") < body.index("if (j < cnt)") < body.index("if (!live) return;")
    assert "__syncthreads" not in body and "break" not in body and "continue" not in body and not re.search(r"A\.act\[[^\]]+\] =[^=]", body)
    assert re.findall(r"atomic\w*\(", body) == ["atomicAdd("]
    assert "lin + L * inv_mass" in body and "ang + I * T" in body and "lin + L;" in body and "ang + T;" in body
    rec = k[k.index("void k_batch_rollout_record("):]
    assert "A.done[lo] == t + 1u && A.act[lo] <= t + 1u" in rec and "if (gi >= A.total)" in rec
    assert len(re.findall(r"A\.act\[\w+\] = ", k)) == 1 and "A.act[i] = t + 1u;" in rec
    assert len(re.findall(r"__global__", k)) == 2 and not re.search(r"void k_batch_actuate", k)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_binding_turns_a_wrong_tensor_down_before_it_calls_c():
    import torch

    class Handle(mgf_amd.WorldBatch):   # no context, no C handle: a call that got as far as C would fail differently
        def __init__(self):
            self._h, self.n_worlds = None, 2

        def actuator_count(self):
            return 4

        def __len__(self):
            return 10

    b, n, T, m = Handle(), 4, 3, 5
    f = torch.float32
    wrong_u = [torch.zeros((T, n), dtype=torch.float64), torch.zeros((T, n), dtype=torch.int32), torch.zeros((T, 2 * n), dtype=f)[:, ::2],
               torch.zeros((T, n - 1), dtype=f), torch.zeros(T * n, dtype=f), torch.zeros((n, T), dtype=f).t()]
    for t in wrong_u:
        with pytest.raises(ValueError) as e:
            b.rollout_dev(t, 0.01, 4)
        assert "on cpu" not in str(e.value), str(e.value)              # turned down for what it is, not for where it is
    body = torch.zeros(m, dtype=torch.int32)
    for name, cols in (("x", 3), ("q", 4), ("v", 3), ("omega", 3)):
        wrong = [torch.zeros((T, m, cols), dtype=torch.float64), torch.zeros((T, m, cols + 1), dtype=f), torch.zeros((T + 1, m, cols), dtype=f),
                 torch.zeros((T, m + 1, cols), dtype=f), torch.zeros((T * m, cols), dtype=f), torch.zeros((T, cols, m), dtype=f).transpose(1, 2)]
        for t in wrong:
            with pytest.raises(ValueError) as e:
                _call(b, T, n, m, name, t)
            assert "on cpu" not in str(e.value), (name, str(e.value))
        with pytest.raises(ValueError, match="on cpu"):
            _call(b, T, n, m, name, torch.zeros((T, m, cols), dtype=f))
    with pytest.raises(ValueError, match="dtype"):
        _call(b, T, n, m, "x", None, body=torch.zeros(m, dtype=torch.int64))
    with pytest.raises(ValueError, match="on cpu"):                     # everything right but the device
        b.rollout_dev(torch.zeros((T, n), dtype=f), 0.01, 4)
    with pytest.raises(ValueError, match="required"):
        b.rollout_dev(None, 0.01, 4)
    with pytest.raises(ValueError, match="not ndarray"):
        b.rollout_dev(np.zeros((T, n), np.float32), 0.01, 4)
    with pytest.raises(ValueError, match="empty rig"):
        b.rollout_dev(T, 0.01, 4)
    # the host form: u is [T, n]; a trace is one of the four
    with pytest.raises(ValueError, match=r"is not \[T, 4\]"):
        b.rollout(np.zeros((T, n + 1), np.float32), 0.01, 4)
    with pytest.raises(ValueError, match="trace"):
        b.rollout(np.zeros((T, n), np.float32), 0.01, 4, trace=("x", "force"))
    with pytest.raises(mgf_amd.MgfError):                               # and a call whose arguments are all in order does reach C
        b.rollout(np.zeros((T, n), np.float32), 0.01, 4, body=[1, 2, 3])


class _Fake:
    """stands for a CUDA tensor in the binding's checks: what _dev_arg reads of one, the device aside"""

    def __init__(self, t):
        self._t = t
        self.dtype, self.shape, self.device = t.dtype, t.shape, t.device

    def data_ptr(self):
        return 1 << 22

    def is_contiguous(self):
        return self._t.is_contiguous()

    def numel(self):
        return self._t.numel()

    def dim(self):
        return self._t.dim()


def _call(b, T, n, m, name, t, body=None):
    """rollout_dev with a u and a body that pass every check of the binding, so that the tensor under test is reached"""
    import torch

    class Cuda(_Fake):
        def __init__(self, t):
            super().__init__(t)
            self.device = torch.device("cuda", 0)
    u = Cuda(torch.zeros((T, n), dtype=torch.float32))
    bd = Cuda(torch.zeros(m, dtype=torch.int32)) if body is None else body
    kw = {} if t is None else {name: t}
    return b.rollout_dev(u, 0.01, 4, body=bd, **kw)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_two_kernels_use_no_scratch_and_spill_nothing():
    if not os.path.exists(os.path.join(ROOT, "mgf_amd", "libmgf_hip.so")) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    rows = kernel_resources("k_batch_rollout")
    assert set(rows) == {"k_batch_rollout_act<0>", "k_batch_rollout_act<1>", "k_batch_rollout_record"}, sorted(rows)
    design = re.sub(r"\s+", " ", read("DESIGN.md"))
    for name, v in sorted(rows.items()):
        print(name, ": vgpr, sgpr, scratch, static lds, sgpr spills, vgpr spills =", v)
        assert v[2] == "0" and v[4] == "0" and v[5] == "0", (name, v)    # no scratch, no spills
        assert "`%s` %s / %s / 0 / 0 / 0" % (name, v[0], v[1]) in design, (name, v)
    assert len(kernel_resources("k_batch_actuate")) == 4                 # the actuators' four are the actuators' alone


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_late_contact_pair_touches_nothing_at_first_and_then_outgrows_a_share_of_one_record_a_body():
    """by the oracle: no constraint before tick FIRST_CONTACT in either world of the pair, then - within the T ticks of a rollout - more
    constraints in one tick than cons_per_body = 1 grants the world, and more than the default grants in none; the sparse world stays
    within its share throughout.  (The batch's constraint list is the oracle's, record for record: tests/test_gpu_world_batch.py.)"""
    scs = RC.late_contact_scenes()
    counts = []
    for sc in scs:
        w = oracle_world(sc)
        counts.append([int(w.step(float(sc["dt"]), sc["iters"]).n_constraints) for _ in range(RC.T)])
    lens = [len(sc["comps"]) for sc in scs]
    assert lens == [27, 18, 8] and all(8 <= n <= 27 for n in lens)
    firsts = []
    for k in (RC.LATE_A, RC.LATE_B):
        c = counts[k]
        first = next(t for t in range(RC.T) if c[t])
        firsts.append(first)
        assert RC.FIRST_CONTACT <= first < RC.T - 1, (k, c)
        assert max(c) > RC.share(lens[k], 1), (k, c)
        assert max(c) <= RC.share(lens[k], 4), (k, c)                     # the twin with the default never runs a tick again
    assert firsts[0] != firsts[1]                                         # the two worlds stall at different ticks
    assert max(counts[RC.SPARSE]) <= RC.share(lens[RC.SPARSE], 1), counts[RC.SPARSE]
    # the rig is weak, names bodies of every world and holds one control that is not finite
    rig, u, planted = RC.late_rig(lens)
    assert len(rig) == 70 and set(rig["world"].tolist()) == {0, 1, 2} and np.all(rig["body"] < np.int64(lens)[rig["world"]])
    assert set(rig["flags"].tolist()) == {0, 1, 2, 3} and np.all(np.abs(rig["gain"]) <= 0.05) and len(planted) == 1 and np.isnan(u[planted[0]])
    assert int(np.sum((rig["world"] == rig["world"][0]) & (rig["body"] == 4))) >= 1
    U = RC.controls(u, planted)
    assert U.shape == (RC.T, 70) and np.all(np.isnan(U[:, planted[0]])) and int(np.isnan(U).sum()) == RC.T
    body, outside = RC.traced(sum(lens), count=30)
    assert outside == 2 and int(np.sum((body < 0) | (body >= sum(lens)))) == 2 and len(set(body.tolist())) == len(body) - 1


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_actuators_kernel_and_host_file_are_as_they_were():
    """the walk is restated, not shared: k_batch_actuator.h still holds one __global__, host_batch_actuator.inc its four launches (what
    tests/test_world_batch_actuators_host.py asserts of them is run here again), and the restated lines are the original's"""
    from tests import test_world_batch_actuators_host as AH
    AH.test_both_pointers_are_looked_up_before_the_first_enqueue_and_the_kernel_has_one_exit()
    orig = read("mgf_amd", "csrc", "k_batch_actuator.h")
    mine = read("mgf_amd", "csrc", "k_batch_rollout.h")
    loop = orig[orig.index("      const float4 w0 = A.rig[3 * i]"):orig.index("      if (OUT)")]
    assert loop.replace("A.u[i]", "u[i]") in mine
    tail = orig[orig.index("      if (MODE == ACTUATE_IMPULSE) {\n        lin = lin + L * inv_mass;"):orig.index("  if (n_skip)")]
    assert tail in mine
