"""The joint rigs of a batch - ball joints, hinges, sliders - share one kernel skeleton (k_batch_joint_loop.h) and one set of host steps
(host_batch_joint.inc), as the observation rigs share host_batch_rig.inc (tests/test_world_batch_rigs_host.py).  Without a GPU: every
property of the shared code is asserted here once, against the shared code - the skeleton's gate, barriers, dataflow loop, bounded spin
and store-back; the host steps' order of refusals, context, pointer look-up and first enqueue; the train's order, its view per pass and
its row per tick; the messages, character for character what the three files said before they were one - and no per-rig file defines a
shared step or holds a copy.  What is a rig's own - its record checks, its rows, its entry points - is asserted in
tests/test_world_batch_joints_host.py, _hinges_host.py and _sliders_host.py."""
import re

import pytest

from tests.util import read

KINDS = {
    "joint": dict(kind="JointKind", rows="JointRows", kernel="k_batch_joint_solve", kfile="k_batch_joint.h", hfile="host_batch_joint.inc", member="joints", words=3, floats=3,
                  table="false", launches="MGF_BATCH_JOINT_LAUNCHES", per_tick="MGF_BATCH_ROLLOUT_JOINT_LAUNCHES_PER_TICK"),
    "hinge": dict(kind="HingeKind", rows="HingeRows", kernel="k_batch_hinge_solve", kfile="k_batch_hinge.h", hfile="host_batch_hinge.inc", member="hinges", words=7, floats=8,
                  table="true", launches="MGF_BATCH_HINGE_LAUNCHES", per_tick="MGF_BATCH_ROLLOUT_HINGE_LAUNCHES_PER_TICK"),
    "slider": dict(kind="SliderKind", rows="SliderRows", kernel="k_batch_slider_solve", kfile="k_batch_slider.h", hfile="host_batch_slider.inc", member="sliders", words=7, floats=8,
                   table="true", launches="MGF_BATCH_SLIDER_LAUNCHES", per_tick="MGF_BATCH_ROLLOUT_SLIDER_LAUNCHES_PER_TICK"),
}
SHARED_STEPS = ("batch_joint_plan", "batch_joint_other_check", "batch_joint_far_ends", "batch_joint_view", "batch_joint_ready", "batch_joint_run", "batch_joint_args",
                "batch_joint_solve", "batch_joint_solve_dev", "batch_joint_target_args", "batch_joint_targets", "batch_joint_hook", "batch_joint_pass", "batch_joint_tick")


def _code(text):
    """the text without its // comments"""
    return re.sub(r"//[^\n]*", "", text)


def _fn(src, name, ret=r"[\w:<> ]+"):
    """the definition of the shared step `name`: from its head to the closing brace in column 0"""
    m = re.search(r"(?:template <class \w+>\n)?static %s ?\b%s\([^;{]*\) \{\n" % (ret, name), src)
    assert m, name
    return src[m.start():src.index("\n}\n", m.end()) + 3]


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_skeleton_holds_the_gate_two_barriers_the_dataflow_loop_a_bounded_spin_and_the_store_back_once():
    k = read("mgf_amd", "csrc", "k_batch_joint_loop.h")
    assert "template <class Rows, bool GATED>\n__device__ __forceinline__ void batch_joint_loop(const BatchJointArgs& A) {" in k
    body = k[k.index("void batch_joint_loop("):]
    body = body[:body.index("\n}\n")]
    gate = "if (GATED && !(A.done[k] == A.tick && A.act[k] == A.tick)) return;"
    assert gate in body and body.index(gate) < body.index("__syncthreads()")                 # the workgroup's early return ahead of the first barrier
    assert body.count("__syncthreads()") == 2 and re.findall(r"atomic\w*\(", body.replace("__hip_atomic_load(", "").replace("__hip_atomic_store(", "")) == ["atomicAdd("]
    assert "atomicAdd(A.skipped, 1ull)" in body                                               # an integer count: no float atomic
    # the slot load and the plan's words, ahead of the first barrier; the setup is the Rows' and gives `skip`
    head = body[:body.index("__syncthreads()")]
    for word in ("s_dyn[2 * s] = srec[4 * (size_t)body];", "s_dyn[2 * s + 1] = srec[4 * (size_t)body + 1];", "s_prog[s] = 0u;", "if (tid == 0) s_fail = 0u;",
                 "sa = pl.y & 0xFFFFu; sb = pl.y >> 16;", "need_a = pl.z & 0xFFFFu; need_b = pl.z >> 16;", "has_b = sb != kJointNoSlot;", "deg_a = slot[sa].y;",
                 "if (has_b) deg_b = slot[sb].y;", "Rows R{};", "skip = R.setup(A, A.rig + Rows::kWords * (size_t)i, i, g0, has_b);", "if (skip) atomicAdd(A.skipped, 1ull);"):
        assert word in head, word
    loop = body[body.index("while (open)"):body.index("if (s_fail != 0u) return;")]
    assert body.count("while (") == 1 and "bool open = mine && A.iters != 0u;" in body
    assert loop.count("__ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP") == 2 and loop.count("__ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP") == 2   # both counters released once
    assert loop.count("__hip_atomic_load(") == 2 and loop.count("__hip_atomic_store(") == 2
    assert loop.index("if (!__any(ready)) __builtin_amdgcn_s_sleep(1);") < loop.index("if (ready) {") < loop.index("s_dyn[2 * sa] = ") < loop.index("__ATOMIC_RELEASE")
    assert k.count("s_sleep") == 1 + k[:k.index("#pragma once")].count("s_sleep") and loop.count("s_sleep") == 1
    # one unpack and one re-pack of the velocities around the rows of one turn
    assert loop.count("s_dyn[2 * sa] = ") == 1 and loop.count("= s_dyn[2 * sa]") == 1 and loop.count("s_dyn[2 * sb] = ") == 1 and loop.count("= s_dyn[2 * sb]") == 1
    assert loop.index("= s_dyn[2 * sa]") < loop.index("R.sweep(va, oa, vb, ob, has_b);") < loop.index("s_dyn[2 * sa] = ") and loop.count("R.sweep(") == 1
    assert "s_dyn[2 * sa + 1] = make_float4(oa.y, oa.z, a1.z, a1.w);" in loop and "s_dyn[2 * sb + 1] = make_float4(ob.y, ob.z, b1.z, b1.w);" in loop   # words 1's im and I_00 kept
    assert "++spins > kBatchSpinLimit" in loop and "A.err[1] = 1u;" in loop and "s_fail = 1u;" in loop and "A.err[0]" not in k
    assert "GATED" not in loop and "A.done" not in loop and "break" not in loop and "continue" not in loop and "return" not in loop
    back = body[body.index("if (s_fail != 0u) return;"):]
    assert body.index("if (s_fail != 0u) return;") > body.rindex("__syncthreads()")
    assert "srec[4 * (size_t)body] = s_dyn[2 * s];" in back and "srec[4 * (size_t)body + 1] = s_dyn[2 * s + 1];" in back and "+ 2]" not in back   # words 0 and 1 alone
    assert back.index("srec[4 * (size_t)body + 1]") < back.index("R.store(A.acc + Rows::kFloats * (size_t)i);") < back.index("if (A.out) R.store(A.out + Rows::kFloats * (size_t)i);")
    assert "__global__" not in k                                                               # no kernel: the three entry points stay in their files
    assert not re.search(r"A\.act\[[^\]]+\] =[^=]", k) and not re.search(r"A\.done\[[^\]]+\] =[^=]", k)
    assert "atan" not in k and "sinf" not in k and "cosf" not in k and "sqrt" not in k
    # one argument struct for the three, the target row null for the ball joints; one end load
    assert k.count("struct BatchJointArgs {") == 1 and "const float* w; " in k
    assert "__device__ __forceinline__ JointEnd joint_end(const Bodies& B, size_t g) {" in k and k.count("B.srec[4 * g") == 4 and k.count("B.delta[g]") == 1
    for name in ("k_batch_joint.h", "k_batch_hinge.h", "k_batch_slider.h", "k_batch_hinge_frame.h", "k_batch_joint_read.h", "k_batch_hinge_read.h", "k_batch_slider_read.h"):
        other = _code(read("mgf_amd", "csrc", name))
        if name == "k_batch_slider_read.h":   # (its one load is not an end's: the linear velocity, which JointEnd does not carry)
            own = "__device__ __forceinline__ V3 slider_read_v(const Bodies& B, size_t g) { return xyz(B.srec[4 * g]); }"
            assert other.count(own) == 1
            other = other.replace(own, "")
        assert "srec[" not in other and ".delta[" not in other and "B.q[" not in other, name     # nobody else loads an end
        assert "BatchHingeArgs" not in other and "BatchSliderArgs" not in other and "struct BatchJointArgs" not in other, name
    kernels = read("mgf_amd", "csrc", "kernels.h")
    assert kernels.index('#include "k_batch_spring.h"') < kernels.index('#include "k_batch_joint_loop.h"') < kernels.index('#include "k_batch_joint.h"')
    assert "batch_joint_loop<Rows, GATED> (k_batch_joint_loop.h)" in kernels
    design = read("DESIGN.md")
    sub = design[design.index("### The joint solvers' skeleton"):design.index("### Joints between bodies")]
    for word in ("batch_joint_loop<Rows, GATED>", "k_batch_joint_loop.h", "setup", "sweep", "store", "kWords", "kFloats", "JointKind", "HingeKind", "SliderKind", "host_batch_joint.inc",
                 "__any", "kBatchSpinLimit", "tools/check_lane_masks.py"):
        assert word in sub, word


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("word", sorted(KINDS))
def test_a_kernel_file_is_one_entry_point_over_its_rows_and_holds_no_copy_of_the_skeleton(word):
    K = KINDS[word]
    k = read("mgf_amd", "csrc", K["kfile"])
    code = _code(k)
    for copy in ("while (", "__hip_atomic_", "s_sleep", "__syncthreads", "__shared__", "s_dyn", "s_prog", "atomicAdd", "A.err", "A.done", "A.act", "A.plan", "A.slots", "A.items"):
        assert copy not in code, copy
    assert len(re.findall(r"__global__ __launch_bounds__\(kBatchBlock\)", k)) == len(re.findall(r"__global__", k)) == 1
    entry = "template <bool GATED>\n__global__ __launch_bounds__(kBatchBlock) void %s(BatchJointArgs A) {\n  batch_joint_loop<%s, GATED>(A);\n}\n" % (K["kernel"], K["rows"])
    assert entry in k                                                                         # the body is a single call of the skeleton
    rows = k[k.index("struct %s {" % K["rows"]):k.index("template <bool GATED>\n__global__")]
    assert "static constexpr uint32_t kWords = %d, kFloats = %d;" % (K["words"], K["floats"]) in rows
    for member in ("bool setup(const BatchJointArgs& A, const float4* rec, uint32_t", "void sweep(V3& va, V3& oa, V3& vb, V3& ob, bool has_b) {", "void store(float* p) const {"):
        assert "__device__ __forceinline__ " + member in rows, member
    assert len(re.findall(r"\n  (?:__device__|bool|void|V3|float)[^\n;]*\) (?:const )?\{", rows)) == rows.count("__device__ __forceinline__ ")   # every member is inlined
    assert "atan" not in k and "sinf" not in k and "cosf" not in k and "sqrt" not in k        # + - * / and comparisons
    assert '#include "k_batch_hinge_frame.h"' in read("mgf_amd", "csrc", "k_batch_hinge.h") and "keeps its own copy" not in read("mgf_amd", "csrc", "k_batch_hinge_frame.h")
    if word != "joint":                                                                       # the frame lines are hinge_frame's, the ends joint_ends'
        setup = rows[rows.index("bool setup("):rows.index("void sweep(")]
        assert setup.index("joint_ends(A.B, g0, w0, has_b, &a, &b);") < setup.index("hinge_frame(a, b, has_b, w1, w2, w3, w4, w5, w6);") and "rotate(" not in setup
        assert "joint_inv2(" in setup and " / " not in setup.replace("w1.w / A.h", "")       # the 2 x 2 inverse is the shared one


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_host_steps_are_written_once_and_no_rig_file_defines_one():
    src = read("mgf_amd", "csrc", "host_batch_joint.inc")
    shared = src[:src.index("struct JointKind {")]
    for name in SHARED_STEPS:
        assert len(re.findall(r"\nstatic [\w:<> ]+\b%s\(" % name, shared)) == 1, name
    for K in KINDS.values():
        own = read("mgf_amd", "csrc", K["hfile"])
        own = own[own.index("struct %s {" % K["kind"]):]
        assert not re.search(r"\nstatic |\ntemplate <class", own), K["hfile"]                  # behind the kind: nothing but the entry points
        for copy in ("<<<", "hipMemcpyAsync", "hipMemsetAsync", "hipStreamSynchronize", ".ensure(", "batch_rig_up(", "batch_push(", "ctx_bind(", "dev_span(", "gave_up", "R.recs[i].other"):
            assert copy not in own, (K["hfile"], copy)
        traits = own[:own.index("};") + 2]
        for line in ("using Rec = mgf_batch_%s;" % K["kind"][:-4].lower(), "using Rows = %s;" % K["rows"], 'static constexpr const char* word = "%s";' % K["kind"][:-4].lower(),
                     "static constexpr bool table = %s;" % K["table"], "launches = %s, per_tick = %s;" % (K["launches"], K["per_tick"]),
                     "mgf_batch::*rig = &mgf_batch::%s;" % K["member"], "static constexpr auto launch = %s<GATED>;" % K["kernel"]):
            assert line in traits, (K["kind"], line)
    hip = read("mgf_amd", "csrc", "mgf_hip.hip")
    assert hip.index('#include "host_batch_joint.inc"') < hip.index('#include "host_batch_hinge.inc"') < hip.index('#include "host_batch_slider.inc"')
    # the state: one type, one member a rig; the loose fields are gone
    host = read("mgf_amd", "csrc", "host_batch.inc")
    state = host[host.index("struct BatchJointRig : BatchRig<Rec> {"):host.index("struct mgf_batch {")]
    for field in ("DBuf<float> acc;", "DBuf<unsigned long long> skipped;", "DBuf<float> w;", "int64_t rows = 1;", "bool zero = true;"):
        assert field in state, field
    for K in KINDS.values():
        assert host.count("BatchJointRig<mgf_batch_%s> %s;" % (K["kind"][:-4].lower(), K["member"])) == 1
    every = "".join(read("mgf_amd", "csrc", f) for f in ("host_batch.inc", "host_batch_rollout.inc", "host_batch_joint.inc", "host_batch_hinge.inc", "host_batch_joint_read.inc",
                                                          "host_batch_slider.inc"))
    assert not re.search(r"\b(j_acc|j_skipped|hg_\w+|sg_\w+)\b", every) and "hinge_unit" not in every and "slider_unit" not in every and "slider_dot" not in every
    assert every.count("static bool joint_unit(double a) { return std::fabs(a - 1.0) <= 1e-3; }") == 1                  # one pair, in double on the host
    assert every.count("static double joint_dot(const mgf_vec3& a, const mgf_vec3& b) { return (double)a.x * b.x + (double)a.y * b.y + (double)a.z * b.z; }") == 1
    stale = host[host.index("static void batch_rigs_stale("):host.index('extern "C" mgf_status mgf_batch_add_bodies(')]
    counter = host[host.index('extern "C" mgf_status mgf_batch_counter('):]
    for K in KINDS.values():
        assert "b->%s.stale = true;" % K["member"] in stale
        assert 'if (!strcmp(name, "%s_skipped")) return batch_joint_skipped(b, b->%s, out);' % (K["member"], K["member"]) in counter
    skipped = _fn(host, "batch_joint_skipped")
    assert skipped.index("if (R.skipped.p)") < skipped.index("ctx_bind(") < skipped.index("d2h(b->ctx, &v, R.skipped.p, 1)") and host.count("batch_joint_skipped(const") == 1


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_shared_steps_keep_the_order_of_refusals_context_look_up_and_first_enqueue():
    src = read("mgf_amd", "csrc", "host_batch_joint.inc")
    # the plan: a stable sort by world, slots in the order of first mention, the rig changed at its end and nowhere else; no device
    plan = _fn(src, "batch_joint_plan", "void")
    assert "static void batch_joint_plan(BatchJointRig<Rec>& R, const Rec* recs, size_t n) {" in plan
    assert "std::stable_sort(" in plan and plan.index("std::stable_sort(") < plan.index("R.recs.assign(") < plan.index("R.stale = true;") < plan.index("R.rows = 1;") < plan.index("R.zero = true;")
    assert plan.index("const auto a = slot(r.body);") < plan.index("r.other >= 0 ? slot(r.other)")
    assert "plan[4 * p + 1] = a.first | (b.first << 16);" in plan and "plan[4 * p + 2] = a.second | (b.second << 16);" in plan
    assert not re.search(r"<<<|Async|hipMalloc|\.ensure\(|h2d\(", plan) and src.count("std::stable_sort(") == 1
    # the set call's far end, and the far ends again when the rig goes up behind added bodies
    other = _fn(src, "batch_joint_other_check")
    assert other.index("r.other < -1 || (r.other >= 0 && (uint32_t)r.other >= b->h_n[(size_t)r.world])") < other.index("r.other == r.body") and other.count("the rig was not changed") == 2
    assert not re.search(r"<<<|Async|hipMalloc|\.ensure\(|h2d\(|b->\*T::rig", other)
    ready = _fn(src, "batch_joint_ready")
    far = _fn(src, "batch_joint_far_ends")
    assert "if (R.stale)" in far and "(uint32_t)R.recs[i].other >= b->h_n[(size_t)R.recs[i].world]" in far
    assert ready.index("batch_joint_far_ends<T>(b)") < ready.index("batch_rig_up(b, R, T::word, 3)") < ready.index("if (T::table && R.zero) {") < ready.index("R.acc.ensure(T::Rows::kFloats * n, s)")
    assert src.count("batch_rig_up(b, R, ") == 1 and "hipMemsetAsync(R.w.p, 0, 4 * n, s)" in ready and "*lds = 36u * most;" in ready and "most = std::max(most, it.z >> 16)" in ready
    assert ready.index("memset(A, 0, sizeof(*A));") < ready.index("batch_joint_view<T>(b, A);") < ready.index("A->w = R.w.p;")
    view = _fn(src, "batch_joint_view", "void")
    for word in ("A->B = b->bodies(0);", "A->w_off = b->d_off.p;", "A->items = reinterpret_cast<const uint4*>(R.dev.p);", "A->rig = R.dev.p + R.off[1];",
                 "A->plan = reinterpret_cast<const uint4*>(R.dev.p + R.off[2]);", "A->slots = reinterpret_cast<const uint2*>(R.dev.p + R.off[2] + R.recs.size());",
                 "A->acc = R.acc.p;", "A->skipped = R.skipped.p;", "A->err = b->d_err.p;"):
        assert word in view, word
    # the target calls: the refusals, the context, (device form) the pointer looked up - and only then the copy; no wait in the device form
    targs = _fn(src, "batch_joint_target_args")
    torder = [targs.index(s) for s in ("batch_rig_handle(b)", "rows < 1 || rows > (1 << 20)", "!w && n > 0", "overflows int64_t")]
    assert torder == sorted(torder) and not re.search(r"<<<|Async|\.ensure\(|ctx_bind", targs)
    tg = _fn(src, "batch_joint_targets")
    order = [tg.index(s) for s in ("batch_joint_target_args<T>(b, w, rows)", "ctx_bind(b->ctx)", 'if (kind == hipMemcpyDeviceToDevice) MGF_TRY(dev_span(b->ctx, w, 4 * words, "w_dev"));',
                                   "R.w.ensure(words, s)", "hipMemcpyAsync(R.w.p, w, 4 * words, kind, s)", "R.rows = rows;", "R.zero = false;")]
    assert order == sorted(order) and tg.count("hipStreamSynchronize") == 1 and "if (kind == hipMemcpyHostToDevice) MGF_HIP_TRY(hipStreamSynchronize(s));" in tg
    # the solve calls: the refusals - h, iters, then the row - the context, (device form) the pointer looked up, and only then the first thing is enqueued
    args = _fn(src, "batch_joint_args")
    aorder = [args.index(s) for s in ("batch_rig_handle(b)", '"h is not finite"', '"iters is negative"', "row < 0 || row >= (b->*T::rig).rows", '"row is outside the target table"')]
    assert aorder == sorted(aorder)
    enqueue = r"batch_joint_run<|batch_joint_ready<|batch_rig_up\(|batch_push\(|hipMemsetAsync|hipMemcpyAsync|<<<|\.ensure\(|h2d\("
    dev = _fn(src, "batch_joint_solve_dev")
    first_enqueue = min(m.start() for m in re.finditer(enqueue, dev))
    assert (dev.index("batch_joint_args<T>(b, h, iters, row)") < dev.index("ctx_bind(") < dev.index('dev_span(b->ctx, impulse_out_dev, 4 * T::Rows::kFloats * n, "impulse_out_dev")')
            < dev.index("if (n == 0 || iters == 0) return MGF_OK;") < first_enqueue)
    assert "hipStreamSynchronize" not in dev and "hipMemcpy" not in dev
    host_form = _fn(src, "batch_joint_solve")
    assert host_form.count("hipStreamSynchronize") == 1 and "hipMemcpyHostToDevice" not in host_form      # one wait
    assert (host_form.index("batch_joint_args<T>(b, h, iters, row)") < host_form.index("ctx_bind(") < host_form.index("if (n == 0 || iters == 0) return MGF_OK;")
            < min(m.start() for m in re.finditer(enqueue, host_form)))
    assert host_form.index("batch_joint_run<T>(") < host_form.index("hipMemcpyAsync(&gave_up, b->d_err.p + 1, 4") < host_form.index("hipStreamSynchronize") < host_form.index("gave up waiting")
    assert "hipMemcpyAsync(impulse_out, R.acc.p, 4 * T::Rows::kFloats * n, hipMemcpyDeviceToHost, s)" in host_form
    run = _fn(src, "batch_joint_run")
    assert run.count("<<<") == 1 and run.index("batch_push(") < run.index("batch_joint_ready<T>(") < run.index("if (T::table) A.w = R.w.p + (size_t)row * R.recs.size();") < run.index("T::template launch<false><<<")
    assert "b->d_launches += T::launches;" in run and "batch_single_parts(" not in src                    # joints read no shapes
    assert src.count("<<<") == 2                                                                           # the call's launch and the train's


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_messages_built_from_a_kinds_word_are_the_ones_the_three_files_held():
    src = read("mgf_amd", "csrc", "host_batch_joint.inc")
    formats = re.findall(r'batch_joint_fail\(MGF_ERR_\w+, "([^"]*)", T::word\)', src)
    assert len(formats) == 5 and all(f.count("%") == 1 and "%s" in f for f in formats)
    assert "static mgf_status batch_joint_fail(mgf_status s, const char* fmt, const char* word) { set_error(fmt, word); return s; }" in src
    built = {f % w for f in formats for w in KINDS}
    held = set()
    for w in KINDS:   # what host_batch_joint.inc, host_batch_hinge.inc and host_batch_slider.inc said, each in its own words
        held |= {"a %s's other is neither -1 nor a body of its world: the rig was not changed" % w, "a %s's other is its body: the rig was not changed" % w,
                 "internal error: a %s's other is outside its world" % w, "internal error: a lane of the %s solver gave up waiting for its turn" % w,
                 "4 * rows * mgf_batch_%s_count overflows int64_t" % w}
    assert built == held
    for fixed in ('"h is not finite"', '"iters is negative"', '"row is outside the target table"', '"rows must be in [1, 2^20]"', '"NULL argument: w"'):
        assert src.count(fixed) == 1, fixed


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_train_solves_ball_joints_hinges_sliders_in_that_order_with_the_view_per_pass_and_the_row_per_tick():
    host = read("mgf_amd", "csrc", "host_batch.inc")
    roll = read("mgf_amd", "csrc", "host_batch_rollout.inc")
    src = read("mgf_amd", "csrc", "host_batch_joint.inc")
    hook = host[host.index("struct BatchJointHook {"):host.index("struct BatchRolloutHook {")]
    assert "BatchJointArgs A;" in hook and "uint32_t lds = 0;" in hook and "bool on = false;" in hook
    assert "BatchJointHook joints, hinges, sliders;" in host[host.index("struct BatchRolloutHook {"):]
    for gone in ("joint_lds", "hinge_lds", "slider_lds", "BatchHingeArgs", "BatchSliderArgs", "batch_hinge_view", "batch_slider_view", "batch_hinge_ready", "batch_slider_ready"):
        assert gone not in host and gone not in roll, gone
    # declared once as templates ahead of the train and of the rollout, defined behind them
    assert host.count("template <class T>\nstatic void batch_joint_pass(const mgf_batch* b, BatchJointHook& H);") == 1
    assert host.count("template <class T>\nstatic mgf_status batch_joint_tick(mgf_batch* b, BatchJointHook& H, uint32_t t, int64_t* launches);") == 1
    assert roll.count("template <class T>\nstatic mgf_status batch_joint_hook(mgf_batch* b, float h, int32_t iters, BatchJointHook* H);") == 1
    core = roll[roll.index("static mgf_status batch_rollout_run("):roll.index('extern "C" mgf_status mgf_batch_rollout_dev(')]
    calls = ["batch_joint_hook<%s>(b, dt, iters, &H.%s)" % (KINDS[w]["kind"], KINDS[w]["member"]) for w in ("joint", "hinge", "slider")]
    order = [core.index("batch_push(")] + [core.index(c) for c in calls] + [core.index("batch_step_run(b, dt, iters, n_ticks, stats, &H)")]
    assert order == sorted(order) and all(core.count(c) == 1 for c in calls)
    hk = _fn(src, "batch_joint_hook")
    assert hk.index("if ((b->*T::rig).recs.empty() || iters <= 0) return MGF_OK;") < hk.index("batch_joint_ready<T>(b, h, iters, nullptr, &H->A, &H->lds)") < hk.index("H->on = true;")
    train = host[host.index("static mgf_status batch_step_run("):host.index('extern "C" mgf_status mgf_batch_step(')]
    passes = ["batch_joint_pass<%s>(b, hook->%s);" % (KINDS[w]["kind"], KINDS[w]["member"]) for w in ("joint", "hinge", "slider")]
    ticks = ["MGF_TRY(batch_joint_tick<%s>(b, hook->%s, t, &hook->launches));" % (KINDS[w]["kind"], KINDS[w]["member"]) for w in ("joint", "hinge", "slider")]
    # what a kernel reads of the handle is looked up again for every pass: inside the loop over the passes, ahead of the loop over the ticks
    order = [train.index("for (uint32_t first = 0, pass = 0;")] + [train.index(p) for p in passes] + [train.index("for (uint32_t t = first; t < NT; ++t)")]
    assert order == sorted(order) and all(train.count(p) == 1 for p in passes)
    # the launches: behind the springs and the actuation, ahead of the tick, each once
    order = [train.index("k_batch_spring_apply<true><<<"), train.index("k_batch_rollout_act<")] + [train.index(t) for t in ticks] + [train.index("batch_collide(")]
    assert order == sorted(order) and all(train.count(t) == 1 for t in ticks)
    assert not re.search(r"k_batch_(joint|hinge|slider)_solve<", train)                        # the train launches them through the helper alone
    ps = _fn(src, "batch_joint_pass", "void")
    assert ps.index("if (!H.on) return;") < ps.index("batch_joint_view<T>(b, &H.A);") < ps.index("H.A.done = b->d_done.p; H.A.act = b->d_act.p;")
    tk = _fn(src, "batch_joint_tick")
    order = [tk.index(s) for s in ("if (!H.on) return MGF_OK;", "H.A.tick = t;", "if (T::table) H.A.w = R.w.p + (size_t)std::min<int64_t>((int64_t)t, R.rows - 1) * R.recs.size();",
                                   "T::template launch<true><<<(unsigned)R.items.size(), kBatchBlock, H.lds, b->ctx->stream>>>(H.A);", "LAUNCH_CHECK();", "*launches += T::per_tick;")]
    assert order == sorted(order) and tk.count("<<<") == 1                                      # tick t reads row min(t, rows - 1); counted once
    # a give-up is the second error word, read back with the first, and its message is as it was
    assert "d2h(ctx, err, b->d_err.p, 2)" in train and 'if (err[1]) return fail(MGF_ERR_HIP, "internal error: a lane of the joint solver gave up waiting for its turn");' in train
    assert not re.search(r"\.done\[[^\]]+\] =[^=]|\.act\[[^\]]+\] =[^=]", src)                  # `done` and `act` are the train's to fill, per tick
    step = host[host.index('extern "C" mgf_status mgf_batch_step('):host.index('extern "C" mgf_status mgf_batch_read_constraints(')]
    assert "batch_step_run(b, dt, iters, n_ticks, stats, nullptr)" in step and not re.search(r"joint|hinge|slider", step)   # mgf_batch_step applies none of them
