"""The encoders of a batch - the hinges', the sliders' - share one kernel skeleton (k_batch_joint_read.h) and one set of host steps
(host_batch_joint_read.inc), as the joint solvers share theirs (tests/test_world_batch_joint_family_host.py).  Without a GPU: every
property of the shared code is asserted here once, against the shared code - the skeleton's bounds test, the lane's gate ahead of every
load, the one load of the ends and the frames, the stores per format; the host steps' order of refusals, context, pointer look-up and
first enqueue; the train's site, its view per pass, its row per tick without a clamp; the messages, character for character what the two
files said before they were one - and no kernel file or rig file defines a shared step or holds a copy.  What is a kind's own - its
record, its arithmetic, its bounds, its compiler output, its binding - is asserted in tests/test_world_batch_hinge_read_host.py and
_slider_read_host.py."""
import os
import re

import pytest

from tests.util import ROOT, read

KINDS = {
    "hinge": dict(kind="HingeKind", reading="HingeReading", kernel="k_batch_read_hinges", kfile="k_batch_hinge_read.h", hfile="host_batch_hinge.inc", member="hinges",
                  caps="HINGE", rec="mgf_hinge_reading"),
    "slider": dict(kind="SliderKind", reading="SliderReading", kernel="k_batch_read_sliders", kfile="k_batch_slider_read.h", hfile="host_batch_slider.inc", member="sliders",
                   caps="SLIDER", rec="mgf_slider_reading"),
}
SHARED_STEPS = ("batch_joint_read_view", "batch_joint_read_ready", "batch_joint_read_run", "batch_joint_read_args", "batch_dev_span16", "batch_joint_read", "batch_joint_read_dev",
                "batch_joint_trace_entry", "batch_joint_set_trace", "batch_joint_trace_rows", "batch_joint_trace_args", "batch_joint_get_trace", "batch_joint_get_trace_dev",
                "batch_joint_read_hook", "batch_joint_read_pass", "batch_joint_read_tick")
READ_FILE = "host_batch_joint_read.inc"
GATE = "if (GATED && !(A.done[k] == A.tick + 1u && A.act[k] <= A.tick + 1u)) return;"
ENQUEUE = r"batch_joint_read_run<|batch_joint_read_ready<|batch_rig_up\(|batch_push\(|hipMemsetAsync|hipMemcpyAsync|<<<|\.ensure\(|h2d\(|hipFree\("


def _code(text):
    """the text without its // comments"""
    return re.sub(r"//[^\n]*", "", text)


def _fn(src, name, ret=r"[\w:<> ]+"):
    """the definition of the shared step `name`: from its head to the closing brace in column 0, or to the end of a one-line body"""
    m = re.search(r"(?:template <class \w+>\n)?static %s ?\b%s\([^;{]*\) \{" % (ret, name), src)
    assert m, name
    if src[m.end()] != "\n":
        return src[m.start():src.index("\n", m.end()) + 1]
    return src[m.start():src.index("\n}\n", m.end()) + 3]


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_skeleton_holds_the_bounds_test_the_lanes_gate_ahead_of_every_load_one_load_of_the_ends_and_the_stores_per_format():
    k = read("mgf_amd", "csrc", "k_batch_joint_read.h")
    assert "template <class Reading, bool GATED, int FORMAT>\n__device__ __forceinline__ void batch_joint_read(const BatchJointReadArgs& A) {" in k
    body = k[k.index("void batch_joint_read("):]
    body = body[:body.index("\n}\n")]
    assert GATE in body
    for load in ("joint_ends(", "rec[1]", "A.w_off[", "A.acc[", "hinge_frame(", "Reading::load(", "Reading::form("):     # the gate ahead of every load of state - a kind's own loads are in its load step
        assert body.index(GATE) < body.index(load), load
    assert body.index("const uint32_t i = blockIdx.x * kBatchBlock + threadIdx.x;") < body.index("if (i >= A.n) return;") < body.index("rec[0]") < body.index("f2u(w0.x)") < body.index(GATE)
    assert "const float4* rec = A.rig + 7 * (size_t)i;" in body and "const float4 w1 = rec[1], w2 = rec[2], w3 = rec[3], w4 = rec[4], w5 = rec[5], w6 = rec[6];" in body
    assert "const size_t g0 = A.w_off[k];" in body and "const bool has_b = f2u(w0.z) != 0xFFFFFFFFu;" in body
    order = [body.index(s) for s in ("joint_ends(A.B, g0, w0, has_b, &a, &b);", "const HingeFrame F = hinge_frame(a, b, has_b, w1, w2, w3, w4, w5, w6);",
                                     "const JointReadWords r = Reading::form(own, w0, w3, w4, w5, a, b, F);", "float4* o = A.out")]
    assert order == sorted(order) and body.count("joint_ends(") == 1 and body.count("hinge_frame(") == 1 and body.count("Reading::") == 3
    # a kind's own loads are issued beside the ends', ahead of the frames' arithmetic: where both kernels had them before they were one
    assert body.index("joint_ends(") < body.index("const typename Reading::Own own = Reading::load(A.B, g0, w0, has_b);") < body.index("hinge_frame(")
    assert not re.search(r"atomic|__shared__|__syncthreads|s_dyn|A\.plan|A\.slots|A\.items| / |A\.h\b", body)    # no plan, no LDS, no atomic, no barrier, no division, no h
    assert not re.search(r"A\.B\.\w+\[[^\]]*\] =[^=]|srec\[[^\]]*\] =[^=]", k)                                   # nothing written but the output
    assert "rotate(" not in body and "cross(" not in body and "dot(" not in body and "srec[" not in _code(k)     # no arithmetic of a kind, no load of an end of its own
    # the stores: two words, four where the entry carries the impulses or their zeros; each FORMAT branch once
    stores = re.findall(r"\bo\[\d\] = ", body)
    assert stores == ["o[0] = ", "o[1] = ", "o[2] = ", "o[3] = ", "o[2] = ", "o[3] = "]
    assert "float4* o = A.out + (FORMAT == kJointReadReading ? 2 : 4) * (size_t)i;" in body and "o[0] = r.lo;" in body and "o[1] = r.hi;" in body
    assert body.count("FORMAT == kJointReadFull)") == 1 and body.count("FORMAT == kJointReadFullZero)") == 1
    assert "o[2] = A.acc[2 * (size_t)i];" in body and "o[3] = A.acc[2 * (size_t)i + 1];" in body and body.count("make_float4(0.0f, 0.0f, 0.0f, 0.0f)") == 2
    assert "__global__" not in k                                                               # no kernel: the two entry points stay in their files
    assert "atan" not in k and "sinf" not in k and "cosf" not in k and "sqrt" not in k
    # one argument struct and one set of format constants for both
    assert k.count("struct BatchJointReadArgs {") == 1 and "constexpr int kJointReadReading = 0, kJointReadFull = 1, kJointReadFullZero = 2;" in k
    args = k[k.index("struct BatchJointReadArgs {"):k.index("template <class Reading")]
    for field in ("Bodies B;", "const uint32_t* w_off;", "const float4* rig;", "const float4* acc;", "float4* out;", "const uint32_t* done;", "const uint32_t* act;", "uint32_t n, tick;"):
        assert field in args, field
    assert '#include "k_batch_hinge_frame.h"' in k
    frame = read("mgf_amd", "csrc", "k_batch_hinge_frame.h")
    for fn in ("HingeFrame hinge_frame(", "float hinge_side("):
        assert "__device__ __forceinline__ " + fn in frame, fn
    assert "__device__ __forceinline__ JointEnd joint_end(" in read("mgf_amd", "csrc", "k_batch_joint_loop.h") and "srec[" not in frame
    assert "F.T2 = cross(F.A, F.T1);" in frame and "F.C = Pb - Pa;" in frame and "cphi <= ch" in frame and "__global__" not in frame
    kernels = read("mgf_amd", "csrc", "kernels.h")
    order = [kernels.index('#include "%s"' % f) for f in ("k_batch_hinge.h", "k_batch_slider.h", "k_batch_joint_read.h", "k_batch_hinge_read.h", "k_batch_slider_read.h", "k_batch_part_query.h")]
    assert order == sorted(order) and "batch_joint_read<Reading, GATED, FORMAT> (k_batch_joint_read.h" in kernels
    design = read("DESIGN.md")
    assert design.index("### The joint solvers' skeleton") < design.index("### The encoders' skeleton") < design.index("### Joints between bodies")
    sub = design[design.index("### The encoders' skeleton"):design.index("### Joints between bodies")]
    for word in ("batch_joint_read<Reading, GATED, FORMAT>", "k_batch_joint_read.h", "BatchJointReadArgs", "HingeReading", "SliderReading", "Reading::load", "form", "kJointReadFullZero", "HingeKind",
                 "SliderKind", "host_batch_joint_read.inc", "BatchJointTrace", "BatchJointReadHook", "done[k] == t + 1 && act[k] <= t + 1", "tools/check_lane_masks.py",
                 "tests/test_world_batch_encoder_family_host.py"):
        assert word in sub, word


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("word", sorted(KINDS))
def test_a_kernel_file_is_one_entry_point_of_one_call_over_its_reading_and_holds_no_copy_of_the_skeleton(word):
    K = KINDS[word]
    k = read("mgf_amd", "csrc", K["kfile"])
    code = _code(k[k.index("#pragma once"):])
    for copy in ("A.done", "A.act", "A.tick", " rec[", "A.rig", "A.w_off", "A.acc", "A.out", "A.n", "o[", "blockIdx", "threadIdx", "FORMAT ==", "joint_ends(", "hinge_frame(", "kJointRead",
                 "struct BatchJointReadArgs", "atomic", "__shared__", "__syncthreads", " / "):
        assert copy not in code, copy
    assert len(re.findall(r"__global__ __launch_bounds__\(kBatchBlock\)", k)) == len(re.findall(r"__global__", k)) == 1
    entry = "template <bool GATED, int FORMAT>\n__global__ __launch_bounds__(kBatchBlock) void %s(BatchJointReadArgs A) {\n  batch_joint_read<%s, GATED, FORMAT>(A);\n}\n" % (K["kernel"], K["reading"])
    assert entry in k                                                                         # the body is a single call of the skeleton
    reading = k[k.index("struct %s {" % K["reading"]):k.index("template <bool GATED, int FORMAT>\n__global__")]
    assert reading.count("__device__ __forceinline__ static JointReadWords form(Own") == 1 and reading.count("return {make_float4(") == 1
    assert reading.count("struct Own {") == 1 and reading.count("__device__ __forceinline__ static Own load(const Bodies&") == 1 and reading.count("__device__") == 2
    assert '#include "k_batch_joint_read.h"' in k and "rotate(" not in code
    assert not re.search(r"A\.B\.\w+\[[^\]]*\] =[^=]|srec\[[^\]]*\] =[^=]", k)                 # nothing written at all: the stores are the skeleton's
    assert not re.search(r"k_batch_\w+_solve|void k_batch_slider|void k_batch_hinge|void k_batch_joint", code)      # (the solvers' kernels are selected by those substrings)
    assert "atan" not in code and "sinf" not in code and "cosf" not in code and "sqrt" not in code
    if word == "hinge":
        assert "srec[" not in code and "B." not in reading.replace("F.B", "")                # the hinge's reading loads nothing of its own
    else:   # the slider's two loads of v - srec word 0 - are in its load step, which the skeleton calls behind the gate
        form = reading[reading.index("static JointReadWords form("):]
        assert "slider_read_v(" not in form and "B." not in form.replace("F.B", "")           # its form loads nothing
        assert code.count("srec[") == 1 and "__device__ __forceinline__ V3 slider_read_v(const Bodies& B, size_t g) { return xyz(B.srec[4 * g]); }" in k
        assert code.count("slider_read_v(") == 3 and reading.count("slider_read_v(") == 2
    # nobody but joint_end loads an end (tests/test_world_batch_joint_family_host.py holds the same of these files)
    assert ".delta[" not in code and "B.q[" not in code and "B.x[" not in code


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_host_steps_are_written_once_and_no_rig_file_defines_one():
    src = read("mgf_amd", "csrc", READ_FILE)
    shared = src[:src.index('extern "C"')]
    for name in SHARED_STEPS:
        assert len(re.findall(r"\nstatic [\w:<> ]+\b%s\(" % name, shared)) == 1, name
    entries = src[src.index('extern "C"'):]
    assert not re.search(r"\nstatic |\ntemplate <class", entries)                              # behind the steps: nothing but the entry points
    for copy in ("<<<", "hipMemcpyAsync", "hipMemsetAsync", "hipStreamSynchronize", ".ensure(", "batch_rig_up(", "batch_push(", "ctx_bind(", "dev_span(", "fail("):
        assert copy not in entries, copy
    for w, K in KINDS.items():                                                                 # the twelve entry points: one call each
        for head, call in (("mgf_status mgf_batch_read_%ss(mgf_batch* b, %s* out)" % (w, K["rec"]), "batch_joint_read<%s>(b, out)" % K["kind"]),
                           ("mgf_status mgf_batch_read_%ss_dev(mgf_batch* b, %s* out_dev)" % (w, K["rec"]), "batch_joint_read_dev<%s>(b, out_dev)" % K["kind"]),
                           ("mgf_status mgf_batch_set_%s_trace(mgf_batch* b, int64_t rows, int32_t format)" % w, "batch_joint_set_trace<%s>(b, rows, format)" % K["kind"]),
                           ("int64_t mgf_batch_%s_trace_rows(const mgf_batch* b)" % w, "batch_joint_trace_rows<%s>(b)" % K["kind"]),
                           ("mgf_status mgf_batch_get_%s_trace(mgf_batch* b, void* out, int64_t row0, int64_t n_rows)" % w, "batch_joint_get_trace<%s>(b, out, row0, n_rows)" % K["kind"]),
                           ("mgf_status mgf_batch_get_%s_trace_dev(mgf_batch* b, void* out_dev, int64_t row0, int64_t n_rows)" % w,
                            "batch_joint_get_trace_dev<%s>(b, out_dev, row0, n_rows)" % K["kind"])):
            assert re.search(r'extern "C" %s \{\s*return %s;\s*\}' % (re.escape(head), re.escape(call)), entries), head
    assert entries.count('extern "C"') == 12
    for w, K in KINDS.items():
        own = read("mgf_amd", "csrc", K["hfile"])
        assert "batch_joint_read" not in _code(own) and "trace_args" not in own and "dev_span" not in own
        traits = own[own.index("struct %s {" % K["kind"]):]
        traits = traits[:traits.index("};") + 2]
        for line in ("using Reading = %s;" % K["rec"], "static constexpr BatchJointTrace mgf_batch::*trace = &mgf_batch::%s_trace;" % w,
                     'static constexpr const char* caps = "%s";' % K["caps"],
                     "read_launches = MGF_BATCH_%s_READ_LAUNCHES, read_per_tick = MGF_BATCH_ROLLOUT_%s_READ_LAUNCHES_PER_TICK;" % (K["caps"], K["caps"]),
                     "trace_reading = MGF_%s_TRACE_READING, trace_full = MGF_%s_TRACE_FULL;" % (K["caps"], K["caps"]),
                     "template <bool GATED, int FORMAT>\n  static constexpr auto read = %s<GATED, FORMAT>;" % K["kernel"]):
            assert line in traits, (K["kind"], line)
    ball = read("mgf_amd", "csrc", "host_batch_joint.inc")
    ball = ball[ball.index("struct JointKind {"):]
    assert "Reading" not in ball[:ball.index("};")] and "read" not in ball[:ball.index("};")]     # the ball joints have no encoder
    hip = read("mgf_amd", "csrc", "mgf_hip.hip")
    assert hip.index('#include "host_batch_hinge.inc"') < hip.index('#include "host_batch_slider.inc"') < hip.index('#include "%s"' % READ_FILE) < hip.index('#include "host_batch_trace.inc"')
    for gone in ("host_batch_hinge_read.inc", "host_batch_slider_read.inc"):
        assert gone not in hip and not os.path.exists(os.path.join(ROOT, "mgf_amd", "csrc", gone)), gone
    # the state: one small struct, two members of the handle; the hook: one struct, two members; the loose fields are gone
    host = read("mgf_amd", "csrc", "host_batch.inc")
    state = host[host.index("struct BatchJointTrace {"):host.index("struct mgf_batch {")]
    for field in ("DBuf<float4> tab;", "int64_t rows = 0;", "int32_t format = 0;", "DBuf<float4> out;"):
        assert state.count(field) == 1, field
    assert host.count("BatchJointTrace hinge_trace, slider_trace;") == 1 and host.count("BatchJointTrace ") == 2       # the struct and its two members of the handle
    hook = host[host.index("struct BatchJointReadHook {"):host.index("struct BatchRolloutHook {")]
    assert "BatchJointReadArgs A;" in hook and "int32_t format = -1;" in hook
    assert host[host.index("struct BatchRolloutHook {"):].count("BatchJointReadHook hinge_read, slider_read;") == 1
    csrc = os.path.join(ROOT, "mgf_amd", "csrc")
    every = "".join(_code(read("mgf_amd", "csrc", f)) for f in sorted(os.listdir(csrc)) if f.endswith((".h", ".inc", ".hip")))
    every += re.sub(r"#[^\n]*", "", read("mgf_amd", "_capi.py"))
    assert not re.search(r"\b(ht_\w+|st_tab|st_rows|st_format|st_out|BatchHingeReadArgs|BatchSliderReadArgs|kHingeRead\w*|kSliderRead\w*|batch_hinge_dev_span)\b", every)
    assert not re.search(r"(?<!mgf_)batch_(hinge|slider)_(read|trace)_\w+|(hinge|slider)_trace_entry", every)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_shared_steps_keep_the_order_of_refusals_context_look_up_and_first_enqueue():
    src = read("mgf_amd", "csrc", READ_FILE)
    # the read calls: the refusals, the context, (device form) the pointer looked up - and only then the first thing is enqueued
    args = _fn(src, "batch_joint_read_args")
    assert args.index("batch_rig_handle(b)") < args.index("!out && !(b->*T::rig).recs.empty()") and not re.search(ENQUEUE, args)
    host_form = _fn(src, "batch_joint_read")
    first = min(m.start() for m in re.finditer(ENQUEUE, host_form))
    assert host_form.index("batch_joint_read_args<T>(b, out)") < host_form.index("ctx_bind(") < host_form.index("b->d_launches = 0;") < host_form.index("if (n == 0) return MGF_OK;") < first
    assert host_form.count("hipStreamSynchronize") == 1 and host_form.count("hipMemcpyAsync") == 1 and "hipMemcpyHostToDevice" not in host_form   # one download, one wait
    assert (host_form.index("DBuf<float4>& stage = (b->*T::trace).out;") < host_form.index("stage.ensure(2 * n, s)") < host_form.index("batch_joint_read_run<T>(b, stage.p)")
            < host_form.index("hipMemcpyAsync(out, stage.p, 32 * n, hipMemcpyDeviceToHost, s)"))
    dev = _fn(src, "batch_joint_read_dev")
    first = min(m.start() for m in re.finditer(ENQUEUE, dev))
    assert dev.index("batch_joint_read_args<T>(b, out_dev)") < dev.index("ctx_bind(") < dev.index("b->d_launches = 0;") < dev.index('batch_dev_span16(b, out_dev, 32 * n, "out_dev")') < first
    assert dev.index("if (n == 0) return MGF_OK;") < first and "hipStreamSynchronize" not in dev and "hipMemcpy" not in dev     # the device form waits for nothing
    span = _fn(src, "batch_dev_span16")
    assert span.index("dev_span(b->ctx, p, bytes, what)") < span.index("& 15u") and "hinge" not in span
    # pending host-side state goes up first, by the path the solve uses; one launch, counted where the solve counts its own
    run = _fn(src, "batch_joint_read_run")
    assert run.count("<<<") == 1 and run.index("batch_push(") < run.index("batch_joint_read_ready<T>(") < run.index("T::template read<false, kJointReadReading><<<")
    assert "b->d_launches += T::read_launches;" in run and "batch_single_parts(" not in src and src.count("<<<") == 4      # a reading reads no shapes; the call's launch and the tick's three
    assert src.count("b->d_launches = 0;") == 2 and _code(src).count("b->d_launches") == 3
    ready = _fn(src, "batch_joint_read_ready")
    order = [ready.index(s) for s in ("batch_joint_far_ends<T>(b)", "batch_rig_up(b, R, T::word, 3)", "R.acc.ensure(8 * n, b->ctx->stream)",
                                      "static_assert(sizeof(typename T::Reading) == 32 && sizeof(float4) == 16", "memset(A, 0, sizeof(*A));", "batch_joint_read_view<T>(b, A)")]
    assert order == sorted(order)                                                              # (the joint rigs' check of the far ends: `other` against the lengths that go up)
    assert "(uint32_t)R.recs[i].other >= b->h_n[(size_t)R.recs[i].world]" in read("mgf_amd", "csrc", "host_batch_joint.inc")
    view = _fn(src, "batch_joint_read_view", "void")
    for word in ("A->B = b->bodies(0);", "A->w_off = b->d_off.p;", "A->rig = R.dev.p + R.off[1];", "A->acc = reinterpret_cast<const float4*>(R.acc.p);", "A->n = (uint32_t)R.recs.size();"):
        assert word in view, word
    # the table: the refusals in the header's order, ahead of the context and of everything that changes the table
    st = _fn(src, "batch_joint_set_trace")
    order = [st.index(s) for s in ("batch_rig_handle(b)", "rows < 0 || rows > (1 << 20)", "format != T::trace_reading && format != T::trace_full", "overflows int64_t", "ctx_bind(",
                                   "R.tab.ensure(words, s)", "hipMemsetAsync(R.tab.p, 0, 16 * words, s)", "R.rows = rows;", "R.format = format;")]
    assert order == sorted(order) and min(m.start() for m in re.finditer(ENQUEUE, st)) > st.index("ctx_bind(")
    assert "(uint64_t)n > (uint64_t)INT64_MAX / 64u / (uint64_t)rows" in st and "(batch_joint_trace_entry<T>(format) / 16u)" in st
    assert "} else if (rows == 0 && R.tab.p) {" in st and st.index("hipStreamSynchronize(s)") < st.index("hipFree(R.tab.p)") < st.index("R.tab.p = nullptr;") and "BatchJointTrace& R = b->*T::trace;" in st   # rows == 0 frees it, behind the stream
    assert "return format == T::trace_full ? 64u : 32u;" in _fn(src, "batch_joint_trace_entry", "size_t")
    assert "return b ? (b->*T::trace).rows : -1;" in _fn(src, "batch_joint_trace_rows", "int64_t")
    ta = _fn(src, "batch_joint_trace_args")
    order = [ta.index(s) for s in ("batch_rig_handle(b)", "row0 < 0", "n_rows < 0", "row0 > R.rows || n_rows > R.rows - row0", "*bytes && !out")]
    assert order == sorted(order) and not re.search(ENQUEUE, ta) and "(b->*T::rig).recs.size() * batch_joint_trace_entry<T>(R.format)" in ta
    get = _fn(src, "batch_joint_get_trace")
    assert get.index("batch_joint_trace_args<T>(") < get.index("ctx_bind(") < get.index("if (bytes == 0) return MGF_OK;") < get.index("hipMemcpyAsync(")
    assert get.count("hipStreamSynchronize") == 1 and "hipMemcpyDeviceToHost" in get and get.count("hipMemcpyAsync") == 1
    gdev = _fn(src, "batch_joint_get_trace_dev")
    assert gdev.index("batch_joint_trace_args<T>(") < gdev.index("ctx_bind(") < gdev.index('dev_span(b->ctx, out_dev, bytes, "out_dev")') < gdev.index("if (bytes == 0) return MGF_OK;") < gdev.index("hipMemcpyAsync(")
    assert "hipStreamSynchronize" not in gdev and "hipMemcpyDeviceToDevice" in gdev
    # a rollout never clears the table: nothing but the set call changes it, and nothing outside this file and the two set calls names it
    assert src.count("hipMemsetAsync") == 1 and src.count("hipFree(") == 1 and src.count("R.rows = ") == 1 and src.count("BatchJointTrace& R") == 4      # one of the four not const
    for f in ("host_batch.inc", "host_batch_rollout.inc", "host_batch_joint.inc"):
        assert not re.search(r"T::trace|\b(hinge|slider)_trace\.", _code(read("mgf_amd", "csrc", f))), f


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_messages_are_the_ones_the_two_files_held():
    src = read("mgf_amd", "csrc", READ_FILE)
    assert src.count('set_error("format is neither MGF_%s_TRACE_READING nor MGF_%s_TRACE_FULL", T::caps, T::caps);') == 1
    assert src.count('batch_joint_fail(MGF_ERR_INVALID, "64 * rows * mgf_batch_%s_count overflows int64_t", T::word)') == 1
    built = set()
    for w, K in KINDS.items():
        built |= {"format is neither MGF_%s_TRACE_READING nor MGF_%s_TRACE_FULL" % (K["caps"], K["caps"]), "64 * rows * mgf_batch_%s_count overflows int64_t" % w}
        own = read("mgf_amd", "csrc", K["hfile"])
        assert 'static constexpr const char* word = "%s";' % w in own and 'static constexpr const char* caps = "%s";' % K["caps"] in own
    assert built == {"format is neither MGF_HINGE_TRACE_READING nor MGF_HINGE_TRACE_FULL", "format is neither MGF_SLIDER_TRACE_READING nor MGF_SLIDER_TRACE_FULL",
                     "64 * rows * mgf_batch_hinge_count overflows int64_t", "64 * rows * mgf_batch_slider_count overflows int64_t"}
    for fixed, n in (('"NULL argument: out"', 2), ('"rows must be in [0, 2^20]"', 1), ('"row0 is negative"', 1), ('"n_rows is negative"', 1),
                     ('"row0 + n_rows is beyond the readings table"', 1), ('"%s is not aligned to 16 bytes"', 1)):
        assert src.count(fixed) == n, fixed
    assert "static mgf_status batch_joint_fail(mgf_status s, const char* fmt, const char* word) { set_error(fmt, word); return s; }" in read("mgf_amd", "csrc", "host_batch_joint.inc")


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_train_reads_hinges_then_sliders_behind_the_record_with_the_view_per_pass_and_row_t_without_a_clamp():
    host = read("mgf_amd", "csrc", "host_batch.inc")
    roll = read("mgf_amd", "csrc", "host_batch_rollout.inc")
    src = read("mgf_amd", "csrc", READ_FILE)
    # declared once as templates ahead of the train and of the rollout, defined behind them
    assert host.count("template <class T>\nstatic void batch_joint_read_pass(const mgf_batch* b, BatchJointReadHook& H);") == 1
    assert host.count("template <class T>\nstatic mgf_status batch_joint_read_tick(mgf_batch* b, BatchJointReadHook& H, uint32_t t, int64_t* launches);") == 1
    assert roll.count("template <class T>\nstatic mgf_status batch_joint_read_hook(mgf_batch* b, int32_t iters, BatchJointReadHook* H);") == 1
    # armed by one helper called twice, behind the solvers' hooks and ahead of the train
    core = roll[roll.index("static mgf_status batch_rollout_run("):roll.index('extern "C" mgf_status mgf_batch_rollout_dev(')]
    arms = ["batch_joint_read_hook<%s>(b, iters, &H.%s_read)" % (KINDS[w]["kind"], w) for w in ("hinge", "slider")]
    order = [core.index("batch_push("), core.index("batch_joint_hook<HingeKind>("), core.index("batch_joint_hook<SliderKind>(")] + [core.index(a) for a in arms] + \
            [core.index("batch_step_run(b, dt, iters, n_ticks, stats, &H)")]
    assert order == sorted(order) and all(core.count(a) == 1 for a in arms)
    tail = roll[roll.index('extern "C" mgf_status mgf_batch_rollout_dev('):]
    assert "hinge_read" not in tail and "slider_read" not in tail and "kJointRead" not in roll                                    # no entry point changes; the formats are the helper's
    hk = _fn(src, "batch_joint_read_hook")
    assert hk.index("if ((b->*T::rig).recs.empty() || R.rows <= 0) return MGF_OK;") < hk.index("batch_joint_read_ready<T>(b, &H->A)") < hk.index("H->format = ")
    assert "H->format = R.format == T::trace_full ? (iters > 0 ? kJointReadFull : kJointReadFullZero) : kJointReadReading;" in hk   # iters == 0: no solve, zeros
    train = host[host.index("static mgf_status batch_step_run("):host.index('extern "C" mgf_status mgf_batch_step(')]
    passes = ["batch_joint_read_pass<%s>(b, hook->%s_read);" % (KINDS[w]["kind"], w) for w in ("hinge", "slider")]
    ticks = ["MGF_TRY(batch_joint_read_tick<%s>(b, hook->%s_read, t, &hook->launches));" % (KINDS[w]["kind"], w) for w in ("hinge", "slider")]
    # what a kernel reads of the handle is looked up again for every pass: inside the loop over the passes, ahead of the loop over the ticks
    order = [train.index("for (uint32_t first = 0, pass = 0;")] + [train.index(p) for p in passes] + [train.index("for (uint32_t t = first; t < NT; ++t)")]
    assert order == sorted(order) and all(train.count(p) == 1 for p in passes)
    # the launches: behind the tick's solve, the record, the touch trace and the sensor trace; hinges then sliders; ahead of the download of `done`
    order = [train.index("k_batch_solve<<<"), train.index("k_batch_rollout_record<<<"), train.index("k_batch_trace_touch<"), train.index("k_batch_scan_rows<")] + \
            [train.index(t) for t in ticks] + [train.index("d2h(ctx, done.data(), b->d_done.p, K)")]
    assert order == sorted(order) and all(train.count(t) == 1 for t in ticks)
    assert not re.search(r"k_batch_read_(hinges|sliders)<|kJointRead|_READ_LAUNCHES_PER_TICK|_trace\b", train)     # the train launches them through the helper alone
    ps = _fn(src, "batch_joint_read_pass", "void")
    assert ps.index("if (H.format < 0) return;") < ps.index("batch_joint_read_view<T>(b, &H.A);") < ps.index("H.A.done = b->d_done.p; H.A.act = b->d_act.p;")
    tk = _fn(src, "batch_joint_read_tick")
    order = [tk.index(s) for s in ("if (H.format < 0 || (int64_t)t >= R.rows) return MGF_OK;", "A.tick = t;",
                                   "A.out = R.tab.p + (size_t)t * A.n * (H.format == kJointReadReading ? 2u : 4u);", "<<<", "LAUNCH_CHECK();", "*launches += T::read_per_tick;")]
    assert order == sorted(order)                                                              # no launch for a tick the table has no row for; row t, from the handle's pointer as it is now
    assert sorted(re.findall(r"T::template read<true, (\w+)><<<blocks, kBatchBlock, 0, s>>>\(A\);", tk)) == ["kJointReadFull", "kJointReadFullZero", "kJointReadReading"]
    assert tk.count("<<<") == 3 and tk.count("else") == 2 and "else if (H.format == kJointReadFullZero)" in tk and "std::min" not in tk and tk.count("LAUNCH_CHECK();") == 1
    assert "const unsigned blocks = (A.n + kBatchBlock - 1) / kBatchBlock;" in tk              # one of the three is launched; no clamp of the row
    assert not re.search(r"\.done\[[^\]]+\] =[^=]|\.act\[[^\]]+\] =[^=]", src)                  # `done` and `act` are the train's to fill
    step = host[host.index('extern "C" mgf_status mgf_batch_step('):host.index('extern "C" mgf_status mgf_batch_read_constraints(')]
    assert "batch_step_run(b, dt, iters, n_ticks, stats, nullptr)" in step and not re.search(r"joint|hinge|slider", step)   # mgf_batch_step traces nothing
