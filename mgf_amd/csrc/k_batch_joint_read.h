// The skeleton of the encoders of a batch: one launch shape and one lane's walk for k_batch_read_hinges and k_batch_read_sliders
// (k_batch_hinge_read.h, k_batch_slider_read.h; host_batch_joint_read.inc).  (Part of the kernel set described in kernels.h.)
//
// batch_joint_read<Reading, GATED, FORMAT>: a lane per joint by the caller's index, ceil(n / kBatchBlock) workgroups over all worlds - no
// plan, no slots, no LDS, no dataflow, no atomic, no division.  The lane reads the record's seven words, then q, x + delta and srec words
// 0 and 1 of both ends (joint_ends, k_batch_joint_loop.h), forms the SETUP frames both kinds share (hinge_frame, k_batch_hinge_frame.h),
// hands them to the kind's Reading - its loads, then its form - and writes its entry with float4 vector stores: two for a reading, four
// where the entry carries the impulses.  The kernel writes nothing but its output.
// GATED (a rollout) is the touch and sensor traces' gate, "world k completed tick t in this pass": done[k] == t + 1 && act[k] <= t + 1
// (k_batch_trace.h, where its three cases are spelled out).  A wave holds joints of several worlds, so the gate is the LANE's own, and it
// is evaluated before any load of state: a lane that is off loads its record's first word and the two gate words and nothing else.
// FORMAT is a template argument, so that nothing that is the same for the whole launch is tested per lane (DESIGN.md section 9,
// tools/check_lane_masks.py):
//   kJointReadReading   32 bytes an entry: the reading (MGF_HINGE_TRACE_READING, MGF_SLIDER_TRACE_READING, and the calls of their own)
//   kJointReadFull      64 bytes: the reading and the joint's eight impulse words as the handle's buffer holds them - tick t's solve
//                       wrote them (MGF_HINGE_TRACE_FULL, MGF_SLIDER_TRACE_FULL)
//   kJointReadFullZero  64 bytes: the reading and eight zeros - a rollout with iters == 0, where no solve is enqueued
//
// Reading is the kind - HingeReading, SliderReading, each in its kernel's file:
//   struct Own; static Own load(B, g0, w0, has_b)     what the kind reads of the state beyond the ends: nothing (the hinge), or the ends'
//                                                     linear velocities (the slider); called beside joint_ends, so that its loads are
//                                                     issued with the ends' and not behind the frames' arithmetic
//   static JointReadWords form(own, w0, w3, w4, w5, a, b, F)
//                                                     the entry's two words from that, the record's words, the ends and the frames;
//                                                     every line a separate f32 operation (-ffp-contract=off)
// Both are __forceinline__; Own goes by value.
#pragma once
#include "k_batch_hinge_frame.h"

namespace mgf {

constexpr int kJointReadReading = 0, kJointReadFull = 1, kJointReadFullZero = 2;  // MGF_*_TRACE_READING, MGF_*_TRACE_FULL, and FULL without a solve

// the two words of 16 bytes of a reading, as a kind's Reading forms them
struct JointReadWords {
  float4 lo, hi;
};

struct BatchJointReadArgs {
  Bodies B;               // every world's bodies
  const uint32_t* w_off;  // the worlds' first bodies
  const float4* rig;      // by the caller's index, seven words a record
  const float4* acc;      // the handle's impulse buffer, two words a joint (kJointReadFull alone)
  float4* out;            // entry i at 2 i (a reading) or 4 i (full) words: the caller's array, or row t of the handle's table
  const uint32_t* done;   // a rollout: ticks of the call world k has completed (BatchArgs::done); null: a call of its own
  const uint32_t* act;    // a rollout: ticks whose actuation world k has behind it, final behind k_batch_rollout_record
  uint32_t n, tick;
};

template <class Reading, bool GATED, int FORMAT>
__device__ __forceinline__ void batch_joint_read(const BatchJointReadArgs& A) {
  const uint32_t i = blockIdx.x * kBatchBlock + threadIdx.x;
  if (i >= A.n) return;
  const float4* rec = A.rig + 7 * (size_t)i;
  const float4 w0 = rec[0];
  const uint32_t k = f2u(w0.x);
  if (GATED && !(A.done[k] == A.tick + 1u && A.act[k] <= A.tick + 1u)) return;  // the tick gate, the lane's own, ahead of every load of state
  const float4 w1 = rec[1], w2 = rec[2], w3 = rec[3], w4 = rec[4], w5 = rec[5], w6 = rec[6];
  const size_t g0 = A.w_off[k];
  const bool has_b = f2u(w0.z) != 0xFFFFFFFFu;  // other == -1: the far end is the world
  JointEnd a, b;
  joint_ends(A.B, g0, w0, has_b, &a, &b);
  const typename Reading::Own own = Reading::load(A.B, g0, w0, has_b);  // (beside the ends' loads, ahead of the frames' arithmetic)
  const HingeFrame F = hinge_frame(a, b, has_b, w1, w2, w3, w4, w5, w6);
  const JointReadWords r = Reading::form(own, w0, w3, w4, w5, a, b, F);
  float4* o = A.out + (FORMAT == kJointReadReading ? 2 : 4) * (size_t)i;
  o[0] = r.lo;
  o[1] = r.hi;
  if (FORMAT == kJointReadFull) {
    o[2] = A.acc[2 * (size_t)i];
    o[3] = A.acc[2 * (size_t)i + 1];
  }
  if (FORMAT == kJointReadFullZero) {
    o[2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    o[3] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
}

}  // namespace mgf
