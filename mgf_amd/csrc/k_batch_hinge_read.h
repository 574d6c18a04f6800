// Hinge encoders of a batch (mgf_batch_read_hinges, mgf_batch_read_hinges_dev, and the readings table behind every tick of a rollout -
// mgf_batch_set_hinge_trace; host_batch_hinge_read.inc).  (Part of the kernel set described in kernels.h.)
//
// A reading is eight floats, (c, sn, rate, side, gap.x, gap.y, gap.z, tilt2), formed from the state as it stands by the hinge's SETUP
// lines (include/mgf_hip.h; the frame lines are k_batch_hinge_frame.h's, written once):
//   c = dot(U1, T1);  sn = dot(U1, T2)      the angle is atan2(sn, c); no arctangent is evaluated here
//   rate = dot(omega_b - omega_a, A)        other == -1: omega_b = 0
//   side                                    +1 or -1 by SETUP's rule with LIMIT and cphi <= ch, otherwise 0: the next solve's limit row
//   gap = C                                 the anchors' gap in the world
//   e1 = dot(B, T1);  e2 = dot(B, T2);  tilt2 = e1 * e1 + e2 * e2     the squared sine of the angle between the two axes
// No division: no hinge is skipped and nothing is counted.  Non-finite state gives non-finite words.
// One launch, k_batch_read_hinges<GATED, FORMAT>: a lane per hinge by the caller's index, ceil(n / kBatchBlock) workgroups over all
// worlds - no plan, no slots, no LDS, no dataflow, no atomic.  The lane reads the record's seven words, then q, x + delta and srec words
// 0 and 1 of both ends, and writes its entry with float4 vector stores: two for a reading, four where the entry carries the impulses.
// (The kernel is not called k_batch_hinge_read: tools/kernel_resources.py selects by substring, and the hinge solver's rows are asked
// for as "k_batch_hinge".)
// GATED (a rollout) is the touch and sensor traces' gate, "world k completed tick t in this pass": done[k] == t + 1 && act[k] <= t + 1
// (k_batch_trace.h, where its three cases are spelled out).  A wave holds hinges of several worlds, so the gate is the LANE's own, and it
// is evaluated before any load of state: a lane that is off loads its record's first word and the two gate words and nothing else.
// FORMAT is a template argument, so that nothing that is the same for the whole launch is tested per lane (DESIGN.md section 9,
// tools/check_lane_masks.py):
//   kHingeReadReading   32 bytes an entry: the reading (MGF_HINGE_TRACE_READING, and the call of its own)
//   kHingeReadFull      64 bytes: the reading and the hinge's eight impulse words (acc.x, acc.y, acc.z, a1, a2, al, am, 0) as the
//                       handle's buffer holds them - tick t's k_batch_hinge_solve wrote them (MGF_HINGE_TRACE_FULL)
//   kHingeReadFullZero  64 bytes: the reading and eight zeros - a rollout with iters == 0, where no solve is enqueued
// The kernel writes nothing but its output.
#pragma once
#include "k_batch_hinge_frame.h"

namespace mgf {

constexpr int kHingeReadReading = 0, kHingeReadFull = 1, kHingeReadFullZero = 2;  // MGF_HINGE_TRACE_READING, MGF_HINGE_TRACE_FULL, and FULL without a solve

struct BatchHingeReadArgs {
  Bodies B;               // every world's bodies
  const uint32_t* w_off;  // the worlds' first bodies
  const float4* rig;      // by the caller's index, seven words a record
  const float4* acc;      // the handle's impulse buffer, two words a hinge (kHingeReadFull alone)
  float4* out;            // entry i at 2 i (a reading) or 4 i (full) words: the caller's array, or row t of the handle's table
  const uint32_t* done;   // a rollout: ticks of the call world k has completed (BatchArgs::done); null: a call of its own
  const uint32_t* act;    // a rollout: ticks whose actuation world k has behind it, final behind k_batch_rollout_record
  uint32_t n, tick;
};

template <bool GATED, int FORMAT>
__global__ __launch_bounds__(kBatchBlock) void k_batch_read_hinges(BatchHingeReadArgs A) {
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
  const HingeFrame F = hinge_frame(a, b, has_b, w1, w2, w3, w4, w5, w6);
  const float c = dot(F.U1, F.T1), sn = dot(F.U1, F.T2);
  const float rate = dot(b.om - a.om, F.A);
  const float side = hinge_side(f2u(w0.w), c, sn, w3.w, w4.w, w5.w);
  const float e1 = dot(F.B, F.T1), e2 = dot(F.B, F.T2);
  const float tilt2 = e1 * e1 + e2 * e2;
  float4* o = A.out + (FORMAT == kHingeReadReading ? 2 : 4) * (size_t)i;
  o[0] = make_float4(c, sn, rate, side);
  o[1] = make_float4(F.C.x, F.C.y, F.C.z, tilt2);
  if (FORMAT == kHingeReadFull) {
    o[2] = A.acc[2 * (size_t)i];
    o[3] = A.acc[2 * (size_t)i + 1];
  }
  if (FORMAT == kHingeReadFullZero) {
    o[2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    o[3] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
}

}  // namespace mgf
