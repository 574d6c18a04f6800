// Slider encoders of a batch (mgf_batch_read_sliders, mgf_batch_read_sliders_dev, and the readings table behind every tick of a rollout -
// mgf_batch_set_slider_trace; host_batch_slider_read.inc).  (Part of the kernel set described in kernels.h.)
//
// A reading is eight floats, (d, rate, side, off1, off2, e.x, e.y, e.z), formed from the state as it stands by the slider's SETUP lines
// (include/mgf_hip.h; the frame lines are k_batch_hinge_frame.h's, written once, the rate is k_batch_slider.h's slider_rate):
//   U2 = cross(B, U1);  ca = ra + C;  sA = cross(ca, A);  sB = cross(rb, A)
//   d = dot(C, A)                           the travel along the axis
//   rate = slider_rate(v_a, omega_a, v_b, omega_b, A, sA, sB)      what the motor and axis rows of the next solve would see;
//                                           other == -1: v_b = omega_b = 0
//   side                                    2 with LOCK, -1 with LIMIT and d < lo, +1 with LIMIT and d > hi, otherwise 0: the next solve's axis row
//   off1 = dot(C, T1);  off2 = dot(C, T2)   the far anchor's distance from the axis: g1, g2 without the bias factor
//   e = ((cross(A, B) + cross(T1, U1)) + cross(T2, U2)) * 0.5      the frames' error, gw without the bias factor
// No division, no h and no beta: no slider is skipped and nothing is counted.  Non-finite state gives non-finite words.
// One launch, k_batch_read_sliders<GATED, FORMAT>: a lane per slider by the caller's index, ceil(n / kBatchBlock) workgroups over all
// worlds - no plan, no slots, no LDS, no dataflow, no atomic.  The lane reads the record's seven words, then q, x + delta and srec words
// 0 and 1 of both ends - JointEnd carries no linear velocity: v is srec word 0's xyz, read here - and writes its entry with float4 vector
// stores: two for a reading, four where the entry carries the impulses.
// (The kernel is not called k_batch_slider_read: tools/kernel_resources.py selects by substring, and the slider solver's rows are asked
// for as "k_batch_slider".)
// GATED (a rollout) is the touch and sensor traces' gate, "world k completed tick t in this pass": done[k] == t + 1 && act[k] <= t + 1
// (k_batch_trace.h, where its three cases are spelled out).  A wave holds sliders of several worlds, so the gate is the LANE's own, and it
// is evaluated before any load of state: a lane that is off loads its record's first word and the two gate words and nothing else.
// FORMAT is a template argument, so that nothing that is the same for the whole launch is tested per lane (DESIGN.md section 9,
// tools/check_lane_masks.py):
//   kSliderReadReading   32 bytes an entry: the reading (MGF_SLIDER_TRACE_READING, and the call of its own)
//   kSliderReadFull      64 bytes: the reading and the slider's eight impulse words (p1, p2, al, am, aw.x, aw.y, aw.z, 0) as the
//                        handle's buffer holds them - tick t's k_batch_slider_solve wrote them (MGF_SLIDER_TRACE_FULL)
//   kSliderReadFullZero  64 bytes: the reading and eight zeros - a rollout with iters == 0, where no solve is enqueued
// The kernel writes nothing but its output.
#pragma once
#include "k_batch_slider.h"

namespace mgf {

constexpr int kSliderReadReading = 0, kSliderReadFull = 1, kSliderReadFullZero = 2;  // MGF_SLIDER_TRACE_READING, MGF_SLIDER_TRACE_FULL, and FULL without a solve

struct BatchSliderReadArgs {
  Bodies B;               // every world's bodies
  const uint32_t* w_off;  // the worlds' first bodies
  const float4* rig;      // by the caller's index, seven words a record
  const float4* acc;      // the handle's impulse buffer, two words a slider (kSliderReadFull alone)
  float4* out;            // entry i at 2 i (a reading) or 4 i (full) words: the caller's array, or row t of the handle's table
  const uint32_t* done;   // a rollout: ticks of the call world k has completed (BatchArgs::done); null: a call of its own
  const uint32_t* act;    // a rollout: ticks whose actuation world k has behind it, final behind k_batch_rollout_record
  uint32_t n, tick;
};

// the linear velocity of body g: srec word 0's xyz, the word joint_end loads for omega.x
__device__ __forceinline__ V3 slider_read_v(const Bodies& B, size_t g) { return xyz(B.srec[4 * g]); }

template <bool GATED, int FORMAT>
__global__ __launch_bounds__(kBatchBlock) void k_batch_read_sliders(BatchSliderReadArgs A) {
  const uint32_t i = blockIdx.x * kBatchBlock + threadIdx.x;
  if (i >= A.n) return;
  const float4* rec = A.rig + 7 * (size_t)i;
  const float4 w0 = rec[0];
  const uint32_t k = f2u(w0.x);
  if (GATED && !(A.done[k] == A.tick + 1u && A.act[k] <= A.tick + 1u)) return;  // the tick gate, the lane's own, ahead of every load of state
  const float4 w1 = rec[1], w2 = rec[2], w3 = rec[3], w4 = rec[4], w5 = rec[5], w6 = rec[6];
  const size_t g0 = A.w_off[k];
  const bool has_b = f2u(w0.z) != 0xFFFFFFFFu;  // other == -1: the far end is the world
  const uint32_t flags = f2u(w0.w);
  JointEnd a, b;
  joint_ends(A.B, g0, w0, has_b, &a, &b);
  const V3 va = slider_read_v(A.B, g0 + f2u(w0.y));
  V3 vb = mk3(0.0f, 0.0f, 0.0f);
  if (has_b) vb = slider_read_v(A.B, g0 + f2u(w0.z));
  const HingeFrame F = hinge_frame(a, b, has_b, w1, w2, w3, w4, w5, w6);
  const V3 U2 = cross(F.B, F.U1);
  const V3 ca = F.ra + F.C;
  const V3 sA = cross(ca, F.A);
  const V3 sB = cross(F.rb, F.A);
  const float d = dot(F.C, F.A);
  const float rate = slider_rate(va, a.om, vb, b.om, F.A, sA, sB);
  float side = 0.0f;
  if ((flags & kSliderLock) != 0u) side = 2.0f;
  else if ((flags & kSliderLimit) != 0u && d < w3.w) side = -1.0f;
  else if ((flags & kSliderLimit) != 0u && d > w4.w) side = 1.0f;
  const float off1 = dot(F.C, F.T1), off2 = dot(F.C, F.T2);
  const V3 e = ((cross(F.A, F.B) + cross(F.T1, F.U1)) + cross(F.T2, U2)) * 0.5f;
  float4* o = A.out + (FORMAT == kSliderReadReading ? 2 : 4) * (size_t)i;
  o[0] = make_float4(d, rate, side, off1);
  o[1] = make_float4(off2, e.x, e.y, e.z);
  if (FORMAT == kSliderReadFull) {
    o[2] = A.acc[2 * (size_t)i];
    o[3] = A.acc[2 * (size_t)i + 1];
  }
  if (FORMAT == kSliderReadFullZero) {
    o[2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    o[3] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
}

}  // namespace mgf
