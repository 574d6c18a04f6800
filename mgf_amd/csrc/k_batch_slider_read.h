// Slider encoders of a batch (mgf_batch_read_sliders, mgf_batch_read_sliders_dev, and the readings table behind every tick of a rollout -
// mgf_batch_set_slider_trace; host_batch_joint_read.inc under SliderKind).  (Part of the kernel set described in kernels.h.)
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
// One launch, k_batch_read_sliders<GATED, FORMAT>: a single call of the encoders' skeleton (batch_joint_read, k_batch_joint_read.h, which
// holds the lane's walk, the gate, the loads and the stores in three formats) over SliderReading, which holds the lines above and two
// loads of its own (its load step, called beside the ends' loads), behind the skeleton's gate as everything here is - JointEnd carries
// no linear velocity: v is srec word 0's xyz.  A full entry's eight impulse words are (p1, p2, al, am, aw.x, aw.y, aw.z, 0), as tick t's k_batch_slider_solve wrote them.
// (The kernel is not called k_batch_slider_read: tools/kernel_resources.py selects by substring, and the slider solver's rows are asked
// for as "k_batch_slider".)
#pragma once
#include "k_batch_joint_read.h"
#include "k_batch_slider.h"

namespace mgf {

// the linear velocity of body g: srec word 0's xyz, the word joint_end loads for omega.x
__device__ __forceinline__ V3 slider_read_v(const Bodies& B, size_t g) { return xyz(B.srec[4 * g]); }

struct SliderReading {
  struct Own {
    V3 va, vb;  // the ends' linear velocities; other == -1: vb = 0
  };
  __device__ __forceinline__ static Own load(const Bodies& B, size_t g0, float4 w0, bool has_b) {
    Own o;
    o.va = slider_read_v(B, g0 + f2u(w0.y));
    o.vb = mk3(0.0f, 0.0f, 0.0f);
    if (has_b) o.vb = slider_read_v(B, g0 + f2u(w0.z));
    return o;
  }
  __device__ __forceinline__ static JointReadWords form(Own own, float4 w0, float4 w3, float4 w4, float4, const JointEnd& a, const JointEnd& b, const HingeFrame& F) {
    const uint32_t flags = f2u(w0.w);
    const V3 U2 = cross(F.B, F.U1);
    const V3 ca = F.ra + F.C;
    const V3 sA = cross(ca, F.A);
    const V3 sB = cross(F.rb, F.A);
    const float d = dot(F.C, F.A);
    const float rate = slider_rate(own.va, a.om, own.vb, b.om, F.A, sA, sB);
    float side = 0.0f;
    if ((flags & kSliderLock) != 0u) side = 2.0f;
    else if ((flags & kSliderLimit) != 0u && d < w3.w) side = -1.0f;
    else if ((flags & kSliderLimit) != 0u && d > w4.w) side = 1.0f;
    const float off1 = dot(F.C, F.T1), off2 = dot(F.C, F.T2);
    const V3 e = ((cross(F.A, F.B) + cross(F.T1, F.U1)) + cross(F.T2, U2)) * 0.5f;
    return {make_float4(d, rate, side, off1), make_float4(off2, e.x, e.y, e.z)};
  }
};

template <bool GATED, int FORMAT>
__global__ __launch_bounds__(kBatchBlock) void k_batch_read_sliders(BatchJointReadArgs A) {
  batch_joint_read<SliderReading, GATED, FORMAT>(A);
}

}  // namespace mgf
