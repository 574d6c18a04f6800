// Body-mounted actuators of a batch (mgf_batch_set_actuators, mgf_batch_actuate, mgf_batch_actuate_dev; host_batch_actuator.inc).
// (Part of the kernel set described in kernels.h.)
//
// An actuator is a direction and an arm fixed in the frame of a body with a gain and a clamp: (world, body, flags, gain, p, lo, d, hi).
// With q the body's row as mgf_batch_read_state returns it and u[i] the caller's control, its wrench (L, A) is
//   c = u[i];  if (c < lo) c = lo;  if (c > hi) c = hi;       (a NaN stays a NaN)
//   s = gain * c
//   e = MGF_ACTUATOR_WORLD_DIR ? d : rotate(q, d)
//   MGF_ACTUATOR_TORQUE: L = 0, A = e * s;  else: L = e * s, r = rotate(q, p), A = cross(r, L)
//   s not finite: L = A = 0, counted in `skipped`
// rotate and cross dev_math.h's (Rotation::rotate_vector), every operation a separate f32 one - as k_batch_sensor_ray forms its
// particle.  What is then done to the body is batch_drive_apply's arithmetic (k_batch_drive.h), restated around a wrench that never
// goes through memory: ACTUATE_IMPULSE v = v + L * inv_mass, omega = omega + I * A (DRIVE_IMPULSE's walk); ACTUATE_FORCE force =
// force + L, torque = torque + A.
//   k_batch_actuate<MODE, OUT>  a lane per RUN of the rig: the host has sorted the actuators by (world, body) when the rig was set
//                               (stable: a body's actuators stay in the caller's order) and cut them into runs of one body.  The lane
//                               resolves its body through the worlds' offset table, loads q and the rows MODE writes once, walks the
//                               run in order and stores the rows once; OUT: the wrench of actuator i into row i of the caller's array
//                               on the way.  A body belongs to one lane: no float atomic, nothing of the answer depends on lane
//                               scheduling.
// The walk is a loop every lane of a wave makes the same number of trips through (the longest run of the wave, __any), with the
// lane's own trips under an `if`: no lane leaves the loop ahead of another, and no condition that is the same for the whole wave - MODE
// and OUT are template arguments for that reason - is evaluated inside it (tools/check_lane_masks.py).
#pragma once
#include "k_batch_dev.h"

namespace mgf {

enum { ACTUATE_IMPULSE = 0, ACTUATE_FORCE = 1 };

struct BatchActuateArgs {
  Bodies B;                     // every world's bodies
  const uint32_t* w_off;        // the worlds' first bodies
  const uint4* runs;            // run r: (world, body, first sorted position, count >= 1)
  const float4* rig;            // by the caller's index, three words a record: (world, body, flags, gain) (p, lo) (d, hi)
  const uint32_t* order;        // sorted position -> the caller's index
  const float* u;               // by the caller's index
  float* out;                   // OUT: six floats an actuator, by the caller's index
  unsigned long long* skipped;  // actuators whose gain * clamp(u) was not finite, cumulative (counter "actuators_skipped")
  uint32_t n_runs;
};

template <int MODE, bool OUT>
__global__ __launch_bounds__(kBatchBlock) void k_batch_actuate(BatchActuateArgs A) {
  const uint32_t r = blockIdx.x * kBatchBlock + threadIdx.x;
  const bool live = r < A.n_runs;
  const uint4 run = live ? A.runs[r] : make_uint4(0u, 0u, 0u, 0u);
  const uint32_t cnt = live ? run.w : 0u;
  const size_t g = live ? (size_t)A.w_off[run.x] + run.y : 0;
  const Bodies& B = A.B;
  Quat rot = mkq(1.0f, mk3(0.0f, 0.0f, 0.0f));
  float4 k0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), k1 = k0, s2 = k0, s3 = k0;  // IMPULSE: srec words 0 and 1; FORCE: sp0 and sp1
  if (live) {
    const float4 bq = B.q[g];
    rot = mkq(bq.x, mk3(bq.y, bq.z, bq.w));
    if (MODE == ACTUATE_IMPULSE) { k0 = B.srec[4 * g]; k1 = B.srec[4 * g + 1]; s2 = B.srec[4 * g + 2]; s3 = B.srec[4 * g + 3]; }
    else { k0 = B.sp0[g]; k1 = B.sp1[g]; }
  }
  // IMPULSE: (v, omega) as batch_drive_apply unpacks them; FORCE: (force, torque)
  V3 lin = MODE == ACTUATE_IMPULSE ? mk3(k0.x, k0.y, k0.z) : xyz(k0);
  V3 ang = MODE == ACTUATE_IMPULSE ? mk3(k0.w, k1.x, k1.y) : xyz(k1);
  const float inv_mass = k1.z;
  const M3 I = m3_cols(mk3(k1.w, s2.x, s2.y), mk3(s2.z, s2.w, s3.x), mk3(s3.y, s3.z, s3.w));
  uint32_t n_skip = 0u;
  for (uint32_t j = 0u; __any(j < cnt); ++j) {
    if (j < cnt) {
      const size_t i = A.order[run.z + j];
      const float4 w0 = A.rig[3 * i], w1 = A.rig[3 * i + 1], w2 = A.rig[3 * i + 2];
      const uint32_t flags = f2u(w0.z);
      float c = A.u[i];
      if (c < w1.w) c = w1.w;
      if (c > w2.w) c = w2.w;
      const float s = w0.w * c;
      const V3 e = (flags & MGF_ACTUATOR_WORLD_DIR) ? xyz(w2) : rotate(rot, xyz(w2));
      V3 L, T;
      if (flags & MGF_ACTUATOR_TORQUE) {
        L = mk3(0.0f, 0.0f, 0.0f);
        T = e * s;
      } else {
        L = e * s;
        T = cross(rotate(rot, xyz(w1)), L);
      }
      if (!__builtin_isfinite(s)) {
        L = mk3(0.0f, 0.0f, 0.0f);
        T = L;
        ++n_skip;
      }
      if (OUT) { st3(A.out + 6 * i, L.x, L.y, L.z); st3(A.out + 6 * i + 3, T.x, T.y, T.z); }
      if (MODE == ACTUATE_IMPULSE) {
        lin = lin + L * inv_mass;
        ang = ang + I * T;
      } else {
        lin = lin + L;
        ang = ang + T;
      }
    }
  }
  if (!live) return;
  if (MODE == ACTUATE_IMPULSE) {
    B.srec[4 * g] = make_float4(lin.x, lin.y, lin.z, ang.x);
    B.srec[4 * g + 1] = make_float4(ang.y, ang.z, k1.z, k1.w);
  } else {
    B.sp0[g] = mk4(lin, k0.w);
    B.sp1[g] = mk4(ang, k1.w);
  }
  if (n_skip) atomicAdd(A.skipped, (unsigned long long)n_skip);
}

}  // namespace mgf
