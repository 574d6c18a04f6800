// Springs between the bodies of a batch (mgf_batch_set_springs, mgf_batch_apply_springs, mgf_batch_apply_springs_dev, and ahead of
// every tick of mgf_batch_rollout / _rollout_dev; host_batch_spring.inc).
// (Part of the kernel set described in kernels.h.)
//
// A spring is a spring-damper between two body-fixed points, or between one and a point of the world: (world, body, other, flags, pa,
// rest, pb, k, c, lo, hi, pad), four 16-byte words.  With x (= x + delta), q, v, omega of each end as k_batch_dev_gather returns them
// and h the call's time step, its wrench is - every line a separate f32 operation, rotate, cross and dot dev_math.h's -
//   ra = rotate(q_a, pa);  Pa = x_a + ra;  Va = v_a + cross(omega_a, ra)
//   other >= 0:  rb = rotate(q_b, pb);  Pb = x_b + rb;  Vb = v_b + cross(omega_b, rb)      other == -1:  Pb = pb;  Vb = 0;  rb = 0
//   d = Pb - Pa;  len = sqrt(dot(d, d));  n = d / len;  rate = dot(Vb - Va, n)
//   f = k * (len - rest) + c * rate;  if (f < lo) f = lo;  if (f > hi) f = hi;  s = f * h
//   L = n * s;  A = cross(ra, L);  Lb = -L;  Ab = cross(rb, Lb)                             (other == -1: Lb = Ab = 0)
//   len == 0, or len or s not finite: all four zero, counted in `skipped`
// A call is two launches, because every wrench is formed from the state BEFORE the call and a body may carry many ends:
//   k_batch_spring_wrench       a lane per spring: the rows of both ends through the worlds' offsets, the twelve floats (L, A, Lb, Ab)
//                               into the handle's buffer and, where given, into the caller's; it reads state only and obeys no gate -
//                               in a rollout only the COUNT of skips does (done, act not null), so that a world that sits a tick out or
//                               runs one again is not counted twice.
//   k_batch_spring_apply<GATED> a lane per RUN of the plan: the host has sorted the 2 n ends - end e = 2 i + side, its (L, A) the six
//                               floats at 6 e of the buffer; a world anchor's far end is not an end - by (world, body) when the rig was
//                               set (stable: a body's ends stay in list order) and cut them into runs of one body.  The lane loads the
//                               body's velocity rows once, walks the run with batch_drive_apply's DRIVE_IMPULSE arithmetic (k_batch_drive.h)
//                               v = v + L * inv_mass, omega = omega + I * A, and stores once: a body belongs to one lane, no float atomic,
//                               and no lane reads a word another lane of the launch writes (the buffer is the launch before's).
//                               GATED (a rollout): the train's gate done[k] == tick && act[k] == tick (k_batch_rollout.h) is a lane's
//                               own and is folded into the run length, as k_batch_rollout_act folds it.
// The walk is a loop every lane of a wave makes the same number of trips through (the longest run of the wave, __any), with the lane's
// own trips under an `if`: no lane leaves the loop ahead of another, and no condition that is the same for the whole wave - GATED is a
// template argument for that reason - is evaluated inside it (tools/check_lane_masks.py).
#pragma once
#include "k_batch_rollout.h"

namespace mgf {

struct BatchSpringArgs {
  Bodies B;                     // every world's bodies
  const uint32_t* w_off;        // the worlds' first bodies
  const uint4* runs;            // run r: (world, body, first sorted position, count >= 1)
  const float4* rig;            // by the caller's index, four words a record: (world, body, other, flags) (pa, rest) (pb, k) (c, lo, hi, pad)
  const uint32_t* order;        // sorted position -> end e = 2 i + side
  float* wr;                    // the handle's: twelve floats a spring, (L, A, Lb, Ab)
  float* out;                   // the caller's, the same rows; null: not asked for
  unsigned long long* skipped;  // springs whose wrench was zeroed, cumulative (counter "springs_skipped")
  const uint32_t* done;         // a rollout: ticks of the call world k has completed (BatchArgs::done); null: a call of its own
  const uint32_t* act;          // a rollout: ticks whose actuation world k has behind it (BatchRolloutArgs::act)
  float h;                      // the time step
  uint32_t n, n_runs, tick;
};

__global__ __launch_bounds__(kBatchBlock) void k_batch_spring_wrench(BatchSpringArgs A) {
  const uint32_t i = blockIdx.x * kBatchBlock + threadIdx.x;
  if (i >= A.n) return;
  const Bodies& B = A.B;
  const float4 w0 = A.rig[4 * (size_t)i], w1 = A.rig[4 * (size_t)i + 1], w2 = A.rig[4 * (size_t)i + 2], w3 = A.rig[4 * (size_t)i + 3];
  const uint32_t world = f2u(w0.x);
  const int32_t other = (int32_t)f2u(w0.z);
  const size_t g0 = A.w_off[world];
  const size_t ga = g0 + f2u(w0.y);
  const float4 qa = B.q[ga], a0 = B.srec[4 * ga], a1 = B.srec[4 * ga + 1];
  const V3 xa = xyz(B.x[ga]) + xyz(B.delta[ga]);  // physics.rs:282, as k_batch_dev_gather
  const V3 ra = rotate(mkq(qa.x, mk3(qa.y, qa.z, qa.w)), xyz(w1));
  const V3 Pa = xa + ra;
  const V3 Va = mk3(a0.x, a0.y, a0.z) + cross(mk3(a0.w, a1.x, a1.y), ra);
  V3 rb = mk3(0.0f, 0.0f, 0.0f), Pb = xyz(w2), Vb = rb;
  if (other >= 0) {
    const size_t gb = g0 + (uint32_t)other;
    const float4 qb = B.q[gb], b0 = B.srec[4 * gb], b1 = B.srec[4 * gb + 1];
    const V3 xb = xyz(B.x[gb]) + xyz(B.delta[gb]);
    rb = rotate(mkq(qb.x, mk3(qb.y, qb.z, qb.w)), xyz(w2));
    Pb = xb + rb;
    Vb = mk3(b0.x, b0.y, b0.z) + cross(mk3(b0.w, b1.x, b1.y), rb);
  }
  const V3 d = Pb - Pa;
  const float len = __builtin_sqrtf(dot(d, d));
  const V3 n = d / len;
  const float rate = dot(Vb - Va, n);
  float f = w2.w * (len - w1.w) + w3.x * rate;
  if (f < w3.y) f = w3.y;
  if (f > w3.z) f = w3.z;
  const float s = f * A.h;
  V3 L = n * s;
  V3 T = cross(ra, L);
  V3 Lb = -L;
  V3 Tb = cross(rb, Lb);
  if (other < 0) {
    Lb = mk3(0.0f, 0.0f, 0.0f);
    Tb = Lb;
  }
  const bool skip = len == 0.0f || !__builtin_isfinite(len) || !__builtin_isfinite(s);
  if (skip) {
    L = mk3(0.0f, 0.0f, 0.0f);
    T = L; Lb = L; Tb = L;
  }
  float* o = A.wr + 12 * (size_t)i;
  st3(o, L.x, L.y, L.z); st3(o + 3, T.x, T.y, T.z); st3(o + 6, Lb.x, Lb.y, Lb.z); st3(o + 9, Tb.x, Tb.y, Tb.z);
  if (A.out) {
    float* c = A.out + 12 * (size_t)i;
    st3(c, L.x, L.y, L.z); st3(c + 3, T.x, T.y, T.z); st3(c + 6, Lb.x, Lb.y, Lb.z); st3(c + 9, Tb.x, Tb.y, Tb.z);
  }
  if (skip && (!A.done || (A.done[world] == A.tick && A.act[world] == A.tick))) atomicAdd(A.skipped, 1ull);
}

template <bool GATED>
__global__ __launch_bounds__(kBatchBlock) void k_batch_spring_apply(BatchSpringArgs A) {
  const uint32_t r = blockIdx.x * kBatchBlock + threadIdx.x;
  const bool in = r < A.n_runs;
  const uint4 run = in ? A.runs[r] : make_uint4(0u, 0u, 0u, 0u);
  const bool live = in && (!GATED || (A.done[run.x] == A.tick && A.act[run.x] == A.tick));  // the tick gate, a lane's own
  const uint32_t cnt = live ? run.w : 0u;
  const size_t g = live ? (size_t)A.w_off[run.x] + run.y : 0;
  const Bodies& B = A.B;
  float4 k0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), k1 = k0, s2 = k0, s3 = k0;  // srec words 0 .. 3
  if (live) { k0 = B.srec[4 * g]; k1 = B.srec[4 * g + 1]; s2 = B.srec[4 * g + 2]; s3 = B.srec[4 * g + 3]; }
  // (v, omega) as batch_drive_apply unpacks them
  V3 lin = mk3(k0.x, k0.y, k0.z);
  V3 ang = mk3(k0.w, k1.x, k1.y);
  const float inv_mass = k1.z;
  const M3 I = m3_cols(mk3(k1.w, s2.x, s2.y), mk3(s2.z, s2.w, s3.x), mk3(s3.y, s3.z, s3.w));
  for (uint32_t j = 0u; __any(j < cnt); ++j) {
    if (j < cnt) {
      const float* w = A.wr + 6 * (size_t)A.order[run.z + j];
      const V3 L = ld3(w), T = ld3(w + 3);
      lin = lin + L * inv_mass;
      ang = ang + I * T;
    }
  }
  if (!live) return;
  B.srec[4 * g] = make_float4(lin.x, lin.y, lin.z, ang.x);
  B.srec[4 * g + 1] = make_float4(ang.y, ang.z, k1.z, k1.w);
}

}  // namespace mgf
