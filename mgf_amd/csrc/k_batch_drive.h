// Driving a batch between ticks (mgf_batch_get_many / _set_many / _set_forces / _apply_impulses / _copy_worlds; host_batch_drive.inc).
// (Part of the kernel set described in kernels.h.)
//   k_batch_drive_get        a lane per record: ConstrainedSet::get (physics.rs:272-304) of body gidx[i] and its force and torque rows,
//                            seven 16-byte words a record
//   k_batch_drive_set<MODE>  a lane per BODY the call names: the host has sorted the records by body (stable: a body's records stay in
//                            the caller's order) and hands over the runs.  DRIVE_VEL (ConstrainedSet::set, physics.rs:306-314) and
//                            DRIVE_FORCE (RigidBodyVec.force / .torque, physics.rs:146-147) take the last record of the run;
//                            DRIVE_IMPULSE walks the run in order, v = v + linear * inv_mass, omega = omega + I * angular, with
//                            sequential f32 operations: a body belongs to one lane, nothing of the answer depends on lane scheduling
//                            and there is no atomic
//   k_batch_drive_copy       a workgroup per (destination world, source world) pair: the persistent rows of the bodies, the packed tick
//                            copy, the collider a query sees (from the source's packed copy where its rows are behind a tick), the last
//                            tick's constraint list and its length - 16-byte words, a word a lane a trip
// Only the rows named are written; no workgroup waits for another.
#pragma once
#include "k_batch.h"

namespace mgf {

enum { DRIVE_VEL = 0, DRIVE_FORCE = 1, DRIVE_IMPULSE = 2 };

struct BatchDriveArgs {
  Bodies B;               // every world's bodies (body g of the batch = world's first body + index within the world)
  const uint32_t* gidx;   // get: record i names body gidx[i]; set: run r is body gidx[r]
  const uint32_t* run;    // set: run r holds the sorted positions [run[r], run[r + 1]) ...
  const uint32_t* order;  // ... sorted position -> the caller's record index
  const float* a0;        // by the caller's index, `stride` floats apart: linear / force (null: not given)
  const float* a1;        //                                              angular / torque (null: not given)
  uint32_t stride;
  uint32_t n;             // get: records; set: runs
  float4* out;            // get: seven words a record: (v, w.x) (w.yz, x.xy) (x.z, restitution, friction, inv_mass) I[0..3] I[4..7] (I[8], force) (torque, -)
};

__global__ __launch_bounds__(kBatchBlock) void k_batch_drive_get(BatchDriveArgs A) {
  const uint32_t i = blockIdx.x * kBatchBlock + threadIdx.x;
  if (i >= A.n) return;
  const Bodies& B = A.B;
  const size_t g = A.gidx[i];
  const float4 s0 = B.srec[4 * g], s1 = B.srec[4 * g + 1], s2 = B.srec[4 * g + 2], s3 = B.srec[4 * g + 3];
  const float4 p0 = B.sp0[g], p1 = B.sp1[g];
  const V3 x = xyz(B.x[g]) + xyz(B.delta[g]);  // physics.rs:282
  float4* o = A.out + 7 * (size_t)i;
  o[0] = s0;
  o[1] = make_float4(s1.x, s1.y, x.x, x.y);
  o[2] = make_float4(x.z, p0.w, p1.w, s1.z);
  o[3] = make_float4(s1.w, s2.x, s2.y, s2.z);
  o[4] = make_float4(s2.w, s3.x, s3.y, s3.z);
  o[5] = make_float4(s3.w, p0.x, p0.y, p0.z);
  o[6] = make_float4(p1.x, p1.y, p1.z, 0.0f);
}

// What one lane does for body g once it knows its records: the positions [lo, hi) of `order` hold their indices in the caller's order
// (IDENT: position p is record p itself, no table).  Shared by k_batch_drive_set and the device-pointer calls (k_batch_dev.h).
template <int MODE, bool IDENT>
__device__ __forceinline__ void batch_drive_apply(const Bodies& B, size_t g, const uint32_t* order, uint32_t lo, uint32_t hi, const float* a0, const float* a1,
                                                  uint32_t stride) {
  if (MODE == DRIVE_IMPULSE) {
    const float4 s0 = B.srec[4 * g], s1 = B.srec[4 * g + 1], s2 = B.srec[4 * g + 2], s3 = B.srec[4 * g + 3];
    V3 v = mk3(s0.x, s0.y, s0.z), w = mk3(s0.w, s1.x, s1.y);
    const float inv_mass = s1.z;
    const M3 I = m3_cols(mk3(s1.w, s2.x, s2.y), mk3(s2.z, s2.w, s3.x), mk3(s3.y, s3.z, s3.w));
    for (uint32_t p = lo; p < hi; ++p) {
      const size_t k = IDENT ? p : order[p];
      const V3 lin = a0 ? ld3(a0 + stride * k) : mk3(0.0f, 0.0f, 0.0f);
      const V3 ang = a1 ? ld3(a1 + stride * k) : mk3(0.0f, 0.0f, 0.0f);
      v = v + lin * inv_mass;
      w = w + I * ang;
    }
    B.srec[4 * g] = make_float4(v.x, v.y, v.z, w.x);
    B.srec[4 * g + 1] = make_float4(w.y, w.z, s1.z, s1.w);
  } else {
    const size_t k = IDENT ? hi - 1u : order[hi - 1u];  // (a run is never empty)
    if (MODE == DRIVE_VEL) {
      const V3 lin = ld3(a0 + stride * k), ang = ld3(a1 + stride * k);
      const float4 s1 = B.srec[4 * g + 1];
      B.srec[4 * g] = make_float4(lin.x, lin.y, lin.z, ang.x);
      B.srec[4 * g + 1] = make_float4(ang.y, ang.z, s1.z, s1.w);
    } else {
      if (a0) { const V3 f = ld3(a0 + stride * k); B.sp0[g] = mk4(f, B.sp0[g].w); }
      if (a1) { const V3 t = ld3(a1 + stride * k); B.sp1[g] = mk4(t, B.sp1[g].w); }
    }
  }
}

template <int MODE>
__global__ __launch_bounds__(kBatchBlock) void k_batch_drive_set(BatchDriveArgs A) {
  const uint32_t r = blockIdx.x * kBatchBlock + threadIdx.x;
  if (r >= A.n) return;
  batch_drive_apply<MODE, false>(A.B, A.gidx[r], A.order, A.run[r], A.run[r + 1], A.a0, A.a1, A.stride);
}

struct BatchCopyArgs {
  Bodies D, S;                 // the bodies of the destination batch and of the source batch (they may be the same batch)
  const uint2* pairs;          // workgroup p: destination world pairs[p].x becomes source world pairs[p].y (equal lengths: the host has checked)
  const uint32_t* d_off;       // the worlds' first bodies
  const uint32_t* s_off;
  CRec* d_cons;                // the lists: world k's at c_off[k]
  const CRec* s_cons;
  const uint32_t* d_coff;
  const uint32_t* d_cap;       // (the host has grown the destination's share to the source's list)
  const uint32_t* s_coff;
  uint32_t* d_count;
  const uint32_t* s_count;
  uint32_t s_stale;            // the source's col0 / col1 are behind its last tick: its colliders are words 0 and 3 of its packed copy
};

__device__ __forceinline__ void batch_copy_words(float4* d, const float4* s, uint32_t words) {
  for (uint32_t e = threadIdx.x; e < words; e += kBatchBlock) d[e] = s[e];
}

// one pair by its workgroup (k_batch_drive_copy; k_batch_dev_copy_where, k_batch_dev.h, for the pairs its mask selects)
__device__ __forceinline__ void batch_copy_pair(const BatchCopyArgs& A, const uint2 pr) {
  const size_t gd = A.d_off[pr.x], gs = A.s_off[pr.y];
  const uint32_t n = min(A.d_off[pr.x + 1] - A.d_off[pr.x], A.s_off[pr.y + 1] - A.s_off[pr.y]);
  const Bodies &D = A.D, &S = A.S;
  batch_copy_words(D.x + gd, S.x + gs, n);
  batch_copy_words(D.q + gd, S.q + gs, n);
  batch_copy_words(D.srec + 4 * gd, S.srec + 4 * gs, 4u * n);
  batch_copy_words(D.sp0 + gd, S.sp0 + gs, n);
  batch_copy_words(D.sp1 + gd, S.sp1 + gs, n);
  batch_copy_words(D.ctor + gd, S.ctor + gs, n);
  batch_copy_words(D.imb + 3 * gd, S.imb + 3 * gs, 3u * n);
  batch_copy_words(D.delta + gd, S.delta + gs, n);
  batch_copy_words(D.fb_c + gd, S.fb_c + gs, n);
  batch_copy_words(D.fb_r + gd, S.fb_r + gs, n);
  // the collider a query sees, and the packed copy the destination's own gather may still read it from.  (Words 1 and 2 of the packed
  // copy are the tick's own - every tick writes them before it reads them, and nothing reads them between ticks: for a source no tick
  // has run on they are whatever the allocation held, and copying them is harmless.)
  for (uint32_t i = threadIdx.x; i < n; i += kBatchBlock) {
    const float4* sp = S.bpk + 4 * (gs + i);
    float4* dp = D.bpk + 4 * (gd + i);
    const float4 c0 = A.s_stale ? sp[0] : S.col0[gs + i], c1 = A.s_stale ? sp[3] : S.col1[gs + i];
    D.col0[gd + i] = c0; D.col1[gd + i] = c1;
    dp[0] = c0; dp[1] = sp[1]; dp[2] = sp[2]; dp[3] = c1;
  }
  const uint32_t C = min(A.s_count[pr.y], A.d_cap[pr.x]);
  static_assert(sizeof(CRec) == 128, "a constraint record is eight 16-byte words");
  batch_copy_words(reinterpret_cast<float4*>(A.d_cons + A.d_coff[pr.x]), reinterpret_cast<const float4*>(A.s_cons + A.s_coff[pr.y]), 8u * C);
  if (threadIdx.x == 0) A.d_count[pr.x] = C;
}

__global__ __launch_bounds__(kBatchBlock) void k_batch_drive_copy(BatchCopyArgs A) { batch_copy_pair(A, A.pairs[blockIdx.x]); }

}  // namespace mgf
