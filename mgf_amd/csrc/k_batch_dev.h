// The device-pointer calls of a batch (mgf_batch_gather_state_dev / _set_many_dev / _set_forces_dev / _apply_impulses_dev /
// _copy_worlds_where; host_batch_dev.inc): the caller's arrays are device memory, nothing goes through the host.
// (Part of the kernel set described in kernels.h.)
//   k_batch_dev_gather        a lane per record: x + delta, q, v, omega, force, torque of body body[i] (null: body i) into the caller's
//                             packed rows - the rows of a body as 16-byte loads, a 12-byte output row as three dword stores
//   k_batch_dev_count         a lane per record: how many records name each body (integer atomics); a record out of range is counted
//                             in `skipped` and takes no further part
//   k_batch_dev_fill          (behind the library's prefix sum of the counts) a lane per record: the record's index into its body's
//                             segment, in whatever order the lanes come
//   k_batch_dev_apply<MODE, SEG>
//                             SEG: a lane per BODY of the batch; a body no record names leaves at once.  A set takes the highest record
//                             index of the segment; an impulse sorts the segment ascending by insertion (the order of the host path's
//                             stable sort, whatever order k_batch_dev_fill's lanes came in) and walks it.  !SEG (body == null: record i is
//                             body i, no body twice): a lane per record.  What is then done to the body is batch_drive_apply
//                             (k_batch_drive.h), the code k_batch_drive_set<MODE> runs: one lane owns a body, sequential f32 operations,
//                             no float atomic, nothing depends on lane scheduling
//   k_batch_dev_copy_where    k_batch_drive_copy for the pairs a mask in device memory selects: the pair's workgroup reads its mask word
//                             and leaves if it is zero
// Every index taken from the caller's memory is checked against the number of bodies before it addresses anything.
#pragma once
#include "k_batch_drive.h"

namespace mgf {

struct BatchDevArgs {
  Bodies B;                      // every world's bodies
  const int32_t* body;           // record i names body body[i] of the batch (flat index); null: body i
  uint32_t n, total;             // records; bodies of the batch
  unsigned long long* skipped;   // records whose index lies outside [0, total), cumulative
  uint32_t* cnt;                 // [total + 1] records per body: up in k_batch_dev_count, back down to zero in k_batch_dev_fill
  const uint32_t* off;           // [total + 1] their exclusive prefix sum
  uint32_t* seg;                 // [n] body g's record indices at off[g] .. off[g + 1]
  const float* a0;               // by record, 3 floats a row: linear / force (null: not given)
  const float* a1;               //                            angular / torque
  float *x, *q, *v, *om, *f, *t; // gather: the caller's rows (null: not asked for)
};

__device__ __forceinline__ void st3(float* o, float a, float b, float c) { o[0] = a; o[1] = b; o[2] = c; }

__global__ __launch_bounds__(kBatchBlock) void k_batch_dev_gather(BatchDevArgs A) {
  const uint32_t i = blockIdx.x * kBatchBlock + threadIdx.x;
  if (i >= A.n) return;
  const uint32_t gi = A.body ? (uint32_t)A.body[i] : i;
  if (gi >= A.total) { atomicAdd(A.skipped, 1ull); return; }
  const Bodies& B = A.B;
  const size_t g = gi, r = 3 * (size_t)i;
  if (A.x) { const V3 x = xyz(B.x[g]) + xyz(B.delta[g]); st3(A.x + r, x.x, x.y, x.z); }  // physics.rs:282, as k_batch_drive_get
  if (A.q) { const float4 q = B.q[g]; float* o = A.q + 4 * (size_t)i; o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w; }
  if (A.v || A.om) {
    const float4 s0 = B.srec[4 * g], s1 = B.srec[4 * g + 1];
    if (A.v) st3(A.v + r, s0.x, s0.y, s0.z);
    if (A.om) st3(A.om + r, s0.w, s1.x, s1.y);
  }
  if (A.f) { const float4 p0 = B.sp0[g]; st3(A.f + r, p0.x, p0.y, p0.z); }
  if (A.t) { const float4 p1 = B.sp1[g]; st3(A.t + r, p1.x, p1.y, p1.z); }
}

__global__ __launch_bounds__(kBatchBlock) void k_batch_dev_count(BatchDevArgs A) {
  const uint32_t i = blockIdx.x * kBatchBlock + threadIdx.x;
  if (i >= A.n) return;
  const uint32_t g = (uint32_t)A.body[i];
  if (g >= A.total) { atomicAdd(A.skipped, 1ull); return; }
  atomicAdd(&A.cnt[g], 1u);
}

__global__ __launch_bounds__(kBatchBlock) void k_batch_dev_fill(BatchDevArgs A) {
  const uint32_t i = blockIdx.x * kBatchBlock + threadIdx.x;
  if (i >= A.n) return;
  const uint32_t g = (uint32_t)A.body[i];
  if (g >= A.total) return;
  // a place of its own in [off[g], off[g + 1]): the count comes back down as the places go (whoever changes body[] between the two
  // launches gets a record dropped here, never a store outside the segments)
  const uint32_t left = atomicSub(&A.cnt[g], 1u);
  const uint32_t lo = A.off[g], len = A.off[g + 1] - lo;
  if (left == 0u || left > len) return;
  A.seg[lo + left - 1u] = i;
}

template <int MODE, bool SEG>
__global__ __launch_bounds__(kBatchBlock) void k_batch_dev_apply(BatchDevArgs A) {
  const uint32_t e = blockIdx.x * kBatchBlock + threadIdx.x;
  if (!SEG) {
    if (e >= A.n) return;
    batch_drive_apply<MODE, true>(A.B, e, nullptr, e, e + 1u, A.a0, A.a1, 3u);
    return;
  }
  if (e >= A.total) return;
  const uint32_t lo = A.off[e], hi = A.off[e + 1];
  if (lo >= hi || hi > A.n) return;
  uint32_t* seg = A.seg;
  if (MODE == DRIVE_IMPULSE) {
    for (uint32_t a = lo + 1u; a < hi; ++a) {  // ascending record index, whatever order the lanes of the fill came in
      const uint32_t v = seg[a];
      uint32_t b = a;
      while (b > lo && seg[b - 1u] > v) { seg[b] = seg[b - 1u]; --b; }
      seg[b] = v;
    }
    for (uint32_t p = lo; p < hi; ++p)
      if (seg[p] >= A.n) return;  // (nothing the fill wrote: every place of a segment is written when body[] stays as it is)
    batch_drive_apply<MODE, false>(A.B, e, seg, lo, hi, A.a0, A.a1, 3u);
  } else {
    uint32_t last = seg[lo];
    for (uint32_t p = lo + 1u; p < hi; ++p) last = max(last, seg[p]);
    if (last >= A.n) return;
    batch_drive_apply<MODE, true>(A.B, e, nullptr, last, last + 1u, A.a0, A.a1, 3u);
  }
}

struct BatchCopyWhereArgs {
  BatchCopyArgs C;
  const int32_t* mask;  // the caller's: pair p is copied iff mask[p] != 0
};

__global__ __launch_bounds__(kBatchBlock) void k_batch_dev_copy_where(BatchCopyWhereArgs A) {
  if (A.mask[blockIdx.x] == 0) return;
  batch_copy_pair(A.C, A.C.pairs[blockIdx.x]);
}

}  // namespace mgf
