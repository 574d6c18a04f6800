// Ray casts and sweeps of a batch for a caller whose queries and hits are device memory (mgf_batch_raycast_many_dev,
// mgf_batch_sweep_many_dev; host_batch_query_dev.inc): the sort by world of host_batch_query.inc's BatchQueryPlan, built on the device.
// (Part of the kernel set described in kernels.h.)
//   k_batch_query_plan_count<WORDS>
//                             a lane per query: a record whose world lies outside [0, n_worlds) - for a cast (WORDS = 13) also one whose
//                             tag is no component's - gets the no-hit record, world -1 in the call's own copy of the worlds, is counted
//                             in `skipped` and takes no further part.  Every other query counts itself into its world (an integer
//                             atomic) and keeps the value that returns as its rank within the world
//   k_batch_query_plan_cut    a lane per world: the work items its queries are cut into, ceil(count / 256)
//   k_batch_query_plan_fill   (behind the library's prefix sums of both) a lane per query: order[start[world] + rank] = the query; the
//                             query whose rank is a multiple of 256 also writes the work item that begins with it, (world, first,
//                             count <= 256) at the world's item start + rank / 256 - the items BatchQueryPlan::fill writes, in its order
//   k_batch_query_ray_dev<SRC> / k_batch_query_sweep_bodies_dev<SRC>
//                             bq_ray_item / bq_sweep_item (k_batch_query.h: the code of k_batch_query_ray / _sweep_bodies) with the work
//                             item from the device's table (kItemPlan: the grid is the host's upper bound, a workgroup at or beyond the
//                             device's item total leaves before it stages anything) or from blockIdx.x by arithmetic (kItemFixed: every
//                             world has `per` queries, query i is world i / per's; no table, the order is the identity)
// The ORDER of a world's queries in `order` is the order in which the lanes' atomics came: it differs from run to run.  That is allowed
// only because no answer depends on it - every query's answer is a function of the query and its world alone (k_batch_query.h: neither
// the lanes a query gets, nor the other queries of its work item change a bit) - and every answer is stored by the caller's index.
// There is no float atomic.  The fill and every later pass read the call's own copy of the worlds and ranks, never the caller's array
// again: whoever changes world_dev behind the count changes no address a later kernel forms.
#pragma once
#include "k_batch_query.h"

namespace mgf {

struct BatchPlanArgs {
  const int32_t* world;         // the caller's: query i is world world[i]'s
  const int32_t* queries;       // the caller's casts as words, 11 each, word 0 the tag (read for casts only)
  int32_t* out;                 // the caller's hits, WORDS words each
  uint32_t n, K;                // queries; worlds of the batch
  uint32_t item_cap;            // items[] holds floor(n / 256) + min(n, K): no plan has more
  unsigned long long* skipped;  // records skipped whole, cumulative (counter "device_skipped")
  uint32_t *cnt, *icnt;         // [K + 1] queries per world; work items per world
  const uint32_t *start, *istart;  // [K + 1] their exclusive prefix sums; istart[K]: the plan's item total
  int32_t* wsan;                // [n] the world of query i, -1: skipped
  uint32_t* rank;               // [n] its rank within the world
  uint4* items;                 // BatchWorkArgs::items
  uint32_t* order;              // BatchWorkArgs::order
};

template <uint32_t WORDS>
__global__ __launch_bounds__(kBatchBlock) void k_batch_query_plan_count(BatchPlanArgs A) {
  const uint32_t i = blockIdx.x * kBatchBlock + threadIdx.x;
  if (i >= A.n) return;
  const int32_t w = A.world[i];
  bool ok = (uint32_t)w < A.K;  // (checked before it addresses anything)
  if (WORDS == 13u && ok) ok = (uint32_t)A.queries[11 * (size_t)i] <= (uint32_t)KIND_CAPSULE;
  if (!ok) {
    int32_t* o = A.out + WORDS * (size_t)i;
#pragma unroll
    for (uint32_t k = 0; k < WORDS; ++k) o[k] = k == 0u ? MGF_HIT_NONE : 0;
    A.wsan[i] = -1;
    atomicAdd(A.skipped, 1ull);
    return;
  }
  A.wsan[i] = w;
  A.rank[i] = atomicAdd(&A.cnt[w], 1u);
}

__global__ __launch_bounds__(kBatchBlock) void k_batch_query_plan_cut(BatchPlanArgs A) {
  const uint32_t k = blockIdx.x * kBatchBlock + threadIdx.x;
  if (k >= A.K) return;
  A.icnt[k] = (A.cnt[k] + 255u) >> 8;
}

__global__ __launch_bounds__(kBatchBlock) void k_batch_query_plan_fill(BatchPlanArgs A) {
  const uint32_t i = blockIdx.x * kBatchBlock + threadIdx.x;
  if (i >= A.n) return;
  const int32_t w = A.wsan[i];
  if (w < 0) return;
  const uint32_t r = A.rank[i], c = A.cnt[w], at = A.start[w] + r;
  if (r >= c || at >= A.n) return;  // (never: the counts are this call's own)
  A.order[at] = i;
  if (r & 255u) return;
  const uint32_t item = A.istart[w] + (r >> 8);
  if (item < A.item_cap) A.items[item] = make_uint4((uint32_t)w, at, min(256u, c - r), 0u);
}

// LDS (dynamic): 32 bytes a body, kBatchQueryRed words - as the kernels of the host-memory calls.
template <int SRC>
__global__ __launch_bounds__(kBatchBlock) void k_batch_query_ray_dev(BatchQueryArgs A, const ParticleIn* parts, BatchItemSrc S) {
  extern __shared__ float4 s_dyn[];
  bq_ray_item<SRC>(A, PlainBodies(A), parts, S, s_dyn);
}
template <int SRC>
__global__ __launch_bounds__(kBatchBlock) void k_batch_query_sweep_bodies_dev(BatchQueryArgs A, const MovingIn* casts, BatchItemSrc S) {
  extern __shared__ float4 s_dyn[];
  bq_sweep_item<SRC>(A, PlainBodies(A), casts, S, s_dyn);
}

}  // namespace mgf
