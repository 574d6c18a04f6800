// What a caller reads of a batch between ticks besides rays and sweeps (mgf_batch_read_body_contacts, mgf_batch_overlap_aabb_many;
// host_batch_observe.inc).  (Part of the kernel set described in kernels.h.)
//   k_batch_observe_contacts  a workgroup per world of the requested range folds the world's constraint list per body (mgf_body_contacts):
//                             the counts, the net normal impulse -normal * normal_impulse where the body is `a` (solver.rs:243-247) and
//                             +normal * normal_impulse where it is `b`, and the sum of the normal impulses, in the body's chain order -
//                             its own range of the list, then its `b` occurrences ascending, the order k_batch_solve builds.  The
//                             ranges are rebuilt from the records on every call (na, degb and rows are the tick's scratch, and the
//                             lists may have moved since: batch_allot carries the records only): per body the length of its own range
//                             and how often it is `b` by integer atomics in LDS, the range's start by a prefix sum, the `b` occurrences
//                             into `rows` in whatever order the lanes come and then sorted per body.  A lane per body walks its chain
//                             with sequential f32 adds: nothing of the answer depends on lane scheduling, and there is no float atomic.
//                             Of the tick's state only `rows` is written - every tick rebuilds it.
//   bo_front                  a workgroup's work item of boxes against the bodies of its world, written once for every kernel that does it
//                             with a workgroup per work item: k_batch_observe_overlap<FILL> and k_batch_zone_first<SRC> (k_batch_zone.h).
//                             The tight bounds BoundedBy<AABB> (bounds.rs:170-190) of the world's colliders col0 / col1 staged in LDS
//                             once; a box gets min(64, 256 / (count rounded up to a power of two)) lanes of one wave, which take the
//                             bodies in chunks of that many, ascending; Overlaps<AABB> (collision.rs:22-29) per lane, and a hit's rank
//                             is the hits of the chunks before plus the hits below its lane in the wave's ballot: the hits of a box
//                             come in ascending body index whatever the lane split.  What a kernel brings is where a box comes from -
//                             load(qi, g0) -> BatchBox, run by the live lanes behind the staging - and what a hit stores -
//                             put(hit, i, rank), run by every lane on every trip, so that a kernel's own condition joins `hit` in
//                             one branch.  Neither holds a barrier nor leaves the kernel; the front returns the box's count.
//   k_batch_observe_overlap<FILL>
//                             a workgroup per work item = (world, up to 256 boxes) of the queries' sort by world (BatchQueryPlan; the
//                             kernel's share of it: BatchWork, k_batch_query.h), through bo_front: the list of a box is in ascending
//                             body index.  Count (FILL = false), the scan of prims.hip, fill.
// No workgroup waits for another.
#pragma once
#include "k_batch_query.h"

namespace mgf {

struct BatchContactsArgs {
  const CRec* cons;         // world k's list at c_off[k], c_count[k] records
  uint32_t* rows;           // same offsets: the `b` occurrences of every body of the world (CSR), rebuilt here
  const uint32_t* c_off;
  const uint32_t* c_count;
  const uint32_t* w_off;
  uint32_t world0;          // workgroup g answers for world world0 + g ...
  uint32_t* out;            // ... six words a body (mgf_body_contacts), the body w_off[world0] first
};

// LDS (dynamic): four words a body.
__global__ __launch_bounds__(kBatchBlock) void k_batch_observe_contacts(BatchContactsArgs A) {
  extern __shared__ float4 s_dyn[];
  __shared__ uint32_t s_tot;
  const uint32_t k = A.world0 + blockIdx.x, T = kBatchBlock, tid = threadIdx.x;
  const uint32_t g0 = A.w_off[k], n = A.w_off[k + 1] - g0, C = A.c_count[k];
  uint32_t* s_first = reinterpret_cast<uint32_t*>(s_dyn);
  uint32_t *s_na = s_first + n, *s_boff = s_first + 2 * (size_t)n, *s_cur = s_first + 3 * (size_t)n;
  const CRec* cons = A.cons + A.c_off[k];
  uint32_t* rows = A.rows + A.c_off[k];
  for (uint32_t i = tid; i < n; i += T) { s_na[i] = 0u; s_boff[i] = 0u; s_cur[i] = 0u; }
  __syncthreads();
  for (uint32_t c = tid; c < C; c += T) {
    const uint32_t a = cons[c].a, b = cons[c].b;
    atomicAdd(&s_na[a], 1u);
    if (b != kNone) atomicAdd(&s_boff[b], 1u);
  }
  __syncthreads();
  for (uint32_t i = tid; i < n; i += T) s_first[i] = s_na[i];
  batch_scan(s_first, n, &s_tot);  // body i's own range: contiguous (the list is in the order of its `a`), from the prefix sum of the lengths
  batch_scan(s_boff, n, &s_tot);
  for (uint32_t c = tid; c < C; c += T) {
    const uint32_t b = cons[c].b;
    if (b != kNone) rows[s_boff[b] + atomicAdd(&s_cur[b], 1u)] = c;
  }
  __syncthreads();
  uint32_t* out = A.out + 6 * (size_t)(g0 - A.w_off[A.world0]);
  for (uint32_t x = tid; x < n; x += T) {
    uint32_t* row = rows + s_boff[x];
    const uint32_t nb = s_cur[x], na = s_na[x], first = s_first[x];
    for (uint32_t a = 1; a < nb; ++a) {  // ascending list index, whatever order the lanes came in
      const uint32_t v = row[a];
      uint32_t b = a;
      while (b > 0 && row[b - 1] > v) { row[b] = row[b - 1]; --b; }
      row[b] = v;
    }
    V3 imp = mk3(0.0f, 0.0f, 0.0f);
    float sum = 0.0f;
    uint32_t n_terrain = 0;
    for (uint32_t c = first; c < first + na; ++c) {
      const CRec* r = &cons[c];
      const float ni = r->nimp;
      imp = imp - ld3(r->n) * ni;  // va -= impulse * inv_mass_a, solver.rs:243-247
      sum = sum + ni;
      if (r->b == kNone) ++n_terrain;
    }
    for (uint32_t e = 0; e < nb; ++e) {
      const CRec* r = &cons[row[e]];
      const float ni = r->nimp;
      imp = imp + ld3(r->n) * ni;
      sum = sum + ni;
    }
    uint32_t* o = out + 6 * (size_t)x;
    o[0] = na + nb; o[1] = n_terrain; o[2] = f2u(imp.x); o[3] = f2u(imp.y); o[4] = f2u(imp.z); o[5] = f2u(sum);
  }
}

struct BatchOverlapArgs : BatchWorkArgs {
  const float* boxes;     // by the caller's index: c.xyz, r.xyz
  uint32_t* cnt;          // by the caller's index: the hits of box i (written when !FILL) ...
  const uint32_t* off;    // ... their exclusive prefix sums (read when FILL)
  uint32_t* out;          // the bodies of box i at off[i], ascending
};

// a live box in world coordinates and the body of its world it does not hold (-1: none): what a loader hands bo_front
struct BatchBox { Box Q; int32_t ign; };

// IGNORE = false: no box of the kernel names a body - `ign` is not looked at.  W comes back split, z as loaded (not live: zeros, -1).
// bodies: where a body's box comes from - box(g), PlainBodies' or PartBodies' (k_batch_query.h).
// Every lane of a wave makes every trip of the loop (n and L are the work item's); there is no exit; a NaN box hits nothing because
// box_overlaps is false for it.
template <bool IDENTITY, bool IGNORE, class Bodies, class Load, class Put>
__device__ __forceinline__ uint32_t bo_front(const BatchWorkArgs& A, const Bodies& bodies, BatchWork& W, float4* s_dyn, BatchBox& z, Load&& load, Put&& put) {
  const uint32_t tid = threadIdx.x, g0 = W.g0, n = W.n;
  float4 *s_c = s_dyn, *s_r = s_dyn + n;
  for (uint32_t i = tid; i < n; i += kBatchBlock) {
    const Box tb = bodies.box((size_t)g0 + i);
    s_c[i] = mk4(tb.c, 0.0f); s_r[i] = mk4(tb.r, 0.0f);
  }
  __syncthreads();
  W.template split<IDENTITY>(A, min(W.shift(), 6u));  // (a box's lanes in one wave: the ballot)
  const uint32_t L = W.L, sub = W.sub;
  const bool live = W.live;
  z.Q.c = mk3(0.0f, 0.0f, 0.0f); z.Q.r = z.Q.c; z.ign = -1;
  if (live) z = load(W.qi, g0);
  const Box Q = z.Q;
  const int32_t ign = z.ign;
  const uint32_t shift = (tid & 63u) - sub;                        // the first lane of the box's group within the wave
  const uint64_t group = L == 64u ? ~0ull : ((1ull << L) - 1ull);  // the group's lanes, from that lane
  uint32_t m = 0;
  for (uint32_t i0 = 0; i0 < n; i0 += L) {  // (n and L are the work item's: every lane of the wave makes every trip)
    const uint32_t i = i0 + sub;
    bool hit = false;
    if (live && i < n && (!IGNORE || (int32_t)i != ign)) {
      Box b; b.c = xyz(s_c[i]); b.r = xyz(s_r[i]);
      hit = box_overlaps(b, Q);
    }
    const uint64_t g = ((uint64_t)__ballot(hit) >> shift) & group;
    put(hit, i, m + (uint32_t)__popcll(g & ((1ull << sub) - 1ull)));
    m += (uint32_t)__popcll(g);
  }
  return m;
}

// k_batch_observe_overlap<FILL> and its part-aware form (k_batch_part_query.h), written once over the bodies' policy
template <bool FILL, class Bodies>
__device__ __forceinline__ void bo_overlap(const BatchOverlapArgs& A, const Bodies& bodies, float4* s_dyn) {
  BatchWork W(A, true);
  BatchBox z;
  uint32_t base = 0u;  // FILL: where the box's list begins
  const uint32_t m = bo_front<false, false>(
      A, bodies, W, s_dyn, z,
      [&](uint32_t qi, uint32_t) {
        if (FILL) base = A.off[qi];
        return BatchBox{{ld3(A.boxes + 6 * (size_t)qi), ld3(A.boxes + 6 * (size_t)qi + 3)}, -1};
      },
      [&](bool hit, uint32_t i, uint32_t rank) {
        if (FILL && hit) A.out[base + rank] = i;
      });
  if (!FILL && W.live && W.sub == 0u) A.cnt[W.qi] = m;
}

// LDS (dynamic): 32 bytes a body.
template <bool FILL>
__global__ __launch_bounds__(kBatchBlock) void k_batch_observe_overlap(BatchOverlapArgs A) {
  extern __shared__ float4 s_dyn[];
  bo_overlap<FILL>(A, PlainBodies(A), s_dyn);
}

}  // namespace mgf
