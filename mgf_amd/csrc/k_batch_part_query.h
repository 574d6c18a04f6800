// Rays, sweeps and box queries of a batch that see the parts of bodies of several components (option "part_queries" on a batch that
// holds part storage; host_batch_part_query.inc).  (Part of the kernel set described in kernels.h.)
//
// The definition is the lone world's (k_query.h: q_ray_body, q_sweep_body, q_body_box): every part of every body not ignored goes through
// q_ray_comp / comp_mcomp, an ordinary body is its collider row and reports part 0, the ranking is (t, kind, index, part) for a ray and
// SweepBest's (t, kind, index, part, order) for a cast, a body's box is comp_bounds of its parts combined in order with box_combine.  The
// parts are the world parts wp0 / wp1 (four slots a body: written when the body is added and by k_batch_parts_front every tick), the
// part count the second word of the constructor row of a body whose first word is 2 (batch_np, k_batch_parts.h) - taken as
// min(count, kMaxParts), so that a bad word in memory cannot lengthen a loop.
// The work split, the fronts and the kernels' bodies are the existing kernels' own, written once in their headers over a policy of the
// bodies (k_batch_query.h, at PlainBodies): a workgroup per work item, 256 / next_pow2(count) lanes a query, bq_reduce across lanes and
// waves; the box front a query's lanes in one wave and a hit's rank from the ballot.  Here is the policy that sees parts, PartBodies -
// the staging, the body-level rejects, the two walks, a body's box - and a kernel per existing kernel that passes it:
//   k_batch_pq_ray<SRC>      bq_ray_item (bq_ray_front)             k_batch_pq_sensor    bs_rays (k_batch_sensor.h)
//   k_batch_pq_sweep<SRC>    bq_sweep_item (bq_sweep_front)         k_batch_pq_feeler    bf_casts (k_batch_feeler.h)
//   k_batch_pq_overlap<FILL> bo_overlap (k_batch_observe.h), k_batch_pq_zone<SRC> bz_first (k_batch_zone.h), k_batch_pq_nearest<SRC>
//                            bn_nearest (k_batch_nearest.h), each through bo_front: the staged box is the union of the parts' bounds
// The passes behind a body pass - k_batch_query_sweep_faces, _ray_obstacles, _sweep_obstacles, q_ray_terrain in the ray front's tail -
// are the existing ones, unchanged.
//
// STAGING (rays and sweeps): 36 bytes a body of dynamic LDS - two rows and a count (at most 36 KB + 256 bytes at 1024 bodies).  An
// ordinary body stages its collider rows and count 1.  A body of several parts stages a REJECT SPHERE (C, RB) in the two rows (kind
// sphere) and its part count (flagged: kPqSeveral); the sphere is computed at staging time from wp0 / wp1 - there is no persistent row,
// nothing for a world copy to carry.  A lane strides over the bodies; for a body of several parts it runs the body-level reject on the
// sphere and only for a surviving body reads the parts (128 bytes a body, from global memory), each through the part-level reject
// (bq_ray_far / q_sweep_far), the single-shape test and offer(..., index, part).  The sweep front walks (body, part) in one loop with
// one place for comp_mcomp: a loop of parts inside the loop of bodies spilled scalar registers.
//
// WHY THE BODY-LEVEL REJECT CHANGES NO ANSWER.  bq_ray_far and q_sweep_far bound a component by the sphere of centre m_k and radius
// ra_k (a sphere: its own; a capsule: the middle of its axis, r + |d| / 2).  The staged sphere holds every one of them:
//   RB >= |m_k - C| + ra_k   for every part k           (C: the mean of the m_k; RB: the largest such sum, times 1.0001, plus
//                                                        1e-5 max|C| + 1e-5 for the rounding of the m_k, the differences and the roots)
// Rays.  bq_ray_far drops part k iff D_k^2 > lim_k^2 + 1e-4 |w_k|^2, with D_k the distance of m_k from the segment p + d s, s in
// [0, dt], w_k = m_k - p and lim_k = 1.01 ra_k + 1e-3.  Since sqrt(a^2 + b^2) <= a + b it is enough that D_k > lim_k + 0.01 |w_k|.  The
// triangle inequality gives D_k >= D_C - |m_k - C| and |w_k| <= |W| + |m_k - C| (D_C, W: the same for C), so
//   D_C > 1.01 RB + 1e-3 + 0.01 |W|   implies   D_k > 1.01 RB - |m_k - C| + 1e-3 + 0.01 |W|
//                                                   >= 1.01 ra_k + 0.01 |m_k - C| + 1e-3 + 0.01 |W| >= lim_k + 0.01 |w_k|
// pq_ray_far_body asks for D_C > 1.011 RB + 1.1e-3 + 0.011 |W|: the extra thousandth of RB and of |W| and the tenth of a millimetre
// are far above what the rounding of either test's s, e and dot(e, e) can move (a few 1e-7 of |W| each).  So a body the body-level
// reject drops has only parts the part-level reject drops too.
// Sweeps.  q_sweep_far drops part k iff D_k > 1.01 (ra_k + cr) + pad, D_k the distance of m_k from the path cc + v s, s in [0, 1].
// D_k >= D_C - |m_k - C| again, so D_C > 1.01 (RB + cr) + pad implies D_k > 1.01 (ra_k + cr) + pad.  pq_sweep_far_body asks for that plus
// 1e-5 (max|W| + max|v|) for the rounding of either test.
// Either way a body-level reject drops only parts that the part-level reject drops, and that reject is conservative for the
// single-shape test: the answers remain the lone world's, whatever the lanes a query gets.
// (NaN and an overflowing square compare false: not far - the part-level test, then the single-shape test decide.)
//
// PART THROUGH THE REDUCTION.  QueryBest's shfl / pack / unpack / merge leave `part` behind (the bodies of the existing kernels have
// one).  PartBest carries it - in the packed candidate's free fourth word - and merges with it; SweepBest carries it already.
//
// BARRIERS.  The fronts': the staging below ends with a front's first and holds no other, a walk holds none and leaves no kernel.
// Between ticks the parts are those of the last tick, or as added before any tick - as col0 / col1; write_state and set_many move none.
// No workgroup waits for another.
#pragma once
#include "k_batch_feeler.h"
#include "k_batch_nearest.h"
#include "k_batch_parts.h"
#include "k_batch_sensor.h"

namespace mgf {

// the rows of every body of the batch a part-aware kernel reads besides BatchWorkArgs: body g's parts at kMaxParts * g
struct BatchPartRows { const float4 *ctor, *wp0, *wp1; };

constexpr uint32_t kPqSeveral = 8u;  // a staged count's flag: the rows hold a reject sphere, the parts are in wp0 / wp1
// the parts a loop walks for body g: 1 for an ordinary body, else min(count, kMaxParts)
__device__ __forceinline__ uint32_t pq_count(const BatchPartRows& P, size_t g) {
  const float4 ct = P.ctor[g];
  return f2u(ct.x) == 2u ? min(max(f2u(ct.y), 1u), (uint32_t)kMaxParts) : 1u;
}
__device__ __forceinline__ bool pq_several(const BatchPartRows& P, size_t g) { return f2u(P.ctor[g].x) == 2u; }

// QueryBest whose `part` travels through bq_reduce
struct PartBest : QueryBest {
  __device__ __forceinline__ PartBest shfl(int off) const {
    PartBest o;
    o.kind = __shfl_xor(have ? kind : -1, off); o.index = (uint32_t)__shfl_xor((int)index, off); o.part = (uint32_t)__shfl_xor((int)part, off);
    o.p = q_shfl3(p, off); o.t = __shfl_xor(t, off);
    o.have = o.kind >= 0;
    return o;
  }
  __device__ __forceinline__ void pack(float4* w) const {
    w[0] = make_float4(u2f((uint32_t)(have ? kind : -1)), u2f(index), t, u2f(part));
    w[1] = mk4(p, 0.0f);
  }
  static __device__ __forceinline__ PartBest unpack(const float4* w) {
    const float4 r0 = w[0], r1 = w[1];
    PartBest o;
    o.kind = (int)f2u(r0.x); o.index = f2u(r0.y); o.part = f2u(r0.w); o.p = xyz(r1); o.t = r0.z;
    o.have = o.kind >= 0;
    return o;
  }
  __device__ __forceinline__ void merge(const PartBest& o) { if (o.have) offer(o.p, o.t, o.kind, o.index, o.part); }
};

// col0 / col1 of an ordinary body, the reject sphere of a body of several parts; the count.  Ends with the front's first barrier.
__device__ __forceinline__ void pq_stage(const BatchWorkArgs& A, const BatchPartRows& P, uint32_t g0, uint32_t n, float4* s_c0, float4* s_c1, uint32_t* s_np) {
  for (uint32_t i = threadIdx.x; i < n; i += kBatchBlock) {
    const size_t g = (size_t)g0 + i;
    const uint32_t np = pq_count(P, g);
    float4 a = A.col0[g], b = A.col1[g];
    if (pq_several(P, g)) {
      V3 m[kMaxParts];
      float ra[kMaxParts];
      V3 c = mk3(0.0f, 0.0f, 0.0f);
#pragma unroll
      for (uint32_t k = 0; k < (uint32_t)kMaxParts; ++k) {  // (constant indices: m and ra stay in registers)
        m[k] = c; ra[k] = 0.0f;
        if (k < np) {
          const float4 pa = P.wp0[kMaxParts * g + k], pb = P.wp1[kMaxParts * g + k];
          const bool sph = (int)f2u(pb.w) == KIND_SPHERE;  // (bq_ray_far's and q_sweep_far's bounding sphere)
          const V3 bd = xyz(pb);
          m[k] = sph ? xyz(pa) : xyz(pa) + bd * 0.5f;
          ra[k] = sph ? pa.w : pa.w + 0.5f * mag(bd);
        }
      }
#pragma unroll
      for (uint32_t k = 0; k < (uint32_t)kMaxParts; ++k)
        if (k < np) c = c + m[k];
      c = c * (1.0f / (float)np);
      float rb = 0.0f;
#pragma unroll
      for (uint32_t k = 0; k < (uint32_t)kMaxParts; ++k)
        if (k < np) rb = fmaxf(rb, mag(m[k] - c) + ra[k]);
      rb = rb * 1.0001f + 1e-5f * q_maxabs(c) + 1e-5f;
      a = mk4(c, rb);
      b = make_float4(0.0f, 0.0f, 0.0f, u2f((uint32_t)KIND_SPHERE));
    }
    s_c0[i] = a; s_c1[i] = b; s_np[i] = pq_several(P, g) ? np | kPqSeveral : 1u;
  }
  __syncthreads();
}

// the body-level rejects (the header's argument); a = the staged sphere (C, RB)
__device__ __forceinline__ bool pq_ray_far_body(float4 a, V3 p, V3 d, float dd, float dt) {
  if (!(dd >= 1e-30f)) return false;
  const V3 w = xyz(a) - p;
  const float s = fminf(fmaxf(dot(w, d) / dd, 0.0f), dt);
  const V3 e = w - d * s;
  const float lim = a.w * 1.011f + 1.1e-3f + 0.011f * mag(w);
  return dot(e, e) > lim * lim;
}
__device__ __forceinline__ bool pq_sweep_far_body(float4 a, const SweepCast& K) {
  const V3 w = xyz(a) - K.cc;
  const float vv = dot(K.v, K.v);
  const float s = vv > 0.0f ? fminf(fmaxf(dot(w, K.v) / vv, 0.0f), 1.0f) : 0.0f;
  const V3 e = w - K.v * s;
  const float lim = (a.w + K.cr) * 1.01f + K.pad + 1e-5f * (q_maxabs(w) + q_maxabs(K.v));
  return dot(e, e) > lim * lim;
}

// q_body_box of body g: comp_bounds of its parts combined in order, or the collider row's
__device__ __forceinline__ Box pq_body_box(const BatchWorkArgs& A, const BatchPartRows& P, size_t g) {
  if (!pq_several(P, g)) return PlainBodies(A).box(g);
  Box tb = comp_bounds(to_comp(P.wp0[kMaxParts * g], P.wp1[kMaxParts * g]));
  const uint32_t np = pq_count(P, g);  // (at least 1)
  for (uint32_t k = 1; k < np; ++k) tb = box_combine(tb, comp_bounds(to_comp(P.wp0[kMaxParts * g + k], P.wp1[kMaxParts * g + k])));
  return tb;
}

// The bodies' policy of the fronts (k_batch_query.h) that sees parts.  Dynamic LDS of a ray or sweep kernel: rows | rows |
// kBatchQueryRed words | counts
struct PartBodies {
  using Best = PartBest;
  const BatchWorkArgs& A;
  const BatchPartRows& P;
  const float4 *c0 = nullptr, *c1 = nullptr;  // the staged rows ...
  const uint32_t* np = nullptr;               // ... and counts
  __device__ __forceinline__ PartBodies(const BatchWorkArgs& a, const BatchPartRows& p) : A(a), P(p) {}
  __device__ __forceinline__ void stage(uint32_t g0, uint32_t n, float4* s_dyn) {
    uint32_t* s_np = reinterpret_cast<uint32_t*>(s_dyn + 2 * (size_t)n + kBatchQueryRed);
    pq_stage(A, P, g0, n, s_dyn, s_dyn + n, s_np);
    c0 = s_dyn; c1 = s_dyn + n; np = s_np;
  }
  __device__ __forceinline__ PartBest ray_walk(const BatchWork& W, V3 p, V3 d, float dt, int32_t ign) const {
    PartBest best;
    const float dd = dot(d, d);
    for (uint32_t i = W.sub; i < W.n; i += W.L) {
      if ((int32_t)i == ign) continue;  // (an ignored body: with every part of it)
      const float4 a = c0[i], b = c1[i];
      const uint32_t cw = np[i], nk = cw & (kPqSeveral - 1u);
      const bool several = cw & kPqSeveral;
      if (several && pq_ray_far_body(a, p, d, dd, dt)) continue;
      const size_t at = (size_t)kMaxParts * ((size_t)W.g0 + i);
#pragma unroll 1
      for (uint32_t k = 0; k < nk; ++k) {
        const float4 pa = several ? P.wp0[at + k] : a, pb = several ? P.wp1[at + k] : b;
        if (bq_ray_far(pa, pb, p, d, dd, dt)) continue;
        V3 ip; float t;
        if (q_ray_comp(p, d, dt, pa, pb, &ip, &t)) best.offer(ip, t, MGF_HIT_BODY, i, k);
      }
    }
    return best;
  }
  __device__ __forceinline__ SweepBest sweep_walk(const BatchWork& W, const SweepCast& K, int32_t ign) const {
    SweepBest best;
    // (a lane's own pointers into the part rows, stepped with i: the rows' bases need no scalar registers through comp_mcomp)
    const float4 *w0 = P.wp0 + (size_t)kMaxParts * ((size_t)W.g0 + W.sub), *w1 = P.wp1 + (size_t)kMaxParts * ((size_t)W.g0 + W.sub);
    // ONE loop over (body i, part k) with one place for comp_mcomp - a loop of parts inside the loop of bodies costs the scalar
    // registers that comp_mcomp has not to spare: a trip tests part k of body i, or skips the body whole (ignored; beyond the reject)
    uint32_t k = 0u;
    for (uint32_t i = W.sub; i < W.n;) {
      const float4 a = c0[i], b = c1[i];
      const uint32_t cw = np[i], nk = cw & (kPqSeveral - 1u);
      const bool several = cw & kPqSeveral;
      bool next = (int32_t)i == ign || (several && k == 0u && pq_sweep_far_body(a, K));  // (an ignored body: with every part of it)
      if (!next) {
        const Comp t = several ? to_comp(w0[k], w1[k]) : to_comp(a, b);
        Contact ct;
        if (!q_sweep_far(t, K) && comp_mcomp(t, K.s, K.v, &ct)) best.offer(ct, MGF_HIT_BODY, i, k, 0u);
        next = ++k >= nk;
      }
      if (next) { k = 0u; i += W.L; w0 += (size_t)kMaxParts * W.L; w1 += (size_t)kMaxParts * W.L; }
    }
    return best;
  }
  __device__ __forceinline__ Box box(size_t g) const { return pq_body_box(A, P, g); }
};

// LDS (dynamic): 36 bytes a body, kBatchQueryRed words (rays, sweeps, the sensors' and the feelers' kernels); 32 bytes a body (the
// boxes' kernels).
template <int SRC>
__global__ __launch_bounds__(kBatchBlock) void k_batch_pq_ray(BatchQueryArgs A, BatchPartRows P, const ParticleIn* parts, BatchItemSrc S) {
  extern __shared__ float4 s_dyn[];
  bq_ray_item<SRC>(A, PartBodies(A, P), parts, S, s_dyn);
}
__global__ __launch_bounds__(kBatchBlock) void k_batch_pq_sensor(BatchSensorArgs A, BatchPartRows P) {
  extern __shared__ float4 s_dyn[];
  bs_rays(A, PartBodies(A, P), s_dyn);
}
template <int SRC>
__global__ __launch_bounds__(kBatchBlock) void k_batch_pq_sweep(BatchQueryArgs A, BatchPartRows P, const MovingIn* casts, BatchItemSrc S) {
  extern __shared__ float4 s_dyn[];
  bq_sweep_item<SRC>(A, PartBodies(A, P), casts, S, s_dyn);
}
__global__ __launch_bounds__(kBatchBlock) void k_batch_pq_feeler(BatchFeelerArgs A, BatchPartRows P) {
  extern __shared__ float4 s_dyn[];
  bf_casts(A, PartBodies(A, P), s_dyn);
}
template <bool FILL>
__global__ __launch_bounds__(kBatchBlock) void k_batch_pq_overlap(BatchOverlapArgs A, BatchPartRows P) {
  extern __shared__ float4 s_dyn[];
  bo_overlap<FILL>(A, PartBodies(A, P), s_dyn);
}
template <int SRC>
__global__ __launch_bounds__(kBatchBlock) void k_batch_pq_zone(BatchZoneArgs A, BatchPartRows P, BatchItemSrc S) {
  extern __shared__ float4 s_dyn[];
  bz_first<SRC>(A, PartBodies(A, P), S, s_dyn);
}
template <int SRC>
__global__ __launch_bounds__(kBatchBlock) void k_batch_pq_nearest(BatchNearestArgs A, BatchPartRows P, BatchItemSrc S) {
  extern __shared__ float4 s_dyn[];
  bn_nearest<SRC>(A, PartBodies(A, P), S, s_dyn);
}

}  // namespace mgf
