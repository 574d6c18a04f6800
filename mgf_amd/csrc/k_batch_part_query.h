// Rays, sweeps and box queries of a batch that see the parts of bodies of several components (option "part_queries" on a batch that
// holds part storage; host_batch_part_query.inc).  (Part of the kernel set described in kernels.h.)
//
// The definition is the lone world's (k_query.h: q_ray_body, q_sweep_body, q_body_box): every part of every body not ignored goes through
// q_ray_comp / comp_mcomp, an ordinary body is its collider row and reports part 0, the ranking is (t, kind, index, part) for a ray and
// SweepBest's (t, kind, index, part, order) for a cast, a body's box is comp_bounds of its parts combined in order with box_combine.  The
// parts are the world parts wp0 / wp1 (four slots a body: written when the body is added and by k_batch_parts_front every tick), the
// part count the second word of the constructor row of a body whose first word is 2 (batch_np, k_batch_parts.h) - taken as
// min(count, kMaxParts), so that a bad word in memory cannot lengthen a loop.
// The work split is k_batch_query.h's and k_batch_observe.h's, restated here so that those kernels keep their compiler figures: a
// workgroup per work item, 256 / next_pow2(count) lanes a query, bq_reduce across lanes and waves; the box fronts a query's lanes in
// one wave and a hit's rank from the ballot.
//   k_batch_pq_ray<SRC>      bq_ray_item over pq_ray_front      k_batch_pq_sensor    k_batch_sensor_ray over pq_ray_front
//   k_batch_pq_sweep<SRC>    bq_sweep_item over pq_sweep_front  k_batch_pq_feeler    k_batch_feeler_bodies over pq_sweep_front
//   k_batch_pq_overlap<FILL> k_batch_observe_overlap, k_batch_pq_zone<SRC> k_batch_zone_first, k_batch_pq_nearest<SRC> k_batch_nearest,
//                            each over pq_bo_front: only the staging differs - the staged box is the union of the parts' bounds
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
// BARRIERS.  As in the fronts restated: no lane leaves ahead of a __syncthreads (kItemPlan: a whole workgroup at or beyond the item
// total leaves before the first); the only other exit is behind bq_reduce; every lane of a wave makes every trip of a ballot loop.
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

// the dynamic LDS of the ray and sweep fronts: rows | rows | kBatchQueryRed words | counts
struct PqLds {
  float4 *c0, *c1, *red;
  uint32_t* np;
  __device__ __forceinline__ PqLds(float4* s_dyn, uint32_t n) : c0(s_dyn), c1(s_dyn + n), red(s_dyn + 2 * (size_t)n) {
    np = reinterpret_cast<uint32_t*>(red + kBatchQueryRed);
  }
};

// bq_ray_front over parts (its remarks hold: load(qi, g0) -> BatchRay, done(qi, p, d, dt))
template <int SRC, class Load, class Done>
__device__ __forceinline__ void pq_ray_front(const BatchQueryArgs& A, const BatchPartRows& P, const BatchItemSrc& S, float4* s_dyn, Load&& load, Done&& done) {
  if (SRC == kItemPlan && blockIdx.x >= *S.n_items) return;
  BatchWork W(A, A.mask & MGF_QUERY_BODIES, bq_item<SRC>(A, S));
  const uint32_t n = W.n;
  const PqLds s(s_dyn, n);
  pq_stage(A, P, W.g0, n, s.c0, s.c1, s.np);
  W.template split<SRC == kItemFixed>(A, W.shift());
  const uint32_t qi = W.qi;
  V3 p = mk3(0.0f, 0.0f, 0.0f), d = p;
  float dt = 0.0f;
  int32_t ign = -1, mask = 0;
  if (W.live) {
    const BatchRay r = load(qi, W.g0);
    p = r.p; d = r.d; dt = r.dt; ign = r.ign;
    mask = A.mask;
    if (d.x == 0.0f && d.y == 0.0f && d.z == 0.0f) mask = 0;  // (no direction: no hit, by definition - k_query_ray)
  }
  PartBest best;
  if (mask & MGF_QUERY_BODIES) {
    const float dd = dot(d, d);
    for (uint32_t i = W.sub; i < n; i += W.L) {
      if ((int32_t)i == ign) continue;  // (an ignored body: with every part of it)
      const float4 a = s.c0[i], b = s.c1[i];
      const uint32_t cw = s.np[i], np = cw & (kPqSeveral - 1u);
      const bool several = cw & kPqSeveral;
      if (several && pq_ray_far_body(a, p, d, dd, dt)) continue;
      const size_t at = (size_t)kMaxParts * ((size_t)W.g0 + i);
#pragma unroll 1
      for (uint32_t k = 0; k < np; ++k) {
        const float4 pa = several ? P.wp0[at + k] : a, pb = several ? P.wp1[at + k] : b;
        if (bq_ray_far(pa, pb, p, d, dd, dt)) continue;
        V3 ip; float t;
        if (q_ray_comp(p, d, dt, pa, pb, &ip, &t)) best.offer(ip, t, MGF_HIT_BODY, i, k);
      }
    }
  }
  bq_reduce(best, W, s.red);
  if (W.sub != 0u || !W.live) return;
  if (mask & MGF_QUERY_TERRAIN) {
    const BatchTerrain M = batch_terrain_of(A.T, W.it.x);  // (the work item's world: wave-uniform loads)
    if (M.n_nodes) q_ray_terrain(M, p, d, dt, nullptr, best);
  }
  q_ray_store(A.out + 7 * (size_t)qi, best);
  done(qi, p, d, dt);
}

// LDS (dynamic): 36 bytes a body, kBatchQueryRed words.
template <int SRC>
__global__ __launch_bounds__(kBatchBlock) void k_batch_pq_ray(BatchQueryArgs A, BatchPartRows P, const ParticleIn* parts, BatchItemSrc S) {
  extern __shared__ float4 s_dyn[];
  pq_ray_front<SRC>(
      A, P, S, s_dyn,
      [&](uint32_t qi, uint32_t) {
        const ParticleIn q = parts[qi];
        return BatchRay{ld3(q.p), ld3(q.d), q.dt, A.ignore ? A.ignore[qi] : -1};
      },
      [](uint32_t, V3, V3, float) {});
}
// k_batch_sensor_ray's loader and store (k_batch_sensor.h)
__global__ __launch_bounds__(kBatchBlock) void k_batch_pq_sensor(BatchSensorArgs A, BatchPartRows P) {
  extern __shared__ float4 s_dyn[];
  pq_ray_front<kItemTable>(
      A, P, BatchItemSrc(), s_dyn,
      [&](uint32_t qi, uint32_t g0) {
        const SensorIn s = A.rig[qi];
        const size_t g = (size_t)g0 + (uint32_t)s.body;
        const float4 bx = A.x[g], bq = A.q[g];
        const Quat rot = mkq(bq.x, mk3(bq.y, bq.z, bq.w));
        return BatchRay{xyz(bx) + rotate(rot, ld3(s.p)), rotate(rot, ld3(s.d)), s.dt, (s.flags & MGF_SENSOR_IGNORE_SELF) ? s.body : -1};
      },
      [&](uint32_t qi, V3 p, V3 d, float dt) {
        if (A.parts) {
          float* o = A.parts + 7 * (size_t)qi;
          o[0] = p.x; o[1] = p.y; o[2] = p.z; o[3] = d.x; o[4] = d.y; o[5] = d.z; o[6] = dt;
        }
      });
}

// bq_sweep_item and bf_sweep_front over parts, one front with a loader - load(qi, g0) -> BatchCast, run by the live lanes behind the
// staging - and done(qi, m) behind the stored hit.  No loader reads the staged rows (the feelers' takes a body's own shape from col0 /
// col1): a mask without bodies stages nothing.  kItemFixed: a cast whose tag is no component's is matched against nothing, keeps the
// no-hit record and is counted by the first of its lanes (bq_sweep_item).
template <int SRC, class Load, class Done>
__device__ __forceinline__ void pq_sweep_front(const BatchQueryArgs& A, const BatchPartRows& P, const BatchItemSrc& S, float4* s_dyn, Load&& load, Done&& done) {
  if (SRC == kItemPlan && blockIdx.x >= *S.n_items) return;
  BatchWork W(A, A.mask & MGF_QUERY_BODIES, bq_item<SRC>(A, S));
  const uint32_t n = W.n;
  const PqLds s(s_dyn, n);
  pq_stage(A, P, W.g0, n, s.c0, s.c1, s.np);
  W.template split<SRC == kItemFixed>(A, W.shift());
  const uint32_t qi = W.qi;
  SweepBest best;
  BatchCast c;
  bool ok = W.live;
  if (ok) {
    c = load(qi, W.g0);
    if (SRC == kItemFixed && (uint32_t)c.m.tag > (uint32_t)KIND_CAPSULE) {
      ok = false;
      if (W.sub == 0u) atomicAdd(S.skipped, 1ull);
    }
  }
  if (ok && n) {  // (n: the mask asks for bodies, and the world has some)
    const SweepCast K = bq_sweep_cast(c.m);
    const int32_t ign = c.ign;
    // (a lane's own pointers into the part rows, stepped with i: the rows' bases need no scalar registers through comp_mcomp)
    const float4 *w0 = P.wp0 + (size_t)kMaxParts * ((size_t)W.g0 + W.sub), *w1 = P.wp1 + (size_t)kMaxParts * ((size_t)W.g0 + W.sub);
    // ONE loop over (body i, part k) with one place for comp_mcomp - a loop of parts inside the loop of bodies costs the scalar
    // registers that comp_mcomp has not to spare: a trip tests part k of body i, or skips the body whole (ignored; beyond the reject)
    uint32_t k = 0u;
    for (uint32_t i = W.sub; i < n;) {
      const float4 a = s.c0[i], b = s.c1[i];
      const uint32_t cw = s.np[i], np = cw & (kPqSeveral - 1u);
      const bool several = cw & kPqSeveral;
      bool next = (int32_t)i == ign || (several && k == 0u && pq_sweep_far_body(a, K));  // (an ignored body: with every part of it)
      if (!next) {
        const Comp t = several ? to_comp(w0[k], w1[k]) : to_comp(a, b);
        Contact ct;
        if (!q_sweep_far(t, K) && comp_mcomp(t, K.s, K.v, &ct)) best.offer(ct, MGF_HIT_BODY, i, k, 0u);
        next = ++k >= np;
      }
      if (next) { k = 0u; i += W.L; w0 += (size_t)kMaxParts * W.L; w1 += (size_t)kMaxParts * W.L; }
    }
  }
  bq_reduce(best, W, s.red);
  if (W.sub != 0u || !W.live) return;
  q_sweep_store(A.out + 13 * (size_t)qi, best);
  done(qi, c.m);
}

// LDS (dynamic): 36 bytes a body, kBatchQueryRed words.
template <int SRC>
__global__ __launch_bounds__(kBatchBlock) void k_batch_pq_sweep(BatchQueryArgs A, BatchPartRows P, const MovingIn* casts, BatchItemSrc S) {
  extern __shared__ float4 s_dyn[];
  pq_sweep_front<SRC>(
      A, P, S, s_dyn, [&](uint32_t qi, uint32_t) { return BatchCast{casts[qi], A.ignore ? A.ignore[qi] : -1}; }, [](uint32_t, const MovingIn&) {});
}
// k_batch_feeler_bodies' loader and store (k_batch_feeler.h).  MGF_FEELER_OWN_SHAPE: the body's collider row as mgf_batch_read_colliders
// packs it, read from col0 / col1 - for a body of several parts a radius-0 sphere at the centre of mass (its staged rows hold the
// reject sphere, which is no shape of the body).
__global__ __launch_bounds__(kBatchBlock) void k_batch_pq_feeler(BatchFeelerArgs A, BatchPartRows P) {
  extern __shared__ float4 s_dyn[];
  pq_sweep_front<kItemTable>(
      A, P, BatchItemSrc(), s_dyn,
      [&](uint32_t qi, uint32_t g0) {
        const FeelerIn f = A.rig[qi];
        const size_t g = (size_t)g0 + (uint32_t)f.body;
        const float4 bx = A.x[g], bq = A.q[g];
        const Quat rot = mkq(bq.x, mk3(bq.y, bq.z, bq.w));
        BatchCast c;
        V3 Pw, D;
        if (f.flags & MGF_FEELER_OWN_SHAPE) {  // (k_pack_colliders' words)
          const float4 a = A.col0[g], b = A.col1[g];
          c.m.tag = (int)f2u(b.w); c.m.r = a.w;
          Pw = xyz(a); D = xyz(b);
        } else {
          c.m.tag = f.tag; c.m.r = f.r;
          Pw = xyz(bx) + rotate(rot, ld3(f.p)); D = rotate(rot, ld3(f.d));
        }
        const V3 v = (f.flags & MGF_FEELER_WORLD_DELTA) ? ld3(f.delta) : rotate(rot, ld3(f.delta));
        c.m.p[0] = Pw.x; c.m.p[1] = Pw.y; c.m.p[2] = Pw.z;
        c.m.d[0] = D.x; c.m.d[1] = D.y; c.m.d[2] = D.z;
        c.m.delta[0] = v.x; c.m.delta[1] = v.y; c.m.delta[2] = v.z;
        c.ign = (f.flags & MGF_FEELER_IGNORE_SELF) ? f.body : -1;
        return c;
      },
      [&](uint32_t qi, const MovingIn& m) { A.casts[qi] = m; });
}

// ---- boxes ----------------------------------------------------------------------------------------------------------------------------
// q_body_box of body g: comp_bounds of its parts combined in order, or comp_bounds of the collider row
__device__ __forceinline__ Box pq_body_box(const BatchWorkArgs& A, const BatchPartRows& P, size_t g) {
  if (!pq_several(P, g)) return comp_bounds(to_comp(A.col0[g], A.col1[g]));
  Box tb = comp_bounds(to_comp(P.wp0[kMaxParts * g], P.wp1[kMaxParts * g]));
  const uint32_t np = pq_count(P, g);  // (at least 1)
  for (uint32_t k = 1; k < np; ++k) tb = box_combine(tb, comp_bounds(to_comp(P.wp0[kMaxParts * g + k], P.wp1[kMaxParts * g + k])));
  return tb;
}

// KEEP IN STEP: pq_bo_front, k_batch_pq_overlap, k_batch_pq_zone and k_batch_pq_nearest are bo_front, k_batch_observe_overlap,
// k_batch_zone_first and k_batch_nearest (k_batch_observe.h, k_batch_zone.h, k_batch_nearest.h) line for line behind the staging: a
// change to one of those is made here as well.  They are restated, not shared, because the host tests of those kernels hold bo_front's
// text and template list and the kernels' bodies as they stand, and their compiler figures.
// bo_front (k_batch_observe.h; its remarks hold) with the bodies' boxes staged from their parts
template <bool IDENTITY, bool IGNORE, class Load, class Put>
__device__ __forceinline__ uint32_t pq_bo_front(const BatchWorkArgs& A, const BatchPartRows& P, BatchWork& W, float4* s_dyn, BatchBox& z, Load&& load, Put&& put) {
  const uint32_t tid = threadIdx.x, g0 = W.g0, n = W.n;
  float4 *s_c = s_dyn, *s_r = s_dyn + n;
  for (uint32_t i = tid; i < n; i += kBatchBlock) {
    const Box tb = pq_body_box(A, P, (size_t)g0 + i);
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

// LDS (dynamic): 32 bytes a body.
template <bool FILL>
__global__ __launch_bounds__(kBatchBlock) void k_batch_pq_overlap(BatchOverlapArgs A, BatchPartRows P) {
  extern __shared__ float4 s_dyn[];
  BatchWork W(A, true);
  BatchBox z;
  uint32_t base = 0u;  // FILL: where the box's list begins
  const uint32_t m = pq_bo_front<false, false>(
      A, P, W, s_dyn, z,
      [&](uint32_t qi, uint32_t) {
        if (FILL) base = A.off[qi];
        return BatchBox{{ld3(A.boxes + 6 * (size_t)qi), ld3(A.boxes + 6 * (size_t)qi + 3)}, -1};
      },
      [&](bool hit, uint32_t i, uint32_t rank) {
        if (FILL && hit) A.out[base + rank] = i;
      });
  if (!FILL && W.live && W.sub == 0u) A.cnt[W.qi] = m;
}

// the two loaders of a zone's box (k_batch_zone_first's): the caller's, and the one formed from the rig's record and the body's x and q
__device__ __forceinline__ BatchBox pq_zone_fixed(const BatchZoneArgs& A, uint32_t qi) {
  return BatchBox{{ld3(A.boxes + 6 * (size_t)qi), ld3(A.boxes + 6 * (size_t)qi + 3)}, A.ignore ? A.ignore[qi] : -1};
}
__device__ __forceinline__ BatchBox pq_zone_mounted(const BatchZoneArgs& A, uint32_t qi, uint32_t g0) {
  const ZoneIn s = A.rig[qi];
  BatchBox b;
  b.Q.c = ld3(s.p); b.Q.r = ld3(s.r);
  if (s.body >= 0) {
    const size_t g = (size_t)g0 + (uint32_t)s.body;
    const float4 bx = A.x[g], bq = A.q[g];
    b.Q.c = xyz(bx) + rotate(mkq(bq.x, mk3(bq.y, bq.z, bq.w)), ld3(s.p));
  }
  b.ign = (s.flags & MGF_SENSOR_IGNORE_SELF) ? s.body : -1;
  return b;
}
__device__ __forceinline__ void pq_zone_box_out(float* boxes_out, uint32_t qi, const Box& Q) {
  float* bo = boxes_out + 6 * (size_t)qi;
  bo[0] = Q.c.x; bo[1] = Q.c.y; bo[2] = Q.c.z; bo[3] = Q.r.x; bo[4] = Q.r.y; bo[5] = Q.r.z;
}

// LDS (dynamic): 32 bytes a body.  k_batch_zone_first over pq_bo_front.
template <int SRC>
__global__ __launch_bounds__(kBatchBlock) void k_batch_pq_zone(BatchZoneArgs A, BatchPartRows P, BatchItemSrc S) {
  extern __shared__ float4 s_dyn[];
  BatchWork W(A, true, bq_item<SRC>(A, S));
  const uint32_t k = A.k;
  BatchBox z;
  const auto fixed = [&](uint32_t qi, uint32_t) { return pq_zone_fixed(A, qi); };
  const auto mounted = [&](uint32_t qi, uint32_t g0) { return pq_zone_mounted(A, qi, g0); };
  const auto record = [&]() { return A.out + (size_t)(1u + k) * W.qi; };  // (of a live lane, W split)
  const auto store = [&](bool hit, uint32_t i, uint32_t rank) {
    if (hit && rank < k) record()[1u + rank] = (int32_t)i;
  };
  const uint32_t m = SRC == kItemFixed ? pq_bo_front<true, true>(A, P, W, s_dyn, z, fixed, store) : pq_bo_front<false, true>(A, P, W, s_dyn, z, mounted, store);
  if (W.live) {
    const uint32_t sub = W.sub;
    int32_t* o = record();
    if (sub == 0u) o[0] = (int32_t)m;
    for (uint32_t s = min(m, k) + sub; s < k; s += W.L) o[1u + s] = -1;
    if (sub == 0u && A.boxes_out) pq_zone_box_out(A.boxes_out, W.qi, z.Q);
  }
}

// LDS (dynamic): 32 bytes a body.  k_batch_nearest over pq_bo_front: the distances are measured from the centre of the staged box.
template <int SRC>
__global__ __launch_bounds__(kBatchBlock) void k_batch_pq_nearest(BatchNearestArgs A, BatchPartRows P, BatchItemSrc S) {
  extern __shared__ float4 s_dyn[];
  BatchWork W(A, true, bq_item<SRC>(A, S));
  const uint32_t k = A.k;
  BatchBox z;
  const auto fixed = [&](uint32_t qi, uint32_t) { return pq_zone_fixed(A, qi); };
  const auto mounted = [&](uint32_t qi, uint32_t g0) { return pq_zone_mounted(A, qi, g0); };
  const auto count_only = [](bool, uint32_t, uint32_t) {};
  const uint32_t m = SRC == kItemFixed ? pq_bo_front<true, true>(A, P, W, s_dyn, z, fixed, count_only) : pq_bo_front<false, true>(A, P, W, s_dyn, z, mounted, count_only);
  const uint32_t n = W.n, L = W.L, sub = W.sub;
  const bool live = W.live, first = live && sub == 0u;
  const float4 *s_c = s_dyn, *s_r = s_dyn + n;  // (as the front staged them)
  const Box Q = z.Q;
  const int32_t ign = z.ign;
  int32_t* o = A.out + (size_t)(1u + k) * W.qi;  // (of a live lane)
  float* od = A.dist2_out ? A.dist2_out + (size_t)k * W.qi : nullptr;
  const auto put = [&](uint32_t slot, uint64_t key) {  // (of the zone's first lane) slot < k: the record's word 1 + slot, its distance
    const bool none = key == kNearestNone;
    o[1u + slot] = none ? -1 : (int32_t)(uint32_t)key;
    if (od) od[slot] = none ? u2f(0x7F800000u) : u2f((uint32_t)(key >> 32));
  };
  uint64_t lo = 0ull;  // the least key a pass may choose: one above the last chosen
  for (uint32_t r0 = 0; r0 < k; r0 += 4u) {
    NearestPick best;
    best.clear();
#pragma unroll 2
    for (uint32_t i0 = 0; i0 < n; i0 += L) {  // (n and L are the work item's: every lane of the wave makes every trip)
      const uint32_t i = i0 + sub, at = min(i, n - 1u);
      const V3 bc = xyz(s_c[at]), br = xyz(s_r[at]);
      const V3 e = bc - Q.c;
      const float ax = fabs_rs(e.x), ay = fabs_rs(e.y), az = fabs_rs(e.z);  // box_overlaps(body, Q): its three tests, no early exit
      const bool hit = (ax <= (br.x + Q.r.x)) & (ay <= (br.y + Q.r.y)) & (az <= (br.z + Q.r.z));
      const uint64_t key = ((uint64_t)f2u(dot(e, e)) << 32) | i;
      const bool ok = live & (i < n) & ((int32_t)i != ign) & hit & (key >= lo);
      best.put(ok ? key : kNearestNone);
    }
    for (uint32_t off = L >> 1; off > 0u; off >>= 1) best.merge(best.shfl((int)off));
    if (first) {
      put(r0, best.t0);
      if (r0 + 1u < k) put(r0 + 1u, best.t1);
      if (r0 + 2u < k) put(r0 + 2u, best.t2);
      if (r0 + 3u < k) put(r0 + 3u, best.t3);
    }
    lo = best.t3 == kNearestNone ? kNearestNone : best.t3 + 1ull;
  }
  if (first) {
    o[0] = (int32_t)m;
    if (A.boxes_out) pq_zone_box_out(A.boxes_out, W.qi, Q);
  }
}

}  // namespace mgf
