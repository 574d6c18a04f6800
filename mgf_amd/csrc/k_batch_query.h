// Ray casts and sweeps against the worlds of a batch (mgf_batch_raycast_many, mgf_batch_sweep_many; host_batch_query.inc).
// (Part of the kernel set described in kernels.h.)
//
// The definition is the lone world's (k_query.h): out[i] is what mgf_world_raycast_many / mgf_world_sweep_many reports for query i on a
// world that holds world[i]'s bodies and the batch's terrain - the same single-shape tests, the same ranking (t, kind, index, part, order
// emitted).  What differs is the work split.  A small world needs no grid: its colliders fit in LDS.
//   k_batch_query_gather        the colliders the last tick built (bpk words 0 and 3, physics.rs:243-251) into the batch's persistent rows
//                               col0 / col1; launched once behind a mgf_batch_step, before the first reader
//   k_batch_query_ray           a workgroup per work item = (world, up to 256 of its particles).  The world's col0 / col1 staged in dynamic
//                               LDS once (32 bytes a body); a particle gets 256 / (count rounded up to a power of two) lanes, which stride
//                               over the bodies behind a bounding-sphere reject; the best by the definition's order through __shfl_xor
//                               within a wave and LDS across waves; the group's first lane then walks the threaded mesh tree
//                               (BatchTerrain: no stack, no scratch) with the padded slab test bounded by the best t so far
//   k_batch_query_sweep_bodies  the same split for swept spheres and capsules: q_sweep_far, then comp_mcomp; writes the 13-word hit record
//   k_batch_query_sweep_faces   a lane per cast takes its record up again and walks the mesh tree with the padded swept box (a capsule's
//                               `reach`; `every` face for a capsule that does not move): tri_msphere / tri_mcapsule.  A launch of its own:
//                               tri_mcapsule beside comp_mcomp needs more scalar registers than there are (as k_batch_faces / k_batch_pairs)
// The order is total and every reject is conservative, so neither the number of lanes a query gets, nor the other queries of its work
// item, nor the split into launches changes a bit of an answer.  No workgroup waits for another.
#pragma once
#include "k_batch.h"
#include "k_query.h"

namespace mgf {

struct BatchQueryArgs {
  const float4* col0;     // the persistent colliders of every world's bodies, world k at [w_off[k], w_off[k + 1])
  const float4* col1;
  const uint32_t* w_off;
  BatchTerrain M;         // n_nodes 0: no terrain
  const uint4* items;     // work item: (world, first, count <= 256, -): the queries at sorted positions [first, first + count)
  const uint32_t* order;  // sorted position -> the caller's query index
  const int32_t* ignore;  // by the caller's index: a body of the query's world, -1: none; null: none for all
  int32_t mask;
  int32_t* out;           // by the caller's index: 7 words a particle (mgf_ray_hit), 13 a cast (mgf_sweep_hit)
};

constexpr uint32_t kBatchQueryRed = 16;  // float4 words behind the staged bodies: four a wave for the reduction across waves

__global__ __launch_bounds__(kBatchBlock) void k_batch_query_gather(const float4* bpk, float4* col0, float4* col1, uint32_t n) {
  const uint32_t g = blockIdx.x * kBatchBlock + threadIdx.x;
  if (g >= n) return;
  col0[g] = bpk[4 * (size_t)g];
  col1[g] = bpk[4 * (size_t)g + 3];
}

// the walk of batch_terrain_walk with any conservative test of a node's box
template <class P, class F>
__device__ __forceinline__ void batch_terrain_walk_if(const BatchTerrain& M, P&& pass, F&& emit) {
  for (uint32_t at = 0; at < M.n_nodes;) {
    const float4 n0 = M.nodes[2 * (size_t)at], n1 = M.nodes[2 * (size_t)at + 1];
    const bool hit = pass(xyz(n0), xyz(n1));
    const uint32_t w0 = f2u(n0.w);
    if (hit && (w0 & 0x80000000u)) emit(w0 & 0x7FFFFFFFu);
    at = hit ? at + 1u : f2u(n1.w);
  }
}

// lanes a query of a work item of `count` queries gets: 256 / (count rounded up to a power of two), as a shift
__device__ __forceinline__ uint32_t bq_lane_shift(uint32_t count) {
  uint32_t s = 8u;
  for (uint32_t p = 1u; p < count; p <<= 1) --s;
  return s;
}

__device__ __forceinline__ void bq_stage(const BatchQueryArgs& A, uint32_t g0, uint32_t n, float4* s_c0, float4* s_c1) {
  for (uint32_t i = threadIdx.x; i < n; i += kBatchBlock) { s_c0[i] = A.col0[(size_t)g0 + i]; s_c1[i] = A.col1[(size_t)g0 + i]; }
  __syncthreads();
}

// May the particle come within the component's bounding sphere at a parameter in [0, dt]?  Every hit of ray_sphere / ray_capsule is a
// point of the component at such a parameter; the radius carries 1 % and a millimetre, and 1e-4 |w|^2 covers the cancellation in the
// tests' discriminants for an origin far away.  (A direction whose square underflows, NaN: not far - the test decides.)
__device__ __forceinline__ bool bq_ray_far(float4 a, float4 b, V3 p, V3 d, float dd, float dt) {
  if (!(dd >= 1e-30f)) return false;
  const bool sph = (int)f2u(b.w) == KIND_SPHERE;
  const V3 bd = xyz(b);
  const V3 c = sph ? xyz(a) : xyz(a) + bd * 0.5f;
  const float R = sph ? a.w : a.w + 0.5f * mag(bd);
  const V3 w = c - p;
  const float s = fminf(fmaxf(dot(w, d) / dd, 0.0f), dt);
  const V3 e = w - d * s;
  const float lim = R * 1.01f + 1e-3f;
  return dot(e, e) > lim * lim + 1e-4f * dot(w, w);
}

__device__ __forceinline__ void bq_ray_terrain(const BatchTerrain& M, V3 p, V3 d, float dt, QueryBest& best) {
  const V3 mx = mk3(M.x[0], M.x[1], M.x[2]);
  const V3 lp = p + -mx;  // the tree's boxes are in the mesh's frame
  batch_terrain_walk_if(
      M,
      [&](V3 c, V3 r) {  // q_ray_terrain's test
        const float pad = 1e-5f * (q_maxabs(c) + q_maxabs(r) + q_maxabs(mx) + q_maxabs(p)) + 1e-6f;
        const float lim = best.have ? fminf(dt, best.t * 1.0001f + 1e-6f) : dt;
        return q_slab(lp, d, c, r, pad, lim);
      },
      [&](uint32_t f) {
        const uint4 fi = M.faces[f];
        const Triangle tri = mkt(xyz(M.verts[fi.x]) + mx, xyz(M.verts[fi.y]) + mx, xyz(M.verts[fi.z]) + mx);
        V3 ip; float t;
        if (ray_triangle(p, d, tri, &ip, &t, dt)) best.offer(ip, t, MGF_HIT_TERRAIN, f, 0u);
      });
}

// LDS (dynamic): 32 bytes a body, kBatchQueryRed words.
__global__ __launch_bounds__(kBatchBlock) void k_batch_query_ray(BatchQueryArgs A, const ParticleIn* parts) {
  extern __shared__ float4 s_dyn[];
  const uint4 it = A.items[blockIdx.x];
  const uint32_t tid = threadIdx.x, g0 = A.w_off[it.x];
  const uint32_t n = (A.mask & MGF_QUERY_BODIES) ? A.w_off[it.x + 1] - g0 : 0u;
  float4 *s_c0 = s_dyn, *s_c1 = s_dyn + n, *s_red = s_dyn + 2 * (size_t)n;
  bq_stage(A, g0, n, s_c0, s_c1);
  const uint32_t sh = bq_lane_shift(it.z), L = 1u << sh, j = tid >> sh, sub = tid & (L - 1u);
  const bool live = j < it.z;
  const uint32_t qi = live ? A.order[it.y + j] : 0u;
  V3 p = mk3(0.0f, 0.0f, 0.0f), d = p;
  float dt = 0.0f;
  int32_t ign = -1, mask = 0;
  if (live) {
    const ParticleIn q = parts[qi];
    p = ld3(q.p); d = ld3(q.d); dt = q.dt;
    ign = A.ignore ? A.ignore[qi] : -1;
    mask = A.mask;
    if (d.x == 0.0f && d.y == 0.0f && d.z == 0.0f) mask = 0;  // (no direction: no hit, by definition - k_query_ray)
  }
  QueryBest best;
  if (mask & MGF_QUERY_BODIES) {
    const float dd = dot(d, d);
    for (uint32_t i = sub; i < n; i += L) {
      if ((int32_t)i == ign) continue;
      const float4 a = s_c0[i], b = s_c1[i];
      if (bq_ray_far(a, b, p, d, dd, dt)) continue;
      V3 ip; float t;
      if (q_ray_comp(p, d, dt, a, b, &ip, &t)) best.offer(ip, t, MGF_HIT_BODY, i, 0u);
    }
  }
  // the best of the query's lanes: within the wave ...
  for (uint32_t off = min(L, 64u) >> 1; off > 0u; off >>= 1) {
    const int ok = __shfl_xor(best.have ? best.kind : -1, (int)off);
    const uint32_t oi = (uint32_t)__shfl_xor((int)best.index, (int)off);
    const float ox = __shfl_xor(best.p.x, (int)off), oy = __shfl_xor(best.p.y, (int)off), oz = __shfl_xor(best.p.z, (int)off);
    const float ot = __shfl_xor(best.t, (int)off);
    if (ok >= 0) best.offer(mk3(ox, oy, oz), ot, ok, oi, 0u);
  }
  // ... and across the waves of a query that has more than one
  if (L > 64u) {
    const uint32_t wv = tid >> 6;
    if ((tid & 63u) == 0u) {
      s_red[2 * wv] = make_float4(u2f((uint32_t)(best.have ? best.kind : -1)), u2f(best.index), best.t, 0.0f);
      s_red[2 * wv + 1] = mk4(best.p, 0.0f);
    }
    __syncthreads();
    if (sub == 0u)
      for (uint32_t w = wv + 1u; w < wv + (L >> 6); ++w) {
        const float4 r0 = s_red[2 * w], r1 = s_red[2 * w + 1];
        if ((int)f2u(r0.x) >= 0) best.offer(xyz(r1), r0.z, (int)f2u(r0.x), f2u(r0.y), 0u);
      }
  }
  if (sub != 0u || !live) return;
  if ((mask & MGF_QUERY_TERRAIN) && A.M.n_nodes) bq_ray_terrain(A.M, p, d, dt, best);
  int32_t* o = A.out + 7 * (size_t)qi;
  if (best.have) {
    o[0] = best.kind; o[1] = (int32_t)best.index; o[2] = (int32_t)best.part;
    o[3] = (int32_t)f2u(best.p.x); o[4] = (int32_t)f2u(best.p.y); o[5] = (int32_t)f2u(best.p.z); o[6] = (int32_t)f2u(best.t);
  } else {
    o[0] = MGF_HIT_NONE; o[1] = 0; o[2] = 0; o[3] = 0; o[4] = 0; o[5] = 0; o[6] = 0;
  }
}

// q_sweep_cast without a grid: the reject's pad keeps its millimetre and the rounding of the path
__device__ __forceinline__ SweepCast bq_sweep_cast(const MovingIn& m) {
  QueryGrid G;
  G.margin = 0.0f;
  return q_sweep_cast(m, G);
}
__device__ __forceinline__ void bq_sweep_merge(SweepBest& best, int tk, uint64_t sub, const Contact& c) {
  if (tk < best.tk || (tk == best.tk && sub < best.sub)) { best.tk = tk; best.sub = sub; best.c = c; }
}

// LDS (dynamic): 32 bytes a body, kBatchQueryRed words.
__global__ __launch_bounds__(kBatchBlock) void k_batch_query_sweep_bodies(BatchQueryArgs A, const MovingIn* casts) {
  extern __shared__ float4 s_dyn[];
  const uint4 it = A.items[blockIdx.x];
  const uint32_t tid = threadIdx.x, g0 = A.w_off[it.x];
  const uint32_t n = (A.mask & MGF_QUERY_BODIES) ? A.w_off[it.x + 1] - g0 : 0u;
  float4 *s_c0 = s_dyn, *s_c1 = s_dyn + n, *s_red = s_dyn + 2 * (size_t)n;
  bq_stage(A, g0, n, s_c0, s_c1);
  const uint32_t sh = bq_lane_shift(it.z), L = 1u << sh, j = tid >> sh, sub = tid & (L - 1u);
  const bool live = j < it.z;
  const uint32_t qi = live ? A.order[it.y + j] : 0u;
  SweepBest best;
  if (live && n) {
    const SweepCast K = bq_sweep_cast(casts[qi]);
    const int32_t ign = A.ignore ? A.ignore[qi] : -1;
    for (uint32_t i = sub; i < n; i += L) {
      if ((int32_t)i == ign) continue;
      const float4 a = s_c0[i], b = s_c1[i];
      Comp t; t.kind = (int)f2u(b.w); t.p = xyz(a); t.d = xyz(b); t.r = a.w;
      if (q_sweep_far(t, K)) continue;
      Contact c;
      if (comp_mcomp(t, K.s, K.v, &c)) best.offer(c, MGF_HIT_BODY, i, 0u, 0u);
    }
  }
  for (uint32_t off = min(L, 64u) >> 1; off > 0u; off >>= 1) {
    const int otk = __shfl_xor(best.tk, (int)off);
    const uint32_t olo = (uint32_t)__shfl_xor((int)(uint32_t)best.sub, (int)off), ohi = (uint32_t)__shfl_xor((int)(uint32_t)(best.sub >> 32), (int)off);
    Contact oc;
    oc.a = mk3(__shfl_xor(best.c.a.x, (int)off), __shfl_xor(best.c.a.y, (int)off), __shfl_xor(best.c.a.z, (int)off));
    oc.b = mk3(__shfl_xor(best.c.b.x, (int)off), __shfl_xor(best.c.b.y, (int)off), __shfl_xor(best.c.b.z, (int)off));
    oc.n = mk3(__shfl_xor(best.c.n.x, (int)off), __shfl_xor(best.c.n.y, (int)off), __shfl_xor(best.c.n.z, (int)off));
    oc.t = __shfl_xor(best.c.t, (int)off);
    bq_sweep_merge(best, otk, ((uint64_t)ohi << 32) | olo, oc);
  }
  if (L > 64u) {
    const uint32_t wv = tid >> 6;
    if ((tid & 63u) == 0u) {
      s_red[4 * wv] = make_float4(u2f((uint32_t)best.tk), u2f((uint32_t)best.sub), u2f((uint32_t)(best.sub >> 32)), best.c.t);
      s_red[4 * wv + 1] = mk4(best.c.a, 0.0f); s_red[4 * wv + 2] = mk4(best.c.b, 0.0f); s_red[4 * wv + 3] = mk4(best.c.n, 0.0f);
    }
    __syncthreads();
    if (sub == 0u)
      for (uint32_t w = wv + 1u; w < wv + (L >> 6); ++w) {
        const float4 r0 = s_red[4 * w];
        bq_sweep_merge(best, (int)f2u(r0.x), ((uint64_t)f2u(r0.z) << 32) | f2u(r0.y), mkc(xyz(s_red[4 * w + 1]), xyz(s_red[4 * w + 2]), xyz(s_red[4 * w + 3]), r0.w));
      }
  }
  if (sub != 0u || !live) return;
  q_sweep_store(A.out + 13 * (size_t)qi, best);
}

// q_sweep_terrain's tests over the threaded tree, a lane per cast (in the caller's order: the faces are the same for every world)
__global__ __launch_bounds__(kBatchBlock) void k_batch_query_sweep_faces(BatchTerrain M, const MovingIn* casts, uint32_t n, int32_t* out) {
  const uint32_t i = blockIdx.x * kBatchBlock + threadIdx.x;
  if (i >= n) return;
  const SweepCast K = bq_sweep_cast(casts[i]);
  int32_t* o = out + 13 * (size_t)i;
  SweepBest best;
  if (o[0] != MGF_HIT_NONE)  // k_batch_query_sweep_bodies' answer (its order within a target does not matter here: this launch offers faces only)
    best.offer(mkc(mk3(u2f(o[3]), u2f(o[4]), u2f(o[5])), mk3(u2f(o[6]), u2f(o[7]), u2f(o[8])), mk3(u2f(o[9]), u2f(o[10]), u2f(o[11])), u2f(o[12])), o[0],
               (uint32_t)o[1], (uint32_t)o[2], 0u);
  const bool every = K.s.kind != KIND_SPHERE && mag2(K.v) == 0.0f;
  const float reach = K.s.kind == KIND_SPHERE ? 0.0f : fmaxf(1.0f, mag(K.s.d));
  const V3 mx = mk3(M.x[0], M.x[1], M.x[2]);
  Box q = swept_bounds(K.s, K.v);
  q.c = q.c + -mx;  // the tree's boxes are in the mesh's frame
  batch_terrain_walk_if(
      M,
      [&](V3 c, V3 r) {
        const float pad = 1e-5f * (q_maxabs(c) + q_maxabs(r) + q_maxabs(mx) + q_maxabs(q.c) + q_maxabs(q.r)) + 1e-6f + reach;
        return every || (fabsf(c.x - q.c.x) <= r.x + q.r.x + pad && fabsf(c.y - q.c.y) <= r.y + q.r.y + pad && fabsf(c.z - q.c.z) <= r.z + q.r.z + pad);
      },
      [&](uint32_t f) {
        const uint4 fi = M.faces[f];
        const Triangle tri = mkt(xyz(M.verts[fi.x]) + mx, xyz(M.verts[fi.y]) + mx, xyz(M.verts[fi.z]) + mx);
        Contact c0, c1;
        if (K.s.kind == KIND_SPHERE) {
          if (tri_msphere(tri, mks(K.s.p, K.s.r), K.v, &c0)) best.offer(c0, MGF_HIT_TERRAIN, f, 0u, 0u);
        } else {
          const int m = tri_mcapsule(tri, mkcap(K.s.p, K.s.d, K.s.r), K.v, c0, c1);
          if (m > 0) best.offer(c0, MGF_HIT_TERRAIN, f, 0u, 0u);
          if (m > 1) best.offer(c1, MGF_HIT_TERRAIN, f, 0u, 1u);
        }
      });
  q_sweep_store(o, best);
}

}  // namespace mgf
