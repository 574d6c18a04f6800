// Ray casts and sweeps against the worlds of a batch (mgf_batch_raycast_many, mgf_batch_sweep_many; host_batch_query.inc).
// (Part of the kernel set described in kernels.h.)
//
// The definition is the lone world's (k_query.h): out[i] is what mgf_world_raycast_many / mgf_world_sweep_many reports for query i on a
// world that holds world[i]'s bodies and that world's terrain (BatchTerrains, k_batch.h) - the same single-shape tests, the same ranking (t, kind, index, part, order
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
//   k_batch_query_ray_obstacles / k_batch_query_sweep_obstacles
//                               a lane per query takes its record up again and puts the query through the obstacles of its world in list
//                               order: q_ray_obstacle (Intersects<Compound>) and compound_contacts_walk (Compound::contacts), the lone
//                               world's own, over the threaded trees of the batch's obstacle table (BatchObstacles, k_batch.h).  Launched
//                               only when the mask asks for obstacles and a world of the batch has one
// Every test, the ranking and the records are k_query.h's own (q_ray_terrain / q_sweep_terrain, QueryBest / SweepBest, q_*_store, q_sweep_load);
// here are the work split (BatchWork), the staging, the cheap rejects and the reduction over a query's lanes (bq_reduce).
// The order is total and every reject is conservative, so neither the number of lanes a query gets, nor the other queries of its work
// item, nor the split into launches changes a bit of an answer.  No workgroup waits for another.
// The two kernels with a workgroup per work item are bq_ray_item<SRC> / bq_sweep_item<SRC> behind a kernel's signature: SRC says where
// the work item comes from - the host's table here (kItemTable), the device-built table or arithmetic on blockIdx.x for the
// device-pointer calls (kItemPlan, kItemFixed: k_batch_query_dev.h).  They are bq_ray_front / bq_sweep_front - the front of a ray cast
// and of a sweep, each written once - over the caller's particles and casts; k_batch_sensor_ray (k_batch_sensor.h) and
// k_batch_feeler_bodies (k_batch_feeler.h) are the same fronts over particles and casts formed from a rig, and the kernels of
// k_batch_part_query.h the same fronts again over bodies that show their parts: what the bodies of a world are to a front is a policy
// (PlainBodies, PartBodies - below, at PlainBodies).  The three lane-per-query passes take the world of query i from
// world[i], or (world == null: every world has `per` queries) as i / per, and leave at once for a negative world - a record the
// device-pointer calls skip - and for a cast whose tag is no component's; the host-memory calls refuse both before anything runs.
#pragma once
#include "k_batch.h"
#include "k_query.h"

namespace mgf {

// what every kernel with a workgroup per work item reads (k_batch_observe_overlap too)
struct BatchWorkArgs {
  const float4* col0;     // the persistent colliders of every world's bodies, world k at [w_off[k], w_off[k + 1])
  const float4* col1;
  const uint32_t* w_off;
  const uint4* items;     // work item: (world, first, count <= 256, -): the queries at sorted positions [first, first + count)
  const uint32_t* order;  // sorted position -> the caller's query index
};
struct BatchQueryArgs : BatchWorkArgs {
  BatchTerrains T;        // a world's terrain: batch_terrain_of(T, world)
  const int32_t* ignore;  // by the caller's index: a body of the query's world, -1: none; null: none for all
  int32_t mask;
  int32_t* out;           // by the caller's index: 7 words a particle (mgf_ray_hit), 13 a cast (mgf_sweep_hit)
};

// Where a workgroup's work item comes from: items[blockIdx.x] as the host wrote it; items[blockIdx.x] of a table built on the device,
// whose length only the device knows (*n_items; the grid is an upper bound); or no table: every world has `per` queries, world k's at
// [k * per, (k + 1) * per) in the caller's order, cut into ceil(per / 256) work items.
enum : int { kItemTable = 0, kItemPlan = 1, kItemFixed = 2 };
struct BatchItemSrc {
  const uint32_t* n_items;      // kItemPlan: the work items of the call
  uint32_t per;                 // kItemFixed: queries a world (> 0)
  unsigned long long* skipped;  // kItemFixed: casts skipped for their tag, cumulative (the plan counts them itself)
};
template <int SRC>
__device__ __forceinline__ uint4 bq_item(const BatchWorkArgs& A, const BatchItemSrc& S) {
  if (SRC != kItemFixed) return A.items[blockIdx.x];
  const uint32_t cuts = (S.per + 255u) >> 8, k = blockIdx.x / cuts, f = (blockIdx.x - k * cuts) << 8;
  return make_uint4(k, k * S.per + f, min(256u, S.per - f), 0u);
}

constexpr uint32_t kBatchQueryRed = 16;  // float4 words behind the staged bodies: four a wave for the reduction across waves

__global__ __launch_bounds__(kBatchBlock) void k_batch_query_gather(const float4* bpk, float4* col0, float4* col1, uint32_t n) {
  const uint32_t g = blockIdx.x * kBatchBlock + threadIdx.x;
  if (g >= n) return;
  col0[g] = bpk[4 * (size_t)g];
  col1[g] = bpk[4 * (size_t)g + 3];
}

// q_mesh_walk over the threaded tree: the walk of batch_terrain_walk with any conservative test of a node's box (no stack: no error)
template <class P, class F>
__device__ __forceinline__ void q_mesh_walk(const BatchTerrain& M, uint32_t*, P&& pass, F&& emit) {
  for (uint32_t at = 0; at < M.n_nodes;) {
    const float4 n0 = M.nodes[2 * (size_t)at], n1 = M.nodes[2 * (size_t)at + 1];
    const bool hit = pass(xyz(n0), xyz(n1));
    const uint32_t w0 = f2u(n0.w);
    if (hit && (w0 & 0x80000000u)) emit(w0 & 0x7FFFFFFFu);
    at = hit ? at + 1u : f2u(n1.w);
  }
}

// q_compound_walk over the threaded tree of an entry of the obstacle table (no stack: no error)
template <class P, class F>
__device__ __forceinline__ void q_compound_walk(const BatchObstacle& D, uint32_t*, P&& pass, F&& emit) {
  for (uint32_t at = 0; at < D.n_nodes;) {
    const float4 n0 = D.nodes[2 * (size_t)at], n1 = D.nodes[2 * (size_t)at + 1];
    Box nb; nb.c = xyz(n0); nb.r = xyz(n1);
    const bool hit = pass(nb);
    const uint32_t w0 = f2u(n0.w);
    if (hit && (w0 & 0x80000000u)) emit(w0 & 0x7FFFFFFFu);
    at = hit ? at + 1u : max(f2u(n1.w), at + 1u);
  }
}

// lanes a query of a work item of `count` queries gets: 256 / (count rounded up to a power of two), as a shift
__device__ __forceinline__ uint32_t bq_lane_shift(uint32_t count) {
  uint32_t s = 8u;
  for (uint32_t p = 1u; p < count; p <<= 1) --s;
  return s;
}

// A workgroup's share of a call: the work item's world - its bodies at [g0, g0 + n) of col0 / col1 - and, once `split`, this lane's
// place in it: lane `sub` of the L that answer one query of the item (the caller's qi; `live`: there is one)
struct BatchWork {
  uint4 it;
  uint32_t g0, n;
  uint32_t L, sub, qi;
  bool live;
  __device__ __forceinline__ BatchWork(const BatchWorkArgs& A, bool bodies, uint4 item) : it(item), g0(A.w_off[it.x]) {
    n = bodies ? A.w_off[it.x + 1] - g0 : 0u;
  }
  __device__ __forceinline__ BatchWork(const BatchWorkArgs& A, bool bodies) : BatchWork(A, bodies, A.items[blockIdx.x]) {}
  // sh: the lanes a query gets, as a shift - shift(), or less
  __device__ __forceinline__ uint32_t shift() const { return bq_lane_shift(it.z); }
  // IDENTITY: sorted position = the caller's index (kItemFixed: there is no order array)
  template <bool IDENTITY = false>
  __device__ __forceinline__ void split(const BatchWorkArgs& A, uint32_t sh) {
    const uint32_t j = threadIdx.x >> sh;
    L = 1u << sh; sub = threadIdx.x & (L - 1u);
    live = j < it.z;
    qi = !live ? 0u : IDENTITY ? it.y + j : A.order[it.y + j];
  }
};

__device__ __forceinline__ void bq_stage(const BatchWorkArgs& A, uint32_t g0, uint32_t n, float4* s_c0, float4* s_c1) {
  for (uint32_t i = threadIdx.x; i < n; i += kBatchBlock) { s_c0[i] = A.col0[(size_t)g0 + i]; s_c1[i] = A.col1[(size_t)g0 + i]; }
  __syncthreads();
}

// The best of a query's L lanes into its first: within the wave through __shfl_xor, then - a query that has more than one wave - across
// them through s_red (Best::kRed words a wave).  Best: QueryBest or SweepBest (k_query.h), which bring shfl, pack / unpack and merge.
template <class Best>
__device__ __forceinline__ void bq_reduce(Best& best, const BatchWork& W, float4* s_red) {
  for (uint32_t off = min(W.L, 64u) >> 1; off > 0u; off >>= 1) best.merge(best.shfl((int)off));
  if (W.L > 64u) {
    const uint32_t wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) best.pack(s_red + Best::kRed * wv);
    __syncthreads();
    if (W.sub == 0u)
      for (uint32_t w = wv + 1u; w < wv + (W.L >> 6); ++w) best.merge(Best::unpack(s_red + Best::kRed * w));
  }
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

// A live query's particle in world coordinates and the body of its world it does not see (-1: none): what a loader hands bq_ray_front
struct BatchRay { V3 p, d; float dt; int32_t ign; };
// A live cast in world coordinates and the body of its world it does not meet (-1: none): what a loader hands bq_sweep_front.
// BatchCast: a cast the loader formed.  BatchCastAt: a cast where the caller keeps it - the front reads of it what it needs, when it
// needs it, as it would of the array itself.
struct BatchCast {
  MovingIn m;
  int32_t ign;
  __device__ __forceinline__ const MovingIn& cast() const { return m; }
};
struct BatchCastAt {
  const MovingIn* at;
  int32_t ign;
  __device__ __forceinline__ const MovingIn& cast() const { return *at; }
};

// q_sweep_cast without a grid: the reject's pad keeps its millimetre and the rounding of the path
__device__ __forceinline__ SweepCast bq_sweep_cast(const MovingIn& m) {
  QueryGrid G;
  G.margin = 0.0f;
  return q_sweep_cast(m, G);
}

// THE BODIES OF A WORK ITEM'S WORLD are a policy of the two fronts below and of bo_front (k_batch_observe.h), each written once:
//   stage(g0, n, s_dyn)               what a lane's walk reads of bodies [g0, g0 + n), into dynamic LDS: two rows of n float4 words, behind
//                                     them the kBatchQueryRed words of bq_reduce, behind those whatever else the policy keeps.  Ends with
//                                     the front's first barrier
//   ray_walk(W, p, d, dt, ign)        the best of lane W.sub's bodies - W.sub, W.sub + W.L, ... - against a particle (a Best: the policy's)
//   sweep_walk(W, K, ign)             the same against a cast (a SweepBest)
//   box(g)                            the tight box of body g of the batch (what bo_front stages)
// PlainBodies, here: a body is its collider row col0 / col1 and reports part 0; Best is QueryBest.  PartBodies (k_batch_part_query.h):
// a body of several components is walked part by part behind a body-level reject and its box is the union of its parts'; Best is
// PartBest, which carries `part` through the reduction.  A walk holds no barrier and leaves no kernel.  (A walk RETURNS its best: one
// that fills the front's through a reference cost every ray kernel two vector and four scalar registers.)
struct PlainBodies {
  using Best = QueryBest;
  const BatchWorkArgs& A;
  const float4 *c0 = nullptr, *c1 = nullptr;  // the staged rows
  __device__ __forceinline__ explicit PlainBodies(const BatchWorkArgs& a) : A(a) {}
  __device__ __forceinline__ void stage(uint32_t g0, uint32_t n, float4* s_dyn) {
    bq_stage(A, g0, n, s_dyn, s_dyn + n);
    c0 = s_dyn; c1 = s_dyn + n;
  }
  __device__ __forceinline__ QueryBest ray_walk(const BatchWork& W, V3 p, V3 d, float dt, int32_t ign) const {
    QueryBest best;
    const float dd = dot(d, d);
    for (uint32_t i = W.sub; i < W.n; i += W.L) {
      if ((int32_t)i == ign) continue;
      const float4 a = c0[i], b = c1[i];
      if (bq_ray_far(a, b, p, d, dd, dt)) continue;
      V3 ip; float t;
      if (q_ray_comp(p, d, dt, a, b, &ip, &t)) best.offer(ip, t, MGF_HIT_BODY, i, 0u);
    }
    return best;
  }
  __device__ __forceinline__ SweepBest sweep_walk(const BatchWork& W, const SweepCast& K, int32_t ign) const {
    SweepBest best;
    for (uint32_t i = W.sub; i < W.n; i += W.L) {
      if ((int32_t)i == ign) continue;
      const Comp t = to_comp(c0[i], c1[i]);
      if (q_sweep_far(t, K)) continue;
      Contact c;
      if (comp_mcomp(t, K.s, K.v, &c)) best.offer(c, MGF_HIT_BODY, i, 0u, 0u);
    }
    return best;
  }
  __device__ __forceinline__ Box box(size_t g) const { return comp_bounds(to_comp(A.col0[g], A.col1[g])); }
};

// A workgroup's work item of rays, written once for every kernel that casts rays with a workgroup per work item: k_batch_query_ray,
// k_batch_query_ray_dev<SRC> (bq_ray_item), k_batch_sensor_ray (k_batch_sensor.h) and their part-aware forms (k_batch_part_query.h).
// What a kernel brings is the bodies' policy, where a particle comes from - load(qi, g0) -> BatchRay, run by the live lanes behind the
// staging - and what else its first lane does behind the stored hit - done(qi, p, d, dt).  Neither hook holds a barrier nor leaves the
// kernel; the policy's only barrier is the one its staging ends with.
// kItemPlan: a workgroup at or beyond the device's item total has no work item - it leaves, the whole of it, before anything is staged
// and ahead of the first __syncthreads.  The only other exit is behind bq_reduce.
template <int SRC, class Bodies, class Load, class Done>
__device__ __forceinline__ void bq_ray_front(const BatchQueryArgs& A, Bodies bodies, const BatchItemSrc& S, float4* s_dyn, Load&& load, Done&& done) {
  if (SRC == kItemPlan && blockIdx.x >= *S.n_items) return;
  BatchWork W(A, A.mask & MGF_QUERY_BODIES, bq_item<SRC>(A, S));
  const uint32_t n = W.n;
  bodies.stage(W.g0, n, s_dyn);
  W.template split<SRC == kItemFixed>(A, W.shift());
  const uint32_t qi = W.qi;
  V3 p = mk3(0.0f, 0.0f, 0.0f), d = p;
  float dt = 0.0f;
  int32_t ign = -1, mask = 0;
  if (W.live) {
    const BatchRay r = load(qi, W.g0);
    p = r.p; d = r.d; dt = r.dt; ign = r.ign;
    mask = A.mask;
    if (!q_ray_castable(d)) mask = 0;  // (no direction, or one outside the band: no hit, by definition - k_query.h)
  }
  typename Bodies::Best best;
  if (mask & MGF_QUERY_BODIES) best = bodies.ray_walk(W, p, d, dt, ign);
  bq_reduce(best, W, s_dyn + 2 * (size_t)n);
  if (W.sub != 0u || !W.live) return;
  if (mask & MGF_QUERY_TERRAIN) {
    const BatchTerrain M = batch_terrain_of(A.T, W.it.x);  // (the work item's world: wave-uniform loads)
    if (M.n_nodes) q_ray_terrain(M, p, d, dt, nullptr, best);
  }
  q_ray_store(A.out + 7 * (size_t)qi, best);
  done(qi, p, d, dt);
}
// the front over the caller's particles: parts[qi] as it stands, A.ignore, nothing behind the hit
template <int SRC, class Bodies>
__device__ __forceinline__ void bq_ray_item(const BatchQueryArgs& A, Bodies bodies, const ParticleIn* parts, const BatchItemSrc& S, float4* s_dyn) {
  bq_ray_front<SRC>(
      A, bodies, S, s_dyn,
      [&](uint32_t qi, uint32_t) {
        const ParticleIn q = parts[qi];
        return BatchRay{ld3(q.p), ld3(q.d), q.dt, A.ignore ? A.ignore[qi] : -1};
      },
      [](uint32_t, V3, V3, float) {});
}
// LDS (dynamic): 32 bytes a body, kBatchQueryRed words.
__global__ __launch_bounds__(kBatchBlock) void k_batch_query_ray(BatchQueryArgs A, const ParticleIn* parts) {
  extern __shared__ float4 s_dyn[];
  bq_ray_item<kItemTable>(A, PlainBodies(A), parts, BatchItemSrc(), s_dyn);
}

// A workgroup's work item of casts, written once as the rays' is (bq_ray_front's remarks): load(qi, g0) -> BatchCast or BatchCastAt,
// done(qi, m) behind the stored hit.  No loader reads the staged rows: a mask without bodies stages nothing.  kItemFixed: no plan has looked at the
// casts - one whose tag is no component's is matched against nothing, keeps the no-hit record and is counted by the first of its lanes.
template <int SRC, class Bodies, class Load, class Done>
__device__ __forceinline__ void bq_sweep_front(const BatchQueryArgs& A, Bodies bodies, const BatchItemSrc& S, float4* s_dyn, Load&& load, Done&& done) {
  if (SRC == kItemPlan && blockIdx.x >= *S.n_items) return;
  BatchWork W(A, A.mask & MGF_QUERY_BODIES, bq_item<SRC>(A, S));
  const uint32_t n = W.n;
  bodies.stage(W.g0, n, s_dyn);
  W.template split<SRC == kItemFixed>(A, W.shift());
  const uint32_t qi = W.qi;
  SweepBest best;
  decltype(load(qi, W.g0)) c;
  bool ok = W.live;
  if (ok) c = load(qi, W.g0);
  if (SRC == kItemFixed && ok && (uint32_t)c.cast().tag > (uint32_t)KIND_CAPSULE) {
    ok = false;
    if (W.sub == 0u) atomicAdd(S.skipped, 1ull);
  }
  if (ok && n) best = bodies.sweep_walk(W, bq_sweep_cast(c.cast()), c.ign);  // (n: the mask asks for bodies, and the world has some)
  bq_reduce(best, W, s_dyn + 2 * (size_t)n);
  if (W.sub != 0u || !W.live) return;
  q_sweep_store(A.out + 13 * (size_t)qi, best);
  done(qi, c.cast());
}
// the front over the caller's casts: casts[qi] as it stands, A.ignore, nothing behind the hit
template <int SRC, class Bodies>
__device__ __forceinline__ void bq_sweep_item(const BatchQueryArgs& A, Bodies bodies, const MovingIn* casts, const BatchItemSrc& S, float4* s_dyn) {
  bq_sweep_front<SRC>(
      A, bodies, S, s_dyn, [&](uint32_t qi, uint32_t) { return BatchCastAt{casts + qi, A.ignore ? A.ignore[qi] : -1}; }, [](uint32_t, const MovingIn&) {});
}
// LDS (dynamic): 32 bytes a body, kBatchQueryRed words.
__global__ __launch_bounds__(kBatchBlock) void k_batch_query_sweep_bodies(BatchQueryArgs A, const MovingIn* casts) {
  extern __shared__ float4 s_dyn[];
  bq_sweep_item<kItemTable>(A, PlainBodies(A), casts, BatchItemSrc(), s_dyn);
}

// the world of query i for a lane-per-query pass; negative: the record is skipped
__device__ __forceinline__ int32_t bq_lane_world(const int32_t* world, uint32_t per, uint32_t i) { return world ? world[i] : (int32_t)(i / per); }

// q_sweep_terrain's tests over the threaded tree, a lane per cast in the caller's order, each over the terrain of its own cast's world
// (bq_lane_world; the walk is per lane as it is)
__global__ __launch_bounds__(kBatchBlock) void k_batch_query_sweep_faces(BatchTerrains T, const int32_t* world, uint32_t per, const MovingIn* casts, uint32_t n,
                                                                          int32_t* out) {
  const uint32_t i = blockIdx.x * kBatchBlock + threadIdx.x;
  if (i >= n) return;
  const int32_t w = bq_lane_world(world, per, i);
  if (w < 0) return;
  const BatchTerrain M = batch_terrain_of(T, (uint32_t)w);
  if (M.n_nodes == 0u) return;
  if ((uint32_t)casts[i].tag > (uint32_t)KIND_CAPSULE) return;
  const SweepCast K = bq_sweep_cast(casts[i]);
  int32_t* o = out + 13 * (size_t)i;
  SweepBest best = q_sweep_load(o);  // k_batch_query_sweep_bodies' answer
  q_sweep_terrain(M, K, nullptr, best);
  q_sweep_store(o, best);
}

// a stored ray record taken up again by a later launch (q_sweep_load's counterpart)
__device__ __forceinline__ QueryBest q_ray_load(const int32_t* o) {
  QueryBest best;
  if (o[0] != MGF_HIT_NONE) { best.have = true; best.kind = o[0]; best.index = (uint32_t)o[1]; best.part = (uint32_t)o[2]; best.p = mk3(u2f(o[3]), u2f(o[4]), u2f(o[5])); best.t = u2f(o[6]); }
  return best;
}

// The obstacles of every query's own world (bq_lane_world), a lane per query in the caller's order: `index` of a hit is the obstacle's place
// in the world's list, `part` the component.
__global__ __launch_bounds__(kBatchBlock) void k_batch_query_ray_obstacles(BatchObstacles O, const uint4* tdesc, const int32_t* world, uint32_t per,
                                                                            const ParticleIn* parts, uint32_t n, int32_t* out) {
  const uint32_t i = blockIdx.x * kBatchBlock + threadIdx.x;
  if (i >= n) return;
  const int32_t w = bq_lane_world(world, per, i);
  if (w < 0) return;
  const uint32_t obst = tdesc[2 * (size_t)w + 1].w, ob0 = batch_obst_first(obst), ob1 = ob0 + batch_obst_count(obst);
  if (ob0 == ob1) return;
  const ParticleIn q = parts[i];
  if (!q_ray_castable(ld3(q.d))) return;  // (no direction, or one outside the band: no hit, by definition - k_query.h)
  int32_t* o = out + 7 * (size_t)i;
  QueryBest best = q_ray_load(o);  // k_batch_query_ray's answer
#pragma unroll 1
  for (uint32_t e = ob0; e < ob1; ++e) q_ray_obstacle(batch_obstacle_of(O, e), e - ob0, q, nullptr, best);
  q_ray_store(o, best);
}
__global__ __launch_bounds__(kBatchBlock) void k_batch_query_sweep_obstacles(BatchObstacles O, const uint4* tdesc, const int32_t* world, uint32_t per,
                                                                              const MovingIn* casts, uint32_t n, int32_t* out) {
  const uint32_t i = blockIdx.x * kBatchBlock + threadIdx.x;
  if (i >= n) return;
  const int32_t w = bq_lane_world(world, per, i);
  if (w < 0) return;
  const uint32_t obst = tdesc[2 * (size_t)w + 1].w, ob0 = batch_obst_first(obst), ob1 = ob0 + batch_obst_count(obst);
  if (ob0 == ob1) return;
  if ((uint32_t)casts[i].tag > (uint32_t)KIND_CAPSULE) return;
  const SweepCast K = bq_sweep_cast(casts[i]);
  int32_t* o = out + 13 * (size_t)i;
  SweepBest best = q_sweep_load(o);  // k_batch_query_sweep_bodies' (and _faces') answer
#pragma unroll 1
  for (uint32_t e = ob0; e < ob1; ++e)
    compound_contacts_walk(batch_obstacle_of(O, e), K.s, K.v, [&](uint32_t ci, const Contact& c) { best.offer(c, MGF_HIT_OBSTACLE, e - ob0, ci, 0u); });
  q_sweep_store(o, best);
}

}  // namespace mgf
