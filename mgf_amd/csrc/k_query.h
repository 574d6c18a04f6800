// Queries against a world's resident bodies, terrain and obstacles between ticks (mgf_world_raycast_many, mgf_world_sweep_many,
// mgf_world_overlap_aabb_many; host_query.inc).  (Part of the kernel set described in kernels.h.)
//
// The bodies are reached through a uniform grid built per call from their CURRENT tight boxes (the tick's own cell grid is
// laid over the fat boxes of the last collide phase and is stale after its integrate; it is not read):
//   k_query_boxes      BoundedBy<AABB> of every owned body (bounds.rs:170-190, the union of the parts' bounds for a body of
//                      several components); bodies wider than a cell go to the query's own large-body list, the others reduce
//                      the grid's bounds
//   k_query_cells<F>   the counting sort: every body in each cell its (margin-padded) box touches, at most 2x2x2; count, scan, fill
//   k_query_ray        a lane per particle: the large bodies, the obstacles (Intersects<Compound>, compound.rs:309-332), the
//                      terrain's BVH, then the grid's cells in DDA order until the next cell starts beyond the best t so far
//   k_query_sweep      a lane per swept sphere or capsule: the large bodies, the obstacles (Compound::contacts' own walk), the terrain's
//                      BVH with the padded swept box; then k_query_sweep_cells walks the grid: a DDA along the path of the cast's
//                      centre, visiting the block of cells its half extent can reach, until the next cell starts beyond the best t
//   k_query_overlap<F> a lane per box: the cells it touches (a body is tested in the first cell it shares with the box), the
//                      large bodies; count, scan, fill, then k_query_sort puts each list into the caller's order
// Which of the targets a hit belongs to never depends on the visiting order: hits are ranked by (t, kind, index, part).
// Every acceleration step is conservative (cells and boxes padded by QueryGrid::margin); each answer comes from the
// reference's single-shape test.
// What a query tests and records is written here once, for these kernels and the batch's (k_batch_query.h, k_batch_observe.h):
//   to_comp(float4, float4)                          a collider's two rows as a Comp
//   q_ray_terrain / q_sweep_terrain<Mesh>            the terrain's node-box and face tests, over either walk of a mesh tree (q_mesh_walk)
//   QueryBest / SweepBest                            the candidate and its ranking; shfl / pack / unpack / merge for the batch's bq_reduce
//   q_ray_store / q_sweep_store / q_sweep_load       the 7- and 13-word records, and a record taken up again by a later launch
//   q_clip / q_next_crossing                         the grid walks: a path clipped to a box, the DDA's next cell face
#pragma once
#include "k_api.h"

namespace mgf {

struct QueryGrid {
  float lo[3];
  float h, inv_h;
  int dims[3];
  float margin;            // world-space pad of every box the grid files or looks up (covers the rounding of the walk)
  float rmin;              // the smallest radius of a component of a body in the grid (q_ray_tube)
  const uint32_t* start;   // cells + 1 offsets into items (exclusive scan of the counts)
  const uint32_t* items;   // slots
  const uint32_t* large;   // slots of the bodies wider than a cell, tested by every query
  const uint32_t* n_large;
};

__device__ __forceinline__ int q_cell(float v, int k, const QueryGrid& G) {
  const float f = floorf((v - G.lo[k]) * G.inv_h);
  const float hi = (float)(G.dims[k] - 1);
  return (int)fminf(fmaxf(f, 0.0f), hi);
}
// cells a body box (or a query box) touches, padded by the margin
__device__ __forceinline__ void q_cell_range(const Box& b, const QueryGrid& G, int lo[3], int hi[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    lo[k] = q_cell(at(b.c, k) - at(b.r, k) - G.margin, k, G);
    hi[k] = q_cell(at(b.c, k) + at(b.r, k) + G.margin, k, G);
  }
}

// a collider or a world-space part as its two rows: (p.xyz, r), (d.xyz, kind)
__device__ __forceinline__ Comp to_comp(float4 a, float4 b) { Comp c; c.kind = (int)f2u(b.w); c.p = xyz(a); c.d = xyz(b); c.r = a.w; return c; }

// BoundedBy<AABB> of slot i: its collider, or the union of its parts in order (what k_integrate's tight box is, unswept)
__device__ __forceinline__ Box q_body_box(const Bodies& B, uint32_t i) {
  const uint32_t pc = B.pcount ? B.pcount[i] : 0u;
  Box tb;
  if (pc) {
    for (uint32_t k = 0; k < pc; ++k) {
      float4 a, b;
      world_part(B, i, k, pc, a, b);
      const Box pb = comp_bounds(to_comp(a, b));
      tb = k == 0 ? pb : box_combine(tb, pb);
    }
  } else {
    tb = comp_bounds(to_comp(B.col0[i], B.col1[i]));
  }
  return tb;
}

// the smallest radius among slot i's components
__device__ __forceinline__ float q_body_rmin(const Bodies& B, uint32_t i) {
  const uint32_t pc = B.pcount ? B.pcount[i] : 0u;
  if (!pc) return B.col0[i].w;
  float r = kInf;
  for (uint32_t k = 0; k < pc; ++k) {
    float4 a, b;
    world_part(B, i, k, pc, a, b);
    r = fminf(r, a.w);
  }
  return r;
}

// bounds[0..2] = ordered-int min of the padded low corners, [3..5] max of the high corners, [8] the min of q_body_rmin (bodies that go to
// the grid): reduced across the wave first, one atomic per wave and word
__global__ __launch_bounds__(kBlock) void k_query_boxes(Bodies B, uint32_t n, float h, float margin, float4* qb_c, float4* qb_r, int* bounds,
                                                        uint32_t* large, uint32_t* n_large) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  int lo[3] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF}, hi[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
  int rm = 0x7FFFFFFF;
  if (i < n) {
    const Box b = q_body_box(B, i);
    const bool wide = !(2.0f * (b.r.x + margin) <= h && 2.0f * (b.r.y + margin) <= h && 2.0f * (b.r.z + margin) <= h);  // (NaN: wide)
    qb_c[i] = mk4(b.c, 0.0f);
    qb_r[i] = mk4(b.r, wide ? 1.0f : 0.0f);
    if (wide) {
      large[atomicAdd(n_large, 1u)] = i;
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) { lo[k] = f_ord(at(b.c, k) - at(b.r, k) - margin); hi[k] = f_ord(at(b.c, k) + at(b.r, k) + margin); }
      rm = f_ord(fmaxf(q_body_rmin(B, i), 0.0f));  // (NaN: 0)
    }
  }
  for (int off = 32; off > 0; off >>= 1) rm = min(rm, __shfl_xor(rm, off));
  if ((threadIdx.x & 63) == 0) atomicMin(bounds + 8, rm);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    int a = lo[k], c = hi[k];
    for (int off = 32; off > 0; off >>= 1) { a = min(a, __shfl_xor(a, off)); c = max(c, __shfl_xor(c, off)); }
    if ((threadIdx.x & 63) == 0) { atomicMin(bounds + k, a); atomicMax(bounds + 3 + k, c); }
  }
}

// counting sort of the grid bodies into the cells they touch; FILL: cnt was cleared again after the scan and is the cursor
template <bool FILL>
__global__ __launch_bounds__(kBlock) void k_query_cells(QueryGrid G, uint32_t n, const float4* qb_c, const float4* qb_r, uint32_t* cnt, uint32_t* items) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const float4 r4 = qb_r[i];
  if (r4.w != 0.0f) return;  // a large body
  Box b; b.c = xyz(qb_c[i]); b.r = xyz(r4);
  int lo[3], hi[3];
  q_cell_range(b, G, lo, hi);
  for (int z = lo[2]; z <= hi[2]; ++z)
    for (int y = lo[1]; y <= hi[1]; ++y)
      for (int x = lo[0]; x <= hi[0]; ++x) {
        const uint32_t c = (uint32_t)x + (uint32_t)G.dims[0] * ((uint32_t)y + (uint32_t)G.dims[1] * (uint32_t)z);
        const uint32_t k = atomicAdd(cnt + c, 1u);
        if (FILL) items[G.start[c] + k] = i;
      }
}

// Intersects<Sphere | Capsule> of a body's collider or part
__device__ __forceinline__ bool q_ray_comp(V3 p, V3 d, float dt, float4 a, float4 b, V3* ip, float* t) {
  if ((int)f2u(b.w) == KIND_SPHERE) return ray_sphere(p, d, mks(xyz(a), a.w), ip, t, dt);
  return ray_capsule(p, d, mkcap(xyz(a), xyz(b), a.w), ip, t, dt);
}

__device__ __forceinline__ V3 q_shfl3(V3 v, int off) { return mk3(__shfl_xor(v.x, off), __shfl_xor(v.y, off), __shfl_xor(v.z, off)); }

struct QueryBest {
  bool have = false;
  int kind = -1;
  uint32_t index = 0, part = 0;
  V3 p = mk3(0.0f, 0.0f, 0.0f);
  float t = 0.0f;
  // (t, kind, index, part) ascending: the rule of the definition, whatever order the targets are visited in
  __device__ __forceinline__ void offer(V3 ip, float it, int k, uint32_t idx, uint32_t pt) {
    if (!(fabsf(it) < kInf)) return;  // a hit whose t is not finite is not a candidate (a NaN taken first could never be replaced)
    const bool better = !have || it < t || (it == t && (k < kind || (k == kind && (idx < index || (idx == index && pt < part)))));
    if (better) { have = true; kind = k; index = idx; part = pt; p = ip; t = it; }
  }
  // for bq_reduce (k_batch_query.h; a batch's bodies have one part: `part` does not travel)
  static constexpr uint32_t kRed = 2;  // float4 words of a packed candidate
  __device__ __forceinline__ QueryBest shfl(int off) const {
    QueryBest o;
    o.kind = __shfl_xor(have ? kind : -1, off); o.index = (uint32_t)__shfl_xor((int)index, off); o.p = q_shfl3(p, off); o.t = __shfl_xor(t, off);
    o.have = o.kind >= 0;
    return o;
  }
  __device__ __forceinline__ void pack(float4* w) const {
    w[0] = make_float4(u2f((uint32_t)(have ? kind : -1)), u2f(index), t, 0.0f);
    w[1] = mk4(p, 0.0f);
  }
  static __device__ __forceinline__ QueryBest unpack(const float4* w) {
    const float4 r0 = w[0], r1 = w[1];
    QueryBest o;
    o.kind = (int)f2u(r0.x); o.index = f2u(r0.y); o.p = xyz(r1); o.t = r0.z;
    o.have = o.kind >= 0;
    return o;
  }
  __device__ __forceinline__ void merge(const QueryBest& o) { if (o.have) offer(o.p, o.t, o.kind, o.index, 0u); }
};
// mgf_ray_hit as seven words
__device__ __forceinline__ void q_ray_store(int32_t* o, const QueryBest& best) {
  if (best.have) {
    o[0] = best.kind; o[1] = (int32_t)best.index; o[2] = (int32_t)best.part;
    o[3] = (int32_t)f2u(best.p.x); o[4] = (int32_t)f2u(best.p.y); o[5] = (int32_t)f2u(best.p.z); o[6] = (int32_t)f2u(best.t);
  } else {
    o[0] = MGF_HIT_NONE; o[1] = 0; o[2] = 0; o[3] = 0; o[4] = 0; o[5] = 0; o[6] = 0;
  }
}

// clip the path p + d t, t in [t0, t1], to the box [lo, hi] (an axis with skip[k] set is not looked at; skip null: none): false - the
// path misses the box
__device__ __forceinline__ bool q_clip(V3 p, V3 d, const float lo[3], const float hi[3], const bool* skip, float& t0, float& t1) {
  bool miss = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float pk = at(p, k), dk = at(d, k);
    if (skip && skip[k]) continue;
    if (dk == 0.0f) {
      if (!(pk >= lo[k] && pk <= hi[k])) miss = true;
    } else {
      float ta = (lo[k] - pk) / dk, tb = (hi[k] - pk) / dk;
      if (ta > tb) { const float s = ta; ta = tb; tb = s; }
      t0 = fmaxf(t0, ta); t1 = fminf(t1, tb);
    }
  }
  return !miss && t0 <= t1;
}
// conservative slab test of a particle against a padded box: may the particle meet the box at a parameter in [0, tmax]?
__device__ __forceinline__ bool q_slab(V3 p, V3 d, V3 c, V3 r, float pad, float tmax) {
  float t0 = 0.0f, t1 = tmax;
#pragma unroll
  for (int k = 0; k < 3; ++k) {  // (q_clip with an early way out: this runs per node of a mesh walk)
    const float pk = at(p, k), dk = at(d, k), lo = at(c, k) - at(r, k) - pad, hi = at(c, k) + at(r, k) + pad;
    if (dk == 0.0f) {
      if (!(pk >= lo && pk <= hi)) return false;
    } else {
      float ta = (lo - pk) / dk, tb = (hi - pk) / dk;
      if (ta > tb) { const float s = ta; ta = tb; tb = s; }
      t0 = fmaxf(t0, ta); t1 = fminf(t1, tb);
    }
  }
  return t0 <= t1;
}
__device__ __forceinline__ float q_maxabs(V3 v) { return fmaxf(fabsf(v.x), fmaxf(fabsf(v.y), fabsf(v.z))); }
// Is a particle of direction d cast at all?  The rule of include/mgf_hip.h, written once for every front that casts rays (k_query_ray,
// bq_ray_front and with it the sensors and the part queries, the cameras, the obstacle passes of the batch and of a rollout's trace): the
// largest |component| of d within [MGF_RAY_DMIN, MGF_RAY_DMAX].  Outside the band - d = 0 and a d with a NaN included - the particle hits
// nothing: the single tests divide by |d|^2 and square |m||d|, and where those underflow or overflow a target nowhere near the line answers.
__device__ __forceinline__ bool q_ray_castable(V3 d) {
  return q_maxabs(d) >= MGF_RAY_DMIN && fabsf(d.x) <= MGF_RAY_DMAX && fabsf(d.y) <= MGF_RAY_DMAX && fabsf(d.z) <= MGF_RAY_DMAX;
}

// The DDA's next step from cell c along p + d t (Amanatides-Woo): the axis whose cell face the path crosses first and the parameter tn
// there, computed afresh from the face - nothing accumulates.  -1: no axis steps.
__device__ __forceinline__ int q_next_crossing(const QueryGrid& G, const int c[3], const int step[3], V3 p, V3 d, float& tn) {
  tn = kInf;
  int ax = -1;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (step[k] == 0) continue;
    const float face = G.lo[k] + (float)(c[k] + (step[k] > 0 ? 1 : 0)) * G.h;
    const float tk = (face - at(p, k)) / at(d, k);
    if (ax < 0 || tk < tn) { tn = tk; ax = k; }
  }
  return ax;
}

struct QueryTargets {
  Bodies B;
  const uint32_t* ext;   // slot -> caller index (null: identity)
  const float4* qb_c;
  const float4* qb_r;
  TerrainDev M;          // n_nodes 0: no terrain
  const CompoundDev* obs;
  uint32_t n_obs;
  uint32_t n;            // owned bodies (slots 0 .. n - 1; qb_r[s].w != 0: s is on the large list)
  uint32_t* err;         // [0]: a traversal stack overflowed
};

__device__ __forceinline__ void q_ray_body(const QueryTargets& T, uint32_t s, V3 p, V3 d, float dt, int32_t ign, QueryBest& best) {
  const uint32_t e = T.ext ? T.ext[s] : s;
  if ((int32_t)e == ign) return;
  const Bodies& B = T.B;
  const uint32_t pc = B.pcount ? B.pcount[s] : 0u;
  V3 ip; float t;
  if (pc) {
    for (uint32_t k = 0; k < pc; ++k) {
      float4 a, b;
      world_part(B, s, k, pc, a, b);
      if (q_ray_comp(p, d, dt, a, b, &ip, &t)) best.offer(ip, t, MGF_HIT_BODY, e, k);
    }
  } else if (q_ray_comp(p, d, dt, B.col0[s], B.col1[s], &ip, &t)) {
    best.offer(ip, t, MGF_HIT_BODY, e, 0u);
  }
}

// The walk of a compound's tree with any test of a node's box, in the order bvh.rs:283-310 visits it: emit(ci) for every leaf whose
// boxes all pass, straight behind the leaf's own pass.  Here the explicit stack over a CompoundDev's TerrainDev; in k_batch_query.h
// the threaded tree of an entry of a batch's obstacle table.
template <class P, class F>
__device__ __forceinline__ void q_compound_walk(const CompoundDev& D, uint32_t* err, P&& pass, F&& emit) {
  uint32_t stack[kStack];
  int sp = 0;
  if (D.tree.n_nodes) stack[sp++] = D.tree.root;
  while (sp > 0) {
    uint32_t top = stack[--sp];
    const float4* raw = reinterpret_cast<const float4*>(&D.tree.nodes[top]);
    float4 n0 = raw[0], n1 = raw[1];
    Box nb; nb.c = xyz(n0); nb.r = xyz(n1);
    if (pass(nb)) {
      uint32_t w0 = f2u(n0.w), w1 = f2u(n1.w);
      if (w0 & 0x80000000u) emit(w0 & 0x7FFFFFFFu);
      else if (sp + 2 <= kStack) { stack[sp++] = w0; stack[sp++] = w1; }
      else *err = 1u;
    }
  }
}
// Intersects<Compound> compound.rs:309-332 (k_compound_intersections' walk), with the component that answered.  C: either form of a
// compound (compound_contacts_walk, k_api.h).  A later hit with an equal t replaces the earlier: the walk's order is the reference's.
template <class C>
__device__ __forceinline__ void q_ray_obstacle(const C& D, uint32_t o, const ParticleIn& q, uint32_t* err, QueryBest& best) {
  V3 pp = ld3(q.p), pd = ld3(q.d), disp = ld3(D.disp);
  const float dt = q.dt;
  Quat rot = mkq(D.rot[0], mk3(D.rot[1], D.rot[2], D.rot[3]));
  Quat conj = mkq(rot.s, -rot.v);
  V3 rp = rotate(conj, pp + -disp) + disp, rd = rotate(conj, pd);
  bool have = false;
  V3 best_p = mk3(0, 0, 0); float best_t = 0.0f;
  uint32_t best_c = 0;
  float t = 0.0f;  // where the particle enters the box of the node last passed
  q_compound_walk(
      D, err,
      [&](const Box& nb) {
        V3 ip;
        return ray_box(rp, rd, nb, &ip, &t, kInf);
      },
      [&](uint32_t ci) {
        if (t > dt) return;
        Comp shape = comp_rotate(to_comp(D.comps[ci]), rot);
        shape.p = shape.p + disp;
        V3 sip; float st;
        if (intersection_dispatch(q, comp_shape(shape), &sip, &st) == 1 && !(have && st > best_t)) { best_p = sip; best_t = st; best_c = ci; have = true; }
      });
  if (have) best.offer(best_p, best_t, MGF_HIT_OBSTACLE, o, best_c);
}

// The terrain's tests are written once, over either walk of a mesh tree: q_mesh_walk(M, err, pass, emit) calls emit(f) for every face f
// whose node boxes (centre, half extent) all pass - here the explicit stack over TerrainDev, in k_batch_query.h the threaded tree over
// BatchTerrain.  Mesh: either struct (x, verts, faces).
template <class P, class F>
__device__ __forceinline__ void q_mesh_walk(const TerrainDev& M, uint32_t* err, P&& pass, F&& emit) {
  uint32_t stack[kStack];
  int sp = 0;
  stack[sp++] = M.root;
  while (sp > 0) {
    const uint32_t top = stack[--sp];
    const float4* raw = reinterpret_cast<const float4*>(&M.nodes[top]);
    const float4 n0 = raw[0], n1 = raw[1];
    if (!pass(xyz(n0), xyz(n1))) continue;
    const uint32_t w0 = f2u(n0.w), w1 = f2u(n1.w);
    if (w0 & 0x80000000u) emit(w0 & 0x7FFFFFFFu);
    else if (sp + 2 <= kStack) { stack[sp++] = w0; stack[sp++] = w1; }
    else *err = 1u;
  }
}
template <class Mesh>
__device__ __forceinline__ Triangle q_face(const Mesh& M, V3 mx, uint32_t f) {
  const uint4 fi = M.faces[f];
  return mkt(xyz(M.verts[fi.x]) + mx, xyz(M.verts[fi.y]) + mx, xyz(M.verts[fi.z]) + mx);
}

// Intersects<Triangle> of every face the padded walk of the mesh BVH reaches: the slab test of a node is bounded by the best t so far
template <class Mesh>
__device__ __forceinline__ void q_ray_terrain(const Mesh& M, V3 p, V3 d, float dt, uint32_t* err, QueryBest& best) {
  const V3 mx = mk3(M.x[0], M.x[1], M.x[2]);
  const V3 lp = p + -mx;  // the tree's boxes are in the mesh's frame
  q_mesh_walk(
      M, err,
      [&](V3 c, V3 r) {
        const float pad = 1e-5f * (q_maxabs(c) + q_maxabs(r) + q_maxabs(mx) + q_maxabs(p)) + 1e-6f;
        const float lim = best.have ? fminf(dt, best.t * 1.0001f + 1e-6f) : dt;
        return q_slab(lp, d, c, r, pad, lim);
      },
      [&](uint32_t f) {
        V3 ip; float t;
        if (ray_triangle(p, d, q_face(M, mx, f), &ip, &t, dt)) best.offer(ip, t, MGF_HIT_TERRAIN, f, 0u);
      });
}

// How far from a sphere's or a capsule's surface the line of a particle may pass and the single test still answer, for a component of
// radius >= rmin whose points are at most m from the particle's origin.  ray_sphere (and ray_capsule's end caps) decide by the sign of
// b^2 - a c, b = m . d, a = |d|^2, c = |m|^2 - r^2, which is a (r^2 - e^2) for a line passing the centre at e.  In f32 each of b^2 and
// a c carries at most 8 roundings of 2^-24 relative to a |m|^2, so the sign is wrong only where |e^2 - r^2| <= 1e-6 |m|^2: e stays below
// sqrt(r^2 + 1e-6 m^2), largest beyond the surface for the smallest r.  (Measured over the query corpus: 2.6e-7 |m|^2 at the most.)
__device__ __forceinline__ float q_ray_tube(float rmin, float m) {
  const float k = 1e-6f * m * m;
  return k / (__builtin_sqrtf(rmin * rmin + k) + rmin + 1e-30f);
}

// the grid cell (x, y, z) and its neighbourhood of r cells every way, for one particle
__device__ __forceinline__ void q_ray_cells(const QueryGrid& G, const QueryTargets& T, const int c[3], int r, V3 p, V3 d, float dt, int32_t ign,
                                            QueryBest& best) {
  for (int z = max(c[2] - r, 0); z <= min(c[2] + r, G.dims[2] - 1); ++z)
    for (int y = max(c[1] - r, 0); y <= min(c[1] + r, G.dims[1] - 1); ++y)
      for (int x = max(c[0] - r, 0); x <= min(c[0] + r, G.dims[0] - 1); ++x) {
        const uint32_t cell = (uint32_t)x + (uint32_t)G.dims[0] * ((uint32_t)y + (uint32_t)G.dims[1] * (uint32_t)z);
        for (uint32_t k = G.start[cell], ke = G.start[cell + 1]; k < ke; ++k) q_ray_body(T, G.items[k], p, d, dt, ign, best);
      }
}

__global__ __launch_bounds__(kBlock) void k_query_ray(QueryGrid G, QueryTargets T, const ParticleIn* parts, int64_t n, const int32_t* ignore, int32_t mask,
                                                      int32_t* out /* 7 words per particle: mgf_ray_hit */) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const ParticleIn q = parts[i];
  const V3 p = ld3(q.p), d = ld3(q.d);
  const float dt = q.dt;
  const int32_t ign = ignore ? ignore[i] : -1;
  QueryBest best;
  if (!q_ray_castable(d)) mask = 0;  // (no direction, or one outside the band: no hit, by definition)
  if (mask & MGF_QUERY_BODIES) {
    const uint32_t nl = *G.n_large;
    for (uint32_t k = 0; k < nl; ++k) q_ray_body(T, G.large[k], p, d, dt, ign, best);
  }
  if (mask & MGF_QUERY_OBSTACLES)
    for (uint32_t o = 0; o < T.n_obs; ++o) q_ray_obstacle(T.obs[o], o, q, T.err, best);
  if ((mask & MGF_QUERY_TERRAIN) && T.M.n_nodes) q_ray_terrain(T.M, p, d, dt, T.err, best);
  if ((mask & MGF_QUERY_BODIES) && G.dims[0] > 0) {
    // The single tests are not local for an origin far away (q_ray_tube): a body the line passes by up to the tube answers.  So the walk
    // is laid over the grid's box GROWN by the tube - the tube at the distance of the box's farthest corner, which bounds every body's -
    // and the margin, and at each cell, inside the grid or beside it, looks as many cells around as the tube at the distance the
    // particle has covered when it leaves the cell (the reach of the cells looked at added: two cells around are 3 sqrt(3) h).  Where
    // the tube is more than two cells, or nothing bounds the distance, a particle whose path meets the grown box is put to every body
    // of the grid.  A particle whose tube stays inside a quarter of the margin walks the grid's own cells, one at a time.  (This takes in
    // what a rule on the particle's own rounding, 4e-7 of |p| and of the stretch against a quarter of the margin, used to add: wherever
    // that fired the tube is at least a cell.)
    float ghi[3];
    V3 fc;
#pragma unroll
    for (int k = 0; k < 3; ++k) ghi[k] = G.lo[k] + (float)G.dims[k] * G.h;
    fc.x = fmaxf(fabsf(p.x - G.lo[0]), fabsf(p.x - ghi[0])); fc.y = fmaxf(fabsf(p.y - G.lo[1]), fabsf(p.y - ghi[1])); fc.z = fmaxf(fabsf(p.z - G.lo[2]), fabsf(p.z - ghi[2]));
    const float dlen = mag(d);
    const float far_tube = q_ray_tube(G.rmin, mag(fc));
    const bool wide = !(far_tube <= 0.25f * G.margin);  // (NaN: wide)
    const bool all = wide && !(far_tube <= 2.0f * G.h);  // more than two cells (NaN, inf: all)
    const float pad = !wide ? 0.0f : (far_tube < kInf ? far_tube + G.margin : kInf);
    const int out_cells = wide ? 3 : 0;  // cells beside the grid the walk may stand in: a walked pad is below three
    const auto every_body = [&]() {
      for (uint32_t b = 0; b < T.n; ++b)
        if (T.qb_r[b].w == 0.0f) q_ray_body(T, b, p, d, dt, ign, best);
    };
    float t0 = 0.0f, t1 = dt;
    float plo[3], phi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { plo[k] = G.lo[k] - pad; phi[k] = ghi[k] + pad; }
    const bool meets = !(pad < kInf) || q_clip(p, d, plo, phi, nullptr, t0, t1);
    if (meets && all) {
      every_body();
    } else if (meets) {
      const V3 e = p + d * t0;
      int c[3], step[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float f = floorf((at(e, k) - G.lo[k]) * G.inv_h);
        c[k] = (int)fminf(fmaxf(f, (float)-out_cells), (float)(G.dims[k] - 1 + out_cells));  // (NaN: the low end)
        step[k] = at(d, k) > 0.0f ? 1 : (at(d, k) < 0.0f ? -1 : 0);
      }
      const float dmax = q_maxabs(d);
      const float tpad = dmax > 0.0f ? G.h / dmax : kInf;  // one cell along the fastest axis: covers the rounding of the crossings
      const int max_steps = G.dims[0] + G.dims[1] + G.dims[2] + 6 * out_cells + 3;
      for (int s = 0; s < max_steps; ++s) {
        float tn;
        const int ax = q_next_crossing(G, c, step, p, d, tn);
        const float tube = q_ray_tube(G.rmin, dlen * fminf(tn, t1) + 6.0f * G.h);
        const int r = !(tube <= 0.25f * G.margin) ? (int)fminf(ceilf(tube * G.inv_h), 3.0f) : 0;  // (NaN: every body)
        if (!(r <= 2)) { every_body(); break; }
        q_ray_cells(G, T, c, r, p, d, dt, ign, best);  // (the cells around c that the grid has: none for a c far beside it)
        if (ax < 0 || !(tn <= t1 + tpad)) break;
        if (best.have && tn > best.t + tpad) break;
        c[ax] += step[ax];
        if (c[ax] < -out_cells || c[ax] >= G.dims[ax] + out_cells) break;
      }
    }
  }
  q_ray_store(out + 7 * i, best);
}

// ---- swept spheres and capsules (mgf_world_sweep_many) ----------------------------------------------------------------------
// The earliest contact of a cast: (t, kind, index, part, order emitted within the target) ascending, whatever order the targets are
// visited in; a contact whose t is not finite is not a candidate (include/mgf_hip.h)
struct SweepBest {
  // the key as two words: t (ordered-int, -0 taken as +0), then kind (2 bits) | index (32) | part (19) | order (1); sub = ~0: no contact
  int tk = 0x7FFFFFFF;
  uint64_t sub = ~0ull;
  Contact c;
  __device__ __forceinline__ bool have() const { return sub != ~0ull; }
  __device__ __forceinline__ void offer(const Contact& k, int kd, uint32_t idx, uint32_t pt, uint32_t ord) {
    if (!(fabsf(k.t) < kInf)) return;
    const int t = f_ord(k.t + 0.0f);
    const uint64_t u = ((uint64_t)kd << 52) | ((uint64_t)idx << 20) | ((uint64_t)(pt & 0x7FFFFu) << 1) | (uint64_t)(ord & 1u);
    if (t < tk || (t == tk && u < sub)) { tk = t; sub = u; c = k; }
  }
  __device__ __forceinline__ int kind() const { return (int)(sub >> 52); }
  __device__ __forceinline__ uint32_t index() const { return (uint32_t)(sub >> 20); }
  __device__ __forceinline__ uint32_t part() const { return (uint32_t)(sub >> 1) & 0x7FFFFu; }
  // for bq_reduce (k_batch_query.h)
  static constexpr uint32_t kRed = 4;  // float4 words of a packed candidate
  __device__ __forceinline__ SweepBest shfl(int off) const {
    SweepBest o;
    o.tk = __shfl_xor(tk, off);
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)sub, off), hi = (uint32_t)__shfl_xor((int)(uint32_t)(sub >> 32), off);
    o.sub = ((uint64_t)hi << 32) | lo;
    o.c.a = q_shfl3(c.a, off); o.c.b = q_shfl3(c.b, off); o.c.n = q_shfl3(c.n, off); o.c.t = __shfl_xor(c.t, off);
    return o;
  }
  __device__ __forceinline__ void pack(float4* w) const {
    w[0] = make_float4(u2f((uint32_t)tk), u2f((uint32_t)sub), u2f((uint32_t)(sub >> 32)), c.t);
    w[1] = mk4(c.a, 0.0f); w[2] = mk4(c.b, 0.0f); w[3] = mk4(c.n, 0.0f);
  }
  static __device__ __forceinline__ SweepBest unpack(const float4* w) {
    const float4 r0 = w[0];
    SweepBest o;
    o.tk = (int)f2u(r0.x); o.sub = ((uint64_t)f2u(r0.z) << 32) | f2u(r0.y);
    o.c = mkc(xyz(w[1]), xyz(w[2]), xyz(w[3]), r0.w);
    return o;
  }
  __device__ __forceinline__ void merge(const SweepBest& o) {
    if (o.tk < tk || (o.tk == tk && o.sub < sub)) { tk = o.tk; sub = o.sub; c = o.c; }
  }
};

// The cast: its shape at t = 0, its sweep, and the bounding sphere (centre cc, radius cr) that the cheap reject moves along the sweep
struct SweepCast {
  Comp s;
  V3 v;
  V3 cc;
  float cr;
  float pad;  // the reject's absolute pad: the grid's margin, a millimetre and the rounding of the path's arithmetic
};

// May a target component, through its bounding sphere, touch the cast's bounding sphere somewhere along the sweep?  Every contact the
// single tests report is a touching of the two shapes at some t in [0, 1]; the radii carry 1 % for the tests' own rounding.
__device__ __forceinline__ bool q_sweep_far(const Comp& A, const SweepCast& K) {
  const bool sa = A.kind == KIND_SPHERE;
  const V3 ma = sa ? A.p : A.p + A.d * 0.5f;
  const float ra = sa ? A.r : A.r + 0.5f * mag(A.d);
  const V3 w = ma - K.cc;
  const float vv = dot(K.v, K.v);
  const float s = vv > 0.0f ? fminf(fmaxf(dot(w, K.v) / vv, 0.0f), 1.0f) : 0.0f;
  const V3 e = w - K.v * s;
  const float lim = (ra + K.cr) * 1.01f + K.pad;
  return dot(e, e) > lim * lim;  // (NaN: not far - the test decides)
}

// every component of slot s: the body's Contacts<Moving<cast>> (collision.rs:1089-1356)
__device__ __forceinline__ void q_sweep_body(const QueryTargets& T, uint32_t s, const SweepCast& K, int32_t ign, SweepBest& best) {
  const uint32_t e = T.ext ? T.ext[s] : s;
  if ((int32_t)e == ign) return;
  const Bodies& B = T.B;
  const uint32_t pc = B.pcount ? B.pcount[s] : 0u;
  const uint32_t np = pc ? pc : 1u;
  for (uint32_t k = 0; k < np; ++k) {
    float4 a, b;
    if (pc) world_part(B, s, k, pc, a, b);
    else { a = B.col0[s]; b = B.col1[s]; }
    const Comp t = to_comp(a, b);
    if (q_sweep_far(t, K)) continue;
    Contact c;
    if (comp_mcomp(t, K.s, K.v, &c)) best.offer(c, MGF_HIT_BODY, e, k, 0u);
  }
}

// Contacts<Moving<_>> for Poly (collision.rs:610-1000) of every face the walk of the mesh BVH with the cast's padded swept box reaches.
// A capsule's face test reaches further than the capsule: its axis test (:698-719) measures the start's distance to the plane along the
// unit axis but steps along the whole one, so it answers at t = 0 for a capsule up to max(1, |d|) from the face - the box grows by that.
// A capsule that does not move tests every face: the fallback (:901-1060) then casts rays of direction 0, whose tests divide by
// |delta|^2 and can answer at t = 0 at a face nowhere near the capsule.
template <class Mesh>
__device__ __forceinline__ void q_sweep_terrain(const Mesh& M, const SweepCast& K, uint32_t* err, SweepBest& best) {
  const bool every = K.s.kind != KIND_SPHERE && mag2(K.v) == 0.0f;
  const float reach = K.s.kind == KIND_SPHERE ? 0.0f : fmaxf(1.0f, mag(K.s.d));
  const V3 mx = mk3(M.x[0], M.x[1], M.x[2]);
  Box q = swept_bounds(K.s, K.v);
  q.c = q.c + -mx;  // the tree's boxes are in the mesh's frame
  q_mesh_walk(
      M, err,
      [&](V3 c, V3 r) {
        const float pad = 1e-5f * (q_maxabs(c) + q_maxabs(r) + q_maxabs(mx) + q_maxabs(q.c) + q_maxabs(q.r)) + 1e-6f + reach;
        return every || (fabsf(c.x - q.c.x) <= r.x + q.r.x + pad && fabsf(c.y - q.c.y) <= r.y + q.r.y + pad && fabsf(c.z - q.c.z) <= r.z + q.r.z + pad);
      },
      [&](uint32_t f) {
        const Triangle tri = q_face(M, mx, f);
        Contact c0, c1;
        if (K.s.kind == KIND_SPHERE) {
          if (tri_msphere(tri, mks(K.s.p, K.s.r), K.v, &c0)) best.offer(c0, MGF_HIT_TERRAIN, f, 0u, 0u);
        } else {
          const int m = tri_mcapsule(tri, mkcap(K.s.p, K.s.d, K.s.r), K.v, c0, c1);
          if (m > 0) best.offer(c0, MGF_HIT_TERRAIN, f, 0u, 0u);
          if (m > 1) best.offer(c1, MGF_HIT_TERRAIN, f, 0u, 1u);
        }
      });
}

// the grid cells [lo, hi] (clamped to the grid)
__device__ __forceinline__ void q_sweep_cells(const QueryGrid& G, const QueryTargets& T, const int lo[3], const int hi[3], const SweepCast& K, int32_t ign,
                                              SweepBest& best) {
  for (int z = max(lo[2], 0); z <= min(hi[2], G.dims[2] - 1); ++z)
    for (int y = max(lo[1], 0); y <= min(hi[1], G.dims[1] - 1); ++y)
      for (int x = max(lo[0], 0); x <= min(hi[0], G.dims[0] - 1); ++x) {
        const uint32_t cell = (uint32_t)x + (uint32_t)G.dims[0] * ((uint32_t)y + (uint32_t)G.dims[1] * (uint32_t)z);
        for (uint32_t k = G.start[cell], ke = G.start[cell + 1]; k < ke; ++k) q_sweep_body(T, G.items[k], K, ign, best);
      }
}

__device__ __forceinline__ SweepCast q_sweep_cast(const MovingIn& m, const QueryGrid& G) {
  SweepCast K;
  K.s.kind = m.tag; K.s.p = ld3(m.p); K.s.d = m.tag == KIND_SPHERE ? mk3(0.0f, 0.0f, 0.0f) : ld3(m.d); K.s.r = m.r;
  K.v = ld3(m.delta);
  const Box sb = comp_bounds(K.s);
  K.cc = sb.c; K.cr = sb.r.x;
  K.pad = G.margin + 1e-3f + 1e-5f * (q_maxabs(K.cc) + q_maxabs(K.v));
  return K;
}
__device__ __forceinline__ void q_sweep_store(int32_t* o, const SweepBest& best) {
  if (best.have()) {
    o[0] = best.kind(); o[1] = (int32_t)best.index(); o[2] = (int32_t)best.part();
    const Contact& c = best.c;
    o[3] = (int32_t)f2u(c.a.x); o[4] = (int32_t)f2u(c.a.y); o[5] = (int32_t)f2u(c.a.z);
    o[6] = (int32_t)f2u(c.b.x); o[7] = (int32_t)f2u(c.b.y); o[8] = (int32_t)f2u(c.b.z);
    o[9] = (int32_t)f2u(c.n.x); o[10] = (int32_t)f2u(c.n.y); o[11] = (int32_t)f2u(c.n.z);
    o[12] = (int32_t)f2u(c.t);
  } else {
#pragma unroll
    for (int k = 0; k < 13; ++k) o[k] = k == 0 ? MGF_HIT_NONE : 0;
  }
}

// a stored record taken up again by a later launch (the order within its target does not matter there: the launches offer different
// kinds of target, or only bodies of one part)
__device__ __forceinline__ SweepBest q_sweep_load(const int32_t* o) {
  SweepBest best;
  if (o[0] != MGF_HIT_NONE)
    best.offer(mkc(mk3(u2f(o[3]), u2f(o[4]), u2f(o[5])), mk3(u2f(o[6]), u2f(o[7]), u2f(o[8])), mk3(u2f(o[9]), u2f(o[10]), u2f(o[11])), u2f(o[12])), o[0],
               (uint32_t)o[1], (uint32_t)o[2], 0u);
  return best;
}

// A lane per cast, in two kernels (one held the walks of all four kinds of target live at once and spilled scalar registers inside its
// nested cell loops): k_query_sweep tests the large bodies, the obstacles and the terrain and writes its best contact; k_query_sweep_cells
// takes that contact up again and walks the grid.  The ranking does not depend on the visiting order, so the split changes no answer.
__global__ __launch_bounds__(kBlock) void k_query_sweep(QueryGrid G, QueryTargets T, const MovingIn* casts, int64_t n, const int32_t* ignore, int32_t mask,
                                                        int32_t* out /* 13 words per cast: mgf_sweep_hit */) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const SweepCast K = q_sweep_cast(casts[i], G);
  const int32_t ign = ignore ? ignore[i] : -1;
  SweepBest best;
  if (mask & MGF_QUERY_BODIES) {
    const uint32_t nl = *G.n_large;
    for (uint32_t k = 0; k < nl; ++k) q_sweep_body(T, G.large[k], K, ign, best);
  }
  if (mask & MGF_QUERY_OBSTACLES)
    for (uint32_t o = 0; o < T.n_obs; ++o)
      compound_contacts_walk(T.obs[o], K.s, K.v, [&](uint32_t ci, const Contact& c) { best.offer(c, MGF_HIT_OBSTACLE, o, ci, 0u); });
  if ((mask & MGF_QUERY_TERRAIN) && T.M.n_nodes) q_sweep_terrain(T.M, K, T.err, best);
  q_sweep_store(out + 13 * i, best);
}

// The grid walk is a DDA along the path of the centre of the cast's box: at each cell c it covers the block c +- R, R = the cells the
// box's half extent (plus the margin) can reach from c, so a body the cast touches at t is in the block of the cell the centre is in at t.
// The first cell visits its whole block, each step after it only the slab of cells the step brings into the block (the walk moves one
// cell along one axis at a time: no cell twice).  The walk stops once the next cell starts beyond the best t by a cell's worth of time,
// as the ray walk does.  (Launched only when bodies are asked for and the grid has cells.)
__global__ __launch_bounds__(kBlock) void k_query_sweep_cells(QueryGrid G, QueryTargets T, const MovingIn* casts, int64_t n, const int32_t* ignore,
                                                              int32_t* out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const SweepCast K = q_sweep_cast(casts[i], G);
  const int32_t ign = ignore ? ignore[i] : -1;
  int32_t* o = out + 13 * i;
  SweepBest best = q_sweep_load(o);  // k_query_sweep's answer
  const Box sb = comp_bounds(K.s);
  const float dmax = q_maxabs(K.v);
  // the block's half extent in cells; a cast whose own rounding (far from the grid, a long sweep) may exceed the margin takes one more.
  // (a block as wide as the grid along an axis covers that axis wherever the centre is: the walk ignores the axis)
  const bool fat = 4e-7f * (q_maxabs(K.cc) + dmax) > 0.25f * G.margin;
  int R[3];
  bool whole[3];
  float elo[3], ehi[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    R[k] = (int)fminf(ceilf((at(sb.r, k) + G.margin) * G.inv_h) + (fat ? 1.0f : 0.0f), (float)G.dims[k]);  // (NaN: the whole grid)
    whole[k] = R[k] >= G.dims[k];
    elo[k] = G.lo[k] - (float)(R[k] + 1) * G.h;
    ehi[k] = G.lo[k] + (float)(G.dims[k] + R[k] + 1) * G.h;
  }
  // clip the centre's path to the grid's box grown by the block (beyond it a block holds no cell of the grid)
  float t0 = 0.0f, t1 = 1.0f;
  if (q_clip(K.cc, K.v, elo, ehi, whole, t0, t1)) {
    const V3 e = K.cc + K.v * t0;
    int c[3], step[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float f = floorf((at(e, k) - G.lo[k]) * G.inv_h);
      c[k] = whole[k] ? 0 : (int)fminf(fmaxf(f, (float)(-R[k] - 1)), (float)(G.dims[k] + R[k]));  // (NaN: the low end)
      step[k] = whole[k] ? 0 : (at(K.v, k) > 0.0f ? 1 : (at(K.v, k) < 0.0f ? -1 : 0));
    }
    const float tpad = dmax > 0.0f ? G.h / dmax : kInf;
    int lo[3], hi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { lo[k] = c[k] - R[k]; hi[k] = c[k] + R[k]; }
    q_sweep_cells(G, T, lo, hi, K, ign, best);
    const int max_steps = G.dims[0] + G.dims[1] + G.dims[2] + 2 * (R[0] + R[1] + R[2]) + 6;
    for (int s = 0; s < max_steps; ++s) {
      float tn;
      const int ax = q_next_crossing(G, c, step, K.cc, K.v, tn);
      if (ax < 0 || !(tn <= t1 + tpad)) break;
      if (best.have() && tn > best.c.t + tpad) break;
      c[ax] += step[ax];
      if (c[ax] < -R[ax] - 1 || c[ax] > G.dims[ax] + R[ax]) break;
#pragma unroll
      for (int k = 0; k < 3; ++k) { lo[k] = c[k] - R[k]; hi[k] = c[k] + R[k]; }
      lo[ax] = hi[ax] = c[ax] + step[ax] * R[ax];  // the slab the step brings in
      q_sweep_cells(G, T, lo, hi, K, ign, best);
    }
  }
  q_sweep_store(o, best);
}

// Overlaps<AABB> (collision.rs:22) of each query box with every body's tight box; a body filed in several cells is tested in the
// first cell (lowest x, y, z) its range shares with the box's.  FILL writes caller indices at off[i], unsorted.
template <bool FILL>
__global__ __launch_bounds__(kBlock) void k_query_overlap(QueryGrid G, const uint32_t* ext, const float4* qb_c, const float4* qb_r, const float* boxes,
                                                          int64_t n, uint32_t* cnt, const uint32_t* off, uint32_t* out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  Box Q; Q.c = ld3(boxes + 6 * i); Q.r = ld3(boxes + 6 * i + 3);
  uint32_t m = 0;
  const uint32_t base = FILL ? off[i] : 0u;
  auto test = [&](uint32_t s) {
    Box b; b.c = xyz(qb_c[s]); b.r = xyz(qb_r[s]);
    if (box_overlaps(b, Q)) {
      if (FILL) out[base + m] = ext ? ext[s] : s;
      ++m;
    }
  };
  const uint32_t nl = *G.n_large;
  for (uint32_t k = 0; k < nl; ++k) test(G.large[k]);
  if (G.dims[0] > 0) {
    bool outside = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float ghi = G.lo[k] + (float)G.dims[k] * G.h;
      if (at(Q.c, k) + at(Q.r, k) + G.margin < G.lo[k] || at(Q.c, k) - at(Q.r, k) - G.margin > ghi) outside = true;
      if (!(at(Q.c, k) == at(Q.c, k)) || !(at(Q.r, k) == at(Q.r, k))) outside = true;  // (NaN: Overlaps is false for every body)
    }
    if (!outside) {
      int lo[3], hi[3];
      Box Qc = Q;  // (a negative half extent: Overlaps can still hold, and only for a body whose box holds Q.c - the cells of Q.c, not an empty range)
      Qc.r = mk3(fmaxf(Q.r.x, 0.0f), fmaxf(Q.r.y, 0.0f), fmaxf(Q.r.z, 0.0f));
      q_cell_range(Qc, G, lo, hi);
      for (int z = lo[2]; z <= hi[2]; ++z)
        for (int y = lo[1]; y <= hi[1]; ++y)
          for (int x = lo[0]; x <= hi[0]; ++x) {
            const uint32_t cell = (uint32_t)x + (uint32_t)G.dims[0] * ((uint32_t)y + (uint32_t)G.dims[1] * (uint32_t)z);
            for (uint32_t k = G.start[cell], ke = G.start[cell + 1]; k < ke; ++k) {
              const uint32_t s = G.items[k];
              Box b; b.c = xyz(qb_c[s]); b.r = xyz(qb_r[s]);
              int blo[3], bhi[3];
              q_cell_range(b, G, blo, bhi);
              if (x != max(blo[0], lo[0]) || y != max(blo[1], lo[1]) || z != max(blo[2], lo[2])) continue;  // tested in another cell
              test(s);
            }
          }
    }
  }
  if (!FILL) cnt[i] = m;
}

// each query's list into ascending order: heap sort by one lane, in place
__global__ __launch_bounds__(kBlock) void k_query_sort(const uint32_t* off, int64_t n, uint32_t* vals) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  uint32_t* a = vals + off[i];
  const uint32_t len = off[i + 1] - off[i];
  auto sift = [&](uint32_t root, uint32_t end) {
    const uint32_t v = a[root];
    while (2 * root + 1 < end) {
      uint32_t ch = 2 * root + 1;
      if (ch + 1 < end && a[ch + 1] > a[ch]) ++ch;
      if (a[ch] <= v) break;
      a[root] = a[ch];
      root = ch;
    }
    a[root] = v;
  };
  for (uint32_t s = len / 2; s-- > 0;) sift(s, len);
  for (uint32_t end = len; end > 1; --end) {
    const uint32_t t = a[0]; a[0] = a[end - 1]; a[end - 1] = t;
    sift(0, end - 1);
  }
}

}  // namespace mgf
