// Queries against a world's resident bodies, terrain and obstacles between ticks (mgf_world_raycast_many,
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
//   k_query_overlap<F> a lane per box: the cells it touches (a body is tested in the first cell it shares with the box), the
//                      large bodies; count, scan, fill, then k_query_sort puts each list into the caller's order
// Which of the targets a hit belongs to never depends on the visiting order: hits are ranked by (t, kind, index, part).
// Every acceleration step is conservative (cells and boxes padded by QueryGrid::margin); each answer comes from the
// reference's single-shape test.
#pragma once
#include "k_api.h"

namespace mgf {

struct QueryGrid {
  float lo[3];
  float h, inv_h;
  int dims[3];
  float margin;            // world-space pad of every box the grid files or looks up (covers the rounding of the walk)
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

// BoundedBy<AABB> of slot i: its collider, or the union of its parts in order (what k_integrate's tight box is, unswept)
__device__ __forceinline__ Box q_body_box(const Bodies& B, uint32_t i) {
  const uint32_t pc = B.pcount ? B.pcount[i] : 0u;
  Box tb;
  if (pc) {
    for (uint32_t k = 0; k < pc; ++k) {
      float4 a, b;
      world_part(B, i, k, pc, a, b);
      Comp part; part.kind = (int)f2u(b.w); part.p = xyz(a); part.d = xyz(b); part.r = a.w;
      const Box pb = comp_bounds(part);
      tb = k == 0 ? pb : box_combine(tb, pb);
    }
  } else {
    const float4 a = B.col0[i], b = B.col1[i];
    Comp c; c.kind = (int)f2u(b.w); c.p = xyz(a); c.d = xyz(b); c.r = a.w;
    tb = comp_bounds(c);
  }
  return tb;
}

// bounds[0..2] = ordered-int min of the padded low corners, [3..5] max of the high corners (bodies that go to the grid): reduced
// across the wave first, one atomic per wave and word
__global__ __launch_bounds__(kBlock) void k_query_boxes(Bodies B, uint32_t n, float h, float margin, float4* qb_c, float4* qb_r, int* bounds,
                                                        uint32_t* large, uint32_t* n_large) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  int lo[3] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF}, hi[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
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
    }
  }
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

struct QueryBest {
  bool have = false;
  int kind = -1;
  uint32_t index = 0, part = 0;
  V3 p = mk3(0.0f, 0.0f, 0.0f);
  float t = 0.0f;
  // (t, kind, index, part) ascending: the rule of the definition, whatever order the targets are visited in
  __device__ __forceinline__ void offer(V3 ip, float it, int k, uint32_t idx, uint32_t pt) {
    const bool better = !have || it < t || (it == t && (k < kind || (k == kind && (idx < index || (idx == index && pt < part)))));
    if (better) { have = true; kind = k; index = idx; part = pt; p = ip; t = it; }
  }
};

// conservative slab test of a particle against a padded box: may the particle meet the box at a parameter in [0, tmax]?
__device__ __forceinline__ bool q_slab(V3 p, V3 d, V3 c, V3 r, float pad, float tmax) {
  float t0 = 0.0f, t1 = tmax;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
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

struct QueryTargets {
  Bodies B;
  const uint32_t* ext;   // slot -> caller index (null: identity)
  const float4* qb_c;
  const float4* qb_r;
  TerrainDev M;          // n_nodes 0: no terrain
  const CompoundDev* obs;
  uint32_t n_obs;
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

// Intersects<Compound> compound.rs:309-332 (k_compound_intersections' walk), with the component that answered
__device__ __forceinline__ void q_ray_obstacle(const CompoundDev& D, uint32_t o, const ParticleIn& q, uint32_t* err, QueryBest& best) {
  V3 pp = ld3(q.p), pd = ld3(q.d), disp = ld3(D.disp);
  const float dt = q.dt;
  Quat rot = mkq(D.rot[0], mk3(D.rot[1], D.rot[2], D.rot[3]));
  Quat conj = mkq(rot.s, -rot.v);
  V3 rp = rotate(conj, pp + -disp) + disp, rd = rotate(conj, pd);
  bool have = false;
  V3 best_p = mk3(0, 0, 0); float best_t = 0.0f;
  uint32_t best_c = 0;
  uint32_t stack[kStack];
  int sp = 0;
  if (D.tree.n_nodes) stack[sp++] = D.tree.root;
  while (sp > 0) {
    uint32_t top = stack[--sp];
    const float4* raw = reinterpret_cast<const float4*>(&D.tree.nodes[top]);
    float4 n0 = raw[0], n1 = raw[1];
    Box nb; nb.c = xyz(n0); nb.r = xyz(n1);
    V3 ip; float t;
    if (ray_box(rp, rd, nb, &ip, &t, kInf)) {
      uint32_t w0 = f2u(n0.w), w1 = f2u(n1.w);
      if (w0 & 0x80000000u) {
        if (!(t > dt)) {
          const uint32_t ci = w0 & 0x7FFFFFFFu;
          Comp shape = comp_rotate(to_comp(D.comps[ci]), rot);
          shape.p = shape.p + disp;
          V3 sip; float st;
          if (intersection_dispatch(q, comp_shape(shape), &sip, &st) == 1 && !(have && st > best_t)) { best_p = sip; best_t = st; best_c = ci; have = true; }
        }
      } else if (sp + 2 <= kStack) { stack[sp++] = w0; stack[sp++] = w1; }
      else *err = 1u;
    }
  }
  if (have) best.offer(best_p, best_t, MGF_HIT_OBSTACLE, o, best_c);
}

// Intersects<Triangle> of every face the padded walk of the mesh BVH reaches
__device__ __forceinline__ void q_ray_terrain(const TerrainDev& M, V3 p, V3 d, float dt, uint32_t* err, QueryBest& best) {
  const V3 mx = mk3(M.x[0], M.x[1], M.x[2]);
  const V3 lp = p + -mx;  // the tree's boxes are in the mesh's frame
  uint32_t stack[kStack];
  int sp = 0;
  stack[sp++] = M.root;
  while (sp > 0) {
    const uint32_t top = stack[--sp];
    const float4* raw = reinterpret_cast<const float4*>(&M.nodes[top]);
    const float4 n0 = raw[0], n1 = raw[1];
    const V3 c = xyz(n0), r = xyz(n1);
    const float pad = 1e-5f * (q_maxabs(c) + q_maxabs(r) + q_maxabs(mx) + q_maxabs(p)) + 1e-6f;
    const float lim = best.have ? fminf(dt, best.t * 1.0001f + 1e-6f) : dt;
    if (!q_slab(lp, d, c, r, pad, lim)) continue;
    const uint32_t w0 = f2u(n0.w), w1 = f2u(n1.w);
    if (w0 & 0x80000000u) {
      const uint32_t f = w0 & 0x7FFFFFFFu;
      const uint4 fi = M.faces[f];
      const Triangle tri = mkt(xyz(M.verts[fi.x]) + mx, xyz(M.verts[fi.y]) + mx, xyz(M.verts[fi.z]) + mx);
      V3 ip; float t;
      if (ray_triangle(p, d, tri, &ip, &t, dt)) best.offer(ip, t, MGF_HIT_TERRAIN, f, 0u);
    } else if (sp + 2 <= kStack) { stack[sp++] = w0; stack[sp++] = w1; }
    else *err = 1u;
  }
}

// the grid cell (x, y, z) - with `fat`, its 3x3x3 neighbourhood - for one particle
__device__ __forceinline__ void q_ray_cells(const QueryGrid& G, const QueryTargets& T, const int c[3], bool fat, V3 p, V3 d, float dt, int32_t ign,
                                            QueryBest& best) {
  const int r = fat ? 1 : 0;
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
  if (d.x == 0.0f && d.y == 0.0f && d.z == 0.0f) mask = 0;  // (no direction: the reference's tests divide by |d|^2 = 0 - no hit, by definition)
  if (mask & MGF_QUERY_BODIES) {
    const uint32_t nl = *G.n_large;
    for (uint32_t k = 0; k < nl; ++k) q_ray_body(T, G.large[k], p, d, dt, ign, best);
  }
  if (mask & MGF_QUERY_OBSTACLES)
    for (uint32_t o = 0; o < T.n_obs; ++o) q_ray_obstacle(T.obs[o], o, q, T.err, best);
  if ((mask & MGF_QUERY_TERRAIN) && T.M.n_nodes) q_ray_terrain(T.M, p, d, dt, T.err, best);
  if ((mask & MGF_QUERY_BODIES) && G.dims[0] > 0) {
    // clip to the grid's box, then walk its cells in the order the particle enters them (Amanatides-Woo, every crossing parameter
    // computed afresh from the cell's face - nothing accumulates)
    float t0 = 0.0f, t1 = dt;
    bool miss = false;
    float ghi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      ghi[k] = G.lo[k] + (float)G.dims[k] * G.h;
      const float pk = at(p, k), dk = at(d, k);
      if (dk == 0.0f) {
        if (!(pk >= G.lo[k] && pk <= ghi[k])) miss = true;
      } else {
        float ta = (G.lo[k] - pk) / dk, tb = (ghi[k] - pk) / dk;
        if (ta > tb) { const float s = ta; ta = tb; tb = s; }
        t0 = fmaxf(t0, ta); t1 = fminf(t1, tb);
      }
    }
    if (!miss && t0 <= t1) {
      const V3 e = p + d * t0;
      int c[3], step[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) { c[k] = q_cell(at(e, k), k, G); step[k] = at(d, k) > 0.0f ? 1 : (at(d, k) < 0.0f ? -1 : 0); }
      const float dmax = q_maxabs(d);
      const float tpad = dmax > 0.0f ? G.h / dmax : kInf;  // one cell along the fastest axis: covers the rounding of the crossings
      // a particle whose own rounding (its origin far from the grid, a long stretch) may exceed the pad looks at the neighbours too
      const bool fat = 4e-7f * (q_maxabs(p) + dmax * t1) > 0.25f * G.margin;
      const int max_steps = G.dims[0] + G.dims[1] + G.dims[2] + 3;
      for (int s = 0; s < max_steps; ++s) {
        q_ray_cells(G, T, c, fat, p, d, dt, ign, best);
        float tn = kInf;
        int ax = -1;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          if (step[k] == 0) continue;
          const float face = G.lo[k] + (float)(c[k] + (step[k] > 0 ? 1 : 0)) * G.h;
          const float tk = (face - at(p, k)) / at(d, k);
          if (ax < 0 || tk < tn) { tn = tk; ax = k; }
        }
        if (ax < 0 || !(tn <= t1 + tpad)) break;
        if (best.have && tn > best.t + tpad) break;
        c[ax] += step[ax];
        if (c[ax] < 0 || c[ax] >= G.dims[ax]) break;
      }
    }
  }
  int32_t* o = out + 7 * i;
  if (best.have) {
    o[0] = best.kind; o[1] = (int32_t)best.index; o[2] = (int32_t)best.part;
    o[3] = (int32_t)f2u(best.p.x); o[4] = (int32_t)f2u(best.p.y); o[5] = (int32_t)f2u(best.p.z); o[6] = (int32_t)f2u(best.t);
  } else {
    o[0] = MGF_HIT_NONE; o[1] = 0; o[2] = 0; o[3] = 0; o[4] = 0; o[5] = 0; o[6] = 0;
  }
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
      q_cell_range(Q, G, lo, hi);
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
