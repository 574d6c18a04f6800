// Many small independent worlds stepped together (mgf_batch_*, DESIGN.md "many small worlds").  (Part of the kernel set described in kernels.h.)
//
// One workgroup runs the whole tick of one world - World::step, mgf_demo/world.rs:227-294, in the canonical constraint order - and no
// workgroup ever waits for another: a batch may hold more worlds than the device holds workgroups, and it shares a device safely.
// A tick is six launches, each a workgroup per world, whatever the number of worlds:
//   k_batch_front   complete_motion + integrate (physics.rs:222-269), the swept tight box and the persistent fat box with the refit rule
//                   (world.rs:235-238), both kept in LDS; per body i its candidates in the list's order - the mesh faces in mesh-BVH DFS
//                   order (mesh.rs:115-139), then the components of the world's obstacles its swept box meets (the oracle's
//                   World::obstacles: the obstacles in list order, the components in the order Compound::contacts visits them,
//                   compound.rs:334-352), then the partners j < i whose fat box overlaps i's tight box, ascending - counted, scanned
//                   and listed
//   k_batch_faces / k_batch_pairs / k_batch_pack
//                   the face tests and the pair tests, a lane per candidate (a component of an obstacle is tested beside the pairs);
//                   then the contacts packed in the list's order: contact c is constraint c (every terrain or obstacle contact a
//                   constraint of its own, world.rs:243-251; a pair's one contact is its manifold, manifold.rs:131-148)
//   k_batch_setup   ContactConstraint::new (solver.rs:101-191) a lane per contact; per body the length of its own range of the list
//                   (it is `a` there) and how often it is `b`
//   k_batch_solve   per body the constraints it takes part in as `b`, sorted: behind its own range that is the body's chain in list
//                   order, and every record gets its rank in the chain of each of its bodies; then Solver::solve (solver.rs:72-78) with
//                   the solver record of every body in LDS: a lane takes the constraints c = t, t + T, .. of every iteration in turn and
//                   solves one as soon as both its bodies' progress counters have reached its rank (the order per body is the list's,
//                   which is all the sequential sweep defines)
// A world whose share of the candidate or constraint storage is too small for the tick puts its bodies back as the tick found them
// (TickUndo) and leaves its tick counter where it was; the host grows the share and runs the tick again (counter "capacity_retries").
// A batch that holds bodies of several components (mgf_batch_add_compound_bodies) runs k_batch_parts.h's front, faces, obstacle, pair and
// pack launches in the first four's places; the kernels here are its tick's last two, and the whole tick of every other batch.
#pragma once
#include "k_api.h"

namespace mgf {

constexpr int kBatchBlock = 256;
constexpr uint32_t kBatchSpinLimit = 1u << 22;  // trips of the solve loop without progress after which a lane gives up (a bug, never a wait for another workgroup)

// The mesh BVH in the order BVH::query visits it (bvh.rs:283-310: push lchild, push rchild, pop rchild first), each node with the index
// of the first node behind its subtree: a walk without a stack - and so without scratch memory - that reports the same leaves in the same order.
//   node = (c.xyz, w0), (r.xyz, skip); leaf: w0 = 0x80000000 | face.
struct BatchTerrain { const float4* nodes; const float4* verts; const uint4* faces; uint32_t n_nodes; float x[3]; uint32_t obst; };
// The meshes of the batch's terrain table, one behind the other in one store each of nodes, vertices and faces (a node's skip index, a
// face's vertex indices and the face index of a leaf are the mesh's own), and what world k has of it: desc[2k] = (first node, first
// vertex, first face, nodes - 0: no terrain), desc[2k + 1] = (the world's mesh position, the world's range of the obstacle descriptors:
// first << 7 | count - BatchObstacles below; a world's environment is one load).
struct BatchTerrains { const float4* nodes; const float4* verts; const uint4* faces; const uint4* desc; };
__device__ __forceinline__ BatchTerrain batch_terrain_of(const BatchTerrains& T, uint32_t k) {
  const uint4 d0 = T.desc[2 * (size_t)k], d1 = T.desc[2 * (size_t)k + 1];
  BatchTerrain M;
  M.nodes = T.nodes + 2 * (size_t)d0.x; M.verts = T.verts + d0.y; M.faces = T.faces + d0.z; M.n_nodes = d0.w;
  M.x[0] = u2f(d1.x); M.x[1] = u2f(d1.y); M.x[2] = u2f(d1.z);
  M.obst = d1.w;
  return M;
}

template <class F>
__device__ __forceinline__ void batch_terrain_walk(const BatchTerrain& M, const Box& q, F&& emit) {
  for (uint32_t at = 0; at < M.n_nodes;) {
    const float4 n0 = M.nodes[2 * (size_t)at], n1 = M.nodes[2 * (size_t)at + 1];
    Box nb; nb.c = xyz(n0); nb.r = xyz(n1);
    const bool hit = box_overlaps(q, nb);
    const uint32_t w0 = f2u(n0.w);
    if (hit && (w0 & 0x80000000u)) emit(w0 & 0x7FFFFFFFu);
    at = hit ? at + 1u : f2u(n1.w);
  }
}

// The static Compound obstacles of the worlds (the oracle's World::obstacles, as mgf_world_add_obstacle's).  The entries of the batch's
// obstacle table sit one behind the other in one store of threaded trees (as a mesh's: a leaf's w0 = 0x80000000 | component, a skip
// index is the entry's own) and one of components; world k's list is a range of the descriptors (the fourth word of the world's
// second terrain descriptor: first << 7 | count), three words each: (first node, nodes, first component, -), (disp, rot.s),
// (rot.xyz, -) - the pose is the list entry's, the geometry the table's.  The tick's kernels find the three stores behind the last
// world's terrain descriptors (desc[2 n_worlds], desc[2 n_worlds + 1]: the pointers' words), read only by a world that has obstacles:
// their argument block is what it was, and k_batch_front has no scalar register to spare.
struct BatchObstacle { const float4* nodes; const CompIn* comps; uint32_t n_nodes; float disp[3]; float rot[4]; };
struct BatchObstacles { const float4* nodes; const CompIn* comps; const uint4* desc; };
constexpr uint32_t kBatchObstCountBits = 7;
__device__ __forceinline__ uint32_t batch_obst_first(uint32_t range) { return range >> kBatchObstCountBits; }
__device__ __forceinline__ uint32_t batch_obst_count(uint32_t range) { return range & ((1u << kBatchObstCountBits) - 1u); }
__device__ __forceinline__ BatchObstacles batch_obstacles_of(const BatchTerrains& T, uint32_t n_worlds) {
  const uint4 h0 = T.desc[2 * (size_t)n_worlds], h1 = T.desc[2 * (size_t)n_worlds + 1];
  BatchObstacles O;
  O.nodes = reinterpret_cast<const float4*>(((uint64_t)h0.y << 32) | h0.x);
  O.comps = reinterpret_cast<const CompIn*>(((uint64_t)h0.w << 32) | h0.z);
  O.desc = reinterpret_cast<const uint4*>(((uint64_t)h1.y << 32) | h1.x);
  return O;
}
__device__ __forceinline__ BatchObstacle batch_obstacle_of(const BatchObstacles& O, uint32_t e) {
  const uint4 d0 = O.desc[3 * (size_t)e], d1 = O.desc[3 * (size_t)e + 1], d2 = O.desc[3 * (size_t)e + 2];
  BatchObstacle D;
  D.nodes = O.nodes + 2 * (size_t)d0.x; D.n_nodes = d0.y; D.comps = O.comps + d0.z;
  D.disp[0] = u2f(d1.x); D.disp[1] = u2f(d1.y); D.disp[2] = u2f(d1.z);
  D.rot[0] = u2f(d1.w); D.rot[1] = u2f(d2.x); D.rot[2] = u2f(d2.y); D.rot[3] = u2f(d2.z);
  return D;
}
// the walk of batch_terrain_walk over an obstacle's tree (compound_contacts_walk, k_api.h): bounded by the node count, no stack
template <class F>
__device__ __forceinline__ void compound_box_walk(const BatchObstacle& D, const Box& q, F&& emit) {
  for (uint32_t at = 0; at < D.n_nodes;) {
    const float4 n0 = D.nodes[2 * (size_t)at], n1 = D.nodes[2 * (size_t)at + 1];
    Box nb; nb.c = xyz(n0); nb.r = xyz(n1);
    const bool hit = box_overlaps(q, nb);
    const uint32_t w0 = f2u(n0.w);
    if (hit && (w0 & 0x80000000u)) emit(w0 & 0x7FFFFFFFu);
    at = hit ? at + 1u : max(f2u(n1.w), at + 1u);
  }
}
// A candidate against an obstacle: (i | (list slot + 1) << kBatchSlotShift, 0x80000000 | component) - a body's index takes ten bits,
// so a face's and a partner's words are what they were, and a candidate with slot bits is no face.
constexpr uint32_t kBatchSlotShift = 10, kBatchBodyMask = (1u << kBatchSlotShift) - 1u;
static_assert(MGF_BATCH_MAX_BODIES <= (1 << kBatchSlotShift) && MGF_BATCH_MAX_WORLD_OBSTACLES < (1 << (32 - kBatchSlotShift)), "a candidate's first word");
static_assert(MGF_BATCH_MAX_WORLD_OBSTACLES < (1 << kBatchObstCountBits), "a world's range of the obstacle descriptors");

// What a failed tick puts back: 7 words a body.
struct TickUndo { float4* p; uint32_t n; };  // (row r of body g at p[r * n + g]: x, q, srec[0], srec[1], delta, fb_c, fb_r)
__device__ __forceinline__ float4& undo_at(const TickUndo& U, int r, size_t g) { return U.p[(size_t)r * U.n + g]; }

struct BatchArgs {
  Bodies B;                  // every world's bodies, world k at [w_off[k], w_off[k + 1]); bpk is the tick's packed copy
  TickUndo U;
  BatchTerrains T;           // world k's terrain: batch_terrain_of(T, k), k the workgroup's index (wave-uniform loads); its obstacles: batch_obstacles_of(T, n_worlds)
  const uint32_t* w_off;
  uint2* cand;               // world k's candidates at q_off[k], q_cap[k] entries: (i, j), (i, 0x80000000 | face) or (i | slot + 1 << 10, 0x80000000 | component)
  const uint32_t* q_off;
  const uint32_t* q_cap;
  uint32_t* q_count;
  uint32_t* ncq;             // per candidate: its contacts (0 .. 2), in `slot` (two of 3 words per candidate)
  float4* slot;
  float4* cont;              // world k's contacts, 4 words each, and ...
  CRec* cons;                // ... its list at c_off[k], c_cap[k] records
  uint32_t* rows;            // same offsets: the `b` occurrences of every body of the world (CSR)
  const uint32_t* c_off;
  const uint32_t* c_cap;
  uint32_t* na;              // per body: the length of its own range of the list; how often it is `b`
  uint32_t* degb;
  uint32_t* stage;           // 8 * tick + the launches of the tick world k is through
  uint32_t* done;            // ticks of this call world k has completed
  uint32_t* need;            // [2k] candidates, [2k + 1] records the tick that did not fit asked for
  uint32_t* c_count;         // length of the world's list of its last tick
  uint32_t* err;             // [0] a lane of a solve loop gave up
  uint32_t* stats;           // [tick][world][8]: n_bodies, n_constraints, n_terrain_constraints, n_pair_candidates, n_refits
  uint32_t n_worlds, tick, iters;
  float dt, fat_margin, baumgarte, slop;
};

// exclusive scan of a[0 .. n) in place by the first wave, the sum to *total; a barrier on both sides
__device__ __forceinline__ void batch_scan(uint32_t* a, uint32_t n, uint32_t* total) {
  __syncthreads();
  if (threadIdx.x < 64) {
    const uint32_t lane = threadIdx.x, per = (n + 63u) / 64u, lo = min(n, lane * per), hi = min(n, lo + per);
    uint32_t s = 0;
    for (uint32_t e = lo; e < hi; ++e) s += a[e];
    uint32_t incl = s;
    for (int off = 1; off < 64; off <<= 1) { const uint32_t t = __shfl_up(incl, off); if ((int)lane >= off) incl += t; }
    uint32_t run = incl - s;
    for (uint32_t e = lo; e < hi; ++e) { const uint32_t v = a[e]; a[e] = run; run += v; }
    if (lane == 63) *total = incl;
  }
  __syncthreads();
}

struct BatchBody { Comp col; V3 d; };  // collider and motion from a body's packed copy
__device__ __forceinline__ BatchBody batch_load(const Bodies& B, size_t g) {
  const float4 c0 = B.bpk[4 * g], dl = B.bpk[4 * g + 1], c1 = B.bpk[4 * g + 3];
  BatchBody r;
  r.col.p = xyz(c0); r.col.r = c0.w; r.col.d = xyz(c1); r.col.kind = (int)f2u(c1.w);
  r.d = xyz(dl);
  return r;
}

// a launch of the tick has found the world's share of the storage too small (this attempt at the tick is over: `stage` may still say otherwise, from the last)
__device__ __forceinline__ bool batch_failed(const BatchArgs& A, uint32_t k) { return (A.need[2 * k] | A.need[2 * k + 1]) != 0u; }

// the bodies of a world whose tick does not happen, as the tick found them (the packed copy is rebuilt by every tick)
__device__ __forceinline__ void batch_undo(const BatchArgs& A, uint32_t g0, uint32_t n) {
  const Bodies& B = A.B;
  for (uint32_t i = threadIdx.x; i < n; i += kBatchBlock) {
    const size_t g = (size_t)g0 + i;
    B.x[g] = undo_at(A.U, 0, g); B.q[g] = undo_at(A.U, 1, g); B.srec[4 * g] = undo_at(A.U, 2, g); B.srec[4 * g + 1] = undo_at(A.U, 3, g);
    B.delta[g] = undo_at(A.U, 4, g); B.fb_c[g] = undo_at(A.U, 5, g); B.fb_r[g] = undo_at(A.U, 6, g);
  }
}

// batch_undo for k_batch_front, whose argument block is `A` alone: the rows' addresses read afresh from the block.  (Kept from the top of
// the kernel for this one rare path they hold fourteen scalar registers through the candidate loops, which have none to spare.)
__device__ __forceinline__ void batch_undo_front(uint32_t g0, uint32_t n) {
  const volatile BatchArgs* K = (const volatile BatchArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  BatchArgs R;
  R.B.x = K->B.x; R.B.q = K->B.q; R.B.srec = K->B.srec; R.B.delta = K->B.delta; R.B.fb_c = K->B.fb_c; R.B.fb_r = K->B.fb_r;
  R.U.p = K->U.p; R.U.n = K->U.n;
  batch_undo(R, g0, n);
}

// LDS: 64 bytes a body of boxes, one word a body of counts.
__global__ __launch_bounds__(kBatchBlock) void k_batch_front(BatchArgs A) {
  extern __shared__ float4 s_dyn[];
  __shared__ uint32_t s_tot, s_stat[2];
  const uint32_t k = blockIdx.x, T = kBatchBlock, tid = threadIdx.x;
  if (A.done[k] != A.tick) return;  // a world whose earlier tick of this call did not fit: the host runs it again from there
  const uint32_t g0 = A.w_off[k], n = A.w_off[k + 1] - g0;
  const Bodies& B = A.B;
  float4 *s_tc = s_dyn, *s_tr = s_dyn + n, *s_fc = s_dyn + 2 * (size_t)n, *s_fr = s_dyn + 3 * (size_t)n;
  uint32_t* s_off = reinterpret_cast<uint32_t*>(s_dyn + 4 * (size_t)n);
  if (tid < 2) s_stat[tid] = 0u;
  __syncthreads();
  // complete_motion + integrate (k_integrate's update of an ordinary body, restated), boxes
  for (uint32_t i = tid; i < n; i += T) {
    const size_t g = (size_t)g0 + i;
    const float4 xw = B.x[g], dl = B.delta[g], qw = B.q[g], s0 = B.srec[4 * g], s1 = B.srec[4 * g + 1];
    const float4 fc0 = B.fb_c[g], fr0 = B.fb_r[g];
    undo_at(A.U, 0, g) = xw; undo_at(A.U, 1, g) = qw; undo_at(A.U, 2, g) = s0; undo_at(A.U, 3, g) = s1; undo_at(A.U, 4, g) = dl;
    undo_at(A.U, 5, g) = fc0; undo_at(A.U, 6, g) = fr0;
    const float4 p0 = B.sp0[g], p1 = B.sp1[g], ct = B.ctor[g];
    V3 x = xyz(xw) + xyz(dl);  // physics.rs:262-269
    V3 v = mk3(s0.x, s0.y, s0.z), w = mk3(s0.w, s1.x, s1.y);
    const float inv_mass = s1.z;
    Quat q = mkq(qw.x, mk3(qw.y, qw.z, qw.w));
    q = normalize(q + mkq(0.0f, w * A.dt) * 0.5f * q);  // physics.rs:226-227
    const M3 R = m3_from_quat(q);                       // physics.rs:231-232
    const M3 I = R * load_imb(B.imb, (uint32_t)g) * transpose(R);
    v = v + xyz(p0) * inv_mass * A.dt;                  // physics.rs:236, 240
    w = w + I * xyz(p1) * A.dt;
    const V3 d = v * A.dt;                              // physics.rs:244-250
    const Comp col = construct((int)f2u(ct.x), ct.y, ct.z, x, q);
    const Box tb = swept_bounds(col, d);
    B.x[g] = mk4(x, 0.0f);
    B.q[g] = make_float4(q.s, q.v.x, q.v.y, q.v.z);
    B.srec[4 * g] = make_float4(v.x, v.y, v.z, w.x);
    B.srec[4 * g + 1] = make_float4(w.y, w.z, inv_mass, I.c[0].x);
    B.srec[4 * g + 2] = make_float4(I.c[0].y, I.c[0].z, I.c[1].x, I.c[1].y);
    B.srec[4 * g + 3] = make_float4(I.c[1].z, I.c[2].x, I.c[2].y, I.c[2].z);
    B.delta[g] = mk4(d, p1.w);
    B.bpk[4 * g] = mk4(col.p, col.r); B.bpk[4 * g + 1] = mk4(d, p1.w);
    B.bpk[4 * g + 2] = mk4(x + d, p0.w); B.bpk[4 * g + 3] = mk4(col.d, u2f((uint32_t)col.kind));
    Box fb; fb.c = xyz(fc0); fb.r = xyz(fr0);
    if (!box_contains(fb, tb)) {  // world.rs:235-238
      fb.c = tb.c;
      fb.r = tb.r + mk3(A.fat_margin, A.fat_margin, A.fat_margin);
      B.fb_c[g] = mk4(fb.c, 0.0f);
      B.fb_r[g] = mk4(fb.r, 0.0f);
      atomicAdd(&s_stat[0], 1u);
    }
    s_tc[i] = mk4(tb.c, 0.0f); s_tr[i] = mk4(tb.r, 0.0f); s_fc[i] = mk4(fb.c, 0.0f); s_fr[i] = mk4(fb.r, 0.0f);
  }
  __syncthreads();
  // the candidates of body i, in the list's order: counted, scanned, listed
  uint2* cand = A.cand + A.q_off[k];
  const BatchTerrain M = batch_terrain_of(A.T, k);
  const V3 mx = mk3(M.x[0], M.x[1], M.x[2]);
  // The world's obstacles: its range of the descriptors and the stores.  Body i's candidates against their components are what
  // Compound::contacts' walk meets per obstacle, in list order (compound.rs:340-346).  The mesh's tree and the obstacles' are walked by
  // one loop - tree 0 the mesh's, tree s the obstacle's at list slot s - 1: one walk's worth of scalar registers, which is all this
  // kernel has.
  const uint32_t ob0 = batch_obst_first(M.obst), nob = batch_obst_count(M.obst);
  BatchObstacles O;
  O.nodes = nullptr; O.comps = nullptr; O.desc = nullptr;
  if (nob) O = batch_obstacles_of(A.T, A.n_worlds);
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    uint32_t npair = 0;
    for (uint32_t i = tid; i < n; i += T) {
      Box q; q.c = xyz(s_tc[i]); q.r = xyz(s_tr[i]);
      uint32_t at = pass ? s_off[i] : 0u;
#pragma unroll 1
      for (uint32_t t = 0; t <= nob; ++t) {
        BatchObstacle D;  // (of a tree: nodes, n_nodes)
        Box qb = q;
        if (t == 0u) {
          D.nodes = M.nodes; D.n_nodes = M.n_nodes;
          qb.c = q.c + -mx;  // Mesh::contacts queries bounds - mesh.x (mesh.rs:121)
        } else {
          D = batch_obstacle_of(O, ob0 + t - 1u);
          if (D.n_nodes) {
            const BatchBody P = batch_load(B, (size_t)g0 + i);
            qb = compound_query_box(D, P.col, P.d);
          }
        }
        const uint32_t w = i | (t << kBatchSlotShift);
        compound_box_walk(D, qb, [&](uint32_t leaf) {  // (batch_terrain_walk's loop)
          if (pass) cand[at] = make_uint2(w, 0x80000000u | leaf);
          ++at;
        });
      }
      const uint32_t at0 = at;
      for (uint32_t j = 0; j < i; ++j) {  // world.rs:256-290, partners ascending
        Box fb; fb.c = xyz(s_fc[j]); fb.r = xyz(s_fr[j]);
        if (!box_overlaps(q, fb)) continue;
        if (pass) cand[at] = make_uint2(i, j);
        ++at;
      }
      npair += at - at0;
      if (!pass) s_off[i] = at;
    }
    if (pass) break;
    if (npair) atomicAdd(&s_stat[1], npair);
    batch_scan(s_off, n, &s_tot);
    if (s_tot > A.q_cap[k]) {
      batch_undo_front(g0, n);
      if (tid == 0) A.need[2 * k] = s_tot;
      return;
    }
  }
  if (tid == 0) {
    uint32_t* st = A.stats + ((size_t)A.tick * A.n_worlds + k) * 8u;
    st[0] = n; st[3] = s_stat[1]; st[4] = s_stat[0]; st[5] = 0u; st[6] = 0u; st[7] = 0u;
    A.q_count[k] = s_tot;
    A.stage[k] = 8u * A.tick + 1u;
  }
}

// The face tests (Mesh::contacts, mesh.rs:115-139), a lane per candidate that is a face, into the candidate's two slots.  (A launch of its
// own: together with the pair tests they need more scalar registers than there are.)
__global__ __launch_bounds__(kBatchBlock) void k_batch_faces(BatchArgs A) {
  __shared__ uint32_t s_ct;
  const uint32_t k = blockIdx.x, T = kBatchBlock, tid = threadIdx.x;
  if (A.done[k] != A.tick || A.stage[k] != 8u * A.tick + 1u || batch_failed(A, k)) return;
  const uint32_t g0 = A.w_off[k], Q = A.q_count[k];
  const Bodies& B = A.B;
  const uint2* cand = A.cand + A.q_off[k];
  uint32_t* ncq = A.ncq + A.q_off[k];
  float4* slot = A.slot + 6 * (size_t)A.q_off[k];
  if (tid == 0) s_ct = 0u;
  __syncthreads();
  {
    const BatchTerrain M = batch_terrain_of(A.T, k);
    const V3 mx = mk3(M.x[0], M.x[1], M.x[2]);
    uint32_t ct = 0;
    for (uint32_t p = tid; p < Q; p += T) {
      const uint2 e = cand[p];
      if (!(e.y & 0x80000000u) || e.x > kBatchBodyMask) continue;
      const BatchBody Pa = batch_load(B, (size_t)g0 + e.x);
      const uint4 fi = M.faces[e.y & 0x7FFFFFFFu];
      const Triangle tri = mkt(xyz(M.verts[fi.x]) + mx, xyz(M.verts[fi.y]) + mx, xyz(M.verts[fi.z]) + mx);  // mesh.rs:122-126
      LocalContact lc[2];
      const int nc = comp_tri_local(Pa.col, Pa.d, tri, mx, lc);
      ncq[p] = (uint32_t)nc;
      ct += (uint32_t)nc;
#pragma unroll
      for (int q = 0; q < 2; ++q) {  // (constant indices: the two contacts stay in registers)
        if (q < nc) {
          float4* o = slot + 6 * (size_t)p + 3 * q;
          o[0] = mk4(lc[q].la, lc[q].g.t); o[1] = mk4(lc[q].lb, 0.0f); o[2] = mk4(lc[q].g.n, 0.0f);
        }
      }
    }
    if (ct) atomicAdd(&s_ct, ct);
  }
  __syncthreads();
  if (tid == 0) {
    A.stats[((size_t)A.tick * A.n_worlds + k) * 8u + 2u] = s_ct;
    A.stage[k] = 8u * A.tick + 2u;
  }
}

// The pair tests, a lane per candidate that is a partner, into the candidate's first slot; in a world with obstacles the candidates
// against a component of one too: Moving<collider>.contacts(&component) through the wrapper of collision.rs:1368-1382 - the component,
// turned about the origin by the entry's rot and moved by its disp, sweeps at -delta against the collider, the result shifted by
// delta * t (k_narrow_obstacles' contacts_dispatch for a sphere or capsule on both sides is comp_mcomp and that shift: one contact at
// most) - and the local points of LocalContacts (collision.rs:1490-1506) with the obstacle in the Mesh's place: the body's side relative
// to its centre at the contact time, the obstacle's relative to its disp.
__global__ __launch_bounds__(kBatchBlock) void k_batch_pairs(BatchArgs A) {
  __shared__ uint32_t s_ct;
  const uint32_t k = blockIdx.x, T = kBatchBlock, tid = threadIdx.x;
  if (A.done[k] != A.tick || A.stage[k] != 8u * A.tick + 2u || batch_failed(A, k)) return;
  const uint32_t g0 = A.w_off[k], M = A.q_count[k];
  const uint32_t obst = A.T.desc[2 * (size_t)k + 1].w, ob0 = batch_obst_first(obst);
  const bool obstacles = batch_obst_count(obst) != 0u;  // (the workgroup's world: uniform)
  BatchObstacles O;
  O.nodes = nullptr; O.comps = nullptr; O.desc = nullptr;
  if (obstacles) O = batch_obstacles_of(A.T, A.n_worlds);
  const Bodies& B = A.B;
  const uint2* cand = A.cand + A.q_off[k];
  uint32_t* ncq = A.ncq + A.q_off[k];
  float4* slot = A.slot + 6 * (size_t)A.q_off[k];
  if (obstacles) {
    if (tid == 0) s_ct = 0u;
    __syncthreads();
  }
  uint32_t ct = 0;
  for (uint32_t p = tid; p < M; p += T) {
    const uint2 e = cand[p];
    if (e.y & 0x80000000u) {
      if (e.x <= kBatchBodyMask) continue;  // a face: k_batch_faces
      const BatchBody Pa = batch_load(B, (size_t)g0 + (e.x & kBatchBodyMask));
      const BatchObstacle D = batch_obstacle_of(O, ob0 + (e.x >> kBatchSlotShift) - 1u);
      const V3 disp = ld3(D.disp);
      Comp shape = comp_rotate_about(to_comp(D.comps[e.y & 0x7FFFFFFFu]), mkq(D.rot[0], mk3(D.rot[1], D.rot[2], D.rot[3])), mk3(0.0f, 0.0f, 0.0f));
      shape.p = shape.p + disp;
      Contact c;
      const bool hit = comp_mcomp(Pa.col, shape, -Pa.d, &c);
      ncq[p] = hit ? 1u : 0u;
      if (hit) {
        const V3 sh = Pa.d * c.t;
        float4* o = slot + 6 * (size_t)p;
        o[0] = mk4((c.a + sh) + -(comp_center(Pa.col) + Pa.d * c.t), c.t); o[1] = mk4((c.b + sh) + -disp, 0.0f); o[2] = mk4(c.n, 0.0f);
        ++ct;
      }
      continue;
    }
    const BatchBody Pa = batch_load(B, (size_t)g0 + e.x), Pb = batch_load(B, (size_t)g0 + e.y);
    LocalContact lc;
    const bool hit = comp_pair_local(Pa.col, Pa.d, Pb.col, Pb.d, &lc);
    ncq[p] = hit ? 1u : 0u;
    if (hit) {
      const V3 nrm = (mk3(0.0f, 0.0f, 0.0f) + lc.g.n) / 1.0f;  // Manifold::from(pruner) of one contact (manifold.rs:135-140)
      float4* o = slot + 6 * (size_t)p;
      o[0] = mk4(lc.la, lc.g.t); o[1] = mk4(lc.lb, 0.0f); o[2] = mk4(nrm, 0.0f);
    }
  }
  if (obstacles) {  // n_terrain_constraints counts the obstacles' contacts too (behind k_batch_faces' count of the faces')
    if (ct) atomicAdd(&s_ct, ct);
    __syncthreads();
    if (tid == 0) A.stats[((size_t)A.tick * A.n_worlds + k) * 8u + 2u] += s_ct;
  }
  if (tid == 0) A.stage[k] = 8u * A.tick + 3u;
}

// The contacts packed, 256 candidates at a time in list order: contact c of the world = constraint c: (la, t), (lb, i), (n, j); an
// obstacle's contact has its list slot + 1 above the ten bits of i (the candidate's first word).
__global__ __launch_bounds__(kBatchBlock) void k_batch_pack(BatchArgs A) {
  __shared__ uint32_t s_wave[kBatchBlock / 64];
  const uint32_t k = blockIdx.x, T = kBatchBlock, tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  if (A.done[k] != A.tick || A.stage[k] != 8u * A.tick + 3u || batch_failed(A, k)) return;
  const uint32_t g0 = A.w_off[k], n = A.w_off[k + 1] - g0, M = A.q_count[k], cap = A.c_cap[k];
  const uint2* cand = A.cand + A.q_off[k];
  const uint32_t* ncq = A.ncq + A.q_off[k];
  const float4* slot = A.slot + 6 * (size_t)A.q_off[k];
  float4* cont = A.cont + 4 * (size_t)A.c_off[k];
  uint32_t carry = 0;
  for (uint32_t p0 = 0; p0 < M; p0 += T) {
    const uint32_t p = p0 + tid;
    const uint32_t nc = p < M ? ncq[p] : 0u;
    uint32_t incl = nc;
    for (int off = 1; off < 64; off <<= 1) { const uint32_t t = __shfl_up(incl, off); if ((int)lane >= off) incl += t; }
    __syncthreads();  // (s_wave of the last trip has been read)
    if (lane == 63) s_wave[wv] = incl;
    __syncthreads();
    uint32_t at = carry + incl - nc;
    for (uint32_t w = 0; w < wv; ++w) at += s_wave[w];
    for (uint32_t w = 0; w < T / 64; ++w) carry += s_wave[w];
    if (nc) {
      const uint2 e = cand[p];
      const uint32_t jb = (e.y & 0x80000000u) ? kNone : e.y;
      for (uint32_t q = 0; q < nc; ++q) {
        if (at + q >= cap) break;
        const float4* in = slot + 6 * (size_t)p + 3 * q;
        float4* o = cont + 4 * (size_t)(at + q);
        const float4 w1 = in[1], w2 = in[2];
        o[0] = in[0]; o[1] = make_float4(w1.x, w1.y, w1.z, u2f(e.x)); o[2] = make_float4(w2.x, w2.y, w2.z, u2f(jb));  // (e.x: the body, and above it the obstacle's slot + 1)
      }
    }
  }
  __syncthreads();
  if (carry > cap) {
    batch_undo(A, g0, n);
    if (tid == 0) A.need[2 * k + 1] = carry;
    return;
  }
  if (tid == 0) {
    uint32_t* st = A.stats + ((size_t)A.tick * A.n_worlds + k) * 8u;
    st[1] = carry;
    A.c_count[k] = carry;
    A.stage[k] = 8u * A.tick + 4u;
  }
}

// ContactConstraint::new a lane per contact.  LDS: three words a body.
__global__ __launch_bounds__(kBatchBlock) void k_batch_setup(BatchArgs A) {
  extern __shared__ float4 s_dyn[];
  const uint32_t k = blockIdx.x, T = kBatchBlock, tid = threadIdx.x;
  if (A.done[k] != A.tick || A.stage[k] != 8u * A.tick + 4u || batch_failed(A, k)) return;
  const uint32_t g0 = A.w_off[k], n = A.w_off[k + 1] - g0, C = A.c_count[k];
  const Bodies& B = A.B;
  uint32_t* s_first = reinterpret_cast<uint32_t*>(s_dyn);
  uint32_t *s_na = s_first + n, *s_degb = s_first + 2 * (size_t)n;
  const float4* cont = A.cont + 4 * (size_t)A.c_off[k];
  CRec* cons = A.cons + A.c_off[k];
  const uint4 tx = A.T.desc[2 * (size_t)k + 1];  // the world's mesh position
  const V3 mx = mk3(u2f(tx.x), u2f(tx.y), u2f(tx.z));
  for (uint32_t i = tid; i < n; i += T) { s_first[i] = kNone; s_na[i] = 0u; s_degb[i] = 0u; }
  __syncthreads();
  for (uint32_t c = tid; c < C; c += T) {
    const uint32_t i = f2u(cont[4 * (size_t)c + 1].w) & kBatchBodyMask, j = f2u(cont[4 * (size_t)c + 2].w);
    atomicMin(&s_first[i], c);
    atomicAdd(&s_na[i], 1u);
    if (j != kNone) atomicAdd(&s_degb[j], 1u);
  }
  __syncthreads();
  for (uint32_t c = tid; c < C; c += T) {
    const float4 w0 = cont[4 * (size_t)c], w1 = cont[4 * (size_t)c + 1], w2 = cont[4 * (size_t)c + 2];
    const uint32_t i = f2u(w1.w) & kBatchBodyMask, os = f2u(w1.w) >> kBatchSlotShift, j = f2u(w2.w);
    const float4 dli = B.bpk[4 * ((size_t)g0 + i) + 1], eii = B.bpk[4 * ((size_t)g0 + i) + 2];
    CRec r;
    if (j == kNone) {  // Static{ center: terrain.center(), friction: 0.0 } world.rs:247; Manifold::from(lc) manifold.rs:120-128
      V3 sc = mx;
      if (os) {  // an obstacle's contact: Shape::center for Compound is its disp (compound.rs:289-291)
        const uint4 od = batch_obstacles_of(A.T, A.n_worlds).desc[3 * (size_t)(batch_obst_first(tx.w) + os - 1u) + 1];
        sc = mk3(u2f(od.x), u2f(od.y), u2f(od.z));
      }
      r = make_constraint(i, kNone, load_dyn(B.srec, g0 + i), xyz(eii), eii.w, dli.w, static_dyn(), sc, 0.0f, 0.0f, xyz(w2), xyz(w0), xyz(w1), A.dt, A.baumgarte,
                          A.slop);
    } else {
      const float4 dlj = B.bpk[4 * ((size_t)g0 + j) + 1], eij = B.bpk[4 * ((size_t)g0 + j) + 2];
      r = make_constraint(i, j, load_dyn(B.srec, g0 + i), xyz(eii), eii.w, dli.w, load_dyn(B.srec, g0 + j), xyz(eij), eij.w, dlj.w, xyz(w2), xyz(w0), xyz(w1), A.dt,
                          A.baumgarte, A.slop);
    }
    r.pad0 = c - s_first[i];  // rank in body i's chain: its own range comes first
    store_crec(&cons[c], r);
  }
  for (uint32_t i = tid; i < n; i += T) { A.na[(size_t)g0 + i] = s_na[i]; A.degb[(size_t)g0 + i] = s_degb[i]; }
  if (tid == 0) A.stage[k] = 8u * A.tick + 5u;
}

// The chains and Solver::solve.  LDS: 64 bytes a body of solver records, four words a body of counts.
__global__ __launch_bounds__(kBatchBlock) void k_batch_solve(BatchArgs A) {
  extern __shared__ float4 s_dyn[];
  __shared__ uint32_t s_tot;
  const uint32_t k = blockIdx.x, T = kBatchBlock, tid = threadIdx.x;
  if (A.done[k] != A.tick || A.stage[k] != 8u * A.tick + 5u || batch_failed(A, k)) return;
  const uint32_t g0 = A.w_off[k], n = A.w_off[k + 1] - g0, C = A.c_count[k];
  float4* srec = A.B.srec + 4 * (size_t)g0;
  uint32_t* s_na = reinterpret_cast<uint32_t*>(s_dyn + 4 * (size_t)n);
  uint32_t *s_degb = s_na + n, *s_boff = s_na + 2 * (size_t)n, *s_cur = s_na + 3 * (size_t)n;
  CRec* cons = A.cons + A.c_off[k];
  uint32_t* rows = A.rows + A.c_off[k];
  // the `b` occurrences of every body in list order, ranks
  for (uint32_t i = tid; i < n; i += T) {
    s_na[i] = A.na[(size_t)g0 + i];
    const uint32_t d = A.degb[(size_t)g0 + i];
    s_degb[i] = d; s_boff[i] = d; s_cur[i] = 0u;
  }
  batch_scan(s_boff, n, &s_tot);
  for (uint32_t c = tid; c < C; c += T) {
    const uint32_t b = cons[c].b;
    if (b != kNone) rows[s_boff[b] + atomicAdd(&s_cur[b], 1u)] = c;
  }
  __syncthreads();
  for (uint32_t x = tid; x < n; x += T) {
    uint32_t* row = rows + s_boff[x];
    const uint32_t nb = s_degb[x], na = s_na[x];
    for (uint32_t a = 1; a < nb; ++a) {  // ascending id = insertion order
      const uint32_t v = row[a];
      uint32_t b = a;
      while (b > 0 && row[b - 1] > v) { row[b] = row[b - 1]; --b; }
      row[b] = v;
    }
    for (uint32_t e = 0; e < nb; ++e) cons[row[e]].round = na + e;  // rank in body x's chain: behind its own range
  }
  __syncthreads();
  for (uint32_t x = tid; x < n; x += T) { s_degb[x] += s_na[x]; s_boff[x] = 0u; }
  const uint32_t* s_deg = s_degb;  // the chain's length
  uint32_t* s_prog = s_boff;       // constraints solved on the body so far, over all iterations
  for (uint32_t e = tid; e < 4u * n; e += T) s_dyn[e] = srec[e];
  __syncthreads();
  {
    uint32_t c = tid, it = 0, spins = 0;
    if (c >= C || A.iters == 0u) c = kNone;
    CRec r;
    uint32_t need_a = 0, need_b = 0;
    if (c != kNone) { r = load_crec_solve(&cons[c]); need_a = r.pad0; need_b = r.round; }
    else { r.a = 0u; r.b = kNone; }
    while (c != kNone) {
      bool ready = __hip_atomic_load(&s_prog[r.a], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == need_a;
      if (ready && r.b != kNone) ready = __hip_atomic_load(&s_prog[r.b], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == need_b;
      if (!__any(ready)) __builtin_amdgcn_s_sleep(1);  // (a wave-wide step of every trip: lanes that wait never hold back lanes of their wave that can run)
      if (ready) {
        BodyDyn Da = load_dyn(s_dyn, r.a);
        BodyDyn Db = r.b == kNone ? static_dyn() : load_dyn(s_dyn, r.b);
        solve_one(r, Da, Db);
        store_vel(s_dyn, r.a, Da);
        if (r.b != kNone) store_vel(s_dyn, r.b, Db);
        __hip_atomic_store(&s_prog[r.a], need_a + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (r.b != kNone) __hip_atomic_store(&s_prog[r.b], need_b + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        cons[c].nimp = r.nimp;
        spins = 0;
        c += T;
        if (c >= C) { c = tid; ++it; }
        if (it >= A.iters) { c = kNone; }
        else {
          r = load_crec_solve(&cons[c]);
          need_a = it * s_deg[r.a] + r.pad0;
          need_b = r.b == kNone ? 0u : it * s_deg[r.b] + r.round;
        }
      } else if (++spins > kBatchSpinLimit) {
        A.err[0] = 1u;
        c = kNone;
      }
    }
  }
  __syncthreads();
  for (uint32_t i = tid; i < n; i += T) { srec[4 * i] = s_dyn[4 * i]; srec[4 * i + 1] = s_dyn[4 * i + 1]; }
  for (uint32_t c = tid; c < C; c += T) { cons[c].pad0 = 0u; cons[c].round = 0u; }  // (the ranks were the tick's own: a record reads as the lone world's)
  if (tid == 0) A.done[k] = A.tick + 1u;
}

// a batch's lists move to larger storage: a workgroup per world
__global__ __launch_bounds__(kBatchBlock) void k_batch_move_lists(const CRec* src, const uint32_t* src_off, CRec* dst, const uint32_t* dst_off, const uint32_t* c_count) {
  const uint32_t k = blockIdx.x;
  const float4* s = reinterpret_cast<const float4*>(src + src_off[k]);
  float4* d = reinterpret_cast<float4*>(dst + dst_off[k]);
  for (uint32_t e = threadIdx.x; e < 8u * c_count[k]; e += kBatchBlock) d[e] = s[e];
}

}  // namespace mgf
