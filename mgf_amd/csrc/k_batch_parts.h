// The tick of a batch that holds bodies of several components (mgf_batch_add_compound_bodies, DESIGN.md "bodies of up to four components").
// (Part of the kernel set described in kernels.h.)
//
// The oracle's World::collide over bodies of 1..4 parts, a workgroup per world as in k_batch.h, seven launches a tick whatever the number of worlds: these
// five take the places of k_batch_front / _faces / _pairs / _pack, and k_batch_setup / k_batch_solve follow them unchanged - they work
// record by record, and a pair's several records are consecutive records of the same two bodies in both bodies' chains.
//   k_batch_parts_front  k_batch_front, and for a body of several parts k_integrate's part loop: the world parts rebuilt from (x, q) and
//                        the local parts, the tight box the union of the parts' swept bounds (the refit rule uses that box), the collider
//                        slot of the packed copy a radius-0 sphere at the centre of mass.  The candidates in the oracle's order with the
//                        part in the first word (body | slot + 1 << 10 | part << 17): the faces the union box meets in mesh-BVH DFS order
//                        and per face the parts in order; the obstacles in list order, per obstacle the parts in order, each with its own
//                        query box; the partners j < i ascending, one candidate a pair of bodies
//   k_batch_parts_faces  a lane per (face, part): <= 2 contacts, the local point of the body's side relative to the body's centre
//   k_batch_parts_obst   a lane per (obstacle component, part) as k_batch_pairs' obstacle branch (a launch of its own: seven a tick)
//   k_batch_parts_pairs  the pairs of bodies 256 candidates at a time in
//                        k_narrow_pairs_parts<4>'s steps - a lane per part pair (parts of i outer) into 16 raw slots of LDS, then a lane per
//                        pair of bodies for ContactPruner::push (manifold.rs:72-102) and Manifold::from(pruner) (:131-148).  What the
//                        pruner keeps (<= 16) goes to a pool of the world - as many entries as its share of the constraint storage, a
//                        run per pair taken with one LDS atomic - and the run's start into the candidate's own slot
//   k_batch_parts_pack   k_batch_pack for up to 16 contacts a candidate: every contact of a manifold a record of its own, with the
//                        manifold's normal, consecutive
// A failed tick puts back the seven undo words a body and nothing of the parts: the world parts are written by the front from (x, q)
// and the local parts before anything reads them, every tick, and nothing reads them between ticks - the rerun rebuilds them from the
// restored pose.
#pragma once
#include "k_batch.h"
#include "k_front_rows.h"

namespace mgf {

constexpr uint32_t kBatchPartShift = 17, kBatchWordMask = (1u << kBatchPartShift) - 1u;  // a candidate's first word below the part: body | slot + 1 << 10
static_assert(kBatchSlotShift + kBatchObstCountBits == kBatchPartShift && kMaxParts <= 4, "ten bits of body, seven of slot, two of part");
constexpr uint32_t kBatchPairSlots = kMaxParts * kMaxParts;  // raw contacts of a pair of bodies; a manifold keeps at most as many
constexpr uint32_t kBatchPairRound = 32;                     // pairs of bodies per round of the pruner (16 raw slots of 48 bytes each: 24 KB)

struct BatchPartsArgs { BatchArgs A; float4* pool; };  // pool: world k's kept pair contacts at 3 * c_off[k], c_cap[k] entries of three words

// a body's constructor word: a body of several parts has kind 2 and its part count in the second word; an ordinary body is its one part
__device__ __forceinline__ uint32_t batch_np(float4 ct) { return f2u(ct.x) == 2u ? f2u(ct.y) : 1u; }
// part k of body g: the world part the front built, or the ordinary body's collider
__device__ __forceinline__ Comp batch_part(const Bodies& B, size_t g, uint32_t k, const Comp& col, bool several) {
  if (!several) return col;
  const float4 a = B.wp0[kMaxParts * g + k], b = B.wp1[kMaxParts * g + k];
  Comp c;
  c.kind = (int)f2u(b.w); c.p = xyz(a); c.r = a.w; c.d = xyz(b);
  return c;
}

// LDS: 64 bytes a body of boxes, one word a body of counts.
__global__ __launch_bounds__(kBatchBlock) void k_batch_parts_front(BatchArgs A) {
  extern __shared__ float4 s_dyn[];
  __shared__ uint32_t s_tot, s_stat[2];
  const uint32_t k = blockIdx.x, T = kBatchBlock, tid = threadIdx.x;
  if (A.done[k] != A.tick) return;
  const uint32_t g0 = A.w_off[k], n = A.w_off[k + 1] - g0;
  const Bodies& B = A.B;
  float4 *s_tc = s_dyn, *s_tr = s_dyn + n, *s_fc = s_dyn + 2 * (size_t)n, *s_fr = s_dyn + 3 * (size_t)n;
  uint32_t* s_off = reinterpret_cast<uint32_t*>(s_dyn + 4 * (size_t)n);
  if (tid < 2) s_stat[tid] = 0u;
  __syncthreads();
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
    Comp col;
    Box tb;
    if (f2u(ct.x) == 2u) {  // a body of several parts (k_integrate): the collider slot carries the centre, the parts collide
      col.kind = KIND_SPHERE; col.p = x; col.d = mk3(0.0f, 0.0f, 0.0f); col.r = 0.0f;
      const uint32_t np = f2u(ct.y);
      for (uint32_t pk = 0; pk < np; ++pk) {
        const float4 l0 = B.lp0[kMaxParts * g + pk], l1 = B.lp1[kMaxParts * g + pk];
        Comp part; part.kind = (int)f2u(l1.w); part.r = l0.w;
        part.p = x + rotate(q, xyz(l0));
        part.d = part.kind == KIND_SPHERE ? mk3(0.0f, 0.0f, 0.0f) : rotate(q, xyz(l1));
        B.wp0[kMaxParts * g + pk] = mk4(part.p, part.r);
        B.wp1[kMaxParts * g + pk] = mk4(part.d, l1.w);
        const Box pb = swept_bounds(part, d);
        tb = pk == 0 ? pb : box_combine(tb, pb);
      }
    } else {
      col = construct((int)f2u(ct.x), ct.y, ct.z, x, q);
      tb = swept_bounds(col, d);
    }
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
  __syncthreads();  // (a body's world parts are read below by the lane that wrote them)
  uint2* cand = A.cand + A.q_off[k];
  const BatchTerrain M = batch_terrain_of(A.T, k);
  const V3 mx = mk3(M.x[0], M.x[1], M.x[2]);
  const uint32_t ob0 = batch_obst_first(M.obst), nob = batch_obst_count(M.obst);
  BatchObstacles O;
  O.nodes = nullptr; O.comps = nullptr; O.desc = nullptr;
  if (nob) O = batch_obstacles_of(A.T, A.n_worlds);
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    uint32_t npair = 0;
    for (uint32_t i = tid; i < n; i += T) {
      const size_t g = (size_t)g0 + i;
      Box q; q.c = xyz(s_tc[i]); q.r = xyz(s_tr[i]);
      uint32_t at = pass ? s_off[i] : 0u;
      const float4 ct = B.ctor[g];
      const uint32_t np = batch_np(ct);
      // tree 0, the mesh's, is walked once with the union box and every leaf lists the parts in order; tree s, the obstacle's at list
      // slot s - 1, once per part with the part's own query box (compound.rs:340-346)
#pragma unroll 1
      for (uint32_t t = 0; t <= nob; ++t) {
        const uint32_t walks = t == 0u ? 1u : np, fan = t == 0u ? np : 1u;
#pragma unroll 1
        for (uint32_t pk = 0; pk < walks; ++pk) {
          BatchObstacle D;  // (of a tree: nodes, n_nodes)
          Box qb = q;
          if (t == 0u) {
            D.nodes = M.nodes; D.n_nodes = M.n_nodes;
            qb.c = q.c + -mx;  // Mesh::contacts queries bounds - mesh.x (mesh.rs:121)
          } else {
            D = batch_obstacle_of(O, ob0 + t - 1u);
            if (D.n_nodes) {
              const BatchBody P = batch_load(B, g);
              qb = compound_query_box(D, batch_part(B, g, pk, P.col, f2u(ct.x) == 2u), P.d);
            }
          }
          const uint32_t w = i | (t << kBatchSlotShift) | (pk << kBatchPartShift);
          compound_box_walk(D, qb, [&](uint32_t leaf) {
            for (uint32_t f = 0; f < fan; ++f) {
              if (pass) cand[at] = make_uint2(w | (f << kBatchPartShift), 0x80000000u | leaf);
              ++at;
            }
          });
        }
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

// k_batch_faces, a lane per (face, part): the part's contacts with the face, the body's side relative to the body's centre.
__global__ __launch_bounds__(kBatchBlock) void k_batch_parts_faces(BatchArgs A) {
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
      if (!(e.y & 0x80000000u) || (e.x & kBatchWordMask) > kBatchBodyMask) continue;
      const size_t g = (size_t)g0 + (e.x & kBatchBodyMask);
      const BatchBody Pa = batch_load(B, g);
      const Comp part = batch_part(B, g, e.x >> kBatchPartShift, Pa.col, f2u(B.ctor[g].x) == 2u);
      const uint4 fi = M.faces[e.y & 0x7FFFFFFFu];
      const Triangle tri = mkt(xyz(M.verts[fi.x]) + mx, xyz(M.verts[fi.y]) + mx, xyz(M.verts[fi.z]) + mx);  // mesh.rs:122-126
      LocalContact lc[2];
      const int nc = comp_tri_local_at(part, Pa.d, tri, mx, comp_center(Pa.col), lc);
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

// The obstacle candidates, a lane each, as k_batch_pairs' with the candidate's part in the collider's place and the body's centre the
// local point's origin.  Between k_batch_parts_faces and k_batch_parts_pairs, whose stage word it leaves alone: beside the part pairs and
// the pruner it needs more scalar registers than there are.  A world without obstacles leaves at once.
__global__ __launch_bounds__(kBatchBlock) void k_batch_parts_obst(BatchArgs A) {
  __shared__ uint32_t s_ct;
  const uint32_t k = blockIdx.x, T = kBatchBlock, tid = threadIdx.x;
  if (A.done[k] != A.tick || A.stage[k] != 8u * A.tick + 2u || batch_failed(A, k)) return;
  const uint32_t obst = A.T.desc[2 * (size_t)k + 1].w, ob0 = batch_obst_first(obst);
  if (batch_obst_count(obst) == 0u) return;  // (the workgroup's world: uniform)
  const uint32_t g0 = A.w_off[k], Q = A.q_count[k];
  const BatchObstacles O = batch_obstacles_of(A.T, A.n_worlds);
  const Bodies& B = A.B;
  const uint2* cand = A.cand + A.q_off[k];
  uint32_t* ncq = A.ncq + A.q_off[k];
  float4* slot = A.slot + 6 * (size_t)A.q_off[k];
  if (tid == 0) s_ct = 0u;
  __syncthreads();
  uint32_t ct = 0;
  for (uint32_t p = tid; p < Q; p += T) {
    const uint2 e = cand[p];
    if (!(e.y & 0x80000000u) || (e.x & kBatchWordMask) <= kBatchBodyMask) continue;  // a pair, a face
    const size_t g = (size_t)g0 + (e.x & kBatchBodyMask);
    const BatchBody Pa = batch_load(B, g);
    const Comp part = batch_part(B, g, e.x >> kBatchPartShift, Pa.col, f2u(B.ctor[g].x) == 2u);
    const BatchObstacle D = batch_obstacle_of(O, ob0 + ((e.x & kBatchWordMask) >> kBatchSlotShift) - 1u);
    const V3 disp = ld3(D.disp);
    Comp shape = comp_rotate_about(to_comp(D.comps[e.y & 0x7FFFFFFFu]), mkq(D.rot[0], mk3(D.rot[1], D.rot[2], D.rot[3])), mk3(0.0f, 0.0f, 0.0f));
    shape.p = shape.p + disp;
    Contact c;
    const bool hit = comp_mcomp(part, shape, -Pa.d, &c);
    ncq[p] = hit ? 1u : 0u;
    if (hit) {
      const V3 sh = Pa.d * c.t;
      float4* o = slot + 6 * (size_t)p;
      o[0] = mk4((c.a + sh) + -(comp_center(Pa.col) + Pa.d * c.t), c.t); o[1] = mk4((c.b + sh) + -disp, 0.0f); o[2] = mk4(c.n, 0.0f);
      ++ct;
    }
  }
  if (ct) atomicAdd(&s_ct, ct);
  __syncthreads();
  if (tid == 0) A.stats[((size_t)A.tick * A.n_worlds + k) * 8u + 2u] += s_ct;  // n_terrain_constraints counts the obstacles' contacts too
}

// The pairs of bodies through k_narrow_pairs_parts<4>'s steps (k_contacts.h), the raw contacts in LDS.
__global__ __launch_bounds__(kBatchBlock) void k_batch_parts_pairs(BatchPartsArgs P) {
  __shared__ NContact s_raw[kBatchPairSlots * kBatchPairRound];
  __shared__ uint32_t s_list[kBatchBlock];
  __shared__ uint32_t s_n, s_pool;
  const BatchArgs& A = P.A;
  const uint32_t k = blockIdx.x, T = kBatchBlock, tid = threadIdx.x;
  if (A.done[k] != A.tick || A.stage[k] != 8u * A.tick + 2u || batch_failed(A, k)) return;
  const uint32_t g0 = A.w_off[k], Q = A.q_count[k];
  const Bodies& B = A.B;
  const uint2* cand = A.cand + A.q_off[k];
  if (tid == 0) s_pool = 0u;
  for (uint32_t p0 = 0; p0 < Q; p0 += T) {  // (whole workgroups walk the loop together: Q is the world's)
    __syncthreads();
    if (tid == 0) s_n = 0u;
    __syncthreads();
    const uint32_t p = p0 + tid;
    bool pair = false;
    if (p < Q) {
      pair = !(cand[p].y & 0x80000000u);  // (a face: k_batch_parts_faces; a component of an obstacle: k_batch_parts_obst)
    }
    {
      const unsigned long long mask = __ballot(pair);
      const uint32_t lane = tid & 63u;
      uint32_t base = 0;
      if (lane == 0u && mask) base = atomicAdd(&s_n, (uint32_t)__popcll(mask));
      base = __shfl(base, 0);
      if (pair) s_list[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = p;
    }
    __syncthreads();
    const uint32_t n_pairs = s_n;
    for (uint32_t r0 = 0; r0 < n_pairs; r0 += kBatchPairRound) {
      const uint32_t here = min(kBatchPairRound, n_pairs - r0);
      // an item per (part pair, pair of bodies), part-pair-major: slot = 4 a + b, parts of i outer -> a.xyz, t | b.xyz, hit | n.xyz
      for (uint32_t w = tid; w < here * kBatchPairSlots; w += T) {
        const uint32_t sl = w / here, idx = w - sl * here, a = sl >> 2, b = sl & 3u;
        const uint2 e = cand[s_list[r0 + idx]];
        const size_t gi = (size_t)g0 + e.x, gj = (size_t)g0 + e.y;
        const float4 cti = B.ctor[gi], ctj = B.ctor[gj];
        NContact raw;
        raw.la = raw.lb = raw.n = make_float4(0, 0, 0, 0);
        if (a < batch_np(cti) && b < batch_np(ctj)) {
          const BatchBody Pi = batch_load(B, gi), Pj = batch_load(B, gj);
          const Comp Pa = batch_part(B, gi, a, Pi.col, f2u(cti.x) == 2u), Pb = batch_part(B, gj, b, Pj.col, f2u(ctj.x) == 2u);
          Contact c;
          if (!comp_pair_far(Pa, Pi.d, Pb, Pj.d) && comp_pair_contact(Pa, Pi.d, Pb, Pj.d, &c)) { raw.la = mk4(c.a, c.t); raw.lb = mk4(c.b, 1.0f); raw.n = mk4(c.n, 0.0f); }
        }
        s_raw[kBatchPairSlots * idx + sl] = raw;
      }
      __syncthreads();
      if (tid < here) {  // ContactPruner::push over the raw contacts in order; what it keeps is a list of slot numbers, four bits each
        // (where the pruner's results go, read afresh from the argument block as batch_undo_front does: held from the top of the kernel
        // they cost eight scalar registers through the part pairs' tests, which have none to spare)
        const volatile BatchPartsArgs* K = (const volatile BatchPartsArgs*)__builtin_amdgcn_kernarg_segment_ptr();
        const uint32_t qo = K->A.q_off[k], co = K->A.c_off[k], cap = K->A.c_cap[k];
        uint32_t* ncq = K->A.ncq + qo;
        float4* slot = K->A.slot + 6 * (size_t)qo;
        float4* pool = K->pool + 3 * (size_t)co;
        const uint32_t pp = s_list[r0 + tid];
        const uint2 e = cand[pp];
        const size_t gi = (size_t)g0 + e.x, gj = (size_t)g0 + e.y;
        const BatchBody Pi = batch_load(B, gi), Pj = batch_load(B, gj);
        PairCentres C;  // (a body's centre: an ordinary body's collider's, the centre of mass of a body of several parts)
        C.ci = comp_center(Pi.col); C.cj = comp_center(Pj.col); C.vA = Pi.d; C.vB = Pj.d;
        const NContact* mine = s_raw + kBatchPairSlots * tid;
        unsigned long long keep = 0ull;
        float min_t = kInf;
        V3 avg = mk3(0.0f, 0.0f, 0.0f);
        const uint32_t cnt = (uint32_t)parts_prune_n<kBatchPairSlots, 4u, unsigned long long>(C, mine, &keep, &min_t, &avg);  // (the lone world's, k_front_rows.h)
        auto kept = [&](uint32_t q) -> uint32_t { return (uint32_t)(keep >> (4u * q)) & 15u; };
        ncq[pp] = cnt;
        if (cnt) {
          const uint32_t at = atomicAdd(&s_pool, cnt);
          slot[6 * (size_t)pp] = make_float4(u2f(at), 0.0f, 0.0f, 0.0f);
          if (at + cnt <= cap) {  // (more than the share holds: the pack counts the list, the tick is undone and run again with more)
            for (uint32_t q = 0; q < cnt; ++q) {
              const LocalContact kc = parts_local(C, mine[kept(q)]);
              float4* o = pool + 3 * (size_t)(at + q);
              o[0] = mk4(kc.la, min_t); o[1] = mk4(kc.lb, 0.0f); o[2] = mk4(avg, 0.0f);
            }
          }
        }
      }
      __syncthreads();
    }
  }
  if (tid == 0) A.stage[k] = 8u * A.tick + 3u;
}

// k_batch_pack for up to 16 contacts a candidate: a face's or an obstacle's from the candidate's slots, a pair's from its run of the pool;
// the first word of a record is the candidate's without the part.
__global__ __launch_bounds__(kBatchBlock) void k_batch_parts_pack(BatchPartsArgs P) {
  __shared__ uint32_t s_wave[kBatchBlock / 64];
  const BatchArgs& A = P.A;
  const uint32_t k = blockIdx.x, T = kBatchBlock, tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  if (A.done[k] != A.tick || A.stage[k] != 8u * A.tick + 3u || batch_failed(A, k)) return;
  const uint32_t g0 = A.w_off[k], n = A.w_off[k + 1] - g0, M = A.q_count[k], cap = A.c_cap[k];
  const uint2* cand = A.cand + A.q_off[k];
  const uint32_t* ncq = A.ncq + A.q_off[k];
  const float4* slot = A.slot + 6 * (size_t)A.q_off[k];
  const float4* pool = P.pool + 3 * (size_t)A.c_off[k];
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
      const bool pair = !(e.y & 0x80000000u);
      const uint32_t jb = pair ? e.y : kNone;
      const uint32_t run = pair ? f2u(slot[6 * (size_t)p].x) : 0u;
      const float4* in = pair ? pool + 3 * (size_t)run : slot + 6 * (size_t)p;
      for (uint32_t q = 0; q < nc; ++q) {
        if (at + q >= cap || run + nc > cap) break;  // (a run beyond the share was not written: the list is too long as well, the tick is undone)
        float4* o = cont + 4 * (size_t)(at + q);
        const float4 w1 = in[3 * q + 1], w2 = in[3 * q + 2];
        o[0] = in[3 * q]; o[1] = make_float4(w1.x, w1.y, w1.z, u2f(e.x & kBatchWordMask)); o[2] = make_float4(w2.x, w2.y, w2.z, u2f(jb));
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

// The part rows of a copied world behind k_batch_drive_copy / k_batch_dev_copy_where (mask: null, or the pairs a device mask selects):
// the local and the world parts, four slots a body each; a source without part storage has ordinary bodies only - empty slots.
struct BatchPartsCopyArgs { Bodies D, S; const uint2* pairs; const uint32_t *d_off, *s_off; const int32_t* mask; uint32_t s_parts; };
__device__ __forceinline__ void batch_parts_copy_row(float4* d, const float4* s, uint32_t words, bool have) {
  for (uint32_t e = threadIdx.x; e < words; e += kBatchBlock) d[e] = have ? s[e] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}
__global__ __launch_bounds__(kBatchBlock) void k_batch_parts_copy(BatchPartsCopyArgs A) {
  if (A.mask && A.mask[blockIdx.x] == 0) return;
  const uint2 pr = A.pairs[blockIdx.x];
  const size_t gd = (size_t)kMaxParts * A.d_off[pr.x], gs = (size_t)kMaxParts * A.s_off[pr.y];
  const uint32_t words = (uint32_t)kMaxParts * min(A.d_off[pr.x + 1] - A.d_off[pr.x], A.s_off[pr.y + 1] - A.s_off[pr.y]);
  const bool have = A.s_parts != 0u;
  batch_parts_copy_row(A.D.lp0 + gd, A.S.lp0 + gs, words, have);
  batch_parts_copy_row(A.D.lp1 + gd, A.S.lp1 + gs, words, have);
  batch_parts_copy_row(A.D.wp0 + gd, A.S.wp0 + gs, words, have);
  batch_parts_copy_row(A.D.wp1 + gd, A.S.wp1 + gs, words, have);
}

}  // namespace mgf
