// Queries against the world between ticks: mgf_world_raycast_many, mgf_world_sweep_many, mgf_world_overlap_aabb_many (k_query.h).
// Part of the single translation unit mgf_hip.hip (included there, in order); not compiled on its own.
//
// Each call builds its own uniform grid over the bodies' CURRENT tight boxes (two synchronisations: the bounds, the cell total).
// The tick's cell grid (cell_lo / cell_cnt, ltb) is not reused: it was laid over the fat boxes before the last integrate moved the
// bodies, and a body of a world with wide bodies is not in it at all.  Nothing of the tick's state is read besides the body store
// and ext_of, and nothing of it is written: sidx_valid, the permutation, the wide-list hysteresis and step_many's guard stay as they are.
// Rays and sweeps are one world_query_run<Q>.  Shared with the batch's front ends (host_batch_query.inc, host_batch_observe.inc):
// query_mask_check, query_tags_check, overlap_offsets, and the timer QueryEvents (host_world.inc) - events kept with the handle.

static mgf_status query_grid(mgf_world* w, QueryGrid* G) {
  mgf_ctx* ctx = w->ctx;
  hipStream_t s = ctx->stream;
  const uint32_t n = w->n_owned;
  MGF_TRY(w->q_misc.ensure(16, s));
  // [0..2] lo, [3..5] hi (ordered ints), [6] large-body count, [7] traversal error, [8] the smallest radius in the grid (ordered int)
  int32_t init[9] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF, (int32_t)0x80000000, (int32_t)0x80000000, (int32_t)0x80000000, 0, 0, 0x7FFFFFFF};
  MGF_TRY(h2d(ctx, w->q_misc.p, reinterpret_cast<const uint32_t*>(init), 9));
  G->rmin = 0.0f;
  G->dims[0] = G->dims[1] = G->dims[2] = 0;
  G->n_large = w->q_misc.p + 6;
  G->start = G->items = nullptr;
  // cell width: the widest fat box the bodies had at rest (every body of such a world spans at most 2 x 2 x 2 cells)
  float h = 2.0f * std::max(w->shape_rmax[0], std::max(w->shape_rmax[1], w->shape_rmax[2]));
  if (!(h > 0.0f) || !std::isfinite(h)) h = 1.0f;
  float margin = 1e-3f * h;
  MGF_TRY(w->q_large.ensure(std::max<uint32_t>(n, 1), s));
  G->large = w->q_large.p;
  w->q_last_large = 0; w->q_last_cells = 0;
  if (n == 0) { G->h = h; G->inv_h = 1.0f / h; G->margin = margin; return MGF_OK; }
  MGF_TRY(w->q_bc.ensure(n, s)); MGF_TRY(w->q_br.ensure(n, s));
  k_query_boxes<<<nblk(n), kBlock, 0, s>>>(w->bodies(), n, h, margin, w->q_bc.p, w->q_br.p, reinterpret_cast<int*>(w->q_misc.p), w->q_large.p,
                                           w->q_misc.p + 6);
  LAUNCH_CHECK();
  int32_t got[9];
  MGF_TRY(d2h(ctx, reinterpret_cast<uint32_t*>(got), w->q_misc.p, 9));
  w->q_last_large = (uint32_t)got[6];
  const uint32_t n_grid = n - (uint32_t)got[6];
  if (n_grid == 0) { G->h = h; G->inv_h = 1.0f / h; G->margin = margin; return MGF_OK; }
  float lo[3], hi[3];
  for (int k = 0; k < 3; ++k) { lo[k] = ord_f(got[k]); hi[k] = ord_f(got[3 + k]); }
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(lo[k]) || !std::isfinite(hi[k])) return fail(MGF_ERR_INVALID, "a body's bounds are not finite: the world cannot be queried");
  // the rounding of a walk grows with the coordinates: the pad follows the scene's magnitude
  const float mag = std::max({std::fabs(lo[0]), std::fabs(lo[1]), std::fabs(lo[2]), std::fabs(hi[0]), std::fabs(hi[1]), std::fabs(hi[2])});
  margin = std::max(margin, 4e-6f * mag);
  const double cap_cells = std::max<double>(4096.0, 2.0 * n_grid);
  int dims[3];
  for (;;) {
    double cells = 1.0;
    for (int k = 0; k < 3; ++k) { dims[k] = (int)std::min(std::floor(((double)hi[k] - (double)lo[k]) / h) + 1.0, 1e9); cells *= dims[k]; }
    if (cells <= cap_cells) break;
    h *= 1.25f;  // (a body that fitted a cell still fits; the large-body list keeps whoever it already holds)
  }
  for (int k = 0; k < 3; ++k) { G->lo[k] = lo[k] - margin; G->dims[k] = dims[k] + 1; }
  G->h = h; G->inv_h = 1.0f / h; G->margin = margin;
  G->rmin = ord_f(got[8]);
  if (!(G->rmin >= 0.0f) || !std::isfinite(G->rmin)) G->rmin = 0.0f;
  const uint32_t cells = (uint32_t)G->dims[0] * (uint32_t)G->dims[1] * (uint32_t)G->dims[2];
  w->q_last_cells = cells;
  MGF_TRY(w->q_cnt.ensure((size_t)cells + 1, s)); MGF_TRY(w->q_start.ensure((size_t)cells + 1, s));
  MGF_HIP_TRY(hipMemsetAsync(w->q_cnt.p, 0, 4 * ((size_t)cells + 1), s));
  k_query_cells<false><<<nblk(n), kBlock, 0, s>>>(*G, n, w->q_bc.p, w->q_br.p, w->q_cnt.p, nullptr);
  LAUNCH_CHECK();
  MGF_TRY(prim_exclusive_scan_u32(ctx, w->q_cnt.p, w->q_start.p, (size_t)cells + 1));
  uint32_t total = 0;
  MGF_TRY(d2h(ctx, &total, w->q_start.p + cells, 1));
  MGF_TRY(w->q_items.ensure(std::max<uint32_t>(total, 1), s));
  G->start = w->q_start.p; G->items = w->q_items.p;
  MGF_HIP_TRY(hipMemsetAsync(w->q_cnt.p, 0, 4 * (size_t)cells, s));
  k_query_cells<true><<<nblk(n), kBlock, 0, s>>>(*G, n, w->q_bc.p, w->q_br.p, w->q_cnt.p, w->q_items.p);
  LAUNCH_CHECK();
  return MGF_OK;
}

// the argument checks every front end of a query shares (host_batch_query.inc, host_batch_observe.inc too)
static mgf_status query_mask_check(int32_t kinds_mask) {
  if (kinds_mask <= 0 || (kinds_mask & ~MGF_QUERY_ALL)) return fail(MGF_ERR_INVALID, "kinds_mask must be a non-empty set of MGF_QUERY_* bits");
  return MGF_OK;
}
static mgf_status query_tags_check(const mgf_moving_component* casts, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (casts[i].shape.tag != 0 && casts[i].shape.tag != 1) return fail(MGF_ERR_INVALID, "a cast's shape tag must be 0 (sphere) or 1 (capsule)");
  return MGF_OK;
}

// events 0 | the grid | 1 | the query pass | 2 (mgf_world_counter "query_build_ns" / "query_run_ns")
static mgf_status query_times(mgf_world* w) {
  MGF_TRY(w->q_tm.wait(2));
  MGF_TRY(w->q_tm.ms(0, 1, &w->q_last_build_ms));
  return w->q_tm.ms(1, 2, &w->q_last_run_ms);
}

// The second half of a box query, the world's and the batch's: the counts to the host, the offsets and *total - the caller's whether
// the lists fit or not - and the two refusals.  *sum: the length of the lists the caller then scans for and fills.
static mgf_status overlap_offsets(mgf_ctx* ctx, const uint32_t* d_cnt, size_t n, uint64_t* out_offsets, int64_t cap, int64_t* total, uint64_t* sum) {
  std::vector<uint32_t> cnt(n);
  MGF_TRY(d2h(ctx, cnt.data(), d_cnt, n));
  *sum = 0;
  for (size_t i = 0; i < n; ++i) { *sum += cnt[i]; out_offsets[i + 1] = *sum; }
  if (total) *total = (int64_t)*sum;
  if ((int64_t)*sum > cap) return fail(MGF_ERR_CAPACITY, "out_bodies too small (*total reports the number required)");
  if (*sum > 0xFFFFFFFFull) return fail(MGF_ERR_CAPACITY, "more than 2^32 - 1 results in one call");
  return MGF_OK;
}

// Q = ParticleIn (d_q = q_parts; k_query_ray, 7 words out) or MovingIn (q_casts; k_query_sweep and k_query_sweep_cells, 13 words out)
template <class Q>
static mgf_status world_query_run(mgf_world* w, DBuf<Q>& d_q, const Q* queries, int64_t n, const int32_t* ignore_body, int32_t kinds_mask, int32_t* out) {
  constexpr bool kRays = std::is_same<Q, ParticleIn>::value;
  constexpr size_t kOut = kRays ? 7 : 13;
  MGF_TRY(ctx_bind(w->ctx));
  if (n == 0) return MGF_OK;
  if (n > (int64_t)INT32_MAX) return fail(MGF_ERR_INVALID, kRays ? "too many particles in one call" : "too many casts in one call");
  mgf_ctx* ctx = w->ctx;
  hipStream_t s = ctx->stream;
  MGF_TRY(d_q.ensure((size_t)n, s));
  MGF_TRY(h2d(ctx, d_q.p, queries, (size_t)n));
  if (ignore_body) { MGF_TRY(w->q_ign.ensure((size_t)n, s)); MGF_TRY(h2d(ctx, w->q_ign.p, ignore_body, (size_t)n)); }
  const int32_t* d_ign = ignore_body ? w->q_ign.p : nullptr;
  MGF_TRY(w->q_hits.ensure(kOut * (size_t)n, s));
  MGF_TRY(w->q_tm.mark(0, s));
  QueryGrid G;
  if (kinds_mask & MGF_QUERY_BODIES) {
    MGF_TRY(query_grid(w, &G));
  } else {  // no cell, no large body
    MGF_TRY(w->q_misc.ensure(16, s));
    MGF_HIP_TRY(hipMemsetAsync(w->q_misc.p, 0, 64, s));
    G.dims[0] = G.dims[1] = G.dims[2] = 0; G.n_large = w->q_misc.p + 6; G.large = nullptr; G.start = G.items = nullptr;
    G.h = G.inv_h = 1.0f; G.margin = 0.0f; G.rmin = 0.0f; G.lo[0] = G.lo[1] = G.lo[2] = 0.0f;
  }
  MGF_TRY(w->q_tm.mark(1, s));
  QueryTargets T;
  T.B = w->bodies(); T.ext = w->ext_ptr(); T.qb_c = w->q_bc.p; T.qb_r = w->q_br.p; T.n = w->n_owned;
  T.err = w->q_misc.p + 7;
  T.M.n_nodes = 0;
  if ((kinds_mask & MGF_QUERY_TERRAIN) && w->terrain) { MGF_TRY(w->terrain->sync()); T.M = w->terrain->dev(T.err); }
  T.obs = w->d_obs.p; T.n_obs = (kinds_mask & MGF_QUERY_OBSTACLES) ? (uint32_t)w->obstacles.size() : 0u;
  if constexpr (kRays) {
    k_query_ray<<<nblk(n), kBlock, 0, s>>>(G, T, d_q.p, n, d_ign, kinds_mask, w->q_hits.p);
    LAUNCH_CHECK();
  } else {
    k_query_sweep<<<nblk(n), kBlock, 0, s>>>(G, T, d_q.p, n, d_ign, kinds_mask, w->q_hits.p);
    LAUNCH_CHECK();
    if ((kinds_mask & MGF_QUERY_BODIES) && G.dims[0] > 0) {
      k_query_sweep_cells<<<nblk(n), kBlock, 0, s>>>(G, T, d_q.p, n, d_ign, w->q_hits.p);
      LAUNCH_CHECK();
    }
  }
  MGF_TRY(w->q_tm.mark(2, s));
  MGF_TRY(d2h(ctx, out, w->q_hits.p, kOut * (size_t)n));
  MGF_TRY(query_times(w));
  uint32_t err = 0;
  MGF_TRY(d2h(ctx, &err, w->q_misc.p + 7, 1));
  if (err) return fail(MGF_ERR_CAPACITY, "BVH traversal stack overflow in a world query");
  return MGF_OK;
}

extern "C" mgf_status mgf_world_raycast_many(mgf_world* w, const mgf_particle* parts, int64_t n, const int32_t* ignore_body, int32_t kinds_mask,
                                             mgf_ray_hit* out) {
  if (!w || n < 0 || (n && (!parts || !out))) return fail(MGF_ERR_INVALID, "NULL argument or negative count");
  MGF_TRY(query_mask_check(kinds_mask));
  static_assert(sizeof(mgf_ray_hit) == 28 && sizeof(mgf_particle) == sizeof(ParticleIn), "k_query_ray writes mgf_ray_hit as seven words");
  return world_query_run(w, w->q_parts, reinterpret_cast<const ParticleIn*>(parts), n, ignore_body, kinds_mask, reinterpret_cast<int32_t*>(out));
}

extern "C" mgf_status mgf_world_sweep_many(mgf_world* w, const mgf_moving_component* casts, int64_t n, const int32_t* ignore_body,
                                           int32_t kinds_mask, mgf_sweep_hit* out) {
  if (!w || n < 0 || (n && (!casts || !out))) return fail(MGF_ERR_INVALID, "NULL argument or negative count");
  MGF_TRY(query_mask_check(kinds_mask));
  static_assert(sizeof(mgf_sweep_hit) == 52 && sizeof(mgf_moving_component) == sizeof(MovingIn), "k_query_sweep writes mgf_sweep_hit as 13 words");
  MGF_TRY(query_tags_check(casts, n));
  return world_query_run(w, w->q_casts, reinterpret_cast<const MovingIn*>(casts), n, ignore_body, kinds_mask, reinterpret_cast<int32_t*>(out));
}

extern "C" mgf_status mgf_world_overlap_aabb_many(mgf_world* w, const mgf_aabb* boxes, int64_t n, uint64_t* out_offsets, uint32_t* out_bodies, int64_t cap,
                                                  int64_t* total) {
  if (!w || n < 0 || (n && !boxes) || !out_offsets || cap < 0 || (cap > 0 && !out_bodies)) return fail(MGF_ERR_INVALID, "NULL argument or negative count");
  MGF_TRY(ctx_bind(w->ctx));
  out_offsets[0] = 0;
  if (total) *total = 0;
  if (n == 0) return MGF_OK;
  if (n > (int64_t)INT32_MAX) return fail(MGF_ERR_INVALID, "too many boxes in one call");
  mgf_ctx* ctx = w->ctx;
  hipStream_t s = ctx->stream;
  MGF_TRY(w->q_boxes.ensure(6 * (size_t)n, s));
  MGF_TRY(h2d(ctx, w->q_boxes.p, reinterpret_cast<const float*>(boxes), 6 * (size_t)n));
  MGF_TRY(w->q_tm.mark(0, s));
  QueryGrid G;
  MGF_TRY(query_grid(w, &G));
  MGF_TRY(w->q_tm.mark(1, s));
  const uint32_t* ext = w->ext_ptr();
  MGF_TRY(w->q_cnt.ensure((size_t)n + 1, s));  // (the grid's counts are dead once its items are filed)
  MGF_TRY(w->q_off.ensure((size_t)n + 1, s));
  k_query_overlap<false><<<nblk(n), kBlock, 0, s>>>(G, ext, w->q_bc.p, w->q_br.p, w->q_boxes.p, n, w->q_cnt.p, nullptr, nullptr);
  LAUNCH_CHECK();
  uint64_t sum = 0;
  MGF_TRY(overlap_offsets(ctx, w->q_cnt.p, (size_t)n, out_offsets, cap, total, &sum));
  MGF_TRY(prim_exclusive_scan_u32(ctx, w->q_cnt.p, w->q_off.p, (size_t)n + 1));
  if (sum) {
    MGF_TRY(w->q_vals.ensure((size_t)sum, s));
    k_query_overlap<true><<<nblk(n), kBlock, 0, s>>>(G, ext, w->q_bc.p, w->q_br.p, w->q_boxes.p, n, nullptr, w->q_off.p, w->q_vals.p);
    LAUNCH_CHECK();
    k_query_sort<<<nblk(n), kBlock, 0, s>>>(w->q_off.p, n, w->q_vals.p);
    LAUNCH_CHECK();
  }
  MGF_TRY(w->q_tm.mark(2, s));
  if (sum) MGF_TRY(d2h(ctx, out_bodies, w->q_vals.p, (size_t)sum));
  return query_times(w);
}
