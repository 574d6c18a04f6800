// The collide phase of the tick: broadphase, narrowphase, constraint setup, links (enqueue + finish).
// Part of the single translation unit mgf_hip.hip (included there, in order); not compiled on its own.
// ---- the tick ----------------------------------------------------------------------------------
// which kernel lists a body's terrain faces: none, one lane per body walking the mesh's tree, or the face grid
enum TerrainPlan { kTerrainNone, kTerrainRows, kTerrainGrid };
static TerrainPlan terrain_plan(const mgf_world* w, bool two_pass) {
  if (two_pass || !w->terrain || w->terrain->m.tree.empty() || !w->n_owned) return kTerrainNone;
  // (a world with obstacles appends their components to the rows behind the faces: the rows then keep the faces in the mesh's own order -
  // the face grid's rows are sorted afterwards)
  return (w->terrain->grid.ready && !w->terrain_grid_off && !w->opt.terrain_tree && w->obstacles.empty()) ? kTerrainGrid : kTerrainRows;
}
static mgf_status world_integrate(mgf_world* w, float dt, bool complete, bool integrate, bool with_bounds, bool with_terrain_rows = false) {
  mgf_ctx* ctx = w->ctx;
  w->invalidate_tick_caches();
  if (w->n_owned == 0) return MGF_OK;
  SceneBounds* sb = with_bounds ? w->sb.p : nullptr;
  const uint32_t* guard = with_bounds ? w->word(kWSkipGuard) : nullptr;
  // the one-synchronisation tick: every body of the world is integrated here, so the scene bounds are gathered on the way
  int* sb_part = (with_terrain_rows && integrate && with_bounds && !w->opt.no_fused_scene_bounds) ? w->sb_part.p : nullptr;
  w->bounds_cover = sb_part ? w->n_owned : 0u;
  MGF_TRY(w->bpk.ensure(4 * (size_t)std::max(w->n, w->n_owned), ctx->stream));
  w->pack_cover = integrate ? w->n_owned : 0u;  // (k_integrate writes every owned body's record)
  // the fused tick, its clearing launch ahead of this one (cell counters zero, the grid's level chosen) and last tick's bounds at hand:
  // the bodies' Morton cells and ranks on the way (CellSort; k_morton_count's launch less)
  CellSort cs;
  memset(&cs, 0, sizeof(cs));
  if (sb_part && w->plan.zero_launched && w->plan.n == w->n_owned && w->sbg_valid && w->opt.cells_in_integrate) {  // (sb_part: the bounds are gathered here too - what collide_enqueue's cells_done asks for)
    cs.grid = w->sb_grid.p; cs.shift = kMortonBits - 2 * (int)w->plan.levels; cs.min_frac = (float)w->opt.grid_min_frac_pct * 0.01f;
    cs.cell_of = w->cell_of.p; cs.rank = w->cell_rank.p; cs.cell_cnt = w->cell_cnt.p;
    w->cells_cover = w->n_owned; w->cells_levels = w->plan.levels;
  }
  WideSpec wd;
  memset(&wd, 0, sizeof(wd));
  w->wide_tick_on = false;
  if (sb_part && integrate && w->opt.wide_list && w->wide_engaged && w->wide_limit[0] > 0.0f) {
    MGF_TRY(w->wide_list.ensure(2 * (size_t)kWideCap, ctx->stream));
    for (int k = 0; k < 3; ++k) wd.limit[k] = w->wide_limit[k];
    wd.list = w->wide_list.p; wd.count = &w->sb.p->pad; wd.ext = w->ext_ptr();
    w->wide_tick_on = true;
  }
  if (with_terrain_rows && integrate && terrain_plan(w, w->opt.two_pass != 0) == kTerrainRows && !w->opt.no_fused_terrain_rows) {
    // the one-synchronisation tick: collide follows at once on the same bodies, so the rows are written here
    MGF_TRY(w->rows_t.ensure((size_t)w->n_owned * w->row_cap_t, ctx->stream));
    MGF_TRY(w->t_cnt.ensure((size_t)w->n_owned + 1, ctx->stream));
    MGF_TRY(w->near_list.ensure(3 * (size_t)w->n_owned, ctx->stream)); MGF_TRY(w->cs_sums.ensure(3 * kCsSumStride, ctx->stream));
    TerrainRowsTail tail{w->terrain->dev(w->word(kWStackOverflow)), w->row_cap_t, w->rows_t.p, w->t_cnt.p, w->word(kWRowOverflow), w->opt.fused_contacts ? w->near_list.p : nullptr, w->cs_sums.p + 2 * kCsSumStride};
    k_integrate<<<nblk(w->n_owned), kBlock, 0, ctx->stream>>>(w->bodies(), w->n_owned, dt, w->params.fat_margin, complete ? 1 : 0, 1, sb, guard, tail, sb_part, cs, wd);
    w->terrain_rows_done = true;
  } else {
    k_integrate<<<nblk(w->n_owned), kBlock, 0, ctx->stream>>>(w->bodies(), w->n_owned, dt, w->params.fat_margin, complete ? 1 : 0, integrate ? 1 : 0,
                                                        sb, guard, NoTail(), sb_part, cs, wd);
  }
  LAUNCH_CHECK();
  return MGF_OK;
}
extern "C" mgf_status mgf_world_complete_motion(mgf_world* w) {
  if (!w) return fail(MGF_ERR_INVALID, "world is NULL");
  MGF_TRY(ctx_bind(w->ctx));
  MGF_TRY(world_integrate(w, 0.0f, true, false, false));
  MGF_HIP_TRY(hipStreamSynchronize(w->ctx->stream));
  return MGF_OK;
}
extern "C" mgf_status mgf_world_integrate(mgf_world* w, float dt) {
  if (!w) return fail(MGF_ERR_INVALID, "world is NULL");
  MGF_TRY(ctx_bind(w->ctx));
  MGF_TRY(world_integrate(w, dt, false, true, false));
  MGF_HIP_TRY(hipStreamSynchronize(w->ctx->stream));
  return MGF_OK;
}

// the narrowphase over a candidate list (`work`: a sub-list by shape-pair type, or null for the whole list), for shapes ka (and kb): 0 sphere, 1 capsule
static mgf_status launch_pairs(mgf_world* w, const Bodies& B, int ka, int kb, const uint32_t* work, const uint32_t* m_ptr, uint32_t cap) {
  if (cap == 0) return MGF_OK;
  static const decltype(&k_narrow_pairs<0, 0>) kern[4] = {k_narrow_pairs<0, 0>, k_narrow_pairs<0, 1>, k_narrow_pairs<1, 0>, k_narrow_pairs<1, 1>};
  kern[2 * ka + kb]<<<nblk(cap), kBlock, 0, w->ctx->stream>>>(B, work, m_ptr, w->p_owner.p, w->p_cand.p, w->p_nc.p, w->p_out.p);
  LAUNCH_CHECK();
  return MGF_OK;
}
static mgf_status launch_terrain(mgf_world* w, const Bodies& B, int ka, const TerrainDev& M, const uint32_t* work, const uint32_t* m_ptr, uint32_t cap) {
  if (cap == 0) return MGF_OK;
  const auto kern = ka == 0 ? k_narrow_terrain<0> : k_narrow_terrain<1>;
  kern<<<nblk(cap), kBlock, 0, w->ctx->stream>>>(B, M, work, m_ptr, w->t_owner.p, w->t_cand.p, w->t_nc.p, w->t_out.p);
  LAUNCH_CHECK();
  return MGF_OK;
}

// Dependency links of the insertion-ordered list cons_nat[0..C) (ConsLinks).
static mgf_status links_ensure(mgf_world* w, uint32_t cap_c, bool zero = false) {
  hipStream_t s = w->ctx->stream;
  uint32_t n = w->n;
  MGF_TRY(w->c_ab.ensure(std::max(cap_c, 1u), s)); MGF_TRY(w->c_succ.ensure(std::max(cap_c, 1u), s)); MGF_TRY(w->c_pred.ensure(2 * (size_t)std::max(cap_c, 1u), s));
  MGF_TRY(w->deg.ensure(n + 1, s)); MGF_TRY(w->adj_off.ensure(n + 1, s)); MGF_TRY(w->adj_fill.ensure(n + 1, s));
  MGF_TRY(w->adj_list.ensure(2 * (size_t)std::max(cap_c, 1u), s));
  if (zero) {
    MGF_HIP_TRY(hipMemsetAsync(w->deg.p, 0, (n + 1) * 4, s));
    MGF_HIP_TRY(hipMemsetAsync(w->adj_fill.p, 0, (n + 1) * 4, s));
  }
  return MGF_OK;
}
// c_ab and deg are filled (by the setup kernels, or k_links_from_records): sorted per-body adjacency, successor
// words, predecessor flags.  C is read on the device (sc->C); grids and buffers are sized by `cap_c`.
static mgf_status build_dag(mgf_world* w, uint32_t cap_c) {
  mgf_ctx* ctx = w->ctx;
  hipStream_t s = ctx->stream;
  uint32_t n = w->n;
  w->depth = 0;
  if (cap_c == 0) return MGF_OK;
  if (cap_c >= kSuccId) return fail(MGF_ERR_CAPACITY, "too many constraints");
  MGF_TRY(prim_exclusive_scan_u32(ctx, w->deg.p, w->adj_off.p, (size_t)n + 1));
  k_adj_fill<<<nblk(cap_c), kBlock, 0, s>>>(w->c_ab.p, &w->sc.p->C, w->adj_off.p, w->adj_fill.p, w->adj_list.p);
  LAUNCH_CHECK();
  k_chain<<<nblk(n), kBlock, 0, s>>>(n, w->links(), w->adj_off.p, w->adj_list.p);
  LAUNCH_CHECK();
  return MGF_OK;
}

// ---- constraint order "demo" (world.rs:233-291 replayed on the host; see WorldOptions::constraint_order) ----
constexpr uint32_t kDemoMaxBodies = 1u << 20;
// Bodies the tree has not seen yet are inserted with their fat AABB as World::add_body does (world.rs:178-184), in body order.
// Must run BEFORE the tick's integrate: that kernel already applies the tick's refits to the device's fat boxes.
static mgf_status demo_sync_tree(mgf_world* w) {
  const size_t have = w->demo_leaf.size(), n = w->n_owned;
  if (have >= n) return MGF_OK;
  if (n > kDemoMaxBodies) return fail(MGF_ERR_INVALID, "constraint_order = demo replays world.rs on the host: at most 1048576 bodies");
  std::vector<float4> c(n - have), r(n - have);
  MGF_TRY(d2h(w->ctx, c.data(), w->fb_c.p + have, n - have));
  MGF_TRY(d2h(w->ctx, r.data(), w->fb_r.p + have, n - have));
  for (size_t i = have; i < n; ++i) {
    Box b; b.c = mk3(c[i - have].x, c[i - have].y, c[i - have].z); b.r = mk3(r[i - have].x, r[i - have].y, r[i - have].z);
    w->demo_leaf.push_back(w->demo_tree.insert(b, i));
  }
  return MGF_OK;
}
// After integrate: the loop of world.rs:233-291 over the bodies - refit in place of the device's broadphase, partners j < i in
// the order BVH::query reports them.  The rows go where k_pair_grid would have put them.
static mgf_status demo_rows(mgf_world* w) {
  mgf_ctx* ctx = w->ctx;
  hipStream_t s = ctx->stream;
  const size_t n = w->n_owned;
  if (w->n != w->n_owned) return fail(MGF_ERR_INVALID, "constraint_order = demo does not combine with ghost bodies (tiles)");
  MGF_HIP_TRY(hipStreamSynchronize(s));
  std::vector<float4> tc(n), tr(n);
  MGF_TRY(d2h(ctx, tc.data(), w->tb_c.p, n));
  MGF_TRY(d2h(ctx, tr.data(), w->tb_r.p, n));
  std::vector<uint32_t> rows(n * (size_t)kRowCap, 0u), cnt(n + 1, 0u);
  const V3 fm = mk3(w->params.fat_margin, w->params.fat_margin, w->params.fat_margin);
  uint64_t cand = 0;
  bool overflow = false;
  for (size_t i = 0; i < n; ++i) {
    Box b; b.c = mk3(tc[i].x, tc[i].y, tc[i].z); b.r = mk3(tr[i].x, tr[i].y, tr[i].z);
    if (!box_contains(w->demo_tree.node(w->demo_leaf[i]).box, b)) {  // world.rs:235-238
      w->demo_tree.remove(w->demo_leaf[i]);
      Box fat = b; fat.r = b.r + fm;                                   // AABB + f32, bounds.rs:91-98
      w->demo_leaf[i] = w->demo_tree.insert(fat, i);
    }
    uint32_t k = 0;
    w->demo_tree.query(b, [&](uint64_t j) {                            // world.rs:265-267: only partners j < i
      if (j >= i) return;
      if (k < (uint32_t)kRowCap) rows[i * (size_t)kRowCap + k] = (uint32_t)j; else overflow = true;
      ++k;
    });
    cnt[i] = k;
    cand += k;
  }
  if (overflow) return fail(MGF_ERR_CAPACITY, "constraint_order = demo: a body has more broadphase partners than a candidate row holds");
  MGF_TRY(w->rows.ensure(std::max<size_t>(n, 1) * kRowCap, s)); MGF_TRY(w->p_cnt.ensure(n + 1, s));
  MGF_TRY(h2d(ctx, w->rows.p, rows.data(), rows.size()));
  MGF_TRY(h2d(ctx, w->p_cnt.p, cnt.data(), cnt.size()));
  w->demo_rows_ready = true;
  w->demo_candidates = cand;
  return MGF_OK;
}

// First half of the tick: drop last tick's ghosts, complete_motion + integrate the owned bodies
// (world.rs:230-231).  After this call a tiled driver may import ghost bodies.
static mgf_status collide_prepare(mgf_world* w, bool solver_follows, bool early, bool speculative);
// (what k_reset_step needs of a world whose tick is about to begin: a driver of several worlds resets them all in one launch, k_reset_step_batch,
// and tells world_begin so)
static mgf_status world_reset_args(mgf_world* w, ResetOne* R) {
  hipStream_t s = w->ctx->stream;
  MGF_TRY(w->sb_part.ensure((size_t)kBoundSlots * kBoundSlotInts, s));
  MGF_TRY(w->cs_sums.ensure(3 * kCsSumStride, s));
  R->sb = w->sb.p; R->err = w->word(kWStackOverflow); R->guard = w->word(kWSkipGuard); R->prev_fail = &w->sc.p->fail; R->sb_part = w->sb_part.p; R->near_cnt = w->cs_sums.p + 2 * kCsSumStride;
  return MGF_OK;
}
static mgf_status world_begin(mgf_world* w, float dt, bool speculative = false, bool collide_follows = false, bool allow_resort = false, bool solver_follows = false,
                              bool reset_launched = false) {
  if (!w) return fail(MGF_ERR_INVALID, "world is NULL");
  MGF_TRY(ctx_bind(w->ctx));
  hipStream_t s = w->ctx->stream;
  w->n = w->n_owned;
  MGF_TRY(maybe_resort(w, allow_resort));  // the store into cell order, if this tick is due (host_perm.inc): ahead of everything that names a slot
  w->demo_rows_ready = false;
  if (w->opt.constraint_order == 1) MGF_TRY(demo_sync_tree(w));
  memset(&w->stats, 0, sizeof(w->stats));
  w->n = w->n_owned;
  w->stats.n_bodies = w->n_owned;
  w->last_dt = dt;
  w->constraints_ready = false;
  w->tick_two_pass = false;
  w->tick_mode1 = false;
  if (w->C) w->prev_C = w->C;
  w->C = w->Ct = w->Mt = w->Mp = 0;
  MGF_TRY(phase_mark(w, 0, s));
  MGF_TRY(w->sb_part.ensure((size_t)kBoundSlots * kBoundSlotInts, s));
  w->plan.zero_launched = false;
  if (allow_resort && w->n_owned > 0 && !w->opt.two_pass) {  // the fused tick: one clearing launch for the whole tick, ahead of k_integrate
    MGF_TRY(collide_prepare(w, solver_follows, true, speculative));
  } else if (!reset_launched) {
    MGF_TRY(w->cs_sums.ensure(3 * kCsSumStride, s));
    k_reset_step<<<1, 64, 0, s>>>(w->sb.p, w->word(kWStackOverflow), w->word(kWSkipGuard), &w->sc.p->fail, speculative ? 1 : 0, w->sb_part.p, w->cs_sums.p + 2 * kCsSumStride);
    LAUNCH_CHECK();
  }
  MGF_TRY(world_integrate(w, dt, true, true, true, collide_follows));
  return MGF_OK;
}
extern "C" mgf_status mgf_world_begin_tick(mgf_world* w, float dt) {
  MGF_TRY(world_begin(w, dt, false, true));  // (ghosts imported before the collide phase join the gathered scene bounds)
  return sync_unless_ordered(w);
}

// Second half: broadphase, narrowphase, ContactConstraint::new over owned + ghost bodies.  Enqueue only:
// nothing is read back, list sizes stay on the device (StepCounts), buffers and grids use the
// capacities cap_t / cap_p / cap_c.
static mgf_status flow5_plan(mgf_world* w, uint32_t cap_c, bool* ok);
static void flow5_zero_entries(mgf_world* w, uint32_t cap_c, ZeroList& z, int first);
static mgf_status flow6_plan(mgf_world* w, uint32_t cap_c, uint32_t iters, bool* ok);
static mgf_status flow6_build_tables(mgf_world* w, uint32_t cap_c, bool* built);
static mgf_status chain_rows_launch(mgf_world* w, const uint32_t* only_if);
static void flow6_zero_entries(mgf_world* w, uint32_t cap_c, ZeroList& z, int first);
static Flow6 flow6_args(mgf_world* w);
// One of the tick's three prefix sums (job 0: cells, 1: candidate rows, 2: constraints per body) by the hand-written single-pass
// k_scan; its status words were cleared by this collide phase's k_zero_many.
static mgf_status tick_scan(mgf_world* w, int job, const uint32_t* a, uint32_t* oa, const uint32_t* b, uint32_t* ob, size_t n_plus_1,
                            const ScanEpilogue* epi = nullptr, const uint32_t* add = nullptr, const int* fold_sb_part = nullptr) {
  ScanJob J;
  memset(&J.epi, 0, sizeof(J.epi));
  if (epi) J.epi = *epi;
  J.add = add;
  J.sb_part = fold_sb_part; J.sb_out = w->sb.p;
  J.in[0] = a; J.out[0] = oa; J.in[1] = b; J.out[1] = ob; J.n = (uint32_t)n_plus_1;
  uint32_t* base = w->scan_ws.p + (size_t)job * (2 * (size_t)w->scan_tiles + 2);
  J.status = reinterpret_cast<unsigned long long*>(base); J.ticket = base + 2 * (size_t)w->scan_tiles;
  const uint32_t tiles = (uint32_t)((n_plus_1 + kScanTile - 1) / kScanTile);
  if (tiles > w->scan_tiles) return fail(MGF_ERR_CAPACITY, "internal: scan workspace too small");
  if (b) k_scan<2><<<tiles, kScanBlock, 0, w->ctx->stream>>>(J);
  else k_scan<1><<<tiles, kScanBlock, 0, w->ctx->stream>>>(J);
  LAUNCH_CHECK();
  return MGF_OK;
}
// scan_ws: per k_scan job 2 * scan_tiles status words (64 bits each) + its ticket (2 words); behind the three jobs the numbering's own
// (option scan_fused, bit 1): room for a status word per 256 bodies and one more - nblk(n) + 1; a run is kNumSubs x 256 bodies - and its ticket
static size_t scan_ws_num_at(const mgf_world* w) { return 3 * (2 * (size_t)w->scan_tiles + 2); }
static size_t scan_ws_words(const mgf_world* w) { return scan_ws_num_at(w) + 2 * ((size_t)nblk(w->n) + 1) + 2; }
// The collide phase's buffers, the cell grid's level and the clearing launch.  `early` (the fused tick, from world_begin): the
// clearing launch is k_tick_clear - it also does k_reset_step's work and runs AHEAD of k_integrate; the collide phase that follows
// on the same bodies finds `plan.zero_launched` and does not clear again (a re-run of the phase inside the tick does).
static bool mixed_world(const mgf_world* w) { return (w->has_sphere && w->has_capsule) || w->has_compound; }
static mgf_status collide_prepare(mgf_world* w, bool solver_follows, bool early, bool speculative) {
  mgf_ctx* ctx = w->ctx;
  hipStream_t s = ctx->stream;
  const uint32_t n = w->n;
  // first tick: room for a few candidates per body; later ticks: last tick's sizes plus slack (collide_finish)
  if (w->cap_p == 0) { w->cap_p = std::max(4 * n, 1024u); w->cap_t = std::max(2 * n, 1024u); w->cap_c = std::max(4 * n, 1024u); }
  const uint32_t cap_p = w->cap_p, cap_c = w->cap_c;
  if (cap_p >= (1u << 27)) return fail(MGF_ERR_CAPACITY, "too many broadphase partners (k_count_contacts keeps a list position in 27 bits)");
  // 2. linear BVH over the fat AABBs
  // 4^levels Morton cells, between one and two bodies per cell on average (option "cell_fill": bodies per cell, in eighths,
  // beyond which the grid gets another level).  A level quarters the cells: a tile whose few thousand ghosts push it just
  // past 4^9 bodies would otherwise enumerate four times the cells per query (measured: 0.19 vs 0.11 ms broadphase).
  uint32_t levels = 4;
  // (cells that the scene covers: a capsule field four times as long as it is high and wide fills a quarter of its grid, and at
  // "two bodies per cell" really had eight - config 3's pair search 0.168 -> 0.142 ms with the level this adds)
  // (r06: a world with capsules gets cells half as full - a capsule's box is a cube of its length whatever way it points (bounds.rs:179-188), a
  // query accepts a few partners of the many its region holds, and where such a world piles up the cells of the rule above hold a dozen
  // bodies each: config 3's pair search 117 -> 101 us)
  const uint64_t cell_fill = (w->has_capsule && !w->has_compound && !w->opt.cell_fill_set) ? std::min<uint64_t>((uint64_t)w->opt.cell_fill, 8u) : (uint64_t)w->opt.cell_fill;
  while ((double)(cell_fill << (2 * levels)) * (double)w->grid_occupancy < 8.0 * (double)n && levels < (uint32_t)kMortonBits / 2) ++levels;
  const uint32_t cells = 1u << (2 * levels), nblocks = cells / kBlock;
  MGF_TRY(w->cell_of.ensure(n, s)); MGF_TRY(w->cell_rank.ensure(n, s)); MGF_TRY(w->sidx.ensure(n, s)); MGF_TRY(w->brank.ensure(n, s));
  w->list_generic = false;
  w->flow5_ok = true; w->flow5_prepped = false; w->flow6_prepped = false; w->f6_fail_known = false; w->canon_ready = false;
  w->scan_tiles = (uint32_t)(((size_t)std::max(cells, n) + 1 + kScanTile - 1) / kScanTile) + 1;
  MGF_TRY(w->scan_ws.ensure(scan_ws_words(w), s));
  MGF_TRY(w->cs_sums.ensure(3 * kCsSumStride, s)); MGF_TRY(w->tcn.ensure(n + 1, s)); MGF_TRY(w->front_cnt.ensure(2 * kTnRegions * kTnCntStride, s));
  MGF_TRY(w->lnodes.ensure(qlevel_offset(levels), s)); MGF_TRY(w->leaves.ensure(n, s));
  MGF_TRY(w->cell_lo.ensure((size_t)cells + 1, s)); MGF_TRY(w->cell_cnt.ensure((size_t)cells + 1, s));
  MGF_TRY(w->sub_lo.ensure(nblocks, s)); MGF_TRY(w->sub_hi.ensure(nblocks, s));
  MGF_TRY(w->sub2_lo.ensure(nblocks / 4 + 1, s)); MGF_TRY(w->sub2_hi.ensure(nblocks / 4 + 1, s));
  const bool rows_done = !early && w->terrain_rows_done;  // this tick's k_integrate listed the owned bodies' terrain faces (ghosts have none)
  MGF_TRY(w->t_cnt.ensure(n + 1, s, rows_done, w->n_owned)); MGF_TRY(w->p_cnt.ensure(n + 1, s));  // (k_integrate may have written the owned bodies' terrain counts)
  MGF_TRY(w->t_off.ensure(n + 1, s)); MGF_TRY(w->p_off.ensure(n + 1, s));
  MGF_TRY(w->cons_nat.ensure(cap_c, s));
  MGF_TRY(links_ensure(w, cap_c));
  MGF_TRY(w->degb.ensure(n + 1, s)); MGF_TRY(w->rev.ensure((size_t)n * w->rev_cap, s));
  const bool bounds_done = !early && w->bounds_cover == n && n > 0;  // ... and gathered the scene bounds (with k_import_ghosts): folded by the clearing launch below
  w->plan.levels = levels; w->plan.cells = cells; w->plan.n = n; w->plan.cap_c = cap_c; w->plan.solver_follows = solver_follows;
  {  // one launch clears every per-tick counter array
    ZeroList z;
    memset(&z, 0, sizeof(z));
    z.p[0] = w->cell_cnt.p; z.words[0] = cells + 1;
    z.p[1] = w->t_cnt.p; z.words[1] = n + 1;  // ghosts have no terrain row
    if (rows_done) { z.p[1] = w->t_cnt.p + w->n_owned; z.words[1] = n - w->n_owned + 1; }  // k_integrate wrote the owned bodies' counts
    z.p[2] = w->degb.p; z.words[2] = n + 1;
    z.p[3] = w->word(kWRevRowOverflow); z.words[3] = 1;  // row-of-b-occurrences overflow flag
    z.p[4] = w->word(kWRowOverflow); z.words[4] = rows_done ? 0 : 1;  // row-overflow flag (re-armed for a re-run inside the tick; k_reset_step cleared it)
    z.p[5] = w->word(kWGridWide); z.words[5] = 1;  // grid-too-wide flag
    z.p[6] = w->word(kWTerrainWide); z.words[6] = 1;  // terrain-grid-too-wide flag
    z.p[7] = w->pair_stat.p; z.words[7] = kPairStatWords;
    z.p[16] = w->word(kWBrickSlow); z.words[16] = 1;  // queries k_pair_brick answered from global memory
    z.p[17] = w->scan_ws.p; z.words[17] = (uint32_t)scan_ws_words(w);  // the three scans' status words and tickets, and the numbering's (k_contacts_rows_index_scan)
    z.p[18] = w->cs_sums.p; z.words[18] = ((early || !rows_done) ? 3 : 2) * kCsSumStride;  // k_terrain_contacts' two counters (and the length of the near list, unless this tick's k_integrate's tail has built it already)
    z.p[20] = w->front_cnt.p; z.words[20] = 2 * kTnRegions * kTnCntStride;                          // k_terrain_near's slot counters and partial counts
    z.p[21] = w->word(kWBigPartsOverflow); z.words[21] = 1;  // k_narrow_pairs_big: a pair of bodies of many parts with more contacts than its lists hold
    z.p[19] = w->tcn.p; z.words[19] = n + 1;                                   // terrain constraints per body: k_terrain_contacts writes the bodies near the mesh only
    w->flow5_zeroed = false; w->flow6_zeroed = false;
    if (solver_follows && w->opt.solver_mode == 6) {  // the same for the solver with message channels
      bool ok = false;
      MGF_TRY(flow6_plan(w, cap_c, w->f6_prep_iters ? w->f6_prep_iters : 10u, &ok));
      if (ok) { flow6_zero_entries(w, cap_c, z, 8); w->flow6_zeroed = true; }
    }
    if (solver_follows && w->opt.solver_mode == 5) {  // the block-local solver's preparation counters ride along
      bool ok = false;
      MGF_TRY(flow5_plan(w, cap_c, &ok));
      if (ok) { flow5_zero_entries(w, cap_c, z, 8); w->flow5_zeroed = true; }
    }
    if (early) {
      k_tick_clear<<<256, kBlock, 0, s>>>(z, w->sb.p, w->word(kWStackOverflow), w->word(kWSkipGuard), &w->sc.p->fail, speculative ? 1 : 0, w->sb_part.p);
      w->plan.zero_launched = true;
    } else {
      if (bounds_done) { z.sb = w->sb.p; z.sb_part = w->sb_part.p; }
      k_zero_many<<<256, kBlock, 0, s>>>(z);
      w->plan.zero_launched = false;
    }
    LAUNCH_CHECK();
  }
  return MGF_OK;
}
// Every decision the collide phase takes about its path, and what its kernels take of the world under them.  collide_plan makes them all, once
// per enqueue, from the world as this tick's k_integrate left it (the conditions and their reasons are written there, nowhere else); the stages
// below only read them.  (The tick slot's brick / fused / front_rows / ... marks are copies.)
struct CollidePlan {
  bool cleared, bounds_done, rows_done, pack_ok, cells_done;                 // what was done ahead of the phase
  bool two_pass, demo, use_grid, fused, wide_now, brick;                     // the pair search
  bool mesh, terrain_any, terrain_grid;                                      // the static mesh and the bodies' faces
  bool lists_merged, contacts_fused, front_rows, side_terrain, tc_job, fork; // the front ends without a narrowphase launch of their own
  bool big;
  uint32_t n, n_obs, MP, t_stride, p_stride, cap_t, cap_p, cap_c, levels, cells;
  float min_frac;
  float3 wlim;
  const SceneBounds* grid_box_of;
  hipStream_t s;  // what the launches take of the world: the main stream, the bodies (packed records only if this tick's), the mesh, the device counts
  Bodies B;
  TerrainDev M;
  StepCounts* sc;
};
// `cleared`: collide_enqueue's finding, taken before collide_prepare may have replaced the plan it is about.
static CollidePlan collide_plan(mgf_world* w, bool cleared) {
  CollidePlan P;
  const uint32_t n = P.n = w->n;
  P.s = w->ctx->stream; P.sc = w->sc.p;
  P.cleared = cleared;
  P.bounds_done = w->bounds_cover == n && n > 0;  // this tick's k_integrate (and k_import_ghosts) gathered the scene bounds
  P.rows_done = w->terrain_rows_done;             // ... and listed the owned bodies' terrain faces (ghosts have none)
  P.pack_ok = w->pack_cover == n && n > 0;        // ... and wrote the packed (collider, motion, info) records; ghosts brought theirs
  P.cells_done = cleared && P.bounds_done && w->cells_cover == n && w->cells_levels == w->plan.levels;  // ... and worked out the cells and ranks (over last tick's box)
  P.B = w->bodies();
  if (!P.pack_ok) P.B.bpk = nullptr;
  P.cap_t = w->cap_t; P.cap_p = w->cap_p; P.cap_c = w->cap_c; P.levels = w->plan.levels; P.cells = w->plan.cells;
  P.min_frac = (float)w->opt.grid_min_frac_pct * 0.01f;  // (thin axes of the scene are widened to this fraction of the longest: grid_box)
  P.grid_box_of = P.cells_done ? w->sb_grid.p : nullptr;  // (null: this tick's own bounds)
  P.demo = w->demo_rows_ready;  // the partner rows came from the host's replay of world.rs: no device pair search
  P.two_pass = (w->opt.two_pass != 0 || w->tick_two_pass) && !P.demo;
  P.use_grid = !P.two_pass && !w->opt.broadphase_tree && !w->grid_too_wide;
  // a world of spheres: the grid broadphase runs the sphere-sphere test on the partners it accepts and lists contacts only
  P.fused = P.use_grid && !w->has_capsule && !w->has_compound && !w->opt.no_fused_narrowphase && !P.demo;
  // the wide bodies of this tick's k_integrate (kept out of the bounds this phase lays its cells over: WideSpec): never partners of the grid's
  // pair search, paired by k_pair_wide behind it.  (Not beside the brick kernel, which reads a query's order id from its leaf record.)
  P.wide_now = w->wide_tick_on && P.bounds_done && P.use_grid && !P.two_pass && !P.demo;
  P.wlim = P.wide_now ? make_float3(w->wide_limit[0], w->wide_limit[1], w->wide_limit[2]) : make_float3(0.0f, 0.0f, 0.0f);
  P.n_obs = (uint32_t)w->obstacles.size();
  P.mesh = w->terrain && !w->terrain->m.tree.empty();
  if (P.mesh) P.M = w->terrain->dev(w->word(kWStackOverflow));
  else memset(&P.M, 0, sizeof(P.M));
  P.terrain_any = P.mesh && w->n_owned;
  P.terrain_grid = !P.two_pass && P.mesh && w->terrain->grid.ready && !w->terrain_grid_off && !w->opt.terrain_tree && !P.n_obs;
  // a world of spheres over a small mesh: the lists, the terrain narrowphase and the contact numbering in one launch (k_lists_spheres) -
  // or (r05) from the rows to the constraint records without candidate lists (k_terrain_contacts, k_contacts_spheres)
  P.lists_merged = P.fused && !P.two_pass && !P.terrain_grid && !P.demo && !mixed_world(w) && !P.n_obs;
  P.contacts_fused = P.lists_merged && w->opt.fused_contacts && (P.rows_done || !P.terrain_any);  // (rows_done: k_integrate's tail also listed the bodies near the mesh)
  // (r06) worlds of single-component bodies that are not all spheres - capsules, mixed: the same list-free front end (k_front_rows.h): the pair
  // search runs the pair test on the partners it accepts (k_pair_grid_n), the bodies near the mesh get their faces and the body-triangle
  // test in one launch (k_near_list + k_terrain_near over the face grid; a small mesh: the rows and records of k_integrate's tail,
  // k_terrain_contacts<true>), k_contacts_rows<false> writes the records
  // (bodies of up to two components: the same with a manifold of up to four contacts per row entry - k_pair_grid_n<true>, k_terrain_contacts<2>,
  // k_contacts_rows_parts; their terrain side over the face grid of a large mesh is not built: the list-based kernels)
  const bool parts2 = w->has_compound && w->max_parts <= 2u;
  // (a tick with wide bodies in a world of two-part bodies takes the list-based kernels: k_pair_wide appends partners or single contacts to the rows,
  // not the manifolds of k_pair_grid_n<true>)
  P.front_rows = !P.fused && P.use_grid && !P.two_pass && !P.demo && (!w->has_compound || (parts2 && !P.wide_now)) && !P.n_obs && w->opt.front_rows &&
                 !w->front_rows_off && n < (1u << 26) &&
                 (!P.terrain_any || (P.terrain_grid && !w->has_compound) || (!P.terrain_grid && P.rows_done && w->opt.fused_contacts));
  P.brick = P.use_grid && !P.demo && w->opt.pair_brick && w->pair_brick_off == 0 && !P.wide_now && !P.front_rows;  // (k_pair_grid_n is the pair search of a front_rows world)
  P.side_terrain = P.front_rows && P.terrain_any && P.terrain_grid;  // its terrain side over the face grid: k_near_list, k_terrain_near, k_terrain_tests
  // (the terrain contacts of the list-free paths over a small mesh - k_terrain_contacts - ride in the scatter's launch, or run beside it)
  P.tc_job = (P.contacts_fused || (P.front_rows && !P.terrain_grid)) && P.terrain_any;
  // (the terrain kernels of the list-free front end on the context's second stream: side_fork)
  P.fork = (P.side_terrain || (P.tc_job && P.front_rows)) && w->opt.side_stream && !w->opt.phase_timing;
  P.MP = w->max_parts > 2u ? (uint32_t)kMaxParts : 2u;  // (what ghosts and arrivals may bring is in max_parts too: option body_kinds, bit 3)
  P.big = w->max_parts > (uint32_t)kMaxParts;  // (r06) a body of more than kMaxParts components: k_narrow_pairs_big, k_narrow_terrain_big
  P.t_stride = w->has_compound ? 2u * (P.big ? w->max_parts : P.MP) : 2u; P.p_stride = w->has_compound ? P.MP * P.MP : 1u;
  return P;
}
static Lbvh tick_tree(mgf_world* w, const CollidePlan& P) {  // (lcol and ltb: ensured by stage_cells)
  Lbvh T;
  T.nodes = w->lnodes.p; T.leaves = w->leaves.p; T.sidx = w->sidx.p; T.cell_lo = w->cell_lo.p;
  T.n = w->n; T.levels = P.levels; T.err = w->word(kWStackOverflow);
  T.dbg = nullptr;
  T.ext = w->ext_ptr();
  T.lcol = P.fused ? w->lcol.p : nullptr;
  T.ltb = (P.use_grid && !P.demo) ? w->ltb.p : nullptr;  // the queries in cell order, with the cells each has to look at
  return T;
}
// The context's second stream for the work of a tick that runs BESIDE its main chain (CollidePlan::fork): behind everything the main stream
// holds so far.  side_done marks the end of the side work; side_join makes the main stream wait for it.
static mgf_status side_fork(mgf_world* w) {
  mgf_ctx* ctx = w->ctx;
  if (!ctx->aux) {  // (the highest priority: its few long waves are placed ahead of the pair search's thousands)
    int lo = 0, hi = 0;
    MGF_HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
    MGF_HIP_TRY(hipStreamCreateWithPriority(&ctx->aux, hipStreamNonBlocking, w->opt.side_stream >= 2 ? lo : hi));
  }
  if (!w->ts->ev_fork) { MGF_HIP_TRY(hipEventCreateWithFlags(&w->ts->ev_fork, hipEventDisableTiming)); MGF_HIP_TRY(hipEventCreateWithFlags(&w->ts->ev_join, hipEventDisableTiming)); }
  MGF_HIP_TRY(hipEventRecord(w->ts->ev_fork, ctx->stream));
  MGF_HIP_TRY(hipStreamWaitEvent(ctx->aux, w->ts->ev_fork, 0));
  return MGF_OK;
}
static mgf_status side_done(mgf_world* w) { MGF_HIP_TRY(hipEventRecord(w->ts->ev_join, w->ctx->aux)); return MGF_OK; }
static mgf_status side_join(mgf_world* w) { MGF_HIP_TRY(hipStreamWaitEvent(w->ctx->stream, w->ts->ev_join, 0)); return MGF_OK; }
static void launch_scatter(mgf_world* w, const CollidePlan& P, const Lbvh& T) {
  k_scatter_leaves<<<nblk(w->n), kBlock, 0, w->ctx->stream>>>(T, w->fb_c.p, w->fb_r.p, w->cell_of.p, w->cell_rank.p, w->brank.p, w->col0.p, w->delta.p, w->tb_c.p, w->tb_r.p, w->sb.p,
                                                            1e-3f, P.min_frac, P.grid_box_of, P.wlim, w->n_owned);
}

// 1. scene bounds, Morton cells and ranks (what k_integrate has not done already), the cells' prefix sum
static mgf_status stage_cells(mgf_world* w, const CollidePlan& P) {
  if (!P.bounds_done) {
    // 64 blocks: every block ends with 9 atomics on the one line of SceneBounds, and same-line atomics serialise
    k_scene_bounds<<<std::min<unsigned>(nblk(P.n), 64u), kBlock, 0, P.s>>>(w->fb_c.p, w->fb_r.p, P.n, w->sb.p);
    LAUNCH_CHECK();
  }
  if (!P.cells_done) {
    const bool fold_in_morton = P.cleared && P.bounds_done;  // (k_tick_clear ran before the bounds existed: k_morton_count folds them)
    k_morton_count<<<nblk(P.n), kBlock, 0, P.s>>>(w->fb_c.p, P.n, w->sb.p, kMortonBits - 2 * (int)P.levels, w->cell_of.p, w->cell_rank.p, w->cell_cnt.p, P.min_frac, make_uint3(0, 0, 0),
                                              fold_in_morton ? w->sb_part.p : nullptr, w->sb.p);
    LAUNCH_CHECK();
  }
  MGF_TRY(tick_scan(w, 0, w->cell_cnt.p, w->cell_lo.p, nullptr, nullptr, (size_t)P.cells + 1, nullptr, nullptr, P.cells_done ? w->sb_part.p : nullptr));
  if (P.fused) MGF_TRY(w->lcol.ensure(2 * (size_t)P.n, P.s));
  if (P.use_grid && !P.demo) MGF_TRY(w->ltb.ensure(2 * (size_t)P.n, P.s));
  return MGF_OK;
}
// 2. The terrain side of the list-free front end over the face grid.  It needs nothing of the cell sort: it runs BESIDE it and the pair search, on
// the context's second stream (the body-triangle tests are one long walk through tri_mcapsule's branches per wave, about a wave per SIMD:
// arithmetic the pair search - bound by its cache look-ups - leaves idle).  Fork behind the tick's clearing launch, join ahead of the constraint scan.
static mgf_status stage_side_terrain(mgf_world* w, const CollidePlan& P) {
  if (!P.side_terrain) return MGF_OK;
  const uint32_t slot_space = std::max(P.cap_t, kTnRegions);  // (kTnRegions regions of at least one slot)
  MGF_TRY(w->t_cand.ensure(slot_space, P.s)); MGF_TRY(w->t_owner.ensure(slot_space, P.s)); MGF_TRY(w->t_out.ensure(2 * (size_t)slot_space, P.s));
  hipStream_t ts = P.s;
  if (P.fork) {
    MGF_TRY(side_fork(w));
    ts = w->opt.side_stream == 3 ? P.s : w->ctx->aux;  // (3: the events without the side stream - what the fork and the join cost by themselves)
  }
  MGF_TRY(w->near_ids.ensure(w->n_owned, P.s)); MGF_TRY(w->tpos.ensure(P.n + 1, P.s));
  const FaceGrid FG = w->terrain->face_grid();
  k_near_list<<<nblk(w->n_owned), kBlock, 0, ts>>>(w->tb_c.p, w->tb_r.p, w->n_owned, P.M, FG.sb, 1e-3f, w->near_ids.p, w->cs_sums.p + 2 * kCsSumStride, w->word(kWSkipGuard));
  LAUNCH_CHECK();
  TerrainNear A;
  A.M = P.M; A.G = FG; A.near_ids = w->near_ids.p; A.near_cnt = w->cs_sums.p + 2 * kCsSumStride; A.face_of_rank = w->terrain->grid.face_of_rank.p;
  const uint32_t region_cap = slot_space / kTnRegions;
  A.pad_abs = 1e-3f; A.cap_t = P.cap_t; A.cnt = w->front_cnt.p; A.region_cap = region_cap; A.slot_body = w->t_owner.p; A.slot_rank = w->t_cand.p; A.tpos = w->tpos.p; A.t_cnt = w->t_cnt.p;
  A.overflow = w->word(kWRowOverflow); A.too_wide = w->word(kWTerrainWide); A.guard = w->word(kWSkipGuard);
  A.check = w->opt.front_rows_check ? 1u : 0u;
  const unsigned tgb = 8u * std::max(1u, std::min((unsigned)((w->n_owned + (kBlock / kTnLanes) - 1) / (kBlock / kTnLanes) + 7u) / 8u, 256u));  // (a multiple of the XCDs)
  k_terrain_near<kTnLanes><<<tgb, kBlock, 0, ts>>>(P.B, A);
  LAUNCH_CHECK();
  TerrainTests X;
  X.M = P.M; X.face_of_rank = w->terrain->grid.face_of_rank.p; X.slot_body = w->t_owner.p; X.slot_rank = w->t_cand.p; X.cnt = w->front_cnt.p; X.region_cap = region_cap;
  X.t_out = w->t_out.p; X.tcn = w->tcn.p; X.sum_ct = w->cs_sums.p + kCsSumStride; X.flag = w->word(kWNarrowMismatch); X.overflow = w->word(kWRowOverflow);
  k_terrain_tests<<<nblk((size_t)region_cap * kTnRegions), kBlock, 0, ts>>>(P.B, X);
  LAUNCH_CHECK();
  if (P.fork) MGF_TRY(side_done(w));
  return MGF_OK;
}
// 3. the leaves into cell order - with the terrain contacts of the list-free paths over a small mesh riding in the launch, or beside it
static mgf_status stage_scatter(mgf_world* w, const CollidePlan& P) {
  const Lbvh T = tick_tree(w, P);
  if (P.tc_job) {
    const uint32_t t_stride0 = w->has_compound ? 2u * P.MP : 2u;  // (bodies of two components: 4 contacts per slot)
    MGF_TRY(w->t_out.ensure((size_t)t_stride0 * P.cap_t, P.s)); MGF_TRY(w->tpos.ensure(P.n + 1, P.s));
    TerrainContacts A;
    A.M = P.M; A.near_list = w->near_list.p; A.near_cnt = w->cs_sums.p + 2 * kCsSumStride;
    A.n_faces = (uint32_t)(w->terrain->faces.size() / 3); A.n_verts = (uint32_t)w->terrain->verts.size(); A.cap_row_t = w->row_cap_t; A.cap_t = P.cap_t;
    A.rows_t = w->rows_t.p; A.sums = w->cs_sums.p; A.t_out = w->t_out.p; A.tcn = w->tcn.p; A.tpos = w->tpos.p; A.guard = w->word(kWSkipGuard);
    A.check = (P.front_rows && w->opt.front_rows_check) ? 1u : 0u; A.flag = w->word(kWNarrowMismatch);
    A.col1 = w->col1.p; A.pcount = w->has_compound ? w->pcount.p : nullptr; A.wp0 = w->wp0.p; A.wp1 = w->wp1.p;
    // (room for an eighth of the bodies per pass; the list's length is on the device)
    const unsigned tg = std::max(1u, std::min(nblk((size_t)w->n_owned * kTcLanes / 8 + 1), 256u));
    if (P.front_rows) {  // (bodies of any kind: a launch of its own - the body-triangle test's registers would be the streaming scatter's too - on the side stream)
      // (side_stream = 3, the events alone, is the face-grid site's experiment - stage_side_terrain: here 3 is the side stream like 1)
      if (P.fork) MGF_TRY(side_fork(w));
      hipStream_t ts = P.fork ? w->ctx->aux : P.s;
      if (w->has_compound) k_terrain_contacts<2><<<tg, kBlock, 0, ts>>>(A);
      else k_terrain_contacts<1><<<tg, kBlock, 0, ts>>>(A);
      LAUNCH_CHECK();
      if (P.fork) MGF_TRY(side_done(w));
      launch_scatter(w, P, T);
    } else if (w->opt.fused_contacts >= 2) {  // (A/B: a launch of its own)
      k_terrain_contacts<0><<<tg, kBlock, 0, P.s>>>(A);
      LAUNCH_CHECK();
      launch_scatter(w, P, T);
    } else {
      k_scatter_leaves_tc<0><<<nblk(P.n) + tg, kBlock, 0, P.s>>>(T, w->fb_c.p, w->fb_r.p, w->cell_of.p, w->cell_rank.p, w->brank.p, w->col0.p, w->delta.p, w->tb_c.p, w->tb_r.p, w->sb.p, 1e-3f,
                                                             P.min_frac, A, tg, P.grid_box_of, P.wlim, w->n_owned);
    }
  } else {
    launch_scatter(w, P, T);
  }
  LAUNCH_CHECK();
  w->sidx_valid = P.n == w->n_owned;  // (the next tick's re-sort of the store may follow this order)
  return MGF_OK;
}
// 4. inner nodes are only needed by the tree walks
static mgf_status stage_inner_nodes(mgf_world* w, const CollidePlan& P) {
  if (P.use_grid) return MGF_OK;
  const Lbvh T = tick_tree(w, P);
  k_lbvh_low<<<P.cells / kBlock, kBlock, 0, P.s>>>(T, w->sub_lo.p, w->sub_hi.p);
  LAUNCH_CHECK();
  if (P.levels > 4) { k_lbvh_top<<<1, 1024, 0, P.s>>>(T, w->sub_lo.p, w->sub_hi.p, w->sub2_lo.p, w->sub2_hi.p); LAUNCH_CHECK(); }
  return MGF_OK;
}
// 5. the candidate buffers; the bodies' terrain faces and obstacle components into fixed-capacity rows (the two-pass path counts them in stage 6)
static mgf_status stage_terrain_rows(mgf_world* w, const CollidePlan& P) {
  MGF_TRY(w->t_cand.ensure(P.cap_t, P.s)); MGF_TRY(w->t_owner.ensure(P.cap_t, P.s));
  MGF_TRY(w->p_cand.ensure(P.cap_p, P.s)); MGF_TRY(w->p_owner.ensure(P.cap_p, P.s));
  MGF_TRY(w->t_nc.ensure(P.cap_t, P.s)); MGF_TRY(w->p_nc.ensure(P.cap_p, P.s));
  MGF_TRY(w->t_pre.ensure(P.cap_t, P.s)); MGF_TRY(w->p_pre.ensure(P.cap_p, P.s));
  static_assert(kBigKeep == (uint32_t)(kMaxParts * kMaxParts), "k_narrow_pairs_big writes k_narrow_pairs_parts<kMaxParts>'s records");
  MGF_TRY(w->t_out.ensure((size_t)P.t_stride * P.cap_t, P.s)); MGF_TRY(w->p_out.ensure((size_t)P.p_stride * P.cap_p, P.s));
  if (P.two_pass) return MGF_OK;
  MGF_TRY(w->rows.ensure((size_t)P.n * kRowCap, P.s));
  MGF_TRY(w->rows_t.ensure((size_t)P.n * w->row_cap_t, P.s, P.rows_done, (size_t)w->n_owned * w->row_cap_t));
  if (P.terrain_any && !P.rows_done && !P.side_terrain) {  // (side_terrain: enqueued in stage 2, on the side stream)
    if (P.terrain_grid) {
      const uint32_t per_block = kCoopBlock / kCoopLanes;
      const uint32_t tg = 8 * (((w->n_owned + per_block - 1) / per_block + 7) / 8);
      k_terrain_grid<<<tg, kCoopBlock, 0, P.s>>>(P.B, w->n_owned, nullptr, P.M, w->terrain->face_grid(), 1e-3f, w->row_cap_t, w->rows_t.p, w->t_cnt.p,
                                               w->word(kWRowOverflow), w->word(kWTerrainWide));
    } else {
      k_terrain_rows<<<nblk(w->n_owned), kBlock, 0, P.s>>>(P.B, w->n_owned, P.M, w->row_cap_t, w->rows_t.p, w->t_cnt.p, w->word(kWRowOverflow));
    }
    LAUNCH_CHECK();
  }
  if (P.n_obs && w->n_owned) {  // the obstacles' components each body's parts may touch, behind its faces
    k_obstacle_rows<<<nblk(w->n_owned), kBlock, 0, P.s>>>(P.B, w->n_owned, w->d_obs.p, P.n_obs, w->row_cap_t, w->rows_t.p, w->t_cnt.p, w->word(kWRowOverflow));
    LAUNCH_CHECK();
  }
  return MGF_OK;
}
// 6. the pair search: one pass, hits written to fixed-capacity rows, and k_pair_wide behind it - or the two-pass path's counting pass
static mgf_status stage_pair_search(mgf_world* w, const CollidePlan& P) {
  const Lbvh T = tick_tree(w, P);
  if (P.two_pass) {
    k_candidates<false><<<8 * xcd_blocks_per(P.n), kBlock, 0, P.s>>>(P.B, P.n, w->n_owned, T, P.M, 1e-3f, w->t_cnt.p, w->p_cnt.p, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    LAUNCH_CHECK();
    if (P.n_obs && w->n_owned) {  // the obstacles' components behind each body's faces, counted ...
      k_obstacle_candidates<false><<<nblk(w->n_owned), kBlock, 0, P.s>>>(P.B, w->n_owned, w->d_obs.p, P.n_obs, w->t_cnt.p, nullptr, nullptr, nullptr, nullptr);
      LAUNCH_CHECK();
    }
    return MGF_OK;
  }
  if (P.brick && !w->pair_brick_attr) {
    MGF_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_pair_brick<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)brick_lds_bytes(true, kBrickCap)));
    MGF_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_pair_brick<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)brick_lds_bytes(false, kBrickCap)));
    w->pair_brick_attr = true;
  }
  const uint32_t per_block = kCoopBlock / kCoopLanes;
  const uint32_t grid = 8 * (((P.n + per_block - 1) / per_block + 7) / 8);
  const uint32_t bricks = 8 * ((((1u << (2 * P.levels)) >> 6) + 7) / 8);
  uint32_t* const overflow = w->word(kWRowOverflow);
  uint32_t* const too_wide = w->word(kWGridWide);
  if (P.demo) {}
  else if (P.front_rows && w->has_compound) { MGF_TRY(w->cnt.ensure(P.n + 1, P.s)); k_pair_grid_n<true><<<grid, kCoopBlock, 0, P.s>>>(P.B, P.n, w->n_owned, T, w->sb.p, 1e-3f, w->rows.p, w->p_cnt.p, overflow, too_wide, w->pair_stat.p, P.min_frac, w->cnt.p); }
  else if (P.front_rows) k_pair_grid_n<false><<<grid, kCoopBlock, 0, P.s>>>(P.B, P.n, w->n_owned, T, w->sb.p, 1e-3f, w->rows.p, w->p_cnt.p, overflow, too_wide, w->pair_stat.p, P.min_frac, nullptr);
  else if (P.brick && P.fused) k_pair_brick<true><<<bricks, kCoopBlock, brick_lds_bytes(true, kBrickCap), P.s>>>(P.n, w->n_owned, T, w->rows.p, w->p_cnt.p, overflow, too_wide, w->pair_stat.p, w->word(kWBrickSlow), kBrickCap);
  else if (P.brick) k_pair_brick<false><<<bricks, kCoopBlock, brick_lds_bytes(false, kBrickCap), P.s>>>(P.n, w->n_owned, T, w->rows.p, w->p_cnt.p, overflow, too_wide, w->pair_stat.p, w->word(kWBrickSlow), kBrickCap);
  else if (P.use_grid && P.fused) k_pair_grid<true><<<grid, kCoopBlock, 0, P.s>>>(P.B, P.n, w->n_owned, T, w->sb.p, 1e-3f, w->rows.p, w->p_cnt.p, overflow, too_wide, w->pair_stat.p, P.min_frac);
  else if (P.use_grid) k_pair_grid<false><<<grid, kCoopBlock, 0, P.s>>>(P.B, P.n, w->n_owned, T, w->sb.p, 1e-3f, w->rows.p, w->p_cnt.p, overflow, too_wide, nullptr, P.min_frac);
  else k_pair_rows<<<grid, kCoopBlock, 0, P.s>>>(P.B, P.n, w->n_owned, T, 1e-3f, w->rows.p, w->p_cnt.p, overflow);
  LAUNCH_CHECK();
  if (P.wide_now) {
    PairWide W;
    W.list = w->wide_list.p; W.count = &w->sb.p->pad; W.T = T; W.sb = w->sb.p; W.box = P.grid_box_of; W.pad_abs = 1e-3f; W.min_frac = P.min_frac; W.n = P.n; W.n_owned = w->n_owned;
    W.contacts = (P.fused || P.front_rows) ? 1u : 0u; W.rows_p = w->rows.p; W.p_cnt = w->p_cnt.p; W.overflow = overflow; W.too_wide = too_wide;
    W.pair_stat = (P.fused || P.front_rows) ? w->pair_stat.p : nullptr; W.guard = w->word(kWSkipGuard);
    k_pair_wide<<<kWideCap, kBlock, 0, P.s>>>(P.B, W);
    LAUNCH_CHECK();
  }
  return MGF_OK;
}
// the list-free front ends (contacts_fused, front_rows): from the rows to the constraint records - numbering, ContactConstraint::new - in one launch
static mgf_status contacts_from_rows(mgf_world* w, const CollidePlan& P, float dt) {
  MGF_TRY(w->base.ensure(P.n + 1, P.s)); MGF_TRY(w->tpos.ensure(P.n + 1, P.s));
  // (option scan_fused, bit 1) a world of spheres with the split launch: the numbering inside k_contacts_rows_index_scan - no scan launch.  The other
  // front ends keep the scan: k_contacts_rows_index<false>'s slot blocks and k_contacts_rows_parts' terrain blocks read base of arbitrary bodies.
  const bool num_fused = (w->opt.scan_fused & 1) && w->opt.contacts_split && !P.front_rows && !P.side_terrain;
  ScanEpilogue E;
  memset(&E, 0, sizeof(E));
  E.kind = 3; E.cap_a = P.cap_t; E.cap_b = P.cap_c; E.row_overflow = w->word(kWRowOverflow); E.grid_wide = P.use_grid ? w->word(kWGridWide) : nullptr;
  E.terrain_wide = (P.front_rows && P.terrain_grid) ? w->word(kWTerrainWide) : nullptr;
  E.wide_n = P.wide_now ? &w->sb.p->pad : nullptr;
  E.guard = w->word(kWSkipGuard); E.sc = P.sc; E.sum_t = w->cs_sums.p; E.sum_ct = w->cs_sums.p + kCsSumStride;
  if (P.side_terrain) { E.sum_t = w->front_cnt.p + (size_t)kTnRegions * kTnCntStride; E.sum_t_parts = kTnRegions; E.sum_t_stride = kTnCntStride; }
  if (!num_fused) MGF_TRY(tick_scan(w, 2, w->p_cnt.p, w->base.p, nullptr, nullptr, (size_t)P.n + 1, &E, w->tcn.p));
  ContactsSpheres A;
  memset(&A, 0, sizeof(A));
  A.epi = E;
  A.sc = P.sc; A.n = P.n; A.cap_row_t = w->row_cap_t; A.cap_c = P.cap_c; A.cap_t = P.cap_t; A.t_out = w->t_out.p;
  A.rows_p = w->rows.p; A.t_cnt = w->t_cnt.p; A.p_cnt = w->p_cnt.p; A.base = w->base.p; A.tcn = w->tcn.p; A.tpos = w->tpos.p;
  A.dt = dt; A.baumgarte = w->params.baumgarte; A.slop = w->params.penetration_slop;
  A.cons = w->cons_nat.p; A.ab = w->c_ab.p; A.degb = w->degb.p; A.rev = w->rev.p; A.rev_cap = w->rev_cap; A.rev_flag = w->word(kWRevRowOverflow); A.flag = w->word(kWNarrowMismatch);
  A.ext = w->ext_ptr();
  A.t_blocks = 0; A.region_cap = 1; A.regions = 0; A.cnt_stride = 0; A.slot_body = nullptr; A.slot_cnt = nullptr;
  if (P.side_terrain) {  // (k_terrain_near's slots: the terrain constraints a lane per slot)
    A.region_cap = std::max(P.cap_t, kTnRegions) / kTnRegions; A.regions = kTnRegions; A.cnt_stride = kTnCntStride; A.slot_body = w->t_owner.p; A.slot_cnt = w->front_cnt.p;
    A.t_blocks = nblk((size_t)A.region_cap * kTnRegions);
  }
  if (P.front_rows && w->has_compound) {
    ContactsParts Q;
    Q.sc = P.sc; Q.n = P.n; Q.cap_c = P.cap_c; Q.cap_t = P.cap_t; Q.t_stride = 4u; Q.rows_p = w->rows.p; Q.t_cnt = w->t_cnt.p; Q.p_cnt = w->p_cnt.p; Q.p_ent = w->cnt.p;
    Q.base = w->base.p; Q.tcn = w->tcn.p; Q.tpos = w->tpos.p; Q.t_out = w->t_out.p; Q.dt = dt; Q.baumgarte = w->params.baumgarte; Q.slop = w->params.penetration_slop;
    Q.cons = w->cons_nat.p; Q.ab = w->c_ab.p; Q.degb = w->degb.p; Q.rev = w->rev.p; Q.rev_cap = w->rev_cap; Q.rev_flag = w->word(kWRevRowOverflow); Q.flag = w->word(kWNarrowMismatch); Q.ext = w->ext_ptr();
    k_contacts_rows_parts<<<2 * nblk(P.n), kBlock, 0, P.s>>>(P.B, P.M, Q);  // (entries' blocks, then the same bodies' terrain blocks)
  }
  else if (w->opt.contacts_split) {  // the numbering now, the partner contacts' records beside the solver's table kernels or behind them (stage_links)
    if (P.front_rows) k_contacts_rows_index<false><<<A.t_blocks + nblk(P.n), kBlock, 0, P.s>>>(P.B, P.M, A);
    else if (num_fused) {
      uint32_t* ws = w->scan_ws.p + scan_ws_num_at(w);
      A.base_out = w->base.p; A.num_runs = (P.n + kNumSubs * kBlock - 1) / (kNumSubs * kBlock);  // (a workgroup: kNumSubs groups of 256 bodies, one ticket)
      A.num_status = reinterpret_cast<unsigned long long*>(ws); A.num_ticket = ws + 2 * ((size_t)nblk(P.n) + 1);
      // (option tables_fused) ... and the solver's block tables, a ticket per solver block, where stage_links would launch k_flow6_blocks on a
      // re-sorted store: mode 6's plan was made and its words cleared by this phase's clearing launch (flow6_zeroed: the solver follows), no
      // re-run with the global solver, blocks of at most a workgroup's bodies and no more of them than the numbering has status words.  The plan is
      // made again here from the host's values of earlier ticks - what flow6_build_tables will find behind this launch, inside the same enqueue.
      bool tab = false;
      Flow6 F;
      if (w->opt.tables_fused && w->opt.solver_mode == 6 && !w->tick_mode1 && w->flow6_zeroed && w->flow5_ok && !w->flow6_prepped) {
        MGF_TRY(flow6_plan(w, P.cap_c, w->f6_prep_iters ? w->f6_prep_iters : 10u, &tab));
        if (tab) {
          F = flow6_args(w);
          tab = F.ident && F.n == P.n && F.nb <= (uint32_t)(kNumSubs * kBlock) && F.nblocks <= nblk(P.n) + 1u;
        }
      }
      if (tab) {
        A.num_runs = F.nblocks;
        k_contacts_rows_index_tables<<<A.num_runs, kNumSubs * kBlock, 0, P.s>>>(P.B, P.M, A, F);
        w->f6_tables_early = true; w->ts->tab_fused = true;
      }
      else k_contacts_rows_index_scan<<<A.num_runs, kNumSubs * kBlock, 0, P.s>>>(P.B, P.M, A);
      w->ts->num_fused = true;
    }
    else k_contacts_rows_index<true><<<nblk(P.n), kBlock, 0, P.s>>>(P.B, P.M, A);
    w->rec_B = P.B; w->rec_A = A; w->rec_sph = !P.front_rows; w->records_pending = true;
  }
  else if (P.front_rows) k_contacts_rows<false><<<A.t_blocks + nblk(P.n), kBlock, 0, P.s>>>(P.B, P.M, A);
  else k_contacts_rows<true><<<nblk(P.n), kBlock, 0, P.s>>>(P.B, P.M, A);
  return MGF_OK;
}
// the record half of a split k_contacts_rows in a launch of its own (no tables are built inside this collide phase: another solver mode, a plan
// that does not fit, a caller's list - or option contacts_split = 4)
static mgf_status records_launch_alone(mgf_world* w, hipStream_t s) {
  const unsigned g = std::max(1u, nblk(w->rec_A.cap_c));
  if (w->rec_sph) k_contacts_rows_records<true><<<g, kBlock, 0, s>>>(w->rec_B, w->rec_A);
  else k_contacts_rows_records<false><<<g, kBlock, 0, s>>>(w->rec_B, w->rec_A);
  LAUNCH_CHECK();
  return MGF_OK;
}
// 7. the candidate lists from the rows (or the two-pass path's filling pass) - or, in their place, the list-free front ends' records
static mgf_status stage_lists(mgf_world* w, const CollidePlan& P, float dt) {
  const bool list_free = P.contacts_fused || P.front_rows;
  if (!list_free) {  // the scan's last thread checks the list sizes against the capacities and fills *P.sc (no launch of its own)
    ScanEpilogue E;
    E.kind = 1; E.cap_a = P.cap_t; E.cap_b = P.cap_p; E.row_overflow = P.two_pass ? nullptr : w->word(kWRowOverflow); E.grid_wide = P.use_grid ? w->word(kWGridWide) : nullptr;
    E.terrain_wide = P.terrain_grid ? w->word(kWTerrainWide) : nullptr; E.guard = w->word(kWSkipGuard); E.sc = P.sc;
    E.wide_n = P.wide_now ? &w->sb.p->pad : nullptr; E.sum_t_parts = 0; E.sum_t_stride = 0;
    MGF_TRY(tick_scan(w, 1, w->t_cnt.p, w->t_off.p, w->p_cnt.p, w->p_off.p, (size_t)P.n + 1, &E));
  }
  if (P.fork) MGF_TRY(side_join(w));  // (the terrain side has parked its contacts: tcn, tpos, t_cnt, the counts)
  if (list_free) {
    MGF_TRY(contacts_from_rows(w, P, dt));
  } else if (P.lists_merged) {
    MGF_TRY(w->cnt.ensure(P.n + 1, P.s)); MGF_TRY(w->base.ensure(P.n + 1, P.s)); MGF_TRY(w->tcn.ensure(P.n + 1, P.s));
    k_lists_spheres<<<nblk(P.n), kBlock, 0, P.s>>>(P.B, P.M, P.sc, P.n, w->row_cap_t, w->rows_t.p, w->rows.p, w->t_off.p, w->p_off.p, w->t_cand.p, w->t_owner.p, w->t_nc.p,
                                               w->t_out.p, w->t_pre.p, w->p_cand.p, w->p_owner.p, w->p_pre.p, w->cnt.p, w->tcn.p, w->ext_ptr());
  } else if (P.two_pass) {
    k_candidates<true><<<8 * xcd_blocks_per(P.n), kBlock, 0, P.s>>>(P.B, P.n, w->n_owned, tick_tree(w, P), P.M, 1e-3f, nullptr, nullptr, w->t_off.p, w->p_off.p, w->t_cand.p, w->t_owner.p,
                                                  w->p_cand.p, w->p_owner.p, P.sc);
    if (P.n_obs && w->n_owned) {  // ... and written
      LAUNCH_CHECK();
      k_obstacle_candidates<true><<<nblk(w->n_owned), kBlock, 0, P.s>>>(P.B, w->n_owned, w->d_obs.p, P.n_obs, w->t_cnt.p, w->t_off.p, w->t_cand.p, w->t_owner.p, P.sc);
    }
  } else {
    k_rows_to_csr<<<nblk(P.n), kBlock, 0, P.s>>>(P.sc, P.n, w->row_cap_t, P.terrain_grid ? w->terrain->grid.face_of_rank.p : nullptr, w->rows_t.p, w->rows.p, w->t_off.p, w->p_off.p, w->t_cand.p, w->t_owner.p, w->p_cand.p, w->p_owner.p);
  }
  LAUNCH_CHECK();
  return MGF_OK;
}
// 8. narrowphase over the candidate lists, one kernel per shape-pair type
static mgf_status stage_narrowphase(mgf_world* w, const CollidePlan& P) {
  const bool static_any = P.mesh || P.n_obs;
  if (P.lists_merged || P.front_rows) {
  } else if (w->has_compound) {  // bodies of several parts: one kernel over every pair of parts (ordinary bodies are bodies of one part)
    if (P.cap_p && P.big) {
      k_narrow_pairs_big<<<std::min(std::max(P.cap_p / 4u, 1u), 4096u), kBlock, 0, P.s>>>(P.B, &P.sc->Mp, w->p_owner.p, w->p_cand.p, w->p_nc.p, w->p_out.p, w->word(kWBigPartsOverflow));
      LAUNCH_CHECK();
    } else if (P.cap_p) {
      const auto kern = P.MP == 2u ? k_narrow_pairs_parts<2> : k_narrow_pairs_parts<kMaxParts>;
      kern<<<nblk(P.cap_p), kBlock, 0, P.s>>>(P.B, &P.sc->Mp, w->p_owner.p, w->p_cand.p, w->p_nc.p, w->p_out.p);
      LAUNCH_CHECK();
    }
    if (static_any && P.cap_t && P.big) {
      k_narrow_terrain_big<<<std::min(std::max(P.cap_t / 4u, 1u), 4096u), kBlock, 0, P.s>>>(P.B, P.M, &P.sc->Mt, w->t_owner.p, w->t_cand.p, w->t_nc.p, w->t_out.p, P.t_stride);
      LAUNCH_CHECK();
    } else if (static_any && P.cap_t) {
      const auto kern = P.MP == 2u ? k_narrow_terrain_parts<2> : k_narrow_terrain_parts<kMaxParts>;
      kern<<<nblk(P.cap_t), kBlock, 0, P.s>>>(P.B, P.M, &P.sc->Mt, w->t_owner.p, w->t_cand.p, w->t_nc.p, w->t_out.p);
      LAUNCH_CHECK();
    }
  } else if (!(w->has_sphere && w->has_capsule)) {
    int k = w->has_capsule ? 1 : 0;
    if (!P.fused) MGF_TRY(launch_pairs(w, P.B, k, k, nullptr, &P.sc->Mp, P.cap_p));  // fused: the list holds contacts, k_setup_pairs<true> evaluates them
    if (static_any) MGF_TRY(launch_terrain(w, P.B, k, P.M, nullptr, &P.sc->Mt, P.cap_t));
  } else {  // spheres and capsules: the candidates binned by shape-pair type
    MGF_TRY(w->work_lists.ensure(4 * (size_t)P.cap_p + 2 * (size_t)P.cap_t, P.s));
    uint32_t* lists_p = w->work_lists.p;
    uint32_t* lists_t = w->work_lists.p + 4 * (size_t)P.cap_p;
    k_bin_pairs<<<nblk(P.cap_p), kBlock, 0, P.s>>>(P.B, &P.sc->Mp, P.cap_p, w->p_owner.p, w->p_cand.p, lists_p, P.sc->bins);
    LAUNCH_CHECK();
    for (int ty = 0; ty < 4; ++ty) MGF_TRY(launch_pairs(w, P.B, ty >> 1, ty & 1, lists_p + (size_t)ty * P.cap_p, &P.sc->bins[ty], P.cap_p));
    if (static_any) {
      k_bin_terrain<<<nblk(P.cap_t), kBlock, 0, P.s>>>(P.B, &P.sc->Mt, P.cap_t, w->t_owner.p, lists_t, P.sc->bins + 4);
      LAUNCH_CHECK();
      for (int ty = 0; ty < 2; ++ty) MGF_TRY(launch_terrain(w, P.B, ty, P.M, lists_t + (size_t)ty * P.cap_t, &P.sc->bins[4 + ty], P.cap_t));
    }
  }
  if (P.n_obs && P.cap_t) {  // the flagged candidates: a body part against a component of an obstacle
    k_narrow_obstacles<<<nblk(P.cap_t), kBlock, 0, P.s>>>(P.B, w->d_obs.p, &P.sc->Mt, w->t_owner.p, w->t_cand.p, w->t_nc.p, w->t_out.p, P.t_stride);
    LAUNCH_CHECK();
  }
  return MGF_OK;
}
// 9. constraint numbering in insertion order + ContactConstraint::new (the list-free front ends have written their records: contacts_from_rows)
static mgf_status stage_setup(mgf_world* w, const CollidePlan& P, float dt) {
  MGF_TRY(w->cnt.ensure(P.n + 1, P.s)); MGF_TRY(w->base.ensure(P.n + 1, P.s)); MGF_TRY(w->tcn.ensure(P.n + 1, P.s));
  if (P.contacts_fused || P.front_rows) return MGF_OK;
  if (!P.lists_merged) {
    k_count_contacts<<<nblk(P.n), kBlock, 0, P.s>>>(P.sc, P.n, w->t_off.p, w->p_off.p, w->t_nc.p, P.fused ? nullptr : w->p_nc.p, w->p_cand.p, w->t_pre.p, w->p_pre.p, w->cnt.p,
                                                P.demo ? 1 : 0, w->tcn.p, w->ext_ptr());
    LAUNCH_CHECK();
  }
  {
    ScanEpilogue E;
    memset(&E, 0, sizeof(E));
    E.kind = 2; E.cap_a = P.cap_c; E.sc = P.sc;
    MGF_TRY(tick_scan(w, 2, w->cnt.p, w->base.p, nullptr, nullptr, (size_t)P.n + 1, &E));
  }
  TerrainSetup TS;
  memset(&TS, 0, sizeof(TS));
  if (P.mesh || P.n_obs) {  // the terrain candidates' constraints are set up by the first blocks of the same launch
    TS.M = P.M; TS.t_owner = w->t_owner.p; TS.t_nc = w->t_nc.p; TS.t_pre = w->t_pre.p; TS.t_in = w->t_out.p; TS.in_stride = P.t_stride; TS.blocks = nblk(P.cap_t);
    if (P.n_obs) { TS.t_cand = w->t_cand.p; TS.obs_center = w->d_obs_center.p; }
  }
  const auto setup = P.fused ? k_setup_pairs<true> : k_setup_pairs<false>;  // (fused: the list holds contacts - no narrowphase counts or records to read)
  setup<<<TS.blocks + nblk(P.cap_p), kBlock, 0, P.s>>>(P.B, P.sc, w->p_owner.p, w->p_cand.p, P.fused ? nullptr : w->p_nc.p, w->p_pre.p, P.fused ? nullptr : w->p_out.p, w->base.p, dt,
                                                         w->params.baumgarte, w->params.penetration_slop, w->cons_nat.p, w->c_ab.p, w->degb.p, w->rev.p, w->rev_cap,
                                                         w->word(kWRevRowOverflow), P.p_stride, w->word(kWNarrowMismatch), TS, w->ext_ptr());
  LAUNCH_CHECK();
  return MGF_OK;
}
// 10. the dependency links: for the block-local solver with message channels straight into its block tables (k_flow6_blocks +
// k_flow6_links), else the (succ, pred) arrays the other solver modes walk
static mgf_status stage_links(mgf_world* w, const CollidePlan& P) {
  if (P.cap_c >= kSuccId) return fail(MGF_ERR_CAPACITY, "too many constraints");
  w->depth = 0;
  bool tables = false;
  if (w->opt.solver_mode == 6 && !w->tick_mode1) MGF_TRY(flow6_build_tables(w, P.cap_c, &tables));
  if (w->records_pending) {  // (the tables' launch did not take them along)
    w->records_pending = false;
    MGF_TRY(records_launch_alone(w, P.s));
    w->ts->split_alone = true;
  }
  w->f6_tables_in_collide = tables; w->f6_collide_iters = w->f6_prep_iters;
  if (!tables) MGF_TRY(chain_rows_launch(w, nullptr));
  w->links_ready = !tables;
  return MGF_OK;
}
static mgf_status collide_enqueue(mgf_world* w, float dt, bool solver_follows = false) {
  hipStream_t s = w->ctx->stream;
  if (w->n == 0) { MGF_HIP_TRY(hipMemsetAsync(w->sc.p, 0, sizeof(StepCounts), s)); return MGF_OK; }
  // the clearing launch ran ahead of k_integrate (the fused tick) if the plan it was made for still holds
  const bool cleared = w->plan.zero_launched && w->plan.n == w->n && w->plan.cap_c == w->cap_c && w->plan.solver_follows == solver_follows && w->cap_p != 0;
  w->plan.zero_launched = false;  // (a re-run of the phase clears again)
  if (!cleared) MGF_TRY(collide_prepare(w, solver_follows, false, false));
  const CollidePlan P = collide_plan(w, cleared);
  w->invalidate_tick_caches();  // (a re-run of the phase computes the bounds and the rows again)
  if (w->pair_brick_off) --w->pair_brick_off;
  w->ts->brick = P.brick;
  w->ts->fused = P.fused || P.front_rows;  // (the accepted partners are counted by the pair search: the read-back takes the statistic along)
  w->ts->front_rows = P.front_rows;
  w->ts->contacts_fused = P.contacts_fused;
  w->ts->cells_early = P.cells_done;
  w->ts->two_pass = P.two_pass;
  w->ts->tree = !P.two_pass && !P.use_grid && !P.demo;
  w->ts->big_parts = P.big;
  w->records_pending = false; w->ts->split_fused = false; w->ts->split_alone = false; w->ts->num_fused = false;
  w->f6_tables_early = false; w->ts->tab_fused = false;
  MGF_TRY(stage_cells(w, P));
  MGF_TRY(stage_side_terrain(w, P));
  MGF_TRY(stage_scatter(w, P));
  MGF_TRY(stage_inner_nodes(w, P));
  MGF_TRY(phase_mark(w, 1, s));
  MGF_TRY(stage_terrain_rows(w, P));
  MGF_TRY(stage_pair_search(w, P));
  MGF_TRY(stage_lists(w, P, dt));
  MGF_TRY(phase_mark(w, 2, s));
  MGF_TRY(stage_narrowphase(w, P));
  MGF_TRY(phase_mark(w, 3, s));
  MGF_TRY(stage_setup(w, P, dt));
  MGF_TRY(stage_links(w, P));
  MGF_TRY(phase_mark(w, 4, s));
  return MGF_OK;
}

// Read the tick's sizes and flags back (the stream must have been synchronised by the caller's copy):
// MGF_OK + *retry=false when the collide phase is complete; *retry=true after growing a capacity or
// switching to the exact two-pass candidate path (the caller re-enqueues the phase).
// the tick's read-back, in three steps so that the next tick can be enqueued between the first and the second
// (`defer`: the publishing launch is the caller's - one for several worlds, k_publish_batch; defer->rb stays null where a copy command went out instead)
static mgf_status readback_enqueue(mgf_world* w, PublishOne* defer = nullptr) {
  hipStream_t s = w->ctx->stream;
  if (defer) memset(defer, 0, sizeof(*defer));
  // one copy of the read-back block (the pair statistic only when the fused broadphase filled it)
  const size_t rb_words = w->ts->fused ? mgf_world::kRbWords : mgf_world::kRbPairStat;
  static_assert(mgf_world::kRbWords < mgf_world::kPinSeqWord, "the sequence word sits behind the block");
  if (w->opt.readback_kernel && w->ts->pin_dev) {
    if (++w->rb_seq == 0u) ++w->rb_seq;
    w->ts->seq = w->rb_seq;
    MGF_TRY(w->sb_grid.ensure(1, s));
    if (defer) {
      defer->rb = w->rb.p; defer->pin = w->ts->pin_dev; defer->words = w->n > 0 ? (uint32_t)rb_words : 0u; defer->seq_word = mgf_world::kPinSeqWord; defer->seq = w->ts->seq;
      defer->sb_words = w->n > 0 ? reinterpret_cast<const uint32_t*>(w->sb.p) : nullptr; defer->grid_words = w->n > 0 ? reinterpret_cast<uint32_t*>(w->sb_grid.p) : nullptr;
    } else {
      k_publish<<<1, kBlock, 0, s>>>(w->rb.p, w->ts->pin_dev, w->n > 0 ? (uint32_t)rb_words : 0u, mgf_world::kPinSeqWord, w->ts->seq,
                                     w->n > 0 ? reinterpret_cast<const uint32_t*>(w->sb.p) : nullptr, w->n > 0 ? reinterpret_cast<uint32_t*>(w->sb_grid.p) : nullptr);
      LAUNCH_CHECK();
    }
    if (w->n > 0 && w->n == w->n_owned) w->sbg_valid = true;  // (the next tick's k_integrate may quantise its cells over these bounds)
    return MGF_OK;
  }
  w->ts->seq = 0;
  if (w->n > 0) MGF_HIP_TRY(hipMemcpyAsync(w->ts->pin, w->rb.p, 4 * rb_words, hipMemcpyDeviceToHost, s));
  MGF_HIP_TRY(hipEventRecord(w->ts->ev[7], s));
  return MGF_OK;
}
// The tick's one wait.  Polling returns a few microseconds sooner than a blocking synchronise wakes up, and the GPU idles until
// the host has enqueued the next tick.  With k_publish the host polls the slot's sequence word in pinned memory; every few thousand
// looks it asks the stream whether it has died or drained without the word.  Without it (a copy command went out): the read-back's event.
static mgf_status readback_wait(mgf_world* w) {
  if (w->ts->seq) {
    const uint32_t want = w->ts->seq;
    volatile uint32_t* word = w->ts->pin + mgf_world::kPinSeqWord;
    for (uint64_t spins = 0;; ++spins) {
      if (__atomic_load_n(const_cast<uint32_t*>(word), __ATOMIC_ACQUIRE) == want) return MGF_OK;
      if ((spins & 0xFFFu) == 0xFFFu) {
        const hipError_t q = hipStreamQuery(w->ctx->stream);
        if (q == hipSuccess) {  // the stream has drained: the word is there, or the launch was lost
          if (__atomic_load_n(const_cast<uint32_t*>(word), __ATOMIC_ACQUIRE) == want) return MGF_OK;
          return fail(MGF_ERR_HIP, "internal error: the tick's read-back did not arrive");
        }
        if (q != hipErrorNotReady) { mgf::set_error("hipStreamQuery failed: %s", hipGetErrorString(q)); return MGF_ERR_HIP; }
      }
    }
  }
  hipError_t q;
  while ((q = hipEventQuery(w->ts->ev[7])) == hipErrorNotReady) {}
  if (q != hipSuccess) { mgf::set_error("hipEventQuery failed: %s", hipGetErrorString(q)); return MGF_ERR_HIP; }
  return MGF_OK;
}
static mgf_status collide_process(mgf_world* w, bool* retry);
static mgf_status collide_finish(mgf_world* w, bool* retry) {
  MGF_TRY(readback_enqueue(w));
  MGF_TRY(readback_wait(w));
  return collide_process(w, retry);
}
static mgf_status collide_process(mgf_world* w, bool* retry) {
  *retry = false;
  if (w->n == 0) { w->constraints_ready = true; return MGF_OK; }
  uint32_t* pin = w->ts->pin;
  StepCounts h = *reinterpret_cast<StepCounts*>(pin + mgf_world::kRbSc);
  w->stats.n_refits = reinterpret_cast<SceneBounds*>(pin + mgf_world::kRbSb)->n_refits;
  w->last_rmax_x = ord_f(reinterpret_cast<SceneBounds*>(pin + mgf_world::kRbSb)->rmax[0]);
  {  // how much of the cell grid the scene covers: every axis gets the same number of cells over a box whose thin axes were widened
     // (grid_box), so a long scene leaves most cells empty - the level rule below counts only the covered part
    const SceneBounds* sbh = reinterpret_cast<SceneBounds*>(pin + mgf_world::kRbSb);
    float e[3], emax = 0.0f;
    for (int k = 0; k < 3; ++k) { e[k] = ord_f(sbh->hi[k]) - ord_f(sbh->lo[k]); emax = std::max(emax, e[k]); w->h_scene_ext[k] = e[k]; w->h_scene_rmax[k] = ord_f(sbh->rmax[k]); }
    const float mf = (float)w->opt.grid_min_frac_pct * 0.01f;
    float occ = 1.0f;
    const uint32_t P = 2u * std::max(w->plan.levels, 4u), nbh[3] = {(P + 2u) / 3u, (P + 1u) / 3u, P / 3u};
    if (emax > 0.0f && mf > 0.0f) for (int k = 0; k < 3; ++k) if (e[k] < mf * emax) {
      const float wide = std::max(e[k], std::min(mf * emax, 1.36f * w->h_scene_rmax[k] * (float)(1u << nbh[k])));  // (grid_box's rule)
      occ *= std::max(e[k], 1e-3f * emax) / wide;
    }
    w->grid_occupancy = (occ > 0.0f && occ <= 1.0f) ? std::max(occ, 0.3f) : 1.0f;  // (at most one level more: config 4's x-slab tiles, 0.29, are at their best level already)
  }
  w->wide_last = w->wide_tick_on ? reinterpret_cast<SceneBounds*>(pin + mgf_world::kRbSb)->pad : 0u;
  w->pair_brick_slow = w->ts->brick ? w->ts->word(kWBrickSlow) : 0;
  if (w->ts->brick) {  // one lane per such query: a few are free, many are not - then k_pair_grid runs, for longer every time this happens
    // (a larger box copy - 1024 records, two blocks per CU - was measured on the settled pile, whose cells hold 1.25 bodies: no faster
    // than k_pair_grid there, 1.536 vs 1.516 ms per tick)
    if (w->pair_brick_slow * 32 > (uint64_t)w->n + 1024) { w->pair_brick_off = w->pair_brick_backoff; w->pair_brick_backoff = std::min(2u * w->pair_brick_backoff, 1u << 20); }
    else w->pair_brick_backoff = 256;
  }
  w->f6_fail_known = w->flow6_prepped; w->f6_fail_host = w->ts->word(kWF6Fail);  // (the preparation ran inside this collide phase)
  w->f6_edges_block = w->flow6_prepped ? w->ts->word(kWF6EdgesBlock) : 0u;
  w->rb_fresh = true;  // solve_flow_finish may read the solver's flags from this copy (async tick: the solver ran before it)
  if (w->ts->word(kWStackOverflow)) return fail(MGF_ERR_CAPACITY, "BVH traversal stack overflow");
  if (w->ts->word(kWBigPartsOverflow)) return fail(MGF_ERR_CAPACITY, "two bodies of many components meet in more than 64 part pairs or a manifold of more than 16 contacts (k_narrow_pairs_big)");
  if (w->ts->word(kWNarrowMismatch)) return fail(MGF_ERR_HIP, "internal error: the broadphase's sphere test and the constraint setup disagree about a contact");
  auto grown = [](uint32_t need) { return (uint32_t)std::min<uint64_t>((uint64_t)need + need / 2 + 1024, 0x7FFFFFF0ull); };
  if (h.fail & kFailSkipped) { *retry = true; return MGF_OK; }  // a speculative tick behind a failed one: the caller re-enqueues it
  if (h.fail & kFailRevRow) { w->rev_cap *= 2; *retry = true; }  // wider rows from now on
  if (h.fail & kFailFlow6) {  // the block-local solver's tables did not fit: its launch did nothing - this tick again with the global dataflow solver
    const uint32_t slots = w->ts->word(kWF6MaxSlots), foreign = w->ts->word(kWF6MaxForeign);
    w->n_flow6_fallbacks++; w->f6_fail_reason = w->ts->word(kWF6Fail);
    w->f6_last_slots = slots; w->f6_last_foreign = foreign;  // (the next tick's LDS split is sized from these)
    w->f6_fail_slots = slots; w->f6_fail_foreign = foreign; w->f6_fail_C = std::max(h.need_C, 1u);  // (... and, while the estimate says no, not tried: flow6_plan)
    w->f6_last_msgs = (uint64_t)w->ts->word(kWF6Edges) * std::max(w->f6_prep_iters, 1u);
    w->f6_last_block_msgs = (uint64_t)w->ts->word(kWF6EdgesBlock) * std::max(w->f6_prep_iters, 1u);
    w->tick_mode1 = true;
    *retry = true;
  }
  if (h.fail & kFailWide) {  // more wide bodies than their list holds: this is no outlier - the tick again without the list, the reference re-learnt
    w->n_wide_overflows++;
    w->wide_engaged = false; w->wide_hold = 64; w->wide_ref[0] = w->wide_ref[1] = w->wide_ref[2] = 0.0f;
    w->invalidate_tick_caches();  // (this tick's bounds left the wide bodies out: the re-run gathers them from the boxes)
    w->wide_tick_on = false;
    *retry = true;
  }
  if (h.fail & kFailTerrainWide) { w->terrain_grid_off = true; *retry = true; }
  else if (h.fail & kFailGridWide) { w->grid_too_wide = true; *retry = true; }
  else if ((h.fail & kFailTerrainRow) && w->ts->front_rows) {  // a body accepts more faces than k_terrain_near lists (kTnHitCap): the list-based kernels from now on
    w->n_row_overflows++;
    w->front_rows_off = true;
    *retry = true;
  }
  else if (h.fail & (kFailRowOverflow | kFailTerrainRow)) {
    w->n_row_overflows++;
    *retry = true;
    if ((h.fail & kFailTerrainRow) && !(h.fail & kFailRowOverflow) && w->row_cap_t < (uint32_t)kRowCapTMax) w->row_cap_t *= 2;  // wider terrain rows from now on
    else w->tick_two_pass = true;  // exact count / fill path for this tick
  }
  if (h.fail & kFailCandCap) {
    if (h.need_Mt > w->cap_t) w->cap_t = grown(h.need_Mt);
    if (h.need_Mp > w->cap_p) w->cap_p = grown(h.need_Mp);
    *retry = true;
  }
  if (h.fail & kFailConsCap) {
    if (h.need_C >= 0x7FFFFFF0u) return fail(MGF_ERR_CAPACITY, "too many constraints");
    w->cap_c = grown(h.need_C);
    *retry = true;
  }
  if (*retry) { w->n_cap_retries++; return MGF_OK; }
  w->n_path_ticks[0] += w->ts->brick; w->n_path_ticks[1] += w->ts->front_rows; w->n_path_ticks[2] += w->ts->contacts_fused; w->n_path_ticks[3] += w->ts->cells_early;
  w->n_split_ticks[0] += w->ts->split_fused; w->n_split_ticks[1] += w->ts->split_alone; w->n_scan_fused_ticks[0] += w->ts->num_fused; w->n_tables_fused_ticks += w->ts->tab_fused;
  w->n_path_ticks[4] += w->ts->two_pass; w->n_path_ticks[5] += w->ts->tree; w->n_path_ticks[6] += w->ts->big_parts;
  if (w->opt.wide_list) {  // the wide bodies' limit for the ticks to come (WideSpec, k_bodies.h)
    if (w->wide_tick_on) {  // (the read-back's rmax is the largest half extent of the bodies that were NOT wide)
      w->n_wide_ticks++;
      for (int k = 0; k < 3; ++k) w->wide_ref[k] = w->h_scene_rmax[k];
      if (w->wide_last == 0) w->wide_engaged = false;
    } else {
      bool jump = false;
      for (int k = 0; k < 3; ++k) {
        // (a world's first reference: its bodies as they were added, at rest - runaways that are there from the first tick are found at once;
        // after a failed tick the scene's own rmax: then it was no outlier)
        if (!(w->wide_ref[k] > 0.0f)) w->wide_ref[k] = (w->shape_rmax[k] > 0.0f && !w->n_wide_overflows) ? std::min(w->shape_rmax[k], w->h_scene_rmax[k]) : w->h_scene_rmax[k];
        jump = jump || w->h_scene_rmax[k] > 1.5f * w->wide_ref[k] + 0.1f;
      }
      if (jump && !w->wide_hold) w->wide_engaged = true;  // (from the next tick on; the reference stays what it was)
      else for (int k = 0; k < 3; ++k) w->wide_ref[k] = std::min(w->h_scene_rmax[k], 1.05f * w->wide_ref[k] + 0.01f);
    }
    // (the reference never follows beyond twice the bodies' extent at rest: a lone body that gains speed tick by tick - one that left the scene
    // and falls - would otherwise take the reference with it; from three times the rest extent on a body is wide whatever the history.  A scene
    // whose bodies all move that fast overflows the list: a re-run every 64 ticks)
    for (int k = 0; k < 3; ++k) if (w->shape_rmax[k] > 0.0f) w->wide_ref[k] = std::min(w->wide_ref[k], 2.0f * w->shape_rmax[k]);
    if (!w->wide_engaged && !w->wide_hold) for (int k = 0; k < 3; ++k) if (w->h_scene_rmax[k] > 1.5f * w->wide_ref[k] + 0.1f) w->wide_engaged = true;
    for (int k = 0; k < 3; ++k) w->wide_limit[k] = 1.5f * w->wide_ref[k] + 0.1f;
    if (w->wide_hold) --w->wide_hold;
  }
  // keep headroom for the next tick (contact counts drift slowly): grow ahead of need, without a re-run
  if ((uint64_t)h.need_Mt * 5 > (uint64_t)w->cap_t * 4) w->cap_t = grown(h.need_Mt);
  if ((uint64_t)h.need_Mp * 5 > (uint64_t)w->cap_p * 4) w->cap_p = grown(h.need_Mp);
  if ((uint64_t)h.need_C * 5 > (uint64_t)w->cap_c * 4) w->cap_c = grown(h.need_C);
  w->Mt = h.Mt; w->Mp = h.Mp; w->C = h.C; w->Ct = h.Ct;
  w->stats.n_terrain_candidates = h.Mt; w->stats.n_pair_candidates = h.Mp;
  if (w->ts->fused) {  // the candidate lists hold contacts only; the accepted partners were counted on the way
    uint64_t acc = 0;
    for (uint32_t k = 0; k < kPairStatWords; ++k) acc += pin[mgf_world::kRbPairStat + k];
    w->stats.n_pair_candidates = acc;
  }
  if (w->demo_rows_ready) w->stats.n_pair_candidates = w->demo_candidates;
  w->stats.n_constraints = h.C; w->stats.n_terrain_constraints = h.Ct;
  w->stats.n_ghost_constraints = w->ts->word(kWGhostCons);
  w->constraints_ready = true;
  float ms;
  MGF_TRY(phase_ms(w, 0, 1, &ms)); w->stats.ms_integrate = ms;
  MGF_TRY(phase_ms(w, 1, 2, &ms)); w->stats.ms_broadphase = ms;
  MGF_TRY(phase_ms(w, 2, 3, &ms)); w->stats.ms_narrowphase = ms;
  MGF_TRY(phase_ms(w, 3, 4, &ms)); w->stats.ms_setup = ms;
  return MGF_OK;
}

extern "C" mgf_status mgf_world_collide(mgf_world* w, float dt, mgf_step_stats* stats) {
  if (!w) return fail(MGF_ERR_INVALID, "world is NULL");
  MGF_TRY(ctx_bind(w->ctx));
  w->constraints_ready = false;
  w->C = w->Ct = w->Mt = w->Mp = 0;
  for (int attempt = 0; attempt < 8; ++attempt) {
    bool retry = false;
    MGF_TRY(collide_enqueue(w, dt, true));  // (a solve call usually follows: its preparation counters are cleared on the way)
    MGF_TRY(collide_finish(w, &retry));
    if (!retry) { if (stats) *stats = w->stats; return MGF_OK; }
  }
  return fail(MGF_ERR_HIP, "internal error: collide phase did not settle its buffer capacities");
}

extern "C" mgf_status mgf_world_build_constraints(mgf_world* w, float dt, mgf_step_stats* stats) {
  MGF_TRY(world_begin(w, dt, false, true));
  if (w->opt.constraint_order == 1) MGF_TRY(demo_rows(w));
  return mgf_world_collide(w, dt, stats);
}
