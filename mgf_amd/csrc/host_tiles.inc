// Spatial tiling: boundary selection, ghost records, migration of bodies between tiles.
// Part of the single translation unit mgf_hip.hip (included there, in order); not compiled on its own.
// One launch of a tile-protocol kernel per kTileBatch tiles (k_tiles.h): blockIdx.y = the tile, grid.x = what the largest tile of the batch needs.
template <class Batch, class Tile>
static mgf_status tile_batches(hipStream_t s, void (*kern)(Batch), const Tile* tiles, const uint32_t* blocks, int L) {
  for (int i0 = 0; i0 < L; i0 += kTileBatch) {
    Batch A;
    memset(&A, 0, sizeof(A));
    const int cnt = std::min(kTileBatch, L - i0);
    uint32_t mx = 0;
    for (int k = 0; k < cnt; ++k) { A.t[k] = tiles[i0 + k]; mx = std::max(mx, blocks[i0 + k]); }
    if (!mx) continue;
    kern<<<dim3(mx, (unsigned)cnt), kBlock, 0, s>>>(A);
    LAUNCH_CHECK();
  }
  return MGF_OK;
}
// The selection of a tile's boundary bodies and migrants (k_tile_select_*): `sel` describes every tile (n > 0); `scatter` = the id lists are
// written as well (their buffers hold n ids each: nothing needs the counts first).  The totals are in each tile's SelTile::tot afterwards.
static mgf_status select_describe(mgf_world* w, float x_left, float x_right, float x_lo, float x_hi, uint32_t* ids_l, uint32_t* ids_r, uint32_t* ids_m, SelTile* S) {
  const uint32_t n = w->n_owned, nb = nblk(n);
  MGF_TRY(w->sel_blk.ensure(4 * (size_t)nb + 4, w->ctx->stream));
  S->fb_c = w->fb_c.p; S->fb_r = w->fb_r.p; S->x = w->x.p; S->n = n;
  S->x_left = x_left; S->x_right = x_right; S->x_lo = x_lo; S->x_hi = x_hi;
  S->blk = w->sel_blk.p; S->tot = w->sel_blk.p + 4 * (size_t)nb; S->tot_host = nullptr;
  S->ids_l = ids_l; S->ids_r = ids_r; S->ids_m = ids_m;
  return MGF_OK;
}
static mgf_status select_counts(hipStream_t s, const SelTile* sel, int L) {
  std::vector<uint32_t> blocks((size_t)L);
  for (int i = 0; i < L; ++i) blocks[(size_t)i] = nblk(sel[i].n);
  MGF_TRY((tile_batches<SelBatch, SelTile>(s, k_tile_select_count, sel, blocks.data(), L)));
  for (int i0 = 0; i0 < L; i0 += kTileBatch) {
    SelBatch A;
    memset(&A, 0, sizeof(A));
    const int cnt = std::min(kTileBatch, L - i0);
    for (int k = 0; k < cnt; ++k) A.t[k] = sel[i0 + k];
    k_tile_select_offsets<<<cnt, kSelScanThreads, 0, s>>>(A);
    LAUNCH_CHECK();
  }
  return MGF_OK;
}
static mgf_status select_scatter(hipStream_t s, const SelTile* sel, int L) {
  std::vector<uint32_t> blocks((size_t)L);
  for (int i = 0; i < L; ++i) blocks[(size_t)i] = nblk(sel[i].n);
  return tile_batches<SelBatch, SelTile>(s, k_tile_select_scatter, sel, blocks.data(), L);
}
extern "C" mgf_status mgf_world_select_tile(mgf_world* w, float x_left, float x_right, float x_lo, float x_hi, uint32_t* ids_left,
                                            uint32_t* ids_right, uint32_t* ids_migrants, int64_t cap, int64_t* counts);
extern "C" mgf_status mgf_world_select_boundary(mgf_world* w, float x_left, float x_right, uint32_t* ids_left, uint32_t* ids_right,
                                                int64_t cap, int64_t* n_left, int64_t* n_right) {
  if (!w || !n_left || !n_right) return fail(MGF_ERR_INVALID, "NULL argument");
  int64_t counts[4] = {0, 0, 0, 0};
  const mgf_status st = mgf_world_select_tile(w, x_left, x_right, -3.0e38f, 3.0e38f, ids_left, ids_right, nullptr, cap, counts);
  *n_left = counts[0]; *n_right = counts[1];
  return st;
}
extern "C" mgf_status mgf_world_export_bodies(mgf_world* w, const uint32_t* ids, int64_t n, float* dst) {
  if (!w || (n && (!ids || !dst))) return fail(MGF_ERR_INVALID, "NULL argument");
  if (w->max_parts > (uint32_t)kTileParts) return fail(MGF_ERR_INVALID, "bodies of more than four parts cannot cross tiles (the tile records carry four part slots)");
  MGF_TRY(ctx_bind(w->ctx));
  MGF_TRY(world_identity(w));  // (bodies are named by the caller's indices here: host_perm.inc)
  if (n > 0) {
    ExpTile E;
    E.B = w->bodies(); E.ids_l = ids; E.ids_r = nullptr; E.nl = (uint32_t)n; E.nr = 0; E.out = dst; E.rec = (uint32_t)kGhostFloats; E.pad = 0;
    const uint32_t blocks = nblk(n);
    MGF_TRY((tile_batches<ExpBatch, ExpTile>(w->ctx->stream, k_export_bodies, &E, &blocks, 1)));
  }
  return sync_unless_ordered(w);
}
template <class T>
static mgf_status grow_keep(mgf_world* w, DBuf<T>& b, size_t per, size_t need) {
  return b.ensure(per * need, w->ctx->stream, true, per * (size_t)w->n_owned);
}
// the part arrays of a world that holds (or may receive) bodies of several components
static mgf_status grow_parts(mgf_world* w, size_t need) {
  if (!w->has_compound) return MGF_OK;
  MGF_TRY(grow_keep(w, w->pcount, 1, need));
  MGF_TRY(grow_keep(w, w->lp0, kMaxParts, need)); MGF_TRY(grow_keep(w, w->lp1, kMaxParts, need));
  MGF_TRY(grow_keep(w, w->wp0, kMaxParts, need)); MGF_TRY(grow_keep(w, w->wp1, kMaxParts, need));
  return MGF_OK;
}
// What arrives through the plain C API (mgf_world_import_ghosts / import_migrants without the tile set's announcement of kinds) may be of
// more parts than this world has slots for - none at all in a world of ordinary bodies: the records' part counts are read first and the
// world is raised to them (option body_kinds does exactly this), so that no part is dropped on the way in (ADVICE r4).
static mgf_status raise_parts_for_records(mgf_world* w, const float* rec, int64_t m, uint32_t stride_floats, uint32_t at) {
  if (m <= 0 || !rec) return MGF_OK;
  MGF_TRY(w->mig_cnt.ensure(2, w->ctx->stream));
  MGF_HIP_TRY(hipMemsetAsync(w->mig_cnt.p, 0, 8, w->ctx->stream));
  k_record_max_parts<<<nblk(m), kBlock, 0, w->ctx->stream>>>(rec, (uint32_t)m, stride_floats, at, w->mig_cnt.p);
  LAUNCH_CHECK();
  uint32_t pc = 0;
  MGF_TRY(d2h(w->ctx, &pc, w->mig_cnt.p, 1));
  if (pc > (uint32_t)kTileParts) return fail(MGF_ERR_INVALID, "a record claims more parts than a tile record carries");
  if (pc > 2u && w->max_parts <= 2u) return mgf_world_set_option(w, "body_kinds", 12);
  if (pc > 0u && !w->has_compound) return mgf_world_set_option(w, "body_kinds", 4);
  return MGF_OK;
}
// (src2 / n_first: the rows from n_first on come from src2 - mgf_tiles_step hands a tile its two neighbours' send buffers as they are)
static mgf_status world_import_ghosts2(mgf_world* w, const float* src, int64_t n_ghost, const float* src2, int64_t n_first);
extern "C" mgf_status mgf_world_import_ghosts(mgf_world* w, const float* src, int64_t n_ghost) {
  // (a stream-ordered world belongs to a tile driver, which announces its neighbours' kinds - option body_kinds - and must not be made to wait here)
  if (w && src && n_ghost > 0 && !w->opt.stream_ordered) { MGF_TRY(ctx_bind(w->ctx)); MGF_TRY(raise_parts_for_records(w, src, n_ghost, (uint32_t)kGhostFloats, 36u)); }
  return world_import_ghosts2(w, src, n_ghost, nullptr, n_ghost);
}
// (the host half: room for the ghosts, what the tick's caches cover afterwards; `I` = what k_import_ghosts needs, I->m == 0: nothing to launch)
static mgf_status world_import_ghosts_prepare(mgf_world* w, const float* src, int64_t n_ghost, const float* src2, int64_t n_first, ImpTile* I) {
  memset(I, 0, sizeof(*I));
  if (w) w->sbg_valid = false;
  if (!w || (n_ghost && !src && !src2) || n_ghost < 0 || n_first < 0 || (n_first < n_ghost && !src2) || (n_first > 0 && n_ghost > 0 && !src)) return fail(MGF_ERR_INVALID, "bad argument");
  MGF_TRY(ctx_bind(w->ctx));
  MGF_TRY(world_identity(w));  // (bodies are named by the caller's indices here: host_perm.inc)
  size_t need = (size_t)w->n_owned + (size_t)n_ghost;
  if (need > 0x7FFFFFF0ull) return fail(MGF_ERR_INVALID, "too many bodies");
  MGF_TRY(grow_keep(w, w->x, 1, need)); MGF_TRY(grow_keep(w, w->q, 1, need)); MGF_TRY(grow_keep(w, w->srec, 4, need));
  MGF_TRY(grow_keep(w, w->sp0, 1, need)); MGF_TRY(grow_keep(w, w->sp1, 1, need)); MGF_TRY(grow_keep(w, w->ctor, 1, need));
  MGF_TRY(grow_keep(w, w->imb, 3, need)); MGF_TRY(grow_keep(w, w->delta, 1, need)); MGF_TRY(grow_keep(w, w->einfo, 1, need));
  MGF_TRY(grow_keep(w, w->col0, 1, need)); MGF_TRY(grow_keep(w, w->col1, 1, need)); MGF_TRY(grow_keep(w, w->tb_c, 1, need));
  MGF_TRY(grow_keep(w, w->tb_r, 1, need)); MGF_TRY(grow_keep(w, w->fb_c, 1, need)); MGF_TRY(grow_keep(w, w->fb_r, 1, need));
  MGF_TRY(grow_parts(w, need));
  MGF_TRY(grow_keep(w, w->bpk, 4, need));
  w->pack_cover = (w->pack_cover >= w->n_owned && w->n_owned > 0) ? (uint32_t)need : 0u;  // k_import_ghosts writes the ghosts' packed records
  if (n_ghost > 0) {
    // the scene bounds gathered by this tick's k_integrate take the ghosts in (only straight after it: n == n_owned == bounds_cover)
    const bool join = w->bounds_cover == w->n_owned && w->n == w->n_owned && w->n_owned > 0;
    I->B = w->bodies(); I->n_owned = w->n_owned; I->m = (uint32_t)n_ghost; I->m1 = (uint32_t)std::min<int64_t>(n_first, n_ghost);
    I->fat_margin = w->params.fat_margin; I->in = src; I->in2 = src2; I->sb_part = join ? w->sb_part.p : nullptr;
    I->rec1 = I->rec2 = (uint32_t)kGhostFloats;  // (the C-ABI's width; mgf_tiles_step sets the widths its neighbours announced)
    w->bounds_cover = join ? (uint32_t)need : 0u;
  } else if (w->n != w->n_owned) {
    w->bounds_cover = 0;  // the ghosts of an earlier import are dropped
  }
  w->n = (uint32_t)need;
  w->constraints_ready = false;
  return MGF_OK;
}
static mgf_status world_import_ghosts2(mgf_world* w, const float* src, int64_t n_ghost, const float* src2, int64_t n_first) {
  ImpTile I;
  MGF_TRY(world_import_ghosts_prepare(w, src, n_ghost, src2, n_first, &I));
  const uint32_t blocks = nblk(I.m);
  MGF_TRY((tile_batches<ImpBatch, ImpTile>(w->ctx->stream, k_import_ghosts, &I, &blocks, 1)));
  return sync_unless_ordered(w);
}
// ---- migration of owned bodies between tiles (SURVEY.md §8e) ---------------------------------------
// mgf_world_select_tile = select_boundary + the bodies whose centre left the slab [x_lo, x_hi).  The common tick has
// no migrant: its cost over select_boundary is one counting kernel, and the counts ride on the same read-back.
extern "C" mgf_status mgf_world_select_tile(mgf_world* w, float x_left, float x_right, float x_lo, float x_hi, uint32_t* ids_left,
                                            uint32_t* ids_right, uint32_t* ids_migrants, int64_t cap, int64_t* counts) {
  if (!w || !counts) return fail(MGF_ERR_INVALID, "NULL argument");
  MGF_TRY(ctx_bind(w->ctx));
  MGF_TRY(world_identity(w));  // (bodies are named by the caller's indices here: host_perm.inc)
  mgf_ctx* ctx = w->ctx;
  hipStream_t s = ctx->stream;
  counts[0] = counts[1] = counts[2] = counts[3] = 0;
  if (w->n_owned == 0) return MGF_OK;
  SelTile S;
  MGF_TRY(select_describe(w, x_left, x_right, x_lo, x_hi, ids_left, ids_right, ids_migrants, &S));
  MGF_TRY(select_counts(s, &S, 1));
  uint32_t* pin = static_cast<uint32_t*>(ctx->pinned);
  MGF_HIP_TRY(hipMemcpyAsync(pin, S.tot, 16, hipMemcpyDeviceToHost, s));
  MGF_HIP_TRY(hipStreamSynchronize(s));
  const uint32_t nl = pin[0], nr = pin[1], ml = pin[2], mr = pin[3];
  counts[0] = nl; counts[1] = nr; counts[2] = ml; counts[3] = mr;
  // (the caller's buffers hold `cap` ids: the lists are written only once the counts are known to fit)
  if ((int64_t)nl > cap || (int64_t)nr > cap || (int64_t)ml + (int64_t)mr > cap) return fail(MGF_ERR_CAPACITY, "id buffers too small");
  if (!ids_left || !ids_right) return fail(MGF_ERR_INVALID, "NULL id buffer");
  if ((ml + mr) && !ids_migrants) return fail(MGF_ERR_INVALID, "NULL migrant id buffer");
  MGF_TRY(select_scatter(s, &S, 1));
  return sync_unless_ordered(w);
}
extern "C" mgf_status mgf_world_export_migrants(mgf_world* w, const uint32_t* ids, int64_t n, float* dst) {
  if (!w || n < 0 || (n && (!ids || !dst))) return fail(MGF_ERR_INVALID, "bad argument");
  if (w->max_parts > (uint32_t)kTileParts) return fail(MGF_ERR_INVALID, "bodies of more than four parts cannot cross tiles (the tile records carry four part slots)");
  MGF_TRY(ctx_bind(w->ctx));
  MGF_TRY(world_identity(w));  // (bodies are named by the caller's indices here: host_perm.inc)
  if (n > 0) {
    k_export_migrants<<<nblk((size_t)n * kMigrantWords), kBlock, 0, w->ctx->stream>>>(w->bodies(), ids, (uint32_t)n, reinterpret_cast<float4*>(dst), kTileParts);
    LAUNCH_CHECK();
  }
  return sync_unless_ordered(w);
}
// Removes the listed owned bodies (distinct ids, any order); the others keep their relative order, so ids above a
// removed one shift down.  Ghosts of the current tick are dropped.
// `trusted` (mgf_tiles_step: the ids are the tile's own migrant list, built on the device - distinct and in range by construction):
// nothing is read back and nothing waits; the caller's next synchronisation covers the launches.
static mgf_status remove_bodies_impl(mgf_world* w, const uint32_t* ids, int64_t n_ids, bool trusted) {
  if (!w || n_ids < 0 || (n_ids && !ids)) return fail(MGF_ERR_INVALID, "bad argument");
  w->invalidate_tick_caches();  // (bounds / terrain rows gathered by k_integrate no longer describe the bodies)
  MGF_TRY(ctx_bind(w->ctx));
  MGF_TRY(world_identity(w));  // (bodies are named by the caller's indices here: host_perm.inc)
  mgf_ctx* ctx = w->ctx;
  hipStream_t s = ctx->stream;
  const uint32_t n = w->n_owned;
  w->n = n;
  w->constraints_ready = false;
  if (n_ids == 0) return MGF_OK;
  if ((uint64_t)n_ids > n) return fail(MGF_ERR_INVALID, "more ids than bodies");
  w->sbg_valid = false; w->ptrs_out = false;  // (from here on the arrays are compacted: raw pointers handed out die with them)
  MGF_TRY(w->bflag_l.ensure(n + 1, s)); MGF_TRY(w->bscan_l.ensure(n + 1, s));
  MGF_TRY(w->mig_cnt.ensure(2, s));
  MGF_TRY(w->mig_tmp.ensure((size_t)n * kBodyWords, s));
  MGF_HIP_TRY(hipMemsetAsync(w->mig_cnt.p, 0, 8, s));
  if ((uint64_t)n_ids <= kRemoveShort) {  // a handful (a tile's hand-over): where every body goes, in one launch
    k_remove_positions_short<<<nblk(n + 1), kBlock, 0, s>>>(ids, (uint32_t)n_ids, n, w->bscan_l.p, w->mig_cnt.p);
    LAUNCH_CHECK();
  } else {
    k_keep_fill<<<nblk(n + 1), kBlock, 0, s>>>(w->bflag_l.p, n);
    LAUNCH_CHECK();
    k_keep_clear<<<nblk(n_ids), kBlock, 0, s>>>(w->bflag_l.p, ids, (uint32_t)n_ids, n, w->mig_cnt.p);
    LAUNCH_CHECK();
    // positions of the kept bodies (k_flag_*: no library call between the launches - the stream stays fed)
    const uint32_t nb = nblk(n + 1);
    MGF_TRY(w->sel_blk.ensure(4 * (size_t)nb + 4, s));
    k_flag_count<<<nb, kBlock, 0, s>>>(w->bflag_l.p, n + 1, w->sel_blk.p);
    LAUNCH_CHECK();
    k_flag_offsets<<<1, kSelScanThreads, 0, s>>>(w->sel_blk.p, nb);
    LAUNCH_CHECK();
    k_flag_positions<<<nb, kBlock, 0, s>>>(w->bflag_l.p, n + 1, w->sel_blk.p, w->bscan_l.p);
    LAUNCH_CHECK();
  }
  const unsigned row_words = w->has_compound ? (unsigned)kBodyWords : 20u;  // (words 20.. are the part arrays')
  k_compact_gather<<<dim3(nblk(n), row_words), kBlock, 0, s>>>(w->bodies(), n, w->bscan_l.p, w->mig_tmp.p);
  LAUNCH_CHECK();
  if (!trusted) {
    uint32_t* pin = static_cast<uint32_t*>(ctx->pinned);
    MGF_HIP_TRY(hipMemcpyAsync(pin, w->mig_cnt.p, 4, hipMemcpyDeviceToHost, s));
    MGF_HIP_TRY(hipStreamSynchronize(s));
    if (pin[0]) return fail(MGF_ERR_INVALID, "remove_bodies: an id is out of range or listed twice");
  }
  const uint32_t n_new = n - (uint32_t)n_ids;
  if (n_new) {
    k_compact_put<<<dim3(nblk(n_new), row_words), kBlock, 0, s>>>(w->bodies(), n, n_new, w->bscan_l.p, w->mig_tmp.p);
    LAUNCH_CHECK();
  }
  w->n_owned = w->n = n_new;
  w->stats.n_bodies = n_new;
  w->sidx_valid = false;
  w->demo_tree.clear(); w->demo_leaf.clear();  // (the world.rs replay's tree names the old indices: rebuilt from the fat boxes at the next tick)
  return sync_unless_ordered(w);
}
extern "C" mgf_status mgf_world_remove_bodies(mgf_world* w, const uint32_t* ids, int64_t n_ids) { return remove_bodies_impl(w, ids, n_ids, false); }
// Appends bodies exported by another world's mgf_world_export_migrants as owned bodies (ghosts are dropped).
// `kinds_hint` (mgf_tiles_step: the kinds of bodies the sending tile holds, bit 0 spheres, bit 1 capsules - the tiles tell each other): the
// arrivals' kinds are taken from it instead of being read back (a superset only costs the choice of a more general kernel).
static mgf_status import_migrants_impl(mgf_world* w, const float* src, int64_t n_in, uint32_t kinds_hint, const float* src2 = nullptr, int64_t n_first = -1) {
  if (n_first < 0 || n_first > n_in) n_first = n_in;  // (src2 / n_first: the records from n_first on come from src2 - with a kinds hint only)
  if (!w || n_in < 0 || (n_first > 0 && !src) || (n_first < n_in && (!src2 || !kinds_hint))) return fail(MGF_ERR_INVALID, "bad argument");
  w->invalidate_tick_caches();  // (bounds / terrain rows gathered by k_integrate no longer describe the bodies)
  MGF_TRY(ctx_bind(w->ctx));
  MGF_TRY(world_identity(w));  // (bodies are named by the caller's indices here: host_perm.inc)
  w->n = w->n_owned;
  w->constraints_ready = false;
  if (n_in == 0) return MGF_OK;
  size_t need = (size_t)w->n_owned + (size_t)n_in;
  if (need > 0x7FFFFFF0ull) return fail(MGF_ERR_INVALID, "too many bodies");
  w->sbg_valid = false; w->ptrs_out = false;  // (from here on the arrays grow: raw pointers handed out die with them)
  if (!kinds_hint) MGF_TRY(raise_parts_for_records(w, src, n_in, 4u * (uint32_t)kMigrantWords, 4u * 20u));  // (word 20 of a migrant record: the part count)
  MGF_TRY(grow_keep(w, w->x, 1, need)); MGF_TRY(grow_keep(w, w->q, 1, need)); MGF_TRY(grow_keep(w, w->srec, 4, need));
  MGF_TRY(grow_keep(w, w->sp0, 1, need)); MGF_TRY(grow_keep(w, w->sp1, 1, need)); MGF_TRY(grow_keep(w, w->ctor, 1, need));
  MGF_TRY(grow_keep(w, w->imb, 3, need)); MGF_TRY(grow_keep(w, w->delta, 1, need)); MGF_TRY(grow_keep(w, w->einfo, 1, need));
  MGF_TRY(grow_keep(w, w->col0, 1, need)); MGF_TRY(grow_keep(w, w->col1, 1, need)); MGF_TRY(grow_keep(w, w->tb_c, 1, need));
  MGF_TRY(grow_keep(w, w->tb_r, 1, need)); MGF_TRY(grow_keep(w, w->fb_c, 1, need)); MGF_TRY(grow_keep(w, w->fb_r, 1, need));
  MGF_TRY(grow_parts(w, need));
  k_import_migrants<<<nblk((size_t)n_in * kMigrantWords), kBlock, 0, w->ctx->stream>>>(w->bodies(), w->n_owned, (uint32_t)n_in,
                                                                                      reinterpret_cast<const float4*>(src), kTileParts,
                                                                                      reinterpret_cast<const float4*>(src2), (uint32_t)n_first);
  LAUNCH_CHECK();
  w->n_owned = w->n = (uint32_t)need;
  w->stats.n_bodies = w->n_owned;
  w->sidx_valid = false;
  // the arrivals may be of a kind this tile has not seen yet (the narrowphase dispatch is chosen on the host)
  if (kinds_hint) {
    if (kinds_hint & 1u) w->has_sphere = true;
    if (kinds_hint & 2u) w->has_capsule = true;
    return MGF_OK;
  }
  MGF_TRY(w->mig_cnt.ensure(2, w->ctx->stream));
  MGF_HIP_TRY(hipMemsetAsync(w->mig_cnt.p, 0, 8, w->ctx->stream));
  k_kind_mask<<<nblk(n_in), kBlock, 0, w->ctx->stream>>>(w->col1.p, w->has_compound ? w->pcount.p : nullptr, w->n_owned - (uint32_t)n_in, (uint32_t)n_in, w->mig_cnt.p);
  LAUNCH_CHECK();
  uint32_t mask = 0;
  MGF_TRY(d2h(w->ctx, &mask, w->mig_cnt.p, 1));
  if (mask & 1) w->has_sphere = true;
  if (mask & 2) w->has_capsule = true;
  return MGF_OK;
}
extern "C" mgf_status mgf_world_import_migrants(mgf_world* w, const float* src, int64_t n_in) { return import_migrants_impl(w, src, n_in, 0u); }
// A caller-defined 32-bit tag per body (kept in the constructor record, travels with a migrant): the tiles driver
// stores the body's global id in it.
extern "C" mgf_status mgf_world_set_tags(mgf_world* w, const uint32_t* tags, int64_t n) {
  if (!w || (n && !tags)) return fail(MGF_ERR_INVALID, "NULL argument");
  if ((uint64_t)n != (uint64_t)w->n_owned) return fail(MGF_ERR_INVALID, "one tag per owned body");
  MGF_TRY(ctx_bind(w->ctx));
  if (n == 0) return MGF_OK;
  MGF_TRY(w->bflag_l.ensure((size_t)n + 1, w->ctx->stream));
  if (w->permuted) {  // the store stays in its internal order: body i's tag goes to slot_of[i] (as mgf_world_write_state does)
    MGF_TRY(perm_host(w));
    std::vector<uint32_t> t((size_t)n);
    for (size_t i = 0; i < (size_t)n; ++i) t[w->h_slot_of[i]] = tags[i];
    MGF_TRY(h2d(w->ctx, w->bflag_l.p, t.data(), (size_t)n));
  } else {
    MGF_TRY(h2d(w->ctx, w->bflag_l.p, tags, (size_t)n));
  }
  k_tags_set<<<nblk(n), kBlock, 0, w->ctx->stream>>>(w->ctor.p, w->bflag_l.p, (uint32_t)n);
  LAUNCH_CHECK();
  MGF_HIP_TRY(hipStreamSynchronize(w->ctx->stream));
  return MGF_OK;
}
extern "C" mgf_status mgf_world_read_tags(mgf_world* w, uint32_t* tags, int64_t cap) {
  if (!w || (cap && !tags)) return fail(MGF_ERR_INVALID, "NULL argument");
  if ((uint64_t)cap < (uint64_t)w->n_owned) return fail(MGF_ERR_CAPACITY, "tag buffer too small");
  MGF_TRY(ctx_bind(w->ctx));
  const uint32_t n = w->n_owned;
  if (n == 0) return MGF_OK;
  MGF_TRY(w->bflag_l.ensure((size_t)n + 1, w->ctx->stream));
  k_tags_get<<<nblk(n), kBlock, 0, w->ctx->stream>>>(w->ctor.p, w->bflag_l.p, n);
  LAUNCH_CHECK();
  if (!w->permuted) return d2h(w->ctx, tags, w->bflag_l.p, (size_t)n);
  MGF_TRY(perm_host(w));
  std::vector<uint32_t> h(n);
  MGF_TRY(d2h(w->ctx, h.data(), w->bflag_l.p, (size_t)n));
  for (uint32_t e = 0; e < n; ++e) tags[e] = h[w->h_slot_of[e]];
  return MGF_OK;
}
extern "C" mgf_status mgf_world_export_velocities(mgf_world* w, const uint32_t* ids, int64_t n, float* dst) {
  if (!w || (n && (!ids || !dst))) return fail(MGF_ERR_INVALID, "NULL argument");
  MGF_TRY(ctx_bind(w->ctx));
  MGF_TRY(world_identity(w));  // (bodies are named by the caller's indices here: host_perm.inc)
  if (n > 0) {
    VelTile V;
    V.srec = w->srec.p; V.ids_l = ids; V.ids_r = nullptr; V.nl = (uint32_t)n; V.nr = 0; V.out = reinterpret_cast<float4*>(dst); V.rec = kVelFloats; V.pad = 0;
    const uint32_t blocks = nblk(n);
    MGF_TRY((tile_batches<VelBatch, VelTile>(w->ctx->stream, k_export_vel, &V, &blocks, 1)));
  }
  return sync_unless_ordered(w);
}
// (the checks of an import of ghost velocities; G->m == 0: nothing to launch)
static mgf_status world_import_ghost_velocities_prepare(mgf_world* w, const float* src, int64_t n_ghost, const float* src2, int64_t n_first, GVelTile* G) {
  memset(G, 0, sizeof(*G));
  if (!w || (n_ghost && !src && !src2) || n_first < 0 || (n_first < n_ghost && !src2) || (n_first > 0 && n_ghost > 0 && !src)) return fail(MGF_ERR_INVALID, "NULL argument");
  MGF_TRY(ctx_bind(w->ctx));
  MGF_TRY(world_identity(w));  // (bodies are named by the caller's indices here: host_perm.inc)
  if ((uint64_t)n_ghost != (uint64_t)(w->n - w->n_owned)) return fail(MGF_ERR_INVALID, "ghost count mismatch");
  if (n_ghost > 0) {
    G->srec = w->srec.p; G->n_owned = w->n_owned; G->m = (uint32_t)n_ghost; G->m1 = (uint32_t)std::min<int64_t>(n_first, n_ghost);
    G->in = reinterpret_cast<const float4*>(src); G->in2 = reinterpret_cast<const float4*>(src2); G->rec = kVelFloats;  // (mgf_tiles_step: kVelFloatsPacked)
  }
  return MGF_OK;
}
extern "C" mgf_status mgf_world_import_ghost_velocities(mgf_world* w, const float* src, int64_t n_ghost) {
  GVelTile G;
  MGF_TRY(world_import_ghost_velocities_prepare(w, src, n_ghost, nullptr, n_ghost, &G));
  const uint32_t blocks = nblk(G.m);
  MGF_TRY((tile_batches<GVelBatch, GVelTile>(w->ctx->stream, k_import_ghost_vel, &G, &blocks, 1)));
  return sync_unless_ordered(w);
}
extern "C" int64_t mgf_world_ghost_len(const mgf_world* w) { return w ? (int64_t)(w->n - w->n_owned) : 0; }
