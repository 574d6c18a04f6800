// The body store in an internal (cell) order.  Part of the single translation unit mgf_hip.hip (included there, in order).
//
// Every list of the tick is spatial - cells, candidate rows, blocks of the solver - while the caller's body indices are whatever
// the caller chose (BASELINE config 2 shuffles them on purpose: SURVEY.md 8d).  With the RigidBodyVec stored in the caller's order,
// every kernel behind the cell sort reaches its bodies through scattered 4..64-byte look-ups (round 2: the solver preparation moved
// ten times its algorithmic bytes).  So the fused tick (mgf_world_step / mgf_world_step_many) keeps the store in CELL ORDER:
//   * slot s of every Bodies array holds the caller's body ext_of[s]; slot_of is the inverse.  Every few ticks (option
//     "resort_every") the rows are moved into the order of the last tick's cell sort (sidx) - between two re-sorts bodies drift a
//     little out of place, which costs locality, never correctness: the cell sort of every tick still runs;
//   * body indices inside the tick (candidate rows, constraint records, solver tables) are SLOTS;
//   * everything that decides an ORDER uses the caller's index (the "order id", k_broadphase.h): the `j < i` filter of
//     world.rs:266, the ascending-partner order of a body's own constraints, the order of the constraints a body takes part in as
//     `b` (k_count_contacts, k_chain_rows, k_flow6_links).  The Gauss-Seidel sequence - which constraint follows which on every
//     body - is therefore exactly that of the caller's order, and the result bit-identical to it, whatever the slots are;
//   * constraint ids follow the slots (a body's own constraints are contiguous, bodies in slot order), so they are NOT the
//     insertion order any more: mgf_world_read_constraints restores it on the way out;
//   * the boundary maps: state reads, get / set, colliders, tags and the constraint read-back translate through slot_of / ext_of;
//     every other entry point that names bodies by index (adding and removing bodies, caller-built constraint lists, the tiling calls,
//     the world.rs replay) first puts the store back into the caller's order (world_identity).
// A re-sort is a relabelling: it commutes with the tick as long as nothing indexed by the old slots outlives it.  It runs at the
// start of a tick (world_begin), where the previous tick's lists are dead, and ahead of k_integrate, whose by-products (terrain
// rows, packed records) are therefore in the new order; sidx itself dies with it (sidx_valid) until the collide phase rebuilds it.

static mgf_status perm_host(mgf_world* w) {  // host copies of ext_of / slot_of, fetched when a boundary call needs them
  if (!w->permuted || w->h_perm_valid) return MGF_OK;
  const size_t n = w->n_owned;
  w->h_ext_of.resize(n); w->h_slot_of.resize(n);
  MGF_TRY(d2h(w->ctx, w->h_ext_of.data(), w->ext_of.p, n));
  for (size_t s = 0; s < n; ++s) w->h_slot_of[w->h_ext_of[s]] = (uint32_t)s;
  w->h_perm_valid = true;
  return MGF_OK;
}
// rows of the new slots k = rows of the old slots order[k]; `order` is a device array of n_owned distinct slots
static mgf_status perm_apply(mgf_world* w, const uint32_t* order, bool to_identity) {
  mgf_ctx* ctx = w->ctx;
  hipStream_t s = ctx->stream;
  const uint32_t n = w->n_owned;
  const uint32_t words = w->has_compound ? (uint32_t)kBodyWords : 20u;  // (words 20.. are the part arrays)
  MGF_TRY(w->perm_tmp.ensure((size_t)words * n, s));
  const dim3 grid(nblk(n), words);
  k_permute_gather<<<grid, kBlock, 0, s>>>(w->bodies(), n, order, w->perm_tmp.p);
  LAUNCH_CHECK();
  if (!to_identity) {
    MGF_TRY(w->ext_new.ensure(n, s)); MGF_TRY(w->slot_of.ensure(n, s));
    k_permute_ids<<<nblk(n), kBlock, 0, s>>>(n, order, w->permuted ? w->ext_of.p : nullptr, w->ext_new.p, w->slot_of.p);
    LAUNCH_CHECK();
    std::swap(w->ext_of.p, w->ext_new.p); std::swap(w->ext_of.cap, w->ext_new.cap);
  }
  k_permute_put<<<grid, kBlock, 0, s>>>(w->bodies(), n, w->perm_tmp.p);
  LAUNCH_CHECK();
  w->permuted = !to_identity;
  w->h_perm_valid = false;
  w->sidx_valid = false;           // (it names the old slots)
  w->ticks_since_resort = 0;
  w->n_resorts++;
  return MGF_OK;
}
// The order of a re-sort that serves the block-local solver best: its blocks are runs of `nb` slots, and what a block costs is its
// SURFACE - every body pair across a block face is a message and a slow hop of the dependency graph.  Runs of a space-filling
// curve over the cell grid are ragged (18 % of a settled pile's pairs cross a face); here the bodies are cut into near-cubic boxes
// holding exactly nb bodies each: x slabs, y rows inside a slab, z columns inside a row, every cut by COUNT (three radix sorts,
// the unit of the level above in the key's high bits).  The fan-outs follow the scene's shape.  *order = device array of old slots.
static uint32_t flow_block_size(const mgf_world* w) {  // (as flow6_plan cuts them)
  const uint32_t need = (w->n_owned + (uint32_t)w->ctx->num_cus - 1u) / (uint32_t)w->ctx->num_cus;
  uint32_t nb = std::max(need, std::min(w->n_owned, 256u));
  if (w->opt.flow5_block > 0) nb = std::max(need, (uint32_t)w->opt.flow5_block);
  return std::max(nb, 1u);
}
static mgf_status partition_order(mgf_world* w, const uint32_t** order) {
  mgf_ctx* ctx = w->ctx;
  hipStream_t s = ctx->stream;
  const uint32_t n = w->n_owned, nb = flow_block_size(w), B = (n + nb - 1u) / nb;
  // fan-outs: boxes as cubic as the scene allows, fx * fy * (columns per row) ~ B
  double e[3];
  for (int k = 0; k < 3; ++k) e[k] = std::max((double)w->h_scene_ext[k], 1e-3);
  const double side = std::cbrt(e[0] * e[1] * e[2] / (double)B);
  uint32_t fx = (uint32_t)std::min<double>(B, std::max(1.0, std::floor(e[0] / side + 0.5)));
  uint32_t fy = (uint32_t)std::min<double>(std::max(1u, B / fx), std::max(1.0, std::floor(e[1] / side + 0.5)));
  fx = std::min(fx, B);
  if ((uint64_t)fx * fy >= (1u << (32 - kPartCoordBits))) return fail(MGF_ERR_CAPACITY, "internal: too many partition units");
  PartPlan P;
  P.nb = nb; P.B = B; P.fx = fx; P.fy = fy;
  for (int k = 0; k < 3; ++k) {  // coarse cells of half the largest fat box's width along the axis (4..10 bits)
    const double cell = std::max((double)w->h_scene_rmax[k], 1e-3 * e[k]);
    uint32_t cb = 4;
    while (cb < 10u && e[k] / (double)(1u << (cb + 1u)) >= cell) ++cb;
    P.cb[k] = cb;
  }
  for (int k = 0; k < 2; ++k) { MGF_TRY(w->part_keys[k].ensure(n, s)); MGF_TRY(w->part_vals[k].ensure(n, s)); }
  const unsigned g = nblk(n);
  auto bits = [](uint32_t v) -> unsigned { return v <= 1u ? 1u : 32u - (unsigned)__builtin_clz(v - 1u) + 1u; };
  // x
  k_part_keys<<<g, kBlock, 0, s>>>(n, nullptr, w->fb_c.p, w->sb.p, 0, P, w->part_keys[0].p, w->part_vals[0].p);
  LAUNCH_CHECK();
  MGF_TRY(prim_sort_pairs_u32(ctx, w->part_keys[0].p, w->part_keys[1].p, w->part_vals[0].p, w->part_vals[1].p, n, kPartCoordBits));
  // y inside the slabs (the slab, high in the key, keeps every body in its slab's run of positions)
  k_part_keys<<<g, kBlock, 0, s>>>(n, w->part_vals[1].p, w->fb_c.p, w->sb.p, 1, P, w->part_keys[0].p, w->part_vals[0].p);
  LAUNCH_CHECK();
  MGF_TRY(prim_sort_pairs_u32(ctx, w->part_keys[0].p, w->part_keys[1].p, w->part_vals[0].p, w->part_vals[1].p, n, std::min(32u, kPartCoordBits + bits(fx))));
  // z inside the rows
  k_part_keys<<<g, kBlock, 0, s>>>(n, w->part_vals[1].p, w->fb_c.p, w->sb.p, 2, P, w->part_keys[0].p, w->part_vals[0].p);
  LAUNCH_CHECK();
  MGF_TRY(prim_sort_pairs_u32(ctx, w->part_keys[0].p, w->part_keys[1].p, w->part_vals[0].p, w->part_vals[1].p, n, std::min(32u, kPartCoordBits + bits(fx * fy))));
  if (B < (1u << 11)) {  // Morton order inside the blocks (block number and 21 code bits share a 32-bit key)
    k_part_keys_block<<<g, kBlock, 0, s>>>(n, w->part_vals[1].p, w->fb_c.p, w->sb.p, nb, w->part_keys[0].p);
    LAUNCH_CHECK();
    MGF_TRY(prim_sort_pairs_u32(ctx, w->part_keys[0].p, w->part_keys[1].p, w->part_vals[1].p, w->part_vals[0].p, n, std::min(32u, 21u + bits(B))));
    *order = w->part_vals[0].p;
    return MGF_OK;
  }
  *order = w->part_vals[1].p;
  return MGF_OK;
}
// The store into a spatial order: compact blocks (partition_order).  Enqueue only.
static mgf_status world_resort(mgf_world* w) {
  if (!w->sidx_valid || w->n != w->n_owned || w->n_owned == 0) return MGF_OK;
  const uint32_t* order = nullptr;
  MGF_TRY(partition_order(w, &order));
  return perm_apply(w, order, false);
}
// The store back into the caller's order (no-op when it is).  The tick's lists name slots: they die with the order.
static mgf_status world_identity(mgf_world* w) {
  if (!w->permuted) return MGF_OK;
  MGF_TRY(ctx_bind(w->ctx));
  w->n = w->n_owned;  // (a permuted store never holds ghosts)
  MGF_TRY(perm_apply(w, w->slot_of.p, true));
  w->invalidate_tick_caches();
  w->constraints_ready = false;
  w->C = w->Ct = 0;
  return MGF_OK;
}
static uint32_t flow_block_size(const mgf_world* w);
// Does the tick that begins now re-sort?  Only the fused tick asks (allow); the world.rs replay keeps the caller's order.
static mgf_status maybe_resort(mgf_world* w, bool allow) {
  if (w->opt.constraint_order == 1) return world_identity(w);
  if (w->opt.solver_mode == 4) return world_identity(w);  // (the experimental slot executor walks constraint ids as the insertion order)
  if (!allow) return MGF_OK;
  if (w->ptrs_out) return MGF_OK;  // (a caller holds raw pointers into the arrays, indexed by its own body indices: mgf_world_device_ptr)
  int64_t every = w->opt.resort_every;
  if (every < 0) every = w->n_owned >= 16384u ? 64 : 0;  // auto: worlds small enough to live in L2 gain nothing; a good order lasts (tools/store_probe.py)
  // (the automatic choice: only where the block-local solver can take the world - a world too large for its LDS tables is solved by
  // the global dataflow launch, which is no faster on a re-sorted store: config 4 as one world, 6.5 against 5.7 ms per tick)
  if (w->opt.resort_every < 0 && flow_block_size(w) + 64u >= kF6NoBody) every = 0;
  if (every == 0) return MGF_OK;  // (a world that was permuted stays as it is: correct in any order)
  ++w->ticks_since_resort;
  // A store that a boundary call put back into the caller's order (write_state, set_tags, export_*: world_identity) is re-sorted
  // after a few ticks, not at the very next one: a caller that makes such a call every tick would pay an un-permute and a re-sort
  // per tick (three radix sorts and two gathers of the whole store) for ticks that run barely faster on the sorted store
  const uint64_t wait = w->permuted ? (uint64_t)every : std::min<uint64_t>((uint64_t)every, w->n_resorts ? 4u : 1u);
  if (w->ticks_since_resort < wait) return MGF_OK;
  return world_resort(w);
}

// canon[r] = id of the r-th constraint of the tick's list in insertion order (null: the ids are the insertion order).  Enqueue only.
static mgf_status canon_ptr(mgf_world* w, uint32_t cap_c, const uint32_t** out) {
  *out = nullptr;
  if (!w->permuted || !w->flow5_ok) return MGF_OK;  // (a caller's list is in the caller's order: world_identity)
  hipStream_t s = w->ctx->stream;
  const uint32_t n = w->n;
  if (!w->canon_ready) {
    MGF_TRY(w->cnt_e.ensure((size_t)n + 1, s)); MGF_TRY(w->base_e.ensure((size_t)n + 1, s)); MGF_TRY(w->canon.ensure(std::max(cap_c, 1u), s));
    k_canon_counts<<<nblk((size_t)n + 1), kBlock, 0, s>>>(n, w->base.p, w->ext_of.p, w->cnt_e.p);
    LAUNCH_CHECK();
    MGF_TRY(prim_exclusive_scan_u32(w->ctx, w->cnt_e.p, w->base_e.p, (size_t)n + 1));
    k_canon_fill<<<nblk(n), kBlock, 0, s>>>(n, w->sc.p, w->base.p, w->ext_of.p, w->base_e.p, w->canon.p);
    LAUNCH_CHECK();
    w->canon_ready = true;
  }
  *out = w->canon.p;
  return MGF_OK;
}
