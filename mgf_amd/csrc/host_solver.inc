// Solver::solve executors (enqueue / finish), mgf_world_step, constraint read-back and caller-supplied lists.
// Part of the single translation unit mgf_hip.hip (included there, in order); not compiled on its own.
// development aid: per-node (ready seen, released) timestamps of a dataflow launch -> /tmp/mgf_flow_trace.bin
static mgf_status dump_flow_trace(mgf_world* w, uint32_t C, int32_t iters) {
  std::vector<uint64_t> h(2 * (size_t)iters * C);
  MGF_TRY(d2h(w->ctx, h.data(), w->flow_trace.p, h.size()));
  if (w->opt.solver_mode == 6 && w->flow6_prepped) {
    std::vector<uint64_t> st(kF6TraceWords * (size_t)w->f5_nblocks);
    MGF_TRY(d2h(w->ctx, st.data(), w->flow_trace.p + h.size(), st.size()));
    if (FILE* f = fopen("/tmp/mgf_flow6_poll.bin", "wb")) { fwrite(st.data(), 8, st.size(), f); fclose(f); }
  }
  // block-local solver: the body -> cell-order rank table and the block size tell which block ran a constraint
  const bool f5 = ((w->opt.solver_mode == 5 && w->flow5_prepped) || (w->opt.solver_mode == 6 && w->flow6_prepped)) && w->f5_nb > 0;
  std::vector<uint32_t> rank(f5 ? (size_t)w->n + (w->n & 1u) : 0);
  if (f5) {
    // (blocks cut from the slots of a re-sorted store: the caller's body index -> its slot; else the tick's cell order)
    const bool slots = w->opt.solver_mode == 6 && w->permuted && w->iota_n >= w->n;
    if (slots) { MGF_TRY(perm_host(w)); for (size_t e = 0; e < w->h_slot_of.size(); ++e) rank[e] = w->h_slot_of[e]; }
    else MGF_TRY(d2h(w->ctx, rank.data(), w->brank.p, (size_t)w->n));
  }
  // constraint ids follow the store's slots: canon[r] = id of the r-th constraint in insertion order (empty: the ids are that order)
  std::vector<uint32_t> canon_h;
  {
    const uint32_t* canon = nullptr;
    MGF_TRY(canon_ptr(w, C, &canon));
    if (canon) { canon_h.resize((size_t)C + (C & 1u)); MGF_TRY(d2h(w->ctx, canon_h.data(), canon, (size_t)C)); }
  }
  if (FILE* f = fopen("/tmp/mgf_flow_trace.bin", "wb")) {
    uint64_t hdr[8] = {C, (uint64_t)iters, f5 ? (uint64_t)rank.size() : 0u, f5 ? (uint64_t)w->f5_nb : 0u, (uint64_t)canon_h.size(), 0u, 0u, 0u};
    fwrite(hdr, 8, 8, f); fwrite(h.data(), 8, h.size(), f);
    if (f5) fwrite(rank.data(), 4, rank.size(), f);
    if (!canon_h.empty()) fwrite(canon_h.data(), 4, canon_h.size(), f);
    fclose(f);
  }
  return MGF_OK;
}

// the CUs a persistent launch may count on: all of them, or this world's share of a device it has been told it shares (option flow_max_blocks)
static uint32_t flow_cus(const mgf_world* w) {
  const uint32_t cus = (uint32_t)std::max(w->ctx->num_cus, 1);
  return w->opt.flow_max_blocks > 0 ? std::max(1u, std::min(cus, (uint32_t)w->opt.flow_max_blocks)) : cus;
}
// Block-local solver: block size (bodies per workgroup) and buffers for a constraint list of up to cap_c.  *ok = false when
// the blocks would not fit the LDS layouts (the global dataflow launch runs instead).
static mgf_status flow5_plan(mgf_world* w, uint32_t cap_c, bool* ok) {
  hipStream_t s = w->ctx->stream;
  // blocks of nb bodies in cell order, one workgroup each, all resident: at most one per CU
  const uint32_t cus = flow_cus(w);
  const uint32_t need = (w->n + cus - 1u) / cus;
  // one block per CU when there are enough bodies (262 144 -> 1024 per block); smaller worlds keep every CU busy with
  // blocks down to 256 bodies (config 5, 65 536 bodies: 0.52 -> 0.45 ms solve)
  uint32_t nb = std::max(need, std::min(w->n, 256u));
  if (w->opt.flow5_block > 0) nb = std::max(need, (uint32_t)w->opt.flow5_block);  // tests: small blocks on small scenes
  if (nb > kF5MaxBodies) { *ok = false; return MGF_OK; }
  w->f5_nb = nb; w->f5_nblocks = (w->n + nb - 1u) / nb;
  *ok = true;
  if (w->flow5_prepped) return MGF_OK;
  MGF_TRY(w->f5_shared.ensure(w->n / 4 + 1, s)); MGF_TRY(w->f5_gcnt.ensure((size_t)cap_c + 1, s)); MGF_TRY(w->f5_lslot.ensure(std::max(cap_c, 1u), s));
  const size_t rows = (size_t)w->f5_nblocks * kF5MaxCons;
  MGF_TRY(w->f5_wg_cnt.ensure(4 * (size_t)w->f5_nblocks * kF5CntStride, s));
  MGF_TRY(w->f5_table.ensure(rows, s)); MGF_TRY(w->flow_arr5.ensure(rows, s));
  return MGF_OK;
}
// what the preparation kernels of the block-local solver need cleared (6 entries of a ZeroList, from `first`)
static void flow5_zero_entries(mgf_world* w, uint32_t cap_c, ZeroList& z, int first) {
  z.p[first + 0] = w->f5_shared.p; z.words[first + 0] = w->n / 4 + 1;
  z.p[first + 1] = w->f5_gcnt.p; z.words[first + 1] = cap_c + 1;
  z.p[first + 2] = w->word(kWFlow5Fail); z.words[first + 2] = 1;
  z.p[first + 3] = w->f5_wg_cnt.p; z.words[first + 3] = 4 * w->f5_nblocks * kF5CntStride;
  z.p[first + 4] = w->word(kWFlow5MaxBlock); z.words[first + 4] = 1;  // largest block of the tick
  z.p[first + 5] = w->word(kWSolverAbort); z.words[first + 5] = 1;  // the solvers' abort flag (k_flow_init resets it for the other modes)
}

// Persistent dataflow launch (modes 1 and 4), enqueue only.  Every lane must be resident, so the grid is sized
// from the occupancy query with one block per CU of margin (the API over-reports by one for some
// kernels on ROCm 7.2).  C is read on the device; `cap_c` bounds the grid.
// The block-local solver's per-list preparation (block size, cross-block marks, slot assignment, slot tables), once per
// constraint list.  Needs nothing from the host but the list's capacity.  *use5 = false when the world does not qualify.
// (Enqueueing it from mgf_world_collide, behind the read-back copy, so that it runs while the host wakes up, was measured on
// the tile path: no gain.)
static mgf_status flow5_prepare(mgf_world* w, uint32_t cap_c, bool* use5) {
  hipStream_t s = w->ctx->stream;
  *use5 = w->opt.solver_mode == 5 && w->flow5_ok && w->n > 0;
  if (*use5) MGF_TRY(flow5_plan(w, cap_c, use5));
  if (!*use5 || w->flow5_prepped) return MGF_OK;
  if (!w->flow5_attr_set) {
    const int lds_n = (int)kF5LdsBytes, lds_w = (int)(64 * (size_t)kF5MaxBodies + kF5LdsWide);
    MGF_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_solve_flow5<false, false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds_n));
    MGF_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_solve_flow5<true, false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds_w));
    MGF_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_solve_flow5<false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds_n));
    MGF_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_solve_flow5<true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds_w));
    w->flow5_attr_set = true;
  }
  // narrow layout (all slot constants in LDS) while the blocks are small, wide layout once they approach its limit
  w->flow5_wide = w->flow5_last_max > w->flow5_narrow_cap() - w->flow5_narrow_cap() / 16;
  if (!w->flow5_zeroed) {  // (otherwise the collide phase cleared these with its own counters)
    ZeroList z;
    memset(&z, 0, sizeof(z));
    flow5_zero_entries(w, cap_c, z, 0);
    k_zero_many<<<64, kBlock, 0, s>>>(z);
    LAUNCH_CHECK();
  }
  w->flow5_zeroed = false;
  Flow5 F = w->flow5();
  const unsigned gc = std::max(1u, nblk(cap_c));
  k_flow5_mark<<<gc, kBlock, 0, s>>>(F, w->links(), &w->sc.p->C);
  LAUNCH_CHECK();
  k_flow5_assign<<<gc, kBlock, 0, s>>>(F, w->links(), &w->sc.p->C);
  LAUNCH_CHECK();
  k_flow5_table<<<gc, kBlock, 0, s>>>(F, w->links(), &w->sc.p->C);
  LAUNCH_CHECK();
  w->flow5_prepped = true;
  return MGF_OK;
}


// ---- block-local solver with message channels (mode 6, k_solver_flow6.h) --------------------------------------------------
constexpr uint32_t kF6LdsBytes = 160u * 1024u;
// the launch's variants: index = TRACE << 5 | QD << 4 | RL << 3 | CL (0..2) << 1 | NL (RL only together with NL: the impulses ride in the staged records)
using F6Kern = void (*)(float4*, CRec*, Flow6, uint32_t, uint32_t, uint32_t*, uint32_t, uint64_t*, uint32_t);
constexpr int kF6Kerns = 64;
template <int I> constexpr F6Kern f6_kern_at() {
  constexpr bool rl = ((I >> 3) & 1) != 0;
  constexpr int cl = ((I >> 1) & 3) > 2 ? 2 : ((I >> 1) & 3);
  return k_solve_flow6<((I >> 5) & 1) != 0, cl, rl || (I & 1) != 0, rl, ((I >> 4) & 1) != 0>;
}
template <int... Is> static F6Kern f6_kern_pick(int k, std::integer_sequence<int, Is...>) {
  static const F6Kern kerns[sizeof...(Is)] = {f6_kern_at<Is>()...};
  return kerns[k];
}
static F6Kern f6_kern(int k) { return f6_kern_pick(k, std::make_integer_sequence<int, kF6Kerns>{}); }
static int f6_kern_index(bool trace, bool qd, bool rl, int cl, bool nl) { return (trace ? 32 : 0) | (qd ? 16 : 0) | (rl ? 8 : 0) | (cl << 1) | (nl ? 1 : 0); }
// Block size, LDS split and buffers for a constraint list of up to cap_c.  *ok = false when the world does not qualify.
static mgf_status flow6_plan(mgf_world* w, uint32_t cap_c, uint32_t iters, bool* ok) {
  hipStream_t s = w->ctx->stream;
  const uint32_t cus = flow_cus(w);
  const uint32_t need = (w->n + cus - 1u) / cus;
  uint32_t nb = std::max(need, std::min(w->n, 256u));
  if (w->opt.flow5_block > 0) nb = std::max(need, (uint32_t)w->opt.flow5_block);  // tests: small blocks on small scenes
  *ok = false;
  if (iters > kF6MaxIters) return MGF_OK;
  // foreign body slots: what the last tick needed plus a quarter; the rest of the LDS goes to constraint slots
  uint32_t fcap = w->opt.flow6_fcap > 0 ? (uint32_t)w->opt.flow6_fcap
                                        : (w->f6_last_foreign ? std::min(1536u, (w->f6_last_foreign + w->f6_last_foreign / 4u + 95u) & ~63u) : 512u);
  if (nb + fcap >= kF6NoBody) { if (nb + 64u >= kF6NoBody) return MGF_OK; fcap = (kF6NoBody - 1u - nb) & ~31u; }
  // What else lives in LDS for the launch, if the last tick's largest block (plus an eighth) still fits beside it: the own bodies'
  // constants (40 bytes per body) and the constraints' accumulated normal impulses (4 bytes per slot) - both, one, or neither
  const uint32_t want_slots = w->opt.flow6_slot_margin > 0 ? w->f6_last_slots + w->f6_last_slots / (uint32_t)w->opt.flow6_slot_margin + 32u
                                                            : w->f6_last_slots + w->f6_last_slots / 8u + 64u;
  auto room = [&](int cl, bool nl, bool rl = false) -> uint32_t {
    const uint32_t fx = f6_lds_bytes(nb, fcap, 0, cl, nl, rl);
    return fx < kF6LdsBytes ? (kF6LdsBytes - fx) / f6_slot_bytes(nl, rl) : 0u;
  };
  int const_lds = 0;
  bool nimp_lds = false, rec_lds = false;
  // (the impulses are read into LDS when a launch starts and written back when it ends: that pays from about four iterations per
  // launch on - a tile's launches of R = 2 iterations are 0.5 % faster without)
  const bool cl_ok = w->opt.flow6_const_lds != 0, nl_ok = w->opt.flow6_nimp_lds != 0 && (iters >= 4u || w->opt.flow6_nimp_lds >= 2);
  const bool fl_ok = cl_ok && w->opt.flow6_foreign_lds != 0;  // the foreign bodies' constants too (r04)
  // the whole solver half of every record (r04): where it fits, a node touches no global memory
  const bool rl_ok = w->opt.flow6_rec_lds != 0 && w->opt.flow6_nimp_lds != 0;
  const uint32_t want_fit = std::max(want_slots, 256u);
  if (rl_ok && fl_ok && room(2, true, true) >= want_fit) { const_lds = 2; nimp_lds = true; rec_lds = true; }
  else if (rl_ok && cl_ok && room(1, true, true) >= want_fit) { const_lds = 1; nimp_lds = true; rec_lds = true; }
  else if (rl_ok && w->opt.flow6_rec_lds >= 2 && room(0, true, true) >= want_fit) { nimp_lds = true; rec_lds = true; }
  else if (fl_ok && nl_ok && room(2, true) >= want_fit) { const_lds = 2; nimp_lds = true; }
  else if (cl_ok && nl_ok && room(1, true) >= want_fit) { const_lds = 1; nimp_lds = true; }
  else if (nl_ok && w->opt.flow6_const_lds < 2 && room(0, true) >= want_fit) nimp_lds = true;  // (measured: worth more than the constants)
  else if (fl_ok && !nl_ok && room(2, false) >= want_fit) const_lds = 2;
  else if (cl_ok && (w->opt.flow6_const_lds >= 2 ? room(1, false) >= 256u : room(1, false) >= want_fit)) const_lds = 1;
  else if (nl_ok && w->opt.flow6_const_lds < 2 && w->opt.flow6_fcap <= 0 && w->f6_last_foreign && w->f6_last_slots) {
    // the settled pile: the impulses fit only with narrow margins (a sixteenth more foreign bodies, a thirty-second more slots than
    // the last tick; the counts drift slowly there, and a tick that outgrows them is re-run with the global solver)
    const uint32_t fcap_std = fcap;
    fcap = std::min(fcap, (w->f6_last_foreign + w->f6_last_foreign / 16u + 47u) & ~31u);
    if (room(0, true) >= std::max(w->f6_last_slots + w->f6_last_slots / 32u + 32u, 256u)) nimp_lds = true;
    else fcap = fcap_std;
  }
  if (room(const_lds, nimp_lds, rec_lds) < 256u) return MGF_OK;
  uint32_t slot_cap = std::min(kF6MaxSlots, room(const_lds, nimp_lds, rec_lds) & ~1u);
  if (w->opt.flow6_test_cap > 0) slot_cap = std::min(slot_cap, (uint32_t)w->opt.flow6_test_cap);
  if (w->f6_fail_C && w->opt.flow6_test_cap <= 0 && !w->flow6_prepped) {
    // a launch of this world did not fit before: the need then, scaled by the constraints since (slots per block follow them; the foreign
    // bodies of a block grow with its surface, not faster than them) - if that still does not fit the split above, not this tick
    const double scale = (double)std::max(w->prev_C, 1u) / (double)w->f6_fail_C;
    const double est_slots = (double)w->f6_fail_slots * scale, est_foreign = (double)w->f6_fail_foreign * std::min(scale, 1.0) ;
    if (est_slots > 0.97 * (double)slot_cap || est_foreign > 0.97 * (double)fcap) { ++w->n_flow6_skipped; return MGF_OK; }
  }
  *ok = true;
  if (w->flow6_prepped) return MGF_OK;  // (the split of a prepared list stays)
  if (w->permuted && w->iota_n < w->n) {
    MGF_TRY(w->iota.ensure(w->n, s));
    w->iota_n = w->iota.cap;
    k_iota<<<nblk(w->iota_n), kBlock, 0, s>>>(w->iota.p, (uint32_t)w->iota_n);
    LAUNCH_CHECK();
  }
  w->f5_nb = nb; w->f5_nblocks = (w->n + nb - 1u) / nb;
  w->f6_fcap = fcap; w->f6_slot_cap = slot_cap; w->f6_rows = slot_cap; w->f6_const_lds = const_lds; w->f6_nimp_lds = nimp_lds; w->f6_rec_lds = rec_lds;
  const size_t nbk = w->f5_nblocks;
  MGF_TRY(w->f6_binfo.ensure((size_t)w->n + 1, s)); MGF_TRY(w->f6_bref.ensure(std::max(cap_c, 1u), s));
  MGF_TRY(w->f6_cflags.ensure(2 * (size_t)std::max(cap_c, 1u) + 4, s)); MGF_TRY(w->f6_skipwb.ensure((size_t)w->n + 4, s));
  MGF_TRY(w->f6_fcnt.ensure(nbk * kF6CntStride, s)); MGF_TRY(w->f6_nslots.ensure(nbk * kF6CntStride, s));
  MGF_TRY(w->f6_fbody.ensure(nbk * fcap, s)); MGF_TRY(w->f6_table.ensure(nbk * slot_cap, s));
  MGF_TRY(w->f6_in_key.ensure(nbk * kF6Chan, s)); MGF_TRY(w->f6_in_cnt.ensure(nbk * kF6Chan, s));
  MGF_TRY(w->f6_out_key.ensure(nbk * kF6Chan, s)); MGF_TRY(w->f6_out_val.ensure(nbk * kF6Chan, s));
  MGF_TRY(w->f6_chan_prefix.ensure(nbk * kF6Chan + 1, s));
  (void)0;
  if (w->f6_tails.cap < nbk * kF6Chan) {  // hint words start at 0 and only ever grow (launch tag in the high half)
    MGF_TRY(w->f6_tails.ensure(nbk * kF6Chan, s));
    MGF_HIP_TRY(hipMemsetAsync(w->f6_tails.p, 0, w->f6_tails.cap * 8, s));
  }
  // channels: a message per edge that crosses a block face and iteration (about a quarter of 2 x constraints do)
  // (every block owns an equal region: sized from the block that received most in the last tick, plus a half)
  const uint64_t per_block = w->f6_last_block_msgs ? w->f6_last_block_msgs + w->f6_last_block_msgs / 2u + 256u
                                                   : std::max<uint64_t>(4096u, (uint64_t)cap_c * std::max(iters, 1u) / std::max<uint64_t>(2 * nbk, 1));
  const uint64_t want = std::min<uint64_t>(40000000ull, per_block * nbk);
  if (want > w->f6_mbox_cap) {
    const bool fresh = w->f6_mbox.cap < want * kF6MsgWords;
    MGF_TRY(w->f6_mbox.ensure((size_t)want * kF6MsgWords, s));
    if (fresh) MGF_HIP_TRY(hipMemsetAsync(w->f6_mbox.p, 0, w->f6_mbox.cap * sizeof(uint4), s));  // no granule may carry a future tag
    w->f6_mbox_cap = (uint32_t)std::min<uint64_t>(w->f6_mbox.cap / kF6MsgWords, 40000000ull);
  }
  return MGF_OK;
}
static Flow6 flow6_args(mgf_world* w) {
  Flow6 F;
  F.C_ptr = &w->sc.p->C; F.sidx = w->sidx.p; F.brank = w->brank.p; F.base = w->base.p;
  // A re-sorted store (host_perm.inc): blocks are runs of SLOTS - the order of the last re-sort, which stays compact for many ticks -
  // instead of runs of the tick's cell order, whose runs of 1024 bodies straddle the cell grid's own boundaries differently every
  // tick (tools/store_probe.py: 9-12 % of the pile's body pairs cross a block face against 12-18 %)
  F.ident = 0u;
  if (w->permuted && w->iota_n >= w->n) { F.sidx = w->iota.p; F.brank = w->iota.p; F.ident = 1u; }
  F.binfo = w->f6_binfo.p; F.bref = w->f6_bref.p; F.skipwb = w->f6_skipwb.p;
  F.fcnt = w->f6_fcnt.p; F.fbody = w->f6_fbody.p; F.nslots = w->f6_nslots.p; F.table = w->f6_table.p;
  F.in_key = w->f6_in_key.p; F.in_cnt = w->f6_in_cnt.p; F.out_key = w->f6_out_key.p; F.out_val = w->f6_out_val.p;
  F.chan_prefix = w->f6_chan_prefix.p; F.mbox = w->f6_mbox.p; F.mbox_cap = w->f6_mbox_cap; F.tails = w->f6_tails.p;
  F.fail = w->word(kWF6Fail); F.tick_fail = &w->sc.p->fail; F.max_slots = w->word(kWF6MaxSlots); F.max_foreign = w->word(kWF6MaxForeign);
  F.nb = w->f5_nb; F.nblocks = w->f5_nblocks; F.n = w->n; F.rows = w->f6_rows; F.fcap = w->f6_fcap; F.slot_cap = w->f6_slot_cap;
  // (measured, profiles/r04_pollers_sweep.txt: two polling waves that also read four positions behind the producers' hint on spec cut the falling
  // pile's launch by 4 %, configs 3 by 3 %; a launch whose constants come from global memory - the settled pile - loses 2 % with a serving wave less)
  const bool busy_cu = w->f6_const_lds == 0;
  F.poll_waves = w->opt.flow6_poll_waves > 0 ? (uint32_t)w->opt.flow6_poll_waves : (busy_cu ? 1u : 2u);
  F.poll_spec_wl = w->opt.flow6_spec_wl >= 0 ? (uint32_t)w->opt.flow6_spec_wl : (busy_cu ? 0u : 4u);
  constexpr uint32_t kPollK = 2u, kPollPrio = 3u;  // quiet sweeps read the channels' heads straight; s_setprio of the polling waves
  F.poll_k = kPollK; F.poll_prio = kPollPrio; F.poll_spec = w->opt.flow6_spec > 0 ? (uint32_t)w->opt.flow6_spec : (busy_cu ? 4u : 8u);
  // (measured, profiles/r04_quad_max_sweep.txt: 48 is best for the falling pile and BASELINE configs 3 and 5; a launch whose bodies' constants come
  // from global memory - the settled pile - is fastest with quad trips only: its one-lane trips wait for six more loads per node)
  F.quad_max = w->opt.flow6_quad_max >= 0 ? (uint32_t)w->opt.flow6_quad_max : (w->f6_const_lds ? 48u : (1u << 20));
  return F;
}
// what the preparation kernels need cleared (8 entries of a ZeroList, from `first`)
static void flow6_zero_entries(mgf_world* w, uint32_t cap_c, ZeroList& z, int first) {
  const uint32_t chw = w->f5_nblocks * kF6Chan;
  z.p[first + 0] = nullptr; z.words[first + 0] = 0;  // (the per-block kernel writes every count)
  z.p[first + 1] = w->f6_in_key.p; z.words[first + 1] = chw;
  z.p[first + 2] = w->f6_in_cnt.p; z.words[first + 2] = chw;
  z.p[first + 3] = w->f6_out_key.p; z.words[first + 3] = chw;
  z.p[first + 4] = reinterpret_cast<uint32_t*>(w->f6_skipwb.p); z.words[first + 4] = w->n / 4 + 1;
  z.p[first + 5] = nullptr; z.words[first + 5] = 0;
  z.p[first + 6] = w->word(kWF6MaxSlots); z.words[first + 6] = kWF6EdgesBlock - kWF6MaxSlots + 1;  // largest block, most foreign bodies, fail, edges per iteration (all / most per block)
  z.p[first + 7] = w->word(kWSolverAbort); z.words[first + 7] = 1;     // the solvers' abort flag
}
// k_chain_rows on the tick's own list.  only_if: a device word; the kernel does nothing while it is 0 (the stand-by's links).
static mgf_status chain_rows_launch(mgf_world* w, const uint32_t* only_if) {
  k_chain_rows<<<nblk(w->n), kBlock, 0, w->ctx->stream>>>(w->n, w->links(), w->base.p, w->degb.p, w->rev.p, w->rev_cap, w->word(kWRevRowOverflow), w->sc.p, w->tcn.p,
                                                          w->n_owned, only_if ? nullptr : w->word(kWGhostCons), only_if, w->ext_ptr());
  LAUNCH_CHECK();
  return MGF_OK;
}
// The block tables of the tick's own constraint list (what does not depend on the iteration count): blocks, foreign bodies,
// rows, links, channels.  Runs at the end of the collide phase (it does the phase's closing bookkeeping on the way:
// k_flow6_links) or, if the solver mode was switched to 6 afterwards, before the first solve.
// a caller's list can be cut into spatial blocks when the bodies' spatial order is known: the slots of a re-sorted store, or the
// cell order of a collide phase that ran on these bodies
static bool flow6_generic_ok(const mgf_world* w) {
  return w->list_generic && (w->permuted || w->sidx_valid);
}
static mgf_status flow6_build_tables(mgf_world* w, uint32_t cap_c, bool* built) {
  hipStream_t s = w->ctx->stream;
  *built = false;
  if (!(w->opt.solver_mode == 6 && !w->tick_mode1 && (w->flow5_ok || flow6_generic_ok(w)) && w->n > 0)) return MGF_OK;
  bool ok = false;
  MGF_TRY(flow6_plan(w, cap_c, w->f6_prep_iters ? w->f6_prep_iters : 10u, &ok));
  if (!ok) return MGF_OK;
  Flow6 F = flow6_args(w);
  if (!w->flow6_zeroed) {  // (otherwise the collide phase cleared these with its own counters)
    ZeroList z;
    memset(&z, 0, sizeof(z));
    flow6_zero_entries(w, cap_c, z, 0);
    k_zero_many<<<64, kBlock, 0, s>>>(z);
    LAUNCH_CHECK();
  }
  w->flow6_zeroed = false;
  if (!w->flow5_ok) {  // a caller's list: tables from its generic dependency links (k_flow6g_*)
    MGF_TRY(w->f6_cslot.ensure(std::max(cap_c, 1u), s)); MGF_TRY(w->f6_clist.ensure((size_t)F.nblocks * F.rows + 1, s));
    MGF_HIP_TRY(hipMemsetAsync(w->f6_nslots.p, 0, (size_t)F.nblocks * kF6CntStride * 4, s));
    k_flow6g_assign<<<std::max(1u, nblk(cap_c)), kBlock, 0, s>>>(F, w->links(), w->f6_cslot.p, w->f6_clist.p);
    LAUNCH_CHECK();
    k_flow6g_blocks<<<F.nblocks, kF6PrepThreads, 0, s>>>(F, w->links(), w->f6_clist.p);
    LAUNCH_CHECK();
    k_flow6g_links<<<std::max(1u, nblk(cap_c)), kBlock, 0, s>>>(F, w->links(), w->f6_cslot.p);
    LAUNCH_CHECK();
    const uint32_t it = w->f6_prep_iters ? w->f6_prep_iters : 10u;
    k_flow6_chan<<<(F.nblocks + kBlock / 64 - 1) / (kBlock / 64), kBlock, 0, s>>>(F, it);
    LAUNCH_CHECK();
    w->flow6_prepped = true;
    w->f6_prep_iters = it;
    *built = true;
    return MGF_OK;
  }
  const int64_t split = w->records_pending ? w->opt.contacts_split : 0;  // (pending: only inside the collide phase that ran k_contacts_rows_index)
  if (split == 3) {  // the partner contacts' records in a launch of their own on the side stream, beside both table kernels
    MGF_TRY(side_fork(w));
    MGF_TRY(records_launch_alone(w, w->ctx->aux));
    MGF_TRY(side_done(w));
  }
  if (!w->f6_tables_early) {  // (option tables_fused: the numbering launch of this collide phase built them, a ticket per block)
    k_flow6_blocks<<<F.nblocks, kF6PrepThreads, 0, s>>>(F, w->links());
    LAUNCH_CHECK();
  }
  w->f6_tables_early = false;
  // (the channel layout - k_flow6_chan's work - is done by the links launch's last block: kWLinksTicket is its ticket, 0 between launches)
  const uint32_t iters = w->f6_prep_iters ? w->f6_prep_iters : 10u;
  MGF_TRY(w->vsnap.ensure(2 * (size_t)std::max(w->n, 1u), s));
  if (split == 1 || split == 2) {  // ... or as foreign blocks of the links launch
    LinksArgs L;
    L.n = w->n; L.degb = w->degb.p; L.rev = w->rev.p; L.rev_cap = w->rev_cap; L.rev_flag = w->word(kWRevRowOverflow); L.sc = w->sc.p; L.n_owned = w->n_owned;
    L.n_ghost_cons = w->word(kWGhostCons); L.ext = w->ext_ptr(); L.ticket = w->word(kWLinksTicket); L.iters = iters; L.srec = w->srec.p; L.vsnap = w->vsnap.p;
    const unsigned rb = std::max(1u, nblk(w->rec_A.cap_c));
    const uint32_t links_first = split == 1 ? 1u : 0u;
    if (w->rec_sph) k_flow6_links_records<true><<<nblk(w->n) + rb, kBlock, 0, s>>>(F, w->links(), L, w->rec_B, w->rec_A, rb, links_first);
    else k_flow6_links_records<false><<<nblk(w->n) + rb, kBlock, 0, s>>>(F, w->links(), L, w->rec_B, w->rec_A, rb, links_first);
    LAUNCH_CHECK();
    w->records_pending = false; w->ts->split_fused = true;
  } else {
    k_flow6_links<<<nblk(w->n), kBlock, 0, s>>>(F, w->links(), w->n, w->degb.p, w->rev.p, w->rev_cap, w->word(kWRevRowOverflow), w->sc.p, w->n_owned, w->word(kWGhostCons), w->ext_ptr(),
                                                w->word(kWLinksTicket), iters, w->srec.p, w->vsnap.p);
    LAUNCH_CHECK();
    if (split == 3) { MGF_TRY(side_join(w)); w->records_pending = false; w->ts->split_fused = true; }
  }
  w->snap_in_links = true;  // (the velocities at this point; good for a launch that follows with nothing in between: the fused tick's)
  w->flow6_prepped = true;
  w->f6_prep_iters = iters;
  *built = true;
  return MGF_OK;
}
static mgf_status flow6_prepare(mgf_world* w, uint32_t cap_c, uint32_t iters, bool* use6) {
  hipStream_t s = w->ctx->stream;
  *use6 = w->opt.solver_mode == 6 && !w->tick_mode1 && (w->flow5_ok || flow6_generic_ok(w)) && w->n > 0;
  if (*use6) MGF_TRY(flow6_plan(w, cap_c, iters, use6));
  if (!*use6) return MGF_OK;
  if (!w->flow6_prepped) {  // (the mode was switched to 6 after the collide phase)
    bool built = false;
    MGF_TRY(flow6_build_tables(w, cap_c, &built));
    if (!built) { *use6 = false; return MGF_OK; }
  }
  // (r06: `>`, not `!=`.  What depends on the iteration count is only whether a block's region of the channel buffer holds its incoming edges
  // `iters` times over - the kernel places a channel at chan_prefix x ITS launch's iterations - so a layout checked for more iterations serves a
  // launch of fewer as it is.  A tile's tick at R = 4 launches 4, 4 and 2 iterations: with `!=` every change of the count cost a k_flow6_chan
  // launch, voided what the host knew of the flags and put the stand-by solver and its links behind the launch: 45 us per tile-tick.)
  if (iters > w->f6_prep_iters) {  // the channels are laid out per iteration count: only the offsets change
    // ... and a layout for more iterations may not fit the channel buffer: what the host knew about the preparation's flags is void
    // (the stand-by and its links are enqueued behind the launch again), and the buffer grows first when the need is known
    w->f6_fail_known = false;
    if (w->f6_edges_block && w->f5_nblocks) {
      const uint64_t want = std::min<uint64_t>(40000000ull, ((uint64_t)w->f6_edges_block * iters + 256u) * w->f5_nblocks);
      if (want > w->f6_mbox_cap) {
        const bool fresh = w->f6_mbox.cap < want * kF6MsgWords;
        MGF_TRY(w->f6_mbox.ensure((size_t)want * kF6MsgWords, s));
        if (fresh) MGF_HIP_TRY(hipMemsetAsync(w->f6_mbox.p, 0, w->f6_mbox.cap * sizeof(uint4), s));  // no granule may carry a future tag
        w->f6_mbox_cap = (uint32_t)std::min<uint64_t>(w->f6_mbox.cap / kF6MsgWords, 40000000ull);
      }
    }
    Flow6 F = flow6_args(w);
    k_flow6_chan<<<(F.nblocks + kBlock / 64 - 1) / (kBlock / 64), kBlock, 0, s>>>(F, iters);
    LAUNCH_CHECK();
    w->f6_prep_iters = iters;
  }
  return MGF_OK;
}

// `fused_tick`: the launch follows this tick's collide phase in the stream with nothing in between (mgf_world_step / step_many).
static mgf_status solve_flow_enqueue(mgf_world* w, int32_t iters, uint32_t cap_c, bool fused_tick = false) {
  mgf_ctx* ctx = w->ctx;
  w->rb_fresh = false;  // whatever the host holds of the flag words predates this launch
  hipStream_t s = ctx->stream;
  const bool links_snap = fused_tick && w->snap_in_links;  // (k_flow6_links copied the velocities on its way; the list's impulses are zero)
  w->snap_in_links = false;
  // (the slot executor walks constraint ids as the insertion order: on a re-sorted store - the mode was switched after the collide
  // phase - the global dataflow launch takes the list, through its `canon` indirection)
  const bool kslots = w->opt.solver_mode == 4 && !(w->permuted && w->flow5_ok);
  bool use5 = false, use6 = false;
  MGF_TRY(flow6_prepare(w, cap_c, (uint32_t)iters, &use6));
  if (!use6 && !w->links_ready) { MGF_TRY(chain_rows_launch(w, nullptr)); w->links_ready = true; }  // (k_flow6_links stood in for k_chain_rows)
  if (iters <= 100) MGF_TRY(flow5_prepare(w, cap_c, &use5));  // iteration counters are 7-bit in LDS
  int& grid = kslots ? w->flowk_grid : w->flow_grid;
  if (grid == 0) {
    int per_cu = 0;
    if (kslots) MGF_HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_solve_flowk<4, false>, kBlock, 0));
    else MGF_HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_solve_flow<false>, kBlock, 0));
    per_cu = std::max(1, std::min(per_cu - 1, 4));
    if (getenv("MGF_FLOW_DEBUG")) fprintf(stderr, "[mgf] dataflow grid: %d blocks/CU x %d CUs\n", per_cu, ctx->num_cus);
    grid = per_cu * (int)flow_cus(w);
  }
  // what solver_abort_fallback restores if the launch gives up (not for stream-ordered launches - several per wait, ghost refreshes in
  // between: a tile set reports the tick as lost instead)
  if (links_snap && use6 && w->f6_tables_in_collide) { w->snap_valid = true; w->snap_nimp = false; }
  else if (!w->opt.stream_ordered && !w->solve_pending) {
    const uint32_t C = w->constraints_ready ? w->C : 0u;  // (a tick in flight: the list is fresh from ContactConstraint::new - zero impulses)
    MGF_TRY(w->vsnap.ensure(2 * (size_t)std::max(w->n, 1u), s));
    if (C) MGF_TRY(w->nsnap.ensure(C, s));
    k_solver_snapshot<<<std::max(1u, nblk(std::max(w->n, C))), kBlock, 0, s>>>(w->srec.p, w->n, w->vsnap.p, w->cons_nat.p, C, C ? w->nsnap.p : nullptr, w->word(kWSkipGuard));
    LAUNCH_CHECK();
    w->snap_valid = true; w->snap_nimp = C != 0u;
  } else {
    w->snap_valid = false;
  }
  const uint32_t* C_ptr = &w->sc.p->C;
  uint32_t* abort_flag = w->word(kWSolverAbort);
  unsigned g = std::min<unsigned>((unsigned)grid, std::max(1u, nblk(cap_c)));
  MGF_TRY(w->flow_arr.ensure(std::max(cap_c, 1u), s));
  if (!use5 && !use6) {  // (the block-local solvers' stand-by initialises its counters itself, when it runs at all)
    k_flow_init<<<std::max(1u, nblk(cap_c)), kBlock, 0, s>>>(C_ptr, w->links(), w->flow_arr.p, abort_flag);
    LAUNCH_CHECK();
  }
  const bool timed = w->opt.time_solver_kernels != 0;
  if (!w->solve_pending) w->ts->kev_used = 0;  // a tiled tick enqueues several launches before it reads the events
  if (timed) {
    while (w->ts->kev.size() < w->ts->kev_used + 2) { hipEvent_t e; MGF_HIP_TRY(hipEventCreate(&e)); w->ts->kev.push_back(e); }
    MGF_HIP_TRY(hipEventRecord(w->ts->kev[w->ts->kev_used], s));
  }
  uint64_t* trace = nullptr;
  if (w->opt.flow_trace) {  // development aid (needs the host-side C: only after a synchronous collide)
    const size_t tail = (size_t)kF6TraceWords * 4096;  // per-block polling statistics and phase clocks (mode 6)
    const size_t words = 2 * (size_t)iters * std::max(w->C, 1u) + tail;
    MGF_TRY(w->flow_trace.ensure(words, s));
    MGF_HIP_TRY(hipMemsetAsync(w->flow_trace.p + words - tail, 0, tail * 8, s));
    trace = w->flow_trace.p;
  }
  const uint32_t spin_limit = w->opt.flow_spin_limit > 0 ? (uint32_t)w->opt.flow_spin_limit : 4u << 20;
  constexpr int sleep = 2;  // how a waiting lane of k_solve_flow / k_solve_flowk idles (their sleep_mode)
  if (use6) {
    Flow6 F = flow6_args(w);
    if (++w->f6_epoch == 0u) ++w->f6_epoch;
    const size_t lds = f6_lds_bytes(F.nb, F.fcap, F.slot_cap, w->f6_const_lds, w->f6_nimp_lds, w->f6_rec_lds);
    const int kidx = f6_kern_index(trace != nullptr, w->opt.flow6_quad != 0, w->f6_rec_lds, w->f6_const_lds, w->f6_nimp_lds);
    const F6Kern kern = f6_kern(kidx);
    if (!(w->f6_attr_mask >> kidx & 1ull)) {  // (the one variant this launch takes, the first time it does: not all 64 of the table up front - ADVICE r4)
      MGF_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kF6LdsBytes));
      w->f6_attr_mask |= 1ull << kidx;
    }
    kern<<<F.nblocks, kF6Threads, lds, s>>>(w->srec.p, w->cons_nat.p, F, (uint32_t)iters, w->f6_epoch, abort_flag, spin_limit, trace, w->C);
    LAUNCH_CHECK();
    // What happens if the preparation raised its flag (a block that does not fit, a channel buffer too small): the launch above did
    // nothing, and
    //  * a tick whose collide phase is still in flight (mgf_world_step / step_many: one synchronisation at the end) carries the flag
    //    on its read-back as kFailFlow6 - whether the tables were built inside the collide phase or the channels re-laid for another
    //    iteration count just above - and the host re-runs the tick from the collide phase with the global dataflow solver.  Nothing
    //    behind the launch may touch the velocities then: NO stand-by (it used to run here, on links k_chain_rows had declined to build);
    //  * a list whose collide phase the host has finished (mgf_world_solve, the tile drivers) is solved by the stand-by k_solve_flow
    //    enqueued right behind, on links built only then - unless the host has read the flags of exactly this layout and they are clean.
    const bool in_flight = !w->constraints_ready;
    const bool sure_ok = w->f6_fail_known && w->f6_fail_host == 0u;
    w->f6_standby = !in_flight && !sure_ok;
    if (w->f6_standby) {
      if (!w->links_ready) MGF_TRY(chain_rows_launch(w, F.fail));
      const uint32_t* canon = nullptr;
      MGF_TRY(canon_ptr(w, cap_c, &canon));
      k_solve_flow<false><<<g, kBlock, 0, s>>>(w->srec.p, w->cons_nat.p, w->links(), w->flow_arr.p, C_ptr, (uint32_t)iters, abort_flag, spin_limit, sleep, nullptr, F.fail, w->word(kWStandbyBar), canon);
    }
  } else if (use5) {
    Flow5 F = w->flow5();
    const size_t lds = 64 * (size_t)F.nb + (w->flow5_wide ? kF5LdsWide : f5_lds_narrow(w->flow5_narrow_cap()));
    auto kern = w->flow5_wide ? (trace ? k_solve_flow5<true, true> : k_solve_flow5<true, false>)
                              : (trace ? k_solve_flow5<false, true> : k_solve_flow5<false, false>);
    kern<<<F.nblocks, kF5Threads, lds, s>>>(w->srec.p, w->cons_nat.p, w->links(), F, w->flow_arr.p, (uint32_t)iters, abort_flag, spin_limit, trace, w->C);
    LAUNCH_CHECK();
    // stand-by: the global dataflow kernel runs only if a block did not fit its workgroup (flag raised by k_flow5_prep)
    const uint32_t* canon = nullptr;
    MGF_TRY(canon_ptr(w, cap_c, &canon));
    k_solve_flow<false><<<g, kBlock, 0, s>>>(w->srec.p, w->cons_nat.p, w->links(), w->flow_arr.p, C_ptr, (uint32_t)iters, abort_flag, spin_limit, sleep, nullptr, F.fail, w->word(kWStandbyBar), canon);
  } else if (kslots) {
    if (trace) k_solve_flowk<4, true><<<g, kBlock, 0, s>>>(w->srec.p, w->cons_nat.p, w->links(), w->flow_arr.p, C_ptr, (uint32_t)iters, abort_flag, spin_limit, sleep, trace);
    else k_solve_flowk<4, false><<<g, kBlock, 0, s>>>(w->srec.p, w->cons_nat.p, w->links(), w->flow_arr.p, C_ptr, (uint32_t)iters, abort_flag, spin_limit, sleep, nullptr);
  } else {
    const uint32_t* canon = nullptr;
    MGF_TRY(canon_ptr(w, cap_c, &canon));
    if (trace) k_solve_flow<true><<<g, kBlock, 0, s>>>(w->srec.p, w->cons_nat.p, w->links(), w->flow_arr.p, C_ptr, (uint32_t)iters, abort_flag, spin_limit, sleep, trace, nullptr, nullptr, canon);
    else k_solve_flow<false><<<g, kBlock, 0, s>>>(w->srec.p, w->cons_nat.p, w->links(), w->flow_arr.p, C_ptr, (uint32_t)iters, abort_flag, spin_limit, sleep, nullptr, nullptr, nullptr, canon);
  }
  LAUNCH_CHECK();
  if (timed) { MGF_HIP_TRY(hipEventRecord(w->ts->kev[w->ts->kev_used + 1], s)); w->ts->kev_used += 2; }
  w->snap_in_links = false;  // (whatever k_flow6_links copied on the way here is this launch's)
  return MGF_OK;
}

// One launch per frontier of the unrolled dependency graph (mode 0): host loop with read-backs.
static mgf_status solve_frontier(mgf_world* w, int32_t iters) {
  mgf_ctx* ctx = w->ctx;
  hipStream_t s = ctx->stream;
  const uint32_t C = w->C;
  const bool timed = w->opt.time_solver_kernels != 0;
  size_t kev_used = 0;
  auto tick = [&](void) -> mgf_status {  // event before/after a solver kernel (option)
    if (!timed) return MGF_OK;
    if (kev_used == w->ts->kev.size()) { hipEvent_t e; MGF_HIP_TRY(hipEventCreate(&e)); w->ts->kev.push_back(e); }
    MGF_HIP_TRY(hipEventRecord(w->ts->kev[kev_used++], s));
    return MGF_OK;
  };
  // frontier lists hold every (constraint, round) once: iters * C entries
  MGF_TRY(w->order.ensure((size_t)iters * C, s));
  if (w->lvl_cap == 0) { w->lvl_cap = 1u << 16; MGF_TRY(w->lvl_off.ensure(w->lvl_cap + 4, s)); }
  Frontier F = w->frontier();
  MGF_HIP_TRY(hipMemsetAsync(w->word(kWFrontier0), 0, 3 * 4, s));
  k_frontier0<<<std::min<unsigned>(nblk(C), 1024u), kBlock, 0, s>>>(C, w->cons_nat.p, w->links(), F);
  LAUNCH_CHECK();
  uint32_t r = 0;
  // grid: frontiers hold roughly C / (per-iteration depth) constraints; grid-stride covers the rest
  unsigned g0 = std::min<unsigned>(std::max<unsigned>(nblk(C) / 4, 1u), 2048u);
  uint32_t batch = std::max<uint32_t>(w->last_launches + 2, 8u);
  uint32_t* pin = static_cast<uint32_t*>(ctx->pinned);
  for (;;) {
    if (r + batch + 2 > w->lvl_cap) return fail(MGF_ERR_CAPACITY, "constraint dependency graph deeper than 65536 launches");
    for (uint32_t k = 0; k < batch; ++k) {
      MGF_TRY(tick());
      k_solve<<<g0, kBlock, 0, s>>>(w->srec.p, w->cons_nat.p, w->links(), F, r + k, (uint32_t)iters);
      LAUNCH_CHECK();
      MGF_TRY(tick());
      w->stats.solver_kernel_launches++;
    }
    r += batch;
    // launch r's list was filled by the last launch under counter r % 3; empty means everything ran
    MGF_HIP_TRY(hipMemcpyAsync(pin, w->word(kWFrontier0) + (r % 3), 4, hipMemcpyDeviceToHost, s));
    MGF_HIP_TRY(hipMemcpyAsync(pin + 1, w->lvl_off.p + r, 4, hipMemcpyDeviceToHost, s));
    MGF_HIP_TRY(hipStreamSynchronize(s));
    if (pin[0] == 0) {
      if ((uint64_t)pin[1] != (uint64_t)iters * C) return fail(MGF_ERR_HIP, "internal error: solver schedule does not cover iters x constraints");
      break;
    }
    batch = 4;
  }
  // number of non-empty launches (for stats and for sizing the next tick's batch)
  std::vector<uint32_t> h(r + 1);
  MGF_TRY(d2h(ctx, h.data(), w->lvl_off.p, r + 1));
  uint32_t used = 0;
  while (used < r && h[used] < (uint64_t)iters * C) ++used;
  w->depth = used;
  w->last_launches = used;
  if (timed) {
    float total = 0.0f, ms;
    for (size_t k = 0; k + 1 < kev_used; k += 2) { MGF_HIP_TRY(hipEventElapsedTime(&ms, w->ts->kev[k], w->ts->kev[k + 1])); total += ms; }
    w->stats.ms_solver_kernels = total;
  }
  return MGF_OK;
}

// The solvers' flag words (mgf_world::kSolverFlagsFirst ..) into the tick slot's pinned copy of the block.  Enqueue only.
static mgf_status solver_flags_fetch(mgf_world* w) {
  MGF_HIP_TRY(hipMemcpyAsync(w->ts->pin + mgf_world::kRbScalars + mgf_world::kSolverFlagsFirst, w->word(kWSolverAbort), 4 * mgf_world::kSolverFlagsWords,
                             hipMemcpyDeviceToHost, w->ctx->stream));
  return MGF_OK;
}
// After a dataflow launch has been synchronised: abort flag, timings.
static mgf_status solve_flow_finish(mgf_world* w) {
  const mgf_world::TickSlot& h = *w->ts;
  // In the one-synchronisation tick the solver was enqueued before collide_finish fetched the read-back block, so that copy already
  // holds the solvers' flags.
  if (!w->rb_fresh) {
    MGF_TRY(solver_flags_fetch(w));
    MGF_HIP_TRY(hipStreamSynchronize(w->ctx->stream));
  }
  w->rb_fresh = false;
  if (h.word(kWSolverAbort)) { w->solver_aborted = true; return fail(MGF_ERR_HIP, "dataflow solver gave up waiting (grid not fully resident?)"); }
  if (w->opt.solver_mode == 5 && w->flow5_prepped) {
    if (h.word(kWFlow5Fail)) w->n_flow5_fallbacks++;
    w->flow5_last_max = h.word(kWFlow5MaxBlock);
  }
  if (w->opt.solver_mode == 6 && w->flow6_prepped) {
    if (h.word(kWF6Fail)) {
      w->n_flow6_fallbacks++; w->f6_fail_reason = h.word(kWF6Fail);
      // (a tick in flight re-runs from its collide phase on kFailFlow6; a finished list must have had its stand-by)
      if (w->constraints_ready && !w->f6_standby) return fail(MGF_ERR_HIP, "internal error: the block-local solver declined and no stand-by launch was enqueued");
    }
    else { w->n_flow6_runs++; w->f6_fail_C = 0; }
    w->f6_last_slots = h.word(kWF6MaxSlots); w->f6_last_foreign = h.word(kWF6MaxForeign);
    w->f6_last_msgs = (uint64_t)h.word(kWF6Edges) * std::max(w->f6_prep_iters, 1u);
    w->f6_last_block_msgs = (uint64_t)h.word(kWF6EdgesBlock) * std::max(w->f6_prep_iters, 1u);
  }
  w->stats.solver_kernel_launches = 1;
  w->depth = 1;
  if (w->opt.time_solver_kernels) {
    float ms, total = 0.0f;
    // (a tick that ended on the polled read-back word instead of a stream synchronisation: the event's own completion may lag it)
    if (w->ts->kev_used >= 2) MGF_HIP_TRY(hipEventSynchronize(w->ts->kev[w->ts->kev_used - 1]));
    for (size_t k = 0; k + 1 < w->ts->kev_used; k += 2) { MGF_HIP_TRY(hipEventElapsedTime(&ms, w->ts->kev[k], w->ts->kev[k + 1])); total += ms; }
    w->stats.ms_solver_kernels = total;
  }
  return MGF_OK;
}

// A driver of several worlds on one stream (the tile set) fetches every world's flags first and waits ONCE: solve_flow_finish then finds
// them in the pinned block (rb_fresh) and does not wait again.  The caller synchronises the stream before it calls mgf_world_finish.
static mgf_status solve_flow_fetch_enqueue(mgf_world* w) {
  if (!w->solve_pending || !w->stats.solver_kernel_launches || w->rb_fresh) return MGF_OK;
  MGF_TRY(solver_flags_fetch(w));
  w->rb_fresh = true;
  return MGF_OK;
}

// Solver::solve has no failure mode (solver.rs:72-78).  A persistent launch that gave up (w->solver_aborted, set by solve_flow_finish)
// left the velocities half-solved: they and the impulses go back to what the launch found, and the list is solved by the
// launch-per-frontier executor - any topological execution of the dependency graph gives the sequential result bit for bit.
// The next solves use that executor at once (the launch waited ~0.5 s before it gave up), for twice as long every time this happens.
// `recollide` (mgf_world_step_many: a speculative tick had been enqueued behind this one - it did nothing, but its clearing launch
// and its unguarded cell sort went over this tick's lists): the collide phase of this tick once more, on the restored velocities.
static mgf_status solver_abort_fallback(mgf_world* w, int32_t iters, bool recollide = false, float dt = 0.0f) {
  hipStream_t s = w->ctx->stream;
  w->solver_aborted = false;
  MGF_HIP_TRY(hipStreamSynchronize(s));
  if (!w->snap_valid)
    return fail(MGF_ERR_HIP, "dataflow solver gave up waiting (grid not fully resident?) and the launches were stream-ordered: no snapshot to solve the list again from");
  k_solver_restore<<<std::max(1u, nblk(std::max(w->n, w->C))), kBlock, 0, s>>>(w->srec.p, w->n, w->vsnap.p, w->cons_nat.p, w->C, w->snap_nimp ? w->nsnap.p : nullptr, w->word(kWSolverAbort));
  LAUNCH_CHECK();
  w->snap_valid = false;
  ++w->n_solver_abort_fallbacks;
  w->abort_backoff = w->abort_backoff_next;
  w->abort_backoff_next = std::min(2u * w->abort_backoff_next, 4096u);
  if (recollide) {
    w->invalidate_tick_caches();  // (the terrain rows' counts were cleared with the other counters)
    w->constraints_ready = false;
    w->C = w->Ct = w->Mt = w->Mp = 0;
    bool done = false;
    for (int attempt = 0; attempt < 8 && !done; ++attempt) {
      bool again = false;
      MGF_TRY(collide_enqueue(w, dt, false));
      MGF_TRY(collide_finish(w, &again));
      done = !again;
    }
    if (!done) return fail(MGF_ERR_HIP, "internal error: collide phase did not settle its buffer capacities");
  }
  if (!w->links_ready) { MGF_TRY(chain_rows_launch(w, nullptr)); w->links_ready = true; }
  w->stats.solver_kernel_launches = 0;
  MGF_TRY(solve_frontier(w, iters));
  MGF_HIP_TRY(hipStreamSynchronize(s));
  w->stats.n_levels = w->depth;
  return MGF_OK;
}
// (a solve that may use a persistent launch: not while the world is backing off after one that gave up)
static bool frontier_only(mgf_world* w) { return w->opt.solver_mode == 0 || w->abort_backoff > 0; }

// Solver::solve solver.rs:72-78 (exact sequential order, see kernels.h).
extern "C" mgf_status mgf_world_solve(mgf_world* w, int32_t iters, mgf_step_stats* stats) {
  if (!w) return fail(MGF_ERR_INVALID, "world is NULL");
  if (iters < 0) return fail(MGF_ERR_INVALID, "iters must be >= 0");
  MGF_TRY(ctx_bind(w->ctx));
  if (!w->constraints_ready) return fail(MGF_ERR_INVALID, "no constraint list: call mgf_world_build_constraints or mgf_world_set_constraints first");
  hipStream_t s = w->ctx->stream;
  w->stats.iters = (uint32_t)iters;
  w->stats.solver_kernel_launches = 0;
  w->stats.ms_solver_kernels = 0.0f;
  w->depth = 0;
  MGF_TRY(phase_mark(w, 5, s));
  const bool frontier = frontier_only(w);
  if (w->C > 0 && iters > 0) {
    if (frontier) {
      if (w->abort_backoff > 0) --w->abort_backoff;
      if (!w->links_ready) { MGF_TRY(chain_rows_launch(w, nullptr)); w->links_ready = true; }  // (k_flow6_links stood in for k_chain_rows)
      MGF_TRY(solve_frontier(w, iters));
    } else {
      MGF_TRY(solve_flow_enqueue(w, iters, w->C));
      if (w->opt.flow_trace) MGF_TRY(dump_flow_trace(w, w->C, iters));
      MGF_TRY(phase_mark(w, 6, s));
      const mgf_status st = solve_flow_finish(w);
      if (st != MGF_OK && w->solver_aborted) MGF_TRY(solver_abort_fallback(w, iters));
      else { MGF_TRY(st); w->abort_backoff_next = 16; }
    }
  }
  if (frontier || !(w->C > 0 && iters > 0)) MGF_TRY(phase_mark(w, 6, s));
  MGF_HIP_TRY(hipStreamSynchronize(s));
  float ms;
  MGF_TRY(phase_ms(w, 5, 6, &ms));
  w->stats.ms_solve = ms;
  w->stats.n_levels = w->depth;
  if (stats) *stats = w->stats;
  return MGF_OK;
}

// Solver::solve without the read-back: the launch is enqueued on the ctx stream and its outcome is checked by
// the next mgf_world_finish (a tiled driver interleaves single iterations with ghost velocity exchanges
// on the same stream).  Solver mode 0 has a host loop and runs synchronously here.
extern "C" mgf_status mgf_world_solve_enqueue(mgf_world* w, int32_t iters) {
  if (!w) return fail(MGF_ERR_INVALID, "world is NULL");
  if (iters < 0) return fail(MGF_ERR_INVALID, "iters must be >= 0");
  if (frontier_only(w) || w->opt.flow_trace) return mgf_world_solve(w, iters, nullptr);
  MGF_TRY(ctx_bind(w->ctx));
  if (!w->constraints_ready) return fail(MGF_ERR_INVALID, "no constraint list: call mgf_world_build_constraints or mgf_world_set_constraints first");
  if (!w->solve_pending) {
    MGF_TRY(phase_mark(w, 5, w->ctx->stream));
    w->stats.iters = 0;
    w->stats.solver_kernel_launches = 0;
    w->stats.ms_solver_kernels = 0.0f;
  }
  if (w->C > 0 && iters > 0) {
    MGF_TRY(solve_flow_enqueue(w, iters, w->C));
    w->stats.solver_kernel_launches++;
  }
  w->stats.iters += (uint32_t)iters;
  w->solve_pending = true;
  return MGF_OK;
}
// Synchronise the ctx stream and report what the enqueued work did (solver abort flag, timings).
extern "C" mgf_status mgf_world_finish(mgf_world* w, mgf_step_stats* stats) {
  if (!w) return fail(MGF_ERR_INVALID, "world is NULL");
  MGF_TRY(ctx_bind(w->ctx));
  hipStream_t s = w->ctx->stream;
  if (w->solve_pending) {
    w->solve_pending = false;
    MGF_TRY(phase_mark(w, 6, s));
    uint32_t launches = w->stats.solver_kernel_launches;
    if (launches) {
      const mgf_status st = solve_flow_finish(w);
      // (one launch since the last wait and a snapshot from before it: solved again; several stream-ordered launches: the tick is lost)
      if (st != MGF_OK && w->solver_aborted && launches == 1 && w->snap_valid) MGF_TRY(solver_abort_fallback(w, (int32_t)w->stats.iters));
      else { if (st != MGF_OK && w->solver_aborted) w->finish_gave_up = true; w->solver_aborted = false; MGF_TRY(st); }  // (finish_gave_up: the tile set repeats such a tick)
    } else MGF_HIP_TRY(hipStreamSynchronize(s));
    w->stats.solver_kernel_launches = launches;
    float ms;
    MGF_TRY(phase_ms(w, 5, 6, &ms));
    w->stats.ms_solve = ms;
    w->stats.n_levels = launches;
    MGF_TRY(phase_ms(w, 0, 6, &ms));
    w->stats.ms_total = ms;
  } else {
    MGF_HIP_TRY(hipStreamSynchronize(s));
  }
  if (stats) *stats = w->stats;
  return MGF_OK;
}

// the collide phase and the solve of a tick whose begin has run, into the stream; nothing is waited for
static mgf_status collide_solve_enqueue(mgf_world* w, float dt, int32_t iters) {
  hipStream_t s = w->ctx->stream;
  MGF_TRY(collide_enqueue(w, dt, w->n > 0 && iters > 0));
  MGF_TRY(phase_mark(w, 5, s));
  if (w->n > 0 && iters > 0) MGF_TRY(solve_flow_enqueue(w, iters, w->cap_c, true));
  return phase_mark(w, 6, s);
}
// ... enqueued and read back until the collide phase has settled its buffer capacities (a miss re-runs the phase: the solver was a no-op)
static mgf_status collide_solve_settle(mgf_world* w, float dt, int32_t iters) {
  for (int attempt = 0; attempt < 8; ++attempt) {
    bool retry = false;
    MGF_TRY(collide_solve_enqueue(w, dt, iters));
    MGF_TRY(collide_finish(w, &retry));
    if (!retry) return MGF_OK;
  }
  return fail(MGF_ERR_HIP, "internal error: collide phase did not settle its buffer capacities");
}
// World::step world.rs:227-294.  With a dataflow solver the whole tick is enqueued without a read-back
// and synchronised once at the end; a capacity miss re-runs the collide phase (the solver was a no-op).
extern "C" mgf_status mgf_world_step(mgf_world* w, float dt, int32_t iters, mgf_step_stats* stats) {
  if (!w) return fail(MGF_ERR_INVALID, "world is NULL");
  if (iters < 0) return fail(MGF_ERR_INVALID, "iters must be >= 0");
  if (frontier_only(w) || w->opt.flow_trace || w->opt.constraint_order == 1) {
    MGF_TRY(mgf_world_build_constraints(w, dt, nullptr));
    MGF_TRY(mgf_world_solve(w, iters, nullptr));
  } else {
    MGF_TRY(world_begin(w, dt, false, true, true, w->n_owned > 0 && iters > 0));
    MGF_TRY(collide_solve_settle(w, dt, iters));
    w->stats.iters = (uint32_t)iters;
    w->stats.solver_kernel_launches = 0;
    w->stats.ms_solver_kernels = 0.0f;
    w->depth = 0;
    if (w->C > 0 && iters > 0) {
      const mgf_status st = solve_flow_finish(w);
      if (st != MGF_OK && w->solver_aborted) MGF_TRY(solver_abort_fallback(w, iters));
      else { MGF_TRY(st); w->abort_backoff_next = 16; }
    }
    float ms;
    MGF_TRY(phase_ms(w, 5, 6, &ms));
    w->stats.ms_solve = ms;
    w->stats.n_levels = w->depth;
  }
  float ms;
  MGF_TRY(phase_ms(w, 0, 6, &ms));
  w->stats.ms_total = ms;
  if (stats) *stats = w->stats;
  return MGF_OK;
}

// the bookkeeping of mgf_world_step after the collide phase has settled
static mgf_status step_complete(mgf_world* w, int32_t iters, mgf_step_stats* stats) {
  w->stats.iters = (uint32_t)iters;
  w->stats.solver_kernel_launches = 0;
  w->stats.ms_solver_kernels = 0.0f;
  w->depth = 0;
  if (w->C > 0 && iters > 0) {
    const mgf_status st = solve_flow_finish(w);
    if (st != MGF_OK && w->solver_aborted) return st;  // (the caller drains what it enqueued behind this tick, then solver_abort_fallback)
    MGF_TRY(st);
    w->abort_backoff_next = 16;
  }
  float ms;
  MGF_TRY(phase_ms(w, 5, 6, &ms));
  w->stats.ms_solve = ms;
  w->stats.n_levels = w->depth;
  MGF_TRY(phase_ms(w, 0, 6, &ms));
  w->stats.ms_total = ms;
  if (stats) *stats = w->stats;
  return MGF_OK;
}
// one whole tick into the stream, read-back copy and its event included; nothing is waited for
static mgf_status tick_enqueue(mgf_world* w, float dt, int32_t iters, bool speculative) {
  MGF_TRY(world_begin(w, dt, speculative, true, true, w->n_owned > 0 && iters > 0));
  MGF_TRY(collide_solve_enqueue(w, dt, iters));
  return readback_enqueue(w);
}

// n ticks back to back (World::step in a host loop), one statistics record per tick.  With a dataflow solver the host
// enqueues tick k + 1 BEFORE it waits for the counts of tick k, so the GPU does not idle while the host turns around
// (~50 us per tick).  Tick k + 1 is then speculative: if tick k failed a capacity check, a device-side guard
// (k_reset_step) turns tick k + 1 into a no-op, the host re-runs tick k the ordinary way and enqueues k + 1 again.
extern "C" mgf_status mgf_world_step_many(mgf_world* w, float dt, int32_t iters, int64_t n, mgf_step_stats* stats) {
  if (!w || n < 0) return fail(MGF_ERR_INVALID, "bad argument");
  if (iters < 0) return fail(MGF_ERR_INVALID, "iters must be >= 0");
  if (frontier_only(w) || w->opt.flow_trace || !w->opt.pipeline || w->opt.constraint_order == 1) {
    for (int64_t k = 0; k < n; ++k) MGF_TRY(mgf_world_step(w, dt, iters, stats ? stats + k : nullptr));
    return MGF_OK;
  }
  MGF_TRY(ctx_bind(w->ctx));
  hipStream_t s = w->ctx->stream;
  int cur = (int)(w->ts - w->slots);
  bool have = false;  // tick k is already in the stream (slot `cur`)
  for (int64_t k = 0; k < n; ++k) {
    w->ts = &w->slots[cur];
    if (!have && w->abort_backoff > 0) {  // (backing off after a persistent launch that gave up: tick by tick, the launch-per-frontier executor)
      MGF_TRY(mgf_world_step(w, dt, iters, stats ? stats + k : nullptr));
      continue;
    }
    if (!have) MGF_TRY(tick_enqueue(w, dt, iters, false));
    const bool spec = k + 1 < n;
    if (spec) {
      w->ts = &w->slots[cur ^ 1];
      MGF_TRY(tick_enqueue(w, dt, iters, true));
      w->ts = &w->slots[cur];
    }
    bool retry = false;
    MGF_TRY(readback_wait(w));
    MGF_TRY(collide_process(w, &retry));
    if (retry) {
      if (spec) {  // drain the tick behind it (the guard made it a no-op) and lower the guard for the re-run
        w->ts = &w->slots[cur ^ 1];
        MGF_TRY(readback_wait(w));
        w->ts = &w->slots[cur];
        MGF_HIP_TRY(hipMemsetAsync(w->word(kWSkipGuard), 0, 4, s));
        // (its clearing launch went over the counters all the same - the terrain rows' counts that this tick's k_integrate wrote among
        // them: the re-run lists the rows again - r05: they used to be taken as still there, and the tick lost its terrain contacts)
        w->invalidate_tick_caches();
      }
      MGF_TRY(collide_solve_settle(w, dt, iters));  // tick k again (its begin has run), as mgf_world_step does
      have = false;
    } else {
      have = spec;
    }
    const mgf_status st = step_complete(w, iters, stats ? stats + k : nullptr);
    if (st != MGF_OK && w->solver_aborted) {
      // the tick's persistent launch gave up.  The tick enqueued behind it saw the flag (k_tick_clear) and did nothing: drain it, lower
      // its guard, solve this tick's list again (solver_abort_fallback); the loop goes on tick by tick while the world backs off
      const bool behind = have;
      if (have) {
        w->ts = &w->slots[cur ^ 1];
        MGF_TRY(readback_wait(w));
        w->ts = &w->slots[cur];
        MGF_HIP_TRY(hipMemsetAsync(w->word(kWSkipGuard), 0, 4, s));
        have = false;
      }
      MGF_TRY(solver_abort_fallback(w, iters, behind, dt));
      float ms;
      MGF_TRY(phase_ms(w, 5, 6, &ms));
      w->stats.ms_solve = ms;
      MGF_TRY(phase_ms(w, 0, 6, &ms));
      w->stats.ms_total = ms;
      if (stats) stats[k] = w->stats;
    } else {
      MGF_TRY(st);
    }
    if (have) cur ^= 1;
  }
  return MGF_OK;
}

static void crec_to_public(const CRec& c, mgf_constraint* o) {
  o->a = (int32_t)c.a;
  o->b = c.b == kNone ? -1 : (int32_t)c.b;
  o->n_contacts = 1;
  o->normal = {c.n[0], c.n[1], c.n[2]}; o->t0 = {c.t0[0], c.t0[1], c.t0[2]}; o->t1 = {c.t1[0], c.t1[1], c.t1[2]};
  o->ra = {c.ra[0], c.ra[1], c.ra[2]}; o->rb = {c.rb[0], c.rb[1], c.rb[2]};
  o->bias = c.bias; o->normal_mass = c.nmass; o->tangent_mass0 = c.tmass0; o->tangent_mass1 = c.tmass1;
  o->normal_impulse = c.nimp; o->friction = c.friction;
}
extern "C" mgf_status mgf_world_read_constraints(mgf_world* w, mgf_constraint* out, int64_t cap, int64_t* count) {
  if (!w) return fail(MGF_ERR_INVALID, "world is NULL");
  MGF_TRY(ctx_bind(w->ctx));
  if (count) *count = w->C;
  if (!out) return MGF_OK;
  if ((int64_t)w->C > cap) return fail(MGF_ERR_CAPACITY, "constraint buffer too small");
  if (w->C == 0) return MGF_OK;
  std::vector<CRec> h(w->C);
  MGF_TRY(d2h(w->ctx, h.data(), w->cons_nat.p, w->C));
  if (!w->permuted) {
    for (uint32_t i = 0; i < w->C; ++i) crec_to_public(h[i], &out[i]);
    return MGF_OK;
  }
  MGF_TRY(perm_host(w));
  if (!w->flow5_ok) {  // a caller's list: already in its insertion order; only the body names are slots
    for (uint32_t i = 0; i < w->C; ++i) {
      crec_to_public(h[i], &out[i]);
      out[i].a = (int32_t)w->h_ext_of[h[i].a];
      if (h[i].b != kNone) out[i].b = (int32_t)w->h_ext_of[h[i].b];
    }
    return MGF_OK;
  }
  // The store is in an internal order (host_perm.inc): records name slots and sit in slot order, a body's own insertions
  // contiguous.  The insertion order of Solver::add_constraint is the caller's body order: walk the bodies in it.
  const size_t n = w->n_owned;
  std::vector<uint32_t> base(n + 1);
  MGF_TRY(d2h(w->ctx, base.data(), w->base.p, n + 1));
  if (base[n] != w->C) return fail(MGF_ERR_HIP, "internal error: constraint ranges do not cover the list");
  size_t o = 0;
  for (size_t e = 0; e < n; ++e) {
    const uint32_t sl = w->h_slot_of[e];
    for (uint32_t c = base[sl]; c < base[sl + 1]; ++c, ++o) {
      crec_to_public(h[c], &out[o]);
      out[o].a = (int32_t)w->h_ext_of[h[c].a];
      if (h[c].b != kNone) out[o].b = (int32_t)w->h_ext_of[h[c].b];
    }
  }
  return MGF_OK;
}
extern "C" mgf_status mgf_world_set_constraints(mgf_world* w, const mgf_constraint* cons, int64_t n) {
  if (!w || (n && !cons)) return fail(MGF_ERR_INVALID, "NULL argument");
  MGF_TRY(ctx_bind(w->ctx));
  MGF_TRY(perm_host(w));  // (the caller's records name bodies by the caller's indices; the store may hold them in other slots: host_perm.inc)
  w->n = std::max(w->n, w->n_owned);
  const uint32_t* so = w->permuted ? w->h_slot_of.data() : nullptr;
  if (n < 0 || n >= 0x7FFFFFF0ll) return fail(MGF_ERR_INVALID, "bad constraint count");
  std::vector<CRec> h((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    const mgf_constraint& c = cons[i];
    if (c.n_contacts != 1) return fail(MGF_ERR_INVALID, "only single-contact manifolds are supported on this path");
    if (c.a < 0 || (uint32_t)c.a >= w->n) return fail(MGF_ERR_STATIC_REF, "obj_a must be a Dynamic body in range");
    if (c.b >= 0 && (uint32_t)c.b >= w->n) return fail(MGF_ERR_INVALID, "obj_b out of range");
    if (c.a == c.b) return fail(MGF_ERR_INVALID, "a constraint needs two different bodies");
    CRec r;
    memset(&r, 0, sizeof(r));
    r.a = (uint32_t)c.a; r.b = c.b < 0 ? kNone : (uint32_t)c.b;
    if (so) {
      if (r.a >= w->n_owned || (r.b != kNone && r.b >= w->n_owned)) return fail(MGF_ERR_INVALID, "body index out of range");
      r.a = so[r.a]; if (r.b != kNone) r.b = so[r.b];
    }
    const float* src[5] = {&c.normal.x, &c.t0.x, &c.t1.x, &c.ra.x, &c.rb.x};
    float* dst[5] = {r.n, r.t0, r.t1, r.ra, r.rb};
    for (int k = 0; k < 5; ++k) memcpy(dst[k], src[k], 12);
    r.bias = c.bias; r.nmass = c.normal_mass; r.tmass0 = c.tangent_mass0; r.tmass1 = c.tangent_mass1; r.nimp = c.normal_impulse;
    r.friction = c.friction;
    h[(size_t)i] = r;
  }
  w->C = (uint32_t)n; w->Ct = 0;
  MGF_TRY(w->cons_nat.ensure(std::max<size_t>((size_t)n, 1), w->ctx->stream));
  MGF_TRY(h2d(w->ctx, w->cons_nat.p, h.data(), (size_t)n));
  memset(&w->stats, 0, sizeof(w->stats));
  w->stats.n_bodies = w->n; w->stats.n_constraints = w->C;
  StepCounts hc;
  memset(&hc, 0, sizeof(hc));
  hc.C = hc.need_C = w->C;
  MGF_TRY(h2d(w->ctx, w->sc.p, &hc, 1));
  w->flow5_ok = false; w->flow5_prepped = false; w->flow6_prepped = false;  // a caller's list has no per-body structure ...
  w->list_generic = true; w->f6_fail_known = false; w->tick_mode1 = false;    // ... the block-local solver builds its tables from the list's links (k_flow6g_*)
  MGF_TRY(links_ensure(w, w->C, true));
  if (w->C) {
    k_links_from_records<<<nblk(w->C), kBlock, 0, w->ctx->stream>>>(w->cons_nat.p, w->C, w->c_ab.p, w->deg.p);
    LAUNCH_CHECK();
  }
  MGF_TRY(build_dag(w, w->C));
  w->links_ready = true;
  w->constraints_ready = true;
  MGF_HIP_TRY(hipStreamSynchronize(w->ctx->stream));
  return MGF_OK;
}
