// mgf_world: the resident body store, options and counters, add_bodies, state access.
// Part of the single translation unit mgf_hip.hip (included there, in order); not compiled on its own.
// ---------------------------------------------------------------------------------------------
// World
// ---------------------------------------------------------------------------------------------
// What mgf_world_set_option stores (the table behind it names every key; the keys that do more than store a value are code there).
// mgf_world_clone copies the struct whole: an option added here is cloned.
struct WorldOptions {
  // the store's order and the cell grid
  int64_t resort_every = -1;           // ticks between two re-sorts of the store in the fused tick; 0 = never; -1 = automatic
  int64_t grid_min_frac_pct = 50;      // body grid: axes shorter than this percentage of the longest one are widened to it (grid_box)
  int64_t cell_fill = 16;              // bodies per Morton cell (in eighths) beyond which the cell grid gets another level
  bool cell_fill_set = false;          // the caller chose it (else a world with capsules uses 8: collide_prepare)
  int64_t cells_in_integrate = 1;      // the fused tick: k_integrate works out the bodies' Morton cells and ranks (over last tick's bounds) - no k_morton_count launch
  int64_t no_fused_scene_bounds = 0;   // 1: always the separate scene-bounds kernel
  int64_t no_fused_terrain_rows = 0;   // 1: always a separate terrain candidate kernel
  // the collide phase's paths
  int64_t two_pass = 0;                // 1 = always use the exact two-pass candidate path (tests the overflow fallback)
  int64_t terrain_tree = 0;            // 1 = always walk the mesh BVH (k_terrain_rows) instead of the face grid
  int64_t broadphase_tree = 0;         // 1 = always walk the tree (k_pair_rows) instead of enumerating grid cells
  int64_t pair_brick = 1;              // grid broadphase with the cells staged in LDS (k_pair_brick); 0 = every look-up from global memory (k_pair_grid)
  int64_t no_fused_narrowphase = 0;
  int64_t fused_contacts = 1;          // (r05) a world of spheres: rows -> constraint records in one launch, no candidate lists (k_contacts_spheres; 0: k_lists_spheres + k_setup_pairs)
  // (r07) k_contacts_rows in two: the numbering (k_contacts_rows_index) ahead of the solver's table kernels, the partner contacts' records beside them.
  // 1: as the last blocks of k_flow6_links' launch (k_flow6_links_records: the link blocks are all resident, the record blocks fill in around them);
  // experiments (EXPERIMENTS.md r07): 2: as its first blocks; 3: a launch of their own on the side stream, joined behind the links; 4: a launch of their
  // own on the main stream, always (what every path without tables in the collide phase does); 0: k_contacts_rows
  int64_t contacts_split = 1;
  // (r08) the tick's prefix sums inside their consumers' launches.  Bit 1: the constraint numbering of a world of spheres inside k_contacts_rows_index's
  // launch (k_contacts_rows_index_scan: no k_scan<1> launch over p_cnt + tcn; needs contacts_split); 0: tick_scan(job 2), then k_contacts_rows_index<true>
  int64_t scan_fused = 1;
  // (r09) the solver's block tables inside the numbering launch (k_contacts_rows_index_tables: what k_flow6_blocks builds - binfo, bref, the foreign bodies,
  // the rows' own part - from what the numbering holds in LDS; a ticket per solver block).  Runs when the numbering launch runs (scan_fused, spheres,
  // contacts_split), solver mode 6 builds its tables inside the collide phase, the store is re-sorted (blocks are runs of slots) and a block is no
  // longer than the launch's workgroup; everything else - and 0 - keeps the k_flow6_blocks launch
  int64_t tables_fused = 1;
  int64_t front_rows = 1;              // (r06) worlds of single-component bodies that are not all spheres: the list-free front end (k_front_rows.h; 0: candidate lists, one narrowphase launch per shape-pair type)
  int64_t front_rows_check = 0;        // tests: the faces k_terrain_near's cheap reject (comp_tri_far) drops go through the reference's tests as well; a contact among them is an internal error
  int64_t side_stream = 1;             // (r06) the terrain kernels of the list-free front end on the context's second stream, beside the pair search (0: one stream)
  // (r06) the wide bodies' list (WideSpec, k_bodies.h): engaged by the host when the scene's largest fat half extent jumps above 1.5 x what the
  // bodies had so far, from the tick after; the limit then follows the bodies that are not wide
  int64_t wide_list = 1;
  // constraint order "demo" (= 1): the reference's own insertion order, world.rs:233-291 - the partners
  // of body i in the DFS order of a world BVH that is refit (remove + insert) inside the loop.  Inherently sequential: the host
  // replays it on the reference-faithful HostBvh and hands the partner rows to the device (small scenes: BASELINE config 1).
  int64_t constraint_order = 0;
  // the solver:
  // 6 (default) = block-local dataflow launch with message channels (k_solve_flow6: every body a block touches, every arrival
  //     counter and the ready queue in LDS; hand-offs across block faces are tagged messages), k_solve_flow as its stand-by;
  // 5 = block-local dataflow launch k_solve_flow5 (bodies shared by two blocks and arrivals from other blocks go through
  //     global memory), same stand-by;
  // 1 = one persistent dataflow launch per Solver::solve, everything through L2 (k_solve_flow);
  // 0 = one launch per frontier of the dependency graph (k_solve, the independent cross-check);
  // 4 = dataflow launch with out-of-order slots per lane (k_solve_flowk)
  int64_t solver_mode = 6;
  int64_t flow_spin_limit = 0;         // tests: polls (x 256) a persistent launch waits before it gives up (0: the default, ~0.5 s)
  int64_t flow_max_blocks = 0;         // the persistent launches use at most this many workgroups (0: one per CU): processes that share a device each take a part
  int64_t flow_trace = 0;
  int64_t flow5_block = 0;             // minimum bodies per block of the block-local solver (tests)
  int64_t flow5_test_cap = 0;          // > 0: pretend a block of mode 5 holds at most this many constraints (tests: forces the k_solve_flow stand-by)
  int64_t flow6_fcap = 0;              // > 0: foreign body slots per block (tests / experiments); 0 = chosen from the last tick
  int64_t flow6_spec_wl = -1;          // worklist sweeps: positions behind the producers' hint read on spec (-1: by the launch's LDS plan)
  int64_t flow6_spec = 0;              // positions behind a channel's head the polling wave's quiet sweep reads on spec (1..8; 0 = by the launch: 8 where the bodies'
                                       // constants sit in LDS - configs 3 / 5, tiles: -1 % - and 4 where they do not: the settled pile loses 3 % at 8)
  int64_t flow6_poll_waves = 0;        // polling waves per block (0: by the launch's LDS plan)
  int64_t flow6_const_lds = 1;         // 1: the own bodies' inverse mass / inertia in LDS when the block's constraints leave room; 2: always; 0: never
  int64_t flow6_foreign_lds = 1;       // mode 6: the FOREIGN bodies' inverse mass / inertia in LDS as well when there is room (k_solve_flow6<., 2, ...>)
  int64_t flow6_quad = 1;              // mode 6: four lanes per node, the solve component-parallel with DPP quad permutes (k_solve_flow6<.., QD>)
  int64_t flow6_quad_max = -1;         // ... while the ready queue holds at most this many nodes (more: a one-lane-per-node trip of up to 64); -1 = automatic (host_solver.inc: flow6_args)
  int64_t flow6_slot_margin = 0;       // mode 6: what the LDS split allows a block's slots to grow over the last tick's largest block: 0 = an eighth + 64, v > 0 = 1 / v + 32 (experiments: tools/scratch/rl_calib.sh)
  int64_t flow6_rec_lds = 1;           // mode 6: the solver half of every constraint record in LDS for the launch when the blocks' slots leave room (k_solve_flow6<.., RL>)
  int64_t flow6_nimp_lds = 1;          // mode 6: the constraints' accumulated normal impulses in LDS for the launch when there is room
  int64_t flow6_test_cap = 0;          // > 0: pretend a block holds at most this many constraints (tests: forces the stand-by kernel)
  // the host's side of the tick
  int64_t pipeline = 1;                // mgf_world_step_many enqueues tick k + 1 before it waits for tick k
  int64_t readback_kernel = 1;         // the tick's read-back: k_publish writes pinned memory + a sequence word the host polls; 0 = hipMemcpyAsync + an event
  int64_t stream_ordered = 0;          // 1: the tiling calls (begin_tick, export_*, import_*) do not synchronise the ctx stream
  int64_t time_solver_kernels = 0;
  int64_t phase_timing = 0;            // HIP events at the tick's phase boundaries (mgf_step_stats::ms_*): each is a barrier packet, ~8-15 us of an idle GPU - off unless asked for
};
// HIP events around the phases of a query call (host_query.inc, host_batch_query.inc, host_batch_observe.inc).  They live with the
// handle, created at the first call that marks them: a query call creates and destroys none.
struct QueryEvents {
  hipEvent_t e[3] = {nullptr, nullptr, nullptr};
  QueryEvents() = default;
  QueryEvents(const QueryEvents&) = delete;
  QueryEvents& operator=(const QueryEvents&) = delete;
  ~QueryEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
  mgf_status mark(int k, hipStream_t s) {
    if (!e[k]) MGF_HIP_TRY(hipEventCreate(&e[k]));
    MGF_HIP_TRY(hipEventRecord(e[k], s));
    return MGF_OK;
  }
  // milliseconds from mark a to mark b; the caller has waited for the stream, or for b (wait)
  mgf_status wait(int k) { MGF_HIP_TRY(hipEventSynchronize(e[k])); return MGF_OK; }
  mgf_status ms(int a, int b, float* out) { MGF_HIP_TRY(hipEventElapsedTime(out, e[a], e[b])); return MGF_OK; }
};

struct mgf_world {
  mgf_ctx* ctx = nullptr;
  mgf_params params;
  WorldOptions opt;
  uint32_t n = 0;        // local bodies = owned + ghosts of the current tick
  uint32_t n_owned = 0;  // bodies of this world's RigidBodyVec (added through add_bodies)
  bool has_sphere = false, has_capsule = false;
  bool has_compound = false;      // a body of several parts exists: the *_parts narrowphase kernels serve every pair
  uint32_t max_parts = 0;         // the most parts any body has (the *_parts kernels are instantiated for 2 and for kMaxParts = 4)
  DBuf<uint32_t> pcount;          // parts per body (0: an ordinary body); the four part arrays hold kMaxParts slots per body
  DBuf<float4> xl0, xl1, xw0, xw1;  // (r06) the parts of bodies of more than kMaxParts components (Bodies::xl0): local and world records, `x_used` of them
  uint32_t x_used = 0;
  DBuf<float4> lp0, lp1, wp0, wp1;
  DBuf<uint32_t> bflag_l, bscan_l;  // scratch of the compaction after a removal (keep flags, their scan); tags in transit
  DBuf<uint32_t> sel_blk;           // the tile selection's per-block counts / offsets and, behind them, its four totals (k_tile_select_*)
  DBuf<uint32_t> mig_cnt;  // migration: [0] left-goers, [1] right-goers (also remove_bodies' error word)
  DBuf<float4> mig_tmp;    // remove_bodies: compacted copy of every body array
  DBuf<float> state_pack;  // mgf_world_read_state: the requested arrays packed in the caller's order (k_pack_state) ...
  void* state_pin = nullptr; size_t state_pin_bytes = 0;  // ... and the pinned memory they are copied into
  // RigidBodyVec
  DBuf<float4> x, q, srec, sp0, sp1, ctor, imb, delta, einfo, col0, col1, tb_c, tb_r, fb_c, fb_r;
  DBuf<float4> bpk;              // (col0, delta, einfo, col1) side by side for the constraint setup: a per-tick copy, see Bodies::bpk
  // the store in an internal (cell) order: see host_perm.inc
  DBuf<uint32_t> ext_of, ext_new, slot_of;   // slot -> the caller's body index, scratch for the next order, and the inverse (valid while `permuted`)
  DBuf<float4> perm_tmp;
  bool permuted = false;
  bool sidx_valid = false;          // sidx (the last collide phase's cell order) names the current slots of the current bodies
  uint64_t ticks_since_resort = 0, n_resorts = 0;
  std::vector<uint32_t> h_ext_of, h_slot_of;
  bool h_perm_valid = false;
  const uint32_t* ext_ptr() const { return permuted ? ext_of.p : nullptr; }
  DBuf<uint32_t> part_keys[2], part_vals[2];  // partition_order's sort buffers
  float h_scene_ext[3] = {0, 0, 0};     // extents of the scene at the last read-back (fat-box centres)
  float h_scene_rmax[3] = {0, 0, 0};    // ... and the largest fat half extents
  bool list_generic = false;            // the constraint list is a caller's (no per-body structure): the block-local solver's tables come from the generic builder (k_flow6g_*)
  DBuf<uint32_t> f6_cslot, f6_clist;
  DBuf<uint32_t> iota;                  // 0, 1, 2, ...: "cell order = slots" for the block-local solver's tables (a re-sorted store: its blocks are runs of slots)
  size_t iota_n = 0;
  DBuf<uint32_t> cnt_e, base_e, canon;  // the tick's list in insertion order (k_canon_*): for the executors that walk ids in order
  bool canon_ready = false;
  // terrain (copy of the caller's Mesh)
  std::unique_ptr<mgf_mesh> terrain;
  // static Compounds as obstacles beside the Mesh (copies of the caller's; the oracle's World::obstacles)
  std::vector<std::unique_ptr<mgf_compound>> obstacles;
  DBuf<CompoundDev> d_obs;
  DBuf<float4> d_obs_center;
  // broadphase
  DBuf<uint32_t> cell_of, cell_rank, sidx;
  DBuf<QNode> lnodes;
  DBuf<LeafRec> leaves;
  DBuf<float4> ltb;              // cell-ordered tight boxes and cell regions (the queries of k_pair_brick)
  DBuf<float4> lcol;             // cell-ordered (collider, motion) copies for the fused sphere test of k_pair_grid
  // the wide bodies' list (option wide_list): the host's state
  bool wide_engaged = false, wide_tick_on = false;
  float wide_ref[3] = {0, 0, 0}, wide_limit[3] = {0, 0, 0};
  float shape_rmax[3] = {0, 0, 0};   // the largest fat half extent the bodies had AT REST when they were added (the reference a world starts from)
  uint32_t wide_hold = 0, wide_last = 0;
  uint64_t n_wide_ticks = 0, n_wide_overflows = 0;
  // ticks whose collide phase settled on each fast path (counted by collide_process; read-only, for tests that must prove a path ran):
  // [0] k_pair_brick, [1] the list-free front end (k_front_rows.h), [2] k_contacts_spheres' rows -> records without candidate lists,
  // [3] cells and ranks worked out by k_integrate over the last tick's box
  uint64_t n_path_ticks[7] = {0, 0, 0, 0, 0, 0, 0};
  // option contacts_split: the record half of this collide phase's k_contacts_rows is still to be launched (set by contacts_from_rows, consumed by
  // stage_links - fused into k_flow6_links' launch or launched alone; never true outside collide_enqueue), its arguments, and the ticks by path
  bool records_pending = false, rec_sph = false;
  Bodies rec_B;
  ContactsSpheres rec_A;
  uint64_t n_split_ticks[2] = {0, 0};  // [0] fused into the links launch (or beside it on the side stream), [1] a launch of their own
  bool f6_tables_early = false;  // this collide phase's numbering launch built k_flow6_blocks' tables (option tables_fused): flow6_build_tables skips that launch
  uint64_t n_tables_fused_ticks = 0;  // option tables_fused: ticks whose block tables were built inside the numbering launch
  uint64_t n_scan_fused_ticks[1] = {0};  // option scan_fused: [0] ticks whose constraints were numbered inside k_contacts_rows_index_scan's launch
  DBuf<float4> wide_list;
  // mgf_world_raycast_many / mgf_world_overlap_aabb_many (host_query.inc): the query's own grid and lists - nothing of the tick's is read or written
  DBuf<float4> q_bc, q_br;
  DBuf<uint32_t> q_cnt, q_start, q_items, q_large, q_misc, q_off, q_vals;
  DBuf<ParticleIn> q_parts; DBuf<int32_t> q_ign, q_hits; DBuf<float> q_boxes;
  DBuf<MovingIn> q_casts;
  uint32_t q_last_large = 0, q_last_cells = 0;
  float q_last_build_ms = 0.0f, q_last_run_ms = 0.0f;
  QueryEvents q_tm;  // 0 | the grid | 1 | the query pass | 2
  bool front_rows_off = false;       // the list-free front end switched off for good: a body accepted more faces than k_terrain_near lists
  uint64_t pair_brick_slow = 0;      // last tick: queries k_pair_brick answered from global memory (one lane each: slow)
  uint32_t pair_brick_off = 0;       // ticks left during which k_pair_grid runs instead (too many such queries: cells much denser or bodies much larger than the box copy allows)
  uint32_t pair_brick_backoff = 256;
  bool pair_brick_attr = false;
  DBuf<float4> sub_lo, sub_hi, sub2_lo, sub2_hi;
  DBuf<uint32_t> cell_lo, cell_cnt;
  DBuf<uint32_t> t_cnt, p_cnt, t_off, p_off, t_cand, t_owner, p_cand, p_owner, rows, rows_t;
  DBuf<uint32_t> flow_arr, flow_arr5;
  DBuf<uint64_t> flow_trace;
  // block-local solver (mode 5)
  DBuf<uint32_t> brank, f5_shared, f5_gcnt, f5_lslot, f5_wg_cnt;
  DBuf<F5Row> f5_table;
  bool flow5_zeroed = false;  // this tick's collide phase cleared the block-local solver's preparation counters too
  bool f6_fail_known = false;        // the host has read the block-local solver's preparation flags of the current list (a collide phase that was finished before the solve: tiles)
  uint32_t f6_fail_host = 0;
  bool f6_standby = false;           // the last block-local launch had the stand-by k_solve_flow enqueued behind it
  uint32_t f6_edges_block = 0;       // edges across block faces per iteration that the busiest block receives (the last prepared list, once read back)
  bool links_ready = false;          // (succ, pred) of the tick's list are built (k_chain_rows); false when k_flow6_links wrote the block tables instead
  bool flow5_ok = false, flow5_prepped = false;  // the constraint list came from collide (own-block ranges valid) / prep done
  uint32_t f5_nb = 0, f5_nblocks = 0;
  // block-local solver with message channels (mode 6, k_solver_flow6.h)
  DBuf<uint4> f6_binfo;
  DBuf<uint32_t> f6_bref, f6_fcnt, f6_fbody, f6_nslots, f6_in_key, f6_in_cnt, f6_out_key, f6_out_val, f6_chan_prefix;
  DBuf<uint8_t> f6_cflags, f6_skipwb;
  DBuf<F6Row> f6_table;
  DBuf<uint4> f6_mbox;
  DBuf<unsigned long long> f6_tails;
  uint32_t f6_mbox_cap = 0;         // messages the channel buffer holds
  uint32_t f6_epoch = 0;            // tag of the launch's messages (never repeats, never 0)
  uint32_t f6_fcap = 512, f6_slot_cap = 0, f6_rows = 0;  // LDS split of the tick (chosen from the last tick's largest block)
  uint32_t f6_last_slots = 0, f6_last_foreign = 0;
  // (r06) what the last launch that did NOT fit needed, and the tick's constraint count then: while the estimate from it - the need scales
  // with the constraints - says the tables still would not fit, the block-local solver is not tried (a try that fails costs the tick a re-run:
  // a compacting pile of 343 000 spheres re-ran 42 of 160 ticks); cleared by a launch that fits
  uint32_t f6_fail_slots = 0, f6_fail_foreign = 0, f6_fail_C = 0, prev_C = 0;
  uint64_t n_flow6_skipped = 0;
  uint64_t f6_last_msgs = 0;        // messages the last prepared list needed
  uint64_t f6_last_block_msgs = 0;  // ... the most any block received
  bool flow6_prepped = false, flow6_zeroed = false;
  uint64_t f6_attr_mask = 0;  // variants of k_solve_flow6 whose dynamic LDS limit has been raised (lazily, at their first launch)
  uint32_t f6_prep_iters = 0;       // the iteration count the channels were laid out for
  uint64_t n_flow6_fallbacks = 0, n_flow6_runs = 0;  // Solver::solve calls the block-local kernel declined / ran
  // A persistent launch that gave up (not all of its workgroups became resident): the pre-launch velocities / impulses are restored and
  // the list is solved by the launch-per-frontier executor (solver_abort_fallback); the next `abort_backoff` solves use that executor at once
  DBuf<float4> vsnap; DBuf<float> nsnap;
  bool snap_valid = false, snap_nimp = false, snap_in_links = false, solver_aborted = false;
  bool finish_gave_up = false;     // mgf_world_finish met a stream-ordered launch that gave up (no snapshot to solve again from): mgf_tiles_step repeats the tick
  DBuf<float4> tick_snap;          // mgf_tiles_step: what a tick changes of a tile's owned bodies before anything can go wrong (x, q, v / w, delta, fat box)
  uint64_t n_solver_abort_fallbacks = 0;
  uint32_t abort_backoff = 0, abort_backoff_next = 16;
  int flow_grid = 0;
  // device-resident list sizes + speculative capacities (see StepCounts)
  // Everything the host reads back at the tick's one synchronisation lives in ONE device block, fetched with one copy:
  // [StepCounts | SceneBounds | scalars (frontier counters, error / flag words) | pair_stat (kPairStatWords partial sums
  // of the partners accepted by the fused broadphase)]
  DBuf<uint32_t> rb;
  static constexpr uint32_t kRbSc = 0, kRbSb = 16, kRbScalars = 32, kRbPairStat = 64, kRbWords = 64 + kPairStatWords;
  static_assert(kWLast < kRbPairStat - kRbScalars, "the flag words (FlagWord, common.h) lie inside the scalars block");
  // the solvers' flags, abort .. mode 6's edge counts: the run of words a solve fetches by itself (solver_flags_fetch, the tile set's batched copy)
  static constexpr uint32_t kSolverFlagsFirst = kWSolverAbort, kSolverFlagsWords = kWF6EdgesBlock - kWSolverAbort + 1;
  template <class T> struct View { T* p = nullptr; };
  View<StepCounts> sc;
  bool rb_fresh = false;         // the pinned copy of the block was fetched after the last solver launch was enqueued
  View<uint32_t> pair_stat;
  uint32_t cap_t = 0, cap_p = 0, cap_c = 0;
  uint64_t n_cap_retries = 0, n_flow5_fallbacks = 0;
  struct TickPlan { bool zero_launched = false, solver_follows = false; uint32_t n = 0, levels = 0, cells = 0, cap_c = 0; } plan;  // collide_prepare
  bool tick_two_pass = false;
  bool tick_mode1 = false;           // this tick's block-local solver tables did not fit: the tick is re-run with the global dataflow solver
  bool f6_tables_in_collide = false; // ... which works because the tables were built inside the collide phase, before its read-back
  uint32_t f6_collide_iters = 0;
  uint32_t row_cap_t = kRowCapT;    // terrain faces per body in the row path (grows on overflow, sticky)
  bool terrain_grid_off = false;    // sticky: the mesh's faces span too many cells for the face grid (k_terrain_grid)
  bool grid_too_wide = false;       // sticky: the largest body spans too many Morton cells for the grid broadphase
  int flowk_grid = 0;
  int f6_const_lds = 0;              // 0: the bodies' constants from global memory; 1: the own bodies' in LDS; 2: the foreign bodies' too
  bool f6_nimp_lds = false, f6_rec_lds = false;
  bool ptrs_out = false;             // mgf_world_device_ptr handed raw pointers out: the store keeps the caller's order until they are released
  uint32_t f6_fail_reason = 0;     // bits of the last fall-back (Flow6::fail)
  bool flow5_attr_set = false;
  bool flow5_wide = false;          // LDS layout of k_solve_flow5 for this tick (chosen from the largest block of the last one)
  uint32_t flow5_last_max = 0;
  uint32_t bounds_cover = 0;              // bodies [0, bounds_cover) are in the partial scene bounds gathered since this tick's k_integrate
                                          // (owned bodies, then imported ghosts); the next collide_enqueue uses them if that is every body
  uint32_t pack_cover = 0;                // bodies [0, pack_cover) have their bpk record written since this tick's k_integrate
  void invalidate_tick_caches() { bounds_cover = 0; terrain_rows_done = false; pack_cover = 0; cells_cover = 0; }  // the bodies were changed behind k_integrate's back
  // The counting sort's first half inside k_integrate (CellSort): the box its cells are quantised over is the previous tick's scene bounds,
  // copied by that tick's k_publish (sbg_valid: such a copy exists and the bodies are the ones it was taken of)
  DBuf<SceneBounds> sb_grid;
  bool sbg_valid = false;
  uint32_t cells_cover = 0, cells_levels = 0;  // bodies [0, cells_cover) have their cell and rank from this tick's k_integrate, for a grid of cells_levels
  DBuf<int> sb_part;                      // kBoundSlots partial scene-bounds records
  bool terrain_rows_done = false;         // this tick's k_integrate wrote rows_t / t_cnt (consumed by the next collide_enqueue)
  uint32_t rb_seq = 0;
  bool solve_pending = false;      // a dataflow launch was enqueued by mgf_world_solve_enqueue and not yet checked
  // constraint order "demo" (option constraint_order = 1): the host's replay of world.rs
  HostBvh demo_tree;
  std::vector<uint64_t> demo_leaf;   // body -> its leaf in demo_tree
  bool demo_rows_ready = false;      // this tick's partner rows (rows / p_cnt) came from the host replay
  uint64_t demo_candidates = 0;
  uint64_t n_row_overflows = 0;
  // narrowphase
  DBuf<uint32_t> scan_ws;        // status words + ticket of the tick's three k_scan launches (zeroed by the tick's clearing launch)
  uint32_t scan_tiles = 0;
  DBuf<uint32_t> t_nc, p_nc, t_pre, p_pre, cnt, tcn, base, work_lists, work_counts;
  DBuf<uint32_t> cs_sums, tpos;        // k_terrain_contacts: its two counters (+ the length of near_list), body -> first slot of its parked terrain contacts
  DBuf<uint32_t> front_cnt;            // k_terrain_near: kTnRegions slot counters + as many partial candidate counts, a cache line each
  DBuf<uint32_t> near_ids;             // k_near_list: the bodies whose tight box can reach the static mesh (face grid plan)
  DBuf<float4> near_list;              // the bodies that list a face, compacted by k_integrate's tail: 3 words each (TerrainRowsTail)
  DBuf<NContact> t_out, p_out;
  // solver
  DBuf<CRec> cons_nat;
  DBuf<uint2> c_ab, c_succ;  // compact dependency links (ConsLinks)
  DBuf<uint8_t> c_pred;
  DBuf<uint32_t> deg, adj_off, adj_fill, adj_list, order, lvl_off;
  DBuf<uint32_t> degb;           // per body: count ...
  DBuf<RevEnt> rev;              // ... and row (rev_cap entries) of the constraints it takes part in as `b`
  uint32_t rev_cap = 16;          // grows on overflow (kFailRevRow), sticky
  View<uint32_t> scalars;  // the flag words (FlagWord, common.h)
  View<SceneBounds> sb;
  uint32_t Mt = 0, Mp = 0, C = 0, Ct = 0, depth = 0, last_launches = 0, lvl_cap = 0;
  size_t order_cap_iters = 0;
  bool constraints_ready = false;
  float last_dt = 0.0f;
  float last_rmax_x = 0.0f;   // largest fat half extent along x among the tick's bodies, ghosts included (tiles: bounds the halo)
  float grid_occupancy = 1.0f;  // the part of the cell grid the scene actually covers (the last tick's bounds against the widened box: grid_box)
  // Per-tick host state that must survive while the NEXT tick is already being enqueued (mgf_world_step_many): phase
  // events, solver-kernel events, the pinned landing area of the read-back block.  Two slots, `ts` is the current one.
  struct TickSlot {
    hipEvent_t ev[8] = {};            // [0..6] phase boundaries (option phase_timing), [7] read-back done
    uint32_t ev_set = 0;              // which of [0..6] have been recorded since the option was switched on
    std::vector<hipEvent_t> kev;      // per-launch solver events (option time_solver_kernels)
    size_t kev_used = 0;
    bool brick = false;               // the tick ran k_pair_brick
    bool fused = false;               // the tick ran the fused sphere filter (the read-back includes the candidate statistic)
    bool front_rows = false;          // the tick ran the list-free front end of a world that is not spheres only (k_front_rows.h)
    bool contacts_fused = false;      // ... k_contacts_spheres: rows to constraint records without candidate lists
    bool cells_early = false;         // ... took its cells and ranks from k_integrate (over the last tick's box)
    bool two_pass = false;            // ... counted and filled its candidate lists in two passes (k_candidates)
    bool tree = false;                // ... searched its pairs in the tree (k_pair_rows), not in the cell grid
    bool split_fused = false, split_alone = false;  // ... wrote its partner records beside k_flow6_links / in a launch of their own (option contacts_split)
    bool tab_fused = false;           // ... and built the solver's block tables there too (option tables_fused)
    bool num_fused = false;           // ... numbered its constraints inside k_contacts_rows_index_scan's launch (option scan_fused, bit 1)
    bool big_parts = false;           // ... ran k_narrow_pairs_big / k_narrow_terrain_big (a body of more than kMaxParts components)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;  // the side stream's start and end inside the tick (no timing: created on first use)
    uint32_t* pin = nullptr;
    uint32_t* pin_dev = nullptr;      // the same memory as the device sees it (k_publish)
    uint32_t word(FlagWord k) const { return pin[kRbScalars + k]; }  // the host copy of a flag word, once the read-back (or solver_flags_fetch) has landed
    uint32_t seq = 0;                 // the read-back in flight carries this sequence number in pin[kPinSeqWord] (0: an event, ev[7], instead)
  };
  static constexpr uint32_t kPinWords = 4096, kPinSeqWord = 4095;
  void* pin_block = nullptr;        // pinned host memory behind slots[..].pin
  TickSlot slots[2];
  TickSlot* ts = &slots[0];
  mgf_step_stats stats;

  Bodies bodies() {
    Bodies B;
    B.x = x.p; B.q = q.p; B.srec = srec.p; B.sp0 = sp0.p; B.sp1 = sp1.p; B.ctor = ctor.p; B.imb = imb.p; B.bpk = bpk.p; B.delta = delta.p;
    B.einfo = einfo.p; B.col0 = col0.p; B.col1 = col1.p; B.tb_c = tb_c.p; B.tb_r = tb_r.p; B.fb_c = fb_c.p; B.fb_r = fb_r.p;
    B.pcount = has_compound ? pcount.p : nullptr; B.lp0 = lp0.p; B.lp1 = lp1.p; B.wp0 = wp0.p; B.wp1 = wp1.p;
    B.xl0 = xl0.p; B.xl1 = xl1.p; B.xw0 = xw0.p; B.xw1 = xw1.p;
    return B;
  }
  uint32_t* word(FlagWord k) { return scalars.p + k; }  // a flag word's device address; its host copy: TickSlot::word
  uint32_t flow5_narrow_cap() const { return f5_narrow_cap(f5_nb); }  // slots of the narrow LDS layout at this block size
  Flow5 flow5() {
    Flow5 F;
    F.sidx = sidx.p; F.brank = brank.p; F.shared = reinterpret_cast<uint8_t*>(f5_shared.p);
    F.gcnt = f5_gcnt.p; F.arr5 = flow_arr5.p; F.lslot = f5_lslot.p; F.wg_cnt = f5_wg_cnt.p;
    F.table = f5_table.p;
    F.fail = word(kWFlow5Fail); F.max_block = word(kWFlow5MaxBlock);
    F.cap_fast = flow5_wide ? kF5MaxFast : flow5_narrow_cap(); F.cap_slow = flow5_wide ? kF5MaxSlow : flow5_narrow_cap();
    F.cap_all = flow5_wide ? kF5MaxCons : flow5_narrow_cap();
    if (opt.flow5_test_cap > 0) F.cap_all = std::min<uint32_t>(F.cap_all, (uint32_t)opt.flow5_test_cap);  // tests: force the stand-by path
    F.slow_x2 = 3u;
    F.poller = flow5_wide ? 0u : 1u;  // one slow wave only polls the outside-arrival counters: with the narrow layout only (measured)
    F.nb = f5_nb; F.nblocks = f5_nblocks; F.n = n;
    return F;
  }
  ConsLinks links() { ConsLinks K; K.ab = c_ab.p; K.succ = c_succ.p; K.pred = c_pred.p; return K; }
  Frontier frontier() { Frontier F; F.order = order.p; F.lvl_off = lvl_off.p; F.cnt = word(kWFrontier0); return F; }
};
// The tick's phase-boundary events (mgf_step_stats::ms_integrate .. ms_total).  A HIP event on this stack is a barrier packet with a
// completion signal - 8 to 15 us of an idle GPU each, eight of them a tick (tools/trace_gaps.py: 45 us of a 0.81 ms tick) - so they
// are recorded only on request (option "phase_timing"); the fields read 0 otherwise.  [7], the read-back's event, is not one of them.
static mgf_status phase_mark(mgf_world* w, int k, hipStream_t s) {
  if (!w->opt.phase_timing) return MGF_OK;
  MGF_HIP_TRY(hipEventRecord(w->ts->ev[k], s));
  w->ts->ev_set |= 1u << k;
  return MGF_OK;
}
static mgf_status phase_ms(mgf_world* w, int a, int b, float* ms) {
  *ms = 0.0f;
  if (!w->opt.phase_timing || (w->ts->ev_set & (1u << a)) == 0u || (w->ts->ev_set & (1u << b)) == 0u) return MGF_OK;
  if (hipEventElapsedTime(ms, w->ts->ev[a], w->ts->ev[b]) != hipSuccess) { (void)hipGetLastError(); *ms = 0.0f; }  // (an event of another tick's slot: no figure)
  return MGF_OK;
}


static mgf_status world_identity(mgf_world* w);  // host_perm.inc
static mgf_status perm_host(mgf_world* w);

extern "C" mgf_status mgf_world_new(mgf_ctx* ctx, const mgf_params* params, mgf_world** out) {
  MGF_TRY(ctx_bind(ctx));
  if (!out) return fail(MGF_ERR_INVALID, "out is NULL");
  std::unique_ptr<mgf_world> w(new mgf_world());
  w->ctx = ctx;
  w->params = params ? *params : mgf_default_params();
  memset(&w->stats, 0, sizeof(w->stats));
  static_assert(sizeof(StepCounts) <= 64 && sizeof(SceneBounds) <= 64, "read-back block layout");
  MGF_TRY(w->rb.ensure(mgf_world::kRbWords, ctx->stream));
  MGF_HIP_TRY(hipMemsetAsync(w->rb.p, 0, 4 * (size_t)mgf_world::kRbWords, ctx->stream));
  w->sc.p = reinterpret_cast<StepCounts*>(w->rb.p + mgf_world::kRbSc);
  w->sb.p = reinterpret_cast<SceneBounds*>(w->rb.p + mgf_world::kRbSb);
  w->scalars.p = w->rb.p + mgf_world::kRbScalars;
  w->pair_stat.p = w->rb.p + mgf_world::kRbPairStat;
  MGF_HIP_TRY(hipMemsetAsync(w->sc.p, 0, sizeof(StepCounts), ctx->stream));
  MGF_HIP_TRY(hipMemsetAsync(w->scalars.p, 0, 64, ctx->stream));
  MGF_HIP_TRY(hipHostMalloc(&w->pin_block, 2 * 4096 * sizeof(uint32_t), hipHostMallocDefault));
  for (int sl = 0; sl < 2; ++sl) {
    for (auto& e : w->slots[sl].ev) MGF_HIP_TRY(hipEventCreate(&e));
    w->slots[sl].pin = static_cast<uint32_t*>(w->pin_block) + 4096 * sl;
    { void* dp = nullptr; if (hipHostGetDevicePointer(&dp, w->slots[sl].pin, 0) != hipSuccess) { (void)hipGetLastError(); dp = nullptr; } w->slots[sl].pin_dev = static_cast<uint32_t*>(dp); }  // (null: the read-back goes by hipMemcpyAsync + event)
    w->slots[sl].pin[mgf_world::kPinSeqWord] = 0u;  // (the world's own: several worlds of a context may have a tick in flight)
  }
  ctx_retain(ctx);
  *out = w.release();
  return MGF_OK;
}
extern "C" void mgf_world_free(mgf_world* w) {
  if (!w) return;
  mgf_ctx* ctx = w->ctx;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  for (auto& sl : w->slots) {
    for (auto& e : sl.ev) if (e) (void)hipEventDestroy(e);
    for (auto& e : sl.kev) (void)hipEventDestroy(e);
    if (sl.ev_fork) (void)hipEventDestroy(sl.ev_fork);
    if (sl.ev_join) (void)hipEventDestroy(sl.ev_join);
  }
  if (w->pin_block) (void)hipHostFree(w->pin_block);
  if (w->state_pin) (void)hipHostFree(w->state_pin);
  delete w;
  ctx_release(ctx);
}
extern "C" int64_t mgf_world_len(const mgf_world* w) { return w ? (int64_t)w->n_owned : 0; }

// The options that are a stored value.  lo > hi: any value is taken; else values outside [lo, hi] are refused with `range`.
// plan: the option changes which kernels the collide phase takes.  Whatever this tick's k_integrate gathered (terrain rows, scene bounds,
// packed records) was gathered under the old plan: such an option, set between mgf_world_begin_tick and mgf_world_collide, must not leave
// rows of the other kind behind.  (Only those: the tile drivers set "body_kinds" at exactly that point of every tick - invalidating there
// cost every tile-tick a second pass over the terrain rows and the scene bounds and the packed records, ~30 us.)
// prep: the block-local solvers' preparation of the current list is stale.
struct OptionEntry { const char* key; int64_t WorldOptions::*field; int64_t lo, hi; const char* range; bool plan, prep; };
static const OptionEntry kOptionTable[] = {
    {"time_solver_kernels", &WorldOptions::time_solver_kernels, 1, 0, nullptr, false, false},
    {"two_pass_candidates", &WorldOptions::two_pass, 1, 0, nullptr, true, false},
    {"broadphase_tree", &WorldOptions::broadphase_tree, 1, 0, nullptr, true, false},
    {"terrain_tree", &WorldOptions::terrain_tree, 1, 0, nullptr, true, false},
    {"no_fused_scene_bounds", &WorldOptions::no_fused_scene_bounds, 1, 0, nullptr, true, false},
    {"no_fused_terrain_rows", &WorldOptions::no_fused_terrain_rows, 1, 0, nullptr, true, false},
    {"grid_min_frac_pct", &WorldOptions::grid_min_frac_pct, 0, 100, "grid_min_frac_pct: 0..100", true, false},
    {"no_fused_narrowphase", &WorldOptions::no_fused_narrowphase, 1, 0, nullptr, false, false},
    {"pair_brick", &WorldOptions::pair_brick, 1, 0, nullptr, false, false},
    {"fused_contacts", &WorldOptions::fused_contacts, 1, 0, nullptr, false, false},
    {"contacts_split", &WorldOptions::contacts_split, 0, 4, "contacts_split: 0..4", false, false},
    {"scan_fused", &WorldOptions::scan_fused, 0, 1, "scan_fused: 0..1", false, false},
    {"tables_fused", &WorldOptions::tables_fused, 0, 1, "tables_fused: 0..1", false, false},
    {"front_rows", &WorldOptions::front_rows, 1, 0, nullptr, false, false},
    {"front_rows_check", &WorldOptions::front_rows_check, 1, 0, nullptr, false, false},
    {"side_stream", &WorldOptions::side_stream, 1, 0, nullptr, false, false},
    {"cells_in_integrate", &WorldOptions::cells_in_integrate, 1, 0, nullptr, false, false},
    {"solver_mode", &WorldOptions::solver_mode, 1, 0, nullptr, false, true},
    {"flow_trace", &WorldOptions::flow_trace, 1, 0, nullptr, false, false},
    {"flow_spin_limit", &WorldOptions::flow_spin_limit, 0, 4 << 20, "flow_spin_limit: 0 .. 4194304", false, false},
    {"flow5_test_cap", &WorldOptions::flow5_test_cap, 1, 0, nullptr, false, false},
    {"flow6_fcap", &WorldOptions::flow6_fcap, 0, 1536, "flow6_fcap out of range", false, false},
    {"flow6_const_lds", &WorldOptions::flow6_const_lds, 1, 0, nullptr, false, false},
    {"flow6_foreign_lds", &WorldOptions::flow6_foreign_lds, 1, 0, nullptr, false, false},
    {"flow6_nimp_lds", &WorldOptions::flow6_nimp_lds, 1, 0, nullptr, false, false},
    {"flow6_rec_lds", &WorldOptions::flow6_rec_lds, 1, 0, nullptr, false, false},
    {"flow6_slot_margin", &WorldOptions::flow6_slot_margin, 0, 1024, "flow6_slot_margin: 0..1024", false, false},
    {"flow6_quad", &WorldOptions::flow6_quad, 1, 0, nullptr, false, false},
    {"flow6_quad_max", &WorldOptions::flow6_quad_max, -1, 1000000, "flow6_quad_max out of range", false, false},
    {"flow6_test_cap", &WorldOptions::flow6_test_cap, 1, 0, nullptr, false, false},
    {"flow6_spec_wl", &WorldOptions::flow6_spec_wl, -1, 8, "flow6_spec_wl: -1..8", false, false},
    {"flow6_spec", &WorldOptions::flow6_spec, 0, 8, "flow6_spec: 0 (by the launch), 1..8", false, false},
    {"flow6_poll_waves", &WorldOptions::flow6_poll_waves, 0, 4, "flow6_poll_waves out of range", false, false},
    {"pipeline", &WorldOptions::pipeline, 1, 0, nullptr, false, false},
    {"stream_ordered", &WorldOptions::stream_ordered, 1, 0, nullptr, false, false},
};
extern "C" mgf_status mgf_world_set_option(mgf_world* w, const char* key, int64_t value) {
  if (!w || !key) return fail(MGF_ERR_INVALID, "NULL argument");
  for (const OptionEntry& e : kOptionTable) {
    if (strcmp(key, e.key)) continue;
    if (e.plan) w->invalidate_tick_caches();
    if (e.lo <= e.hi && (value < e.lo || value > e.hi)) return fail(MGF_ERR_INVALID, e.range);
    w->opt.*e.field = value;
    if (e.prep) { w->flow5_prepped = false; w->flow6_prepped = false; }
    return MGF_OK;
  }
  // the keys that do more than store a value
  if (!strcmp(key, "phase_timing")) { w->opt.phase_timing = value != 0; for (auto& sl : w->slots) sl.ev_set = 0; return MGF_OK; }
  if (!strcmp(key, "readback_kernel")) { w->opt.readback_kernel = value != 0; return MGF_OK; }
  if (!strcmp(key, "constraint_order")) {
    w->invalidate_tick_caches();  // (it changes the plan)
    if (value != 0 && value != 1) return fail(MGF_ERR_INVALID, "constraint_order: 0 = canonical, 1 = demo (world.rs order)");
    if (value != w->opt.constraint_order) { w->demo_tree.clear(); w->demo_leaf.clear(); }
    w->opt.constraint_order = value;
    if (value == 1) MGF_TRY(world_identity(w));  // (the replay walks the bodies in the caller's order)
    return MGF_OK;
  }
  if (!strcmp(key, "cell_fill")) {
    w->invalidate_tick_caches();  // (it changes the plan)
    if (value < 1 || value > 1024) return fail(MGF_ERR_INVALID, "cell_fill out of range");
    w->opt.cell_fill = value; w->opt.cell_fill_set = true;
    return MGF_OK;
  }
  if (!strcmp(key, "wide_list")) { w->opt.wide_list = value; if (!value) w->wide_engaged = false; return MGF_OK; }
  if (!strcmp(key, "flow5_block")) { w->opt.flow5_block = value; w->flow5_prepped = false; return MGF_OK; }  // (mode 5's preparation alone, as ever)
  if (!strcmp(key, "flow_max_blocks")) {
    if (value < 0 || value > 4096) return fail(MGF_ERR_INVALID, "flow_max_blocks: 0 (one workgroup per CU) .. 4096");
    w->opt.flow_max_blocks = value; w->flow_grid = 0; w->flowk_grid = 0; w->flow5_prepped = false; w->flow6_prepped = false;
    return MGF_OK;
  }
  if (!strcmp(key, "resort_every")) {  // the fused tick keeps the store in cell order, re-sorted every `value` ticks (host_perm.inc); 0 = the caller's order
    if (value < -1 || value > 1000000) return fail(MGF_ERR_INVALID, "resort_every out of range");
    w->opt.resort_every = value;
    if (value == 0) MGF_TRY(world_identity(w));
    return MGF_OK;
  }
  if (!strcmp(key, "body_kinds")) {  // OR-in: kinds (bit0 sphere, bit1 capsule, bit2 several parts, bit3 more than two parts) that ghosts / arrivals of this world may have
    if (value & 1) w->has_sphere = true;
    if (value & 2) w->has_capsule = true;
    if ((value & 12) == 12) w->max_parts = std::max(w->max_parts, (uint32_t)kMaxParts);  // (the *_parts kernels for four part slots)
    else if (value & 4) w->max_parts = std::max(w->max_parts, 2u);
    if ((value & 4) && !w->has_compound) {  // part arrays for every body so far: empty slots
      MGF_TRY(ctx_bind(w->ctx));
      const size_t o = w->n_owned;
      std::vector<uint32_t> pz(o, 0u);
      std::vector<float4> fz(kMaxParts * o, make_float4(0, 0, 0, 0));
      MGF_TRY(append(w->ctx, w->pcount, 0, pz));
      MGF_TRY(append(w->ctx, w->lp0, 0, fz)); MGF_TRY(append(w->ctx, w->lp1, 0, fz));
      MGF_TRY(append(w->ctx, w->wp0, 0, fz)); MGF_TRY(append(w->ctx, w->wp1, 0, fz));
      w->has_compound = true;
    }
    return MGF_OK;
  }
  if (!strcmp(key, "list_capacity")) {  // tests: force the speculative list capacities (the next tick must re-run its collide phase)
    if (value < 1 || value > 0x7FFFFFF0ll) return fail(MGF_ERR_INVALID, "list_capacity out of range");
    w->cap_t = w->cap_p = w->cap_c = (uint32_t)value;
    return MGF_OK;
  }
  return fail(MGF_ERR_INVALID, "unknown option");
}

extern "C" mgf_status mgf_world_counter(const mgf_world* w, const char* name, int64_t* out) {
  if (!w || !name || !out) return fail(MGF_ERR_INVALID, "NULL argument");
  if (!strcmp(name, "pair_brick_slow_queries")) { *out = (int64_t)w->pair_brick_slow; return MGF_OK; }
  if (!strcmp(name, "pair_brick_off_ticks")) { *out = (int64_t)w->pair_brick_off; return MGF_OK; }
  if (!strncmp(name, "scene_rmax_milli_", 17) && name[17] >= 'x' && name[17] <= 'z' && !name[18]) { *out = (int64_t)std::ceil((double)w->h_scene_rmax[name[17] - 'x'] * 1000.0); return MGF_OK; }
  if (!strncmp(name, "scene_ext_milli_", 16) && name[16] >= 'x' && name[16] <= 'z' && !name[17]) { *out = (int64_t)std::ceil((double)w->h_scene_ext[name[16] - 'x'] * 1000.0); return MGF_OK; }
  if (!strcmp(name, "grid_levels")) { *out = (int64_t)w->plan.levels; return MGF_OK; }
  if (!strcmp(name, "max_fat_half_extent_x_milli")) { *out = (int64_t)std::ceil((double)w->last_rmax_x * 1000.0); return MGF_OK; }
  if (!strncmp(name, "cross_probe_", 12)) {
    // development probe: share (ppm) of the tick's body pairs that straddle two blocks of 1024 bodies when the bodies are ordered by
    // a space-filling curve over their positions: cross_probe_morton / cross_probe_hilbert (10 bits per axis over the scene's box)
    *out = 0;
    mgf_world* mw = const_cast<mgf_world*>(w);
    const size_t n = w->n;
    if (!w->constraints_ready || w->C == 0 || n == 0) return MGF_OK;
    MGF_TRY(ctx_bind(mw->ctx));
    std::vector<float4> x(n);
    MGF_TRY(d2h(mw->ctx, x.data(), mw->x.p, n));
    float lo[3] = {3e38f, 3e38f, 3e38f}, hi[3] = {-3e38f, -3e38f, -3e38f};
    for (const float4& v : x) { const float c[3] = {v.x, v.y, v.z}; for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], c[k]); hi[k] = std::max(hi[k], c[k]); } }
    float ext = 0.0f;
    for (int k = 0; k < 3; ++k) ext = std::max(ext, hi[k] - lo[k]);
    const bool hilbert = name[12] == 'h';
    std::vector<std::pair<uint32_t, uint32_t>> key(n);
    for (size_t i = 0; i < n; ++i) {
      uint32_t X[3];
      const float c[3] = {x[i].x, x[i].y, x[i].z};
      for (int k = 0; k < 3; ++k) X[k] = (uint32_t)std::min(1023.0f, std::max(0.0f, (c[k] - lo[k]) / ext * 1023.0f));
      if (hilbert) {  // Skilling's transform: axes -> transposed Hilbert index, 10 bits
        const uint32_t M = 1u << 9;
        for (uint32_t Q = M; Q > 1; Q >>= 1) {
          const uint32_t P = Q - 1;
          for (int k = 0; k < 3; ++k) {
            if (X[k] & Q) X[0] ^= P;
            else { const uint32_t t = (X[0] ^ X[k]) & P; X[0] ^= t; X[k] ^= t; }
          }
        }
        for (int k = 1; k < 3; ++k) X[k] ^= X[k - 1];
        uint32_t t = 0;
        for (uint32_t Q = M; Q > 1; Q >>= 1) if (X[2] & Q) t ^= Q - 1;
        for (int k = 0; k < 3; ++k) X[k] ^= t;
      }
      uint32_t code = 0;
      for (int b = 9; b >= 0; --b) for (int k = 0; k < 3; ++k) code = (code << 1) | ((X[k] >> b) & 1u);
      key[i] = {code, (uint32_t)i};
    }
    std::sort(key.begin(), key.end());
    std::vector<uint32_t> rank(n);
    for (size_t r = 0; r < n; ++r) rank[key[r].second] = (uint32_t)r;
    std::vector<uint2> ab(w->C);
    MGF_TRY(d2h(mw->ctx, ab.data(), mw->c_ab.p, (size_t)w->C));
    uint64_t pairs = 0, cross = 0;
    for (const uint2& e : ab) {
      if (e.y == kNone) continue;
      ++pairs;
      if (rank[e.x] / 1024u != rank[e.y] / 1024u) ++cross;
    }
    *out = pairs ? (int64_t)(1000000.0 * (double)cross / (double)pairs) : 0;
    return MGF_OK;
  }
  if (!strcmp(name, "store_displacement_x1000") || !strcmp(name, "cross_block_pairs_by_cell_ppm") || !strcmp(name, "cross_block_pairs_by_slot_ppm")) {
    // development probes (tools/store_probe.py): how far the store's order has drifted from the last tick's cell order - mean
    // |slot - cell rank| - and the share of the tick's body pairs that straddle two blocks of 1024 bodies when blocks are runs of
    // the cell order / of the slots
    *out = 0;
    mgf_world* mw = const_cast<mgf_world*>(w);
    const size_t n = w->n;
    if (!w->sidx_valid || n == 0) return MGF_OK;
    MGF_TRY(ctx_bind(mw->ctx));
    std::vector<uint32_t> rank(n);
    MGF_TRY(d2h(mw->ctx, rank.data(), mw->brank.p, n));
    if (name[0] == 's') {
      double acc = 0.0;
      for (size_t s = 0; s < n; ++s) acc += std::fabs((double)rank[s] - (double)s);
      *out = (int64_t)(1000.0 * acc / (double)n);
      return MGF_OK;
    }
    if (!w->constraints_ready || w->C == 0) return MGF_OK;
    std::vector<uint2> ab(w->C);
    MGF_TRY(d2h(mw->ctx, ab.data(), mw->c_ab.p, (size_t)w->C));
    const bool by_slot = name[21] == 's';
    uint64_t pairs = 0, cross = 0;
    for (const uint2& e : ab) {
      if (e.y == kNone) continue;
      ++pairs;
      const uint32_t ga = (by_slot ? e.x : rank[e.x]) / 1024u, gb = (by_slot ? e.y : rank[e.y]) / 1024u;
      if (ga != gb) ++cross;
    }
    *out = pairs ? (int64_t)(1000000.0 * (double)cross / (double)pairs) : 0;
    return MGF_OK;
  }
  if (!strcmp(name, "store_resorts")) { *out = (int64_t)w->n_resorts; return MGF_OK; }
  if (!strcmp(name, "store_permuted")) { *out = w->permuted ? 1 : 0; return MGF_OK; }
  if (!strcmp(name, "row_overflows")) { *out = (int64_t)w->n_row_overflows; return MGF_OK; }
  if (!strcmp(name, "capacity_retries")) { *out = (int64_t)w->n_cap_retries; return MGF_OK; }
  if (!strcmp(name, "flow5_fallbacks")) { *out = (int64_t)w->n_flow5_fallbacks; return MGF_OK; }
  if (!strcmp(name, "flow6_fallbacks")) { *out = (int64_t)w->n_flow6_fallbacks; return MGF_OK; }
  if (!strcmp(name, "wide_bodies")) { *out = (int64_t)w->wide_last; return MGF_OK; }
  if (!strcmp(name, "query_large_bodies")) { *out = (int64_t)w->q_last_large; return MGF_OK; }
  if (!strcmp(name, "query_cells")) { *out = (int64_t)w->q_last_cells; return MGF_OK; }
  if (!strcmp(name, "query_build_ns")) { *out = (int64_t)std::llround((double)w->q_last_build_ms * 1e6); return MGF_OK; }
  if (!strcmp(name, "query_run_ns")) { *out = (int64_t)std::llround((double)w->q_last_run_ms * 1e6); return MGF_OK; }
  if (!strcmp(name, "pair_brick_ticks")) { *out = (int64_t)w->n_path_ticks[0]; return MGF_OK; }
  if (!strcmp(name, "front_rows_ticks")) { *out = (int64_t)w->n_path_ticks[1]; return MGF_OK; }
  if (!strcmp(name, "fused_contacts_ticks")) { *out = (int64_t)w->n_path_ticks[2]; return MGF_OK; }
  if (!strcmp(name, "early_cells_ticks")) { *out = (int64_t)w->n_path_ticks[3]; return MGF_OK; }
  if (!strcmp(name, "two_pass_ticks")) { *out = (int64_t)w->n_path_ticks[4]; return MGF_OK; }
  if (!strcmp(name, "tree_ticks")) { *out = (int64_t)w->n_path_ticks[5]; return MGF_OK; }
  if (!strcmp(name, "big_parts_ticks")) { *out = (int64_t)w->n_path_ticks[6]; return MGF_OK; }
  if (!strcmp(name, "contacts_split_fused")) { *out = (int64_t)w->n_split_ticks[0]; return MGF_OK; }
  if (!strcmp(name, "contacts_split_standalone")) { *out = (int64_t)w->n_split_ticks[1]; return MGF_OK; }
  if (!strcmp(name, "scan_fused_numbering_ticks")) { *out = (int64_t)w->n_scan_fused_ticks[0]; return MGF_OK; }
  if (!strcmp(name, "tables_fused_ticks")) { *out = (int64_t)w->n_tables_fused_ticks; return MGF_OK; }
  if (!strcmp(name, "scan_fused_look")) { *out = (int64_t)kNumLook * 64; return MGF_OK; }  // (runs per sweep of the numbering's look-back ...
  if (!strcmp(name, "scan_fused_run")) { *out = (int64_t)kNumSubs * kBlock; return MGF_OK; }  // ... and bodies per run)
  if (!strcmp(name, "contacts_records_pending")) { *out = w->records_pending ? 1 : 0; return MGF_OK; }
  if (!strcmp(name, "max_parts")) { *out = (int64_t)w->max_parts; return MGF_OK; }
  if (!strcmp(name, "wide_ticks")) { *out = (int64_t)w->n_wide_ticks; return MGF_OK; }
  if (!strcmp(name, "wide_overflows")) { *out = (int64_t)w->n_wide_overflows; return MGF_OK; }
  if (!strcmp(name, "flow6_skipped")) { *out = (int64_t)w->n_flow6_skipped; return MGF_OK; }
  if (!strcmp(name, "solver_abort_fallbacks")) { *out = (int64_t)w->n_solver_abort_fallbacks; return MGF_OK; }
  if (!strcmp(name, "device_ptrs_out")) { *out = w->ptrs_out ? 1 : 0; return MGF_OK; }  // 1: raw pointers are out - the store is pinned to the caller's order (slower ticks)
  if (!strcmp(name, "flow6_runs")) { *out = (int64_t)w->n_flow6_runs; return MGF_OK; }
  if (!strcmp(name, "flow6_const_lds")) { *out = w->f6_const_lds; return MGF_OK; }
  if (!strcmp(name, "flow6_nimp_lds")) { *out = w->f6_nimp_lds ? 1 : 0; return MGF_OK; }
  if (!strcmp(name, "flow6_rec_lds")) { *out = w->f6_rec_lds ? 1 : 0; return MGF_OK; }
  if (!strcmp(name, "flow6_fail_reason")) { *out = (int64_t)w->f6_fail_reason; return MGF_OK; }
  if (!strcmp(name, "flow6_max_slots")) { *out = (int64_t)w->f6_last_slots; return MGF_OK; }
  if (!strcmp(name, "flow6_max_foreign")) { *out = (int64_t)w->f6_last_foreign; return MGF_OK; }
  if (!strcmp(name, "flow6_slot_cap")) { *out = (int64_t)w->f6_slot_cap; return MGF_OK; }
  if (!strcmp(name, "flow6_fcap")) { *out = (int64_t)w->f6_fcap; return MGF_OK; }
  if (!strcmp(name, "grid_too_wide")) { *out = w->grid_too_wide ? 1 : 0; return MGF_OK; }
  if (!strcmp(name, "terrain_grid")) { *out = (w->terrain && w->terrain->grid.ready && !w->terrain_grid_off && !w->opt.terrain_tree) ? 1 : 0; return MGF_OK; }
  if (!strcmp(name, "terrain_row_capacity")) { *out = (int64_t)w->row_cap_t; return MGF_OK; }
  if (!strcmp(name, "front_rows")) { *out = (w->opt.front_rows && !w->front_rows_off) ? 1 : 0; return MGF_OK; }
  if (!strcmp(name, "front_near") || !strcmp(name, "front_slots") || !strcmp(name, "front_faces")) {  // the last tick's: bodies near the mesh, faces that passed the cheap reject, faces accepted
    mgf_world* mw = const_cast<mgf_world*>(w);
    uint32_t v = 0;
    if (!strcmp(name, "front_near")) {
      if (mw->cs_sums.p) { MGF_TRY(ctx_bind(mw->ctx)); MGF_HIP_TRY(hipStreamSynchronize(mw->ctx->stream)); MGF_TRY(d2h(mw->ctx, &v, mw->cs_sums.p + 2 * (size_t)kCsSumStride, 1)); }
    } else if (mw->front_cnt.p) {
      std::vector<uint32_t> h(2 * (size_t)kTnRegions * kTnCntStride);
      MGF_TRY(ctx_bind(mw->ctx)); MGF_HIP_TRY(hipStreamSynchronize(mw->ctx->stream)); MGF_TRY(d2h(mw->ctx, h.data(), mw->front_cnt.p, h.size()));
      for (uint32_t r = 0; r < kTnRegions; ++r) v += h[(size_t)((!strcmp(name, "front_slots") ? 0u : kTnRegions) + r) * kTnCntStride];
    }
    *out = (int64_t)v;
    return MGF_OK;
  }
  if (!strcmp(name, "rev_row_capacity")) { *out = (int64_t)w->rev_cap; return MGF_OK; }
  if (!strcmp(name, "body_kinds")) { *out = (w->has_sphere ? 1 : 0) | (w->has_capsule ? 2 : 0) | (w->has_compound ? 4 : 0) | (w->has_compound && w->max_parts > 2u ? 8 : 0); return MGF_OK; }
  if (!strcmp(name, "flow5_blocks")) { *out = (int64_t)w->f5_nblocks; return MGF_OK; }
  if (!strncmp(name, "flow5_class", 11) && (name[11] == '0' || name[11] == '1' || name[11] == '2') && !name[12]) {
    // constraints of the last prepared tick in class 0 / 1 / 2 (all-LDS / global counter / LDS counter + shared body)
    *out = 0;
    if (!w->flow5_prepped || w->f5_nblocks == 0) return MGF_OK;
    std::vector<uint32_t> h(4 * (size_t)w->f5_nblocks * kF5CntStride);
    mgf_world* mw = const_cast<mgf_world*>(w);
    MGF_TRY(ctx_bind(mw->ctx));
    MGF_TRY(d2h(mw->ctx, h.data(), mw->f5_wg_cnt.p, h.size()));
    int k = name[11] - '0';
    for (uint32_t g = 0; g < w->f5_nblocks; ++g) *out += (int64_t)h[(size_t)(4 * g + k) * kF5CntStride];
    return MGF_OK;
  }
  if (!strcmp(name, "flow5_max_block") || !strcmp(name, "flow5_max_fast")) {  // largest block (all classes / class 0) of the last prepared tick
    *out = 0;
    if (!w->flow5_prepped || w->f5_nblocks == 0) return MGF_OK;
    std::vector<uint32_t> h(4 * (size_t)w->f5_nblocks * kF5CntStride);
    mgf_world* mw = const_cast<mgf_world*>(w);
    MGF_TRY(ctx_bind(mw->ctx));
    MGF_TRY(d2h(mw->ctx, h.data(), mw->f5_wg_cnt.p, h.size()));
    const bool fast = name[10] == 'f';
    for (uint32_t g = 0; g < w->f5_nblocks; ++g) {
      int64_t v = h[(size_t)(4 * g) * kF5CntStride];
      if (!fast) v += (int64_t)h[(size_t)(4 * g + 1) * kF5CntStride] + h[(size_t)(4 * g + 2) * kF5CntStride];
      *out = std::max(*out, v);
    }
    return MGF_OK;
  }
  return fail(MGF_ERR_INVALID, "unknown counter");
}

// The static mesh's face grid: face boxes = the leaf bounds of the reference tree, counting-sorted into Morton cells with
// the same kernels as the bodies; DFS ranks and parent links from the host tree.
static mgf_status build_face_grid(mgf_mesh* t) {
  mgf_ctx* ctx = t->ctx;
  hipStream_t s = ctx->stream;
  mgf_mesh::Grid& G = t->grid;
  G.ready = false;
  const size_t nf = t->faces.size() / 3;
  if (nf < 64 || t->m.tree.empty()) return MGF_OK;  // tiny meshes: the tree walk is cheap
  std::vector<uint32_t> rank_of, face_of, leaf_of, parent;
  t->m.tree.dfs_ranks(nf, &rank_of, &face_of, &leaf_of, &parent);
  if (face_of.size() != nf) return MGF_OK;  // a face without a leaf (or two): not a Mesh::push_face tree, keep the walk
  std::vector<float4> bc(nf), br(nf);
  for (size_t f = 0; f < nf; ++f) {
    const Box& b = t->m.tree.node(leaf_of[f]).box;
    bc[f] = make_float4(b.c.x, b.c.y, b.c.z, 0.0f); br[f] = make_float4(b.r.x, b.r.y, b.r.z, 0.0f);
  }
  uint32_t levels = 4;
  while (((uint64_t)1 << (2 * levels)) < nf && levels < (uint32_t)kMortonBits / 2) ++levels;
  // Cells per axis: about one cell per face in all (2^(2 levels) >= faces), the bits dealt out one by one to the axis whose cells are
  // still the longest - but no axis gets cells shorter than the largest face box along it (a query is padded by that much on either
  // side anyway: finer cells mean more cells to visit, not fewer faces), and none more than the 10 bits of the quantisation.  A
  // heightfield's vertical axis ends up with no bits at all: in the Morton grid of the bodies, which gives every axis the same number
  // of cells, a capsule near the floor visited 32 layers of almost empty cells (k_terrain_grid 108 us on config 3; now 1 layer).
  {
    float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f}, rmax[3] = {0, 0, 0};
    for (size_t f = 0; f < nf; ++f) {
      const float c[3] = {bc[f].x, bc[f].y, bc[f].z}, r[3] = {br[f].x, br[f].y, br[f].z};
      for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], c[k]); hi[k] = std::max(hi[k], c[k]); rmax[k] = std::max(rmax[k], r[k]); }
    }
    uint32_t bits[3] = {0, 0, 0};
    for (uint32_t given = 0; given < 2 * levels; ++given) {
      int best = -1;
      float best_len = 0.0f;
      for (int k = 0; k < 3; ++k) {
        const float len = (hi[k] - lo[k]) / (float)(1u << bits[k]);  // this axis' cells now
        if (bits[k] < 10u && len * 0.5f >= 2.0f * rmax[k] && len * 0.5f > 0.0f && len > best_len) { best = k; best_len = len; }
      }
      if (best < 0) break;
      ++bits[best];
    }
    G.bits[0] = bits[0]; G.bits[1] = bits[1]; G.bits[2] = bits[2];
  }
  const uint32_t cells = 1u << (G.bits[0] + G.bits[1] + G.bits[2]);
  G.levels = levels; G.n_faces = (uint32_t)nf;
  MGF_TRY(G.fb_c.ensure(nf, s)); MGF_TRY(G.fb_r.ensure(nf, s)); MGF_TRY(G.cell_of.ensure(nf, s)); MGF_TRY(G.cell_rank.ensure(nf, s));
  MGF_TRY(G.cell_cnt.ensure((size_t)cells + 1, s)); MGF_TRY(G.cell_lo.ensure((size_t)cells + 1, s)); MGF_TRY(G.sidx.ensure(nf, s));
  MGF_TRY(G.brank.ensure(nf, s)); MGF_TRY(G.leaves.ensure(nf, s)); MGF_TRY(G.sb.ensure(1, s));
  MGF_TRY(G.rank_of_face.ensure(nf, s)); MGF_TRY(G.face_of_rank.ensure(nf, s)); MGF_TRY(G.leaf_of_face.ensure(nf, s));
  MGF_TRY(G.parent.ensure(std::max<size_t>(parent.size(), 1), s));
  MGF_TRY(h2d(ctx, G.fb_c.p, bc.data(), nf)); MGF_TRY(h2d(ctx, G.fb_r.p, br.data(), nf));
  MGF_TRY(h2d(ctx, G.rank_of_face.p, rank_of.data(), nf)); MGF_TRY(h2d(ctx, G.face_of_rank.p, face_of.data(), nf));
  MGF_TRY(h2d(ctx, G.leaf_of_face.p, leaf_of.data(), nf)); MGF_TRY(h2d(ctx, G.parent.p, parent.data(), parent.size()));
  MGF_HIP_TRY(hipMemsetAsync(G.cell_cnt.p, 0, ((size_t)cells + 1) * 4, s));
  SceneBounds sb0;
  for (int k = 0; k < 3; ++k) { sb0.lo[k] = 0x7FFFFFFF; sb0.hi[k] = (int)0x80000000; sb0.rmax[k] = 0; }
  sb0.n_refits = 0; sb0.pad = 0; sb0.pad2 = 0;
  MGF_TRY(h2d(ctx, G.sb.p, &sb0, 1));
  k_scene_bounds<<<std::min<unsigned>(nblk(nf), 256u), kBlock, 0, s>>>(G.fb_c.p, G.fb_r.p, (uint32_t)nf, G.sb.p);
  LAUNCH_CHECK();
  if (G.bits[0] + G.bits[1] + G.bits[2] == 0) return MGF_OK;  // (a mesh no axis of which can be cut: the tree walk)
  k_morton_count<<<nblk(nf), kBlock, 0, s>>>(G.fb_c.p, (uint32_t)nf, G.sb.p, kMortonBits - 2 * (int)levels, G.cell_of.p, G.cell_rank.p, G.cell_cnt.p, 0.0f,
                                             make_uint3(G.bits[0], G.bits[1], G.bits[2]));
  LAUNCH_CHECK();
  MGF_TRY(prim_exclusive_scan_u32(ctx, G.cell_cnt.p, G.cell_lo.p, (size_t)cells + 1));
  FaceGrid FG = t->face_grid();
  k_scatter_leaves<<<nblk(nf), kBlock, 0, s>>>(FG.T, G.fb_c.p, G.fb_r.p, G.cell_of.p, G.cell_rank.p, G.brank.p, nullptr, nullptr, nullptr, nullptr, nullptr, 0.0f, 0.0f);
  LAUNCH_CHECK();
  MGF_HIP_TRY(hipStreamSynchronize(s));
  G.ready = true;
  return MGF_OK;
}

extern "C" mgf_status mgf_world_set_terrain(mgf_world* w, const mgf_mesh* mesh) {
  if (!w) return fail(MGF_ERR_INVALID, "world is NULL");
  w->invalidate_tick_caches();  // (bounds / terrain rows gathered by k_integrate no longer describe the bodies)
  MGF_TRY(ctx_bind(w->ctx));
  if (!mesh) { w->terrain.reset(); return MGF_OK; }
  std::unique_ptr<mgf_mesh> t(new mgf_mesh());
  t->ctx = w->ctx;
  t->x = mesh->x;
  t->verts = mesh->verts;
  t->faces = mesh->faces;
  t->m.tree = mesh->m.tree;
  t->geom_version = 1;
  MGF_TRY(t->sync());
  MGF_TRY(build_face_grid(t.get()));
  w->terrain = std::move(t);
  w->terrain_grid_off = false;
  return MGF_OK;
}


// A static Compound (compound.rs:230-352) as an obstacle of the world, beside the Mesh: every tick each body's parts are put through
// Compound::contacts (:334-352) after the body's terrain contacts, obstacles in the order they were added, and every contact is a
// constraint against Static{center: the compound's displacement, friction: 0} (world.rs:243-251 with the compound in the Mesh's
// place; the reference's World holds a Mesh only - the definition is the oracle's World::obstacles).  The compound is copied.
extern "C" mgf_status mgf_world_add_obstacle(mgf_world* w, const mgf_compound* c) {
  if (!w || !c) return fail(MGF_ERR_INVALID, "NULL argument");
  if (w->obstacles.size() >= kObstacleMax) return fail(MGF_ERR_CAPACITY, "at most 256 obstacles");
  if (c->comps.size() >= kObstacleCompMax) return fail(MGF_ERR_CAPACITY, "an obstacle holds at most 2^18 components");
  MGF_TRY(ctx_bind(w->ctx));
  w->invalidate_tick_caches();
  std::unique_ptr<mgf_compound> o(new mgf_compound());
  o->ctx = w->ctx;
  o->comps = c->comps;
  o->m.tree = c->m.tree;
  o->disp = c->disp; o->rot = c->rot;
  MGF_TRY(o->sync());
  w->obstacles.push_back(std::move(o));
  std::vector<CompoundDev> h;
  std::vector<float4> hc;
  for (auto& ob : w->obstacles) { h.push_back(ob->dev(w->word(kWStackOverflow))); hc.push_back(make_float4(ob->disp.x, ob->disp.y, ob->disp.z, 0.0f)); }
  MGF_TRY(w->d_obs.ensure(h.size(), w->ctx->stream)); MGF_TRY(w->d_obs_center.ensure(h.size(), w->ctx->stream));
  MGF_TRY(h2d(w->ctx, w->d_obs.p, h.data(), h.size())); MGF_TRY(h2d(w->ctx, w->d_obs_center.p, hc.data(), hc.size()));
  w->constraints_ready = false;
  return MGF_OK;
}

// RigidBodyVec::add_body physics.rs:200-218 + World::add_body world.rs:178-184 (initial fat AABB).
extern "C" mgf_status mgf_world_add_bodies(mgf_world* w, const mgf_component* comps, int64_t n, const float* mass, const float* restitution,
                                           const float* friction, const mgf_vec3* world_force, uint64_t* first_id) {
  if (!w || (n && (!comps || !mass || !restitution || !friction || !world_force))) return fail(MGF_ERR_INVALID, "NULL argument");
  MGF_TRY(world_identity(w));
  w->sidx_valid = false;
  w->invalidate_tick_caches();  // (bounds / terrain rows gathered by k_integrate no longer describe the bodies)
  MGF_TRY(ctx_bind(w->ctx));
  w->n = w->n_owned;  // ghosts of a previous tick are dropped
  if (first_id) *first_id = w->n_owned;
  if (n <= 0) return MGF_OK;
  if ((uint64_t)w->n_owned + (uint64_t)n > 0x7FFFFFF0ull) return fail(MGF_ERR_INVALID, "too many bodies");
  size_t N = (size_t)n;
  std::vector<float4> hx(N), hq(N), hs(4 * N), h0(N), h1(N), hc(N), hi(3 * N), hd(N), he(N), c0(N), c1(N), tc(N), tr(N), fc(N), fr(N);
  bool hs_ = w->has_sphere, hc_ = w->has_capsule;
  for (size_t i = 0; i < N; ++i) {
    const mgf_component& mc = comps[i];
    if (mc.tag != MGF_SPHERE && mc.tag != MGF_CAPSULE) return fail(MGF_ERR_INVALID, "component tag must be sphere or capsule");
    if (!(mc.r > 0.0f)) return fail(MGF_ERR_INVALID, "radius must be > 0 (geom.rs:300,328)");
    Comp k = comp_of(mc);
    if (k.kind == KIND_SPHERE) k.d = mk3(0, 0, 0);
    // Component::deconstruct compound.rs:42-52
    V3 px; Quat pq; float half_h = 0.0f;
    if (k.kind == KIND_SPHERE) { px = k.p; pq = mkq(1.0f, mk3(0, 0, 0)); hs_ = true; }
    else {
      float h = mag(k.d);
      pq = quat_from_arc(mk3(0.0f, 1.0f, 0.0f) * h, k.d);
      px = k.p + k.d * 0.5f;
      half_h = h * 0.5f;
      hc_ = true;
    }
    Comp local = k; local.p = k.p + -px;  // collider - x.to_vec()
    M3 inv;
    if (!invert(tensor_of(local, mass[i]), &inv)) return fail(MGF_ERR_SINGULAR, "inertia tensor is not invertible (physics.rs:212)");
    float inv_mass = 1.0f / mass[i];
    V3 force = mk3(world_force[i].x, world_force[i].y, world_force[i].z) * mass[i];
    hx[i] = make_float4(px.x, px.y, px.z, 0.0f);
    hq[i] = make_float4(pq.s, pq.v.x, pq.v.y, pq.v.z);
    hs[4 * i] = make_float4(0, 0, 0, 0);
    hs[4 * i + 1] = make_float4(0, 0, inv_mass, inv.c[0].x);
    hs[4 * i + 2] = make_float4(inv.c[0].y, inv.c[0].z, inv.c[1].x, inv.c[1].y);
    hs[4 * i + 3] = make_float4(inv.c[1].z, inv.c[2].x, inv.c[2].y, inv.c[2].z);
    h0[i] = make_float4(force.x, force.y, force.z, restitution[i]);
    h1[i] = make_float4(0, 0, 0, friction[i]);
    uint32_t kind_bits = (uint32_t)k.kind;
    float kf; memcpy(&kf, &kind_bits, 4);
    hc[i] = make_float4(kf, k.r, half_h, 0.0f);
    for (int c = 0; c < 3; ++c) hi[3 * i + c] = make_float4(inv.c[c].x, inv.c[c].y, inv.c[c].z, 0.0f);
    hd[i] = make_float4(0, 0, 0, friction[i]);
    he[i] = make_float4(px.x, px.y, px.z, restitution[i]);
    c0[i] = make_float4(k.p.x, k.p.y, k.p.z, k.r);
    c1[i] = make_float4(k.d.x, k.d.y, k.d.z, kf);
    Box tb = swept_bounds(k, mk3(0, 0, 0));
    tc[i] = make_float4(tb.c.x, tb.c.y, tb.c.z, 0); tr[i] = make_float4(tb.r.x, tb.r.y, tb.r.z, 0);
    V3 fm = mk3(w->params.fat_margin, w->params.fat_margin, w->params.fat_margin);
    V3 frr = tb.r + fm;
    fc[i] = tc[i]; fr[i] = make_float4(frr.x, frr.y, frr.z, 0);
    w->shape_rmax[0] = std::max(w->shape_rmax[0], frr.x); w->shape_rmax[1] = std::max(w->shape_rmax[1], frr.y); w->shape_rmax[2] = std::max(w->shape_rmax[2], frr.z);
  }
  mgf_ctx* ctx = w->ctx;
  size_t o = w->n_owned;
  w->sbg_valid = false; w->ptrs_out = false;  // (only here, where the arrays grow: raw pointers handed out die with them, the next tick quantises its cells over its own bounds - a rejected or empty call leaves a zero-copy user's pointers pinned)
  MGF_TRY(append(ctx, w->x, o, hx)); MGF_TRY(append(ctx, w->q, o, hq)); MGF_TRY(append(ctx, w->srec, 4 * o, hs));
  MGF_TRY(append(ctx, w->sp0, o, h0)); MGF_TRY(append(ctx, w->sp1, o, h1)); MGF_TRY(append(ctx, w->ctor, o, hc));
  MGF_TRY(append(ctx, w->imb, 3 * o, hi)); MGF_TRY(append(ctx, w->delta, o, hd)); MGF_TRY(append(ctx, w->einfo, o, he));
  MGF_TRY(append(ctx, w->col0, o, c0)); MGF_TRY(append(ctx, w->col1, o, c1)); MGF_TRY(append(ctx, w->tb_c, o, tc));
  MGF_TRY(append(ctx, w->tb_r, o, tr)); MGF_TRY(append(ctx, w->fb_c, o, fc)); MGF_TRY(append(ctx, w->fb_r, o, fr));
  if (w->has_compound) {  // ordinary bodies in a world that has bodies of several parts: empty part slots
    std::vector<uint32_t> pz(N, 0u);
    std::vector<float4> fz(kMaxParts * N, make_float4(0, 0, 0, 0));
    MGF_TRY(append(ctx, w->pcount, o, pz));
    MGF_TRY(append(ctx, w->lp0, kMaxParts * o, fz)); MGF_TRY(append(ctx, w->lp1, kMaxParts * o, fz));
    MGF_TRY(append(ctx, w->wp0, kMaxParts * o, fz)); MGF_TRY(append(ctx, w->wp1, kMaxParts * o, fz));
  }
  w->n_owned += (uint32_t)n;
  w->n = w->n_owned;
  w->has_sphere = hs_; w->has_capsule = hc_;
  w->constraints_ready = false;
  return MGF_OK;
}

// Bodies of several components (BASELINE config 5).  NOT in the reference (physics.rs:200 takes one Component); the
// definition is the oracle's RigidBodyVec::add_compound_body: mass = sum, x = centre of mass, q = identity, tensor = sum
// of the components' tensors about the centre of mass (physics.rs:30-93), parts fixed in the body frame.
extern "C" mgf_status mgf_world_add_compound_bodies(mgf_world* w, const mgf_component* comps, const float* comp_mass, const int64_t* offsets,
                                                    int64_t n, const float* restitution, const float* friction, const mgf_vec3* world_force,
                                                    uint64_t* first_id) {
  if (!w || (n && (!comps || !comp_mass || !offsets || !restitution || !friction || !world_force))) return fail(MGF_ERR_INVALID, "NULL argument");
  MGF_TRY(world_identity(w));
  w->sidx_valid = false;
  w->invalidate_tick_caches();  // (bounds / terrain rows gathered by k_integrate no longer describe the bodies)
  MGF_TRY(ctx_bind(w->ctx));
  w->n = w->n_owned;
  if (first_id) *first_id = w->n_owned;
  if (n <= 0) return MGF_OK;
  if ((uint64_t)w->n_owned + (uint64_t)n > 0x7FFFFFF0ull) return fail(MGF_ERR_INVALID, "too many bodies");
  const size_t N = (size_t)n, o = w->n_owned;
  std::vector<float4> hx(N), hq(N), hs(4 * N), h0(N), h1(N), hc(N), hi(3 * N), hd(N), he(N), c0(N), c1(N), tc(N), tr(N), fc(N), fr(N);
  std::vector<uint32_t> hp(N);
  std::vector<float4> l0(kMaxParts * N, make_float4(0, 0, 0, 0)), l1(l0), w0(l0), w1(l0);
  std::vector<float4> xa0, xa1, xb0, xb1;  // (the pool's new records: local, world)
  bool hs_ = w->has_sphere, hc_ = w->has_capsule;
  for (size_t b = 0; b < N; ++b) {
    const int64_t k0 = offsets[b], k1 = offsets[b + 1];
    if (k1 <= k0 || k1 - k0 > kBigParts) return fail(MGF_ERR_INVALID, "a body needs 1..32 components");
    Comp part[kBigParts];
    float total = 0.0f;
    V3 acc = mk3(0, 0, 0);
    for (int64_t k = k0; k < k1; ++k) {
      const mgf_component& mc = comps[k];
      if (mc.tag != MGF_SPHERE && mc.tag != MGF_CAPSULE) return fail(MGF_ERR_INVALID, "component tag must be sphere or capsule");
      if (!(mc.r > 0.0f)) return fail(MGF_ERR_INVALID, "radius must be > 0 (geom.rs:300,328)");
      Comp c = comp_of(mc);
      if (c.kind == KIND_SPHERE) { c.d = mk3(0, 0, 0); hs_ = true; } else hc_ = true;
      part[k - k0] = c;
      total += comp_mass[k];
      acc = acc + comp_center(c) * comp_mass[k];
    }
    const V3 com = acc / total;
    M3 t = m3_cols(mk3(0, 0, 0), mk3(0, 0, 0), mk3(0, 0, 0));
    for (int64_t k = k0; k < k1; ++k) { Comp l = part[k - k0]; l.p = l.p + -com; t = t + tensor_of(l, comp_mass[k]); }
    M3 inv;
    if (!invert(t, &inv)) return fail(MGF_ERR_SINGULAR, "inertia tensor is not invertible");
    const float inv_mass = 1.0f / total;
    const V3 force = mk3(world_force[b].x, world_force[b].y, world_force[b].z) * total;
    hx[b] = make_float4(com.x, com.y, com.z, 0.0f);
    hq[b] = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
    hs[4 * b] = make_float4(0, 0, 0, 0);
    hs[4 * b + 1] = make_float4(0, 0, inv_mass, inv.c[0].x);
    hs[4 * b + 2] = make_float4(inv.c[0].y, inv.c[0].z, inv.c[1].x, inv.c[1].y);
    hs[4 * b + 3] = make_float4(inv.c[1].z, inv.c[2].x, inv.c[2].y, inv.c[2].z);
    h0[b] = make_float4(force.x, force.y, force.z, restitution[b]);
    h1[b] = make_float4(0, 0, 0, friction[b]);
    uint32_t kind_bits = 2u;  // constructor kind: a body of several parts
    float kf; memcpy(&kf, &kind_bits, 4);
    hc[b] = make_float4(kf, 0.0f, 0.0f, 0.0f);
    for (int c = 0; c < 3; ++c) hi[3 * b + c] = make_float4(inv.c[c].x, inv.c[c].y, inv.c[c].z, 0.0f);
    hd[b] = make_float4(0, 0, 0, friction[b]);
    he[b] = make_float4(com.x, com.y, com.z, restitution[b]);
    uint32_t sph = (uint32_t)KIND_SPHERE; float sf; memcpy(&sf, &sph, 4);
    c0[b] = make_float4(com.x, com.y, com.z, 0.0f);  // the carrier: a radius-0 sphere at the centre of mass
    c1[b] = make_float4(0, 0, 0, sf);
    Box tb;
    for (int64_t k = k0; k < k1; ++k) {
      const Comp& c = part[k - k0];
      uint32_t kb = (uint32_t)c.kind; float kbf; memcpy(&kbf, &kb, 4);
      const V3 lp = c.p + -com;
      if (k1 - k0 > kMaxParts) {  // a body of many parts: into the pool, its offset into the body's first local slot (Bodies::xl0)
        if (k == k0) { const uint32_t off = w->x_used + (uint32_t)xa0.size(); float of; memcpy(&of, &off, 4); l0[kMaxParts * b] = make_float4(of, 0.0f, 0.0f, 0.0f); }
        xa0.push_back(make_float4(lp.x, lp.y, lp.z, c.r)); xa1.push_back(make_float4(c.d.x, c.d.y, c.d.z, kbf));
        xb0.push_back(make_float4(c.p.x, c.p.y, c.p.z, c.r)); xb1.push_back(make_float4(c.d.x, c.d.y, c.d.z, kbf));
      } else {
      l0[kMaxParts * b + (k - k0)] = make_float4(lp.x, lp.y, lp.z, c.r);
      l1[kMaxParts * b + (k - k0)] = make_float4(c.d.x, c.d.y, c.d.z, kbf);
      w0[kMaxParts * b + (k - k0)] = make_float4(c.p.x, c.p.y, c.p.z, c.r);
      w1[kMaxParts * b + (k - k0)] = make_float4(c.d.x, c.d.y, c.d.z, kbf);
      }
      Box pb = swept_bounds(c, mk3(0, 0, 0));
      tb = k == k0 ? pb : box_combine(tb, pb);
    }
    hp[b] = (uint32_t)(k1 - k0);
    tc[b] = make_float4(tb.c.x, tb.c.y, tb.c.z, 0); tr[b] = make_float4(tb.r.x, tb.r.y, tb.r.z, 0);
    const V3 fm = mk3(w->params.fat_margin, w->params.fat_margin, w->params.fat_margin), frr = tb.r + fm;
    fc[b] = tc[b]; fr[b] = make_float4(frr.x, frr.y, frr.z, 0);
    w->shape_rmax[0] = std::max(w->shape_rmax[0], frr.x); w->shape_rmax[1] = std::max(w->shape_rmax[1], frr.y); w->shape_rmax[2] = std::max(w->shape_rmax[2], frr.z);
  }
  mgf_ctx* ctx = w->ctx;
  if (!w->has_compound && o > 0) {  // the bodies added so far are ordinary: empty part slots for them
    std::vector<uint32_t> pz(o, 0u);
    std::vector<float4> fz(kMaxParts * o, make_float4(0, 0, 0, 0));
    MGF_TRY(append(ctx, w->pcount, 0, pz));
    MGF_TRY(append(ctx, w->lp0, 0, fz)); MGF_TRY(append(ctx, w->lp1, 0, fz)); MGF_TRY(append(ctx, w->wp0, 0, fz)); MGF_TRY(append(ctx, w->wp1, 0, fz));
  }
  w->sbg_valid = false; w->ptrs_out = false;  // (only here, where the arrays grow: raw pointers handed out die with them, the next tick quantises its cells over its own bounds - a rejected or empty call leaves a zero-copy user's pointers pinned)
  MGF_TRY(append(ctx, w->x, o, hx)); MGF_TRY(append(ctx, w->q, o, hq)); MGF_TRY(append(ctx, w->srec, 4 * o, hs));
  MGF_TRY(append(ctx, w->sp0, o, h0)); MGF_TRY(append(ctx, w->sp1, o, h1)); MGF_TRY(append(ctx, w->ctor, o, hc));
  MGF_TRY(append(ctx, w->imb, 3 * o, hi)); MGF_TRY(append(ctx, w->delta, o, hd)); MGF_TRY(append(ctx, w->einfo, o, he));
  MGF_TRY(append(ctx, w->col0, o, c0)); MGF_TRY(append(ctx, w->col1, o, c1)); MGF_TRY(append(ctx, w->tb_c, o, tc));
  MGF_TRY(append(ctx, w->tb_r, o, tr)); MGF_TRY(append(ctx, w->fb_c, o, fc)); MGF_TRY(append(ctx, w->fb_r, o, fr));
  MGF_TRY(append(ctx, w->pcount, o, hp));
  MGF_TRY(append(ctx, w->lp0, kMaxParts * o, l0)); MGF_TRY(append(ctx, w->lp1, kMaxParts * o, l1));
  MGF_TRY(append(ctx, w->wp0, kMaxParts * o, w0)); MGF_TRY(append(ctx, w->wp1, kMaxParts * o, w1));
  if (!xa0.empty()) {
    MGF_TRY(append(ctx, w->xl0, w->x_used, xa0)); MGF_TRY(append(ctx, w->xl1, w->x_used, xa1));
    MGF_TRY(append(ctx, w->xw0, w->x_used, xb0)); MGF_TRY(append(ctx, w->xw1, w->x_used, xb1));
    w->x_used += (uint32_t)xa0.size();
  }
  w->has_compound = true;
  for (size_t b = 0; b < N; ++b) w->max_parts = std::max(w->max_parts, (uint32_t)(offsets[b + 1] - offsets[b]));
  w->n_owned += (uint32_t)n;
  w->n = w->n_owned;
  w->has_sphere = hs_; w->has_capsule = hc_;
  w->constraints_ready = false;
  return MGF_OK;
}

// ---- state access ----------------------------------------------------------------------------
// the pinned staging area of the state transfers (mgf_world_read_state / write_state)
static mgf_status state_pin_ensure(mgf_world* w, size_t bytes) {
  if (w->state_pin_bytes >= bytes) return MGF_OK;
  if (w->state_pin) { (void)hipStreamSynchronize(w->ctx->stream); (void)hipHostFree(w->state_pin); w->state_pin = nullptr; w->state_pin_bytes = 0; }
  const size_t want = bytes + bytes / 4;
  MGF_HIP_TRY(hipHostMalloc(&w->state_pin, want, hipHostMallocDefault));
  w->state_pin_bytes = want;
  return MGF_OK;
}
extern "C" mgf_status mgf_world_read_state(mgf_world* w, mgf_vec3* x, mgf_quat* q, mgf_vec3* v, mgf_vec3* omega, mgf_vec3* delta, int64_t cap) {
  if (!w) return fail(MGF_ERR_INVALID, "world is NULL");
  MGF_TRY(ctx_bind(w->ctx));
  const size_t n = w->n_owned;
  if ((int64_t)n > cap) return fail(MGF_ERR_CAPACITY, "state buffers too small");
  if (n == 0) return MGF_OK;
  // packed on the device in the caller's order (body e sits in slot slot_of[e]: host_perm.inc), one copy into pinned memory, then into the
  // caller's arrays: what crosses PCIe is what the caller gets
  hipStream_t s = w->ctx->stream;
  const size_t fl[5] = {x ? 3 * n : 0, q ? 4 * n : 0, v ? 3 * n : 0, omega ? 3 * n : 0, delta ? 3 * n : 0};
  size_t off[6] = {0, 0, 0, 0, 0, 0};
  for (int k = 0; k < 5; ++k) off[k + 1] = off[k] + ((fl[k] + 3) & ~(size_t)3);  // (every section 16-byte aligned: q goes out as float4)
  if (off[5] == 0) return MGF_OK;
  MGF_TRY(w->state_pack.ensure(off[5], s));
  MGF_TRY(state_pin_ensure(w, 4 * off[5]));
  float* P = w->state_pack.p;
  k_pack_state<<<nblk(n), kBlock, 0, s>>>(w->bodies(), (uint32_t)n, w->permuted ? w->slot_of.p : nullptr, x ? P + off[0] : nullptr, q ? P + off[1] : nullptr,
                                          v ? P + off[2] : nullptr, omega ? P + off[3] : nullptr, delta ? P + off[4] : nullptr);
  LAUNCH_CHECK();
  MGF_HIP_TRY(hipMemcpyAsync(w->state_pin, P, 4 * off[5], hipMemcpyDeviceToHost, s));
  MGF_HIP_TRY(hipStreamSynchronize(s));
  const float* H = static_cast<const float*>(w->state_pin);
  if (x) memcpy(x, H + off[0], 4 * fl[0]);
  if (q) memcpy(q, H + off[1], 4 * fl[1]);
  if (v) memcpy(v, H + off[2], 4 * fl[2]);
  if (omega) memcpy(omega, H + off[3], 4 * fl[3]);
  if (delta) memcpy(delta, H + off[4], 4 * fl[4]);
  return MGF_OK;
}
extern "C" mgf_status mgf_world_write_state(mgf_world* w, const mgf_vec3* x, const mgf_quat* q, const mgf_vec3* v, const mgf_vec3* omega,
                                            const mgf_vec3* delta, int64_t n_in) {
  if (w) w->sbg_valid = false;  // (the next tick quantises its cells over its own bounds)
  if (!w) return fail(MGF_ERR_INVALID, "world is NULL");
  MGF_TRY(ctx_bind(w->ctx));
  w->invalidate_tick_caches();  // (bounds / terrain rows gathered by k_integrate no longer describe the bodies)
  size_t n = w->n_owned;
  if ((size_t)n_in != n) return fail(MGF_ERR_INVALID, "n must equal the number of bodies");
  // A store in its internal order stays there (ADVICE r3): body i's row is slot_of[i], as the read paths translate.  (Putting the store
  // back into the caller's order first cost an un-permute now and three radix sorts a few ticks later, for a caller that writes every tick.)
  if (w->permuted) { w->n = w->n_owned; w->constraints_ready = false; w->C = w->Ct = 0; }  // (the tick's lists do not describe the new state)
  if (n == 0) return MGF_OK;
  // the caller's arrays through pinned memory in one copy, scattered into the slots on the device (k_unpack_state): nothing is read back
  hipStream_t s = w->ctx->stream;
  const size_t fl[5] = {x ? 3 * n : 0, q ? 4 * n : 0, v ? 3 * n : 0, omega ? 3 * n : 0, delta ? 3 * n : 0};
  size_t off[6] = {0, 0, 0, 0, 0, 0};
  for (int k = 0; k < 5; ++k) off[k + 1] = off[k] + ((fl[k] + 3) & ~(size_t)3);
  if (off[5]) {
    MGF_TRY(w->state_pack.ensure(off[5], s));
    MGF_TRY(state_pin_ensure(w, 4 * off[5]));
    float* H = static_cast<float*>(w->state_pin);
    if (x) memcpy(H + off[0], x, 4 * fl[0]);
    if (q) memcpy(H + off[1], q, 4 * fl[1]);
    if (v) memcpy(H + off[2], v, 4 * fl[2]);
    if (omega) memcpy(H + off[3], omega, 4 * fl[3]);
    if (delta) memcpy(H + off[4], delta, 4 * fl[4]);
    float* P = w->state_pack.p;
    MGF_HIP_TRY(hipMemcpyAsync(P, H, 4 * off[5], hipMemcpyHostToDevice, s));
    k_unpack_state<<<nblk(n), kBlock, 0, s>>>(w->bodies(), (uint32_t)n, w->permuted ? w->slot_of.p : nullptr, x ? P + off[0] : nullptr, q ? P + off[1] : nullptr,
                                              v ? P + off[2] : nullptr, omega ? P + off[3] : nullptr, delta ? P + off[4] : nullptr);
    LAUNCH_CHECK();
  }
  k_refresh_einfo<<<nblk(n), kBlock, 0, s>>>(w->bodies(), (uint32_t)n);
  LAUNCH_CHECK();
  MGF_HIP_TRY(hipStreamSynchronize(s));
  return MGF_OK;
}
extern "C" mgf_status mgf_world_read_colliders(mgf_world* w, mgf_moving_component* out, int64_t cap) {
  if (!w || !out) return fail(MGF_ERR_INVALID, "NULL argument");
  MGF_TRY(ctx_bind(w->ctx));
  size_t n = w->n_owned;
  if ((int64_t)n > cap) return fail(MGF_ERR_CAPACITY, "buffer too small");
  static_assert(sizeof(mgf_moving_component) == 44, "eleven 4-byte words, no padding: k_pack_colliders writes the struct as it lies");
  if (n == 0) return MGF_OK;
  hipStream_t s = w->ctx->stream;
  MGF_TRY(w->state_pack.ensure(11 * n, s));
  MGF_TRY(state_pin_ensure(w, 44 * n));
  k_pack_colliders<<<nblk(n), kBlock, 0, s>>>(w->bodies(), (uint32_t)n, w->permuted ? w->slot_of.p : nullptr, reinterpret_cast<uint32_t*>(w->state_pack.p));
  LAUNCH_CHECK();
  MGF_HIP_TRY(hipMemcpyAsync(w->state_pin, w->state_pack.p, 44 * n, hipMemcpyDeviceToHost, s));
  MGF_HIP_TRY(hipStreamSynchronize(s));
  memcpy(out, w->state_pin, 44 * n);
  return MGF_OK;
}
// ConstrainedSet::get physics.rs:273-304
extern "C" mgf_status mgf_world_get(mgf_world* w, const mgf_body_ref* r, mgf_velocity* vel, mgf_rigid_body_info* info) {
  if (!w || !r) return fail(MGF_ERR_INVALID, "NULL argument");
  MGF_TRY(ctx_bind(w->ctx));
  if (r->tag == 1) {
    if (vel) { vel->linear = {0, 0, 0}; vel->angular = {0, 0, 0}; }
    if (info) { info->x = r->center; info->restitution = 0.0f; info->friction = r->friction; info->inv_mass = 0.0f; for (float& f : info->inv_moment) f = 0.0f; }
    return MGF_OK;
  }
  if (r->index >= w->n_owned) return fail(MGF_ERR_INVALID, "index out of bounds");
  MGF_TRY(perm_host(w));
  const size_t slot = w->permuted ? w->h_slot_of[r->index] : (size_t)r->index;
  float4 s[4], e, d;
  MGF_TRY(d2h(w->ctx, s, w->srec.p + 4 * slot, 4));
  MGF_TRY(d2h(w->ctx, &e, w->einfo.p + slot, 1));
  MGF_TRY(d2h(w->ctx, &d, w->delta.p + slot, 1));
  if (vel) { vel->linear = {s[0].x, s[0].y, s[0].z}; vel->angular = {s[0].w, s[1].x, s[1].y}; }
  if (info) {
    info->x = {e.x, e.y, e.z}; info->restitution = e.w; info->friction = d.w; info->inv_mass = s[1].z;
    float im[9] = {s[1].w, s[2].x, s[2].y, s[2].z, s[2].w, s[3].x, s[3].y, s[3].z, s[3].w};
    memcpy(info->inv_moment, im, sizeof(im));
  }
  return MGF_OK;
}
// ConstrainedSet::set physics.rs:306-314
extern "C" mgf_status mgf_world_set(mgf_world* w, const mgf_body_ref* r, const mgf_velocity* vel) {
  if (!w || !r || !vel) return fail(MGF_ERR_INVALID, "NULL argument");
  MGF_TRY(ctx_bind(w->ctx));
  if (r->tag == 1) return MGF_OK;
  if (r->index >= w->n_owned) return fail(MGF_ERR_INVALID, "index out of bounds");
  MGF_TRY(perm_host(w));
  const size_t slot = w->permuted ? w->h_slot_of[r->index] : (size_t)r->index;
  float4 s[2];
  MGF_TRY(d2h(w->ctx, s, w->srec.p + 4 * slot, 2));
  s[0] = make_float4(vel->linear.x, vel->linear.y, vel->linear.z, vel->angular.x);
  s[1].x = vel->angular.y; s[1].y = vel->angular.z;
  return h2d(w->ctx, w->srec.p + 4 * slot, s, 2);
}
extern "C" mgf_status mgf_world_device_ptr(mgf_world* w, const char* name, void** ptr, int64_t* bytes) {
  if (!w || !name || !ptr) return fail(MGF_ERR_INVALID, "NULL argument");
  const size_t per = !strcmp(name, "x") || !strcmp(name, "q") || !strcmp(name, "delta") ? 16 : (!strcmp(name, "solver_rec") ? 64 : 0);
  if (!per) return fail(MGF_ERR_INVALID, "unknown array name");  // (before anything is pinned: a failed look-up must not cost the world its re-sort - ADVICE r4)
  MGF_TRY(world_identity(w));  // (the caller addresses the arrays by its own indices)
  w->invalidate_tick_caches();  // (bounds / terrain rows gathered by k_integrate no longer describe the bodies)
  // ... and it goes on addressing them that way: the store stays in the caller's order (no re-sort, host_perm.inc) until the
  // pointers are given back with mgf_world_release_device_ptrs - or die with the arrays (add / remove / import of bodies)
  w->ptrs_out = true;
  *ptr = !strcmp(name, "x") ? (void*)w->x.p : !strcmp(name, "q") ? (void*)w->q.p : !strcmp(name, "delta") ? (void*)w->delta.p : (void*)w->srec.p;
  if (bytes) *bytes = (int64_t)(per * w->n_owned);
  return MGF_OK;
}

extern "C" mgf_status mgf_world_release_device_ptrs(mgf_world* w) {
  if (!w) return fail(MGF_ERR_INVALID, "world is NULL");
  w->ptrs_out = false;
  return MGF_OK;
}

// The tiling entry points are synchronous by default (the caller may touch its buffers as soon as the call
// returns); with option stream_ordered = 1 they only enqueue on the ctx stream - for a caller that issues its
// own work (copies, RCCL) on that same stream (mgf_ctx_set_stream).
static mgf_status sync_unless_ordered(mgf_world* w) {
  if (!w->opt.stream_ordered) MGF_HIP_TRY(hipStreamSynchronize(w->ctx->stream));
  return MGF_OK;
}
