// mgf_batch_*: many small independent worlds, resident in HBM, stepped together - one launch per tick, a workgroup per world (k_batch.h).
// Part of the single translation unit mgf_hip.hip (included there, in order); not compiled on its own.
//
// The bodies of all worlds sit in one set of arrays, world after world.  Bodies are added on the host side of a mirror of those arrays
// (a world in the middle of the batch grows by insertion); the mirror goes up before the first call that needs the device and comes
// back down if bodies are added after that.  Every world has a share of the candidate and of the constraint storage; a tick that needs
// more than its share undoes itself on the device and is run again with more (counter "capacity_retries").
// The terrain is a table of meshes, copied one behind the other into one store each of nodes, vertices and faces as they are added, and
// per world an entry of the table (or none) and a mesh position; the kernels read a descriptor per world (BatchTerrains, k_batch.h), which
// goes up before the first tick or query behind a change.
// The obstacles are a table of static Compounds in the same way - every entry's threaded tree and components behind the last entry's in
// one store each - and per world a list of (entry, disp, rot); the kernels read a descriptor per list entry (BatchObstacles, k_batch.h).
// Both tables and all lists live beside the mirror: adding bodies behind a tick, or none yet, leaves them as they are.

// A rig of a batch - sensors, cameras, zones, contact sensors, feelers: the records in the caller's order, what is built from them when the rig is set, and the
// device copy of both (host_batch_rig.inc)
template <class Rec>
struct BatchRig {
  std::vector<Rec> recs;
  std::vector<uint4> items;     // BatchQueryPlan's work items: (world, first, count <= 256, -); the cameras': their tiles
  std::vector<uint32_t> order;  // ... and its order: sorted position -> the caller's index (the cameras have none)
  bool stale = false;           // the device copy is behind the rig or the batch's layout (mgf_batch_add_bodies)
  DBuf<float4> dev;             // the sections batch_rig_up lists, one behind the other ...
  size_t off[4] = {0, 0, 0, 0}; // ... section k at off[k]: items, records, order, worlds
};

// What the encoders of a joint rig keep in the handle (host_batch_joint_read.inc): a member for the hinges' and one for the sliders'
struct BatchJointTrace {
  DBuf<float4> tab;                     // the readings table, `rows` rows of an entry a joint: two words, four with the impulses (mgf_batch_set_hinge_trace, _set_slider_trace)
  int64_t rows = 0;                     // ... its rows; 0: no trace
  int32_t format = 0;                   // ... and MGF_HINGE_TRACE_READING / _FULL, MGF_SLIDER_TRACE_READING / _FULL
  DBuf<float4> out;                     // what the host-memory read of the rig downloads: two words a joint
};

// A rig of joints - ball joints, hinges, sliders (host_batch_joint.inc): the rig, and what a solve of it leaves in the handle
template <class Rec>
struct BatchJointRig : BatchRig<Rec> {
  DBuf<float> acc;                      // the impulses over a call, the kind's Rows::kFloats floats a joint
  DBuf<unsigned long long> skipped;     // joints that were skipped (a singular K, a word of the setup not finite), cumulative (counter "<kind>s_skipped")
  DBuf<float> w;                        // the motors' target table, `rows` rows of a float a joint (mgf_batch_set_hinge_targets, _slider_targets); the ball joints have none
  int64_t rows = 1;                     // ... its rows
  bool zero = true;                     // ... and: the rig was set behind the last table - it is one row of zeros, made where the rig goes up
};

struct mgf_batch {
  mgf_ctx* ctx = nullptr;
  mgf_params params;
  uint32_t K = 0;
  // the persistent rows of Bodies (k_bodies.h), words of 16 bytes a body; the last four - the local and the world parts, kMaxParts slots
  // a body - exist only in a batch that holds a body of several components (`parts`, mgf_batch_add_compound_bodies)
  enum { AX, AQ, ASREC, ASP0, ASP1, ACTOR, AIMB, ADELTA, AFBC, AFBR, ACOL0, ACOL1, ALP0, ALP1, AWP0, AWP1, kArr, kArrPlain = ALP0 };
  static constexpr int kWords[kArr] = {1, 1, 4, 1, 1, 1, 3, 1, 1, 1, 1, 1, kMaxParts, kMaxParts, kMaxParts, kMaxParts};
  bool parts = false;                // the batch has part rows: its tick is k_batch_parts.h's, the calls that read shapes are refused
  bool part_queries = false;         // option "part_queries": with part rows, rays, sweeps and box queries answer part by part (host_batch_part_query.inc)
  int n_arr() const { return parts ? (int)kArr : (int)kArrPlain; }
  DBuf<float4> pool;                 // ... and the kept contacts of its pairs of bodies, three words an entry, as many as constraint records
  std::vector<float4> hm[kArr];
  DBuf<float4> dm[kArr];
  DBuf<float4> bpk, undo;          // the tick's packed copy (4 a body); what a tick that did not fit puts back (7 a body)
  std::vector<uint32_t> h_n, h_off;  // bodies per world; their prefix sums (K + 1)
  bool dev_valid = false;            // the device arrays hold the state (else the mirror does)
  // the terrain table (its meshes concatenated on the device) and every world's entry of it (-1: none) and mesh position
  struct TerrainEntry { uint32_t node0, n_nodes, vert0, face0; V3 x; };
  std::vector<TerrainEntry> t_table;
  DBuf<float4> t_nodes, t_verts;
  DBuf<uint4> t_faces, t_desc;
  size_t t_n_nodes = 0, t_n_verts = 0, t_n_faces = 0;  // the stores' lengths (nodes: two words each)
  std::vector<int32_t> h_wt;
  std::vector<V3> h_wx;
  bool t_desc_stale = true;   // the descriptors on the device are behind the table or the assignments
  uint32_t t_worlds = 0;      // worlds whose terrain has a node, as of the descriptors on the device
  // the obstacle table and every world's list of it: (entry, pose) in the order the tick meets them
  struct ObstacleEntry { uint32_t node0, n_nodes, comp0; V3 disp; Quat rot; };
  struct ObstacleRef { uint32_t entry; V3 disp; Quat rot; };
  std::vector<ObstacleEntry> o_table;
  DBuf<float4> o_nodes;
  DBuf<CompIn> o_comps;
  DBuf<uint4> o_desc;
  std::vector<uint32_t> h_orange;       // per world first << 7 | count of its descriptors, as of the descriptors on the device
  size_t o_n_nodes = 0, o_n_comps = 0;  // the stores' lengths (nodes: two words each)
  std::vector<std::vector<ObstacleRef>> h_wo;
  bool o_desc_stale = true;   // the descriptors on the device are behind the lists (or the stores have moved)
  uint32_t o_worlds = 0;      // worlds whose list has an entry, as of the descriptors on the device
  // constraint storage
  std::vector<uint32_t> h_coff, h_cap, h_floor, h_qfloor, h_ccount;  // offsets / shares of the lists / the least a world has asked for (records, candidates) / length of the last tick's list
  bool lists_valid = false;
  DBuf<CRec> cons;
  DBuf<float4> cont, slot;
  DBuf<uint2> cand;
  DBuf<uint32_t> rows, d_off, d_coff, d_cap, d_qoff, d_qcap, d_qcount, ncq, d_done, d_stage, d_need, d_ccount, d_err, d_stats, d_na, d_degb;
  DBuf<float> pack;
  int64_t cons_per_body = 4;  // option "cons_per_body": a world's first share of the constraint storage; of the candidate storage it gets four times that
  int64_t capacity_retries = 0;
  uint32_t lds_set = 0;
  // the queries (host_batch_query.inc).  col0 / col1 are the collider a query sees: the component a body was added as until a tick has run
  // on it, then what that tick built - gathered from bpk by one launch before the first reader behind a mgf_batch_step (cols_stale)
  bool cols_stale = false;
  DBuf<float4> q_in;
  DBuf<int32_t> q_out;
  DBuf<uint32_t> q_cnt, q_off, q_vals;  // mgf_batch_overlap_aabb_many: hits per box, their prefix sums, the lists
  QueryEvents q_tm;  // 0 | a query pass | 1
  int64_t q_launches = 0;
  float q_run_ms = 0.0f;
  int64_t d_launches = 0;  // kernel launches of the last get / set / forces / impulses / copy call (host_batch_drive.inc, host_batch_dev.inc)
  // the device-pointer calls (host_batch_dev.inc)
  bool ccount_stale = false;            // a masked copy has changed d_ccount behind h_ccount: batch_ccount_fresh before the next reader
  DBuf<unsigned long long> v_skipped;   // records whose index was out of range, cumulative (counter "device_skipped")
  DBuf<uint32_t> v_cnt, v_off, v_seg;   // the setters' records per body, their prefix sums, the segments
  std::vector<uint2> w_pairs;           // mgf_batch_copy_worlds_where: the last call's pair table, as it is on the device in ...
  DBuf<uint2> w_pairs_d;                // ... this; uploaded (from w_pairs, which stays) only when the arrays differ
  bool w_pairs_up = false;
  int64_t w_uploads = 0;                // counter "pair_table_uploads"
  // the device-pointer queries (host_batch_query_dev.inc): the plan BatchQueryPlan builds on the host, built on the device
  DBuf<uint32_t> p_cnt, p_off;          // [2 (K + 1)] queries | work items per world; their prefix sums
  DBuf<int32_t> p_world;                // [n] the call's own copy of the worlds, -1: a skipped record
  DBuf<uint32_t> p_rank, p_order;       // [n] a query's rank within its world; sorted position -> the caller's index
  DBuf<uint4> p_items;                  // the work items
  // the rigs (host_batch_rig.inc): body-mounted ray sensors, depth cameras, box zones, contact sensors and feelers (host_batch_sensor.inc, _camera.inc, _zone.inc, _touch.inc, _feeler.inc)
  BatchRig<mgf_batch_sensor> sensors;   // on the device: items | records | order | worlds
  BatchRig<mgf_batch_camera> cameras;   // on the device: tiles | records - (camera, the camera's first pixel, x0 | y0 << 16, -): a tile of kCamTileW x kCamTileH pixels
  BatchRig<mgf_batch_zone> zones;       // on the device: items | records | order
  BatchRig<mgf_batch_touch> touches;    // on the device: items | records | order - the contact sensors (host_batch_touch.inc)
  BatchRig<mgf_batch_feeler> feelers;   // on the device: items | records | order | worlds - the feelers (host_batch_feeler.inc)
  BatchRig<mgf_batch_actuator> actuators;  // on the device: runs | records | order - the actuators; `items` holds the runs of one body (host_batch_actuator.inc)
  BatchRig<mgf_batch_spring> springs;   // on the device: runs | records | order - the springs; `items` holds the runs of one body's ENDS, `order` the ends (host_batch_spring.inc)
  BatchJointRig<mgf_batch_joint> joints;   // on the device: items | records | plan, slots - the ball joints; `items` holds a world's joints each, `order` the plan and the slots (host_batch_joint.inc)
  BatchJointRig<mgf_batch_hinge> hinges;   // on the device: items | records | plan, slots - the hinges, laid out as the ball joints are (host_batch_hinge.inc)
  BatchJointRig<mgf_batch_slider> sliders;  // on the device: items | records | plan, slots - the sliders, laid out as the ball joints are (host_batch_slider.inc)
  // ... and what a call on one of them has nowhere else to put
  DBuf<float> s_parts;                  // the particles of a sensor cast: 7 words a sensor
  size_t c_pixels = 0;                  // the pixels of the camera rig, camera by camera
  DBuf<float> c_parts, c_depth;         // of a camera cast: 7 words a pixel, one word a pixel
  DBuf<int32_t> c_world;                // [pixels] a pixel's world, written by the tile pass for the obstacle pass
  DBuf<int32_t> z_out;                  // what the host-memory read of the zones downloads: 1 + k words a zone, then - where asked for - six a zone
                                        // (host_batch_nearest.inc: records | k distances a zone | boxes)
  DBuf<float4> touch_out;               // what the host-memory read of the contact sensors downloads: four words a sensor
  DBuf<float> f_casts;                  // the casts of a feeler cast where the caller takes none: 11 words a feeler
  DBuf<unsigned long long> a_skipped;   // actuators whose gain * clamp(u) was not finite, cumulative (counter "actuators_skipped")
  DBuf<float> sp_wr;                    // the impulses of the springs, twelve floats a spring: written by one launch of a call, applied by the next
  DBuf<unsigned long long> sp_skipped;  // springs whose wrench was zeroed (len == 0, len or f * h not finite), cumulative (counter "springs_skipped")
  BatchJointTrace hinge_trace, slider_trace;  // the hinges' and the sliders' readings tables and staging buffers (host_batch_joint_read.inc)
  // the rollouts (host_batch_rollout.inc)
  DBuf<uint32_t> d_act;                 // per world, beside d_done: ticks of the call whose actuation the world has behind it (k_batch_rollout.h)
  int64_t r_launches = 0;               // launches of the last rollout call beyond its ticks' own (counter "rollout_launches")

  size_t total() const { return h_off.empty() ? 0 : h_off.back(); }
  Bodies bodies(size_t first) const {
    Bodies B;
    memset(&B, 0, sizeof(B));
    B.x = dm[AX].p + first; B.q = dm[AQ].p + first; B.srec = dm[ASREC].p + 4 * first; B.sp0 = dm[ASP0].p + first; B.sp1 = dm[ASP1].p + first;
    B.ctor = dm[ACTOR].p + first; B.imb = dm[AIMB].p + 3 * first; B.delta = dm[ADELTA].p + first; B.fb_c = dm[AFBC].p + first;
    B.fb_r = dm[AFBR].p + first; B.col0 = dm[ACOL0].p + first; B.col1 = dm[ACOL1].p + first; B.bpk = bpk.p + 4 * first;
    if (parts) {
      B.lp0 = dm[ALP0].p + kMaxParts * first; B.lp1 = dm[ALP1].p + kMaxParts * first;
      B.wp0 = dm[AWP0].p + kMaxParts * first; B.wp1 = dm[AWP1].p + kMaxParts * first;
    }
    return B;
  }
};
constexpr int mgf_batch::kWords[mgf_batch::kArr];

static void batch_offsets(mgf_batch* b) {
  b->h_off.assign(b->K + 1, 0u);
  for (uint32_t k = 0; k < b->K; ++k) b->h_off[k + 1] = b->h_off[k] + b->h_n[k];
}
// the bodies of the largest of the worlds [k0, k0 + nw), of the whole batch: what a kernel with a workgroup per world sizes its dynamic LDS by
static uint32_t batch_nmax(const mgf_batch* b, uint32_t k0, uint32_t nw) {
  uint32_t nmax = 0;
  for (uint32_t k = k0; k < k0 + nw; ++k) nmax = std::max(nmax, b->h_n[k]);
  return nmax;
}
static uint32_t batch_nmax(const mgf_batch* b) { return batch_nmax(b, 0u, b->K); }
// col0 / col1 of the bodies the last mgf_batch_step ran on: every world has completed every tick of the call (a tick that was undone was
// run again before the call returned), so bpk words 0 and 3 are their colliders.  The launches that follow on the stream see the rows.
static mgf_status batch_cols_refresh(mgf_batch* b, int64_t* launches) {
  if (!b->cols_stale || !b->dev_valid) return MGF_OK;
  const size_t n = b->total();
  if (n) {
    k_batch_query_gather<<<(unsigned)((n + kBatchBlock - 1) / kBatchBlock), kBatchBlock, 0, b->ctx->stream>>>(b->bpk.p, b->dm[mgf_batch::ACOL0].p,
                                                                                                       b->dm[mgf_batch::ACOL1].p, (uint32_t)n);
    LAUNCH_CHECK();
    if (launches) ++*launches;
  }
  b->cols_stale = false;
  return MGF_OK;
}
// the device arrays back into the mirror (bodies are being added behind a tick)
static mgf_status batch_pull(mgf_batch* b) {
  if (!b->dev_valid) return MGF_OK;
  MGF_TRY(batch_cols_refresh(b, nullptr));
  const size_t n = b->total();
  for (int a = 0; a < b->n_arr(); ++a) {
    b->hm[a].resize(n * mgf_batch::kWords[a]);
    MGF_TRY(d2h(b->ctx, b->hm[a].data(), b->dm[a].p, b->hm[a].size()));
  }
  b->dev_valid = false;
  return MGF_OK;
}
// h_ccount as the device has it, before a reader on the host: a masked copy (mgf_batch_copy_worlds_where) leaves it unknown
static mgf_status batch_ccount_fresh(mgf_batch* b) {
  if (!b->ccount_stale) return MGF_OK;
  if (b->dev_valid) MGF_TRY(d2h(b->ctx, b->h_ccount.data(), b->d_ccount.p, b->K));
  b->ccount_stale = false;
  return MGF_OK;
}
// every world's share of the constraint storage; the lists of the last tick move along when `keep`
static mgf_status batch_allot(mgf_batch* b, bool keep) {
  mgf_ctx* ctx = b->ctx;
  hipStream_t s = ctx->stream;
  std::vector<uint32_t> coff(b->K + 1, 0u), cap(b->K), qoff(b->K + 1, 0u), qcap(b->K);
  for (uint32_t k = 0; k < b->K; ++k) {
    const uint64_t qwant = std::max<uint64_t>({64ull, 4ull * (uint64_t)b->cons_per_body * b->h_n[k], (uint64_t)b->h_qfloor[k]});
    qcap[k] = (uint32_t)std::min<uint64_t>(qwant, 0x0FFFFFFFull);
    if ((uint64_t)qoff[k] + qcap[k] > 0x7FFFFFF0ull) return fail(MGF_ERR_OOM, "the batch's candidate lists exceed 2^31 entries");
    qoff[k + 1] = qoff[k] + qcap[k];
    const uint64_t want = std::max<uint64_t>({16ull, (uint64_t)b->cons_per_body * b->h_n[k], (uint64_t)b->h_floor[k]});
    cap[k] = (uint32_t)std::min<uint64_t>(want, 0x0FFFFFFFull);
    if ((uint64_t)coff[k] + cap[k] > 0x7FFFFFF0ull) return fail(MGF_ERR_OOM, "the batch's constraint lists exceed 2^31 records");
    coff[k + 1] = coff[k] + cap[k];
  }
  DBuf<CRec> ncons;
  DBuf<uint32_t> ncoff;
  MGF_TRY(ncons.ensure(std::max<size_t>(coff[b->K], 1), s));
  MGF_TRY(ncoff.ensure(b->K + 1, s));
  MGF_TRY(h2d(ctx, ncoff.p, coff.data(), coff.size()));
  if (keep && b->lists_valid && b->K) {
    k_batch_move_lists<<<b->K, kBatchBlock, 0, s>>>(b->cons.p, b->d_coff.p, ncons.p, ncoff.p, b->d_ccount.p);
    LAUNCH_CHECK();
    MGF_HIP_TRY(hipStreamSynchronize(s));
  } else {
    std::fill(b->h_ccount.begin(), b->h_ccount.end(), 0u);
    b->ccount_stale = false;
    MGF_TRY(b->d_ccount.ensure(std::max<size_t>(b->K, 1), s));
    MGF_HIP_TRY(hipMemsetAsync(b->d_ccount.p, 0, 4 * (size_t)b->K, s));
  }
  std::swap(b->cons.p, ncons.p); std::swap(b->cons.cap, ncons.cap);
  std::swap(b->d_coff.p, ncoff.p); std::swap(b->d_coff.cap, ncoff.cap);
  MGF_TRY(b->rows.ensure(std::max<size_t>(coff[b->K], 1), s));
  MGF_TRY(b->cont.ensure(4 * std::max<size_t>(coff[b->K], 1), s));
  if (b->parts) MGF_TRY(b->pool.ensure(3 * std::max<size_t>(coff[b->K], 1), s));
  MGF_TRY(b->cand.ensure(std::max<size_t>(qoff[b->K], 1), s));
  MGF_TRY(b->ncq.ensure(std::max<size_t>(qoff[b->K], 1), s)); MGF_TRY(b->slot.ensure(6 * std::max<size_t>(qoff[b->K], 1), s));
  MGF_TRY(b->d_qoff.ensure(b->K + 1, s)); MGF_TRY(b->d_qcap.ensure(std::max<size_t>(b->K, 1), s)); MGF_TRY(b->d_qcount.ensure(std::max<size_t>(b->K, 1), s));
  MGF_TRY(h2d(ctx, b->d_qoff.p, qoff.data(), qoff.size()));
  MGF_TRY(h2d(ctx, b->d_qcap.p, qcap.data(), qcap.size()));
  MGF_TRY(b->d_cap.ensure(std::max<size_t>(b->K, 1), s));
  MGF_TRY(h2d(ctx, b->d_cap.p, cap.data(), cap.size()));
  b->h_coff = coff; b->h_cap = cap;
  b->lists_valid = true;
  return MGF_OK;
}
// the mirror onto the device
static mgf_status batch_push(mgf_batch* b) {
  if (b->dev_valid) return MGF_OK;
  mgf_ctx* ctx = b->ctx;
  hipStream_t s = ctx->stream;
  batch_offsets(b);
  const size_t n = b->total();
  for (int a = 0; a < b->n_arr(); ++a) {
    MGF_TRY(b->dm[a].ensure(std::max<size_t>(n * mgf_batch::kWords[a], 1), s));
    MGF_TRY(h2d(ctx, b->dm[a].p, b->hm[a].data(), n * mgf_batch::kWords[a]));
  }
  MGF_TRY(b->bpk.ensure(std::max<size_t>(4 * n, 1), s));
  MGF_TRY(b->undo.ensure(std::max<size_t>(7 * n, 1), s));
  MGF_TRY(b->d_off.ensure(b->K + 1, s));
  MGF_TRY(h2d(ctx, b->d_off.p, b->h_off.data(), b->h_off.size()));
  MGF_TRY(b->d_na.ensure(std::max<size_t>(n, 1), s)); MGF_TRY(b->d_degb.ensure(std::max<size_t>(n, 1), s));
  MGF_TRY(b->d_done.ensure(b->K, s)); MGF_TRY(b->d_stage.ensure(b->K, s)); MGF_TRY(b->d_need.ensure(2 * (size_t)b->K, s)); MGF_TRY(b->d_err.ensure(4, s));
  MGF_HIP_TRY(hipMemsetAsync(b->d_err.p, 0, 16, s));
  b->lists_valid = false;  // (the lists named the bodies of another layout)
  MGF_TRY(batch_allot(b, false));
  b->dev_valid = true;
  return MGF_OK;
}

static mgf_status batch_bind(mgf_batch* b) {
  if (!b) return fail(MGF_ERR_INVALID, "batch is NULL");
  return ctx_bind(b->ctx);
}

extern "C" mgf_status mgf_batch_new(mgf_ctx* ctx, const mgf_params* params, int64_t n_worlds, mgf_batch** out) {
  if (!out) return fail(MGF_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (n_worlds <= 0 || n_worlds > (1 << 20)) return fail(MGF_ERR_INVALID, "n_worlds must be in 1 .. 2^20");
  MGF_TRY(ctx_bind(ctx));
  std::unique_ptr<mgf_batch> b(new mgf_batch());
  b->ctx = ctx;
  b->params = params ? *params : mgf_default_params();
  b->K = (uint32_t)n_worlds;
  b->h_wt.assign(b->K, -1); b->h_wx.assign(b->K, mk3(0, 0, 0));
  b->h_wo.assign(b->K, {}); b->h_orange.assign(b->K, 0u);
  b->h_n.assign(b->K, 0u); b->h_floor.assign(b->K, 0u); b->h_qfloor.assign(b->K, 0u); b->h_ccount.assign(b->K, 0u);
  batch_offsets(b.get());
  ctx_retain(ctx);
  *out = b.release();
  return MGF_OK;
}
extern "C" void mgf_batch_free(mgf_batch* b) {
  if (!b) return;
  mgf_ctx* ctx = b->ctx;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  delete b;
  ctx_release(ctx);
}
extern "C" int64_t mgf_batch_len(const mgf_batch* b, int64_t world) {
  if (!b || world < -1 || world >= (int64_t)b->K) return -1;
  if (world < 0) { int64_t t = 0; for (uint32_t n : b->h_n) t += n; return t; }
  return b->h_n[(size_t)world];
}
extern "C" mgf_status mgf_batch_set_option(mgf_batch* b, const char* key, int64_t value) {
  if (!b || !key) return fail(MGF_ERR_INVALID, "NULL argument");
  if (!strcmp(key, "cons_per_body")) {
    if (value < 1 || value > 4096) return fail(MGF_ERR_INVALID, "cons_per_body must be in 1 .. 4096");
    MGF_TRY(ctx_bind(b->ctx));
    b->cons_per_body = value;
    std::fill(b->h_floor.begin(), b->h_floor.end(), 0u);
    std::fill(b->h_qfloor.begin(), b->h_qfloor.end(), 0u);
    if (b->dev_valid) { b->lists_valid = false; MGF_TRY(batch_allot(b, false)); }
    return MGF_OK;
  }
  if (!strcmp(key, "part_queries")) {  // (no device work: the next query call launches the other kernels)
    if (value != 0 && value != 1) return fail(MGF_ERR_INVALID, "part_queries must be 0 or 1");
    b->part_queries = value == 1;
    return MGF_OK;
  }
  return fail(MGF_ERR_INVALID, "unknown batch option");
}
// a joint rig's skip counter (on the device: the stream is waited for)
template <class Rec>
static mgf_status batch_joint_skipped(const mgf_batch* b, const BatchJointRig<Rec>& R, int64_t* out) {
  unsigned long long v = 0;
  if (R.skipped.p) { MGF_TRY(ctx_bind(b->ctx)); MGF_TRY(d2h(b->ctx, &v, R.skipped.p, 1)); }
  *out = (int64_t)v;
  return MGF_OK;
}
extern "C" mgf_status mgf_batch_counter(const mgf_batch* b, const char* name, int64_t* out) {
  if (!b || !name || !out) return fail(MGF_ERR_INVALID, "NULL argument");
  if (!strcmp(name, "launches_per_tick")) { *out = b->parts ? 7 : 6; return MGF_OK; }
  if (!strcmp(name, "capacity_retries")) { *out = b->capacity_retries; return MGF_OK; }
  if (!strcmp(name, "query_launches")) { *out = b->q_launches; return MGF_OK; }
  if (!strcmp(name, "query_run_ns")) { *out = (int64_t)((double)b->q_run_ms * 1e6); return MGF_OK; }
  if (!strcmp(name, "drive_launches")) { *out = b->d_launches; return MGF_OK; }
  if (!strcmp(name, "rollout_launches")) { *out = b->r_launches; return MGF_OK; }
  if (!strcmp(name, "pair_table_uploads")) { *out = b->w_uploads; return MGF_OK; }
  if (!strcmp(name, "device_skipped")) {  // (on the device: the stream is waited for)
    unsigned long long v = 0;
    if (b->v_skipped.p) { MGF_TRY(ctx_bind(b->ctx)); MGF_TRY(d2h(b->ctx, &v, b->v_skipped.p, 1)); }
    *out = (int64_t)v;
    return MGF_OK;
  }
  if (!strcmp(name, "actuators_skipped")) {  // (on the device: the stream is waited for)
    unsigned long long v = 0;
    if (b->a_skipped.p) { MGF_TRY(ctx_bind(b->ctx)); MGF_TRY(d2h(b->ctx, &v, b->a_skipped.p, 1)); }
    *out = (int64_t)v;
    return MGF_OK;
  }
  if (!strcmp(name, "springs_skipped")) {  // (on the device: the stream is waited for)
    unsigned long long v = 0;
    if (b->sp_skipped.p) { MGF_TRY(ctx_bind(b->ctx)); MGF_TRY(d2h(b->ctx, &v, b->sp_skipped.p, 1)); }
    *out = (int64_t)v;
    return MGF_OK;
  }
  if (!strcmp(name, "joints_skipped")) return batch_joint_skipped(b, b->joints, out);
  if (!strcmp(name, "hinges_skipped")) return batch_joint_skipped(b, b->hinges, out);
  if (!strcmp(name, "sliders_skipped")) return batch_joint_skipped(b, b->sliders, out);
  return fail(MGF_ERR_INVALID, "unknown batch counter");
}

// The mesh BVH in the order a query visits it, every node with the index of the first node behind its subtree (BatchTerrain, k_batch.h).
static void batch_thread_tree(const HostBvh& t, uint64_t id, std::vector<float4>* out) {
  const HostBvh::Node& n = t.node(id);
  const size_t at = out->size() / 2;
  out->push_back(make_float4(n.box.c.x, n.box.c.y, n.box.c.z, 0.0f));
  out->push_back(make_float4(n.box.r.x, n.box.r.y, n.box.r.z, 0.0f));
  uint32_t w0 = 0u;
  if (n.leaf) w0 = 0x80000000u | (uint32_t)(n.value & 0x7fffffffu);
  else { batch_thread_tree(t, n.kid[1], out); batch_thread_tree(t, n.kid[0], out); }  // (bvh.rs:283-310: the right child is popped first)
  const uint32_t skip = (uint32_t)(out->size() / 2);
  memcpy(&(*out)[2 * at].w, &w0, 4);
  memcpy(&(*out)[2 * at + 1].w, &skip, 4);
}
// a copy of the mesh behind the table's last entry
static mgf_status batch_table_add(mgf_batch* b, const mgf_mesh* mesh) {
  std::vector<float4> nodes;
  if (!mesh->m.tree.empty()) batch_thread_tree(mesh->m.tree, mesh->m.tree.root(), &nodes);
  std::vector<float4> hv(mesh->verts.size());
  for (size_t i = 0; i < hv.size(); ++i) hv[i] = make_float4(mesh->verts[i].x, mesh->verts[i].y, mesh->verts[i].z, 0.0f);
  std::vector<uint4> hf(mesh->faces.size() / 3);
  for (size_t i = 0; i < hf.size(); ++i) hf[i] = make_uint4(mesh->faces[3 * i], mesh->faces[3 * i + 1], mesh->faces[3 * i + 2], 0);
  if (b->t_n_nodes + nodes.size() / 2 > 0x7FFFFFF0ull || b->t_n_verts + hv.size() > 0x7FFFFFF0ull || b->t_n_faces + hf.size() > 0x7FFFFFF0ull)
    return fail(MGF_ERR_OOM, "the batch's terrain table exceeds 2^31 nodes, vertices or faces");
  MGF_TRY(append(b->ctx, b->t_nodes, 2 * b->t_n_nodes, nodes));
  MGF_TRY(append(b->ctx, b->t_verts, b->t_n_verts, hv));
  MGF_TRY(append(b->ctx, b->t_faces, b->t_n_faces, hf));
  mgf_batch::TerrainEntry e;
  e.node0 = (uint32_t)b->t_n_nodes; e.n_nodes = (uint32_t)(nodes.size() / 2); e.vert0 = (uint32_t)b->t_n_verts; e.face0 = (uint32_t)b->t_n_faces;
  e.x = mesh->x;
  b->t_table.push_back(e);
  b->t_n_nodes += nodes.size() / 2; b->t_n_verts += hv.size(); b->t_n_faces += hf.size();
  return MGF_OK;
}
// every world's descriptor onto the device, before the first launch behind a change of the table or of an assignment
static mgf_status batch_terrain_sync(mgf_batch* b) {
  if (!b->t_desc_stale) return MGF_OK;
  hipStream_t s = b->ctx->stream;
  std::vector<uint4> d(2 * (size_t)b->K + 2, make_uint4(0u, 0u, 0u, 0u));
  uint32_t with = 0;
  for (uint32_t k = 0; k < b->K; ++k) {
    d[2 * (size_t)k + 1].w = b->h_orange[k];  // the world's obstacles (batch_obstacle_sync)
    if (b->h_wt[k] < 0) continue;
    const mgf_batch::TerrainEntry& e = b->t_table[(size_t)b->h_wt[k]];
    const V3 x = b->h_wx[k];
    uint32_t xb[3];
    memcpy(&xb[0], &x.x, 4); memcpy(&xb[1], &x.y, 4); memcpy(&xb[2], &x.z, 4);
    d[2 * (size_t)k] = make_uint4(e.node0, e.vert0, e.face0, e.n_nodes);
    d[2 * (size_t)k + 1] = make_uint4(xb[0], xb[1], xb[2], b->h_orange[k]);
    if (e.n_nodes) ++with;
  }
  {  // behind the worlds' descriptors: where the obstacle stores are (batch_obstacles_of, k_batch.h)
    const uint64_t pn = reinterpret_cast<uint64_t>(b->o_nodes.p), pc = reinterpret_cast<uint64_t>(b->o_comps.p), pd = reinterpret_cast<uint64_t>(b->o_desc.p);
    d[2 * (size_t)b->K] = make_uint4((uint32_t)pn, (uint32_t)(pn >> 32), (uint32_t)pc, (uint32_t)(pc >> 32));
    d[2 * (size_t)b->K + 1] = make_uint4((uint32_t)pd, (uint32_t)(pd >> 32), 0u, 0u);
  }
  MGF_TRY(b->t_desc.ensure(d.size(), s));
  MGF_TRY(b->t_nodes.ensure(1, s)); MGF_TRY(b->t_verts.ensure(1, s)); MGF_TRY(b->t_faces.ensure(1, s));
  MGF_TRY(h2d(b->ctx, b->t_desc.p, d.data(), d.size()));
  b->t_worlds = with;
  b->t_desc_stale = false;
  return MGF_OK;
}
static BatchTerrains batch_terrains(const mgf_batch* b) {
  BatchTerrains T;
  T.nodes = b->t_nodes.p; T.verts = b->t_verts.p; T.faces = b->t_faces.p; T.desc = b->t_desc.p;
  return T;
}
// The table emptied, `mesh` its entry 0 and every world's terrain, at the mesh's position; NULL: an empty table, no world has terrain.
extern "C" mgf_status mgf_batch_set_terrain(mgf_batch* b, const mgf_mesh* mesh) {
  MGF_TRY(batch_bind(b));
  b->t_table.clear();
  b->t_n_nodes = b->t_n_verts = b->t_n_faces = 0;
  std::fill(b->h_wt.begin(), b->h_wt.end(), -1);
  b->t_desc_stale = true;
  if (!mesh) return MGF_OK;
  MGF_TRY(batch_table_add(b, mesh));
  std::fill(b->h_wt.begin(), b->h_wt.end(), 0);
  std::fill(b->h_wx.begin(), b->h_wx.end(), mesh->x);
  return MGF_OK;
}
extern "C" mgf_status mgf_batch_add_terrain(mgf_batch* b, const mgf_mesh* mesh, int32_t* id) {
  if (!b) return fail(MGF_ERR_INVALID, "batch is NULL");
  if (!mesh || !id) return fail(MGF_ERR_INVALID, "NULL argument");
  MGF_TRY(ctx_bind(b->ctx));
  if (b->t_table.size() >= 0x7FFFFFFFull) return fail(MGF_ERR_OOM, "the batch's terrain table is full");
  MGF_TRY(batch_table_add(b, mesh));
  *id = (int32_t)(b->t_table.size() - 1);
  return MGF_OK;
}
extern "C" mgf_status mgf_batch_set_world_terrain(mgf_batch* b, const int32_t* world, const int32_t* terrain, const mgf_vec3* pos, int64_t n) {
  if (!b) return fail(MGF_ERR_INVALID, "batch is NULL");
  if (n < 0) return fail(MGF_ERR_INVALID, "n is negative");
  if (n && (!world || !terrain)) return fail(MGF_ERR_INVALID, "NULL argument");
  for (int64_t i = 0; i < n; ++i) {
    if (world[i] < 0) return fail(MGF_ERR_INVALID, "world index out of range");
    if (terrain[i] < -1) return fail(MGF_ERR_INVALID, "terrain id out of range");
  }
  MGF_TRY(ctx_bind(b->ctx));
  for (int64_t i = 0; i < n; ++i) {
    if ((uint32_t)world[i] >= b->K) return fail(MGF_ERR_INVALID, "world index out of range");
    if (terrain[i] >= 0 && (size_t)terrain[i] >= b->t_table.size()) return fail(MGF_ERR_INVALID, "terrain id out of range");
  }
  for (int64_t i = 0; i < n; ++i) {
    const size_t k = (size_t)world[i];
    b->h_wt[k] = terrain[i];
    if (terrain[i] < 0) b->h_wx[k] = mk3(0, 0, 0);
    else b->h_wx[k] = pos ? mk3(pos[i].x, pos[i].y, pos[i].z) : b->t_table[(size_t)terrain[i]].x;
  }
  if (n) b->t_desc_stale = true;
  return MGF_OK;
}
extern "C" int64_t mgf_batch_terrain_count(const mgf_batch* b) { return b ? (int64_t)b->t_table.size() : -1; }

static BatchObstacles batch_obstacles(const mgf_batch* b) {
  BatchObstacles O;
  O.nodes = b->o_nodes.p; O.comps = b->o_comps.p; O.desc = b->o_desc.p;
  return O;
}
// every list entry's descriptor onto the device, before the first launch behind a change of a list (batch_terrain_sync's counterpart).
// Every index a kernel takes from a descriptor is in range here: an entry's nodes and components lie within the stores, a skip index
// and a leaf's component within the entry (batch_thread_tree over the compound's own tree).
static mgf_status batch_obstacle_sync(mgf_batch* b) {
  if (!b->o_desc_stale) return MGF_OK;
  hipStream_t s = b->ctx->stream;
  std::vector<uint4> d;
  uint32_t with = 0;
  size_t total = 0;
  for (uint32_t k = 0; k < b->K; ++k) total += b->h_wo[k].size();
  if (total >= (1ull << (32 - kBatchObstCountBits))) return fail(MGF_ERR_OOM, "the batch's obstacle lists exceed 2^25 entries");
  for (uint32_t k = 0; k < b->K; ++k) {
    for (const mgf_batch::ObstacleRef& r : b->h_wo[k]) {
      const mgf_batch::ObstacleEntry& e = b->o_table[r.entry];
      uint32_t w[7];
      const float f[7] = {r.disp.x, r.disp.y, r.disp.z, r.rot.s, r.rot.v.x, r.rot.v.y, r.rot.v.z};
      memcpy(w, f, sizeof(w));
      d.push_back(make_uint4(e.node0, e.n_nodes, e.comp0, 0u));
      d.push_back(make_uint4(w[0], w[1], w[2], w[3]));
      d.push_back(make_uint4(w[4], w[5], w[6], 0u));
    }
    const uint32_t cnt = (uint32_t)b->h_wo[k].size();
    b->h_orange[k] = cnt ? ((uint32_t)(d.size() / 3 - cnt) << kBatchObstCountBits) | cnt : 0u;
    if (cnt) ++with;
  }
  MGF_TRY(b->o_desc.ensure(std::max<size_t>(d.size(), 1), s));
  MGF_TRY(b->o_nodes.ensure(1, s)); MGF_TRY(b->o_comps.ensure(1, s));
  MGF_TRY(h2d(b->ctx, b->o_desc.p, d.data(), d.size()));
  b->o_worlds = with;
  b->o_desc_stale = false;
  b->t_desc_stale = true;  // (the worlds' ranges and the stores' addresses travel with the terrain descriptors)
  return MGF_OK;
}
// a world's environment - its obstacle list, then its terrain descriptor, which names the list - before the first launch behind a change
static mgf_status batch_env_sync(mgf_batch* b) {
  MGF_TRY(batch_obstacle_sync(b));
  return batch_terrain_sync(b);
}
// A copy of the compound - components, tree and current pose - behind the obstacle table's last entry; no world changes.  An empty
// compound is an entry that meets nothing and keeps its place in a world's list.
extern "C" mgf_status mgf_batch_add_obstacle(mgf_batch* b, const mgf_compound* c, int32_t* id) {
  if (!b) return fail(MGF_ERR_INVALID, "batch is NULL");
  if (!c || !id) return fail(MGF_ERR_INVALID, "NULL argument");
  if (c->comps.size() >= kObstacleCompMax) return fail(MGF_ERR_CAPACITY, "an obstacle holds at most 2^18 components");
  MGF_TRY(ctx_bind(b->ctx));
  if (b->o_table.size() >= 0x7FFFFFFFull) return fail(MGF_ERR_OOM, "the batch's obstacle table is full");
  std::vector<float4> nodes;
  if (!c->m.tree.empty()) batch_thread_tree(c->m.tree, c->m.tree.root(), &nodes);
  std::vector<CompIn> hc(c->comps.size());
  static_assert(sizeof(CompIn) == sizeof(mgf_component), "a compound's components go up as they are");
  if (!hc.empty()) memcpy(hc.data(), c->comps.data(), hc.size() * sizeof(CompIn));
  if (b->o_n_nodes + nodes.size() / 2 > 0x7FFFFFF0ull || b->o_n_comps + hc.size() > 0x7FFFFFF0ull)
    return fail(MGF_ERR_OOM, "the batch's obstacle table exceeds 2^31 nodes or components");
  MGF_TRY(append(b->ctx, b->o_nodes, 2 * b->o_n_nodes, nodes));
  MGF_TRY(append(b->ctx, b->o_comps, b->o_n_comps, hc));
  mgf_batch::ObstacleEntry e;
  e.node0 = (uint32_t)b->o_n_nodes; e.n_nodes = (uint32_t)(nodes.size() / 2); e.comp0 = (uint32_t)b->o_n_comps;
  e.disp = c->disp; e.rot = c->rot;
  b->o_table.push_back(e);
  b->o_n_nodes += nodes.size() / 2; b->o_n_comps += hc.size();
  b->o_desc_stale = true;  // (a store that grew may have moved)
  *id = (int32_t)(b->o_table.size() - 1);
  return MGF_OK;
}
// Every world some record names gets its list replaced by its records, in array order (-1: a record that contributes nothing).
extern "C" mgf_status mgf_batch_set_world_obstacles(mgf_batch* b, const int32_t* world, const int32_t* obstacle, const mgf_vec3* disp, const mgf_quat* rot,
                                                    int64_t n) {
  if (!b) return fail(MGF_ERR_INVALID, "batch is NULL");
  if (n < 0) return fail(MGF_ERR_INVALID, "n is negative");
  if (n && (!world || !obstacle)) return fail(MGF_ERR_INVALID, "NULL argument");
  for (int64_t i = 0; i < n; ++i) {
    if (world[i] < 0) return fail(MGF_ERR_INVALID, "world index out of range");
    if (obstacle[i] < -1) return fail(MGF_ERR_INVALID, "obstacle id out of range");
  }
  MGF_TRY(ctx_bind(b->ctx));
  std::vector<uint32_t> cnt(b->K, 0u);
  for (int64_t i = 0; i < n; ++i) {
    if ((uint32_t)world[i] >= b->K) return fail(MGF_ERR_INVALID, "world index out of range");
    if (obstacle[i] < 0) continue;
    if ((size_t)obstacle[i] >= b->o_table.size()) return fail(MGF_ERR_INVALID, "obstacle id out of range");
    if (++cnt[(size_t)world[i]] > MGF_BATCH_MAX_WORLD_OBSTACLES)
      return fail(MGF_ERR_INVALID, "a world of a batch has at most MGF_BATCH_MAX_WORLD_OBSTACLES (64) obstacles: nothing was changed");
  }
  for (int64_t i = 0; i < n; ++i) b->h_wo[(size_t)world[i]].clear();
  for (int64_t i = 0; i < n; ++i) {
    if (obstacle[i] < 0) continue;
    const mgf_batch::ObstacleEntry& e = b->o_table[(size_t)obstacle[i]];
    mgf_batch::ObstacleRef r;
    r.entry = (uint32_t)obstacle[i];
    r.disp = disp ? mk3(disp[i].x, disp[i].y, disp[i].z) : e.disp;
    r.rot = rot ? mkq(rot[i].s, mk3(rot[i].x, rot[i].y, rot[i].z)) : e.rot;
    b->h_wo[(size_t)world[i]].push_back(r);
  }
  if (n) b->o_desc_stale = true;
  return MGF_OK;
}
extern "C" int64_t mgf_batch_obstacle_count(const mgf_batch* b) { return b ? (int64_t)b->o_table.size() : -1; }
extern "C" int64_t mgf_batch_world_obstacle_count(const mgf_batch* b, int64_t world) {
  if (!b || world < 0 || world >= (int64_t)b->K) return -1;
  return (int64_t)b->h_wo[(size_t)world].size();
}

// RigidBodyVec::add_body physics.rs:200-218 + World::add_body world.rs:178-184 (initial fat AABB), as mgf_world_add_bodies, for one world of the batch.
// The rigs name (world, body): behind a change of the batch's layout they are checked against the new lengths when they go up again
static void batch_rigs_stale(mgf_batch* b) {
  b->sensors.stale = true;
  b->cameras.stale = true;
  b->zones.stale = true;
  b->touches.stale = true;
  b->feelers.stale = true;
  b->actuators.stale = true;
  b->springs.stale = true;
  b->joints.stale = true;
  b->hinges.stale = true;
  b->sliders.stale = true;
}

// the rows of `n` new bodies (empty part slots where the caller has filled none) behind world k's last body
static mgf_status batch_insert(mgf_batch* b, uint32_t k, const std::vector<float4>* add, size_t n) {
  const size_t at = b->h_off[k + 1];
  for (int a = 0; a < b->n_arr(); ++a) b->hm[a].insert(b->hm[a].begin() + at * mgf_batch::kWords[a], add[a].begin(), add[a].end());
  b->h_n[k] += (uint32_t)n;
  batch_offsets(b);
  std::fill(b->h_ccount.begin(), b->h_ccount.end(), 0u);
  b->ccount_stale = false;
  return MGF_OK;
}
// The rows of one ordinary body (RigidBodyVec::add_body physics.rs:200-218, World::add_body world.rs:178-184) into slot i of `add`.
static mgf_status batch_body_rows(const mgf_batch* b, const mgf_component& mc, float mass, float restitution, float friction, const mgf_vec3& world_force,
                                  std::vector<float4>* add, size_t i) {
  Comp c = comp_of(mc);
  if (c.kind == KIND_SPHERE) c.d = mk3(0, 0, 0);
  // Component::deconstruct compound.rs:42-52
  V3 px; Quat pq; float half_h = 0.0f;
  if (c.kind == KIND_SPHERE) { px = c.p; pq = mkq(1.0f, mk3(0, 0, 0)); }
  else {
    const float h = mag(c.d);
    pq = quat_from_arc(mk3(0.0f, 1.0f, 0.0f) * h, c.d);
    px = c.p + c.d * 0.5f;
    half_h = h * 0.5f;
  }
  Comp local = c; local.p = c.p + -px;  // collider - x.to_vec()
  M3 inv;
  if (!invert(tensor_of(local, mass), &inv)) return fail(MGF_ERR_SINGULAR, "inertia tensor is not invertible (physics.rs:212)");
  const float inv_mass = 1.0f / mass;
  const V3 force = mk3(world_force.x, world_force.y, world_force.z) * mass;
  add[mgf_batch::AX][i] = make_float4(px.x, px.y, px.z, 0.0f);
  add[mgf_batch::AQ][i] = make_float4(pq.s, pq.v.x, pq.v.y, pq.v.z);
  float4* sr = &add[mgf_batch::ASREC][4 * i];
  sr[0] = make_float4(0, 0, 0, 0);
  sr[1] = make_float4(0, 0, inv_mass, inv.c[0].x);
  sr[2] = make_float4(inv.c[0].y, inv.c[0].z, inv.c[1].x, inv.c[1].y);
  sr[3] = make_float4(inv.c[1].z, inv.c[2].x, inv.c[2].y, inv.c[2].z);
  add[mgf_batch::ASP0][i] = make_float4(force.x, force.y, force.z, restitution);
  add[mgf_batch::ASP1][i] = make_float4(0, 0, 0, friction);
  const uint32_t kind_bits = (uint32_t)c.kind;
  float kf; memcpy(&kf, &kind_bits, 4);
  add[mgf_batch::ACTOR][i] = make_float4(kf, c.r, half_h, 0.0f);
  for (int col = 0; col < 3; ++col) add[mgf_batch::AIMB][3 * i + col] = make_float4(inv.c[col].x, inv.c[col].y, inv.c[col].z, 0.0f);
  add[mgf_batch::ADELTA][i] = make_float4(0, 0, 0, friction);
  const Box tb = swept_bounds(c, mk3(0, 0, 0));
  const V3 fr = tb.r + mk3(b->params.fat_margin, b->params.fat_margin, b->params.fat_margin);
  add[mgf_batch::AFBC][i] = make_float4(tb.c.x, tb.c.y, tb.c.z, 0.0f);
  add[mgf_batch::AFBR][i] = make_float4(fr.x, fr.y, fr.z, 0.0f);
  add[mgf_batch::ACOL0][i] = make_float4(c.p.x, c.p.y, c.p.z, c.r);  // (what a query sees until a tick has run on the body)
  add[mgf_batch::ACOL1][i] = make_float4(c.d.x, c.d.y, c.d.z, kf);
  return MGF_OK;
}

extern "C" mgf_status mgf_batch_add_bodies(mgf_batch* b, int64_t world, const mgf_component* comps, int64_t n, const float* mass, const float* restitution,
                                           const float* friction, const mgf_vec3* world_force, uint64_t* first_id) {
  if (!b) return fail(MGF_ERR_INVALID, "batch is NULL");
  if (n < 0) return fail(MGF_ERR_INVALID, "n is negative");
  if (n && (!comps || !mass || !restitution || !friction || !world_force)) return fail(MGF_ERR_INVALID, "NULL argument");
  if (world < 0) return fail(MGF_ERR_INVALID, "world index out of range");
  if (n > MGF_BATCH_MAX_BODIES) return fail(MGF_ERR_INVALID, "a world of a batch holds at most MGF_BATCH_MAX_BODIES (1024) bodies");
  for (int64_t i = 0; i < n; ++i) {
    if (comps[i].tag != MGF_SPHERE && comps[i].tag != MGF_CAPSULE) return fail(MGF_ERR_INVALID, "component tag must be sphere (0) or capsule (1)");
    if (!(comps[i].r > 0.0f)) return fail(MGF_ERR_INVALID, "radius must be > 0 (geom.rs:300,328)");
  }
  MGF_TRY(ctx_bind(b->ctx));
  if (world >= (int64_t)b->K) return fail(MGF_ERR_INVALID, "world index out of range");
  const uint32_t k = (uint32_t)world;
  if ((int64_t)b->h_n[k] + n > MGF_BATCH_MAX_BODIES) return fail(MGF_ERR_INVALID, "a world of a batch holds at most MGF_BATCH_MAX_BODIES (1024) bodies: nothing was added");
  if (first_id) *first_id = b->h_n[k];
  if (n == 0) return MGF_OK;
  const size_t N = (size_t)n;
  std::vector<float4> add[mgf_batch::kArr];
  for (int a = 0; a < mgf_batch::kArr; ++a) add[a].resize(N * mgf_batch::kWords[a]);
  for (size_t i = 0; i < N; ++i) MGF_TRY(batch_body_rows(b, comps[i], mass[i], restitution[i], friction[i], world_force[i], add, i));
  MGF_TRY(batch_pull(b));
  MGF_TRY(batch_insert(b, k, add, N));
  batch_rigs_stale(b);
  return MGF_OK;
}

// The batch gets part rows - empty slots for the bodies it holds, all of them ordinary - where its state is: in the mirror, or on the
// device behind whatever the stream still runs.  From here on its tick is k_batch_parts.h's.
static mgf_status batch_parts_enable(mgf_batch* b) {
  if (b->parts) return MGF_OK;
  hipStream_t s = b->ctx->stream;
  const size_t words = (size_t)kMaxParts * b->total();
  for (int a = mgf_batch::kArrPlain; a < mgf_batch::kArr; ++a) {
    if (b->dev_valid) {
      MGF_TRY(b->dm[a].ensure(std::max<size_t>(words, 1), s));
      MGF_HIP_TRY(hipMemsetAsync(b->dm[a].p, 0, 16 * words, s));
    } else {
      b->hm[a].assign(words, make_float4(0, 0, 0, 0));
    }
  }
  if (b->dev_valid) MGF_TRY(b->pool.ensure(3 * std::max<size_t>(b->h_coff.empty() ? 0 : b->h_coff[b->K], 1), s));
  b->parts = true;
  return MGF_OK;
}
// the calls that read the shapes of bodies do not see parts unless asked to: refused on a batch that holds a body of several components,
// except - for the calls that have a part-aware body pass (part_aware: all but the cameras') - under option "part_queries"
static mgf_status batch_single_parts(const mgf_batch* b, const char* call, bool part_aware = true) {
  if (!b->parts || (part_aware && b->part_queries)) return MGF_OK;
  return fail(MGF_ERR_INVALID, (std::string(call) + ": the batch holds bodies of several components, which this call does not see yet").c_str());
}

// Bodies of 1..4 components for one world of the batch, as mgf_world_add_compound_bodies (the oracle's RigidBodyVec::add_compound_body:
// mass = sum, x = centre of mass, q = identity, tensor = sum of the components' tensors about the centre of mass, parts fixed in the
// body frame).  A body of one component is the ordinary body mgf_batch_add_bodies adds, with the component's mass.
extern "C" mgf_status mgf_batch_add_compound_bodies(mgf_batch* b, int64_t world, const mgf_component* comps, const float* comp_mass, const int64_t* offsets, int64_t n,
                                                    const float* restitution, const float* friction, const mgf_vec3* world_force, uint64_t* first_id) {
  if (!b) return fail(MGF_ERR_INVALID, "batch is NULL");
  if (!comps || !offsets || !first_id) return fail(MGF_ERR_INVALID, "NULL argument");
  if (n < 0) return fail(MGF_ERR_INVALID, "n is negative");
  if (n && (!comp_mass || !restitution || !friction || !world_force)) return fail(MGF_ERR_INVALID, "NULL argument");
  if (world < 0) return fail(MGF_ERR_INVALID, "world index out of range");
  if (n > MGF_BATCH_MAX_BODIES) return fail(MGF_ERR_INVALID, "a world of a batch holds at most MGF_BATCH_MAX_BODIES (1024) bodies");
  if (offsets[0] != 0) return fail(MGF_ERR_INVALID, "offsets[0] must be 0");
  bool several = false;
  for (int64_t r = 0; r < n; ++r) {
    const int64_t cnt = offsets[r + 1] - offsets[r];
    if (cnt < 1 || cnt > kMaxParts)
      return fail(MGF_ERR_INVALID, "a body of a batch needs 1..4 components (the batch takes four, the lone world 32): nothing was added");
    several = several || cnt > 1;
  }
  for (int64_t c = 0; c < offsets[n]; ++c) {
    if (comps[c].tag != MGF_SPHERE && comps[c].tag != MGF_CAPSULE) return fail(MGF_ERR_INVALID, "component tag must be sphere (0) or capsule (1)");
    if (!(comps[c].r > 0.0f)) return fail(MGF_ERR_INVALID, "radius must be > 0 (geom.rs:300,328)");
  }
  MGF_TRY(ctx_bind(b->ctx));
  if (world >= (int64_t)b->K) return fail(MGF_ERR_INVALID, "world index out of range");
  const uint32_t k = (uint32_t)world;
  if ((int64_t)b->h_n[k] + n > MGF_BATCH_MAX_BODIES) return fail(MGF_ERR_INVALID, "a world of a batch holds at most MGF_BATCH_MAX_BODIES (1024) bodies: nothing was added");
  *first_id = b->h_n[k];
  if (n == 0) return MGF_OK;
  const size_t N = (size_t)n;
  std::vector<float4> add[mgf_batch::kArr];
  for (int a = 0; a < mgf_batch::kArr; ++a) add[a].resize(N * mgf_batch::kWords[a]);
  const V3 fm = mk3(b->params.fat_margin, b->params.fat_margin, b->params.fat_margin);
  for (size_t r = 0; r < N; ++r) {
    const int64_t k0 = offsets[r], k1 = offsets[r + 1];
    if (k1 - k0 == 1) {
      MGF_TRY(batch_body_rows(b, comps[k0], comp_mass[k0], restitution[r], friction[r], world_force[r], add, r));
      continue;
    }
    Comp part[kMaxParts];  // (mgf_world_add_compound_bodies, operation for operation)
    float total = 0.0f;
    V3 acc = mk3(0, 0, 0);
    for (int64_t c = k0; c < k1; ++c) {
      Comp p = comp_of(comps[c]);
      if (p.kind == KIND_SPHERE) p.d = mk3(0, 0, 0);
      part[c - k0] = p;
      total += comp_mass[c];
      acc = acc + comp_center(p) * comp_mass[c];
    }
    const V3 com = acc / total;
    M3 t = m3_cols(mk3(0, 0, 0), mk3(0, 0, 0), mk3(0, 0, 0));
    for (int64_t c = k0; c < k1; ++c) { Comp l = part[c - k0]; l.p = l.p + -com; t = t + tensor_of(l, comp_mass[c]); }
    M3 inv;
    if (!invert(t, &inv)) return fail(MGF_ERR_SINGULAR, "inertia tensor is not invertible");
    const float inv_mass = 1.0f / total;
    const V3 force = mk3(world_force[r].x, world_force[r].y, world_force[r].z) * total;
    add[mgf_batch::AX][r] = make_float4(com.x, com.y, com.z, 0.0f);
    add[mgf_batch::AQ][r] = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
    float4* sr = &add[mgf_batch::ASREC][4 * r];
    sr[0] = make_float4(0, 0, 0, 0);
    sr[1] = make_float4(0, 0, inv_mass, inv.c[0].x);
    sr[2] = make_float4(inv.c[0].y, inv.c[0].z, inv.c[1].x, inv.c[1].y);
    sr[3] = make_float4(inv.c[1].z, inv.c[2].x, inv.c[2].y, inv.c[2].z);
    add[mgf_batch::ASP0][r] = make_float4(force.x, force.y, force.z, restitution[r]);
    add[mgf_batch::ASP1][r] = make_float4(0, 0, 0, friction[r]);
    const uint32_t kind_bits = 2u, cnt_bits = (uint32_t)(k1 - k0);  // constructor kind: a body of several parts, and how many (batch_np, k_batch_parts.h)
    float kf, cf; memcpy(&kf, &kind_bits, 4); memcpy(&cf, &cnt_bits, 4);
    add[mgf_batch::ACTOR][r] = make_float4(kf, cf, 0.0f, 0.0f);
    for (int col = 0; col < 3; ++col) add[mgf_batch::AIMB][3 * r + col] = make_float4(inv.c[col].x, inv.c[col].y, inv.c[col].z, 0.0f);
    add[mgf_batch::ADELTA][r] = make_float4(0, 0, 0, friction[r]);
    const uint32_t sph = (uint32_t)KIND_SPHERE; float sf; memcpy(&sf, &sph, 4);
    add[mgf_batch::ACOL0][r] = make_float4(com.x, com.y, com.z, 0.0f);  // the carrier: a radius-0 sphere at the centre of mass
    add[mgf_batch::ACOL1][r] = make_float4(0, 0, 0, sf);
    Box tb;
    for (int64_t c = k0; c < k1; ++c) {
      const Comp& p = part[c - k0];
      const uint32_t kb = (uint32_t)p.kind; float kbf; memcpy(&kbf, &kb, 4);
      const V3 lp = p.p + -com;
      const size_t at = (size_t)kMaxParts * r + (size_t)(c - k0);
      add[mgf_batch::ALP0][at] = make_float4(lp.x, lp.y, lp.z, p.r);
      add[mgf_batch::ALP1][at] = make_float4(p.d.x, p.d.y, p.d.z, kbf);
      add[mgf_batch::AWP0][at] = make_float4(p.p.x, p.p.y, p.p.z, p.r);
      add[mgf_batch::AWP1][at] = make_float4(p.d.x, p.d.y, p.d.z, kbf);
      const Box pb = swept_bounds(p, mk3(0, 0, 0));
      tb = c == k0 ? pb : box_combine(tb, pb);
    }
    const V3 frr = tb.r + fm;
    add[mgf_batch::AFBC][r] = make_float4(tb.c.x, tb.c.y, tb.c.z, 0.0f);
    add[mgf_batch::AFBR][r] = make_float4(frr.x, frr.y, frr.z, 0.0f);
  }
  MGF_TRY(batch_pull(b));
  if (several) MGF_TRY(batch_parts_enable(b));
  MGF_TRY(batch_insert(b, k, add, N));
  batch_rigs_stale(b);
  return MGF_OK;
}

static mgf_status batch_range(mgf_batch* b, int64_t world, size_t* first, size_t* n) {
  if (world < -1 || world >= (int64_t)b->K) return fail(MGF_ERR_INVALID, "world index out of range");
  *first = world < 0 ? 0 : b->h_off[(size_t)world];
  *n = world < 0 ? b->total() : b->h_n[(size_t)world];
  return MGF_OK;
}
// As mgf_world_read_state / mgf_world_write_state for one world, or (world = -1) for all bodies of the batch, worlds concatenated in order.
extern "C" mgf_status mgf_batch_read_state(mgf_batch* b, int64_t world, mgf_vec3* x, mgf_quat* q, mgf_vec3* v, mgf_vec3* omega, mgf_vec3* delta, int64_t cap) {
  if (!b) return fail(MGF_ERR_INVALID, "batch is NULL");
  if (world < -1) return fail(MGF_ERR_INVALID, "world index out of range");
  MGF_TRY(ctx_bind(b->ctx));
  size_t first, n;
  MGF_TRY(batch_range(b, world, &first, &n));
  if ((int64_t)n > cap) return fail(MGF_ERR_CAPACITY, "state buffers too small");
  if (n == 0) return MGF_OK;
  MGF_TRY(batch_push(b));
  hipStream_t s = b->ctx->stream;
  const size_t fl[5] = {x ? 3 * n : 0, q ? 4 * n : 0, v ? 3 * n : 0, omega ? 3 * n : 0, delta ? 3 * n : 0};
  size_t off[6] = {0, 0, 0, 0, 0, 0};
  for (int k = 0; k < 5; ++k) off[k + 1] = off[k] + ((fl[k] + 3) & ~(size_t)3);  // (every section 16-byte aligned: q goes out as float4)
  if (off[5] == 0) return MGF_OK;
  MGF_TRY(b->pack.ensure(off[5], s));
  float* P = b->pack.p;
  k_pack_state<<<nblk(n), kBlock, 0, s>>>(b->bodies(first), (uint32_t)n, nullptr, x ? P + off[0] : nullptr, q ? P + off[1] : nullptr, v ? P + off[2] : nullptr,
                                          omega ? P + off[3] : nullptr, delta ? P + off[4] : nullptr);
  LAUNCH_CHECK();
  void* dst[5] = {x, q, v, omega, delta};
  for (int k = 0; k < 5; ++k)
    if (fl[k]) MGF_HIP_TRY(hipMemcpyAsync(dst[k], P + off[k], 4 * fl[k], hipMemcpyDeviceToHost, s));
  MGF_HIP_TRY(hipStreamSynchronize(s));
  return MGF_OK;
}
extern "C" mgf_status mgf_batch_write_state(mgf_batch* b, int64_t world, const mgf_vec3* x, const mgf_quat* q, const mgf_vec3* v, const mgf_vec3* omega,
                                            const mgf_vec3* delta, int64_t n_in) {
  if (!b) return fail(MGF_ERR_INVALID, "batch is NULL");
  if (world < -1) return fail(MGF_ERR_INVALID, "world index out of range");
  if (n_in < 0) return fail(MGF_ERR_INVALID, "n is negative");
  MGF_TRY(ctx_bind(b->ctx));
  size_t first, n;
  MGF_TRY(batch_range(b, world, &first, &n));
  if ((size_t)n_in != n) return fail(MGF_ERR_INVALID, "n must equal the number of bodies");
  if (n == 0) return MGF_OK;
  MGF_TRY(batch_push(b));
  hipStream_t s = b->ctx->stream;
  const size_t fl[5] = {x ? 3 * n : 0, q ? 4 * n : 0, v ? 3 * n : 0, omega ? 3 * n : 0, delta ? 3 * n : 0};
  size_t off[6] = {0, 0, 0, 0, 0, 0};
  for (int k = 0; k < 5; ++k) off[k + 1] = off[k] + ((fl[k] + 3) & ~(size_t)3);
  if (off[5] == 0) return MGF_OK;
  MGF_TRY(b->pack.ensure(off[5], s));
  float* P = b->pack.p;
  const void* src[5] = {x, q, v, omega, delta};
  for (int k = 0; k < 5; ++k)
    if (fl[k]) MGF_HIP_TRY(hipMemcpyAsync(P + off[k], src[k], 4 * fl[k], hipMemcpyHostToDevice, s));
  k_unpack_state<<<nblk(n), kBlock, 0, s>>>(b->bodies(first), (uint32_t)n, nullptr, x ? P + off[0] : nullptr, q ? P + off[1] : nullptr, v ? P + off[2] : nullptr,
                                            omega ? P + off[3] : nullptr, delta ? P + off[4] : nullptr);
  LAUNCH_CHECK();
  MGF_HIP_TRY(hipStreamSynchronize(s));
  return MGF_OK;
}

// The launches of a tick ahead of k_batch_setup and k_batch_solve, a workgroup per world each: the four of a batch of ordinary bodies ...
static mgf_status batch_collide(mgf_batch* b, const BatchArgs& A, uint32_t nmax) {
  hipStream_t s = b->ctx->stream;
  const uint32_t K = b->K;
  k_batch_front<<<K, kBatchBlock, 68u * nmax, s>>>(A);
  LAUNCH_CHECK();
  k_batch_faces<<<K, kBatchBlock, 0, s>>>(A);
  LAUNCH_CHECK();
  k_batch_pairs<<<K, kBatchBlock, 0, s>>>(A);
  LAUNCH_CHECK();
  k_batch_pack<<<K, kBatchBlock, 0, s>>>(A);
  LAUNCH_CHECK();
  return MGF_OK;
}
// ... and the five of a batch that holds bodies of several components (k_batch_parts.h)
static mgf_status batch_collide_parts(mgf_batch* b, const BatchArgs& A, uint32_t nmax) {
  hipStream_t s = b->ctx->stream;
  const uint32_t K = b->K;
  BatchPartsArgs PA;
  PA.A = A; PA.pool = b->pool.p;
  k_batch_parts_front<<<K, kBatchBlock, 68u * nmax, s>>>(A);
  LAUNCH_CHECK();
  k_batch_parts_faces<<<K, kBatchBlock, 0, s>>>(A);
  LAUNCH_CHECK();
  k_batch_parts_obst<<<K, kBatchBlock, 0, s>>>(A);
  LAUNCH_CHECK();
  k_batch_parts_pairs<<<K, kBatchBlock, 0, s>>>(PA);
  LAUNCH_CHECK();
  k_batch_parts_pack<<<K, kBatchBlock, 0, s>>>(PA);
  LAUNCH_CHECK();
  return MGF_OK;
}

// What a rollout (host_batch_rollout.inc, k_batch_rollout.h) hangs into the step's launch train: row t of the controls applied ahead of
// tick t's launches, row t of the traces written behind them - both under the train's own gate, so that they are skipped and run again
// world by world as the tick's launches are.
// ... and of one kind of joints (host_batch_joint.inc): its launch, solved behind the actuation and ahead of the tick, which integrates what it leaves
struct BatchJointHook {
  BatchJointArgs A;  // out, h and iters; the train fills the rest in, the handle's view per PASS, the target table's row per TICK
  uint32_t lds = 0;  // ... and its dynamic LDS
  bool on = false;   // the rig is not empty
};
// ... and of one kind of encoders (host_batch_joint_read.inc): its launch behind the record of every tick that has a row in the kind's readings table
struct BatchJointReadHook {
  BatchJointReadArgs A;  // n; the train fills the rest in, the handle's view per PASS, the table's row per TICK
  int32_t format = -1;   // kJointReadReading / _Full / _FullZero (k_batch_joint_read.h); -1: no trace of the kind
};
struct BatchRolloutHook {
  BatchRolloutArgs A;    // everything but done, act, tick and count, which the train fills in
  int32_t mode = 0;      // MGF_ACTUATE_IMPULSE / _FORCE
  bool act = false;      // the rig is not empty: k_batch_rollout_act ahead of every tick
  BatchSpringArgs S;     // the springs' two launches (k_batch_spring.h), everything but done, act and tick
  bool springs = false;  // the spring rig is not empty: they go ahead of the actuation, which a damper must not see
  BatchJointHook joints, hinges, sliders;  // k_batch_joint.h, k_batch_hinge.h, k_batch_slider.h: solved in this order
  BatchTraceTouchArgs T;  // the touch trace (k_batch_trace.h): V.out - row 0 - and n_touch; the train fills the rest in, the lists' view per PASS
  int32_t touch = -1;    // MGF_ROLLOUT_TOUCH_FULL / _SHORT: k_batch_trace_touch behind every tick's record; -1: no touch trace
  BatchSensorArgs R;     // the sensor trace's cast (k_batch_scan.h): mask, out and parts - the handle's scratch; the train fills the rest in per PASS
  BatchScanRowsArgs W;   // ... and its rows: out - row 0 - and n_sensor; the train fills the rest in per PASS
  int32_t scan = -1;     // MGF_ROLLOUT_SENSOR_HIT / _DEPTH: k_batch_scan_rays and k_batch_scan_rows behind every tick's touch trace; -1: no sensor trace
  BatchJointReadHook hinge_read, slider_read;  // k_batch_read_hinges, k_batch_read_sliders behind every tick t < the kind's table's rows, in this order
  int64_t launches = 0;  // what the hook added to the train's launches
};
// (host_batch_joint.inc, _hinge.inc, _slider.inc, behind this file) the kinds of joints, and a kind's part of the train: per pass what its kernel reads of the handle, per tick its launch
struct JointKind;
struct HingeKind;
struct SliderKind;
template <class T>
static void batch_joint_pass(const mgf_batch* b, BatchJointHook& H);
template <class T>
static mgf_status batch_joint_tick(mgf_batch* b, BatchJointHook& H, uint32_t t, int64_t* launches);
// (host_batch_joint_read.inc, behind this file) a kind of encoders' part of the train: per pass what its kernel reads of the handle, per tick its launch into the table's row
template <class T>
static void batch_joint_read_pass(const mgf_batch* b, BatchJointReadHook& H);
template <class T>
static mgf_status batch_joint_read_tick(mgf_batch* b, BatchJointReadHook& H, uint32_t t, int64_t* launches);
static uint32_t batch_touch_tile(const mgf_batch* b);  // (host_batch_touch.inc, behind this file) the words of dynamic LDS the contact sensors' fold stages
// (host_batch_query.inc, behind this file) the dynamic LDS of a ray cast with a workgroup per work item; what a cast reads of the handle; has it obstacles to meet
static uint32_t batch_ray_lds(const mgf_batch* b);
static void batch_work_args(const mgf_batch* b, BatchWorkArgs* A);
static bool batch_has_obstacles(const mgf_batch* b, int32_t kinds_mask);

// The step's launch train, behind the refusals: n_ticks x World::step (world.rs:227-294) of every world, six (seven) launches a tick, one
// host wait per pass - and with a hook a rollout's two launches a tick among them, the springs' two where that rig is not empty and the
// touch trace's one and the sensor trace's two where they are asked for, and the joints' one where that rig is not empty, and the
// hinges' one where theirs is not, and the hinge trace's one behind every tick that has a row in the readings table, and the sliders'
// one behind the hinges' where that rig is not empty, and the slider trace's one behind the hinge trace's for every tick that has a row in
// the sliders' readings table.
// hook == nullptr: mgf_batch_step, launch for launch.
static mgf_status batch_step_run(mgf_batch* b, float dt, int32_t iters, int64_t n_ticks, mgf_step_stats* stats, BatchRolloutHook* hook) {
  MGF_TRY(batch_push(b));
  MGF_TRY(batch_env_sync(b));
  if (n_ticks == 0) return MGF_OK;
  mgf_ctx* ctx = b->ctx;
  hipStream_t s = ctx->stream;
  const uint32_t K = b->K, NT = (uint32_t)n_ticks;
  const uint32_t nmax = batch_nmax(b);
  const uint32_t lds = 80u * nmax;  // k_batch_solve: 64 bytes a body of solver records, four words of counts (k_batch_front: 64 + 4, k_batch_setup: 12)
  if (lds > b->lds_set) {
    MGF_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_batch_front), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(68u * MGF_BATCH_MAX_BODIES)));
    MGF_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_batch_parts_front), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(68u * MGF_BATCH_MAX_BODIES)));
    MGF_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_batch_solve), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(80u * MGF_BATCH_MAX_BODIES)));
    b->lds_set = 80u * MGF_BATCH_MAX_BODIES;
  }
  MGF_TRY(b->d_stats.ensure((size_t)NT * K * 8, s));
  b->cols_stale = true;  // (the tick's launches - six, seven with bodies of several components - stay as they are: the colliders are gathered before the first reader)
  MGF_HIP_TRY(hipMemsetAsync(b->d_done.p, 0, 4 * (size_t)K, s));
  MGF_HIP_TRY(hipMemsetAsync(b->d_need.p, 0, 8 * (size_t)K, s));
  MGF_HIP_TRY(hipMemsetAsync(b->d_stage.p, 0, 4 * (size_t)K, s));
  if (hook) {  // (the word beside `done`, zeroed where `done` is)
    MGF_TRY(b->d_act.ensure(K, s));
    MGF_HIP_TRY(hipMemsetAsync(b->d_act.p, 0, 4 * (size_t)K, s));
    hook->A.done = b->d_done.p; hook->A.act = b->d_act.p;
    hook->S.done = b->d_done.p; hook->S.act = b->d_act.p;
  }
  const unsigned hook_act_blocks = hook ? (unsigned)((hook->A.n_runs + kBatchBlock - 1) / kBatchBlock) : 0u;
  const unsigned hook_rec_blocks = hook ? (unsigned)((std::max(hook->A.m, K) + kBatchBlock - 1) / kBatchBlock) : 0u;
  std::vector<uint32_t> done(K), need(2 * (size_t)K);
  for (uint32_t first = 0, pass = 0; first < NT; ++pass) {
    BatchArgs A;
    memset(&A, 0, sizeof(A));
    A.B = b->bodies(0);
    float4* u = b->undo.p;
    const size_t n = b->total();
    A.U.p = u; A.U.n = (uint32_t)n;
    A.T = batch_terrains(b);
    A.w_off = b->d_off.p; A.cons = b->cons.p; A.rows = b->rows.p; A.c_off = b->d_coff.p; A.c_cap = b->d_cap.p;
    A.cand = b->cand.p; A.q_off = b->d_qoff.p; A.q_cap = b->d_qcap.p; A.q_count = b->d_qcount.p; A.cont = b->cont.p; A.ncq = b->ncq.p; A.slot = b->slot.p;
    A.na = b->d_na.p; A.degb = b->d_degb.p; A.stage = b->d_stage.p;
    A.done = b->d_done.p; A.need = b->d_need.p; A.c_count = b->d_ccount.p; A.err = b->d_err.p; A.stats = b->d_stats.p;
    A.n_worlds = K; A.iters = (uint32_t)iters;
    A.dt = dt; A.fat_margin = b->params.fat_margin; A.baumgarte = b->params.baumgarte; A.slop = b->params.penetration_slop;
    if (hook) {  // (looked up again for every pass, as the views below are)
      batch_joint_pass<JointKind>(b, hook->joints);
      batch_joint_pass<HingeKind>(b, hook->hinges);
      batch_joint_pass<SliderKind>(b, hook->sliders);
      batch_joint_read_pass<HingeKind>(b, hook->hinge_read);  // (the same rule for the encoders' traces: the rig, the impulse buffer and the TABLE)
      batch_joint_read_pass<SliderKind>(b, hook->slider_read);
    }
    if (hook && hook->touch >= 0) {  // (batch_allot moves the lists between passes: the view is rebuilt with BatchArgs, never kept from an earlier pass)
      BatchRig<mgf_batch_touch>& R = b->touches;
      BatchTouchArgs& V = hook->T.V;
      V.items = reinterpret_cast<const uint4*>(R.dev.p);
      V.order = reinterpret_cast<const uint32_t*>(R.dev.p + R.off[2]);
      V.rig = reinterpret_cast<const TouchIn*>(R.dev.p + R.off[1]);
      V.cons = b->cons.p; V.c_off = b->d_coff.p; V.c_count = b->d_ccount.p; V.w_off = b->d_off.p;
      V.q = b->dm[mgf_batch::AQ].p;
      V.tile = batch_touch_tile(b);
      hook->T.done = b->d_done.p; hook->T.act = b->d_act.p;
    }
    if (hook && hook->scan >= 0) {  // (the same rule for the sensor trace: what it reads of the handle is looked up again for every pass)
      BatchRig<mgf_batch_sensor>& R = b->sensors;
      BatchSensorArgs& V = hook->R;
      batch_work_args(b, &V);
      V.items = reinterpret_cast<const uint4*>(R.dev.p);
      V.order = reinterpret_cast<const uint32_t*>(R.dev.p + R.off[2]);
      V.rig = reinterpret_cast<const SensorIn*>(R.dev.p + R.off[1]);
      V.T = A.T;
      V.x = b->dm[mgf_batch::AX].p; V.q = b->dm[mgf_batch::AQ].p;
      BatchScanRowsArgs& W = hook->W;
      W.hits = V.out; W.parts = reinterpret_cast<const ParticleIn*>(V.parts);
      W.worlds = reinterpret_cast<const int32_t*>(R.dev.p + R.off[3]);
      W.O = batch_obstacles(b); W.tdesc = b->t_desc.p;
      W.obstacles = batch_has_obstacles(b, V.mask) ? 1u : 0u;
      W.done = b->d_done.p; W.act = b->d_act.p;
    }
    for (uint32_t t = first; t < NT; ++t) {
      A.tick = t;
      if (hook) { hook->A.tick = t; hook->A.count = pass == 0 ? 1u : 0u; }  // (an index outside the batch is counted once a tick)
      if (hook && hook->springs) {  // (under the same gate as the actuation behind them: `act` moves behind the tick)
        hook->S.tick = t;
        k_batch_spring_wrench<<<(hook->S.n + kBatchBlock - 1) / kBatchBlock, kBatchBlock, 0, s>>>(hook->S);
        LAUNCH_CHECK();
        k_batch_spring_apply<true><<<(hook->S.n_runs + kBatchBlock - 1) / kBatchBlock, kBatchBlock, 0, s>>>(hook->S);
        LAUNCH_CHECK();
        hook->launches += MGF_BATCH_ROLLOUT_SPRING_LAUNCHES_PER_TICK;
      }
      if (hook && hook->act) {
        if (hook->mode == MGF_ACTUATE_IMPULSE) k_batch_rollout_act<ACTUATE_IMPULSE><<<hook_act_blocks, kBatchBlock, 0, s>>>(hook->A);
        else k_batch_rollout_act<ACTUATE_FORCE><<<hook_act_blocks, kBatchBlock, 0, s>>>(hook->A);
        LAUNCH_CHECK();
        ++hook->launches;
      }
      if (hook) {  // (behind every external impulse and just ahead of the integration: the ball joints, behind them the hinges, behind them the sliders, under one gate)
        MGF_TRY(batch_joint_tick<JointKind>(b, hook->joints, t, &hook->launches));
        MGF_TRY(batch_joint_tick<HingeKind>(b, hook->hinges, t, &hook->launches));
        MGF_TRY(batch_joint_tick<SliderKind>(b, hook->sliders, t, &hook->launches));
      }
      if (b->parts) MGF_TRY(batch_collide_parts(b, A, nmax));
      else MGF_TRY(batch_collide(b, A, nmax));
      k_batch_setup<<<K, kBatchBlock, 12u * nmax, s>>>(A);
      LAUNCH_CHECK();
      k_batch_solve<<<K, kBatchBlock, lds, s>>>(A);
      LAUNCH_CHECK();
      if (hook) {
        k_batch_rollout_record<<<hook_rec_blocks, kBatchBlock, 0, s>>>(hook->A);
        LAUNCH_CHECK();
        ++hook->launches;
      }
      if (hook && hook->touch >= 0) {  // (behind the record: act[k] is final; a workgroup per work item of the contact sensors' plan)
        hook->T.tick = t;
        const unsigned items = (unsigned)b->touches.items.size(), lds_touch = 4u * hook->T.V.tile;
        if (hook->touch == MGF_ROLLOUT_TOUCH_SHORT) k_batch_trace_touch<kTraceTouchShort><<<items, kBatchBlock, lds_touch, s>>>(hook->T);
        else k_batch_trace_touch<kTraceTouchFull><<<items, kBatchBlock, lds_touch, s>>>(hook->T);
        LAUNCH_CHECK();
        hook->launches += MGF_BATCH_ROLLOUT_TOUCH_LAUNCHES_PER_TICK;
      }
      if (hook && hook->scan >= 0) {  // (behind the record: act[k] is final; the cast for every world from bpk, then the rows of the worlds that completed tick t)
        hook->W.tick = t;
        const unsigned rows = (unsigned)((hook->W.n_sensor + kBatchBlock - 1) / kBatchBlock);
        k_batch_scan_rays<<<(unsigned)b->sensors.items.size(), kBatchBlock, batch_ray_lds(b), s>>>(hook->R, b->bpk.p);
        LAUNCH_CHECK();
        if (hook->scan == MGF_ROLLOUT_SENSOR_DEPTH) k_batch_scan_rows<kScanDepth><<<rows, kBatchBlock, 0, s>>>(hook->W);
        else k_batch_scan_rows<kScanHit><<<rows, kBatchBlock, 0, s>>>(hook->W);
        LAUNCH_CHECK();
        hook->launches += MGF_BATCH_ROLLOUT_SENSOR_LAUNCHES_PER_TICK;
      }
      if (hook) {  // (behind the record: act[k] is final; the hinges' readings, then the sliders', row t - and no launch for a tick a table has no row for)
        MGF_TRY(batch_joint_read_tick<HingeKind>(b, hook->hinge_read, t, &hook->launches));
        MGF_TRY(batch_joint_read_tick<SliderKind>(b, hook->slider_read, t, &hook->launches));
      }
    }
    MGF_TRY(d2h(ctx, done.data(), b->d_done.p, K));
    uint32_t err[2] = {0u, 0u};  // [0] k_batch_solve's, [1] k_batch_joint_solve's and k_batch_hinge_solve's (and k_batch_slider_solve's)
    MGF_TRY(d2h(ctx, err, b->d_err.p, 2));
    if (err[0]) return fail(MGF_ERR_HIP, "internal error: a lane of the batch solver gave up waiting for its turn");
    if (err[1]) return fail(MGF_ERR_HIP, "internal error: a lane of the joint solver gave up waiting for its turn");
    first = *std::min_element(done.begin(), done.end());
    if (first >= NT) break;
    // Solver::solve and World::step have no capacity failure (solver.rs:72-78): the worlds whose tick did not fit get what it asked for, and half again
    MGF_TRY(d2h(ctx, need.data(), b->d_need.p, 2 * (size_t)K));
    for (uint32_t k = 0; k < K; ++k) {
      b->h_qfloor[k] = std::max(b->h_qfloor[k], need[2 * k] + need[2 * k] / 2);
      b->h_floor[k] = std::max(b->h_floor[k], need[2 * k + 1] + need[2 * k + 1] / 2);
    }
    MGF_HIP_TRY(hipMemsetAsync(b->d_need.p, 0, 8 * (size_t)K, s));
    ++b->capacity_retries;
    MGF_TRY(batch_allot(b, true));
  }
  MGF_TRY(d2h(ctx, b->h_ccount.data(), b->d_ccount.p, K));
  b->ccount_stale = false;
  if (stats) {
    std::vector<uint32_t> h((size_t)NT * K * 8);
    MGF_TRY(d2h(ctx, h.data(), b->d_stats.p, h.size()));
    for (size_t r = 0; r < (size_t)NT * K; ++r) {
      mgf_step_stats& o = stats[r];
      memset(&o, 0, sizeof(o));
      o.n_bodies = h[8 * r]; o.n_constraints = h[8 * r + 1]; o.n_terrain_constraints = h[8 * r + 2]; o.n_pair_candidates = h[8 * r + 3];
      o.n_refits = h[8 * r + 4]; o.iters = (uint32_t)iters;
    }
  }
  return MGF_OK;
}

// n_ticks x World::step (world.rs:227-294) of every world: one launch per tick, no host wait between the ticks.
extern "C" mgf_status mgf_batch_step(mgf_batch* b, float dt, int32_t iters, int64_t n_ticks, mgf_step_stats* stats) {
  if (!b) return fail(MGF_ERR_INVALID, "batch is NULL");
  if (n_ticks < 0) return fail(MGF_ERR_INVALID, "n_ticks is negative");
  if (iters < 0) return fail(MGF_ERR_INVALID, "iters is negative");
  if (n_ticks > (1 << 20)) return fail(MGF_ERR_INVALID, "n_ticks must be at most 2^20");
  MGF_TRY(ctx_bind(b->ctx));
  return batch_step_run(b, dt, iters, n_ticks, stats, nullptr);
}

// The Solver's constraint list of world `world`'s last tick, in insertion order (bodies named by their index in the world).
extern "C" mgf_status mgf_batch_read_constraints(mgf_batch* b, int64_t world, mgf_constraint* out, int64_t cap, int64_t* count) {
  if (!b) return fail(MGF_ERR_INVALID, "batch is NULL");
  if (world < 0) return fail(MGF_ERR_INVALID, "world index out of range");
  MGF_TRY(ctx_bind(b->ctx));
  if (world >= (int64_t)b->K) return fail(MGF_ERR_INVALID, "world index out of range");
  MGF_TRY(batch_ccount_fresh(b));
  const uint32_t C = b->dev_valid ? b->h_ccount[(size_t)world] : 0u;
  if (count) *count = C;
  if (!out) return MGF_OK;
  if ((int64_t)C > cap) return fail(MGF_ERR_CAPACITY, "constraint buffer too small");
  if (C == 0) return MGF_OK;
  std::vector<CRec> h(C);
  MGF_TRY(d2h(b->ctx, h.data(), b->cons.p + b->h_coff[(size_t)world], C));
  for (uint32_t i = 0; i < C; ++i) crec_to_public(h[i], &out[i]);
  return MGF_OK;
}
