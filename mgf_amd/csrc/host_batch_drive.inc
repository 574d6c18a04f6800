// mgf_batch_get_many, mgf_batch_set_many, mgf_batch_set_forces, mgf_batch_apply_impulses, mgf_batch_copy_worlds: acting on a batch between
// ticks, on the device (k_batch_drive.h).  Part of the single translation unit mgf_hip.hip (included there, in order); not compiled on its own.
//
// The four per-body calls write the rows the tick already reads (srec: velocities; sp0 / sp1: force and torque) and nothing else: fat
// boxes, colliders, the packed copy and the constraint list stay as the last tick left them, as mgf_world_set leaves the lone world's.
// Records that name the same body are resolved on the host: one stable sort of the record indices by body, the runs handed to the
// kernel, a lane per run - the last record of a run wins a set, an impulse run is walked in the caller's order.  One upload, one launch
// and one host wait per call, whatever n and the number of worlds (counter "drive_launches").
// The copy is a workgroup per pair; a destination whose share of the constraint storage is smaller than the source's list gets a larger
// one first through batch_allot(keep), the path a tick that did not fit takes.

// the checks of a per-body call that need neither the handle's contents nor a device
static mgf_status batch_drive_args(const mgf_batch* b, const int32_t* world, const int32_t* body, int64_t n) {
  if (!b) return fail(MGF_ERR_INVALID, "batch is NULL");
  if (n < 0) return fail(MGF_ERR_INVALID, "n is negative");
  if (n > (int64_t)INT32_MAX) return fail(MGF_ERR_INVALID, "too many records in one call");
  if (n && (!world || !body)) return fail(MGF_ERR_INVALID, "NULL argument");
  for (int64_t i = 0; i < n; ++i) {
    if (world[i] < 0) return fail(MGF_ERR_INVALID, "world index out of range");
    if (body[i] < 0) return fail(MGF_ERR_INVALID, "body index out of range");
  }
  return MGF_OK;
}
// the checks that need the handle, every record's body of the batch, the mirror pushed; the call's counter starts from zero
static mgf_status batch_drive_open(mgf_batch* b, const int32_t* world, const int32_t* body, size_t n, std::vector<uint32_t>* g) {
  MGF_TRY(ctx_bind(b->ctx));
  g->resize(n);
  for (size_t i = 0; i < n; ++i) {
    if ((uint32_t)world[i] >= b->K) return fail(MGF_ERR_INVALID, "world index out of range");
    if ((uint32_t)body[i] >= b->h_n[(size_t)world[i]]) return fail(MGF_ERR_INVALID, "body index out of range");
    (*g)[i] = b->h_off[(size_t)world[i]] + (uint32_t)body[i];
  }
  b->d_launches = 0;
  if (n) MGF_TRY(batch_push(b));
  return MGF_OK;
}

extern "C" mgf_status mgf_batch_get_many(mgf_batch* b, const int32_t* world, const int32_t* body, int64_t n_in, mgf_velocity* vel, mgf_rigid_body_info* info,
                                         mgf_vec3* force, mgf_vec3* torque) {
  MGF_TRY(batch_drive_args(b, world, body, n_in));
  static_assert(sizeof(mgf_velocity) == 24 && sizeof(mgf_rigid_body_info) == 60, "k_batch_drive_get writes them as 6 and 15 words");
  const size_t n = (size_t)n_in;
  std::vector<uint32_t> g;
  MGF_TRY(batch_drive_open(b, world, body, n, &g));
  if (n == 0) return MGF_OK;
  hipStream_t s = b->ctx->stream;
  const size_t w_idx = (n + 3) / 4;
  MGF_TRY(b->q_in.ensure(w_idx + 7 * n, s));
  MGF_HIP_TRY(hipMemcpyAsync(b->q_in.p, g.data(), 4 * n, hipMemcpyHostToDevice, s));
  BatchDriveArgs A;
  memset(&A, 0, sizeof(A));
  A.B = b->bodies(0);
  A.gidx = reinterpret_cast<const uint32_t*>(b->q_in.p);
  A.n = (uint32_t)n;
  A.out = b->q_in.p + w_idx;
  k_batch_drive_get<<<(unsigned)((n + kBatchBlock - 1) / kBatchBlock), kBatchBlock, 0, s>>>(A);
  LAUNCH_CHECK();
  ++b->d_launches;
  std::vector<float> h(28 * n);
  MGF_HIP_TRY(hipMemcpyAsync(h.data(), A.out, 112 * n, hipMemcpyDeviceToHost, s));
  MGF_HIP_TRY(hipStreamSynchronize(s));
  for (size_t i = 0; i < n; ++i) {
    const float* r = &h[28 * i];
    if (vel) memcpy(&vel[i], r, 24);
    if (info) memcpy(&info[i], r + 6, 60);
    if (force) memcpy(&force[i], r + 21, 12);
    if (torque) memcpy(&torque[i], r + 24, 12);
  }
  return MGF_OK;
}

// The records sorted by body (stable), the runs, and the call's one or two arrays of `stride` floats a record, in ONE upload - run
// bodies | run starts | order | a0 | a1, every section from a 16-byte boundary - and the launch.
template <int MODE>
static mgf_status batch_drive_run(mgf_batch* b, const std::vector<uint32_t>& g, const float* a0, const float* a1, uint32_t stride) {
  const size_t n = g.size();
  hipStream_t s = b->ctx->stream;
  std::vector<uint32_t> order(n);
  for (size_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t l, uint32_t r) { return g[l] < g[r]; });
  std::vector<uint32_t> run_g, run;
  for (size_t p = 0; p < n; ++p)
    if (p == 0 || g[order[p]] != g[order[p - 1]]) { run_g.push_back(g[order[p]]); run.push_back((uint32_t)p); }
  run.push_back((uint32_t)n);
  const size_t R = run_g.size();
  const size_t w_g = (R + 3) / 4, w_run = (R + 1 + 3) / 4, w_ord = (n + 3) / 4, w_a = ((size_t)stride * n + 3) / 4;
  const bool packed = stride == 6u;  // (mgf_velocity: linear and angular of a record side by side, one section)
  const size_t o_run = w_g, o_ord = o_run + w_run, o_a0 = o_ord + w_ord, o_a1 = o_a0 + (a0 ? w_a : 0), total = o_a1 + (a1 && !packed ? w_a : 0);
  std::vector<float4> h(total);
  memcpy(h.data(), run_g.data(), 4 * R);
  memcpy(h.data() + o_run, run.data(), 4 * (R + 1));
  memcpy(h.data() + o_ord, order.data(), 4 * n);
  if (a0) memcpy(h.data() + o_a0, a0, 4 * (size_t)stride * n);
  if (a1 && !packed) memcpy(h.data() + o_a1, a1, 4 * (size_t)stride * n);
  MGF_TRY(b->q_in.ensure(total, s));
  MGF_HIP_TRY(hipMemcpyAsync(b->q_in.p, h.data(), 16 * total, hipMemcpyHostToDevice, s));
  BatchDriveArgs A;
  memset(&A, 0, sizeof(A));
  A.B = b->bodies(0);
  A.gidx = reinterpret_cast<const uint32_t*>(b->q_in.p);
  A.run = reinterpret_cast<const uint32_t*>(b->q_in.p + o_run);
  A.order = reinterpret_cast<const uint32_t*>(b->q_in.p + o_ord);
  A.a0 = a0 ? reinterpret_cast<const float*>(b->q_in.p + o_a0) : nullptr;
  A.a1 = !a1 ? nullptr : packed ? A.a0 + 3 : reinterpret_cast<const float*>(b->q_in.p + o_a1);
  A.stride = stride;
  A.n = (uint32_t)R;
  k_batch_drive_set<MODE><<<(unsigned)((R + kBatchBlock - 1) / kBatchBlock), kBatchBlock, 0, s>>>(A);
  LAUNCH_CHECK();
  ++b->d_launches;
  MGF_HIP_TRY(hipStreamSynchronize(s));  // (`h` is read by the copy until here)
  return MGF_OK;
}

extern "C" mgf_status mgf_batch_set_many(mgf_batch* b, const int32_t* world, const int32_t* body, int64_t n, const mgf_velocity* vel) {
  if (!b) return fail(MGF_ERR_INVALID, "batch is NULL");
  if (!vel) return fail(MGF_ERR_INVALID, "NULL argument");
  MGF_TRY(batch_drive_args(b, world, body, n));
  std::vector<uint32_t> g;
  MGF_TRY(batch_drive_open(b, world, body, (size_t)n, &g));
  if (n == 0) return MGF_OK;
  const float* v = reinterpret_cast<const float*>(vel);
  return batch_drive_run<DRIVE_VEL>(b, g, v, v + 3, 6u);
}

extern "C" mgf_status mgf_batch_set_forces(mgf_batch* b, const int32_t* world, const int32_t* body, int64_t n, const mgf_vec3* force, const mgf_vec3* torque) {
  MGF_TRY(batch_drive_args(b, world, body, n));
  std::vector<uint32_t> g;
  MGF_TRY(batch_drive_open(b, world, body, (size_t)n, &g));
  if (n == 0 || (!force && !torque)) return MGF_OK;
  return batch_drive_run<DRIVE_FORCE>(b, g, reinterpret_cast<const float*>(force), reinterpret_cast<const float*>(torque), 3u);
}

extern "C" mgf_status mgf_batch_apply_impulses(mgf_batch* b, const int32_t* world, const int32_t* body, int64_t n, const mgf_vec3* linear,
                                               const mgf_vec3* angular) {
  MGF_TRY(batch_drive_args(b, world, body, n));
  std::vector<uint32_t> g;
  MGF_TRY(batch_drive_open(b, world, body, (size_t)n, &g));
  if (n == 0) return MGF_OK;
  return batch_drive_run<DRIVE_IMPULSE>(b, g, reinterpret_cast<const float*>(linear), reinterpret_cast<const float*>(angular), 3u);
}

// the refusals of a copy, none of which changes anything (mgf_batch_copy_worlds, mgf_batch_copy_worlds_where)
static mgf_status batch_copy_check(mgf_batch* dst, const int32_t* dst_world, const mgf_batch* src, const int32_t* src_world, int64_t n_in) {
  if (!dst || !src) return fail(MGF_ERR_INVALID, "batch is NULL");
  if (n_in < 0) return fail(MGF_ERR_INVALID, "n is negative");
  if (n_in > (int64_t)INT32_MAX) return fail(MGF_ERR_INVALID, "too many pairs in one call");
  if (n_in && (!dst_world || !src_world)) return fail(MGF_ERR_INVALID, "NULL argument");
  for (int64_t i = 0; i < n_in; ++i)
    if (dst_world[i] < 0 || src_world[i] < 0) return fail(MGF_ERR_INVALID, "world index out of range");
  if (dst->ctx != src->ctx) return fail(MGF_ERR_INVALID, "the two batches belong to different contexts");
  MGF_TRY(ctx_bind(dst->ctx));
  const size_t n = (size_t)n_in;
  std::vector<uint8_t> is_dst(dst->K, 0);
  for (size_t i = 0; i < n; ++i) {
    const uint32_t kd = (uint32_t)dst_world[i], ks = (uint32_t)src_world[i];
    if (kd >= dst->K || ks >= src->K) return fail(MGF_ERR_INVALID, "world index out of range");
    if (dst->h_n[kd] != src->h_n[ks]) return fail(MGF_ERR_INVALID, "a destination world and its source hold different numbers of bodies: nothing was copied");
    if (is_dst[kd]) return fail(MGF_ERR_INVALID, "a destination world is named twice: nothing was copied");
    is_dst[kd] = 1;
  }
  if (dst == src)
    for (size_t i = 0; i < n; ++i)
      if (is_dst[(size_t)src_world[i]]) return fail(MGF_ERR_INVALID, "a world is both a source and a destination: nothing was copied");
  return MGF_OK;
}
// Both batches on the device, and the lists must fit: a destination with a smaller share asks for what the source's list needs, as a tick
// that did not fit does (the larger share stays, as after a re-run tick, until "cons_per_body" is set again; a failed allotment leaves
// the floors as they were)
static mgf_status batch_copy_open(mgf_batch* dst, const int32_t* dst_world, mgf_batch* src, const int32_t* src_world, size_t n) {
  MGF_TRY(batch_push(src));
  MGF_TRY(batch_push(dst));
  if (src->parts) MGF_TRY(batch_parts_enable(dst));  // (a destination of ordinary bodies gets part rows before anything of the copy is enqueued)
  MGF_TRY(batch_ccount_fresh(src));  // (behind a masked copy into `src`, host_batch_dev.inc)
  bool grow = false;
  const std::vector<uint32_t> floor_was = dst->h_floor;
  for (size_t i = 0; i < n; ++i) {
    const uint32_t kd = (uint32_t)dst_world[i], need = src->h_ccount[(size_t)src_world[i]];
    if (need > dst->h_cap[kd]) { dst->h_floor[kd] = std::max(dst->h_floor[kd], need); grow = true; }
  }
  if (grow) {
    if (dst->lists_valid && dst->K) ++dst->d_launches;  // (k_batch_move_lists)
    const mgf_status st = batch_allot(dst, true);
    if (st != MGF_OK) { dst->h_floor = floor_was; return st; }
  }
  return MGF_OK;
}
static BatchCopyArgs batch_copy_args(const mgf_batch* dst, const mgf_batch* src, const uint2* pairs) {
  BatchCopyArgs A;
  memset(&A, 0, sizeof(A));
  A.D = dst->bodies(0); A.S = src->bodies(0);
  A.pairs = pairs;
  A.d_off = dst->d_off.p; A.s_off = src->d_off.p;
  A.d_cons = dst->cons.p; A.s_cons = src->cons.p;
  A.d_coff = dst->d_coff.p; A.d_cap = dst->d_cap.p; A.s_coff = src->d_coff.p;
  A.d_count = dst->d_ccount.p; A.s_count = src->d_ccount.p;
  A.s_stale = src->cols_stale ? 1u : 0u;
  return A;
}

// the part rows of the copied worlds, behind the copy's own launch: a clone of a world of bodies of several components has its parts,
// and a world of ordinary bodies copied over one has none (a batch without part rows has neither: no launch)
static mgf_status batch_copy_parts(mgf_batch* dst, const mgf_batch* src, const uint2* pairs, size_t n, const int32_t* mask) {
  if (!dst->parts) return MGF_OK;
  BatchPartsCopyArgs A;
  memset(&A, 0, sizeof(A));
  A.D = dst->bodies(0); A.S = src->bodies(0);
  A.s_parts = src->parts ? 1u : 0u;
  A.pairs = pairs; A.d_off = dst->d_off.p; A.s_off = src->d_off.p; A.mask = mask;
  k_batch_parts_copy<<<(unsigned)n, kBatchBlock, 0, dst->ctx->stream>>>(A);
  LAUNCH_CHECK();
  ++dst->d_launches;
  return MGF_OK;
}

extern "C" mgf_status mgf_batch_copy_worlds(mgf_batch* dst, const int32_t* dst_world, const mgf_batch* src_in, const int32_t* src_world, int64_t n_in) {
  MGF_TRY(batch_copy_check(dst, dst_world, src_in, src_world, n_in));
  mgf_batch* src = const_cast<mgf_batch*>(src_in);  // (its mirror may have to go up, its colliders are read where they are: nothing of its state changes)
  const size_t n = (size_t)n_in;
  dst->d_launches = 0;
  if (n == 0) return MGF_OK;
  MGF_TRY(batch_copy_open(dst, dst_world, src, src_world, n));
  hipStream_t s = dst->ctx->stream;
  std::vector<uint2> pairs(n);
  for (size_t i = 0; i < n; ++i) pairs[i] = make_uint2((uint32_t)dst_world[i], (uint32_t)src_world[i]);
  MGF_TRY(dst->q_in.ensure((n + 1) / 2, s));
  MGF_HIP_TRY(hipMemcpyAsync(dst->q_in.p, pairs.data(), 8 * n, hipMemcpyHostToDevice, s));
  const BatchCopyArgs A = batch_copy_args(dst, src, reinterpret_cast<const uint2*>(dst->q_in.p));
  k_batch_drive_copy<<<(unsigned)n, kBatchBlock, 0, s>>>(A);
  LAUNCH_CHECK();
  ++dst->d_launches;
  MGF_TRY(batch_copy_parts(dst, src, A.pairs, n, nullptr));
  MGF_HIP_TRY(hipStreamSynchronize(s));  // (`pairs` is read by the copy until here)
  for (size_t i = 0; i < n; ++i) dst->h_ccount[(size_t)dst_world[i]] = src->h_ccount[(size_t)src_world[i]];
  return MGF_OK;
}
