// mgf_batch_read_colliders, mgf_batch_raycast_many, mgf_batch_sweep_many: the queries of host_query.inc for the worlds of a batch
// (k_batch_query.h).  Part of the single translation unit mgf_hip.hip (included there, in order); not compiled on its own.
//
// A call sorts its query indices by world (one stable counting sort), cuts every world's run into work items of up to 256 queries,
// uploads items, queries, order, ignore list and (for the sweeps' face pass and the obstacle pass, a lane per query) the worlds in ONE copy, launches a workgroup per work item - the number of launches depends on
// neither the number of worlds nor the number of queries - and downloads the hits: one host wait per call.  Nothing of the tick's state
// is written; of it only bpk is read, once, by the collider gather behind a mgf_batch_step (batch_cols_refresh).
// batch_query_args / _worlds / _open / _upload are every front end's steps ahead of its launches, the box query's
// (host_batch_observe.inc) too; the kinds_mask and tag checks are host_query.inc's.  What every cast of a batch shares beyond that is
// here once, for the device-pointer calls, the sensors and the cameras (the files behind this one) as well: batch_call_begin,
// batch_work_args, batch_ray_lds, and the passes with a lane per query - batch_ray_obstacles, batch_sweep_tail.

extern "C" mgf_status mgf_batch_read_colliders(mgf_batch* b, int64_t world, mgf_moving_component* out, int64_t cap) {
  if (!b) return fail(MGF_ERR_INVALID, "batch is NULL");
  if (!out) return fail(MGF_ERR_INVALID, "NULL argument");
  if (world < -1) return fail(MGF_ERR_INVALID, "world index out of range");
  MGF_TRY(ctx_bind(b->ctx));
  size_t first, n;
  MGF_TRY(batch_range(b, world, &first, &n));
  if ((int64_t)n > cap) return fail(MGF_ERR_CAPACITY, "buffer too small");
  if (n == 0) return MGF_OK;
  MGF_TRY(batch_push(b));
  MGF_TRY(batch_cols_refresh(b, nullptr));
  hipStream_t s = b->ctx->stream;
  MGF_TRY(b->pack.ensure(11 * n, s));
  k_pack_colliders<<<nblk(n), kBlock, 0, s>>>(b->bodies(first), (uint32_t)n, nullptr, reinterpret_cast<uint32_t*>(b->pack.p));
  LAUNCH_CHECK();
  MGF_HIP_TRY(hipMemcpyAsync(out, b->pack.p, 44 * n, hipMemcpyDeviceToHost, s));
  MGF_HIP_TRY(hipStreamSynchronize(s));
  return MGF_OK;
}

// the checks of a query call that need neither the handle's contents nor a device (q: the queries; out: where the call's answers go)
static mgf_status batch_query_args(const mgf_batch* b, const int32_t* world, const void* q, int64_t n, const void* out) {
  if (!b) return fail(MGF_ERR_INVALID, "batch is NULL");
  if (n < 0) return fail(MGF_ERR_INVALID, "n is negative");
  if (n && (!world || !q || !out)) return fail(MGF_ERR_INVALID, "NULL argument");
  return MGF_OK;
}
static mgf_status batch_query_worlds(const int32_t* world, int64_t n, const char* too_many) {
  if (n > (int64_t)INT32_MAX) return fail(MGF_ERR_INVALID, too_many);
  for (int64_t i = 0; i < n; ++i)
    if (world[i] < 0) return fail(MGF_ERR_INVALID, "world index out of range");
  return MGF_OK;
}

// the query indices of a call by world, in the caller's order within a world (one stable counting sort); work items of up to 256 queries
struct BatchQueryPlan {
  std::vector<uint32_t> start;  // world k's queries at the sorted positions [start[k], start[k + 1])
  size_t n_items = 0;
  BatchQueryPlan(uint32_t K, const int32_t* world, size_t n) : start((size_t)K + 1, 0u) {
    for (size_t i = 0; i < n; ++i) ++start[(size_t)world[i] + 1];
    for (uint32_t k = 0; k < K; ++k) start[k + 1] += start[k];
    for (uint32_t k = 0; k < K; ++k) n_items += (start[k + 1] - start[k] + 255u) / 256u;
  }
  // items[n_items] = (world, first, count <= 256, -); order[n]: sorted position -> the caller's query index
  void fill(const int32_t* world, size_t n, uint4* items, uint32_t* order) const {
    const uint32_t K = (uint32_t)start.size() - 1u;
    size_t at = 0;
    for (uint32_t k = 0; k < K; ++k)
      for (uint32_t f = start[k]; f < start[k + 1]; f += 256u) items[at++] = make_uint4(k, f, std::min(256u, start[k + 1] - f), 0u);
    std::vector<uint32_t> cur(start.begin(), start.end() - 1);
    for (size_t i = 0; i < n; ++i) order[cur[(size_t)world[i]]++] = (uint32_t)i;
  }
};

// every call that counts its launches and times its passes opens with this ("query_launches", "query_run_ns")
static void batch_call_begin(mgf_batch* b) { b->q_launches = 0; b->q_run_ms = 0.0f; }

// the checks that need the handle; the call's counters start from zero
static mgf_status batch_query_open(mgf_batch* b, const int32_t* world, size_t n) {
  MGF_TRY(ctx_bind(b->ctx));
  for (size_t i = 0; i < n; ++i)
    if ((uint32_t)world[i] >= b->K) return fail(MGF_ERR_INVALID, "world index out of range");
  batch_call_begin(b);
  return MGF_OK;
}

// What every kernel with a workgroup per work item reads of the handle, and the dynamic LDS of those that cast rays or sweep: 32 bytes
// a body of the largest world, kBatchQueryRed words (at most 32 KB + 256 bytes: two workgroups a CU at the largest world)
static void batch_work_args(const mgf_batch* b, BatchWorkArgs* A) {
  A->col0 = b->dm[mgf_batch::ACOL0].p; A->col1 = b->dm[mgf_batch::ACOL1].p; A->w_off = b->d_off.p;
}
static uint32_t batch_ray_lds(const mgf_batch* b) { return 32u * batch_nmax(b) + 16u * kBatchQueryRed; }

// The passes with a lane per query behind a body pass, for every front end of the casts.  Which of them a call has: the sweeps' face
// pass when a world of the batch has a terrain to sweep against, the obstacle pass when one has an obstacle to meet.
static bool batch_has_faces(const mgf_batch* b, int32_t kinds_mask) { return (kinds_mask & MGF_QUERY_TERRAIN) && b->t_worlds; }
static bool batch_has_obstacles(const mgf_batch* b, int32_t kinds_mask) { return (kinds_mask & MGF_QUERY_OBSTACLES) && b->o_worlds; }
// worlds: a query's world by the caller's index, or (null) every world has `per` queries; parts / casts, out: n records of device memory
static mgf_status batch_ray_obstacles(mgf_batch* b, const int32_t* worlds, uint32_t per, const ParticleIn* parts, size_t n, int32_t* out) {
  k_batch_query_ray_obstacles<<<(unsigned)((n + kBatchBlock - 1) / kBatchBlock), kBatchBlock, 0, b->ctx->stream>>>(batch_obstacles(b), b->t_desc.p, worlds, per, parts,
                                                                                                             (uint32_t)n, out);
  LAUNCH_CHECK();
  ++b->q_launches;
  return MGF_OK;
}
static mgf_status batch_sweep_tail(mgf_batch* b, bool faces, bool obstacles, const int32_t* worlds, uint32_t per, const MovingIn* casts, size_t n, int32_t* out) {
  const unsigned nb = (unsigned)((n + kBatchBlock - 1) / kBatchBlock);
  hipStream_t s = b->ctx->stream;
  if (faces) {
    k_batch_query_sweep_faces<<<nb, kBatchBlock, 0, s>>>(batch_terrains(b), worlds, per, casts, (uint32_t)n, out);
    LAUNCH_CHECK();
    ++b->q_launches;
  }
  if (obstacles) {
    k_batch_query_sweep_obstacles<<<nb, kBatchBlock, 0, s>>>(batch_obstacles(b), b->t_desc.p, worlds, per, casts, (uint32_t)n, out);
    LAUNCH_CHECK();
    ++b->q_launches;
  }
  return MGF_OK;
}

// What the ray, sweep and box queries do ahead of their launches (n > 0): the bodies added since pushed, the plan, ONE upload -
// items | queries | order | ignore | world, every section from a 16-byte boundary - and the colliders refreshed behind a tick.
struct BatchQueryUpload {
  size_t n_items = 0;
  const float4* queries = nullptr;  // the caller's q_bytes a query, in the caller's order
  const int32_t* ignore = nullptr;  // null: none given
  const int32_t* world = nullptr;   // by the caller's index; null: not asked for
  uint32_t lds = 0;                 // 32 bytes a body of the largest world (at most 32 KB)
  std::vector<float4> host;         // what the copy reads: alive until the call has waited for the stream
};
static mgf_status batch_query_upload(mgf_batch* b, const int32_t* world, const void* queries, size_t q_bytes, size_t n, const int32_t* ignore_body,
                                     BatchWorkArgs* A, BatchQueryUpload* U, bool with_world = false) {
  MGF_TRY(batch_push(b));
  hipStream_t s = b->ctx->stream;
  const BatchQueryPlan plan(b->K, world, n);
  const size_t w_q = (n * q_bytes + 15) / 16, w_idx = (4 * n + 15) / 16;
  const size_t o_q = plan.n_items, o_order = o_q + w_q, o_ign = o_order + w_idx, o_world = o_ign + (ignore_body ? w_idx : 0),
               total = o_world + (with_world ? w_idx : 0);
  std::vector<float4>& h = U->host;
  h.resize(total);
  memcpy(h.data() + o_q, queries, n * q_bytes);
  plan.fill(world, n, reinterpret_cast<uint4*>(h.data()), reinterpret_cast<uint32_t*>(h.data() + o_order));
  if (ignore_body) memcpy(h.data() + o_ign, ignore_body, 4 * n);
  if (with_world) memcpy(h.data() + o_world, world, 4 * n);
  MGF_TRY(b->q_in.ensure(total, s));
  MGF_HIP_TRY(hipMemcpyAsync(b->q_in.p, h.data(), 16 * total, hipMemcpyHostToDevice, s));
  MGF_TRY(batch_cols_refresh(b, &b->q_launches));
  batch_work_args(b, A);
  A->items = reinterpret_cast<const uint4*>(b->q_in.p);
  A->order = reinterpret_cast<const uint32_t*>(b->q_in.p + o_order);
  U->n_items = plan.n_items; U->queries = b->q_in.p + o_q;
  U->ignore = ignore_body ? reinterpret_cast<const int32_t*>(b->q_in.p + o_ign) : nullptr;
  U->world = with_world ? reinterpret_cast<const int32_t*>(b->q_in.p + o_world) : nullptr;
  U->lds = 32u * batch_nmax(b);
  return MGF_OK;
}

// Q = ParticleIn (7 words out) or MovingIn (13 words out)
template <class Q>
static mgf_status batch_query_run(mgf_batch* b, const int32_t* world, const Q* queries, int64_t n_in, const int32_t* ignore_body, int32_t kinds_mask,
                                  int32_t* out) {
  constexpr bool kRays = std::is_same<Q, ParticleIn>::value;
  constexpr size_t kOut = kRays ? 7 : 13;
  const size_t n = (size_t)n_in;
  MGF_TRY(batch_single_parts(b, "mgf_batch_raycast_many / mgf_batch_sweep_many"));
  MGF_TRY(batch_query_open(b, world, n));
  if (n == 0) return MGF_OK;
  hipStream_t s = b->ctx->stream;
  BatchQueryArgs A;
  memset(&A, 0, sizeof(A));
  BatchQueryUpload U;
  MGF_TRY(batch_env_sync(b));
  const bool faces = !kRays && batch_has_faces(b, kinds_mask), obstacles = batch_has_obstacles(b, kinds_mask);
  MGF_TRY(batch_query_upload(b, world, queries, sizeof(Q), n, ignore_body, &A, &U, faces || obstacles));
  MGF_TRY(b->q_out.ensure(kOut * n, s));
  const uint32_t lds = batch_ray_lds(b);
  A.T = batch_terrains(b);
  A.ignore = U.ignore;
  A.mask = kinds_mask;
  A.out = b->q_out.p;
  const Q* dq = reinterpret_cast<const Q*>(U.queries);
  MGF_TRY(b->q_tm.mark(0, s));
  const bool pq = batch_part_queries(b);  // the body pass sees parts (host_batch_part_query.inc)
  if constexpr (kRays) {
    if (pq) MGF_TRY(batch_pq_bodies<kItemTable>(b, A, dq, BatchItemSrc(), (unsigned)U.n_items));
    else k_batch_query_ray<<<(unsigned)U.n_items, kBatchBlock, lds, s>>>(A, dq);
    LAUNCH_CHECK();
    ++b->q_launches;
    if (obstacles) MGF_TRY(batch_ray_obstacles(b, U.world, 0u, dq, n, A.out));
  } else {
    if (pq) MGF_TRY(batch_pq_bodies<kItemTable>(b, A, dq, BatchItemSrc(), (unsigned)U.n_items));
    else k_batch_query_sweep_bodies<<<(unsigned)U.n_items, kBatchBlock, lds, s>>>(A, dq);
    LAUNCH_CHECK();
    ++b->q_launches;
    MGF_TRY(batch_sweep_tail(b, faces, obstacles, U.world, 0u, dq, n, A.out));
  }
  MGF_TRY(b->q_tm.mark(1, s));
  MGF_HIP_TRY(hipMemcpyAsync(out, b->q_out.p, 4 * kOut * n, hipMemcpyDeviceToHost, s));
  MGF_HIP_TRY(hipStreamSynchronize(s));
  return b->q_tm.ms(0, 1, &b->q_run_ms);
}

extern "C" mgf_status mgf_batch_raycast_many(mgf_batch* b, const int32_t* world, const mgf_particle* parts, int64_t n, const int32_t* ignore_body,
                                             int32_t kinds_mask, mgf_ray_hit* out) {
  MGF_TRY(batch_query_args(b, world, parts, n, out));
  MGF_TRY(query_mask_check(kinds_mask));
  MGF_TRY(batch_query_worlds(world, n, "too many queries in one call"));
  static_assert(sizeof(mgf_ray_hit) == 28 && sizeof(mgf_particle) == sizeof(ParticleIn), "k_batch_query_ray writes mgf_ray_hit as seven words");
  return batch_query_run(b, world, reinterpret_cast<const ParticleIn*>(parts), n, ignore_body, kinds_mask, reinterpret_cast<int32_t*>(out));
}

extern "C" mgf_status mgf_batch_sweep_many(mgf_batch* b, const int32_t* world, const mgf_moving_component* casts, int64_t n, const int32_t* ignore_body,
                                           int32_t kinds_mask, mgf_sweep_hit* out) {
  MGF_TRY(batch_query_args(b, world, casts, n, out));
  MGF_TRY(query_mask_check(kinds_mask));
  MGF_TRY(batch_query_worlds(world, n, "too many queries in one call"));
  static_assert(sizeof(mgf_sweep_hit) == 52 && sizeof(mgf_moving_component) == sizeof(MovingIn), "k_batch_query_sweep_bodies writes mgf_sweep_hit as 13 words");
  MGF_TRY(query_tags_check(casts, n));
  return batch_query_run(b, world, reinterpret_cast<const MovingIn*>(casts), n, ignore_body, kinds_mask, reinterpret_cast<int32_t*>(out));
}
