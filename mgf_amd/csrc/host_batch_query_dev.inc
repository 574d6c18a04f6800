// mgf_batch_raycast_many_dev, mgf_batch_sweep_many_dev: the queries of host_batch_query.inc for a caller whose worlds, queries, ignore
// list and hits are device memory (k_batch_query_dev.h).  Part of the single translation unit mgf_hip.hip (included there, in order,
// behind host_batch_query.inc and host_batch_dev.inc); not compiled on its own.
//
// Everything is enqueued on the context's stream and the call returns without waiting.  With the batch on the device, the terrain and
// obstacle tables unchanged and the handle's scratch large enough a call makes no host wait and no copy between host and device; there
// are no HIP events ("query_run_ns" = 0).  The order of a call is host_batch_dev.inc's: the refusals that need no device, the handle's
// own, EVERY device pointer looked up (dev_span), the overlap of the hits with an input - and only then the first thing is enqueued.
// world_dev given: the plan is built on the device - count | cut | the library's two prefix sums | fill, MGF_BATCH_DEV_QUERY_PLAN_LAUNCHES
// kernels of ours - and the body pass runs on a grid of the host's upper bound of the number of work items.  world_dev == NULL: every
// world has n / n_worlds queries, a work item follows from the workgroup's index, nothing is planned.  Then the passes of the
// host-memory call, over the call's own sanitised copy of the worlds.

// [a, a + na) and [b, b + nb) share a byte
static bool dev_bytes_overlap(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b || !na || !nb) return false;
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + nb && pb < pa + na;
}

// The arrays of a device-pointer call that must not share a byte: the first n_out of the list are written, and each of them is held
// against every entry behind it, in list order.  The first pair that overlaps is refused by name ("a overlaps b"; `inputs`, if given,
// stands for the name of whatever is not written).
struct DevBytes { const void* p; size_t bytes; const char* name; };
static mgf_status dev_outputs_overlap(const DevBytes* a, size_t n, size_t n_out, const char* inputs = nullptr) {
  for (size_t i = 0; i < n_out; ++i)
    for (size_t j = i + 1; j < n; ++j)
      if (dev_bytes_overlap(a[i].p, a[i].bytes, a[j].p, a[j].bytes)) {
        set_error("%s overlaps %s", a[i].name, j < n_out || !inputs ? a[j].name : inputs);
        return MGF_ERR_INVALID;
      }
  return MGF_OK;
}

// Q = ParticleIn (7 words out) or MovingIn (13 words out)
template <class Q>
static mgf_status batch_query_dev_run(mgf_batch* b, const int32_t* world_dev, const Q* q_dev, int64_t n_in, const int32_t* ignore_dev, int32_t kinds_mask,
                                      int32_t* out_dev) {
  constexpr bool kRays = std::is_same<Q, ParticleIn>::value;
  constexpr uint32_t kOut = kRays ? 7u : 13u;
  MGF_TRY(batch_dev_args(b, n_in));
  if (n_in && (!q_dev || !out_dev)) return fail(MGF_ERR_INVALID, "NULL argument");
  MGF_TRY(query_mask_check(kinds_mask));
  const size_t n = (size_t)n_in;
  MGF_TRY(batch_single_parts(b, "mgf_batch_raycast_many_dev / mgf_batch_sweep_many_dev"));
  MGF_TRY(ctx_bind(b->ctx));
  if (!world_dev && n % b->K) return fail(MGF_ERR_INVALID, "without world indices n is a multiple of the number of worlds");
  MGF_TRY(dev_span(b->ctx, world_dev, 4 * n, "world_dev"));
  MGF_TRY(dev_span(b->ctx, q_dev, sizeof(Q) * n, kRays ? "parts_dev" : "casts_dev"));
  MGF_TRY(dev_span(b->ctx, ignore_dev, 4 * n, "ignore_body_dev"));
  MGF_TRY(dev_span(b->ctx, out_dev, 4 * kOut * n, "out_dev"));
  // (a kernel of a later pass reads the queries again after an earlier one wrote hits)
  const DevBytes arrays[4] = {{out_dev, 4 * kOut * n, "out_dev"}, {world_dev, 4 * n, "world_dev"}, {q_dev, sizeof(Q) * n, "q_dev"}, {ignore_dev, 4 * n, "ignore_dev"}};
  MGF_TRY(dev_outputs_overlap(arrays, 4, 1, "an input array"));  // "out_dev overlaps an input array"
  batch_call_begin(b);
  if (n == 0) return MGF_OK;
  BatchDevArgs D;
  MGF_TRY(batch_dev_begin(b, &D));  // the mirror up, the counter of skipped records there
  MGF_TRY(batch_env_sync(b));
  MGF_TRY(batch_cols_refresh(b, &b->q_launches));
  hipStream_t s = b->ctx->stream;
  const uint32_t K = b->K;
  const bool faces = !kRays && batch_has_faces(b, kinds_mask), obstacles = batch_has_obstacles(b, kinds_mask);
  const uint32_t lds = batch_ray_lds(b);
  BatchQueryArgs A;
  memset(&A, 0, sizeof(A));
  batch_work_args(b, &A);
  A.T = batch_terrains(b);
  A.ignore = ignore_dev;
  A.mask = kinds_mask;
  A.out = out_dev;
  BatchItemSrc S;
  memset(&S, 0, sizeof(S));
  S.skipped = D.skipped;
  const bool pq = batch_part_queries(b);  // the body pass sees parts (host_batch_part_query.inc)
  const int32_t* lane_world = nullptr;  // what the lane-per-query passes take a query's world from (null: i / per)
  if (world_dev) {
    const size_t item_cap = n / 256 + std::min<size_t>(n, K);
    MGF_TRY(b->p_cnt.ensure(2 * ((size_t)K + 1), s)); MGF_TRY(b->p_off.ensure(2 * ((size_t)K + 1), s));
    MGF_TRY(b->p_world.ensure(n, s)); MGF_TRY(b->p_rank.ensure(n, s)); MGF_TRY(b->p_order.ensure(n, s)); MGF_TRY(b->p_items.ensure(item_cap, s));
    BatchPlanArgs P;
    memset(&P, 0, sizeof(P));
    P.world = world_dev; P.queries = reinterpret_cast<const int32_t*>(q_dev); P.out = out_dev;
    P.n = (uint32_t)n; P.K = K; P.item_cap = (uint32_t)item_cap;
    P.skipped = D.skipped;
    P.cnt = b->p_cnt.p; P.icnt = b->p_cnt.p + K + 1; P.start = b->p_off.p; P.istart = b->p_off.p + K + 1;
    P.wsan = b->p_world.p; P.rank = b->p_rank.p; P.items = b->p_items.p; P.order = b->p_order.p;
    MGF_HIP_TRY(hipMemsetAsync(b->p_cnt.p, 0, 8 * ((size_t)K + 1), s));
    k_batch_query_plan_count<kOut><<<batch_dev_blocks(n), kBatchBlock, 0, s>>>(P);
    LAUNCH_CHECK();
    k_batch_query_plan_cut<<<batch_dev_blocks(K), kBatchBlock, 0, s>>>(P);
    LAUNCH_CHECK();
    MGF_TRY(prim_exclusive_scan_u32(b->ctx, P.cnt, b->p_off.p, (size_t)K + 1));  // (a library primitive: not counted among the launches)
    MGF_TRY(prim_exclusive_scan_u32(b->ctx, P.icnt, b->p_off.p + K + 1, (size_t)K + 1));
    k_batch_query_plan_fill<<<batch_dev_blocks(n), kBatchBlock, 0, s>>>(P);
    LAUNCH_CHECK();
    b->q_launches += MGF_BATCH_DEV_QUERY_PLAN_LAUNCHES;
    A.items = P.items; A.order = P.order;
    S.n_items = P.istart + K;
    lane_world = P.wsan;
    if (pq) MGF_TRY(batch_pq_bodies<kItemPlan>(b, A, q_dev, S, (unsigned)item_cap));
    else if constexpr (kRays) k_batch_query_ray_dev<kItemPlan><<<(unsigned)item_cap, kBatchBlock, lds, s>>>(A, q_dev, S);
    else k_batch_query_sweep_bodies_dev<kItemPlan><<<(unsigned)item_cap, kBatchBlock, lds, s>>>(A, q_dev, S);
  } else {
    S.per = (uint32_t)(n / K);  // (n > 0 and a multiple of K: at least 1)
    const unsigned grid = (unsigned)((size_t)K * ((S.per + 255u) / 256u));
    if (pq) MGF_TRY(batch_pq_bodies<kItemFixed>(b, A, q_dev, S, grid));
    else if constexpr (kRays) k_batch_query_ray_dev<kItemFixed><<<grid, kBatchBlock, lds, s>>>(A, q_dev, S);
    else k_batch_query_sweep_bodies_dev<kItemFixed><<<grid, kBatchBlock, lds, s>>>(A, q_dev, S);
  }
  LAUNCH_CHECK();
  ++b->q_launches;
  if constexpr (!kRays) return batch_sweep_tail(b, faces, obstacles, lane_world, S.per, q_dev, n, A.out);
  else return obstacles ? batch_ray_obstacles(b, lane_world, S.per, q_dev, n, A.out) : MGF_OK;
}

extern "C" mgf_status mgf_batch_raycast_many_dev(mgf_batch* b, const int32_t* world_dev, const mgf_particle* parts_dev, int64_t n, const int32_t* ignore_body_dev,
                                                 int32_t kinds_mask, mgf_ray_hit* out_dev) {
  return batch_query_dev_run(b, world_dev, reinterpret_cast<const ParticleIn*>(parts_dev), n, ignore_body_dev, kinds_mask, reinterpret_cast<int32_t*>(out_dev));
}

extern "C" mgf_status mgf_batch_sweep_many_dev(mgf_batch* b, const int32_t* world_dev, const mgf_moving_component* casts_dev, int64_t n,
                                               const int32_t* ignore_body_dev, int32_t kinds_mask, mgf_sweep_hit* out_dev) {
  return batch_query_dev_run(b, world_dev, reinterpret_cast<const MovingIn*>(casts_dev), n, ignore_body_dev, kinds_mask, reinterpret_cast<int32_t*>(out_dev));
}
