// mgf_batch_read_body_contacts, mgf_batch_overlap_aabb_many: what a caller reads of a batch every tick besides rays and sweeps
// (k_batch_observe.h).  Part of the single translation unit mgf_hip.hip (included there, in order); not compiled on its own.
//
// Both are read-only looks between ticks with the machinery of host_batch_query.inc: a workgroup per world (or per work item of the
// queries' sort by world), a number of launches that depends on neither the number of worlds nor the number of bodies or boxes, the
// counters "query_launches" / "query_run_ns".  Of the tick's state only `rows` is written (the per-body ranges of the constraint list
// are rebuilt from the records on every call; every tick rebuilds `rows` too).

extern "C" mgf_status mgf_batch_read_body_contacts(mgf_batch* b, int64_t world, mgf_body_contacts* out, int64_t cap) {
  if (!b) return fail(MGF_ERR_INVALID, "batch is NULL");
  if (!out) return fail(MGF_ERR_INVALID, "NULL argument");
  if (world < -1) return fail(MGF_ERR_INVALID, "world index out of range");
  static_assert(sizeof(mgf_body_contacts) == 24, "k_batch_observe_contacts writes mgf_body_contacts as six words");
  MGF_TRY(ctx_bind(b->ctx));
  size_t first, n;
  MGF_TRY(batch_range(b, world, &first, &n));
  if ((int64_t)n > cap) return fail(MGF_ERR_CAPACITY, "buffer too small");
  b->q_launches = 0; b->q_run_ms = 0.0f;
  if (n == 0) return MGF_OK;
  MGF_TRY(batch_push(b));  // (bodies added behind a tick: the lists are empty, c_count is zero - every record comes out zero)
  hipStream_t s = b->ctx->stream;
  for (hipEvent_t& e : b->q_ev)
    if (!e) MGF_HIP_TRY(hipEventCreate(&e));
  MGF_TRY(b->q_out.ensure(6 * n, s));
  const uint32_t k0 = world < 0 ? 0u : (uint32_t)world, nw = world < 0 ? b->K : 1u;
  uint32_t nmax = 0;
  for (uint32_t k = k0; k < k0 + nw; ++k) nmax = std::max(nmax, b->h_n[k]);
  BatchContactsArgs A;
  A.cons = b->cons.p; A.rows = b->rows.p; A.c_off = b->d_coff.p; A.c_count = b->d_ccount.p; A.w_off = b->d_off.p;
  A.world0 = k0;
  A.out = reinterpret_cast<uint32_t*>(b->q_out.p);
  MGF_HIP_TRY(hipEventRecord(b->q_ev[0], s));
  k_batch_observe_contacts<<<nw, kBatchBlock, 16u * nmax, s>>>(A);
  LAUNCH_CHECK();
  ++b->q_launches;
  MGF_HIP_TRY(hipEventRecord(b->q_ev[1], s));
  MGF_HIP_TRY(hipMemcpyAsync(out, b->q_out.p, 24 * n, hipMemcpyDeviceToHost, s));
  MGF_HIP_TRY(hipStreamSynchronize(s));
  MGF_HIP_TRY(hipEventElapsedTime(&b->q_run_ms, b->q_ev[0], b->q_ev[1]));
  return MGF_OK;
}

extern "C" mgf_status mgf_batch_overlap_aabb_many(mgf_batch* b, const int32_t* world, const mgf_aabb* boxes, int64_t n_in, uint64_t* out_offsets,
                                                  uint32_t* out_bodies, int64_t cap, int64_t* total) {
  if (!b) return fail(MGF_ERR_INVALID, "batch is NULL");
  if (n_in < 0) return fail(MGF_ERR_INVALID, "n is negative");
  if (cap < 0) return fail(MGF_ERR_INVALID, "cap is negative");
  if ((n_in && (!world || !boxes)) || !out_offsets || (cap > 0 && !out_bodies)) return fail(MGF_ERR_INVALID, "NULL argument");
  if (n_in > (int64_t)INT32_MAX) return fail(MGF_ERR_INVALID, "too many boxes in one call");
  for (int64_t i = 0; i < n_in; ++i)
    if (world[i] < 0) return fail(MGF_ERR_INVALID, "world index out of range");
  static_assert(sizeof(mgf_aabb) == 24, "k_batch_observe_overlap reads mgf_aabb as six words");
  MGF_TRY(ctx_bind(b->ctx));
  const uint32_t K = b->K;
  const size_t n = (size_t)n_in;
  for (size_t i = 0; i < n; ++i)
    if ((uint32_t)world[i] >= K) return fail(MGF_ERR_INVALID, "world index out of range");
  b->q_launches = 0; b->q_run_ms = 0.0f;
  out_offsets[0] = 0;
  if (total) *total = 0;
  if (n == 0) return MGF_OK;
  MGF_TRY(batch_push(b));
  mgf_ctx* ctx = b->ctx;
  hipStream_t s = ctx->stream;
  for (hipEvent_t& e : b->q_ev)
    if (!e) MGF_HIP_TRY(hipEventCreate(&e));
  const BatchQueryPlan plan(K, world, n);
  const size_t n_items = plan.n_items;
  // one upload: items | boxes | order, every section from a 16-byte boundary
  const size_t w_q = (24 * n + 15) / 16, w_idx = (4 * n + 15) / 16, o_q = n_items, o_order = o_q + w_q, up = o_order + w_idx;
  std::vector<float4> h(up);
  memcpy(h.data() + o_q, boxes, 24 * n);
  plan.fill(world, n, reinterpret_cast<uint4*>(h.data()), reinterpret_cast<uint32_t*>(h.data() + o_order));
  MGF_TRY(b->q_in.ensure(up, s));
  MGF_TRY(b->q_cnt.ensure(n + 1, s)); MGF_TRY(b->q_off.ensure(n + 1, s));
  MGF_HIP_TRY(hipMemcpyAsync(b->q_in.p, h.data(), 16 * up, hipMemcpyHostToDevice, s));
  MGF_HIP_TRY(hipMemsetAsync(b->q_cnt.p + n, 0, 4, s));
  MGF_TRY(batch_cols_refresh(b, &b->q_launches));
  uint32_t nmax = 0;
  for (uint32_t c : b->h_n) nmax = std::max(nmax, c);
  const uint32_t lds = 32u * nmax;  // (at most 32 KB)
  BatchOverlapArgs A;
  memset(&A, 0, sizeof(A));
  A.col0 = b->dm[mgf_batch::ACOL0].p; A.col1 = b->dm[mgf_batch::ACOL1].p; A.w_off = b->d_off.p;
  A.items = reinterpret_cast<const uint4*>(b->q_in.p);
  A.order = reinterpret_cast<const uint32_t*>(b->q_in.p + o_order);
  A.boxes = reinterpret_cast<const float*>(b->q_in.p + o_q);
  A.cnt = b->q_cnt.p; A.off = b->q_off.p;
  MGF_HIP_TRY(hipEventRecord(b->q_ev[0], s));
  k_batch_observe_overlap<false><<<(unsigned)n_items, kBatchBlock, lds, s>>>(A);
  LAUNCH_CHECK();
  ++b->q_launches;
  MGF_HIP_TRY(hipEventRecord(b->q_ev[1], s));
  // the offsets and the total are the caller's whether the lists fit or not (the world's contract)
  std::vector<uint32_t> cnt(n);
  MGF_TRY(d2h(ctx, cnt.data(), b->q_cnt.p, n));
  uint64_t sum = 0;
  for (size_t i = 0; i < n; ++i) { sum += cnt[i]; out_offsets[i + 1] = sum; }
  if (total) *total = (int64_t)sum;
  MGF_HIP_TRY(hipEventElapsedTime(&b->q_run_ms, b->q_ev[0], b->q_ev[1]));
  if ((int64_t)sum > cap) return fail(MGF_ERR_CAPACITY, "out_bodies too small (*total reports the number required)");
  if (sum > 0xFFFFFFFFull) return fail(MGF_ERR_CAPACITY, "more than 2^32 - 1 results in one call");
  if (sum == 0) return MGF_OK;
  MGF_TRY(b->q_vals.ensure((size_t)sum, s));
  A.out = b->q_vals.p;
  MGF_HIP_TRY(hipEventRecord(b->q_ev[0], s));
  MGF_TRY(prim_exclusive_scan_u32(ctx, b->q_cnt.p, b->q_off.p, n + 1));  // (a library primitive: not counted among the launches)
  k_batch_observe_overlap<true><<<(unsigned)n_items, kBatchBlock, lds, s>>>(A);
  LAUNCH_CHECK();
  ++b->q_launches;
  MGF_HIP_TRY(hipEventRecord(b->q_ev[1], s));
  MGF_HIP_TRY(hipMemcpyAsync(out_bodies, b->q_vals.p, 4 * (size_t)sum, hipMemcpyDeviceToHost, s));
  MGF_HIP_TRY(hipStreamSynchronize(s));
  float fill_ms = 0.0f;
  MGF_HIP_TRY(hipEventElapsedTime(&fill_ms, b->q_ev[0], b->q_ev[1]));
  b->q_run_ms += fill_ms;
  return MGF_OK;
}
