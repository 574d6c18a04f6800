// mgf_batch_read_body_contacts, mgf_batch_overlap_aabb_many: what a caller reads of a batch every tick besides rays and sweeps
// (k_batch_observe.h).  Part of the single translation unit mgf_hip.hip (included there, in order); not compiled on its own.
//
// Both are read-only looks between ticks with the machinery of host_batch_query.inc: a workgroup per world (or per work item of the
// queries' sort by world), a number of launches that depends on neither the number of worlds nor the number of bodies or boxes, the
// counters "query_launches" / "query_run_ns".  Of the tick's state only `rows` is written (the per-body ranges of the constraint list
// are rebuilt from the records on every call; every tick rebuilds `rows` too).  The box query opens as a ray query does
// (batch_query_args / _worlds / _open / _upload) and turns its counts into offsets as the world's does (overlap_offsets, host_query.inc).

extern "C" mgf_status mgf_batch_read_body_contacts(mgf_batch* b, int64_t world, mgf_body_contacts* out, int64_t cap) {
  if (!b) return fail(MGF_ERR_INVALID, "batch is NULL");
  if (!out) return fail(MGF_ERR_INVALID, "NULL argument");
  if (world < -1) return fail(MGF_ERR_INVALID, "world index out of range");
  static_assert(sizeof(mgf_body_contacts) == 24, "k_batch_observe_contacts writes mgf_body_contacts as six words");
  MGF_TRY(ctx_bind(b->ctx));
  size_t first, n;
  MGF_TRY(batch_range(b, world, &first, &n));
  if ((int64_t)n > cap) return fail(MGF_ERR_CAPACITY, "buffer too small");
  batch_call_begin(b);
  if (n == 0) return MGF_OK;
  MGF_TRY(batch_push(b));  // (bodies added behind a tick: the lists are empty, c_count is zero - every record comes out zero)
  hipStream_t s = b->ctx->stream;
  MGF_TRY(b->q_out.ensure(6 * n, s));
  const uint32_t k0 = world < 0 ? 0u : (uint32_t)world, nw = world < 0 ? b->K : 1u;
  const uint32_t nmax = batch_nmax(b, k0, nw);
  BatchContactsArgs A;
  A.cons = b->cons.p; A.rows = b->rows.p; A.c_off = b->d_coff.p; A.c_count = b->d_ccount.p; A.w_off = b->d_off.p;
  A.world0 = k0;
  A.out = reinterpret_cast<uint32_t*>(b->q_out.p);
  MGF_TRY(b->q_tm.mark(0, s));
  k_batch_observe_contacts<<<nw, kBatchBlock, 16u * nmax, s>>>(A);
  LAUNCH_CHECK();
  ++b->q_launches;
  MGF_TRY(b->q_tm.mark(1, s));
  MGF_HIP_TRY(hipMemcpyAsync(out, b->q_out.p, 24 * n, hipMemcpyDeviceToHost, s));
  MGF_HIP_TRY(hipStreamSynchronize(s));
  return b->q_tm.ms(0, 1, &b->q_run_ms);
}

extern "C" mgf_status mgf_batch_overlap_aabb_many(mgf_batch* b, const int32_t* world, const mgf_aabb* boxes, int64_t n_in, uint64_t* out_offsets,
                                                  uint32_t* out_bodies, int64_t cap, int64_t* total) {
  if (!b) return fail(MGF_ERR_INVALID, "batch is NULL");
  if (n_in < 0) return fail(MGF_ERR_INVALID, "n is negative");
  if (cap < 0) return fail(MGF_ERR_INVALID, "cap is negative");
  if ((n_in && (!world || !boxes)) || !out_offsets || (cap > 0 && !out_bodies)) return fail(MGF_ERR_INVALID, "NULL argument");
  MGF_TRY(batch_query_worlds(world, n_in, "too many boxes in one call"));
  static_assert(sizeof(mgf_aabb) == 24, "k_batch_observe_overlap reads mgf_aabb as six words");
  const size_t n = (size_t)n_in;
  MGF_TRY(batch_single_parts(b, "mgf_batch_overlap_aabb_many"));
  MGF_TRY(batch_query_open(b, world, n));
  out_offsets[0] = 0;
  if (total) *total = 0;
  if (n == 0) return MGF_OK;
  mgf_ctx* ctx = b->ctx;
  hipStream_t s = ctx->stream;
  BatchOverlapArgs A;
  memset(&A, 0, sizeof(A));
  BatchQueryUpload U;
  MGF_TRY(batch_query_upload(b, world, boxes, sizeof(mgf_aabb), n, nullptr, &A, &U));
  MGF_TRY(b->q_cnt.ensure(n + 1, s)); MGF_TRY(b->q_off.ensure(n + 1, s));
  MGF_HIP_TRY(hipMemsetAsync(b->q_cnt.p + n, 0, 4, s));
  A.boxes = reinterpret_cast<const float*>(U.queries);
  A.cnt = b->q_cnt.p; A.off = b->q_off.p;
  MGF_TRY(b->q_tm.mark(0, s));
  const bool pq = batch_part_queries(b);  // a body's box: the union of its parts' (host_batch_part_query.inc)
  if (pq) MGF_TRY(batch_pq_overlap<false>(b, A, (unsigned)U.n_items, U.lds));
  else k_batch_observe_overlap<false><<<(unsigned)U.n_items, kBatchBlock, U.lds, s>>>(A);
  LAUNCH_CHECK();
  ++b->q_launches;
  MGF_TRY(b->q_tm.mark(1, s));
  uint64_t sum = 0;
  const mgf_status fits = overlap_offsets(ctx, b->q_cnt.p, n, out_offsets, cap, total, &sum);  // (waits for the stream)
  if (fits != MGF_OK && fits != MGF_ERR_CAPACITY) return fits;
  MGF_TRY(b->q_tm.ms(0, 1, &b->q_run_ms));  // the count pass is timed whether the lists then fit or not
  MGF_TRY(fits);
  if (sum == 0) return MGF_OK;
  MGF_TRY(b->q_vals.ensure((size_t)sum, s));
  A.out = b->q_vals.p;
  MGF_TRY(b->q_tm.mark(0, s));
  MGF_TRY(prim_exclusive_scan_u32(ctx, b->q_cnt.p, b->q_off.p, n + 1));  // (a library primitive: not counted among the launches)
  if (pq) MGF_TRY(batch_pq_overlap<true>(b, A, (unsigned)U.n_items, U.lds));
  else k_batch_observe_overlap<true><<<(unsigned)U.n_items, kBatchBlock, U.lds, s>>>(A);
  LAUNCH_CHECK();
  ++b->q_launches;
  MGF_TRY(b->q_tm.mark(1, s));
  MGF_HIP_TRY(hipMemcpyAsync(out_bodies, b->q_vals.p, 4 * (size_t)sum, hipMemcpyDeviceToHost, s));
  MGF_HIP_TRY(hipStreamSynchronize(s));
  float fill_ms = 0.0f;
  MGF_TRY(b->q_tm.ms(0, 1, &fill_ms));
  b->q_run_ms += fill_ms;
  return MGF_OK;
}
