// mgf_batch_read_zones_nearest, mgf_batch_read_zones_nearest_dev, mgf_batch_overlap_nearest_dev: the zone rig's three reads with the
// nearest-first record - per box the count and the k nearest bodies, and their squared distances where asked for (k_batch_nearest.h).
// Part of the single translation unit mgf_hip.hip (included there, in order, behind host_batch_zone.inc); not compiled on its own.
//
// The rig, its plan, its upload and the refusals that need no device are the zones' (host_batch_zone.inc, host_batch_rig.inc): these
// calls read b->zones and never change it.  What differs is the limit on k (MGF_BATCH_ZONE_NEAREST_MAX_K), one more array - dist2,
// k words a box - and the kernel.  A read is MGF_BATCH_NEAREST_LAUNCHES = 1 launch - and the collider gather behind a step - and, for
// the device forms, no host wait and no copy between host and device.  The order of both device-pointer calls is
// host_batch_query_dev.inc's: the refusals that need no device, the handle's own, EVERY device pointer looked up (dev_span), the overlap
// of what is written with everything else - and only then the first thing is enqueued.

static mgf_status nearest_k_check(int32_t k) {
  if (k < 0 || k > MGF_BATCH_ZONE_NEAREST_MAX_K) return fail(MGF_ERR_INVALID, "k is outside [0, MGF_BATCH_ZONE_NEAREST_MAX_K]");
  return MGF_OK;
}

// what both launches share: the zones' arguments and where the distances go
static void batch_nearest_args(const mgf_batch* b, int32_t k, int32_t* out_dev, float* dist2_dev, BatchNearestArgs* A) {
  memset(A, 0, sizeof(*A));
  batch_work_args(b, A);
  A->k = (uint32_t)k;
  A->out = out_dev;
  A->dist2_out = dist2_dev;
}

// The launch of a rig read, behind every check (n > 0): out_dev, dist2_dev and boxes_dev are device memory of n records each, the
// caller's or the handle's; dist2_dev and boxes_dev may be null.
static mgf_status batch_nearest_run(mgf_batch* b, int32_t k, int32_t* out_dev, float* dist2_dev, float* boxes_dev) {
  BatchRig<mgf_batch_zone>& R = b->zones;
  MGF_TRY(batch_push(b));
  MGF_TRY(batch_rig_up(b, R, "zone", 3, true));
  MGF_TRY(batch_cols_refresh(b, &b->q_launches));
  BatchNearestArgs A;
  batch_nearest_args(b, k, out_dev, dist2_dev, &A);
  A.items = reinterpret_cast<const uint4*>(R.dev.p);
  A.order = reinterpret_cast<const uint32_t*>(R.dev.p + R.off[2]);
  A.x = b->dm[mgf_batch::AX].p; A.q = b->dm[mgf_batch::AQ].p;
  A.rig = reinterpret_cast<const ZoneIn*>(R.dev.p + R.off[1]);
  A.boxes_out = boxes_dev;
  BatchItemSrc S;
  memset(&S, 0, sizeof(S));
  if (batch_part_queries(b)) MGF_TRY(batch_pq_nearest<kItemTable>(b, A, S, (unsigned)R.items.size(), batch_zone_lds(b)));  // (a body's box: the union of its parts')
  else k_batch_nearest<kItemTable><<<(unsigned)R.items.size(), kBatchBlock, batch_zone_lds(b), b->ctx->stream>>>(A, S);
  LAUNCH_CHECK();
  b->q_launches += MGF_BATCH_NEAREST_LAUNCHES;
  return MGF_OK;
}

// the refusals of both rig reads that need no device; *n: the zones of the rig
static mgf_status batch_nearest_read_args(const mgf_batch* b, int32_t k, const void* out, int64_t cap, size_t* n) {
  MGF_TRY(batch_rig_handle(b));
  MGF_TRY(nearest_k_check(k));
  MGF_TRY(batch_rig_cap(cap));
  *n = b->zones.recs.size();
  return batch_rig_fits(*n, cap, out != nullptr);
}

extern "C" mgf_status mgf_batch_read_zones_nearest(mgf_batch* b, int32_t k, int32_t* out, float* dist2_out, mgf_aabb* boxes_out, int64_t cap) {
  size_t n = 0;
  MGF_TRY(batch_nearest_read_args(b, k, out, cap, &n));
  MGF_TRY(batch_single_parts(b, "mgf_batch_read_zones_nearest"));
  MGF_TRY(ctx_bind(b->ctx));
  batch_call_begin(b);
  if (n == 0) return MGF_OK;
  hipStream_t s = b->ctx->stream;
  const size_t words = ((size_t)k + 1) * n, dwords = dist2_out ? (size_t)k * n : 0, bwords = boxes_out ? 6 * n : 0;
  MGF_TRY(b->z_out.ensure(words + dwords + bwords, s));  // records | distances | boxes: one download
  float* dist2_dev = dist2_out ? reinterpret_cast<float*>(b->z_out.p + words) : nullptr;
  float* boxes_dev = boxes_out ? reinterpret_cast<float*>(b->z_out.p + words + dwords) : nullptr;
  MGF_TRY(batch_nearest_run(b, k, b->z_out.p, dist2_dev, boxes_dev));
  if (!dwords && !bwords) {
    MGF_HIP_TRY(hipMemcpyAsync(out, b->z_out.p, 4 * words, hipMemcpyDeviceToHost, s));
    MGF_HIP_TRY(hipStreamSynchronize(s));
    return MGF_OK;
  }
  std::vector<int32_t> h(words + dwords + bwords);
  MGF_HIP_TRY(hipMemcpyAsync(h.data(), b->z_out.p, 4 * h.size(), hipMemcpyDeviceToHost, s));
  MGF_HIP_TRY(hipStreamSynchronize(s));
  memcpy(out, h.data(), 4 * words);
  if (dwords) memcpy(dist2_out, h.data() + words, 4 * dwords);
  if (bwords) memcpy(boxes_out, h.data() + words + dwords, 4 * bwords);
  return MGF_OK;
}

extern "C" mgf_status mgf_batch_read_zones_nearest_dev(mgf_batch* b, int32_t k, int32_t* out_dev, float* dist2_out_dev, mgf_aabb* boxes_out_dev,
                                                       int64_t cap) {
  size_t n = 0;
  MGF_TRY(batch_nearest_read_args(b, k, out_dev, cap, &n));
  MGF_TRY(batch_single_parts(b, "mgf_batch_read_zones_nearest_dev"));
  MGF_TRY(ctx_bind(b->ctx));
  const size_t out_bytes = 4 * ((size_t)k + 1) * n, dist2_bytes = 4 * (size_t)k * n;
  MGF_TRY(dev_span(b->ctx, out_dev, out_bytes, "out_dev"));
  MGF_TRY(dev_span(b->ctx, dist2_out_dev, dist2_bytes, "dist2_out_dev"));
  MGF_TRY(dev_span(b->ctx, boxes_out_dev, 24 * n, "boxes_out_dev"));
  const DevBytes arrays[3] = {{out_dev, out_bytes, "out_dev"}, {dist2_out_dev, dist2_bytes, "dist2_out_dev"}, {boxes_out_dev, 24 * n, "boxes_out_dev"}};
  MGF_TRY(dev_outputs_overlap(arrays, 3, 3));
  batch_call_begin(b);
  if (n == 0) return MGF_OK;
  return batch_nearest_run(b, k, out_dev, dist2_out_dev, reinterpret_cast<float*>(boxes_out_dev));
}

// The same kernel over boxes the caller computed on the device: the fixed layout of mgf_batch_overlap_first_dev, and that call's
// refusals in its order.
extern "C" mgf_status mgf_batch_overlap_nearest_dev(mgf_batch* b, const mgf_aabb* boxes_dev, int64_t n_in, const int32_t* ignore_body_dev, int32_t k,
                                                    int32_t* out_dev, float* dist2_out_dev) {
  MGF_TRY(batch_dev_args(b, n_in));
  if (n_in && (!boxes_dev || !out_dev)) return fail(MGF_ERR_INVALID, "NULL argument");
  MGF_TRY(nearest_k_check(k));
  static_assert(sizeof(mgf_aabb) == 24, "k_batch_nearest reads mgf_aabb as six words");
  const size_t n = (size_t)n_in;
  MGF_TRY(batch_single_parts(b, "mgf_batch_overlap_nearest_dev"));
  MGF_TRY(ctx_bind(b->ctx));
  if (n % b->K) return fail(MGF_ERR_INVALID, "n is a multiple of the number of worlds");
  const size_t out_bytes = 4 * ((size_t)k + 1) * n, dist2_bytes = 4 * (size_t)k * n;
  MGF_TRY(dev_span(b->ctx, boxes_dev, 24 * n, "boxes_dev"));
  MGF_TRY(dev_span(b->ctx, ignore_body_dev, 4 * n, "ignore_body_dev"));
  MGF_TRY(dev_span(b->ctx, out_dev, out_bytes, "out_dev"));
  MGF_TRY(dev_span(b->ctx, dist2_out_dev, dist2_bytes, "dist2_out_dev"));
  // (a workgroup reads its boxes while another has already written its records)
  const DevBytes arrays[4] = {{out_dev, out_bytes, "out_dev"}, {dist2_out_dev, dist2_bytes, "dist2_out_dev"}, {boxes_dev, 24 * n, "boxes_dev"},
                              {ignore_body_dev, 4 * n, "ignore_body_dev"}};
  MGF_TRY(dev_outputs_overlap(arrays, 4, 2, "an input array"));  // "out_dev overlaps dist2_out_dev", "dist2_out_dev overlaps an input array"
  batch_call_begin(b);
  if (n == 0) return MGF_OK;
  MGF_TRY(batch_push(b));
  MGF_TRY(batch_cols_refresh(b, &b->q_launches));
  BatchNearestArgs A;
  batch_nearest_args(b, k, out_dev, dist2_out_dev, &A);
  A.boxes = reinterpret_cast<const float*>(boxes_dev);
  A.ignore = ignore_body_dev;
  BatchItemSrc S;
  memset(&S, 0, sizeof(S));
  S.per = (uint32_t)(n / b->K);  // (n > 0 and a multiple of K: at least 1)
  const unsigned grid = (unsigned)((size_t)b->K * ((S.per + 255u) / 256u));
  if (batch_part_queries(b)) MGF_TRY(batch_pq_nearest<kItemFixed>(b, A, S, grid, batch_zone_lds(b)));
  else k_batch_nearest<kItemFixed><<<grid, kBatchBlock, batch_zone_lds(b), b->ctx->stream>>>(A, S);
  LAUNCH_CHECK();
  b->q_launches += MGF_BATCH_NEAREST_LAUNCHES;
  return MGF_OK;
}
