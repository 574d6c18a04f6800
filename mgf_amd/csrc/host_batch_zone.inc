// mgf_batch_set_zones, mgf_batch_zone_count, mgf_batch_read_zones, mgf_batch_read_zones_dev, mgf_batch_overlap_first_dev: box zones -
// per box the count and the first k bodies, a record of fixed width - answered from the poses and colliders resident on the device
// (k_batch_zone.h).  Part of the single translation unit mgf_hip.hip (included there, in order, behind host_batch_camera.inc); not
// compiled on its own.
//
// mgf_batch_overlap_aabb_many answers in CSR form: its caller must know the total before it can size the lists, and that costs a host
// wait.  A record of 1 + k words per box needs no total, so count and fill are one pass and nothing waits.
// What the rig shares with the sensors' and the cameras' is host_batch_rig.inc's: the prologue and the world / body / flags check of the
// set call, the sort by world and the work items (batch_rig_plan), the upload - items | records | order, ONE copy (batch_rig_up) - and
// the pieces of what a read refuses before it looks at a device.  A read is then MGF_BATCH_ZONE_LAUNCHES = 1 launch - and the collider
// gather behind a step - with no plan, no index array and, for the device form, no host wait and no copy between host and device.
// The order of both device-pointer calls is host_batch_query_dev.inc's: the refusals that need no device, the handle's own, EVERY device
// pointer looked up (dev_span), the overlap of what is written with everything else - and only then the first thing is enqueued.

extern "C" mgf_status mgf_batch_set_zones(mgf_batch* b, const mgf_batch_zone* z, int64_t n_in) {
  MGF_TRY(batch_rig_set_args(b, z, n_in));
  static_assert(sizeof(mgf_batch_zone) == sizeof(ZoneIn) && sizeof(mgf_batch_zone) == 40, "the rig goes up as the caller's records");
  const size_t n = (size_t)n_in;
  for (size_t i = 0; i < n; ++i) {
    MGF_TRY(batch_rig_ref_check(b, z[i].world, z[i].body, z[i].flags, "zone", true));
    if (z[i].body < 0 && (z[i].flags & MGF_SENSOR_IGNORE_SELF))
      return fail(MGF_ERR_INVALID, "a zone fixed in the world (body = -1) has no body of its own to ignore: the rig was not changed");
    if (z[i].reserved != 0) return fail(MGF_ERR_INVALID, "a zone's reserved word is not 0: the rig was not changed");
  }
  batch_rig_plan(b, b->zones, z, n);
  return MGF_OK;
}

extern "C" int64_t mgf_batch_zone_count(const mgf_batch* b) { return b ? (int64_t)b->zones.recs.size() : -1; }

// what both launches share: the colliders, the offsets, k and where the records go
static void batch_zone_args(const mgf_batch* b, int32_t k, int32_t* out_dev, BatchZoneArgs* A) {
  memset(A, 0, sizeof(*A));
  batch_work_args(b, A);
  A->k = (uint32_t)k;
  A->out = out_dev;
}
static uint32_t batch_zone_lds(const mgf_batch* b) { return 32u * batch_nmax(b); }  // (at most 32 KB)

// The launch of a read, behind every check (n > 0): out_dev and boxes_dev are device memory of n records each, the caller's or the
// handle's; boxes_dev may be null.
static mgf_status batch_zone_run(mgf_batch* b, int32_t k, int32_t* out_dev, float* boxes_dev) {
  BatchRig<mgf_batch_zone>& R = b->zones;
  MGF_TRY(batch_push(b));
  MGF_TRY(batch_rig_up(b, R, "zone", 3, true));
  MGF_TRY(batch_cols_refresh(b, &b->q_launches));
  BatchZoneArgs A;
  batch_zone_args(b, k, out_dev, &A);
  A.items = reinterpret_cast<const uint4*>(R.dev.p);
  A.order = reinterpret_cast<const uint32_t*>(R.dev.p + R.off[2]);
  A.x = b->dm[mgf_batch::AX].p; A.q = b->dm[mgf_batch::AQ].p;
  A.rig = reinterpret_cast<const ZoneIn*>(R.dev.p + R.off[1]);
  A.boxes_out = boxes_dev;
  BatchItemSrc S;
  memset(&S, 0, sizeof(S));
  if (batch_part_queries(b)) MGF_TRY(batch_pq_zone<kItemTable>(b, A, S, (unsigned)R.items.size(), batch_zone_lds(b)));  // (a body's box: the union of its parts')
  else k_batch_zone_first<kItemTable><<<(unsigned)R.items.size(), kBatchBlock, batch_zone_lds(b), b->ctx->stream>>>(A, S);
  LAUNCH_CHECK();
  b->q_launches += MGF_BATCH_ZONE_LAUNCHES;
  return MGF_OK;
}

static mgf_status zone_k_check(int32_t k) {
  if (k < 0 || k > MGF_BATCH_MAX_BODIES) return fail(MGF_ERR_INVALID, "k is outside [0, MGF_BATCH_MAX_BODIES]");
  return MGF_OK;
}

// the refusals of both read calls that need no device; *n: the zones of the rig
static mgf_status batch_zone_read_args(const mgf_batch* b, int32_t k, const void* out, int64_t cap, size_t* n) {
  MGF_TRY(batch_rig_handle(b));
  MGF_TRY(zone_k_check(k));
  MGF_TRY(batch_rig_cap(cap));
  *n = b->zones.recs.size();
  return batch_rig_fits(*n, cap, out != nullptr);
}

extern "C" mgf_status mgf_batch_read_zones(mgf_batch* b, int32_t k, int32_t* out, mgf_aabb* boxes_out, int64_t cap) {
  size_t n = 0;
  MGF_TRY(batch_zone_read_args(b, k, out, cap, &n));
  MGF_TRY(batch_single_parts(b, "mgf_batch_read_zones"));
  MGF_TRY(ctx_bind(b->ctx));
  batch_call_begin(b);
  if (n == 0) return MGF_OK;
  hipStream_t s = b->ctx->stream;
  const size_t words = ((size_t)k + 1) * n;
  MGF_TRY(b->z_out.ensure(words + (boxes_out ? 6 * n : 0), s));  // records | boxes: one download
  float* boxes_dev = boxes_out ? reinterpret_cast<float*>(b->z_out.p + words) : nullptr;
  MGF_TRY(batch_zone_run(b, k, b->z_out.p, boxes_dev));
  if (!boxes_out) {
    MGF_HIP_TRY(hipMemcpyAsync(out, b->z_out.p, 4 * words, hipMemcpyDeviceToHost, s));
    MGF_HIP_TRY(hipStreamSynchronize(s));
    return MGF_OK;
  }
  std::vector<int32_t> h(words + 6 * n);
  MGF_HIP_TRY(hipMemcpyAsync(h.data(), b->z_out.p, 4 * h.size(), hipMemcpyDeviceToHost, s));
  MGF_HIP_TRY(hipStreamSynchronize(s));
  memcpy(out, h.data(), 4 * words);
  memcpy(boxes_out, h.data() + words, 24 * n);
  return MGF_OK;
}

extern "C" mgf_status mgf_batch_read_zones_dev(mgf_batch* b, int32_t k, int32_t* out_dev, mgf_aabb* boxes_out_dev, int64_t cap) {
  size_t n = 0;
  MGF_TRY(batch_zone_read_args(b, k, out_dev, cap, &n));
  MGF_TRY(batch_single_parts(b, "mgf_batch_read_zones_dev"));
  MGF_TRY(ctx_bind(b->ctx));
  const size_t out_bytes = 4 * ((size_t)k + 1) * n;
  MGF_TRY(dev_span(b->ctx, out_dev, out_bytes, "out_dev"));
  MGF_TRY(dev_span(b->ctx, boxes_out_dev, 24 * n, "boxes_out_dev"));
  const DevBytes arrays[2] = {{out_dev, out_bytes, "out_dev"}, {boxes_out_dev, 24 * n, "boxes_out_dev"}};
  MGF_TRY(dev_outputs_overlap(arrays, 2, 2));
  batch_call_begin(b);
  if (n == 0) return MGF_OK;
  return batch_zone_run(b, k, out_dev, reinterpret_cast<float*>(boxes_out_dev));
}

// The same kernel over boxes the caller computed on the device: the fixed layout of mgf_batch_raycast_many_dev with world_dev == NULL
// (a work item follows from the workgroup's index: no table, no order, nothing uploaded), and that call's refusals in its order.
extern "C" mgf_status mgf_batch_overlap_first_dev(mgf_batch* b, const mgf_aabb* boxes_dev, int64_t n_in, const int32_t* ignore_body_dev, int32_t k,
                                                  int32_t* out_dev) {
  MGF_TRY(batch_dev_args(b, n_in));
  if (n_in && (!boxes_dev || !out_dev)) return fail(MGF_ERR_INVALID, "NULL argument");
  MGF_TRY(zone_k_check(k));
  static_assert(sizeof(mgf_aabb) == 24, "k_batch_zone_first reads mgf_aabb as six words");
  const size_t n = (size_t)n_in;
  MGF_TRY(batch_single_parts(b, "mgf_batch_overlap_first_dev"));
  MGF_TRY(ctx_bind(b->ctx));
  if (n % b->K) return fail(MGF_ERR_INVALID, "n is a multiple of the number of worlds");
  const size_t out_bytes = 4 * ((size_t)k + 1) * n;
  MGF_TRY(dev_span(b->ctx, boxes_dev, 24 * n, "boxes_dev"));
  MGF_TRY(dev_span(b->ctx, ignore_body_dev, 4 * n, "ignore_body_dev"));
  MGF_TRY(dev_span(b->ctx, out_dev, out_bytes, "out_dev"));
  // (a workgroup reads its boxes while another has already written its records)
  const DevBytes arrays[3] = {{out_dev, out_bytes, "out_dev"}, {boxes_dev, 24 * n, "boxes_dev"}, {ignore_body_dev, 4 * n, "ignore_body_dev"}};
  MGF_TRY(dev_outputs_overlap(arrays, 3, 1, "an input array"));  // "out_dev overlaps an input array"
  batch_call_begin(b);
  if (n == 0) return MGF_OK;
  MGF_TRY(batch_push(b));
  MGF_TRY(batch_cols_refresh(b, &b->q_launches));
  BatchZoneArgs A;
  batch_zone_args(b, k, out_dev, &A);
  A.boxes = reinterpret_cast<const float*>(boxes_dev);
  A.ignore = ignore_body_dev;
  BatchItemSrc S;
  memset(&S, 0, sizeof(S));
  S.per = (uint32_t)(n / b->K);  // (n > 0 and a multiple of K: at least 1)
  const unsigned grid = (unsigned)((size_t)b->K * ((S.per + 255u) / 256u));
  if (batch_part_queries(b)) MGF_TRY(batch_pq_zone<kItemFixed>(b, A, S, grid, batch_zone_lds(b)));
  else k_batch_zone_first<kItemFixed><<<grid, kBatchBlock, batch_zone_lds(b), b->ctx->stream>>>(A, S);
  LAUNCH_CHECK();
  b->q_launches += MGF_BATCH_ZONE_LAUNCHES;
  return MGF_OK;
}
