// mgf_batch_set_cameras, mgf_batch_camera_count, mgf_batch_camera_pixels, mgf_batch_cast_cameras, mgf_batch_cast_cameras_dev: depth
// cameras fixed in the frame of a body, cast from the poses resident on the device (k_batch_camera.h).  Part of the single translation
// unit mgf_hip.hip (included there, in order, behind host_batch_sensor.inc); not compiled on its own.
//
// A rig is static, and an image follows from its camera's record alone: what goes up is the records (64 bytes a camera) and the tile
// table (16 bytes a tile of kCamTileW x kCamTileH pixels) - tiles | records, ONE copy - before the first cast behind a change of the
// rig or of the batch's layout (mgf_batch_add_bodies: the rig names (world, body), as the sensors' does).  No record per pixel exists on
// the host, and none on the device but what a cast is asked to write.  A cast is then one launch - and the obstacle pass with the depth
// pass behind it, and the collider gather behind a step - with no plan and, for the device form, no host wait and no copy between host
// and device.  What the rig shares with the sensors' and the zones' is host_batch_rig.inc's: the prologue and the world / body / flags
// check of the set call, the upload (batch_rig_up) and the pieces of what a cast refuses before it looks at a device; its work items are
// its tiles, built here, and it has no order.
// The order of mgf_batch_cast_cameras_dev is host_batch_sensor.inc's: the refusals that need no device, the handle's own, EVERY device
// pointer looked up (dev_span), the overlap of the outputs pair by pair - depth with hits, depth with particles, hits with particles -
// and only then the first thing is enqueued.

static bool camera_finite3(const mgf_vec3& v) { return std::isfinite(v.x) && std::isfinite(v.y) && std::isfinite(v.z); }

extern "C" mgf_status mgf_batch_set_cameras(mgf_batch* b, const mgf_batch_camera* cams, int64_t n_in) {
  MGF_TRY(batch_rig_set_args(b, cams, n_in));
  static_assert(sizeof(mgf_batch_camera) == sizeof(CameraIn) && sizeof(mgf_batch_camera) == 64, "the rig goes up as the caller's records");
  const size_t n = (size_t)n_in;
  uint64_t pixels = 0, n_tiles = 0;
  for (size_t i = 0; i < n; ++i) {
    const mgf_batch_camera& c = cams[i];
    MGF_TRY(batch_rig_ref_check(b, c.world, c.body, c.flags, "camera"));
    if (c.reserved != 0) return fail(MGF_ERR_INVALID, "a camera's reserved word is not 0: the rig was not changed");
    if (c.width < 1 || c.width > MGF_CAMERA_MAX_SIDE || c.height < 1 || c.height > MGF_CAMERA_MAX_SIDE)
      return fail(MGF_ERR_INVALID, "a camera's width or height is outside [1, 4096]: the rig was not changed");
    if (!camera_finite3(c.p) || !std::isfinite(c.r.s) || !std::isfinite(c.r.x) || !std::isfinite(c.r.y) || !std::isfinite(c.r.z) || !std::isfinite(c.tan_x) ||
        !std::isfinite(c.tan_y))
      return fail(MGF_ERR_INVALID, "a camera's p, r, tan_x or tan_y is not finite: the rig was not changed");
    if (!(c.far > 0.0f)) return fail(MGF_ERR_INVALID, "a camera's far is NaN or not above 0: the rig was not changed");
    pixels += (uint64_t)c.width * (uint64_t)c.height;
    if (pixels > (uint64_t)INT32_MAX) return fail(MGF_ERR_INVALID, "more than INT32_MAX pixels: the rig was not changed");
    n_tiles += (uint64_t)((c.width + kCamTileW - 1) / kCamTileW) * (uint64_t)((c.height + kCamTileH - 1) / kCamTileH);
  }
  // (no device is needed: a cast that was enqueued reads the device copy, which is replaced in stream order when the next cast puts the rig up)
  std::vector<uint4> tiles;
  tiles.reserve((size_t)n_tiles);
  uint32_t first = 0;
  for (size_t i = 0; i < n; ++i) {
    for (uint32_t y0 = 0; y0 < (uint32_t)cams[i].height; y0 += kCamTileH)
      for (uint32_t x0 = 0; x0 < (uint32_t)cams[i].width; x0 += kCamTileW) tiles.push_back(make_uint4((uint32_t)i, first, x0 | (y0 << 16), 0u));
    first += (uint32_t)cams[i].width * (uint32_t)cams[i].height;
  }
  b->cameras.recs.assign(cams, cams + n);
  b->cameras.items.swap(tiles);
  b->c_pixels = (size_t)pixels;
  b->cameras.stale = true;
  return MGF_OK;
}

extern "C" int64_t mgf_batch_camera_count(const mgf_batch* b) { return b ? (int64_t)b->cameras.recs.size() : -1; }
extern "C" int64_t mgf_batch_camera_pixels(const mgf_batch* b) { return b ? (int64_t)b->c_pixels : -1; }

static uint32_t batch_camera_lds(const mgf_batch* b) { return 36u * batch_nmax(b) + 16u; }

// The launches of a cast, behind every check (pixels > 0): device memory of one record a pixel each, the caller's or the handle's; each
// may be null, but not depth_dev and out_dev both.
static mgf_status batch_camera_run(mgf_batch* b, int32_t kinds_mask, float* depth_dev, int32_t* out_dev, float* parts_dev) {
  BatchRig<mgf_batch_camera>& R = b->cameras;
  const size_t n = b->c_pixels;
  MGF_TRY(batch_push(b));
  MGF_TRY(batch_env_sync(b));
  MGF_TRY(batch_rig_up(b, R, "camera", 2));  // tiles | records
  MGF_TRY(batch_cols_refresh(b, &b->q_launches));
  hipStream_t s = b->ctx->stream;
  const bool obstacles = batch_has_obstacles(b, kinds_mask);
  if (obstacles) {  // the obstacle pass takes the particles, the records and the worlds up again
    if (!parts_dev) { MGF_TRY(b->c_parts.ensure(7 * n, s)); parts_dev = b->c_parts.p; }
    if (!out_dev) { MGF_TRY(b->q_out.ensure(7 * n, s)); out_dev = b->q_out.p; }
    MGF_TRY(b->c_world.ensure(n, s));
  }
  BatchCameraArgs A;
  memset(&A, 0, sizeof(A));
  A.col0 = b->dm[mgf_batch::ACOL0].p; A.col1 = b->dm[mgf_batch::ACOL1].p; A.w_off = b->d_off.p;
  A.T = batch_terrains(b);
  A.x = b->dm[mgf_batch::AX].p; A.q = b->dm[mgf_batch::AQ].p;
  A.tiles = reinterpret_cast<const uint4*>(R.dev.p);
  A.cams = reinterpret_cast<const CameraIn*>(R.dev.p + R.off[1]);
  A.mask = kinds_mask;
  A.depth = obstacles ? nullptr : depth_dev;
  A.out = out_dev;
  A.parts = parts_dev;
  A.world = obstacles ? b->c_world.p : nullptr;
  k_batch_camera_tile<<<(unsigned)R.items.size(), kBatchBlock, batch_camera_lds(b), s>>>(A);
  LAUNCH_CHECK();
  b->q_launches += MGF_BATCH_CAMERA_LAUNCHES;
  if (obstacles) {
    MGF_TRY(batch_ray_obstacles(b, b->c_world.p, 0u, reinterpret_cast<const ParticleIn*>(parts_dev), n, out_dev));
    if (depth_dev) {  // (hits alone: the records are final as they stand)
      k_batch_camera_depth<<<batch_dev_blocks(n), kBatchBlock, 0, s>>>(out_dev, parts_dev, (uint32_t)n, depth_dev);
      LAUNCH_CHECK();
      ++b->q_launches;
    }
  }
  return MGF_OK;
}

// the refusals of both cast calls that need no device; *n: the pixels of the rig
static mgf_status batch_camera_args(const mgf_batch* b, int32_t kinds_mask, const void* depth, const void* hits, int64_t cap, size_t* n) {
  MGF_TRY(batch_rig_handle(b));
  MGF_TRY(batch_rig_cap(cap));
  MGF_TRY(query_mask_check(kinds_mask));
  *n = b->c_pixels;
  return batch_rig_fits(*n, cap, depth || hits, "NULL argument: depth and hits are both NULL");
}

extern "C" mgf_status mgf_batch_cast_cameras(mgf_batch* b, int32_t kinds_mask, float* depth, mgf_ray_hit* hits, mgf_particle* parts_out, int64_t cap) {
  size_t n = 0;
  MGF_TRY(batch_camera_args(b, kinds_mask, depth, hits, cap, &n));
  MGF_TRY(batch_single_parts(b, "mgf_batch_cast_cameras", false));
  MGF_TRY(ctx_bind(b->ctx));
  batch_call_begin(b);
  if (n == 0) return MGF_OK;
  hipStream_t s = b->ctx->stream;
  if (depth) MGF_TRY(b->c_depth.ensure(n, s));
  if (hits) MGF_TRY(b->q_out.ensure(7 * n, s));
  if (parts_out) MGF_TRY(b->c_parts.ensure(7 * n, s));
  MGF_TRY(batch_camera_run(b, kinds_mask, depth ? b->c_depth.p : nullptr, hits ? b->q_out.p : nullptr, parts_out ? b->c_parts.p : nullptr));
  if (depth) MGF_HIP_TRY(hipMemcpyAsync(depth, b->c_depth.p, 4 * n, hipMemcpyDeviceToHost, s));
  if (hits) MGF_HIP_TRY(hipMemcpyAsync(hits, b->q_out.p, 28 * n, hipMemcpyDeviceToHost, s));
  if (parts_out) MGF_HIP_TRY(hipMemcpyAsync(parts_out, b->c_parts.p, 28 * n, hipMemcpyDeviceToHost, s));
  MGF_HIP_TRY(hipStreamSynchronize(s));
  return MGF_OK;
}

extern "C" mgf_status mgf_batch_cast_cameras_dev(mgf_batch* b, int32_t kinds_mask, float* depth_dev, mgf_ray_hit* hits_dev, mgf_particle* parts_out_dev,
                                                 int64_t cap) {
  size_t n = 0;
  MGF_TRY(batch_camera_args(b, kinds_mask, depth_dev, hits_dev, cap, &n));
  MGF_TRY(batch_single_parts(b, "mgf_batch_cast_cameras_dev", false));
  MGF_TRY(ctx_bind(b->ctx));
  MGF_TRY(dev_span(b->ctx, depth_dev, 4 * n, "depth_dev"));
  MGF_TRY(dev_span(b->ctx, hits_dev, 28 * n, "hits_dev"));
  MGF_TRY(dev_span(b->ctx, parts_out_dev, 28 * n, "parts_out_dev"));
  // (the obstacle pass reads the particles again after the tile pass wrote hits, and the depth pass reads both)
  const DevBytes arrays[3] = {{depth_dev, 4 * n, "depth_dev"}, {hits_dev, 28 * n, "hits_dev"}, {parts_out_dev, 28 * n, "parts_out_dev"}};
  MGF_TRY(dev_outputs_overlap(arrays, 3, 3));
  batch_call_begin(b);
  if (n == 0) return MGF_OK;
  return batch_camera_run(b, kinds_mask, depth_dev, reinterpret_cast<int32_t*>(hits_dev), reinterpret_cast<float*>(parts_out_dev));
}
