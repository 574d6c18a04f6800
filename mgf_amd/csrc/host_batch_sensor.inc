// mgf_batch_set_sensors, mgf_batch_sensor_count, mgf_batch_cast_sensors, mgf_batch_cast_sensors_dev: ray sensors fixed in the frame of
// a body, cast from the poses resident on the device (k_batch_sensor.h).  Part of the single translation unit mgf_hip.hip (included
// there, in order, behind host_batch_query_dev.inc); not compiled on its own.
//
// A rig is static: which body, where on it, which way, how far.  Everything that depends on the rig alone is done once, when it is set:
// the checks, the sort by world and the work items (BatchQueryPlan, host_batch_query.inc).  The rig goes up - items | records | order |
// worlds, ONE copy - before the first cast behind a change of the rig or of the batch's layout (mgf_batch_add_bodies: the rig names
// (world, body), a body's flat offset is w_off[world] + body on the device, and the check body < length is made again against the lengths
// that go up with it).  A cast is then one launch - and the obstacle pass, and the collider gather behind a step - with no plan, no
// index array and, for the device form, no host wait and no copy between host and device.
// The order of mgf_batch_cast_sensors_dev is host_batch_query_dev.inc's: the refusals that need no device, the handle's own, EVERY
// device pointer looked up (dev_span), the overlap of the two outputs - and only then the first thing is enqueued.

extern "C" mgf_status mgf_batch_set_sensors(mgf_batch* b, const mgf_batch_sensor* s, int64_t n_in) {
  MGF_TRY(batch_dev_args(b, n_in));
  if (n_in && !s) return fail(MGF_ERR_INVALID, "NULL argument");
  static_assert(sizeof(mgf_batch_sensor) == sizeof(SensorIn) && sizeof(mgf_batch_sensor) == 40, "the rig goes up as the caller's records");
  const size_t n = (size_t)n_in;
  for (size_t i = 0; i < n; ++i) {
    if (s[i].world < 0 || (uint32_t)s[i].world >= b->K) return fail(MGF_ERR_INVALID, "world index out of range: the rig was not changed");
    if (s[i].body < 0 || (uint32_t)s[i].body >= b->h_n[(size_t)s[i].world]) return fail(MGF_ERR_INVALID, "body index out of range: the rig was not changed");
    if (s[i].flags & ~MGF_SENSOR_IGNORE_SELF) return fail(MGF_ERR_INVALID, "a sensor's flags hold a bit beyond MGF_SENSOR_IGNORE_SELF: the rig was not changed");
  }
  // (no device is needed: a cast that was enqueued reads the device copy, which is replaced in stream order when the next cast puts the rig up)
  std::vector<int32_t> world(n);
  for (size_t i = 0; i < n; ++i) world[i] = s[i].world;
  const BatchQueryPlan plan(b->K, world.data(), n);
  b->s_rig.assign(s, s + n);
  b->s_items.resize(plan.n_items);
  b->s_order.resize(n);
  plan.fill(world.data(), n, b->s_items.data(), b->s_order.data());
  b->s_stale = true;
  return MGF_OK;
}

extern "C" int64_t mgf_batch_sensor_count(const mgf_batch* b) { return b ? (int64_t)b->s_rig.size() : -1; }

// the rig onto the device (n > 0): items | records | order | worlds, every section from a 16-byte boundary
static mgf_status batch_sensors_up(mgf_batch* b) {
  if (!b->s_stale) return MGF_OK;
  const size_t n = b->s_rig.size(), n_items = b->s_items.size();
  for (const mgf_batch_sensor& r : b->s_rig)
    if ((uint32_t)r.body >= b->h_n[(size_t)r.world]) return fail(MGF_ERR_INVALID, "internal error: a sensor names a body its world does not hold");
  const size_t w_rig = (40 * n + 15) / 16, w_idx = (4 * n + 15) / 16;
  const size_t o_rig = n_items, o_order = o_rig + w_rig, o_world = o_order + w_idx, total = o_world + w_idx;
  std::vector<float4> h(total);
  memcpy(h.data(), b->s_items.data(), 16 * n_items);
  memcpy(h.data() + o_rig, b->s_rig.data(), 40 * n);
  memcpy(h.data() + o_order, b->s_order.data(), 4 * n);
  int32_t* hw = reinterpret_cast<int32_t*>(h.data() + o_world);
  for (size_t i = 0; i < n; ++i) hw[i] = b->s_rig[i].world;
  MGF_TRY(b->s_dev.ensure(total, b->ctx->stream));
  MGF_TRY(h2d(b->ctx, b->s_dev.p, h.data(), total));
  b->s_o_rig = o_rig; b->s_o_order = o_order; b->s_o_world = o_world;
  b->s_stale = false;
  return MGF_OK;
}

// The launches of a cast, behind every check (n > 0): out_dev and parts_dev are device memory of n records each, the caller's or the
// handle's; parts_dev may be null.
static mgf_status batch_sensor_run(mgf_batch* b, int32_t kinds_mask, int32_t* out_dev, float* parts_dev) {
  const size_t n = b->s_rig.size();
  MGF_TRY(batch_push(b));
  MGF_TRY(batch_env_sync(b));
  MGF_TRY(batch_sensors_up(b));
  MGF_TRY(batch_cols_refresh(b, &b->q_launches));
  hipStream_t s = b->ctx->stream;
  const bool obstacles = (kinds_mask & MGF_QUERY_OBSTACLES) && b->o_worlds;  // as batch_query_run
  if (obstacles && !parts_dev) {  // the obstacle pass takes the particles up again
    MGF_TRY(b->s_parts.ensure(7 * n, s));
    parts_dev = b->s_parts.p;
  }
  uint32_t nmax = 0;
  for (uint32_t c : b->h_n) nmax = std::max(nmax, c);
  const uint32_t lds = 32u * nmax + 16u * kBatchQueryRed;
  BatchSensorArgs A;
  memset(&A, 0, sizeof(A));
  A.col0 = b->dm[mgf_batch::ACOL0].p; A.col1 = b->dm[mgf_batch::ACOL1].p; A.w_off = b->d_off.p;
  A.items = reinterpret_cast<const uint4*>(b->s_dev.p);
  A.order = reinterpret_cast<const uint32_t*>(b->s_dev.p + b->s_o_order);
  A.T = batch_terrains(b);
  A.mask = kinds_mask;
  A.out = out_dev;
  A.x = b->dm[mgf_batch::AX].p; A.q = b->dm[mgf_batch::AQ].p;
  A.rig = reinterpret_cast<const SensorIn*>(b->s_dev.p + b->s_o_rig);
  A.parts = parts_dev;
  k_batch_sensor_ray<<<(unsigned)b->s_items.size(), kBatchBlock, lds, s>>>(A);
  LAUNCH_CHECK();
  b->q_launches += MGF_BATCH_SENSOR_LAUNCHES;
  if (obstacles) {
    k_batch_query_ray_obstacles<<<batch_dev_blocks(n), kBatchBlock, 0, s>>>(batch_obstacles(b), b->t_desc.p, reinterpret_cast<const int32_t*>(b->s_dev.p + b->s_o_world),
                                                                           0u, reinterpret_cast<const ParticleIn*>(parts_dev), (uint32_t)n, out_dev);
    LAUNCH_CHECK();
    ++b->q_launches;
  }
  return MGF_OK;
}

// the refusals of both cast calls that need no device; *n: the sensors of the rig
static mgf_status batch_sensor_args(const mgf_batch* b, int32_t kinds_mask, const void* out, int64_t cap, size_t* n) {
  if (!b) return fail(MGF_ERR_INVALID, "batch is NULL");
  if (cap < 0) return fail(MGF_ERR_INVALID, "cap is negative");
  MGF_TRY(query_mask_check(kinds_mask));
  *n = b->s_rig.size();
  if ((int64_t)*n > cap) return fail(MGF_ERR_CAPACITY, "buffer too small");
  if (*n && !out) return fail(MGF_ERR_INVALID, "NULL argument");
  return MGF_OK;
}

extern "C" mgf_status mgf_batch_cast_sensors(mgf_batch* b, int32_t kinds_mask, mgf_ray_hit* out, mgf_particle* parts_out, int64_t cap) {
  size_t n = 0;
  MGF_TRY(batch_sensor_args(b, kinds_mask, out, cap, &n));
  MGF_TRY(ctx_bind(b->ctx));
  b->q_launches = 0; b->q_run_ms = 0.0f;
  if (n == 0) return MGF_OK;
  hipStream_t s = b->ctx->stream;
  MGF_TRY(b->q_out.ensure(7 * n, s));
  if (parts_out) MGF_TRY(b->s_parts.ensure(7 * n, s));
  MGF_TRY(batch_sensor_run(b, kinds_mask, b->q_out.p, parts_out ? b->s_parts.p : nullptr));
  MGF_HIP_TRY(hipMemcpyAsync(out, b->q_out.p, 28 * n, hipMemcpyDeviceToHost, s));
  if (parts_out) MGF_HIP_TRY(hipMemcpyAsync(parts_out, b->s_parts.p, 28 * n, hipMemcpyDeviceToHost, s));
  MGF_HIP_TRY(hipStreamSynchronize(s));
  return MGF_OK;
}

extern "C" mgf_status mgf_batch_cast_sensors_dev(mgf_batch* b, int32_t kinds_mask, mgf_ray_hit* out_dev, mgf_particle* parts_out_dev, int64_t cap) {
  size_t n = 0;
  MGF_TRY(batch_sensor_args(b, kinds_mask, out_dev, cap, &n));
  MGF_TRY(ctx_bind(b->ctx));
  MGF_TRY(dev_span(b->ctx, out_dev, 28 * n, "out_dev"));
  MGF_TRY(dev_span(b->ctx, parts_out_dev, 28 * n, "parts_out_dev"));
  // (the obstacle pass reads the particles again after the body pass wrote hits)
  if (dev_bytes_overlap(out_dev, 28 * n, parts_out_dev, 28 * n)) return fail(MGF_ERR_INVALID, "out_dev overlaps parts_out_dev");
  b->q_launches = 0; b->q_run_ms = 0.0f;
  if (n == 0) return MGF_OK;
  return batch_sensor_run(b, kinds_mask, reinterpret_cast<int32_t*>(out_dev), reinterpret_cast<float*>(parts_out_dev));
}
