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

// what a record of a rig - a sensor's, a camera's, a zone's - names: a world of the batch, a body of that world (or_world: or -1, the
// world itself - a zone's), no flag but the one defined
static mgf_status batch_rig_ref_check(const mgf_batch* b, int32_t world, int32_t body, int32_t flags, const char* what, bool or_world = false) {
  if (world < 0 || (uint32_t)world >= b->K) return fail(MGF_ERR_INVALID, "world index out of range: the rig was not changed");
  if (!(or_world && body == -1) && (body < 0 || (uint32_t)body >= b->h_n[(size_t)world]))
    return fail(MGF_ERR_INVALID, "body index out of range: the rig was not changed");
  if (flags & ~MGF_SENSOR_IGNORE_SELF) {
    set_error("a %s's flags hold a bit beyond MGF_SENSOR_IGNORE_SELF: the rig was not changed", what);
    return MGF_ERR_INVALID;
  }
  return MGF_OK;
}

extern "C" mgf_status mgf_batch_set_sensors(mgf_batch* b, const mgf_batch_sensor* s, int64_t n_in) {
  MGF_TRY(batch_dev_args(b, n_in));
  if (n_in && !s) return fail(MGF_ERR_INVALID, "NULL argument");
  static_assert(sizeof(mgf_batch_sensor) == sizeof(SensorIn) && sizeof(mgf_batch_sensor) == 40, "the rig goes up as the caller's records");
  const size_t n = (size_t)n_in;
  for (size_t i = 0; i < n; ++i) MGF_TRY(batch_rig_ref_check(b, s[i].world, s[i].body, s[i].flags, "sensor"));
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

// A rig onto the device: the sections one behind the other, every one from a 16-byte boundary, in ONE copy.  off[k]: where section k
// begins in `dev`, in words of 16 bytes.
struct RigSection { const void* p; size_t bytes; };
static mgf_status batch_rig_upload(mgf_batch* b, DBuf<float4>& dev, const RigSection* sec, size_t n_sec, size_t* off) {
  size_t total = 0;
  for (size_t k = 0; k < n_sec; ++k) { off[k] = total; total += (sec[k].bytes + 15) / 16; }
  std::vector<float4> h(total);
  for (size_t k = 0; k < n_sec; ++k)
    if (sec[k].bytes) memcpy(h.data() + off[k], sec[k].p, sec[k].bytes);
  MGF_TRY(dev.ensure(total, b->ctx->stream));
  return h2d(b->ctx, dev.p, h.data(), total);
}

// the rig onto the device (n > 0): items | records | order | worlds
static mgf_status batch_sensors_up(mgf_batch* b) {
  if (!b->s_stale) return MGF_OK;
  const size_t n = b->s_rig.size();
  std::vector<int32_t> world(n);
  for (size_t i = 0; i < n; ++i) {
    const mgf_batch_sensor& r = b->s_rig[i];
    if ((uint32_t)r.body >= b->h_n[(size_t)r.world]) return fail(MGF_ERR_INVALID, "internal error: a sensor names a body its world does not hold");
    world[i] = r.world;
  }
  const RigSection sec[4] = {{b->s_items.data(), 16 * b->s_items.size()}, {b->s_rig.data(), 40 * n}, {b->s_order.data(), 4 * n}, {world.data(), 4 * n}};
  size_t off[4];
  MGF_TRY(batch_rig_upload(b, b->s_dev, sec, 4, off));
  b->s_o_rig = off[1]; b->s_o_order = off[2]; b->s_o_world = off[3];
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
  const bool obstacles = batch_has_obstacles(b, kinds_mask);
  if (obstacles && !parts_dev) {  // the obstacle pass takes the particles up again
    MGF_TRY(b->s_parts.ensure(7 * n, s));
    parts_dev = b->s_parts.p;
  }
  BatchSensorArgs A;
  memset(&A, 0, sizeof(A));
  batch_work_args(b, &A);
  A.items = reinterpret_cast<const uint4*>(b->s_dev.p);
  A.order = reinterpret_cast<const uint32_t*>(b->s_dev.p + b->s_o_order);
  A.T = batch_terrains(b);
  A.mask = kinds_mask;
  A.out = out_dev;
  A.x = b->dm[mgf_batch::AX].p; A.q = b->dm[mgf_batch::AQ].p;
  A.rig = reinterpret_cast<const SensorIn*>(b->s_dev.p + b->s_o_rig);
  A.parts = parts_dev;
  k_batch_sensor_ray<<<(unsigned)b->s_items.size(), kBatchBlock, batch_ray_lds(b), s>>>(A);
  LAUNCH_CHECK();
  b->q_launches += MGF_BATCH_SENSOR_LAUNCHES;
  if (!obstacles) return MGF_OK;
  return batch_ray_obstacles(b, reinterpret_cast<const int32_t*>(b->s_dev.p + b->s_o_world), 0u, reinterpret_cast<const ParticleIn*>(parts_dev), n, out_dev);
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
  batch_call_begin(b);
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
  const DevBytes arrays[2] = {{out_dev, 28 * n, "out_dev"}, {parts_out_dev, 28 * n, "parts_out_dev"}};
  MGF_TRY(dev_outputs_overlap(arrays, 2, 2));
  batch_call_begin(b);
  if (n == 0) return MGF_OK;
  return batch_sensor_run(b, kinds_mask, reinterpret_cast<int32_t*>(out_dev), reinterpret_cast<float*>(parts_out_dev));
}
