// mgf_batch_set_sensors, mgf_batch_sensor_count, mgf_batch_cast_sensors, mgf_batch_cast_sensors_dev: ray sensors fixed in the frame of
// a body, cast from the poses resident on the device (k_batch_sensor.h).  Part of the single translation unit mgf_hip.hip (included
// there, in order, behind host_batch_rig.inc); not compiled on its own.
//
// What the rig shares with the cameras' and the zones' is host_batch_rig.inc's: the prologue and the checks of a set call, the sort by
// world and the work items (batch_rig_plan), the upload - items | records | order | worlds, ONE copy (batch_rig_up) - and the pieces
// of what a cast refuses before it looks at a device.  A cast is then one launch - and the obstacle pass, and the collider gather behind
// a step - with no plan, no index array and, for the device form, no host wait and no copy between host and device.
// The order of mgf_batch_cast_sensors_dev is host_batch_query_dev.inc's: the refusals that need no device, the handle's own, EVERY
// device pointer looked up (dev_span), the overlap of the two outputs - and only then the first thing is enqueued.

extern "C" mgf_status mgf_batch_set_sensors(mgf_batch* b, const mgf_batch_sensor* s, int64_t n_in) {
  MGF_TRY(batch_rig_set_args(b, s, n_in));
  static_assert(sizeof(mgf_batch_sensor) == sizeof(SensorIn) && sizeof(mgf_batch_sensor) == 40, "the rig goes up as the caller's records");
  const size_t n = (size_t)n_in;
  for (size_t i = 0; i < n; ++i) MGF_TRY(batch_rig_ref_check(b, s[i].world, s[i].body, s[i].flags, "sensor"));
  batch_rig_plan(b, b->sensors, s, n);
  return MGF_OK;
}

extern "C" int64_t mgf_batch_sensor_count(const mgf_batch* b) { return b ? (int64_t)b->sensors.recs.size() : -1; }

// The launches of a cast, behind every check (n > 0): out_dev and parts_dev are device memory of n records each, the caller's or the
// handle's; parts_dev may be null.
static mgf_status batch_sensor_run(mgf_batch* b, int32_t kinds_mask, int32_t* out_dev, float* parts_dev) {
  BatchRig<mgf_batch_sensor>& R = b->sensors;
  const size_t n = R.recs.size();
  MGF_TRY(batch_push(b));
  MGF_TRY(batch_env_sync(b));
  MGF_TRY(batch_rig_up(b, R, "sensor", 4));
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
  A.items = reinterpret_cast<const uint4*>(R.dev.p);
  A.order = reinterpret_cast<const uint32_t*>(R.dev.p + R.off[2]);
  A.T = batch_terrains(b);
  A.mask = kinds_mask;
  A.out = out_dev;
  A.x = b->dm[mgf_batch::AX].p; A.q = b->dm[mgf_batch::AQ].p;
  A.rig = reinterpret_cast<const SensorIn*>(R.dev.p + R.off[1]);
  A.parts = parts_dev;
  if (batch_part_queries(b)) MGF_TRY(batch_pq_sensor(b, A, (unsigned)R.items.size()));  // (the body pass sees parts)
  else k_batch_sensor_ray<<<(unsigned)R.items.size(), kBatchBlock, batch_ray_lds(b), s>>>(A);
  LAUNCH_CHECK();
  b->q_launches += MGF_BATCH_SENSOR_LAUNCHES;
  if (!obstacles) return MGF_OK;
  return batch_ray_obstacles(b, reinterpret_cast<const int32_t*>(R.dev.p + R.off[3]), 0u, reinterpret_cast<const ParticleIn*>(parts_dev), n, out_dev);
}

// the refusals of both cast calls that need no device; *n: the sensors of the rig
static mgf_status batch_sensor_args(const mgf_batch* b, int32_t kinds_mask, const void* out, int64_t cap, size_t* n) {
  MGF_TRY(batch_rig_handle(b));
  MGF_TRY(batch_rig_cap(cap));
  MGF_TRY(query_mask_check(kinds_mask));
  *n = b->sensors.recs.size();
  return batch_rig_fits(*n, cap, out != nullptr);
}

extern "C" mgf_status mgf_batch_cast_sensors(mgf_batch* b, int32_t kinds_mask, mgf_ray_hit* out, mgf_particle* parts_out, int64_t cap) {
  size_t n = 0;
  MGF_TRY(batch_sensor_args(b, kinds_mask, out, cap, &n));
  MGF_TRY(batch_single_parts(b, "mgf_batch_cast_sensors"));
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
  MGF_TRY(batch_single_parts(b, "mgf_batch_cast_sensors_dev"));
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
