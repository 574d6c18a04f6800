// mgf_batch_rollout_observe, mgf_batch_rollout_observe_dev: a rollout (host_batch_rollout.inc) that can also write, behind tick t, row t
// of the contact sensors' reports and row t of the ray sensors' answers - the loop  [apply_springs_dev(dt)] | actuate_dev(u[t]) | step(1) |
// gather_state_dev(row t) | [read_touches_dev(row t)] | cast_sensors_dev(sensor_mask, row t)  in one call with the step's one host wait
// per pass (k_batch_scan.h).  Part of the single translation unit mgf_hip.hip (included there, in order, behind host_batch_trace.inc);
// not compiled on its own.
//
// Nothing of a rollout is written again here: the refusals are batch_rollout_args' with the sensor trace's slotted in behind the touch
// trace's at every stage, the core is batch_rollout_run with both traces handed on, and the launches -
// MGF_BATCH_ROLLOUT_SENSOR_LAUNCHES_PER_TICK = 2 a tick a pass, behind the touch trace's, counted in "rollout_launches" - are the
// train's (batch_step_run, host_batch.inc), which looks the kernels' view up again for every pass.  The rig is the ray sensors'
// (mgf_batch_set_sensors), its upload host_batch_rig.inc's, the dynamic LDS batch_ray_lds', the scratch the handle's q_out and s_parts.
// No collider gather: the cast stages from bpk.  "query_launches", "drive_launches" and cols_stale are not touched.
// traces == NULL: mgf_batch_rollout / _rollout_dev.  No sensor trace: mgf_batch_rollout_touches / _touches_dev with the struct's touch
// fields; no touch trace either: mgf_batch_rollout again.  Launch for launch.
// The order of both calls: the refusals that need no handle, the handle's own, (device form) EVERY device pointer looked up for its
// n_ticks-fold extent and the outputs held against each other and against the inputs - and only then the first thing is enqueued.

// the refusals of both forms, in the header's order; no device is touched and nothing is enqueued.  traces == NULL: *tt and *ts come back null
static mgf_status batch_scan_args(const mgf_batch* b, int32_t iters, int64_t n_ticks, const float* u, int64_t n_act, int32_t mode, const int32_t* body,
                                  int64_t m, const mgf_rollout_traces* traces, RolloutBytes* bytes, RolloutTouch* touch, RolloutScan* scan,
                                  const RolloutTouch** tt, const RolloutScan** ts) {
  *tt = nullptr; *ts = nullptr;
  if (!traces) return batch_rollout_args(b, iters, n_ticks, u, n_act, mode, body, m, bytes);
  static_assert(sizeof(mgf_rollout_traces) == 64, "the struct is part of the C-ABI");
  touch->out = traces->touch; touch->n = traces->n_touch; touch->format = traces->touch_format; touch->lax = true;
  scan->out = traces->sensor; scan->n = traces->n_sensor; scan->format = traces->sensor_format; scan->mask = traces->sensor_mask;
  scan->reserved = false;
  for (int k = 0; k < 5; ++k) scan->reserved = scan->reserved || traces->reserved[k] != 0;
  MGF_TRY(batch_rollout_args(b, iters, n_ticks, u, n_act, mode, body, m, bytes, touch, scan));
  // the cast reads the shapes of bodies, and TickBodies' staging reads them as one collider a body: refused on part storage, "part_queries" or not
  if (!scan->off()) MGF_TRY(batch_single_parts(b, "mgf_batch_rollout_observe / mgf_batch_rollout_observe_dev", false));
  if (!touch->off()) *tt = touch;
  if (!scan->off()) *ts = scan;
  return MGF_OK;
}

extern "C" mgf_status mgf_batch_rollout_observe_dev(mgf_batch* b, float dt, int32_t iters, int64_t n_ticks, const float* u_dev, int64_t n_act, int32_t mode,
                                                    const int32_t* body_dev, int64_t m, float* x_dev, float* q_dev, float* v_dev, float* omega_dev,
                                                    const mgf_rollout_traces* traces, mgf_step_stats* stats) {
  RolloutBytes n;
  RolloutTouch touch;
  RolloutScan scan;
  const RolloutTouch* tt;
  const RolloutScan* ts;
  MGF_TRY(batch_scan_args(b, iters, n_ticks, u_dev, n_act, mode, body_dev, m, traces, &n, &touch, &scan, &tt, &ts));
  void* touch_dev = tt ? tt->out : nullptr;
  void* sensor_dev = ts ? ts->out : nullptr;
  MGF_TRY(ctx_bind(b->ctx));
  MGF_TRY(dev_span(b->ctx, u_dev, n.u, "u_dev"));
  MGF_TRY(dev_span(b->ctx, body_dev, n.body, "body_dev"));
  MGF_TRY(dev_span(b->ctx, x_dev, n.out[0], "x_dev"));
  MGF_TRY(dev_span(b->ctx, q_dev, n.out[1], "q_dev"));
  MGF_TRY(dev_span(b->ctx, v_dev, n.out[2], "v_dev"));
  MGF_TRY(dev_span(b->ctx, omega_dev, n.out[3], "omega_dev"));
  MGF_TRY(dev_span(b->ctx, touch_dev, n.touch, "traces->touch"));
  MGF_TRY(dev_span(b->ctx, sensor_dev, n.sensor, "traces->sensor"));
  const DevBytes arrays[8] = {{x_dev, n.out[0], "x_dev"}, {q_dev, n.out[1], "q_dev"}, {v_dev, n.out[2], "v_dev"}, {omega_dev, n.out[3], "omega_dev"},
                              {touch_dev, n.touch, "traces->touch"}, {sensor_dev, n.sensor, "traces->sensor"}, {u_dev, n.u, "u_dev"}, {body_dev, n.body, "body_dev"}};
  MGF_TRY(dev_outputs_overlap(arrays, 8, 6));
  return batch_rollout_run(b, dt, iters, n_ticks, u_dev, n_act, mode, body_dev, m, x_dev, q_dev, v_dev, omega_dev, stats, tt, ts);
}

// The host form: one upload (u | body), the device core, one download (x | q | v | omega | touch | sensor).  As in mgf_batch_rollout the
// handle's buffer is cleared, not filled from the caller's rows: a row of an index outside the batch comes back as zeros.  (Every report
// and every answer is written: every world completes every tick of a call that returns MGF_OK.)
extern "C" mgf_status mgf_batch_rollout_observe(mgf_batch* b, float dt, int32_t iters, int64_t n_ticks, const float* u, int64_t n_act, int32_t mode,
                                                const int32_t* body, int64_t m, float* x, float* q, float* v, float* omega, const mgf_rollout_traces* traces,
                                                mgf_step_stats* stats) {
  RolloutBytes n;
  RolloutTouch touch;
  RolloutScan scan;
  const RolloutTouch* tt;
  const RolloutScan* ts;
  MGF_TRY(batch_scan_args(b, iters, n_ticks, u, n_act, mode, body, m, traces, &n, &touch, &scan, &tt, &ts));
  MGF_TRY(ctx_bind(b->ctx));
  hipStream_t s = b->ctx->stream;
  // the handle's buffer, every section from a 16-byte boundary: u | body | x | q | v | omega | touch | sensor
  const void* host_in[2] = {u, body};
  void* host_out[6] = {x, q, v, omega, tt ? tt->out : nullptr, ts ? ts->out : nullptr};
  const size_t bytes[8] = {n.u, body ? n.body : 0, n.out[0], n.out[1], n.out[2], n.out[3], n.touch, n.sensor};
  size_t off[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = 0; k < 8; ++k) off[k + 1] = off[k] + ((k < 2 ? host_in[k] != nullptr : host_out[k - 2] != nullptr) ? (bytes[k] + 15) / 16 : 0);
  void* dev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  std::vector<float4> stage;
  if (off[8]) {
    MGF_TRY(b->q_in.ensure(off[8], s));
    for (int k = 0; k < 8; ++k)
      if (off[k + 1] > off[k]) dev[k] = b->q_in.p + off[k];
    if (off[2]) {
      stage.resize(off[2]);
      for (int k = 0; k < 2; ++k)
        if (dev[k]) memcpy(stage.data() + off[k], host_in[k], bytes[k]);
      MGF_TRY(h2d(b->ctx, b->q_in.p, stage.data(), off[2]));
    }
    if (off[8] > off[2]) MGF_HIP_TRY(hipMemsetAsync(b->q_in.p + off[2], 0, 16 * (off[8] - off[2]), s));
  }
  if (tt) touch.out = dev[6];
  if (ts) scan.out = dev[7];
  MGF_TRY(batch_rollout_run(b, dt, iters, n_ticks, static_cast<const float*>(dev[0]), n_act, mode, static_cast<const int32_t*>(dev[1]), m, static_cast<float*>(dev[2]),
                            static_cast<float*>(dev[3]), static_cast<float*>(dev[4]), static_cast<float*>(dev[5]), stats, tt, ts));
  if (off[8] > off[2]) {
    stage.resize(off[8] - off[2]);
    MGF_TRY(d2h(b->ctx, stage.data(), b->q_in.p + off[2], stage.size()));
    for (int k = 2; k < 8; ++k)
      if (dev[k]) memcpy(host_out[k - 2], stage.data() + (off[k] - off[2]), bytes[k]);
  }
  return MGF_OK;
}
