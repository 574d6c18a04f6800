// mgf_batch_rollout_touches, mgf_batch_rollout_touches_dev: a rollout (host_batch_rollout.inc) that also writes row t of the contact
// sensors' reports behind tick t - the loop  [apply_springs_dev(dt)] | actuate_dev(u[t]) | step(1) | gather_state_dev(row t) |
// read_touches_dev(touch + t * n_touch)  in one call with the step's one host wait per pass (k_batch_trace.h).  Part of the single
// translation unit mgf_hip.hip (included there, in order, behind host_batch_spring.inc); not compiled on its own.
//
// Nothing of a rollout is written a second time here: the refusals are batch_rollout_args' with the touch trace's slotted in, the core
// is batch_rollout_run with the trace handed on, and the launch - MGF_BATCH_ROLLOUT_TOUCH_LAUNCHES_PER_TICK = 1 a tick a pass, behind
// k_batch_rollout_record, counted in "rollout_launches" - is the train's (batch_step_run, host_batch.inc), which rebuilds the view of the
// constraint lists for every pass: a capacity re-run moves them.  The rig is the contact sensors' (mgf_batch_set_touches), the plan and
// the upload are host_batch_rig.inc's, the dynamic LDS is batch_touch_tile's.  "query_launches" and "drive_launches" are not touched.
// touch == NULL or n_touch == 0 (an empty rig): mgf_batch_rollout / _rollout_dev, launch for launch.
// The order of both calls: the refusals that need no handle, the handle's own, (device form) EVERY device pointer looked up for its
// n_ticks-fold extent and the outputs held against each other and against the inputs - and only then the first thing is enqueued.

// the refusals of both forms, in the header's order; no device is touched and nothing is enqueued
static mgf_status batch_trace_args(const mgf_batch* b, int32_t iters, int64_t n_ticks, const float* u, int64_t n_act, int32_t mode, const int32_t* body,
                                   int64_t m, const void* touch, int64_t n_touch, int32_t touch_format, RolloutBytes* bytes, RolloutTouch* tt) {
  tt->out = const_cast<void*>(touch); tt->n = n_touch; tt->format = touch_format;
  return batch_rollout_args(b, iters, n_ticks, u, n_act, mode, body, m, bytes, tt);
}

extern "C" mgf_status mgf_batch_rollout_touches_dev(mgf_batch* b, float dt, int32_t iters, int64_t n_ticks, const float* u_dev, int64_t n_act, int32_t mode,
                                                    const int32_t* body_dev, int64_t m, float* x_dev, float* q_dev, float* v_dev, float* omega_dev,
                                                    void* touch_dev, int64_t n_touch, int32_t touch_format, mgf_step_stats* stats) {
  RolloutBytes n;
  RolloutTouch tt;
  MGF_TRY(batch_trace_args(b, iters, n_ticks, u_dev, n_act, mode, body_dev, m, touch_dev, n_touch, touch_format, &n, &tt));
  MGF_TRY(ctx_bind(b->ctx));
  MGF_TRY(dev_span(b->ctx, u_dev, n.u, "u_dev"));
  MGF_TRY(dev_span(b->ctx, body_dev, n.body, "body_dev"));
  MGF_TRY(dev_span(b->ctx, x_dev, n.out[0], "x_dev"));
  MGF_TRY(dev_span(b->ctx, q_dev, n.out[1], "q_dev"));
  MGF_TRY(dev_span(b->ctx, v_dev, n.out[2], "v_dev"));
  MGF_TRY(dev_span(b->ctx, omega_dev, n.out[3], "omega_dev"));
  MGF_TRY(dev_span(b->ctx, touch_dev, n.touch, "touch_dev"));
  const DevBytes arrays[7] = {{x_dev, n.out[0], "x_dev"}, {q_dev, n.out[1], "q_dev"}, {v_dev, n.out[2], "v_dev"}, {omega_dev, n.out[3], "omega_dev"},
                              {touch_dev, n.touch, "touch_dev"}, {u_dev, n.u, "u_dev"}, {body_dev, n.body, "body_dev"}};
  MGF_TRY(dev_outputs_overlap(arrays, 7, 5));
  return batch_rollout_run(b, dt, iters, n_ticks, u_dev, n_act, mode, body_dev, m, x_dev, q_dev, v_dev, omega_dev, stats, &tt);
}

// The host form: one upload (u | body), the device core, one download (x | q | v | omega | touch).  As in mgf_batch_rollout the handle's
// buffer is cleared, not filled from the caller's rows: a row of an index outside the batch comes back as zeros.  (Every report is
// written: every world completes every tick of a call that returns MGF_OK.)
extern "C" mgf_status mgf_batch_rollout_touches(mgf_batch* b, float dt, int32_t iters, int64_t n_ticks, const float* u, int64_t n_act, int32_t mode,
                                                const int32_t* body, int64_t m, float* x, float* q, float* v, float* omega, void* touch, int64_t n_touch,
                                                int32_t touch_format, mgf_step_stats* stats) {
  RolloutBytes n;
  RolloutTouch tt;
  MGF_TRY(batch_trace_args(b, iters, n_ticks, u, n_act, mode, body, m, touch, n_touch, touch_format, &n, &tt));
  MGF_TRY(ctx_bind(b->ctx));
  hipStream_t s = b->ctx->stream;
  // the handle's buffer, every section from a 16-byte boundary: u | body | x | q | v | omega | touch
  const void* host_in[2] = {u, body};
  void* host_out[5] = {x, q, v, omega, touch};
  const size_t bytes[7] = {n.u, body ? n.body : 0, n.out[0], n.out[1], n.out[2], n.out[3], n.touch};
  size_t off[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = 0; k < 7; ++k) off[k + 1] = off[k] + ((k < 2 ? host_in[k] != nullptr : host_out[k - 2] != nullptr) ? (bytes[k] + 15) / 16 : 0);
  void* dev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  std::vector<float4> stage;
  if (off[7]) {
    MGF_TRY(b->q_in.ensure(off[7], s));
    for (int k = 0; k < 7; ++k)
      if (off[k + 1] > off[k]) dev[k] = b->q_in.p + off[k];
    if (off[2]) {
      stage.resize(off[2]);
      for (int k = 0; k < 2; ++k)
        if (dev[k]) memcpy(stage.data() + off[k], host_in[k], bytes[k]);
      MGF_TRY(h2d(b->ctx, b->q_in.p, stage.data(), off[2]));
    }
    if (off[7] > off[2]) MGF_HIP_TRY(hipMemsetAsync(b->q_in.p + off[2], 0, 16 * (off[7] - off[2]), s));
  }
  tt.out = dev[6];
  MGF_TRY(batch_rollout_run(b, dt, iters, n_ticks, static_cast<const float*>(dev[0]), n_act, mode, static_cast<const int32_t*>(dev[1]), m, static_cast<float*>(dev[2]),
                            static_cast<float*>(dev[3]), static_cast<float*>(dev[4]), static_cast<float*>(dev[5]), stats, &tt));
  if (off[7] > off[2]) {
    stage.resize(off[7] - off[2]);
    MGF_TRY(d2h(b->ctx, stage.data(), b->q_in.p + off[2], stage.size()));
    for (int k = 2; k < 7; ++k)
      if (dev[k]) memcpy(host_out[k - 2], stage.data() + (off[k] - off[2]), bytes[k]);
  }
  return MGF_OK;
}
