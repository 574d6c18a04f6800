// mgf_batch_set_sliders, mgf_batch_slider_count, mgf_batch_set_slider_targets, mgf_batch_set_slider_targets_dev, mgf_batch_solve_sliders,
// mgf_batch_solve_sliders_dev: slider (prismatic) joints between two bodies of a world, or between one and the world - three angular
// rows that hold other's frame onto body's, two linear rows that hold other's anchor on the axis through body's, and along the axis an
// optional limit of the travel, an optional velocity motor with a force cap, or a lock (a weld) - solved by sequential impulses over
// the velocities resident on the device (k_batch_slider.h).  Part of the single translation unit mgf_hip.hip (included there, in
// order, behind host_batch_hinge_read.inc); not compiled on its own.
//
// The tenth rig.  What it shares with the others is host_batch_rig.inc's: the prologue and the world / body check of the set call, the
// upload - items | records | plan and slots, ONE copy (batch_rig_up) - and the check of `body` against the lengths that go up with it;
// `other` is held against them here, ahead of it.  The plan is the ball joints' (batch_joint_plan, host_batch_joint.inc): the sliders
// sorted by world, a world's named bodies numbered as local slots, per slider its two slots and its rank in each body's chain.
// The motors' target speeds are a table of the handle's, W[rows][slider_count] in device memory (mgf_batch_set_slider_targets / _dev): a
// solve call names the row it reads, a rollout's tick t reads row min(t, rows - 1).  Setting the rig makes the table one row of zeros.
// A call is MGF_BATCH_SLIDER_LAUNCHES = 1 launch ("drive_launches") whatever the sliders and the worlds.  Nothing here reads a shape, so a
// batch with bodies of several components is not refused.  The device forms make no host wait and no copy between host and device; the
// host form of the solve downloads the impulses where asked and waits once.
// A rollout (host_batch_rollout.inc) takes the same launch into the step's train behind the hinges' and ahead of the tick:
// batch_slider_ready fills the hook's arguments, batch_step_run (host_batch.inc) launches it.

static bool slider_unit(double a) { return std::fabs(a - 1.0) <= 1e-3; }
static double slider_dot(const mgf_vec3& a, const mgf_vec3& b) { return (double)a.x * b.x + (double)a.y * b.y + (double)a.z * b.z; }

extern "C" mgf_status mgf_batch_set_sliders(mgf_batch* b, const mgf_batch_slider* j, int64_t n_in) {
  MGF_TRY(batch_rig_set_args(b, j, n_in));
  static_assert(sizeof(mgf_batch_slider) == 112, "the rig goes up as the caller's records: seven words of 16 bytes");
  static_assert(MGF_BATCH_MAX_WORLD_SLIDERS == kBatchBlock, "k_batch_slider_solve has a lane per slider of a world");
  static_assert(MGF_SLIDER_LIMIT == kSliderLimit && MGF_SLIDER_MOTOR == kSliderMotor && MGF_SLIDER_LOCK == kSliderLock, "the kernel's flag bits are the header's");
  const size_t n = (size_t)n_in;
  std::vector<uint32_t> per_world(n ? b->K : 0, 0u);
  for (size_t i = 0; i < n; ++i) {
    const mgf_batch_slider& r = j[i];
    MGF_TRY(batch_rig_ref_check(b, r.world, r.body, 0, "slider"));  // (the flag word is this rig's own: below)
    if (r.other < -1 || (r.other >= 0 && (uint32_t)r.other >= b->h_n[(size_t)r.world]))
      return fail(MGF_ERR_INVALID, "a slider's other is neither -1 nor a body of its world: the rig was not changed");
    if (r.other == r.body) return fail(MGF_ERR_INVALID, "a slider's other is its body: the rig was not changed");
    if (r.flags & ~(uint32_t)(MGF_SLIDER_LIMIT | MGF_SLIDER_MOTOR | MGF_SLIDER_LOCK))
      return fail(MGF_ERR_INVALID, "a slider's flags hold a bit beyond MGF_SLIDER_LIMIT | MGF_SLIDER_MOTOR | MGF_SLIDER_LOCK: the rig was not changed");
    if ((r.flags & MGF_SLIDER_LOCK) && (r.flags & (MGF_SLIDER_LIMIT | MGF_SLIDER_MOTOR)))
      return fail(MGF_ERR_INVALID, "a slider's MGF_SLIDER_LOCK stands beside MGF_SLIDER_LIMIT or MGF_SLIDER_MOTOR: the rig was not changed");
    if (!actuator_finite3(r.pa) || !actuator_finite3(r.pb) || !actuator_finite3(r.ax) || !actuator_finite3(r.ua) || !actuator_finite3(r.bx) ||
        !actuator_finite3(r.ub) || !std::isfinite(r.beta) || std::isnan(r.fmax) || r.fmax == -INFINITY || !std::isfinite(r.lo) || !std::isfinite(r.hi) ||
        !std::isfinite(r.pad0) || !std::isfinite(r.pad1))
      return fail(MGF_ERR_INVALID, "a word of a slider is not finite (fmax may be +inf): the rig was not changed");
    if (r.pad0 != 0.0f || r.pad1 != 0.0f) return fail(MGF_ERR_INVALID, "a slider's pad0 or pad1 is not 0: the rig was not changed");
    if (r.beta < 0.0f || r.beta > 1.0f) return fail(MGF_ERR_INVALID, "a slider's beta is not in [0, 1]: the rig was not changed");
    if (r.fmax < 0.0f) return fail(MGF_ERR_INVALID, "a slider's fmax is negative: the rig was not changed");
    if (r.lo > r.hi) return fail(MGF_ERR_INVALID, "a slider's lo is above its hi: the rig was not changed");
    if (!slider_unit(slider_dot(r.ax, r.ax)) || !slider_unit(slider_dot(r.ua, r.ua)) || !slider_unit(slider_dot(r.bx, r.bx)) || !slider_unit(slider_dot(r.ub, r.ub)))
      return fail(MGF_ERR_INVALID, "a slider's ax, ua, bx or ub is not of unit length: the rig was not changed");
    if (std::fabs(slider_dot(r.ax, r.ua)) > 1e-3 || std::fabs(slider_dot(r.bx, r.ub)) > 1e-3)
      return fail(MGF_ERR_INVALID, "a slider's reference is not perpendicular to its axis: the rig was not changed");
    if (++per_world[(size_t)r.world] > MGF_BATCH_MAX_WORLD_SLIDERS)
      return fail(MGF_ERR_INVALID, "a world holds at most MGF_BATCH_MAX_WORLD_SLIDERS (256) sliders: the rig was not changed");
  }
  batch_joint_plan(b->sliders, j, n);
  b->sg_rows = 1;  // (the table: one row of zeros, made where the rig goes up)
  b->sg_zero = true;
  return MGF_OK;
}

extern "C" int64_t mgf_batch_slider_count(const mgf_batch* b) { return b ? (int64_t)b->sliders.recs.size() : -1; }

// the refusals of both target calls that need no device
static mgf_status batch_slider_target_args(const mgf_batch* b, const float* w, int64_t rows) {
  MGF_TRY(batch_rig_handle(b));
  if (rows < 1 || rows > (1 << 20)) return fail(MGF_ERR_INVALID, "rows must be in [1, 2^20]");
  const size_t n = b->sliders.recs.size();
  if (!w && n > 0) return fail(MGF_ERR_INVALID, "NULL argument: w");
  if ((uint64_t)n > (uint64_t)INT64_MAX / 4u / (uint64_t)rows) return fail(MGF_ERR_INVALID, "4 * rows * mgf_batch_slider_count overflows int64_t");
  return MGF_OK;
}

// the table taken into the handle's memory: `kind` says where w lies
static mgf_status batch_slider_targets(mgf_batch* b, const float* w, int64_t rows, hipMemcpyKind kind) {
  hipStream_t s = b->ctx->stream;
  const size_t words = (size_t)rows * b->sliders.recs.size();
  if (words) {
    MGF_TRY(b->sg_w.ensure(words, s));
    MGF_HIP_TRY(hipMemcpyAsync(b->sg_w.p, w, 4 * words, kind, s));
    if (kind == hipMemcpyHostToDevice) MGF_HIP_TRY(hipStreamSynchronize(s));  // (the caller's array is his again when the call returns)
  }
  b->sg_rows = rows;
  b->sg_zero = false;
  return MGF_OK;
}

extern "C" mgf_status mgf_batch_set_slider_targets(mgf_batch* b, const float* w, int64_t rows) {
  MGF_TRY(batch_slider_target_args(b, w, rows));
  MGF_TRY(ctx_bind(b->ctx));
  return batch_slider_targets(b, w, rows, hipMemcpyHostToDevice);
}

extern "C" mgf_status mgf_batch_set_slider_targets_dev(mgf_batch* b, const float* w_dev, int64_t rows) {
  MGF_TRY(batch_slider_target_args(b, w_dev, rows));
  MGF_TRY(ctx_bind(b->ctx));
  MGF_TRY(dev_span(b->ctx, w_dev, 4 * (size_t)rows * b->sliders.recs.size(), "w_dev"));
  return batch_slider_targets(b, w_dev, rows, hipMemcpyDeviceToDevice);
}

// What the kernel reads of the handle, as it is now: a rollout's train looks it up again for every pass, as the other hooks' views are.
static void batch_slider_view(const mgf_batch* b, BatchSliderArgs* A) {
  const BatchRig<mgf_batch_slider>& R = b->sliders;
  A->B = b->bodies(0);
  A->w_off = b->d_off.p;
  A->items = reinterpret_cast<const uint4*>(R.dev.p);
  A->rig = R.dev.p + R.off[1];
  A->plan = reinterpret_cast<const uint4*>(R.dev.p + R.off[2]);
  A->slots = reinterpret_cast<const uint2*>(R.dev.p + R.off[2] + R.recs.size());  // (behind the plan's n words of 16 bytes)
  A->acc = b->sg_acc.p;
  A->skipped = b->sg_skipped.p;
  A->err = b->d_err.p;
}

// What the launch reads, behind batch_push (n > 0): the rig up, the target table, the handle's impulse buffer and skip counter there.
// `out_dev`: device memory of 8 n floats or null.  Shared with the rollouts, whose train fills done, act, tick and the table's row in
// (A->w is row 0 here).  *lds: the launch's dynamic LDS.
static mgf_status batch_slider_ready(mgf_batch* b, float h, int32_t iters, float* out_dev, BatchSliderArgs* A, uint32_t* lds) {
  BatchRig<mgf_batch_slider>& R = b->sliders;
  hipStream_t s = b->ctx->stream;
  const size_t n = R.recs.size();
  if (R.stale)  // (bodies may have been added: the far ends against the lengths that go up, as batch_rig_up holds `body`)
    for (size_t i = 0; i < n; ++i)
      if (R.recs[i].other >= 0 && (uint32_t)R.recs[i].other >= b->h_n[(size_t)R.recs[i].world])
        return fail(MGF_ERR_INVALID, "internal error: a slider's other is outside its world");
  MGF_TRY(batch_rig_up(b, R, "slider", 3));
  if (b->sg_zero) {  // (the rig was set behind the last table: one row of zeros)
    MGF_TRY(b->sg_w.ensure(n, s));
    MGF_HIP_TRY(hipMemsetAsync(b->sg_w.p, 0, 4 * n, s));
    b->sg_rows = 1;
    b->sg_zero = false;
  }
  MGF_TRY(b->sg_acc.ensure(8 * n, s));
  if (!b->sg_skipped.p) {
    MGF_TRY(b->sg_skipped.ensure(1, s));
    MGF_HIP_TRY(hipMemsetAsync(b->sg_skipped.p, 0, sizeof(unsigned long long), s));
  }
  memset(A, 0, sizeof(*A));
  batch_slider_view(b, A);
  A->w = b->sg_w.p;
  A->out = out_dev;
  A->h = h;
  A->iters = (uint32_t)iters;
  uint32_t most = 0;
  for (const uint4& it : R.items) most = std::max(most, it.z >> 16);
  *lds = 36u * most;  // 32 bytes a slot of (v, omega), one progress word
  return MGF_OK;
}

// The launch of a call, behind every check (n > 0, iters > 0, row inside the table).
static mgf_status batch_slider_run(mgf_batch* b, float h, int32_t iters, int64_t row, float* out_dev) {
  hipStream_t s = b->ctx->stream;
  MGF_TRY(batch_push(b));
  BatchSliderArgs A;
  uint32_t lds = 0;
  MGF_TRY(batch_slider_ready(b, h, iters, out_dev, &A, &lds));
  A.w = b->sg_w.p + (size_t)row * b->sliders.recs.size();
  k_batch_slider_solve<false><<<(unsigned)b->sliders.items.size(), kBatchBlock, lds, s>>>(A);
  LAUNCH_CHECK();
  b->d_launches += MGF_BATCH_SLIDER_LAUNCHES;
  return MGF_OK;
}

// the refusals of both solve calls that need no device: the ball joints', and the row behind them
static mgf_status batch_slider_args(const mgf_batch* b, float h, int32_t iters, int64_t row) {
  MGF_TRY(batch_joint_args(b, h, iters));
  if (row < 0 || row >= b->sg_rows) return fail(MGF_ERR_INVALID, "row is outside the target table");
  return MGF_OK;
}

extern "C" mgf_status mgf_batch_solve_sliders(mgf_batch* b, float h, int32_t iters, int64_t row, float* impulse_out) {
  MGF_TRY(batch_slider_args(b, h, iters, row));
  MGF_TRY(ctx_bind(b->ctx));
  b->d_launches = 0;
  const size_t n = b->sliders.recs.size();
  if (n == 0 || iters == 0) return MGF_OK;
  hipStream_t s = b->ctx->stream;
  MGF_TRY(batch_slider_run(b, h, iters, row, nullptr));
  uint32_t gave_up = 0;
  if (impulse_out) MGF_HIP_TRY(hipMemcpyAsync(impulse_out, b->sg_acc.p, 32 * n, hipMemcpyDeviceToHost, s));  // (the handle's buffer holds every impulse)
  MGF_HIP_TRY(hipMemcpyAsync(&gave_up, b->d_err.p + 1, 4, hipMemcpyDeviceToHost, s));
  MGF_HIP_TRY(hipStreamSynchronize(s));
  if (gave_up) return fail(MGF_ERR_HIP, "internal error: a lane of the slider solver gave up waiting for its turn");
  return MGF_OK;
}

extern "C" mgf_status mgf_batch_solve_sliders_dev(mgf_batch* b, float h, int32_t iters, int64_t row, float* impulse_out_dev) {
  MGF_TRY(batch_slider_args(b, h, iters, row));
  MGF_TRY(ctx_bind(b->ctx));
  b->d_launches = 0;
  const size_t n = b->sliders.recs.size();
  MGF_TRY(dev_span(b->ctx, impulse_out_dev, 32 * n, "impulse_out_dev"));
  if (n == 0 || iters == 0) return MGF_OK;
  return batch_slider_run(b, h, iters, row, impulse_out_dev);
}
