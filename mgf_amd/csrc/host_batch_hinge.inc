// mgf_batch_set_hinges, mgf_batch_hinge_count, mgf_batch_set_hinge_targets, mgf_batch_set_hinge_targets_dev, mgf_batch_solve_hinges,
// mgf_batch_solve_hinges_dev: hinge (revolute) joints between two bodies of a world, or between one and the world - a ball joint, two
// angular rows that keep the axes parallel, an optional limit of the hinge angle and an optional velocity motor with a torque cap -
// solved by sequential impulses over the velocities resident on the device (k_batch_hinge.h).  Part of the single translation unit
// mgf_hip.hip (included there, in order, behind host_batch_joint.inc); not compiled on its own.
//
// The ninth rig.  What it shares with the others is host_batch_rig.inc's: the prologue and the world / body check of the set call, the
// upload - items | records | plan and slots, ONE copy (batch_rig_up) - and the check of `body` against the lengths that go up with it;
// `other` is held against them here, ahead of it.  The plan is the ball joints' (batch_joint_plan, host_batch_joint.inc): the hinges
// sorted by world, a world's hinged bodies numbered as local slots, per hinge its two slots and its rank in each body's chain.
// The motors' target speeds are a table of the handle's, W[rows][hinge_count] in device memory (mgf_batch_set_hinge_targets / _dev): a
// solve call names the row it reads, a rollout's tick t reads row min(t, rows - 1).  Setting the rig makes the table one row of zeros.
// A call is MGF_BATCH_HINGE_LAUNCHES = 1 launch ("drive_launches") whatever the hinges and the worlds.  Nothing here reads a shape, so a
// batch with bodies of several components is not refused.  The device forms make no host wait and no copy between host and device; the
// host form of the solve downloads the impulses where asked and waits once.
// A rollout (host_batch_rollout.inc) takes the same launch into the step's train behind the ball joints' and ahead of the tick:
// batch_hinge_ready fills the hook's arguments, batch_step_run (host_batch.inc) launches it.

static bool hinge_unit(double a) { return std::fabs(a - 1.0) <= 1e-3; }
static double hinge_dot(const mgf_vec3& a, const mgf_vec3& b) { return (double)a.x * b.x + (double)a.y * b.y + (double)a.z * b.z; }

extern "C" mgf_status mgf_batch_set_hinges(mgf_batch* b, const mgf_batch_hinge* j, int64_t n_in) {
  MGF_TRY(batch_rig_set_args(b, j, n_in));
  static_assert(sizeof(mgf_batch_hinge) == 112, "the rig goes up as the caller's records: seven words of 16 bytes");
  static_assert(MGF_BATCH_MAX_WORLD_HINGES == kBatchBlock, "k_batch_hinge_solve has a lane per hinge of a world");
  static_assert(MGF_HINGE_LIMIT == kHingeLimit && MGF_HINGE_MOTOR == kHingeMotor, "the kernel's flag bits are the header's");
  const size_t n = (size_t)n_in;
  std::vector<uint32_t> per_world(n ? b->K : 0, 0u);
  for (size_t i = 0; i < n; ++i) {
    const mgf_batch_hinge& r = j[i];
    MGF_TRY(batch_rig_ref_check(b, r.world, r.body, 0, "hinge"));  // (the flag word is this rig's own: below)
    if (r.other < -1 || (r.other >= 0 && (uint32_t)r.other >= b->h_n[(size_t)r.world]))
      return fail(MGF_ERR_INVALID, "a hinge's other is neither -1 nor a body of its world: the rig was not changed");
    if (r.other == r.body) return fail(MGF_ERR_INVALID, "a hinge's other is its body: the rig was not changed");
    if (r.flags & ~(uint32_t)(MGF_HINGE_LIMIT | MGF_HINGE_MOTOR))
      return fail(MGF_ERR_INVALID, "a hinge's flags hold a bit beyond MGF_HINGE_LIMIT | MGF_HINGE_MOTOR: the rig was not changed");
    if (!actuator_finite3(r.pa) || !actuator_finite3(r.pb) || !actuator_finite3(r.ax) || !actuator_finite3(r.ua) || !actuator_finite3(r.bx) ||
        !actuator_finite3(r.ub) || !std::isfinite(r.beta) || std::isnan(r.tmax) || r.tmax == -INFINITY || !std::isfinite(r.cm) || !std::isfinite(r.sm) ||
        !std::isfinite(r.ch) || !std::isfinite(r.sh))
      return fail(MGF_ERR_INVALID, "a word of a hinge is not finite (tmax may be +inf): the rig was not changed");
    if (r.beta < 0.0f || r.beta > 1.0f) return fail(MGF_ERR_INVALID, "a hinge's beta is not in [0, 1]: the rig was not changed");
    if (r.tmax < 0.0f) return fail(MGF_ERR_INVALID, "a hinge's tmax is negative: the rig was not changed");
    if (!hinge_unit(hinge_dot(r.ax, r.ax)) || !hinge_unit(hinge_dot(r.ua, r.ua)) || !hinge_unit(hinge_dot(r.bx, r.bx)) || !hinge_unit(hinge_dot(r.ub, r.ub)) ||
        !hinge_unit((double)r.cm * r.cm + (double)r.sm * r.sm) || !hinge_unit((double)r.ch * r.ch + (double)r.sh * r.sh))
      return fail(MGF_ERR_INVALID, "a hinge's ax, ua, bx, ub, (cm, sm) or (ch, sh) is not of unit length: the rig was not changed");
    if (std::fabs(hinge_dot(r.ax, r.ua)) > 1e-3 || std::fabs(hinge_dot(r.bx, r.ub)) > 1e-3)
      return fail(MGF_ERR_INVALID, "a hinge's reference is not perpendicular to its axis: the rig was not changed");
    if (r.sh < 0.0f) return fail(MGF_ERR_INVALID, "a hinge's sh is negative: the rig was not changed");
    if (++per_world[(size_t)r.world] > MGF_BATCH_MAX_WORLD_HINGES)
      return fail(MGF_ERR_INVALID, "a world holds at most MGF_BATCH_MAX_WORLD_HINGES (256) hinges: the rig was not changed");
  }
  batch_joint_plan(b->hinges, j, n);
  b->hg_rows = 1;  // (the table: one row of zeros, made where the rig goes up)
  b->hg_zero = true;
  b->ht_rows = 0;  // (the readings table is rows of the OLD rig's hinges: the trace is off until mgf_batch_set_hinge_trace names it again)
  return MGF_OK;
}

extern "C" int64_t mgf_batch_hinge_count(const mgf_batch* b) { return b ? (int64_t)b->hinges.recs.size() : -1; }

// the refusals of both target calls that need no device
static mgf_status batch_hinge_target_args(const mgf_batch* b, const float* w, int64_t rows) {
  MGF_TRY(batch_rig_handle(b));
  if (rows < 1 || rows > (1 << 20)) return fail(MGF_ERR_INVALID, "rows must be in [1, 2^20]");
  const size_t n = b->hinges.recs.size();
  if (!w && n > 0) return fail(MGF_ERR_INVALID, "NULL argument: w");
  if ((uint64_t)n > (uint64_t)INT64_MAX / 4u / (uint64_t)rows) return fail(MGF_ERR_INVALID, "4 * rows * mgf_batch_hinge_count overflows int64_t");
  return MGF_OK;
}

// the table taken into the handle's memory: `kind` says where w lies
static mgf_status batch_hinge_targets(mgf_batch* b, const float* w, int64_t rows, hipMemcpyKind kind) {
  hipStream_t s = b->ctx->stream;
  const size_t words = (size_t)rows * b->hinges.recs.size();
  if (words) {
    MGF_TRY(b->hg_w.ensure(words, s));
    MGF_HIP_TRY(hipMemcpyAsync(b->hg_w.p, w, 4 * words, kind, s));
    if (kind == hipMemcpyHostToDevice) MGF_HIP_TRY(hipStreamSynchronize(s));  // (the caller's array is his again when the call returns)
  }
  b->hg_rows = rows;
  b->hg_zero = false;
  return MGF_OK;
}

extern "C" mgf_status mgf_batch_set_hinge_targets(mgf_batch* b, const float* w, int64_t rows) {
  MGF_TRY(batch_hinge_target_args(b, w, rows));
  MGF_TRY(ctx_bind(b->ctx));
  return batch_hinge_targets(b, w, rows, hipMemcpyHostToDevice);
}

extern "C" mgf_status mgf_batch_set_hinge_targets_dev(mgf_batch* b, const float* w_dev, int64_t rows) {
  MGF_TRY(batch_hinge_target_args(b, w_dev, rows));
  MGF_TRY(ctx_bind(b->ctx));
  MGF_TRY(dev_span(b->ctx, w_dev, 4 * (size_t)rows * b->hinges.recs.size(), "w_dev"));
  return batch_hinge_targets(b, w_dev, rows, hipMemcpyDeviceToDevice);
}

// What the kernel reads of the handle, as it is now: a rollout's train looks it up again for every pass, as the other hooks' views are.
static void batch_hinge_view(const mgf_batch* b, BatchHingeArgs* A) {
  const BatchRig<mgf_batch_hinge>& R = b->hinges;
  A->B = b->bodies(0);
  A->w_off = b->d_off.p;
  A->items = reinterpret_cast<const uint4*>(R.dev.p);
  A->rig = R.dev.p + R.off[1];
  A->plan = reinterpret_cast<const uint4*>(R.dev.p + R.off[2]);
  A->slots = reinterpret_cast<const uint2*>(R.dev.p + R.off[2] + R.recs.size());  // (behind the plan's n words of 16 bytes)
  A->acc = b->hg_acc.p;
  A->skipped = b->hg_skipped.p;
  A->err = b->d_err.p;
}

// What the launch reads, behind batch_push (n > 0): the rig up, the target table, the handle's impulse buffer and skip counter there.
// `out_dev`: device memory of 8 n floats or null.  Shared with the rollouts, whose train fills done, act, tick and the table's row in
// (A->w is row 0 here).  *lds: the launch's dynamic LDS.
static mgf_status batch_hinge_ready(mgf_batch* b, float h, int32_t iters, float* out_dev, BatchHingeArgs* A, uint32_t* lds) {
  BatchRig<mgf_batch_hinge>& R = b->hinges;
  hipStream_t s = b->ctx->stream;
  const size_t n = R.recs.size();
  if (R.stale)  // (bodies may have been added: the far ends against the lengths that go up, as batch_rig_up holds `body`)
    for (size_t i = 0; i < n; ++i)
      if (R.recs[i].other >= 0 && (uint32_t)R.recs[i].other >= b->h_n[(size_t)R.recs[i].world])
        return fail(MGF_ERR_INVALID, "internal error: a hinge's other is outside its world");
  MGF_TRY(batch_rig_up(b, R, "hinge", 3));
  if (b->hg_zero) {  // (the rig was set behind the last table: one row of zeros)
    MGF_TRY(b->hg_w.ensure(n, s));
    MGF_HIP_TRY(hipMemsetAsync(b->hg_w.p, 0, 4 * n, s));
    b->hg_rows = 1;
    b->hg_zero = false;
  }
  MGF_TRY(b->hg_acc.ensure(8 * n, s));
  if (!b->hg_skipped.p) {
    MGF_TRY(b->hg_skipped.ensure(1, s));
    MGF_HIP_TRY(hipMemsetAsync(b->hg_skipped.p, 0, sizeof(unsigned long long), s));
  }
  memset(A, 0, sizeof(*A));
  batch_hinge_view(b, A);
  A->w = b->hg_w.p;
  A->out = out_dev;
  A->h = h;
  A->iters = (uint32_t)iters;
  uint32_t most = 0;
  for (const uint4& it : R.items) most = std::max(most, it.z >> 16);
  *lds = 36u * most;  // 32 bytes a slot of (v, omega), one progress word
  return MGF_OK;
}

// The launch of a call, behind every check (n > 0, iters > 0, row inside the table).
static mgf_status batch_hinge_run(mgf_batch* b, float h, int32_t iters, int64_t row, float* out_dev) {
  hipStream_t s = b->ctx->stream;
  MGF_TRY(batch_push(b));
  BatchHingeArgs A;
  uint32_t lds = 0;
  MGF_TRY(batch_hinge_ready(b, h, iters, out_dev, &A, &lds));
  A.w = b->hg_w.p + (size_t)row * b->hinges.recs.size();
  k_batch_hinge_solve<false><<<(unsigned)b->hinges.items.size(), kBatchBlock, lds, s>>>(A);
  LAUNCH_CHECK();
  b->d_launches += MGF_BATCH_HINGE_LAUNCHES;
  return MGF_OK;
}

// the refusals of both solve calls that need no device: the ball joints', and the row behind them
static mgf_status batch_hinge_args(const mgf_batch* b, float h, int32_t iters, int64_t row) {
  MGF_TRY(batch_joint_args(b, h, iters));
  if (row < 0 || row >= b->hg_rows) return fail(MGF_ERR_INVALID, "row is outside the target table");
  return MGF_OK;
}

extern "C" mgf_status mgf_batch_solve_hinges(mgf_batch* b, float h, int32_t iters, int64_t row, float* impulse_out) {
  MGF_TRY(batch_hinge_args(b, h, iters, row));
  MGF_TRY(ctx_bind(b->ctx));
  b->d_launches = 0;
  const size_t n = b->hinges.recs.size();
  if (n == 0 || iters == 0) return MGF_OK;
  hipStream_t s = b->ctx->stream;
  MGF_TRY(batch_hinge_run(b, h, iters, row, nullptr));
  uint32_t gave_up = 0;
  if (impulse_out) MGF_HIP_TRY(hipMemcpyAsync(impulse_out, b->hg_acc.p, 32 * n, hipMemcpyDeviceToHost, s));  // (the handle's buffer holds every impulse)
  MGF_HIP_TRY(hipMemcpyAsync(&gave_up, b->d_err.p + 1, 4, hipMemcpyDeviceToHost, s));
  MGF_HIP_TRY(hipStreamSynchronize(s));
  if (gave_up) return fail(MGF_ERR_HIP, "internal error: a lane of the hinge solver gave up waiting for its turn");
  return MGF_OK;
}

extern "C" mgf_status mgf_batch_solve_hinges_dev(mgf_batch* b, float h, int32_t iters, int64_t row, float* impulse_out_dev) {
  MGF_TRY(batch_hinge_args(b, h, iters, row));
  MGF_TRY(ctx_bind(b->ctx));
  b->d_launches = 0;
  const size_t n = b->hinges.recs.size();
  MGF_TRY(dev_span(b->ctx, impulse_out_dev, 32 * n, "impulse_out_dev"));
  if (n == 0 || iters == 0) return MGF_OK;
  return batch_hinge_run(b, h, iters, row, impulse_out_dev);
}
