// mgf_batch_set_springs, mgf_batch_spring_count, mgf_batch_apply_springs, mgf_batch_apply_springs_dev: spring-dampers between two
// body-fixed points of a world, or between one and a point of the world, turned into impulses from the state resident on the device and
// applied there (k_batch_spring.h).  Part of the single translation unit mgf_hip.hip (included there, in order, behind
// host_batch_rollout.inc); not compiled on its own.
//
// The seventh rig, and the second on the action side: what a caller otherwise assembles per tick from gather_state of both ends - two
// arms turned by two quaternions, point velocities, a length, a unit vector, a clamp, two cross products, a sum per body - and hands to
// mgf_batch_apply_impulses_dev, a spring answers from the rig and the resident rows.  What the rig shares with the others is
// host_batch_rig.inc's: the prologue and the world / body check of the set call, the upload - runs | records | order, ONE copy
// (batch_rig_up) - and the check of `body` against the lengths that go up with it; `other` is held against them here, ahead of it.
// The plan is the actuators' with ENDS for actuators: the 2 n ends (end e = 2 i + side; a world anchor's far end is none) sorted by
// (world, body) - stable, a body's ends stay in list order - and cut into runs of one body, a lane each.
// A call is MGF_BATCH_SPRING_LAUNCHES = 2 launches ("drive_launches") whatever the springs and the worlds: every wrench is formed from
// the state before the call, so the wrenches are complete before the first velocity is written.  Nothing here reads a shape, so a
// batch with bodies of several components is not refused.  The device form makes no host wait and no copy between host and device;
// the host form downloads the wrenches where asked and waits once.
// A rollout (host_batch_rollout.inc) takes the same two launches into the step's train ahead of every tick: batch_spring_ready fills
// the hook's arguments, batch_step_run (host_batch.inc) launches them.

// The records become the rig: reached only behind every check of every record - this is the first change of the rig.  R.items holds the
// runs of ends: (world, body, first sorted position, count); R.order the ends in sorted order.  No device is needed.
static void batch_spring_plan(BatchRig<mgf_batch_spring>& R, const mgf_batch_spring* recs, size_t n) {
  std::vector<uint32_t> order;
  order.reserve(2 * n);
  for (size_t i = 0; i < n; ++i) {
    order.push_back((uint32_t)(2 * i));
    if (recs[i].other >= 0) order.push_back((uint32_t)(2 * i + 1));
  }
  auto body = [&](uint32_t e) { return (uint32_t)((e & 1u) ? recs[e >> 1].other : recs[e >> 1].body); };
  auto key = [&](uint32_t e) { return ((uint64_t)(uint32_t)recs[e >> 1].world << 32) | body(e); };
  std::stable_sort(order.begin(), order.end(), [&](uint32_t l, uint32_t r) { return key(l) < key(r); });
  std::vector<uint4> runs;
  for (size_t p = 0; p < order.size(); ++p) {
    if (p == 0 || key(order[p]) != key(order[p - 1])) runs.push_back(make_uint4((uint32_t)recs[order[p] >> 1].world, body(order[p]), (uint32_t)p, 0u));
    ++runs.back().w;
  }
  R.recs.assign(recs, recs + n);
  R.items.swap(runs);
  R.order.swap(order);
  R.stale = true;
}

extern "C" mgf_status mgf_batch_set_springs(mgf_batch* b, const mgf_batch_spring* sp, int64_t n_in) {
  MGF_TRY(batch_rig_set_args(b, sp, n_in));
  static_assert(sizeof(mgf_batch_spring) == 64, "the rig goes up as the caller's records: four words of 16 bytes");
  const size_t n = (size_t)n_in;
  for (size_t i = 0; i < n; ++i) {
    const mgf_batch_spring& r = sp[i];
    MGF_TRY(batch_rig_ref_check(b, r.world, r.body, 0, "spring"));  // (the flag word is this rig's own: below)
    if (r.other < -1 || (r.other >= 0 && (uint32_t)r.other >= b->h_n[(size_t)r.world]))
      return fail(MGF_ERR_INVALID, "a spring's other is neither -1 nor a body of its world: the rig was not changed");
    if (r.other == r.body) return fail(MGF_ERR_INVALID, "a spring's other is its body: the rig was not changed");
    if (r.flags != 0u) return fail(MGF_ERR_INVALID, "a spring's flags are not 0: the rig was not changed");
    if (!actuator_finite3(r.pa) || !actuator_finite3(r.pb) || !std::isfinite(r.k) || !std::isfinite(r.c) || !std::isfinite(r.rest))
      return fail(MGF_ERR_INVALID, "a spring's pa, pb, k, c or rest is not finite: the rig was not changed");
    if (r.rest < 0.0f) return fail(MGF_ERR_INVALID, "a spring's rest is negative: the rig was not changed");
    if (std::isnan(r.lo) || std::isnan(r.hi) || r.lo > r.hi)
      return fail(MGF_ERR_INVALID, "a spring's lo or hi is a NaN, or lo > hi: the rig was not changed");
  }
  batch_spring_plan(b->springs, sp, n);
  return MGF_OK;
}

extern "C" int64_t mgf_batch_spring_count(const mgf_batch* b) { return b ? (int64_t)b->springs.recs.size() : -1; }

// What both launches read, behind batch_push (n > 0): the rig up, the handle's wrench buffer and skip counter there.  `out_dev`: device
// memory of 12 n floats or null.  Shared with the rollouts, whose train fills done, act and tick in.
static mgf_status batch_spring_ready(mgf_batch* b, float h, float* out_dev, BatchSpringArgs* A) {
  BatchRig<mgf_batch_spring>& R = b->springs;
  hipStream_t s = b->ctx->stream;
  const size_t n = R.recs.size();
  if (R.stale)  // (bodies may have been added: the far ends against the lengths that go up, as batch_rig_up holds `body`)
    for (size_t i = 0; i < n; ++i)
      if (R.recs[i].other >= 0 && (uint32_t)R.recs[i].other >= b->h_n[(size_t)R.recs[i].world])
        return fail(MGF_ERR_INVALID, "internal error: a spring's other is outside its world");
  MGF_TRY(batch_rig_up(b, R, "spring", 3));
  MGF_TRY(b->sp_wr.ensure(12 * n, s));
  if (!b->sp_skipped.p) {
    MGF_TRY(b->sp_skipped.ensure(1, s));
    MGF_HIP_TRY(hipMemsetAsync(b->sp_skipped.p, 0, sizeof(unsigned long long), s));
  }
  memset(A, 0, sizeof(*A));
  A->B = b->bodies(0);
  A->w_off = b->d_off.p;
  A->runs = reinterpret_cast<const uint4*>(R.dev.p);
  A->rig = R.dev.p + R.off[1];
  A->order = reinterpret_cast<const uint32_t*>(R.dev.p + R.off[2]);
  A->wr = b->sp_wr.p;
  A->out = out_dev;
  A->skipped = b->sp_skipped.p;
  A->h = h;
  A->n = (uint32_t)n;
  A->n_runs = (uint32_t)R.items.size();
  return MGF_OK;
}

// The launches of a call, behind every check (n > 0).
static mgf_status batch_spring_run(mgf_batch* b, float h, float* out_dev) {
  hipStream_t s = b->ctx->stream;
  MGF_TRY(batch_push(b));
  BatchSpringArgs A;
  MGF_TRY(batch_spring_ready(b, h, out_dev, &A));
  k_batch_spring_wrench<<<batch_dev_blocks(A.n), kBatchBlock, 0, s>>>(A);
  LAUNCH_CHECK();
  k_batch_spring_apply<false><<<batch_dev_blocks(A.n_runs), kBatchBlock, 0, s>>>(A);
  LAUNCH_CHECK();
  b->d_launches += MGF_BATCH_SPRING_LAUNCHES;
  return MGF_OK;
}

// the refusals of both apply calls that need no device
static mgf_status batch_spring_args(const mgf_batch* b, float h) {
  MGF_TRY(batch_rig_handle(b));
  if (!std::isfinite(h)) return fail(MGF_ERR_INVALID, "h is not finite");
  return MGF_OK;
}

extern "C" mgf_status mgf_batch_apply_springs(mgf_batch* b, float h, float* wrench_out) {
  MGF_TRY(batch_spring_args(b, h));
  MGF_TRY(ctx_bind(b->ctx));
  b->d_launches = 0;
  const size_t n = b->springs.recs.size();
  if (n == 0) return MGF_OK;
  hipStream_t s = b->ctx->stream;
  MGF_TRY(batch_spring_run(b, h, nullptr));
  if (wrench_out) MGF_HIP_TRY(hipMemcpyAsync(wrench_out, b->sp_wr.p, 48 * n, hipMemcpyDeviceToHost, s));  // (the handle's buffer holds every wrench)
  MGF_HIP_TRY(hipStreamSynchronize(s));
  return MGF_OK;
}

extern "C" mgf_status mgf_batch_apply_springs_dev(mgf_batch* b, float h, float* wrench_out_dev) {
  MGF_TRY(batch_spring_args(b, h));
  MGF_TRY(ctx_bind(b->ctx));
  b->d_launches = 0;
  const size_t n = b->springs.recs.size();
  MGF_TRY(dev_span(b->ctx, wrench_out_dev, 48 * n, "wrench_out_dev"));
  if (n == 0) return MGF_OK;
  return batch_spring_run(b, h, wrench_out_dev);
}
