// mgf_batch_set_actuators, mgf_batch_actuator_count, mgf_batch_actuate, mgf_batch_actuate_dev: actuators - a direction and an arm fixed
// in the frame of a body, with a gain and a clamp - turned into wrenches from the poses resident on the device and applied there
// (k_batch_actuator.h).  Part of the single translation unit mgf_hip.hip (included there, in order, behind host_batch_feeler.inc); not
// compiled on its own.
//
// The sixth rig, and the first on the action side: what mgf_batch_apply_impulses answers for wrenches a caller assembles from
// gather_state every tick - directions and arms turned by q, a cross product, a sum per body - an actuator answers from the rig, the
// resident q and one control value.  What the rig shares with the others is host_batch_rig.inc's: the prologue and the world / body
// check of the set call, the upload - runs | records | order, ONE copy (batch_rig_up) - and the check of the bodies against the lengths
// that go up with it.  The plan is this rig's own: the others sort by world and cut into work items of a workgroup, this one sorts by
// (world, body) - stable, a body's actuators stay in the caller's order - and cuts into runs of one body, a lane each.  A run names
// (world, body), not a flat index: bodies added to an earlier world move the body, and the kernel finds it through the worlds' offsets.
// A call is MGF_BATCH_ACTUATOR_LAUNCHES = 1 launch ("drive_launches") whatever the actuators and the worlds; nothing here reads a shape,
// so a batch with bodies of several components is not refused (no batch_single_parts).  The device form makes no host wait and no
// copy between host and device; the host form uploads u, downloads the wrenches where asked, and waits once.
// The order of mgf_batch_actuate_dev is host_batch_query_dev.inc's: the refusals that need no device, the handle's own, EVERY device
// pointer looked up (dev_span), the overlap of the two arrays - and only then the first thing is enqueued.

static bool actuator_finite3(const mgf_vec3& v) { return std::isfinite(v.x) && std::isfinite(v.y) && std::isfinite(v.z); }

// The records become the rig, sorted by (world, body): reached only behind every check of every record - this is the first change of
// the rig.  R.items holds the runs: (world, body, first sorted position, count).  No device is needed.
static void batch_actuator_plan(BatchRig<mgf_batch_actuator>& R, const mgf_batch_actuator* recs, size_t n) {
  std::vector<uint32_t> order(n);
  for (size_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
  auto key = [&](uint32_t i) { return ((uint64_t)(uint32_t)recs[i].world << 32) | (uint32_t)recs[i].body; };
  std::stable_sort(order.begin(), order.end(), [&](uint32_t l, uint32_t r) { return key(l) < key(r); });
  std::vector<uint4> runs;
  for (size_t p = 0; p < n; ++p) {
    if (p == 0 || key(order[p]) != key(order[p - 1])) runs.push_back(make_uint4((uint32_t)recs[order[p]].world, (uint32_t)recs[order[p]].body, (uint32_t)p, 0u));
    ++runs.back().w;
  }
  R.recs.assign(recs, recs + n);
  R.items.swap(runs);
  R.order.swap(order);
  R.stale = true;
}

extern "C" mgf_status mgf_batch_set_actuators(mgf_batch* b, const mgf_batch_actuator* a, int64_t n_in) {
  MGF_TRY(batch_rig_set_args(b, a, n_in));
  static_assert(sizeof(mgf_batch_actuator) == 48, "the rig goes up as the caller's records: three words of 16 bytes");
  const size_t n = (size_t)n_in;
  for (size_t i = 0; i < n; ++i) {
    MGF_TRY(batch_rig_ref_check(b, a[i].world, a[i].body, 0, "actuator"));  // (the flag word is this rig's own: below)
    if (a[i].flags & ~(uint32_t)(MGF_ACTUATOR_TORQUE | MGF_ACTUATOR_WORLD_DIR))
      return fail(MGF_ERR_INVALID, "an actuator's flags hold a bit beyond MGF_ACTUATOR_WORLD_DIR: the rig was not changed");
    if (!actuator_finite3(a[i].p) || !actuator_finite3(a[i].d) || !std::isfinite(a[i].gain))
      return fail(MGF_ERR_INVALID, "an actuator's p, d or gain is not finite: the rig was not changed");
    if (std::isnan(a[i].lo) || std::isnan(a[i].hi) || a[i].lo > a[i].hi)
      return fail(MGF_ERR_INVALID, "an actuator's lo or hi is a NaN, or lo > hi: the rig was not changed");
  }
  batch_actuator_plan(b->actuators, a, n);
  return MGF_OK;
}

extern "C" int64_t mgf_batch_actuator_count(const mgf_batch* b) { return b ? (int64_t)b->actuators.recs.size() : -1; }

// The launch of a call, behind every check (n > 0): u_dev is device memory of n floats, out_dev of 6 n or null - the caller's or the
// handle's.
static mgf_status batch_actuator_run(mgf_batch* b, int32_t mode, const float* u_dev, float* out_dev) {
  BatchRig<mgf_batch_actuator>& R = b->actuators;
  hipStream_t s = b->ctx->stream;
  MGF_TRY(batch_push(b));
  MGF_TRY(batch_rig_up(b, R, "actuator", 3));
  if (!b->a_skipped.p) {
    MGF_TRY(b->a_skipped.ensure(1, s));
    MGF_HIP_TRY(hipMemsetAsync(b->a_skipped.p, 0, sizeof(unsigned long long), s));
  }
  BatchActuateArgs A;
  memset(&A, 0, sizeof(A));
  A.B = b->bodies(0);
  A.w_off = b->d_off.p;
  A.runs = reinterpret_cast<const uint4*>(R.dev.p);
  A.rig = R.dev.p + R.off[1];
  A.order = reinterpret_cast<const uint32_t*>(R.dev.p + R.off[2]);
  A.u = u_dev;
  A.out = out_dev;
  A.skipped = b->a_skipped.p;
  A.n_runs = (uint32_t)R.items.size();
  const unsigned blocks = batch_dev_blocks(R.items.size());
  if (mode == MGF_ACTUATE_IMPULSE) {
    if (out_dev) k_batch_actuate<ACTUATE_IMPULSE, true><<<blocks, kBatchBlock, 0, s>>>(A);
    else k_batch_actuate<ACTUATE_IMPULSE, false><<<blocks, kBatchBlock, 0, s>>>(A);
  } else {
    if (out_dev) k_batch_actuate<ACTUATE_FORCE, true><<<blocks, kBatchBlock, 0, s>>>(A);
    else k_batch_actuate<ACTUATE_FORCE, false><<<blocks, kBatchBlock, 0, s>>>(A);
  }
  LAUNCH_CHECK();
  b->d_launches += MGF_BATCH_ACTUATOR_LAUNCHES;
  return MGF_OK;
}

// the refusals of both apply calls that need no device; *count: the actuators of the rig
static mgf_status batch_actuator_args(const mgf_batch* b, const float* u, int64_t n, int32_t mode, size_t* count) {
  MGF_TRY(batch_rig_handle(b));
  if (n < 0) return fail(MGF_ERR_INVALID, "n is negative");
  if (mode != MGF_ACTUATE_IMPULSE && mode != MGF_ACTUATE_FORCE) return fail(MGF_ERR_INVALID, "mode is neither MGF_ACTUATE_IMPULSE nor MGF_ACTUATE_FORCE");
  *count = b->actuators.recs.size();
  if ((uint64_t)n != (uint64_t)*count) return fail(MGF_ERR_INVALID, "n is not mgf_batch_actuator_count: a control vector of another length than the rig");
  if (*count && !u) return fail(MGF_ERR_INVALID, "NULL argument");
  return MGF_OK;
}

extern "C" mgf_status mgf_batch_actuate(mgf_batch* b, const float* u, int64_t n_in, int32_t mode, float* wrench_out) {
  size_t n = 0;
  MGF_TRY(batch_actuator_args(b, u, n_in, mode, &n));
  MGF_TRY(ctx_bind(b->ctx));
  b->d_launches = 0;
  if (n == 0) return MGF_OK;
  hipStream_t s = b->ctx->stream;
  const size_t w_u = (n + 3) / 4, w_out = wrench_out ? (6 * n + 3) / 4 : 0;  // u | wrenches, each from a 16-byte boundary
  MGF_TRY(b->q_in.ensure(w_u + w_out, s));
  float* u_dev = reinterpret_cast<float*>(b->q_in.p);
  float* out_dev = wrench_out ? reinterpret_cast<float*>(b->q_in.p + w_u) : nullptr;
  MGF_HIP_TRY(hipMemcpyAsync(u_dev, u, 4 * n, hipMemcpyHostToDevice, s));
  MGF_TRY(batch_actuator_run(b, mode, u_dev, out_dev));
  if (wrench_out) MGF_HIP_TRY(hipMemcpyAsync(wrench_out, out_dev, 24 * n, hipMemcpyDeviceToHost, s));
  MGF_HIP_TRY(hipStreamSynchronize(s));  // (`u` is read by the copy until here)
  return MGF_OK;
}

extern "C" mgf_status mgf_batch_actuate_dev(mgf_batch* b, const float* u_dev, int64_t n_in, int32_t mode, float* wrench_out_dev) {
  size_t n = 0;
  MGF_TRY(batch_actuator_args(b, u_dev, n_in, mode, &n));
  MGF_TRY(ctx_bind(b->ctx));
  MGF_TRY(dev_span(b->ctx, u_dev, 4 * n, "u_dev"));
  MGF_TRY(dev_span(b->ctx, wrench_out_dev, 24 * n, "wrench_out_dev"));
  const DevBytes arrays[2] = {{wrench_out_dev, 24 * n, "wrench_out_dev"}, {u_dev, 4 * n, "u_dev"}};
  MGF_TRY(dev_outputs_overlap(arrays, 2, 1));
  b->d_launches = 0;
  if (n == 0) return MGF_OK;
  return batch_actuator_run(b, mode, u_dev, wrench_out_dev);
}
