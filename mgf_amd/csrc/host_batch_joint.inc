// The joint rigs of a batch - ball joints, hinges, sliders: what the three share, written once, and behind it the ball joints' own calls
// (mgf_batch_set_joints, mgf_batch_joint_count, mgf_batch_solve_joints, mgf_batch_solve_joints_dev).  Part of the single translation
// unit mgf_hip.hip (included there, in order, behind host_batch_spring.inc and ahead of host_batch_hinge.inc and
// host_batch_slider.inc); not compiled on its own.
//
// A joint makes the velocities of two bodies agree where a spring is an explicit force that needs a stiffness the time step cannot
// carry: sequential impulses over the velocities resident on the device, `iters` sweeps over a world's joints in list order
// (k_batch_joint_loop.h).  What a joint rig shares with the other rigs is host_batch_rig.inc's: the prologue and the world / body check
// of the set call, the upload - items | records | plan and slots, ONE copy (batch_rig_up) - and the check of `body` against the
// lengths that go up with it; `other` is held against them here, ahead of it.
// The plan: the joints sorted by world - stable, a world's joints stay in list order - and cut into items of one world, a workgroup
// each; a world's named bodies numbered as local slots in the order the list first names them (`body` ahead of `other`); per joint
// its two slots and its rank in each body's chain of joints, per slot the body and the chain's length.  Nothing is sorted or scanned
// on the device.
// A KIND (JointKind below, HingeKind, SliderKind in their files) names what differs: the record, the kernel's Rows - whose kFloats is
// the impulse row - the word of the messages, whether the motors have a target table, the launch constants, the handle's member and
// the kernel pair.  The target table is W[rows][count] in device memory: a solve call names the row it reads, a rollout's tick t reads
// row min(t, rows - 1); setting the rig makes it one row of zeros.
// A solve is T::launches = 1 launch ("drive_launches") whatever the joints and the worlds.  Nothing here reads a shape, so a batch with
// bodies of several components is not refused.  The device forms make no host wait and no copy between host and device; the host form
// of a solve downloads the impulses where asked and waits once.
// A rollout (host_batch_rollout.inc) takes the same launch into the step's train between the actuation and the tick, ball joints, then
// hinges, then sliders: batch_joint_ready fills a kind's hook, batch_step_run (host_batch.inc) calls batch_joint_pass for every pass and
// batch_joint_tick for every tick.

static mgf_status batch_joint_fail(mgf_status s, const char* fmt, const char* word) { set_error(fmt, word); return s; }
// the set calls' tests of a record's axes, in double: a unit length, a dot product
static bool joint_unit(double a) { return std::fabs(a - 1.0) <= 1e-3; }
static double joint_dot(const mgf_vec3& a, const mgf_vec3& b) { return (double)a.x * b.x + (double)a.y * b.y + (double)a.z * b.z; }

// The records become the rig: reached only behind every check of every record - this is the first change of the rig.  R.items holds the
// worlds' items: (world, first sorted position, count | slots << 16, first slot); R.order four words a sorted position - (the caller's
// index, slot_a | slot_b << 16, rank_a | rank_b << 16, 0) - and behind them two words a slot: (body, deg).  The target table becomes one
// row of zeros, made where the rig goes up.  No device is needed.  The plan reads a record's world, body and other alone.
template <class Rec>
static void batch_joint_plan(BatchJointRig<Rec>& R, const Rec* recs, size_t n) {
  std::vector<uint32_t> sorted(n);
  for (size_t i = 0; i < n; ++i) sorted[i] = (uint32_t)i;
  std::stable_sort(sorted.begin(), sorted.end(), [&](uint32_t l, uint32_t r) { return recs[l].world < recs[r].world; });
  std::vector<uint4> items;
  std::vector<uint32_t> plan(4 * n), slots;
  std::vector<uint32_t> slot_of(MGF_BATCH_MAX_BODIES, kJointNoSlot);  // of the item at hand: body -> slot
  size_t first_slot = 0;
  auto slot = [&](int32_t body) {
    uint32_t& s = slot_of[(size_t)body];
    if (s == kJointNoSlot) {
      s = (uint32_t)(slots.size() / 2 - first_slot);
      slots.push_back((uint32_t)body);
      slots.push_back(0u);
    }
    const uint32_t rank = slots[2 * (first_slot + s) + 1]++;  // the chain so far: this joint's rank in it
    return std::make_pair(s, rank);
  };
  for (size_t p = 0; p < n; ++p) {
    const Rec& r = recs[sorted[p]];
    if (p == 0 || r.world != recs[sorted[p - 1]].world) {
      std::fill(slot_of.begin(), slot_of.end(), kJointNoSlot);
      first_slot = slots.size() / 2;
      items.push_back(make_uint4((uint32_t)r.world, (uint32_t)p, 0u, (uint32_t)first_slot));
    }
    const auto a = slot(r.body);
    const auto b = r.other >= 0 ? slot(r.other) : std::make_pair(kJointNoSlot, 0u);
    plan[4 * p] = sorted[p];
    plan[4 * p + 1] = a.first | (b.first << 16);
    plan[4 * p + 2] = a.second | (b.second << 16);
    plan[4 * p + 3] = 0u;
    items.back().z = (uint32_t)(p - items.back().y + 1) | ((uint32_t)(slots.size() / 2 - first_slot) << 16);
  }
  plan.insert(plan.end(), slots.begin(), slots.end());
  R.recs.assign(recs, recs + n);
  R.items.swap(items);
  R.order.swap(plan);
  R.stale = true;
  R.rows = 1;
  R.zero = true;
}

// the set call's check of a record's far end, behind batch_rig_ref_check
template <class T>
static mgf_status batch_joint_other_check(const mgf_batch* b, const typename T::Rec& r) {
  if (r.other < -1 || (r.other >= 0 && (uint32_t)r.other >= b->h_n[(size_t)r.world]))
    return batch_joint_fail(MGF_ERR_INVALID, "a %s's other is neither -1 nor a body of its world: the rig was not changed", T::word);
  if (r.other == r.body) return batch_joint_fail(MGF_ERR_INVALID, "a %s's other is its body: the rig was not changed", T::word);
  return MGF_OK;
}

// a rig that goes up behind added bodies: the far ends against the lengths that go up, as batch_rig_up holds `body`
template <class T>
static mgf_status batch_joint_far_ends(const mgf_batch* b) {
  const auto& R = b->*T::rig;
  if (R.stale)
    for (size_t i = 0; i < R.recs.size(); ++i)
      if (R.recs[i].other >= 0 && (uint32_t)R.recs[i].other >= b->h_n[(size_t)R.recs[i].world])
        return batch_joint_fail(MGF_ERR_INVALID, "internal error: a %s's other is outside its world", T::word);
  return MGF_OK;
}

// What the kernel reads of the handle, as it is now: a rollout's train looks it up again for every pass, as the other hooks' views are.
template <class T>
static void batch_joint_view(const mgf_batch* b, BatchJointArgs* A) {
  const auto& R = b->*T::rig;
  A->B = b->bodies(0);
  A->w_off = b->d_off.p;
  A->items = reinterpret_cast<const uint4*>(R.dev.p);
  A->rig = R.dev.p + R.off[1];
  A->plan = reinterpret_cast<const uint4*>(R.dev.p + R.off[2]);
  A->slots = reinterpret_cast<const uint2*>(R.dev.p + R.off[2] + R.recs.size());  // (behind the plan's n words of 16 bytes)
  A->acc = R.acc.p;
  A->skipped = R.skipped.p;
  A->err = b->d_err.p;
}

// What the launch reads, behind batch_push (n > 0): the rig up, the target table where the kind has one, the handle's impulse buffer
// and skip counter there.  `out_dev`: device memory of kFloats n floats or null.  Shared with the rollouts, whose train fills done, act,
// tick and the table's row in (A->w is row 0 here).  *lds: the launch's dynamic LDS.
template <class T>
static mgf_status batch_joint_ready(mgf_batch* b, float h, int32_t iters, float* out_dev, BatchJointArgs* A, uint32_t* lds) {
  static_assert(sizeof(typename T::Rec) == 16 * T::Rows::kWords, "the rig goes up as the caller's records: the kernel's words of 16 bytes");
  auto& R = b->*T::rig;
  hipStream_t s = b->ctx->stream;
  const size_t n = R.recs.size();
  MGF_TRY(batch_joint_far_ends<T>(b));
  MGF_TRY(batch_rig_up(b, R, T::word, 3));
  if (T::table && R.zero) {  // (the rig was set behind the last table: one row of zeros)
    MGF_TRY(R.w.ensure(n, s));
    MGF_HIP_TRY(hipMemsetAsync(R.w.p, 0, 4 * n, s));
    R.rows = 1;
    R.zero = false;
  }
  MGF_TRY(R.acc.ensure(T::Rows::kFloats * n, s));
  if (!R.skipped.p) {
    MGF_TRY(R.skipped.ensure(1, s));
    MGF_HIP_TRY(hipMemsetAsync(R.skipped.p, 0, sizeof(unsigned long long), s));
  }
  memset(A, 0, sizeof(*A));
  batch_joint_view<T>(b, A);
  A->w = R.w.p;  // (null: the ball joints')
  A->out = out_dev;
  A->h = h;
  A->iters = (uint32_t)iters;
  uint32_t most = 0;
  for (const uint4& it : R.items) most = std::max(most, it.z >> 16);
  *lds = 36u * most;  // 32 bytes a slot of (v, omega), one progress word
  return MGF_OK;
}

// The launch of a call, behind every check (n > 0, iters > 0, row inside the table).
template <class T>
static mgf_status batch_joint_run(mgf_batch* b, float h, int32_t iters, int64_t row, float* out_dev) {
  auto& R = b->*T::rig;
  MGF_TRY(batch_push(b));
  BatchJointArgs A;
  uint32_t lds = 0;
  MGF_TRY(batch_joint_ready<T>(b, h, iters, out_dev, &A, &lds));
  if (T::table) A.w = R.w.p + (size_t)row * R.recs.size();
  T::template launch<false><<<(unsigned)R.items.size(), kBatchBlock, lds, b->ctx->stream>>>(A);
  LAUNCH_CHECK();
  b->d_launches += T::launches;
  return MGF_OK;
}

// the refusals of both solve calls that need no device; `row` is 0 where the kind has no table
template <class T>
static mgf_status batch_joint_args(const mgf_batch* b, float h, int32_t iters, int64_t row) {
  MGF_TRY(batch_rig_handle(b));
  if (!std::isfinite(h)) return fail(MGF_ERR_INVALID, "h is not finite");
  if (iters < 0) return fail(MGF_ERR_INVALID, "iters is negative");
  if (row < 0 || row >= (b->*T::rig).rows) return fail(MGF_ERR_INVALID, "row is outside the target table");
  return MGF_OK;
}

// mgf_batch_solve_joints, _hinges, _sliders
template <class T>
static mgf_status batch_joint_solve(mgf_batch* b, float h, int32_t iters, int64_t row, float* impulse_out) {
  MGF_TRY(batch_joint_args<T>(b, h, iters, row));
  MGF_TRY(ctx_bind(b->ctx));
  b->d_launches = 0;
  const auto& R = b->*T::rig;
  const size_t n = R.recs.size();
  if (n == 0 || iters == 0) return MGF_OK;
  hipStream_t s = b->ctx->stream;
  MGF_TRY(batch_joint_run<T>(b, h, iters, row, nullptr));
  uint32_t gave_up = 0;
  if (impulse_out) MGF_HIP_TRY(hipMemcpyAsync(impulse_out, R.acc.p, 4 * T::Rows::kFloats * n, hipMemcpyDeviceToHost, s));  // (the handle's buffer holds every impulse)
  MGF_HIP_TRY(hipMemcpyAsync(&gave_up, b->d_err.p + 1, 4, hipMemcpyDeviceToHost, s));
  MGF_HIP_TRY(hipStreamSynchronize(s));
  if (gave_up) return batch_joint_fail(MGF_ERR_HIP, "internal error: a lane of the %s solver gave up waiting for its turn", T::word);
  return MGF_OK;
}

// mgf_batch_solve_joints_dev, _hinges_dev, _sliders_dev
template <class T>
static mgf_status batch_joint_solve_dev(mgf_batch* b, float h, int32_t iters, int64_t row, float* impulse_out_dev) {
  MGF_TRY(batch_joint_args<T>(b, h, iters, row));
  MGF_TRY(ctx_bind(b->ctx));
  b->d_launches = 0;
  const size_t n = (b->*T::rig).recs.size();
  MGF_TRY(dev_span(b->ctx, impulse_out_dev, 4 * T::Rows::kFloats * n, "impulse_out_dev"));
  if (n == 0 || iters == 0) return MGF_OK;
  return batch_joint_run<T>(b, h, iters, row, impulse_out_dev);
}

// the refusals of both target calls that need no device
template <class T>
static mgf_status batch_joint_target_args(const mgf_batch* b, const float* w, int64_t rows) {
  MGF_TRY(batch_rig_handle(b));
  if (rows < 1 || rows > (1 << 20)) return fail(MGF_ERR_INVALID, "rows must be in [1, 2^20]");
  const size_t n = (b->*T::rig).recs.size();
  if (!w && n > 0) return fail(MGF_ERR_INVALID, "NULL argument: w");
  if ((uint64_t)n > (uint64_t)INT64_MAX / 4u / (uint64_t)rows) return batch_joint_fail(MGF_ERR_INVALID, "4 * rows * mgf_batch_%s_count overflows int64_t", T::word);
  return MGF_OK;
}

// mgf_batch_set_hinge_targets, _slider_targets and their device forms: the table taken into the handle's memory, `kind` says where w lies
template <class T>
static mgf_status batch_joint_targets(mgf_batch* b, const float* w, int64_t rows, hipMemcpyKind kind) {
  MGF_TRY(batch_joint_target_args<T>(b, w, rows));
  MGF_TRY(ctx_bind(b->ctx));
  auto& R = b->*T::rig;
  hipStream_t s = b->ctx->stream;
  const size_t words = (size_t)rows * R.recs.size();
  if (kind == hipMemcpyDeviceToDevice) MGF_TRY(dev_span(b->ctx, w, 4 * words, "w_dev"));
  if (words) {
    MGF_TRY(R.w.ensure(words, s));
    MGF_HIP_TRY(hipMemcpyAsync(R.w.p, w, 4 * words, kind, s));
    if (kind == hipMemcpyHostToDevice) MGF_HIP_TRY(hipStreamSynchronize(s));  // (the caller's array is his again when the call returns)
  }
  R.rows = rows;
  R.zero = false;
  return MGF_OK;
}

// A kind's hook for a rollout, behind batch_push: on where its rig is not empty and iters > 0 (iters == 0: the solve calls enqueue nothing)
template <class T>
static mgf_status batch_joint_hook(mgf_batch* b, float h, int32_t iters, BatchJointHook* H) {
  if ((b->*T::rig).recs.empty() || iters <= 0) return MGF_OK;
  MGF_TRY(batch_joint_ready<T>(b, h, iters, nullptr, &H->A, &H->lds));
  H->on = true;
  return MGF_OK;
}

// A kind's part of the step's train (batch_step_run, host_batch.inc), where its hook is on.  Every pass: what the kernel reads of the
// handle, looked up again.
template <class T>
static void batch_joint_pass(const mgf_batch* b, BatchJointHook& H) {
  if (!H.on) return;
  batch_joint_view<T>(b, &H.A);
  H.A.done = b->d_done.p; H.A.act = b->d_act.p;
}

// Every tick: the launch, behind every external impulse and just ahead of the integration, under the springs' gate - `act` moves behind
// the tick; tick t reads the target table's row min(t, rows - 1).
template <class T>
static mgf_status batch_joint_tick(mgf_batch* b, BatchJointHook& H, uint32_t t, int64_t* launches) {
  if (!H.on) return MGF_OK;
  const auto& R = b->*T::rig;
  H.A.tick = t;
  if (T::table) H.A.w = R.w.p + (size_t)std::min<int64_t>((int64_t)t, R.rows - 1) * R.recs.size();
  T::template launch<true><<<(unsigned)R.items.size(), kBatchBlock, H.lds, b->ctx->stream>>>(H.A);
  LAUNCH_CHECK();
  *launches += T::per_tick;
  return MGF_OK;
}

// ---- the ball joints: the eighth rig, the spring's hard counterpart ----

struct JointKind {
  using Rec = mgf_batch_joint;
  using Rows = JointRows;
  static constexpr const char* word = "joint";
  static constexpr bool table = false;
  static constexpr int64_t launches = MGF_BATCH_JOINT_LAUNCHES, per_tick = MGF_BATCH_ROLLOUT_JOINT_LAUNCHES_PER_TICK;
  static constexpr BatchJointRig<Rec> mgf_batch::*rig = &mgf_batch::joints;
  template <bool GATED>
  static constexpr auto launch = k_batch_joint_solve<GATED>;
};

extern "C" mgf_status mgf_batch_set_joints(mgf_batch* b, const mgf_batch_joint* j, int64_t n_in) {
  MGF_TRY(batch_rig_set_args(b, j, n_in));
  static_assert(MGF_BATCH_MAX_WORLD_JOINTS == kBatchBlock, "k_batch_joint_solve has a lane per joint of a world");
  const size_t n = (size_t)n_in;
  std::vector<uint32_t> per_world(n ? b->K : 0, 0u);
  for (size_t i = 0; i < n; ++i) {
    const mgf_batch_joint& r = j[i];
    MGF_TRY(batch_rig_ref_check(b, r.world, r.body, 0, "joint"));  // (the flag word is this rig's own: below)
    MGF_TRY(batch_joint_other_check<JointKind>(b, r));
    if (r.flags != 0u || r.pad != 0.0f) return fail(MGF_ERR_INVALID, "a joint's flags or pad are not 0: the rig was not changed");
    if (!actuator_finite3(r.pa) || !actuator_finite3(r.pb)) return fail(MGF_ERR_INVALID, "a joint's pa or pb is not finite: the rig was not changed");
    if (!std::isfinite(r.beta) || r.beta < 0.0f || r.beta > 1.0f) return fail(MGF_ERR_INVALID, "a joint's beta is not in [0, 1]: the rig was not changed");
    if (++per_world[(size_t)r.world] > MGF_BATCH_MAX_WORLD_JOINTS)
      return fail(MGF_ERR_INVALID, "a world holds at most MGF_BATCH_MAX_WORLD_JOINTS (256) joints: the rig was not changed");
  }
  batch_joint_plan(b->joints, j, n);
  return MGF_OK;
}

extern "C" int64_t mgf_batch_joint_count(const mgf_batch* b) { return b ? (int64_t)b->joints.recs.size() : -1; }
extern "C" mgf_status mgf_batch_solve_joints(mgf_batch* b, float h, int32_t iters, float* impulse_out) { return batch_joint_solve<JointKind>(b, h, iters, 0, impulse_out); }
extern "C" mgf_status mgf_batch_solve_joints_dev(mgf_batch* b, float h, int32_t iters, float* impulse_out_dev) {
  return batch_joint_solve_dev<JointKind>(b, h, iters, 0, impulse_out_dev);
}
