// mgf_batch_set_joints, mgf_batch_joint_count, mgf_batch_solve_joints, mgf_batch_solve_joints_dev: point-to-point (ball) joints between
// two body-fixed points of a world, or between one and a point of the world, solved by sequential impulses over the velocities resident
// on the device (k_batch_joint.h).  Part of the single translation unit mgf_hip.hip (included there, in order, behind
// host_batch_spring.inc); not compiled on its own.
//
// The eighth rig, the spring's hard counterpart: where a spring is an explicit force that needs a stiffness the time step cannot carry
// to hold a limb on a torso, a joint makes the velocities of its two anchor points agree, `iters` sweeps over a world's joints in list
// order.  What the rig shares with the others is host_batch_rig.inc's: the prologue and the world / body check of the set call, the
// upload - items | records | plan and slots, ONE copy (batch_rig_up) - and the check of `body` against the lengths that go up with it;
// `other` is held against them here, ahead of it.
// The plan: the joints sorted by world - stable, a world's joints stay in list order - and cut into items of one world, a workgroup
// each; a world's jointed bodies numbered as local slots in the order the list first names them (`body` ahead of `other`); per joint
// its two slots and its rank in each body's chain of joints, per slot the body and the chain's length.  Nothing is sorted or scanned
// on the device.
// A call is MGF_BATCH_JOINT_LAUNCHES = 1 launch ("drive_launches") whatever the joints and the worlds.  Nothing here reads a shape, so a
// batch with bodies of several components is not refused.  The device form makes no host wait and no copy between host and device;
// the host form downloads the impulses where asked and waits once.
// A rollout (host_batch_rollout.inc) takes the same launch into the step's train between the actuation and the tick: batch_joint_ready
// fills the hook's arguments, batch_step_run (host_batch.inc) launches it.

// The records become the rig: reached only behind every check of every record - this is the first change of the rig.  R.items holds the
// worlds' items: (world, first sorted position, count | slots << 16, first slot); R.order four words a sorted position - (the caller's
// index, slot_a | slot_b << 16, rank_a | rank_b << 16, 0) - and behind them two words a slot: (body, deg).  No device is needed.
// Rec: mgf_batch_joint, or mgf_batch_hinge (host_batch_hinge.inc) - the plan reads a record's world, body and other alone.
template <class Rec>
static void batch_joint_plan(BatchRig<Rec>& R, const Rec* recs, size_t n) {
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
}

extern "C" mgf_status mgf_batch_set_joints(mgf_batch* b, const mgf_batch_joint* j, int64_t n_in) {
  MGF_TRY(batch_rig_set_args(b, j, n_in));
  static_assert(sizeof(mgf_batch_joint) == 48, "the rig goes up as the caller's records: three words of 16 bytes");
  static_assert(MGF_BATCH_MAX_WORLD_JOINTS == kBatchBlock, "k_batch_joint_solve has a lane per joint of a world");
  const size_t n = (size_t)n_in;
  std::vector<uint32_t> per_world(n ? b->K : 0, 0u);
  for (size_t i = 0; i < n; ++i) {
    const mgf_batch_joint& r = j[i];
    MGF_TRY(batch_rig_ref_check(b, r.world, r.body, 0, "joint"));  // (the flag word is this rig's own: below)
    if (r.other < -1 || (r.other >= 0 && (uint32_t)r.other >= b->h_n[(size_t)r.world]))
      return fail(MGF_ERR_INVALID, "a joint's other is neither -1 nor a body of its world: the rig was not changed");
    if (r.other == r.body) return fail(MGF_ERR_INVALID, "a joint's other is its body: the rig was not changed");
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

// What the kernel reads of the handle, as it is now: a rollout's train looks it up again for every pass, as the other hooks' views are.
static void batch_joint_view(const mgf_batch* b, BatchJointArgs* A) {
  const BatchRig<mgf_batch_joint>& R = b->joints;
  A->B = b->bodies(0);
  A->w_off = b->d_off.p;
  A->items = reinterpret_cast<const uint4*>(R.dev.p);
  A->rig = R.dev.p + R.off[1];
  A->plan = reinterpret_cast<const uint4*>(R.dev.p + R.off[2]);
  A->slots = reinterpret_cast<const uint2*>(R.dev.p + R.off[2] + R.recs.size());  // (behind the plan's n words of 16 bytes)
  A->acc = b->j_acc.p;
  A->skipped = b->j_skipped.p;
  A->err = b->d_err.p;
}

// What the launch reads, behind batch_push (n > 0): the rig up, the handle's impulse buffer and skip counter there.  `out_dev`: device
// memory of 3 n floats or null.  Shared with the rollouts, whose train fills done, act and tick in.  *lds: the launch's dynamic LDS.
static mgf_status batch_joint_ready(mgf_batch* b, float h, int32_t iters, float* out_dev, BatchJointArgs* A, uint32_t* lds) {
  BatchRig<mgf_batch_joint>& R = b->joints;
  hipStream_t s = b->ctx->stream;
  const size_t n = R.recs.size();
  if (R.stale)  // (bodies may have been added: the far ends against the lengths that go up, as batch_rig_up holds `body`)
    for (size_t i = 0; i < n; ++i)
      if (R.recs[i].other >= 0 && (uint32_t)R.recs[i].other >= b->h_n[(size_t)R.recs[i].world])
        return fail(MGF_ERR_INVALID, "internal error: a joint's other is outside its world");
  MGF_TRY(batch_rig_up(b, R, "joint", 3));
  MGF_TRY(b->j_acc.ensure(3 * n, s));
  if (!b->j_skipped.p) {
    MGF_TRY(b->j_skipped.ensure(1, s));
    MGF_HIP_TRY(hipMemsetAsync(b->j_skipped.p, 0, sizeof(unsigned long long), s));
  }
  memset(A, 0, sizeof(*A));
  batch_joint_view(b, A);
  A->out = out_dev;
  A->h = h;
  A->iters = (uint32_t)iters;
  uint32_t most = 0;
  for (const uint4& it : R.items) most = std::max(most, it.z >> 16);
  *lds = 36u * most;  // 32 bytes a slot of (v, omega), one progress word
  return MGF_OK;
}

// The launch of a call, behind every check (n > 0, iters > 0).
static mgf_status batch_joint_run(mgf_batch* b, float h, int32_t iters, float* out_dev) {
  hipStream_t s = b->ctx->stream;
  MGF_TRY(batch_push(b));
  BatchJointArgs A;
  uint32_t lds = 0;
  MGF_TRY(batch_joint_ready(b, h, iters, out_dev, &A, &lds));
  k_batch_joint_solve<false><<<(unsigned)b->joints.items.size(), kBatchBlock, lds, s>>>(A);
  LAUNCH_CHECK();
  b->d_launches += MGF_BATCH_JOINT_LAUNCHES;
  return MGF_OK;
}

// the refusals of both solve calls that need no device
static mgf_status batch_joint_args(const mgf_batch* b, float h, int32_t iters) {
  MGF_TRY(batch_rig_handle(b));
  if (!std::isfinite(h)) return fail(MGF_ERR_INVALID, "h is not finite");
  if (iters < 0) return fail(MGF_ERR_INVALID, "iters is negative");
  return MGF_OK;
}

extern "C" mgf_status mgf_batch_solve_joints(mgf_batch* b, float h, int32_t iters, float* impulse_out) {
  MGF_TRY(batch_joint_args(b, h, iters));
  MGF_TRY(ctx_bind(b->ctx));
  b->d_launches = 0;
  const size_t n = b->joints.recs.size();
  if (n == 0 || iters == 0) return MGF_OK;
  hipStream_t s = b->ctx->stream;
  MGF_TRY(batch_joint_run(b, h, iters, nullptr));
  uint32_t gave_up = 0;
  if (impulse_out) MGF_HIP_TRY(hipMemcpyAsync(impulse_out, b->j_acc.p, 12 * n, hipMemcpyDeviceToHost, s));  // (the handle's buffer holds every impulse)
  MGF_HIP_TRY(hipMemcpyAsync(&gave_up, b->d_err.p + 1, 4, hipMemcpyDeviceToHost, s));
  MGF_HIP_TRY(hipStreamSynchronize(s));
  if (gave_up) return fail(MGF_ERR_HIP, "internal error: a lane of the joint solver gave up waiting for its turn");
  return MGF_OK;
}

extern "C" mgf_status mgf_batch_solve_joints_dev(mgf_batch* b, float h, int32_t iters, float* impulse_out_dev) {
  MGF_TRY(batch_joint_args(b, h, iters));
  MGF_TRY(ctx_bind(b->ctx));
  b->d_launches = 0;
  const size_t n = b->joints.recs.size();
  MGF_TRY(dev_span(b->ctx, impulse_out_dev, 12 * n, "impulse_out_dev"));
  if (n == 0 || iters == 0) return MGF_OK;
  return batch_joint_run(b, h, iters, impulse_out_dev);
}
