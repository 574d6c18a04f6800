// mgf_batch_set_hinges, mgf_batch_hinge_count, mgf_batch_set_hinge_targets, mgf_batch_set_hinge_targets_dev, mgf_batch_solve_hinges,
// mgf_batch_solve_hinges_dev: hinge (revolute) joints between two bodies of a world, or between one and the world - a ball joint, two
// angular rows that keep the axes parallel, an optional limit of the hinge angle and an optional velocity motor with a torque cap -
// solved by sequential impulses over the velocities resident on the device (k_batch_hinge.h).  Part of the single translation unit
// mgf_hip.hip (included there, in order, behind host_batch_joint.inc); not compiled on its own.
//
// The ninth rig.  Every step but the checks of a record is the joint rigs' (host_batch_joint.inc), under HingeKind: the plan, the
// target table, the upload, the launch - MGF_BATCH_HINGE_LAUNCHES = 1 - and a rollout's launch behind the ball joints' and ahead of the
// tick.

struct HingeKind {
  using Rec = mgf_batch_hinge;
  using Rows = HingeRows;
  static constexpr const char* word = "hinge";
  static constexpr bool table = true;
  static constexpr int64_t launches = MGF_BATCH_HINGE_LAUNCHES, per_tick = MGF_BATCH_ROLLOUT_HINGE_LAUNCHES_PER_TICK;
  static constexpr BatchJointRig<Rec> mgf_batch::*rig = &mgf_batch::hinges;
  template <bool GATED>
  static constexpr auto launch = k_batch_hinge_solve<GATED>;
  // the kind's encoders (host_batch_joint_read.inc)
  using Reading = mgf_hinge_reading;
  static constexpr BatchJointTrace mgf_batch::*trace = &mgf_batch::hinge_trace;
  static constexpr const char* caps = "HINGE";
  static constexpr int64_t read_launches = MGF_BATCH_HINGE_READ_LAUNCHES, read_per_tick = MGF_BATCH_ROLLOUT_HINGE_READ_LAUNCHES_PER_TICK;
  static constexpr int32_t trace_reading = MGF_HINGE_TRACE_READING, trace_full = MGF_HINGE_TRACE_FULL;
  template <bool GATED, int FORMAT>
  static constexpr auto read = k_batch_read_hinges<GATED, FORMAT>;
};

extern "C" mgf_status mgf_batch_set_hinges(mgf_batch* b, const mgf_batch_hinge* j, int64_t n_in) {
  MGF_TRY(batch_rig_set_args(b, j, n_in));
  static_assert(MGF_BATCH_MAX_WORLD_HINGES == kBatchBlock, "k_batch_hinge_solve has a lane per hinge of a world");
  static_assert(MGF_HINGE_LIMIT == kHingeLimit && MGF_HINGE_MOTOR == kHingeMotor, "the kernel's flag bits are the header's");
  const size_t n = (size_t)n_in;
  std::vector<uint32_t> per_world(n ? b->K : 0, 0u);
  for (size_t i = 0; i < n; ++i) {
    const mgf_batch_hinge& r = j[i];
    MGF_TRY(batch_rig_ref_check(b, r.world, r.body, 0, "hinge"));  // (the flag word is this rig's own: below)
    MGF_TRY(batch_joint_other_check<HingeKind>(b, r));
    if (r.flags & ~(uint32_t)(MGF_HINGE_LIMIT | MGF_HINGE_MOTOR))
      return fail(MGF_ERR_INVALID, "a hinge's flags hold a bit beyond MGF_HINGE_LIMIT | MGF_HINGE_MOTOR: the rig was not changed");
    if (!actuator_finite3(r.pa) || !actuator_finite3(r.pb) || !actuator_finite3(r.ax) || !actuator_finite3(r.ua) || !actuator_finite3(r.bx) ||
        !actuator_finite3(r.ub) || !std::isfinite(r.beta) || std::isnan(r.tmax) || r.tmax == -INFINITY || !std::isfinite(r.cm) || !std::isfinite(r.sm) ||
        !std::isfinite(r.ch) || !std::isfinite(r.sh))
      return fail(MGF_ERR_INVALID, "a word of a hinge is not finite (tmax may be +inf): the rig was not changed");
    if (r.beta < 0.0f || r.beta > 1.0f) return fail(MGF_ERR_INVALID, "a hinge's beta is not in [0, 1]: the rig was not changed");
    if (r.tmax < 0.0f) return fail(MGF_ERR_INVALID, "a hinge's tmax is negative: the rig was not changed");
    if (!joint_unit(joint_dot(r.ax, r.ax)) || !joint_unit(joint_dot(r.ua, r.ua)) || !joint_unit(joint_dot(r.bx, r.bx)) || !joint_unit(joint_dot(r.ub, r.ub)) ||
        !joint_unit((double)r.cm * r.cm + (double)r.sm * r.sm) || !joint_unit((double)r.ch * r.ch + (double)r.sh * r.sh))
      return fail(MGF_ERR_INVALID, "a hinge's ax, ua, bx, ub, (cm, sm) or (ch, sh) is not of unit length: the rig was not changed");
    if (std::fabs(joint_dot(r.ax, r.ua)) > 1e-3 || std::fabs(joint_dot(r.bx, r.ub)) > 1e-3)
      return fail(MGF_ERR_INVALID, "a hinge's reference is not perpendicular to its axis: the rig was not changed");
    if (r.sh < 0.0f) return fail(MGF_ERR_INVALID, "a hinge's sh is negative: the rig was not changed");
    if (++per_world[(size_t)r.world] > MGF_BATCH_MAX_WORLD_HINGES)
      return fail(MGF_ERR_INVALID, "a world holds at most MGF_BATCH_MAX_WORLD_HINGES (256) hinges: the rig was not changed");
  }
  batch_joint_plan(b->hinges, j, n);
  b->hinge_trace.rows = 0;  // (the readings table is rows of the OLD rig's hinges: the trace is off until mgf_batch_set_hinge_trace names it again)
  return MGF_OK;
}

extern "C" int64_t mgf_batch_hinge_count(const mgf_batch* b) { return b ? (int64_t)b->hinges.recs.size() : -1; }
extern "C" mgf_status mgf_batch_set_hinge_targets(mgf_batch* b, const float* w, int64_t rows) { return batch_joint_targets<HingeKind>(b, w, rows, hipMemcpyHostToDevice); }
extern "C" mgf_status mgf_batch_set_hinge_targets_dev(mgf_batch* b, const float* w_dev, int64_t rows) {
  return batch_joint_targets<HingeKind>(b, w_dev, rows, hipMemcpyDeviceToDevice);
}
extern "C" mgf_status mgf_batch_solve_hinges(mgf_batch* b, float h, int32_t iters, int64_t row, float* impulse_out) {
  return batch_joint_solve<HingeKind>(b, h, iters, row, impulse_out);
}
extern "C" mgf_status mgf_batch_solve_hinges_dev(mgf_batch* b, float h, int32_t iters, int64_t row, float* impulse_out_dev) {
  return batch_joint_solve_dev<HingeKind>(b, h, iters, row, impulse_out_dev);
}
