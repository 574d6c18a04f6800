// mgf_batch_set_sliders, mgf_batch_slider_count, mgf_batch_set_slider_targets, mgf_batch_set_slider_targets_dev, mgf_batch_solve_sliders,
// mgf_batch_solve_sliders_dev: slider (prismatic) joints between two bodies of a world, or between one and the world - three angular
// rows that hold other's frame onto body's, two linear rows that hold other's anchor on the axis through body's, and along the axis an
// optional limit of the travel, an optional velocity motor with a force cap, or a lock (a weld) - solved by sequential impulses over
// the velocities resident on the device (k_batch_slider.h).  Part of the single translation unit mgf_hip.hip (included there, in
// order, behind host_batch_hinge.inc); not compiled on its own.
//
// The tenth rig.  Every step but the checks of a record is the joint rigs' (host_batch_joint.inc), under SliderKind: the plan, the
// target table, the upload, the launch - MGF_BATCH_SLIDER_LAUNCHES = 1 - and a rollout's launch behind the hinges' and ahead of the
// tick.

struct SliderKind {
  using Rec = mgf_batch_slider;
  using Rows = SliderRows;
  static constexpr const char* word = "slider";
  static constexpr bool table = true;
  static constexpr int64_t launches = MGF_BATCH_SLIDER_LAUNCHES, per_tick = MGF_BATCH_ROLLOUT_SLIDER_LAUNCHES_PER_TICK;
  static constexpr BatchJointRig<Rec> mgf_batch::*rig = &mgf_batch::sliders;
  template <bool GATED>
  static constexpr auto launch = k_batch_slider_solve<GATED>;
  // the kind's encoders (host_batch_joint_read.inc)
  using Reading = mgf_slider_reading;
  static constexpr BatchJointTrace mgf_batch::*trace = &mgf_batch::slider_trace;
  static constexpr const char* caps = "SLIDER";
  static constexpr int64_t read_launches = MGF_BATCH_SLIDER_READ_LAUNCHES, read_per_tick = MGF_BATCH_ROLLOUT_SLIDER_READ_LAUNCHES_PER_TICK;
  static constexpr int32_t trace_reading = MGF_SLIDER_TRACE_READING, trace_full = MGF_SLIDER_TRACE_FULL;
  template <bool GATED, int FORMAT>
  static constexpr auto read = k_batch_read_sliders<GATED, FORMAT>;
};

extern "C" mgf_status mgf_batch_set_sliders(mgf_batch* b, const mgf_batch_slider* j, int64_t n_in) {
  MGF_TRY(batch_rig_set_args(b, j, n_in));
  static_assert(MGF_BATCH_MAX_WORLD_SLIDERS == kBatchBlock, "k_batch_slider_solve has a lane per slider of a world");
  static_assert(MGF_SLIDER_LIMIT == kSliderLimit && MGF_SLIDER_MOTOR == kSliderMotor && MGF_SLIDER_LOCK == kSliderLock, "the kernel's flag bits are the header's");
  const size_t n = (size_t)n_in;
  std::vector<uint32_t> per_world(n ? b->K : 0, 0u);
  for (size_t i = 0; i < n; ++i) {
    const mgf_batch_slider& r = j[i];
    MGF_TRY(batch_rig_ref_check(b, r.world, r.body, 0, "slider"));  // (the flag word is this rig's own: below)
    MGF_TRY(batch_joint_other_check<SliderKind>(b, r));
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
    if (!joint_unit(joint_dot(r.ax, r.ax)) || !joint_unit(joint_dot(r.ua, r.ua)) || !joint_unit(joint_dot(r.bx, r.bx)) || !joint_unit(joint_dot(r.ub, r.ub)))
      return fail(MGF_ERR_INVALID, "a slider's ax, ua, bx or ub is not of unit length: the rig was not changed");
    if (std::fabs(joint_dot(r.ax, r.ua)) > 1e-3 || std::fabs(joint_dot(r.bx, r.ub)) > 1e-3)
      return fail(MGF_ERR_INVALID, "a slider's reference is not perpendicular to its axis: the rig was not changed");
    if (++per_world[(size_t)r.world] > MGF_BATCH_MAX_WORLD_SLIDERS)
      return fail(MGF_ERR_INVALID, "a world holds at most MGF_BATCH_MAX_WORLD_SLIDERS (256) sliders: the rig was not changed");
  }
  batch_joint_plan(b->sliders, j, n);
  b->slider_trace.rows = 0;  // (the readings table is rows of the OLD rig's sliders: the trace is off until mgf_batch_set_slider_trace names it again)
  return MGF_OK;
}

extern "C" int64_t mgf_batch_slider_count(const mgf_batch* b) { return b ? (int64_t)b->sliders.recs.size() : -1; }
extern "C" mgf_status mgf_batch_set_slider_targets(mgf_batch* b, const float* w, int64_t rows) { return batch_joint_targets<SliderKind>(b, w, rows, hipMemcpyHostToDevice); }
extern "C" mgf_status mgf_batch_set_slider_targets_dev(mgf_batch* b, const float* w_dev, int64_t rows) {
  return batch_joint_targets<SliderKind>(b, w_dev, rows, hipMemcpyDeviceToDevice);
}
extern "C" mgf_status mgf_batch_solve_sliders(mgf_batch* b, float h, int32_t iters, int64_t row, float* impulse_out) {
  return batch_joint_solve<SliderKind>(b, h, iters, row, impulse_out);
}
extern "C" mgf_status mgf_batch_solve_sliders_dev(mgf_batch* b, float h, int32_t iters, int64_t row, float* impulse_out_dev) {
  return batch_joint_solve_dev<SliderKind>(b, h, iters, row, impulse_out_dev);
}
