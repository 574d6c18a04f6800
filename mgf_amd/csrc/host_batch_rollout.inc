// mgf_batch_rollout, mgf_batch_rollout_dev: n_ticks ticks of a batch with a row of controls applied ahead of every tick and a row of
// state written behind it - the loop  mgf_batch_actuate_dev(u[t]) | mgf_batch_step(1) | mgf_batch_gather_state_dev(row t)  in one call
// with the step's one host wait per pass (k_batch_rollout.h).  Part of the single translation unit mgf_hip.hip (included there, in
// order, behind host_batch_actuator.inc); not compiled on its own.
//
// The launch train is the step's own (batch_step_run, host_batch.inc) with a hook: k_batch_rollout_act ahead of a tick's launches where
// the rig is not empty, k_batch_rollout_record behind them - MGF_BATCH_ROLLOUT_LAUNCHES_PER_TICK = 2 at most, whatever the worlds, the
// actuators and the traced bodies ("rollout_launches").  Both obey the train's gate world by world, and the word `act` beside `done`
// keeps a world whose tick is run again from being actuated twice (k_batch_rollout.h).  Where the spring rig is not empty its two
// launches (k_batch_spring.h, MGF_BATCH_ROLLOUT_SPRING_LAUNCHES_PER_TICK) go ahead of the actuation under the same two words, and
// where the joint rig is not empty its one launch (k_batch_joint.h, MGF_BATCH_ROLLOUT_JOINT_LAUNCHES_PER_TICK) behind the actuation,
// and where the hinge rig is not empty its one launch (k_batch_hinge.h, MGF_BATCH_ROLLOUT_HINGE_LAUNCHES_PER_TICK) behind the joints'.
// Where the slider rig is not empty its one launch (k_batch_slider.h, MGF_BATCH_ROLLOUT_SLIDER_LAUNCHES_PER_TICK) goes behind the hinges'.
// Where the hinge rig is not empty and the readings table has rows (mgf_batch_set_hinge_trace), the hinge trace's one launch
// (k_batch_hinge_read.h, MGF_BATCH_ROLLOUT_HINGE_READ_LAUNCHES_PER_TICK) goes behind the record of every tick t < rows.
// Where the slider rig is not empty and its readings table has rows (mgf_batch_set_slider_trace), the slider trace's one launch
// (k_batch_slider_read.h, MGF_BATCH_ROLLOUT_SLIDER_READ_LAUNCHES_PER_TICK) goes behind the hinge trace's of every tick t < rows
// (both through host_batch_joint_read.inc).
// The rig is the actuators' (BatchRig::items: no plan and no upload format of its own), the trace rows are k_batch_dev_gather's.
// "drive_launches" is not touched.
// The order of both calls: the refusals that need no handle, the handle's own, (device form) EVERY device pointer looked up for its
// n_ticks-fold extent and the outputs held against each other and against the inputs - and only then the first thing is enqueued.

// (host_batch_spring.inc, behind this file) the springs' arguments for the train: the rig up, the wrench buffer and the skip counter there
static mgf_status batch_spring_ready(mgf_batch* b, float h, float* out_dev, BatchSpringArgs* A);
// (host_batch_joint.inc, behind this file) a kind of joints' arguments for the train: the rig and the target table up, the impulse buffer and the skip counter there
template <class T>
static mgf_status batch_joint_hook(mgf_batch* b, float h, int32_t iters, BatchJointHook* H);
// (host_batch_joint_read.inc, behind this file) a kind of encoders' arguments for the train, where its readings table has rows: the rig up, the impulse buffer there
template <class T>
static mgf_status batch_joint_read_hook(mgf_batch* b, int32_t iters, BatchJointReadHook* H);

struct RolloutBytes { size_t u, body, out[4], touch, sensor; };  // what the call touches of u, body, x, q, v, omega, touch, sensor
// the touch trace of mgf_batch_rollout_touches / _touches_dev (host_batch_trace.inc): rows of n reports, device memory when it reaches the core.
// lax (mgf_batch_rollout_observe, host_batch_scan.inc): NULL rows or n == 0 name no trace - off() - where mgf_batch_rollout_touches holds them against the rig
struct RolloutTouch {
  void* out; int64_t n; int32_t format; bool lax = false;
  bool off() const { return lax && (!out || n == 0); }
};
// the sensor trace of mgf_batch_rollout_observe / _observe_dev (host_batch_scan.inc): rows of n answers of the ray sensors; NULL rows or n == 0: no trace
struct RolloutScan {
  void* out; int64_t n; int32_t format, mask; bool reserved;  // reserved: a reserved word of the caller's struct is not 0
  bool off() const { return !out || n == 0; }
};

// the refusals of both forms, in the header's order; nothing is enqueued here.  tt: the call traces the contact sensors
// (mgf_batch_rollout_touches), whose refusals are slotted in where that header states them; null: mgf_batch_rollout's own, unchanged.
// ts: the call may trace the ray sensors (mgf_batch_rollout_observe), whose refusals stand behind the touch trace's at every stage
static mgf_status batch_rollout_args(const mgf_batch* b, int32_t iters, int64_t n_ticks, const float* u, int64_t n_act, int32_t mode, const int32_t* body,
                                     int64_t m, RolloutBytes* bytes, const RolloutTouch* tt = nullptr, const RolloutScan* ts = nullptr) {
  MGF_TRY(batch_rig_handle(b));
  if (n_ticks < 0) return fail(MGF_ERR_INVALID, "n_ticks is negative");
  if (iters < 0) return fail(MGF_ERR_INVALID, "iters is negative");
  if (n_act < 0) return fail(MGF_ERR_INVALID, "n_act is negative");
  if (m < 0) return fail(MGF_ERR_INVALID, "m is negative");
  if (tt && tt->n < 0) return fail(MGF_ERR_INVALID, "n_touch is negative");
  if (ts && ts->n < 0) return fail(MGF_ERR_INVALID, "n_sensor is negative");
  if (n_ticks > (1 << 20)) return fail(MGF_ERR_INVALID, "n_ticks must be at most 2^20");
  if (mode != MGF_ACTUATE_IMPULSE && mode != MGF_ACTUATE_FORCE) return fail(MGF_ERR_INVALID, "mode is neither MGF_ACTUATE_IMPULSE nor MGF_ACTUATE_FORCE");
  if (tt && tt->format != MGF_ROLLOUT_TOUCH_FULL && tt->format != MGF_ROLLOUT_TOUCH_SHORT)
    return fail(MGF_ERR_INVALID, "touch_format is neither MGF_ROLLOUT_TOUCH_FULL nor MGF_ROLLOUT_TOUCH_SHORT");
  if (ts && ts->format != MGF_ROLLOUT_SENSOR_HIT && ts->format != MGF_ROLLOUT_SENSOR_DEPTH)
    return fail(MGF_ERR_INVALID, "sensor_format is neither MGF_ROLLOUT_SENSOR_HIT nor MGF_ROLLOUT_SENSOR_DEPTH");
  if (ts && !ts->off()) MGF_TRY(query_mask_check(ts->mask));  // (a struct that names no sensor trace may leave the mask 0)
  if (ts && ts->reserved) return fail(MGF_ERR_INVALID, "a reserved word of mgf_rollout_traces is not 0");
  if (m > (int64_t)INT32_MAX) return fail(MGF_ERR_INVALID, "too many traced bodies in one call");
  // (n_ticks <= 2^20 and m < 2^31: 16 * n_ticks * m < 2^55)
  if (n_ticks > 0 && n_act > INT64_MAX / 4 / n_ticks) return fail(MGF_ERR_INVALID, "4 * n_ticks * n_act overflows int64_t");
  if (tt && n_ticks > 0 && tt->n > INT64_MAX / 64 / n_ticks) return fail(MGF_ERR_INVALID, "64 * n_ticks * n_touch overflows int64_t");
  if (ts && n_ticks > 0 && ts->n > INT64_MAX / 28 / n_ticks) return fail(MGF_ERR_INVALID, "28 * n_ticks * n_sensor overflows int64_t");
  if ((uint64_t)n_act != (uint64_t)b->actuators.recs.size()) return fail(MGF_ERR_INVALID, "n_act is not mgf_batch_actuator_count: control rows of another length than the rig");
  if (tt && !tt->off() && (uint64_t)tt->n != (uint64_t)b->touches.recs.size()) return fail(MGF_ERR_INVALID, "n_touch is not mgf_batch_touch_count: report rows of another length than the rig");
  if (ts && !ts->off() && (uint64_t)ts->n != (uint64_t)b->sensors.recs.size()) return fail(MGF_ERR_INVALID, "n_sensor is not mgf_batch_sensor_count: answer rows of another length than the rig");
  if (n_act > 0 && n_ticks > 0 && !u) return fail(MGF_ERR_INVALID, "NULL argument: u");
  if (tt && !tt->off() && tt->n > 0 && n_ticks > 0 && !tt->out) return fail(MGF_ERR_INVALID, "NULL argument: touch");
  if (!body && m > mgf_batch_len(b, -1)) return fail(MGF_ERR_INVALID, "without body indices m is at most the number of bodies");
  const size_t T = (size_t)n_ticks, M = (size_t)m;
  bytes->u = 4 * T * (size_t)n_act; bytes->body = 4 * M;
  bytes->out[0] = 12 * T * M; bytes->out[1] = 16 * T * M; bytes->out[2] = 12 * T * M; bytes->out[3] = 12 * T * M;
  bytes->touch = tt ? (tt->format == MGF_ROLLOUT_TOUCH_SHORT ? 16u : 64u) * T * (size_t)tt->n : 0;
  if (tt && tt->off()) bytes->touch = 0;
  bytes->sensor = ts && !ts->off() ? (ts->format == MGF_ROLLOUT_SENSOR_DEPTH ? 4u : 28u) * T * (size_t)ts->n : 0;
  return MGF_OK;
}

// The device core, behind every check: the arrays are device memory (the caller's or the handle's).  tt: rows of the contact sensors'
// reports behind every tick as well (k_batch_trace.h); null, no sensors or no rows: mgf_batch_rollout's train, launch for launch.
// ts: rows of the ray sensors' answers behind every tick as well (k_batch_scan.h); null, no sensors or no rows: the train without them.
static mgf_status batch_rollout_run(mgf_batch* b, float dt, int32_t iters, int64_t n_ticks, const float* u_dev, int64_t n_act, int32_t mode, const int32_t* body_dev,
                                    int64_t m, float* x, float* q, float* v, float* omega, mgf_step_stats* stats, const RolloutTouch* tt = nullptr,
                                    const RolloutScan* ts = nullptr) {
  b->r_launches = 0;
  const bool trace = m > 0 && (x || q || v || omega);
  const bool springs = !b->springs.recs.empty();  // (then even a call without controls and traces is not mgf_batch_step: the springs act ahead of every tick)
  const bool touches = tt && tt->n > 0 && tt->out;
  const bool scan = ts && ts->n > 0 && ts->out;
  const bool joints = !b->joints.recs.empty();  // (the same holds for the joints: they are solved ahead of every tick)
  const bool hinges = !b->hinges.recs.empty();  // (and for the hinges, solved behind them)
  const bool sliders = !b->sliders.recs.empty();  // (and for the sliders, solved behind the hinges)
  if (n_ticks == 0 || (n_act == 0 && !trace && !springs && !joints && !hinges && !sliders && !touches && !scan)) return batch_step_run(b, dt, iters, n_ticks, stats, nullptr);
  hipStream_t s = b->ctx->stream;
  BatchRig<mgf_batch_actuator>& R = b->actuators;
  MGF_TRY(batch_push(b));
  BatchRolloutHook H;
  memset(&H.A, 0, sizeof(H.A));
  memset(&H.T, 0, sizeof(H.T));
  memset(&H.R, 0, sizeof(H.R));
  memset(&H.W, 0, sizeof(H.W));
  if (n_act > 0) {
    MGF_TRY(batch_rig_up(b, R, "actuator", 3));
    if (!b->a_skipped.p) {
      MGF_TRY(b->a_skipped.ensure(1, s));
      MGF_HIP_TRY(hipMemsetAsync(b->a_skipped.p, 0, sizeof(unsigned long long), s));
    }
    H.A.runs = reinterpret_cast<const uint4*>(R.dev.p);
    H.A.rig = R.dev.p + R.off[1];
    H.A.order = reinterpret_cast<const uint32_t*>(R.dev.p + R.off[2]);
    H.A.u = u_dev;
    H.A.a_skipped = b->a_skipped.p;
    H.A.n_runs = (uint32_t)R.items.size();
    H.A.n_act = (uint32_t)n_act;
    H.act = true;
  }
  if (trace) {
    if (!b->v_skipped.p) {
      MGF_TRY(b->v_skipped.ensure(1, s));
      MGF_HIP_TRY(hipMemsetAsync(b->v_skipped.p, 0, sizeof(unsigned long long), s));
    }
    H.A.body = body_dev; H.A.m = (uint32_t)m;
    H.A.x = x; H.A.q = q; H.A.v = v; H.A.om = omega;
    H.A.v_skipped = b->v_skipped.p;
  }
  if (springs) {
    MGF_TRY(batch_spring_ready(b, dt, nullptr, &H.S));
    H.springs = true;
  }
  MGF_TRY(batch_joint_hook<JointKind>(b, dt, iters, &H.joints));  // (where the rig is not empty and iters > 0: with iters == 0 the solve calls enqueue nothing)
  MGF_TRY(batch_joint_hook<HingeKind>(b, dt, iters, &H.hinges));
  MGF_TRY(batch_joint_hook<SliderKind>(b, dt, iters, &H.sliders));
  MGF_TRY(batch_joint_read_hook<HingeKind>(b, iters, &H.hinge_read));  // (where the rig is not empty and its readings table has rows: the kind's read kernel behind every tick t < rows)
  MGF_TRY(batch_joint_read_hook<SliderKind>(b, iters, &H.slider_read));
  if (touches) {  // (the sensors' rig up ahead of the train; the lists' view is the train's to fill, pass by pass)
    MGF_TRY(batch_rig_up(b, b->touches, "contact sensor", 3));
    static_assert(sizeof(mgf_touch_report) == 64 && sizeof(TouchWord) == 16, "k_batch_trace_touch writes a report as four words of 16 bytes, a short one as one");
    H.T.V.out = reinterpret_cast<TouchWord*>(tt->out);
    H.T.n_touch = (uint32_t)tt->n;
    H.touch = tt->format;
  }
  if (scan) {  // (the sensors' rig up ahead of the train; the cast writes the handle's scratch, the rows go to the caller's; the rest is the train's to fill, pass by pass)
    MGF_TRY(batch_rig_up(b, b->sensors, "sensor", 4));
    MGF_TRY(b->q_out.ensure(7 * (size_t)ts->n, s));
    MGF_TRY(b->s_parts.ensure(7 * (size_t)ts->n, s));
    static_assert(sizeof(mgf_ray_hit) == 28 && sizeof(ParticleIn) == 28, "k_batch_scan_rows takes a hit and a particle up as seven words each");
    H.R.mask = ts->mask;
    H.R.out = b->q_out.p; H.R.parts = b->s_parts.p;
    H.W.out = ts->out; H.W.n_sensor = (uint32_t)ts->n;
    H.scan = ts->format;
  }
  H.A.B = b->bodies(0);
  H.A.w_off = b->d_off.p;
  H.A.total = (uint32_t)b->total();
  H.A.n_worlds = b->K;
  H.mode = mode;
  const mgf_status st = batch_step_run(b, dt, iters, n_ticks, stats, &H);
  b->r_launches = H.launches;
  return st;
}

extern "C" mgf_status mgf_batch_rollout_dev(mgf_batch* b, float dt, int32_t iters, int64_t n_ticks, const float* u_dev, int64_t n_act, int32_t mode,
                                            const int32_t* body_dev, int64_t m, float* x_dev, float* q_dev, float* v_dev, float* omega_dev, mgf_step_stats* stats) {
  RolloutBytes n;
  MGF_TRY(batch_rollout_args(b, iters, n_ticks, u_dev, n_act, mode, body_dev, m, &n));
  MGF_TRY(ctx_bind(b->ctx));
  MGF_TRY(dev_span(b->ctx, u_dev, n.u, "u_dev"));
  MGF_TRY(dev_span(b->ctx, body_dev, n.body, "body_dev"));
  MGF_TRY(dev_span(b->ctx, x_dev, n.out[0], "x_dev"));
  MGF_TRY(dev_span(b->ctx, q_dev, n.out[1], "q_dev"));
  MGF_TRY(dev_span(b->ctx, v_dev, n.out[2], "v_dev"));
  MGF_TRY(dev_span(b->ctx, omega_dev, n.out[3], "omega_dev"));
  const DevBytes arrays[6] = {{x_dev, n.out[0], "x_dev"}, {q_dev, n.out[1], "q_dev"}, {v_dev, n.out[2], "v_dev"}, {omega_dev, n.out[3], "omega_dev"},
                              {u_dev, n.u, "u_dev"}, {body_dev, n.body, "body_dev"}};
  MGF_TRY(dev_outputs_overlap(arrays, 6, 4));
  return batch_rollout_run(b, dt, iters, n_ticks, u_dev, n_act, mode, body_dev, m, x_dev, q_dev, v_dev, omega_dev, stats);
}

// The host form: one upload (u | body), the device core, one download (x | q | v | omega).  A row of an index outside the batch, which
// the device form leaves as the caller had it, comes back as zeros: the handle's buffer is cleared, not filled from the caller's rows.
extern "C" mgf_status mgf_batch_rollout(mgf_batch* b, float dt, int32_t iters, int64_t n_ticks, const float* u, int64_t n_act, int32_t mode, const int32_t* body,
                                        int64_t m, float* x, float* q, float* v, float* omega, mgf_step_stats* stats) {
  RolloutBytes n;
  MGF_TRY(batch_rollout_args(b, iters, n_ticks, u, n_act, mode, body, m, &n));
  MGF_TRY(ctx_bind(b->ctx));
  hipStream_t s = b->ctx->stream;
  float* host_out[4] = {x, q, v, omega};
  // the handle's buffer, every section from a 16-byte boundary: u | body | x | q | v | omega
  size_t off[7] = {0, 0, 0, 0, 0, 0, 0};
  off[1] = (n.u + 15) / 16;
  off[2] = off[1] + (body ? (n.body + 15) / 16 : 0);
  for (int k = 0; k < 4; ++k) off[3 + k] = off[2 + k] + (host_out[k] ? (n.out[k] + 15) / 16 : 0);
  float* dev_out[4] = {nullptr, nullptr, nullptr, nullptr};
  const float* u_dev = nullptr;
  const int32_t* body_dev = nullptr;
  std::vector<float4> stage;
  if (off[6]) {
    MGF_TRY(b->q_in.ensure(off[6], s));
    if (n.u) u_dev = reinterpret_cast<const float*>(b->q_in.p);
    if (body && n.body) body_dev = reinterpret_cast<const int32_t*>(b->q_in.p + off[1]);
    for (int k = 0; k < 4; ++k)
      if (host_out[k] && n.out[k]) dev_out[k] = reinterpret_cast<float*>(b->q_in.p + off[2 + k]);
    if (off[2]) {
      stage.resize(off[2]);
      if (n.u) memcpy(stage.data(), u, n.u);
      if (body_dev) memcpy(stage.data() + off[1], body, n.body);
      MGF_TRY(h2d(b->ctx, b->q_in.p, stage.data(), off[2]));
    }
    if (off[6] > off[2]) MGF_HIP_TRY(hipMemsetAsync(b->q_in.p + off[2], 0, 16 * (off[6] - off[2]), s));
  }
  MGF_TRY(batch_rollout_run(b, dt, iters, n_ticks, u_dev, n_act, mode, body_dev, m, dev_out[0], dev_out[1], dev_out[2], dev_out[3], stats));
  if (off[6] > off[2]) {
    stage.resize(off[6] - off[2]);
    MGF_TRY(d2h(b->ctx, stage.data(), b->q_in.p + off[2], stage.size()));
    for (int k = 0; k < 4; ++k)
      if (dev_out[k]) memcpy(host_out[k], stage.data() + (off[2 + k] - off[2]), n.out[k]);
  }
  return MGF_OK;
}
