// The encoders of a batch's hinges and sliders - mgf_batch_read_hinges, _read_hinges_dev, _set_hinge_trace, _hinge_trace_rows,
// _get_hinge_trace, _get_hinge_trace_dev and the same six for sliders: per joint a reading of 32 bytes formed from the state resident on
// the device (k_batch_joint_read.h; the hinge's and the slider's words in k_batch_hinge_read.h and k_batch_slider_read.h) - as a call of
// its own and as a table of the handle's that every rollout fills, a row a tick.  Every step is written once, over the kinds of
// host_batch_hinge.inc and host_batch_slider.inc; the ball joints have no encoder.  Part of the single translation unit mgf_hip.hip
// (included there, in order, behind host_batch_slider.inc); not compiled on its own.
//
// The rig is the kind's: nothing is set here but the table (the handle's BatchJointTrace, T::trace).  A read is T::read_launches = 1 launch
// ("drive_launches"), a lane per joint, behind batch_push and the rig's upload, so that what set_many, add_bodies or the rig's set call
// left on the host is what it sees.  Nothing here reads a shape and nothing but the caller's array, or the table, is written.
// The readings table mirrors the target table: R[rows][count] entries of 32 bytes (T::trace_reading) or 64 (T::trace_full: the reading
// and the eight impulse words of the tick's solve), allocated and zeroed by the set-trace call, 0 rows - the default, and what setting
// the rig makes of it - being no trace.  A rollout (host_batch_rollout.inc) takes the launch into the step's train behind the record of
// every tick t < rows, the hinges' ahead of the sliders': batch_joint_read_hook fills a kind's hook, batch_step_run (host_batch.inc)
// calls batch_joint_read_pass for every pass and batch_joint_read_tick for every tick.

// What the kernel reads of the handle, as it is now: a rollout's train looks it up again for every pass, as the other hooks' views are.
template <class T>
static void batch_joint_read_view(const mgf_batch* b, BatchJointReadArgs* A) {
  const auto& R = b->*T::rig;
  A->B = b->bodies(0);
  A->w_off = b->d_off.p;
  A->rig = R.dev.p + R.off[1];
  A->acc = reinterpret_cast<const float4*>(R.acc.p);
  A->n = (uint32_t)R.recs.size();
}

// What the launch reads, behind batch_push (n > 0): the rig up - by batch_joint_ready's steps - and the impulse buffer there.
// Shared with the rollouts, whose train fills done, act, tick and the table's row in.
template <class T>
static mgf_status batch_joint_read_ready(mgf_batch* b, BatchJointReadArgs* A) {
  auto& R = b->*T::rig;
  const size_t n = R.recs.size();
  MGF_TRY(batch_joint_far_ends<T>(b));  // (bodies may have been added)
  MGF_TRY(batch_rig_up(b, R, T::word, 3));
  MGF_TRY(R.acc.ensure(8 * n, b->ctx->stream));
  static_assert(sizeof(typename T::Reading) == 32 && sizeof(float4) == 16, "the kernel writes a reading as two words of 16 bytes");
  memset(A, 0, sizeof(*A));
  batch_joint_read_view<T>(b, A);
  return MGF_OK;
}

// The launch of a call, behind every check (n > 0): out_dev is device memory of 32 n bytes.
template <class T>
static mgf_status batch_joint_read_run(mgf_batch* b, void* out_dev) {
  MGF_TRY(batch_push(b));
  BatchJointReadArgs A;
  MGF_TRY(batch_joint_read_ready<T>(b, &A));
  A.out = reinterpret_cast<float4*>(out_dev);
  T::template read<false, kJointReadReading><<<(A.n + kBatchBlock - 1) / kBatchBlock, kBatchBlock, 0, b->ctx->stream>>>(A);
  LAUNCH_CHECK();
  b->d_launches += T::read_launches;
  return MGF_OK;
}

// the refusals of both read calls that need no device
template <class T>
static mgf_status batch_joint_read_args(const mgf_batch* b, const void* out) {
  MGF_TRY(batch_rig_handle(b));
  if (!out && !(b->*T::rig).recs.empty()) return fail(MGF_ERR_INVALID, "NULL argument: out");
  return MGF_OK;
}

// a device pointer the kernel stores words of 16 bytes through, or a copy goes to: the look-up of the device-pointer calls, and the words' alignment
static mgf_status batch_dev_span16(const mgf_batch* b, const void* p, size_t bytes, const char* what) {
  MGF_TRY(dev_span(b->ctx, p, bytes, what));
  if (p && bytes && (reinterpret_cast<uintptr_t>(p) & 15u)) { set_error("%s is not aligned to 16 bytes", what); return MGF_ERR_INVALID; }
  return MGF_OK;
}

// mgf_batch_read_hinges, _read_sliders
template <class T>
static mgf_status batch_joint_read(mgf_batch* b, void* out) {
  MGF_TRY(batch_joint_read_args<T>(b, out));
  MGF_TRY(ctx_bind(b->ctx));
  b->d_launches = 0;
  const size_t n = (b->*T::rig).recs.size();
  if (n == 0) return MGF_OK;
  hipStream_t s = b->ctx->stream;
  DBuf<float4>& stage = (b->*T::trace).out;
  MGF_TRY(stage.ensure(2 * n, s));
  MGF_TRY(batch_joint_read_run<T>(b, stage.p));
  MGF_HIP_TRY(hipMemcpyAsync(out, stage.p, 32 * n, hipMemcpyDeviceToHost, s));
  MGF_HIP_TRY(hipStreamSynchronize(s));
  return MGF_OK;
}

// mgf_batch_read_hinges_dev, _read_sliders_dev
template <class T>
static mgf_status batch_joint_read_dev(mgf_batch* b, void* out_dev) {
  MGF_TRY(batch_joint_read_args<T>(b, out_dev));
  MGF_TRY(ctx_bind(b->ctx));
  b->d_launches = 0;
  const size_t n = (b->*T::rig).recs.size();
  MGF_TRY(batch_dev_span16(b, out_dev, 32 * n, "out_dev"));
  if (n == 0) return MGF_OK;
  return batch_joint_read_run<T>(b, out_dev);
}

template <class T>
static size_t batch_joint_trace_entry(int32_t format) { return format == T::trace_full ? 64u : 32u; }

// mgf_batch_set_hinge_trace, _set_slider_trace
template <class T>
static mgf_status batch_joint_set_trace(mgf_batch* b, int64_t rows, int32_t format) {
  MGF_TRY(batch_rig_handle(b));
  if (rows < 0 || rows > (1 << 20)) return fail(MGF_ERR_INVALID, "rows must be in [0, 2^20]");
  if (format != T::trace_reading && format != T::trace_full) {
    set_error("format is neither MGF_%s_TRACE_READING nor MGF_%s_TRACE_FULL", T::caps, T::caps);
    return MGF_ERR_INVALID;
  }
  BatchJointTrace& R = b->*T::trace;
  const size_t n = (b->*T::rig).recs.size();
  if (rows > 0 && (uint64_t)n > (uint64_t)INT64_MAX / 64u / (uint64_t)rows) return batch_joint_fail(MGF_ERR_INVALID, "64 * rows * mgf_batch_%s_count overflows int64_t", T::word);
  MGF_TRY(ctx_bind(b->ctx));
  hipStream_t s = b->ctx->stream;
  const size_t words = (size_t)rows * n * (batch_joint_trace_entry<T>(format) / 16u);
  if (words) {
    MGF_TRY(R.tab.ensure(words, s));
    MGF_HIP_TRY(hipMemsetAsync(R.tab.p, 0, 16 * words, s));
  } else if (rows == 0 && R.tab.p) {  // (off: the table is freed behind whatever the stream still does with it)
    MGF_HIP_TRY(hipStreamSynchronize(s));
    MGF_HIP_TRY(hipFree(R.tab.p));
    R.tab.p = nullptr;
    R.tab.cap = 0;
  }
  R.rows = rows;
  R.format = format;
  return MGF_OK;
}

// mgf_batch_hinge_trace_rows, _slider_trace_rows
template <class T>
static int64_t batch_joint_trace_rows(const mgf_batch* b) { return b ? (b->*T::trace).rows : -1; }

// the refusals of both get calls that need no device; *bytes: what the call copies, from *at bytes into the table
template <class T>
static mgf_status batch_joint_trace_args(const mgf_batch* b, const void* out, int64_t row0, int64_t n_rows, size_t* at, size_t* bytes) {
  MGF_TRY(batch_rig_handle(b));
  if (row0 < 0) return fail(MGF_ERR_INVALID, "row0 is negative");
  if (n_rows < 0) return fail(MGF_ERR_INVALID, "n_rows is negative");
  const BatchJointTrace& R = b->*T::trace;
  if (row0 > R.rows || n_rows > R.rows - row0) return fail(MGF_ERR_INVALID, "row0 + n_rows is beyond the readings table");
  const size_t row = (b->*T::rig).recs.size() * batch_joint_trace_entry<T>(R.format);  // (rows <= 2^20 and the table's bytes were held against int64_t when it was set)
  *at = (size_t)row0 * row;
  *bytes = (size_t)n_rows * row;
  if (*bytes && !out) return fail(MGF_ERR_INVALID, "NULL argument: out");
  return MGF_OK;
}

// mgf_batch_get_hinge_trace, _get_slider_trace
template <class T>
static mgf_status batch_joint_get_trace(mgf_batch* b, void* out, int64_t row0, int64_t n_rows) {
  size_t at = 0, bytes = 0;
  MGF_TRY(batch_joint_trace_args<T>(b, out, row0, n_rows, &at, &bytes));
  MGF_TRY(ctx_bind(b->ctx));
  if (bytes == 0) return MGF_OK;
  hipStream_t s = b->ctx->stream;
  MGF_HIP_TRY(hipMemcpyAsync(out, reinterpret_cast<const char*>((b->*T::trace).tab.p) + at, bytes, hipMemcpyDeviceToHost, s));
  MGF_HIP_TRY(hipStreamSynchronize(s));
  return MGF_OK;
}

// mgf_batch_get_hinge_trace_dev, _get_slider_trace_dev
template <class T>
static mgf_status batch_joint_get_trace_dev(mgf_batch* b, void* out_dev, int64_t row0, int64_t n_rows) {
  size_t at = 0, bytes = 0;
  MGF_TRY(batch_joint_trace_args<T>(b, out_dev, row0, n_rows, &at, &bytes));
  MGF_TRY(ctx_bind(b->ctx));
  MGF_TRY(dev_span(b->ctx, out_dev, bytes, "out_dev"));
  if (bytes == 0) return MGF_OK;
  MGF_HIP_TRY(hipMemcpyAsync(out_dev, reinterpret_cast<const char*>((b->*T::trace).tab.p) + at, bytes, hipMemcpyDeviceToDevice, b->ctx->stream));
  return MGF_OK;
}

// A kind's trace hook for a rollout, behind batch_push and the kind's batch_joint_hook: on where its rig is not empty and its readings
// table has rows; with iters == 0 no solve wrote an impulse, and a full entry carries zeros
template <class T>
static mgf_status batch_joint_read_hook(mgf_batch* b, int32_t iters, BatchJointReadHook* H) {
  const BatchJointTrace& R = b->*T::trace;
  if ((b->*T::rig).recs.empty() || R.rows <= 0) return MGF_OK;
  MGF_TRY(batch_joint_read_ready<T>(b, &H->A));
  H->format = R.format == T::trace_full ? (iters > 0 ? kJointReadFull : kJointReadFullZero) : kJointReadReading;
  return MGF_OK;
}

// A kind's trace in the step's train (batch_step_run, host_batch.inc), where its hook is on.  Every pass: the rig, the impulse buffer and
// the TABLE are looked up again.
template <class T>
static void batch_joint_read_pass(const mgf_batch* b, BatchJointReadHook& H) {
  if (H.format < 0) return;
  batch_joint_read_view<T>(b, &H.A);
  H.A.done = b->d_done.p; H.A.act = b->d_act.p;
}

// Every tick: the launch, behind the record - act[k] is final - into row t from the handle's pointer as it is now; no launch for a tick
// the table has no row for
template <class T>
static mgf_status batch_joint_read_tick(mgf_batch* b, BatchJointReadHook& H, uint32_t t, int64_t* launches) {
  const BatchJointTrace& R = b->*T::trace;
  if (H.format < 0 || (int64_t)t >= R.rows) return MGF_OK;
  BatchJointReadArgs& A = H.A;
  const unsigned blocks = (A.n + kBatchBlock - 1) / kBatchBlock;
  hipStream_t s = b->ctx->stream;
  A.tick = t;
  A.out = R.tab.p + (size_t)t * A.n * (H.format == kJointReadReading ? 2u : 4u);
  if (H.format == kJointReadFull) T::template read<true, kJointReadFull><<<blocks, kBatchBlock, 0, s>>>(A);
  else if (H.format == kJointReadFullZero) T::template read<true, kJointReadFullZero><<<blocks, kBatchBlock, 0, s>>>(A);
  else T::template read<true, kJointReadReading><<<blocks, kBatchBlock, 0, s>>>(A);
  LAUNCH_CHECK();
  *launches += T::read_per_tick;
  return MGF_OK;
}

extern "C" mgf_status mgf_batch_read_hinges(mgf_batch* b, mgf_hinge_reading* out) { return batch_joint_read<HingeKind>(b, out); }
extern "C" mgf_status mgf_batch_read_hinges_dev(mgf_batch* b, mgf_hinge_reading* out_dev) { return batch_joint_read_dev<HingeKind>(b, out_dev); }
extern "C" mgf_status mgf_batch_set_hinge_trace(mgf_batch* b, int64_t rows, int32_t format) { return batch_joint_set_trace<HingeKind>(b, rows, format); }
extern "C" int64_t mgf_batch_hinge_trace_rows(const mgf_batch* b) { return batch_joint_trace_rows<HingeKind>(b); }
extern "C" mgf_status mgf_batch_get_hinge_trace(mgf_batch* b, void* out, int64_t row0, int64_t n_rows) { return batch_joint_get_trace<HingeKind>(b, out, row0, n_rows); }
extern "C" mgf_status mgf_batch_get_hinge_trace_dev(mgf_batch* b, void* out_dev, int64_t row0, int64_t n_rows) {
  return batch_joint_get_trace_dev<HingeKind>(b, out_dev, row0, n_rows);
}

extern "C" mgf_status mgf_batch_read_sliders(mgf_batch* b, mgf_slider_reading* out) { return batch_joint_read<SliderKind>(b, out); }
extern "C" mgf_status mgf_batch_read_sliders_dev(mgf_batch* b, mgf_slider_reading* out_dev) { return batch_joint_read_dev<SliderKind>(b, out_dev); }
extern "C" mgf_status mgf_batch_set_slider_trace(mgf_batch* b, int64_t rows, int32_t format) { return batch_joint_set_trace<SliderKind>(b, rows, format); }
extern "C" int64_t mgf_batch_slider_trace_rows(const mgf_batch* b) { return batch_joint_trace_rows<SliderKind>(b); }
extern "C" mgf_status mgf_batch_get_slider_trace(mgf_batch* b, void* out, int64_t row0, int64_t n_rows) { return batch_joint_get_trace<SliderKind>(b, out, row0, n_rows); }
extern "C" mgf_status mgf_batch_get_slider_trace_dev(mgf_batch* b, void* out_dev, int64_t row0, int64_t n_rows) {
  return batch_joint_get_trace_dev<SliderKind>(b, out_dev, row0, n_rows);
}
