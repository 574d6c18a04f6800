// mgf_batch_read_sliders, mgf_batch_read_sliders_dev, mgf_batch_set_slider_trace, mgf_batch_slider_trace_rows, mgf_batch_get_slider_trace,
// mgf_batch_get_slider_trace_dev: the sliders' encoders - per slider its travel along the axis, its rate, the side of its limit or its
// lock, the far anchor's distance from the axis and the frames' error, formed from the state resident on the device
// (k_batch_slider_read.h) - as a call of its own and as a table of the handle's that every rollout fills, a row a tick.  Part of the
// single translation unit mgf_hip.hip (included there, in order, behind host_batch_slider.inc); not compiled on its own.
//
// The rig is the sliders' (host_batch_slider.inc): nothing is set here but the table.  A read is MGF_BATCH_SLIDER_READ_LAUNCHES = 1
// launch ("drive_launches"), a lane per slider, behind batch_push and the rig's upload, so that what set_many, add_bodies or set_sliders
// left on the host is what it sees.  Nothing here reads a shape and nothing but the caller's array, or the table, is written.
// The readings table mirrors the hinges': R[rows][slider_count] entries of 32 bytes (MGF_SLIDER_TRACE_READING) or 64
// (MGF_SLIDER_TRACE_FULL: the reading and the eight impulse words of the tick's solve), allocated and zeroed by
// mgf_batch_set_slider_trace, 0 rows - the default, and what mgf_batch_set_sliders makes of it - being no trace.  A rollout
// (host_batch_rollout.inc) takes the launch into the step's train behind the hinge trace's of every tick t < rows:
// batch_slider_read_ready fills the hook's arguments, batch_step_run (host_batch.inc) looks the handle's view up again for every pass
// and launches it.  A device pointer is looked up, and held to 16 bytes, by the hinge encoders' batch_hinge_dev_span.

// What the kernel reads of the handle, as it is now: a rollout's train looks it up again for every pass, as the other hooks' views are.
static void batch_slider_read_view(const mgf_batch* b, BatchSliderReadArgs* A) {
  const BatchRig<mgf_batch_slider>& R = b->sliders;
  A->B = b->bodies(0);
  A->w_off = b->d_off.p;
  A->rig = R.dev.p + R.off[1];
  A->acc = reinterpret_cast<const float4*>(b->sliders.acc.p);
  A->n = (uint32_t)R.recs.size();
}

// What the launch reads, behind batch_push (n > 0): the rig up - by the joint rigs' steps - and the impulse buffer there.
// Shared with the rollouts, whose train fills done, act, tick and the table's row in.
static mgf_status batch_slider_read_ready(mgf_batch* b, BatchSliderReadArgs* A) {
  BatchJointRig<mgf_batch_slider>& R = b->sliders;
  const size_t n = R.recs.size();
  MGF_TRY(batch_joint_far_ends<SliderKind>(b));  // (bodies may have been added)
  MGF_TRY(batch_rig_up(b, R, "slider", 3));
  MGF_TRY(R.acc.ensure(8 * n, b->ctx->stream));
  static_assert(sizeof(mgf_slider_reading) == 32 && sizeof(float4) == 16, "k_batch_read_sliders writes a reading as two words of 16 bytes");
  memset(A, 0, sizeof(*A));
  batch_slider_read_view(b, A);
  return MGF_OK;
}

// The launch of a call, behind every check (n > 0): out_dev is device memory of 32 n bytes.
static mgf_status batch_slider_read_run(mgf_batch* b, void* out_dev) {
  MGF_TRY(batch_push(b));
  BatchSliderReadArgs A;
  MGF_TRY(batch_slider_read_ready(b, &A));
  A.out = reinterpret_cast<float4*>(out_dev);
  k_batch_read_sliders<false, kSliderReadReading><<<(A.n + kBatchBlock - 1) / kBatchBlock, kBatchBlock, 0, b->ctx->stream>>>(A);
  LAUNCH_CHECK();
  b->d_launches += MGF_BATCH_SLIDER_READ_LAUNCHES;
  return MGF_OK;
}

// the refusals of both read calls that need no device
static mgf_status batch_slider_read_args(const mgf_batch* b, const void* out) {
  MGF_TRY(batch_rig_handle(b));
  if (!out && !b->sliders.recs.empty()) return fail(MGF_ERR_INVALID, "NULL argument: out");
  return MGF_OK;
}

extern "C" mgf_status mgf_batch_read_sliders(mgf_batch* b, mgf_slider_reading* out) {
  MGF_TRY(batch_slider_read_args(b, out));
  MGF_TRY(ctx_bind(b->ctx));
  b->d_launches = 0;
  const size_t n = b->sliders.recs.size();
  if (n == 0) return MGF_OK;
  hipStream_t s = b->ctx->stream;
  MGF_TRY(b->st_out.ensure(2 * n, s));
  MGF_TRY(batch_slider_read_run(b, b->st_out.p));
  MGF_HIP_TRY(hipMemcpyAsync(out, b->st_out.p, 32 * n, hipMemcpyDeviceToHost, s));
  MGF_HIP_TRY(hipStreamSynchronize(s));
  return MGF_OK;
}

extern "C" mgf_status mgf_batch_read_sliders_dev(mgf_batch* b, mgf_slider_reading* out_dev) {
  MGF_TRY(batch_slider_read_args(b, out_dev));
  MGF_TRY(ctx_bind(b->ctx));
  b->d_launches = 0;
  const size_t n = b->sliders.recs.size();
  MGF_TRY(batch_hinge_dev_span(b, out_dev, 32 * n, "out_dev"));
  if (n == 0) return MGF_OK;
  return batch_slider_read_run(b, out_dev);
}

static size_t slider_trace_entry(int32_t format) { return format == MGF_SLIDER_TRACE_FULL ? 64u : 32u; }

extern "C" mgf_status mgf_batch_set_slider_trace(mgf_batch* b, int64_t rows, int32_t format) {
  MGF_TRY(batch_rig_handle(b));
  if (rows < 0 || rows > (1 << 20)) return fail(MGF_ERR_INVALID, "rows must be in [0, 2^20]");
  if (format != MGF_SLIDER_TRACE_READING && format != MGF_SLIDER_TRACE_FULL)
    return fail(MGF_ERR_INVALID, "format is neither MGF_SLIDER_TRACE_READING nor MGF_SLIDER_TRACE_FULL");
  const size_t n = b->sliders.recs.size();
  if (rows > 0 && (uint64_t)n > (uint64_t)INT64_MAX / 64u / (uint64_t)rows) return fail(MGF_ERR_INVALID, "64 * rows * mgf_batch_slider_count overflows int64_t");
  MGF_TRY(ctx_bind(b->ctx));
  hipStream_t s = b->ctx->stream;
  const size_t words = (size_t)rows * n * (slider_trace_entry(format) / 16u);
  if (words) {
    MGF_TRY(b->st_tab.ensure(words, s));
    MGF_HIP_TRY(hipMemsetAsync(b->st_tab.p, 0, 16 * words, s));
  } else if (rows == 0 && b->st_tab.p) {  // (off: the table is freed behind whatever the stream still does with it)
    MGF_HIP_TRY(hipStreamSynchronize(s));
    MGF_HIP_TRY(hipFree(b->st_tab.p));
    b->st_tab.p = nullptr;
    b->st_tab.cap = 0;
  }
  b->st_rows = rows;
  b->st_format = format;
  return MGF_OK;
}

extern "C" int64_t mgf_batch_slider_trace_rows(const mgf_batch* b) { return b ? b->st_rows : -1; }

// the refusals of both get calls that need no device; *bytes: what the call copies, from *at bytes into the table
static mgf_status batch_slider_trace_args(const mgf_batch* b, const void* out, int64_t row0, int64_t n_rows, size_t* at, size_t* bytes) {
  MGF_TRY(batch_rig_handle(b));
  if (row0 < 0) return fail(MGF_ERR_INVALID, "row0 is negative");
  if (n_rows < 0) return fail(MGF_ERR_INVALID, "n_rows is negative");
  if (row0 > b->st_rows || n_rows > b->st_rows - row0) return fail(MGF_ERR_INVALID, "row0 + n_rows is beyond the readings table");
  const size_t row = b->sliders.recs.size() * slider_trace_entry(b->st_format);  // (rows <= 2^20 and the table's bytes were held against int64_t when it was set)
  *at = (size_t)row0 * row;
  *bytes = (size_t)n_rows * row;
  if (*bytes && !out) return fail(MGF_ERR_INVALID, "NULL argument: out");
  return MGF_OK;
}

extern "C" mgf_status mgf_batch_get_slider_trace(mgf_batch* b, void* out, int64_t row0, int64_t n_rows) {
  size_t at = 0, bytes = 0;
  MGF_TRY(batch_slider_trace_args(b, out, row0, n_rows, &at, &bytes));
  MGF_TRY(ctx_bind(b->ctx));
  if (bytes == 0) return MGF_OK;
  hipStream_t s = b->ctx->stream;
  MGF_HIP_TRY(hipMemcpyAsync(out, reinterpret_cast<const char*>(b->st_tab.p) + at, bytes, hipMemcpyDeviceToHost, s));
  MGF_HIP_TRY(hipStreamSynchronize(s));
  return MGF_OK;
}

extern "C" mgf_status mgf_batch_get_slider_trace_dev(mgf_batch* b, void* out_dev, int64_t row0, int64_t n_rows) {
  size_t at = 0, bytes = 0;
  MGF_TRY(batch_slider_trace_args(b, out_dev, row0, n_rows, &at, &bytes));
  MGF_TRY(ctx_bind(b->ctx));
  MGF_TRY(dev_span(b->ctx, out_dev, bytes, "out_dev"));
  if (bytes == 0) return MGF_OK;
  MGF_HIP_TRY(hipMemcpyAsync(out_dev, reinterpret_cast<const char*>(b->st_tab.p) + at, bytes, hipMemcpyDeviceToDevice, b->ctx->stream));
  return MGF_OK;
}
