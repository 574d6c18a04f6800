// mgf_batch_set_touches, mgf_batch_touch_count, mgf_batch_read_touches, mgf_batch_read_touches_dev: contact sensors - per (body, partner
// filter) the last tick's constraint list folded on the device, a record of fixed width (k_batch_touch.h).  Part of the single
// translation unit mgf_hip.hip (included there, in order, behind host_batch_nearest.inc); not compiled on its own.
//
// mgf_batch_read_body_contacts sums over every partner of a body; "touched by whom" needed mgf_batch_read_constraints once per world and
// a fold on the host.  A sensor names the partner, and its report of 64 bytes needs no total, so a read is one pass and nothing waits.
// The fourth rig beside sensors, cameras and zones: the prologue and the world / body check of the set call, the sort by world and the
// work items (batch_rig_plan), the upload - items | records | order, ONE copy (batch_rig_up) - and the pieces of what a read refuses
// before it looks at a device are host_batch_rig.inc's.  A read is MGF_BATCH_TOUCH_LAUNCHES = 1 launch whatever the worlds, sensors and
// list lengths - no collider gather: nothing here reads a shape, which is also why a batch with bodies of several components is not
// refused (no batch_single_parts) - and, for the device form, no host wait and no copy between host and device.
// The order of the device-pointer call is host_batch_query_dev.inc's: the refusals that need no device, the handle's own, the device
// pointer looked up (dev_span) - and only then the first thing is enqueued.

extern "C" mgf_status mgf_batch_set_touches(mgf_batch* b, const mgf_batch_touch* t, int64_t n_in) {
  MGF_TRY(batch_rig_set_args(b, t, n_in));
  static_assert(sizeof(mgf_batch_touch) == sizeof(TouchIn) && sizeof(mgf_batch_touch) == 16, "the rig goes up as the caller's records");
  const size_t n = (size_t)n_in;
  for (size_t i = 0; i < n; ++i) {
    MGF_TRY(batch_rig_ref_check(b, t[i].world, t[i].body, 0, "contact sensor"));  // (the flag word is this rig's own: below)
    if (t[i].other < MGF_TOUCH_ANY || (t[i].other >= 0 && (uint32_t)t[i].other >= b->h_n[(size_t)t[i].world]))
      return fail(MGF_ERR_INVALID, "a contact sensor's other is neither a body of its world nor MGF_TOUCH_STATIC, _ANY_BODY or _ANY: the rig was not changed");
    if (t[i].other == t[i].body) return fail(MGF_ERR_INVALID, "a contact sensor's other is its own body: the rig was not changed");
    if (t[i].flags & ~MGF_TOUCH_BODY_FRAME)
      return fail(MGF_ERR_INVALID, "a contact sensor's flags hold a bit beyond MGF_TOUCH_BODY_FRAME: the rig was not changed");
  }
  BatchRig<mgf_batch_touch>& R = b->touches;
  batch_rig_plan(b, R, t, n);
  for (uint4& it : R.items)  // the work item's fourth word: one of its sensors needs the `b` occurrences of its body from the whole list
    for (uint32_t j = it.y; j < it.y + it.z; ++j) it.w |= t[R.order[j]].other <= MGF_TOUCH_ANY_BODY ? 1u : 0u;
  return MGF_OK;
}

extern "C" int64_t mgf_batch_touch_count(const mgf_batch* b) { return b ? (int64_t)b->touches.recs.size() : -1; }

// the tile of the list's `b` column a workgroup stages: 16 bytes a body of the batch's largest world, at least 256 words (at most 16 KB)
static uint32_t batch_touch_tile(const mgf_batch* b) { return std::max(4u * batch_nmax(b), 256u); }

// The launch of a read, behind every check (n > 0): out_dev is device memory of n reports, the caller's or the handle's.
// (Bodies added behind a tick: batch_push leaves c_count zero - every report is the no-match one.)
static mgf_status batch_touch_run(mgf_batch* b, mgf_touch_report* out_dev) {
  BatchRig<mgf_batch_touch>& R = b->touches;
  MGF_TRY(batch_push(b));
  MGF_TRY(batch_rig_up(b, R, "contact sensor", 3));
  static_assert(sizeof(mgf_touch_report) == 64 && sizeof(TouchWord) == 16, "k_batch_touch writes mgf_touch_report as four words of 16 bytes");
  BatchTouchArgs A;
  memset(&A, 0, sizeof(A));
  A.items = reinterpret_cast<const uint4*>(R.dev.p);
  A.order = reinterpret_cast<const uint32_t*>(R.dev.p + R.off[2]);
  A.rig = reinterpret_cast<const TouchIn*>(R.dev.p + R.off[1]);
  A.cons = b->cons.p; A.c_off = b->d_coff.p; A.c_count = b->d_ccount.p; A.w_off = b->d_off.p;
  A.q = b->dm[mgf_batch::AQ].p;
  A.tile = batch_touch_tile(b);
  A.out = reinterpret_cast<TouchWord*>(out_dev);
  k_batch_touch<<<(unsigned)R.items.size(), kBatchBlock, 4u * A.tile, b->ctx->stream>>>(A);
  LAUNCH_CHECK();
  b->q_launches += MGF_BATCH_TOUCH_LAUNCHES;
  return MGF_OK;
}

// the refusals of both read calls that need no device; *n: the sensors of the rig
static mgf_status batch_touch_read_args(const mgf_batch* b, const void* out, int64_t cap, size_t* n) {
  MGF_TRY(batch_rig_handle(b));
  MGF_TRY(batch_rig_cap(cap));
  *n = b->touches.recs.size();
  return batch_rig_fits(*n, cap, out != nullptr);
}

extern "C" mgf_status mgf_batch_read_touches(mgf_batch* b, mgf_touch_report* out, int64_t cap) {
  size_t n = 0;
  MGF_TRY(batch_touch_read_args(b, out, cap, &n));
  MGF_TRY(ctx_bind(b->ctx));
  batch_call_begin(b);
  if (n == 0) return MGF_OK;
  hipStream_t s = b->ctx->stream;
  MGF_TRY(b->touch_out.ensure(4 * n, s));
  MGF_TRY(batch_touch_run(b, reinterpret_cast<mgf_touch_report*>(b->touch_out.p)));
  MGF_HIP_TRY(hipMemcpyAsync(out, b->touch_out.p, 64 * n, hipMemcpyDeviceToHost, s));
  MGF_HIP_TRY(hipStreamSynchronize(s));
  return MGF_OK;
}

extern "C" mgf_status mgf_batch_read_touches_dev(mgf_batch* b, mgf_touch_report* out_dev, int64_t cap) {
  size_t n = 0;
  MGF_TRY(batch_touch_read_args(b, out_dev, cap, &n));
  MGF_TRY(ctx_bind(b->ctx));
  MGF_TRY(dev_span(b->ctx, out_dev, 64 * n, "out_dev"));
  batch_call_begin(b);
  if (n == 0) return MGF_OK;
  return batch_touch_run(b, out_dev);
}
