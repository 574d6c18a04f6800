// mgf_batch_gather_state_dev, mgf_batch_set_many_dev, mgf_batch_set_forces_dev, mgf_batch_apply_impulses_dev,
// mgf_batch_read_body_contacts_dev, mgf_batch_copy_worlds_where: the calls of host_batch_drive.inc / host_batch_observe.inc for a caller
// whose arrays are device memory (k_batch_dev.h).  Part of the single translation unit mgf_hip.hip (included there, in order); not compiled
// on its own.
//
// Every call is enqueued on the context's stream and returns without waiting for it.  With the mirror pushed, the handle's scratch
// buffers large enough and (masked copy) the pair table unchanged a call makes no host wait and no copy between host and device.
// The order of every call: the refusals that need no device, the handle's own (n against the number of bodies), then EVERY device
// pointer is looked up (dev_span: device or managed memory of the context's device, the bytes the call touches inside the allocation) -
// and only then the first thing is enqueued.  A host pointer a kernel dereferences is a device fault; it is refused here instead.
// Records that name a body twice are resolved on the device as the host path's stable sort resolves them: records per body by integer
// atomics, the library's prefix sum, every record into its body's segment, a lane per body that orders its segment by record index.

static mgf_status dev_span(const mgf_ctx* ctx, const void* p, size_t bytes, const char* what) {
  if (!p || bytes == 0) return MGF_OK;
  if (reinterpret_cast<uintptr_t>(p) & 3u) { set_error("%s is not aligned to 4 bytes", what); return MGF_ERR_INVALID; }
  hipPointerAttribute_t at;
  memset(&at, 0, sizeof(at));
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();
    set_error("%s is not device memory", what);
    return MGF_ERR_INVALID;
  }
  if ((at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged) || at.device != ctx->device) {
    set_error("%s is not device memory of the context's device", what);
    return MGF_ERR_INVALID;
  }
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) != hipSuccess) {
    (void)hipGetLastError();
    set_error("%s: its allocation cannot be found", what);
    return MGF_ERR_INVALID;
  }
  const size_t at_byte = (size_t)(reinterpret_cast<const char*>(p) - reinterpret_cast<const char*>(base));
  if (at_byte > size || bytes > size - at_byte) { set_error("%s: the allocation ends before the bytes the call touches", what); return MGF_ERR_INVALID; }
  return MGF_OK;
}

// the checks of a record call that need neither the handle's contents nor a device ...
static mgf_status batch_dev_args(const mgf_batch* b, int64_t n) {
  if (!b) return fail(MGF_ERR_INVALID, "batch is NULL");
  if (n < 0) return fail(MGF_ERR_INVALID, "n is negative");
  if (n > (int64_t)INT32_MAX) return fail(MGF_ERR_INVALID, "too many records in one call");
  return MGF_OK;
}
// ... and those that need them: nothing is enqueued here.  The call's launch counter starts from zero.
static mgf_status batch_dev_open(mgf_batch* b, const int32_t* body_dev, size_t n) {
  MGF_TRY(ctx_bind(b->ctx));
  if (!body_dev && n > b->total()) return fail(MGF_ERR_INVALID, "without body indices n is at most the number of bodies");
  b->d_launches = 0;
  return dev_span(b->ctx, body_dev, 4 * n, "body_dev");
}
// behind the pointer checks: the mirror up, the counter of skipped records there
static mgf_status batch_dev_begin(mgf_batch* b, BatchDevArgs* A) {
  MGF_TRY(batch_push(b));
  hipStream_t s = b->ctx->stream;
  if (!b->v_skipped.p) {
    MGF_TRY(b->v_skipped.ensure(1, s));
    MGF_HIP_TRY(hipMemsetAsync(b->v_skipped.p, 0, sizeof(unsigned long long), s));
  }
  memset(A, 0, sizeof(*A));
  A->B = b->bodies(0);
  A->total = (uint32_t)b->total();
  A->skipped = b->v_skipped.p;
  return MGF_OK;
}
static unsigned batch_dev_blocks(size_t n) { return (unsigned)((n + kBatchBlock - 1) / kBatchBlock); }

extern "C" mgf_status mgf_batch_gather_state_dev(mgf_batch* b, const int32_t* body_dev, int64_t n_in, float* x, float* q, float* v, float* omega, float* force,
                                                 float* torque) {
  MGF_TRY(batch_dev_args(b, n_in));
  const size_t n = (size_t)n_in;
  MGF_TRY(batch_dev_open(b, body_dev, n));
  MGF_TRY(dev_span(b->ctx, x, 12 * n, "x")); MGF_TRY(dev_span(b->ctx, q, 16 * n, "q")); MGF_TRY(dev_span(b->ctx, v, 12 * n, "v"));
  MGF_TRY(dev_span(b->ctx, omega, 12 * n, "omega")); MGF_TRY(dev_span(b->ctx, force, 12 * n, "force")); MGF_TRY(dev_span(b->ctx, torque, 12 * n, "torque"));
  if (n == 0 || (!x && !q && !v && !omega && !force && !torque)) return MGF_OK;
  BatchDevArgs A;
  MGF_TRY(batch_dev_begin(b, &A));
  A.body = body_dev; A.n = (uint32_t)n;
  A.x = x; A.q = q; A.v = v; A.om = omega; A.f = force; A.t = torque;
  k_batch_dev_gather<<<batch_dev_blocks(n), kBatchBlock, 0, b->ctx->stream>>>(A);
  LAUNCH_CHECK();
  ++b->d_launches;
  return MGF_OK;
}

// One launch where record i is body i; else count | the library's prefix sum | fill | apply: MGF_BATCH_DEV_SET_LAUNCHES kernels of ours.
template <int MODE>
static mgf_status batch_dev_set(mgf_batch* b, const int32_t* body_dev, int64_t n_in, const float* a0, const float* a1) {
  MGF_TRY(batch_dev_args(b, n_in));
  const size_t n = (size_t)n_in;
  MGF_TRY(batch_dev_open(b, body_dev, n));
  MGF_TRY(dev_span(b->ctx, a0, 12 * n, "the first array")); MGF_TRY(dev_span(b->ctx, a1, 12 * n, "the second array"));
  if (n == 0 || (MODE == DRIVE_FORCE && !a0 && !a1)) return MGF_OK;  // (as the host-memory calls)
  BatchDevArgs A;
  MGF_TRY(batch_dev_begin(b, &A));
  hipStream_t s = b->ctx->stream;
  A.body = body_dev; A.n = (uint32_t)n; A.a0 = a0; A.a1 = a1;
  if (!body_dev) {
    k_batch_dev_apply<MODE, false><<<batch_dev_blocks(n), kBatchBlock, 0, s>>>(A);
    LAUNCH_CHECK();
    ++b->d_launches;
    return MGF_OK;
  }
  const size_t total = A.total;
  MGF_TRY(b->v_cnt.ensure(total + 1, s)); MGF_TRY(b->v_off.ensure(total + 1, s)); MGF_TRY(b->v_seg.ensure(n, s));
  A.cnt = b->v_cnt.p; A.off = b->v_off.p; A.seg = b->v_seg.p;
  MGF_HIP_TRY(hipMemsetAsync(b->v_cnt.p, 0, 4 * (total + 1), s));
  k_batch_dev_count<<<batch_dev_blocks(n), kBatchBlock, 0, s>>>(A);
  LAUNCH_CHECK();
  MGF_TRY(prim_exclusive_scan_u32(b->ctx, b->v_cnt.p, b->v_off.p, total + 1));  // (a library primitive: not counted among the launches)
  k_batch_dev_fill<<<batch_dev_blocks(n), kBatchBlock, 0, s>>>(A);
  LAUNCH_CHECK();
  k_batch_dev_apply<MODE, true><<<batch_dev_blocks(total), kBatchBlock, 0, s>>>(A);
  LAUNCH_CHECK();
  b->d_launches += MGF_BATCH_DEV_SET_LAUNCHES;
  return MGF_OK;
}

extern "C" mgf_status mgf_batch_set_many_dev(mgf_batch* b, const int32_t* body_dev, int64_t n, const float* linear, const float* angular) {
  if (!b) return fail(MGF_ERR_INVALID, "batch is NULL");
  if (!linear || !angular) return fail(MGF_ERR_INVALID, "NULL argument");
  return batch_dev_set<DRIVE_VEL>(b, body_dev, n, linear, angular);
}
extern "C" mgf_status mgf_batch_set_forces_dev(mgf_batch* b, const int32_t* body_dev, int64_t n, const float* force, const float* torque) {
  return batch_dev_set<DRIVE_FORCE>(b, body_dev, n, force, torque);
}
extern "C" mgf_status mgf_batch_apply_impulses_dev(mgf_batch* b, const int32_t* body_dev, int64_t n, const float* linear, const float* angular) {
  return batch_dev_set<DRIVE_IMPULSE>(b, body_dev, n, linear, angular);
}

// mgf_batch_read_body_contacts with the caller's buffer as the kernel's output: no copy, no wait, no HIP-event time ("query_run_ns" = 0)
extern "C" mgf_status mgf_batch_read_body_contacts_dev(mgf_batch* b, int64_t world, mgf_body_contacts* out_dev, int64_t cap) {
  if (!b) return fail(MGF_ERR_INVALID, "batch is NULL");
  if (!out_dev) return fail(MGF_ERR_INVALID, "NULL argument");
  if (world < -1) return fail(MGF_ERR_INVALID, "world index out of range");
  MGF_TRY(ctx_bind(b->ctx));
  size_t first, n;
  MGF_TRY(batch_range(b, world, &first, &n));
  if ((int64_t)n > cap) return fail(MGF_ERR_CAPACITY, "buffer too small");
  MGF_TRY(dev_span(b->ctx, out_dev, 24 * n, "out_dev"));
  batch_call_begin(b);
  if (n == 0) return MGF_OK;
  MGF_TRY(batch_push(b));
  const uint32_t k0 = world < 0 ? 0u : (uint32_t)world, nw = world < 0 ? b->K : 1u;
  const uint32_t nmax = batch_nmax(b, k0, nw);
  BatchContactsArgs A;
  A.cons = b->cons.p; A.rows = b->rows.p; A.c_off = b->d_coff.p; A.c_count = b->d_ccount.p; A.w_off = b->d_off.p;
  A.world0 = k0;
  A.out = reinterpret_cast<uint32_t*>(out_dev);
  k_batch_observe_contacts<<<nw, kBatchBlock, 16u * nmax, b->ctx->stream>>>(A);
  LAUNCH_CHECK();
  ++b->q_launches;
  return MGF_OK;
}

// mgf_batch_copy_worlds for the pairs mask_dev selects.  The host does not know the mask: every named destination's share grows to its
// source's list (a larger share than needed may stay; no record is lost), and h_ccount of dst is unknown afterwards (ccount_stale).
extern "C" mgf_status mgf_batch_copy_worlds_where(mgf_batch* dst, const int32_t* dst_world, const mgf_batch* src_in, const int32_t* src_world, int64_t n_in,
                                                  const int32_t* mask_dev) {
  MGF_TRY(batch_copy_check(dst, dst_world, src_in, src_world, n_in));
  if (n_in && !mask_dev) return fail(MGF_ERR_INVALID, "NULL argument");
  mgf_batch* src = const_cast<mgf_batch*>(src_in);
  const size_t n = (size_t)n_in;
  MGF_TRY(dev_span(dst->ctx, mask_dev, 4 * n, "mask_dev"));
  dst->d_launches = 0;
  if (n == 0) return MGF_OK;
  MGF_TRY(batch_copy_open(dst, dst_world, src, src_world, n));
  hipStream_t s = dst->ctx->stream;
  bool same = dst->w_pairs_up && dst->w_pairs.size() == n;
  for (size_t i = 0; same && i < n; ++i) same = dst->w_pairs[i].x == (uint32_t)dst_world[i] && dst->w_pairs[i].y == (uint32_t)src_world[i];
  if (!same) {
    MGF_HIP_TRY(hipStreamSynchronize(s));  // (the last upload may still be reading w_pairs, a launch the table)
    dst->w_pairs_up = false;
    dst->w_pairs.resize(n);
    for (size_t i = 0; i < n; ++i) dst->w_pairs[i] = make_uint2((uint32_t)dst_world[i], (uint32_t)src_world[i]);
    MGF_TRY(dst->w_pairs_d.ensure(n, s));
    MGF_HIP_TRY(hipMemcpyAsync(dst->w_pairs_d.p, dst->w_pairs.data(), 8 * n, hipMemcpyHostToDevice, s));
    dst->w_pairs_up = true;
    ++dst->w_uploads;
  }
  BatchCopyWhereArgs A;
  A.C = batch_copy_args(dst, src, dst->w_pairs_d.p);
  A.mask = mask_dev;
  k_batch_dev_copy_where<<<(unsigned)n, kBatchBlock, 0, s>>>(A);
  LAUNCH_CHECK();
  ++dst->d_launches;
  MGF_TRY(batch_copy_parts(dst, src, dst->w_pairs_d.p, n, mask_dev));
  dst->ccount_stale = true;
  return MGF_OK;
}
