// mgf_batch_set_feelers, mgf_batch_feeler_count, mgf_batch_cast_feelers, mgf_batch_cast_feelers_dev: feelers - spheres and capsules with
// a displacement, fixed in the frame of a body - swept from the poses resident on the device (k_batch_feeler.h).  Part of the single
// translation unit mgf_hip.hip (included there, in order, behind host_batch_touch.inc); not compiled on its own.
//
// The fifth rig beside sensors, cameras, zones and contact sensors, and the sweep's counterpart of the first: what mgf_batch_sweep_many
// answers for a cast the caller assembles from gather_state every tick, a feeler answers from the rig and the resident x and q - and it
// can cast the body's own collider, which a caller reaches only through mgf_batch_read_colliders and the host.
// What the rig shares with the others is host_batch_rig.inc's: the prologue and the world / body check of the set call, the sort by
// world and the work items (batch_rig_plan), the upload - items | records | order | worlds, ONE copy - and the pieces of what a cast
// refuses before it looks at a device.  The passes over terrain faces and obstacles are batch_sweep_tail's (host_batch_query.inc),
// unchanged, over the stored casts.  A cast is then MGF_BATCH_FEELER_LAUNCHES = 1 launch - and the face pass, the obstacle pass, and the
// collider gather behind a step - with no plan, no index array and, for the device form, no host wait and no copy between host and
// device.
// The order of mgf_batch_cast_feelers_dev is host_batch_query_dev.inc's: the refusals that need no device, the handle's own, EVERY
// device pointer looked up (dev_span), the overlap of the two outputs - and only then the first thing is enqueued.

extern "C" mgf_status mgf_batch_set_feelers(mgf_batch* b, const mgf_batch_feeler* f, int64_t n_in) {
  MGF_TRY(batch_rig_set_args(b, f, n_in));
  static_assert(sizeof(mgf_batch_feeler) == sizeof(FeelerIn) && sizeof(mgf_batch_feeler) == 64, "the rig goes up as the caller's records");
  static_assert(MGF_FEELER_IGNORE_SELF == MGF_SENSOR_IGNORE_SELF, "one value for the bit every rig knows");
  const size_t n = (size_t)n_in;
  for (size_t i = 0; i < n; ++i) {
    MGF_TRY(batch_rig_ref_check(b, f[i].world, f[i].body, 0, "feeler"));  // (the flag word is this rig's own: below)
    const int32_t fl = f[i].flags;
    if (fl & ~(MGF_FEELER_IGNORE_SELF | MGF_FEELER_WORLD_DELTA | MGF_FEELER_OWN_SHAPE))
      return fail(MGF_ERR_INVALID, "a feeler's flags hold a bit beyond MGF_FEELER_OWN_SHAPE: the rig was not changed");
    if (!(fl & MGF_FEELER_OWN_SHAPE) && f[i].tag != MGF_SPHERE && f[i].tag != MGF_CAPSULE)
      return fail(MGF_ERR_INVALID, "a feeler's tag must be 0 (sphere) or 1 (capsule) without MGF_FEELER_OWN_SHAPE: the rig was not changed");
    if ((fl & MGF_FEELER_OWN_SHAPE) && !(fl & MGF_FEELER_IGNORE_SELF))
      return fail(MGF_ERR_INVALID, "MGF_FEELER_OWN_SHAPE without MGF_FEELER_IGNORE_SELF - the body would meet itself at t = 0: the rig was not changed");
    if (f[i].reserved[0] || f[i].reserved[1]) return fail(MGF_ERR_INVALID, "a feeler's reserved words must be 0: the rig was not changed");
  }
  batch_rig_plan(b, b->feelers, f, n);
  return MGF_OK;
}

extern "C" int64_t mgf_batch_feeler_count(const mgf_batch* b) { return b ? (int64_t)b->feelers.recs.size() : -1; }

// The launches of a cast, behind every check (n > 0): out_dev and casts_dev are device memory of n records each, the caller's or the
// handle's; neither is null - the later passes take a cast up again from casts_dev.
static mgf_status batch_feeler_run(mgf_batch* b, int32_t kinds_mask, int32_t* out_dev, MovingIn* casts_dev) {
  BatchRig<mgf_batch_feeler>& R = b->feelers;
  const size_t n = R.recs.size();
  MGF_TRY(batch_push(b));
  MGF_TRY(batch_env_sync(b));
  MGF_TRY(batch_rig_up(b, R, "feeler", 4));
  MGF_TRY(batch_cols_refresh(b, &b->q_launches));
  static_assert(sizeof(mgf_sweep_hit) == 52 && sizeof(mgf_moving_component) == sizeof(MovingIn) && sizeof(MovingIn) == 44,
                "k_batch_feeler_bodies writes mgf_sweep_hit as 13 words and mgf_moving_component as 11");
  BatchFeelerArgs A;
  memset(&A, 0, sizeof(A));
  batch_work_args(b, &A);
  A.items = reinterpret_cast<const uint4*>(R.dev.p);
  A.order = reinterpret_cast<const uint32_t*>(R.dev.p + R.off[2]);
  A.mask = kinds_mask;
  A.out = out_dev;
  A.x = b->dm[mgf_batch::AX].p; A.q = b->dm[mgf_batch::AQ].p;
  A.rig = reinterpret_cast<const FeelerIn*>(R.dev.p + R.off[1]);
  A.casts = casts_dev;
  if (batch_part_queries(b)) MGF_TRY(batch_pq_feeler(b, A, (unsigned)R.items.size()));  // (the body pass sees parts)
  else k_batch_feeler_bodies<<<(unsigned)R.items.size(), kBatchBlock, batch_ray_lds(b), b->ctx->stream>>>(A);
  LAUNCH_CHECK();
  b->q_launches += MGF_BATCH_FEELER_LAUNCHES;
  return batch_sweep_tail(b, batch_has_faces(b, kinds_mask), batch_has_obstacles(b, kinds_mask), reinterpret_cast<const int32_t*>(R.dev.p + R.off[3]), 0u, casts_dev,
                          n, out_dev);
}

// the refusals of both cast calls that need no device; *n: the feelers of the rig
static mgf_status batch_feeler_args(const mgf_batch* b, int32_t kinds_mask, const void* out, int64_t cap, size_t* n) {
  MGF_TRY(batch_rig_handle(b));
  MGF_TRY(batch_rig_cap(cap));
  MGF_TRY(query_mask_check(kinds_mask));
  *n = b->feelers.recs.size();
  return batch_rig_fits(*n, cap, out != nullptr);
}

extern "C" mgf_status mgf_batch_cast_feelers(mgf_batch* b, int32_t kinds_mask, mgf_sweep_hit* out, mgf_moving_component* casts_out, int64_t cap) {
  size_t n = 0;
  MGF_TRY(batch_feeler_args(b, kinds_mask, out, cap, &n));
  MGF_TRY(batch_single_parts(b, "mgf_batch_cast_feelers"));
  MGF_TRY(ctx_bind(b->ctx));
  batch_call_begin(b);
  if (n == 0) return MGF_OK;
  hipStream_t s = b->ctx->stream;
  MGF_TRY(b->q_out.ensure(13 * n, s));
  MGF_TRY(b->f_casts.ensure(11 * n, s));
  MGF_TRY(batch_feeler_run(b, kinds_mask, b->q_out.p, reinterpret_cast<MovingIn*>(b->f_casts.p)));
  MGF_HIP_TRY(hipMemcpyAsync(out, b->q_out.p, 52 * n, hipMemcpyDeviceToHost, s));
  if (casts_out) MGF_HIP_TRY(hipMemcpyAsync(casts_out, b->f_casts.p, 44 * n, hipMemcpyDeviceToHost, s));
  MGF_HIP_TRY(hipStreamSynchronize(s));
  return MGF_OK;
}

extern "C" mgf_status mgf_batch_cast_feelers_dev(mgf_batch* b, int32_t kinds_mask, mgf_sweep_hit* out_dev, mgf_moving_component* casts_out_dev, int64_t cap) {
  size_t n = 0;
  MGF_TRY(batch_feeler_args(b, kinds_mask, out_dev, cap, &n));
  MGF_TRY(batch_single_parts(b, "mgf_batch_cast_feelers_dev"));
  MGF_TRY(ctx_bind(b->ctx));
  MGF_TRY(dev_span(b->ctx, out_dev, 52 * n, "out_dev"));
  MGF_TRY(dev_span(b->ctx, casts_out_dev, 44 * n, "casts_out_dev"));
  // (the later passes read the casts again after the body pass wrote hits)
  const DevBytes arrays[2] = {{out_dev, 52 * n, "out_dev"}, {casts_out_dev, 44 * n, "casts_out_dev"}};
  MGF_TRY(dev_outputs_overlap(arrays, 2, 2));
  batch_call_begin(b);
  if (n == 0) return MGF_OK;
  if (!casts_out_dev) MGF_TRY(b->f_casts.ensure(11 * n, b->ctx->stream));
  return batch_feeler_run(b, kinds_mask, reinterpret_cast<int32_t*>(out_dev), casts_out_dev ? reinterpret_cast<MovingIn*>(casts_out_dev) : reinterpret_cast<MovingIn*>(b->f_casts.p));
}
