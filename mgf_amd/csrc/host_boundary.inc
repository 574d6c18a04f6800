// The reference's library-level boundary on its own (SURVEY.md §8b): ContactConstraint::new for caller-built manifolds,
// a Solver handle, RigidBodyVec::clone.  mgf_demo/world.rs:243-251,279-287 calls ContactConstraint::new per contact with
// its own Manifold and hands the result to a Solver it owns; a caller that does its own collision detection uses these.
// Part of the single translation unit mgf_hip.hip (included there, in order); not compiled on its own.

// ContactConstraint::new solver.rs:101-191, n manifolds at once on the world's resident RigidBodyVec.
extern "C" mgf_status mgf_constraints_new(mgf_world* w, const mgf_body_ref* refs_a, const mgf_body_ref* refs_b, const mgf_manifold* manifolds,
                                          int64_t n, float dt, mgf_constraint* out, int64_t cap, int64_t* count) {
  if (!w || n < 0 || (n && (!refs_a || !refs_b || !manifolds))) return fail(MGF_ERR_INVALID, "bad argument");
  MGF_TRY(ctx_bind(w->ctx));
  MGF_TRY(perm_host(w));  // (bodies are named by the caller's indices; the kernel reads their slots: host_perm.inc)
  const uint32_t* so = w->permuted ? w->h_slot_of.data() : nullptr;
  std::vector<ManifoldRow> rows;
  std::vector<uint2> names;
  for (int64_t i = 0; i < n; ++i) {
    const mgf_body_ref& ra = refs_a[i];
    const mgf_body_ref& rb = refs_b[i];
    const mgf_manifold& m = manifolds[i];
    // every call site of the reference passes a Dynamic obj_a (world.rs:245,281); the records of this build hold one
    if (ra.tag != 0) return fail(MGF_ERR_STATIC_REF, "obj_a must be RigidBodyRef::Dynamic");
    if (ra.index >= w->n_owned) return fail(MGF_ERR_INVALID, "obj_a out of range");
    if (rb.tag == 0 && rb.index >= w->n_owned) return fail(MGF_ERR_INVALID, "obj_b out of range");
    if (rb.tag != 0 && rb.tag != 1) return fail(MGF_ERR_INVALID, "obj_b: unknown RigidBodyRef tag");
    if (rb.tag == 0 && rb.index == ra.index) return fail(MGF_ERR_INVALID, "a constraint needs two different bodies");
    if (m.n_contacts < 0 || m.n_contacts > MGF_MANIFOLD_CAP) return fail(MGF_ERR_INVALID, "manifold: n_contacts out of range");
    for (int32_t k = 0; k < m.n_contacts; ++k) {
      ManifoldRow r;
      r.a = ra.index; r.b = rb.tag == 0 ? rb.index : kNone;
      names.push_back(make_uint2(r.a, r.b));
      if (so) { r.a = so[r.a]; if (r.b != kNone) r.b = so[r.b]; }
      r.cb[0] = rb.center.x; r.cb[1] = rb.center.y; r.cb[2] = rb.center.z; r.fric_b = rb.friction;
      memcpy(r.n, &m.normal.x, 12); memcpy(r.t0, &m.tangent[0].x, 12); memcpy(r.t1, &m.tangent[1].x, 12);
      memcpy(r.la, &m.local_a[k].x, 12); memcpy(r.lb, &m.local_b[k].x, 12);
      rows.push_back(r);
    }
  }
  if (count) *count = (int64_t)rows.size();
  if ((int64_t)rows.size() > cap) return fail(MGF_ERR_CAPACITY, "constraint buffer too small");
  if (rows.empty()) return MGF_OK;
  if (!out) return fail(MGF_ERR_INVALID, "out is NULL");
  hipStream_t s = w->ctx->stream;
  DBuf<ManifoldRow> d_rows;
  DBuf<CRec> d_out;
  MGF_TRY(d_rows.ensure(rows.size(), s)); MGF_TRY(d_out.ensure(rows.size(), s));
  MGF_TRY(h2d(w->ctx, d_rows.p, rows.data(), rows.size()));
  k_constraints_new<<<nblk(rows.size()), kBlock, 0, s>>>(w->bodies(), d_rows.p, (uint32_t)rows.size(), dt, w->params.baumgarte,
                                                       w->params.penetration_slop, d_out.p);
  LAUNCH_CHECK();
  std::vector<CRec> h(rows.size());
  MGF_TRY(d2h(w->ctx, h.data(), d_out.p, rows.size()));
  for (size_t i = 0; i < h.size(); ++i) {
    crec_to_public(h[i], &out[i]);
    out[i].a = (int32_t)names[i].x; out[i].b = names[i].y == kNone ? -1 : (int32_t)names[i].y;
  }
  return MGF_OK;
}

// Solver<ContactConstraint> solver.rs:53-79: the insertion-ordered list lives with the handle; solve runs it on a world's
// resident RigidBodyVec with the tick's own executors (exact sequential order) and keeps the constraints' state
// (normal_impulse) for the next call, as the reference's `&mut self` does.
struct mgf_solver {
  std::vector<mgf_constraint> cons;
};
extern "C" mgf_status mgf_solver_new(mgf_solver** out) {
  if (!out) return fail(MGF_ERR_INVALID, "out is NULL");
  *out = new mgf_solver();
  return MGF_OK;
}
extern "C" void mgf_solver_free(mgf_solver* s) { delete s; }
extern "C" int64_t mgf_solver_len(const mgf_solver* s) { return s ? (int64_t)s->cons.size() : 0; }
extern "C" mgf_status mgf_solver_clear(mgf_solver* s) {
  if (!s) return fail(MGF_ERR_INVALID, "solver is NULL");
  s->cons.clear();
  return MGF_OK;
}
extern "C" mgf_status mgf_solver_add_constraints(mgf_solver* s, const mgf_constraint* cons, int64_t n) {
  if (!s || n < 0 || (n && !cons)) return fail(MGF_ERR_INVALID, "bad argument");
  for (int64_t i = 0; i < n; ++i) {
    if (cons[i].n_contacts != 1) return fail(MGF_ERR_INVALID, "a record holds one contact (mgf_constraints_new flattens a manifold)");
    if (cons[i].a < 0) return fail(MGF_ERR_STATIC_REF, "obj_a must be a Dynamic body");
  }
  s->cons.insert(s->cons.end(), cons, cons + n);
  return MGF_OK;
}
extern "C" mgf_status mgf_solver_add_constraint(mgf_solver* s, const mgf_constraint* c) { return mgf_solver_add_constraints(s, c, c ? 1 : 0); }
extern "C" mgf_status mgf_solver_read_constraints(const mgf_solver* s, mgf_constraint* out, int64_t cap, int64_t* count) {
  if (!s) return fail(MGF_ERR_INVALID, "solver is NULL");
  if (count) *count = (int64_t)s->cons.size();
  if (!out) return MGF_OK;
  if ((int64_t)s->cons.size() > cap) return fail(MGF_ERR_CAPACITY, "constraint buffer too small");
  if (!s->cons.empty()) memcpy(out, s->cons.data(), s->cons.size() * sizeof(mgf_constraint));
  return MGF_OK;
}
// Solver::solve(&mut rbv, iters): the world's tick list is replaced by the solver's (mgf_world_set_constraints).
extern "C" mgf_status mgf_solver_solve(mgf_solver* s, mgf_world* w, int32_t iters, mgf_step_stats* stats) {
  if (!s || !w) return fail(MGF_ERR_INVALID, "NULL argument");
  if (iters < 0) return fail(MGF_ERR_INVALID, "iters must be >= 0");
  w->n = w->n_owned;  // a Solver sees the RigidBodyVec: a tick's ghosts are dropped
  mgf_status st = mgf_world_set_constraints(w, s->cons.data(), (int64_t)s->cons.size());
  if (st == MGF_OK) st = mgf_world_solve(w, iters, stats);
  if (st == MGF_OK && !s->cons.empty()) st = mgf_world_read_constraints(w, s->cons.data(), (int64_t)s->cons.size(), nullptr);
  return st;
}

// RigidBodyVec: Clone (physics.rs:140) + the rest of the world (terrain copy, parameters, options): an independent world
// on the same context that steps identically.
template <class T>
static mgf_status clone_buf(mgf_ctx* ctx, DBuf<T>& dst, const DBuf<T>& src, size_t count) {
  if (count == 0 || !src.p) return MGF_OK;
  MGF_TRY(dst.ensure(count, ctx->stream));
  MGF_HIP_TRY(hipMemcpyAsync(dst.p, src.p, count * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
  return MGF_OK;
}
extern "C" mgf_status mgf_world_clone(mgf_world* src, mgf_world** out) {
  if (!src || !out) return fail(MGF_ERR_INVALID, "NULL argument");
  *out = nullptr;
  mgf_world* w = nullptr;
  MGF_TRY(mgf_world_new(src->ctx, &src->params, &w));
  std::unique_ptr<mgf_world, void (*)(mgf_world*)> guard(w, mgf_world_free);
  mgf_ctx* ctx = src->ctx;
  const size_t n = src->n_owned;
  MGF_TRY(clone_buf(ctx, w->x, src->x, n)); MGF_TRY(clone_buf(ctx, w->q, src->q, n)); MGF_TRY(clone_buf(ctx, w->srec, src->srec, 4 * n));
  MGF_TRY(clone_buf(ctx, w->sp0, src->sp0, n)); MGF_TRY(clone_buf(ctx, w->sp1, src->sp1, n)); MGF_TRY(clone_buf(ctx, w->ctor, src->ctor, n));
  MGF_TRY(clone_buf(ctx, w->imb, src->imb, 3 * n)); MGF_TRY(clone_buf(ctx, w->delta, src->delta, n)); MGF_TRY(clone_buf(ctx, w->einfo, src->einfo, n));
  MGF_TRY(clone_buf(ctx, w->col0, src->col0, n)); MGF_TRY(clone_buf(ctx, w->col1, src->col1, n)); MGF_TRY(clone_buf(ctx, w->tb_c, src->tb_c, n));
  MGF_TRY(clone_buf(ctx, w->tb_r, src->tb_r, n)); MGF_TRY(clone_buf(ctx, w->fb_c, src->fb_c, n)); MGF_TRY(clone_buf(ctx, w->fb_r, src->fb_r, n));
  if (src->has_compound) {
    MGF_TRY(clone_buf(ctx, w->pcount, src->pcount, n));
    MGF_TRY(clone_buf(ctx, w->lp0, src->lp0, kMaxParts * n)); MGF_TRY(clone_buf(ctx, w->lp1, src->lp1, kMaxParts * n));
    MGF_TRY(clone_buf(ctx, w->wp0, src->wp0, kMaxParts * n)); MGF_TRY(clone_buf(ctx, w->wp1, src->wp1, kMaxParts * n));
    MGF_TRY(clone_buf(ctx, w->xl0, src->xl0, src->x_used)); MGF_TRY(clone_buf(ctx, w->xl1, src->xl1, src->x_used));
    MGF_TRY(clone_buf(ctx, w->xw0, src->xw0, src->x_used)); MGF_TRY(clone_buf(ctx, w->xw1, src->xw1, src->x_used));
    w->x_used = src->x_used;
  }
  if (src->permuted) {  // the store's internal order travels with it (host_perm.inc); the clone's first tick has no cell order to re-sort by
    MGF_TRY(clone_buf(ctx, w->ext_of, src->ext_of, n)); MGF_TRY(clone_buf(ctx, w->slot_of, src->slot_of, n));
    w->permuted = true;
  }
  w->ticks_since_resort = src->ticks_since_resort;
  MGF_HIP_TRY(hipStreamSynchronize(ctx->stream));
  w->n = w->n_owned = src->n_owned;
  w->has_sphere = src->has_sphere; w->has_capsule = src->has_capsule; w->has_compound = src->has_compound; w->max_parts = src->max_parts;
  w->stats.n_bodies = w->n_owned;
  if (src->terrain) MGF_TRY(mgf_world_set_terrain(w, src->terrain.get()));
  for (const auto& ob : src->obstacles) MGF_TRY(mgf_world_add_obstacle(w, ob.get()));
  // options and the sticky plans a world settles into (so that the clone takes the same kernels from its first tick)
  w->opt = src->opt;
  w->opt.flow_spin_limit = 0;  // (a test's short fuse for one world's persistent launches: a clone never took it along)
  w->demo_tree = src->demo_tree; w->demo_leaf = src->demo_leaf;
  w->grid_occupancy = src->grid_occupancy;
  w->row_cap_t = src->row_cap_t; w->rev_cap = src->rev_cap; w->pair_brick_off = src->pair_brick_off; w->pair_brick_backoff = src->pair_brick_backoff;
  w->terrain_grid_off = src->terrain_grid_off; w->grid_too_wide = src->grid_too_wide; w->front_rows_off = src->front_rows_off;
  w->cap_t = src->cap_t; w->cap_p = src->cap_p; w->cap_c = src->cap_c; w->flow5_last_max = src->flow5_last_max;
  w->f6_fail_slots = src->f6_fail_slots; w->f6_fail_foreign = src->f6_fail_foreign; w->f6_fail_C = src->f6_fail_C; w->prev_C = src->prev_C;
  w->f6_last_slots = src->f6_last_slots; w->f6_last_foreign = src->f6_last_foreign; w->f6_last_msgs = src->f6_last_msgs;
  w->f6_last_block_msgs = src->f6_last_block_msgs; w->f6_prep_iters = src->f6_prep_iters;
  w->wide_engaged = src->wide_engaged; w->wide_hold = src->wide_hold;
  for (int k = 0; k < 3; ++k) { w->wide_ref[k] = src->wide_ref[k]; w->wide_limit[k] = src->wide_limit[k]; w->shape_rmax[k] = src->shape_rmax[k]; }
  for (int k = 0; k < 3; ++k) { w->h_scene_ext[k] = src->h_scene_ext[k]; w->h_scene_rmax[k] = src->h_scene_rmax[k]; }
  *out = guard.release();
  return MGF_OK;
}
