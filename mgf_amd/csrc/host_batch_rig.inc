// What the rigs of a batch - body-mounted ray sensors, depth cameras, box zones, contact sensors, feelers (host_batch_sensor.inc,
// host_batch_camera.inc, host_batch_zone.inc, host_batch_touch.inc, host_batch_feeler.inc) - share, written once around BatchRig<Rec>
// (host_batch.inc, beside the handle that holds the five).  Part of the single translation unit mgf_hip.hip (included there, in order,
// behind host_batch_query_dev.inc and ahead of the five); not compiled on its own.
//
// A rig is static: which body, where on it, and what the record says beyond that.  Everything that depends on the rig alone is done once,
// when it is set: the checks (batch_rig_set_args, batch_rig_ref_check and the rig's own), and - sensors and zones - the sort by world and
// the work items (batch_rig_plan: BatchQueryPlan, host_batch_query.inc).  The rig goes up - its sections in ONE copy (batch_rig_up) -
// before the first cast or read behind a change of the rig or of the batch's layout (mgf_batch_add_bodies -> batch_rigs_stale,
// host_batch.inc: the rig names (world, body), a body's flat offset is w_off[world] + body on the device, and the check body < length is
// made again against the lengths that go up with it).  What a cast or a read refuses before it looks at a device is written here as
// well, piece by piece, because the order of the pieces is the call's own (batch_rig_handle, batch_rig_cap, batch_rig_fits).

// what both set calls and mgf_batch_set_cameras refuse before they look at a record
static mgf_status batch_rig_set_args(const mgf_batch* b, const void* recs, int64_t n_in) {
  MGF_TRY(batch_dev_args(b, n_in));
  if (n_in && !recs) return fail(MGF_ERR_INVALID, "NULL argument");
  return MGF_OK;
}

// what a record of a rig - a sensor's, a camera's, a zone's, a contact sensor's - names: a world of the batch, a body of that world
// (or_world: or -1, the world itself - a zone's), no flag but the one defined (a contact sensor's flag word is its own: it passes 0)
static mgf_status batch_rig_ref_check(const mgf_batch* b, int32_t world, int32_t body, int32_t flags, const char* what, bool or_world = false) {
  if (world < 0 || (uint32_t)world >= b->K) return fail(MGF_ERR_INVALID, "world index out of range: the rig was not changed");
  if (!(or_world && body == -1) && (body < 0 || (uint32_t)body >= b->h_n[(size_t)world]))
    return fail(MGF_ERR_INVALID, "body index out of range: the rig was not changed");
  if (flags & ~MGF_SENSOR_IGNORE_SELF) {
    set_error("a %s's flags hold a bit beyond MGF_SENSOR_IGNORE_SELF: the rig was not changed", what);
    return MGF_ERR_INVALID;
  }
  return MGF_OK;
}

// The records become the rig, sorted by world (sensors, zones): reached only behind every check of every record - this is the first
// change of the rig.  (No device is needed: a call that was enqueued reads the device copy, which is replaced in stream order when the
// next one puts the rig up.)
template <class Rec>
static void batch_rig_plan(const mgf_batch* b, BatchRig<Rec>& R, const Rec* recs, size_t n) {
  std::vector<int32_t> world(n);
  for (size_t i = 0; i < n; ++i) world[i] = recs[i].world;
  const BatchQueryPlan plan(b->K, world.data(), n);
  R.recs.assign(recs, recs + n);
  R.items.resize(plan.n_items);
  R.order.resize(n);
  plan.fill(world.data(), n, R.items.data(), R.order.data());
  R.stale = true;
}

// Sections onto the device one behind the other, every one from a 16-byte boundary, in ONE copy.  off[k]: where section k begins in
// `dev`, in words of 16 bytes.
struct RigSection { const void* p; size_t bytes; };
static mgf_status batch_rig_upload(mgf_batch* b, DBuf<float4>& dev, const RigSection* sec, size_t n_sec, size_t* off) {
  size_t total = 0;
  for (size_t k = 0; k < n_sec; ++k) { off[k] = total; total += (sec[k].bytes + 15) / 16; }
  std::vector<float4> h(total);
  for (size_t k = 0; k < n_sec; ++k)
    if (sec[k].bytes) memcpy(h.data() + off[k], sec[k].p, sec[k].bytes);
  MGF_TRY(dev.ensure(total, b->ctx->stream));
  return h2d(b->ctx, dev.p, h.data(), total);
}

// The rig onto the device where the copy there is behind (n > 0): the first n_sec of items | records | order | worlds - the cameras'
// two (tiles | records), the zones' three, the sensors' and the feelers' four (the passes with a lane per query read a record's world
// by the caller's index).
// or_world: a body of -1 is the world itself.
template <class Rec>
static mgf_status batch_rig_up(mgf_batch* b, BatchRig<Rec>& R, const char* what, size_t n_sec, bool or_world = false) {
  if (!R.stale) return MGF_OK;
  const size_t n = R.recs.size();
  std::vector<int32_t> world(n_sec > 3 ? n : 0);
  for (size_t i = 0; i < n; ++i) {
    const Rec& r = R.recs[i];
    if (!(or_world && r.body < 0) && (uint32_t)r.body >= b->h_n[(size_t)r.world]) {
      set_error("internal error: a %s names a body its world does not hold", what);
      return MGF_ERR_INVALID;
    }
    if (n_sec > 3) world[i] = r.world;
  }
  const RigSection sec[4] = {{R.items.data(), 16 * R.items.size()}, {R.recs.data(), sizeof(Rec) * n}, {R.order.data(), 4 * R.order.size()}, {world.data(), 4 * world.size()}};
  MGF_TRY(batch_rig_upload(b, R.dev, sec, n_sec, R.off));
  R.stale = false;
  return MGF_OK;
}

// What a cast or a read of a rig refuses before it looks at a device, around the call's own check - the sensors' and the cameras' mask
// behind batch_rig_cap, the zones' k ahead of it.  n: the records the call writes; out: is there anywhere to write them.
static mgf_status batch_rig_handle(const mgf_batch* b) { return b ? MGF_OK : fail(MGF_ERR_INVALID, "batch is NULL"); }
static mgf_status batch_rig_cap(int64_t cap) { return cap < 0 ? fail(MGF_ERR_INVALID, "cap is negative") : MGF_OK; }
static mgf_status batch_rig_fits(size_t n, int64_t cap, bool out, const char* null_msg = "NULL argument") {
  if ((int64_t)n > cap) return fail(MGF_ERR_CAPACITY, "buffer too small");
  if (n && !out) return fail(MGF_ERR_INVALID, null_msg);
  return MGF_OK;
}
