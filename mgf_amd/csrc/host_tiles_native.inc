// The tile protocol of SURVEY.md §8e under the C-ABI: this process's x-slab tiles of one scene stepped together, neighbour
// exchange between tiles of the same process by device copies and between processes (one per GPU) by RCCL point-to-point
// transfers over xGMI, all on the context's stream.  The semantics are those of mgf_amd/tiles.py (which stays as the
// transport-agnostic reference driver of the CPU tests): Gauss-Seidel inside a tile, ghost velocities refreshed every R
// solver iterations, bodies handed to the tile that holds their centre at the end of the tick.
// Part of the single translation unit mgf_hip.hip (included there, in order); not compiled on its own.
#include <dlfcn.h>
#include <rccl/rccl.h>

namespace {
// librccl is loaded at run time (dlopen): libmgf_hip.so has no link-time dependency on it, a single-GPU user never loads it,
// and a process that already holds a librccl (torch ships one with the same soname) shares that copy.
struct Rccl {
  void* lib = nullptr;
  decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
  decltype(&ncclCommInitRank) CommInitRank = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclSend) Send = nullptr;
  decltype(&ncclRecv) Recv = nullptr;
  decltype(&ncclGroupStart) GroupStart = nullptr;
  decltype(&ncclGroupEnd) GroupEnd = nullptr;
  decltype(&ncclAllReduce) AllReduce = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
};
Rccl g_rccl;
bool g_rccl_override_allowed = false;  // mgf_rccl_allow_override: the environment alone does not choose what this library loads
mgf_status rccl_load() {
  if (g_rccl.lib) return MGF_OK;
  // MGF_RCCL_LIB names the library to bind instead (a site's own RCCL build; the tests' several-ranks-on-one-GPU stand-in,
  // tests/fake_rccl) - honoured only after the host program has called mgf_rccl_allow_override(1); then nothing else is tried
  const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  void* h = nullptr;
  const char* forced = g_rccl_override_allowed ? getenv("MGF_RCCL_LIB") : nullptr;
  if (forced && *forced) h = dlopen(forced, RTLD_NOW | RTLD_LOCAL);
  else for (const char* n : names) { h = dlopen(n, RTLD_NOW | RTLD_GLOBAL); if (h) break; }
  if (!h) { set_error("librccl not found (%s)", dlerror()); return MGF_ERR_HIP; }
  Rccl r;
  r.lib = h;
#define MGF_RCCL_SYM(field, name) r.field = reinterpret_cast<decltype(r.field)>(dlsym(h, name)); if (!r.field) { set_error("librccl lacks %s", name); return MGF_ERR_HIP; }
  MGF_RCCL_SYM(GetUniqueId, "ncclGetUniqueId") MGF_RCCL_SYM(CommInitRank, "ncclCommInitRank") MGF_RCCL_SYM(CommDestroy, "ncclCommDestroy")
  MGF_RCCL_SYM(Send, "ncclSend") MGF_RCCL_SYM(Recv, "ncclRecv") MGF_RCCL_SYM(GroupStart, "ncclGroupStart") MGF_RCCL_SYM(GroupEnd, "ncclGroupEnd")
  MGF_RCCL_SYM(AllReduce, "ncclAllReduce") MGF_RCCL_SYM(GetErrorString, "ncclGetErrorString")
#undef MGF_RCCL_SYM
  g_rccl = r;
  return MGF_OK;
}
#define MGF_RCCL_TRY(expr)                                                                        \
  do {                                                                                            \
    ncclResult_t _r = (expr);                                                                     \
    if (_r != ncclSuccess) { set_error("%s failed: %s", #expr, g_rccl.GetErrorString(_r)); return MGF_ERR_HIP; } \
  } while (0)

struct TileState {
  mgf_world* w = nullptr;
  float x_lo = 0, x_hi = 0;
  DBuf<uint32_t> ids;            // [3 * cap]: left-face bodies, right-face bodies, migrants (left-goers first)
  uint32_t cap = 0;
  DBuf<float> send_body, send_vel, ghost_in, vel_in, mig_out, mig_in;
  uint32_t nl = 0, nr = 0, ml = 0, mr = 0;   // boundary bodies towards the left / right face, migrants going left / right
  uint32_t gl = 0, gr = 0;                   // ghosts received from the left / right neighbour
  uint32_t al = 0, ar = 0;                   // migrants arriving from the left / right neighbour
  uint32_t kinds_l = 0, kinds_r = 0;         // body kinds of the neighbours
  uint32_t rec_send = 72, rec_l = 72, rec_r = 72;  // floats per ghost record: this tile's, its left / right neighbour's (k_tiles.h: 72, or 40 from a world of single-component bodies)
  uint64_t migrated_in = 0, migrated_out = 0;
  const float* in_l = nullptr;   // where the rows of the last in-place exchange are: the left neighbour's, the right neighbour's
  const float* in_r = nullptr;   // (a local neighbour's send buffer itself, or this tile's receive buffer for a neighbouring rank)
};
}  // namespace

struct mgf_tiles {
  mgf_ctx* ctx = nullptr;
  std::vector<std::unique_ptr<TileState>> tp;  // (DBuf members: held by pointer)
  struct TileRefs { std::vector<std::unique_ptr<TileState>>* v; TileState& operator[](size_t i) const { return *(*v)[i]; } size_t size() const { return v->size(); } } t{&tp};
  int first = 0, total = 0;    // this process owns the tiles [first, first + t.size()) of `total`
  float halo = 1.0f;
  int refresh_every = 2;
  bool migrate = true;
  uint32_t* pin = nullptr;     // pinned: 8 words per local tile + 16 for the messages of the two outer faces + 4 for the tick's status + 4 per tile for the selection's totals
  uint32_t* pin_dev = nullptr; // the same memory as the device sees it (null: read-backs go by copy commands)
  DBuf<uint32_t> sel_tot;      // device: the tiles' selection totals (nl, nr, ml, mr), side by side
  // RCCL (tiles of other processes)
  ncclComm_t comm = nullptr;
  int rank = 0, n_ranks = 1;
  DBuf<int32_t> msg;           // device: [0..3] to the left, [4..7] to the right, [8..11] from the left, [12..15] from the right, [16..17] status in / agreed
  uint64_t ticks = 0;          // mgf_tiles_step calls so far
  // what the exchanges cost (mgf_tiles_counter): rows that crossed a RANK face (bytes out / in), rows copied between this rank's own
  // tiles, exchange calls, and the stream time between the events around them (waiting for the neighbour included)
  uint64_t x_bytes_out = 0, x_bytes_in = 0, x_bytes_local = 0, x_calls = 0, x_ns = 0, host_waits = 0;
  std::vector<hipEvent_t> ev;  // event pairs of the current tick's exchanges
  size_t ev_used = 0;
  // (r06) ... and by kind of exchange - the row width tells: ghost bodies, ghost velocities, hand-overs - the calls' own durations (us; the
  // first 65 536 of each), so that the first run on real links shows which step of the protocol costs what (counters "exchange_p50_ns_bodies" ...)
  std::vector<uint8_t> ev_kind;
  std::vector<float> x_us[3];
  int64_t test_fail_tick = -1; // tests: this rank fails in the collide phase of that tick (mgf_tiles_set_option "test_fail_tick")
  bool retry_lost = true;      // a tick in which a persistent solver launch gave up (on any rank) is repeated from a snapshot with the launch-per-frontier executor ("retry_lost_ticks")
  uint64_t ticks_retried = 0;
  bool time_exchanges = false; // HIP events around every exchange ("exchange_timing"; an event is a barrier packet: off unless asked for)
  bool has_left_rank() const { return comm && first > 0 && rank > 0; }
  bool has_right_rank() const { return comm && first + (int)t.size() < total && rank + 1 < n_ranks; }
};

extern "C" mgf_status mgf_rccl_allow_override(int32_t allow) {
  if (g_rccl.lib) return fail(MGF_ERR_INVALID, "the collectives library is already bound: call mgf_rccl_allow_override before any mgf_rccl_* / mgf_tiles_connect call");
  g_rccl_override_allowed = allow != 0;
  return MGF_OK;
}
extern "C" mgf_status mgf_rccl_unique_id(void* id128) {
  if (!id128) return fail(MGF_ERR_INVALID, "NULL argument");
  MGF_TRY(rccl_load());
  ncclUniqueId id;
  MGF_RCCL_TRY(g_rccl.GetUniqueId(&id));
  memcpy(id128, id.internal, NCCL_UNIQUE_ID_BYTES);
  return MGF_OK;
}
extern "C" mgf_status mgf_tiles_create(mgf_ctx* ctx, int32_t n_local, mgf_world* const* worlds, const float* x_lo, const float* x_hi,
                                       int32_t first_tile, int32_t n_tiles_total, float halo, int32_t refresh_every, int32_t migrate,
                                       mgf_tiles** out) {
  if (!ctx || !out || n_local < 1 || !worlds || !x_lo || !x_hi || first_tile < 0 || first_tile + n_local > n_tiles_total)
    return fail(MGF_ERR_INVALID, "bad argument");
  if (!(halo > 0.0f) || refresh_every < 1) return fail(MGF_ERR_INVALID, "halo must be > 0 and refresh_every >= 1");
  MGF_TRY(ctx_bind(ctx));
  std::unique_ptr<mgf_tiles> T(new mgf_tiles());
  T->ctx = ctx; T->first = first_tile; T->total = n_tiles_total; T->halo = halo; T->refresh_every = refresh_every; T->migrate = migrate != 0;
  for (int i = 0; i < n_local; ++i) T->tp.emplace_back(new TileState());
  for (int i = 0; i < n_local; ++i) {
    if (!worlds[i] || worlds[i]->ctx != ctx) return fail(MGF_ERR_INVALID, "every tile's world must live on the tiles' context");
    if (worlds[i]->max_parts > (uint32_t)kTileParts) return fail(MGF_ERR_INVALID, "bodies of more than four parts cannot cross tiles (the tile records carry four part slots)");
    T->t[(size_t)i].w = worlds[i]; T->t[(size_t)i].x_lo = x_lo[i]; T->t[(size_t)i].x_hi = x_hi[i];
    worlds[i]->opt.stream_ordered = 1;  // the tiling calls only enqueue: the driver synchronises where it needs a number
    // (a slab's cell grid is widened along its thin axis - grid_box - and its occupancy rule then adds a level: one level coarser serves the falling
    // pile of config 4 better, 5.52 -> 5.44 ms for 8 tiles, and changes nothing at rest or for config 5's tiles; a caller's own cell_fill stands)
    if (!worlds[i]->opt.cell_fill_set && worlds[i]->opt.cell_fill < 32) worlds[i]->opt.cell_fill = 32;
    if (!worlds[i]->f6_prep_iters) worlds[i]->f6_prep_iters = (uint32_t)refresh_every;  // (the most iterations one solver launch of this set runs: the channel buffer is sized for it, not for ten)
  }
  MGF_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&T->pin), (8 * (size_t)n_local + 16 + 4 + 4 * (size_t)n_local) * 4, hipHostMallocDefault));
  { void* dp = nullptr; if (hipHostGetDevicePointer(&dp, T->pin, 0) != hipSuccess) { (void)hipGetLastError(); dp = nullptr; } T->pin_dev = static_cast<uint32_t*>(dp); }
  MGF_TRY(T->msg.ensure(20, ctx->stream));
  ctx_retain(ctx);
  *out = T.release();
  return MGF_OK;
}
extern "C" void mgf_tiles_free(mgf_tiles* T) {
  if (!T) return;
  mgf_ctx* ctx = T->ctx;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  if (T->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(T->comm);
  if (T->pin) (void)hipHostFree(T->pin);
  for (hipEvent_t e : T->ev) (void)hipEventDestroy(e);
  delete T;
  ctx_release(ctx);
}
// Joins the RCCL communicator of the run: rank r of n_ranks owns a contiguous range of tiles, its neighbours are ranks r - 1
// and r + 1.  `id128` is the 128-byte id rank 0 obtained from mgf_rccl_unique_id and handed to the others by whatever
// channel the host program has.
extern "C" mgf_status mgf_tiles_connect(mgf_tiles* T, const void* id128, int32_t rank, int32_t n_ranks) {
  if (!T || !id128 || n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(MGF_ERR_INVALID, "bad argument");
  MGF_TRY(ctx_bind(T->ctx));
  MGF_TRY(rccl_load());
  ncclUniqueId id;
  memcpy(id.internal, id128, NCCL_UNIQUE_ID_BYTES);
  MGF_RCCL_TRY(g_rccl.CommInitRank(&T->comm, n_ranks, id, rank));
  T->rank = rank; T->n_ranks = n_ranks;
  return MGF_OK;
}
// Pre-flight: every rank contributes 1 to a sum over the communicator (0 ranks = not connected: all tiles are local).
extern "C" mgf_status mgf_tiles_preflight(mgf_tiles* T, int32_t* n_ranks_seen) {
  if (!T || !n_ranks_seen) return fail(MGF_ERR_INVALID, "NULL argument");
  *n_ranks_seen = 0;
  if (!T->comm) return MGF_OK;
  MGF_TRY(ctx_bind(T->ctx));
  hipStream_t s = T->ctx->stream;
  int32_t one = 1;
  MGF_TRY(h2d(T->ctx, T->msg.p, &one, 1));
  MGF_RCCL_TRY(g_rccl.AllReduce(T->msg.p, T->msg.p + 1, 1, ncclInt32, ncclSum, T->comm, s));
  return d2h(T->ctx, n_ranks_seen, T->msg.p + 1, 1);
}
// options of a tile set: "exchange_timing" = 1: HIP events around every exchange feed the counter "exchange_ns" (off by default: each
// event is a barrier packet in the stream); "test_fail_tick" = the mgf_tiles_step call (0-based) in which this rank fails in its collide phase (tests of the
// status agreement: no rank may hang, every rank must report the tick as lost); -1 = never
extern "C" mgf_status mgf_tiles_set_option(mgf_tiles* T, const char* key, int64_t value) {
  if (!T || !key) return fail(MGF_ERR_INVALID, "NULL argument");
  if (!strcmp(key, "test_fail_tick")) { T->test_fail_tick = value; return MGF_OK; }
  if (!strcmp(key, "exchange_timing")) { T->time_exchanges = value != 0; T->ev_used = 0; T->ev_kind.clear(); return MGF_OK; }
  if (!strcmp(key, "retry_lost_ticks")) { T->retry_lost = value != 0; return MGF_OK; }
  return fail(MGF_ERR_INVALID, "unknown option");
}
// counters of a tile set since its creation: "exchange_bytes_out" / "exchange_bytes_in" (rows that crossed a face between RANKS),
// "exchange_bytes_local" (rows copied between this rank's own tiles), "exchange_calls", "exchange_ns" (stream time of the exchanges,
// the wait for the neighbouring rank included; counted while option "exchange_timing" is on), "host_waits" (waits of the host on the stream inside mgf_tiles_step: counts, neighbour counts, a read-back per tile, a finish per tile, status, hand-overs), "ticks"; -1 = unknown key
extern "C" int64_t mgf_tiles_counter(const mgf_tiles* T, const char* key) {
  if (!T || !key) return -1;
  if (!strcmp(key, "exchange_bytes_out")) return (int64_t)T->x_bytes_out;
  if (!strcmp(key, "exchange_bytes_in")) return (int64_t)T->x_bytes_in;
  if (!strcmp(key, "exchange_bytes_local")) return (int64_t)T->x_bytes_local;
  if (!strcmp(key, "exchange_calls")) return (int64_t)T->x_calls;
  if (!strcmp(key, "exchange_ns")) return (int64_t)T->x_ns;
  if (!strncmp(key, "exchange_", 9)) {  // exchange_{calls|mean_ns|p50_ns|p99_ns|max_ns}_{bodies|velocities|handover}
    static const char* kinds[3] = {"bodies", "velocities", "handover"};
    for (int k = 0; k < 3; ++k) {
      const size_t lk = strlen(kinds[k]), l = strlen(key);
      if (l <= lk + 1 || strcmp(key + l - lk, kinds[k]) || key[l - lk - 1] != '_') continue;
      const std::string what(key + 9, l - lk - 1 - 9);
      std::vector<float> v = T->x_us[k];
      if (what == "calls") return (int64_t)v.size();
      if (v.empty()) return 0;
      std::sort(v.begin(), v.end());
      double r = -1.0;
      if (what == "mean_ns") { double a = 0; for (float x : v) a += x; r = a / (double)v.size(); }
      else if (what == "p50_ns") r = v[v.size() / 2];
      else if (what == "p99_ns") r = v[std::min(v.size() - 1, (size_t)((double)v.size() * 0.99))];
      else if (what == "max_ns") r = v.back();
      if (r >= 0.0) return (int64_t)(r * 1e3);
    }
  }
  if (!strcmp(key, "host_waits")) return (int64_t)T->host_waits;
  if (!strcmp(key, "ticks")) return (int64_t)T->ticks;
  if (!strcmp(key, "ticks_retried")) return (int64_t)T->ticks_retried;
  return -1;
}
extern "C" int64_t mgf_tiles_migrated(const mgf_tiles* T, int32_t tile, int32_t direction_in) {
  if (!T || tile < 0 || tile >= (int32_t)T->t.size()) return 0;
  return (int64_t)(direction_in ? T->t[(size_t)tile].migrated_in : T->t[(size_t)tile].migrated_out);
}

// One tick of the set.  *gave_up: the tick was abandoned on every rank and the only thing that went wrong anywhere was a persistent
// solver launch that gave up waiting (a device shared with another process): nothing has changed owner - the caller may put the bodies
// back and repeat it.
static mgf_status tiles_step_once(mgf_tiles* T, float dt, int32_t iters, mgf_step_stats* stats, bool* gave_up) {
  *gave_up = false;
  MGF_TRY(ctx_bind(T->ctx));
  mgf_ctx* ctx = T->ctx;
  hipStream_t s = ctx->stream;
  const int L = (int)T->t.size();
  const float big = 3.0e38f;
  auto has_left = [&](int i) { return T->first + i > 0; };
  auto has_right = [&](int i) { return T->first + i + 1 < T->total; };
  // A rank that fails in the middle of a tick must not leave its neighbours waiting in a receive (ADVICE r2 / VERDICT r2 item 4):
  // a LOCAL failure - a capacity that does not settle, a halo smaller than a body, a solver that gave up - is noted, the rank's
  // remaining COMPUTE of the tick is skipped, and the tick's COMMUNICATION goes on to its end with payloads of the agreed sizes
  // (garbage from here on); the ranks then agree on the tick's status (one all-reduced word, read at the wait the tick ends with
  // anyway) and all of them return an error before any body changes owner.  Only a failing transfer itself is fatal on the spot.
  mgf_status local = MGF_OK;
  std::string local_msg;
  auto note = [&](mgf_status st) { if (st != MGF_OK && local == MGF_OK) { local = st; local_msg = mgf_last_error(); } };
  for (int i = 0; i < L; ++i) T->t[(size_t)i].w->finish_gave_up = false;
#define TILE_TRY(expr) do { if (local == MGF_OK) note(expr); } while (0)
  // ---- A: complete_motion + integrate, boundary and migrant selection of every tile (counts, offsets and the id lists: three launches
  // for all the tiles, k_tile_select_*); ONE wait for all the counts
  for (int i0 = 0; i0 < L && local == MGF_OK; i0 += kWorldBatch) {  // every tile's k_reset_step in one launch, ahead of the integrations
    ResetBatch A;
    memset(&A, 0, sizeof(A));
    const int cnt = std::min(kWorldBatch, L - i0);
    for (int k = 0; k < cnt; ++k) TILE_TRY(world_reset_args(T->t[(size_t)(i0 + k)].w, &A.t[k]));
    if (local != MGF_OK) break;
    k_reset_step_batch<<<cnt, 64, 0, s>>>(A);
    LAUNCH_CHECK();
  }
  const bool resets_done = local == MGF_OK;
  std::vector<SelTile> sel;
  std::vector<int> sel_tile;  // which tile each entry of `sel` describes
  uint32_t* pin_tot = T->pin + 8 * (size_t)L + 20;  // [4 * L]
  MGF_TRY(T->sel_tot.ensure(4 * (size_t)L, s));
  auto select_enqueue = [&](int i) -> mgf_status {
    TileState& t = T->t[(size_t)i];
    mgf_world* w = t.w;
    MGF_TRY(world_identity(w));  // (the tiling protocol names bodies by their own indices: host_perm.inc)
    MGF_TRY(world_begin(w, dt, false, true, false, false, resets_done));
    const uint32_t n = w->n_owned;
    if (n == 0) return MGF_OK;
    if (n > t.cap) { t.cap = n + n / 4 + 64; MGF_TRY(t.ids.ensure(3 * (size_t)t.cap, s)); }
    const float x_left = has_left(i) ? t.x_lo + T->halo : -big, x_right = has_right(i) ? t.x_hi - T->halo : big;
    const float x_lo = (has_left(i) && T->migrate) ? t.x_lo : -big, x_hi = (has_right(i) && T->migrate) ? t.x_hi : big;
    SelTile S;
    MGF_TRY(select_describe(w, x_left, x_right, x_lo, x_hi, t.ids.p, t.ids.p + t.cap, t.ids.p + 2 * (size_t)t.cap, &S));
    S.tot = T->sel_tot.p + 4 * (size_t)i;  // (the tiles' totals side by side: one copy brings them all - or none: the kernel writes the pinned words itself)
    if (T->pin_dev) S.tot_host = T->pin_dev + 8 * (size_t)L + 20 + 4 * (size_t)i;
    sel.push_back(S); sel_tile.push_back(i);
    return MGF_OK;
  };
  for (int i = 0; i < L; ++i) {
    uint32_t* pin = T->pin + 8 * (size_t)i;
    pin[0] = pin[1] = pin[2] = pin[3] = 0;
    TILE_TRY(select_enqueue(i));
  }
  if (local == MGF_OK && !sel.empty()) {
    TILE_TRY(select_counts(s, sel.data(), (int)sel.size()));
    TILE_TRY(select_scatter(s, sel.data(), (int)sel.size()));
    if (local == MGF_OK && !T->pin_dev) MGF_HIP_TRY(hipMemcpyAsync(pin_tot, T->sel_tot.p, 16 * (size_t)L, hipMemcpyDeviceToHost, s));
  }
  MGF_HIP_TRY(hipStreamSynchronize(s)); ++T->host_waits;
  for (size_t k = 0; k < sel.size() && local == MGF_OK; ++k) memcpy(T->pin + 8 * (size_t)sel_tile[k], pin_tot + 4 * (size_t)sel_tile[k], 16);
  for (int i = 0; i < L; ++i) {
    TileState& t = T->t[(size_t)i];
    const uint32_t* pin = T->pin + 8 * (size_t)i;
    t.nl = pin[0]; t.nr = pin[1]; t.ml = pin[2]; t.mr = pin[3];
    if (local != MGF_OK) t.nl = t.nr = t.ml = t.mr = 0;  // (a failed rank announces nothing to send)
    // (r06) a world without bodies of several components sends 40-float records (k_tiles.h: kGhostFloatsPlain): what it announces as its kinds
    // below - bit 2 - tells the receiver which
    t.rec_send = t.w->has_compound ? (uint32_t)kGhostFloats : (uint32_t)kGhostFloatsPlain;
  }
  {  // what the neighbours are about to receive: both faces' ghost records of every tile in one launch
    std::vector<ExpTile> ex;
    std::vector<uint32_t> blocks;
    for (int i = 0; i < L && local == MGF_OK; ++i) {
      TileState& t = T->t[(size_t)i];
      TILE_TRY(t.send_body.ensure((size_t)kGhostFloats * std::max(t.nl + t.nr, 1u), s));
      TILE_TRY(t.send_vel.ensure(8 * (size_t)std::max(t.nl + t.nr, 1u), s));
      if (local != MGF_OK || !(t.nl + t.nr)) continue;
      ExpTile E;
      E.B = t.w->bodies(); E.ids_l = t.ids.p; E.ids_r = t.ids.p + t.cap; E.nl = t.nl; E.nr = t.nr; E.out = t.send_body.p;
      E.rec = t.rec_send; E.pad = 0;
      ex.push_back(E); blocks.push_back(nblk(t.nl + t.nr));
    }
    if (local == MGF_OK && !ex.empty()) TILE_TRY((tile_batches<ExpBatch, ExpTile>(s, k_export_bodies, ex.data(), blocks.data(), (int)ex.size())));
  }
  if (local != MGF_OK) for (int i = 0; i < L; ++i) { TileState& t = T->t[(size_t)i]; t.nl = t.nr = t.ml = t.mr = 0; }
  // ---- B: what each neighbour is about to receive (ghost rows, migrants, kinds of bodies)
  auto kinds_of = [](const mgf_world* w) { return (uint32_t)((w->has_sphere ? 1 : 0) | (w->has_capsule ? 2 : 0) | (w->has_compound ? 4 : 0) | (w->has_compound && w->max_parts > 2u ? 8 : 0)); };
  for (int i = 0; i < L; ++i) {
    TileState& t = T->t[(size_t)i];
    t.gl = t.gr = t.al = t.ar = 0; t.kinds_l = t.kinds_r = 0;
    if (i > 0) { const TileState& o = T->t[(size_t)i - 1]; t.gl = o.nr; t.al = o.mr; t.kinds_l = kinds_of(o.w); }
    if (i + 1 < L) { const TileState& o = T->t[(size_t)i + 1]; t.gr = o.nl; t.ar = o.ml; t.kinds_r = kinds_of(o.w); }
  }
  if (T->has_left_rank() || T->has_right_rank()) {
    // (word 3 of a message: the sender's status so far - a neighbour learns at once that this tick is lost)
    int32_t h[8] = {(int32_t)T->t[0].nl, (int32_t)T->t[0].ml, (int32_t)kinds_of(T->t[0].w), local != MGF_OK ? 1 : 0,
                    (int32_t)T->t[(size_t)L - 1].nr, (int32_t)T->t[(size_t)L - 1].mr, (int32_t)kinds_of(T->t[(size_t)L - 1].w), local != MGF_OK ? 1 : 0};
    memcpy(T->pin + 8 * (size_t)L, h, sizeof(h));
    MGF_HIP_TRY(hipMemcpyAsync(T->msg.p, T->pin + 8 * (size_t)L, sizeof(h), hipMemcpyHostToDevice, s));
    MGF_HIP_TRY(hipMemsetAsync(T->msg.p + 8, 0, 32, s));
    MGF_RCCL_TRY(g_rccl.GroupStart());
    if (T->has_left_rank()) { MGF_RCCL_TRY(g_rccl.Send(T->msg.p, 4, ncclInt32, T->rank - 1, T->comm, s)); MGF_RCCL_TRY(g_rccl.Recv(T->msg.p + 8, 4, ncclInt32, T->rank - 1, T->comm, s)); }
    if (T->has_right_rank()) { MGF_RCCL_TRY(g_rccl.Send(T->msg.p + 4, 4, ncclInt32, T->rank + 1, T->comm, s)); MGF_RCCL_TRY(g_rccl.Recv(T->msg.p + 12, 4, ncclInt32, T->rank + 1, T->comm, s)); }
    MGF_RCCL_TRY(g_rccl.GroupEnd());
    int32_t* back = reinterpret_cast<int32_t*>(T->pin + 8 * (size_t)L + 8);
    MGF_HIP_TRY(hipMemcpyAsync(back, T->msg.p + 8, 32, hipMemcpyDeviceToHost, s));
    MGF_HIP_TRY(hipStreamSynchronize(s)); ++T->host_waits;
    if (T->has_left_rank()) { T->t[0].gl = (uint32_t)back[0]; T->t[0].al = (uint32_t)back[1]; T->t[0].kinds_l = (uint32_t)back[2]; }
    if (T->has_right_rank()) { T->t[(size_t)L - 1].gr = (uint32_t)back[4]; T->t[(size_t)L - 1].ar = (uint32_t)back[5]; T->t[(size_t)L - 1].kinds_r = (uint32_t)back[6]; }
    if ((T->has_left_rank() && back[3]) || (T->has_right_rank() && back[7])) {
      set_error("tiles: a neighbouring rank failed in this tick");
      note(MGF_ERR_HIP);
    }
  }
  for (int i = 0; i < L; ++i) {  // the widths of the ghost records each tile is about to receive: its neighbours' kinds say
    TileState& t = T->t[(size_t)i];
    t.rec_l = (t.kinds_l & 4u) ? (uint32_t)kGhostFloats : (uint32_t)kGhostFloatsPlain;
    t.rec_r = (t.kinds_r & 4u) ? (uint32_t)kGhostFloats : (uint32_t)kGhostFloatsPlain;
  }
  // A generic exchange of rows across every tile face: `src(i)` holds tile i's rows for its left neighbour (n_to_left(i)
  // of them) followed by those for its right neighbour; `dst(i)` receives the left neighbour's rows, then the right one's.
  // `in_place`: rows from a tile of this rank are not copied - the receiving tile's import kernel reads the neighbour's send buffer
  // where it is (TileState::in_l / in_r; everything is ordered on one stream, and a send buffer is rewritten only by the next export).
  // `kind`: 0 ghost bodies, 1 ghost velocities, 2 hand-over (the latency statistics).  Widths in floats: `w_src(i)` of the rows tile i sends,
  // `w_left(i)` / `w_right(i)` of the rows it receives from its left / right neighbour (= that neighbour's w_src).
  auto exchange_w = [&](int kind, auto w_src, auto w_left, auto w_right, auto src, auto dst, auto n_to_left, auto n_to_right, auto n_from_left, auto n_from_right, bool in_place) -> mgf_status {
    const bool remote = T->has_left_rank() || T->has_right_rank();
    if (T->time_exchanges) {
      if (T->ev_used + 2 > T->ev.size()) { hipEvent_t a, b; MGF_HIP_TRY(hipEventCreate(&a)); MGF_HIP_TRY(hipEventCreate(&b)); T->ev.push_back(a); T->ev.push_back(b); }
      MGF_HIP_TRY(hipEventRecord(T->ev[T->ev_used], s));
      T->ev_kind.resize(T->ev.size() / 2);
      T->ev_kind[T->ev_used / 2] = kind;
    }
    ++T->x_calls;
    if (remote) MGF_RCCL_TRY(g_rccl.GroupStart());
    for (int i = 0; i < L; ++i) {
      float* d = dst(i);
      const uint32_t fl = n_from_left(i), fr = n_from_right(i);
      const size_t ws = w_src(i), wl = w_left(i), wr = w_right(i);
      T->t[(size_t)i].in_l = d; T->t[(size_t)i].in_r = d + wl * fl;
      if (i > 0) {
        if (in_place) T->t[(size_t)i].in_l = src(i - 1) + wl * n_to_left(i - 1);
        else if (fl) MGF_HIP_TRY(hipMemcpyAsync(d, src(i - 1) + wl * n_to_left(i - 1), 4 * wl * fl, hipMemcpyDeviceToDevice, s));
        T->x_bytes_local += 4 * wl * fl;
      } else if (T->has_left_rank()) {
        T->x_bytes_in += 4 * wl * fl; T->x_bytes_out += 4 * ws * n_to_left(i);
        if (fl) MGF_RCCL_TRY(g_rccl.Recv(d, wl * fl, ncclFloat32, T->rank - 1, T->comm, s));
        if (n_to_left(i)) MGF_RCCL_TRY(g_rccl.Send(src(i), ws * n_to_left(i), ncclFloat32, T->rank - 1, T->comm, s));
      }
      if (i + 1 < L) {
        if (in_place) T->t[(size_t)i].in_r = src(i + 1);
        else if (fr) MGF_HIP_TRY(hipMemcpyAsync(d + wl * fl, src(i + 1), 4 * wr * fr, hipMemcpyDeviceToDevice, s));
        T->x_bytes_local += 4 * wr * fr;
      } else if (T->has_right_rank()) {
        T->x_bytes_in += 4 * wr * fr; T->x_bytes_out += 4 * ws * n_to_right(i);
        if (fr) MGF_RCCL_TRY(g_rccl.Recv(d + wl * fl, wr * fr, ncclFloat32, T->rank + 1, T->comm, s));
        if (n_to_right(i)) MGF_RCCL_TRY(g_rccl.Send(src(i) + ws * n_to_left(i), ws * n_to_right(i), ncclFloat32, T->rank + 1, T->comm, s));
      }
    }
    if (remote) MGF_RCCL_TRY(g_rccl.GroupEnd());
    if (T->time_exchanges) { MGF_HIP_TRY(hipEventRecord(T->ev[T->ev_used + 1], s)); T->ev_used += 2; }
    return MGF_OK;
  };
  auto exchange = [&](size_t width, auto src, auto dst, auto n_to_left, auto n_to_right, auto n_from_left, auto n_from_right, bool in_place) -> mgf_status {
    auto w = [&](int) { return width; };
    return exchange_w(width == kVelFloatsPacked ? 1 : 2, w, w, w, src, dst, n_to_left, n_to_right, n_from_left, n_from_right, in_place);
  };
  // (after a stream synchronisation: the exchanges' event pairs of this tick so far)
  auto exchange_times = [&]() {
    for (size_t k = 0; k + 1 < T->ev_used; k += 2) {
      float ms = 0.0f;
      if (hipEventElapsedTime(&ms, T->ev[k], T->ev[k + 1]) == hipSuccess) {
        T->x_ns += (uint64_t)((double)ms * 1e6);
        const int kind = k / 2 < T->ev_kind.size() ? T->ev_kind[k / 2] : 0;
        if (T->x_us[kind].size() < 65536) T->x_us[kind].push_back(ms * 1e3f);
      }
    }
    T->ev_used = 0;
  };
  // ---- C: ghost bodies (buffers and transfers whatever the tick's status: the neighbours' sends must be met)
  for (int i = 0; i < L; ++i) {
    TileState& t = T->t[(size_t)i];
    MGF_TRY(t.send_body.ensure((size_t)kGhostFloats * std::max(t.nl + t.nr, 1u), s));
    MGF_TRY(t.send_vel.ensure(8 * (size_t)std::max(t.nl + t.nr, 1u), s));
    MGF_TRY(t.ghost_in.ensure((size_t)kGhostFloats * std::max(t.gl + t.gr, 1u), s));
    MGF_TRY(t.vel_in.ensure(8 * (size_t)std::max(t.gl + t.gr, 1u), s));
  }
  MGF_TRY(exchange_w(0, [&](int i) { return (size_t)T->t[(size_t)i].rec_send; }, [&](int i) { return (size_t)T->t[(size_t)i].rec_l; }, [&](int i) { return (size_t)T->t[(size_t)i].rec_r; },
                     [&](int i) { return T->t[(size_t)i].send_body.p; }, [&](int i) { return T->t[(size_t)i].ghost_in.p; },
                   [&](int i) { return T->t[(size_t)i].nl; }, [&](int i) { return T->t[(size_t)i].nr; },
                   [&](int i) { return T->t[(size_t)i].gl; }, [&](int i) { return T->t[(size_t)i].gr; }, true));
  {  // (every tile's ghosts in one launch)
    std::vector<ImpTile> im;
    std::vector<uint32_t> blocks;
    for (int i = 0; i < L; ++i) {
      TileState& t = T->t[(size_t)i];
      const uint32_t k = t.kinds_l | t.kinds_r;
      if (k) TILE_TRY(mgf_world_set_option(t.w, "body_kinds", (int64_t)k));
      ImpTile I;
      memset(&I, 0, sizeof(I));
      TILE_TRY(world_import_ghosts_prepare(t.w, t.in_l, (int64_t)(t.gl + t.gr), t.in_r, (int64_t)t.gl, &I));
      I.rec1 = t.rec_l; I.rec2 = t.rec_r;
      if (local == MGF_OK && I.m) { im.push_back(I); blocks.push_back(nblk(I.m)); }
    }
    if (local == MGF_OK && !im.empty()) TILE_TRY((tile_batches<ImpBatch, ImpTile>(s, k_import_ghosts, im.data(), blocks.data(), (int)im.size())));
  }
  // ---- D: collide, every tile enqueued before the first read-back is waited for
  std::vector<char> enq((size_t)L, 0);
  std::vector<PublishOne> pubs((size_t)L);
  for (auto& pb : pubs) memset(&pb, 0, sizeof(pb));
  for (int i = 0; i < L; ++i) {
    mgf_world* w = T->t[(size_t)i].w;
    if (local != MGF_OK) break;
    w->constraints_ready = false;
    w->C = w->Ct = w->Mt = w->Mp = 0;
    TILE_TRY(collide_enqueue(w, dt, true));
    TILE_TRY(readback_enqueue(w, &pubs[(size_t)i]));
    enq[(size_t)i] = local == MGF_OK;
  }
  for (int i0 = 0; i0 < L; i0 += kWorldBatch) {  // the tiles' read-back blocks into their pinned slots: one launch (a workgroup per tile)
    PublishBatch A;
    memset(&A, 0, sizeof(A));
    int cnt = 0;
    for (int i = i0; i < std::min(L, i0 + kWorldBatch); ++i) if (enq[(size_t)i] && pubs[(size_t)i].rb) A.t[cnt++] = pubs[(size_t)i];
    if (!cnt) continue;
    k_publish_batch<<<cnt, kBlock, 0, s>>>(A);
    LAUNCH_CHECK();
  }
  auto collide_settle = [&](int i) -> mgf_status {
    mgf_world* w = T->t[(size_t)i].w;
    bool retry = false;
    MGF_TRY(readback_wait(w));
    MGF_TRY(collide_process(w, &retry));
    for (int attempt = 0; retry && attempt < 8; ++attempt) {
      MGF_TRY(collide_enqueue(w, dt, true));
      MGF_TRY(collide_finish(w, &retry));
    }
    if (retry) return fail(MGF_ERR_HIP, "internal error: collide phase did not settle its buffer capacities");
    // A body is sent to the neighbour when its fat box comes within `halo` of the slab face; it can touch a body the
    // neighbour owns only through that body's fat half extent - which must therefore not exceed the halo, or contacts across
    // the face would be dropped silently.
    if (T->total > 1 && w->n > 0 && (w->last_rmax_x > T->halo || T->test_fail_tick == (int64_t)T->ticks)) {
      set_error("tiles: a body's fat half extent along x (%.3f) exceeds the halo (%.3f): contacts across tile faces would be missed - create the tiles with a larger halo",
                (double)w->last_rmax_x, (double)T->halo);
      return MGF_ERR_INVALID;
    }
    return MGF_OK;
  };
  {  // ONE wait - for the read-back enqueued last: the stream is in order, the other tiles' copies are there when it is
    int last = -1;
    for (int i = 0; i < L; ++i) if (enq[(size_t)i]) last = i;
    if (last >= 0) { ++T->host_waits; TILE_TRY(readback_wait(T->t[(size_t)last].w)); }
  }
  for (int i = 0; i < L; ++i)
    if (enq[(size_t)i]) TILE_TRY(collide_settle(i));
  // ---- E: Solver::solve in chunks of R iterations, ghost velocities refreshed from their owners in between
  int left_it = iters;
  while (left_it > 0) {
    const int k = std::min(T->refresh_every, left_it);
    left_it -= k;
    for (int i = 0; i < L; ++i) TILE_TRY(mgf_world_solve_enqueue(T->t[(size_t)i].w, k));
    if (left_it > 0 && T->total > 1) {
      if (local == MGF_OK) {  // both faces' velocity records of every tile in one launch: the left face's first
        std::vector<VelTile> ve;
        std::vector<uint32_t> blocks;
        for (int i = 0; i < L; ++i) {
          TileState& t = T->t[(size_t)i];
          if (!(t.nl + t.nr)) continue;
          VelTile V;
          V.srec = t.w->srec.p; V.ids_l = t.ids.p; V.ids_r = t.ids.p + t.cap; V.nl = t.nl; V.nr = t.nr; V.out = reinterpret_cast<float4*>(t.send_vel.p);
          V.rec = kVelFloatsPacked; V.pad = 0;
          ve.push_back(V); blocks.push_back(nblk(t.nl + t.nr));
        }
        if (!ve.empty()) TILE_TRY((tile_batches<VelBatch, VelTile>(s, k_export_vel, ve.data(), blocks.data(), (int)ve.size())));
      }
      MGF_TRY(exchange(kVelFloatsPacked, [&](int i) { return T->t[(size_t)i].send_vel.p; }, [&](int i) { return T->t[(size_t)i].vel_in.p; },
                       [&](int i) { return T->t[(size_t)i].nl; }, [&](int i) { return T->t[(size_t)i].nr; },
                       [&](int i) { return T->t[(size_t)i].gl; }, [&](int i) { return T->t[(size_t)i].gr; }, true));
      std::vector<GVelTile> gv;
      std::vector<uint32_t> blocks;
      for (int i = 0; i < L; ++i) {
        TileState& t = T->t[(size_t)i];
        GVelTile G;
        memset(&G, 0, sizeof(G));
        TILE_TRY(world_import_ghost_velocities_prepare(t.w, t.in_l, (int64_t)(t.gl + t.gr), t.in_r, (int64_t)t.gl, &G));
        G.rec = kVelFloatsPacked;
        if (local == MGF_OK && G.m) { gv.push_back(G); blocks.push_back(nblk(G.m)); }
      }
      if (local == MGF_OK && !gv.empty()) TILE_TRY((tile_batches<GVelBatch, GVelTile>(s, k_import_ghost_vel, gv.data(), blocks.data(), (int)gv.size())));
    }
  }
  // ---- F: the one place the host waits for the solvers - and where the ranks agree on the tick's status
  {  // every tile's solver flags - one launch per batch writes them into the tiles' pinned blocks - then one wait for all of them
    std::vector<FlagTile> fl;
    for (int i = 0; i < L && local == MGF_OK; ++i) {
      mgf_world* w = T->t[(size_t)i].w;
      if (!w->solve_pending || !w->stats.solver_kernel_launches || w->rb_fresh) continue;
      if (!w->ts->pin_dev) { TILE_TRY(solve_flow_fetch_enqueue(w)); continue; }
      FlagTile F;
      F.src = w->word(kWSolverAbort); F.dst = w->ts->pin_dev + mgf_world::kRbScalars + mgf_world::kSolverFlagsFirst; F.words = mgf_world::kSolverFlagsWords; F.pad = 0;
      fl.push_back(F);
      w->rb_fresh = true;
    }
    for (size_t i0 = 0; i0 < fl.size(); i0 += kTileBatch) {
      FlagBatch A;
      memset(&A, 0, sizeof(A));
      for (size_t k = 0; k < (size_t)kTileBatch && i0 + k < fl.size(); ++k) A.t[k] = fl[i0 + k];
      k_fetch_flags<<<1, 16 * kTileBatch, 0, s>>>(A);
      LAUNCH_CHECK();
    }
  }
  MGF_HIP_TRY(hipStreamSynchronize(s)); ++T->host_waits;
  for (int i = 0; i < L; ++i) TILE_TRY(mgf_world_finish(T->t[(size_t)i].w, stats ? stats + i : nullptr));
  int32_t* agreed = reinterpret_cast<int32_t*>(T->pin + 8 * (size_t)L + 16);
  // the tick's status, agreed by maximum: 0 fine, 1 a persistent solver launch gave up (and nothing else went wrong here), 2 anything else
  bool only_gave_up = local != MGF_OK;
  if (local != MGF_OK) { bool any = false; for (int i = 0; i < L; ++i) any = any || T->t[(size_t)i].w->finish_gave_up; only_gave_up = any; }
  agreed[0] = local == MGF_OK ? 0 : (only_gave_up ? 1 : 2);
  if (T->comm && T->n_ranks > 1) {
    agreed[1] = agreed[0];
    MGF_HIP_TRY(hipMemcpyAsync(T->msg.p + 16, agreed + 1, 4, hipMemcpyHostToDevice, s));
    MGF_RCCL_TRY(g_rccl.AllReduce(T->msg.p + 16, T->msg.p + 17, 1, ncclInt32, ncclMax, T->comm, s));
    MGF_HIP_TRY(hipMemcpyAsync(agreed, T->msg.p + 17, 4, hipMemcpyDeviceToHost, s));
    MGF_HIP_TRY(hipStreamSynchronize(s)); ++T->host_waits;
  }
  exchange_times();
  ++T->ticks;
  if (agreed[0] == 1) *gave_up = true;  // (here or on another rank; every rank sees the same word)
  if (local != MGF_OK) { set_error("%s", local_msg.c_str()); return local; }
  if (agreed[0]) return fail(MGF_ERR_HIP, "tiles: another rank failed in this tick; the tick was abandoned on every rank (no body changed owner)");
#undef TILE_TRY
  // ---- G: bodies whose centre left their slab change owner (rare; both ends of a hand-over know it from the counts)
  bool any = false;
  for (int i = 0; i < L; ++i) { const TileState& t = T->t[(size_t)i]; any = any || t.ml || t.mr || t.al || t.ar; }
  if (any) {
    for (int i = 0; i < L; ++i) {
      TileState& t = T->t[(size_t)i];
      MGF_TRY(t.mig_out.ensure((size_t)MGF_MIGRANT_FLOATS * std::max(t.ml + t.mr, 1u), s));
      MGF_TRY(t.mig_in.ensure((size_t)MGF_MIGRANT_FLOATS * std::max(t.al + t.ar, 1u), s));
      if (t.ml + t.mr) MGF_TRY(mgf_world_export_migrants(t.w, t.ids.p + 2 * (size_t)t.cap, (int64_t)(t.ml + t.mr), t.mig_out.p));
    }
    MGF_TRY(exchange((size_t)MGF_MIGRANT_FLOATS, [&](int i) { return T->t[(size_t)i].mig_out.p; }, [&](int i) { return T->t[(size_t)i].mig_in.p; },
                     [&](int i) { return T->t[(size_t)i].ml; }, [&](int i) { return T->t[(size_t)i].mr; },
                     [&](int i) { return T->t[(size_t)i].al; }, [&](int i) { return T->t[(size_t)i].ar; }, true));
    std::vector<FlagTile> hand_flags;
    // (everything is ordered on the stream: the hand-over needs no wait of its own - the ids are the tiles' own lists, the arrivals' kinds
    // are what the neighbours announced; r04: two waits per tile and tick less)
    for (int i = 0; i < L; ++i) {
      TileState& t = T->t[(size_t)i];
      if (t.ml + t.mr) MGF_TRY(remove_bodies_impl(t.w, t.ids.p + 2 * (size_t)t.cap, (int64_t)(t.ml + t.mr), true));
      if (t.al + t.ar) {
        // (what the neighbours announced: bit 0 spheres, bit 1 capsules; bodies of several components - bits 2 and 3 - were made known to this tile
        // when the masks were exchanged (option body_kinds).  A neighbour of such bodies only announces neither plain kind: the high bit
        // says "a hint", so that this tile does not take on both plain kinds - and the general kernels - for good.)
        const uint32_t mask = (t.al ? t.kinds_l : 0u) | (t.ar ? t.kinds_r : 0u);
        const uint32_t hint = mask ? ((mask & 3u) | 0x80000000u) : 3u;
        MGF_TRY(import_migrants_impl(t.w, t.in_l, (int64_t)(t.al + t.ar), hint, t.in_r, (int64_t)t.al));  // (the neighbours' records where they lie)
      }
      t.migrated_out += t.ml + t.mr; t.migrated_in += t.al + t.ar;
      // (the trusted removal reads nothing back on its own: its flag - an id out of range or listed twice - rides on this wait; ADVICE r4)
      T->pin[8 * (size_t)i + 4] = 0u;
      if (t.ml + t.mr) {
        if (T->pin_dev) { FlagTile F; F.src = t.w->mig_cnt.p; F.dst = T->pin_dev + 8 * (size_t)i + 4; F.words = 1; F.pad = 0; hand_flags.push_back(F); }
        else MGF_HIP_TRY(hipMemcpyAsync(T->pin + 8 * (size_t)i + 4, t.w->mig_cnt.p, 4, hipMemcpyDeviceToHost, s));
      }
    }
    for (size_t i0 = 0; i0 < hand_flags.size(); i0 += kTileBatch) {
      FlagBatch A;
      memset(&A, 0, sizeof(A));
      for (size_t k = 0; k < (size_t)kTileBatch && i0 + k < hand_flags.size(); ++k) A.t[k] = hand_flags[i0 + k];
      k_fetch_flags<<<1, 16 * kTileBatch, 0, s>>>(A);
      LAUNCH_CHECK();
    }
    MGF_HIP_TRY(hipStreamSynchronize(s)); ++T->host_waits;
    exchange_times();
    for (int i = 0; i < L; ++i)
      if (T->pin[8 * (size_t)i + 4]) return fail(MGF_ERR_HIP, "internal error: the hand-over's device-built list of leaving bodies held an id twice or out of range; the tile's bodies are no longer trustworthy");
  }
  return MGF_OK;
}


static mgf_status snapshot_batches(hipStream_t s, const std::vector<SnapTile>& sn, const std::vector<uint32_t>& blocks, int restore) {
  for (size_t i0 = 0; i0 < sn.size(); i0 += kTileBatch) {
    SnapBatch A;
    memset(&A, 0, sizeof(A));
    const size_t cnt = std::min((size_t)kTileBatch, sn.size() - i0);
    uint32_t mx = 0;
    for (size_t k = 0; k < cnt; ++k) { A.t[k] = sn[i0 + k]; mx = std::max(mx, blocks[i0 + k]); }
    if (!mx) continue;
    k_tick_snapshot<<<dim3(mx, (unsigned)cnt), kBlock, 0, s>>>(A, restore);
    LAUNCH_CHECK();
  }
  return MGF_OK;
}
// mgf_tiles_step: the tick, and - Solver::solve has no failure mode (solver.rs:72-78) - once more if a persistent solver launch gave up
// anywhere: every tile's owned bodies go back to where the tick found them (k_tick_snapshot), the tiles' worlds back off to the
// launch-per-frontier executor, and the whole tick - exchanges and all, on every rank: they agreed on the status - is repeated.
extern "C" mgf_status mgf_tiles_step(mgf_tiles* T, float dt, int32_t iters, mgf_step_stats* stats) {
  if (!T) return fail(MGF_ERR_INVALID, "tiles is NULL");
  if (iters < 0) return fail(MGF_ERR_INVALID, "iters must be >= 0");
  MGF_TRY(ctx_bind(T->ctx));
  hipStream_t s = T->ctx->stream;
  const int L = (int)T->t.size();
  if (T->retry_lost) {
    std::vector<SnapTile> sn;
    std::vector<uint32_t> blocks;
    for (int i = 0; i < L; ++i) {
      mgf_world* w = T->t[(size_t)i].w;
      MGF_TRY(world_identity(w));
      if (!w->n_owned) continue;
      MGF_TRY(w->tick_snap.ensure((size_t)kTickSnapWords * w->n_owned, s));
      SnapTile S;
      S.B = w->bodies(); S.n = w->n_owned; S.pad = 0; S.snap = w->tick_snap.p;
      sn.push_back(S); blocks.push_back(nblk(w->n_owned));
    }
    MGF_TRY(snapshot_batches(s, sn, blocks, 0));
  }
  bool gave_up = false;
  mgf_status st = tiles_step_once(T, dt, iters, stats, &gave_up);
  if (st == MGF_OK || !gave_up || !T->retry_lost) return st;
  const std::string first_msg = mgf_last_error();
  for (int i = 0; i < L; ++i) {
    mgf_world* w = T->t[(size_t)i].w;
    w->n = w->n_owned;
    w->constraints_ready = false; w->solve_pending = false;
    w->invalidate_tick_caches();
    if (w->n_owned) {
      SnapTile S;
      S.B = w->bodies(); S.n = w->n_owned; S.pad = 0; S.snap = w->tick_snap.p;
      MGF_TRY(snapshot_batches(s, std::vector<SnapTile>{S}, std::vector<uint32_t>{nblk(w->n_owned)}, 1));
    }
    MGF_HIP_TRY(hipMemsetAsync(w->word(kWSolverAbort), 0, 4, s));  // the solvers' abort flag
    if (w->abort_backoff == 0) { w->abort_backoff = w->abort_backoff_next; w->abort_backoff_next = std::min(2u * w->abort_backoff_next, 4096u); }
    ++w->n_solver_abort_fallbacks;
  }
  MGF_HIP_TRY(hipStreamSynchronize(s));
  ++T->ticks_retried;
  --T->ticks;  // (the repeated tick is the same tick)
  st = tiles_step_once(T, dt, iters, stats, &gave_up);
  if (st != MGF_OK) set_error("tiles: the tick was repeated after a solver launch gave up (%s) and failed again: %s", first_msg.c_str(), mgf_last_error());
  return st;
}
