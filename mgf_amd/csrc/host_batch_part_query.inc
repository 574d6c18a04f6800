// The part-aware body passes of a batch's queries (k_batch_part_query.h): what the entry points of host_batch_query.inc, _query_dev.inc,
// _observe.inc, _sensor.inc, _feeler.inc, _zone.inc and _nearest.inc launch in the place of their own body pass when the batch holds
// part storage and option "part_queries" is 1 (batch_part_queries).  Part of the single translation unit mgf_hip.hip (included there,
// in order, behind host_batch.inc and ahead of host_batch_query.inc); not compiled on its own.
//
// A helper is the ONE launch it stands for - the same grid, the same argument block with the part rows beside it, LDS of 36 bytes a
// body where the rows carry a count - and nothing else: the prologue, the plan, the uploads, the passes behind the body pass, the
// counters and the waits stay the caller's, so a call makes today's number of launches, whatever the number of worlds, and a _dev
// form still makes no host wait.  The cameras have no such helper: mgf_batch_cast_cameras(_dev) stay refused (batch_single_parts).

// does this batch answer its queries part by part?  (without part storage the option changes no launch)
static bool batch_part_queries(const mgf_batch* b) { return b->parts && b->part_queries; }

static BatchPartRows batch_part_rows(const mgf_batch* b) {
  BatchPartRows P;
  P.ctor = b->dm[mgf_batch::ACTOR].p; P.wp0 = b->dm[mgf_batch::AWP0].p; P.wp1 = b->dm[mgf_batch::AWP1].p;
  return P;
}
// rows | rows | kBatchQueryRed words | counts (PqLds): at most 36 KB + 256 bytes, below the 64 KB a launch gets without an attribute
static uint32_t batch_pq_lds(const mgf_batch* b) { return 36u * batch_nmax(b) + 16u * kBatchQueryRed; }
static_assert(36u * MGF_BATCH_MAX_BODIES + 16u * kBatchQueryRed <= 48u * 1024u, "the part-aware fronts' LDS needs no attribute call");

// the body pass of the ray casts and sweeps: Q = ParticleIn or MovingIn; SRC: where a work item comes from (k_batch_query.h)
template <int SRC, class Q>
static mgf_status batch_pq_bodies(mgf_batch* b, const BatchQueryArgs& A, const Q* q, const BatchItemSrc& S, unsigned grid) {
  hipStream_t s = b->ctx->stream;
  if constexpr (std::is_same<Q, ParticleIn>::value) k_batch_pq_ray<SRC><<<grid, kBatchBlock, batch_pq_lds(b), s>>>(A, batch_part_rows(b), q, S);
  else k_batch_pq_sweep<SRC><<<grid, kBatchBlock, batch_pq_lds(b), s>>>(A, batch_part_rows(b), q, S);
  LAUNCH_CHECK();
  return MGF_OK;
}
static mgf_status batch_pq_sensor(mgf_batch* b, const BatchSensorArgs& A, unsigned grid) {
  k_batch_pq_sensor<<<grid, kBatchBlock, batch_pq_lds(b), b->ctx->stream>>>(A, batch_part_rows(b));
  LAUNCH_CHECK();
  return MGF_OK;
}
static mgf_status batch_pq_feeler(mgf_batch* b, const BatchFeelerArgs& A, unsigned grid) {
  k_batch_pq_feeler<<<grid, kBatchBlock, batch_pq_lds(b), b->ctx->stream>>>(A, batch_part_rows(b));
  LAUNCH_CHECK();
  return MGF_OK;
}
// the box fronts: lds is what the caller gives the kernel this one stands for (32 bytes a body: U.lds, batch_zone_lds)
template <bool FILL>
static mgf_status batch_pq_overlap(mgf_batch* b, const BatchOverlapArgs& A, unsigned grid, uint32_t lds) {
  k_batch_pq_overlap<FILL><<<grid, kBatchBlock, lds, b->ctx->stream>>>(A, batch_part_rows(b));
  LAUNCH_CHECK();
  return MGF_OK;
}
template <int SRC>
static mgf_status batch_pq_zone(mgf_batch* b, const BatchZoneArgs& A, const BatchItemSrc& S, unsigned grid, uint32_t lds) {
  k_batch_pq_zone<SRC><<<grid, kBatchBlock, lds, b->ctx->stream>>>(A, batch_part_rows(b), S);
  LAUNCH_CHECK();
  return MGF_OK;
}
template <int SRC>
static mgf_status batch_pq_nearest(mgf_batch* b, const BatchNearestArgs& A, const BatchItemSrc& S, unsigned grid, uint32_t lds) {
  k_batch_pq_nearest<SRC><<<grid, kBatchBlock, lds, b->ctx->stream>>>(A, batch_part_rows(b), S);
  LAUNCH_CHECK();
  return MGF_OK;
}
