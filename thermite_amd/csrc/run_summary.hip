// run_summary.hip -- what run_summary.h declares and does not define in place: the resident batch, the contig layout's
// way to the device and the tile pass.
#include <hip/hip_runtime.h>

#include "coverage_device.h"
#include "run_summary.h"

using namespace thm;

int resident_batch(thm_aligner* a, AlnBatch* b) {
  int rc = thm_batch_sync(a);
  if (rc != THM_OK) return rc;
  HIPCHK(a, hipSetDevice(a->device));
  BatchSizes z;
  rc = fetch_batch_sizes(a, nullptr, nullptr, nullptr, &z);
  if (rc != THM_OK) return rc;
  // the two CIGAR passes, as thm_batch_fetch_cigars runs them (THM_T_CIGAR belongs to that call)
  uint64_t n_words = 0;
  unsigned any_flags = 0;
  const float t_cigar = a->timings[THM_T_CIGAR];
  rc = run_cigar_passes(a, compacted_cigar_params(a, z), z.n_alns, &n_words, &any_flags);
  a->timings[THM_T_CIGAR] = t_cigar;
  if (rc != THM_OK) return rc;
  if (any_flags & THM_DIGEST_MALFORMED) return fail(a, THM_ERR_INTERNAL, "malformed op stream in the compacted pool");
  b->n_reads = a->n_reads;
  b->n_alns = z.n_alns;
  b->n_words = n_words;
  b->aln_off = a->ext.aln_off;
  b->alns = a->out.alns;
  b->digests = a->cig.dig;
  b->words = a->cig.words;
  b->status = z.any_failed ? a->reads.status : nullptr;
  b->n_refs = (uint32_t)a->ix->refs.size();
  b->ref_sq = a->bam.ref_sq;
  return THM_OK;
}

hipError_t SqLayout::on_device(thm_aligner* a) {
  const size_t n_refs = a->ix->refs.size();
  h_ref_sq.assign(n_refs, -1);
  hipError_t e = alloc_exact(base, h_base.size() * 8);
  if (e == hipSuccess) e = hipMemcpy(base, h_base.data(), h_base.size() * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess && n_refs) e = hipMemcpy(h_ref_sq.data(), a->bam.ref_sq, n_refs * 4, hipMemcpyDeviceToHost);
  return e;
}

int tile_pass(thm_aligner* a, TileScratch& t, const uint32_t* diff, uint64_t n, bool want_counts) {
  hipStream_t st = a->stream;
  const uint64_t nt = cov::n_tiles(n);
  HIPCHK(a, t.tile_sum.ensure(nt + 1));
  HIPCHK(a, t.tile_cnt.ensure(nt + 1));
  HIPCHK(a, t.carry.ensure(nt + 2));
  if (want_counts) HIPCHK(a, t.point_at.ensure(nt + 2));
  // (the tile kernel reads diff and n of its parameters and writes tile_sum and tile_cnt: the other fields are the
  // point kernel's, which coverage.hip fills in behind this pass)
  CovTileParams p{};
  p.diff = diff;
  p.n = n;
  p.tile_sum = t.tile_sum;
  p.tile_cnt = t.tile_cnt;
  HIPCHK(a, launch_cov_tiles(p, st));
  if (const int rc = scan_u64(a, t.scan_tmp, t.tile_sum, t.carry, nt, st); rc != THM_OK) return rc;
  if (want_counts)
    if (const int rc = scan_u64(a, t.scan_tmp, t.tile_cnt, t.point_at, nt, st); rc != THM_OK) return rc;
  return THM_OK;
}
