// coverage.hip -- host side of thm_coverage (include/thermite_io.h): the per-base coverage tracks of a run, accumulated
// on the device over its batches from what is resident after thm_batch_run -- the compacted thm_aln records, the per-read
// offsets, the CIGAR words and digests of the CIGAR passes, and the ref -> @SQ table of the BAM encoder.  A track is a
// difference array over every base of every contig; only totals, finished runs of equal depth and windows of depths come
// back to the host.  The kernels are kernels_coverage.hip, the per-item functions and the layout coverage_device.h; the
// batch, the view's upload and checks, the contig layout, the totals and the tile pass are run_summary.h's, shared with
// quant.hip and pileup.hip.  DESIGN.md sections 4.18 and 4.20.
//
// Synchronisations of the stream.  add: thm_batch_sync's, one of fetch_batch_sizes, one of the CIGAR passes, one behind
// the count pass, one behind the deposit.  add_view: one behind the upload, then the last two.  fetch: one behind the
// tile scans (a range with entries), one behind the point scan (with change points), one at the end.  depth: one.
// reset: one.
#include <hip/hip_runtime.h>

#include <cstring>

#include "aligner_internal.h"
#include "coverage_device.h"
#include "io_internal.h"
#include "launch_io.h"
#include "run_summary.h"

using namespace thm;

struct thm_coverage {
  thm_aligner* a = nullptr;
  uint32_t flags = 0, n_tracks = 0;
  SqLayout sq;          // the contigs of a track
  DArr<uint32_t> diff;  // [n_tracks * sq.entries()]
  thm_cov_totals totals;
  // one batch's scratch
  DArr<uint8_t> track;
  BatchTotals<cov::N_TOTALS> tot;
  AlnView view;  // what thm_coverage_add_view uploads
  // a fetch's and a depth call's scratch and results
  TileScratch tiles;
  DArr<uint64_t> point_entry, point_live, run_at;
  DArr<uint32_t> point_depth, d_depth;
  DArr<thm_cov_run> d_runs;
  DArr<unsigned long long> d_stats;
  HBuf h_out;
  Event ev[2], ev_fetch[2];

  uint64_t track_entries() const { return sq.entries(); }
  uint64_t held_bytes() const {
    return sq.base.cap() + diff.cap() + track.cap() + tot.d.cap + view.cap() + tiles.cap() + point_entry.cap() + point_live.cap() + run_at.cap() +
           point_depth.cap() + d_depth.cap() + d_runs.cap() + d_stats.cap();
  }
};

namespace {

// One batch that stands on the device.  No array changes before the batch has passed the device's checks.
int add_batch(thm_coverage* c, const char* who, int refused, CovBatch b, thm_cov_info* info) {
  thm_aligner* a = c->a;
  hipStream_t st = a->stream;
  const uint64_t n_alns = b.n_alns;
  if (n_alns && !b.n_reads) return fail(a, THM_ERR_INTERNAL, "%s: %llu alignments of no read", who, (unsigned long long)n_alns);
  if (n_alns > 0xFFFFFFFFull - c->totals.n_alns)
    return fail(a, THM_ERR_INVALID_ARG, "%s: %llu alignments behind the %llu counted would be more than 2^32-1: a depth could wrap", who,
                (unsigned long long)n_alns, (unsigned long long)c->totals.n_alns);
  b.n_sq = c->sq.n_sq;
  b.flags = c->flags;
  b.base = c->sq.base;
  HIPCHK(a, ensure_events(c->ev));
  HIPCHK(a, c->track.ensure(n_alns, 16));
  HIPCHK(a, c->tot.reserve());
  CovCountParams cp;
  cp.b = b;
  cp.track = c->track;
  cp.totals = c->tot.totals();
  cp.bad = c->tot.bad();
  HIPCHK(a, hipEventRecord(c->ev[0], st));
  HIPCHK(a, c->tot.clear(st));
  HIPCHK(a, launch_cov_count(cp, a->n_cu, st));
  HIPCHK(a, c->tot.fetch(st));
  HIPCHK(a, hipStreamSynchronize(st));
  const unsigned long long* h_tot = c->tot.h;
  if (c->tot.refused())
    return fail(a, refused, "%s: alignment %llu has a ref without an @SQ line, a CIGAR range outside the pool, or ends beyond its contig", who,
                c->tot.first_bad());
  if (h_tot[cov::T_ALNS] != n_alns) return fail(a, THM_ERR_INTERNAL, "%s: %llu alignments counted of %llu", who, h_tot[cov::T_ALNS], (unsigned long long)n_alns);
  CovDepositParams dp;
  dp.b = b;
  dp.track = c->track;
  dp.diff = c->diff;
  dp.track_entries = c->track_entries();
  HIPCHK(a, launch_cov_deposit(dp, st));
  HIPCHK(a, hipEventRecord(c->ev[1], st));
  HIPCHK(a, hipStreamSynchronize(st));
  (void)elapsed_ms(c->ev[0], c->ev[1], &info->add_ms);
  c->tot.accumulate(&info->batch, &c->totals);
  info->held_bytes = c->held_bytes();
  return THM_OK;
}

// the checks of thm_coverage_add_view, on the host before anything goes up
int check_view(thm_coverage* c, const thm_cigar_view* v) {
  thm_aligner* a = c->a;
  const char* who = "thm_coverage_add_view";
  return check_cigar_view(a, who, v, c->sq.h_ref_sq,
                          [&](uint64_t i, const thm_aln& al, const thm_aln_digest& d) { return c->sq.check_contig(a, who, i, al, d.ref_len); });
}

}  // namespace

extern "C" {

int32_t thm_coverage_create(thm_aligner* a, uint32_t flags, uint64_t max_bytes, thm_coverage** out) {
  if (!out) return THM_ERR_INVALID_ARG;
  *out = nullptr;
  if (!a) return THM_ERR_INVALID_ARG;
  if (flags & ~(THM_COV_STRANDED | THM_COV_MULTI)) return fail(a, THM_ERR_INVALID_ARG, "thm_coverage_create: unknown bits in flags %#x", flags);
  const thm_index* ix = a->ix;
  HIPCHK(a, hipSetDevice(a->device));
  int rc = bam_tables_on_device(a);
  if (rc != THM_OK) return rc;
  std::vector<std::pair<std::string, uint64_t>> sq;
  (void)thm::sq_of_name(ix, &sq);
  thm_coverage* c = new thm_coverage();
  c->a = a;
  c->flags = flags;
  c->n_tracks = cov::n_tracks(flags);
  memset(&c->totals, 0, sizeof c->totals);
  c->sq.lay_out(sq);
  const uint64_t entries = c->n_tracks * c->track_entries();
  const unsigned long long need = entries * 4 + c->sq.h_base.size() * 8;
  if (max_bytes && need > max_bytes) {
    delete c;
    return fail(a, THM_ERR_OOM, "thm_coverage_create: %u tracks over %zu contigs need %llu bytes, the cap is %llu", cov::n_tracks(flags), sq.size(), need,
                (unsigned long long)max_bytes);
  }
  hipError_t e = c->sq.on_device(a);
  if (e == hipSuccess) e = alloc_exact(c->diff, entries * 4 + 16);
  if (e == hipSuccess) e = hipMemset(c->diff, 0, entries * 4 + 16);
  if (e != hipSuccess) {
    delete c;
    return fail(a, e == hipErrorOutOfMemory ? THM_ERR_OOM : THM_ERR_HIP, "thm_coverage_create: %s (%llu bytes needed, the cap is %llu)", hipGetErrorString(e), need,
                (unsigned long long)max_bytes);
  }
  *out = c;
  return THM_OK;
}

void thm_coverage_free(thm_coverage* c) { free_summary(c); }

int32_t thm_coverage_add(thm_coverage* c, thm_cov_info* info) {
  if (!c || !info) return THM_ERR_INVALID_ARG;
  memset(info, 0, sizeof(*info));
  CovBatch b{};
  if (const int rc = resident_batch(c->a, &b); rc != THM_OK) return rc;
  return add_batch(c, "thm_coverage_add", THM_ERR_INTERNAL, b, info);
}

int32_t thm_coverage_add_view(thm_coverage* c, const thm_cigar_view* v, thm_cov_info* info) {
  if (!c || !v || !info) return THM_ERR_INVALID_ARG;
  memset(info, 0, sizeof(*info));
  CovBatch b{};
  int rc = check_view(c, v);
  if (rc == THM_OK) rc = c->view.upload(c->a, v, &b);
  if (rc != THM_OK) return rc;
  return add_batch(c, "thm_coverage_add_view", THM_ERR_INVALID_ARG, b, info);
}

int32_t thm_coverage_fetch(thm_coverage* c, uint32_t track, uint32_t first_ref, uint32_t n_refs, thm_cov_view* out) {
  if (!c || !out) return THM_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  thm_aligner* a = c->a;
  if (track >= c->n_tracks) return fail(a, THM_ERR_INVALID_ARG, "thm_coverage_fetch: track %u of %u", track, c->n_tracks);
  if (first_ref > c->sq.n_sq || n_refs > c->sq.n_sq - first_ref)
    return fail(a, THM_ERR_INVALID_ARG, "thm_coverage_fetch: @SQ entries [%u, +%u) of %u", first_ref, n_refs, c->sq.n_sq);
  HIPCHK(a, hipSetDevice(a->device));
  hipStream_t st = a->stream;
  HIPCHK(a, ensure_events(c->ev_fetch));
  HIPCHK(a, c->d_stats.ensure(4));
  const uint64_t g0 = c->sq.h_base[first_ref], g1 = c->sq.h_base[first_ref + n_refs];
  CovTileParams tp;
  memset(&tp, 0, sizeof tp);
  tp.diff = c->diff + (uint64_t)track * c->track_entries() + g0;
  tp.n = g1 - g0;
  tp.g0 = g0;
  const uint64_t nt = cov::n_tiles(tp.n);
  HIPCHK(a, hipEventRecord(c->ev_fetch[0], st));
  HIPCHK(a, hipMemsetAsync(c->d_stats, 0, 3 * 8, st));
  unsigned long long n_points = 0, n_runs = 0, stats[3] = {0, 0, 0};
  if (nt) {
    if (const int rc = tile_pass(a, c->tiles, tp.diff, tp.n, true); rc != THM_OK) return rc;
    tp.carry = c->tiles.carry;
    tp.point_at = c->tiles.point_at;
    HIPCHK(a, hipMemcpyAsync(&n_points, c->tiles.point_at + nt, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(a, hipStreamSynchronize(st));
    if (n_points > tp.n) return fail(a, THM_ERR_INTERNAL, "thm_coverage_fetch: %llu change points among %llu entries", n_points, (unsigned long long)tp.n);
  }
  if (n_points) {
    HIPCHK(a, c->point_entry.ensure(n_points));
    HIPCHK(a, c->point_depth.ensure(n_points));
    HIPCHK(a, c->point_live.ensure(n_points + 1));
    HIPCHK(a, c->run_at.ensure(n_points + 2));
    tp.point_entry = c->point_entry;
    tp.point_depth = c->point_depth;
    tp.point_live = c->point_live;
    HIPCHK(a, launch_cov_points(tp, st));
    if (const int rc = scan_u64(a, c->tiles.scan_tmp, tp.point_live, c->run_at, n_points, st, &n_runs); rc != THM_OK) return rc;
    HIPCHK(a, hipStreamSynchronize(st));
    if (n_runs > n_points) return fail(a, THM_ERR_INTERNAL, "thm_coverage_fetch: %llu runs from %llu change points", n_runs, n_points);
  }
  HIPCHK(a, c->h_out.ensure(n_runs * sizeof(thm_cov_run) + 16));
  if (n_runs) {
    HIPCHK(a, c->d_runs.ensure(n_runs));
    CovRunParams rp;
    rp.point_entry = c->point_entry;
    rp.point_depth = c->point_depth;
    rp.run_at = c->run_at;
    rp.n_points = n_points;
    rp.base = c->sq.base;
    rp.n_sq = c->sq.n_sq;
    rp.runs = c->d_runs;
    rp.stats = c->d_stats;
    HIPCHK(a, launch_cov_runs(rp, st));
    HIPCHK(a, hipMemcpyAsync(c->h_out.p, c->d_runs, n_runs * sizeof(thm_cov_run), hipMemcpyDeviceToHost, st));
    HIPCHK(a, hipMemcpyAsync(stats, c->d_stats, sizeof stats, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(a, hipEventRecord(c->ev_fetch[1], st));
  HIPCHK(a, hipStreamSynchronize(st));
  (void)elapsed_ms(c->ev_fetch[0], c->ev_fetch[1], &out->fetch_ms);
  out->track = track;
  out->first_ref = first_ref;
  out->n_refs = n_refs;
  out->max_depth = (uint32_t)stats[2];
  out->n_runs = n_runs;
  out->runs = c->h_out.as<thm_cov_run>();
  out->n_covered = stats[0];
  out->n_bases = stats[1];
  out->totals = c->totals;
  return THM_OK;
}

int32_t thm_coverage_depth(thm_coverage* c, uint32_t track, uint32_t ref_id, uint64_t start, uint64_t n, thm_cov_depth_view* out) {
  if (!c || !out) return THM_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  thm_aligner* a = c->a;
  if (track >= c->n_tracks) return fail(a, THM_ERR_INVALID_ARG, "thm_coverage_depth: track %u of %u", track, c->n_tracks);
  if (ref_id >= c->sq.n_sq) return fail(a, THM_ERR_INVALID_ARG, "thm_coverage_depth: refID %u of %u", ref_id, c->sq.n_sq);
  const uint64_t len = c->sq.len(ref_id);
  if (n > cov::MAX_DEPTH_WINDOW || start > len || n > len - start)
    return fail(a, THM_ERR_INVALID_ARG, "thm_coverage_depth: the window [%llu, +%llu) must hold at most 2^24 bases and lie inside the %llu bases of refID %u",
                (unsigned long long)start, (unsigned long long)n, (unsigned long long)len, ref_id);
  HIPCHK(a, hipSetDevice(a->device));
  hipStream_t st = a->stream;
  HIPCHK(a, ensure_events(c->ev_fetch));
  HIPCHK(a, c->h_out.ensure(n * 4 + 16));
  HIPCHK(a, hipEventRecord(c->ev_fetch[0], st));
  if (n) {
    HIPCHK(a, c->d_depth.ensure(n));
    CovWindowParams wp;
    wp.diff = c->diff + (uint64_t)track * c->track_entries() + c->sq.h_base[ref_id];
    // (held_bytes is the same whether a fetch or a depth call came first: both size the scratch of the count scan)
    HIPCHK(a, c->tiles.point_at.ensure(cov::n_tiles(start + n) + 2));
    if (const int rc = tile_pass(a, c->tiles, wp.diff, start + n, false); rc != THM_OK) return rc;
    wp.carry = c->tiles.carry;
    wp.start = start;
    wp.n = n;
    wp.out = c->d_depth;
    HIPCHK(a, launch_cov_window(wp, st));
    HIPCHK(a, hipMemcpyAsync(c->h_out.p, c->d_depth, n * 4, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(a, hipEventRecord(c->ev_fetch[1], st));
  HIPCHK(a, hipStreamSynchronize(st));
  (void)elapsed_ms(c->ev_fetch[0], c->ev_fetch[1], &out->depth_ms);
  out->n = n;
  out->depth = c->h_out.as<uint32_t>();
  return THM_OK;
}

int32_t thm_coverage_reset(thm_coverage* c) {
  if (!c) return THM_ERR_INVALID_ARG;
  thm_aligner* a = c->a;
  HIPCHK(a, hipSetDevice(a->device));
  HIPCHK(a, hipMemsetAsync(c->diff, 0, (uint64_t)c->n_tracks * c->track_entries() * 4, a->stream));
  HIPCHK(a, hipStreamSynchronize(a->stream));
  memset(&c->totals, 0, sizeof c->totals);
  return THM_OK;
}

}  // extern "C"
