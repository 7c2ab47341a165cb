// coverage.hip -- host side of thm_coverage (include/thermite_io.h): the per-base coverage tracks of a run, accumulated
// on the device over its batches from what is resident after thm_batch_run -- the compacted thm_aln records, the per-read
// offsets, the CIGAR words and digests of the CIGAR passes, and the ref -> @SQ table of the BAM encoder.  A track is a
// difference array over every base of every contig; only totals, finished runs of equal depth and windows of depths come
// back to the host.  The kernels are kernels_coverage.hip, the per-item functions and the layout coverage_device.h;
// DESIGN.md section 4.18.
#include <hip/hip_runtime.h>

#include <cstring>

#include "aligner_internal.h"
#include "coverage_device.h"
#include "io_internal.h"
#include "launch_io.h"

using namespace thm;

struct thm_coverage {
  thm_aligner* a = nullptr;
  uint32_t flags = 0, n_tracks = 0, n_sq = 0;
  std::vector<int32_t> h_ref_sq;  // what bam.ref_sq holds, for the checks of thm_coverage_add_view
  std::vector<uint64_t> h_base;   // [n_sq + 1] first entry of every contig in a track
  DArr<uint64_t> base;
  DArr<uint32_t> diff;            // [n_tracks * h_base[n_sq]]
  thm_cov_totals totals;
  // one batch's scratch
  DArr<uint8_t> track;
  DBuf d_tot;  // the totals (unsigned long long) and behind them the `bad` word
  // the view thm_coverage_add_view uploads
  DArr<uint64_t> v_off;
  DArr<thm_aln> v_alns;
  DArr<thm_aln_digest> v_dig;
  DArr<uint32_t> v_words;
  DArr<int32_t> v_stat;
  // a fetch's and a depth call's scratch and results
  DArr<uint64_t> tile_sum, tile_cnt, carry, point_at, scan_tmp, point_entry, point_live, run_at;
  DArr<uint32_t> point_depth, d_depth;
  DArr<thm_cov_run> d_runs;
  DArr<unsigned long long> d_stats;
  HBuf h_out;
  Event ev[2], ev_fetch[2];

  uint64_t track_entries() const { return h_base[n_sq]; }
  uint64_t held_bytes() const {
    return base.cap() + diff.cap() + track.cap() + d_tot.cap + v_off.cap() + v_alns.cap() + v_dig.cap() + v_words.cap() + v_stat.cap() + tile_sum.cap() +
           tile_cnt.cap() + carry.cap() + point_at.cap() + scan_tmp.cap() + point_entry.cap() + point_live.cap() + run_at.cap() + point_depth.cap() +
           d_depth.cap() + d_runs.cap() + d_stats.cap();
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
  b.n_refs = (uint32_t)a->ix->refs.size();
  b.n_sq = c->n_sq;
  b.flags = c->flags;
  b.ref_sq = a->bam.ref_sq;
  b.base = c->base;
  HIPCHK(a, ensure_events(c->ev));
  HIPCHK(a, c->track.ensure(n_alns, 16));
  HIPCHK(a, c->d_tot.ensure((cov::N_TOTALS + 1) * 8));
  CovCountParams cp;
  cp.b = b;
  cp.track = c->track;
  cp.totals = c->d_tot.as<unsigned long long>();
  cp.bad = cp.totals + cov::N_TOTALS;
  HIPCHK(a, hipEventRecord(c->ev[0], st));
  HIPCHK(a, hipMemsetAsync(cp.totals, 0, cov::N_TOTALS * 8, st));
  HIPCHK(a, hipMemsetAsync(cp.bad, 0xff, 8, st));
  HIPCHK(a, launch_cov_count(cp, a->n_cu, st));
  unsigned long long h_tot[cov::N_TOTALS + 1];
  HIPCHK(a, hipMemcpyAsync(h_tot, cp.totals, sizeof h_tot, hipMemcpyDeviceToHost, st));
  HIPCHK(a, hipStreamSynchronize(st));
  if (h_tot[cov::N_TOTALS] != ~0ull)
    return fail(a, refused, "%s: alignment %llu has a ref without an @SQ line, a CIGAR range outside the pool, or ends beyond its contig", who,
                h_tot[cov::N_TOTALS]);
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
  uint64_t* batch = (uint64_t*)&info->batch;
  uint64_t* total = (uint64_t*)&c->totals;
  for (int k = 0; k < cov::N_TOTALS; k++) {
    batch[k] = h_tot[k];
    total[k] += h_tot[k];
  }
  info->held_bytes = c->held_bytes();
  return THM_OK;
}

// the checks of thm_coverage_add_view, on the host before anything goes up
int check_view(thm_coverage* c, const thm_cigar_view* v) {
  thm_aligner* a = c->a;
  const char* who = "thm_coverage_add_view";
  const thm_index* ix = a->ix;
  const uint64_t n = v->n_reads, n_alns = v->n_alns, n_words = v->n_cigar_words;
  if ((n && !v->read_aln_off) || (n_alns && (!v->alns || !v->digests || !n)) || (n_words && !v->cigar))
    return fail(a, THM_ERR_INVALID_ARG, "%s: null offsets, alignments, digests or words", who);
  if (n) {
    if (v->read_aln_off[0] != 0) return fail(a, THM_ERR_INVALID_ARG, "%s: read_aln_off[0] must be 0", who);
    for (uint64_t r = 0; r < n; r++)
      if (v->read_aln_off[r + 1] < v->read_aln_off[r]) return fail(a, THM_ERR_INVALID_ARG, "%s: the offsets descend at read %llu", who, (unsigned long long)r);
    if (v->read_aln_off[n] != n_alns)
      return fail(a, THM_ERR_INVALID_ARG, "%s: the offsets end at %llu, the view has %llu alignments", who, (unsigned long long)v->read_aln_off[n], (unsigned long long)n_alns);
  }
  for (uint64_t i = 0; i < n_alns; i++) {
    const thm_aln& al = v->alns[i];
    const thm_aln_digest& d = v->digests[i];
    const unsigned long long at = i;
    if (al.aln_type > THM_ALN_INTERGENIC) return fail(a, THM_ERR_INVALID_ARG, "%s: alignment %llu: aln_type %u is none", who, at, (unsigned)al.aln_type);
    if (al.aln_type == THM_ALN_EXONIC && al.tx_or_gene_idx >= ix->txs.size())
      return fail(a, THM_ERR_INVALID_ARG, "%s: alignment %llu: tx_or_gene_idx %u is outside the index's %zu transcripts", who, at, al.tx_or_gene_idx, ix->txs.size());
    if (al.aln_type == THM_ALN_INTRONIC && al.tx_or_gene_idx >= ix->genes.size())
      return fail(a, THM_ERR_INVALID_ARG, "%s: alignment %llu: tx_or_gene_idx %u is outside the index's %zu genes", who, at, al.tx_or_gene_idx, ix->genes.size());
    if (al.ref_id >= c->h_ref_sq.size() || c->h_ref_sq[al.ref_id] < 0 || (uint32_t)c->h_ref_sq[al.ref_id] >= c->n_sq)
      return fail(a, THM_ERR_INVALID_ARG, "%s: alignment %llu: ref_id %u has no @SQ line", who, at, al.ref_id);
    if (d.cigar_off > n_words || d.n_cigar > n_words - d.cigar_off)
      return fail(a, THM_ERR_INVALID_ARG, "%s: alignment %llu: CIGAR words [%llu, +%u) are outside the pool of %llu", who, at, (unsigned long long)d.cigar_off, d.n_cigar,
                  (unsigned long long)n_words);
    const uint32_t s = (uint32_t)c->h_ref_sq[al.ref_id];
    const uint64_t len = c->h_base[s + 1] - c->h_base[s] - 1;
    if (al.ystart > len || d.ref_len > len - al.ystart)
      return fail(a, THM_ERR_INVALID_ARG, "%s: alignment %llu: position %llu + %llu lies beyond the %llu bases of its contig", who, at, (unsigned long long)al.ystart,
                  (unsigned long long)d.ref_len, (unsigned long long)len);
  }
  return THM_OK;
}

// tile sums and counts of diff[0, n) (entries of one track from `first` on) and the scan of the sums
int tile_pass(thm_coverage* c, CovTileParams& p, bool counts) {
  thm_aligner* a = c->a;
  hipStream_t st = a->stream;
  const uint64_t nt = cov::n_tiles(p.n);
  HIPCHK(a, c->tile_sum.ensure(nt + 1));
  HIPCHK(a, c->tile_cnt.ensure(nt + 1));
  HIPCHK(a, c->carry.ensure(nt + 2));
  HIPCHK(a, c->point_at.ensure(nt + 2));
  p.tile_sum = c->tile_sum;
  p.tile_cnt = c->tile_cnt;
  p.carry = c->carry;
  p.point_at = c->point_at;
  HIPCHK(a, launch_cov_tiles(p, st));
  if (const int rc = scan_u64(a, c->scan_tmp, p.tile_sum, c->carry, nt, st); rc != THM_OK) return rc;
  if (counts)
    if (const int rc = scan_u64(a, c->scan_tmp, p.tile_cnt, c->point_at, nt, st); rc != THM_OK) return rc;
  return THM_OK;
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
  c->n_sq = (uint32_t)sq.size();
  memset(&c->totals, 0, sizeof c->totals);
  c->h_base.assign(sq.size() + 1, 0);
  for (size_t s = 0; s < sq.size(); s++) c->h_base[s + 1] = c->h_base[s] + sq[s].second + 1;
  const uint64_t entries = c->n_tracks * c->track_entries();
  const unsigned long long need = entries * 4 + c->h_base.size() * 8;
  if (max_bytes && need > max_bytes) {
    delete c;
    return fail(a, THM_ERR_OOM, "thm_coverage_create: %u tracks over %zu contigs need %llu bytes, the cap is %llu", cov::n_tracks(flags), sq.size(), need,
                (unsigned long long)max_bytes);
  }
  const size_t n_refs = ix->refs.size();
  c->h_ref_sq.assign(n_refs, -1);
  // (allocated to the byte: the arrays are the object's size, not a buffer that grows)
  hipError_t e = hipMalloc(&c->base.b.p, c->h_base.size() * 8);
  if (e == hipSuccess) c->base.b.cap = c->h_base.size() * 8;
  if (e == hipSuccess) e = hipMalloc(&c->diff.b.p, entries * 4 + 16);
  if (e == hipSuccess) c->diff.b.cap = entries * 4 + 16;
  if (e == hipSuccess) e = hipMemcpy(c->base, c->h_base.data(), c->h_base.size() * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(c->diff, 0, entries * 4 + 16);
  if (e == hipSuccess && n_refs) e = hipMemcpy(c->h_ref_sq.data(), a->bam.ref_sq, n_refs * 4, hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    delete c;
    return fail(a, e == hipErrorOutOfMemory ? THM_ERR_OOM : THM_ERR_HIP, "thm_coverage_create: %s (%llu bytes needed, the cap is %llu)", hipGetErrorString(e), need,
                (unsigned long long)max_bytes);
  }
  *out = c;
  return THM_OK;
}

void thm_coverage_free(thm_coverage* c) {
  if (!c) return;
  int cur = 0;
  (void)hipGetDevice(&cur);
  (void)hipSetDevice(c->a->device);
  (void)hipStreamSynchronize(c->a->stream);
  delete c;
  (void)hipSetDevice(cur);
}

int32_t thm_coverage_add(thm_coverage* c, thm_cov_info* info) {
  if (!c || !info) return THM_ERR_INVALID_ARG;
  memset(info, 0, sizeof(*info));
  thm_aligner* a = c->a;
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
  CovBatch b;
  memset(&b, 0, sizeof b);
  b.n_reads = a->n_reads;
  b.n_alns = z.n_alns;
  b.n_words = n_words;
  b.aln_off = a->ext.aln_off;
  b.alns = a->out.alns;
  b.digests = a->cig.dig;
  b.words = a->cig.words;
  b.status = z.any_failed ? a->reads.status : nullptr;
  return add_batch(c, "thm_coverage_add", THM_ERR_INTERNAL, b, info);
}

int32_t thm_coverage_add_view(thm_coverage* c, const thm_cigar_view* v, thm_cov_info* info) {
  if (!c || !v || !info) return THM_ERR_INVALID_ARG;
  memset(info, 0, sizeof(*info));
  thm_aligner* a = c->a;
  int rc = check_view(c, v);
  if (rc != THM_OK) return rc;
  HIPCHK(a, hipSetDevice(a->device));
  hipStream_t st = a->stream;
  const uint64_t n = v->n_reads, n_alns = v->n_alns, n_words = v->n_cigar_words;
  const uint64_t zero = 0;
  HIPCHK(a, c->v_off.ensure(n + 1));
  HIPCHK(a, c->v_alns.ensure(n_alns + 1));
  HIPCHK(a, c->v_dig.ensure(n_alns + 1));
  HIPCHK(a, c->v_words.ensure(n_words + 4));
  HIPCHK(a, hipMemcpyAsync(c->v_off, n ? v->read_aln_off : &zero, (n + 1) * 8, hipMemcpyHostToDevice, st));
  if (n_alns) HIPCHK(a, hipMemcpyAsync(c->v_alns, v->alns, n_alns * sizeof(thm_aln), hipMemcpyHostToDevice, st));
  if (n_alns) HIPCHK(a, hipMemcpyAsync(c->v_dig, v->digests, n_alns * sizeof(thm_aln_digest), hipMemcpyHostToDevice, st));
  if (n_words) HIPCHK(a, hipMemcpyAsync(c->v_words, v->cigar, n_words * 4, hipMemcpyHostToDevice, st));
  if (v->read_status && n) {
    HIPCHK(a, c->v_stat.ensure(n));
    HIPCHK(a, hipMemcpyAsync(c->v_stat, v->read_status, n * 4, hipMemcpyHostToDevice, st));
  }
  HIPCHK(a, hipStreamSynchronize(st));  // (`zero` and the caller's arrays have been read)
  CovBatch b;
  memset(&b, 0, sizeof b);
  b.n_reads = n;
  b.n_alns = n_alns;
  b.n_words = n_words;
  b.aln_off = c->v_off;
  b.alns = c->v_alns;
  b.digests = c->v_dig;
  b.words = c->v_words;
  b.status = v->read_status && n ? c->v_stat.get() : nullptr;
  return add_batch(c, "thm_coverage_add_view", THM_ERR_INVALID_ARG, b, info);
}

int32_t thm_coverage_fetch(thm_coverage* c, uint32_t track, uint32_t first_ref, uint32_t n_refs, thm_cov_view* out) {
  if (!c || !out) return THM_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  thm_aligner* a = c->a;
  if (track >= c->n_tracks) return fail(a, THM_ERR_INVALID_ARG, "thm_coverage_fetch: track %u of %u", track, c->n_tracks);
  if (first_ref > c->n_sq || n_refs > c->n_sq - first_ref)
    return fail(a, THM_ERR_INVALID_ARG, "thm_coverage_fetch: @SQ entries [%u, +%u) of %u", first_ref, n_refs, c->n_sq);
  HIPCHK(a, hipSetDevice(a->device));
  hipStream_t st = a->stream;
  HIPCHK(a, ensure_events(c->ev_fetch));
  HIPCHK(a, c->d_stats.ensure(4));
  const uint64_t g0 = c->h_base[first_ref], g1 = c->h_base[first_ref + n_refs];
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
    if (const int rc = tile_pass(c, tp, true); rc != THM_OK) return rc;
    HIPCHK(a, hipMemcpyAsync(&n_points, c->point_at + nt, 8, hipMemcpyDeviceToHost, st));
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
    if (const int rc = scan_u64(a, c->scan_tmp, tp.point_live, c->run_at, n_points, st, &n_runs); rc != THM_OK) return rc;
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
    rp.base = c->base;
    rp.n_sq = c->n_sq;
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
  if (ref_id >= c->n_sq) return fail(a, THM_ERR_INVALID_ARG, "thm_coverage_depth: refID %u of %u", ref_id, c->n_sq);
  const uint64_t len = c->h_base[ref_id + 1] - c->h_base[ref_id] - 1;
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
    CovTileParams tp;
    memset(&tp, 0, sizeof tp);
    tp.diff = c->diff + (uint64_t)track * c->track_entries() + c->h_base[ref_id];
    tp.n = start + n;
    tp.g0 = c->h_base[ref_id];
    if (const int rc = tile_pass(c, tp, false); rc != THM_OK) return rc;
    CovWindowParams wp;
    wp.diff = tp.diff;
    wp.carry = c->carry;
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
