// run_summary.h -- the host side that the summaries of a run share (quant.hip, coverage.hip, pileup.hip, cells.hip): each walks the
// alignments of a batch -- the one resident after thm_batch_run, or a caller's thm_cigar_view -- and accumulates something
// on the aligner's device.  Here are the description of that batch (thm::AlnBatch, launch_io.h) from either source, the
// host's checks of a view, the totals of a batch with the first refused alignment behind them, the contig layout and the
// tile pass of the two summaries over a difference array, and the free.  What a summary accumulates, and every pass
// behind its count kernel, is its own.  DESIGN.md section 4.20.
#ifndef THERMITE_RUN_SUMMARY_H
#define THERMITE_RUN_SUMMARY_H
#include <string>
#include <utility>
#include <vector>

#include "aligner_internal.h"
#include "launch_io.h"

// The batch that is resident after thm_batch_run -> *b: waits for the run, runs the two CIGAR passes as
// thm_batch_fetch_cigars does (THM_T_CIGAR belongs to that call and is left as it was) and refuses a malformed op stream.
// Synchronises the stream as thm_batch_sync, fetch_batch_sizes and run_cigar_passes do; the aligner's device is current.
int resident_batch(thm_aligner* a, thm::AlnBatch* b);

// the device copy of a thm_cigar_view
struct AlnView {
  DArr<uint64_t> off;
  DArr<thm_aln> alns;
  DArr<thm_aln_digest> dig;
  DArr<uint32_t> words;
  DArr<int32_t> stat;
  size_t cap() const { return off.cap() + alns.cap() + dig.cap() + words.cap() + stat.cap(); }
  // A checked view -> the device and *b.  One synchronisation of the stream, in front of which `more` enqueues what else
  // of the caller's must have been read when the call returns (pileup's reads).  The aligner's device is current.
  template <class More>
  int upload(thm_aligner* a, const thm_cigar_view* v, thm::AlnBatch* b, More&& more) {
    HIPCHK(a, hipSetDevice(a->device));
    hipStream_t st = a->stream;
    const uint64_t n = v->n_reads, n_alns = v->n_alns, n_words = v->n_cigar_words;
    const uint64_t zero = 0;
    const bool with_status = v->read_status && n;
    HIPCHK(a, off.ensure(n + 1));
    HIPCHK(a, alns.ensure(n_alns + 1));
    HIPCHK(a, dig.ensure(n_alns + 1));
    HIPCHK(a, words.ensure(n_words + 4));
    HIPCHK(a, hipMemcpyAsync(off, n ? v->read_aln_off : &zero, (n + 1) * 8, hipMemcpyHostToDevice, st));
    if (n_alns) HIPCHK(a, hipMemcpyAsync(alns, v->alns, n_alns * sizeof(thm_aln), hipMemcpyHostToDevice, st));
    if (n_alns) HIPCHK(a, hipMemcpyAsync(dig, v->digests, n_alns * sizeof(thm_aln_digest), hipMemcpyHostToDevice, st));
    if (n_words) HIPCHK(a, hipMemcpyAsync(words, v->cigar, n_words * 4, hipMemcpyHostToDevice, st));
    if (with_status) {
      HIPCHK(a, stat.ensure(n));
      HIPCHK(a, hipMemcpyAsync(stat, v->read_status, n * 4, hipMemcpyHostToDevice, st));
    }
    if (const int rc = more(); rc != THM_OK) return rc;
    HIPCHK(a, hipStreamSynchronize(st));  // (`zero` and the caller's arrays have been read)
    b->n_reads = n;
    b->n_alns = n_alns;
    b->n_words = n_words;
    b->aln_off = off;
    b->alns = alns;
    b->digests = dig;
    b->words = words;
    b->status = with_status ? stat.get() : nullptr;
    b->n_refs = (uint32_t)a->ix->refs.size();
    b->ref_sq = a->bam.ref_sq;
    return THM_OK;
  }
  int upload(thm_aligner* a, const thm_cigar_view* v, thm::AlnBatch* b) {
    return upload(a, v, b, [] { return (int)THM_OK; });
  }
};

// The checks of a thm_*_add_view, on the host before anything goes up: the arrays are there, the offsets begin at 0,
// ascend and end at n_alns, and every alignment has a type, an index inside the index's tables for it, a ref with an
// @SQ line (h_ref_sq: what bam.ref_sq holds) and its words inside the pool.  Behind these, per_aln(i, alignment, digest)
// makes the summary's own checks of alignment i and returns THM_OK or what fail() gave it.
template <class PerAln>
int check_cigar_view(thm_aligner* a, const char* who, const thm_cigar_view* v, const std::vector<int32_t>& h_ref_sq, PerAln&& per_aln) {
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
    if (al.ref_id >= h_ref_sq.size() || h_ref_sq[al.ref_id] < 0) return fail(a, THM_ERR_INVALID_ARG, "%s: alignment %llu: ref_id %u has no @SQ line", who, at, al.ref_id);
    if (d.cigar_off > n_words || d.n_cigar > n_words - d.cigar_off)
      return fail(a, THM_ERR_INVALID_ARG, "%s: alignment %llu: CIGAR words [%llu, +%u) are outside the pool of %llu", who, at, (unsigned long long)d.cigar_off, d.n_cigar,
                  (unsigned long long)n_words);
    if (const int rc = per_aln(i, al, d); rc != THM_OK) return rc;
  }
  return THM_OK;
}

// The contigs of coverage_device.h's layout, one entry more than bases each, in @SQ order, and the ref -> @SQ table the
// host checks a view with: what thm_coverage and thm_pileup keep of it on both sides.
struct SqLayout {
  uint32_t n_sq = 0;
  std::vector<int32_t> h_ref_sq;  // [n_refs] what bam.ref_sq holds, once on_device has run
  std::vector<uint64_t> h_base;   // [n_sq + 1] first entry of every contig
  DArr<uint64_t> base;            // ... on the device
  uint64_t entries() const { return h_base[n_sq]; }
  uint64_t len(uint32_t s) const { return h_base[s + 1] - h_base[s] - 1; }
  // from the @SQ lines (name, bases) of thm::sq_of_name: nothing of the device is touched, so a cap can still refuse
  void lay_out(const std::vector<std::pair<std::string, uint64_t>>& sq) {
    n_sq = (uint32_t)sq.size();
    h_base.assign(sq.size() + 1, 0);
    for (size_t s = 0; s < sq.size(); s++) h_base[s + 1] = h_base[s] + sq[s].second + 1;
  }
  // The contig checks of alignment i of a view, behind check_cigar_view's: its ref's @SQ entry is one of the layout's,
  // and [ystart, ystart + ref_len) lies inside that contig.
  int check_contig(thm_aligner* a, const char* who, uint64_t i, const thm_aln& al, uint64_t ref_len) const {
    const uint32_t s = (uint32_t)h_ref_sq[al.ref_id];
    if (s >= n_sq) return fail(a, THM_ERR_INVALID_ARG, "%s: alignment %llu: ref_id %u has no @SQ line", who, (unsigned long long)i, al.ref_id);
    if (al.ystart > len(s) || ref_len > len(s) - al.ystart)
      return fail(a, THM_ERR_INVALID_ARG, "%s: alignment %llu: position %llu + %llu lies beyond the %llu bases of its contig", who, (unsigned long long)i,
                  (unsigned long long)al.ystart, (unsigned long long)ref_len, (unsigned long long)len(s));
    return THM_OK;
  }
  // base on the device and h_ref_sq from it (after bam_tables_on_device; the aligner's device is current)
  hipError_t on_device(thm_aligner* a);
};

// allocated to the byte: for the arrays that are an object's size, not a buffer that grows
template <class T>
hipError_t alloc_exact(DArr<T>& d, size_t bytes) {
  const hipError_t e = hipMalloc(&d.b.p, bytes);
  if (e == hipSuccess) d.b.cap = bytes;
  return e;
}

// The N totals of one batch as its count kernel sums them, and behind them the `bad` word: the first alignment that
// fails a check of the device's (an atomic minimum; ~0: none).
template <int N>
struct BatchTotals {
  DBuf d;
  unsigned long long h[N + 1];  // what came back, once the stream has been synchronised behind fetch()
  hipError_t reserve() { return d.ensure((N + 1) * 8); }
  unsigned long long* totals() const { return d.as<unsigned long long>(); }
  unsigned long long* bad() const { return totals() + N; }
  hipError_t clear(hipStream_t st) {
    const hipError_t e = hipMemsetAsync(totals(), 0, N * 8, st);
    return e != hipSuccess ? e : hipMemsetAsync(bad(), 0xff, 8, st);
  }
  hipError_t fetch(hipStream_t st) { return hipMemcpyAsync(h, totals(), sizeof h, hipMemcpyDeviceToHost, st); }
  bool refused() const { return h[N] != ~0ull; }
  unsigned long long first_bad() const { return h[N]; }
  // a batch that has gone in: its totals into *batch and onto *total (structs of N 64-bit counters in the kernels' order)
  template <class Totals>
  void accumulate(Totals* batch, Totals* total) const {
    static_assert(sizeof(Totals) == N * sizeof(uint64_t), "the totals are N 64-bit counters");
    uint64_t* b = (uint64_t*)batch;
    uint64_t* t = (uint64_t*)total;
    for (int k = 0; k < N; k++) {
      b[k] = h[k];
      t[k] += h[k];
    }
  }
};

// scratch of the tile pass over a range of a difference array
struct TileScratch {
  DArr<uint64_t> tile_sum, tile_cnt, carry, point_at, scan_tmp;
  size_t cap() const { return tile_sum.cap() + tile_cnt.cap() + carry.cap() + point_at.cap() + scan_tmp.cap(); }
};
// Tile sums and counts of diff[0, n) (cov_tiles_kernel) and the scan of the sums into t.carry; with want_counts the scan
// of the counts into t.point_at as well (without, point_at is not touched).  Nothing is synchronised.
int tile_pass(thm_aligner* a, TileScratch& t, const uint32_t* diff, uint64_t n, bool want_counts);

// the body of thm_*_free: the aligner's stream has finished before the buffers go
template <class Summary>
void free_summary(Summary* s) {
  if (!s) return;
  int cur = 0;
  (void)hipGetDevice(&cur);
  (void)hipSetDevice(s->a->device);
  (void)hipStreamSynchronize(s->a->stream);
  delete s;
  (void)hipSetDevice(cur);
}

#endif
