// pileup.hip -- host side of thm_pileup (include/thermite_io.h): the per-base allele counts of a run, accumulated on the
// device over its batches from what is resident after thm_batch_run -- the raw reads, the compacted thm_aln records, the
// per-read offsets, the CIGAR words and digests of the CIGAR passes, the ref -> @SQ table of the BAM encoder -- and the
// index's text.  The depth is a difference array as thm_coverage keeps one; the observations that differ from the
// reference are a sorted table of (key, count), merged batch by batch as quant.hip merges its junction rows; only totals
// and rows of sites come back to the host.  The kernels are kernels_pileup.hip, the per-item functions and the key
// pileup_device.h; the batch, the view's upload and checks, the contig layout, the totals and the tile pass are
// run_summary.h's, shared with quant.hip and coverage.hip.  DESIGN.md sections 4.19 and 4.20.
//
// Synchronisations of the stream.  add: thm_batch_sync's, one of fetch_batch_sizes, one of the CIGAR passes, one behind
// the count pass, with events one in sort_reduce and with reduced rows one in merge_rows, one behind the deposit.
// add_view: one behind the upload (the reads go up in front of it), then as add from the count pass on.  fetch: one in
// row_bounds (a table with rows), one behind the scan of the kept rows (a range with rows), one at the end.  window: one
// in row_bounds, one at the end.  reset: one.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstring>

#include "aligner_internal.h"
#include "io_internal.h"
#include "launch_io.h"
#include "pileup_device.h"
#include "run_summary.h"

using namespace thm;

struct thm_pileup {
  thm_aligner* a = nullptr;
  uint32_t flags = 0;
  uint64_t max_bytes = 0, array_bytes = 0;
  SqLayout sq;           // the contigs of the depth
  DArr<uint64_t> tstart;
  DArr<uint32_t> diff;   // [sq.entries()]
  // the running event table, sorted by key, in tab[cur]; the other takes the next merge
  DArr<uint64_t> tab_key[2];
  DArr<uint32_t> tab_cnt[2];
  int cur = 0;
  uint64_t n_tab = 0;
  thm_pile_totals totals;
  // one batch's scratch
  DArr<uint64_t> ev_cnt, ev_off, aln_read, keys, skeys, flag, first, head_at, red_key, where, is_new, new_at, cat_key;
  DArr<uint32_t> red_cnt, cat_cnt;
  DArr<uint8_t> used;
  BatchTotals<pile::N_TOTALS> tot;
  DBuf cub_tmp;  // hipcub's scratch
  // what thm_pileup_add_view uploads: the view, and the reads
  AlnView view;
  DArr<uint64_t> v_base_off;
  DArr<uint8_t> v_bases;
  // a fetch's and a window's scratch and results; tiles.scan_tmp is every scan's of the object, tiles.point_at stays empty
  TileScratch tiles;
  DArr<uint64_t> bounds, keep, site_at;
  DArr<thm_pile_site> d_sites;
  HBuf h_out;
  Event ev[2], ev_fetch[2];

  uint64_t entries() const { return sq.entries(); }
  uint64_t held_bytes() const {
    size_t n = tot.d.cap + cub_tmp.cap + view.cap() + tiles.cap();
    for (const DArr<uint64_t>* x : {&sq.base, &tstart, &tab_key[0], &tab_key[1], &ev_cnt, &ev_off, &aln_read, &keys, &skeys, &flag, &first, &head_at, &red_key, &where,
                                    &is_new, &new_at, &cat_key, &v_base_off, &bounds, &keep, &site_at})
      n += x->cap();
    for (const DArr<uint32_t>* x : {&diff, &tab_cnt[0], &tab_cnt[1], &red_cnt, &cat_cnt}) n += x->cap();
    return n + used.cap() + v_bases.cap() + d_sites.cap();
  }
};

namespace {

constexpr uint64_t ROW_BYTES = 12;  // a row of the table: the key and its count

// the index's text on the aligner's device (the view's pointer: the buffer begins 16 bytes in front of the text)
const uint8_t* text_of(const thm_aligner* a) { return a->dix->wide ? a->dix->view64.text : a->dix->view.text; }

// keys[0, n) sorted and reduced by key into red_key / red_cnt -> *m rows.  Synchronises the stream once.
int sort_reduce(thm_pileup* c, uint64_t n, uint64_t* m) {
  thm_aligner* a = c->a;
  hipStream_t st = a->stream;
  *m = 0;
  if (n == 0) return THM_OK;
  if (n > 0x7FFFFFFFull) return fail(a, THM_ERR_UNSUPPORTED, "thm_pileup: 2^31 events or more in one batch");
  HIPCHK(a, c->skeys.ensure(n));
  HIPCHK(a, c->flag.ensure(n + 1));
  HIPCHK(a, c->first.ensure(n + 2));
  const int bits = pile::key_bits(c->entries());
  size_t tmp_bytes = 0;
  HIPCHK(a, hipcub::DeviceRadixSort::SortKeys(nullptr, tmp_bytes, c->keys.get(), c->skeys.get(), n, 0, bits, st));
  HIPCHK(a, c->cub_tmp.ensure(tmp_bytes + 16));
  HIPCHK(a, hipcub::DeviceRadixSort::SortKeys(c->cub_tmp.p, tmp_bytes, c->keys.get(), c->skeys.get(), n, 0, bits, st));
  PileReduceParams p;
  memset(&p, 0, sizeof p);
  p.skey = c->skeys;
  p.n = n;
  p.flag = c->flag;
  p.first = c->first;
  HIPCHK(a, launch_pile_heads(p, st));
  unsigned long long n_keys = 0;
  if (const int rc = scan_u64(a, c->tiles.scan_tmp, p.flag, c->first, n, st, &n_keys); rc != THM_OK) return rc;
  HIPCHK(a, hipStreamSynchronize(st));
  if (n_keys == 0 || n_keys > n) return fail(a, THM_ERR_INTERNAL, "thm_pileup: %llu keys among %llu events", n_keys, (unsigned long long)n);
  HIPCHK(a, c->head_at.ensure(n_keys + 1));
  HIPCHK(a, c->red_key.ensure(n_keys));
  HIPCHK(a, c->red_cnt.ensure(n_keys));
  p.head_at = c->head_at;
  p.red_key = c->red_key;
  p.red_cnt = c->red_cnt;
  p.n_keys = n_keys;
  HIPCHK(a, launch_pile_runs(p, st));
  *m = n_keys;
  return THM_OK;
}

// The reduced rows of a batch into the running table: rows whose key the table holds add to it in place; with new keys,
// the table's rows and the new ones are sorted together into the other of the two table buffers, and *swap says so: the
// caller swaps once nothing can fail any more.  Refuses, before any row changes, a table that would not fit the cap.
int merge_rows(thm_pileup* c, const char* who, uint64_t n_red, bool* swap, uint64_t* n_merged) {
  thm_aligner* a = c->a;
  hipStream_t st = a->stream;
  const uint64_t n_tab = c->n_tab;
  *swap = false;
  *n_merged = n_tab;
  if (n_red == 0) return THM_OK;
  HIPCHK(a, c->where.ensure(n_red));
  HIPCHK(a, c->is_new.ensure(n_red + 1));
  HIPCHK(a, c->new_at.ensure(n_red + 2));
  PileMergeParams p;
  memset(&p, 0, sizeof p);
  p.tab_key = c->tab_key[c->cur];
  p.n_tab = n_tab;
  p.red_key = c->red_key;
  p.red_cnt = c->red_cnt;
  p.n_red = n_red;
  p.where = c->where;
  p.is_new = c->is_new;
  p.new_at = c->new_at;
  HIPCHK(a, launch_pile_lookup(p, st));
  unsigned long long n_new = 0;
  if (const int rc = scan_u64(a, c->tiles.scan_tmp, p.is_new, c->new_at, n_red, st, &n_new); rc != THM_OK) return rc;
  HIPCHK(a, hipStreamSynchronize(st));
  if (n_new > n_red) return fail(a, THM_ERR_INTERNAL, "thm_pileup: %llu new keys among %llu rows", n_new, (unsigned long long)n_red);
  const uint64_t n_cat = n_tab + n_new;
  const unsigned long long need = c->array_bytes + n_cat * ROW_BYTES;
  if (c->max_bytes && need > c->max_bytes)
    return fail(a, THM_ERR_OOM, "%s: the arrays and a table of %llu rows need %llu bytes, the cap is %llu", who, (unsigned long long)n_cat, need,
                (unsigned long long)c->max_bytes);
  if (n_cat > 0x7FFFFFFFull) return fail(a, THM_ERR_UNSUPPORTED, "%s: 2^31 rows or more in the event table", who);
  if (n_new == 0) {
    p.dst_key = c->tab_key[c->cur];
    p.dst_cnt = c->tab_cnt[c->cur];
    HIPCHK(a, launch_pile_update(p, st));
    return THM_OK;
  }
  const int other = c->cur ^ 1;
  HIPCHK(a, c->tab_key[other].ensure(n_cat));
  HIPCHK(a, c->tab_cnt[other].ensure(n_cat));
  if (n_tab == 0) {
    // (the reduced rows are sorted and distinct: they are the table)
    p.dst_key = c->tab_key[other];
    p.dst_cnt = c->tab_cnt[other];
    HIPCHK(a, launch_pile_update(p, st));
  } else {
    HIPCHK(a, c->cat_key.ensure(n_cat));
    HIPCHK(a, c->cat_cnt.ensure(n_cat));
    const int bits = pile::key_bits(c->entries());
    size_t tmp_bytes = 0;
    HIPCHK(a, hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, c->cat_key.get(), c->tab_key[other].get(), c->cat_cnt.get(), c->tab_cnt[other].get(), n_cat, 0,
                                                 bits, st));
    HIPCHK(a, c->cub_tmp.ensure(tmp_bytes + 16));
    HIPCHK(a, hipMemcpyAsync(c->cat_key, c->tab_key[c->cur], n_tab * 8, hipMemcpyDeviceToDevice, st));
    HIPCHK(a, hipMemcpyAsync(c->cat_cnt, c->tab_cnt[c->cur], n_tab * 4, hipMemcpyDeviceToDevice, st));
    p.dst_key = c->cat_key;
    p.dst_cnt = c->cat_cnt;
    HIPCHK(a, launch_pile_update(p, st));
    HIPCHK(a, hipcub::DeviceRadixSort::SortPairs(c->cub_tmp.p, tmp_bytes, c->cat_key.get(), c->tab_key[other].get(), c->cat_cnt.get(), c->tab_cnt[other].get(), n_cat, 0,
                                                 bits, st));
  }
  *swap = true;
  *n_merged = n_cat;
  return THM_OK;
}

// One batch that stands on the device.  Nothing of the object changes before the batch has passed the device's checks
// and the table's cap.
int add_batch(thm_pileup* c, const char* who, int refused, PileBatch b, thm_pile_info* info) {
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
  b.tstart = c->tstart;
  b.text = text_of(a);
  HIPCHK(a, ensure_events(c->ev));
  HIPCHK(a, c->ev_cnt.ensure(n_alns + 1));
  HIPCHK(a, c->ev_off.ensure(n_alns + 2));
  HIPCHK(a, c->aln_read.ensure(n_alns + 1));
  HIPCHK(a, c->used.ensure(n_alns, 16));
  HIPCHK(a, c->tot.reserve());
  PileCountParams cp;
  cp.b = b;
  cp.ev_cnt = c->ev_cnt;
  cp.aln_read = c->aln_read;
  cp.used = c->used;
  cp.totals = c->tot.totals();
  cp.bad = c->tot.bad();
  HIPCHK(a, hipEventRecord(c->ev[0], st));
  HIPCHK(a, c->tot.clear(st));
  HIPCHK(a, launch_pile_count(cp, a->n_cu, st));
  unsigned long long n_events = 0;
  if (n_alns) {
    if (const int rc = scan_u64(a, c->tiles.scan_tmp, cp.ev_cnt, c->ev_off, n_alns, st, &n_events); rc != THM_OK) return rc;
  }
  HIPCHK(a, c->tot.fetch(st));
  HIPCHK(a, hipStreamSynchronize(st));
  const unsigned long long* h_tot = c->tot.h;
  if (c->tot.refused())
    return fail(a, refused,
                "%s: alignment %llu has a ref without an @SQ line, a CIGAR range outside the pool, ends beyond its contig, or its M + I + S is not its read's length",
                who, c->tot.first_bad());
  if (h_tot[pile::T_ALNS] != n_alns) return fail(a, THM_ERR_INTERNAL, "%s: %llu alignments counted of %llu", who, h_tot[pile::T_ALNS], (unsigned long long)n_alns);
  if (n_events != h_tot[pile::T_MISMATCHES] + h_tot[pile::T_DEL_BASES] + h_tot[pile::T_INS])
    return fail(a, THM_ERR_INTERNAL, "%s: %llu events scanned, %llu counted", who, n_events,
                h_tot[pile::T_MISMATCHES] + h_tot[pile::T_DEL_BASES] + h_tot[pile::T_INS]);
  PileExtractParams ep;
  ep.b = b;
  ep.ev_off = c->ev_off;
  ep.aln_read = c->aln_read;
  ep.used = c->used;
  ep.keys = nullptr;
  ep.diff = c->diff;
  bool swap = false;
  uint64_t n_merged = c->n_tab;
  if (n_events) {
    HIPCHK(a, c->keys.ensure(n_events));
    ep.keys = c->keys;
    HIPCHK(a, launch_pile_extract(ep, st));
    uint64_t n_red = 0;
    int rc = sort_reduce(c, n_events, &n_red);
    if (rc == THM_OK) rc = merge_rows(c, who, n_red, &swap, &n_merged);
    if (rc != THM_OK) return rc;
  }
  HIPCHK(a, launch_pile_deposit(ep, st));
  HIPCHK(a, hipEventRecord(c->ev[1], st));
  HIPCHK(a, hipStreamSynchronize(st));
  if (swap) c->cur ^= 1;
  c->n_tab = n_merged;
  (void)elapsed_ms(c->ev[0], c->ev[1], &info->add_ms);
  c->tot.accumulate(&info->batch, &c->totals);
  info->n_events = c->n_tab;
  info->held_bytes = c->held_bytes();
  return THM_OK;
}

// the checks of thm_pileup_add_view, on the host before anything goes up: the reads' offsets, then the view
int check_view(thm_pileup* c, const thm_cigar_view* v, const uint8_t* bases, const uint64_t* base_off) {
  thm_aligner* a = c->a;
  const char* who = "thm_pileup_add_view";
  const uint64_t n = v->n_reads;
  if (n) {
    if (!base_off) return fail(a, THM_ERR_INVALID_ARG, "%s: null offsets, alignments, digests or words", who);
    if (base_off[0] != 0) return fail(a, THM_ERR_INVALID_ARG, "%s: base_off[0] must be 0", who);
    for (uint64_t r = 0; r < n; r++)
      if (base_off[r + 1] < base_off[r]) return fail(a, THM_ERR_INVALID_ARG, "%s: base_off descends at read %llu", who, (unsigned long long)r);
    if (base_off[n] && !bases) return fail(a, THM_ERR_INVALID_ARG, "%s: null bases", who);
  }
  uint64_t r = 0;  // the read of alignment i: the alignments come in the order of their reads
  return check_cigar_view(a, who, v, c->sq.h_ref_sq, [&](uint64_t i, const thm_aln& al, const thm_aln_digest& d) {
    while (v->read_aln_off[r + 1] <= i) r++;
    if (const int rc = c->sq.check_contig(a, who, i, al, d.ref_len); rc != THM_OK) return rc;
    if ((d.flags & THM_DIGEST_LONG_RUN) || d.n_cigar == 0) return (int)THM_OK;
    const pile::Shape sh = pile::shape_of(v->cigar + d.cigar_off, d.n_cigar, al.ystart);
    if (sh.qlen != base_off[r + 1] - base_off[r])
      return fail(a, THM_ERR_INVALID_ARG, "%s: alignment %llu: its M + I + S is %llu, read %llu has %llu bases", who, (unsigned long long)i,
                  (unsigned long long)sh.qlen, (unsigned long long)r, (unsigned long long)(base_off[r + 1] - base_off[r]));
    return (int)THM_OK;
  });
}

// the rows of the entries [e0, e1) of the layout -> p.r0, p.r1; synchronises the stream
int row_bounds(thm_pileup* c, PileFetchParams& p, uint64_t e0, uint64_t e1) {
  thm_aligner* a = c->a;
  hipStream_t st = a->stream;
  memset(&p, 0, sizeof p);
  p.keys = c->tab_key[c->cur];
  p.cnts = c->tab_cnt[c->cur];
  p.n_tab = c->n_tab;
  p.e0 = e0;
  p.e1 = e1;
  p.base = c->sq.base;
  p.tstart = c->tstart;
  p.text = text_of(a);
  p.n_sq = c->sq.n_sq;
  if (c->n_tab == 0) return THM_OK;
  HIPCHK(a, c->bounds.ensure(2));
  p.bounds = c->bounds;
  HIPCHK(a, launch_pile_bounds(p, st));
  uint64_t h[2] = {0, 0};
  HIPCHK(a, hipMemcpyAsync(h, c->bounds, sizeof h, hipMemcpyDeviceToHost, st));
  HIPCHK(a, hipStreamSynchronize(st));
  if (h[0] > h[1] || h[1] > c->n_tab) return fail(a, THM_ERR_INTERNAL, "thm_pileup: rows [%llu, %llu) of %llu", (unsigned long long)h[0], (unsigned long long)h[1], (unsigned long long)c->n_tab);
  p.r0 = h[0];
  p.r1 = h[1];
  return THM_OK;
}

}  // namespace

extern "C" {

int32_t thm_pileup_create(thm_aligner* a, uint32_t flags, uint64_t max_bytes, thm_pileup** out) {
  if (!out) return THM_ERR_INVALID_ARG;
  *out = nullptr;
  if (!a) return THM_ERR_INVALID_ARG;
  if (flags & ~THM_PILE_MULTI) return fail(a, THM_ERR_INVALID_ARG, "thm_pileup_create: unknown bits in flags %#x", flags);
  const thm_index* ix = a->ix;
  HIPCHK(a, hipSetDevice(a->device));
  int rc = bam_tables_on_device(a);
  if (rc != THM_OK) return rc;
  std::vector<std::pair<std::string, uint64_t>> sq;
  const std::vector<int32_t> sq_of_name = thm::sq_of_name(ix, &sq);
  thm_pileup* c = new thm_pileup();
  c->a = a;
  c->flags = flags;
  c->max_bytes = max_bytes;
  memset(&c->totals, 0, sizeof c->totals);
  c->sq.lay_out(sq);
  const uint64_t entries = c->entries();
  const unsigned long long need = entries * 4 + c->sq.h_base.size() * 8 + sq.size() * 8;
  c->array_bytes = need;
  if (max_bytes && need > max_bytes) {
    delete c;
    return fail(a, THM_ERR_OOM, "thm_pileup_create: the depth of %zu contigs needs %llu bytes, the cap is %llu", sq.size(), need, (unsigned long long)max_bytes);
  }
  // the forward copy of every contig in the text is its sequence
  std::vector<uint64_t> tstart(sq.size() + 1, ~0ull);
  for (size_t r = 0; r < ix->refs.size(); r++) {
    const thm_ref& ref = ix->refs[r];
    if (ref.strand != 1 || ref.name_id >= sq_of_name.size() || sq_of_name[ref.name_id] < 0) continue;
    const size_t s = (size_t)sq_of_name[ref.name_id];
    if (s < sq.size() && ref.len == sq[s].second) tstart[s] = ref.start_idx;
  }
  for (size_t s = 0; s < sq.size(); s++)
    if (tstart[s] == ~0ull || tstart[s] + sq[s].second > ix->text.size()) {
      delete c;
      return fail(a, THM_ERR_INVALID_ARG, "thm_pileup_create: the text holds no forward copy of contig %s", sq[s].first.c_str());
    }
  hipError_t e = c->sq.on_device(a);
  if (e == hipSuccess) e = alloc_exact(c->tstart, tstart.size() * 8);
  if (e == hipSuccess) e = alloc_exact(c->diff, entries * 4 + 16);
  if (e == hipSuccess) e = hipMemcpy(c->tstart, tstart.data(), tstart.size() * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(c->diff, 0, entries * 4 + 16);
  if (e != hipSuccess) {
    delete c;
    return fail(a, e == hipErrorOutOfMemory ? THM_ERR_OOM : THM_ERR_HIP, "thm_pileup_create: %s (%llu bytes needed, the cap is %llu)", hipGetErrorString(e), need,
                (unsigned long long)max_bytes);
  }
  *out = c;
  return THM_OK;
}

void thm_pileup_free(thm_pileup* c) { free_summary(c); }

int32_t thm_pileup_add(thm_pileup* c, thm_pile_info* info) {
  if (!c || !info) return THM_ERR_INVALID_ARG;
  memset(info, 0, sizeof(*info));
  thm_aligner* a = c->a;
  PileBatch b{};
  if (const int rc = resident_batch(a, &b); rc != THM_OK) return rc;
  b.bases = a->reads.bases;
  b.base_off = a->reads.offsets;
  return add_batch(c, "thm_pileup_add", THM_ERR_INTERNAL, b, info);
}

int32_t thm_pileup_add_view(thm_pileup* c, const thm_cigar_view* v, const uint8_t* bases, const uint64_t* base_off, thm_pile_info* info) {
  if (!c || !v || !info) return THM_ERR_INVALID_ARG;
  memset(info, 0, sizeof(*info));
  thm_aligner* a = c->a;
  int rc = check_view(c, v, bases, base_off);
  if (rc != THM_OK) return rc;
  const uint64_t n = v->n_reads, n_bases = n ? base_off[n] : 0;
  const uint64_t zero = 0;
  PileBatch b{};
  rc = c->view.upload(a, v, &b, [&] {
    hipStream_t st = a->stream;
    HIPCHK(a, c->v_base_off.ensure(n + 1));
    HIPCHK(a, c->v_bases.ensure(n_bases + 16));
    HIPCHK(a, hipMemcpyAsync(c->v_base_off, n ? base_off : &zero, (n + 1) * 8, hipMemcpyHostToDevice, st));
    if (n_bases) HIPCHK(a, hipMemcpyAsync(c->v_bases, bases, n_bases, hipMemcpyHostToDevice, st));
    return (int)THM_OK;
  });
  if (rc != THM_OK) return rc;
  b.bases = c->v_bases;
  b.base_off = c->v_base_off;
  return add_batch(c, "thm_pileup_add_view", THM_ERR_INVALID_ARG, b, info);
}

int32_t thm_pileup_fetch(thm_pileup* c, uint32_t first_ref, uint32_t n_refs, uint32_t min_alt, thm_pile_view* out) {
  if (!c || !out) return THM_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  thm_aligner* a = c->a;
  if (min_alt == 0) return fail(a, THM_ERR_INVALID_ARG, "thm_pileup_fetch: min_alt must be 1 or more (thm_pileup_window returns every position)");
  if (first_ref > c->sq.n_sq || n_refs > c->sq.n_sq - first_ref)
    return fail(a, THM_ERR_INVALID_ARG, "thm_pileup_fetch: @SQ entries [%u, +%u) of %u", first_ref, n_refs, c->sq.n_sq);
  HIPCHK(a, hipSetDevice(a->device));
  hipStream_t st = a->stream;
  HIPCHK(a, ensure_events(c->ev_fetch));
  const uint64_t g0 = c->sq.h_base[first_ref], g1 = c->sq.h_base[first_ref + n_refs];
  HIPCHK(a, hipEventRecord(c->ev_fetch[0], st));
  PileFetchParams p;
  if (const int rc = row_bounds(c, p, g0, g1); rc != THM_OK) return rc;
  const uint64_t n_rows = p.r1 - p.r0;
  unsigned long long n_sites = 0;
  if (n_rows) {
    HIPCHK(a, c->keep.ensure(n_rows + 1));
    HIPCHK(a, c->site_at.ensure(n_rows + 2));
    p.min_alt = min_alt;
    p.keep = c->keep;
    p.site_at = c->site_at;
    HIPCHK(a, launch_pile_keep(p, st));
    if (const int rc = scan_u64(a, c->tiles.scan_tmp, p.keep, c->site_at, n_rows, st, &n_sites); rc != THM_OK) return rc;
    HIPCHK(a, hipStreamSynchronize(st));
    if (n_sites > n_rows) return fail(a, THM_ERR_INTERNAL, "thm_pileup_fetch: %llu sites from %llu rows", n_sites, (unsigned long long)n_rows);
  }
  HIPCHK(a, c->h_out.ensure(n_sites * sizeof(thm_pile_site) + 16));
  if (n_sites) {
    HIPCHK(a, c->d_sites.ensure(n_sites));
    if (const int rc = tile_pass(a, c->tiles, c->diff + g0, g1 - g0, false); rc != THM_OK) return rc;
    p.n_sites = n_sites;
    p.diff = c->diff + g0;
    p.n = g1 - g0;
    p.g0 = g0;
    p.carry = c->tiles.carry;
    p.sites = c->d_sites;
    HIPCHK(a, launch_pile_sites(p, st));
    HIPCHK(a, hipMemcpyAsync(c->h_out.p, c->d_sites, n_sites * sizeof(thm_pile_site), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(a, hipEventRecord(c->ev_fetch[1], st));
  HIPCHK(a, hipStreamSynchronize(st));
  (void)elapsed_ms(c->ev_fetch[0], c->ev_fetch[1], &out->fetch_ms);
  out->first_ref = first_ref;
  out->n_refs = n_refs;
  out->min_alt = min_alt;
  out->n_sites = n_sites;
  out->sites = c->h_out.as<thm_pile_site>();
  out->n_events = n_rows;
  out->totals = c->totals;
  return THM_OK;
}

int32_t thm_pileup_window(thm_pileup* c, uint32_t ref_id, uint64_t start, uint64_t n, thm_pile_view* out) {
  if (!c || !out) return THM_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  thm_aligner* a = c->a;
  if (ref_id >= c->sq.n_sq) return fail(a, THM_ERR_INVALID_ARG, "thm_pileup_window: refID %u of %u", ref_id, c->sq.n_sq);
  const uint64_t g0 = c->sq.h_base[ref_id], len = c->sq.len(ref_id);
  if (n > pile::MAX_WINDOW || start > len || n > len - start)
    return fail(a, THM_ERR_INVALID_ARG, "thm_pileup_window: the window [%llu, +%llu) must hold at most 2^20 bases and lie inside the %llu bases of refID %u",
                (unsigned long long)start, (unsigned long long)n, (unsigned long long)len, ref_id);
  HIPCHK(a, hipSetDevice(a->device));
  hipStream_t st = a->stream;
  HIPCHK(a, ensure_events(c->ev_fetch));
  HIPCHK(a, c->h_out.ensure(n * sizeof(thm_pile_site) + 16));
  HIPCHK(a, hipEventRecord(c->ev_fetch[0], st));
  PileFetchParams p;
  if (const int rc = row_bounds(c, p, g0 + start, g0 + start + n); rc != THM_OK) return rc;
  if (n) {
    HIPCHK(a, c->d_sites.ensure(n));
    if (const int rc = tile_pass(a, c->tiles, c->diff + g0, start + n, false); rc != THM_OK) return rc;
    p.diff = c->diff + g0;
    p.n = start + n;
    p.g0 = g0;
    p.carry = c->tiles.carry;
    p.start = start;
    p.sites = c->d_sites;
    HIPCHK(a, launch_pile_window(p, st));
    HIPCHK(a, hipMemcpyAsync(c->h_out.p, c->d_sites, n * sizeof(thm_pile_site), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(a, hipEventRecord(c->ev_fetch[1], st));
  HIPCHK(a, hipStreamSynchronize(st));
  (void)elapsed_ms(c->ev_fetch[0], c->ev_fetch[1], &out->fetch_ms);
  out->first_ref = ref_id;
  out->n_refs = 1;
  out->n_sites = n;
  out->sites = c->h_out.as<thm_pile_site>();
  out->n_events = p.r1 - p.r0;
  out->totals = c->totals;
  return THM_OK;
}

int32_t thm_pileup_reset(thm_pileup* c) {
  if (!c) return THM_ERR_INVALID_ARG;
  thm_aligner* a = c->a;
  HIPCHK(a, hipSetDevice(a->device));
  HIPCHK(a, hipMemsetAsync(c->diff, 0, c->entries() * 4, a->stream));
  HIPCHK(a, hipStreamSynchronize(a->stream));
  c->n_tab = 0;
  memset(&c->totals, 0, sizeof c->totals);
  return THM_OK;
}

}  // extern "C"
