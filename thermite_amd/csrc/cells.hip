// cells.hip -- host side of thm_cells (include/thermite_io.h): the cell-by-gene matrix of distinct molecules of a run,
// accumulated on the device over its batches from what is resident after thm_batch_run -- the compacted thm_aln records,
// the per-read offsets, the read names the BAM layer keeps there, and the tx -> gene table of the BAM encoder.  The
// molecules are a sorted table of 16-byte rows (cells_device.h has the key) and, behind it, the reduced rows of the
// batches that have not been merged yet; only totals and the rows of cells and entries come back to the host.  The
// kernels are kernels_cells.hip; the batch, the view's upload and checks, the totals and the free are run_summary.h's,
// shared with quant.hip, coverage.hip and pileup.hip.  DESIGN.md section 4.21.
//
// Synchronisations of the stream.  add: thm_batch_sync's, one of fetch_batch_sizes, one of the CIGAR passes, one behind
// the classify pass, with counted reads one in sort_reduce and with a merge one more in its sort_reduce, one at the end.
// add_view: one behind the upload (the names go up in front of it), then as add from the classify pass on.  fetch: with
// pending rows one in the merge's sort_reduce; with rows one behind the three scans and one behind the two; one at the
// end.  reset: one.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstring>
#include <utility>

#include "aligner_internal.h"
#include "cells_device.h"
#include "launch_io.h"
#include "run_summary.h"

using namespace thm;

namespace {

constexpr uint64_t ROW_BYTES = 16;              // a row: the two words of its key, the count inside the first
constexpr uint64_t MAX_ROWS = 0x7FFFFFFFull;    // of one sort

// molecule rows on the device, an array per word
struct Rows {
  DArr<uint64_t> hc, lo;
  hipError_t ensure(uint64_t n) {
    const hipError_t e = hc.ensure(n);
    return e != hipSuccess ? e : lo.ensure(n);
  }
  size_t bytes() const { return hc.cap() + lo.cap(); }
};

}  // namespace

struct thm_cells {
  thm_aligner* a = nullptr;
  uint32_t flags = 0, cb_len = 0, umi_len = 0;
  uint64_t max_bytes = 0;
  std::vector<int32_t> h_ref_sq;  // what bam.ref_sq holds, for the checks of thm_cells_add_view
  // the running table, sorted, distinct keys, in tab[cur]; the other takes the next merge
  Rows tab[2];
  int cur = 0;
  uint64_t n_tab = 0;
  // the reduced rows of the batches since the last merge, one sorted segment behind the other
  Rows pend;
  uint64_t n_pend = 0;
  thm_cells_totals totals;
  // one batch's scratch
  DArr<uint64_t> counted, at, flag, first, head_at, scan_tmp;
  Rows read_key, keys, tmp, red;
  BatchTotals<cells::N_TOTALS> tot;
  DBuf cub_tmp;  // hipcub's scratch
  // what thm_cells_add_view uploads: the view, and the names
  AlnView view;
  DArr<uint64_t> v_name_off;
  DArr<uint8_t> v_names;
  // a fetch's scratch and results
  DArr<uint64_t> bflag, eflag, cnt, b_at, e_at, pre, bc_start, ent_start, keep, kept_entries, cell_at, ent_at;
  DArr<thm_cell> d_cells;
  DArr<thm_cell_entry> d_entries;
  HBuf h_out;  // the cells, and behind them the entries
  Event ev[2], ev_fetch[2];

  uint64_t held_bytes() const {
    size_t n = tab[0].bytes() + tab[1].bytes() + pend.bytes() + read_key.bytes() + keys.bytes() + tmp.bytes() + red.bytes() + tot.d.cap + cub_tmp.cap + view.cap();
    for (const DArr<uint64_t>* x : {&counted, &at, &flag, &first, &head_at, &scan_tmp, &v_name_off, &bflag, &eflag, &cnt, &b_at, &e_at, &pre, &bc_start, &ent_start,
                                    &keep, &kept_entries, &cell_at, &ent_at})
      n += x->cap();
    return n + v_names.cap() + d_cells.cap() + d_entries.cap();
  }
};

namespace {

// `r` with room for `want` rows, its first `have` rows kept (a DArr's ensure keeps nothing)
int grow_keep(thm_cells* c, Rows& r, uint64_t have, uint64_t want) {
  thm_aligner* a = c->a;
  if (want * 8 <= r.hc.cap() && want * 8 <= r.lo.cap()) return THM_OK;
  Rows bigger;
  HIPCHK(a, bigger.ensure(want + want / 2));
  if (have) {
    HIPCHK(a, hipMemcpyAsync(bigger.hc, r.hc, have * 8, hipMemcpyDeviceToDevice, a->stream));
    HIPCHK(a, hipMemcpyAsync(bigger.lo, r.lo, have * 8, hipMemcpyDeviceToDevice, a->stream));
    HIPCHK(a, hipStreamSynchronize(a->stream));  // (the old arrays go with `bigger` at the end of this scope)
  }
  std::swap(r.hc.b.p, bigger.hc.b.p);
  std::swap(r.hc.b.cap, bigger.hc.b.cap);
  std::swap(r.lo.b.p, bigger.lo.b.p);
  std::swap(r.lo.b.cap, bigger.lo.b.cap);
  return THM_OK;
}

// in[0, n) (any order; overwritten: the sorted rows end there) sorted by (barcode, gene, UMI) and reduced by key into
// `out` -> *m rows.  Two stable passes over the bits in use, the low word first.  `unit`: every count of `in` is 1.
// Synchronises the stream once: `out` is sized by the count.
int sort_reduce(thm_cells* c, Rows& in, uint64_t n, bool unit, Rows& out, uint64_t* m) {
  thm_aligner* a = c->a;
  hipStream_t st = a->stream;
  *m = 0;
  if (n == 0) return THM_OK;
  if (n > MAX_ROWS) return fail(a, THM_ERR_UNSUPPORTED, "thm_cells: 2^31 rows or more in one sort");
  HIPCHK(a, c->tmp.ensure(n));
  HIPCHK(a, c->flag.ensure(n + 1));
  HIPCHK(a, c->first.ensure(n + 2));
  const int lo_bits = cells::gene_bits((uint32_t)a->ix->genes.size()) + 2 * (int)c->umi_len, hc_bits = 2 * (int)c->cb_len;
  uint64_t *in_hc = in.hc.get(), *in_lo = in.lo.get(), *t_hc = c->tmp.hc.get(), *t_lo = c->tmp.lo.get();
  size_t b1 = 0, b2 = 0;
  HIPCHK(a, hipcub::DeviceRadixSort::SortPairs(nullptr, b1, in_lo, t_lo, in_hc, t_hc, n, 0, lo_bits, st));
  HIPCHK(a, hipcub::DeviceRadixSort::SortPairs(nullptr, b2, t_hc, in_hc, t_lo, in_lo, n, 0, hc_bits, st));
  size_t tmp_bytes = b1 > b2 ? b1 : b2;
  HIPCHK(a, c->cub_tmp.ensure(tmp_bytes + 16));
  // least significant word first, both passes stable: rows of one barcode keep the order of their low words
  HIPCHK(a, hipcub::DeviceRadixSort::SortPairs(c->cub_tmp.p, tmp_bytes, in_lo, t_lo, in_hc, t_hc, n, 0, lo_bits, st));
  HIPCHK(a, hipcub::DeviceRadixSort::SortPairs(c->cub_tmp.p, tmp_bytes, t_hc, in_hc, t_lo, in_lo, n, 0, hc_bits, st));
  CellsReduceParams p;
  memset(&p, 0, sizeof p);
  p.hc = in_hc;
  p.lo = in_lo;
  p.n = n;
  p.flag = c->flag;
  p.first = c->first;
  p.unit = unit ? 1u : 0u;
  HIPCHK(a, launch_cells_heads(p, st));
  unsigned long long n_keys = 0;
  if (const int rc = scan_u64(a, c->scan_tmp, p.flag, c->first, n, st, &n_keys); rc != THM_OK) return rc;
  HIPCHK(a, hipStreamSynchronize(st));
  if (n_keys == 0 || n_keys > n) return fail(a, THM_ERR_INTERNAL, "thm_cells: %llu molecules among %llu rows", n_keys, (unsigned long long)n);
  HIPCHK(a, c->head_at.ensure(n_keys + 1));
  HIPCHK(a, out.ensure(n_keys));
  p.head_at = c->head_at;
  p.n_keys = n_keys;
  p.out_hc = out.hc;
  p.out_lo = out.lo;
  HIPCHK(a, launch_cells_head_at(p, st));
  HIPCHK(a, launch_cells_reduce(p, st));
  *m = n_keys;
  return THM_OK;
}

// The table, the pending rows and the first n_red rows of c->red, sorted and reduced together into the other of the two
// table buffers -> *n_cat rows.  Nothing of the object changes: the caller swaps once nothing can fail any more.
int merge_all(thm_cells* c, uint64_t n_red, uint64_t* n_cat) {
  thm_aligner* a = c->a;
  hipStream_t st = a->stream;
  Rows& dst = c->tab[c->cur ^ 1];
  const uint64_t n_tab = c->n_tab, n_pend = c->n_pend, n = n_tab + n_pend + n_red;
  *n_cat = 0;
  if (n == 0) return THM_OK;
  if (n_tab == 0 && n_pend == 0) {
    // (the reduced rows are sorted and distinct: they are the table)
    HIPCHK(a, dst.ensure(n_red));
    HIPCHK(a, hipMemcpyAsync(dst.hc, c->red.hc, n_red * 8, hipMemcpyDeviceToDevice, st));
    HIPCHK(a, hipMemcpyAsync(dst.lo, c->red.lo, n_red * 8, hipMemcpyDeviceToDevice, st));
    *n_cat = n_red;
    return THM_OK;
  }
  Rows& cat = c->keys;  // (a batch's compacted keys have been reduced into c->red by now)
  HIPCHK(a, cat.ensure(n));
  const Rows* src[3] = {&c->tab[c->cur], &c->pend, &c->red};
  const uint64_t cnt[3] = {n_tab, n_pend, n_red};
  uint64_t at = 0;
  for (int k = 0; k < 3; k++) {
    if (cnt[k]) {
      HIPCHK(a, hipMemcpyAsync(cat.hc + at, src[k]->hc, cnt[k] * 8, hipMemcpyDeviceToDevice, st));
      HIPCHK(a, hipMemcpyAsync(cat.lo + at, src[k]->lo, cnt[k] * 8, hipMemcpyDeviceToDevice, st));
    }
    at += cnt[k];
  }
  return sort_reduce(c, cat, n, false, dst, n_cat);
}

// One batch that stands on the device.  Nothing of the object changes before the batch has passed the device's checks
// and the cap.
int add_batch(thm_cells* c, const char* who, int refused, CellsBatch b, thm_cells_info* info) {
  thm_aligner* a = c->a;
  hipStream_t st = a->stream;
  const thm_index* ix = a->ix;
  const uint64_t n = b.n_reads;
  if (b.n_alns && !n) return fail(a, THM_ERR_INTERNAL, "%s: %llu alignments of no read", who, (unsigned long long)b.n_alns);
  if (n > 0xFFFFFFFFull - c->totals.n_reads)
    return fail(a, THM_ERR_INVALID_ARG, "%s: %llu reads behind the %llu counted would be more than 2^32-1: a molecule's count could wrap", who,
                (unsigned long long)n, (unsigned long long)c->totals.n_reads);
  b.n_txs = (uint32_t)ix->txs.size();
  b.n_genes = (uint32_t)ix->genes.size();
  b.tx_gene = a->bam.tx_gene;
  b.flags = c->flags;
  b.cb_len = c->cb_len;
  b.umi_len = c->umi_len;
  HIPCHK(a, ensure_events(c->ev));
  HIPCHK(a, c->counted.ensure(n + 1));
  HIPCHK(a, c->at.ensure(n + 2));
  HIPCHK(a, c->read_key.ensure(n + 1));
  HIPCHK(a, c->tot.reserve());
  CellsClassifyParams cp;
  cp.b = b;
  cp.counted = c->counted;
  cp.hc = c->read_key.hc;
  cp.lo = c->read_key.lo;
  cp.totals = c->tot.totals();
  cp.bad = c->tot.bad();
  HIPCHK(a, hipEventRecord(c->ev[0], st));
  HIPCHK(a, c->tot.clear(st));
  HIPCHK(a, launch_cells_classify(cp, a->n_cu, st));
  unsigned long long n_counted = 0;
  if (n) {
    if (const int rc = scan_u64(a, c->scan_tmp, cp.counted, c->at, n, st, &n_counted); rc != THM_OK) return rc;
  }
  HIPCHK(a, c->tot.fetch(st));
  HIPCHK(a, hipStreamSynchronize(st));
  const unsigned long long* h_tot = c->tot.h;
  if (c->tot.refused())
    return fail(a, refused, "%s: alignment %llu lies outside the view, or has a type or an index outside the index's tables", who, c->tot.first_bad());
  if (h_tot[cells::T_READS] != n || n_counted != h_tot[cells::T_COUNTED])
    return fail(a, THM_ERR_INTERNAL, "%s: %llu reads classified of %llu, %llu keys scanned, %llu counted", who, h_tot[cells::T_READS], (unsigned long long)n, n_counted,
                h_tot[cells::T_COUNTED]);
  bool swap = false;
  uint64_t n_tab = c->n_tab, n_pend = c->n_pend;
  if (n_counted) {
    HIPCHK(a, c->keys.ensure(n_counted));
    CellsCompactParams kp;
    kp.n_reads = n;
    kp.counted = cp.counted;
    kp.at = c->at;
    kp.hc = cp.hc;
    kp.lo = cp.lo;
    kp.out_hc = c->keys.hc;
    kp.out_lo = c->keys.lo;
    HIPCHK(a, launch_cells_compact(kp, st));
    uint64_t n_red = 0;
    if (const int rc = sort_reduce(c, c->keys, n_counted, true, c->red, &n_red); rc != THM_OK) return rc;
    // The merge policy: the rows wait behind the pending ones until there are as many of them as the table has rows --
    // then, or where only a merge can tell whether the cap holds, everything is sorted and reduced together.
    const uint64_t n_held = n_tab + n_pend + n_red;
    const bool over = c->max_bytes && n_held * ROW_BYTES > c->max_bytes;
    if (n_pend + n_red >= n_tab || over) {
      uint64_t n_cat = 0;
      if (const int rc = merge_all(c, n_red, &n_cat); rc != THM_OK) return rc;
      if (c->max_bytes && n_cat * ROW_BYTES > c->max_bytes) {
        HIPCHK(a, hipStreamSynchronize(st));  // (nothing is left running over buffers that the next call may grow)
        return fail(a, THM_ERR_OOM, "%s: a table of %llu molecules needs %llu bytes, the cap is %llu", who, (unsigned long long)n_cat,
                    (unsigned long long)(n_cat * ROW_BYTES), (unsigned long long)c->max_bytes);
      }
      swap = true;
      n_tab = n_cat;
      n_pend = 0;
    } else {
      if (const int rc = grow_keep(c, c->pend, n_pend, n_pend + n_red); rc != THM_OK) return rc;
      HIPCHK(a, hipMemcpyAsync(c->pend.hc + n_pend, c->red.hc, n_red * 8, hipMemcpyDeviceToDevice, st));
      HIPCHK(a, hipMemcpyAsync(c->pend.lo + n_pend, c->red.lo, n_red * 8, hipMemcpyDeviceToDevice, st));
      n_pend += n_red;
    }
  }
  HIPCHK(a, hipEventRecord(c->ev[1], st));
  HIPCHK(a, hipStreamSynchronize(st));
  if (swap) c->cur ^= 1;
  c->n_tab = n_tab;
  c->n_pend = n_pend;
  (void)elapsed_ms(c->ev[0], c->ev[1], &info->add_ms);
  c->tot.accumulate(&info->batch, &c->totals);
  info->n_molecules = n_tab + n_pend;
  info->n_pending = n_pend;
  info->held_bytes = c->held_bytes();
  return THM_OK;
}

// the checks of thm_cells_add_view, on the host before anything goes up: the names' offsets, then the view
int check_view(thm_cells* c, const thm_cigar_view* v, const uint8_t* names, const uint64_t* name_off) {
  thm_aligner* a = c->a;
  const char* who = "thm_cells_add_view";
  const uint64_t n = v->n_reads;
  if (n) {
    if (!name_off) return fail(a, THM_ERR_INVALID_ARG, "%s: null name offsets", who);
    if (name_off[0] != 0) return fail(a, THM_ERR_INVALID_ARG, "%s: name_off[0] must be 0", who);
    for (uint64_t r = 0; r < n; r++)
      if (name_off[r + 1] < name_off[r]) return fail(a, THM_ERR_INVALID_ARG, "%s: name_off descends at read %llu", who, (unsigned long long)r);
    if (name_off[n] && !names) return fail(a, THM_ERR_INVALID_ARG, "%s: null names", who);
  }
  return check_cigar_view(a, who, v, c->h_ref_sq, [](uint64_t, const thm_aln&, const thm_aln_digest&) { return (int)THM_OK; });
}

}  // namespace

extern "C" {

int32_t thm_cells_create(thm_aligner* a, uint32_t flags, uint32_t cb_len, uint32_t umi_len, uint64_t max_bytes, thm_cells** out) {
  if (!out) return THM_ERR_INVALID_ARG;
  *out = nullptr;
  if (!a) return THM_ERR_INVALID_ARG;
  if (flags & ~THM_CELLS_INTRONIC) return fail(a, THM_ERR_INVALID_ARG, "thm_cells_create: unknown bits in flags %#x", flags);
  if (cb_len < 1 || cb_len > THM_CELLS_MAX_LEN || umi_len < 1 || umi_len > THM_CELLS_MAX_LEN)
    return fail(a, THM_ERR_INVALID_ARG, "thm_cells_create: cb_len %u and umi_len %u must each be 1..16", cb_len, umi_len);
  const thm_index* ix = a->ix;
  if (ix->genes.size() > 0x3FFFFFFFull) return fail(a, THM_ERR_UNSUPPORTED, "thm_cells_create: 2^30 genes or more");
  HIPCHK(a, hipSetDevice(a->device));
  const int rc = bam_tables_on_device(a);
  if (rc != THM_OK) return rc;
  thm_cells* c = new thm_cells();
  c->a = a;
  c->flags = flags;
  c->cb_len = cb_len;
  c->umi_len = umi_len;
  c->max_bytes = max_bytes;
  memset(&c->totals, 0, sizeof c->totals);
  const size_t n_refs = ix->refs.size();
  c->h_ref_sq.assign(n_refs, -1);
  if (n_refs) {
    const hipError_t e = hipMemcpy(c->h_ref_sq.data(), a->bam.ref_sq, n_refs * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
      delete c;
      return fail(a, THM_ERR_HIP, "thm_cells_create: %s", hipGetErrorString(e));
    }
  }
  *out = c;
  return THM_OK;
}

void thm_cells_free(thm_cells* c) { free_summary(c); }

int32_t thm_cells_add(thm_cells* c, thm_cells_info* info) {
  if (!c || !info) return THM_ERR_INVALID_ARG;
  memset(info, 0, sizeof(*info));
  thm_aligner* a = c->a;
  if (!a->uploaded || !a->bam.reads_named)
    return fail(a, THM_ERR_INVALID_ARG, "thm_batch_fetch_bam: the batch was not uploaded by thm_batch_upload_reads (no names)");
  CellsBatch b{};
  if (const int rc = resident_batch(a, &b); rc != THM_OK) return rc;
  b.names = a->bam.names;
  b.name_off = a->bam.name_off;
  return add_batch(c, "thm_cells_add", THM_ERR_INTERNAL, b, info);
}

int32_t thm_cells_add_view(thm_cells* c, const thm_cigar_view* v, const uint8_t* names, const uint64_t* name_off, thm_cells_info* info) {
  if (!c || !v || !info) return THM_ERR_INVALID_ARG;
  memset(info, 0, sizeof(*info));
  thm_aligner* a = c->a;
  int rc = check_view(c, v, names, name_off);
  if (rc != THM_OK) return rc;
  const uint64_t n = v->n_reads, n_bytes = n ? name_off[n] : 0;
  const uint64_t zero = 0;
  CellsBatch b{};
  rc = c->view.upload(a, v, &b, [&] {
    hipStream_t st = a->stream;
    HIPCHK(a, c->v_name_off.ensure(n + 1));
    HIPCHK(a, c->v_names.ensure(n_bytes + 16));
    HIPCHK(a, hipMemcpyAsync(c->v_name_off, n ? name_off : &zero, (n + 1) * 8, hipMemcpyHostToDevice, st));
    if (n_bytes) HIPCHK(a, hipMemcpyAsync(c->v_names, names, n_bytes, hipMemcpyHostToDevice, st));
    return (int)THM_OK;
  });
  if (rc != THM_OK) return rc;
  b.names = c->v_names;
  b.name_off = c->v_name_off;
  return add_batch(c, "thm_cells_add_view", THM_ERR_INVALID_ARG, b, info);
}

int32_t thm_cells_fetch(thm_cells* c, uint32_t min_umis, thm_cells_view* out) {
  if (!c || !out) return THM_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  thm_aligner* a = c->a;
  if (min_umis == 0) return fail(a, THM_ERR_INVALID_ARG, "thm_cells_fetch: min_umis must be 1 or more");
  HIPCHK(a, hipSetDevice(a->device));
  hipStream_t st = a->stream;
  HIPCHK(a, ensure_events(c->ev_fetch));
  HIPCHK(a, hipEventRecord(c->ev_fetch[0], st));
  if (c->n_pend) {
    // (the same molecules in another arrangement: a fetch that fails behind this has changed nothing a fetch returns)
    uint64_t n_cat = 0;
    if (const int rc = merge_all(c, 0, &n_cat); rc != THM_OK) return rc;
    HIPCHK(a, hipStreamSynchronize(st));
    c->cur ^= 1;
    c->n_tab = n_cat;
    c->n_pend = 0;
  }
  const uint64_t n = c->n_tab;
  CellsFetchParams p;
  memset(&p, 0, sizeof p);
  unsigned long long n_barcodes = 0, n_all_entries = 0, n_cells = 0, n_entries = 0;
  if (n) {
    for (DArr<uint64_t>* x : {&c->bflag, &c->eflag, &c->cnt}) HIPCHK(a, x->ensure(n + 1));
    for (DArr<uint64_t>* x : {&c->b_at, &c->e_at, &c->pre}) HIPCHK(a, x->ensure(n + 2));
    p.hc = c->tab[c->cur].hc;
    p.lo = c->tab[c->cur].lo;
    p.n = n;
    p.umi_len = c->umi_len;
    p.min_umis = min_umis;
    p.bflag = c->bflag;
    p.eflag = c->eflag;
    p.cnt = c->cnt;
    p.b_at = c->b_at;
    p.e_at = c->e_at;
    p.pre = c->pre;
    HIPCHK(a, launch_cells_levels(p, st));
    int rc = scan_u64(a, c->scan_tmp, p.bflag, c->b_at, n, st, &n_barcodes);
    if (rc == THM_OK) rc = scan_u64(a, c->scan_tmp, p.eflag, c->e_at, n, st, &n_all_entries);
    if (rc == THM_OK) rc = scan_u64(a, c->scan_tmp, p.cnt, c->pre, n, st);
    if (rc != THM_OK) return rc;
    HIPCHK(a, hipStreamSynchronize(st));
    if (n_barcodes == 0 || n_barcodes > n_all_entries || n_all_entries > n)
      return fail(a, THM_ERR_INTERNAL, "thm_cells_fetch: %llu barcodes and %llu entries from %llu rows", n_barcodes, n_all_entries, (unsigned long long)n);
    HIPCHK(a, c->bc_start.ensure(n_barcodes + 1));
    HIPCHK(a, c->ent_start.ensure(n_all_entries + 1));
    for (DArr<uint64_t>* x : {&c->keep, &c->kept_entries}) HIPCHK(a, x->ensure(n_barcodes + 1));
    for (DArr<uint64_t>* x : {&c->cell_at, &c->ent_at}) HIPCHK(a, x->ensure(n_barcodes + 2));
    p.n_barcodes = n_barcodes;
    p.n_all_entries = n_all_entries;
    p.bc_start = c->bc_start;
    p.ent_start = c->ent_start;
    p.keep = c->keep;
    p.kept_entries = c->kept_entries;
    p.cell_at = c->cell_at;
    p.ent_at = c->ent_at;
    HIPCHK(a, launch_cells_starts(p, st));
    HIPCHK(a, launch_cells_barcodes(p, st));
    rc = scan_u64(a, c->scan_tmp, p.keep, c->cell_at, n_barcodes, st, &n_cells);
    if (rc == THM_OK) rc = scan_u64(a, c->scan_tmp, p.kept_entries, c->ent_at, n_barcodes, st, &n_entries);
    if (rc != THM_OK) return rc;
    HIPCHK(a, hipStreamSynchronize(st));
    if (n_cells > n_barcodes || n_entries > n_all_entries)
      return fail(a, THM_ERR_INTERNAL, "thm_cells_fetch: %llu cells of %llu barcodes, %llu entries of %llu", n_cells, n_barcodes, n_entries, n_all_entries);
  }
  const size_t cell_bytes = n_cells * sizeof(thm_cell), entry_bytes = n_entries * sizeof(thm_cell_entry);
  HIPCHK(a, c->h_out.ensure(cell_bytes + entry_bytes + 16));
  if (n_cells) {
    HIPCHK(a, c->d_cells.ensure(n_cells));
    HIPCHK(a, c->d_entries.ensure(n_entries));
    p.cells = c->d_cells;
    p.entries = c->d_entries;
    HIPCHK(a, launch_cells_rows(p, st));
    HIPCHK(a, hipMemcpyAsync(c->h_out.p, c->d_cells, cell_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(a, hipMemcpyAsync(c->h_out.as<uint8_t>() + cell_bytes, c->d_entries, entry_bytes, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(a, hipEventRecord(c->ev_fetch[1], st));
  HIPCHK(a, hipStreamSynchronize(st));
  (void)elapsed_ms(c->ev_fetch[0], c->ev_fetch[1], &out->fetch_ms);
  out->cb_len = c->cb_len;
  out->umi_len = c->umi_len;
  out->min_umis = min_umis;
  out->n_cells = n_cells;
  out->cells = c->h_out.as<thm_cell>();
  out->n_entries = n_entries;
  out->entries = (const thm_cell_entry*)(c->h_out.as<uint8_t>() + cell_bytes);
  out->n_molecules = n;
  out->n_barcodes = n_barcodes;
  out->n_cells_below = n_barcodes - n_cells;
  out->totals = c->totals;
  return THM_OK;
}

int32_t thm_cells_reset(thm_cells* c) {
  if (!c) return THM_ERR_INVALID_ARG;
  thm_aligner* a = c->a;
  HIPCHK(a, hipSetDevice(a->device));
  HIPCHK(a, hipStreamSynchronize(a->stream));
  c->n_tab = 0;
  c->n_pend = 0;
  memset(&c->totals, 0, sizeof c->totals);
  return THM_OK;
}

}  // extern "C"
