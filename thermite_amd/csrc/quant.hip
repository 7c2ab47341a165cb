// quant.hip -- host side of thm_quant (include/thermite_io.h): the gene and junction count tables of a run, accumulated on
// the device over its batches from what is resident after thm_batch_run -- the compacted thm_aln records, the per-read
// offsets, the CIGAR words and digests of the CIGAR passes, and the tx -> gene and ref -> @SQ tables of the BAM encoder.
// Only totals and the finished tables come back to the host.  The kernels are kernels_quant.hip, the per-alignment
// functions quant_device.h; the batch, the view's upload and checks and the totals are run_summary.h's, shared with
// coverage.hip and pileup.hip.  DESIGN.md sections 4.17 and 4.20.
//
// Synchronisations of the stream.  add: thm_batch_sync's, one of fetch_batch_sizes, one of the CIGAR passes, one behind
// the count pass, with hits one in sort_reduce, one in merge_rows and with new keys one more in its sort_reduce, one
// behind the gene pass.  add_view: one behind the upload, then as add from the count pass on.  fetch: one.  reset: one.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstring>

#include "aligner_internal.h"
#include "launch_io.h"
#include "quant_device.h"
#include "run_summary.h"

using namespace thm;

namespace {

constexpr uint64_t MAX_ROWS = 0xFFFFFFFEull;  // a permutation entry is 32 bits, 0xFFFFFFFF the "not found" of the lookup

// bytes held by some buffers
template <class... B>
size_t held(const B&... b) {
  return (size_t(0) + ... + b.cap());
}

// junction rows on the device, an array per field
struct RowBuf {
  DArr<uint64_t> hi, lo, nu, nm;
  DArr<uint32_t> ov;
  hipError_t ensure(uint64_t n) {
    hipError_t e = hi.ensure(n);
    if (e == hipSuccess) e = lo.ensure(n);
    if (e == hipSuccess) e = nu.ensure(n);
    if (e == hipSuccess) e = nm.ensure(n);
    if (e == hipSuccess) e = ov.ensure(n);
    return e;
  }
  QuantRows rows() const { return QuantRows{hi, lo, nu, nm, ov}; }
  size_t bytes() const { return hi.cap() + lo.cap() + nu.cap() + nm.cap() + ov.cap(); }
};

}  // namespace

struct thm_quant {
  thm_aligner* a = nullptr;
  uint32_t n_sq = 0;
  std::vector<int32_t> h_ref_sq;  // what bam.ref_sq holds, for the checks of thm_quant_add_view
  DArr<uint8_t> tx_forward;       // [n_txs] thm_tx::strand
  DArr<unsigned long long> genes;  // [n_genes * 4], the running gene table
  RowBuf tab[2];                  // the running junction table, sorted, in tab[cur]; the other takes the next merge
  int cur = 0;
  uint64_t n_tab = 0;
  thm_quant_totals totals;
  // one batch's scratch
  RowBuf hits, red, cat;
  DArr<uint64_t> hit_cnt, hit_off, scan_tmp, key_a, key_b, flag, first, is_new, new_at;
  DArr<uint8_t> multi;
  DArr<uint32_t> perm_a, perm_b, where;
  BatchTotals<quant::N_TOTALS> tot;
  DBuf cub_tmp;  // hipcub's scratch
  AlnView view;  // what thm_quant_add_view uploads
  DArr<thm_quant_junction> d_rows;  // the table as records, for the fetch
  HBuf h_out;                       // the genes, and behind them the junctions
  Event ev[2], ev_fetch[2];

  uint64_t held_bytes() const {
    return tab[0].bytes() + tab[1].bytes() + hits.bytes() + red.bytes() + cat.bytes() + tot.d.cap + cub_tmp.cap +
           held(tx_forward, genes, d_rows, hit_cnt, hit_off, multi, scan_tmp, perm_a, perm_b, key_a, key_b, flag, first, where, is_new, new_at, view);
  }
};

namespace {

// `in` (n rows, any order) sorted by key and reduced by key into `out` -> *m rows.  The 128-bit key is sorted as two
// stable 64-bit passes over a permutation, low word first.  Synchronises the stream once: `out` is sized by the count.
int sort_reduce(thm_quant* q, const QuantRows& in, uint64_t n, RowBuf& out, uint64_t* m) {
  thm_aligner* a = q->a;
  hipStream_t st = a->stream;
  *m = 0;
  if (n == 0) return THM_OK;
  HIPCHK(a, q->perm_a.ensure(n));
  HIPCHK(a, q->perm_b.ensure(n));
  HIPCHK(a, q->key_a.ensure(n));
  HIPCHK(a, q->key_b.ensure(n));
  HIPCHK(a, q->flag.ensure(n + 1));
  HIPCHK(a, q->first.ensure(n + 2));
  HIPCHK(a, scan_reserve(q->scan_tmp, n));
  uint32_t *pa = q->perm_a, *pb = q->perm_b;
  uint64_t *ka = q->key_a, *kb = q->key_b;
  const int hi_bits = quant::key_hi_bits(q->n_sq);
  size_t b1 = 0, b2 = 0;
  HIPCHK(a, hipcub::DeviceRadixSort::SortPairs(nullptr, b1, in.lo, kb, pa, pb, n, 0, quant::KEY_LO_BITS, st));
  HIPCHK(a, hipcub::DeviceRadixSort::SortPairs(nullptr, b2, ka, kb, pb, pa, n, 0, hi_bits, st));
  size_t tmp_bytes = b1 > b2 ? b1 : b2;
  HIPCHK(a, q->cub_tmp.ensure(tmp_bytes + 16));
  HIPCHK(a, launch_bam_sort_iota(pa, n, st));
  // least significant word first, every pass stable: rows with equal high words keep the order of their low words
  HIPCHK(a, hipcub::DeviceRadixSort::SortPairs(q->cub_tmp.p, tmp_bytes, in.lo, kb, pa, pb, n, 0, quant::KEY_LO_BITS, st));
  HIPCHK(a, launch_quant_gather(in.hi, pb, n, ka, st));
  HIPCHK(a, hipcub::DeviceRadixSort::SortPairs(q->cub_tmp.p, tmp_bytes, ka, kb, pb, pa, n, 0, hi_bits, st));
  QuantReduceParams p;
  memset(&p, 0, sizeof p);
  p.in = in;
  p.perm = pa;
  p.s_hi = kb;
  p.n = n;
  p.flag = q->flag;
  p.first = q->first;
  HIPCHK(a, launch_quant_heads(p, st));
  unsigned long long n_keys = 0;
  if (const int rc = scan_u64(a, q->scan_tmp, p.flag, q->first, n, st, &n_keys); rc != THM_OK) return rc;
  HIPCHK(a, hipStreamSynchronize(st));
  if (n_keys == 0 || n_keys > n) return fail(a, THM_ERR_INTERNAL, "thm_quant: %llu keys among %llu rows", n_keys, (unsigned long long)n);
  HIPCHK(a, out.ensure(n_keys));
  HIPCHK(a, hipMemsetAsync(out.nu, 0, n_keys * 8, st));
  HIPCHK(a, hipMemsetAsync(out.nm, 0, n_keys * 8, st));
  HIPCHK(a, hipMemsetAsync(out.ov, 0, n_keys * 4, st));
  p.out = out.rows();
  HIPCHK(a, launch_quant_reduce(p, st));
  *m = n_keys;
  return THM_OK;
}

// The reduced rows of a batch (q->red, n_red of them) into the running table: rows whose key the table holds add to it
// in place; new keys are sorted in together with the table's rows, into the other of the two table buffers.
int merge_rows(thm_quant* q, uint64_t n_red) {
  thm_aligner* a = q->a;
  hipStream_t st = a->stream;
  const uint64_t n_tab = q->n_tab;
  HIPCHK(a, q->where.ensure(n_red));
  HIPCHK(a, q->is_new.ensure(n_red + 1));
  HIPCHK(a, q->new_at.ensure(n_red + 2));
  HIPCHK(a, scan_reserve(q->scan_tmp, n_red));
  QuantMergeParams p;
  memset(&p, 0, sizeof p);
  p.tab = q->tab[q->cur].rows();
  p.n_tab = n_tab;
  p.red = q->red.rows();
  p.n_red = n_red;
  p.where = q->where;
  p.is_new = q->is_new;
  p.new_at = q->new_at;
  HIPCHK(a, launch_quant_lookup(p, st));
  unsigned long long n_new = 0;
  if (const int rc = scan_u64(a, q->scan_tmp, p.is_new, q->new_at, n_red, st, &n_new); rc != THM_OK) return rc;
  HIPCHK(a, hipStreamSynchronize(st));
  if (n_new > n_red) return fail(a, THM_ERR_INTERNAL, "thm_quant: %llu new keys among %llu rows", n_new, (unsigned long long)n_red);
  const uint64_t n_cat = n_tab + n_new;
  if (n_cat > MAX_ROWS) return fail(a, THM_ERR_UNSUPPORTED, "thm_quant: more than 2^32-2 distinct junctions");
  if (n_new) HIPCHK(a, q->cat.ensure(n_cat));
  p.cat = q->cat.rows();
  HIPCHK(a, launch_quant_update(p, st));
  if (n_new == 0) return THM_OK;
  if (n_tab) {
    const RowBuf& t = q->tab[q->cur];
    HIPCHK(a, hipMemcpyAsync(q->cat.hi, t.hi, n_tab * 8, hipMemcpyDeviceToDevice, st));
    HIPCHK(a, hipMemcpyAsync(q->cat.lo, t.lo, n_tab * 8, hipMemcpyDeviceToDevice, st));
    HIPCHK(a, hipMemcpyAsync(q->cat.nu, t.nu, n_tab * 8, hipMemcpyDeviceToDevice, st));
    HIPCHK(a, hipMemcpyAsync(q->cat.nm, t.nm, n_tab * 8, hipMemcpyDeviceToDevice, st));
    HIPCHK(a, hipMemcpyAsync(q->cat.ov, t.ov, n_tab * 4, hipMemcpyDeviceToDevice, st));
  }
  uint64_t m = 0;
  const int rc = sort_reduce(q, q->cat.rows(), n_cat, q->tab[q->cur ^ 1], &m);
  if (rc != THM_OK) return rc;
  if (m != n_cat) return fail(a, THM_ERR_INTERNAL, "thm_quant: %llu rows after a merge of %llu distinct keys", (unsigned long long)m, (unsigned long long)n_cat);
  q->cur ^= 1;
  q->n_tab = m;
  return THM_OK;
}

// One batch that stands on the device.  Nothing of the tables changes before the batch has passed the device's checks.
int add_batch(thm_quant* q, const char* who, QuantBatch b, thm_quant_info* info) {
  thm_aligner* a = q->a;
  hipStream_t st = a->stream;
  const thm_index* ix = a->ix;
  const uint64_t n_alns = b.n_alns;
  if (n_alns >= MAX_ROWS) return fail(a, THM_ERR_UNSUPPORTED, "%s: 2^32-2 alignments or more in one batch", who);
  b.n_txs = (uint32_t)ix->txs.size();
  b.n_genes = (uint32_t)ix->genes.size();
  b.tx_gene = a->bam.tx_gene;
  b.tx_forward = q->tx_forward;
  HIPCHK(a, ensure_events(q->ev));
  HIPCHK(a, q->hit_cnt.ensure(n_alns + 1));
  HIPCHK(a, q->hit_off.ensure(n_alns + 2));
  HIPCHK(a, q->multi.ensure(n_alns, 16));
  HIPCHK(a, scan_reserve(q->scan_tmp, n_alns));
  HIPCHK(a, q->tot.reserve());
  QuantCountParams cp;
  cp.b = b;
  cp.hit_cnt = q->hit_cnt;
  cp.multi = q->multi;
  cp.totals = q->tot.totals();
  cp.bad = q->tot.bad();
  HIPCHK(a, hipEventRecord(q->ev[0], st));
  HIPCHK(a, q->tot.clear(st));
  HIPCHK(a, launch_quant_count(cp, a->n_cu, st));
  unsigned long long n_hits = 0;
  if (n_alns) {
    if (const int rc = scan_u64(a, q->scan_tmp, cp.hit_cnt, q->hit_off, n_alns, st, &n_hits); rc != THM_OK) return rc;
  }
  HIPCHK(a, q->tot.fetch(st));
  HIPCHK(a, hipStreamSynchronize(st));
  const unsigned long long* h_tot = q->tot.h;
  if (q->tot.refused())
    return fail(a, THM_ERR_INTERNAL, "%s: alignment %llu has an index, a CIGAR range or an intron outside the index's tables", who, q->tot.first_bad());
  if (n_hits != h_tot[quant::T_HITS]) return fail(a, THM_ERR_INTERNAL, "%s: %llu hits scanned, %llu counted", who, n_hits, h_tot[quant::T_HITS]);
  if (n_hits > MAX_ROWS) return fail(a, THM_ERR_UNSUPPORTED, "%s: more than 2^32-2 junction hits in one batch", who);
  if (n_hits) {
    HIPCHK(a, q->hits.ensure(n_hits));
    QuantExtractParams ep;
    ep.b = b;
    ep.hit_off = q->hit_off;
    ep.multi = cp.multi;
    ep.out = q->hits.rows();
    HIPCHK(a, launch_quant_extract(ep, st));
    uint64_t n_red = 0;
    int rc = sort_reduce(q, ep.out, n_hits, q->red, &n_red);
    if (rc == THM_OK) rc = merge_rows(q, n_red);
    if (rc != THM_OK) return rc;
  }
  QuantGenesParams gp;
  gp.b = b;
  gp.multi = cp.multi;
  gp.genes = q->genes;
  // (the fetch's row buffer is sized here, before anything is counted: held_bytes is what the object holds with a fetch)
  HIPCHK(a, q->d_rows.ensure(q->n_tab, 16));
  HIPCHK(a, launch_quant_genes(gp, a->n_cu, st));
  HIPCHK(a, hipEventRecord(q->ev[1], st));
  HIPCHK(a, hipStreamSynchronize(st));
  (void)elapsed_ms(q->ev[0], q->ev[1], &info->add_ms);
  q->tot.accumulate(&info->batch, &q->totals);
  info->n_junctions = q->n_tab;
  info->held_bytes = q->held_bytes();
  return THM_OK;
}

// the checks of thm_quant_add_view, on the host before anything goes up
int check_view(thm_quant* q, const thm_cigar_view* v) {
  thm_aligner* a = q->a;
  const char* who = "thm_quant_add_view";
  return check_cigar_view(a, who, v, q->h_ref_sq, [&](uint64_t i, const thm_aln& al, const thm_aln_digest& d) {
    if (d.flags & THM_DIGEST_LONG_RUN) return (int)THM_OK;
    const unsigned long long at = i;
    uint64_t span = 0;
    const uint32_t n_hits = quant::count_hits(v->cigar + d.cigar_off, d.n_cigar, &span);
    if (al.ystart > 0xFFFFFFFFull || al.ystart + span > 0xFFFFFFFFull)
      return fail(a, THM_ERR_INVALID_ARG, "%s: alignment %llu: position %llu + %llu is 2^32 or more", who, at, (unsigned long long)al.ystart, (unsigned long long)span);
    if (n_hits && al.aln_type != THM_ALN_EXONIC)
      return fail(a, THM_ERR_INVALID_ARG, "%s: alignment %llu: an N word in an alignment that is not exonic has no strand", who, at);
    return (int)THM_OK;
  });
}

}  // namespace

extern "C" {

int32_t thm_quant_create(thm_aligner* a, thm_quant** out) {
  if (!out) return THM_ERR_INVALID_ARG;
  *out = nullptr;
  if (!a) return THM_ERR_INVALID_ARG;
  const thm_index* ix = a->ix;
  for (size_t r = 0; r < ix->refs.size(); r++)
    if (ix->refs[r].len >= (1ull << 32))
      return fail(a, THM_ERR_UNSUPPORTED, "thm_quant_create: contig %zu has %llu bases, 2^32 or more", r, (unsigned long long)ix->refs[r].len);
  if (ix->genes.size() > 0x3FFFFFFFull) return fail(a, THM_ERR_UNSUPPORTED, "thm_quant_create: 2^30 genes or more");
  HIPCHK(a, hipSetDevice(a->device));
  int rc = bam_tables_on_device(a);
  if (rc != THM_OK) return rc;
  thm_quant* q = new thm_quant();
  q->a = a;
  memset(&q->totals, 0, sizeof q->totals);
  const size_t n_refs = ix->refs.size(), n_txs = ix->txs.size(), n_genes = ix->genes.size();
  q->h_ref_sq.assign(n_refs, -1);
  std::vector<uint8_t> fwd(n_txs + 1, 0);
  for (size_t t = 0; t < n_txs; t++) fwd[t] = ix->txs[t].strand ? 1 : 0;
  hipError_t e = q->tx_forward.ensure(fwd.size());
  if (e == hipSuccess) e = q->genes.ensure(n_genes * 4 + 1);
  if (e == hipSuccess) e = hipMemcpy(q->tx_forward, fwd.data(), fwd.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(q->genes, 0, (n_genes * 4 + 1) * 8);
  if (e == hipSuccess && n_refs) e = hipMemcpy(q->h_ref_sq.data(), a->bam.ref_sq, n_refs * 4, hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    delete q;
    return fail(a, e == hipErrorOutOfMemory ? THM_ERR_OOM : THM_ERR_HIP, "thm_quant_create: %s", hipGetErrorString(e));
  }
  int32_t top = -1;
  for (int32_t s : q->h_ref_sq) top = s > top ? s : top;
  q->n_sq = (uint32_t)(top + 1);
  *out = q;
  return THM_OK;
}

void thm_quant_free(thm_quant* q) { free_summary(q); }

int32_t thm_quant_add(thm_quant* q, thm_quant_info* info) {
  if (!q || !info) return THM_ERR_INVALID_ARG;
  memset(info, 0, sizeof(*info));
  QuantBatch b{};
  if (const int rc = resident_batch(q->a, &b); rc != THM_OK) return rc;
  return add_batch(q, "thm_quant_add", b, info);
}

int32_t thm_quant_add_view(thm_quant* q, const thm_cigar_view* v, thm_quant_info* info) {
  if (!q || !v || !info) return THM_ERR_INVALID_ARG;
  memset(info, 0, sizeof(*info));
  QuantBatch b{};
  int rc = check_view(q, v);
  if (rc == THM_OK) rc = q->view.upload(q->a, v, &b);
  if (rc != THM_OK) return rc;
  return add_batch(q, "thm_quant_add_view", b, info);
}

int32_t thm_quant_fetch(thm_quant* q, thm_quant_view* out) {
  if (!q || !out) return THM_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  thm_aligner* a = q->a;
  HIPCHK(a, hipSetDevice(a->device));
  hipStream_t st = a->stream;
  const uint64_t n_genes = a->ix->genes.size(), n = q->n_tab;
  const size_t gene_bytes = n_genes * sizeof(thm_quant_gene), row_bytes = n * sizeof(thm_quant_junction);
  HIPCHK(a, ensure_events(q->ev_fetch));
  HIPCHK(a, q->d_rows.ensure(n, 16));
  HIPCHK(a, q->h_out.ensure(gene_bytes + row_bytes + 16));
  HIPCHK(a, hipEventRecord(q->ev_fetch[0], st));
  HIPCHK(a, launch_quant_rows(q->tab[q->cur].rows(), n, q->d_rows, st));
  if (gene_bytes) HIPCHK(a, hipMemcpyAsync(q->h_out.p, q->genes, gene_bytes, hipMemcpyDeviceToHost, st));
  if (row_bytes) HIPCHK(a, hipMemcpyAsync(q->h_out.as<uint8_t>() + gene_bytes, q->d_rows, row_bytes, hipMemcpyDeviceToHost, st));
  HIPCHK(a, hipEventRecord(q->ev_fetch[1], st));
  HIPCHK(a, hipStreamSynchronize(st));
  (void)elapsed_ms(q->ev_fetch[0], q->ev_fetch[1], &out->fetch_ms);
  out->n_genes = n_genes;
  out->genes = q->h_out.as<thm_quant_gene>();
  out->n_junctions = n;
  out->junctions = (const thm_quant_junction*)(q->h_out.as<uint8_t>() + gene_bytes);
  out->totals = q->totals;
  return THM_OK;
}

int32_t thm_quant_reset(thm_quant* q) {
  if (!q) return THM_ERR_INVALID_ARG;
  thm_aligner* a = q->a;
  HIPCHK(a, hipSetDevice(a->device));
  HIPCHK(a, hipMemsetAsync(q->genes, 0, (a->ix->genes.size() * 4 + 1) * 8, a->stream));
  HIPCHK(a, hipStreamSynchronize(a->stream));
  q->n_tab = 0;
  memset(&q->totals, 0, sizeof q->totals);
  return THM_OK;
}

}  // extern "C"
