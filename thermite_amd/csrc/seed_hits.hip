// seed_hits.hip -- host side of thm_align_seed_hits_batch (include/thermite.h): align_seed_hit
// (reference src/aligner.rs:198-314) for hits the caller chooses.  The checks that decide a hit's status on the host,
// the band classes (as classify() in extend_plan.h cuts them for reads), the launches of seed_hit_kernel
// (kernels_seed_hit.hip) and the canonical layout of the result.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "aligner_internal.h"

using namespace thm;

namespace {

struct Launch {
  int cpl;                 // 1..4, or 0: any width
  uint32_t max_len, max_bw;
  uint64_t list_off, n;    // the launch's hits: list[list_off .. list_off + n)
  bool retries;            // the any-width launch that also takes the register-resident launches' retries
};

template <class C>
int run_seed_hits(thm_aligner* a, const std::vector<Launch>& launches, uint64_t n_list_host, uint64_t pool_cap,
                  uint32_t mk_cap_slow) {
  hipStream_t s = a->stream;
  unsigned long long* ctl = a->sh.ctl;  // [0] op pool cursor, [1] retry count (list length of the retry launch)
  SeedHitParamsT<C> p;
  memset(&p, 0, sizeof p);
  if constexpr (sizeof(C) == 8)
    p.ix = a->dix->view64;
  else
    p.ix = a->dix->view;
  p.reads.bases = a->sh.san + 16;
  p.reads.offsets = a->sh.off;
  p.hits = a->sh.hits;
  p.hit_read = a->sh.read;
  p.bw = a->sh.bw;
  p.xd = a->sh.xd;
  p.retry = a->sh.list + n_list_host;
  p.retry_count = ctl + 1;
  p.out = a->sh.out;
  p.status = a->sh.status;
  p.cand_ops = a->sh.ops;
  p.cand_ops_cap = pool_cap;
  p.ops_cursor = ctl;
  p.counters = a->d_counters;
  p.fault = a->d_fault;
  HIPCHK(a, hipMemsetAsync(ctl, 0, 64, s));
  int rc = reset_queue(a);
  if (rc != THM_OK) return rc;
  unsigned q = 0;
  for (const Launch& l : launches) {
    p.list = a->sh.list + l.list_off;
    p.n_list = l.n;
    p.n_list_dev = l.retries ? ctl + 1 : nullptr;
    p.queue = a->d_queue + (q++) * EXT_QSTRIDE;
    p.max_read_len = l.max_len;
    p.max_bw = l.max_bw;
    p.mk_cap = l.cpl == 0 ? mk_cap_slow : (uint32_t)FAST_MAX_YCLIPS;
    p.trace_scratch = nullptr;
    p.slow_scratch = nullptr;
    p.slow_scratch_per_wave = 0;
    int n_blocks;
    if (l.cpl == 0) {
      const uint64_t per_wave = slow_wave_bytes(l.max_len, l.max_bw, p.mk_cap);
      const uint64_t waves = slow_launch_waves(per_wave, a->n_cu, l.retries ? (uint64_t)a->n_cu * 8 : std::max<uint64_t>(l.n, 1));
      n_blocks = (int)(waves / 4);
      HIPCHK(a, a->sh.slow.ensure((size_t)waves * per_wave, 256));
      p.slow_scratch = a->sh.slow;
      p.slow_scratch_per_wave = per_wave;
    } else {
      const size_t lds = extend_lds_bytes(l.max_len, l.max_bw, l.cpl);
      n_blocks = grid_blocks(a, l.n, 4, lds_blocks_per_cu(lds, 4));
      const size_t trace_per_wave = extend_trace_scratch_bytes(l.max_len, l.max_bw, l.cpl);
      HIPCHK(a, a->sh.trace.ensure((size_t)n_blocks * 4 * trace_per_wave + 64));
      p.trace_scratch = a->sh.trace.as<unsigned long long>();
    }
    HIPCHK(a, launch_seed_hits(p, l.cpl, n_blocks, s));
  }
  return THM_OK;
}

}  // namespace

extern "C" {

int32_t thm_align_seed_hits_batch(thm_aligner* a, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads,
                                  const uint64_t* hit_off, const thm_mem* hits, uint64_t n_hits,
                                  const uint32_t* band_width, const int32_t* x_drop, uint32_t max_band_width,
                                  thm_hits_view* out) {
  if (!a || !out) return THM_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  if (!offsets || !hit_off) return fail(a, THM_ERR_INVALID_ARG, "thm_align_seed_hits_batch: null offsets or hit_off");
  if (n_hits && (!hits || !band_width || !x_drop)) return fail(a, THM_ERR_INVALID_ARG, "thm_align_seed_hits_batch: null hits, band_width or x_drop");
  if (offsets[0] != 0 || hit_off[0] != 0) return fail(a, THM_ERR_INVALID_ARG, "offsets[0] and hit_off[0] must be 0");
  for (uint64_t r = 0; r < n_reads; r++) {
    if (offsets[r + 1] < offsets[r]) return fail(a, THM_ERR_INVALID_ARG, "read offsets are not monotone");
    if (hit_off[r + 1] < hit_off[r]) return fail(a, THM_ERR_INVALID_ARG, "hit offsets are not monotone");
  }
  if (hit_off[n_reads] != n_hits) return fail(a, THM_ERR_INVALID_ARG, "hit_off[n_reads] = %llu != n_hits = %llu",
                                              (unsigned long long)hit_off[n_reads], (unsigned long long)n_hits);
  const uint64_t n_bases = offsets[n_reads];
  if (n_bases && !bases) return fail(a, THM_ERR_INVALID_ARG, "thm_align_seed_hits_batch: null bases");
  if (n_reads >= 0xFFFFFFFFull || n_hits >= 0xFFFFFFFFull) return fail(a, THM_ERR_UNSUPPORTED, "more than 2^32-1 reads or hits in one call");
  a->h_hit_alns.clear();
  a->h_hit_status.clear();
  a->h_hit_ops.clear();
  out->alns = a->h_hit_alns.data();
  out->ops = a->h_hit_ops.data();
  if (n_hits == 0) return THM_OK;
  HIPCHK(a, hipSetDevice(a->device));
  const thm_index* ix = a->ix;

  // ---- per-hit checks: what panics in the reference, what this build does not hold ----
  std::vector<int32_t> status(n_hits, THM_OK);
  std::vector<uint32_t> hit_read(n_hits);
  for (uint64_t r = 0; r < n_reads; r++)
    for (uint64_t h = hit_off[r]; h < hit_off[r + 1]; h++) hit_read[h] = (uint32_t)r;
  const uint32_t mk_cap_slow = std::max<uint32_t>(ix->max_tx_exons, 1);
  for (uint64_t h = 0; h < n_hits; h++) {
    const uint64_t L = offsets[hit_read[h] + 1] - offsets[hit_read[h]];
    const thm_mem& m = hits[h];
    const uint32_t bw = band_width[h];
    int32_t st = THM_OK;
    if (L > MAX_READ_LEN) {
      st = THM_ERR_UNSUPPORTED;
    } else if ((uint64_t)m.query_idx + m.len > L || bw > max_band_width || x_drop[h] < (int64_t)bw) {
      st = THM_ERR_OUT_OF_CONTRACT;  // &read[q + len..] (src/aligner.rs:360), assert! at src/swg.rs:32, SURVEY A.5
    } else if (m.ref_idx >= ix->n || m.ref_idx + m.len > ix->n) {
      st = THM_ERR_OUT_OF_CONTRACT;  // Index::idx_to_ref past the last Ref / seq_slice past the text
    } else {
      // the hit must end before its contig copy's '$': ref_seq[hit.ref_idx + hit.len..] of the window (:213-227)
      uint64_t off = 0;
      const int32_t k = thm_index_idx_to_ref(ix, m.ref_idx, &off);
      if (k < 0 || m.ref_idx + m.len > ix->refs[k].end_idx - 1) st = THM_ERR_OUT_OF_CONTRACT;
      else if (bw > 2 * MAX_READ_LEN || extend_slow_scratch_bytes((uint32_t)L, bw, mk_cap_slow) > SLOW_SCRATCH_BUDGET)
        st = THM_ERR_UNSUPPORTED;  // its DP trace alone exceeds the device-memory budget
    }
    status[h] = st;
  }

  // ---- band classes: register-resident cpl 1..4 while the LDS carve fits, else the any-width kernel ----
  std::vector<uint32_t> by_cls[5];
  for (uint64_t h = 0; h < n_hits; h++) {
    if (status[h] != THM_OK) continue;
    const int cpl = cells_per_lane(band_width[h]);
    by_cls[cpl <= 4 ? cpl : 0].push_back((uint32_t)h);
  }
  auto len_of = [&](uint32_t h) { return (uint32_t)(offsets[hit_read[h] + 1] - offsets[hit_read[h]]); };
  std::vector<Launch> launches;
  std::vector<uint32_t> list;
  uint32_t fast_len = 0, fast_bw = 0;
  for (int cpl = 1; cpl <= 4; cpl++) {
    std::vector<uint32_t>& v = by_cls[cpl];
    if (v.empty()) continue;
    uint32_t bw = 0;
    for (uint32_t h : v) bw = std::max(bw, band_width[h]);
    // shortest reads first: the longest prefix whose LDS carve fits stays, the rest takes the any-width kernel
    std::stable_sort(v.begin(), v.end(), [&](uint32_t x, uint32_t y) { return len_of(x) < len_of(y); });
    size_t keep = v.size();
    while (keep > 0 && extend_lds_bytes(len_of(v[keep - 1]), bw, cpl) > EXTEND_LDS_LIMIT) keep--;
    for (size_t i = keep; i < v.size(); i++) by_cls[0].push_back(v[i]);
    if (keep == 0) continue;
    Launch l{cpl, len_of(v[keep - 1]), bw, list.size(), keep, false};
    list.insert(list.end(), v.begin(), v.begin() + keep);
    launches.push_back(l);
    fast_len = std::max(fast_len, l.max_len);
    fast_bw = std::max(fast_bw, bw);
  }
  // any-width launches: hits by band, cut where the class's buffers would exceed the budget
  {
    std::vector<uint32_t>& v = by_cls[0];
    std::stable_sort(v.begin(), v.end(), [&](uint32_t x, uint32_t y) { return band_width[x] < band_width[y]; });
    size_t i = 0;
    while (i < v.size()) {
      uint32_t ml = 0, mb = 0;
      size_t j = i;
      for (; j < v.size(); j++) {
        const uint32_t l2 = std::max(ml, len_of(v[j])), b2 = std::max(mb, band_width[v[j]]);
        if (j > i && extend_slow_scratch_bytes(l2, b2, mk_cap_slow) > SLOW_SCRATCH_BUDGET) break;
        ml = l2;
        mb = b2;
      }
      launches.push_back(Launch{0, ml, mb, list.size(), j - i, false});
      list.insert(list.end(), v.begin() + i, v.begin() + j);
      i = j;
    }
  }
  const uint64_t n_list_host = list.size();
  // an alignment across more introns than the register-resident kernels' marker list holds: those hits are redone
  // by one more any-width launch, sized for every register-resident hit
  const bool retry_possible = fast_len > 0 && ix->max_tx_exons > (uint32_t)FAST_MAX_YCLIPS + 1;
  if (retry_possible) launches.push_back(Launch{0, fast_len, fast_bw, n_list_host, 0, true});

  // ---- upload ----
  hipStream_t s = a->stream;
  HIPCHK(a, a->sh.bases.ensure(n_bases, 64));
  HIPCHK(a, a->sh.san.ensure(n_bases, 256 + 16));
  HIPCHK(a, a->sh.off.ensure(n_reads + 1));
  HIPCHK(a, a->sh.hits.ensure(n_hits));
  HIPCHK(a, a->sh.read.ensure(n_hits));
  HIPCHK(a, a->sh.bw.ensure(n_hits));
  HIPCHK(a, a->sh.xd.ensure(n_hits));
  HIPCHK(a, a->sh.list.ensure(n_list_host + n_hits, 16));
  HIPCHK(a, a->sh.out.ensure(n_hits));
  HIPCHK(a, a->sh.status.ensure(n_hits));
  HIPCHK(a, a->sh.ctl.ensure(8));
  if (n_bases) HIPCHK(a, hipMemcpyAsync(a->sh.bases, bases, n_bases, hipMemcpyHostToDevice, s));
  HIPCHK(a, hipMemcpyAsync(a->sh.off, offsets, (n_reads + 1) * 8, hipMemcpyHostToDevice, s));
  HIPCHK(a, hipMemcpyAsync(a->sh.hits, hits, n_hits * sizeof(thm_mem), hipMemcpyHostToDevice, s));
  HIPCHK(a, hipMemcpyAsync(a->sh.read, hit_read.data(), n_hits * 4, hipMemcpyHostToDevice, s));
  HIPCHK(a, hipMemcpyAsync(a->sh.bw, band_width, n_hits * 4, hipMemcpyHostToDevice, s));
  HIPCHK(a, hipMemcpyAsync(a->sh.xd, x_drop, n_hits * 4, hipMemcpyHostToDevice, s));
  if (n_list_host) HIPCHK(a, hipMemcpyAsync(a->sh.list, list.data(), n_list_host * 4, hipMemcpyHostToDevice, s));
  HIPCHK(a, hipMemcpyAsync(a->sh.status, status.data(), n_hits * 4, hipMemcpyHostToDevice, s));
  // upper-cased, sanitised copy (sanitize_kernel, the normalisation thm_align_batch applies: src/aligner.rs:125)
  HIPCHK(a, launch_sanitize(a->sh.bases, a->sh.san + 16, n_bases, n_bases + 128, s));

  // ---- run; an op pool that overflows is grown and the run replayed (counters restored first) ----
  uint64_t pool_cap = 0;
  for (uint32_t h : list) pool_cap += 4ull * len_of(h) + 4ull * band_width[h] + 64;  // two paths of <= 2 (L + bw) ops, clips
  pool_cap += (uint64_t)a->n_cu * 64 * 4096;
  HIPCHK(a, hipMemcpyAsync(a->d_counters + THM_N_COUNTERS, a->d_counters, THM_N_COUNTERS * 8,
                           hipMemcpyDeviceToDevice, s));
  unsigned long long ctl[2] = {0, 0};
  int fault = 0;
  for (int attempt = 0;; attempt++) {
    HIPCHK(a, a->sh.ops.ensure(pool_cap, 64));
    int rc = a->dix->wide ? run_seed_hits<uint64_t>(a, launches, n_list_host, pool_cap, mk_cap_slow)
                          : run_seed_hits<uint32_t>(a, launches, n_list_host, pool_cap, mk_cap_slow);
    if (rc != THM_OK) return rc;
    HIPCHK(a, hipMemcpyAsync(ctl, a->sh.ctl, sizeof ctl, hipMemcpyDeviceToHost, s));
    HIPCHK(a, hipMemcpyAsync(&fault, a->d_fault, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(a, hipStreamSynchronize(s));
    if (fault & FAULT_INTERNAL) return fail(a, THM_ERR_INTERNAL, "seed_hit_kernel reported an internal inconsistency");
    if (!(fault & FAULT_OPS_POOL)) break;
    if (attempt >= 4) return fail(a, THM_ERR_INTERNAL, "op pool kept overflowing");
    pool_cap = std::max<uint64_t>(pool_cap * 2, ctl[0] + ctl[0] / 2 + 65536);
    HIPCHK(a, hipMemcpyAsync(a->d_counters, a->d_counters + THM_N_COUNTERS, THM_N_COUNTERS * 8,
                             hipMemcpyDeviceToDevice, s));
    HIPCHK(a, hipMemcpyAsync(a->sh.status, status.data(), n_hits * 4, hipMemcpyHostToDevice, s));
  }

  // ---- fetch and lay out: records in hit order, op streams back to back (gx ops, then tx ops) ----
  const uint64_t used = std::min<uint64_t>(ctl[0], pool_cap);
  std::vector<thm_aln> raw(n_hits);
  std::vector<uint8_t> pool_h(used);
  a->h_hit_status.resize(n_hits);
  HIPCHK(a, hipMemcpyAsync(raw.data(), a->sh.out, n_hits * sizeof(thm_aln), hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipMemcpyAsync(a->h_hit_status.data(), a->sh.status, n_hits * 4, hipMemcpyDeviceToHost, s));
  if (used) HIPCHK(a, hipMemcpyAsync(pool_h.data(), a->sh.ops, used, hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipStreamSynchronize(s));
  a->h_hit_alns.assign(n_hits, thm_aln());
  uint64_t n_failed = 0;
  for (uint64_t h = 0; h < n_hits; h++) {
    if (a->h_hit_status[h] != THM_OK) {
      n_failed++;
      continue;
    }
    thm_aln r = raw[h];
    if (r.ops_off + r.ops_len > used || (r.tx_ops_len && r.tx_ops_off + r.tx_ops_len > used))
      return fail(a, THM_ERR_INTERNAL, "hit %llu: op stream outside the pool", (unsigned long long)h);
    const uint64_t go = a->h_hit_ops.size();
    a->h_hit_ops.insert(a->h_hit_ops.end(), pool_h.begin() + r.ops_off, pool_h.begin() + r.ops_off + r.ops_len);
    const uint64_t to = a->h_hit_ops.size();
    if (r.tx_ops_len)
      a->h_hit_ops.insert(a->h_hit_ops.end(), pool_h.begin() + r.tx_ops_off, pool_h.begin() + r.tx_ops_off + r.tx_ops_len);
    r.ops_off = go;
    r.tx_ops_off = r.aln_type == THM_ALN_EXONIC ? to : 0;
    a->h_hit_alns[h] = r;
  }
  out->n_hits = n_hits;
  out->n_op_bytes = a->h_hit_ops.size();
  out->alns = a->h_hit_alns.data();
  out->ops = a->h_hit_ops.data();
  out->n_failed_hits = n_failed;
  out->hit_status = n_failed ? a->h_hit_status.data() : nullptr;
  return THM_OK;
}

}  // extern "C"
