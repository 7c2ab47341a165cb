// kernels_seed_hit.hip -- align_seed_hit (reference src/aligner.rs:198-314) for caller-chosen hits, one hit per
// wavefront: the kernel behind thm_align_seed_hits_batch (host side: seed_hits.hip).  Built from the wave-level helpers
// extend_kernel uses (extend_device.h).
#include <hip/hip_runtime.h>

#include "extend_device.h"

namespace thm {
namespace dev {

// One hit per wavefront: align_seed_hit (src/aligner.rs:198-314) statement by statement, from the helpers extend_kernel
// uses -- without align_read's loop around it (no band narrowing, no score filter, no intron_mode check, no
// filter_overlapping) and without extend_kernel's reuse of the genome extensions for a transcript (an exact shortcut:
// here every transcript target runs its two SwgExtend::extend calls).  CPL and the buffers as in extend_kernel.
template <class C, int CPL>
__global__ __launch_bounds__(256, 4) void seed_hit_kernel(SeedHitParamsT<C> p) {
  typedef typename CoordTraits<C>::S S;
  constexpr bool GS = (CPL == 0);
  typedef WctxT<GS> Wctx;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int lane = lane_id();
  const int wave = bcast_first((int)(threadIdx.x >> 6));
  const unsigned wave_global = blockIdx.x * (blockDim.x >> 6) + (unsigned)wave;
  const ExtCaps caps = ext_caps(p.max_read_len, p.max_bw, CPL);
  const uint32_t lcap = caps.lcap;
  Wctx c;
  carve_wave<CPL>(c, p, caps, smem, wave, wave_global, false);  // (the candidate keys are not used here)
  const auto& ix = p.ix;
  const uint64_t n_list = p.n_list_dev ? (uint64_t)uload(p.n_list_dev) : p.n_list;
  unsigned long long k_hits = 0, k_cells = 0, k_cols = 0, k_calls = 0, k_win = 0, k_opb = 0;
  int batch_fault = 0;

  for (;;) {
    unsigned g = 0;
    if (lane == 0) g = atomicAdd(p.queue, 1u);
    g = (unsigned)bcast_first((int)g);
    if (g >= n_list) break;
    const uint32_t hidx = uload(&p.list[g]);
    const thm_mem hit = uload(&p.hits[hidx]);
    const uint32_t rd_idx = uload(&p.hit_read[hidx]);
    const uint64_t r0 = uload(&p.reads.offsets[rd_idx]);
    const int L = (int)(uload(&p.reads.offsets[rd_idx + 1]) - r0);
    c.L = L;
    #pragma unroll 1
    for (int t = lane; t < (int)lcap; t += 64) c.rd[t] = (t < L) ? p.reads.bases[r0 + t] : (uint8_t)0;
    wsync(c);
    const int bw = (int)uload(&p.bw[hidx]), xd = uload(&p.xd[hidx]);
    const S hr = (S)hit.ref_idx;
    const int q = (int)hit.query_idx, len = (int)hit.len;
    const RefInfoT<C> ref = idx_to_ref<C>(ix, (C)hr);
    const C qs = (C)hr, qe = (C)(hr + len);

    // ---- genome window (:209-227): staged as extend_kernel stages it (unclamped, the text is padded) ----
    const S rs = (S)ref.start;
    const S seq_start = max((hr > L + bw) ? hr - (S)(L + bw) : (S)0, rs);
    const S seq_end = min(hr + (S)(len + L + bw), (S)ref.end - 1);
    const S gw_a = max(hr - (S)(L + bw), (S)0);
    const S gw_b = min(hr + (S)(len + L + bw), (S)ix.n);
    const unsigned gw_mis = (unsigned)((uintptr_t)(ix.text + gw_a) & 15u);
    const int gw_n = (int)(gw_b - gw_a) + (int)gw_mis;
    if (gw_n > c.wcap) {
      c.fault |= FAULT_INTERNAL;
    } else {
      const uint4* gw_src = (const uint4*)(ix.text + gw_a - gw_mis);
      uint4* wdst = (uint4*)c.wing;
      #pragma unroll 1
      for (int t2 = lane; t2 * 16 < gw_n; t2 += 64) wdst[t2] = gw_src[t2];
    }
    c.winbytes += (unsigned)(seq_end - seq_start);
    wsync(c);
    LrMemo gmemo, tmemo;
    const PathT<S> gx = extend_lr<CPL, S>(c, c.wing, gw_a - (S)gw_mis, seq_start, seq_end, hr, q, len, bw, xd, c.pa, gmemo);

    // ---- every transcript exon_to_tx.find yields (:229-258) ----
    PathT<S> best = gx;
    bool have_best = false;
    uint32_t best_tx = 0, best_tlen = 0;
    uint8_t* cur_buf = c.pb;
    uint8_t* best_buf = c.pc;
    GridQueryT<C, ExonEntryT<C>> eg;
    grid_begin<C>(eg, ix.exon_grid_off, ix.exon_grid, qs, qe);
    for (;;) {
      uint32_t tx_idx = 0, ent_idx = 0;
      if (!grid_next(eg, tx_idx, ent_idx)) break;
      const ExonEntryT<C> ge = uload(&eg.ent[ent_idx]);
      const TxSeedT<S> ts = lift_seed_to_tx<S>(c, ix, ge, tx_idx, qs, qe, hr, q, len);  // lift_mem_to_tx (src/txome.rs:82-103)
      if (!ts.ok) continue;
      // window of the transcript around the lifted seed
      const int tlen = (int)ts.seq_len;
      const int ws = (ts.t_r > L + bw) ? ts.t_r - (L + bw) : 0;
      const int we = min(tlen, ts.t_r + ts.t_len + L + bw + 1);
      const int w0 = stage_window(c, c.win, ix.tx_seq + ts.seq_off, ws, we);
      const SeedMatch sm = seed_match_wave(c, w0, tlen, ts.t_r, ts.t_q, ts.t_len);  // extend_seed_match (src/aligner.rs:410-426)
      const PathT<S> pth = extend_lr<CPL, S>(c, c.win, (S)w0, (S)0, (S)tlen, (S)sm.t_r, sm.t_q, sm.t_len, bw, xd, cur_buf, tmemo);
      if (!have_best || pth.score > best.score) {  // strictly better (:249)
        have_best = true;
        best_tx = tx_idx;
        best_tlen = ge.seq_len;
        best = pth;
        uint8_t* tmp = cur_buf;
        cur_buf = best_buf;
        best_buf = tmp;
      }
      if (pth.score >= L * MATCH_SCORE) break;  // cannot beat an exact match (:253-257)
    }

    // ---- exonic vs unspliced (:263-313) ----
    const bool exonic = have_best && best.score >= gx.score;
    int aln_type = THM_ALN_INTERGENIC;
    uint32_t type_idx = THM_NO_IDX;
    S cy0 = gx.ystart, cy1 = gx.yend;
    const uint8_t* g_path = c.pa;
    int g_n = gx.nops, g_ny = 0;
    int sc = gx.score, xs_ = gx.xstart, xe_ = gx.xend;
    if (exonic) {
      // lift_tx_to_gx (src/txome.rs:110-160)
      g_path = best_buf;
      g_n = best.nops;
      aln_type = THM_ALN_EXONIC;
      type_idx = best_tx;
      sc = best.score;
      xs_ = best.xstart;
      xe_ = best.xend;
      g_ny = lift_markers<S>(c, ix, uload(&ix.txs[best_tx]), best_buf, best.nops, best.xend < L, (int)best.ystart, (int)best.yend,
                             cy0, cy1);
    } else {
      // first interval gene_intervals.find yields (:283-288, :306)
      GridQueryT<C, GridEntryT<C>> gg;
      grid_begin<C>(gg, ix.gene_grid_off, ix.gene_grid, (C)cy0, (C)cy1);
      uint32_t gene = 0, gene_ent = 0;
      if (grid_next(gg, gene, gene_ent)) {
        aln_type = THM_ALN_INTRONIC;
        type_idx = gene;
      }
    }
    if (c.fault & FAULT_RETRY) {
      // more introns than this kernel's marker list holds: the any-width launch redoes the hit
      c.fault &= ~(FAULT_RETRY | FAULT_CONTRACT);
      if (lane == 0) {
        const unsigned long long slot = atomicAdd(p.retry_count, 1ull);
        p.retry[slot] = hidx;
      }
      c.cells = c.cols = c.calls = c.winbytes = 0;
      continue;
    }
    if (c.fault & FAULT_CONTRACT) {
      // a lift that panics in the reference: per-hit status, no record
      c.fault &= ~FAULT_CONTRACT;
      if (lane == 0) p.status[hidx] = THM_ERR_OUT_OF_CONTRACT;
    } else {
      const ChrSpanT<C> cs = chr_span<C>(ix, ref, cy0, cy1);  // concat_to_chr_aln (:429-449)
      int nb = 0, tnb = 0;
      const unsigned long long off = emit_alignment(c, p, g_path, g_n, xs_, xe_, cs.rev, g_ny, nb);
      unsigned long long toff2 = 0;
      if (exonic) toff2 = emit_alignment(c, p, best_buf, best.nops, best.xstart, best.xend, false, 0, tnb);
      if (lane == 0) {
        thm_aln a;
        a.ystart = cs.ch0;
        a.yend = cs.ch1;
        a.ylen = (uint64_t)cs.cref.len;
        a.ops_off = off;
        a.tx_ystart = exonic ? (uint64_t)best.ystart : 0;
        a.tx_yend = exonic ? (uint64_t)best.yend : 0;
        a.tx_ylen = exonic ? (uint64_t)best_tlen : 0;
        a.tx_ops_off = exonic ? toff2 : 0;
        a.score = sc;
        a.ref_id = ref.id;
        a.xstart = (uint32_t)xs_;
        a.xend = (uint32_t)xe_;
        a.xlen = (uint32_t)L;
        a.ops_len = (uint32_t)nb;
        a.tx_or_gene_idx = type_idx;
        a.tx_score = exonic ? best.score : 0;
        a.tx_xstart = exonic ? (uint32_t)best.xstart : 0;
        a.tx_xend = exonic ? (uint32_t)best.xend : 0;
        a.tx_ops_len = (uint32_t)tnb;
        a.strand = ref.strand ? 1 : 0;
        a.primary = 0;
        a.aln_type = (uint8_t)aln_type;
        a.pad_ = 0;
        p.out[hidx] = a;
        p.status[hidx] = THM_OK;
      }
      k_opb += (unsigned long long)(nb + tnb);
    }
    batch_fault |= c.fault;
    c.fault = 0;
    k_hits++;
    k_cells += c.cells;
    k_cols += c.cols;
    k_calls += c.calls;
    k_win += c.winbytes;
    c.cells = c.cols = c.calls = c.winbytes = 0;
    wsync(c);
  }
  batch_fault |= c.fault;
  if (lane == 0) {
    if (batch_fault & (FAULT_OPS_POOL | FAULT_INTERNAL)) atomicOr(p.fault, batch_fault & (FAULT_OPS_POOL | FAULT_INTERNAL));
    if (k_hits) {
      atomicAdd(&p.counters[THM_CNT_HITS], k_hits);
      atomicAdd(&p.counters[THM_CNT_SWG_CALLS], k_calls);
      atomicAdd(&p.counters[THM_CNT_DP_CELLS], k_cells);
      atomicAdd(&p.counters[THM_CNT_DP_COLS], k_cols);
      atomicAdd(&p.counters[THM_CNT_OP_BYTES], k_opb);
      atomicAdd(&p.counters[THM_CNT_WINDOW_BYTES], k_win);
    }
  }
}

}  // namespace dev

template <class C>
static hipError_t launch_seed_hits_t(const SeedHitParamsT<C>& p, int cpl, int n_blocks, hipStream_t s) {
  const size_t lds = cpl == 0 ? 0 : extend_lds_bytes(p.max_read_len, p.max_bw, cpl);
  auto go = [&](auto kern) { return launch_with_lds(kern, n_blocks, 256, lds, s, p); };
  switch (cpl) {
    case 0: return go(dev::seed_hit_kernel<C, 0>);
    case 1: return go(dev::seed_hit_kernel<C, 1>);
    case 2: return go(dev::seed_hit_kernel<C, 2>);
    case 3: return go(dev::seed_hit_kernel<C, 3>);
    case 4: return go(dev::seed_hit_kernel<C, 4>);
    default: return hipErrorInvalidValue;
  }
}
hipError_t launch_seed_hits(const SeedHitParamsT<uint32_t>& p, int cpl, int n_blocks, hipStream_t s) { return launch_seed_hits_t(p, cpl, n_blocks, s); }
hipError_t launch_seed_hits(const SeedHitParamsT<uint64_t>& p, int cpl, int n_blocks, hipStream_t s) { return launch_seed_hits_t(p, cpl, n_blocks, s); }

}  // namespace thm
