// kernels_extend.hip -- the per-read aligner: one read per wavefront.
//
// extend_kernel restates aligner::align_read (reference src/aligner.rs:123-190) with align_seed_hit
// (src/aligner.rs:198-314) and filter_overlapping (src/aligner.rs:317-349) in its body; the wave-level helpers below
// them, and the table of the reference functions they restate, are in extend_device.h.
//
// The hits of one read are processed strictly in the reference's order because
// band_width / x_drop / max_aln_score are loop-carried (src/aligner.rs:143-175).
// Reads are independent, so the parallelism is: reads over wavefronts, band
// cells over lanes.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "extend_device.h"

namespace thm {
namespace dev {

#ifndef THM_READ_RUN
#define THM_READ_RUN 4
#endif
constexpr int READ_RUN = THM_READ_RUN;  // consecutive reads per queue atomic of the wave-per-read kernels
constexpr int TEAM_MAX_CHUNKS = 16384;  // chunks a team keeps book of (reads beyond that stay with the sequential path)
constexpr int TEAM_CHUNK = 4;           // hits per chunk of a team

// (ExtCaps / ext_caps, SlowLayout / slow_layout: extend_plan.h)

#ifndef THM_KARG_QUAL
#define THM_KARG_QUAL volatile
#endif
// C: coordinate width.  CPL: band slots per lane of the register-resident DP (1..4), or 0 for the any-width
// kernel (band in tiles, wave-private buffers in global memory): the slow path for reads whose band or length
// exceeds what LDS and registers hold.  MINW: waves per SIMD the register budget is set for.
//
// TEAM > 0: the kernel for reads with very many seed hits (plan_kernel lists them).  A workgroup of
// TEAM wavefronts works on ONE read at a time.  The hits of a read must be taken in order because band, X-drop
// and best score are carried from hit to hit (src/aligner.rs:143-175) -- but they change only when a hit beats the
// best score so far, which happens a handful of times per read, early.  So the hits are cut into the chunks of
// up to 64 the loop below walks anyway, and in every round wave w takes chunk (base + w), starting from the state
// that is known to hold at chunk `base` -- speculating that the chunks before its own leave the state alone.
// After the round the chunks up to and including the first one that changed the state are valid (each of them did
// start from the true state); their candidates and counters are kept, the state moves on, and the chunks behind
// them are redone in the next round.  Exact: every hit that is kept was extended under exactly the band, X-drop
// and threshold the sequential loop would have used.  Speed-up on a read whose state has settled: TEAM-fold.
template <class C, int CPL, int MINW, int TEAM = 0>
__global__ __launch_bounds__(TEAM > 0 ? 64 * TEAM : 256, TEAM > 0 ? 1 : MINW) void extend_kernel(ExtendParamsT<C> p_by_value) {
  typedef typename CoordTraits<C>::S S;
  constexpr bool GS = (CPL == 0);
  constexpr bool TM = TEAM > 0;
  constexpr int TW = TM ? TEAM : 1;
  // team state (LDS, unused when TEAM == 0)
  __shared__ int t_res[TW][8];        // per wave and round: accepted candidates, state changed?, band, X-drop, best score, per-read fault bits
  __shared__ int t_state[4];          // the state in force at chunk t_ctl[1]: band, X-drop, best score
  __shared__ unsigned t_ctl[4];       // [0] list slot of the read, [1] first chunk of the round, [2] accepted so far, [3] per-read fault bits
  __shared__ unsigned char t_nacc[TM ? TEAM_MAX_CHUNKS : 1];  // accepted candidates per finished chunk (<= TEAM_CHUNK)
  static_assert(!TM || sizeof(t_res) + sizeof(t_state) + sizeof(t_ctl) + sizeof(t_nacc) <= TEAM_STATIC_LDS, "extend_plan.h: TEAM_STATIC_LDS");
  typedef WctxT<GS> Wctx;
  // The parameter block (about 80 dwords) is read from the kernel-argument segment where it is
  // needed (scalar loads, THM_KARG_QUAL = volatile keeps them at their use sites) instead of being
  // loaded at entry: the kernel is far over the scalar register budget, and every parameter that
  // lives in a register across the hit loop is spilled to VGPR lanes and read back with v_readlane.
#if __HIP_DEVICE_COMPILE__
  typedef THM_KARG_QUAL const __attribute__((address_space(4))) ExtendParamsT<C> KArgs;
  KArgs& p = *(KArgs*)__builtin_amdgcn_kernarg_segment_ptr();
#else
  const ExtendParamsT<C>& p = p_by_value;
#endif
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int lane = lane_id();
  const int wave = bcast_first((int)(threadIdx.x >> 6));  // wave-uniform: LDS bases stay on the scalar unit
  const unsigned wave_global = blockIdx.x * (blockDim.x >> 6) + (unsigned)wave;
  // ---- wave-private buffers (LDS carve must match extend_lds_bytes; global layout = slow_layout) ----
  const ExtCaps caps = ext_caps(p.max_read_len, p.max_bw, CPL);
  const uint32_t lcap = caps.lcap;
  Wctx c;
  carve_wave<CPL>(c, p, caps, smem, wave, wave_global, true);
#ifdef THM_PROF
  for (int t = 0; t < 10; t++) c.prof_acc[t] = 0;
  for (int t = 0; t < 6; t++) c.prof_cols[t] = 0;
  c.prof_hit = c.prof_tx = 0;
  c.prof_last = __builtin_amdgcn_s_memtime();
#endif

#ifdef THM_TIMELINE
  // diagnosis build (tools/timeline.py): when do the waves of the wave-per-read kernel run out of work, and how long do
  // reads take?
  const unsigned long long tl_start = __builtin_amdgcn_s_memrealtime();  // 100 MHz
  unsigned long long tl_last = tl_start;
  unsigned tl_last_hits = 0, tl_reads = 0, tl_tx = 0;
  unsigned long long tl_longest = 0;
  auto tl_close = [&](unsigned long long now) {  // the read that started at tl_last ends now
    if (!tl_reads) return;
    const unsigned long long d = now - tl_last;  // 10 ns units
    const unsigned long long key = (d << 32) | ((unsigned long long)min(tl_tx, 65535u) << 16) | tl_last_hits;
    if (key > tl_longest) tl_longest = key;
  };
#endif
  // SMEM pool overflow in the seed stage: the per-read SMEM runs are incomplete (the host grows the pool and
  // replays the batch); nothing of them may be read
  if (uload(p.fault_seed) != 0) return;
  auto& ix = p.ix;
  unsigned long long k_aligned = 0, k_unmapped = 0, k_alns = 0, k_reads = 0, k_opb = 0;
  unsigned k_type[3] = {0, 0, 0};  // wave-uniform (counted with ballots)
  unsigned long long k_cells = 0, k_cols = 0, k_calls = 0, k_win = 0;
  int batch_fault = 0;

  // Reads are handed out by atomic counters, READ_RUN consecutive reads at a time (the second to fourth read of a run
  // start without the atomic's round trip, and their records and bases share cache lines with the first: 3.95 ->
  // 3.89 ms).  Small chunks balance the waves
  // (the cost per read varies by orders of magnitude: repeats), but one hot word serves only ~88 M
  // returning atomics per second; so there are EXT_NQ counters on separate cache lines, each over
  // its own contiguous share of the batch, and a wave that finds its counter exhausted moves on to
  // the next one.
  const bool list_only = GS || p.list_only != 0;
  const unsigned n_total = (list_only || p.skip_scan != 0) ? 0u : (unsigned)p.reads.n_reads;
  const unsigned q_share = (n_total + EXT_NQ - 1) / EXT_NQ;
  unsigned my_q = wave_global % EXT_NQ, q_tried = 0;
  // Longest jobs first: reads with many seed hits (repeats; up to a few hundred hits, i.e.
  // milliseconds, against ~50 us for a typical read) are listed by plan_kernel and handed
  // out before everything else, one per wave; left in input order the last ones would start near
  // the end of the batch and the whole grid would wait for them (a quarter of the kernel's time
  // on the benchmark workload).  The any-width kernel works from its list alone.
  bool heavy_phase = true;
  // (see ExtendParamsT::team) the team list is the team kernel's while it is short, else the wave-per-read kernel's
  const unsigned n_team_all = (GS || p.team_count == nullptr) ? 0u : (unsigned)uload(p.team_count);
  const bool team_active = n_team_all <= p.team_limit;
  const unsigned n_heavy_own = TM ? 0u : (unsigned)uload(p.heavy_count);
  const unsigned n_heavy = TM ? (team_active ? n_team_all : 0u) : n_heavy_own + ((!GS && !team_active && !list_only) ? n_team_all : 0u);
  const unsigned list_q = (GS ? EXT_NQ + 1 : EXT_NQ) * EXT_QSTRIDE;
  // (Issuing the atomic for the next read while the current one is worked on was tried: the pending return value
  // stays live across the whole hit loop and costs 400 bytes per lane of spills -- three times slower.)
  unsigned pend_idx = 0, pend_n = 0;  // rest of the run of consecutive reads one queue atomic handed out
  // run length: at most READ_RUN, and short enough that every wave of the grid gets about eight runs (small batches)
  const unsigned read_run = max(1u, min((unsigned)READ_RUN, n_total / (gridDim.x * 4u * 8u)));
  for (;;) {
    bool from_heavy = false, got = false;
    unsigned idx = 0;
    if (!TM && pend_n) {
      idx = pend_idx++;
      pend_n--;
      got = true;
    }
    if constexpr (TM) {
      // one read for the whole workgroup
      if (threadIdx.x == 0) t_ctl[0] = atomicAdd(p.queue + (EXT_NQ + 2) * EXT_QSTRIDE, 1u);
      __syncthreads();
      const unsigned g = t_ctl[0];
      __syncthreads();
      if (g >= n_heavy) break;
      idx = (unsigned)uload(&p.team[g]);
      got = true;
      from_heavy = true;
      heavy_phase = false;
    }
    if (!got && heavy_phase) {
      unsigned g = 0;
      if (lane == 0) g = atomicAdd(p.queue + list_q, 1u);
      g = (unsigned)bcast_first((int)g);
      if (g < n_heavy) {
        idx = (g < n_heavy_own) ? (unsigned)uload(&p.heavy[g]) : (unsigned)uload(&p.team[g - n_heavy_own]);
        got = true;
        from_heavy = true;
      } else {
        heavy_phase = false;
      }
    }
    while (!got && q_tried < EXT_NQ && n_total) {
      unsigned g = 0;
      if (lane == 0) g = atomicAdd(p.queue + my_q * EXT_QSTRIDE, read_run);
      g = (unsigned)bcast_first((int)g);
      const unsigned lo = my_q * q_share, hi = min(lo + q_share, n_total);
      if (lo < hi && g < hi - lo) {
        idx = lo + g;
        pend_idx = idx + 1;
        pend_n = min(read_run - 1u, hi - lo - g - 1u);
        got = true;
        break;
      }
      my_q = (my_q + 1) % EXT_NQ;
      q_tried++;
    }
    if (!got) break;
    // everything needed to start on the read, in one scalar load (launch.h, ReadRecT)
    const ReadRecT<C> rec = uload(&p.read_recs[idx]);
    // not this launch's read: the slow class (and reads beyond every class) are listed by plan_kernel
    if (rec.len > p.max_read_len) continue;
    const uint64_t r0 = rec.base_off;
    const int L = (int)rec.len;
    c.L = L;
    #pragma unroll 1
    for (int t = lane; t < (int)lcap; t += 64) c.rd[t] = (t < L) ? p.reads.bases[r0 + t] : (uint8_t)0;  // already upper-cased and sanitised
    wsync(c);

    // thresholds, reference src/aligner.rs:130-138 (binary32 product, truncation toward zero)
    const float prod = p.opts.min_aln_score_percent * (float)L;
    int ms_pct = (prod != prod) ? 0 : (prod >= 2147483648.0f ? 2147483647 : (prod <= -2147483648.0f ? (-2147483647 - 1) : (int)prod));
    const int min_aln_score = max(ms_pct, p.opts.min_aln_score);
    int max_aln_score = min_aln_score;
    int band_width = (min_aln_score < 0) ? 0 : max(L - min_aln_score, 0);
    int x_drop = band_width;
    const int range = (int)p.opts.multimap_score_range;  // `as i32`: the comparisons (:156, :178)
    // The narrowing (:162-171) takes the untruncated u64 in usize arithmetic.  Band, X-drop and score are at most L <= 65535,
    // so L + r - score >= r: a range of 65535 or more never narrows, and min(range, 2^20) as an int narrows exactly.
    const int narrow = (int)min(p.opts.multimap_score_range, (uint64_t)NARROW_RANGE_MAX);
    const bool intron_mode = p.opts.intron_mode != 0;
    bool band_bad = false;
    if (band_width > (int)p.max_bw || (CPL > 0 && 2 * band_width + 1 > 64 * CPL)) {
      c.fault |= FAULT_BAND;
      band_bad = true;
      band_width = x_drop = 0;
    }

    const uint64_t cand0 = rec.cand_off;
    Cand* cands = p.cands + cand0;
    uint32_t* order = p.order + 2 * cand0;  // two scratch lists of the read's hit count each
    const uint64_t n_hits_cap = rec.n_hits;
    if (!GS && !from_heavy && n_hits_cap >= HEAVY_HITS) continue;  // went out with the heavy reads
#ifdef THM_TIMELINE
    {
      const unsigned long long now = __builtin_amdgcn_s_memrealtime();
      tl_close(now);
      tl_last = now;
      tl_last_hits = (unsigned)min(n_hits_cap, (uint64_t)65535);
      tl_tx = 0;
      tl_reads++;
    }
#endif
    uint32_t n_acc = 0;
    unsigned acc_bytes = 0;  // op bytes and type of the most recent accepted candidate
    int acc_type = 0;

    PROF_MARK(c, PS_SETUP);
    const uint64_t s0 = rec.smem_off;
    uint32_t n_sm = rec.smem_cnt;
    if (cand0 + n_hits_cap > p.cand_cap) {  // candidate pool too small: the host grows it and reruns
      c.fault |= FAULT_OPS_POOL;
      n_sm = 0;
    }
    if (band_bad) n_sm = 0;  // no hit is extended
#ifdef THM_PROF
    c.prof_hit = 0;
#endif
    // ---- team bookkeeping (TEAM > 0; see the comment at the kernel's head) ----
    unsigned t_base = 0, t_total = 0;
    if constexpr (TM) {
      for (uint32_t si = 0; si < n_sm; si++) {  // chunks of the read: every SMEM's occurrences in chunks of TEAM_CHUNK
        const uint64_t cnt = (si == 0) ? (uint64_t)(rec.hi0 - rec.lo0) : (uint64_t)(uload(&p.smems[s0 + si].hi) - uload(&p.smems[s0 + si].lo));
        t_total += (unsigned)((cnt + TEAM_CHUNK - 1) / TEAM_CHUNK);
      }
      if (threadIdx.x == 0) {
        t_state[0] = band_width;
        t_state[1] = x_drop;
        t_state[2] = max_aln_score;
        t_ctl[1] = 0;
        t_ctl[2] = 0;
        t_ctl[3] = 0;
      }
      __syncthreads();
    }
    for (;;) {  // rounds of the team; a single pass otherwise
    unsigned cc = 0;            // chunk counter of the walk
    uint64_t h_start = 0;       // hit ordinal of the chunk's first hit = its first candidate slot
    const unsigned my_chunk = t_base + (unsigned)wave;
    int st_bw = 0, st_xd = 0, st_max = 0;
    unsigned sv_cells = 0, sv_cols = 0, sv_calls = 0, sv_win = 0;
    if constexpr (TM) {
      band_width = t_state[0];
      x_drop = t_state[1];
      max_aln_score = t_state[2];
      st_bw = band_width;
      st_xd = x_drop;
      st_max = max_aln_score;
      n_acc = 0;
      sv_cells = c.cells;
      sv_cols = c.cols;
      sv_calls = c.calls;
      sv_win = c.winbytes;
    }
    for (uint32_t si = 0; si < n_sm; si++) {
      SmemT<C> sm;
      if (si == 0) {  // the first SMEM travels in the read's record
        sm.lo = rec.lo0;
        sm.hi = rec.hi0;
        sm.qpos = rec.qpos0;
        sm.len = rec.len0;
      } else {
        sm = uload(&p.smems[s0 + si]);
      }
      const int q = sm.qpos, len = sm.len;
      C rr = sm.hi;
      if constexpr (TM) {
        // a team works in chunks of TEAM_CHUNK hits (the finer the chunks, the less is redone when a hit moves the
        // state); a wave goes straight to its own chunk of the round
        const uint64_t cnt = (uint64_t)(sm.hi - sm.lo);
        const unsigned n_ch = (unsigned)((cnt + TEAM_CHUNK - 1) / TEAM_CHUNK);
        if (my_chunk < cc || my_chunk >= cc + n_ch) {
          cc += n_ch;
          h_start += cnt;
          continue;
        }
        const unsigned k = my_chunk - cc;
        rr = sm.hi - (C)k * (C)TEAM_CHUNK;
        h_start += (uint64_t)k * TEAM_CHUNK;
        cc = my_chunk;
      }
      while (rr > sm.lo) {
        const uint32_t chunk = (uint32_t)min((C)(TM ? TEAM_CHUNK : 64), (C)(rr - sm.lo));
        if (TM && cc != my_chunk) break;  // the wave's one chunk of this round is done
        Cand* const cslot = TM ? cands + h_start : cands;  // a team's chunk writes its candidates from its first hit's slot
        const uint64_t slot_cap = TM ? (uint64_t)chunk : n_hits_cap;
        C my_sa = 0;
        if (si == 0 && rr == sm.hi && chunk == 1)
          my_sa = rec.sa0;  // ... and so does its first (here: only) occurrence
        else if ((uint32_t)lane < chunk)
          my_sa = ix.sa[rr - 1 - lane];
        for (uint32_t t = 0; t < chunk; t++) {
          const S hr = (S)readlane_c(my_sa, bcast_first((int)t));
          // ================= align_seed_hit (src/aligner.rs:198-314) =================
          const int bw = band_width, xd = x_drop;
          // The genome window is requested before the contig lookup so that the two memory
          // latencies overlap; it is loaded unclamped (the text is padded) and clamped to the
          // contig logically below (:212-215).
          const S gw_a = max(hr - (S)(L + bw), (S)0);
          const S gw_b = min(hr + (S)(len + L + bw), (S)ix.n);
          const unsigned gw_mis = (unsigned)((uintptr_t)(ix.text + gw_a) & 15u);
          const int gw_n = (int)(gw_b - gw_a) + (int)gw_mis;
          const uint4* gw_src = (const uint4*)(ix.text + gw_a - gw_mis);
          uint4 gw_v = make_uint4(0, 0, 0, 0);
          if (gw_n <= c.wcap && lane * 16 < gw_n) gw_v = gw_src[lane];
          const RefInfoT<C> ref = idx_to_ref<C>(ix, (C)hr);
          const C qs = (C)hr, qe = (C)(hr + len);  // the seed on the concatenated text

          // One loop runs the genome extension (target 0) and then one extension per
          // transcript yielded by exon_to_tx.find (:231-258), so that the extension
          // code is instantiated once.
          PathT<S> gx, best;
          gx.score = gx.nops = gx.xstart = gx.xend = 0;
          gx.ystart = gx.yend = 0;
          best = gx;
          bool have_best = false;
          uint32_t best_tx = 0;
          uint8_t* cur_buf = c.pb;
          uint8_t* best_buf = c.pc;
          bool genome_done = false;
          LrMemo gmemo, tmemo;
          GridQueryT<C, ExonEntryT<C>> eg;
          uint32_t best_ent = 0;  // the exon-grid entry the best transcript was reached through
          for (;;) {
            S win0, lo_abs, hi_abs, t_r;
            int t_q, t_len;
            uint8_t* buf;
            uint32_t tx_idx = 0, cur_ent = 0;
            bool by_coords = false;
            if (!genome_done) {
              // genome window (:212-215)
              const S rs = (S)ref.start;
              const S seq_start = max((hr > L + bw) ? hr - (S)(L + bw) : (S)0, rs);
              const S seq_end = min(hr + (S)(len + L + bw), (S)ref.end - 1);
              if (gw_n > c.wcap) {
                c.fault |= FAULT_INTERNAL;
              } else {
                uint4* wdst = (uint4*)c.wing;
                if (lane * 16 < gw_n) wdst[lane] = gw_v;
#pragma unroll 1
                for (int t2 = lane + 64; t2 * 16 < gw_n; t2 += 64) wdst[t2] = gw_src[t2];
              }
              c.winbytes += (unsigned)(seq_end - seq_start);
              wsync(c);
              PROF_MARK(c, PS_STAGE);
              win0 = gw_a - (S)gw_mis;
              lo_abs = seq_start;
              hi_abs = seq_end;
              t_r = hr;
              t_q = q;
              t_len = len;
              buf = c.pa;
            } else {
              // next interval exon_to_tx.find would yield (interval grid, same order)
              uint32_t ent_idx = 0;
              const bool found = grid_next(eg, tx_idx, ent_idx);
              PROF_MARK(c, PS_TREE);
              if (!found) break;
#ifdef THM_TIMELINE
              tl_tx++;
#endif
              cur_ent = ent_idx;
              // the entry carries what is needed of its transcript and exon (thermite_internal.h, ExonEntryT)
              const ExonEntryT<C> ge = uload(&eg.ent[ent_idx]);
              S xs, xe;
              int exon_sum;
              thm_tx tx;
              tx.seq_off = ge.seq_off;
              tx.seq_len = ge.seq_len;
              if (ge.prev_end <= qs) {
                // lift_mem_to_tx (src/txome.rs:82-103), written out: mirrors lift_seed_to_tx (extend_device.h).  This exon is the
                // first of its transcript that intersects the seed
                xs = (S)ge.start;
                xe = (S)ge.end;
                exon_sum = (int)ge.txoff;
              } else {
                // the previous exon reaches into the seed (a seed across a short intron), or the exons of this transcript
                // do not ascend: first exon in transcript order that intersects, by looking at them all
                tx = uload(&ix.txs[tx_idx]);
                int fe = -1;
                for (uint32_t e0 = 0; e0 < tx.n_exons && fe < 0; e0 += 64) {
                  const uint32_t e = e0 + (uint32_t)lane;
                  bool hit = false;
                  if (e < tx.n_exons) {
                    const thm_exon x = ix.exons[tx.exon_begin + e];
                    const C x0 = (C)x.start, x1 = (C)x.end;
                    hit = (qs >= x0 && qs < x1) || (x0 >= qs && x0 < qe);
                  }
                  const unsigned long long m = __ballot(hit);
                  if (m) fe = (int)e0 + __builtin_ctzll(m);
                }
                if (fe < 0) {  // unreachable!() in the reference
                  c.fault |= FAULT_CONTRACT;
                  continue;
                }
                const thm_exon x = uload(&ix.exons[tx.exon_begin + fe]);
                exon_sum = (int)uload(&ix.exon_txoff[tx.exon_begin + fe]);
                xs = (S)x.start;
                xe = (S)x.end;
              }
              int tr_ = (int)((hr > xs) ? hr - xs : (S)0) + exon_sum;
              const int start_offset = (int)((xs > hr) ? xs - hr : (S)0);
              const int t_end = (int)(min(hr + (S)len, xe) - xs) + exon_sum;
              t_q = q + start_offset;
              t_len = t_end - tr_;
              const int tlen = (int)tx.seq_len;
              // The seed lies inside this exon, and so does every base the genome extensions looked at (R.jmax /
              // Lt.jmax columns beyond the seed, results that do not depend on anything further: `broke`): the
              // transcript reads the same bases there (its sequence is assembled from the exons), extend_seed_match
              // finds the same mismatch next to the seed, and the two SwgExtend::extend calls return what they
              // returned for the genome window.  Known from the coordinates alone: no transcript window is staged.
              by_coords = ge.prev_end <= qs && t_q == q && t_len == len && gmemo.R.broke && gmemo.Lt.broke &&
                          hr + (S)(len + gmemo.R.jmax) <= xe && hr - (S)gmemo.Lt.jmax >= xs;
              int w0 = 0;
              // window of the transcript around the lifted seed
              const int ws = (tr_ > L + bw) ? tr_ - (L + bw) : 0;
              const int we = min(tlen, tr_ + t_len + L + bw + 1);
              if (by_coords) c.winbytes += (unsigned)(we - ws);  // THM_CNT_WINDOW_BYTES counts the target's window, staged or not
              if (!by_coords) {
              w0 = stage_window(c, c.win, ix.tx_seq + tx.seq_off, ws, we);
              // extend_seed_match (src/aligner.rs:410-426), written out: mirrors seed_match_wave (extend_device.h)
              {
                int ext = 0;
                for (bool done = false; !done;) {
                  const int tt = ext + lane;
                  const int rp = tr_ + t_len + tt;
                  const int qp = t_q + t_len + tt;
                  const bool ok = (rp < tlen) && (qp < L) && (c.win[rp - w0] == c.rd[qp]);
                  const unsigned long long bad = __ballot(!ok);
                  if (bad) {
                    ext += __builtin_ctzll(bad);
                    done = true;
                  } else {
                    ext += 64;
                  }
                }
                t_len += ext;
                ext = 0;
                for (bool done = false; !done;) {
                  const int tt = ext + lane + 1;
                  const int rp = tr_ - tt;
                  const int qp = t_q - tt;
                  const bool ok = (rp >= 0) && (qp >= 0) && (c.win[rp - w0] == c.rd[qp]);
                  const unsigned long long bad = __ballot(!ok);
                  if (bad) {
                    ext += __builtin_ctzll(bad);
                    done = true;
                  } else {
                    ext += 64;
                  }
                }
                tr_ -= ext;
                t_q -= ext;
                t_len += ext;
              }
              }
              win0 = (S)w0;
              t_r = (S)tr_;
              lo_abs = 0;
              hi_abs = (S)tlen;
              buf = cur_buf;
              PROF_MARK(c, PS_TXPREP);
            }
            PathT<S> pth;
            bool reused = false;
            if (genome_done && by_coords) {
              reused = true;
              pth.score = gx.score;
              pth.nops = gx.nops;
              pth.xstart = gx.xstart;
              pth.xend = gx.xend;
              pth.ystart = t_r - gmemo.Lt.yend;
              pth.yend = t_r + t_len + gmemo.R.yend;
#pragma unroll 1
              for (int t2 = lane; t2 < gx.nops; t2 += 64) buf[t2] = c.pa[t2];
              wsync(c);
              c.calls += 2;  // two extend() calls in the reference's terms
              PROF_MARK(c, PS_TXPREP);
            } else if (genome_done && t_q == q && t_len == len) {
              // Same seed on the read: if the transcript window agrees with the genome
              // window on every column the genome extensions looked at (the hit sits
              // inside one exon and the alignment does not reach its ends), the two
              // SwgExtend::extend calls would return what they returned for the genome.
              const int xr = L - (t_q + t_len);
              const int yr = (int)min(hi_abs - (t_r + t_len), (S)(xr + bw + 1));
              const S rel = t_r - lo_abs;
              const S y0 = lo_abs + (rel > L + bw ? rel - (L + bw) : (S)0);
              const int yl = (int)min(t_r - y0, (S)(t_q + bw + 1));
              const SwgResult& R = gmemo.R;
              const SwgResult& Lt = gmemo.Lt;
              bool ok = (R.broke ? yr >= R.jmax : yr == gmemo.yr) && (Lt.broke ? yl >= Lt.jmax : yl == gmemo.yl);
              if (ok) {
                const uint8_t* tr2 = c.win + (int)(t_r + t_len - win0);
                const uint8_t* gr_ = c.wing + gmemo.yoff_r;
                const uint8_t* tl_ = c.win + (int)(t_r - 1 - win0);
                const uint8_t* gl_ = c.wing + gmemo.yoff_l;
                bool differ = false;
#pragma unroll 1
                for (int j0 = 0; j0 < R.jmax; j0 += 64) {
                  const int j = j0 + lane;
                  differ = differ || (j < R.jmax && tr2[j] != gr_[j]);
                }
#pragma unroll 1
                for (int j0 = 0; j0 < Lt.jmax; j0 += 64) {
                  const int j = j0 + lane;
                  differ = differ || (j < Lt.jmax && tl_[-j] != gl_[-j]);
                }
                ok = __ballot(differ) == 0ull;
              }
              if (ok) {
                reused = true;
                pth.score = gx.score;
                pth.nops = gx.nops;
                pth.xstart = gx.xstart;
                pth.xend = gx.xend;
                pth.ystart = t_r - Lt.yend;
                pth.yend = t_r + t_len + R.yend;
#pragma unroll 1
                for (int t2 = lane; t2 < gx.nops; t2 += 64) buf[t2] = c.pa[t2];
                wsync(c);
                c.calls += 2;  // two extend() calls in the reference's terms
                PROF_MARK(c, PS_TXPREP);
              }
            }
#ifdef THM_PROF
            c.prof_tx = genome_done ? 1 : 0;
#endif
            if (!reused)
              pth = extend_lr<CPL, S>(c, genome_done ? c.win : c.wing, win0, lo_abs, hi_abs, t_r, t_q, t_len, bw, xd, buf,
                                      genome_done ? tmemo : gmemo);
            if (!genome_done) {
              gx = pth;
              genome_done = true;
              // (asking before the genome extension, so that the two round trips run under it, was tried: the query's
              // registers stay live across the DP loops -- 7 % slower)
              grid_begin<C>(eg, ix.exon_grid_off, ix.exon_grid, qs, qe);
            } else {
              if (!have_best || pth.score > best.score) {  // strictly better (:249)
                have_best = true;
                best_tx = tx_idx;
                best_ent = cur_ent;
                best = pth;
                uint8_t* tmp = cur_buf;
                cur_buf = best_buf;
                best_buf = tmp;
              }
              if (pth.score >= L * MATCH_SCORE) break;  // cannot beat an exact match (:253-257)
            }
          }

          // ---- exonic vs unspliced (:263-313) ----
          int aln_type;
          uint32_t type_idx = THM_NO_IDX;
          S cy0, cy1;  // concatenated coordinates of the genome alignment
          const uint8_t* g_path;
          int g_n, g_ny = 0;
          int sc, xs_, xe_;
          const bool exonic = have_best && best.score >= gx.score;
          if (exonic) {
            g_path = best_buf;
            g_n = best.nops;
            aln_type = THM_ALN_EXONIC;
            type_idx = best_tx;
            sc = best.score;
            xs_ = best.xstart;
            xe_ = best.xend;
            cy0 = cy1 = 0;  // set by the lift below, only if the alignment is kept
          } else {
            cy0 = gx.ystart;
            cy1 = gx.yend;
            g_path = c.pa;
            g_n = gx.nops;
            sc = gx.score;
            xs_ = gx.xstart;
            xe_ = gx.xend;
            aln_type = THM_ALN_INTERGENIC;
          }
          // ================= back in align_read's loop (:146-174) =================
          bool accept = intron_mode || exonic;
          if (sc < p.opts.min_aln_score || sc < min_aln_score || sc < max_aln_score - range) accept = false;
          if (accept) {
            uint32_t best_tlen = 0;
            if (exonic) {
              // lift_tx_to_gx (src/txome.rs:110-160).  An alignment that stays inside the exon its seed was lifted through
              // has no intron to insert: its ends move by the exon's offset.  (Ending exactly on the exon's last base
              // still receives the intron when a clip follows, :132-141 -- that case takes the general path.)
              const ExonEntryT<C> ge = uload(&eg.ent[best_ent]);
              best_tlen = ge.seq_len;
              const int ys_ = (int)best.ystart, ye_ = (int)best.yend;
              const int e_lo = (int)ge.txoff, e_hi = e_lo + (int)(ge.end - ge.start);
              const bool inside = ge.prev_end <= qs && ys_ >= e_lo && ys_ < e_hi &&
                                  (ye_ < e_hi || (ye_ == e_hi && (ge.exon_idx + 1 >= ge.n_exons || !(best.xend < L))));
              if (inside) {
                cy0 = (S)ge.start + (S)(ys_ - e_lo);
                cy1 = (S)ge.start + (S)(ye_ - e_lo);
                g_ny = 0;
                PROF_MARK(c, PS_LIFT);
              } else {
                g_ny = lift_markers<S>(c, ix, uload(&ix.txs[best_tx]), best_buf, best.nops, best.xend < L, ys_, ye_, cy0, cy1);
              }
            } else {
              // first interval gene_intervals.find yields (:283-288, :306); only reached in intron mode
              GridQueryT<C, GridEntryT<C>> gg;
              grid_begin<C>(gg, ix.gene_grid_off, ix.gene_grid, (C)cy0, (C)cy1);
              uint32_t gene = 0, gene_ent = 0;
              if (grid_next(gg, gene, gene_ent)) {
                aln_type = THM_ALN_INTRONIC;
                type_idx = gene;
              }
              PROF_MARK(c, PS_TREE);
            }
            const ChrSpanT<C> cs = chr_span<C>(ix, ref, cy0, cy1);  // concat_to_chr_aln (:429-449)
            const RefInfoT<C>& cref = cs.cref;
            const uint64_t ch0 = cs.ch0, ch1 = cs.ch1;
            const bool rev = cs.rev;
            int nb = 0, tnb = 0;
            const unsigned long long off = emit_alignment(c, p, g_path, g_n, xs_, xe_, rev, g_ny, nb);
            unsigned long long toff2 = 0;
            if (exonic) toff2 = emit_alignment(c, p, best_buf, best.nops, best.xstart, best.xend, false, 0, tnb);
            if (n_acc >= slot_cap) {
              c.fault |= FAULT_INTERNAL;
            } else if (lane == 0) {
              Cand cd;
              cd.ystart = ch0;
              cd.yend = ch1;
              cd.ylen = cref.len;
              cd.ops_off = off;
              cd.ops_len = (uint32_t)nb;
              cd.score = sc;
              cd.ref_id = ref.id;
              cd.xstart = (uint32_t)xs_;
              cd.xend = (uint32_t)xe_;
              cd.tx_or_gene_idx = type_idx;
              cd.name_rank = ref.name_rank;
              cd.strand = ref.strand ? 1 : 0;
              cd.aln_type = (uint8_t)aln_type;
              cd.primary = 0;
              cd.pad_ = 0;
              cd.tx_ystart = cd.tx_yend = cd.tx_ylen = 0;
              cd.tx_ops_off = 0;
              cd.tx_ops_len = 0;
              cd.tx_score = 0;
              cd.tx_xstart = cd.tx_xend = 0;
              if (exonic) {
                cd.tx_ystart = (uint64_t)best.ystart;
                cd.tx_yend = (uint64_t)best.yend;
                cd.tx_ylen = best_tlen;
                cd.tx_ops_off = toff2;
                cd.tx_ops_len = (uint32_t)tnb;
                cd.tx_score = best.score;
                cd.tx_xstart = (uint32_t)best.xstart;
                cd.tx_xend = (uint32_t)best.xend;
              }
              cslot[n_acc] = cd;
              if (!GS && !TM && n_acc < (uint32_t)KEYCAP) {
                CandKey k;
                k.ystart = ch0;
                k.yend = ch1;
                k.score = sc;
                k.name_rank = ref.name_rank;
                k.bytes = (uint32_t)(nb + tnb);
                k.strand_type = (ref.strand ? 1u : 0u) | ((uint32_t)aln_type << 8);
                c.ck[n_acc] = k;
              }
            }
            n_acc++;
            acc_bytes = (unsigned)(nb + tnb);
            acc_type = aln_type;
            PROF_MARK(c, PS_EMIT);
            // narrow the band (:162-172)
            const int lim = max(L + narrow - sc, 0);
            band_width = min(band_width, lim);
            x_drop = min(x_drop, lim);
            max_aln_score = max(max_aln_score, sc);
          }
#ifdef THM_PROF
          c.prof_hit++;
#endif
        }
        rr -= chunk;
        h_start += chunk;
        cc++;
      }
    }
    if constexpr (!TM) {
      break;
    } else {
      // ---- end of a round: which chunks are valid? ----
      if (t_total > (unsigned)TEAM_MAX_CHUNKS) c.fault |= FAULT_INTERNAL;  // plan_kernel keeps such reads away from the team
      const bool active = my_chunk < t_total;
      const bool changed = active && (band_width != st_bw || x_drop != st_xd || max_aln_score != st_max);
      if (lane == 0) {
        t_res[wave][0] = active ? (int)n_acc : 0;
        t_res[wave][1] = changed ? 1 : 0;
        t_res[wave][2] = band_width;
        t_res[wave][3] = x_drop;
        t_res[wave][4] = max_aln_score;
        t_res[wave][5] = active ? (c.fault & (FAULT_RETRY | FAULT_CONTRACT)) : 0;  // (FAULT_BAND is set before the rounds, by every wave alike)
      }
      __syncthreads();
      int valid = (int)min((unsigned)TEAM, t_total > t_base ? t_total - t_base : 0u);
      int wstar = -1;
      for (int w2 = 0; w2 < valid; w2++)
        if (t_res[w2][1]) {
          wstar = w2;
          break;
        }
      if (wstar >= 0) valid = wstar + 1;
      c.fault &= ~(FAULT_RETRY | FAULT_CONTRACT);  // per-read outcomes travel through t_ctl[3] (valid chunks only)
      if (wave >= valid) {  // speculation failed (or no chunk): this round's work of the wave does not count
        c.cells = sv_cells;
        c.cols = sv_cols;
        c.calls = sv_calls;
        c.winbytes = sv_win;
      }
      if (threadIdx.x == 0) {
        unsigned acc = 0, fl = 0;
        for (int w2 = 0; w2 < valid; w2++) {
          if (t_base + (unsigned)w2 < (unsigned)TEAM_MAX_CHUNKS) t_nacc[t_base + w2] = (unsigned char)t_res[w2][0];
          acc += (unsigned)t_res[w2][0];
          fl |= (unsigned)t_res[w2][5];
        }
        if (wstar >= 0) {
          t_state[0] = t_res[wstar][2];
          t_state[1] = t_res[wstar][3];
          t_state[2] = t_res[wstar][4];
        }
        t_ctl[1] = t_base + (unsigned)valid;
        t_ctl[2] += acc;
        t_ctl[3] |= fl;
      }
      __syncthreads();
      t_base = t_ctl[1];
      if (t_base >= t_total) break;
    }
    }  // rounds
    // team: the whole workgroup goes through the final section (the two rank sorts are shared out over the waves);
    // everything that has a side effect or keeps the read's books is wave 0's
    const bool lead = !TM || wave == 0;
    if constexpr (TM) {
      n_acc = t_ctl[2];
      max_aln_score = t_state[2];
      c.fault |= (int)t_ctl[3];
    }
    PROF_MARK(c, PS_OTHER);
#ifdef THM_PROF_FINAL
    const unsigned long long tf0 = __builtin_amdgcn_s_memtime();
#endif
    // per-read outcomes that are not alignments
    if (c.fault & FAULT_RETRY) {
      // more introns in one alignment than this kernel's marker list holds: the any-width kernel redoes the read
      c.fault &= ~(FAULT_RETRY | FAULT_CONTRACT);
      if (lead && lane == 0) {
        const unsigned long long slot = atomicAdd(p.retry_count, 1ull);
        p.retry[slot] = idx;
      }
      c.cells = c.cols = c.calls = c.winbytes = 0;
      continue;
    }
    if (c.fault & FAULT_BAND) {
      c.fault &= ~FAULT_BAND;
      n_acc = 0;
      if (lead && lane == 0) {
        p.read_status[idx] = THM_ERR_INTERNAL;
        atomicAdd(p.n_contract, 1ull);  // (tells the host to fetch the statuses)
      }
    }
    if (c.fault & FAULT_CONTRACT) {
      // a condition that panics in the reference (lift_mem_to_tx / lift_tx_to_gx): no alignments, per-read status
      c.fault &= ~FAULT_CONTRACT;
      n_acc = 0;
      if (lead && lane == 0) {
        p.read_status[idx] = THM_ERR_OUT_OF_CONTRACT;
        atomicAdd(p.n_contract, 1ull);
      }
    }
    batch_fault |= c.fault;
#ifdef THM_PROF_FINAL
    const unsigned long long tf1 = __builtin_amdgcn_s_memtime();
#endif
    uint32_t nres = 0;
    unsigned long long opb = 0;
    if (!TM && n_acc == 1 && range >= 0) {
      // the common case: one candidate, which passes retain() (its score is the maximum) unless the range is negative as
      // i32 -- then retain() asks for more than the maximum and keeps nothing (nres stays 0)
      nres = 1;
      if (lane == 0) order[0] = 0;
      opb = acc_bytes;
      k_type[0] += (acc_type == THM_ALN_EXONIC);
      k_type[1] += (acc_type == THM_ALN_INTRONIC);
      k_type[2] += (acc_type == THM_ALN_INTERGENIC);
    } else if (!GS && !TM && n_acc > 1 && n_acc <= (uint32_t)KEYCAP) {
      // ============ retain / filter_overlapping / sort / primary (:177-187), a handful of candidates: lane t holds
      // candidate t's keys; ranks by comparing against every other candidate through readlane, no memory traffic ======
      wsync(c);
      CandKey k;
      k.ystart = k.yend = 0;
      k.score = 0;
      k.name_rank = k.bytes = k.strand_type = 0;
      if ((uint32_t)lane < n_acc) k = c.ck[lane];
      const uint32_t my_strand = k.strand_type & 0xffu;
      // retain(score >= max - range): the survivors keep their order (= lane order)
      const bool keep = (uint32_t)lane < n_acc && k.score >= max_aln_score - range;
      const unsigned long long mk = __ballot(keep);
      const uint32_t m = (uint32_t)__popcll(mk);
      auto rl64 = [](uint64_t v, int l) {
        return ((uint64_t)(unsigned)__builtin_amdgcn_readlane((int)(v >> 32), l) << 32) | (unsigned)__builtin_amdgcn_readlane((int)(v & 0xffffffffu), l);
      };
      int res_ci = 0;  // lane s: index of the s-th surviving candidate of the sweep
      if (m == 1) {
        nres = 1;
        res_ci = (int)__builtin_ctzll(mk);
      } else if (m > 1) {
        // stable sort by (ref_name, strand, ystart) (:322-327): rank among the survivors
        uint32_t r1 = 0;
        for (unsigned long long w = mk; w; w &= w - 1ull) {
          const int u = (int)__builtin_ctzll(w);
          const uint32_t ur = (uint32_t)__builtin_amdgcn_readlane((int)k.name_rank, u);
          const uint32_t us = (uint32_t)__builtin_amdgcn_readlane((int)my_strand, u);
          const uint64_t uy = rl64(k.ystart, u);
          bool less;
          if (ur != k.name_rank)
            less = ur < k.name_rank;
          else if (us != my_strand)
            less = us < my_strand;
          else if (uy != k.ystart)
            less = uy < k.ystart;
          else
            less = u < lane;
          r1 += less ? 1u : 0u;
        }
        // sweep (:329-346)
        uint64_t max_end = 0, l_yend = 0;
        uint32_t l_rank = 0, l_strand = 0;
        int l_score = 0;
        for (uint32_t sidx = 0; sidx < m; sidx++) {
          const int ci = (int)__builtin_ctzll(__ballot(keep && r1 == sidx));
          const uint64_t a_ystart = rl64(k.ystart, ci), a_yend = rl64(k.yend, ci);
          const uint32_t a_rank = (uint32_t)__builtin_amdgcn_readlane((int)k.name_rank, ci);
          const uint32_t a_strand = (uint32_t)__builtin_amdgcn_readlane((int)my_strand, ci);
          const int a_score = __builtin_amdgcn_readlane(k.score, ci);
          if (nres == 0 || a_ystart >= max_end || a_rank != l_rank || a_strand != l_strand) {
            max_end = a_yend;
            if ((uint32_t)lane == nres) res_ci = ci;
            nres++;
            l_rank = a_rank;
            l_strand = a_strand;
            l_score = a_score;
            l_yend = a_yend;
          } else {
            if (a_score > l_score) {
              if ((uint32_t)lane == nres - 1) res_ci = ci;
              l_score = a_score;
              l_yend = a_yend;
            }
            max_end = max(max_end, l_yend);
          }
        }
      }
      // stable sort by -score (:183); order[] is what compact_kernel follows
      const bool mine = (uint32_t)lane < nres;
      const int my_sc = __shfl(k.score, res_ci);
      uint32_t r2 = 0;
      for (uint32_t u = 0; u < nres; u++) {
        const int su = __builtin_amdgcn_readlane(my_sc, (int)u);
        r2 += (su > my_sc || (su == my_sc && (int)u < lane)) ? 1u : 0u;
      }
      if (mine) order[r2] = (uint32_t)res_ci;
      const uint32_t my_bytes = (uint32_t)__shfl((int)k.bytes, res_ci);
      // (the shuffles run with every lane active: ds_bpermute returns 0 for a source lane that is masked off)
      const uint32_t my_st = (uint32_t)__shfl((int)k.strand_type, res_ci);
      const int ty = mine ? (int)(my_st >> 8) : -1;
      unsigned long long ob = mine ? (unsigned long long)my_bytes : 0ull;
      for (int o = 32; o > 0; o >>= 1) ob += __shfl_xor(ob, o);
      opb = ob;
      k_type[0] += (unsigned)__popcll(__ballot(ty == THM_ALN_EXONIC));
      k_type[1] += (unsigned)__popcll(__ballot(ty == THM_ALN_INTRONIC));
      k_type[2] += (unsigned)__popcll(__ballot(ty == THM_ALN_INTERGENIC));
    } else if (TM ? n_acc >= 1 : n_acc > 1) {
      // between the steps: every store visible to every wave that reads it (a workgroup barrier for a team)
      auto step = [&] {
        if constexpr (TM)
          __syncthreads();
        else
          __threadfence_block();
      };
      const uint32_t t0_first = TM ? (uint32_t)wave * 64u : 0u, t0_step = TM ? 64u * (uint32_t)TW : 64u;
      step();
    // ============ retain / filter_overlapping / sort / primary (:177-187) ============
    uint32_t* la = order;               // list A
    uint32_t* lb = order + n_hits_cap;  // list B
    uint32_t m = 0;
    // retain(score >= max - range), keeps order
    if constexpr (TM) {
      // the candidates of chunk cc sit in the slots from its first hit on, t_nacc[cc] of them
      if (lead) {
      unsigned cc2 = 0;
      uint64_t hs = 0;
      for (uint32_t si = 0; si < n_sm; si++) {
        C lo2, hi2;
        if (si == 0) {
          lo2 = rec.lo0;
          hi2 = rec.hi0;
        } else {
          const SmemT<C> sm2 = uload(&p.smems[s0 + si]);
          lo2 = sm2.lo;
          hi2 = sm2.hi;
        }
        C left = hi2 - lo2;
        while (left > 0) {
          const uint32_t chunk = (uint32_t)min((C)TEAM_CHUNK, left);
          const uint32_t na = cc2 < (unsigned)TEAM_MAX_CHUNKS ? (uint32_t)t_nacc[cc2] : 0u;
          const uint32_t slot = (uint32_t)hs + (uint32_t)lane;
          const bool keep = (uint32_t)lane < na && (cands[slot].score >= max_aln_score - range);
          const unsigned long long mk = __ballot(keep);
          if (keep) la[m + __popcll(mk & ((1ull << lane) - 1ull))] = slot;
          m += (uint32_t)__popcll(mk);
          left -= chunk;
          hs += chunk;
          cc2++;
        }
      }
      if (lane == 0) t_ctl[1] = m;
      }
      __syncthreads();
      m = t_ctl[1];
    } else {
    #pragma unroll 1
    for (uint32_t t0 = 0; t0 < n_acc; t0 += 64) {
      const uint32_t t = t0 + lane;
      const bool keep = (t < n_acc) && (cands[t].score >= max_aln_score - range);
      const unsigned long long mk = __ballot(keep);
      if (keep) la[m + __popcll(mk & ((1ull << lane) - 1ull))] = t;
      m += (uint32_t)__popcll(mk);
    }
    }
    step();
    if (m == 1) {
      nres = 1;
    } else if (m > 1) {
      // stable sort by (ref_name, strand, ystart) (:322-327): rank sort la -> lb
      #pragma unroll 1
      for (uint32_t t0 = t0_first; t0 < m; t0 += t0_step) {
        const uint32_t t = t0 + lane;
        if (t < m) {
          const Cand a = cands[la[t]];
          uint32_t rank = 0;
          for (uint32_t u = 0; u < m; u++) {
            const Cand b = cands[la[u]];
            bool less;
            if (b.name_rank != a.name_rank)
              less = b.name_rank < a.name_rank;
            else if (b.strand != a.strand)
              less = b.strand < a.strand;
            else if (b.ystart != a.ystart)
              less = b.ystart < a.ystart;
            else
              less = u < t;
            rank += less ? 1u : 0u;
          }
          lb[rank] = la[t];
        }
      }
      step();
      // sweep (:329-346): result into la
      if (lead) {
      uint64_t max_end = 0;
      uint32_t l_rank = 0, l_strand = 0;
      int l_score = 0;
      uint64_t l_yend = 0;
      for (uint32_t s = 0; s < m; s++) {
        const uint32_t ci = (uint32_t)bcast_first((int)lb[s]);
        const Cand a = cands[ci];
        if (nres == 0 || a.ystart >= max_end || a.name_rank != l_rank || a.strand != l_strand) {
          max_end = a.yend;
          if (lane == 0) la[nres] = ci;
          nres++;
          l_rank = a.name_rank;
          l_strand = a.strand;
          l_score = a.score;
          l_yend = a.yend;
        } else {
          if (a.score > l_score) {
            if (lane == 0) la[nres - 1] = ci;
            l_score = a.score;
            l_yend = a.yend;
          }
          max_end = max(max_end, l_yend);
        }
      }
      if (TM && lane == 0) t_ctl[1] = nres;
      }
      step();
      if constexpr (TM) nres = t_ctl[1];
      // stable sort by -score (:183): rank sort la -> lb, then copy back
      #pragma unroll 1
      for (uint32_t t0 = t0_first; t0 < nres; t0 += t0_step) {
        const uint32_t t = t0 + lane;
        if (t < nres) {
          const int sa_ = cands[la[t]].score;
          uint32_t rank = 0;
          for (uint32_t u = 0; u < nres; u++) {
            const int sb = cands[la[u]].score;
            rank += (sb > sa_ || (sb == sa_ && u < t)) ? 1u : 0u;
          }
          lb[rank] = la[t];
        }
      }
      step();
      #pragma unroll 1
      for (uint32_t t = t0_first + lane; t < nres; t += t0_step) la[t] = lb[t];
      step();
    }
      // per-read totals (a team: wave 0's)
      #pragma unroll 1
      for (uint32_t t0 = 0; lead && t0 < nres; t0 += 64) {
        const uint32_t t = t0 + (uint32_t)lane;
        int ty = -1;
        if (t < nres) {
          const Cand a = cands[la[t]];
          opb += a.ops_len + a.tx_ops_len;
          ty = a.aln_type;
        }
        k_type[0] += (unsigned)__popcll(__ballot(ty == THM_ALN_EXONIC));
        k_type[1] += (unsigned)__popcll(__ballot(ty == THM_ALN_INTRONIC));
        k_type[2] += (unsigned)__popcll(__ballot(ty == THM_ALN_INTERGENIC));
      }
      for (int o = 32; o > 0; o >>= 1) opb += __shfl_xor(opb, o);
    }
#ifdef THM_PROF_FINAL
    const unsigned long long tf2 = __builtin_amdgcn_s_memtime();
#endif
    if (lead && lane == 0) {
      p.read_n_alns[idx] = nres;
      p.read_op_bytes[idx] = opb;
    }
#ifdef THM_PROF_FINAL
    {
      const unsigned long long tf3 = __builtin_amdgcn_s_memtime();
      c.prof_cols[3] += tf1 - tf0;
      c.prof_cols[4] += tf2 - tf1;
      c.prof_cols[5] += tf3 - tf2;
      c.prof_cols[1] += (n_acc > 1) ? 1 : 0;
      c.prof_cols[2] += 1;
    }
#endif
    PROF_MARK(c, PS_FINAL);
    if (lead) {
      k_reads++;
      if (nres)
        k_aligned++;
      else
        k_unmapped++;
      k_alns += nres;
      k_opb += opb;
    }
    k_cells += c.cells;
    k_cols += c.cols;
    k_calls += c.calls;
    k_win += c.winbytes;
    c.cells = c.cols = c.calls = c.winbytes = 0;
    wsync(c);
  }
#ifdef THM_TIMELINE
  if (!TM && !GS && lane == 0 && p.prof && tl_reads) {
    const unsigned long long tl_end = __builtin_amdgcn_s_memrealtime();
    atomicMax(&p.prof[0], ~tl_start);  // earliest start
    atomicMax(&p.prof[1], ~tl_end);    // first wave to leave (the work counters ran dry)
    atomicMax(&p.prof[2], tl_end);     // last wave to leave
    atomicMax(&p.prof[3], (tl_end << 20) | min((tl_end - tl_last) / 100ull, 1048575ull));  // ... and the duration (us) of its last read
    tl_close(tl_end);
    atomicMax(&p.prof[4], tl_longest);  // the longest read: duration << 32 | transcript targets << 16 | hits
    atomicAdd(&p.prof[5], 1ull);
    atomicAdd(&p.prof[6], tl_end - tl_start);
    atomicAdd(&p.prof[7], (unsigned long long)tl_reads);
    if (p.list_only == 0) {
      // waves leaving per 100 us, on the launch's clock (every wave has started by now: prof[0] is final)
      const unsigned long long t0 = ~atomicMax(&p.prof[0], 0ull);
      const unsigned long long rel = (tl_end - t0) / 10000ull;  // 100 us units
      const int b = rel < 30 ? 0 : (int)min(rel - 29ull, 7ull);  // < 3.0 ms, 3.0-3.1, ..., 3.5-3.6, >= 3.6 ms
      atomicAdd(&p.prof[8 + b], 1ull);
    }
  }
#endif
#ifdef THM_PROF
  if (lane == 0 && p.prof)
    {
      for (int t = 0; t < 10; t++) atomicAdd(&p.prof[t], c.prof_acc[t]);
      for (int t = 0; t < 6; t++) atomicAdd(&p.prof[10 + t], c.prof_cols[t]);
    }
#endif
  batch_fault |= c.fault & (FAULT_OPS_POOL | FAULT_INTERNAL);
  if (lane == 0) {
    if (batch_fault) atomicOr(p.fault, batch_fault & (FAULT_OPS_POOL | FAULT_INTERNAL));
    if (k_reads | k_calls | k_cells | k_win) {
      unsigned long long* row = p.wave_counters + (size_t)wave_global * THM_N_COUNTERS;
      row[THM_CNT_READS] = k_reads;
      row[THM_CNT_ALIGNED] = k_aligned;
      row[THM_CNT_UNMAPPED] = k_unmapped;
      row[THM_CNT_ALNS] = k_alns;
      row[THM_CNT_EXONIC] = (unsigned long long)k_type[0];
      row[THM_CNT_INTRONIC] = (unsigned long long)k_type[1];
      row[THM_CNT_INTERGENIC] = (unsigned long long)k_type[2];
      row[THM_CNT_SWG_CALLS] = k_calls;
      row[THM_CNT_DP_CELLS] = k_cells;
      row[THM_CNT_DP_COLS] = k_cols;
      row[THM_CNT_OP_BYTES] = k_opb;
      row[THM_CNT_WINDOW_BYTES] = k_win;
    }
  }
}

}  // namespace dev

constexpr int EXT_MINW_CPL34 = 4;  // default register budget of the three- and four-cell kernels (waves per SIMD)
static int env_in_range(const char* name, int lo, int hi) {  // the knob's value if it is one of lo..hi, else 0 (unset)
  const char* e = getenv(name);
  const int v = e ? atoi(e) : 0;
  return (v >= lo && v <= hi) ? v : 0;
}
static int ext_minw_env() {  // THM_EXT_MINW = 4..8 (0: unset); which of them a kernel has: extend_waves_per_simd
  static const int v = env_in_range("THM_EXT_MINW", 4, 8);
  return v;
}
static int ext_minw_cpl3_env() {  // THM_EXT_MINW_CPL3 = 3 | 4 | 5 | 6 (0: unset)
  static const int v = env_in_range("THM_EXT_MINW_CPL3", 3, 6);
  return v;
}
static int ext_minw_wide_env() {  // THM_EXT_MINW_WIDE = 4 | 5 (0: unset)
  static const int v = env_in_range("THM_EXT_MINW_WIDE", 4, 5);
  return v;
}
// waves per SIMD the wave-per-read kernel chosen for (cpl, coordinate width) is compiled for = workgroups of 4 waves
// that fit a CU; the host launches no more than that (a workgroup beyond it starts when the first ones leave, finds
// the work counters dry and only delays the end of the launch)
int extend_waves_per_simd(int cpl, bool wide) {
  const int minw_env = ext_minw_env();
  if (cpl == 0) return 2;
  if (cpl > 2) {
    // three and four cells per lane (bands beyond +-63: BASELINE config 5's +-64): tuning knob THM_EXT_MINW_CPL3 = 3 | 4 | 5 | 6
    const int v34 = ext_minw_cpl3_env();
    return (v34 && !wide) ? v34 : EXT_MINW_CPL34;
  }
  if (wide) {
    const int wide_env = ext_minw_wide_env();
    return wide_env ? wide_env : 5;
  }
  if (minw_env) {
    if (cpl == 1) return (minw_env == 4 || minw_env == 5 || minw_env == 6) ? minw_env : 8;
    return (minw_env == 4 || minw_env == 5 || minw_env == 8) ? minw_env : 6;
  }
  return cpl == 1 ? 6 : 5;
}

template <class C>
static hipError_t launch_extend_t(const ExtendParamsT<C>& p, int cpl, int n_blocks, hipStream_t s, bool team) {
  const size_t lds4 = cpl == 0 ? 0 : extend_lds_bytes(p.max_read_len, p.max_bw, cpl);
  const size_t lds = team ? lds4 / 4 * TEAM_WAVES : lds4;
  const unsigned threads = team ? 64u * TEAM_WAVES : 256u;
  auto go = [&](auto kern) { return launch_with_lds(kern, n_blocks, threads, lds, s, p); };
  if (team) {
    if (cpl == 1) return go(dev::extend_kernel<C, 1, 4, TEAM_WAVES>);
    if (cpl == 2) return go(dev::extend_kernel<C, 2, 4, TEAM_WAVES>);
    return hipErrorInvalidValue;
  }
  // register budget: MINW waves per SIMD.  Measured on the 32-bit-coordinate kernels (round 2, benchmark workload,
  // same box).  One cell per lane: 3.67 ms at 6 waves against 3.78 at 5, 3.90 at 8 (560 bytes per lane of spills), 3.96
  // at 4 -> 6.  Two cells per lane: 3.89 ms at 6 (80 VGPRs, 136 bytes per lane of spills), 3.96 at 5 (96 VGPRs, 76 bytes),
  // 4.30 at 7, 4.23 at 8, 4.64 at 4; but at 6 waves the spills move 3.2 GB per 500 k-read launch through the memory
  // system (rocprofv3 FETCH_SIZE / WRITE_SIZE) against 1.2 GB at 5 and 0.53 GB of algorithmic bytes: 1 % of throughput
  // for 2.6x less traffic -> 5.  Wider bands run at 4.  Tuning knob THM_EXT_MINW = 4 | 5 | 6 | 8 for the one- and
  // two-cell kernels.  The 64-bit-coordinate kernels (more live state per hit) were at 4 waves per SIMD until the end of
  // round 2: 5 is 8 % faster (4.29 -> 3.95 ms on the benchmark workload with THM_FORCE_WIDE; knob THM_EXT_MINW_WIDE = 4 | 5).
  if (cpl == 0) return go(dev::extend_kernel<C, 0, 2>);
  if constexpr (sizeof(C) == 8) {
    const int minw = extend_waves_per_simd(cpl, true);
    switch (cpl) {
      case 1: return minw == 5 ? go(dev::extend_kernel<C, 1, 5>) : go(dev::extend_kernel<C, 1, 4>);
      case 2: return minw == 5 ? go(dev::extend_kernel<C, 2, 5>) : go(dev::extend_kernel<C, 2, 4>);
      case 3: return go(dev::extend_kernel<C, 3, 4>);
      case 4: return go(dev::extend_kernel<C, 4, 4>);
      default: return hipErrorInvalidValue;
    }
  } else {
    const int minw = extend_waves_per_simd(cpl, false);
    switch (cpl) {
      case 1:
        if (minw == 4) return go(dev::extend_kernel<C, 1, 4>);
        if (minw == 5) return go(dev::extend_kernel<C, 1, 5>);
        if (minw == 6) return go(dev::extend_kernel<C, 1, 6>);
        return go(dev::extend_kernel<C, 1, 8>);
      case 2:
        if (minw == 4) return go(dev::extend_kernel<C, 2, 4>);
        if (minw == 5) return go(dev::extend_kernel<C, 2, 5>);
        if (minw == 8) return go(dev::extend_kernel<C, 2, 8>);
        return go(dev::extend_kernel<C, 2, 6>);
      case 3:
        if (minw == 3) return go(dev::extend_kernel<C, 3, 3>);
        if (minw == 5) return go(dev::extend_kernel<C, 3, 5>);
        if (minw == 6) return go(dev::extend_kernel<C, 3, 6>);
        return go(dev::extend_kernel<C, 3, 4>);
      case 4:
        if (minw == 3) return go(dev::extend_kernel<C, 4, 3>);
        if (minw == 5) return go(dev::extend_kernel<C, 4, 5>);
        if (minw == 6) return go(dev::extend_kernel<C, 4, 6>);
        return go(dev::extend_kernel<C, 4, 4>);
      default: return hipErrorInvalidValue;
    }
  }
}
hipError_t launch_extend(const ExtendParamsT<uint32_t>& p, int cpl, int n_blocks, hipStream_t s, bool team) { return launch_extend_t(p, cpl, n_blocks, s, team); }
hipError_t launch_extend(const ExtendParamsT<uint64_t>& p, int cpl, int n_blocks, hipStream_t s, bool team) { return launch_extend_t(p, cpl, n_blocks, s, team); }

}  // namespace thm
