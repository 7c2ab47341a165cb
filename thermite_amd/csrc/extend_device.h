// extend_device.h -- the wave-level device helpers of the aligner kernels: extend_kernel (kernels_extend.hip, one read
// per wavefront) and seed_hit_kernel (kernels_seed_hit.hip, one caller-chosen hit per wavefront).
//
// Together with the two kernels they restate aligner::align_read (reference src/aligner.rs:123-190) and everything
// below it on the device:
//     align_seed_hit        src/aligner.rs:198-314
//     extend_left_right     src/aligner.rs:352-407   (two SwgExtend::extend calls, swg_device.h)
//     extend_seed_match     src/aligner.rs:410-426
//     concat_to_chr_aln     src/aligner.rs:429-449
//     filter_overlapping    src/aligner.rs:317-349
//     lift_mem_to_tx        src/txome.rs:82-103
//     lift_tx_to_gx         src/txome.rs:110-160
//     Index::idx_to_ref     src/index.rs:287-290
//     Index::seq_slice      src/index.rs:304-323     (a plain slice of the text: both strands are stored)
//     IntervalTree::find    bio 0.37.1, answered from the interval grids in the same yield order
//
// Control flow is wave-uniform and wave-uniform values are kept on the scalar unit (readfirstlane) so that tree nodes,
// exons and transcript records come through the scalar cache and do not occupy vector registers.  Everything here is
// inlined into its caller: each kernel's translation unit gets its own copy, and neither kernel's code depends on the
// other's.  (The FAULT_* bits the helpers set: launch.h.)
#ifndef THERMITE_EXTEND_DEVICE_H
#define THERMITE_EXTEND_DEVICE_H

#include <hip/hip_runtime.h>

#include "launch.h"
#include "swg_device.h"

namespace thm {
namespace dev {

// signed type that holds a text coordinate of width C and small negative offsets from it
template <class C>
struct CoordTraits {
  typedef int S;
};
template <>
struct CoordTraits<uint64_t> {
  typedef long long S;
};
__device__ __forceinline__ uint32_t readlane_c(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }
__device__ __forceinline__ uint64_t readlane_c(uint64_t v, int l) {
  return ((uint64_t)(unsigned)__builtin_amdgcn_readlane((int)(v >> 32), l) << 32) | (unsigned)__builtin_amdgcn_readlane((int)(v & 0xffffffffu), l);
}

__device__ __forceinline__ unsigned long long bcast64(unsigned long long v) {
  return ((unsigned long long)(unsigned)bcast_first((int)(v >> 32)) << 32) | (unsigned)bcast_first((int)(v & 0xffffffffu));
}
__device__ __forceinline__ void wfence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }

template <class C>
struct RefInfoT {
  C start, end, len;  // C = uint32_t (text below 2^31 symbols) keeps this arithmetic on the 32-bit scalar unit
  uint32_t id;
  uint32_t name_rank;
  bool strand;
};
// Index::idx_to_ref: refs.partition_point(|x| x.end_idx <= idx) -- answered in two loads: the contig copy that
// holds the first symbol of idx's bin, then forward over the (rare) boundaries inside the bin
template <class C, class IX>
__device__ RefInfoT<C> idx_to_ref(const IX& ix, C idx) {
  uint32_t lo = uload(&ix.ref_bin[idx >> GRID_SHIFT]);
  RefRecT<C> r = uload(&ix.ref_recs[lo]);
  while (r.end <= idx && lo + 1 < ix.n_refs) {
    lo++;
    r = uload(&ix.ref_recs[lo]);
  }
  RefInfoT<C> o;
  o.start = r.start;
  o.end = r.end;
  o.len = r.len;
  o.id = lo;
  o.name_rank = r.name_rank;
  o.strand = r.strand != 0;
  return o;
}

// (CandKey, KEYCAP: extend_plan.h)

// wave-private buffers: LDS in the register-resident kernels, a slice of global memory in the any-width
// kernel (GS).  Lanes exchange data through them, so every exchange is followed by wsync(): a wavefront-scope
// fence for LDS, a workgroup-scope one (waits for the stores; same-CU L1 is coherent) for global memory.
template <bool GS_>
struct WctxT {
  static constexpr bool GS = GS_;
  uint8_t* rd;   // sanitised read, zero padded
  uint8_t* win;   // window the extension reads (genome or transcript; 16-byte aligned copy)
  uint8_t* wing;  // the hit's genome window, kept while its transcripts are tried
  unsigned long long* trace;    // LDS: trace of a one-cell-per-lane extension (16 bytes per column)
  unsigned long long* trace_g;  // global memory: trace of a wider extension (rare for 91 bp reads; keeps the LDS footprint small)
  uint8_t* pa;  // three path buffers (op kinds 0..3), rotated by pointer swap
  uint8_t* pb;
  uint8_t* pc;
  int* mk_k;      // intron markers of the alignment being emitted: op index they precede ...
  uint32_t* ycl;  // ... and their lengths
  int mk_cap;
  CandKey* ck;    // keys of the first KEYCAP accepted candidates (register-resident kernels only)
  int* dp;        // any-width kernel: column state of swg_extend_tiled (4 arrays of dp_stride ints)
  int dp_stride;
  int L, opcap, wcap;
  unsigned cells, cols, calls, winbytes;
  int fault;
  unsigned long long pool_off;  // wave-private slice of the global op pool (bump allocated)
  unsigned pool_left;
#ifdef THM_PROF
  unsigned long long prof_last;
  unsigned long long prof_acc[10];
  unsigned long long prof_cols[6];
  int prof_hit, prof_tx;  // index of the hit within its read, 1 while a transcript target is extended
#endif
};
template <class W>
__device__ __forceinline__ void wsync(const W&) {
  if (W::GS)
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  else
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}

// Section timing for tuning builds (-DTHM_PROF, libthermite_amd_prof.so): every
// mark charges the shader clocks since the previous mark to one slot.
enum { PS_SETUP = 0, PS_STAGE = 1, PS_DP = 2, PS_TRACEBACK = 3, PS_TREE = 4, PS_TXPREP = 5, PS_LIFT = 6, PS_EMIT = 7,
       PS_FINAL = 8, PS_OTHER = 9 };
#ifdef THM_PROF
#define PROF_MARK(c, slot)                                       \
  do {                                                           \
    const unsigned long long t_ = __builtin_amdgcn_s_memtime();  \
    (c).prof_acc[slot] += t_ - (c).prof_last;                    \
    (c).prof_last = t_;                                          \
  } while (0)
#else
#define PROF_MARK(c, slot) \
  do {                     \
  } while (0)
#endif

// One query of an interval grid (thermite_internal.h): the intervals overlapping
// [qs, qe) come out in IntervalTree::find order, i.e. by ascending pre-order rank.
// Up to 64 candidate entries sit one per lane in registers; larger candidate sets
// (dense loci) are re-read from memory on every step.
template <class C, class E>
struct GridQueryT {
  const E* ent;  // candidates [0, cnt): GridEntryT<C> (genes) or ExonEntryT<C> (exons)
  uint32_t cnt;
  C qs, qe;
  uint32_t b0;
  int last;     // rank of the interval yielded last (-1 before the first)
  int my_rank;  // this lane's candidate: its rank if it overlaps and is the primary copy, else -1
  uint32_t my_val;
};
template <class C, class E>
__device__ __forceinline__ int grid_entry_rank(const E& e, C qs, C qe, uint32_t b0) {
  const bool overlap = qs < e.end && e.start < qe;
  const uint32_t home = max(b0, (uint32_t)(e.start >> GRID_SHIFT));  // first queried bin this interval is listed in
  const bool primary = (e.rank & 0xffu) == (home & 0xffu);
  return (overlap && primary) ? (int)(e.rank >> 8) : -1;
}
template <class C, class E>
__device__ void grid_begin(GridQueryT<C, E>& g, const uint32_t* off, const E* entries, C qs, C qe) {
  const uint32_t b0 = (uint32_t)(qs >> GRID_SHIFT), b1 = (uint32_t)((qe > qs ? qe - 1 : qs) >> GRID_SHIFT);
  const uint32_t e0 = uload(&off[b0]), e1 = uload(&off[b1 + 1]);
  g.ent = entries + e0;
  g.cnt = e1 - e0;
  g.qs = qs;
  g.qe = qe;
  g.b0 = b0;
  g.last = -1;
  g.my_rank = -1;
  g.my_val = 0;
  if (g.cnt <= 64 && (uint32_t)lane_id() < g.cnt) {
    const E* e = &g.ent[lane_id()];
    // the four leading fields only (an exon entry carries more: read by the caller for the one entry that wins)
    struct Head {
      C start, end;
      uint32_t value, rank;
    } h;
    h.start = e->start;
    h.end = e->end;
    h.value = e->value;
    h.rank = e->rank;
    g.my_rank = grid_entry_rank<C>(h, qs, qe, b0);
    g.my_val = h.value;
  }
}
// next overlapping interval in yield order (its value and its index among the candidates); false when exhausted
template <class C, class E>
__device__ bool grid_next(GridQueryT<C, E>& g, uint32_t& value, uint32_t& ent_idx) {
  const int BIG = 0x0fffffff;
  if (g.cnt == 0) return false;
  if (g.cnt <= 64) {
    const int cand = (g.my_rank > g.last) ? g.my_rank : BIG;
    const int best = wave_min(cand);
    if (best == BIG) return false;
    const unsigned long long m = __ballot(g.my_rank == best);
    ent_idx = (uint32_t)__builtin_ctzll(m);
    value = (uint32_t)__builtin_amdgcn_readlane((int)g.my_val, (int)ent_idx);
    g.last = best;
    return true;
  }
  int best = BIG;
  uint32_t bval = 0, bidx = 0;
#pragma unroll 1
  for (uint32_t c0 = 0; c0 < g.cnt; c0 += 64) {
    const uint32_t i = c0 + (uint32_t)lane_id();
    int r = -1;
    uint32_t v = 0;
    if (i < g.cnt) {
      const E* e = &g.ent[i];
      struct Head {
        C start, end;
        uint32_t value, rank;
      } h;
      h.start = e->start;
      h.end = e->end;
      h.value = e->value;
      h.rank = e->rank;
      r = grid_entry_rank<C>(h, g.qs, g.qe, g.b0);
      v = h.value;
    }
    const int cand = (r > g.last) ? r : BIG;
    const int cb = wave_min(cand);
    if (cb < best) {
      best = cb;
      const unsigned long long m = __ballot(cand == cb);
      const int wl = (int)__builtin_ctzll(m);
      bval = (uint32_t)__builtin_amdgcn_readlane((int)v, wl);
      bidx = c0 + (uint32_t)wl;
    }
  }
  if (best == BIG) return false;
  value = bval;
  ent_idx = bidx;
  g.last = best;
  return true;
}

template <class S>
struct PathT {
  int score, xstart, xend, nops;
  S ystart, yend;  // in the coordinates r / lo_abs were given in
};

// what extend_lr did for the hit's genome window, for reuse by its transcripts
struct LrMemo {
  SwgResult R, Lt;
  int nr, nl;
  int yr, yl;    // columns that were available to the right / left extension
  int yoff_r;    // offset in the window buffer of y[0] of the right extension
  int yoff_l;    // offset of y[0] of the left extension (which walks backwards)
};

// One SwgExtend::extend + trace.  The band slots that can ever hold a cell number
// min(2*bw+1, |x|+1): when that fits 64 the one-cell-per-lane code is exact even
// inside a kernel compiled for a wider band (slots >= |x|+1 are never valid), and
// it issues half the instructions per column.  CPL == 0: the any-width kernel (band in
// tiles, everything in global memory).
template <int CPL, class W>
__device__ __forceinline__ int swg_and_trace(W& c, const uint8_t* xs, int dx, int xlen, const uint8_t* ys, int dy, int ylen,
                                             int bw, int xd, uint8_t* ops, int stride, int max_ops, SwgResult& r) {
  int n;
#ifndef THM_NO_SHORTCUT
  if (swg_one_mismatch_shortcut(xs, dx, xlen, ys, dy, ylen, xd, ops, stride, max_ops, r, n)) {
    wsync(c);
    PROF_MARK(c, PS_DP);
    return n;
  }
#endif
  if constexpr (CPL == 0) {
    r = swg_extend_tiled(xs, dx, xlen, ys, dy, ylen, bw, xd, c.trace_g, c.dp, c.dp_stride);
    tiled_sync();
    PROF_MARK(c, PS_DP);
    n = swg_traceback_tiled(c.trace_g, r.xend, r.yend, bw, ops, stride, max_ops);
  } else if (CPL > 1 && min(2 * bw + 1, xlen + 1) <= 64) {
    r = swg_extend_wave<1>(xs, dx, xlen, ys, dy, ylen, bw, xd, c.trace);
    wsync(c);
    PROF_MARK(c, PS_DP);
    n = swg_traceback_wave<1>(c.trace, r.xend, r.yend, bw, ops, stride, max_ops);
  } else if (CPL > 2 && min(2 * bw + 1, xlen + 1) <= 128) {
    // fits two cells per lane: a third fewer instructions per column than the kernel's own width, and the trace stays in
    // LDS (ext_caps: these kernels' LDS trace holds two cells per lane)
    unsigned long long* tr = c.trace;
    r = swg_extend_wave<2>(xs, dx, xlen, ys, dy, ylen, bw, xd, tr);
    wsync(c);
    PROF_MARK(c, PS_DP);
    n = swg_traceback_wave<2>(tr, r.xend, r.yend, bw, ops, stride, max_ops);
  } else {
    // more than 64 band slots: the trace (CPL * 16 bytes per column) goes to the wave's scratch in global
    // memory; the stores of lane 0 must be visible to the loads of all lanes, hence the agent-scope fence
    constexpr int K = CPL > 0 ? CPL : 1;
    unsigned long long* tr = (K > 1) ? c.trace_g : c.trace;
    r = swg_extend_wave<K>(xs, dx, xlen, ys, dy, ylen, bw, xd, tr);
    if (K > 1)
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
    else
      wsync(c);
    PROF_MARK(c, PS_DP);
    n = swg_traceback_wave<K>(tr, r.xend, r.yend, bw, ops, stride, max_ops);
  }
  wsync(c);
  PROF_MARK(c, PS_TRACEBACK);
  return n;
}

// extend_left_right, reference src/aligner.rs:352-407.  `win` holds ref_seq bytes
// from absolute coordinate win0; ref_seq itself spans [lo_abs, hi_abs).
template <int CPL, class S, class W>
__device__ PathT<S> extend_lr(W& c, const uint8_t* win, S win0, S lo_abs, S hi_abs, S r, int q, int len, int bw, int xd,
                              uint8_t* buf, LrMemo& memo) {
  const int L = c.L;
  PathT<S> p;
  PROF_MARK(c, PS_OTHER);
  // right: x = read[q+len..], y = ref_seq[r+len..]   (:360-362)
  const int xr = L - (q + len);
  const S yr_avail = hi_abs - (r + len);
  const int yr = (int)min(yr_avail, (S)(xr + bw + 1));
  SwgResult R, Lt;
  int nr = swg_and_trace<CPL>(c, c.rd + q + len, 1, xr, win + (int)(r + len - win0), 1, yr, bw, xd, buf + c.opcap - 1, -1,
                              c.opcap, R);
  // left: both reversed, y = ref_seq[r.saturating_sub(L+bw)..r]   (:364-375)
  const int xl = q;
  const S rel = r - lo_abs;
  const S y0 = lo_abs + (rel > L + bw ? rel - (L + bw) : (S)0);
  const int yl = (int)min(r - y0, (S)(xl + bw + 1));
  int nl = swg_and_trace<CPL>(c, c.rd + q - 1, -1, xl, win + (int)(r - 1 - win0), -1, yl, bw, xd, buf, 1,
                              c.opcap - max(nr, 0), Lt);
  c.cells += R.cells + Lt.cells;
  c.cols += R.cols + Lt.cols;
  c.calls += 2;
#ifdef THM_PROF
  {  // how much of the DP runs on at most 32 band slots (two such problems could share a wave)
    const bool nr_ = min(2 * bw + 1, xr + 1) <= 32, nl_ = min(2 * bw + 1, xl + 1) <= 32;
    c.prof_cols[0] += R.cols + Lt.cols;
    c.prof_cols[1] += (nr_ ? R.cols : 0) + (nl_ ? Lt.cols : 0);
    c.prof_cols[2] += (nr_ && nl_) ? min(R.cols, Lt.cols) : 0;
    c.prof_cols[3] += (c.prof_hit == 0) ? R.cols + Lt.cols : 0;
    c.prof_cols[4] += c.prof_tx ? R.cols + Lt.cols : 0;
    // extensions of the shape "one mismatch, then exact to the end of x" (their result is known without DP)
    {
      const uint8_t* yR = win + (int)(r + len - win0);
      const uint8_t* yL = win + (int)(r - 1 - win0);
      bool dr = false, dl = false;
      for (int t0 = 1; t0 < xr; t0 += 64) {
        const int t = t0 + lane_id();
        dr = dr || (t < xr && (t >= yr || c.rd[q + len + t] != yR[t]));
      }
      for (int t0 = 1; t0 < xl; t0 += 64) {
        const int t = t0 + lane_id();
        dl = dl || (t < xl && (t >= yl || c.rd[q - 1 - t] != yL[-t]));
      }
      const bool m1r = xr >= 3 && yr >= xr && __ballot(dr) == 0ull, m1l = xl >= 3 && yl >= xl && __ballot(dl) == 0ull;
      c.prof_cols[5] += (m1r ? R.cols : 0) + (m1l ? Lt.cols : 0);
    }
  }
#endif
  if (nr < 0 || nl < 0 || nl + len + nr > c.opcap) {
    c.fault |= FAULT_INTERNAL;
    nl = 0;
    nr = 0;
  }
  const int lane = lane_id();
  // rev(left.ops) ++ Match x len ++ right.ops   (:388-394); the clips are implied by xstart / xend
  #pragma unroll 1
  for (int t = lane; t < len; t += 64) buf[nl + t] = OPK_MATCH;
  #pragma unroll 1
  for (int t0 = 0; t0 < nr; t0 += 64) {
    const int t = t0 + lane;
    uint8_t v = 0;
    if (t < nr) v = buf[c.opcap - nr + t];
    wsync(c);
    if (t < nr) buf[nl + len + t] = v;
    wsync(c);
  }
  PROF_MARK(c, PS_TRACEBACK);
  memo.R = R;
  memo.Lt = Lt;
  memo.nr = nr;
  memo.nl = nl;
  memo.yr = yr;
  memo.yl = yl;
  memo.yoff_r = (int)(r + len - win0);
  memo.yoff_l = (int)(r - 1 - win0);
  p.nops = nl + len + nr;
  p.score = Lt.score + len * MATCH_SCORE + R.score;
  p.ystart = r - Lt.yend;
  p.yend = r + len + R.yend;
  p.xstart = q - Lt.xend;
  p.xend = q + len + R.xend;
  return p;
}

// Stage [a, b) of a global byte array into c.win with 16-byte loads.  Returns the
// coordinate that c.win[0] corresponds to (a rounded down to the 16-byte grid of
// the source address; the arrays carry 16 bytes of padding at both ends of use).
template <class W>
__device__ int stage_window(W& c, uint8_t* dst, const uint8_t* src, int a, int b) {
  const unsigned mis = (unsigned)((uintptr_t)(src + a) & 15u);
  const int n = (b - a) + (int)mis;
  if (n > c.wcap) {
    c.fault |= FAULT_INTERNAL;
    return a;
  }
  const uint4* g = (const uint4*)(src + a - mis);
  uint4* w = (uint4*)dst;
  for (int t = lane_id(); t * 16 < n; t += 64) w[t] = g[t];
  c.winbytes += (unsigned)(b - a);
  wsync(c);
  PROF_MARK(c, PS_STAGE);
  return a - (int)mis;
}

// lift_tx_to_gx, reference src/txome.rs:110-160, without materialising the lifted
// list: returns the introns as markers (c.mk_k[m] = index of the path op the
// Yclip precedes, nops = "after the last op"; c.ycl[m] = its length) and the
// lifted start / end.  A Yclip is pushed before the first op at which the
// transcript position has reached an exon end (:133-141); the reference's op list
// includes a trailing Xclip when the read is clipped on the right, which gets its
// own loop iteration -- so an alignment that ends exactly on an exon boundary
// still receives the intron (the edge case noted at src/txome.rs:132).
template <class S, class W, class IX>
__device__ int lift_markers(W& c, const IX& ix, const thm_tx& tx, const uint8_t* path, int n, bool trailing_clip,
                            int ystart, int yend, S& gx_ystart, S& gx_yend) {
  const thm_exon* ex = ix.exons + tx.exon_begin;
  const uint64_t* toff = ix.exon_txoff + tx.exon_begin;
  const int ne = (int)tx.n_exons;
  const int lane = lane_id();
  // exon where the alignment starts: while exon_sum + len <= i  (:123-126)
  int lo = 0, hi = ne;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const thm_exon xm = uload(&ex[mid]);
    if ((int)(uload(&toff[mid]) + (xm.end - xm.start)) <= ystart)
      lo = mid + 1;
    else
      hi = mid;
  }
  int e = lo;
  if (e >= ne) {  // index panic in the reference
    c.fault |= FAULT_CONTRACT;
    gx_ystart = gx_yend = 0;
    return 0;
  }
  thm_exon cur = uload(&ex[e]);
  int exon_sum = (int)uload(&toff[e]);
  gx_ystart = (S)cur.start + (S)(ystart - exon_sum);
  // transcript positions advance on Match / Subst / Del; total must equal yend - ystart (:154)
  int n_adv = 0;
  #pragma unroll 1
  for (int k0 = 0; k0 < n; k0 += 64) {
    const int k = k0 + lane;
    const uint8_t op = (k < n) ? path[k] : (uint8_t)OPK_INS;
    n_adv += __popcll(__ballot(op != OPK_INS));
  }
  if (n_adv != yend - ystart) c.fault |= FAULT_CONTRACT;
  int n_y = 0;
  for (;;) {
    const int bnd = exon_sum + (int)(cur.end - cur.start);  // transcript offset of this exon's end
    if (e + 1 >= ne || bnd > yend) break;
    // index of the op that follows the advancing op which brings the position to bnd
    const int need = bnd - ystart;  // 1-based rank among advancing ops
    int kstar = -1, seen = 0;
    for (int k0 = 0; k0 < n && kstar < 0; k0 += 64) {
      const int k = k0 + lane;
      const uint8_t op = (k < n) ? path[k] : (uint8_t)OPK_INS;
      const unsigned long long m = __ballot(op != OPK_INS);
      const int cnt = __popcll(m);
      if (seen + cnt >= need) {
        const int rank = need - seen;  // rank within this chunk, >= 1
        const unsigned long long le = (lane == 63) ? ~0ull : ((2ull << lane) - 1ull);
        const bool mine = ((m >> lane) & 1ull) && ((int)__popcll(m & le) == rank);
        const unsigned long long sel = __ballot(mine);
        kstar = k0 + __builtin_ctzll(sel) + 1;
      }
      seen += cnt;
    }
    if (kstar < 0) break;                        // cannot happen when n_adv is consistent
    if (kstar >= n && !trailing_clip) break;     // boundary reached by the very last op: no further iteration
    if (n_y >= c.mk_cap) {
      // more introns than the marker list holds: the any-width kernel (list sized by the longest transcript) takes the read
      c.fault |= W::GS ? FAULT_INTERNAL : FAULT_RETRY;
      break;
    }
    const thm_exon nxt = uload(&ex[e + 1]);
    if (lane == 0) {
      c.mk_k[n_y] = kstar;
      c.ycl[n_y] = (uint32_t)(nxt.start - cur.end);
    }
    n_y++;
    exon_sum = bnd;
    cur = nxt;
    e++;
  }
  gx_yend = (S)cur.start + (S)(yend - exon_sum);
  wsync(c);
  PROF_MARK(c, PS_LIFT);
  return n_y;
}

// Serialise [Xclip(xstart)] path-with-introns [Xclip(L-xend)] straight into the
// global op pool, every lane writing its own bytes; `reverse` mirrors the whole
// list (concat_to_chr_aln on a reverse-strand Ref, src/aligner.rs:440-447).
// Returns the pool offset, byte count in n_bytes.
template <class W, class PP>
__device__ unsigned long long emit_alignment(W& c, const PP& p, const uint8_t* path, int n, int xstart, int xend,
                                             bool reverse, int n_y, int& n_bytes) {
  const int lane = lane_id();
  const int lead = xstart, trail = c.L - xend;
  const int lead5 = lead > 0 ? 5 : 0, trail5 = trail > 0 ? 5 : 0;
  const int total = lead5 + n + 5 * n_y + trail5;
  n_bytes = total;
  // the op pool is handed out to waves in 4 KiB slices (one atomic per slice, not per alignment)
  if ((unsigned)total > c.pool_left) {
    const unsigned grab = max(4096u, (unsigned)total);
    unsigned long long g = 0;
    if (lane == 0) g = atomicAdd(p.ops_cursor, (unsigned long long)grab);
    g = bcast64(g);
    if (g + grab > p.cand_ops_cap) {
      // pool exhausted: the host grows it and replays the batch; this attempt must not leave byte
      // counts behind that exceed what was allocated (the scans and compact_kernel still run)
      c.fault |= FAULT_OPS_POOL;
      c.pool_left = 0;
      n_bytes = 0;
      return 0;
    }
    c.pool_off = g;
    c.pool_left = grab;
  }
  const unsigned long long off = c.pool_off;
  c.pool_off += (unsigned)total;
  c.pool_left -= (unsigned)total;
  uint8_t* o = p.cand_ops + off;
  auto put5 = [&](int pos, uint8_t kind, uint32_t v) {
    o[pos] = kind;
    o[pos + 1] = (uint8_t)v;
    o[pos + 2] = (uint8_t)(v >> 8);
    o[pos + 3] = (uint8_t)(v >> 16);
    o[pos + 4] = (uint8_t)(v >> 24);
  };
  // forward byte position of an element; the reversed position is total - (pos + size)
  #pragma unroll 1
  for (int k0 = 0; k0 < n; k0 += 64) {
    const int k = k0 + lane;
    if (k < n) {
      int before = 0;
      for (int m = 0; m < n_y; m++) before += (c.mk_k[m] <= k) ? 1 : 0;
      const int pos = lead5 + k + 5 * before;
      o[reverse ? total - (pos + 1) : pos] = path[k];
    }
  }
  #pragma unroll 1
  for (int m = lane; m < n_y; m += 64) {
    const int pos = lead5 + c.mk_k[m] + 5 * m;
    put5(reverse ? total - (pos + 5) : pos, THM_OP_YCLIP, c.ycl[m]);
  }
  if (lane == 0 && lead > 0) put5(reverse ? total - 5 : 0, THM_OP_XCLIP, (uint32_t)lead);
  if (lane == 1 && trail > 0) put5(reverse ? 0 : total - 5, THM_OP_XCLIP, (uint32_t)trail);
  return off;
}

// ---- the steps of align_seed_hit that extend_kernel and seed_hit_kernel take alike, written once ----

// The wave-private buffers of wave `wave` of its workgroup (`wave_global` of the grid): a carve of LDS for the
// register-resident kernels (it must match extend_lds_bytes), slow_layout in global memory for the any-width kernel
// (CPL == 0).  keys: the kernel keeps candidate keys (their LDS is part of the carve either way).
template <int CPL, class W, class P>
__device__ __forceinline__ void carve_wave(W& c, const P& p, const ExtCaps& caps, uint8_t* smem, int wave, unsigned wave_global,
                                           bool keys) {
  const uint32_t lcap = caps.lcap, wcap = caps.wcap, opcap = caps.opcap;
  if constexpr (W::GS) {
    const SlowLayout sl = slow_layout(p.max_read_len, p.max_bw, p.mk_cap);
    uint8_t* base = p.slow_scratch + (size_t)wave_global * p.slow_scratch_per_wave;
    c.rd = base + sl.rd;
    c.win = base + sl.win;
    c.wing = base + sl.wing;
    c.trace = nullptr;
    c.trace_g = (unsigned long long*)(base + sl.trace);
    c.pa = base + sl.pa;
    c.pb = base + sl.pb;
    c.pc = base + sl.pc;
    c.mk_k = (int*)(base + sl.mk_k);
    c.ycl = (uint32_t*)(base + sl.ycl);
    c.dp = (int*)(base + sl.dp);
    c.dp_stride = (int)sl.dp_stride;
    c.mk_cap = (int)p.mk_cap;
    c.ck = nullptr;
  } else {
    const uint32_t per_wave = lcap + 2u * wcap + caps.trb + 3u * opcap + 8u * FAST_MAX_YCLIPS + (uint32_t)(KEYCAP * sizeof(CandKey));
    uint8_t* base = smem + (size_t)wave * per_wave;
    c.rd = base;
    c.win = c.rd + lcap;
    c.wing = c.win + wcap;
    c.trace = (unsigned long long*)(c.wing + wcap);
    c.trace_g = p.trace_scratch + (size_t)wave_global * ((size_t)(caps.ycols + 1u) * (CPL > 0 ? CPL : 1) * 2u);
    c.pa = (uint8_t*)c.trace + caps.trb;
    c.pb = c.pa + opcap;
    c.pc = c.pb + opcap;
    c.mk_k = (int*)(c.pc + opcap);
    c.ycl = (uint32_t*)(c.mk_k + FAST_MAX_YCLIPS);
    c.ck = keys ? (CandKey*)(c.ycl + FAST_MAX_YCLIPS) : nullptr;
    c.dp = nullptr;
    c.dp_stride = 0;
    c.mk_cap = FAST_MAX_YCLIPS;
  }
  c.opcap = (int)opcap;
  c.wcap = (int)wcap;
  c.cells = c.cols = c.calls = c.winbytes = 0;
  c.fault = 0;
  c.pool_off = 0;
  c.pool_left = 0;
}

// lift_mem_to_tx (src/txome.rs:82-103) for the seed [qs, qe) = [hr, hr + len) at read position q and the transcript
// tx_idx that the exon-grid entry `ge` was yielded for: the seed in transcript coordinates, the exon [xs, xe) it was
// lifted through and where the transcript's sequence lies.  ok = false: no exon of the transcript intersects the seed
// (unreachable!() in the reference; FAULT_CONTRACT is set).
template <class S>
struct TxSeedT {
  S xs, xe;
  int t_r, t_q, t_len;
  uint64_t seq_off, seq_len;
  bool ok;
};
template <class S, class C, class W, class IX>
__device__ __forceinline__ TxSeedT<S> lift_seed_to_tx(W& c, const IX& ix, const ExonEntryT<C>& ge, uint32_t tx_idx, C qs, C qe, S hr,
                                                      int q, int len) {
  TxSeedT<S> o;
  int exon_sum;
  o.seq_off = ge.seq_off;
  o.seq_len = ge.seq_len;
  o.ok = true;
  if (ge.prev_end <= qs) {
    // this exon is the first of its transcript that intersects the seed
    o.xs = (S)ge.start;
    o.xe = (S)ge.end;
    exon_sum = (int)ge.txoff;
  } else {
    // the previous exon reaches into the seed (a seed across a short intron), or the exons of this transcript
    // do not ascend: first exon in transcript order that intersects, by looking at them all
    const thm_tx tx = uload(&ix.txs[tx_idx]);
    o.seq_off = tx.seq_off;
    o.seq_len = tx.seq_len;
    int fe = -1;
    for (uint32_t e0 = 0; e0 < tx.n_exons && fe < 0; e0 += 64) {
      const uint32_t e = e0 + (uint32_t)lane_id();
      bool hit = false;
      if (e < tx.n_exons) {
        const thm_exon x = ix.exons[tx.exon_begin + e];
        const C x0 = (C)x.start, x1 = (C)x.end;
        hit = (qs >= x0 && qs < x1) || (x0 >= qs && x0 < qe);
      }
      const unsigned long long m = __ballot(hit);
      if (m) fe = (int)e0 + __builtin_ctzll(m);
    }
    if (fe < 0) {
      c.fault |= FAULT_CONTRACT;
      o.ok = false;
      o.xs = o.xe = 0;
      o.t_r = o.t_q = o.t_len = 0;
      return o;
    }
    const thm_exon x = uload(&ix.exons[tx.exon_begin + fe]);
    exon_sum = (int)uload(&ix.exon_txoff[tx.exon_begin + fe]);
    o.xs = (S)x.start;
    o.xe = (S)x.end;
  }
  o.t_r = (int)((hr > o.xs) ? hr - o.xs : (S)0) + exon_sum;
  const int start_offset = (int)((o.xs > hr) ? o.xs - hr : (S)0);
  const int t_end = (int)(min(hr + (S)len, o.xe) - o.xs) + exon_sum;
  o.t_q = q + start_offset;
  o.t_len = t_end - o.t_r;
  return o;
}

// extend_seed_match (src/aligner.rs:410-426) on the transcript window staged in c.win (c.win[0] = transcript
// position w0, the transcript is tlen long): ballots of the first mismatch to the right, then to the left
struct SeedMatch {
  int t_r, t_q, t_len;
};
template <class W>
__device__ __forceinline__ SeedMatch seed_match_wave(const W& c, int w0, int tlen, int t_r, int t_q, int t_len) {
  const int lane = lane_id();
  int ext = 0;
  for (bool done = false; !done;) {
    const int tt = ext + lane;
    const int rp = t_r + t_len + tt;
    const int qp = t_q + t_len + tt;
    const bool ok = (rp < tlen) && (qp < c.L) && (c.win[rp - w0] == c.rd[qp]);
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
    const int rp = t_r - tt;
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
  SeedMatch o;
  o.t_r = t_r - ext;
  o.t_q = t_q - ext;
  o.t_len = t_len + ext;
  return o;
}

// concat_to_chr_aln (src/aligner.rs:429-449) for the alignment [cy0, cy1) on the concatenated text.
// Index::idx_to_ref(ystart): the alignment starts inside the contig copy of its hit (`ref`: the genome window is
// clamped to it, a transcript's exons lie on one copy), so the lookup is the hit's own; anything else goes through
// the search.  rev: the op list is mirrored (a reverse-strand copy).
template <class C>
struct ChrSpanT {
  RefInfoT<C> cref;
  uint64_t ch0, ch1;
  bool rev;
};
template <class C, class S, class IX>
__device__ __forceinline__ ChrSpanT<C> chr_span(const IX& ix, const RefInfoT<C>& ref, S cy0, S cy1) {
  ChrSpanT<C> o;
  o.cref = ((C)cy0 >= ref.start && (C)cy0 < ref.end) ? ref : idx_to_ref<C>(ix, (C)cy0);
  if (o.cref.strand) {
    o.ch0 = (uint64_t)((C)cy0 - o.cref.start);
    o.ch1 = (uint64_t)((C)cy1 - o.cref.start);
    o.rev = false;
  } else {
    o.ch0 = (uint64_t)(C)(o.cref.len - ((C)cy1 - o.cref.start));
    o.ch1 = (uint64_t)(C)(o.cref.len - ((C)cy0 - o.cref.start));
    o.rev = true;
  }
  return o;
}

}  // namespace dev
}  // namespace thm

#endif  // THERMITE_EXTEND_DEVICE_H
