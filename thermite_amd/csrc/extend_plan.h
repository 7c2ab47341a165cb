// extend_plan.h -- the geometry of the extend stage, stated once: the per-wave buffer sizes the kernels carve up, the
// length classes of a batch, and the plan of one run's launches (grids, scratch slices, the waves' counter rows).
//
// Plain C++17: no HIP runtime header, so that a host program can evaluate the plan (tests/cpp/extend_plan_main.cpp).
// Under hipcc the buffer-size functions are __host__ __device__, and the kernels of kernels_extend.hip and kernels_seed_hit.hip call the same
// inline functions as the host's sizing.
#ifndef THERMITE_EXTEND_PLAN_H
#define THERMITE_EXTEND_PLAN_H
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "thermite_internal.h"

#if defined(__HIPCC__)
#define EXT_HD __host__ __device__ inline
#else
#define EXT_HD inline
#endif

namespace thm {

constexpr int TEAM_WAVES = 16;
// intron markers one alignment can carry in the register-resident kernel (LDS); an alignment across more
// introns sends its read to the any-width kernel, whose marker list is sized by the longest transcript
constexpr int FAST_MAX_YCLIPS = 64;
constexpr size_t EXTEND_LDS_LIMIT = 160 * 1024;  // gfx950: one workgroup may take the whole LDS of its CU
// does a team workgroup (TEAM_WAVES waves' buffers + the team's own static LDS: per-chunk book, round results) fit?
// lds4 = extend_lds_bytes(...) of an ordinary 4-wave workgroup
constexpr size_t TEAM_STATIC_LDS = 16384 + TEAM_WAVES * 32 + 64;  // t_nacc[TEAM_MAX_CHUNKS], t_res, t_state, t_ctl (kernels_extend.hip)
inline bool team_fits_lds(size_t lds4) { return lds4 / 4 * TEAM_WAVES + TEAM_STATIC_LDS + 256 <= EXTEND_LDS_LIMIT; }
constexpr int FINISH_BLOCKS_PER_CU = 8;  // the finisher strides over the batch with at most this many workgroups per CU
constexpr int DPT_SLOTS = 16;            // band slots of the thread-per-problem DP kernel (registers of one thread)
// Reads with this many seed hits and more stay with the workgroup-per-read / wave-per-read kernels: the control kernel
// replays a read's hits in one thread, and a thread with thousands of hits would be the tail of its launch.
constexpr unsigned TPR_MAX_HITS = 32;
constexpr int TPR_CTL_BLOCKS_PER_CU = 4, TPR_DP_BLOCKS_PER_CU = 8;
// device memory the any-width kernel may take for its wave-private buffers (traces grow with length x band)
constexpr uint64_t SLOW_SCRATCH_BUDGET = 24ull << 30;

// band slots per lane of a wavefront that holds a band of +-bw (1 for bw = 0)
constexpr int cells_per_lane(uint32_t bw) { return (int)((2 * bw + 1 + 63) / 64); }

namespace dev {

// What retain / filter_overlapping / the final sort (src/aligner.rs:177-187) look at, per accepted candidate: kept in
// LDS for the first KEYCAP candidates of a read, so that the usual multi-candidate read (a handful) is finished
// from registers without going back to the candidate array in global memory.
struct CandKey {
  uint64_t ystart, yend;
  int32_t score;
  uint32_t name_rank;
  uint32_t bytes;        // serialised op bytes (genome + transcript streams)
  uint32_t strand_type;  // strand | aln_type << 8
};
static_assert(sizeof(CandKey) == 32, "CandKey layout");
constexpr int KEYCAP = 16;

// per-wave buffer sizes, shared by the kernel's carve-up and the host's sizing functions
struct ExtCaps {
  uint32_t lcap, wcap, ycols, trb, opcap;
};
// cpl: cells per lane of the kernel's widest band (0: the any-width kernel)
EXT_HD ExtCaps ext_caps(uint32_t max_read_len, uint32_t max_bw, int cpl = 1) {
  ExtCaps k;
  k.lcap = (max_read_len + 31u) & ~15u;
  k.wcap = (2u * (max_read_len + max_bw) + max_read_len + 48u) & ~15u;
  k.ycols = max_read_len + max_bw + 2u;
  // LDS trace: one cell per lane (16 bytes per column).  The kernels for bands beyond 128 slots (three and four cells per
  // lane: 150 bp reads with a band of +-64) keep room for two cells per lane: most of their extensions have 65..128 slots
  // (min(2 bw + 1, |x| + 1)), and a trace in global memory -- a store per column, an agent-scope fence, a traceback of
  // dependent global loads -- is what such a launch was spending its time on.  Wider extensions still use trace_g.
  k.trb = (k.ycols + 1u) * (cpl >= 3 ? 32u : 16u);
  k.opcap = (2u * max_read_len + 2u * max_bw + 31u) & ~15u;
  return k;
}
// any-width kernel: layout of one wave's slice of global memory
struct SlowLayout {
  uint64_t rd, win, wing, pa, pb, pc, mk_k, ycl, dp, trace, total;
  uint32_t dp_stride;
};
EXT_HD SlowLayout slow_layout(uint32_t max_read_len, uint32_t max_bw, uint32_t mk_cap) {
  const ExtCaps k = ext_caps(max_read_len, max_bw);
  SlowLayout s;
  uint64_t o = 0;
  auto take = [&](uint64_t bytes) {
    const uint64_t at = o;
    o += (bytes + 63u) & ~63ull;
    return at;
  };
  s.rd = take(k.lcap);
  s.win = take(k.wcap);
  s.wing = take(k.wcap);
  s.pa = take(k.opcap);
  s.pb = take(k.opcap);
  s.pc = take(k.opcap);
  s.mk_k = take((uint64_t)mk_cap * 4);
  s.ycl = take((uint64_t)mk_cap * 4);
  const uint32_t tiles = (2u * max_bw + 1u + 63u) / 64u;
  s.dp_stride = tiles * 64u + 64u;
  s.dp = take((uint64_t)s.dp_stride * 4u * 4u);
  s.trace = take((uint64_t)(k.ycols + 1u) * tiles * 16u);
  s.total = o;
  return s;
}

}  // namespace dev

// LDS of a 4-wave workgroup of the register-resident kernels (the carve of extend_kernel)
inline size_t extend_lds_bytes(uint32_t max_read_len, uint32_t max_bw, int cpl) {
  const dev::ExtCaps k = dev::ext_caps(max_read_len, max_bw, cpl);
  const uint32_t per_wave = k.lcap + 2u * k.wcap + k.trb + 3u * k.opcap + 8u * FAST_MAX_YCLIPS + (uint32_t)(dev::KEYCAP * sizeof(dev::CandKey));
  return 4 * (size_t)per_wave;
}
// global trace scratch of one wave (extensions over more than 64 band slots), in bytes
inline size_t extend_trace_scratch_bytes(uint32_t max_read_len, uint32_t max_bw, int cpl) {
  return cpl > 1 ? (size_t)(max_read_len + max_bw + 3u) * (size_t)cpl * 16u : 0;
}
// everything one wave of the any-width kernel keeps in global memory, in bytes
inline size_t extend_slow_scratch_bytes(uint32_t max_read_len, uint32_t max_bw, uint32_t mk_cap) {
  return (size_t)dev::slow_layout(max_read_len, max_bw, mk_cap).total;
}
// workgroups for n_items at waves_per_block items each, no more than blocks_per_cu per CU, at least one
inline int grid_blocks(int n_cu, uint64_t n_items, int waves_per_block, int blocks_per_cu) {
  const uint64_t need = (n_items + waves_per_block - 1) / waves_per_block;
  const uint64_t cap = (uint64_t)n_cu * blocks_per_cu;
  return (int)std::max<uint64_t>(1, std::min(need, cap));
}
// workgroups of lds_per_block bytes of LDS that fit a CU, `cap` at most
inline int lds_blocks_per_cu(size_t lds_per_block, int cap) {
  return (int)std::max<size_t>(1, std::min<size_t>((size_t)cap, EXTEND_LDS_LIMIT / std::max<size_t>(lds_per_block, 1)));
}
// Waves of an any-width launch: what the budget holds at per_wave_bytes (the wave's scratch, rounded to 256), 8 per CU at
// most, no more than `want` (the list's length; 8 x n_cu where retries can lengthen it), in whole workgroups of four.
inline uint64_t slow_wave_bytes(uint32_t max_read_len, uint32_t max_bw, uint32_t mk_cap) {
  return (extend_slow_scratch_bytes(max_read_len, max_bw, mk_cap) + 255) & ~255ull;
}
// Where the budget sets the count, rounding up to a whole workgroup would go past it (reads of 65535 bases with a band
// as wide: 4 GiB per wave, five fit, eight would not): then the count is rounded down.  Only a class of more than a
// quarter of the budget per wave, which classify() still takes, exceeds it -- with its one workgroup.
inline uint64_t slow_launch_waves(uint64_t per_wave_bytes, int n_cu, uint64_t want) {
  const uint64_t held = SLOW_SCRATCH_BUDGET / std::max<uint64_t>(per_wave_bytes, 1);
  const uint64_t up = (std::max<uint64_t>(1, std::min(std::min<uint64_t>(held, (uint64_t)n_cu * 8), want)) + 3) / 4 * 4;
  return (up > held && up > 4) ? up - 4 : up;
}

// bw0(L) of reference src/aligner.rs:130-138; non-decreasing in L
inline int band_for_len(const thm_align_opts& o, uint32_t L) {
  volatile float prod = o.min_aln_score_percent * (float)L;
  float pv = prod;
  int pct = (pv != pv) ? 0 : (pv >= 2147483648.0f ? 2147483647 : (pv <= -2147483648.0f ? (-2147483647 - 1) : (int)pv));
  int ms = std::max(pct, o.min_aln_score);
  if (ms < 0) return 0;
  return std::max((int)L - ms, 0);
}

// Length classes of the extend stage for the current options.  Band and buffer sizes grow with the read
// length, so each class is a range of lengths:
//   fast   L <= fast_max: band within +-127 and the wave-private buffers within LDS -> register-resident kernel;
//   slow   fast_max < L <= slow_max: any-width kernel (band in tiles, buffers in global memory);
//   beyond slow_max: the DP trace alone would exceed the memory budget -> per-read THM_ERR_UNSUPPORTED.
struct ExtClasses {
  uint32_t fast_max = 0, fast_len = 0, fast_bw = 0;  // threshold; longest fast read present and its band
  uint32_t slow_max = 0, slow_len = 0, slow_bw = 0;
  uint64_t n_slow = 0;
};
// len_hist: the lengths present in the batch, ascending, with their read counts
inline ExtClasses classify(const std::vector<std::pair<uint32_t, uint64_t>>& len_hist, const thm_align_opts& opts, uint32_t mk_cap_slow) {
  ExtClasses c;
  bool fast_open = true;
  for (const auto& lc : len_hist) {
    const uint32_t L = lc.first;
    const uint32_t bw = (uint32_t)band_for_len(opts, L);
    const int cpl = cells_per_lane(bw);
    if (fast_open && cpl <= 4 && extend_lds_bytes(L, bw, cpl) <= EXTEND_LDS_LIMIT) {
      c.fast_len = L;
      c.fast_bw = bw;
      continue;
    }
    fast_open = false;
    if (extend_slow_scratch_bytes(L, bw, mk_cap_slow) > SLOW_SCRATCH_BUDGET) break;
    c.slow_len = L;
    c.slow_bw = bw;
    c.n_slow += lc.second;
  }
  c.fast_max = c.fast_len;
  c.slow_max = std::max(c.slow_len, c.fast_len);
  return c;
}

struct ExtendPlanIn {
  uint64_t n_reads = 0;
  int n_cu = 1;
  ExtClasses cls;
  uint32_t mk_cap_slow = 1;     // intron markers per alignment of the any-width kernel (the longest transcript's exons)
  bool retry_possible = false;  // the fast kernel can run out of intron markers: the any-width launch takes its retries
  int waves_per_simd = 4;       // extend_waves_per_simd(cells_per_lane(cls.fast_bw), coordinate width)
  bool use_tpr = false;
  // LDS per workgroup of the problem-parallel path's two DP kernels at this class's buffer sizes: kernels_tpr.hip's own
  // carves, extend_dp_lds_bytes(tpr_dp_x_cap, tpr_dp_y_cap) and extend_dpt_lds_bytes(tpr_dpt_tcols)
  size_t dp_lds = 0, dpt_lds = 0;
  uint32_t fin_classes = 0;     // classes the finisher takes in this run (0: it does not run)
};
// Per-wave x and y bytes of the wave-per-problem DP kernel, and the columns of the thread-per-problem kernel's LDS trace
// (class 0: at most DPT_SLOTS band slots hold cells -- such a problem has a band of at most +-7 (|y| <= |x| + 8) or an x
// of at most 15 symbols (|y| <= 16 + bw); at most 128 columns, 64 KiB of LDS per workgroup: longer ones are the
// wave-per-problem kernel's)
inline uint32_t tpr_dp_x_cap(const ExtClasses& c) { return (c.fast_len + 64u + 15u) & ~15u; }
inline uint32_t tpr_dp_y_cap(const ExtClasses& c) { return (c.fast_len + c.fast_bw + 2u + 64u + 15u) & ~15u; }
inline uint32_t tpr_dpt_tcols(const ExtClasses& c) {
  return std::min<uint32_t>(std::min<uint32_t>(tpr_dp_y_cap(c), 128u), std::max<uint32_t>(c.fast_len + DPT_SLOTS / 2 + 2, DPT_SLOTS + c.fast_bw + 2));
}

// One run of the extend stage: every launch's grid and scratch, and where each launch's waves leave their counters.
// Rows of the counter buffer (ExtendParamsT::wave_counters, THM_N_COUNTERS words each), one section per launch, in this
// order; a launch that does not run has an empty section:
//   [row_main, row_team)          wave-per-read kernel, a row per wave
//   [row_team, row_slow)          team kernel (beside the main kernel), a row per wave
//   [row_slow, row_tpr_ctl)       any-width launch, a row per wave
//   [row_tpr_ctl, row_tpr_bail)   problem-parallel path: control kernel, a row per workgroup
//   [row_tpr_bail, row_fin)       ... the wave-per-read launch over what the control kernel leaves, a row per wave
//   [row_fin, n_rows)             the finisher, a row per workgroup
struct ExtendPlan {
  // fast class
  uint32_t fast_len = 0, fast_bw = 0;
  int cpl = 1;
  size_t lds = 0;
  int ext_blocks = 1;    // workgroups that fit the machine at once: LDS and the kernel's register budget
  bool team_ok = false;  // the team kernel takes the reads the plan kernel lists for it
  // global trace scratch (extensions over more than 64 band slots): the team kernel runs BESIDE the main kernel, so its
  // waves have their own slices behind the main kernel's.  Offsets in bytes.
  size_t trace_per_wave = 0, trace_main_off = 0, trace_team_off = 0, trace_bytes = 0;
  // slow class (and the fast kernel's retries)
  bool slow = false;
  uint32_t slow_len = 0, slow_bw = 0, mk_cap_slow = 1;
  uint64_t slow_per_wave = 0, slow_waves = 0;
  // problem-parallel path (pipeline_tpr.hip)
  bool tpr = false;
  uint32_t tpr_max_hits = 0;  // PlanParams::tpr_max_hits
  int ctl_blocks = 0, dp_blocks = 0, dpt_blocks = 0, bail_blocks = 0;
  uint32_t dp_x_cap = 0, dp_y_cap = 0, dpt_tcols = 0;
  int fin_blocks = 0;
  uint64_t row_main = 0, row_team = 0, row_slow = 0, row_tpr_ctl = 0, row_tpr_bail = 0, row_fin = 0, n_rows = 0;
};

inline ExtendPlan plan_extend(const ExtendPlanIn& in) {
  const ExtClasses& cls = in.cls;
  const uint64_t n = in.n_reads;
  ExtendPlan p;
  p.fast_len = cls.fast_len;
  p.fast_bw = cls.fast_bw;
  p.mk_cap_slow = in.mk_cap_slow;
  p.cpl = cells_per_lane(cls.fast_bw);
  p.lds = extend_lds_bytes(cls.fast_len, cls.fast_bw, p.cpl);
  p.ext_blocks = std::min(grid_blocks(in.n_cu, n, 4, lds_blocks_per_cu(p.lds, 8)), in.n_cu * in.waves_per_simd);
  p.team_ok = p.cpl <= 2 && team_fits_lds(p.lds);
  const uint64_t main_waves = (uint64_t)p.ext_blocks * 4, team_waves = p.team_ok ? (uint64_t)in.n_cu * TEAM_WAVES : 0;
  p.trace_per_wave = extend_trace_scratch_bytes(cls.fast_len, cls.fast_bw, p.cpl);
  p.trace_team_off = (size_t)main_waves * p.trace_per_wave;
  p.trace_bytes = (size_t)(main_waves + team_waves) * p.trace_per_wave;
  p.slow = cls.n_slow || in.retry_possible;
  if (p.slow) {
    p.slow_len = std::max(cls.slow_len, cls.fast_len);
    p.slow_bw = std::max(cls.slow_bw, cls.fast_bw);
    p.slow_per_wave = slow_wave_bytes(p.slow_len, p.slow_bw, in.mk_cap_slow);
    p.slow_waves = slow_launch_waves(p.slow_per_wave, in.n_cu, in.retry_possible ? (uint64_t)in.n_cu * 8 : std::max<uint64_t>(cls.n_slow, 1));
  }
  // extension problems as the unit of wavefront work (kernels_tpr.hip): rounds of [control kernel, thread per read | DP
  // kernel, wave per request]; what it cannot take goes on the wave-per-read kernel's list
  p.tpr = in.use_tpr && n > 0 && p.cpl <= 4;
  p.tpr_max_hits = (in.use_tpr && p.cpl <= 4) ? TPR_MAX_HITS : 0u;
  if (p.tpr) {
    p.ctl_blocks = (int)std::min<uint64_t>((n + 255) / 256, (uint64_t)in.n_cu * TPR_CTL_BLOCKS_PER_CU);
    // DP workgroups that fit the machine at once (LDS: x, y, trace and op buffer of four waves; a thread's trace columns)
    p.dp_x_cap = tpr_dp_x_cap(cls);
    p.dp_y_cap = tpr_dp_y_cap(cls);
    p.dp_blocks = in.n_cu * lds_blocks_per_cu(in.dp_lds, TPR_DP_BLOCKS_PER_CU);
    p.dpt_tcols = tpr_dpt_tcols(cls);
    p.dpt_blocks = in.n_cu * lds_blocks_per_cu(in.dpt_lds, 8);
    p.bail_blocks = std::min(p.ext_blocks, in.n_cu);  // (a few thousand reads: one workgroup per CU leaves the machine to the rounds)
  }
  // the finisher (kernels_finish.hip) in front of the wave-per-read kernel
  p.fin_blocks = (!p.tpr && in.fin_classes && n > 0) ? (int)std::min<uint64_t>((n + 255) / 256, (uint64_t)in.n_cu * FINISH_BLOCKS_PER_CU) : 0;
  p.row_team = p.row_main + main_waves;
  p.row_slow = p.row_team + team_waves;
  p.row_tpr_ctl = p.row_slow + p.slow_waves;
  p.row_tpr_bail = p.row_tpr_ctl + (uint64_t)p.ctl_blocks;
  p.row_fin = p.row_tpr_bail + (uint64_t)p.bail_blocks * 4;
  p.n_rows = p.row_fin + (uint64_t)p.fin_blocks;
  return p;
}

}  // namespace thm
#endif
