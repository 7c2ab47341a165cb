// The extend stage's launch plan (thermite_amd/csrc/extend_plan.h) on the host: the plan over a grid of batches, options
// and machines, its invariants at every point, and a few values derived by hand.  Prints the points it checked; the first
// violated invariant is printed with its point and ends the program with status 1.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "extend_plan.h"

using namespace thm;

namespace {

struct Point {
  const char* what = "";
  uint32_t len = 0;
  int band = 0;
  ExtendPlanIn in;
};
const Point* g_at = nullptr;
uint64_t g_checks = 0;

void require(bool ok, const char* expr, int line) {
  g_checks++;
  if (ok) return;
  const ExtendPlanIn& i = g_at->in;
  fprintf(stderr, "extend_plan_main.cpp:%d: %s\n  at %s: L %u band %d n_reads %" PRIu64 " n_cu %d waves_per_simd %d retry %d tpr %d (LDS %zu, %zu) fin %u\n",
          line, expr, g_at->what, g_at->len, g_at->band, i.n_reads, i.n_cu, i.waves_per_simd, (int)i.retry_possible, (int)i.use_tpr, i.dp_lds, i.dpt_lds,
          i.fin_classes);
  exit(1);
}
#define REQUIRE(e) require((e), #e, __LINE__)

// waves per SIMD the wave-per-read kernels are compiled for (extend_waves_per_simd without its tuning knobs)
int waves_per_simd(int cpl, bool wide) { return cpl > 2 ? 4 : (wide ? 5 : (cpl == 1 ? 6 : 5)); }

thm_align_opts opts_for_score(int min_aln_score, float percent) {
  thm_align_opts o{};
  o.min_seed_len = 20;
  o.min_aln_score_percent = percent;
  o.min_aln_score = min_aln_score;
  return o;
}

void check_plan(const Point& pt) {
  g_at = &pt;
  const ExtendPlanIn& in = pt.in;
  const ExtendPlan p = plan_extend(in);
  // the row sections: in the documented order, back to back, summing to n_rows
  const uint64_t at[7] = {p.row_main, p.row_team, p.row_slow, p.row_tpr_ctl, p.row_tpr_bail, p.row_fin, p.n_rows};
  REQUIRE(at[0] == 0);
  uint64_t sum = 0;
  for (int k = 0; k < 6; k++) {
    REQUIRE(at[k] <= at[k + 1]);
    sum += at[k + 1] - at[k];
  }
  REQUIRE(sum == p.n_rows);
  const uint64_t main_rows = at[1] - at[0], team_rows = at[2] - at[1], slow_rows = at[3] - at[2], ctl_rows = at[4] - at[3], bail_rows = at[5] - at[4],
                 fin_rows = at[6] - at[5];
  // every launch has the rows its waves (workgroups) write, and a launch that is absent has none
  REQUIRE(main_rows == (uint64_t)p.ext_blocks * 4);
  REQUIRE(team_rows == (p.team_ok ? (uint64_t)in.n_cu * TEAM_WAVES : 0));
  REQUIRE((team_rows != 0) == p.team_ok);
  REQUIRE(p.slow == (in.cls.n_slow != 0 || in.retry_possible));
  REQUIRE((slow_rows != 0) == p.slow);
  REQUIRE(slow_rows == p.slow_waves);
  REQUIRE(p.tpr == (in.use_tpr && in.n_reads > 0));
  REQUIRE((ctl_rows != 0) == p.tpr && (bail_rows != 0) == p.tpr);
  REQUIRE(ctl_rows == (uint64_t)p.ctl_blocks && bail_rows == (uint64_t)p.bail_blocks * 4);
  REQUIRE((fin_rows != 0) == (p.fin_blocks != 0) && fin_rows == (uint64_t)p.fin_blocks);
  REQUIRE((p.fin_blocks != 0) == (!p.tpr && in.fin_classes != 0 && in.n_reads > 0));
  REQUIRE(!(p.fin_blocks && p.tpr));
  REQUIRE((uint64_t)p.fin_blocks <= (in.n_reads + 255) / 256 && p.fin_blocks <= in.n_cu * FINISH_BLOCKS_PER_CU);
  // trace slices: the team's begins where the main kernel's ends
  REQUIRE(p.trace_main_off == 0);
  REQUIRE(p.trace_team_off == p.trace_main_off + main_rows * p.trace_per_wave);
  REQUIRE(p.trace_bytes == main_rows * p.trace_per_wave + team_rows * p.trace_per_wave);
  REQUIRE(p.trace_team_off % 8 == 0);
  REQUIRE((p.trace_per_wave == 0) == (p.cpl == 1));
  // the any-width launch
  if (p.slow) {
    REQUIRE(p.slow_waves % 4 == 0 && p.slow_waves >= 4);
    REQUIRE(p.slow_waves <= (uint64_t)in.n_cu * 8 + 3);
    REQUIRE(p.slow_per_wave % 256 == 0 && p.slow_per_wave >= extend_slow_scratch_bytes(p.slow_len, p.slow_bw, in.mk_cap_slow));
    // (no class of the grid takes more than a quarter of the budget per wave: check_slow_waves for what holds beyond)
    if (p.slow_per_wave <= SLOW_SCRATCH_BUDGET) REQUIRE(p.slow_waves * p.slow_per_wave <= SLOW_SCRATCH_BUDGET);
    REQUIRE(p.slow_len >= in.cls.fast_len && p.slow_len >= in.cls.slow_len && p.slow_bw >= in.cls.fast_bw && p.slow_bw >= in.cls.slow_bw);
  } else {
    REQUIRE(p.slow_waves == 0 && p.slow_per_wave == 0);
  }
  // the main kernel's grid
  REQUIRE(p.cpl == cells_per_lane(in.cls.fast_bw) && p.cpl >= 1 && p.cpl <= 4);
  REQUIRE(p.lds == extend_lds_bytes(in.cls.fast_len, in.cls.fast_bw, p.cpl) && p.lds <= EXTEND_LDS_LIMIT);
  REQUIRE(p.ext_blocks >= 1 && p.ext_blocks <= in.n_cu * in.waves_per_simd);
  REQUIRE((uint64_t)p.ext_blocks * p.lds <= (uint64_t)in.n_cu * EXTEND_LDS_LIMIT);
  REQUIRE(!p.team_ok || p.cpl <= 2);
  REQUIRE(!p.team_ok || p.lds / 4 * TEAM_WAVES + TEAM_STATIC_LDS <= EXTEND_LDS_LIMIT);
  // the problem-parallel path's grids
  REQUIRE(p.tpr_max_hits == (in.use_tpr ? TPR_MAX_HITS : 0u));
  if (p.tpr) {
    REQUIRE(p.ctl_blocks >= 1 && p.dp_blocks >= in.n_cu && p.dpt_blocks >= in.n_cu && p.bail_blocks >= 1 && p.bail_blocks <= p.ext_blocks);
    REQUIRE(p.dp_x_cap % 16 == 0 && p.dp_y_cap % 16 == 0 && p.dp_x_cap >= in.cls.fast_len + 64 && p.dp_y_cap >= in.cls.fast_len + in.cls.fast_bw + 66);
    REQUIRE(p.dp_x_cap == tpr_dp_x_cap(in.cls) && p.dp_y_cap == tpr_dp_y_cap(in.cls) && p.dpt_tcols == tpr_dpt_tcols(in.cls));
    REQUIRE(p.dpt_tcols <= 128 && p.dpt_tcols <= p.dp_y_cap);
    // as many workgroups per CU as the kernel's LDS allows, within the cap, one at least
    const size_t lds[2] = {in.dp_lds, in.dpt_lds};
    const int blocks[2] = {p.dp_blocks, p.dpt_blocks}, cap[2] = {TPR_DP_BLOCKS_PER_CU, 8};
    for (int k = 0; k < 2; k++) {
      const int per_cu = blocks[k] / in.n_cu;
      REQUIRE(blocks[k] % in.n_cu == 0 && per_cu >= 1 && per_cu <= cap[k]);
      REQUIRE(per_cu == 1 || (uint64_t)per_cu * lds[k] <= EXTEND_LDS_LIMIT);
      REQUIRE(per_cu == cap[k] || (uint64_t)(per_cu + 1) * lds[k] > EXTEND_LDS_LIMIT);
    }
  } else {
    REQUIRE(p.ctl_blocks == 0 && p.dp_blocks == 0 && p.dpt_blocks == 0 && p.bail_blocks == 0);
  }
}

// can the register-resident kernels / the any-width kernel hold reads of length L under these options?
bool holds_fast(const thm_align_opts& o, uint32_t L) {
  const uint32_t bw = (uint32_t)band_for_len(o, L);
  return cells_per_lane(bw) <= 4 && extend_lds_bytes(L, bw, cells_per_lane(bw)) <= EXTEND_LDS_LIMIT;
}
bool holds_slow(const thm_align_opts& o, uint32_t L, uint32_t mk_cap) {
  return extend_slow_scratch_bytes(L, (uint32_t)band_for_len(o, L), mk_cap) <= SLOW_SCRATCH_BUDGET;
}

const uint32_t LENS[] = {1, 20, 91, 150, 260, 1000, 6000, 65535};

// classify over a histogram of all the grid's lengths: a fast prefix, then a slow run, then nothing
void check_classify(const Point& pt, const thm_align_opts& o, uint32_t mk_cap) {
  g_at = &pt;
  std::vector<std::pair<uint32_t, uint64_t>> hist;
  for (uint32_t L : LENS) hist.emplace_back(L, (uint64_t)L + 1);
  const ExtClasses c = classify(hist, o, mk_cap);
  REQUIRE(c.fast_max <= c.slow_max && c.fast_max == c.fast_len);
  uint64_t n_slow = 0;
  int stage = 0;  // 0: fast, 1: slow, 2: beyond
  int prev_bw = 0;
  for (const auto& lc : hist) {
    const uint32_t L = lc.first;
    const int bw = band_for_len(o, L);
    REQUIRE(bw >= prev_bw && bw >= 0 && (uint32_t)bw <= L);  // non-decreasing in L
    prev_bw = bw;
    if (stage == 0 && !holds_fast(o, L)) stage = 1;
    if (stage == 1 && !holds_slow(o, L, mk_cap)) stage = 2;
    if (stage == 0) {
      REQUIRE(L <= c.fast_max);
    } else if (stage == 1) {
      REQUIRE(L > c.fast_max && L <= c.slow_max);
      n_slow += lc.second;
    } else {
      REQUIRE(L > c.slow_max);
    }
    if (L == c.fast_len) REQUIRE((uint32_t)bw == c.fast_bw);
    if (L == c.slow_len && c.slow_len > c.fast_len) REQUIRE((uint32_t)bw == c.slow_bw);
  }
  REQUIRE(n_slow == c.n_slow);
}

uint64_t grid() {
  const int BANDS[] = {0, 31, 32, 61, 63, 64, 127, 128, -30 /* L - 30 */};
  const uint64_t N_READS[] = {0, 1, 3, 3000, 500000};
  const int N_CU[] = {1, 8, 256};
  uint64_t points = 0;
  for (uint32_t L : LENS)
    for (int b : BANDS)
      for (int by_percent = 0; by_percent < 2; by_percent++) {
        const int band = b < 0 ? (int)L + b : b;
        if (band < 0 || band > (int)L) continue;  // (a band is at most the read's length)
        // band = L - max((int)(percent * L), min_aln_score): by the absolute score, or by the fraction that truncates to it
        thm_align_opts o = opts_for_score((int)L - band, 0.0f);
        if (by_percent) {
          o = opts_for_score(0, ((float)((int)L - band) + 0.25f) / (float)L);
          if (o.min_aln_score_percent > 1.0f) continue;
        }
        Point pt;
        pt.what = by_percent ? "grid (band by min_aln_score_percent)" : "grid (band by min_aln_score)";
        pt.len = L;
        pt.band = band;
        g_at = &pt;
        REQUIRE(band_for_len(o, L) == band);
        for (int retry = 0; retry < 2; retry++) {
          const uint32_t mk_cap = retry ? 200u : 8u;  // retries are possible when a transcript has more exons than FAST_MAX_YCLIPS + 1
          check_classify(pt, o, mk_cap);
          for (uint64_t n : N_READS)
            for (int mixed = 0; mixed < 2; mixed++) {
              // the batch: n reads of length L, or a quarter of them beside reads of 91 bases
              std::vector<std::pair<uint32_t, uint64_t>> hist;
              if (mixed && L != 91 && n >= 4) {
                hist.emplace_back(91u, n - n / 4);
                hist.emplace_back(L, n / 4);
                std::sort(hist.begin(), hist.end());
              } else if (mixed) {
                continue;
              } else if (n) {
                hist.emplace_back(L, n);
              }
              const ExtClasses cls = classify(hist, o, mk_cap);
              for (int n_cu : N_CU)
                for (int wide = 0; wide < 2; wide++)
                  // the usual path; the problem-parallel path with DP kernels of little LDS, of the headline shape's, and
                  // of more than a CU holds
                  for (int tpr = 0; tpr < 4; tpr++)
                    for (uint32_t fin : {0u, 3u}) {
                      const size_t DP_LDS[] = {0, 1, 17536, EXTEND_LDS_LIMIT + 1}, DPT_LDS[] = {0, 4096, 51712, 2 * EXTEND_LDS_LIMIT};
                      pt.in.dp_lds = DP_LDS[tpr];
                      pt.in.dpt_lds = DPT_LDS[tpr];
                      pt.in.n_reads = n;
                      pt.in.n_cu = n_cu;
                      pt.in.cls = cls;
                      pt.in.mk_cap_slow = mk_cap;
                      pt.in.retry_possible = retry != 0;
                      pt.in.waves_per_simd = waves_per_simd(cells_per_lane(cls.fast_bw), wide != 0);
                      pt.in.use_tpr = tpr != 0;
                      pt.in.fin_classes = fin;
                      check_plan(pt);
                      points++;
                    }
            }
        }
      }
  return points;
}

// The any-width launch's wave count apart from the plan: whole workgroups, and within the budget wherever one workgroup
// of four waves is (a class of more than a quarter of the budget per wave, which classify() still takes, gets its one
// workgroup and exceeds it: the exception is pinned here, not hidden by the grid, which has no such class)
void check_slow_waves() {
  Point pt;
  pt.what = "slow_launch_waves";
  g_at = &pt;
  const uint64_t B = SLOW_SCRATCH_BUDGET;
  const uint64_t PER_WAVE[] = {256, 1 << 20, 12 << 20, (12 << 20) + 256, 36 << 20, B / 2049, B / 2048, B / 700, B / 9, B / 8, B / 7, B / 6, B / 5 + 256, B / 5,
                               B / 4 - 256, B / 4};
  for (uint64_t pw : PER_WAVE)
    for (int n_cu : {1, 8, 256})
      for (uint64_t want : {(uint64_t)1, (uint64_t)3, (uint64_t)4, (uint64_t)5, (uint64_t)700, (uint64_t)n_cu * 8}) {
        pt.in.n_cu = n_cu;
        pt.in.n_reads = want;
        const uint64_t w = slow_launch_waves(pw, n_cu, want);
        REQUIRE(w % 4 == 0 && w >= 4 && w <= (uint64_t)n_cu * 8 + 3 && w < want + 4);
        REQUIRE(w * pw <= B);
        // and no workgroup fewer than the budget, the machine and the list allow
        REQUIRE(w + 4 > std::min(std::min(B / pw, (uint64_t)n_cu * 8), want) || (w + 4) * pw > B);
      }
  for (uint64_t pw : {B / 4 + 256, B / 3, B / 2, B})
    REQUIRE(slow_launch_waves(pw, 256, 2048) == 4);  // 4 x pw > B: the one workgroup a launch cannot go below
}

// Values worked out by hand from the formulas of ext_caps / extend_lds_bytes and the grid rules.
void anchors() {
  Point pt;
  pt.what = "anchor";
  g_at = &pt;
  {
    // The headline shape: 500000 reads of 91 bases, min_aln_score 30 -> band 91 - 30 = +-61, 123 slots -> 2 cells per lane.
    //   lcap = (91 + 31) & ~15 = 112; wcap = (2 * 152 + 91 + 48) & ~15 = 443 & ~15 = 432; ycols = 91 + 61 + 2 = 154;
    //   trb = 155 * 16 = 2480; opcap = (182 + 122 + 31) & ~15 = 320; markers 8 * 64 = 512; keys 16 * 32 = 512
    //   per wave 112 + 864 + 2480 + 960 + 512 + 512 = 5440; lds = 4 * 5440 = 21760
    //   workgroups per CU by LDS: min(8, 163840 / 21760 = 7) = 7 -> 1792; by registers 256 * 5 = 1280 -> ext_blocks 1280
    //   team: 21760 / 4 * 16 + 16960 + 256 = 104256 <= 163840 -> fits
    //   trace per wave (91 + 61 + 3) * 2 * 16 = 4960; finisher min(ceil(500000 / 256) = 1954, 2048) = 1954
    //   rows: 1280 * 4 + 256 * 16 + 1954 = 11170
    pt.len = 91;
    pt.band = 61;
    const ExtClasses cls = classify({{91u, 500000u}}, opts_for_score(30, 0.0f), 8);
    REQUIRE(cls.fast_len == 91 && cls.fast_bw == 61 && cls.n_slow == 0);
    pt.in = ExtendPlanIn{500000, 256, cls, 8, false, waves_per_simd(2, false), false, 0, 0, 3};
    const ExtendPlan p = plan_extend(pt.in);
    REQUIRE(p.cpl == 2 && p.lds == 21760 && p.ext_blocks == 1280 && p.team_ok);
    REQUIRE(p.trace_per_wave == 4960 && p.trace_team_off == 5120u * 4960u && p.trace_bytes == (5120u + 4096u) * 4960u);
    REQUIRE(p.fin_blocks == 1954 && p.n_rows == 11170 && p.row_team == 5120 && p.row_slow == 9216 && p.row_fin == 9216);
    // ... the same batch on the problem-parallel path: no finisher; control kernel min(1954, 256 * 4) = 1024 workgroups;
    // the wave-per-read launches beside and behind the rounds min(1280, 256) = 256 workgroups.  The DP kernels' LDS at
    // this shape, 17536 and 51712 bytes per workgroup, are what a kernel trace of the library shows for x_cap 160, y_cap
    // 224 and 101 trace columns: 163840 / 17536 = 9 -> the cap of 8 per CU, 2048 workgroups; 163840 / 51712 = 3 -> 768
    // (the grids of extend_dp_kernel and extend_dpt_kernel in profiles/extend_plan/launches_b_*.txt, 256 CUs)
    pt.in.use_tpr = true;
    pt.in.dp_lds = 17536;
    pt.in.dpt_lds = 51712;
    const ExtendPlan q = plan_extend(pt.in);
    REQUIRE(q.tpr && q.fin_blocks == 0 && q.ctl_blocks == 1024 && q.bail_blocks == 256);
    REQUIRE(q.row_tpr_ctl == 9216 && q.row_tpr_bail == 10240 && q.row_fin == 11264 && q.n_rows == 11264);
    REQUIRE(q.dp_blocks == 2048 && q.dpt_blocks == 768);
    REQUIRE(q.dp_x_cap == 160 && q.dp_y_cap == 224 && q.dpt_tcols == 101);  // (91 + 79) & ~15; (91 + 61 + 81) & ~15; max(91 + 10, 16 + 63)
  }
  {
    // 150 bases, min_aln_score 86 -> band +-64, 129 slots -> 3 cells per lane (no team kernel; two trace cells per lane in LDS).
    //   lcap = 181 & ~15 = 176; wcap = (2 * 214 + 150 + 48) & ~15 = 626 & ~15 = 624; ycols = 216; trb = 217 * 32 = 6944;
    //   opcap = (300 + 128 + 31) & ~15 = 448; per wave 176 + 1248 + 6944 + 1344 + 512 + 512 = 10736; lds = 42944
    //   workgroups per CU by LDS: 163840 / 42944 = 3 -> 768; by registers 256 * 4 = 1024 -> ext_blocks 768
    //   trace per wave (150 + 64 + 3) * 3 * 16 = 10416; rows 768 * 4 + 1954 = 5026
    pt.len = 150;
    pt.band = 64;
    const ExtClasses cls = classify({{150u, 500000u}}, opts_for_score(86, 0.0f), 8);
    REQUIRE(cls.fast_len == 150 && cls.fast_bw == 64 && cls.n_slow == 0);
    pt.in = ExtendPlanIn{500000, 256, cls, 8, false, waves_per_simd(3, false), false, 0, 0, 3};
    const ExtendPlan p = plan_extend(pt.in);
    REQUIRE(p.cpl == 3 && p.lds == 42944 && p.ext_blocks == 768 && !p.team_ok);
    REQUIRE(p.trace_per_wave == 10416 && p.trace_team_off == p.trace_bytes && p.trace_bytes == 3072u * 10416u);
    REQUIRE(p.fin_blocks == 1954 && p.n_rows == 5026 && p.row_team == 3072 && p.row_fin == 3072);
  }
  {
    // Three reads of 1000 bases beside 2997 of 91, min_aln_score 30: band +-970 is beyond four cells per lane -> slow class.
    // One workgroup of four waves (the list has three reads); with retries possible 8 waves per CU.
    pt.len = 1000;
    pt.band = 970;
    const ExtClasses cls = classify({{91u, 2997u}, {1000u, 3u}}, opts_for_score(30, 0.0f), 8);
    REQUIRE(cls.fast_len == 91 && cls.slow_len == 1000 && cls.slow_bw == 970 && cls.n_slow == 3 && cls.slow_max == 1000);
    pt.in = ExtendPlanIn{3000, 8, cls, 8, false, waves_per_simd(2, false), false, 0, 0, 3};
    ExtendPlan p = plan_extend(pt.in);
    // main: min(ceil(3000 / 4) = 750, 8 * 7 = 56, 8 * 5 = 40) = 40 workgroups; team 8 * 16 rows; finisher ceil(3000 / 256) = 12
    REQUIRE(p.ext_blocks == 40 && p.slow_waves == 4 && p.row_slow == 160 + 128 && p.row_tpr_ctl == 292 && p.n_rows == 292 + 12);
    pt.in.retry_possible = true;
    p = plan_extend(pt.in);
    REQUIRE(p.slow_waves == 64 && p.n_rows == 288 + 64 + 12);
  }
}

}  // namespace

int main() {
  const uint64_t points = grid();
  check_slow_waves();
  anchors();
  printf("points %" PRIu64 " checks %" PRIu64 "\n", points, g_checks);
  return 0;
}
