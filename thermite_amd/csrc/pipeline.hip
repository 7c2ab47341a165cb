// pipeline.hip -- the batched read-level entry points of include/thermite.h:
//   thm_batch_upload / thm_batch_run / thm_batch_sync / thm_batch_fetch,
//   thm_align_batch (= the three in sequence) and thm_smems_batch.
//
// One batch = count -> scan -> fill on the device:
//   seed kernels    SMEMs per read (pool + per-read run), hit counts
//   scan            hit counts -> per-read slice of the candidate array (its last phase is the plan kernel's)
//   plan kernel     lists: reads with many hits (longest jobs first), reads of the slow class; a record per read
//   extend kernel   align_read per read; accepted alignments into the slice,
//                   op streams into a bump-allocated pool; final order list.
//                   Reads whose band or length exceeds what the register-resident kernel
//                   holds (the slow class) run afterwards in the any-width kernel.
//   scans           alignment counts / op bytes -> output offsets
//   compact kernel  canonical output (alignments in read order, op streams
//                   back to back), so the D2H copy is a plain memcpy
// Pool capacities are heuristics; a kernel that runs out sets a fault bit and
// thm_batch_sync grows the pools and replays the batch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "aligner_internal.h"
#include "smem_finish.h"

using namespace thm;

// THM_SEED_FILL = 0 | 1 | 2: which form of the seed kernels' fill pass runs (launch_seed)
uint32_t seed_fill_mode() {
  static const uint32_t v = [] {
    const char* e = getenv("THM_SEED_FILL");
    const int v = e ? atoi(e) : 0;
    return (uint32_t)(v >= 0 && v <= 2 ? v : 0);
  }();
  return v;
}
// THM_TEAM_DIV_PER_CU (tuning knob): TEAM_DIV_PER_CU of the plan kernel's team threshold (launch.h)
unsigned team_div_per_cu() {
  static const unsigned v = [] {
    const char* e = getenv("THM_TEAM_DIV_PER_CU");
    const int v = e ? atoi(e) : 0;
    return v > 0 ? (unsigned)v : TEAM_DIV_PER_CU;
  }();
  return v;
}

namespace {

template <class C>
const DeviceIndexT<C>& dev_view(const thm_aligner* a);
template <>
const DeviceIndexT<uint32_t>& dev_view<uint32_t>(const thm_aligner* a) {
  return a->dix->view;
}
template <>
const DeviceIndexT<uint64_t>& dev_view<uint64_t>(const thm_aligner* a) {
  return a->dix->view64;
}

// finish_scan: the hit-count scan runs to its end here (thm_smems_batch); a full run leaves its last phase to
// plan_pack_kernel
template <class C>
int enqueue_seed_t(thm_aligner* a, uint32_t min_seed_len, bool finish_scan) {
  const uint64_t n = a->n_reads;
  hipStream_t s = a->stream;
  HIPCHK(a, a->seed.off.ensure(n + 1));
  HIPCHK(a, a->seed.cnt.ensure(n + 1));
  HIPCHK(a, a->seed.hits.ensure(n + 1));
  HIPCHK(a, a->seed.cand_off.ensure(n + 2));
  HIPCHK(a, a->seed.scan_tmp.ensure(2 * scan_tmp_entries(n + 1), 64));  // (twice: the two-array scan of the output offsets)
  HIPCHK(a, a->reads.status.ensure(n + 1, 16));
  // typical: 1-2 SMEMs per read; waves take the pool in 256-entry slices, hence the fixed slack
  const uint64_t smem_min = a->dbg_smem_cap ? a->dbg_smem_cap : n * 4 + (4u << 20);
  if (a->seed.smem_cap < smem_min) a->seed.smem_cap = smem_min;
  HIPCHK(a, a->seed.smems.ensure(a->seed.smem_cap * sizeof(SmemT<C>)));
  if (!a->dbg_smem_cap) a->seed.smem_cap = std::max<uint64_t>(a->seed.smem_cap, a->seed.smems.cap / sizeof(SmemT<C>));
  // to_ascii_uppercase (src/aligner.rs:125) + sanitising, once per run for both kernels
  // (16 bytes in front: a left extension is read in whole 8-byte words that may begin a few bytes before the first read)
  HIPCHK(a, a->reads.san.ensure(a->n_bases, 256 + 16));
  // The same launch starts the run: control block (list counts, cursors, fault words, the queue words of both
  // stages), per-read statuses and the 16 bytes in front zeroed, counters copied to their snapshot row (as they stood
  // before this attempt, so that a replay after a pool overflow does not count twice).
  {
    RunResetParams rp;
    rp.ctl = a->d_ctl.as<uint4>();
    rp.ctl_vec4 = (uint32_t)(thm_aligner::CTL_BYTES / 16);
    rp.status = reinterpret_cast<uint4*>(a->reads.status.get());
    rp.status_vec4 = ((n + 1) * 4 + 15) / 16;
    rp.san_head = reinterpret_cast<uint4*>(a->reads.san.get());
    rp.counters = a->d_counters;
    HIPCHK(a, launch_sanitize_reset(a->reads.bases, a->reads.san + 16, a->n_bases, a->n_bases + 128, rp, s));
  }
  // length classes of the seed stage (launch.h): short reads take the byte-per-position paths
  uint64_t n_long = 0;
  uint32_t max_short = 0, max_long = 0;
  for (const auto& lc : a->len_hist) {
    if (lc.first <= SHORT_READ_MAX) {
      max_short = std::max(max_short, lc.first);
    } else {
      max_long = std::max(max_long, lc.first);
      n_long += lc.second;
    }
  }
  const uint64_t n_short = n - n_long;
  // ragged per-position rows (launch.h, ms_row)
  const uint64_t items = ms_row(a->n_bases, n) + 64;
  HIPCHK(a, a->seed.ms_end.ensure(items, 64));
  HIPCHK(a, a->seed.ms_lo.ensure(items * sizeof(C) + 64));
  HIPCHK(a, a->seed.ms_hi.ensure(items * sizeof(C) + 64));
  auto cells_of = [&](uint32_t max_len) -> uint64_t {
    const uint32_t P = (max_len >= min_seed_len) ? max_len - min_seed_len + 1 : 1;
    return (P + 7) / 8;
  };
  const uint64_t cells = n_short * cells_of(max_short) + n_long * cells_of(max_long);
  HIPCHK(a, a->seed.work_reads.ensure(n + 1));
  HIPCHK(a, a->seed.work_long.ensure(n_long + 1));
  HIPCHK(a, a->seed.work_cells.ensure(std::max(cells, n) + 1));
  const int n_blocks = grid_blocks(a, n, 4, lds_blocks_per_cu(std::min(seed_select_lds_bytes(std::max(max_short, 1u)), SEED_SELECT_LDS_LIMIT), 8));
  SeedParamsT<C> sp;
  sp.ix = dev_view<C>(a);
  sp.reads.bases = a->reads.san + 16;
  sp.reads.offsets = a->reads.offsets;
  sp.reads.n_reads = n;
  sp.min_seed_len = min_seed_len;
  sp.max_len_short = max_short;
  sp.max_len_long = max_long;
  sp.n_long = n_long;
  sp.ms_end = a->seed.ms_end;
  sp.ms_lo = a->seed.ms_lo.as<C>();
  sp.ms_hi = a->seed.ms_hi.as<C>();
  sp.work_short = a->seed.work_reads;
  sp.work_long = a->seed.work_long;
  sp.work_cells = a->seed.work_cells;
  sp.work_counts = a->s_work_counts;
  sp.flags = (a->dbg_seed_noinfer ? 0u : SEED_INFER) | (a->dbg_seed_stats ? SEED_STATS : 0u) | (a->dbg_seed_nodirect ? SEED_NODIRECT : 0u) |
             (a->dbg_seed_nobounds ? 0u : SEED_BOUNDS);
  sp.smems = a->seed.smems.as<SmemT<C>>();
  sp.smem_cap = a->seed.smem_cap;
  sp.cursor = a->d_cursors;
  sp.read_smem_off = a->seed.off;
  sp.read_smem_cnt = a->seed.cnt;
  sp.read_hits = a->seed.hits;
  sp.read_status = a->reads.status;
  sp.counters = a->d_counters;
  sp.queue = a->d_queue;
  sp.fault = a->d_fault;
  sp.sel_scratch = nullptr;
  sp.sel_scratch_per_wave = 0;
  const uint32_t fill_mode = seed_fill_mode();
  sp.fill_mode = fill_mode;
  sp.fill_keys = nullptr;
  sp.fill_perm = nullptr;
  sp.fill_hist = nullptr;
  if (fill_mode == 2) {
    const uint64_t slots = (std::max(cells, n) + 1) * 8;
    HIPCHK(a, a->seed.fill_keys.ensure(slots));
    HIPCHK(a, a->seed.fill_perm.ensure(slots));
    HIPCHK(a, a->seed.fill_hist.ensure(2 * (FILL_BUCKETS + 1) + 1));
    HIPCHK(a, hipMemsetAsync(a->seed.fill_hist, 0, (2 * (FILL_BUCKETS + 1) + 1) * 4, s));
    sp.fill_keys = a->seed.fill_keys;
    sp.fill_perm = a->seed.fill_perm;
    sp.fill_hist = a->seed.fill_hist;
  }
  if (n_long && seed_select_lds_bytes(max_long) > SEED_SELECT_LDS_LIMIT) {
    // reads of thousands of bases: the selection kernel's per-read lists go to global memory
    const int nb = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)n_blocks, (n_long + 3) / 4));
    sp.sel_scratch_per_wave = (seed_select_scratch_bytes(max_long) + 255) & ~255ull;
    HIPCHK(a, a->seed.sel_scratch.ensure((size_t)nb * 4 * sp.sel_scratch_per_wave, 256));
    sp.sel_scratch = a->seed.sel_scratch;
  }
  HIPCHK(a, launch_seed(sp, n_blocks, s));
  // hit counts -> offsets of each read's slice (also the Mem offsets of thm_smems_batch)
  if (finish_scan)
    HIPCHK(a, launch_exclusive_scan_u64(a->seed.hits, a->seed.cand_off, n, a->seed.scan_tmp, s));
  else
    HIPCHK(a, launch_scan_tiles_sums_u64(a->seed.hits, a->seed.cand_off, n, a->seed.scan_tmp, s));
  return THM_OK;
}

int enqueue_seed(thm_aligner* a, uint32_t min_seed_len, bool finish_scan) {
  return a->dix->wide ? enqueue_seed_t<uint64_t>(a, min_seed_len, finish_scan) : enqueue_seed_t<uint32_t>(a, min_seed_len, finish_scan);
}

// the extend stage's lists and the per-read records, one launch (kernels_seed.hip, plan_pack_kernel)
template <class C>
int enqueue_plan_pack_t(thm_aligner* a, const PlanParams& pp) {
  HIPCHK(a, a->ext.recs.ensure((a->n_reads + 1) * sizeof(ReadRecT<C>)));
  PackParamsT<C> pk;
  pk.sa = dev_view<C>(a).sa;
  pk.offsets = a->reads.offsets;
  pk.n_reads = a->n_reads;
  pk.smems = a->seed.smems.as<SmemT<C>>();
  pk.read_smem_off = a->seed.off;
  pk.read_smem_cnt = a->seed.cnt;
  pk.read_cand_off = a->seed.cand_off;
  pk.tile_offs = a->seed.scan_tmp;
  pk.fault_seed = a->d_fault;
  pk.recs = a->ext.recs.as<ReadRecT<C>>();
  HIPCHK(a, launch_plan_pack(pp, pk, a->stream));
  return THM_OK;
}

// The extend stage of one run over its plan (extend_plan.h): the finisher, then the team kernel beside the wave-per-read
// kernel (or the problem-parallel path in their place), the any-width launch, and the reduction of the waves' counters.
template <class C>
int enqueue_extend_t(thm_aligner* a, const ExtendPlan& plan) {
  const uint64_t n = a->n_reads;
  hipStream_t s = a->stream;
  const int cpl = plan.cpl;
  a->fin_blocks = (uint32_t)plan.fin_blocks;
  HIPCHK(a, a->ext.trace.ensure(plan.trace_bytes + 64));
  // The counter rows are zero from one run to the next (launch_counters_reduce zeroes what it read, and no launch writes
  // past its run's n_rows): only a new allocation is zeroed here -- or the rows of an enqueue that failed half way.
  HIPCHK(a, a->ext.wcnt.ensure(plan.n_rows * THM_N_COUNTERS, 64));
  if (a->ext.wcnt_clean_cap != a->ext.wcnt.cap()) HIPCHK(a, hipMemsetAsync(a->ext.wcnt, 0, a->ext.wcnt.cap(), s));
  a->ext.wcnt_clean_cap = 0;
  // ---- fast class: the main kernel's parameter block; the other launches take copies of it ----
  ExtendParamsT<C> ep;
  ep.ix = dev_view<C>(a);
  ep.reads.bases = a->reads.san + 16;
  ep.reads.offsets = a->reads.offsets;
  ep.reads.n_reads = n;
  ep.opts = a->run_opts;
  ep.smems = a->seed.smems.as<SmemT<C>>();
  // one record per read (offsets, SMEM run, candidate slice, first SMEM and its first occurrence): enqueue_plan_pack_t
  ep.read_recs = a->ext.recs.as<ReadRecT<C>>();
  ep.heavy = a->seed.heavy;
  ep.heavy_count = a->s_work_counts + 2;
  ep.team = a->seed.team;
  ep.team_count = a->s_work_counts + 7;
  ep.team_limit = 2u * (uint32_t)a->n_cu;
  ep.cands = a->ext.cands;
  ep.cand_cap = a->ext.cand_cap;
  ep.order = a->ext.order;
  ep.cand_ops = a->ext.ops;
  ep.cand_ops_cap = a->ext.cand_ops_cap;
  ep.ops_cursor = a->d_cursors + 1;
  ep.read_n_alns = a->ext.nalns;
  ep.read_op_bytes = a->ext.opbytes;
  ep.read_status = a->reads.status;
  ep.retry = a->seed.slow;
  ep.retry_count = a->s_work_counts + 5;
  ep.n_contract = a->s_work_counts + 6;
  ep.counters = a->d_counters;
  ep.wave_counters = counter_rows(a, plan.row_main);
  ep.queue = a->d_queue_ext;  // (not the seed stage's words: both sets were zeroed when the run began)
  ep.fault = a->d_fault + 1;
  ep.fault_seed = a->d_fault;
  ep.prof = a->d_counters + 2 * THM_N_COUNTERS;
  ep.max_read_len = plan.fast_len;
  ep.max_bw = plan.fast_bw;
  if (a->dbg_band_clip) ep.max_bw = std::min<uint32_t>(ep.max_bw, a->dbg_band_clip - 1);  // test hook: reads beyond get THM_ERR_INTERNAL
  ep.mk_cap = FAST_MAX_YCLIPS;
  ep.list_only = 0;
  ep.skip_scan = 0;
  ep.trace_scratch = a->ext.trace.as<unsigned long long>() + plan.trace_main_off / 8;
  ep.slow_scratch = nullptr;
  ep.slow_scratch_per_wave = 0;
  // ---- the finisher (kernels_finish.hip), in front of the wave-per-read kernel ----
  // It runs before the fork, with the machine to itself.  (On the main kernel's stream, beside the team kernel -- whose reads
  // are never the finisher's -- it was measured at 120 - 430 us instead: a team workgroup takes a whole CU's registers, and
  // the main kernel waited for the finisher all that time)
  if (plan.fin_blocks) {
    HIPCHK(a, a->ext.finstats.ensure((size_t)plan.fin_blocks * 4));
    FinishParamsT<C> fp;
    fp.ix = ep.ix;
    fp.reads = ep.reads;
    fp.opts = ep.opts;
    fp.smems = ep.smems;
    fp.recs = a->ext.recs.as<ReadRecT<C>>();
    fp.cands = ep.cands;
    fp.cand_cap = ep.cand_cap;
    fp.order = ep.order;
    fp.read_n_alns = ep.read_n_alns;
    fp.read_op_bytes = ep.read_op_bytes;
    fp.rows = counter_rows(a, plan.row_fin);
    fp.stats = a->ext.finstats;
    fp.fault_seed = ep.fault_seed;
    fp.max_read_len = ep.max_read_len;
    fp.max_bw = ep.max_bw;
    fp.cpl = (uint32_t)cpl;
    fp.classes = a->fin_run_classes;
    fp.run_half = a->ops_run_half;
    HIPCHK(a, launch_smem_finish(fp, plan.fin_blocks, s));
  }
  if (plan.tpr) {
    const int rc = enqueue_tpr_rounds(a, plan, ep);
    if (rc != THM_OK) return rc;
  } else if (plan.team_ok) {
    // Reads with very many hits: a workgroup per read (speculative chunks of hits, kernels_extend.hip TEAM) BESIDE the
    // wave-per-read kernel: such reads are the long jobs of a batch, a launch behind the main kernel would put them on the
    // critical path.  A team workgroup needs a whole CU's registers, so it must be placed before the persistent waves of
    // the main kernel fill the machine: the team kernel goes first on this stream, the main kernel on the second stream
    // behind an event (the event's latency is the team's head start; the other way round the team kernel started 10 us
    // late and waited for the main kernel to drain -- rocprofv3 kernel trace, tools/overlap_trace.py).
    HIPCHK(a, hipEventRecord(a->ev_fork, s));
    HIPCHK(a, launch_extend(team_params(a, plan, ep), cpl, a->n_cu, s, true));
    HIPCHK(a, hipStreamWaitEvent(a->stream2, a->ev_fork, 0));
    HIPCHK(a, launch_extend(ep, cpl, plan.ext_blocks, a->stream2));
    HIPCHK(a, hipEventRecord(a->ev_join, a->stream2));
    HIPCHK(a, hipStreamWaitEvent(s, a->ev_join, 0));
  } else {
    HIPCHK(a, launch_extend(ep, cpl, plan.ext_blocks, s));
  }
  // ---- slow class (and the fast kernel's retries) ----
  if (plan.slow) {
    HIPCHK(a, a->ext.slow.ensure((size_t)plan.slow_waves * plan.slow_per_wave, 256));
    ep.wave_counters = counter_rows(a, plan.row_slow);
    ep.max_read_len = plan.slow_len;
    ep.max_bw = plan.slow_bw;
    ep.mk_cap = plan.mk_cap_slow;
    ep.list_only = 1;
    ep.heavy = a->seed.slow;
    ep.heavy_count = a->s_work_counts + 5;
    ep.team = nullptr;
    ep.team_count = nullptr;
    ep.slow_scratch = a->ext.slow;
    ep.slow_scratch_per_wave = plan.slow_per_wave;
    HIPCHK(a, launch_extend(ep, 0, (int)(plan.slow_waves / 4), s));
  }
  HIPCHK(a, launch_counters_reduce(a->ext.wcnt, (uint32_t)plan.n_rows, a->d_counters, s));
  a->ext.wcnt_clean_cap = a->ext.wcnt.cap();
  return THM_OK;
}

int enqueue_run(thm_aligner* a) {
  const uint64_t n = a->n_reads;
  hipStream_t s = a->stream;
  HIPCHK(a, hipEventRecord(a->ev[0], s));
  // (the seed stage's first kernel zeroes the run's control words and takes the counter snapshot)
  int rc = enqueue_seed(a, (uint32_t)a->run_opts.min_seed_len, false);
  if (rc != THM_OK) return rc;
  HIPCHK(a, hipEventRecord(a->ev[1], s));

  const uint64_t cand_min = a->dbg_cand_cap ? a->dbg_cand_cap : n * 3 + 1024;
  // op bytes: about 2 L per exonic alignment (genome + transcript op streams), 384 per read at least
  const uint64_t ops_min = a->dbg_ops_cap ? a->dbg_ops_cap : std::max<uint64_t>(n * 384, a->n_bases * 3) + 65536;
  if (a->ext.cand_cap < cand_min) a->ext.cand_cap = cand_min;
  if (a->ext.cand_ops_cap < ops_min) a->ext.cand_ops_cap = ops_min;
  a->out.alns_cap = a->ext.cand_cap;
  a->out.ops_cap = a->ext.cand_ops_cap;
  HIPCHK(a, a->ext.cands.ensure(a->ext.cand_cap));
  HIPCHK(a, a->ext.order.ensure(a->ext.cand_cap * 2));
  HIPCHK(a, a->ext.heavy.ensure((a->ext.cand_cap / 2 + 16) * 2));
  HIPCHK(a, a->ext.rel.ensure(a->ext.cand_cap));
  HIPCHK(a, a->ext.ops.ensure(a->ext.cand_ops_cap, 64));
  HIPCHK(a, a->ext.nalns.ensure(n + 1));
  HIPCHK(a, a->ext.opbytes.ensure(n + 1));
  HIPCHK(a, a->ext.aln_off.ensure(n + 2));
  HIPCHK(a, a->ext.ops_off.ensure(n + 2));
  HIPCHK(a, a->out.alns.ensure(a->ext.cand_cap));
  // (a finished read's op bytes are not taken from the pool: 2 L at most per read on top of what the pool holds)
  HIPCHK(a, a->out.ops.ensure(a->ext.cand_ops_cap + 2 * a->n_bases, 64));
  HIPCHK(a, a->seed.heavy.ensure(n + 1));
  HIPCHK(a, a->seed.slow.ensure(n + 1));
  HIPCHK(a, a->seed.team.ensure(n + 1));

  // length classes for the run's options; lists for the extend stage
  const uint32_t mk_cap_slow = std::max<uint32_t>(a->ix->max_tx_exons, 1);
  const bool retry_possible = a->ix->max_tx_exons > (uint32_t)FAST_MAX_YCLIPS + 1;
  const ExtClasses cls = classify(a->len_hist, a->run_opts, mk_cap_slow);
  a->n_slow_host = cls.n_slow;
  a->fast_max_len = cls.fast_max;
  a->slow_max_len = cls.slow_max;
  // The finisher's op run (smem_finish.h): Match x H, Subst, Match x H at the front of the op pool, H = the longest read of
  // the fast class so far.  It is written when the finisher is wanted and the pool is new (growth, replay) or H grows.  Once
  // it exists, EVERY run on this aligner starts the pool's cursor behind it -- also a run without the finisher (both classes
  // switched off, the problem-parallel path, a batch without a read of the fast class) -- so nothing ever writes there.  The
  // one run that cannot keep it, a pool (test hook) too small to hold it, forgets it: it is written again when next wanted.
  const bool run_valid = a->ops_run_half > 0 && a->ops_run_ptr == a->ext.ops.get() && a->ops_run_cap == a->ext.ops.cap();
  if (!run_valid) a->ops_run_half = 0;
  const bool fin_wanted = !a->tpr.use_tpr && a->fin_classes && cls.fast_len > 0;
  if (fin_wanted && a->ops_run_half < cls.fast_len && fin::run_bytes(cls.fast_len) <= a->ext.cand_ops_cap) {
    HIPCHK(a, hipMemsetAsync(a->ext.ops, THM_OP_MATCH, fin::run_bytes(cls.fast_len), s));
    HIPCHK(a, hipMemsetAsync(a->ext.ops + cls.fast_len, THM_OP_SUBST, 1, s));
    a->ops_run_ptr = a->ext.ops.get();
    a->ops_run_cap = a->ext.ops.cap();
    a->ops_run_half = cls.fast_len;
  }
  if (a->ops_run_half && fin::run_bytes(a->ops_run_half) > a->ext.cand_ops_cap) a->ops_run_half = 0;  // this run writes over it
  const uint64_t ops_start = a->ops_run_half ? fin::run_bytes(a->ops_run_half) : 0;
  a->fin_run_classes = (fin_wanted && a->ops_run_half >= cls.fast_len) ? a->fin_classes : 0;
  // every launch of the extend stage: grids, scratch slices, counter rows (extend_plan.h)
  ExtendPlanIn pin;
  pin.n_reads = n;
  pin.n_cu = a->n_cu;
  pin.cls = cls;
  pin.mk_cap_slow = mk_cap_slow;
  pin.retry_possible = retry_possible;
  pin.waves_per_simd = extend_waves_per_simd(cells_per_lane(cls.fast_bw), a->dix->wide);
  pin.use_tpr = a->tpr.use_tpr;
  pin.dp_lds = extend_dp_lds_bytes(tpr_dp_x_cap(cls), tpr_dp_y_cap(cls));
  pin.dpt_lds = extend_dpt_lds_bytes(tpr_dpt_tcols(cls));
  pin.fin_classes = a->fin_run_classes;
  const ExtendPlan plan = plan_extend(pin);
  PlanParams pp;
  pp.offsets = a->reads.offsets;
  pp.read_hits = a->seed.hits;
  pp.n_reads = n;
  pp.fast_max_len = cls.fast_max;
  pp.slow_max_len = cls.slow_max;
  pp.heavy = a->seed.heavy;
  pp.slow = a->seed.slow;
  pp.team = a->seed.team;
  pp.team_ok = plan.team_ok ? 1u : 0u;
  pp.total_hits = a->seed.cand_off + n;
  pp.team_div = team_div_per_cu() * (uint32_t)std::max(a->n_cu, 1);
  pp.tpr_max_hits = plan.tpr_max_hits;
  pp.counts = a->s_work_counts;
  pp.read_status = a->reads.status;
  pp.read_n_alns = a->ext.nalns;
  pp.read_op_bytes = a->ext.opbytes;
  pp.ops_cursor = a->d_cursors + 1;
  pp.ops_start = ops_start;
  rc = a->dix->wide ? enqueue_plan_pack_t<uint64_t>(a, pp) : enqueue_plan_pack_t<uint32_t>(a, pp);
  if (rc != THM_OK) return rc;
  HIPCHK(a, hipEventRecord(a->ev[2], s));

  rc = a->dix->wide ? enqueue_extend_t<uint64_t>(a, plan) : enqueue_extend_t<uint32_t>(a, plan);
  if (rc != THM_OK) return rc;
  HIPCHK(a, hipEventRecord(a->ev[3], s));

  HIPCHK(a, launch_exclusive_scan2(a->ext.nalns, a->ext.opbytes, a->ext.aln_off,
                                   a->ext.ops_off, n, a->seed.scan_tmp, s));
  CompactParams cp;
  cp.n_reads = n;
  cp.read_cand_off = a->seed.cand_off;
  cp.cands = a->ext.cands;
  cp.order = a->ext.order;
  cp.cand_ops = a->ext.ops;
  cp.read_n_alns = a->ext.nalns;
  cp.read_aln_off = a->ext.aln_off;
  cp.read_ops_off = a->ext.ops_off;
  cp.read_offsets = a->reads.offsets;
  cp.alns = a->out.alns;
  cp.ops = a->out.ops;
  cp.fault = a->d_fault;
  cp.alns_cap = a->ext.cand_cap;
  cp.ops_cap = a->ext.cand_ops_cap + 2 * a->n_bases;
  // (a heavy read has more than 8 alignments and a descriptor stands for 4 of them: cand_cap / 2 entries hold either list)
  cp.heavy_cap = a->ext.cand_cap / 2 + 16;
  cp.heavy_cnt = a->d_cursors + 2;  // zeroed with the cursors when the batch starts
  cp.heavy_list = a->ext.heavy;
  cp.heavy_desc = a->ext.heavy + cp.heavy_cap;
  cp.rel = a->ext.rel;
  HIPCHK(a, launch_compact(cp, s));
  HIPCHK(a, hipEventRecord(a->ev[4], s));
  return THM_OK;
}

// host-visible status words of the last enqueue
struct RunStatus {
  int fault_seed = 0, fault_ext = 0;
  unsigned long long smem_used = 0, ops_used = 0, total_hits = 0;
};
int read_status(thm_aligner* a, RunStatus* st) {
  hipStream_t s = a->stream;
  int f[2] = {0, 0};
  unsigned long long cur[2] = {0, 0};
  HIPCHK(a, hipMemcpyAsync(f, a->d_fault, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipMemcpyAsync(cur, a->d_cursors, 16, hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipMemcpyAsync(&st->total_hits, a->seed.cand_off + a->n_reads, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipStreamSynchronize(s));
  st->fault_seed = f[0];
  st->fault_ext = f[1];
  st->smem_used = cur[0];
  st->ops_used = cur[1];
  return THM_OK;
}

template <class C>
int expand_mems_t(thm_aligner* a, uint64_t n) {
  ExpandParamsT<C> xp;
  xp.ix = dev_view<C>(a);
  xp.n_reads = n;
  xp.smems = a->seed.smems.as<SmemT<C>>();
  xp.read_smem_off = a->seed.off;
  xp.read_smem_cnt = a->seed.cnt;
  xp.read_mem_off = a->seed.cand_off;
  xp.mems = a->out.mems;
  HIPCHK(a, launch_expand(xp, a->stream));
  return THM_OK;
}

}  // namespace

int batch_length_classes(thm_aligner* a, const uint64_t* offsets, uint64_t n_reads) {
  if (n_reads >= 0xFFFFFFF0ull) return fail(a, THM_ERR_UNSUPPORTED, "more than 2^32-16 reads in one batch");
  if (offsets[0] != 0) return fail(a, THM_ERR_INVALID_ARG, "offsets[0] must be 0");
  // the lengths present in the batch (usually one or a handful): histogram by sorting the distinct ones
  uint32_t lmax = 0;
  uint64_t n_over = 0;
  a->len_hist.clear();
  {
    std::vector<uint64_t> cnt(1024, 0);
    std::vector<std::pair<uint32_t, uint64_t>> big;
    for (uint64_t i = 0; i < n_reads; i++) {
      if (offsets[i + 1] < offsets[i]) return fail(a, THM_ERR_INVALID_ARG, "read offsets are not monotone");
      const uint64_t L = offsets[i + 1] - offsets[i];
      if (L > MAX_READ_LEN) {  // the read gets its own status; the batch goes on
        n_over++;
        continue;
      }
      if (L < cnt.size())
        cnt[L]++;
      else
        big.emplace_back((uint32_t)L, 1);
      lmax = std::max<uint32_t>(lmax, (uint32_t)L);
    }
    for (uint32_t L = 0; L < cnt.size(); L++)
      if (cnt[L]) a->len_hist.emplace_back(L, cnt[L]);
    std::sort(big.begin(), big.end());
    for (const auto& b : big) {
      if (!a->len_hist.empty() && a->len_hist.back().first == b.first)
        a->len_hist.back().second++;
      else
        a->len_hist.push_back(b);
    }
  }
  a->n_over = n_over;
  a->n_reads = n_reads;
  a->n_bases = offsets[n_reads];
  a->max_read_len = lmax;
  return THM_OK;
}

int fetch_batch_sizes(thm_aligner* a, HArr<uint64_t>* h_off, const uint64_t* d_extra, uint64_t* extra, BatchSizes* z) {
  const uint64_t n = a->n_reads;
  hipStream_t s = a->stream;
  uint64_t w[2] = {0, 0}, n_contract = 0;
  uint64_t* sizes = w;  // alignments, op bytes
  if (h_off) {
    HIPCHK(a, h_off->ensure(n + 2));
    sizes = *h_off + n;
    HIPCHK(a, hipMemcpyAsync(*h_off, a->ext.aln_off, (n + 1) * 8, hipMemcpyDeviceToHost, s));
  } else {
    HIPCHK(a, hipMemcpyAsync(&sizes[0], a->ext.aln_off + n, 8, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(a, hipMemcpyAsync(&sizes[1], a->ext.ops_off + n, 8, hipMemcpyDeviceToHost, s));
  if (d_extra) HIPCHK(a, hipMemcpyAsync(extra, d_extra, 8, hipMemcpyDeviceToHost, s));
  // per-read statuses travel only when a read can have failed: reads beyond the classes are known to the host,
  // out-of-contract reads are counted by the device (the word behind the list counters)
  HIPCHK(a, hipMemcpyAsync(&n_contract, a->s_work_counts + 6, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipStreamSynchronize(s));
  z->n_alns = sizes[0];
  z->n_ops = sizes[1];
  if (z->n_alns > a->out.alns_cap || z->n_ops > a->out.ops_cap) return fail(a, THM_ERR_INTERNAL, "compacted batch exceeds its pools");
  uint64_t n_beyond = a->n_over;
  for (const auto& lc : a->len_hist)
    if (lc.first > a->slow_max_len) n_beyond += lc.second;
  z->any_failed = n_beyond || n_contract;
  return THM_OK;
}

int enqueue_statuses(thm_aligner* a, bool any_failed, HArr<int32_t>& h_stat) {
  if (!any_failed) return THM_OK;
  HIPCHK(a, h_stat.ensure(a->n_reads + 1));
  HIPCHK(a, hipMemcpyAsync(h_stat, a->reads.status, a->n_reads * 4, hipMemcpyDeviceToHost, a->stream));
  return THM_OK;
}

void failed_reads(const thm_aligner* a, bool any_failed, const HArr<int32_t>& h_stat, uint64_t* n_failed, const int32_t** status) {
  *n_failed = 0;
  *status = nullptr;
  if (!any_failed) return;
  const int32_t* st = h_stat;
  uint64_t bad = 0;
  for (uint64_t i = 0; i < a->n_reads; i++) bad += st[i] != THM_OK;
  *n_failed = bad;
  if (bad) *status = st;
}

CigarParams compacted_cigar_params(const thm_aligner* a, const BatchSizes& z) {
  CigarParams p;
  memset(&p, 0, sizeof p);
  p.ops = a->out.ops;
  p.ops_bytes = z.n_ops;
  p.n_streams = 2 * z.n_alns;
  p.alns = a->out.alns;
  return p;
}

extern "C" {

int32_t thm_batch_upload(thm_aligner* a, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads) {
  if (!a || !offsets || (!bases && n_reads && offsets[n_reads] > 0)) return THM_ERR_INVALID_ARG;
  HIPCHK(a, hipSetDevice(a->device));
  a->uploaded = a->ran = a->synced = false;
  a->bam.reads_named = false;  // (thm_batch_upload_reads sets it)
  const int rc = batch_length_classes(a, offsets, n_reads);
  if (rc != THM_OK) return rc;
  HIPCHK(a, a->reads.bases.ensure(a->n_bases, 64));
  HIPCHK(a, a->reads.offsets.ensure(n_reads + 1));
  if (a->n_bases) HIPCHK(a, hipMemcpyAsync(a->reads.bases, bases, a->n_bases, hipMemcpyHostToDevice, a->stream));
  HIPCHK(a, hipMemcpyAsync(a->reads.offsets, offsets, (n_reads + 1) * 8, hipMemcpyHostToDevice, a->stream));
  HIPCHK(a, hipStreamSynchronize(a->stream));
  a->uploaded = true;
  return THM_OK;
}

int32_t thm_batch_run(thm_aligner* a) {
  if (!a) return THM_ERR_INVALID_ARG;
  if (!a->uploaded) return fail(a, THM_ERR_INVALID_ARG, "thm_batch_run before thm_batch_upload");
  HIPCHK(a, hipSetDevice(a->device));
  a->ran = false;
  a->synced = false;
  a->run_opts = a->opts;  // a replay is this run again: under these, not under what set_opts brings later
  int rc = enqueue_run(a);
  if (rc == THM_OK) a->ran = true;
  return rc;
}

int32_t thm_batch_sync(thm_aligner* a) {
  if (!a) return THM_ERR_INVALID_ARG;
  if (!a->ran) return fail(a, THM_ERR_INVALID_ARG, "thm_batch_sync before thm_batch_run");
  if (a->synced) return THM_OK;
  HIPCHK(a, hipSetDevice(a->device));
  for (int attempt = 0; attempt < 6; attempt++) {
    RunStatus st;
    int rc = read_status(a, &st);
    if (rc != THM_OK) return rc;
    // a seed-pool overflow comes first: the extend kernel did not run on that attempt (its fault word means nothing)
    if (!st.fault_seed && (st.fault_ext & 2)) return fail(a, THM_ERR_INTERNAL, "extend kernel reported an internal inconsistency (fault word 0x%x)", st.fault_ext);
    const bool grow = st.fault_seed || (st.fault_ext & 1);
    if (!grow) {
      for (int k = 0; k < 4; k++) (void)elapsed_ms(a->ev[k], a->ev[k + 1], &a->timings[k]);
      (void)elapsed_ms(a->ev[0], a->ev[4], &a->timings[THM_T_TOTAL]);
      a->synced = true;
      return THM_OK;
    }
    // grow whatever overflowed and replay (counters of the failed attempt are discarded by the caller's reset)
    if (st.fault_seed) a->seed.smem_cap = std::max<uint64_t>(a->seed.smem_cap * 2, st.smem_used + 1024);
    if (st.total_hits > a->ext.cand_cap) a->ext.cand_cap = st.total_hits + st.total_hits / 8 + 1024;
    if (st.ops_used > a->ext.cand_ops_cap) a->ext.cand_ops_cap = st.ops_used + st.ops_used / 2 + 65536;
    if (a->ext.cand_cap * sizeof(Cand) > (160ull << 30))
      return fail(a, THM_ERR_OOM, "batch has %llu seed hits: candidate pool would exceed 160 GiB", st.total_hits);
    HIPCHK(a, hipMemcpyAsync(a->d_counters, a->d_counters + THM_N_COUNTERS, THM_N_COUNTERS * 8,
                             hipMemcpyDeviceToDevice, a->stream));
    a->n_replays++;
    rc = enqueue_run(a);
    if (rc != THM_OK) return rc;
  }
  return fail(a, THM_ERR_INTERNAL, "pools kept overflowing after 6 attempts");
}

int32_t thm_batch_fetch(thm_aligner* a, thm_batch_view* out) {
  if (!a || !out) return THM_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  int rc = thm_batch_sync(a);
  if (rc != THM_OK) return rc;
  const uint64_t n = a->n_reads;
  hipStream_t s = a->stream;
  BatchHost& h = a->out.host.next();  // the other set still backs the previous view
  BatchSizes z;  // offsets, and behind them the op-pool size, in one round trip
  rc = fetch_batch_sizes(a, &h.off, nullptr, nullptr, &z);
  if (rc != THM_OK) return rc;
  const uint64_t n_alns = z.n_alns, n_ops = z.n_ops;
  HIPCHK(a, h.alns.ensure(n_alns));
  HIPCHK(a, h.ops.ensure(n_ops));
  if (n_alns) HIPCHK(a, hipMemcpyAsync(h.alns, a->out.alns, n_alns * sizeof(thm_aln), hipMemcpyDeviceToHost, s));
  if (n_ops) HIPCHK(a, hipMemcpyAsync(h.ops, a->out.ops, n_ops, hipMemcpyDeviceToHost, s));
  rc = enqueue_statuses(a, z.any_failed, h.stat);
  if (rc != THM_OK) return rc;
  HIPCHK(a, hipStreamSynchronize(s));
  out->n_reads = n;
  out->n_alns = n_alns;
  out->n_op_bytes = n_ops;
  out->read_aln_off = h.off;
  out->alns = h.alns;
  out->ops = h.ops;
  failed_reads(a, z.any_failed, h.stat, &out->n_failed_reads, &out->read_status);
  return THM_OK;
}

int32_t thm_align_batch(thm_aligner* a, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads,
                        thm_batch_view* out) {
  int rc = thm_batch_upload(a, bases, offsets, n_reads);
  if (rc != THM_OK) return rc;
  rc = thm_batch_run(a);
  if (rc != THM_OK) return rc;
  return thm_batch_fetch(a, out);
}

int32_t thm_smems_batch(thm_aligner* a, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads,
                        uint64_t min_seed_len, thm_mems_view* out) {
  if (!a || !out) return THM_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  if (min_seed_len < 1 || min_seed_len > 65535) return fail(a, THM_ERR_INVALID_ARG, "min_seed_len out of range");
  int rc = thm_batch_upload(a, bases, offsets, n_reads);
  if (rc != THM_OK) return rc;
  const uint64_t n = n_reads;
  hipStream_t s = a->stream;
  RunStatus st;
  for (int attempt = 0;; attempt++) {
    // (the counters' snapshot is taken by the seed stage's first kernel; a replay starts from it)
    if (attempt > 0)
      HIPCHK(a, hipMemcpyAsync(a->d_counters, a->d_counters + THM_N_COUNTERS, THM_N_COUNTERS * 8,
                               hipMemcpyDeviceToDevice, s));
    rc = enqueue_seed(a, (uint32_t)min_seed_len, true);
    if (rc != THM_OK) return rc;
    rc = read_status(a, &st);
    if (rc != THM_OK) return rc;
    if (!st.fault_seed) break;
    if (attempt >= 6) return fail(a, THM_ERR_INTERNAL, "smem pool kept overflowing");
    a->n_replays++;
    a->seed.smem_cap = std::max<uint64_t>(a->seed.smem_cap * 2, st.smem_used + 1024);
  }
  a->uploaded = false;  // the seed-only pass leaves no aligned batch behind
  const uint64_t n_mems = st.total_hits;
  if (n_mems * sizeof(thm_mem) > (64ull << 30)) return fail(a, THM_ERR_OOM, "%llu seed hits in one batch", st.total_hits);
  HIPCHK(a, a->out.mems.ensure(n_mems, 64));
  rc = a->dix->wide ? expand_mems_t<uint64_t>(a, n) : expand_mems_t<uint32_t>(a, n);
  if (rc != THM_OK) return rc;
  a->h_off.assign(n + 1, 0);
  a->h_mems.resize(n_mems);
  HIPCHK(a, hipMemcpyAsync(a->h_off.data(), a->seed.cand_off, (n + 1) * 8, hipMemcpyDeviceToHost, s));
  if (n_mems) HIPCHK(a, hipMemcpyAsync(a->h_mems.data(), a->out.mems, n_mems * sizeof(thm_mem), hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipStreamSynchronize(s));
  out->n_reads = n;
  out->n_mems = n_mems;
  out->read_mem_off = a->h_off.data();
  out->mems = a->h_mems.data();
  return THM_OK;
}

}  // extern "C"
