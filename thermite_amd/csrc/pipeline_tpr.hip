// pipeline_tpr.hip -- host side of the opt-in problem-parallel path of the extend stage (THM_TPR=1; DESIGN.md section
// 4.6): extension problems as the unit of wavefront work (kernels_tpr.hip).  Hit summaries, then rounds of [control kernel,
// thread per read | the two DP kernels, thread and wave per request]; the reads with many hits take the wave-per-read and
// team kernels beside the rounds, and what the control kernel leaves takes one more wave-per-read launch behind them.
// Its buffers, streams and events are thm_aligner::tpr (aligner_internal.h); its grids and counter rows are the plan's.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "aligner_internal.h"

using namespace thm;

namespace {

template <class C>
int enqueue_tpr_rounds_t(thm_aligner* a, const ExtendPlan& plan, const ExtendParamsT<C>& ep) {
  const uint64_t n = a->n_reads;
  hipStream_t s = a->stream;
  TprState& t = a->tpr;
  const uint64_t rec_cap = std::min<uint64_t>(4 * n + 65536, 64ull << 20);
  HIPCHK(a, t.t_memos.ensure(n, 64));
  HIPCHK(a, t.t_recs.ensure(rec_cap, 64));
  HIPCHK(a, t.t_qlist.ensure((size_t)DP_NQ * rec_cap, 64));
  HIPCHK(a, t.t_act[0].ensure(n, 64));
  HIPCHK(a, t.t_act[1].ensure(n, 64));
  HIPCHK(a, t.t_bail.ensure(n + 1));
  HIPCHK(a, t.t_queue2.ensure(thm::QUEUE_BYTES / sizeof(unsigned int)));  // (a multiple of 16: aligner_internal.h)
  HIPCHK(a, hipMemsetAsync(t.t_queue2, 0, thm::QUEUE_BYTES, s));
  HIPCHK(a, t.t_ctl.ensure(TPRC_BYTES));
  HIPCHK(a, hipMemsetAsync(t.t_ctl.p, 0, TPRC_BYTES, s));
  unsigned long long* ctl = t.t_ctl.as<unsigned long long>();
  TprParamsT<C> tq;
  tq.recs_rw = a->ext.recs.as<ReadRecT<C>>();
  tq.memos = t.t_memos;
  tq.recs = t.t_recs;
  tq.rec_cap = rec_cap;
  tq.rec_cursor = ctl + TPRC_REC_CUR;
  tq.q_list = t.t_qlist;
  tq.q_stride = rec_cap;
  tq.q_cur = ctl + TPRC_Q_CUR;
  tq.bail = t.t_bail;
  tq.bail_count = ctl + TPRC_BAIL_CNT;
  tq.team = nullptr;  // (the team kernel is running already; a read of this path has fewer hits than it takes anyway)
  tq.team_count = nullptr;
  tq.max_hits = TPR_MAX_HITS;
  tq.dpt_cols = plan.dpt_tcols;
  tq.stats = ctl + TPRC_STATS;
  ExtendParamsT<C> zp = ep;
  zp.wave_counters = counter_rows(a, plan.row_tpr_ctl);
  DpParams dq;
  dq.recs = tq.recs;
  dq.q_list = tq.q_list;
  dq.q_stride = tq.q_stride;
  dq.q_cur = ctl + TPRC_Q_CUR;
  dq.q_done = ctl + TPRC_Q_DONE;
  dq.fault = ep.fault;
  dq.x_cap = plan.dp_x_cap;
  dq.y_cap = plan.dp_y_cap;
  {
    const size_t tb = extend_dp_trace_bytes(plan.dp_y_cap, plan.cpl);
    HIPCHK(a, t.t_trace.ensure((size_t)plan.dp_blocks * 4 * tb + 64));
    dq.trace_scratch = t.t_trace.as<unsigned long long>();
    dq.trace_per_wave = tb / 8;
    dq.tcols = plan.dpt_tcols;
  }
  // hit summaries: everything about a hit that does not depend on the state align_read carries, all hits side by side
  {
    const uint64_t slot_cap = a->ext.cand_cap;
    HIPCHK(a, t.t_hdr.ensure(slot_cap, 64));
    HIPCHK(a, t.t_sums.ensure(slot_cap, 64));
    HIPCHK(a, hipMemsetAsync(t.t_hdr, 0xFF, slot_cap * sizeof(HitHdr), s));
    HitParamsT<C> hq;
    hq.ix = ep.ix;
    hq.reads = ep.reads;
    hq.opts = ep.opts;
    hq.smems = ep.smems;
    hq.read_recs = ep.read_recs;
    hq.max_read_len = ep.max_read_len;
    hq.max_hits = TPR_MAX_HITS;
    hq.hdr = t.t_hdr;
    hq.sums = t.t_sums;
    hq.total_hits = a->seed.cand_off + n;
    hq.slot_cap = slot_cap;
    hq.fault_seed = a->d_fault;
    HIPCHK(a, launch_hit_expand(hq, s));
    HIPCHK(a, launch_hit_summaries(hq, a->n_cu * 12, s));
    tq.sums = t.t_sums;
  }
  // The reads with HEAVY_HITS hits and more (the lists of plan_kernel) are the wave-per-read / workgroup-per-read
  // kernels': they run BESIDE the rounds below, on their own streams.
  {
    ExtendParamsT<C> hp = ep;
    hp.skip_scan = 1;
    hp.team_limit = 16u * (uint32_t)a->n_cu;  // no scan of the batch to share the machine with: the team kernel keeps every read it can take
    HIPCHK(a, hipEventRecord(a->ev_fork, s));
    HIPCHK(a, hipStreamWaitEvent(a->stream2, a->ev_fork, 0));
    HIPCHK(a, hipStreamWaitEvent(t.stream3, a->ev_fork, 0));
    if (plan.team_ok) HIPCHK(a, launch_extend(team_params(a, plan, hp), plan.cpl, a->n_cu, a->stream2, true));
    HIPCHK(a, launch_extend(hp, plan.cpl, plan.bail_blocks, t.stream3));
    HIPCHK(a, hipEventRecord(a->ev_join, a->stream2));
    HIPCHK(a, hipEventRecord(t.ev_join3, t.stream3));
  }
  // round 0's list: the reads of this path by descending hit count
  HIPCHK(a, launch_tpr_order(a->ext.recs.as<ReadRecT<C>>(), n, ep.max_read_len, TPR_MAX_HITS, ctl + TPRC_BINS, t.t_act[0], ctl + TPRC_N_ACT,
                             a->d_fault, s));
  const int n_rounds = t.tpr_rounds;  // rounds of requests a read may take (then: the wave-per-read kernel)
  for (int r = 0; r <= n_rounds; r++) {
    tq.round = (uint32_t)r;
    tq.act_in = t.t_act[r & 1];
    tq.n_act_in = ctl + TPRC_N_ACT + r;
    tq.act_out = t.t_act[(r + 1) & 1];
    tq.n_act_out = ctl + TPRC_N_ACT + r + 1;
    tq.last_round = r == n_rounds ? 1u : 0u;
    HIPCHK(a, launch_extend_ctl(zp, tq, plan.ctl_blocks, s));
    if (r == n_rounds) break;
    dq.work = (unsigned int*)((uint8_t*)t.t_ctl.p + TPRC_WORK_BYTES + (size_t)r * 4 * 64);
    // the two DP kernels of a round side by side: the thread-per-problem one has a few hundred wavefronts of long
    // serial work (one column after the other, per thread), the wave-per-problem one fills the machine
    HIPCHK(a, hipEventRecord(t.ev_dpt_fork, s));
    HIPCHK(a, hipStreamWaitEvent(t.stream4, t.ev_dpt_fork, 0));
    HIPCHK(a, launch_extend_dpt(dq, plan.dpt_blocks, t.stream4));
    HIPCHK(a, hipEventRecord(t.ev_dpt_join, t.stream4));
    HIPCHK(a, launch_extend_dp(dq, plan.cpl, plan.dp_blocks, s));
    HIPCHK(a, hipStreamWaitEvent(s, t.ev_dpt_join, 0));
    HIPCHK(a, hipMemcpyAsync(ctl + TPRC_Q_DONE, ctl + TPRC_Q_CUR, DP_NQ * 8, hipMemcpyDeviceToDevice, s));
  }
  // what the control kernel left (capacities, rounds): one more wave-per-read launch over that list, behind the others
  HIPCHK(a, hipStreamWaitEvent(s, a->ev_join, 0));
  HIPCHK(a, hipStreamWaitEvent(s, t.ev_join3, 0));
  {
    ExtendParamsT<C> bp = ep;
    bp.skip_scan = 1;
    bp.heavy = t.t_bail;
    bp.heavy_count = ctl + TPRC_BAIL_CNT;
    bp.team = nullptr;
    bp.team_count = nullptr;
    bp.queue = t.t_queue2;
    bp.wave_counters = counter_rows(a, plan.row_tpr_bail);
    HIPCHK(a, launch_extend(bp, plan.cpl, plan.bail_blocks, s));
  }
  return THM_OK;
}

}  // namespace

int enqueue_tpr_rounds(thm_aligner* a, const ExtendPlan& plan, const ExtendParamsT<uint32_t>& base) { return enqueue_tpr_rounds_t(a, plan, base); }
int enqueue_tpr_rounds(thm_aligner* a, const ExtendPlan& plan, const ExtendParamsT<uint64_t>& base) { return enqueue_tpr_rounds_t(a, plan, base); }
