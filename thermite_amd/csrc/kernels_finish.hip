// kernels_finish.hip -- the finisher: one thread per read, behind plan_pack_kernel and in front of the wave-per-read
// extend kernel.  A read whose SMEMs decide its whole result (smem_finish.h: class E, class S) gets what extend_kernel's
// final section writes for a read with at most one alignment -- the candidate, order[0], read_n_alns, read_op_bytes -- and
// its record's len set to fin::MARK, which extend_kernel passes over with the test it already makes for reads of other
// classes (rec.len > max_read_len).  Everything else is left exactly as it was.  The op streams are windows of the run at
// the front of the op pool (pipeline.hip writes it): no op byte is written here.
//
// Counters: a workgroup sums what its reads add and leaves the sums in its own row of the extend stage's counter rows
// (plain stores, only non-zero words: the rows stay all zero between runs, launch_counters_reduce zeroes what it read).
// The per-class counts of thm_debug_smem_finish_stats go to the workgroup's row of `stats` (four words, always written).
#include <hip/hip_runtime.h>

#include "launch.h"
#include "smem_finish.h"

namespace thm {
namespace dev {

constexpr int FIN_SLOTS = THM_N_COUNTERS + 4;

template <class C>
__global__ __launch_bounds__(256) void smem_finish_kernel(FinishParamsT<C> p) {
  __shared__ unsigned long long part[FIN_SLOTS];
  // SMEM pool overflow in the seed stage: the SMEM runs are incomplete, nothing of them may be read (the batch is replayed)
  // (the workgroup's statistics row is zeroed on the way: thm_debug_smem_finish_stats never sums rows of an earlier batch)
  if (*p.fault_seed != 0) {
    if (threadIdx.x < 4) p.stats[(size_t)blockIdx.x * 4 + threadIdx.x] = 0;
    return;
  }
  if (threadIdx.x < FIN_SLOTS) part[threadIdx.x] = 0;
  __syncthreads();
  fin::Tables<C> tb;
  tb.ref_bin = p.ix.ref_bin;
  tb.ref_recs = p.ix.ref_recs;
  tb.n_refs = p.ix.n_refs;
  tb.exon_grid_off = p.ix.exon_grid_off;
  tb.exon_grid = p.ix.exon_grid;
  tb.gene_grid_off = p.ix.gene_grid_off;
  tb.gene_grid = p.ix.gene_grid;
  // per thread: reads, aligned, alns, the three types, calls, op bytes, window bytes; finished / left per class
  unsigned k_reads = 0, k_alns = 0, k_type[3] = {0, 0, 0}, k_calls = 0, k_opb = 0, k_win = 0, k_st[4] = {0, 0, 0, 0};
  const uint64_t n = p.reads.n_reads, step = (uint64_t)gridDim.x * 256;
  for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += step) {
    const ReadRecT<C> rec = p.recs[r];
    if (rec.len == 0 || rec.len > p.max_read_len) continue;          // not the fast class's
    if (rec.cand_off + (uint64_t)rec.n_hits > p.cand_cap) continue;  // candidate pool too small: extend_kernel raises the fault
    const int L = (int)rec.len;
    const uint64_t occ0 = (uint64_t)(rec.hi0 - rec.lo0);
    fin::Outcome o;
    o.what = fin::LEAVE;
    o.shape = fin::SHAPE_NONE;
    if ((p.classes & fin::CLASS_E) && fin::shape_exact(rec.smem_cnt, rec.n_hits, rec.qpos0, rec.len0, occ0, rec.len)) {
      o = fin::finish_exact<C>(tb, rec.sa0, L, fin::setup(p.opts, L, p.max_bw, (int)p.cpl), p.run_half);
    } else if ((p.classes & fin::CLASS_S) && rec.smem_cnt == 2 && rec.n_hits == 2 && occ0 == 1) {
      const SmemT<C> s1 = p.smems[rec.smem_off + 1];
      if (s1.hi > s1.lo && s1.hi - s1.lo == 1) {
        fin::Hit<C> h1, h2;
        h1.hr = rec.sa0;
        h1.q = rec.qpos0;
        h1.len = rec.len0;
        h2.hr = p.ix.sa[s1.hi - 1];
        h2.q = s1.qpos;
        h2.len = s1.len;
        int sp = 0;
        C a0 = 0;
        if (fin::shape_subst<C>(rec.smem_cnt, rec.n_hits, 1, 1, h1, h2, rec.len, sp, a0))
          o = fin::finish_subst<C>(tb, p.reads.bases + rec.base_off, h1, h2, L, sp, a0, fin::setup(p.opts, L, p.max_bw, (int)p.cpl), p.run_half);
      }
    }
    if (o.shape != fin::SHAPE_NONE) k_st[2 * (o.shape - 1) + (o.what == fin::FINISHED ? 0 : 1)]++;
    if (o.what != fin::FINISHED) continue;
    if (o.accepted) {
      Cand cd;
      cd.ystart = o.ystart;
      cd.yend = o.yend;
      cd.ylen = o.ylen;
      cd.tx_ystart = o.tx_ystart;
      cd.tx_yend = o.tx_yend;
      cd.tx_ylen = o.tx_ylen;
      cd.ops_off = o.ops_off;
      cd.tx_ops_off = o.tx_ops_off;
      cd.score = o.score;
      cd.ref_id = o.ref_id;
      cd.xstart = 0;
      cd.xend = rec.len;
      cd.ops_len = rec.len;
      const bool exonic = o.aln_type == THM_ALN_EXONIC;
      cd.tx_ops_len = exonic ? rec.len : 0u;
      cd.tx_or_gene_idx = o.type_idx;
      cd.tx_score = exonic ? o.score : 0;
      cd.tx_xstart = 0;
      cd.tx_xend = exonic ? rec.len : 0u;
      cd.name_rank = o.name_rank;
      cd.strand = o.strand;
      cd.aln_type = o.aln_type;
      cd.primary = 0;
      cd.pad_ = 0;
      p.cands[rec.cand_off] = cd;
      p.order[2 * rec.cand_off] = 0;
      k_alns++;
      k_type[0] += o.aln_type == THM_ALN_EXONIC;
      k_type[1] += o.aln_type == THM_ALN_INTRONIC;
      k_type[2] += o.aln_type == THM_ALN_INTERGENIC;
      k_opb += o.op_bytes;
    }
    p.read_n_alns[r] = (uint32_t)o.accepted;
    p.read_op_bytes[r] = o.accepted ? (uint64_t)o.op_bytes : 0ull;
    p.recs[r].len = fin::MARK;
    k_reads++;
    k_calls += o.calls;
    k_win += o.window_bytes;
  }
  // workgroup sums: wave reduction, one LDS atomic per wave and word
  unsigned v[11] = {k_reads, k_alns, k_type[0], k_type[1], k_type[2], k_calls, k_opb, k_win, k_st[0], k_st[1], k_st[2]};
  unsigned v11 = k_st[3];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < 11; k++) v[k] += __shfl_xor(v[k], o);
    v11 += __shfl_xor(v11, o);
  }
  if ((threadIdx.x & 63u) == 0) {
    const int slot[11] = {THM_CNT_READS, THM_CNT_ALNS, THM_CNT_EXONIC, THM_CNT_INTRONIC, THM_CNT_INTERGENIC, THM_CNT_SWG_CALLS,
                          THM_CNT_OP_BYTES, THM_CNT_WINDOW_BYTES, THM_N_COUNTERS + 0, THM_N_COUNTERS + 1, THM_N_COUNTERS + 2};
#pragma unroll
    for (int k = 0; k < 11; k++)
      if (v[k]) atomicAdd(&part[slot[k]], (unsigned long long)v[k]);
    if (v11) atomicAdd(&part[THM_N_COUNTERS + 3], (unsigned long long)v11);
  }
  __syncthreads();
  if (threadIdx.x < THM_N_COUNTERS) {
    unsigned long long w = part[threadIdx.x];
    // a finished read has 0 or 1 alignments: aligned = alns, unmapped = reads - alns
    if (threadIdx.x == THM_CNT_ALIGNED) w = part[THM_CNT_ALNS];
    if (threadIdx.x == THM_CNT_UNMAPPED) w = part[THM_CNT_READS] - part[THM_CNT_ALNS];
    if (w) p.rows[(size_t)blockIdx.x * THM_N_COUNTERS + threadIdx.x] = w;
  } else if (threadIdx.x < FIN_SLOTS) {
    p.stats[(size_t)blockIdx.x * 4 + (threadIdx.x - THM_N_COUNTERS)] = part[threadIdx.x];
  }
}

}  // namespace dev

template <class C>
static hipError_t launch_smem_finish_t(const FinishParamsT<C>& p, int n_blocks, hipStream_t s) {
  if (n_blocks <= 0 || p.reads.n_reads == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::smem_finish_kernel<C>, dim3((unsigned)n_blocks), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_smem_finish(const FinishParamsT<uint32_t>& p, int n_blocks, hipStream_t s) { return launch_smem_finish_t(p, n_blocks, s); }
hipError_t launch_smem_finish(const FinishParamsT<uint64_t>& p, int n_blocks, hipStream_t s) { return launch_smem_finish_t(p, n_blocks, s); }

}  // namespace thm
