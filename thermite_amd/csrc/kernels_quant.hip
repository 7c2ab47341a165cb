// kernels_quant.hip -- the device side of the gene and junction count tables of a run (include/thermite_io.h:
// thm_quant_add; host side quant.hip; what one thread does with one alignment is quant_device.h).
//
//   count    grid-stride, one thread per alignment: its read by binary search (so NH, and a read with thousands of
//            alignments is thousands of independent lookups), the range checks, the number of its N words; then one thread
//            per read for the read totals.  The totals are summed in registers, per wavefront by shuffles, per workgroup in
//            LDS, and reach global memory as one add per total and workgroup.
//   extract  one thread per alignment with hits: the walk again, one row per hit at the place the scan gave it
//   gather   out[i] = in[perm[i]] (the high key words in the order of the first sort pass)
//   heads    over the sorted permutation: 1 where a key begins
//   reduce   by key: a segmented sum (and maximum) over the wavefront by shuffles -- rows of one key are neighbours --
//            then one integer atomic per key and wavefront, so a junction with 70 000 hits is some 1100 atomics
//   lookup   one thread per reduced row: binary search in the running table
//   update   found rows add into the table in place (keys of the reduced rows are distinct: plain stores), new rows go
//            behind the table's rows in the concatenation
//   genes    grid-stride, one thread per alignment.  Every workgroup keeps a direct-mapped, tagged cache of GENE_SLOTS
//            counters in LDS: a counter that owns its slot is summed there and flushed as one global add per slot; a
//            counter that meets a slot owned by another goes to global memory at once.  So 500 000 reads on chrM's 13
//            genes are a few adds per workgroup, and a table of 36 000 genes x 4 counters is as correct as a small one.
//   rows     the table as thm_quant_junction records for the copy to the host
// Integer atomics only: no result depends on the order of arrival.
#include <hip/hip_runtime.h>

#include "launch_io.h"
#include "quant_device.h"
#include "summary_tile.h"

namespace thm {
namespace dev {

using ull = unsigned long long;
constexpr uint32_t GENE_SLOTS = 2048;  // 16 KB of LDS: tags and counts
constexpr uint32_t NOT_FOUND = 0xFFFFFFFFu;

__device__ inline uint64_t shfl_down_u64(uint64_t v, int d) {
  const uint32_t lo = (uint32_t)__shfl_down((int)(uint32_t)v, d), hi = (uint32_t)__shfl_down((int)(uint32_t)(v >> 32), d);
  return (uint64_t)hi << 32 | lo;
}

// the words of alignment a, or false where they do not lie inside the pool
__device__ inline bool aln_words(const QuantBatch& b, const thm_aln_digest& d, const uint32_t** w) {
  if (d.cigar_off > b.n_words || (uint64_t)d.n_cigar > b.n_words - d.cigar_off) return false;
  *w = b.words + d.cigar_off;
  return true;
}

__global__ __launch_bounds__(256) void quant_count_kernel(const QuantCountParams p) {
  __shared__ ull sh_tot[quant::N_TOTALS];
  const QuantBatch& b = p.b;
  uint32_t t[quant::N_TOTALS];
  for (int k = 0; k < quant::N_TOTALS; k++) t[k] = 0;
  if (threadIdx.x < quant::N_TOTALS) sh_tot[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t stride = (uint64_t)gridDim.x * 256u, first = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  for (uint64_t a = first; a < b.n_alns; a += stride) {
    const uint64_t r = quant::read_of(b.aln_off, b.n_reads, a);
    const bool multi = b.aln_off[r + 1] - b.aln_off[r] > 1;
    const thm_aln& al = b.alns[a];
    const thm_aln_digest& d = b.digests[a];
    const uint32_t type = al.aln_type;
    const uint32_t c = quant::gene_counter(type, al.tx_or_gene_idx, multi, b.tx_gene, b.n_txs, b.n_genes);
    const uint32_t* w = nullptr;
    uint32_t n_hits = 0;
    bool ok = c != quant::BAD_INDEX && al.ref_id < b.n_refs && aln_words(b, d, &w);
    if (ok && b.ref_sq[al.ref_id] < 0) ok = false;
    if (ok) {
      if (d.flags & THM_DIGEST_LONG_RUN)
        t[quant::T_LONG_RUN]++;
      else
        n_hits = quant::count_hits(w, d.n_cigar);
      if (n_hits && type != THM_ALN_EXONIC) ok = false;  // (the strand of a hit is its transcript's)
    }
    if (!ok) {
      atomicMin(p.bad, (ull)a);
      n_hits = 0;
    }
    p.hit_cnt[a] = n_hits;
    p.multi[a] = multi ? 1 : 0;
    t[quant::T_ALNS]++;
    if (c == quant::NO_COUNTER) t[multi ? quant::T_INTERGENIC_MULTI : quant::T_INTERGENIC_UNIQUE]++;
    if (n_hits) {
      t[quant::T_SPLICED]++;
      t[quant::T_HITS] += n_hits;
    }
  }
  for (uint64_t r = first; r < b.n_reads; r += stride) {
    const uint64_t nh = b.aln_off[r + 1] - b.aln_off[r];
    t[quant::T_READS]++;
    if (b.status && b.status[r] != THM_OK)
      t[quant::T_FAILED]++;
    else if (nh == 0)
      t[quant::T_UNMAPPED]++;
    else
      t[nh == 1 ? quant::T_UNIQUE_READS : quant::T_MULTI_READS]++;
  }
  block_totals(t, sh_tot, p.totals);
}

struct HitWriter {
  const QuantRows& out;
  uint64_t at;
  uint32_t ref;
  bool forward, multi;
  __device__ void operator()(uint32_t k, const quant::Hit& h) const {
    const uint64_t i = at + k;
    out.hi[i] = quant::key_hi(ref, h.start);
    out.lo[i] = quant::key_lo(h.end, forward);
    out.n_unique[i] = multi ? 0 : 1;
    out.n_multi[i] = multi ? 1 : 0;
    out.overhang[i] = quant::overhang(h);
  }
};

__global__ __launch_bounds__(256) void quant_extract_kernel(const QuantExtractParams p) {
  const uint64_t a = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (a >= p.b.n_alns) return;
  const uint64_t at = p.hit_off[a], n = p.hit_off[a + 1] - at;
  if (n == 0) return;
  // (count has checked every index of an alignment it gave hits)
  const thm_aln& al = p.b.alns[a];
  const thm_aln_digest& d = p.b.digests[a];
  const HitWriter wr{p.out, at, (uint32_t)p.b.ref_sq[al.ref_id], p.b.tx_forward[al.tx_or_gene_idx] != 0, p.multi[a] != 0};
  (void)quant::walk(p.b.words + d.cigar_off, d.n_cigar, al.ystart, wr);
}

__global__ __launch_bounds__(256) void quant_genes_kernel(const QuantGenesParams p) {
  __shared__ uint32_t tag[GENE_SLOTS];  // counter + 1; 0: free
  __shared__ uint32_t cnt[GENE_SLOTS];
  for (uint32_t k = threadIdx.x; k < GENE_SLOTS; k += 256) tag[k] = 0, cnt[k] = 0;
  __syncthreads();
  const QuantBatch& b = p.b;
  const uint64_t stride = (uint64_t)gridDim.x * 256u;
  for (uint64_t a = (uint64_t)blockIdx.x * 256u + threadIdx.x; a < b.n_alns; a += stride) {
    const thm_aln& al = b.alns[a];
    const uint32_t c = quant::gene_counter(al.aln_type, al.tx_or_gene_idx, p.multi[a] != 0, b.tx_gene, b.n_txs, b.n_genes);
    if (c == quant::NO_COUNTER || c == quant::BAD_INDEX) continue;
    const uint32_t slot = c & (GENE_SLOTS - 1);
    const uint32_t was = atomicCAS(&tag[slot], 0u, c + 1);
    if (was == 0 || was == c + 1)
      atomicAdd(&cnt[slot], 1u);
    else
      atomicAdd(&p.genes[c], 1ull);
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < GENE_SLOTS; k += 256)
    if (tag[k] && cnt[k]) atomicAdd(&p.genes[tag[k] - 1], (ull)cnt[k]);
}

__global__ __launch_bounds__(256) void quant_gather_kernel(const uint64_t* in, const uint32_t* perm, uint64_t n, uint64_t* out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i < n) out[i] = in[perm[i]];
}

__global__ __launch_bounds__(256) void quant_heads_kernel(const QuantReduceParams p) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= p.n) return;
  p.flag[i] = i == 0 || p.s_hi[i] != p.s_hi[i - 1] || p.in.lo[p.perm[i]] != p.in.lo[p.perm[i - 1]] ? 1 : 0;
}

__global__ __launch_bounds__(256) void quant_reduce_kernel(const QuantReduceParams p) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  const bool in = i < p.n;
  // the key's row of the output; lanes past the end form a run of their own that nobody writes
  uint32_t seg = NOT_FOUND;
  uint64_t nu = 0, nm = 0;
  uint32_t ov = 0;
  bool head = false;
  uint32_t row = 0;
  if (in) {
    head = p.flag[i] != 0;
    seg = (uint32_t)(p.first[i] + (head ? 1 : 0) - 1);
    row = p.perm[i];
    nu = p.in.n_unique[row];
    nm = p.in.n_multi[row];
    ov = p.in.overhang[row];
  }
  // rows of one key are neighbours: after the step of distance d a lane holds the sum of its run's lanes [lane, lane + 2d)
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t s2 = (uint32_t)__shfl_down((int)seg, d);
    const uint64_t nu2 = shfl_down_u64(nu, d), nm2 = shfl_down_u64(nm, d);
    const uint32_t ov2 = (uint32_t)__shfl_down((int)ov, d);
    if (lane + d < 64 && s2 == seg) {
      nu += nu2;
      nm += nm2;
      ov = ov2 > ov ? ov2 : ov;
    }
  }
  const uint32_t before = (uint32_t)__shfl_up((int)seg, 1);
  if (!in) return;
  if (lane == 0 || before != seg) {  // the run's first lane in this wavefront
    if (nu) atomicAdd((ull*)&p.out.n_unique[seg], (ull)nu);
    if (nm) atomicAdd((ull*)&p.out.n_multi[seg], (ull)nm);
    if (ov) atomicMax(&p.out.overhang[seg], ov);
  }
  if (head) {
    p.out.hi[seg] = p.s_hi[i];
    p.out.lo[seg] = p.in.lo[row];
  }
}

__global__ __launch_bounds__(256) void quant_lookup_kernel(const QuantMergeParams p) {
  const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (j >= p.n_red) return;
  const uint64_t hi = p.red.hi[j], lo = p.red.lo[j];
  // the first row of the table that is not below (hi, lo)
  uint64_t a = 0, z = p.n_tab;
  while (a < z) {
    const uint64_t mid = (a + z) >> 1;
    const uint64_t mh = p.tab.hi[mid];
    if (mh < hi || (mh == hi && p.tab.lo[mid] < lo))
      a = mid + 1;
    else
      z = mid;
  }
  const bool found = a < p.n_tab && p.tab.hi[a] == hi && p.tab.lo[a] == lo;
  p.where[j] = found ? (uint32_t)a : NOT_FOUND;
  p.is_new[j] = found ? 0 : 1;
}

__global__ __launch_bounds__(256) void quant_update_kernel(const QuantMergeParams p) {
  const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (j >= p.n_red) return;
  const uint32_t w = p.where[j];
  const uint64_t nu = p.red.n_unique[j], nm = p.red.n_multi[j];
  const uint32_t ov = p.red.overhang[j];
  if (w != NOT_FOUND) {
    p.tab.n_unique[w] += nu;
    p.tab.n_multi[w] += nm;
    if (ov > p.tab.overhang[w]) p.tab.overhang[w] = ov;
  } else {
    const uint64_t at = p.n_tab + p.new_at[j];
    p.cat.hi[at] = p.red.hi[j];
    p.cat.lo[at] = p.red.lo[j];
    p.cat.n_unique[at] = nu;
    p.cat.n_multi[at] = nm;
    p.cat.overhang[at] = ov;
  }
}

__global__ __launch_bounds__(256) void quant_rows_kernel(const QuantRows in, uint64_t n, thm_quant_junction* out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i < n) out[i] = quant::row(in.hi[i], in.lo[i], in.n_unique[i], in.n_multi[i], in.overhang[i]);
}

}  // namespace dev

// grid-stride kernels: enough workgroups to fill the device, few enough that each sums many items before its atomics
static unsigned quant_grid(uint64_t n, int n_cu) {
  const uint64_t need = (n + 255) / 256, cap = (uint64_t)(n_cu > 0 ? n_cu : 256) * 8;
  return (unsigned)(need < cap ? (need ? need : 1) : cap);
}

hipError_t launch_quant_count(const QuantCountParams& p, int n_cu, hipStream_t s) {
  const uint64_t n = p.b.n_alns > p.b.n_reads ? p.b.n_alns : p.b.n_reads;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::quant_count_kernel, dim3(quant_grid(n, n_cu)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_quant_extract(const QuantExtractParams& p, hipStream_t s) {
  if (p.b.n_alns == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::quant_extract_kernel, dim3(blocks256(p.b.n_alns)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_quant_genes(const QuantGenesParams& p, int n_cu, hipStream_t s) {
  if (p.b.n_alns == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::quant_genes_kernel, dim3(quant_grid(p.b.n_alns, n_cu)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_quant_gather(const uint64_t* in, const uint32_t* perm, uint64_t n, uint64_t* out, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::quant_gather_kernel, dim3(blocks256(n)), dim3(256), 0, s, in, perm, n, out);
  return hipGetLastError();
}
hipError_t launch_quant_heads(const QuantReduceParams& p, hipStream_t s) {
  if (p.n == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::quant_heads_kernel, dim3(blocks256(p.n)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_quant_reduce(const QuantReduceParams& p, hipStream_t s) {
  if (p.n == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::quant_reduce_kernel, dim3(blocks256(p.n)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_quant_lookup(const QuantMergeParams& p, hipStream_t s) {
  if (p.n_red == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::quant_lookup_kernel, dim3(blocks256(p.n_red)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_quant_update(const QuantMergeParams& p, hipStream_t s) {
  if (p.n_red == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::quant_update_kernel, dim3(blocks256(p.n_red)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_quant_rows(const QuantRows& in, uint64_t n, thm_quant_junction* out, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::quant_rows_kernel, dim3(blocks256(n)), dim3(256), 0, s, in, n, out);
  return hipGetLastError();
}

}  // namespace thm
