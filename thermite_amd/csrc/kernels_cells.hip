// kernels_cells.hip -- the device side of the cell-by-gene UMI count matrix of a run (include/thermite_io.h:
// thm_cells_add / _fetch; host side cells.hip; what one thread does with one read, the tag and the key are
// cells_device.h).
//
//   classify  grid-stride, one thread per read: status, NH and the annotation of its one alignment decide its class; only
//             a read that is still a candidate then has its name looked at -- the scan for the first space, the tag
//             behind it -- and gets a key and a flag.  Byte loads inside the read's own name, so nothing outside
//             [name_off[0], name_off[n]) is read.  The names of a wavefront's 64 reads are neighbours in the pool, some
//             2 to 4 KB that its lanes walk side by side: every line fetched is used by the lanes around (DESIGN.md
//             4.21 has why this is not a lane group per read).  The totals are summed in registers, per wavefront by
//             shuffles, per workgroup in LDS, and reach global memory as one add per total and workgroup.
//   compact   the keys of the counted reads to the places the scan of the flags gave them
//   heads     over the sorted rows: 1 where a molecule begins
//   head_at   where every molecule begins, by the scan of the heads
//   reduce    one thread per molecule: its key, and its reads -- the length of its run where every row is one read, the
//             sum of the rows' counts where table and pending rows are merged (a run then has at most one row of the table
//             and one per pending batch)
//   levels    over the table: 1 where a barcode begins, 1 where a (barcode, gene) begins, the row's reads as 64 bits
//   starts    where every barcode and every (barcode, gene) begins, by the scans of those flags
//   barcodes  one thread per barcode: its molecules are its rows; kept or not; the entries it brings
//   rows      one thread per barcode writes its cell, one per (barcode, gene) its entry, both at the numbers the scans
//             over the kept ones gave; sums of reads are differences of the scan of the rows' reads
// No atomics but the totals' and the first bad alignment's, all integer: no result depends on the order of arrival.
#include <hip/hip_runtime.h>

#include "cells_device.h"
#include "launch_io.h"
#include "summary_tile.h"

namespace thm {
namespace dev {

using ull = unsigned long long;

__global__ __launch_bounds__(256) void cells_classify_kernel(const CellsClassifyParams p) {
  __shared__ ull sh_tot[cells::N_TOTALS];
  const CellsBatch& b = p.b;
  uint32_t t[cells::N_TOTALS];
  for (int k = 0; k < cells::N_TOTALS; k++) t[k] = 0;
  if (threadIdx.x < cells::N_TOTALS) sh_tot[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t stride = (uint64_t)gridDim.x * 256u;
  for (uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x; r < b.n_reads; r += stride) {
    const uint64_t a0 = b.aln_off[r], nh = b.aln_off[r + 1] - a0;
    const bool ok = !b.status || b.status[r] == THM_OK;
    uint32_t gene = 0;
    // (offsets that ascend and end at n_alns have a0 < n_alns wherever nh >= 1; others are refused like a bad index)
    int c = nh == 1 && a0 >= b.n_alns ? (int)cells::BAD_INDEX
                                      : cells::class_before_tag(ok, nh, b.alns + a0, b.flags, b.tx_gene, b.n_txs, b.n_genes, &gene);
    if (c == cells::BAD_INDEX) {
      atomicMin(p.bad, (ull)a0);
      c = cells::T_UNTAGGED;  // (the call is refused: no total of it is used)
    } else if (c == cells::T_COUNTED) {
      const uint64_t nb = b.name_off[r], ne = b.name_off[r + 1];
      uint32_t bc = 0, umi = 0;
      if (ne >= nb && cells::parse_tag(b.names, nb, cells::qname_end(b.names, nb, ne), b.cb_len, b.umi_len, &bc, &umi)) {
        p.hc[r] = cells::key_hc(bc, 1u);
        p.lo[r] = cells::key_lo(gene, umi, b.umi_len);
      } else {
        c = cells::T_UNTAGGED;
      }
    }
    p.counted[r] = c == cells::T_COUNTED ? 1 : 0;
    t[cells::T_READS]++;
    t[c]++;
  }
  block_totals(t, sh_tot, p.totals);
}

__global__ __launch_bounds__(256) void cells_compact_kernel(const CellsCompactParams p) {
  const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (r >= p.n_reads || !p.counted[r]) return;
  const uint64_t at = p.at[r];
  p.out_hc[at] = p.hc[r];
  p.out_lo[at] = p.lo[r];
}

__global__ __launch_bounds__(256) void cells_heads_kernel(const CellsReduceParams p) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= p.n) return;
  p.flag[i] = i == 0 || !cells::same_molecule(p.hc[i], p.lo[i], p.hc[i - 1], p.lo[i - 1]) ? 1 : 0;
}

__global__ __launch_bounds__(256) void cells_head_at_kernel(const CellsReduceParams p) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i > p.n) return;
  if (i == p.n)
    p.head_at[p.n_keys] = p.n;
  else if (p.flag[i])
    p.head_at[p.first[i]] = i;
}

__global__ __launch_bounds__(256) void cells_reduce_kernel(const CellsReduceParams p) {
  const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (k >= p.n_keys) return;
  const uint64_t s = p.head_at[k], e = p.head_at[k + 1];
  uint64_t cnt = e - s;
  if (!p.unit) {
    cnt = 0;
    for (uint64_t i = s; i < e; i++) cnt += cells::count_of(p.hc[i]);
  }
  // (thm_cells_add keeps the object's reads at 2^32 - 1 or fewer: a molecule's count fits)
  p.out_hc[k] = cells::key_hc(cells::barcode_of(p.hc[s]), (uint32_t)cnt);
  p.out_lo[k] = p.lo[s];
}

__global__ __launch_bounds__(256) void cells_levels_kernel(const CellsFetchParams p) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= p.n) return;
  const uint64_t hc = p.hc[i];
  const bool bhead = i == 0 || cells::barcode_of(hc) != cells::barcode_of(p.hc[i - 1]);
  const bool ehead = bhead || cells::gene_of(p.lo[i], p.umi_len) != cells::gene_of(p.lo[i - 1], p.umi_len);
  p.bflag[i] = bhead ? 1 : 0;
  p.eflag[i] = ehead ? 1 : 0;
  p.cnt[i] = cells::count_of(hc);
}

__global__ __launch_bounds__(256) void cells_starts_kernel(const CellsFetchParams p) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i > p.n) return;
  if (i == p.n) {
    p.bc_start[p.n_barcodes] = p.n;
    p.ent_start[p.n_all_entries] = p.n;
    return;
  }
  if (p.bflag[i]) p.bc_start[p.b_at[i]] = i;
  if (p.eflag[i]) p.ent_start[p.e_at[i]] = i;
}

__global__ __launch_bounds__(256) void cells_barcodes_kernel(const CellsFetchParams p) {
  const uint64_t b = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (b >= p.n_barcodes) return;
  const uint64_t s = p.bc_start[b], e = p.bc_start[b + 1];
  const bool keep = e - s >= p.min_umis;
  p.keep[b] = keep ? 1 : 0;
  p.kept_entries[b] = keep ? p.e_at[e] - p.e_at[s] : 0;
}

// threads [0, n_all_entries): an entry each; threads behind them: a barcode each
__global__ __launch_bounds__(256) void cells_rows_kernel(const CellsFetchParams p) {
  const uint64_t x = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (x < p.n_all_entries) {
    const uint64_t s = p.ent_start[x], z = p.ent_start[x + 1];
    const uint64_t b = p.b_at[s] + p.bflag[s] - 1;  // the barcode that holds row s
    if (!p.keep[b]) return;
    thm_cell_entry en;
    en.cell = (uint32_t)p.cell_at[b];
    en.gene = cells::gene_of(p.lo[s], p.umi_len);
    en.n_umis = (uint32_t)(z - s);
    en.n_reads = (uint32_t)(p.pre[z] - p.pre[s]);
    p.entries[p.ent_at[b] + (x - p.e_at[p.bc_start[b]])] = en;
    return;
  }
  const uint64_t b = x - p.n_all_entries;
  if (b >= p.n_barcodes || !p.keep[b]) return;
  const uint64_t s = p.bc_start[b], e = p.bc_start[b + 1];
  thm_cell c;
  c.n_reads = p.pre[e] - p.pre[s];
  c.barcode = cells::barcode_of(p.hc[s]);
  c.n_umis = (uint32_t)(e - s);
  c.n_genes = (uint32_t)(p.e_at[e] - p.e_at[s]);
  c.pad_ = 0;
  p.cells[p.cell_at[b]] = c;
}

}  // namespace dev

// grid-stride: enough workgroups to fill the device, few enough that each sums many reads before its atomics
static unsigned cells_grid(uint64_t n, int n_cu) {
  const uint64_t need = (n + 255) / 256, cap = (uint64_t)(n_cu > 0 ? n_cu : 256) * 8;
  return (unsigned)(need < cap ? (need ? need : 1) : cap);
}

hipError_t launch_cells_classify(const CellsClassifyParams& p, int n_cu, hipStream_t s) {
  if (p.b.n_reads == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::cells_classify_kernel, dim3(cells_grid(p.b.n_reads, n_cu)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_cells_compact(const CellsCompactParams& p, hipStream_t s) {
  if (p.n_reads == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::cells_compact_kernel, dim3(blocks256(p.n_reads)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_cells_heads(const CellsReduceParams& p, hipStream_t s) {
  if (p.n == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::cells_heads_kernel, dim3(blocks256(p.n)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_cells_head_at(const CellsReduceParams& p, hipStream_t s) {
  if (p.n == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::cells_head_at_kernel, dim3(blocks256(p.n + 1)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_cells_reduce(const CellsReduceParams& p, hipStream_t s) {
  if (p.n_keys == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::cells_reduce_kernel, dim3(blocks256(p.n_keys)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_cells_levels(const CellsFetchParams& p, hipStream_t s) {
  if (p.n == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::cells_levels_kernel, dim3(blocks256(p.n)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_cells_starts(const CellsFetchParams& p, hipStream_t s) {
  if (p.n == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::cells_starts_kernel, dim3(blocks256(p.n + 1)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_cells_barcodes(const CellsFetchParams& p, hipStream_t s) {
  if (p.n_barcodes == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::cells_barcodes_kernel, dim3(blocks256(p.n_barcodes)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_cells_rows(const CellsFetchParams& p, hipStream_t s) {
  if (p.n_barcodes == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::cells_rows_kernel, dim3(blocks256(p.n_all_entries + p.n_barcodes)), dim3(256), 0, s, p);
  return hipGetLastError();
}

}  // namespace thm
