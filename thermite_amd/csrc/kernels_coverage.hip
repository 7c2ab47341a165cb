// kernels_coverage.hip -- the device side of the per-base coverage tracks of a run (include/thermite_io.h:
// thm_coverage_add / _fetch / _depth; host side coverage.hip; what one thread does with one item, and the layout of the
// difference arrays, is coverage_device.h).
//
//   count    grid-stride, one thread per alignment: its read by binary search (so NH), its track, the checks that keep
//            every add inside the arrays, its blocks and bases; then one thread per read for the read totals.  The totals
//            are summed in registers, per wavefront by shuffles, per workgroup in LDS, and reach global memory as one add
//            per total and workgroup.  Nothing of the arrays is touched: after this pass the call can still refuse.
//   deposit  one thread per alignment with a track: the walk again, diff[s] += 1 and diff[e] -= 1 (mod 2^32) per block.
//            Integer atomics without a return value: no result depends on the order of arrival.
//   tiles    one workgroup per tile of cov::TILE entries of the range: the sum of its entries and how many are not 0
//   points   one workgroup per tile, the tile through LDS: every thread sums its PER_THREAD consecutive entries, a scan
//            over the workgroup plus the tile's carry gives the depth in front of each thread, and the thread writes
//            (entry, depth) for each of its non-zero entries -- the change points -- at the place the scans gave it
//   runs     one thread per change point: with a depth, it and its successor are a run
//   window   points' tile pass again for the tiles of a window, the depths written back through LDS
// The depth of the whole genome exists nowhere: a tile's depths live in registers and LDS while its workgroup runs.
#include <hip/hip_runtime.h>

#include "coverage_device.h"
#include "launch_io.h"
#include "summary_tile.h"

namespace thm {
namespace dev {

using ull = unsigned long long;
__global__ __launch_bounds__(256) void cov_count_kernel(const CovCountParams p) {
  __shared__ ull sh_tot[cov::N_TOTALS];
  const CovBatch& b = p.b;
  uint64_t t[cov::N_TOTALS];
  for (int k = 0; k < cov::N_TOTALS; k++) t[k] = 0;
  if (threadIdx.x < cov::N_TOTALS) sh_tot[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t stride = (uint64_t)gridDim.x * 256u, first = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  for (uint64_t a = first; a < b.n_alns; a += stride) {
    const uint64_t r = quant::read_of(b.aln_off, b.n_reads, a);
    const bool multi = b.aln_off[r + 1] - b.aln_off[r] > 1;
    const thm_aln& al = b.alns[a];
    const thm_aln_digest& d = b.digests[a];
    const bool long_run = (d.flags & THM_DIGEST_LONG_RUN) != 0;
    uint32_t track = cov::track_of(b.flags, multi, al.strand == 1);
    uint32_t sq = 0, n_blocks = 0;
    uint64_t bases = 0;
    if (!cov::check_aln(al.ref_id, al.ystart, d.cigar_off, d.n_cigar, long_run, b.words, b.n_words, b.ref_sq, b.n_refs, b.base, b.n_sq, &sq, &n_blocks,
                        &bases)) {
      atomicMin(p.bad, (ull)a);
      track = cov::NO_TRACK;
    }
    t[cov::T_ALNS]++;
    if (track == cov::NO_TRACK) {
      t[cov::T_SKIPPED_MULTI]++;
    } else if (long_run) {
      t[cov::T_LONG_RUN]++;
      track = cov::NO_TRACK;
    } else {
      // (the index is static in every statement: the totals stay in registers)
      for (uint32_t k = 0; k < cov::MAX_TRACKS; k++) {
        const bool mine = track == k;
        t[cov::T_TRACK0 + 3 * k] += mine ? 1u : 0u;
        t[cov::T_TRACK0 + 3 * k + 1] += mine ? n_blocks : 0u;
        t[cov::T_TRACK0 + 3 * k + 2] += mine ? bases : 0u;
      }
    }
    p.track[a] = (uint8_t)track;
  }
  read_totals(b, t[cov::T_READS], t[cov::T_FAILED]);
  block_totals(t, sh_tot, p.totals);
}

__global__ __launch_bounds__(256) void cov_deposit_kernel(const CovDepositParams p) {
  const uint64_t a = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (a >= p.b.n_alns) return;
  const uint32_t track = p.track[a];
  if (track == cov::NO_TRACK) return;
  // (count has checked the ref, the words and the walk's end of every alignment it gave a track)
  const thm_aln& al = p.b.alns[a];
  const thm_aln_digest& d = p.b.digests[a];
  const uint64_t at = p.b.base[p.b.ref_sq[al.ref_id]];
  uint64_t end = 0;
  (void)cov::walk_blocks(p.b.words + d.cigar_off, d.n_cigar, al.ystart, BlockAdder{p.diff + (uint64_t)track * p.track_entries + at}, &end);
}

__global__ __launch_bounds__(256) void cov_tiles_kernel(const CovTileParams p) {
  __shared__ uint32_t sh[8];
  const uint64_t t0 = (uint64_t)blockIdx.x * cov::TILE;
  uint32_t sum = 0, cnt = 0;
  for (uint32_t k = 0; k < cov::PER_THREAD; k++) {
    const uint64_t x = t0 + k * 256u + threadIdx.x;
    const uint32_t v = x < p.n ? p.diff[x] : 0u;
    sum += v;
    cnt += v ? 1u : 0u;
  }
  sum = cov_wave_sum_u32(sum);
  cnt = cov_wave_sum_u32(cnt);
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) sh[wave] = sum, sh[4 + wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    p.tile_sum[blockIdx.x] = (uint32_t)(sh[0] + sh[1] + sh[2] + sh[3]);
    p.tile_cnt[blockIdx.x] = sh[4] + sh[5] + sh[6] + sh[7];
  }
}

__global__ __launch_bounds__(256) void cov_points_kernel(const CovTileParams p) {
  __shared__ uint32_t lds[COV_LDS];
  __shared__ uint32_t sh[8];
  uint32_t v[cov::PER_THREAD];
  uint32_t sum_before, cnt_before;
  const uint64_t tile = blockIdx.x;
  cov_tile_scan(p.diff, p.n, tile, lds, sh, v, &sum_before, &cnt_before);
  uint32_t depth = (uint32_t)p.carry[tile] + sum_before;
  uint64_t at = p.point_at[tile] + cnt_before;
  const uint64_t end = p.point_at[tile + 1];  // (no write leaves the tile's own places)
  const uint64_t x0 = p.g0 + tile * cov::TILE + threadIdx.x * cov::PER_THREAD;
  for (uint32_t j = 0; j < cov::PER_THREAD; j++) {
    if (v[j] == 0) continue;
    depth += v[j];
    if (at < end) {
      p.point_entry[at] = x0 + j;
      p.point_depth[at] = depth;
      p.point_live[at] = depth ? 1 : 0;
    }
    at++;
  }
}

__global__ __launch_bounds__(256) void cov_runs_kernel(const CovRunParams p) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  uint64_t covered = 0, bases = 0;
  uint32_t depth = 0;
  if (i < p.n_points) {
    depth = p.point_depth[i];
    if (depth) {
      const uint64_t next = i + 1 < p.n_points ? p.point_entry[i + 1] : ~0ull;
      const thm_cov_run r = cov::run_of(p.base, p.n_sq, p.point_entry[i], depth, next);
      const uint64_t at = p.run_at[i];
      if (at < p.run_at[p.n_points]) p.runs[at] = r;
      covered = r.end - r.start;
      bases = covered * depth;
    }
  }
  covered = cov_wave_sum_u64(covered);
  bases = cov_wave_sum_u64(bases);
  depth = cov_wave_max_u32(depth);
  if ((threadIdx.x & 63u) == 0 && depth) {
    atomicAdd(&p.stats[0], (ull)covered);
    atomicAdd(&p.stats[1], (ull)bases);
    atomicMax(&p.stats[2], (ull)depth);
  }
}

__global__ __launch_bounds__(256) void cov_window_kernel(const CovWindowParams p) {
  __shared__ uint32_t lds[COV_LDS];
  __shared__ uint32_t sh[8];
  uint32_t v[cov::PER_THREAD];
  uint32_t sum_before, cnt_before;
  const uint64_t tile = p.start / cov::TILE + blockIdx.x, stop = p.start + p.n;
  cov_tile_scan(p.diff, stop, tile, lds, sh, v, &sum_before, &cnt_before);
  uint32_t depth = (uint32_t)p.carry[tile] + sum_before;
  // (every thread has its entries in v[]: the tile's place in LDS takes the depths)
  for (uint32_t j = 0; j < cov::PER_THREAD; j++) {
    depth += v[j];
    lds[threadIdx.x * (cov::PER_THREAD + 1) + j] = depth;
  }
  __syncthreads();
  const uint64_t t0 = tile * cov::TILE;
  for (uint32_t k = 0; k < cov::PER_THREAD; k++) {
    const uint32_t i = k * 256u + threadIdx.x;
    const uint64_t x = t0 + i;
    if (x >= p.start && x < stop) p.out[x - p.start] = lds[i + (i >> 4)];
  }
}

}  // namespace dev

hipError_t launch_cov_count(const CovCountParams& p, int n_cu, hipStream_t s) {
  const uint64_t n = p.b.n_alns > p.b.n_reads ? p.b.n_alns : p.b.n_reads;
  if (n == 0) return hipSuccess;
  // grid-stride: enough workgroups to fill the device, few enough that each sums many items before its atomics
  const uint64_t need = (n + 255) / 256, cap = (uint64_t)(n_cu > 0 ? n_cu : 256) * 8;
  hipLaunchKernelGGL(dev::cov_count_kernel, dim3((unsigned)(need < cap ? need : cap)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_cov_deposit(const CovDepositParams& p, hipStream_t s) {
  if (p.b.n_alns == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::cov_deposit_kernel, dim3(blocks256(p.b.n_alns)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_cov_tiles(const CovTileParams& p, hipStream_t s) {
  if (p.n == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::cov_tiles_kernel, dim3((unsigned)cov::n_tiles(p.n)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_cov_points(const CovTileParams& p, hipStream_t s) {
  if (p.n == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::cov_points_kernel, dim3((unsigned)cov::n_tiles(p.n)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_cov_runs(const CovRunParams& p, hipStream_t s) {
  if (p.n_points == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::cov_runs_kernel, dim3(blocks256(p.n_points)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_cov_window(const CovWindowParams& p, hipStream_t s) {
  if (p.n == 0) return hipSuccess;
  const uint64_t first = p.start / cov::TILE, last = (p.start + p.n - 1) / cov::TILE;
  hipLaunchKernelGGL(dev::cov_window_kernel, dim3((unsigned)(last - first + 1)), dim3(256), 0, s, p);
  return hipGetLastError();
}

}  // namespace thm
