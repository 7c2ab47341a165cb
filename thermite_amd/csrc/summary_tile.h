// summary_tile.h -- the device-only pieces that the kernels of the run summaries share (kernels_quant.hip,
// kernels_coverage.hip, kernels_pileup.hip): the sums over a wavefront, the way a count kernel's totals leave its
// workgroup and the read totals in front of it; and, for the two over a difference array in coverage_device.h's layout,
// the two adds a block deposits and the pass that brings one tile of cov::TILE entries through LDS and scans it over the
// workgroup.
#ifndef THERMITE_SUMMARY_TILE_H
#define THERMITE_SUMMARY_TILE_H
#include <hip/hip_runtime.h>

#include "coverage_device.h"
#include "launch_io.h"

namespace thm {
namespace dev {

constexpr uint32_t COV_LDS = cov::TILE + cov::TILE / cov::PER_THREAD;  // a word of padding per thread: stride 17, no bank conflict
static_assert(cov::TILE_THREADS == 256 && cov::PER_THREAD == 16, "the kernels are written for 256 threads of 16 entries");

__device__ inline uint64_t cov_wave_sum_u64(uint64_t v) {
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d);
    v += (uint64_t)hi << 32 | lo;
  }
  return v;
}
__device__ inline uint32_t cov_wave_sum_u32(uint32_t v) {
  for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
  return v;
}
__device__ inline uint32_t cov_wave_max_u32(uint32_t v) {
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)v, d);
    v = o > v ? o : v;
  }
  return v;
}
__device__ inline uint64_t wave_sum(uint64_t v) { return cov_wave_sum_u64(v); }
__device__ inline uint32_t wave_sum(uint32_t v) { return cov_wave_sum_u32(v); }

// The end of a count kernel of 256 threads: the N totals a thread has summed in registers (T: as wide as its kernel
// needs them) are summed per wavefront by shuffles, per workgroup in sh_tot (zeroed behind a barrier by the kernel's
// beginning), and reach global memory as one add per total and workgroup.
template <int N, class T>
__device__ inline void block_totals(const T (&t)[N], unsigned long long* sh_tot, unsigned long long* totals) {
  for (int k = 0; k < N; k++) {
    const T s = wave_sum(t[k]);
    if ((threadIdx.x & 63u) == 0 && s) atomicAdd(&sh_tot[k], (unsigned long long)s);
  }
  __syncthreads();
  if (threadIdx.x < N && sh_tot[threadIdx.x]) atomicAdd(&totals[threadIdx.x], sh_tot[threadIdx.x]);
}

// the read totals of a batch, grid-stride with one thread per read: the reads, and those that failed
__device__ inline void read_totals(const AlnBatch& b, uint64_t& n_reads, uint64_t& n_failed) {
  const uint64_t stride = (uint64_t)gridDim.x * 256u;
  for (uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x; r < b.n_reads; r += stride) {
    n_reads++;
    if (b.status && b.status[r] != THM_OK) n_failed++;
  }
}

// what the deposit kernels hand to cov::walk_blocks: a block [s, e) is two integer adds (mod 2^32) without a return value
struct BlockAdder {
  uint32_t* dst;  // the contig's first entry (in the alignment's track)
  __device__ void operator()(uint64_t s, uint64_t e) const {
    (void)atomicAdd(dst + s, 1u);
    (void)atomicAdd(dst + e, 0xFFFFFFFFu);
  }
};

// Tile `tile` of diff[0, n) into LDS, the thread's own PER_THREAD consecutive entries into v[], and the exclusive scans
// over the workgroup of their sum and of the number of non-zero ones.  The tile stays in `lds` (entry i at i + i / 16).
__device__ inline void cov_tile_scan(const uint32_t* diff, uint64_t n, uint64_t tile, uint32_t* lds, uint32_t* sh, uint32_t (&v)[cov::PER_THREAD],
                                     uint32_t* sum_before, uint32_t* cnt_before) {
  const uint64_t t0 = tile * cov::TILE;
  for (uint32_t k = 0; k < cov::PER_THREAD; k++) {
    const uint32_t i = k * 256u + threadIdx.x;
    const uint64_t x = t0 + i;
    lds[i + (i >> 4)] = x < n ? diff[x] : 0u;
  }
  __syncthreads();
  uint32_t sum = 0, cnt = 0;
  for (uint32_t j = 0; j < cov::PER_THREAD; j++) {
    v[j] = lds[threadIdx.x * (cov::PER_THREAD + 1) + j];
    sum += v[j];
    cnt += v[j] ? 1u : 0u;
  }
  // inclusive over the wavefront, then the wavefronts in front
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t isum = sum, icnt = cnt;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t s2 = (uint32_t)__shfl_up((int)isum, d), c2 = (uint32_t)__shfl_up((int)icnt, d);
    if (lane >= (uint32_t)d) isum += s2, icnt += c2;
  }
  if (lane == 63) sh[wave] = isum, sh[4 + wave] = icnt;
  __syncthreads();
  uint32_t ws = 0, wc = 0;
  for (uint32_t w = 0; w < 4; w++)
    if (w < wave) ws += sh[w], wc += sh[4 + w];
  *sum_before = ws + isum - sum;
  *cnt_before = wc + icnt - cnt;
}

// ... and the depths of the tile's entries in their places in `lds`, for every thread to read behind a barrier
__device__ inline void cov_tile_depths(const uint32_t* diff, uint64_t n, uint64_t tile, uint32_t carry, uint32_t* lds, uint32_t* sh) {
  uint32_t v[cov::PER_THREAD];
  uint32_t sum_before, cnt_before;
  cov_tile_scan(diff, n, tile, lds, sh, v, &sum_before, &cnt_before);
  uint32_t depth = carry + sum_before;
  // (every thread has its entries in v[]: the tile's place in LDS takes the depths)
  for (uint32_t j = 0; j < cov::PER_THREAD; j++) {
    depth += v[j];
    lds[threadIdx.x * (cov::PER_THREAD + 1) + j] = depth;
  }
  __syncthreads();
}

}  // namespace dev
}  // namespace thm
#endif
