// kernels_util.hip -- small plumbing kernels: exclusive prefix sums that turn
// per-read counts into offsets (count -> scan -> fill), and the sum of the
// counter rows the extend kernels' waves leave.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "launch.h"
#include "lut_direct.h"

namespace thm {
namespace dev {

// lut_direct.h: the text position into every single-suffix entry of the device copy of the k-mer table, once per device
// copy.  One thread per entry; an entry whose lo is not a rank (no valid table has one) is left alone.
template <class C>
__global__ __launch_bounds__(256) void lut_tag_kernel(LutEntryT<C>* lut, const C* sa, uint64_t n_entries, uint64_t n,
                                                      unsigned long long* count) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  bool tagged = false;
  if (i < n_entries) {
    const LutEntryT<C> e = lut[i];
    if (lutd::single_suffix(e.lo, e.hi) && (uint64_t)e.lo < n) {
      lut[i].hi = lutd::encode(sa[e.lo]);
      tagged = true;
    }
  }
  const unsigned long long m = __ballot(tagged);
  if (m && (threadIdx.x & 63u) == (unsigned)__builtin_ctzll(m)) atomicAdd(count, (unsigned long long)__popcll(m));
}

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ITEMS = 8;
static_assert(SCAN_TILE == SCAN_THREADS * SCAN_ITEMS, "launch.h: SCAN_TILE");

// exclusive scan of `v` over the block (256 threads); returns the thread's prefix, total in *tot
__device__ uint64_t block_excl_scan(uint64_t v, uint64_t* sh, uint64_t* tot) {
  const int t = (int)threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int o = 1; o < SCAN_THREADS; o <<= 1) {
    uint64_t a = (t >= o) ? sh[t - o] : 0;
    __syncthreads();
    sh[t] += a;
    __syncthreads();
  }
  const uint64_t incl = sh[t];
  *tot = sh[SCAN_THREADS - 1];
  __syncthreads();
  return incl - v;
}

__global__ __launch_bounds__(SCAN_THREADS) void scan_tiles_kernel(const uint64_t* in, uint64_t* out, uint64_t n,
                                                                  uint64_t* tile_sums) {
  __shared__ uint64_t sh[SCAN_THREADS];
  const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_ITEMS;
  uint64_t v[SCAN_ITEMS], s = 0;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; k++) {
    v[k] = (base + k < n) ? in[base + k] : 0;
    s += v[k];
  }
  uint64_t tot;
  uint64_t pre = block_excl_scan(s, sh, &tot);
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; k++) {
    if (base + k < n) out[base + k] = pre;
    pre += v[k];
  }
  if (threadIdx.x == 0) tile_sums[blockIdx.x] = tot;
}

// one block: exclusive scan of the tile sums in place, grand total to *total_out
__global__ __launch_bounds__(SCAN_THREADS) void scan_sums_kernel(uint64_t* tile_sums, uint64_t n_tiles,
                                                                 uint64_t* total_out) {
  __shared__ uint64_t sh[SCAN_THREADS];
  uint64_t carry = 0;
  for (uint64_t b0 = 0; b0 < n_tiles; b0 += SCAN_THREADS) {
    const uint64_t i = b0 + threadIdx.x;
    const uint64_t v = (i < n_tiles) ? tile_sums[i] : 0;
    uint64_t tot;
    const uint64_t pre = block_excl_scan(v, sh, &tot);
    if (i < n_tiles) tile_sums[i] = carry + pre;
    carry += tot;
  }
  if (threadIdx.x == 0) *total_out = carry;
}

__global__ __launch_bounds__(SCAN_THREADS) void scan_add_kernel(uint64_t* out, uint64_t n, const uint64_t* tile_offs) {
  const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_ITEMS;
  const uint64_t add = tile_offs[blockIdx.x];
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; k++)
    if (base + k < n) out[base + k] += add;
}

// Two arrays in one pass (alignment counts, u32, and op bytes, u64): the tile sums of `a` in tile_sums[0 .. tiles), those
// of `b` behind them
__global__ __launch_bounds__(SCAN_THREADS) void scan2_tiles_kernel(const uint32_t* in_a, const uint64_t* in_b, uint64_t* out_a,
                                                                   uint64_t* out_b, uint64_t n, uint64_t* tile_sums) {
  __shared__ uint64_t sh[SCAN_THREADS];
  const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_ITEMS;
  uint64_t va[SCAN_ITEMS], vb[SCAN_ITEMS], sa = 0, sb = 0;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; k++) {
    va[k] = (base + k < n) ? (uint64_t)in_a[base + k] : 0;
    vb[k] = (base + k < n) ? in_b[base + k] : 0;
    sa += va[k];
    sb += vb[k];
  }
  uint64_t tot_a, tot_b;
  uint64_t pre_a = block_excl_scan(sa, sh, &tot_a);
  uint64_t pre_b = block_excl_scan(sb, sh, &tot_b);
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; k++) {
    if (base + k < n) {
      out_a[base + k] = pre_a;
      out_b[base + k] = pre_b;
    }
    pre_a += va[k];
    pre_b += vb[k];
  }
  if (threadIdx.x == 0) {
    tile_sums[blockIdx.x] = tot_a;
    tile_sums[gridDim.x + blockIdx.x] = tot_b;
  }
}

// two blocks: block 0 scans the tile sums of `a`, block 1 those of `b`
__global__ __launch_bounds__(SCAN_THREADS) void scan2_sums_kernel(uint64_t* tile_sums, uint64_t n_tiles, uint64_t* total_a,
                                                                  uint64_t* total_b) {
  __shared__ uint64_t sh[SCAN_THREADS];
  uint64_t* sums = tile_sums + (uint64_t)blockIdx.x * n_tiles;
  uint64_t carry = 0;
  for (uint64_t b0 = 0; b0 < n_tiles; b0 += SCAN_THREADS) {
    const uint64_t i = b0 + threadIdx.x;
    const uint64_t v = (i < n_tiles) ? sums[i] : 0;
    uint64_t tot;
    const uint64_t pre = block_excl_scan(v, sh, &tot);
    if (i < n_tiles) sums[i] = carry + pre;
    carry += tot;
  }
  if (threadIdx.x == 0) *(blockIdx.x ? total_b : total_a) = carry;
}

__global__ __launch_bounds__(SCAN_THREADS) void scan2_add_kernel(uint64_t* out_a, uint64_t* out_b, uint64_t n, const uint64_t* tile_offs) {
  const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_ITEMS;
  const uint64_t add_a = tile_offs[blockIdx.x], add_b = tile_offs[gridDim.x + blockIdx.x];
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; k++)
    if (base + k < n) {
      out_a[base + k] += add_a;
      out_b[base + k] += add_b;
    }
}

// Calibration of the memory-side counters (rocprofv3 FETCH_SIZE) on a gather of known size in the access patterns
// of the two hot stages (MI355X_MICROARCH.md, HBM: "calibrate on a known byte count in your own access pattern"):
//   pattern 0  every thread loads 8 aligned bytes at a pseudo-random offset of the table (index probes);
//   pattern 1  every thread loads 4 aligned bytes at a pseudo-random offset (suffix-array entries);
//   pattern 2  groups of 16 lanes load 256 contiguous bytes (16 B per lane) at a pseudo-random 16-byte-aligned
//              offset (window staging of the extend kernel).
__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}
__global__ __launch_bounds__(256) void calib_gather_kernel(const uint8_t* table, uint64_t span, uint64_t n_threads, int pattern,
                                                           unsigned long long* sink) {
  const uint64_t tid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (tid >= n_threads) return;
  unsigned long long acc = 0;
  if (pattern == 0) {
    const uint64_t o = (mix64(tid) % (span / 8)) * 8;
    acc = *(const unsigned long long*)(table + o);
  } else if (pattern == 1) {
    const uint64_t o = (mix64(tid) % (span / 4)) * 4;
    acc = *(const unsigned*)(table + o);
  } else {
    const uint64_t o = (mix64(tid >> 4) % ((span - 256) / 16)) * 16 + (tid & 15) * 16;
    const uint4 v = *(const uint4*)(table + o);
    acc = v.x ^ v.y ^ v.z ^ v.w;
  }
  if (acc == 0x7f4a7c15ull) *sink = acc;  // keeps the loads alive (a value all three patterns can produce)
}

// counters[k] += sum of wave_counters[row][k] (the rows the extend kernels' waves left), and every row that held
// something is zeroed again: the rows are clean when the next run starts, whatever its number of rows.  A workgroup
// takes REDUCE_GROUPS rows at a time (a row is one 128-byte line), sums them in LDS and adds its sums with one atomic
// per counter (the sums are integers: the order of the workgroups does not show).
constexpr int REDUCE_GROUPS = 64, REDUCE_MAX_BLOCKS = 32;
__global__ __launch_bounds__(REDUCE_GROUPS * THM_N_COUNTERS) void counters_reduce_kernel(unsigned long long* rows, uint32_t n_rows,
                                                                                       unsigned long long* counters) {
  __shared__ unsigned long long part[REDUCE_GROUPS][THM_N_COUNTERS];
  static_assert(THM_N_COUNTERS == 16, "one thread per counter and row group");
  const int k = (int)(threadIdx.x & 15u), g = (int)(threadIdx.x >> 4);
  const uint32_t step = gridDim.x * REDUCE_GROUPS;
  unsigned long long sum = 0;
  // four rows in flight per thread (the stores would otherwise order the loads behind them)
  for (uint32_t r0 = blockIdx.x * REDUCE_GROUPS + (uint32_t)g; r0 < n_rows; r0 += 4 * step) {
    unsigned long long v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint64_t r = (uint64_t)r0 + (uint64_t)j * step;
      v[j] = r < n_rows ? rows[r * THM_N_COUNTERS + k] : 0ull;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (v[j]) {
        sum += v[j];
        rows[((uint64_t)r0 + (uint64_t)j * step) * THM_N_COUNTERS + k] = 0;
      }
    }
  }
  part[g][k] = sum;
  __syncthreads();
  if (g == 0) {
    unsigned long long t = 0;
    for (int i = 0; i < REDUCE_GROUPS; i++) t += part[i][k];
    if (t) atomicAdd(&counters[k], t);
  }
}

}  // namespace dev

hipError_t launch_calib_gather(const uint8_t* table, uint64_t span, uint64_t n_threads, int pattern, unsigned long long* sink,
                               hipStream_t s) {
  if (n_threads == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::calib_gather_kernel, dim3((unsigned)((n_threads + 255) / 256)), dim3(256), 0, s, table, span, n_threads,
                     pattern, sink);
  return hipGetLastError();
}

template <class C>
static hipError_t launch_lut_tag_t(LutEntryT<C>* lut, const C* sa, uint64_t n_entries, uint64_t n, unsigned long long* count,
                                   hipStream_t s) {
  if (n_entries == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::lut_tag_kernel<C>, dim3((unsigned)((n_entries + 255) / 256)), dim3(256), 0, s, lut, sa, n_entries, n, count);
  return hipGetLastError();
}
hipError_t launch_lut_tag(LutEntryT<uint32_t>* lut, const uint32_t* sa, uint64_t n_entries, uint64_t n, unsigned long long* count,
                          hipStream_t s) {
  return launch_lut_tag_t(lut, sa, n_entries, n, count, s);
}
hipError_t launch_lut_tag(LutEntryT<uint64_t>* lut, const uint64_t* sa, uint64_t n_entries, uint64_t n, unsigned long long* count,
                          hipStream_t s) {
  return launch_lut_tag_t(lut, sa, n_entries, n, count, s);
}

size_t scan_tmp_entries(uint64_t n) { return (size_t)((n + SCAN_TILE - 1) / SCAN_TILE) + 1; }

// out has n+1 entries: out[i] = sum(in[0..i)), out[n] = total
hipError_t launch_exclusive_scan_u64(const uint64_t* in, uint64_t* out, uint64_t n, uint64_t* tmp, hipStream_t s) {
  if (n == 0) return hipMemsetAsync(out, 0, 8, s);
  const uint64_t tiles = (n + SCAN_TILE - 1) / SCAN_TILE;
  hipLaunchKernelGGL(dev::scan_tiles_kernel, dim3((unsigned)tiles), dim3(dev::SCAN_THREADS), 0, s, in, out, n, tmp);
  hipLaunchKernelGGL(dev::scan_sums_kernel, dim3(1), dim3(dev::SCAN_THREADS), 0, s, tmp, tiles, out + n);
  hipLaunchKernelGGL(dev::scan_add_kernel, dim3((unsigned)tiles), dim3(dev::SCAN_THREADS), 0, s, out, n, tmp);
  return hipGetLastError();
}

hipError_t launch_scan_tiles_sums_u64(const uint64_t* in, uint64_t* out, uint64_t n, uint64_t* tmp, hipStream_t s) {
  if (n == 0) return hipMemsetAsync(out, 0, 8, s);
  const uint64_t tiles = (n + SCAN_TILE - 1) / SCAN_TILE;
  hipLaunchKernelGGL(dev::scan_tiles_kernel, dim3((unsigned)tiles), dim3(dev::SCAN_THREADS), 0, s, in, out, n, tmp);
  hipLaunchKernelGGL(dev::scan_sums_kernel, dim3(1), dim3(dev::SCAN_THREADS), 0, s, tmp, tiles, out + n);
  return hipGetLastError();
}

hipError_t launch_exclusive_scan2(const uint32_t* in_a, const uint64_t* in_b, uint64_t* out_a, uint64_t* out_b, uint64_t n,
                                  uint64_t* tmp, hipStream_t s) {
  if (n == 0) {
    hipError_t e = hipMemsetAsync(out_a, 0, 8, s);
    return e != hipSuccess ? e : hipMemsetAsync(out_b, 0, 8, s);
  }
  const uint64_t tiles = (n + SCAN_TILE - 1) / SCAN_TILE;
  hipLaunchKernelGGL(dev::scan2_tiles_kernel, dim3((unsigned)tiles), dim3(dev::SCAN_THREADS), 0, s, in_a, in_b, out_a, out_b, n, tmp);
  hipLaunchKernelGGL(dev::scan2_sums_kernel, dim3(2), dim3(dev::SCAN_THREADS), 0, s, tmp, tiles, out_a + n, out_b + n);
  hipLaunchKernelGGL(dev::scan2_add_kernel, dim3((unsigned)tiles), dim3(dev::SCAN_THREADS), 0, s, out_a, out_b, n, tmp);
  return hipGetLastError();
}

hipError_t launch_counters_reduce(unsigned long long* wave_counters, uint32_t n_rows, unsigned long long* counters, hipStream_t s) {
  if (n_rows == 0) return hipSuccess;
  const unsigned blocks = std::min<unsigned>((n_rows + dev::REDUCE_GROUPS - 1) / dev::REDUCE_GROUPS, dev::REDUCE_MAX_BLOCKS);
  hipLaunchKernelGGL(dev::counters_reduce_kernel, dim3(blocks), dim3(dev::REDUCE_GROUPS * THM_N_COUNTERS), 0, s, wave_counters, n_rows,
                     counters);
  return hipGetLastError();
}

}  // namespace thm
