// kernels_bam_sort.hip -- the device side of the coordinate sort of a run's BAM records (include/thermite_io.h:
// thm_bam_sorter; host side bam_sort.hip; the functions spread over threads here are bam_sort_device.h).
//
//   keys    one thread per record of the batch just added: its sort key from refID, pos and flag, its length, and its
//           place in the arena (the records themselves are copied there as they are)
//   iota    the ordinals 0 .. n-1 the radix sort carries along as values
//   order   one thread per sorted record: length and place by sorted ordinal (the host scans the lengths)
//   gather  a window [w0, w1) of the sorted stream into a staging buffer the deflater reads, in two shapes: record-centric,
//           a wavefront per record (the default: the faster one at the default window), or
//           output-centric, every lane owning one aligned 16-byte piece of the window (THM_SORT_GATHER=pieces)
//
// The gather is the hot one.  The output-centric kernel stands first.  Records are byte-packed, so a piece's source
// begins at any byte address; a piece that lies inside one record (14 of 15 for a 240-byte record) is four or five
// aligned dword loads funnel-shifted by the source's misalignment and one dwordx4 store, so a wavefront's stores cover
// 1 KiB without a gap.  A piece that holds a record boundary, or the window's ragged end, is copied byte by byte, record
// by record.  Thread 0 of a workgroup narrows the records of the workgroup's 4 KiB to a range first, so that the lanes'
// binary searches run over a handful of offsets.
#include <hip/hip_runtime.h>

#include "bam_sort_device.h"
#include "launch_io.h"

namespace thm {
namespace dev {

__global__ __launch_bounds__(256) void bam_sort_keys_kernel(const BamSortKeysParams p) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= p.n) return;
  const uint64_t at = p.off[i];
  p.key[i] = bsort::record_key(p.data + at, p.n_sq);
  p.len[i] = (uint32_t)(p.off[i + 1] - at);
  p.loc[i] = p.base + at;
}

__global__ __launch_bounds__(256) void bam_sort_iota_kernel(uint32_t* ord, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i < n) ord[i] = (uint32_t)i;
}

__global__ __launch_bounds__(256) void bam_sort_order_kernel(const uint32_t* ord, const uint32_t* len, const uint64_t* loc, uint64_t n,
                                                             uint64_t* s_len, uint64_t* s_loc) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t o = ord[i];
  s_len[i] = len[o];
  s_loc[i] = loc[o];
}

// where byte `loc` of the arena is
__device__ inline const uint8_t* arena_at(const BamSortGatherParams& p, uint64_t loc) {
  const uint32_t s = bsort::segment_of(p.seg_start, p.n_seg, loc);
  return p.seg[s] + (loc - p.seg_start[s]);
}

__global__ __launch_bounds__(256) void bam_sort_gather_kernel(const BamSortGatherParams p) {
  __shared__ uint64_t range[2];
  const uint64_t b0 = p.w0 + (uint64_t)blockIdx.x * (256u * bsort::PIECE);  // < w1: the grid covers the window exactly
  if (threadIdx.x == 0) {
    const uint64_t b1 = b0 + 256u * bsort::PIECE < p.w1 ? b0 + 256u * bsort::PIECE : p.w1;
    bsort::window_records(p.off, p.n, b0, b1, &range[0], &range[1]);
  }
  __syncthreads();
  const uint64_t p0 = b0 + (uint64_t)threadIdx.x * bsort::PIECE;
  if (p0 >= p.w1) return;
  const uint64_t p1 = p0 + bsort::PIECE < p.w1 ? p0 + bsort::PIECE : p.w1;
  const uint64_t first = range[0];
  uint64_t r = first + bsort::record_at(p.off + first, range[1] - first, p0);
  uint8_t* out = p.out + (p0 - p.w0);
  const uint64_t begin = p.off[r], end = p.off[r + 1];
  if (end >= p1 && p1 - p0 == bsort::PIECE) {
    // the whole piece from one record
    const uint8_t* src = arena_at(p, p.loc[r] + (p0 - begin));
    const uint32_t mis = (uint32_t)((uintptr_t)src & 3u);
    const uint32_t* a = (const uint32_t*)(src - mis);
    uint4 v;
    if (mis == 0) {
      v = make_uint4(a[0], a[1], a[2], a[3]);
    } else {
      const uint32_t d0 = a[0], d1 = a[1], d2 = a[2], d3 = a[3], d4 = a[4], sh = 8 * mis;
      v = make_uint4((uint32_t)(((uint64_t)d1 << 32 | d0) >> sh), (uint32_t)(((uint64_t)d2 << 32 | d1) >> sh),
                     (uint32_t)(((uint64_t)d3 << 32 | d2) >> sh), (uint32_t)(((uint64_t)d4 << 32 | d3) >> sh));
    }
    *(uint4*)out = v;
    return;
  }
  // a record boundary inside the piece, or the window's last, short piece
  for (uint64_t at = p0; at < p1; r++) {
    const uint64_t rb = p.off[r], re = p.off[r + 1];
    const bsort::Part q = bsort::clip(rb, re, p0, p1);
    const uint8_t* src = arena_at(p, p.loc[r]) + q.src;
    for (uint64_t k = 0; k < q.n; k++) out[q.dst + k] = src[k];
    at = re;
  }
}

// The record-centric shape: one wavefront per record that overlaps the window (grid-stride over them), the part of
// the record inside the window copied as bam_emit_kernel<true> writes a record out -- a byte head up to the destination's
// dword boundary, aligned dword stores fed by aligned dword loads funnel-shifted by the source's misalignment against the
// destination, a byte tail.  A wavefront's stores cover 256 consecutive bytes; a record of 240 bytes leaves the last
// lanes idle and begins and ends with partial lines.
__global__ __launch_bounds__(256) void bam_sort_gather_records_kernel(const BamSortGatherParams p) {
  __shared__ uint64_t range[2];
  if (threadIdx.x == 0) bsort::window_records(p.off, p.n, p.w0, p.w1, &range[0], &range[1]);
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * 4u;
  for (uint64_t r = range[0] + wave; r < range[1]; r += n_waves) {
    const bsort::Part q = bsort::clip(p.off[r], p.off[r + 1], p.w0, p.w1);
    const uint8_t* src = arena_at(p, p.loc[r]) + q.src;
    uint8_t* dst = p.out + q.dst;
    uint64_t head = (4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u;
    if (head > q.n) head = q.n;
    if (lane < head) dst[lane] = src[lane];
    const uint64_t n_dw = (q.n - head) / 4, tail = (q.n - head) & 3u;
    const uint8_t* s = src + head;
    const uint32_t mis = (uint32_t)((uintptr_t)s & 3u), sh = 8 * mis;
    const uint32_t* a = (const uint32_t*)(s - mis);
    uint32_t* d = (uint32_t*)(dst + head);
    if (mis == 0) {
      for (uint64_t i = lane; i < n_dw; i += 64) d[i] = a[i];
    } else {
      for (uint64_t i = lane; i < n_dw; i += 64) d[i] = (uint32_t)(((uint64_t)a[i + 1] << 32 | a[i]) >> sh);
    }
    if (lane < tail) dst[head + 4 * n_dw + lane] = src[head + 4 * n_dw + lane];
  }
}

}  // namespace dev

hipError_t launch_bam_sort_keys(const BamSortKeysParams& p, hipStream_t s) {
  if (p.n == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::bam_sort_keys_kernel, dim3(blocks256(p.n)), dim3(256), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_bam_sort_iota(uint32_t* ord, uint64_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::bam_sort_iota_kernel, dim3(blocks256(n)), dim3(256), 0, s, ord, n);
  return hipGetLastError();
}

hipError_t launch_bam_sort_order(const uint32_t* ord, const uint32_t* len, const uint64_t* loc, uint64_t n, uint64_t* s_len,
                                 uint64_t* s_loc, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::bam_sort_order_kernel, dim3(blocks256(n)), dim3(256), 0, s, ord, len, loc, n, s_len, s_loc);
  return hipGetLastError();
}

hipError_t launch_bam_sort_gather(const BamSortGatherParams& p, bool by_records, int n_cu, hipStream_t s) {
  if (p.w1 <= p.w0) return hipSuccess;
  if (by_records) {
    // no more waves than the window can have records, no more workgroups than 16 a CU
    const uint64_t need = ((p.w1 - p.w0) / bsort::MIN_RECORD + 2 + 3) / 4, cap = (uint64_t)(n_cu > 0 ? n_cu : 256) * 16;
    hipLaunchKernelGGL(dev::bam_sort_gather_records_kernel, dim3((unsigned)(need < cap ? need : cap)), dim3(256), 0, s, p);
    return hipGetLastError();
  }
  const uint64_t pieces = (p.w1 - p.w0 + bsort::PIECE - 1) / bsort::PIECE;
  hipLaunchKernelGGL(dev::bam_sort_gather_kernel, dim3(blocks256(pieces)), dim3(256), 0, s, p);
  return hipGetLastError();
}

}  // namespace thm
