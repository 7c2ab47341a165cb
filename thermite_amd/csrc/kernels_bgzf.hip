// kernels_bgzf.hip -- BGZF members deflated on the device (host side bgzf.hip).
//
// bgzf_deflate_kernel: one workgroup of 256 threads per BGZF block of 0xff00 input bytes, on a persistent grid.  The
// steps are the functions of bgzf_device.h; this file only spreads them over the threads:
//   stage    the block's input into LDS (64 KiB), table (2^14 positions, 64 KiB) and histograms zeroed
//   match    tile by tile: every thread looks up its position's candidate and probes the distances 1..8, barrier, the
//            tile's positions enter the table by atomicMax (the latest position wins whatever the order of arrival),
//            barrier; the entries go to the workgroup's scratch in global memory
//   parse    threads 0..63 each parse one segment of 1020 bytes, threads 64..127 take the CRC of one
//   codes    leaves ranked by all threads; code lengths, run-length header and codes by thread 0 while thread 64
//            combines the CRCs; the table's place is zeroed and becomes the staging area
//   emit     segment bit counts, their scan, then every segment at its bit offset (atomicOr on LDS words)
//   member   header | payload (staged, or stored when that is not larger) | CRC-32 | ISIZE into the block's slot, as dwords
// bgzf_compact_kernel: the slots, each at a stride of 64 KiB, to their places behind one another.
// Every store to global memory is a plain C++ store.
#include <hip/hip_runtime.h>

#include "bgzf_device.h"
#include "launch_io.h"

namespace thm {
namespace dev {

using namespace bgz;

constexpr uint32_t BGZ_THREADS = 256;
constexpr uint32_t IN_WORDS = (BLOCK_IN + 16) / 4;  // (find_match never reads past n; the pad keeps the staging loop simple)
static_assert(TILE == BGZ_THREADS, "one position per thread and tile");

__global__ __launch_bounds__(256) void bgzf_deflate_kernel(const BgzfParams p) {
  __shared__ uint32_t in_w[IN_WORDS];
  __shared__ uint32_t table[1u << HASH_BITS];  // positions + 1; the staging area once the matches are found
  __shared__ Small sm;
  const uint32_t tid = threadIdx.x;
  const uint8_t* in = (const uint8_t*)in_w;
  uint32_t* mt = p.match + (size_t)blockIdx.x * BLOCK_IN;
  sm.crc_tab[tid] = crc_table_entry(tid);
  for (uint64_t b = blockIdx.x; b < p.n_blocks; b += gridDim.x) {
    const uint64_t base = b * BLOCK_IN;
    const uint32_t n = p.n - base < BLOCK_IN ? (uint32_t)(p.n - base) : BLOCK_IN;
    // ---- stage (p.in is 4-byte aligned, and so is every block's first byte)
    const uint32_t* src = (const uint32_t*)(p.in + base);
    const uint32_t full = n / 4;
    for (uint32_t i = tid; i < IN_WORDS; i += BGZ_THREADS) {
      uint32_t v = 0;
      if (i < full) {
        v = src[i];
      } else if (i == full) {
        for (uint32_t k = 0; k < (n & 3); k++) v |= (uint32_t)p.in[base + 4 * i + k] << (8 * k);
      }
      in_w[i] = v;
    }
    for (uint32_t i = tid; i < (1u << HASH_BITS); i += BGZ_THREADS) table[i] = 0;
    for (uint32_t i = tid; i < 288; i += BGZ_THREADS) sm.lfreq[i] = 0;
    if (tid < 32) sm.dfreq[tid] = 0;
    __syncthreads();
    // ---- match
    for (uint32_t t0 = 0; t0 < n; t0 += TILE) {
      const uint32_t pos = t0 + tid;
      const bool hashed = pos + 4 <= n;
      uint32_t h = 0;
      if (pos < n) {
        uint32_t m = 0;
        if (hashed) {
          h = hash4(load32(in, pos));
          m = find_match(in, n, pos, table[h]);
        }
        mt[pos] = m;
      }
      __syncthreads();
      if (hashed) max_word(&table[h], pos + 1);
      __syncthreads();
    }
    // ---- parse, CRC
    const uint32_t n_seg = (n + SEG - 1) / SEG;
    if (tid < n_seg) {
      const uint32_t lo = tid * SEG, hi = lo + SEG < n ? lo + SEG : n;
      sm.seg_ntok[tid] = parse_segment(in, mt, lo, hi, sm);
    } else if (tid >= N_SEG && tid - N_SEG < n_seg) {
      const uint32_t s = tid - N_SEG, lo = s * SEG, hi = lo + SEG < n ? lo + SEG : n;
      sm.seg_crc[s] = crc_bytes(sm.crc_tab, in, lo, hi);
    }
    if (tid == 255) sm.lfreq[256] = 1;  // end of block (no segment counts it)
    __syncthreads();
    // ---- codes
    for (uint32_t s = tid; s < 286; s += BGZ_THREADS) rank_symbol(sm.lfreq, 286, s, sm.leaves_l);
    if (tid < 30) rank_symbol(sm.dfreq, 30, tid, sm.leaves_d);
    for (uint32_t i = tid; i < STAGE_WORDS; i += BGZ_THREADS) table[i] = 0;
    __syncthreads();
    if (tid == 0) {
      sm.n_leaves_l = count_used(sm.lfreq, 286);
      sm.n_leaves_d = count_used(sm.dfreq, 30);
      build_codes(sm);
    } else if (tid == N_SEG) {
      sm.crc = crc_combine_segments(sm.seg_crc, n);
    }
    __syncthreads();
    // ---- emit
    if (tid < n_seg) sm.seg_bits[tid] = segment_bits(mt + tid * SEG, sm.seg_ntok[tid], sm);
    __syncthreads();
    if (tid == 0) {
      uint32_t off = sm.hdr_bits;
      for (uint32_t s = 0; s < n_seg; s++) {
        const uint32_t bits = sm.seg_bits[s];
        sm.seg_bits[s] = off;
        off += bits;
      }
      sm.total_bits = off + sm.llen[256];
      sm.stored = (sm.total_bits + 7) / 8 >= n + 5;
    }
    __syncthreads();
    if (!sm.stored) {
      if (tid < n_seg) emit_segment(mt + tid * SEG, sm.seg_ntok[tid], sm, table, sm.seg_bits[tid]);
      else if (tid == N_SEG) emit_header(sm, table, sm.total_bits - sm.llen[256]);
    }
    __syncthreads();
    // ---- member (the slot is 64 KiB: the last dword's pad bytes stay inside it)
    const uint32_t m = member_len(sm, n);
    uint32_t* dst = (uint32_t*)(p.slots + b * SLOT);
    for (uint32_t j = tid; 4 * j < m; j += BGZ_THREADS) {
      uint32_t v = 0;
      for (uint32_t k = 0; k < 4; k++)
        if (4 * j + k < m) v |= member_byte(sm, in, n, table, 4 * j + k) << (8 * k);
      dst[j] = v;
    }
    if (tid == 0) p.sizes[b] = m;
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void bgzf_compact_kernel(const BgzfParams p) {
  const uint32_t tid = threadIdx.x;
  for (uint64_t b = blockIdx.x; b < p.n_blocks; b += gridDim.x) {
    const uint8_t* src = p.slots + b * SLOT;
    const uint32_t* sw = (const uint32_t*)src;
    const uint64_t o = p.off[b];
    const uint32_t m = (uint32_t)(p.off[b + 1] - o);  // at most BLOCK_IN + 31
    uint8_t* dst = p.out + o;                         // p.out is 4-byte aligned
    uint32_t head = (4 - (uint32_t)(o & 3)) & 3;
    if (head > m) head = m;
    if (tid < head) dst[tid] = src[tid];
    const uint32_t nd = (m - head) / 4;
    uint32_t* dw = (uint32_t*)(dst + head);
    for (uint32_t j = tid; j < nd; j += 256) {
      // source bytes head + 4 j .. + 3 from the two aligned dwords that hold them (both inside the 64 KiB slot)
      const uint32_t s = head + 4 * j, sh = 8 * (s & 3), lo = sw[s >> 2];
      dw[j] = sh ? (lo >> sh) | (sw[(s >> 2) + 1] << (32 - sh)) : lo;
    }
    const uint32_t t0 = head + 4 * nd;
    if (tid < m - t0) dst[t0 + tid] = src[t0 + tid];
  }
}

}  // namespace dev

unsigned bgzf_grid(uint64_t n_blocks, int n_cu) {
  const uint64_t cap = (uint64_t)(n_cu > 0 ? n_cu : 256);  // the LDS of a CU holds one workgroup
  return (unsigned)(n_blocks < cap ? n_blocks : cap);
}

hipError_t launch_bgzf_deflate(const BgzfParams& p, int n_cu, hipStream_t s) {
  if (p.n_blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::bgzf_deflate_kernel, dim3(bgzf_grid(p.n_blocks, n_cu)), dim3(256), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_bgzf_compact(const BgzfParams& p, int n_cu, hipStream_t s) {
  if (p.n_blocks == 0) return hipSuccess;
  const uint64_t cap = (uint64_t)(n_cu > 0 ? n_cu : 256) * 8;
  hipLaunchKernelGGL(dev::bgzf_compact_kernel, dim3((unsigned)(p.n_blocks < cap ? p.n_blocks : cap)), dim3(256), 0, s, p);
  return hipGetLastError();
}

}  // namespace thm
