// kernels_fastq.hip -- the device FASTQ parser (host side fastq.hip): a block of whole 4-line
// records as raw bytes -> names, bases and qualities back to back with their offsets, in the buffers the rest of the
// pipeline reads.  Every kernel is one step of fastq_device.h spread over threads:
//   count     a wave per chunk of CHUNK bytes: newlines per chunk (their scan places the chunk's line starts)
//   starts    the same walk: every newline writes the start of the line behind it
//   records   a thread per record: the parse rule -> name and sequence length, or the decline flag
//   gather    GATHER_LANES lanes per record: the three spans to their places
// The block is read twice by waves (count, starts), touched at the line ends by records and read once more by gather.
#include <hip/hip_runtime.h>

#include "fastq_device.h"
#include "launch_io.h"

namespace thm {
namespace dev {

using namespace fq;

constexpr uint32_t FQ_THREADS = 256, FQ_WAVES = FQ_THREADS / 64;

// the masks of one step of a wave's walk: lane l looks at the word at `at + 4 l` (the block is 4-byte aligned and
// padded, bytes at or behind `hi` do not count)
__device__ inline void step_masks(const uint8_t* raw, uint64_t at, uint64_t hi, uint32_t lane, uint64_t m[4], uint32_t* mine) {
  const uint64_t i = at + 4ull * lane;
  const uint32_t w = i < hi ? *(const uint32_t*)(raw + i) : 0u;
  const uint32_t b = newline_bits(w, i, hi);
  for (uint32_t j = 0; j < 4; j++) m[j] = __ballot((b >> j) & 1u);
  *mine = b;
}

__global__ __launch_bounds__(256) void fastq_count_kernel(const FastqParams p) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t n_waves = (uint64_t)gridDim.x * FQ_WAVES;
  for (uint64_t c = (uint64_t)blockIdx.x * FQ_WAVES + (threadIdx.x >> 6); c < p.n_chunks; c += n_waves) {
    const uint64_t lo = c * CHUNK, hi = lo + CHUNK < p.n ? lo + CHUNK : p.n;
    uint64_t cnt = 0;
    for (uint64_t at = lo; at < hi; at += STEP) {
      uint64_t m[4];
      uint32_t mine;
      step_masks(p.raw, at, hi, lane, m, &mine);
      cnt += step_count(m);
    }
    if (lane == 0) p.chunk_cnt[c] = cnt;
  }
}

__global__ __launch_bounds__(256) void fastq_starts_kernel(const FastqParams p) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t n_waves = (uint64_t)gridDim.x * FQ_WAVES;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    p.line_start[0] = 0;
    if (p.n_lines > p.n_newlines) p.line_start[p.n_lines] = p.n + 1;  // behind a last line without its newline
  }
  for (uint64_t c = (uint64_t)blockIdx.x * FQ_WAVES + (threadIdx.x >> 6); c < p.n_chunks; c += n_waves) {
    const uint64_t lo = c * CHUNK, hi = lo + CHUNK < p.n ? lo + CHUNK : p.n;
    uint64_t k = p.chunk_base[c];  // newlines of the block before this step
    for (uint64_t at = lo; at < hi; at += STEP) {
      uint64_t m[4];
      uint32_t mine;
      step_masks(p.raw, at, hi, lane, m, &mine);
      for (uint32_t j = 0; j < 4; j++)
        if ((mine >> j) & 1u) {
          const uint64_t idx = k + step_rank(m, lane, j) + 1;
          if (idx <= p.n_newlines) p.line_start[idx] = at + 4ull * lane + j + 1;  // (always, unless the counts were wrong)
        }
      k += step_count(m);
    }
  }
}

__global__ __launch_bounds__(256) void fastq_records_kernel(const FastqParams p) {
  const uint64_t r = (uint64_t)blockIdx.x * FQ_THREADS + threadIdx.x;
  if (r >= p.n_records) return;
  // (line starts ascend and end at n or n + 1 by construction; a table that does not is never followed into the block)
  bool sane = true;
  for (uint32_t k = 0; k < 4; k++) sane = sane && p.line_start[4 * r + k] < p.line_start[4 * r + k + 1] && p.line_start[4 * r + k + 1] <= p.n + 1;
  Record rec;
  if (!sane) {
    p.name_len[r] = 0;
    p.seq_len[r] = 0;
    *p.flag = 2u;
  } else if (record_rule(p.raw, p.line_start, r, &rec)) {
    p.name_len[r] = rec.name_len;
    p.seq_len[r] = rec.seq_len;
  } else {
    p.name_len[r] = 0;
    p.seq_len[r] = 0;
    *p.flag = 1u;  // (a plain store: whichever value lands, the block is declined)
  }
}

__global__ __launch_bounds__(256) void fastq_gather_kernel(const FastqParams p) {
  constexpr uint32_t PER_BLOCK = FQ_THREADS / GATHER_LANES;
  const uint32_t lane = threadIdx.x % GATHER_LANES;
  const uint64_t stride = (uint64_t)gridDim.x * PER_BLOCK;
  for (uint64_t r = (uint64_t)blockIdx.x * PER_BLOCK + threadIdx.x / GATHER_LANES; r < p.n_records; r += stride) {
    // the block passed the rule: the extents are the ones the lengths were taken from
    uint64_t at;
    (void)line_extent(p.raw, p.line_start, 4 * r, &at);
    const uint64_t no = p.name_off[r], so = p.offsets[r];
    const uint64_t nl = p.name_off[r + 1] - no, sl = p.offsets[r + 1] - so;
    copy_bytes(p.names + no, p.raw + at + 1, nl, lane, GATHER_LANES);
    copy_bytes(p.bases + so, p.raw + p.line_start[4 * r + 1], sl, lane, GATHER_LANES);
    copy_bytes(p.quals + so, p.raw + p.line_start[4 * r + 3], sl, lane, GATHER_LANES);
  }
}

static unsigned fq_grid(uint64_t need, int n_cu) {
  const uint64_t cap = (uint64_t)(n_cu > 0 ? n_cu : 256) * 8;
  return (unsigned)(need < 1 ? 1 : need < cap ? need : cap);
}

}  // namespace dev

hipError_t launch_fastq_count(const FastqParams& p, int n_cu, hipStream_t s) {
  if (p.n_chunks == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::fastq_count_kernel, dim3(dev::fq_grid((p.n_chunks + dev::FQ_WAVES - 1) / dev::FQ_WAVES, n_cu)), dim3(dev::FQ_THREADS), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_fastq_starts(const FastqParams& p, int n_cu, hipStream_t s) {
  if (p.n_chunks == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::fastq_starts_kernel, dim3(dev::fq_grid((p.n_chunks + dev::FQ_WAVES - 1) / dev::FQ_WAVES, n_cu)), dim3(dev::FQ_THREADS), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_fastq_records(const FastqParams& p, hipStream_t s) {
  if (p.n_records == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::fastq_records_kernel, dim3((unsigned)((p.n_records + dev::FQ_THREADS - 1) / dev::FQ_THREADS)), dim3(dev::FQ_THREADS), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_fastq_gather(const FastqParams& p, int n_cu, hipStream_t s) {
  if (p.n_records == 0) return hipSuccess;
  constexpr uint32_t per_block = dev::FQ_THREADS / fq::GATHER_LANES;
  hipLaunchKernelGGL(dev::fastq_gather_kernel, dim3(dev::fq_grid((p.n_records + per_block - 1) / per_block, n_cu * 4)), dim3(dev::FQ_THREADS), 0, s, p);
  return hipGetLastError();
}

}  // namespace thm
