// kernels_bai.hip -- the device side of the BAI index of a coordinate-sorted run (include/thermite_io.h:
// thm_bam_sorter_index; host side bai.hip; the functions spread over threads here are bai_device.h).
//
//   fields       one thread per sorted record: refID, pos, flag and the CIGAR from the record's bytes in the arena (byte
//                loads: a record stands at any address) -> key = refID << 16 | bin, beg, end, the mapped bit; per
//                reference the mapped records and n_intv, reduced per wavefront and per workgroup before the atomics
//   run_heads    flags where a run of one (refID, bin) begins; the record range of every reference (the records are in
//                reference order, so a boundary is a plain store)
//   runs         by the scan of the flags: key and raw [begin, end) of every run
//   chunk_heads  over the runs sorted by key: where a bin begins, and where a chunk begins (the merge test on neighbours)
//   chunks       by the two scans: the chunks, the bin of every chunk, the first chunk of every bin, the bins of every reference
//   linear       mapped records: 64-bit atomic minima of raw offsets into the table of all references' windows -- the first
//                record of a window, and records that reach into later windows, no others
//   fill         a wavefront per reference walks its windows from the top: an empty one takes the value above
//   ref_sizes    bytes of every reference in the file (the host scans them)
//   emit         the finished bytes: a workgroup per reference (n_bin, the pseudo-bin, n_intv, ioffset[]), a thread per chunk
//                (the chunk; the first of a bin also the bin's head).  Raw offsets become virtual offsets here and only here.
#include <hip/hip_runtime.h>

#include "bai_device.h"
#include "launch_io.h"

namespace thm {
namespace dev {

using ull = unsigned long long;
constexpr uint32_t NO_REF = 0xffffffffu;

__device__ inline const uint8_t* bai_record(const BaiRecords& r, uint64_t i) {
  const uint64_t loc = r.loc[i];
  const uint32_t s = bsort::segment_of(r.seg_start, r.n_seg, loc);
  return r.seg[s] + (loc - r.seg_start[s]);
}

__device__ inline uint32_t wave_max_u32(uint32_t v) {
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t u = (uint32_t)__shfl_xor((int)v, d);
    v = u > v ? u : v;
  }
  return v;
}

__global__ __launch_bounds__(256) void bai_fields_kernel(const BaiFieldsParams p) {
  __shared__ ull sh_mapped, sh_intv;
  __shared__ uint32_t sh_ref;
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  uint32_t ref = NO_REF, intv = 0;
  bool mapped = false;
  if (i < p.r.n) {
    const uint64_t len = p.r.off[i + 1] - p.r.off[i];
    const bai::Fields f = bai::fields(bai_record(p.r, i), len);
    if (!f.ok) atomicMin(&p.err[1], (ull)i);
    uint32_t bin = 0;
    if (f.ref_id >= 0) {
      if (f.end > bai::MAX_END)
        atomicMin(&p.err[0], (ull)i);
      else
        bin = bai::reg2bin(f.beg, (int64_t)f.end);
      ref = (uint32_t)f.ref_id;
      mapped = f.mapped;
      if (mapped && f.end <= bai::MAX_END) intv = bai::last_window(f.end) + 1;
    }
    p.key[i] = bai::key(f.ref_id, bin, p.r.n_sq);
    p.beg[i] = f.beg | (f.mapped ? bai::MAPPED_BIT : 0u);
    p.end[i] = f.end > 0xffffffffull ? 0xffffffffu : (uint32_t)f.end;
  }
  // the workgroup's first record names the reference that is summed in LDS; a wavefront adds once per reference it holds
  if (threadIdx.x == 0) {
    sh_ref = ref;
    sh_mapped = 0;
    sh_intv = 0;
  }
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u, first_ref = sh_ref;
  ull todo = __ballot(ref != NO_REF);
  while (todo) {
    const int leader = __ffsll(todo) - 1;
    const uint32_t r = (uint32_t)__shfl((int)ref, leader);
    const bool mine = ref == r;
    const ull m = __ballot(mine);
    const ull cnt = (ull)__popcll(__ballot(mine && mapped));
    const uint32_t w = wave_max_u32(mine ? intv : 0u);
    if ((int)lane == leader) {
      if (r == first_ref) {
        if (cnt) atomicAdd(&sh_mapped, cnt);
        if (w) atomicMax(&sh_intv, (ull)w);
      } else {
        if (cnt) atomicAdd(&p.ref_mapped[r], cnt);
        if (w) atomicMax(&p.ref_intv[r], (ull)w);
      }
    }
    todo &= ~m;
  }
  __syncthreads();
  if (threadIdx.x == 0 && first_ref != NO_REF) {
    if (sh_mapped) atomicAdd(&p.ref_mapped[first_ref], sh_mapped);
    if (sh_intv) atomicMax(&p.ref_intv[first_ref], sh_intv);
  }
}

__global__ __launch_bounds__(256) void bai_run_heads_kernel(const BaiRunParams p) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i > p.n) return;
  const bool has_prev = i > 0, has_cur = i < p.n;
  const uint64_t k = has_cur ? p.key[i] : (uint64_t)p.n_sq << 16, kp = has_prev ? p.key[i - 1] : 0;
  if (has_cur) p.flag[i] = bai::run_head(has_prev, kp, k, p.n_sq) ? 1 : 0;
  const uint32_t rc = bai::key_ref(k), rp = has_prev ? bai::key_ref(kp) : NO_REF;
  if (rc != rp) {
    if (rc < p.n_sq)
      p.ref_first[rc] = i;
    else
      *p.n_coor = i;  // (the one boundary to the records without a reference, or the end)
    if (has_prev && rp < p.n_sq) p.ref_end[rp] = i;
  }
}

__global__ __launch_bounds__(256) void bai_runs_kernel(const BaiRunParams p) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i > p.n) return;
  const bool has_prev = i > 0, has_cur = i < p.n;
  const uint64_t k = has_cur ? p.key[i] : 0, kp = has_prev ? p.key[i - 1] : 0;
  if (has_cur && bai::run_head(has_prev, kp, k, p.n_sq)) {
    const uint64_t j = p.idx[i];
    p.run_key[j] = k;
    p.run_beg[j] = p.off[i];
  }
  if (bai::run_end(has_prev, kp, has_cur, k, p.n_sq)) p.run_end[p.idx[i] - 1] = p.off[i];  // (a run began before i)
}

__global__ __launch_bounds__(256) void bai_chunk_heads_kernel(const BaiChunkParams p) {
  const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (j >= p.n_runs) return;
  bool bin = true, chunk = true;
  if (j > 0) {
    bin = p.skey[j] != p.skey[j - 1];
    chunk = bin || !bai::merges(p.run_end[p.ord[j - 1]], p.run_beg[p.ord[j]]);
  }
  p.bin_flag[j] = bin ? 1 : 0;
  p.chunk_flag[j] = chunk ? 1 : 0;
}

__global__ __launch_bounds__(256) void bai_chunks_kernel(const BaiChunkParams p) {
  const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (j > p.n_runs) return;
  const bool has_cur = j < p.n_runs, has_prev = j > 0;
  const bool chunk = has_cur && p.chunk_flag[j], bin = has_cur && p.bin_flag[j];
  const uint64_t c = p.chunk_idx[j], b = p.bin_idx[j];
  if (chunk) {
    p.chunk_beg[c] = p.run_beg[p.ord[j]];
    p.chunk_bin[c] = (uint32_t)(b + (bin ? 1 : 0) - 1);
  }
  if (has_prev && (!has_cur || chunk)) p.chunk_end[c - 1] = p.run_end[p.ord[j - 1]];
  if (bin) {
    p.bin_key[b] = p.skey[j];
    p.bin_chunk0[b] = c;
  }
  if (!has_cur) p.bin_chunk0[b] = c;  // [n_bins] = n_chunks
  const uint32_t rc = has_cur ? bai::key_ref(p.skey[j]) : NO_REF - 1, rp = has_prev ? bai::key_ref(p.skey[j - 1]) : NO_REF;
  if (rc != rp) {
    if (has_cur) p.ref_bin0[rc] = b;
    if (has_prev) p.ref_bin1[rp] = b;
  }
}

__global__ __launch_bounds__(256) void bai_linear_kernel(const BaiLinearParams p) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= p.n) return;
  const uint32_t bw = p.beg[i];
  if (!(bw & bai::MAPPED_BIT)) return;
  const uint32_t beg = bw & ~bai::MAPPED_BIT, r = bai::key_ref(p.key[i]);
  const uint32_t w0 = bai::first_window(beg), w1 = bai::last_window(p.end[i]);  // w1 < n_intv of r: fields took the maximum
  ull* t = p.table + p.intv_off[r];
  const ull at = p.off[i];
  bool prev_same = false;
  uint32_t prev_beg = 0;
  if (i > 0) {
    const uint32_t pw = p.beg[i - 1];
    prev_same = bai::key_ref(p.key[i - 1]) == r && (pw & bai::MAPPED_BIT);
    prev_beg = pw & ~bai::MAPPED_BIT;
  }
  if (bai::enters_first_window(prev_same, prev_beg, beg)) atomicMin(&t[w0], at);
  for (uint32_t w = w0 + 1; w <= w1; w++) atomicMin(&t[w], at);
}

__device__ inline uint64_t shfl_up_u64(uint64_t v, int d) {
  const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d);
  return (uint64_t)hi << 32 | lo;
}
__device__ inline uint64_t shfl_u64(uint64_t v, int lane) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, lane), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), lane);
  return (uint64_t)hi << 32 | lo;
}

// one wavefront per reference, 64 windows a step from the top down; lane 0 has the topmost window of the step
__global__ __launch_bounds__(64) void bai_fill_kernel(const BaiLinearParams p) {
  const uint32_t r = blockIdx.x, lane = threadIdx.x;
  const uint64_t lo = p.intv_off[r];
  uint64_t carry = bai::NONE;
  for (uint64_t top = p.intv_off[r + 1]; top > lo;) {
    const uint64_t cnt = top - lo < 64 ? top - lo : 64;
    const bool in = lane < cnt;
    const uint64_t at = in ? top - 1 - lane : lo;
    uint64_t v = in ? (uint64_t)p.table[at] : bai::NONE;
    for (int d = 1; d < 64; d <<= 1) {
      const uint64_t u = shfl_up_u64(v, d);
      if ((int)lane >= d) v = bai::fill(v, u);
    }
    v = bai::fill(v, carry);
    if (in) p.table[at] = v;
    carry = shfl_u64(v, 63);  // (lanes past cnt hold the lowest window's value)
    top -= cnt;
  }
}

__global__ __launch_bounds__(256) void bai_ref_sizes_kernel(const BaiEmitParams p) {
  const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (r >= p.n_sq) return;
  const uint64_t b0 = p.ref_bin0[r], b1 = p.ref_bin1[r];
  p.ref_size[r] = bai::ref_bytes(b1 - b0, p.bin_chunk0[b1] - p.bin_chunk0[b0], p.ref_end[r] > p.ref_first[r], p.ref_intv[r]);
}

__global__ __launch_bounds__(256) void bai_emit_refs_kernel(const BaiEmitParams p) {
  const uint32_t r = blockIdx.x;
  if (r == 0 && threadIdx.x == 0) {
    bai::put32(p.out, 0, 0x01494142u);  // "BAI\1"
    bai::put32(p.out, 4, p.n_sq);
    bai::put64(p.out, p.n_bytes - bai::TAIL_BYTES, p.n_no_coor);
  }
  if (r >= p.n_sq) return;
  const uint64_t at = bai::HEAD_BYTES + p.ref_at[r];
  const uint64_t b0 = p.ref_bin0[r], b1 = p.ref_bin1[r], nb = b1 - b0, nc = p.bin_chunk0[b1] - p.bin_chunk0[b0];
  const uint64_t first = p.ref_first[r], end = p.ref_end[r], n_intv = p.ref_intv[r];
  const bool has = end > first;
  const uint64_t lin = bai::linear_at(at, nb, nc, has);
  if (threadIdx.x == 0) {
    bai::put32(p.out, at, (uint32_t)(nb + (has ? 1 : 0)));
    if (has) {
      const uint64_t ps = bai::bin_at(at, nb, nc);
      bai::put32(p.out, ps, bai::PSEUDO_BIN);
      bai::put32(p.out, ps + 4, 2);
      bai::put64(p.out, ps + 8, bai::voff(p.coff, p.off[first]));
      bai::put64(p.out, ps + 16, bai::voff(p.coff, p.off[end]));
      bai::put64(p.out, ps + 24, p.ref_mapped[r]);
      bai::put64(p.out, ps + 32, end - first - p.ref_mapped[r]);
    }
    bai::put32(p.out, lin, (uint32_t)n_intv);
  }
  const unsigned long long* t = p.table + p.intv_off[r];
  for (uint64_t w = threadIdx.x; w < n_intv; w += 256) bai::put64(p.out, lin + 4 + 8 * w, bai::voff(p.coff, t[w]));
}

__global__ __launch_bounds__(256) void bai_emit_chunks_kernel(const BaiEmitParams p) {
  const uint64_t c = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (c >= p.n_chunks) return;
  const uint64_t b = p.chunk_bin[c], k = p.bin_key[b];
  const uint32_t r = bai::key_ref(k);
  const uint64_t b0 = p.ref_bin0[r], c0 = p.bin_chunk0[b];
  const uint64_t at = bai::bin_at(bai::HEAD_BYTES + p.ref_at[r], b - b0, c0 - p.bin_chunk0[b0]);
  if (c == c0) {
    bai::put32(p.out, at, bai::key_bin(k));
    bai::put32(p.out, at + 4, (uint32_t)(p.bin_chunk0[b + 1] - c0));
  }
  const uint64_t ca = bai::chunk_at(at, c - c0);
  bai::put64(p.out, ca, bai::voff(p.coff, p.chunk_beg[c]));
  bai::put64(p.out, ca + 8, bai::voff(p.coff, p.chunk_end[c]));
}

}  // namespace dev

static unsigned bai_blocks(uint64_t n) { return (unsigned)((n + 255) / 256); }

hipError_t launch_bai_fields(const BaiFieldsParams& p, hipStream_t s) {
  if (p.r.n == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::bai_fields_kernel, dim3(bai_blocks(p.r.n)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_bai_run_heads(const BaiRunParams& p, hipStream_t s) {
  hipLaunchKernelGGL(dev::bai_run_heads_kernel, dim3(bai_blocks(p.n + 1)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_bai_runs(const BaiRunParams& p, hipStream_t s) {
  hipLaunchKernelGGL(dev::bai_runs_kernel, dim3(bai_blocks(p.n + 1)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_bai_chunk_heads(const BaiChunkParams& p, hipStream_t s) {
  if (p.n_runs == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::bai_chunk_heads_kernel, dim3(bai_blocks(p.n_runs)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_bai_chunks(const BaiChunkParams& p, hipStream_t s) {
  if (p.n_runs == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::bai_chunks_kernel, dim3(bai_blocks(p.n_runs + 1)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_bai_linear(const BaiLinearParams& p, hipStream_t s) {
  if (p.n == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::bai_linear_kernel, dim3(bai_blocks(p.n)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_bai_fill(const BaiLinearParams& p, hipStream_t s) {
  if (p.n_sq == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::bai_fill_kernel, dim3(p.n_sq), dim3(64), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_bai_ref_sizes(const BaiEmitParams& p, hipStream_t s) {
  if (p.n_sq == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::bai_ref_sizes_kernel, dim3(bai_blocks(p.n_sq)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_bai_emit(const BaiEmitParams& p, hipStream_t s) {
  hipLaunchKernelGGL(dev::bai_emit_refs_kernel, dim3(p.n_sq ? p.n_sq : 1), dim3(256), 0, s, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || p.n_chunks == 0) return e;
  hipLaunchKernelGGL(dev::bai_emit_chunks_kernel, dim3(bai_blocks(p.n_chunks)), dim3(256), 0, s, p);
  return hipGetLastError();
}

}  // namespace thm
