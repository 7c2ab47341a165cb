// kernels_swg.hip -- operator-level kernel: a batch of independent
// SwgExtend::extend problems (reference src/swg.rs:31-167), one problem per
// wavefront, pulled from a device work queue.  This is the surface the
// reference's known-answer tests pin (src/swg.rs:249-317).
#include <hip/hip_runtime.h>

#include "launch.h"
#include "swg_device.h"

namespace thm {
namespace dev {

// per-wave layout of the any-width variant's slice of global memory (CPL == 0)
struct SwgSlowLayout {
  uint64_t xs, ys, ops, dp, trace, total;
  uint32_t dp_stride, ops_cap;
};
__host__ __device__ inline SwgSlowLayout swg_slow_layout(uint32_t x_cap, uint32_t y_cap, uint32_t max_bw) {
  SwgSlowLayout s;
  uint64_t o = 0;
  auto take = [&](uint64_t bytes) {
    const uint64_t at = o;
    o += (bytes + 63u) & ~63ull;
    return at;
  };
  s.ops_cap = x_cap + y_cap + 16;
  s.xs = take(x_cap);
  s.ys = take(y_cap);
  s.ops = take(s.ops_cap);
  const uint32_t tiles = (2u * max_bw + 1u + 63u) / 64u;
  s.dp_stride = tiles * 64u + 64u;
  s.dp = take((uint64_t)s.dp_stride * 16u);
  s.trace = take((uint64_t)(y_cap + 2u) * tiles * 16u);
  s.total = o;
  return s;
}

// CPL = band slots per lane (1..4), or 0: band of any width (swg_extend_tiled, buffers in global memory)
template <int CPL>
__global__ __launch_bounds__(256) void swg_batch_kernel(SwgBatchParams p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int lane = lane_id();
  const int wave = bcast_first((int)(threadIdx.x >> 6));  // wave-uniform: LDS bases stay on the scalar unit
  uint8_t *xs, *ys, *opsb;
  unsigned long long* trace;
  int* dp = nullptr;
  int dp_stride = 0;
  uint32_t ops_cap;
  if constexpr (CPL == 0) {
    const SwgSlowLayout sl = swg_slow_layout(p.x_cap, p.y_cap, p.max_bw);
    uint8_t* base = p.scratch + (size_t)(blockIdx.x * (blockDim.x >> 6) + (unsigned)wave) * p.scratch_per_wave;
    xs = base + sl.xs;
    ys = base + sl.ys;
    opsb = base + sl.ops;
    trace = (unsigned long long*)(base + sl.trace);
    dp = (int*)(base + sl.dp);
    dp_stride = (int)sl.dp_stride;
    ops_cap = sl.ops_cap;
  } else {
    const uint32_t tr_bytes = (p.y_cap + 1) * CPL * 16;
    ops_cap = p.x_cap + p.y_cap + 16;
    const uint32_t per_wave = p.x_cap + p.y_cap + tr_bytes + ops_cap;
    uint8_t* base = smem + (size_t)wave * per_wave;
    xs = base;
    ys = xs + p.x_cap;
    trace = (unsigned long long*)(ys + p.y_cap);
    opsb = (uint8_t*)trace + tr_bytes;
  }
  auto sync = [] {
    if (CPL == 0)
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    else
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  };

  unsigned long long n_cells = 0, n_cols = 0, n_calls = 0;
  constexpr unsigned QCHUNK = 8;  // problems per queue atomic (a single hot word serves ~88 M atomics/s)
  unsigned q_next = 0, q_end = 0;
  for (;;) {
    if (q_next == q_end) {
      unsigned g = 0;
      if (lane == 0) g = atomicAdd(p.queue, QCHUNK);
      g = (unsigned)bcast_first((int)g);
      if (g >= p.n) break;
      q_next = g;
      q_end = (unsigned)min((uint64_t)g + QCHUNK, p.n);
    }
    const unsigned idx = q_next++;
    const uint64_t x0 = p.xo[idx], y0 = p.yo[idx];
    const int xlen = (int)(p.xo[idx + 1] - x0);
    const int ylen_full = (int)(p.yo[idx + 1] - y0);
    const int bw = (int)p.bw[idx];
    const int xd = p.xd[idx];
    // only the first xlen+bw+1 columns are reachable
    const int ylen = min(ylen_full, xlen + bw + 1);
    #pragma unroll 1
    for (int t = lane; t < xlen; t += 64) xs[t] = p.xb[x0 + t];
    #pragma unroll 1
    for (int t = lane; t < ylen; t += 64) ys[t] = p.yb[y0 + t];
    sync();

    SwgResult r;
    int nops;
#ifndef THM_NO_SHORTCUT
    if (swg_one_mismatch_shortcut(xs, 1, xlen, ys, 1, ylen, xd, opsb + ops_cap - 1, -1, (int)ops_cap, r, nops)) {
      // result known without DP (swg_device.h)
    } else
#endif
    if constexpr (CPL == 0) {
      r = swg_extend_tiled(xs, 1, xlen, ys, 1, ylen, bw, xd, trace, dp, dp_stride);
      sync();
      nops = swg_traceback_tiled(trace, r.xend, r.yend, bw, opsb + ops_cap - 1, -1, (int)ops_cap);
    } else {
      r = swg_extend_wave<(CPL > 0 ? CPL : 1)>(xs, 1, xlen, ys, 1, ylen, bw, xd, trace);
      sync();
      // path from the max cell back to the origin, laid out so that it reads forward
      nops = swg_traceback_wave<(CPL > 0 ? CPL : 1)>(trace, r.xend, r.yend, bw, opsb + ops_cap - 1, -1, (int)ops_cap);
    }
    sync();
    if (nops < 0) {
      if (lane == 0) atomicExch(p.fault, 1);
      nops = 0;
    }
    uint8_t* out = p.ops + p.ops_off[idx];
    const uint8_t* src = opsb + ops_cap - nops;
    #pragma unroll 1
    for (int t = lane; t < nops; t += 64) out[t] = src[t];
    uint32_t total = (uint32_t)nops;
    if (r.xend < xlen) {  // reference :178-180 Xclip(len - i), last after the reverse
      if (lane == 0) {
        const uint32_t clip = (uint32_t)(xlen - r.xend);
        out[nops] = THM_OP_XCLIP;
        out[nops + 1] = (uint8_t)(clip);
        out[nops + 2] = (uint8_t)(clip >> 8);
        out[nops + 3] = (uint8_t)(clip >> 16);
        out[nops + 4] = (uint8_t)(clip >> 24);
      }
      total += 5;
    }
    if (lane == 0) {
      thm_swg_aln a;
      a.ops_off = p.ops_off[idx];
      a.ops_len = total;
      a.score = r.score;
      a.xend = (uint32_t)r.xend;
      a.yend = (uint32_t)r.yend;
      p.out[idx] = a;
    }
    n_cells += r.cells;
    n_cols += r.cols;
    n_calls += 1;
  }
  if (lane == 0 && n_calls) {
    atomicAdd(&p.counters[THM_CNT_SWG_CALLS], n_calls);
    atomicAdd(&p.counters[THM_CNT_DP_CELLS], n_cells);
    atomicAdd(&p.counters[THM_CNT_DP_COLS], n_cols);
  }
}

// per-wave layout of extend_left_right's any-width variant (CPL == 0): one side's x and y at a time, the op buffer
// holds both sides (left from the front, right from the back)
struct ElrSlowLayout {
  uint64_t xs, ys, ops, dp, trace, total;
  uint32_t dp_stride, ops_cap;
};
__host__ __device__ inline uint32_t elr_ops_cap(uint32_t x_cap, uint32_t y_cap) { return 2u * (x_cap + y_cap) + 16u; }
__host__ __device__ inline ElrSlowLayout elr_slow_layout(uint32_t x_cap, uint32_t y_cap, uint32_t max_bw) {
  ElrSlowLayout s;
  uint64_t o = 0;
  auto take = [&](uint64_t bytes) {
    const uint64_t at = o;
    o += (bytes + 63u) & ~63ull;
    return at;
  };
  s.ops_cap = elr_ops_cap(x_cap, y_cap);
  s.xs = take(x_cap);
  s.ys = take(y_cap);
  s.ops = take(s.ops_cap);
  const uint32_t tiles = (2u * max_bw + 1u + 63u) / 64u;
  s.dp_stride = tiles * 64u + 64u;
  s.dp = take((uint64_t)s.dp_stride * 16u);
  s.trace = take((uint64_t)(y_cap + 2u) * tiles * 16u);
  s.total = o;
  return s;
}

// extend_left_right (reference src/aligner.rs:352-407), one problem per wavefront, pulled from the work queue.  The
// right side's x / y and then the left side's reversed copies are staged into the same buffers, and each goes through
// the SwgExtend::extend of swg_device.h.  The left traceback writes walk order (end cell first) from the front of the op
// buffer -- that is rev(left.operations) -- and the right one writes forward order from the back, as extend_lr does.
// CPL as in swg_batch_kernel.
template <int CPL>
__global__ __launch_bounds__(256) void elr_batch_kernel(ElrBatchParams p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int lane = lane_id();
  const int wave = bcast_first((int)(threadIdx.x >> 6));
  uint8_t *xs, *ys, *opsb;
  unsigned long long* trace;
  int* dp = nullptr;
  int dp_stride = 0;
  uint32_t ops_cap;
  if constexpr (CPL == 0) {
    const ElrSlowLayout sl = elr_slow_layout(p.x_cap, p.y_cap, p.max_bw);
    uint8_t* base = p.scratch + (size_t)(blockIdx.x * (blockDim.x >> 6) + (unsigned)wave) * p.scratch_per_wave;
    xs = base + sl.xs;
    ys = base + sl.ys;
    opsb = base + sl.ops;
    trace = (unsigned long long*)(base + sl.trace);
    dp = (int*)(base + sl.dp);
    dp_stride = (int)sl.dp_stride;
    ops_cap = sl.ops_cap;
  } else {
    const uint32_t tr_bytes = (p.y_cap + 1) * CPL * 16;
    ops_cap = elr_ops_cap(p.x_cap, p.y_cap);
    const uint32_t per_wave = p.x_cap + p.y_cap + tr_bytes + ops_cap;
    uint8_t* base = smem + (size_t)wave * per_wave;
    xs = base;
    ys = xs + p.x_cap;
    trace = (unsigned long long*)(ys + p.y_cap);
    opsb = (uint8_t*)trace + tr_bytes;
  }
  auto sync = [] {
    if (CPL == 0)
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    else
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  };
  // one SwgExtend::extend of the staged x / y; ops written from `ops` with `stride`, at most max_ops of them
  auto extend = [&](int xlen, int ylen, int bw, int xd, uint8_t* ops, int stride, int max_ops, SwgResult& r) {
    int nops;
    if (swg_one_mismatch_shortcut(xs, 1, xlen, ys, 1, ylen, xd, ops, stride, max_ops, r, nops)) {
      // result known without DP (swg_device.h)
    } else if constexpr (CPL == 0) {
      r = swg_extend_tiled(xs, 1, xlen, ys, 1, ylen, bw, xd, trace, dp, dp_stride);
      sync();
      nops = swg_traceback_tiled(trace, r.xend, r.yend, bw, ops, stride, max_ops);
    } else {
      r = swg_extend_wave<(CPL > 0 ? CPL : 1)>(xs, 1, xlen, ys, 1, ylen, bw, xd, trace);
      sync();
      nops = swg_traceback_wave<(CPL > 0 ? CPL : 1)>(trace, r.xend, r.yend, bw, ops, stride, max_ops);
    }
    sync();
    return nops;
  };

  unsigned long long n_cells = 0, n_cols = 0, n_calls = 0;
  constexpr unsigned QCHUNK = 8;
  unsigned q_next = 0, q_end = 0;
  for (;;) {
    if (q_next == q_end) {
      unsigned g = 0;
      if (lane == 0) g = atomicAdd(p.queue, QCHUNK);
      g = (unsigned)bcast_first((int)g);
      if (g >= p.n) break;
      q_next = g;
      q_end = (unsigned)min((uint64_t)g + QCHUNK, p.n);
    }
    const unsigned idx = q_next++;
    const uint64_t x0 = p.xo[idx], y0 = p.yo[idx];
    const int L = (int)(p.xo[idx + 1] - x0);
    const int64_t ylen_full = (int64_t)(p.yo[idx + 1] - y0);
    const thm_mem h = p.hits[idx];
    const int q = (int)h.query_idx, len = (int)h.len;
    const int64_t r = (int64_t)h.ref_idx;
    const int bw = (int)p.bw[idx];
    const int xd = p.xd[idx];
    // right: x = read[q+len..], y = ref[r+len..], of which the first |x| + bw + 1 columns are reachable
    const int xr = L - (q + len);
    const int yr = (int)min(ylen_full - (r + len), (int64_t)(xr + bw + 1));
    // left, both reversed: x = read[..q], y = ref[r.saturating_sub(L + bw)..r]   (:364-375)
    const int xl = q;
    const int yl = (int)min(r - (r > L + bw ? r - (L + bw) : (int64_t)0), (int64_t)(xl + bw + 1));
    #pragma unroll 1
    for (int t = lane; t < xr; t += 64) xs[t] = p.xb[x0 + q + len + t];
    #pragma unroll 1
    for (int t = lane; t < yr; t += 64) ys[t] = p.yb[y0 + r + len + t];
    sync();
    SwgResult R, Lt;
    int nr = extend(xr, yr, bw, xd, opsb + ops_cap - 1, -1, (int)ops_cap, R);
    #pragma unroll 1
    for (int t = lane; t < xl; t += 64) xs[t] = p.xb[x0 + q - 1 - t];
    #pragma unroll 1
    for (int t = lane; t < yl; t += 64) ys[t] = p.yb[y0 + r - 1 - t];
    sync();
    int nl = extend(xl, yl, bw, xd, opsb, 1, (int)ops_cap - max(nr, 0), Lt);
    if (nr < 0 || nl < 0) {
      if (lane == 0) atomicExch(p.fault, 1);
      nr = nl = 0;
    }
    // [Xclip(q - left.xend)] rev(left ops) Match x len right ops [Xclip(|x_r| - right.xend)]
    const int lead = xl - Lt.xend, trail = xr - R.xend;
    const int lead5 = lead > 0 ? 5 : 0, trail5 = trail > 0 ? 5 : 0;
    const int total = lead5 + nl + len + nr + trail5;
    uint8_t* out = p.ops + p.ops_off[idx];
    auto put5 = [&](int pos, uint32_t v) {
      out[pos] = THM_OP_XCLIP;
      out[pos + 1] = (uint8_t)v;
      out[pos + 2] = (uint8_t)(v >> 8);
      out[pos + 3] = (uint8_t)(v >> 16);
      out[pos + 4] = (uint8_t)(v >> 24);
    };
    #pragma unroll 1
    for (int t = lane; t < nl; t += 64) out[lead5 + t] = opsb[t];
    #pragma unroll 1
    for (int t = lane; t < len; t += 64) out[lead5 + nl + t] = (uint8_t)OPK_MATCH;
    #pragma unroll 1
    for (int t = lane; t < nr; t += 64) out[lead5 + nl + len + t] = opsb[ops_cap - nr + t];
    if (lane == 0 && lead > 0) put5(0, (uint32_t)lead);
    if (lane == 1 && trail > 0) put5(total - 5, (uint32_t)trail);
    if (lane == 0) {
      thm_lr_aln a;
      a.ystart = (uint64_t)(r - Lt.yend);
      a.yend = (uint64_t)(r + len + R.yend);
      a.ylen = (uint64_t)ylen_full;
      a.ops_off = p.ops_off[idx];
      a.score = Lt.score + len * MATCH_SCORE + R.score;
      a.xstart = (uint32_t)(q - Lt.xend);
      a.xend = (uint32_t)(q + len + R.xend);
      a.xlen = (uint32_t)L;
      a.ops_len = (uint32_t)total;
      a.pad_ = 0;
      p.out[idx] = a;
    }
    sync();  // the op buffer and x / y are rewritten by the next problem
    n_cells += R.cells + Lt.cells;
    n_cols += R.cols + Lt.cols;
    n_calls += 2;
  }
  if (lane == 0 && n_calls) {
    atomicAdd(&p.counters[THM_CNT_SWG_CALLS], n_calls);
    atomicAdd(&p.counters[THM_CNT_DP_CELLS], n_cells);
    atomicAdd(&p.counters[THM_CNT_DP_COLS], n_cols);
  }
}

// wave primitive self-test (checked against numpy on the GPU box)
__global__ void wave_prims_kernel(const int* in, int* out) {
  const int l = lane_id();
  const int v = in[l];
  out[l] = wave_incl_max_scan(v);
  out[64 + l] = wave_excl_max_scan(v);
  out[128 + l] = wave_max(v);
  out[192 + l] = wave_min(v);
  out[256 + l] = wave_shr1(v, -7);
  out[320 + l] = wave_shl1(v, -9);
}

}  // namespace dev

size_t swg_batch_scratch_bytes(const SwgBatchParams& p) { return (size_t)dev::swg_slow_layout(p.x_cap, p.y_cap, p.max_bw).total; }

size_t swg_batch_lds_bytes(const SwgBatchParams& p, int cpl) {
  if (cpl == 0) return 0;
  const size_t tr = (size_t)(p.y_cap + 1) * cpl * 16;
  return 4 * ((size_t)p.x_cap + p.y_cap + tr + p.x_cap + p.y_cap + 16);
}

hipError_t launch_swg_batch(const SwgBatchParams& p, int cpl, int n_blocks, hipStream_t s) {
  const size_t lds = swg_batch_lds_bytes(p, cpl);
  auto go = [&](auto kern) { return launch_with_lds(kern, n_blocks, 256, lds, s, p); };
  switch (cpl) {
    case 0: return go(dev::swg_batch_kernel<0>);
    case 1: return go(dev::swg_batch_kernel<1>);
    case 2: return go(dev::swg_batch_kernel<2>);
    case 3: return go(dev::swg_batch_kernel<3>);
    case 4: return go(dev::swg_batch_kernel<4>);
    default: return hipErrorInvalidValue;
  }
}

size_t elr_batch_scratch_bytes(const ElrBatchParams& p) { return (size_t)dev::elr_slow_layout(p.x_cap, p.y_cap, p.max_bw).total; }

size_t elr_batch_lds_bytes(const ElrBatchParams& p, int cpl) {
  if (cpl == 0) return 0;
  const size_t tr = (size_t)(p.y_cap + 1) * cpl * 16;
  return 4 * ((size_t)p.x_cap + p.y_cap + tr + dev::elr_ops_cap(p.x_cap, p.y_cap));
}

hipError_t launch_elr_batch(const ElrBatchParams& p, int cpl, int n_blocks, hipStream_t s) {
  const size_t lds = elr_batch_lds_bytes(p, cpl);
  auto go = [&](auto kern) { return launch_with_lds(kern, n_blocks, 256, lds, s, p); };
  switch (cpl) {
    case 0: return go(dev::elr_batch_kernel<0>);
    case 1: return go(dev::elr_batch_kernel<1>);
    case 2: return go(dev::elr_batch_kernel<2>);
    case 3: return go(dev::elr_batch_kernel<3>);
    case 4: return go(dev::elr_batch_kernel<4>);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_wave_prims(const int* in, int* out, hipStream_t s) {
  hipLaunchKernelGGL(dev::wave_prims_kernel, dim3(1), dim3(64), 0, s, in, out);
  return hipGetLastError();
}

}  // namespace thm
