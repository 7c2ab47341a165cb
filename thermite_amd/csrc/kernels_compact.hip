// kernels_compact.hip -- the last kernels of a step: the candidates the extend stage kept (launch.h, Cand) become the
// batch's thm_aln records and op streams in their final layout.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdlib>

#include "compact_copy.h"
#include "launch.h"

namespace thm {
namespace dev {

// ---- final layout: alignments of read r at alns[read_aln_off[r]..], op streams back to back in the same order (gx
// ops, then tx ops of an exonic alignment) ----
// A read's alignments follow one another in its op stream, so where an alignment's op bytes go is known only after the
// lengths of the read's earlier ones: a serial chain of dependent loads per read.  compact_kernel walks it in one thread
// per read, which is fine for a few alignments; with a read of 58 (the chr21-sized text) or 1 300 alignments (the
// 2.2 G-symbol text, whose repeat families are larger) the launch would last as long as that read.  Reads beyond
// COMPACT_HEAVY_N alignments therefore go through two more kernels: a scan of their op lengths (one workgroup per
// read), then the copies, four alignments per group, all groups of the grid at once.
constexpr uint32_t COMPACT_HEAVY_N = 8, COMPACT_CHUNK = 4;

// A candidate record as the 16 lanes of a group hold it: lane j its dwords j and 16 + j (Cand and thm_aln are 28 dwords
// each; two coalesced loads, two coalesced stores, and the record never occupies 28 registers of every lane).
struct CandRegs {
  uint32_t lo, hi;
};
static_assert(sizeof(Cand) == 112 && sizeof(thm_aln) == 112, "emit_record permutes the dwords of these layouts");
static_assert(offsetof(Cand, ops_off) == 48 && offsetof(Cand, tx_ops_off) == 56 && offsetof(Cand, score) == 64 &&
                  offsetof(Cand, ops_len) == 80 && offsetof(Cand, tx_ops_len) == 84 && offsetof(Cand, strand) == 108 &&
                  offsetof(thm_aln, ops_off) == 24 && offsetof(thm_aln, tx_ops_off) == 56 && offsetof(thm_aln, xlen) == 80 &&
                  offsetof(thm_aln, ops_len) == 84 && offsetof(thm_aln, tx_ops_len) == 104 && offsetof(thm_aln, strand) == 108,
              "emit_record permutes the dwords of these layouts");

__device__ __forceinline__ CandRegs cand_load(const Cand* c, int sub) {
  const uint32_t* w = reinterpret_cast<const uint32_t*>(c);
  CandRegs r;
  r.lo = w[sub];
  r.hi = sub < 12 ? w[16 + sub] : 0u;
  return r;
}

// the op pool and the batch's op bytes as compact_copy.h reaches them (both allocations start on a 256-byte boundary)
struct OpsMem {
  const uint8_t* src;
  uint8_t* dst;
  __device__ __forceinline__ uint32_t ld32(uint64_t o) const { return *reinterpret_cast<const uint32_t*>(src + o); }
  __device__ __forceinline__ uint32_t ld8(uint64_t o) const { return src[o]; }
  __device__ __forceinline__ void st32(uint64_t o, uint32_t v) { *reinterpret_cast<uint32_t*>(dst + o) = v; }
  __device__ __forceinline__ void st8(uint64_t o, uint8_t v) { dst[o] = v; }
};

// One alignment as a group moves it: the record, the genome op stream to ops[o..], the transcript op stream behind it.
// load() issues every load of the alignment (record, first 256 bytes of either stream) and store() none before all of
// them: several alignments of a group are in flight between the two.  Longer streams loop in store().
struct AlnCopy {
  CandRegs c;
  ccopy::LaneRegs gx, tx;
  uint64_t gx_src, tx_src, o;
  uint32_t gx_len, tx_len;

  __device__ __forceinline__ void load(const CompactParams& p, const Cand* cand, uint64_t gx_src_, uint64_t tx_src_, uint32_t gx_len_, uint32_t tx_len_,
                                       uint64_t o_, int sub) {
    gx_src = gx_src_, tx_src = tx_src_, gx_len = gx_len_, tx_len = tx_len_, o = o_;
    const OpsMem mem{p.cand_ops, p.ops};
    c = cand_load(cand, sub);
    ccopy::lane_load(mem, gx_src, o, gx_len, 0, sub, gx);
    ccopy::lane_load(mem, tx_src, o + gx_len, tx_len, 0, sub, tx);
  }

  // Between the loads and the stores: every load issued so far is back (vmcnt(0), the other counters left alone).  Said
  // once and outside any branch, because the stores stand in branches of their own and a wait the compiler places inside a
  // branch does not count for the code behind it: it waited before every single store, and on gfx9 that wait includes the
  // store before -- a round trip per store.
  static __device__ __forceinline__ void loads_done() { __builtin_amdgcn_s_waitcnt(0x0F70); }

  // after loads_done()
  __device__ __forceinline__ void store(const CompactParams& p, uint64_t ai, uint32_t xlen, bool primary, int sub) {
    OpsMem mem{p.cand_ops, p.ops};
    const uint64_t go = o, to = o + gx_len;
    ccopy::lane_store(mem, gx_src, go, gx_len, 0, sub, gx);
    ccopy::lane_store(mem, tx_src, to, tx_len, 0, sub, tx);
    #pragma unroll 1
    for (uint32_t trip = 1; trip < ccopy::trips(go, gx_len); trip++) {
      ccopy::lane_load(mem, gx_src, go, gx_len, trip, sub, gx);
      loads_done();
      ccopy::lane_store(mem, gx_src, go, gx_len, trip, sub, gx);
    }
    #pragma unroll 1
    for (uint32_t trip = 1; trip < ccopy::trips(to, tx_len); trip++) {
      ccopy::lane_load(mem, tx_src, to, tx_len, trip, sub, tx);
      loads_done();
      ccopy::lane_store(mem, tx_src, to, tx_len, trip, sub, tx);
    }
    // the record: thm_aln dword i comes from Cand dword src(i), or is one of ops_off / tx_ops_off / xlen / the flag bytes
    //   i        0  1  2  3  4  5  6  7  8  9 10 11 12 13 14 15 | 16 17 18 19 20 21 22 23 24 25 26 27
    //   src(i)   0  1  2  3  4  5  go go 6  7  8  9 10 11 to to | 16 17 18 19 xl 20 22 23 24 25 21 fl
    const uint32_t flags = __shfl(c.hi, 11, 16);
    const int src_lo = (int)((0x00BA987600543210ull >> (4 * sub)) & 15u);
    const int src_hi = (int)((0x0000B59876403210ull >> (4 * sub)) & 15u);  // (lane of c.hi = Cand dword - 16)
    uint32_t w0 = __shfl(c.lo, src_lo, 16), w1 = __shfl(c.hi, src_hi, 16);
    const uint64_t txo = ((flags >> 8) & 0xFFu) == THM_ALN_EXONIC ? to : 0ull;
    if (sub == 6) w0 = (uint32_t)go;
    if (sub == 7) w0 = (uint32_t)(go >> 32);
    if (sub == 14) w0 = (uint32_t)txo;
    if (sub == 15) w0 = (uint32_t)(txo >> 32);
    if (sub == 4) w1 = xlen;
    // Cand: strand, aln_type, primary, pad -> thm_aln: strand, primary (src/aligner.rs:185-187), aln_type, pad
    if (sub == 11) w1 = (flags & 0xFFu) | ((primary ? 1u : 0u) << 8) | (((flags >> 8) & 0xFFu) << 16);
    uint32_t* out = reinterpret_cast<uint32_t*>(p.alns + ai);
    out[sub] = w0;
    if (sub < 12) out[16 + sub] = w1;
  }
};

// a faulted attempt (pool overflow) is replayed by the host with larger pools: its counts and offsets are not to be trusted
__device__ __forceinline__ bool compact_faulted(const CompactParams& p) { return p.fault[0] != 0 || (p.fault[1] & FAULT_OPS_POOL) != 0; }

// One workgroup per tile of COMPACT_TILE consecutive reads, two phases.
//   A, a thread per read: the read's count, offsets and length (coalesced, independent loads), then for each of its
//      alignments the candidate's index (order[]) and the four words of the Cand that say where its op bytes are.  The
//      result is one descriptor per alignment in LDS, at the alignment's place within the tile: a tile's alignments
//      are a contiguous range of alns[].
//   B, a 16-lane group per alignment: the descriptor holds the record's index and both op sources, so a group issues
//      every load of K alignments at once and only then stores (AlnCopy).
// The descriptors of COMPACT_SLOTS alignments fit; a tile with more (a read beyond COMPACT_HEAVY_N alignments counts, its
// slots stay empty) goes through both phases once per COMPACT_SLOTS of them.
constexpr uint32_t COMPACT_TILE = 256, COMPACT_SLOTS = 512;
constexpr uint64_t NO_CAND = ~0ull;

template <int K>
__global__ __launch_bounds__(COMPACT_TILE) void compact_kernel(CompactParams p) {
  __shared__ uint64_t s_cand[COMPACT_SLOTS], s_gx[COMPACT_SLOTS], s_tx[COMPACT_SLOTS], s_o[COMPACT_SLOTS];
  __shared__ uint32_t s_gx_len[COMPACT_SLOTS], s_tx_len[COMPACT_SLOTS], s_xlen[COMPACT_SLOTS];
  __shared__ uint8_t s_primary[COMPACT_SLOTS];
  if (compact_faulted(p)) return;
  const uint32_t tid = threadIdx.x;
  const int sub = (int)(tid & 15u);
  const uint32_t grp = tid >> 4;
  const uint64_t r0 = (uint64_t)blockIdx.x * COMPACT_TILE, r = r0 + tid;
  const uint64_t r_end = min((unsigned long long)(r0 + COMPACT_TILE), (unsigned long long)p.n_reads);
  const uint64_t aln_base = p.read_aln_off[r0], n_slots = p.read_aln_off[r_end] - aln_base;
  uint32_t n = 0, xlen = 0;
  uint64_t cand0 = 0, a0 = 0, o = 0;
  if (r < p.n_reads) {
    n = p.read_n_alns[r];
    cand0 = p.read_cand_off[r];
    a0 = p.read_aln_off[r];
    o = p.read_ops_off[r];
    xlen = (uint32_t)(p.read_offsets[r + 1] - p.read_offsets[r]);
  }
  if (n > COMPACT_HEAVY_N) {
    const unsigned long long h = atomicAdd(&p.heavy_cnt[0], 1ull);
    if (h < p.heavy_cap) p.heavy_list[h] = r;
    n = 0;
  }
  uint32_t t = 0;  // the read's alignments before t have their descriptors
  for (uint64_t c0 = 0; c0 < n_slots; c0 += COMPACT_SLOTS) {
    const uint32_t cnt = (uint32_t)min((unsigned long long)COMPACT_SLOTS, (unsigned long long)(n_slots - c0));
    for (uint32_t i = tid; i < cnt; i += COMPACT_TILE) s_cand[i] = NO_CAND;
    __syncthreads();
    while (t < n && a0 + t - aln_base < c0 + COMPACT_SLOTS) {  // (one read in forty has a second alignment)
      const uint32_t slot = (uint32_t)(a0 + t - aln_base - c0);
      const uint64_t ci = cand0 + p.order[2 * cand0 + t];
      const Cand* cd = p.cands + ci;
      const uint64_t gx_src = cd->ops_off, tx_src = cd->tx_ops_off;
      const uint32_t gx_len = cd->ops_len, tx_len = cd->tx_ops_len;
      // never without a fault; keeps every store in bounds
      if (a0 + t < p.alns_cap && o + gx_len + tx_len <= p.ops_cap) {
        s_cand[slot] = ci;
        s_gx[slot] = gx_src;
        s_tx[slot] = tx_src;
        s_o[slot] = o;
        s_gx_len[slot] = gx_len;
        s_tx_len[slot] = tx_len;
        s_xlen[slot] = xlen;
        s_primary[slot] = t == 0;
      }
      o += gx_len + tx_len;
      t++;
    }
    __syncthreads();
    for (uint32_t b = 0; b < cnt; b += 16 * K) {
      AlnCopy ac[K];
      bool live[K];
      #pragma unroll
      for (int k = 0; k < K; k++) {
        const uint32_t d = b + grp + 16u * (uint32_t)k;
        live[k] = d < cnt && s_cand[d] != NO_CAND;
        if (live[k]) ac[k].load(p, p.cands + s_cand[d], s_gx[d], s_tx[d], s_gx_len[d], s_tx_len[d], s_o[d], sub);
      }
      AlnCopy::loads_done();
      #pragma unroll
      for (int k = 0; k < K; k++) {
        const uint32_t d = b + grp + 16u * (uint32_t)k;
        if (live[k]) ac[k].store(p, aln_base + c0 + d, s_xlen[d], s_primary[d] != 0, sub);
      }
    }
    __syncthreads();
  }
}

// heavy reads, step 1: rel[a0 + t] = op bytes of the read's alignments before t; one descriptor per COMPACT_CHUNK alignments
__global__ __launch_bounds__(256) void compact_heavy_scan_kernel(CompactParams p) {
  __shared__ uint32_t wave_sum[4];
  __shared__ unsigned long long desc_base;
  if (compact_faulted(p)) return;
  const uint64_t H = min((unsigned long long)p.heavy_cap, p.heavy_cnt[0]);
  const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (uint64_t h = blockIdx.x; h < H; h += gridDim.x) {
    const uint64_t r = p.heavy_list[h];
    const uint32_t n = p.read_n_alns[r];
    const uint64_t cand0 = p.read_cand_off[r], a0 = p.read_aln_off[r];
    const Cand* cands = p.cands + cand0;
    const uint32_t* la = p.order + 2 * cand0;
    uint32_t carry = 0;
    for (uint32_t tile = 0; tile < n; tile += 256) {
      const uint32_t t = tile + (uint32_t)tid;
      uint32_t len = 0;
      if (t < n) {
        const Cand* cd = &cands[la[t]];
        len = cd->ops_len + cd->tx_ops_len;
      }
      uint32_t inc = len;  // inclusive scan within the wave
      #pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(inc, o);
        if (lane >= o) inc += v;
      }
      if (lane == 63) wave_sum[wv] = inc;
      __syncthreads();
      uint32_t before = carry, total = 0;
      #pragma unroll
      for (int k = 0; k < 4; k++) {
        if (k < wv) before += wave_sum[k];
        total += wave_sum[k];
      }
      if (t < n && a0 + t < p.alns_cap) p.rel[a0 + t] = before + inc - len;
      carry += total;
      __syncthreads();
    }
    const uint32_t nd = (n + COMPACT_CHUNK - 1) / COMPACT_CHUNK;
    if (tid == 0) desc_base = atomicAdd(&p.heavy_cnt[1], (unsigned long long)nd);
    __syncthreads();
    const unsigned long long base = desc_base;
    for (uint32_t k = (uint32_t)tid; k < nd; k += 256)
      if (base + k < p.heavy_cap) p.heavy_desc[base + k] = (r << 24) | (uint64_t)k;
    __syncthreads();
  }
}

// heavy reads, step 2: a 16-lane group per descriptor
__global__ __launch_bounds__(256) void compact_heavy_copy_kernel(CompactParams p) {
  const int sub = (int)(threadIdx.x & 15u);
  if (compact_faulted(p)) return;
  const uint64_t D = min((unsigned long long)p.heavy_cap, p.heavy_cnt[1]);
  const uint64_t n_groups = (uint64_t)gridDim.x * 16;
  for (uint64_t d = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 4; d < D; d += n_groups) {
    const uint64_t desc = p.heavy_desc[d], r = desc >> 24;
    const uint32_t t0 = (uint32_t)(desc & 0xFFFFFFu) * COMPACT_CHUNK, n = p.read_n_alns[r];
    const uint64_t cand0 = p.read_cand_off[r], a0 = p.read_aln_off[r], o0 = p.read_ops_off[r];
    const Cand* cands = p.cands + cand0;
    const uint32_t* la = p.order + 2 * cand0;
    const uint32_t xlen = (uint32_t)(p.read_offsets[r + 1] - p.read_offsets[r]);
    for (uint32_t t = t0; t < n && t < t0 + COMPACT_CHUNK; t++) {
      if (a0 + t >= p.alns_cap) break;
      const Cand* cd = &cands[la[t]];
      const uint32_t gx_len = cd->ops_len, tx_len = cd->tx_ops_len;
      const uint64_t o = o0 + p.rel[a0 + t];
      if (o + gx_len + tx_len > p.ops_cap) continue;  // never without a fault; keeps every store in bounds
      AlnCopy ac;
      ac.load(p, cd, cd->ops_off, cd->tx_ops_off, gx_len, tx_len, o, sub);
      AlnCopy::loads_done();
      ac.store(p, a0 + t, xlen, t == 0, sub);
    }
  }
}

}  // namespace dev

// alignments in flight per 16-lane group in phase B of the compact kernel: 2 unless THM_COMPACT_K = 1 | 4 says otherwise (tuning;
// stage_ms.compact of the benchmark 0.144 / 0.136 / 0.161 ms at 1 / 2 / 4: four alignments in flight take 186 registers)
int compact_k() {
  static const int v = [] {
    const char* e = getenv("THM_COMPACT_K");
    const int v = e ? atoi(e) : 2;
    return v == 1 || v == 2 || v == 4 ? v : 2;
  }();
  return v;
}

hipError_t launch_compact(const CompactParams& p, hipStream_t s) {
  static const unsigned n_cu = [] {
    int dev = 0, cu = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev);
    return (unsigned)cu;
  }();
  // a workgroup per tile (1 954 for a batch of 500 000 reads, each alive for tens of microseconds): no stride loop
  const unsigned blocks = (unsigned)((p.n_reads + dev::COMPACT_TILE - 1) / dev::COMPACT_TILE);
  if (blocks == 0) return hipSuccess;
  const int k_alns = compact_k();
  if (k_alns == 1)
    hipLaunchKernelGGL(dev::compact_kernel<1>, dim3(blocks), dim3(dev::COMPACT_TILE), 0, s, p);
  else if (k_alns == 2)
    hipLaunchKernelGGL(dev::compact_kernel<2>, dim3(blocks), dim3(dev::COMPACT_TILE), 0, s, p);
  else
    hipLaunchKernelGGL(dev::compact_kernel<4>, dim3(blocks), dim3(dev::COMPACT_TILE), 0, s, p);
  // the reads left on the heavy list (counts on the device: both launches find them empty for most batches)
  hipLaunchKernelGGL(dev::compact_heavy_scan_kernel, dim3(n_cu), dim3(256), 0, s, p);
  hipLaunchKernelGGL(dev::compact_heavy_copy_kernel, dim3(n_cu * 4), dim3(256), 0, s, p);
  return hipGetLastError();
}

}  // namespace thm
