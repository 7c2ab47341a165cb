// kernels_pileup.hip -- the device side of the per-base allele counts of a run (include/thermite_io.h: thm_pileup_add /
// _fetch / _window; host side pileup.hip; what one lane does with one item, the key of an event and the row of a position
// are pileup_device.h; the difference array is coverage_device.h's).
//
//   count    a group of pile::GROUP lanes per alignment, four alignments per wavefront, grid-stride: its read by binary
//            search (so NH), whether it is used, the checks that keep every later store inside the arrays, what its words
//            add up to, and -- the lanes a chunk each -- how many of its M bases differ from the text.  The totals are
//            summed in registers, per wavefront by shuffles, per workgroup in LDS, and reach global memory as one add per
//            total and workgroup.  Nothing is touched: after this pass the call can still refuse.
//   extract  the group again over the used alignments: all lanes walk the words together; within an M word each lane
//            loads pile::CHUNK consecutive SEQ bytes and text bytes as one word each (a reverse alignment's from the
//            read's end, turned round and complemented in registers), a scan over the group places its mismatches behind
//            the alignment's scanned offset; the lanes share a D word's bases; lane 0 writes an I word's one event.
//   heads, runs   over the sorted keys: where a key begins; then key and count (the distance to the next beginning)
//   lookup, update   the reduced rows against the running table, as kernels_quant.hip merges its junction rows
//   deposit  one thread per used alignment: diff[s] += 1 and diff[e] -= 1 (mod 2^32) per block, without a return value
//   bounds   the rows of a range of entries, by binary search
//   keep     one thread per row of the range: 1 where it begins a position whose events are min_alt or more
//   sites    one workgroup per tile of cov::TILE entries of the range: the tile's rows by binary search (none: it leaves
//            at once), the tile through LDS and scanned to depths, a row per kept position
//   window   the same tile pass over the tiles of a window, a row per position, its table rows found inside the tile's
#include <hip/hip_runtime.h>

#include "launch_io.h"
#include "pileup_device.h"
#include "summary_tile.h"

namespace thm {
namespace dev {

using ull = unsigned long long;
static_assert(pile::GROUP == 16 && pile::CHUNK == 8, "the kernels are written for groups of 16 lanes and chunks of one 64-bit word");
constexpr uint32_t PILE_GROUPS = 256 / pile::GROUP;  // alignments a workgroup works on at a time

// sum over the lanes of a group
__device__ inline uint64_t pile_group_sum(uint64_t v) {
  for (int d = 8; d >= 1; d >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 16), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 16);
    v += (uint64_t)hi << 32 | lo;
  }
  return v;
}
// exclusive scan of v over the lanes of a group, and the group's sum
__device__ inline uint32_t pile_group_scan(uint32_t v, uint32_t lane, uint32_t* total) {
  uint32_t inc = v;
  for (int d = 1; d < 16; d <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)inc, d, 16);
    if (lane >= (uint32_t)d) inc += o;
  }
  *total = (uint32_t)__shfl((int)inc, 15, 16);
  return inc - v;
}

// The walk of one checked alignment by its group.  WRITE: every event's key goes to keys[at ..), never at or behind
// `end`; otherwise the lane's share of the mismatches is returned (the deleted bases and the I words are in its Shape).
template <bool WRITE>
__device__ inline uint64_t pile_walk(const PileBatch& b, const thm_aln& al, const thm_aln_digest& d, uint32_t sq, uint64_t r, uint32_t lane, uint64_t* keys,
                                     uint64_t at, uint64_t end) {
  const uint8_t* text_c = b.text + b.tstart[sq];
  const uint64_t g_c = b.base[sq];
  const uint8_t* read = b.bases + b.base_off[r];
  const uint64_t read_len = b.base_off[r + 1] - b.base_off[r];
  const bool forward = al.strand == 1;
  const uint32_t* words = b.words + d.cigar_off;
  uint64_t p = al.ystart, q = 0, mine = 0;
  for (uint32_t i = 0; i < d.n_cigar; i++) {
    const uint32_t w = words[i], code = w & 15u;
    const uint64_t len = w >> 4;
    if (code == quant::OP_M) {
      // (the trip count depends on the word alone: the group stays together for the scan)
      for (uint64_t s0 = 0; s0 < len; s0 += pile::GROUP * pile::CHUNK) {
        const uint64_t c0 = s0 + lane * pile::CHUNK;
        uint32_t kinds = 0;
        const uint32_t mask = c0 < len ? pile::m_chunk(text_c, read, read_len, forward, p, q, len, c0, &kinds) : 0u;
        if (WRITE) {
          uint32_t total;
          uint64_t to = at + pile_group_scan(__popc(mask), lane, &total);
          for (uint32_t k = 0; k < pile::CHUNK; k++)
            if (mask >> k & 1u) {
              if (to < end) keys[to] = pile::key_of(g_c + p + c0 + k, kinds >> (4 * k) & 15u);
              to++;
            }
          at += total;
        } else {
          mine += __popc(mask);
        }
      }
      p += len;
      q += len;
    } else if (code == quant::OP_D) {
      if (WRITE) {
        for (uint64_t k = lane; k < len; k += pile::GROUP)
          if (at + k < end) keys[at + k] = pile::key_of(g_c + p + k, pile::KIND_DEL);
        at += len;
      }
      p += len;
    } else if (code == quant::OP_N) {
      p += len;
    } else if (code == quant::OP_I) {
      if (WRITE) {
        if (lane == 0 && at < end) keys[at] = pile::key_of(g_c + pile::ins_pos(p, al.ystart), pile::KIND_INS);
        at += 1;
      }
      q += len;
    } else if (code == quant::OP_S) {
      q += len;
    }
  }
  return mine;
}

__global__ __launch_bounds__(256) void pile_count_kernel(const PileCountParams p) {
  __shared__ ull sh_tot[pile::N_TOTALS];
  const PileBatch& b = p.b;
  uint64_t t[pile::N_TOTALS];
  for (int k = 0; k < pile::N_TOTALS; k++) t[k] = 0;
  if (threadIdx.x < pile::N_TOTALS) sh_tot[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t lane = threadIdx.x & (pile::GROUP - 1);
  const uint64_t n_groups = (uint64_t)gridDim.x * PILE_GROUPS, first_group = (uint64_t)blockIdx.x * PILE_GROUPS + threadIdx.x / pile::GROUP;
  for (uint64_t a = first_group; a < b.n_alns; a += n_groups) {
    const uint64_t r = quant::read_of(b.aln_off, b.n_reads, a);
    const bool multi = b.aln_off[r + 1] - b.aln_off[r] > 1;
    const thm_aln& al = b.alns[a];
    const thm_aln_digest& d = b.digests[a];
    const bool long_run = (d.flags & THM_DIGEST_LONG_RUN) != 0;
    bool used = !multi || (b.flags & THM_PILE_MULTI);
    uint32_t sq = 0;
    pile::Shape sh;
    if (!pile::check_aln(al.ref_id, al.ystart, d.cigar_off, d.n_cigar, long_run, b.words, b.n_words, b.ref_sq, b.n_refs, b.base, b.n_sq,
                         b.base_off[r + 1] - b.base_off[r], &sq, &sh)) {
      if (lane == 0) atomicMin(p.bad, (ull)a);
      used = false;
    }
    const uint64_t one = lane == 0 ? 1u : 0u;  // what the alignment has once is counted by its first lane
    uint64_t events = 0;
    t[pile::T_ALNS] += one;
    if (!used) {
      t[pile::T_SKIPPED_MULTI] += one;
    } else if (long_run) {
      t[pile::T_LONG_RUN] += one;
      used = false;
    } else {
      t[pile::T_USED] += one;
      t[pile::T_BLOCKS] += one * sh.n_blocks;
      t[pile::T_M_BASES] += one * sh.m_bases;
      t[pile::T_DEL_BASES] += one * sh.del_bases;
      t[pile::T_INS] += one * sh.ins;
      t[pile::T_INS_BASES] += one * sh.ins_bases;
      if (sh.end > al.ystart) {
        const uint64_t mine = pile_walk<false>(b, al, d, sq, r, lane, nullptr, 0, 0);
        t[pile::T_MISMATCHES] += mine;
        events = mine + one * (sh.del_bases + sh.ins);
      } else {
        used = false;  // (no reference base consumed: nothing to walk or deposit)
      }
    }
    events = pile_group_sum(events);
    if (lane == 0) {
      p.ev_cnt[a] = events;
      p.aln_read[a] = r;
      p.used[a] = used ? 1 : 0;
    }
  }
  read_totals(b, t[pile::T_READS], t[pile::T_FAILED]);
  block_totals(t, sh_tot, p.totals);
}

__global__ __launch_bounds__(256) void pile_extract_kernel(const PileExtractParams p) {
  const uint64_t a = (uint64_t)blockIdx.x * PILE_GROUPS + threadIdx.x / pile::GROUP;
  // (an alignment without events has nothing to write: its depth is the deposit's)
  if (a >= p.b.n_alns || !p.used[a] || p.ev_off[a + 1] == p.ev_off[a]) return;
  // (count has checked the ref, the words, the walk's end and the query length of every alignment it marked used)
  const thm_aln& al = p.b.alns[a];
  (void)pile_walk<true>(p.b, al, p.b.digests[a], (uint32_t)p.b.ref_sq[al.ref_id], p.aln_read[a], threadIdx.x & (pile::GROUP - 1), p.keys, p.ev_off[a],
                        p.ev_off[a + 1]);
}

__global__ __launch_bounds__(256) void pile_deposit_kernel(const PileExtractParams p) {
  const uint64_t a = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (a >= p.b.n_alns || !p.used[a]) return;
  const thm_aln& al = p.b.alns[a];
  const thm_aln_digest& d = p.b.digests[a];
  uint64_t end = 0;
  (void)cov::walk_blocks(p.b.words + d.cigar_off, d.n_cigar, al.ystart, BlockAdder{p.diff + p.b.base[p.b.ref_sq[al.ref_id]]}, &end);
}

__global__ __launch_bounds__(256) void pile_heads_kernel(const PileReduceParams p) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i < p.n) p.flag[i] = i == 0 || p.skey[i] != p.skey[i - 1] ? 1 : 0;
}

// where every key begins, then key and count: a key's count is the distance to the next key's beginning
__global__ __launch_bounds__(256) void pile_head_at_kernel(const PileReduceParams p) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i < p.n && p.flag[i] && p.first[i] < p.n_keys) p.head_at[p.first[i]] = i;
  if (i == 0) p.head_at[p.n_keys] = p.n;
}
__global__ __launch_bounds__(256) void pile_runs_kernel(const PileReduceParams p) {
  const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (k >= p.n_keys) return;
  const uint64_t at = p.head_at[k];
  p.red_key[k] = p.skey[at];
  p.red_cnt[k] = (uint32_t)(p.head_at[k + 1] - at);
}

__global__ __launch_bounds__(256) void pile_lookup_kernel(const PileMergeParams p) {
  const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (j >= p.n_red) return;
  const uint64_t key = p.red_key[j], at = pile::lower_bound(p.tab_key, 0, p.n_tab, key);
  const bool found = at < p.n_tab && p.tab_key[at] == key;
  p.where[j] = found ? at : ~0ull;
  p.is_new[j] = found ? 0 : 1;
}
// (the keys of the reduced rows are distinct: no two threads add to one row)
__global__ __launch_bounds__(256) void pile_update_kernel(const PileMergeParams p) {
  const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (j >= p.n_red) return;
  const uint64_t at = p.where[j];
  if (at != ~0ull) {
    const uint32_t sum = p.dst_cnt[at] + p.red_cnt[j];
    p.dst_cnt[at] = sum < p.red_cnt[j] ? 0xFFFFFFFFu : sum;  // (only an ins count can get there: it stays at the top)
  } else {
    p.dst_key[p.n_tab + p.new_at[j]] = p.red_key[j];
    p.dst_cnt[p.n_tab + p.new_at[j]] = p.red_cnt[j];
  }
}

__global__ void pile_bounds_kernel(const PileFetchParams p) {
  if (threadIdx.x < 2) p.bounds[threadIdx.x] = pile::lower_bound(p.keys, 0, p.n_tab, pile::key_of(threadIdx.x ? p.e1 : p.e0, 0));
}

__global__ __launch_bounds__(256) void pile_keep_kernel(const PileFetchParams p) {
  const uint64_t j = p.r0 + (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (j >= p.r1) return;
  const bool head = j == p.r0 || pile::key_entry(p.keys[j]) != pile::key_entry(p.keys[j - 1]);
  p.keep[j - p.r0] = head && pile::alt_of(p.keys, p.cnts, j, p.r1) >= p.min_alt ? 1 : 0;
}

__global__ __launch_bounds__(256) void pile_sites_kernel(const PileFetchParams p) {
  __shared__ uint32_t lds[COV_LDS];
  __shared__ uint32_t sh[8];
  const uint64_t tile = blockIdx.x, e0 = p.g0 + tile * cov::TILE;
  const uint64_t e1 = e0 + cov::TILE < p.g0 + p.n ? e0 + cov::TILE : p.g0 + p.n;
  // (the same two searches in every thread: the tile's rows, or none and the workgroup leaves together)
  const uint64_t lo = pile::lower_bound(p.keys, p.r0, p.r1, pile::key_of(e0, 0)), hi = pile::lower_bound(p.keys, lo, p.r1, pile::key_of(e1, 0));
  if (lo == hi) return;
  cov_tile_depths(p.diff, p.n, tile, (uint32_t)p.carry[tile], lds, sh);
  for (uint64_t j = lo + threadIdx.x; j < hi; j += 256u) {
    if (!p.keep[j - p.r0]) continue;
    const uint64_t at = p.site_at[j - p.r0], e = pile::key_entry(p.keys[j]);
    const uint32_t i = (uint32_t)(e - e0);
    if (at < p.n_sites) p.sites[at] = pile::site_of(p.keys, p.cnts, j, hi, e, lds[i + (i >> 4)], p.base, p.n_sq, p.tstart, p.text);
  }
}

__global__ __launch_bounds__(256) void pile_window_kernel(const PileFetchParams p) {
  __shared__ uint32_t lds[COV_LDS];
  __shared__ uint32_t sh[8];
  const uint64_t tile = p.start / cov::TILE + blockIdx.x, t0 = tile * cov::TILE;  // positions of the contig; p.n = start + the window's length
  const uint64_t t1 = t0 + cov::TILE < p.n ? t0 + cov::TILE : p.n;
  const uint64_t lo = pile::lower_bound(p.keys, p.r0, p.r1, pile::key_of(p.g0 + t0, 0)), hi = pile::lower_bound(p.keys, lo, p.r1, pile::key_of(p.g0 + t1, 0));
  cov_tile_depths(p.diff, p.n, tile, (uint32_t)p.carry[tile], lds, sh);
  for (uint32_t k = 0; k < cov::PER_THREAD; k++) {
    const uint32_t i = k * 256u + threadIdx.x;
    const uint64_t x = t0 + i;
    if (x < p.start || x >= p.n) continue;
    const uint64_t e = p.g0 + x;
    p.sites[x - p.start] = pile::site_of(p.keys, p.cnts, pile::lower_bound(p.keys, lo, hi, pile::key_of(e, 0)), hi, e, lds[i + (i >> 4)], p.base, p.n_sq,
                                         p.tstart, p.text);
  }
}

}  // namespace dev

hipError_t launch_pile_count(const PileCountParams& p, int n_cu, hipStream_t s) {
  const uint64_t by_alns = (p.b.n_alns + dev::PILE_GROUPS - 1) / dev::PILE_GROUPS, by_reads = (p.b.n_reads + 255) / 256;
  const uint64_t need = by_alns > by_reads ? by_alns : by_reads;
  if (need == 0) return hipSuccess;
  // grid-stride: enough workgroups to fill the device, few enough that each sums many items before its atomics
  const uint64_t cap = (uint64_t)(n_cu > 0 ? n_cu : 256) * 8;
  hipLaunchKernelGGL(dev::pile_count_kernel, dim3((unsigned)(need < cap ? need : cap)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_pile_extract(const PileExtractParams& p, hipStream_t s) {
  if (p.b.n_alns == 0) return hipSuccess;
  // (a group of lanes per alignment: PILE_GROUPS alignments a workgroup)
  hipLaunchKernelGGL(dev::pile_extract_kernel, dim3(blocks256(p.b.n_alns * pile::GROUP)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_pile_deposit(const PileExtractParams& p, hipStream_t s) {
  if (p.b.n_alns == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::pile_deposit_kernel, dim3(blocks256(p.b.n_alns)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_pile_heads(const PileReduceParams& p, hipStream_t s) {
  if (p.n == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::pile_heads_kernel, dim3(blocks256(p.n)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_pile_runs(const PileReduceParams& p, hipStream_t s) {
  if (p.n == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::pile_head_at_kernel, dim3(blocks256(p.n)), dim3(256), 0, s, p);
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  hipLaunchKernelGGL(dev::pile_runs_kernel, dim3(blocks256(p.n_keys)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_pile_lookup(const PileMergeParams& p, hipStream_t s) {
  if (p.n_red == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::pile_lookup_kernel, dim3(blocks256(p.n_red)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_pile_update(const PileMergeParams& p, hipStream_t s) {
  if (p.n_red == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::pile_update_kernel, dim3(blocks256(p.n_red)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_pile_bounds(const PileFetchParams& p, hipStream_t s) {
  hipLaunchKernelGGL(dev::pile_bounds_kernel, dim3(1), dim3(64), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_pile_keep(const PileFetchParams& p, hipStream_t s) {
  if (p.r1 == p.r0) return hipSuccess;
  hipLaunchKernelGGL(dev::pile_keep_kernel, dim3(blocks256(p.r1 - p.r0)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_pile_sites(const PileFetchParams& p, hipStream_t s) {
  if (p.n == 0 || p.n_sites == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::pile_sites_kernel, dim3((unsigned)cov::n_tiles(p.n)), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_pile_window(const PileFetchParams& p, hipStream_t s) {
  if (p.n == p.start) return hipSuccess;
  const uint64_t first = p.start / cov::TILE, last = (p.n - 1) / cov::TILE;
  hipLaunchKernelGGL(dev::pile_window_kernel, dim3((unsigned)(last - first + 1)), dim3(256), 0, s, p);
  return hipGetLastError();
}

}  // namespace thm
