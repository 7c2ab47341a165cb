// coverage_device.h -- what the kernels of the coverage tracks (kernels_coverage.hip) do per item, each a plain function
// of the item it works on: the track of an alignment, the walk over its genome CIGAR words that finds the covered blocks,
// the checks that keep every add inside the arrays, the layout of the difference arrays, the tile arithmetic of the
// fetch, and the run a change point makes with its successor.  They compile for the host too:
// tests/cpp/coverage_model_main.cpp drives the same functions serially, which is how the tracks are checked without a
// device.  The contract is in include/thermite_io.h above thm_coverage_create; DESIGN.md section 4.18 has the passes.
//
// Layout.  The contigs stand behind one another in @SQ order, each with one entry more than it has bases:
// base[s + 1] = base[s] + len[s] + 1, and a track is uint32[base[n_sq]].  A block [s, e) of contig c is diff[base[c] + s]
// += 1 and diff[base[c] + e] -= 1 (mod 2^32), e <= len[c], so the last entry of a contig only ever closes blocks: the
// prefix sum over the whole array is the depth, it is 0 on every contig's last entry, and therefore a prefix sum that
// begins at any contig's first entry needs no carry from the contigs before it.  A change point -- depth[x] != depth[x-1]
// -- is an entry with diff[x] != 0.
#ifndef THERMITE_COVERAGE_DEVICE_H
#define THERMITE_COVERAGE_DEVICE_H
#include <cstdint>

#include "quant_device.h"

#define COV_HD QUANT_HD

namespace thm {
namespace cov {

// The fetch works on tiles of TILE entries, counted from the first entry of the range it is asked for: a workgroup of
// TILE_THREADS threads per tile, PER_THREAD consecutive entries per thread.
constexpr uint32_t TILE_THREADS = 256, PER_THREAD = 16, TILE = TILE_THREADS * PER_THREAD;
static_assert(TILE <= 65536, "tests/cov_common.py places its tile shapes for tiles of at most 65 536 positions");
constexpr uint64_t MAX_DEPTH_WINDOW = 1ull << 24;
constexpr uint32_t NO_TRACK = 0xFFu;
constexpr uint32_t MAX_TRACKS = 4;
// the totals of one batch, in the order of thm_cov_totals
enum { T_READS = 0, T_FAILED, T_ALNS, T_SKIPPED_MULTI, T_LONG_RUN, T_TRACK0, N_TOTALS = T_TRACK0 + 3 * MAX_TRACKS };
static_assert(sizeof(thm_cov_totals) == N_TOTALS * 8, "the kernels index thm_cov_totals as an array");
static_assert(sizeof(thm_cov_run) == 24, "thm_cov_run is 24 bytes");

COV_HD uint32_t n_strands(uint32_t flags) { return (flags & THM_COV_STRANDED) ? 2u : 1u; }
COV_HD uint32_t n_tracks(uint32_t flags) { return n_strands(flags) * ((flags & THM_COV_MULTI) ? 2u : 1u); }
// the track of an alignment, or NO_TRACK for a multi-mapped one where those have no tracks
COV_HD uint32_t track_of(uint32_t flags, bool multi, bool forward) {
  if (multi && !(flags & THM_COV_MULTI)) return NO_TRACK;
  const uint32_t strand_idx = (flags & THM_COV_STRANDED) && !forward ? 1u : 0u;
  return (multi ? 1u : 0u) * n_strands(flags) + strand_idx;
}

// The walk over the n genome CIGAR words of an alignment that begins at ystart: emit(start, end) for every block, in
// order; returns the number of blocks.  *end_pos gets the position behind the last word, *bases (may be null) the summed
// block lengths.  Positions saturate nowhere: a word is below 2^28 bases and n below 2^32, so the sums stay below 2^60
// behind any ystart the checks let through.
template <class Emit>
COV_HD uint32_t walk_blocks(const uint32_t* words, uint32_t n, uint64_t ystart, Emit&& emit, uint64_t* end_pos, uint64_t* bases = nullptr) {
  uint64_t pos = ystart, begin = ystart, sum = 0;
  uint32_t n_blocks = 0;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t w = words[i], code = w & 15u;
    const uint64_t len = w >> 4;
    if (code == quant::OP_M || code == quant::OP_D) {
      pos += len;
    } else if (code == quant::OP_N) {
      if (pos > begin) {
        emit(begin, pos);
        sum += pos - begin;
        n_blocks++;
      }
      pos += len;
      begin = pos;
    }
  }
  if (pos > begin) {
    emit(begin, pos);
    sum += pos - begin;
    n_blocks++;
  }
  *end_pos = pos;
  if (bases) *bases = sum;
  return n_blocks;
}
struct NoBlock {
  COV_HD void operator()(uint64_t, uint64_t) const {}
};

// Where an alignment lies, before any array is touched: its ref has a refID below n_sq (-> *sq), its words lie inside the
// pool, and it begins inside its contig.  Returns the contig's length, NOT_LOCATED where one of these fails.  The first
// of the checks of every summary over this layout (check_aln below, pile::check_aln).
constexpr uint64_t NOT_LOCATED = ~0ull;
COV_HD uint64_t locate_aln(uint32_t ref_id, uint64_t ystart, uint64_t cigar_off, uint32_t n_cigar, uint64_t n_words, const int32_t* ref_sq, uint32_t n_refs,
                           const uint64_t* base, uint32_t n_sq, uint32_t* sq) {
  if (ref_id >= n_refs) return NOT_LOCATED;
  const int32_t s = ref_sq[ref_id];
  if (s < 0 || (uint32_t)s >= n_sq) return NOT_LOCATED;
  *sq = (uint32_t)s;
  if (cigar_off > n_words || (uint64_t)n_cigar > n_words - cigar_off) return NOT_LOCATED;
  const uint64_t len = base[s + 1] - base[s] - 1;
  return ystart > len ? NOT_LOCATED : len;
}

// The device's checks of one alignment, before any array is touched: locate_aln's, and the walk from ystart ends inside
// the contig.  *sq gets the refID; for an alignment with words *n_blocks and *bases what the walk counted.
COV_HD bool check_aln(uint32_t ref_id, uint64_t ystart, uint64_t cigar_off, uint32_t n_cigar, bool long_run, const uint32_t* words, uint64_t n_words,
                      const int32_t* ref_sq, uint32_t n_refs, const uint64_t* base, uint32_t n_sq, uint32_t* sq, uint32_t* n_blocks, uint64_t* bases) {
  *n_blocks = 0;
  *bases = 0;
  const uint64_t len = locate_aln(ref_id, ystart, cigar_off, n_cigar, n_words, ref_sq, n_refs, base, n_sq, sq);
  if (len == NOT_LOCATED) return false;
  if (long_run) return true;
  uint64_t end = 0;
  *n_blocks = walk_blocks(words + cigar_off, n_cigar, ystart, NoBlock(), &end, bases);
  return end <= len;
}

// the contig that holds entry g of the layout: the last s in [0, n_sq) with base[s] <= g
COV_HD uint32_t sq_of(const uint64_t* base, uint32_t n_sq, uint64_t g) {
  uint32_t lo = 0, hi = n_sq;
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (base[mid] <= g)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

COV_HD uint64_t n_tiles(uint64_t n_entries) { return (n_entries + TILE - 1) / TILE; }

// The run that the change point at entry g with depth d != 0 begins: up to its successor `next` (the entry of the next
// change point; ~0 where there is none), or to the contig's end where that comes first.
COV_HD thm_cov_run run_of(const uint64_t* base, uint32_t n_sq, uint64_t g, uint32_t d, uint64_t next) {
  const uint32_t s = sq_of(base, n_sq, g);
  const uint64_t end_entry = base[s + 1] - 1;  // the entry behind the contig's last base
  thm_cov_run r;
  r.ref_id = s;
  r.depth = d;
  r.start = g - base[s];
  r.end = (next < end_entry ? next : end_entry) - base[s];
  return r;
}

}  // namespace cov
}  // namespace thm
#endif
