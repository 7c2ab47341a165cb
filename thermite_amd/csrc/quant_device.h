// quant_device.h -- what the kernels of the count tables (kernels_quant.hip) do per alignment, each a plain function of
// the item it works on: which gene counter an alignment adds to, the walk over its genome CIGAR words that finds the
// junction hits with their anchors, the 128-bit key of a hit, and the row a key unpacks to.  They compile for the host
// too: tests/cpp/quant_model_main.cpp drives the same functions serially, a std::map standing in for the sorts and the
// reduce-by-key, which is how the tables are checked without a device.  The contract is in include/thermite_io.h above
// thm_quant_create; DESIGN.md section 4.17 has the passes.
#ifndef THERMITE_QUANT_DEVICE_H
#define THERMITE_QUANT_DEVICE_H
#include <cstdint>

#include "../../include/thermite_io.h"

#if defined(__HIPCC__)
#define QUANT_HD __host__ __device__ inline
#else
#define QUANT_HD inline
#endif

namespace thm {
namespace quant {

constexpr uint32_t NO_COUNTER = 0xFFFFFFFFu;
constexpr uint32_t BAD_INDEX = 0xFFFFFFFEu;
// the totals of one batch, in the order of thm_quant_totals
enum { T_READS = 0, T_FAILED, T_UNMAPPED, T_UNIQUE_READS, T_MULTI_READS, T_ALNS, T_INTERGENIC_UNIQUE, T_INTERGENIC_MULTI, T_SPLICED,
       T_HITS, T_LONG_RUN, N_TOTALS };
static_assert(sizeof(thm_quant_totals) == N_TOTALS * 8, "the kernels index thm_quant_totals as an array");

// BAM CIGAR codes of the words (thm_aln_digest): M I D N S
enum { OP_M = 0, OP_I = 1, OP_D = 2, OP_N = 3, OP_S = 4 };

// The gene counter an alignment adds to, as an index into the gene table seen as uint64[n_genes * 4] (row = gene,
// column = exonic_unique, exonic_multi, intronic_unique, intronic_multi); NO_COUNTER for an intergenic alignment,
// BAD_INDEX where a table index is out of range.
QUANT_HD uint32_t gene_counter(uint32_t aln_type, uint32_t tx_or_gene_idx, bool multi, const uint32_t* tx_gene, uint32_t n_txs,
                               uint32_t n_genes) {
  uint32_t gene;
  uint32_t col = multi ? 1u : 0u;
  if (aln_type == THM_ALN_EXONIC) {
    if (tx_or_gene_idx >= n_txs) return BAD_INDEX;
    gene = tx_gene[tx_or_gene_idx];
  } else if (aln_type == THM_ALN_INTRONIC) {
    gene = tx_or_gene_idx;
    col += 2;
  } else if (aln_type == THM_ALN_INTERGENIC) {
    return NO_COUNTER;
  } else {
    return BAD_INDEX;
  }
  if (gene >= n_genes || n_genes > 0x3FFFFFFFu) return BAD_INDEX;
  return gene * 4u + col;
}

// One junction hit of an alignment: the intron [start, end) on the contig (0-based, half open) and its two anchors.
struct Hit {
  uint64_t start, end;
  uint32_t left, right;
};
QUANT_HD uint32_t overhang(const Hit& h) { return h.left < h.right ? h.left : h.right; }

// The walk over the n genome CIGAR words of an alignment that begins at ystart: emit(k, hit) for the k-th N word, in
// order; returns the number of hits.  M, D and N words move the position, M words lengthen the anchor, an N word ends
// one anchor and begins the next; I, D and S words add nothing to an anchor and interrupt none.  *end_pos (may be null)
// gets the position behind the last word.
template <class Emit>
QUANT_HD uint32_t walk(const uint32_t* words, uint32_t n, uint64_t ystart, Emit&& emit, uint64_t* end_pos = nullptr) {
  uint64_t pos = ystart;
  uint64_t anchor = 0;  // M bases since the last N word (or the start)
  uint32_t n_hits = 0;
  bool pending = false;
  Hit h{0, 0, 0, 0};
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t w = words[i], code = w & 15u;
    const uint64_t len = w >> 4;
    if (code == OP_M) {
      anchor += len;
      pos += len;
    } else if (code == OP_D) {
      pos += len;
    } else if (code == OP_N) {
      const uint32_t a32 = anchor > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)anchor;
      if (pending) {
        h.right = a32;
        emit(n_hits - 1, h);
      }
      h.start = pos;
      h.end = pos + len;
      h.left = a32;
      pending = true;
      n_hits++;
      anchor = 0;
      pos += len;
    }
  }
  if (pending) {
    h.right = anchor > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)anchor;
    emit(n_hits - 1, h);
  }
  if (end_pos) *end_pos = pos;
  return n_hits;
}
struct NoEmit {
  QUANT_HD void operator()(uint32_t, const Hit&) const {}
};
QUANT_HD uint32_t count_hits(const uint32_t* words, uint32_t n, uint64_t* end_pos = nullptr) { return walk(words, n, 0, NoEmit(), end_pos); }

// The key of a row: rows ascend by (hi, lo), which is ref, start, end, forward before reverse.  start and end are below
// 2^32 (thm_quant_create refuses longer contigs).
QUANT_HD uint64_t key_hi(uint32_t ref, uint64_t start) { return (uint64_t)ref << 32 | (uint32_t)start; }
QUANT_HD uint64_t key_lo(uint64_t end, bool forward) { return (uint64_t)(uint32_t)end << 1 | (forward ? 0u : 1u); }
constexpr int KEY_LO_BITS = 33;
QUANT_HD int key_hi_bits(uint32_t n_sq) {
  int b = 0;
  while (b < 32 && (n_sq >> b)) b++;
  return 32 + (b ? b : 1);
}

QUANT_HD thm_quant_junction row(uint64_t hi, uint64_t lo, uint64_t n_unique, uint64_t n_multi, uint32_t max_overhang) {
  thm_quant_junction j;
  j.ref_id = (uint32_t)(hi >> 32);
  j.strand = (lo & 1u) ? 0u : 1u;
  j.start = (uint32_t)hi;
  j.end = lo >> 1;
  j.n_unique = n_unique;
  j.n_multi = n_multi;
  j.max_overhang = max_overhang;
  j.pad_ = 0;
  return j;
}

// The read that holds alignment a: the last r in [0, n_reads) with off[r] <= a (reads without alignments are skipped:
// a later read with the same offset is the one whose range holds a).  Every alignment looks its read up on its own, so
// a read with thousands of alignments is thousands of independent searches.
QUANT_HD uint64_t read_of(const uint64_t* off, uint64_t n_reads, uint64_t a) {
  uint64_t lo = 0, hi = n_reads;
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) >> 1;
    if (off[mid] <= a)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

}  // namespace quant
}  // namespace thm
#endif
