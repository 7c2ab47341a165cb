// pileup_device.h -- what the kernels of the per-base allele counts (kernels_pileup.hip) do per item, each a plain
// function of the item it works on: the kind of a byte, the shape of an alignment's genome CIGAR and the checks that keep
// every later store inside the arrays, the chunk of SEQ a lane compares with the text, the key of an event, and the row a
// position's depth and table rows assemble to.  They compile for the host too: tests/cpp/pileup_model_main.cpp drives the
// same functions serially, which is how the counts are checked without a device.  The contract is in
// include/thermite_io.h above thm_pileup_create; DESIGN.md section 4.19 has the passes.
//
// Layout.  The depth lives in one difference array in coverage_device.h's layout (entry base[c] + x for position x of
// contig c).  An event -- an observation that differs from the reference, a deleted base, an insertion -- is the 64-bit key
// (base[c] + x) << 3 | kind with kinds 0..4 = A C G T N, 5 = del, 6 = ins; the table is (key, count) ascending by key, so
// the rows of one position stand together, at most seven of them, and the rows of a contig and of a tile are ranges.
#ifndef THERMITE_PILEUP_DEVICE_H
#define THERMITE_PILEUP_DEVICE_H
#include <cstdint>

#include "coverage_device.h"

namespace thm {
namespace pile {

// An alignment is walked by a group of GROUP lanes; within an M word each lane compares CHUNK consecutive bases per step.
constexpr uint32_t CHUNK = 8, GROUP = 16;
constexpr uint32_t KIND_N = 4, KIND_DEL = 5, KIND_INS = 6, N_KINDS = 7;
constexpr uint64_t MAX_WINDOW = 1ull << 20;
// the totals of one batch, in the order of thm_pile_totals
enum { T_READS = 0, T_FAILED, T_ALNS, T_SKIPPED_MULTI, T_LONG_RUN, T_USED, T_BLOCKS, T_M_BASES, T_MISMATCHES, T_DEL_BASES, T_INS, T_INS_BASES, N_TOTALS };
static_assert(sizeof(thm_pile_totals) == N_TOTALS * 8, "the kernels index thm_pile_totals as an array");
static_assert(sizeof(thm_pile_site) == 48, "thm_pile_site is 48 bytes");

COV_HD uint32_t kind(uint8_t c) {
  c &= 0xDFu;  // (upper-cases the letters; no other byte becomes one of the four)
  return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : KIND_N;
}
COV_HD uint32_t complement(uint32_t k) { return k < 4 ? 3u - k : KIND_N; }

COV_HD uint64_t key_of(uint64_t entry, uint32_t k) { return entry << 3 | k; }
COV_HD uint64_t key_entry(uint64_t key) { return key >> 3; }
COV_HD uint32_t key_kind(uint64_t key) { return (uint32_t)(key & 7u); }
// the bits a key of a layout of `entries` entries can have set
COV_HD int key_bits(uint64_t entries) {
  int b = 0;
  while (b < 61 && (entries >> b)) b++;
  return b + 3;
}

// What the words of an alignment add up to: the position behind the last word, the query bases they consume (M + I + S),
// and the observations by class.
struct Shape {
  uint64_t end, qlen, m_bases, del_bases, ins, ins_bases;
  uint32_t n_blocks;
};
COV_HD Shape shape_of(const uint32_t* words, uint32_t n, uint64_t ystart) {
  Shape s{ystart, 0, 0, 0, 0, 0, 0};
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t w = words[i], code = w & 15u;
    const uint64_t len = w >> 4;
    if (code == quant::OP_M) {
      s.m_bases += len;
      s.qlen += len;
    } else if (code == quant::OP_D) {
      s.del_bases += len;
    } else if (code == quant::OP_I) {
      s.ins += 1;
      s.ins_bases += len;
      s.qlen += len;
    } else if (code == quant::OP_S) {
      s.qlen += len;
    }
  }
  uint64_t end = ystart;
  s.n_blocks = cov::walk_blocks(words, n, ystart, cov::NoBlock(), &end);
  s.end = end;
  if (end == ystart) s.m_bases = s.del_bases = s.ins = s.ins_bases = 0;  // no reference base consumed: nothing is observed
  return s;
}
// the position an I word is observed at, the walk standing at p
COV_HD uint64_t ins_pos(uint64_t p, uint64_t ystart) { return p > ystart ? p - 1 : ystart; }

// The device's checks of one alignment, before anything is touched: cov::locate_aln's, the walk from ystart ends inside
// the contig, and, for an alignment with words, they consume the read_len bytes of its read.  *sq gets the refID, *shape
// what the words add up to.
COV_HD bool check_aln(uint32_t ref_id, uint64_t ystart, uint64_t cigar_off, uint32_t n_cigar, bool long_run, const uint32_t* words, uint64_t n_words,
                      const int32_t* ref_sq, uint32_t n_refs, const uint64_t* base, uint32_t n_sq, uint64_t read_len, uint32_t* sq, Shape* shape) {
  *shape = Shape{ystart, 0, 0, 0, 0, 0, 0};
  const uint64_t len = cov::locate_aln(ref_id, ystart, cigar_off, n_cigar, n_words, ref_sq, n_refs, base, n_sq, sq);
  if (len == cov::NOT_LOCATED) return false;
  if (long_run || n_cigar == 0) return true;
  *shape = shape_of(words + cigar_off, n_cigar, ystart);
  return shape->end <= len && shape->qlen == read_len;
}

// n <= CHUNK bytes at p as a little-endian word: a whole chunk in one load, a part of one byte by byte, so that no load
// leaves [p, p + n)
COV_HD uint64_t load_chunk(const uint8_t* p, uint32_t n) {
  uint64_t w = 0;
  if (n == CHUNK) {
    __builtin_memcpy(&w, p, CHUNK);
  } else {
    for (uint32_t i = 0; i < n; i++) w |= (uint64_t)p[i] << (8 * i);
  }
  return w;
}
// The read bytes that SEQ[q, q + n) stands for, byte i of the word for SEQ[q + i]: read[q + i] of a forward alignment;
// of a reverse one read[len - 1 - q - i], the n bytes in front of len - q loaded together and turned round in registers
// (compare_chunk complements them).  0 < n <= CHUNK, q + n <= len.
COV_HD uint64_t seq_chunk(const uint8_t* read, uint64_t len, bool forward, uint64_t q, uint32_t n) {
  if (forward) return load_chunk(read + q, n);
  return __builtin_bswap64(load_chunk(read + (len - q - n), n)) >> (8 * (CHUNK - n));
}
// The kinds SEQ shows in a chunk (4 bits a base, base i at bit 4 i) and the mask of the bases i < n whose kind is not the
// text's.
COV_HD uint32_t compare_chunk(uint64_t seq, uint64_t text, uint32_t n, bool forward, uint32_t* kinds) {
  uint32_t mask = 0, ks = 0;
  for (uint32_t i = 0; i < CHUNK; i++) {
    uint32_t k = kind((uint8_t)(seq >> (8 * i)));
    if (!forward) k = complement(k);
    ks |= k << (4 * i);
    mask |= (i < n && k != kind((uint8_t)(text >> (8 * i)))) ? 1u << i : 0u;
  }
  *kinds = ks;
  return mask;
}
// The chunk of the M word (position p, query offset q, length len) that begins c0 bases into it, c0 < len: the mask of
// its mismatches, and their kinds.  text_c is the first text byte of the contig.
COV_HD uint32_t m_chunk(const uint8_t* text_c, const uint8_t* read, uint64_t read_len, bool forward, uint64_t p, uint64_t q, uint64_t len, uint64_t c0,
                        uint32_t* kinds) {
  const uint32_t n = len - c0 < CHUNK ? (uint32_t)(len - c0) : CHUNK;
  return compare_chunk(seq_chunk(read, read_len, forward, q + c0, n), load_chunk(text_c + p + c0, n), n, forward, kinds);
}

// first row of keys[lo, hi) that is not below `key`
COV_HD uint64_t lower_bound(const uint64_t* keys, uint64_t lo, uint64_t hi, uint64_t key) {
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < key)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}
// the events at the position of row j, summed over its rows in keys[j, hi): what min_alt is compared with
COV_HD uint64_t alt_of(const uint64_t* keys, const uint32_t* cnts, uint64_t j, uint64_t hi) {
  const uint64_t e = key_entry(keys[j]);
  uint64_t alt = 0;
  for (; j < hi && key_entry(keys[j]) == e; j++) alt += cnts[j];
  return alt;
}
// The row of layout entry e with depth `depth`, its table rows beginning at row j of keys[j, hi) (none: j == hi or
// another entry there).  The reference allele's count is the depth minus the deleted bases and the other kinds.
COV_HD thm_pile_site site_of(const uint64_t* keys, const uint32_t* cnts, uint64_t j, uint64_t hi, uint64_t e, uint32_t depth, const uint64_t* base,
                             uint32_t n_sq, const uint64_t* tstart, const uint8_t* text) {
  uint32_t c[N_KINDS] = {0, 0, 0, 0, 0, 0, 0};
  for (; j < hi && key_entry(keys[j]) == e; j++) {
    // (a static index in every statement: the counts stay in registers)
    const uint32_t k = key_kind(keys[j]);
    for (uint32_t i = 0; i < N_KINDS; i++) c[i] += i == k ? cnts[j] : 0u;
  }
  const uint32_t sq = cov::sq_of(base, n_sq, e);
  thm_pile_site s;
  s.ref_id = sq;
  s.pos = e - base[sq];
  s.ref_base = text[tstart[sq] + s.pos];
  s.pad_[0] = s.pad_[1] = s.pad_[2] = 0;
  s.depth = depth;
  const uint32_t rk = kind(s.ref_base), others = c[0] + c[1] + c[2] + c[3] + c[4];
  for (uint32_t i = 0; i < 5; i++) s.cnt[i] = i == rk ? depth - c[KIND_DEL] - others : c[i];
  s.del = c[KIND_DEL];
  s.ins = c[KIND_INS];
  return s;
}

}  // namespace pile
}  // namespace thm
#endif
