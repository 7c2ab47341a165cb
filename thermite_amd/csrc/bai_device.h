// bai_device.h -- what the kernels of the BAI index (kernels_bai.hip) spread over threads, each a plain function of the
// item it works on: a record's fields from its bytes, its bin, the virtual offset of a stream offset, the tests that cut
// the sorted stream into chunks, the windows of the linear index a record covers, and where everything stands in the
// finished file.  They compile for the host too: tests/cpp/bai_model_main.cpp drives the same functions serially, plain
// loops standing in for the scans and sorts, which is how the index is checked without a device.  The contract is in
// include/thermite_io.h above thm_bam_sorter_index; DESIGN.md section 4.16 has the passes.
//
// Everything before the emitter works on raw offsets of the sorted stream (bam_sort_device.h: off[]); only the emitter
// turns them into virtual offsets, with coff[m] the file offset of BGZF member m (coff[n_members]: the trailer).
#ifndef THERMITE_BAI_DEVICE_H
#define THERMITE_BAI_DEVICE_H
#include <cstdint>

#include "bam_sort_device.h"

#define BAI_HD BSORT_M inline

namespace thm {
namespace bai {

constexpr uint64_t CUT = 0xff00;           // raw bytes a BGZF member of the sorted stream holds (bgz::BLOCK_IN)
constexpr uint32_t PSEUDO_BIN = 37450;     // the bin that carries a reference's span and counts
constexpr uint32_t LINEAR_SHIFT = 14;      // 16 kb windows of the linear index
constexpr uint64_t MAX_END = 1ull << 29;   // BAI addresses [0, 2^29)
constexpr uint64_t NONE = ~0ull;           // an empty entry of the linear table; no record of the error kinds
constexpr uint32_t MAPPED_BIT = 1u << 31;  // of the packed `beg` word (beg itself is below 2^31)

// UCSC binning scheme, SAM specification section 5.3 (the one copy: io_writer.cpp and kernels_bam.hip call it too)
BAI_HD uint32_t reg2bin(int64_t beg, int64_t end) {
  --end;
  if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
  if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
  if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
  if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
  if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
  return 0;
}

BAI_HD uint32_t load_le16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }

// What the index takes from one record (`rec` at any alignment, `len` bytes with its block_size word): the record's own
// bin field is not read.  end is beg + the reference bases its CIGAR consumes (M, D, N, =, X), beg + 1 when that is none.
struct Fields {
  int32_t ref_id;
  uint32_t beg;   // max(pos, 0)
  uint64_t end;   // may exceed MAX_END: the caller refuses the record then
  bool mapped;    // !(flag & 4)
  bool ok;        // false: the CIGAR does not lie inside the record
};
BAI_HD Fields fields(const uint8_t* rec, uint64_t len) {
  Fields f;
  f.ref_id = (int32_t)bsort::load_le32(rec + 4);
  const int32_t pos = (int32_t)bsort::load_le32(rec + 8);
  f.beg = pos > 0 ? (uint32_t)pos : 0u;
  const uint32_t l_name = rec[12], n_ops = load_le16(rec + 16);
  f.mapped = !(load_le16(rec + 18) & 4u);
  const uint64_t cigar = 36u + l_name;
  f.ok = cigar + 4ull * n_ops <= len;
  uint64_t span = 0;
  if (f.ok && f.ref_id >= 0)
    for (uint32_t k = 0; k < n_ops; k++) {
      const uint32_t w = bsort::load_le32(rec + cigar + 4ull * k);
      if (0x18Du >> (w & 15u) & 1u) span += w >> 4;  // ops 0, 2, 3, 7, 8
    }
  f.end = (uint64_t)f.beg + (span ? span : 1);
  return f;
}

// The key the chunks are sorted by.  Records without a reference get rank n_sq and take no part.
BAI_HD uint64_t key(int32_t ref_id, uint32_t bin, uint32_t n_sq) { return ref_id >= 0 ? (uint64_t)(uint32_t)ref_id << 16 | bin : (uint64_t)n_sq << 16; }
BAI_HD uint32_t key_ref(uint64_t k) { return (uint32_t)(k >> 16); }
BAI_HD uint32_t key_bin(uint64_t k) { return (uint32_t)(k & 0xffffu); }
BAI_HD uint32_t key_bits(uint32_t n_sq) { return 16 + bsort::bit_width(n_sq); }

// v(s): the virtual offset of byte s of the sorted stream.  s == total with total a multiple of CUT gives the trailer
// member, offset 0.
BAI_HD uint64_t voff(const uint64_t* coff, uint64_t s) { return coff[s / CUT] << 16 | s % CUT; }

// Record i (key k, the one before it kp; i == 0 has none) begins a run of one (refID, bin): a chunk before merging.
BAI_HD bool run_head(bool has_prev, uint64_t kp, uint64_t k, uint32_t n_sq) { return key_ref(k) < n_sq && (!has_prev || k != kp); }
// ... and ends the run of the record before it (i == n: there is no record i, and the last run ends)
BAI_HD bool run_end(bool has_prev, uint64_t kp, bool has_cur, uint64_t k, uint32_t n_sq) {
  return has_prev && key_ref(kp) < n_sq && (!has_cur || k != kp);
}

// The merge test of the contract, pred.end >> 16 >= chunk.beg >> 16, on raw offsets: coff[] rises strictly (no member is
// empty), so coff[a] >= coff[b] exactly when a >= b.
BAI_HD bool merges(uint64_t pred_end, uint64_t beg) { return pred_end / CUT >= beg / CUT; }

// the windows [first, last] of the linear index a record overlaps
BAI_HD uint32_t first_window(uint32_t beg) { return beg >> LINEAR_SHIFT; }
BAI_HD uint32_t last_window(uint64_t end) { return (uint32_t)((end - 1) >> LINEAR_SHIFT); }
// A mapped record enters its first window unless the record before it, mapped and of the same reference, begins in the
// same window (that one, or one before it, has entered it with a smaller offset).
BAI_HD bool enters_first_window(bool prev_same_ref_mapped, uint32_t prev_beg, uint32_t beg) {
  return !prev_same_ref_mapped || first_window(prev_beg) != first_window(beg);
}
// the backward fill: an empty window takes the nearest set one above; set ones rise with the window, so this is a minimum
BAI_HD uint64_t fill(uint64_t own, uint64_t above) { return own < above ? own : above; }

// ---- the file: magic, n_ref, per reference { n_bin, bins { bin, n_chunk, chunks }, [pseudo-bin], n_intv, ioffset[] },
// n_no_coor.  Every field stands on a multiple of 4.
constexpr uint64_t HEAD_BYTES = 8, TAIL_BYTES = 8, PSEUDO_BYTES = 8 + 2 * 16;
// bytes of a reference with n_bins real bins holding n_chunks chunks, n_intv windows, with records or not
BAI_HD uint64_t ref_bytes(uint64_t n_bins, uint64_t n_chunks, bool has_records, uint64_t n_intv) {
  return 4 + 8 * n_bins + 16 * n_chunks + (has_records ? PSEUDO_BYTES : 0) + 4 + 8 * n_intv;
}
// where, in a reference that begins at ref_at, the bin stands that has bins_before bins and chunks_before chunks before it
BAI_HD uint64_t bin_at(uint64_t ref_at, uint64_t bins_before, uint64_t chunks_before) { return ref_at + 4 + 8 * bins_before + 16 * chunks_before; }
BAI_HD uint64_t chunk_at(uint64_t bin_at_, uint64_t k) { return bin_at_ + 8 + 16 * k; }
// n_intv of a reference: behind all its bins and the pseudo-bin
BAI_HD uint64_t linear_at(uint64_t ref_at, uint64_t n_bins, uint64_t n_chunks, bool has_records) {
  return bin_at(ref_at, n_bins, n_chunks) + (has_records ? PSEUDO_BYTES : 0);
}
BAI_HD uint64_t file_bytes(uint64_t all_ref_bytes) { return HEAD_BYTES + all_ref_bytes + TAIL_BYTES; }

// little-endian fields at a multiple of 4: dword stores, an 8-byte field as two
BAI_HD void put32(uint8_t* out, uint64_t at, uint32_t v) { *(uint32_t*)(out + at) = v; }
BAI_HD void put64(uint8_t* out, uint64_t at, uint64_t v) {
  put32(out, at, (uint32_t)v);
  put32(out, at + 4, (uint32_t)(v >> 32));
}

}  // namespace bai
}  // namespace thm
#endif
