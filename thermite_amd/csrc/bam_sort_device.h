// bam_sort_device.h -- what the kernels of the coordinate sort (kernels_bam_sort.hip) spread over threads, each a plain
// function of the item it works on: the sort key of one BAM record, and the addressing of a window of the sorted byte
// stream -- which records overlap it, and which bytes of a record go where in it.  They compile for the host too:
// tests/cpp/bam_sort_model_main.cpp drives the same functions serially, which is how the order and the window cuts are
// checked without a device.
//
// The sorted stream is the records of a run back to back in key order; off[r] is where sorted
// record r begins in it (off[n] its length).  A window [w0, w1) of it is assembled from whole records that lie anywhere,
// at any alignment, in the arena; records that straddle w0 or w1 contribute the part inside, and a record may be longer
// than the window.  A lane of the gather kernel treats the 16 bytes it owns as a window of its own.
#ifndef THERMITE_BAM_SORT_DEVICE_H
#define THERMITE_BAM_SORT_DEVICE_H
#include <cstdint>

#if defined(__HIPCC__)
#define BSORT_M __host__ __device__
#else
#define BSORT_M
#endif
#define BSORT_HD BSORT_M inline

namespace thm {
namespace bsort {

constexpr uint32_t MIN_RECORD = 36;  // block_size and the fixed fields: no BAM record is shorter
constexpr uint32_t PIECE = 16;       // bytes of the window one lane of the gather writes

// number of bits x takes (bit_width(4) == 3)
BSORT_HD uint32_t bit_width(uint64_t x) {
  uint32_t b = 0;
  while (x) {
    b++;
    x >>= 1;
  }
  return b;
}

// the bits of the key that can be set: rank goes up to n_sq, the unmapped one
BSORT_HD uint32_t key_bits(uint32_t n_sq) { return 33 + bit_width(n_sq); }

// reference index (unmapped last), position, forward before reverse
BSORT_HD uint64_t key(int32_t ref_id, int32_t pos, uint32_t flag, uint32_t n_sq) {
  const uint64_t rank = ref_id >= 0 ? (uint64_t)(uint32_t)ref_id : (uint64_t)n_sq;
  return rank << 33 | (uint64_t)(uint32_t)(pos + 1) << 1 | (flag >> 4 & 1);
}

BSORT_HD uint32_t load_le32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// ... of the record that begins at `rec` (any alignment): refID, pos and flag at bytes 4, 8 and 18
BSORT_HD uint64_t record_key(const uint8_t* rec, uint32_t n_sq) {
  return key((int32_t)load_le32(rec + 4), (int32_t)load_le32(rec + 8), (uint32_t)rec[18] | (uint32_t)rec[19] << 8, n_sq);
}

// the sorted record that holds byte `at` of the stream, at < off[n]: the last r with off[r] <= at (no record is empty)
BSORT_HD uint64_t record_at(const uint64_t* off, uint64_t n, uint64_t at) {
  uint64_t lo = 0, hi = n;  // off[lo] <= at < off[hi]
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= at)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// the records [first, last) that overlap the window [w0, w1), w0 < w1 <= off[n]
BSORT_HD void window_records(const uint64_t* off, uint64_t n, uint64_t w0, uint64_t w1, uint64_t* first, uint64_t* last) {
  *first = record_at(off, n, w0);
  *last = record_at(off, n, w1 - 1) + 1;
}

// the part of a record, which takes [begin, end) of the stream, that lies in [w0, w1): n bytes from byte `src` of the
// record to byte `dst` of the window (n == 0: they do not overlap)
struct Part {
  uint64_t src, dst, n;
};
BSORT_HD Part clip(uint64_t begin, uint64_t end, uint64_t w0, uint64_t w1) {
  const uint64_t lo = begin > w0 ? begin : w0, hi = end < w1 ? end : w1;
  Part p;
  p.src = lo - begin;
  p.dst = lo - w0;
  p.n = hi > lo ? hi - lo : 0;
  return p;
}

// the arena segment that holds global offset `loc`: the last s with seg_start[s] <= loc (seg_start[0] == 0; a record never
// straddles two segments)
BSORT_HD uint32_t segment_of(const uint64_t* seg_start, uint32_t n_seg, uint64_t loc) {
  uint32_t lo = 0, hi = n_seg;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (seg_start[mid] <= loc)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

}  // namespace bsort
}  // namespace thm
#endif
