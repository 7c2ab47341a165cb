// bam_sort_internal.h -- the state of a thm_bam_sorter, shared by bam_sort.hip (add, finish, the windows) and bai.hip
// (the index over what finish left on the device).
#ifndef THERMITE_BAM_SORT_INTERNAL_H
#define THERMITE_BAM_SORT_INTERNAL_H
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <deque>
#include <vector>

#include "aligner_internal.h"
#include "launch_io.h"

namespace thm {

// one allocation of the arena, exactly as large as asked for (a DBuf rounds up by a quarter)
struct SortSegment {
  void* p = nullptr;
  SortSegment() = default;
  SortSegment(const SortSegment&) = delete;
  SortSegment& operator=(const SortSegment&) = delete;
  ~SortSegment() {
    if (p) (void)hipFree(p);
  }
};

}  // namespace thm

// Stable radix sort of n (u64 key, u32 ordinal) pairs by the low `bits` bits of the key, on `st`: vals becomes 0 .. n - 1,
// then hipcub's DoubleBuffer sort runs, least significant digit first and every pass stable, so equal keys keep their
// ordinals' order.  The result stands in *keys_out / *vals_out, each one of the two arrays handed in; `tmp` is hipcub's
// scratch, sized by its own query.  `started`, where given, is recorded once the scratch is there, in front of the kernels.
inline int sort_pairs_u64_u32(thm_aligner* a, DBuf& tmp, uint64_t* keys, uint64_t* keys_alt, uint32_t* vals, uint32_t* vals_alt, uint64_t n,
                              int bits, hipStream_t st, uint64_t** keys_out, uint32_t** vals_out, hipEvent_t started = nullptr) {
  hipcub::DoubleBuffer<uint64_t> dk(keys, keys_alt);
  hipcub::DoubleBuffer<uint32_t> dv(vals, vals_alt);
  size_t tmp_bytes = 0;
  HIPCHK(a, hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, dk, dv, n, 0, bits, st));
  HIPCHK(a, tmp.ensure(tmp_bytes + 16));
  if (started) HIPCHK(a, hipEventRecord(started, st));
  HIPCHK(a, thm::launch_bam_sort_iota(vals, n, st));
  HIPCHK(a, hipcub::DeviceRadixSort::SortPairs(tmp.p, tmp_bytes, dk, dv, n, 0, bits, st));
  *keys_out = dk.Current();
  *vals_out = dv.Current();
  return THM_OK;
}

// the pinned results of a window (thm_bam_sorter_next), two sets used alternately
struct SortHost {
  HArr<uint8_t> data;
  HArr<uint64_t> off;
};

struct thm_bam_sorter {
  thm_aligner* a = nullptr;
  uint64_t max_bytes = 0;
  uint32_t n_sq = 0;
  // the arena: one segment per add, a record's place a global offset (seg_start[s] + its offset in segment s)
  std::deque<thm::SortSegment> segs;
  std::vector<uint64_t> seg_start;
  // per record, in add order: key, length, place; grown by doubling
  DArr<uint64_t> key, loc;
  DArr<uint32_t> len;
  uint64_t rec_cap = 0, n_rec = 0, n_bytes = 0;
  bool finished = false;
  bool by_records = true;  // THM_SORT_GATHER=pieces: the output-centric gather instead (DESIGN.md section 4.15 has both times)
  // after finish: offsets of the sorted records in the sorted stream, their places, the segment table
  DArr<uint64_t> s_off, s_loc, d_seg_start;
  DArr<const uint8_t*> d_seg_ptr;
  uint64_t cursor = 0;
  DArr<uint8_t> stage;  // the window the gather writes and the deflater reads
  Alternating<SortHost> host;
  HArr<int32_t> h_stat;
  DArr<uint8_t> dbg_in;  // thm_debug_bam_sorter_add_records
  DArr<uint64_t> dbg_off;
  Event ev[4];           // add or sort: [0], [1]; gather: [2], [3]
  // for thm_bam_sorter_index (bai.hip): the compressed size of every member handed out, in stream order; whether a
  // window left raw (then there are none); whether the exhausted view has been returned
  std::vector<uint64_t> member_bytes;
  bool raw_taken = false, exhausted = false;
  HArr<uint8_t> h_bai;  // the finished index of the last call
  Event ev_bai[2];
};

#endif
