// bam_sort_internal.h -- the state of a thm_bam_sorter, shared by bam_sort.hip (add, finish, the windows) and bai.hip
// (the index over what finish left on the device).
#ifndef THERMITE_BAM_SORT_INTERNAL_H
#define THERMITE_BAM_SORT_INTERNAL_H
#include <hip/hip_runtime.h>

#include <deque>
#include <vector>

#include "aligner_internal.h"

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

struct thm_bam_sorter {
  thm_aligner* a = nullptr;
  uint64_t max_bytes = 0;
  uint32_t n_sq = 0;
  // the arena: one segment per add, a record's place a global offset (seg_start[s] + its offset in segment s)
  std::deque<thm::SortSegment> segs;
  std::vector<uint64_t> seg_start;
  // per record, in add order: key (u64), length (u32), place (u64); grown by doubling
  DBuf key, len, loc;
  uint64_t rec_cap = 0, n_rec = 0, n_bytes = 0;
  bool finished = false;
  bool by_records = true;  // THM_SORT_GATHER=pieces: the output-centric gather instead (DESIGN.md section 4.15 has both times)
  // after finish: offsets of the sorted records in the sorted stream, their places, the segment table
  DBuf s_off, s_loc, d_seg_start, d_seg_ptr;
  uint64_t cursor = 0;
  DBuf stage;  // the window the gather writes and the deflater reads
  HBuf h_data[2], h_off[2], h_stat;
  int cur = 0;
  DBuf dbg_in, dbg_off;  // thm_debug_bam_sorter_add_records
  Event ev[4];           // add or sort: [0], [1]; gather: [2], [3]
  // for thm_bam_sorter_index (bai.hip): the compressed size of every member handed out, in stream order; whether a
  // window left raw (then there are none); whether the exhausted view has been returned
  std::vector<uint64_t> member_bytes;
  bool raw_taken = false, exhausted = false;
  HBuf h_bai;        // the finished index of the last call
  Event ev_bai[2];
};

#endif
