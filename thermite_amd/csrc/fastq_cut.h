// fastq_cut.h -- where the host cuts FASTQ input into batches: the pure rules of the whole-file driver (io_driver.cpp)
// and of the upload entry points (fastq.hip, inflate.hip, gzip.hip).  No HIP runtime, no I/O: tests/cpp/driver_cut_main.cpp
// checks every function against a naive restatement.
#ifndef THERMITE_FASTQ_CUT_H
#define THERMITE_FASTQ_CUT_H
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace thm {

// where the batch of a block that is not the last ends: behind its first 4 * (newlines / 4) lines; *n_lines: those
inline uint64_t fastq_host_cut(const uint8_t* blk, uint64_t n, uint64_t* n_lines) {
  uint64_t nl = 0;
  for (const uint8_t* q = blk; (q = (const uint8_t*)memchr(q, '\n', (size_t)(blk + n - q))) != nullptr; q++) nl++;
  const uint64_t want = 4 * (nl / 4);
  *n_lines = want;
  if (want == 0) return 0;
  uint64_t seen = 0;
  const uint8_t* q = blk;
  while ((q = (const uint8_t*)memchr(q, '\n', (size_t)(blk + n - q))) != nullptr) {
    q++;
    if (++seen == want) break;
  }
  return (uint64_t)(q - blk);
}

// A block of a mapped plain file from `pos` on: the position behind the want_lines-th newline from there (the end of
// the file where it has fewer), found a span at a time; *n_lines: the block's lines, a last line without a newline
// counted.
inline size_t mapped_cut(const char* map, size_t map_len, size_t pos, uint64_t want_lines, uint64_t* n_lines, size_t span_bytes = (size_t)1 << 20) {
  uint64_t have = 0;
  size_t p = pos;
  while (p < map_len && have < want_lines) {
    const size_t span = std::min(map_len - p, span_bytes);
    uint64_t nl = 0;
    for (size_t i = 0; i < span; i++) nl += map[p + i] == '\n';
    if (have + nl < want_lines) {
      have += nl;
      p += span;
      continue;
    }
    const char* q = map + p;
    while (have < want_lines) {
      q = (const char*)memchr(q, '\n', (size_t)(map + p + span - q)) + 1;
      have++;
    }
    p = (size_t)(q - map);
  }
  if (p == map_len && p > pos && map[p - 1] != '\n') have++;
  *n_lines = have;
  return p;
}

// A group of whole BGZF members from member k on (k < n_members), by inflated size: members are taken until their sizes
// reach want_bytes, one at the least; the index behind the group.  tab[i].isize is member i's inflated size.
template <class Tab>
size_t member_group_end(const Tab& tab, size_t n_members, size_t k, double want_bytes) {
  double have = 0;
  do have += (double)tab[k++].isize;
  while (k < n_members && have < want_bytes);
  return k;
}

}  // namespace thm
#endif
