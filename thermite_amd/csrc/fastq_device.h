// fastq_device.h -- the steps of the device FASTQ parser (kernels_fastq.hip), each a plain function of the item it works
// on (a step of a wave's walk, a line, a record), so that the kernels are nothing but these functions spread over
// threads.  They compile for the host too: tests/cpp/fastq_model_main.cpp runs the same steps serially, which is how
// the parse rules are checked without a device (that file gives the sanitizer build line).
//
// The contract is fastq_parse_block's (io_fastq.cpp), strict form only.  A block of n bytes is
// device-parsable iff
//   its line count (newlines, plus one when the last byte is none) is a multiple of 4,
//   line 4r, with all its trailing CRs stripped, is non-empty and begins with '@',
//   line 4r+2, likewise, is non-empty and begins with '+',
//   lines 4r+1 and 4r+3, likewise, have the same length (0 allowed),
// and then name = line 4r without its '@', bases = line 4r+1 as given, qualities = line 4r+3: lines are told apart by
// their index mod 4, never by their first byte.  Anything else is declined -- one flag word, nothing more -- and goes
// to the host parser, which accepts a little more (blank lines at the end of the input, an empty read without its
// quality line there) and words the error messages.
//
//   count    per chunk of CHUNK bytes: a wave walks it STEP bytes at a time, four bytes a lane; newline_bits() of every
//            lane's word, one ballot per byte position, step_count() of the four masks
//   starts   the same walk: the newline at byte j of lane l is number step_rank() of its step, and line_start[k + 1] =
//            its position + 1 for the k-th newline of the block; line_start[0] = 0, and behind a last line without a
//            newline stands n + 1: line l is [line_start[l], line_start[l + 1] - 1) whichever it is
//   records  per record: record_rule() over its four lines (line_extent() strips the CRs) -> name and sequence length,
//            or the flag; two scans turn the lengths into name_off and offsets
//   gather   per record: its three spans copied to their places, copy_bytes() over a group of lanes
#ifndef THERMITE_FASTQ_DEVICE_H
#define THERMITE_FASTQ_DEVICE_H
#include <cstdint>

#if defined(__HIPCC__)
#define FQ_M __host__ __device__
#else
#define FQ_M
#endif
#define FQ_HD FQ_M inline

namespace thm {
namespace fq {

constexpr uint32_t STEP = 256;        // bytes of a wave's step: 64 lanes x one 4-byte word
constexpr uint32_t CHUNK = 4096;      // bytes per newline count: one wave's walk
constexpr uint32_t GATHER_LANES = 32; // lanes that copy one record
static_assert(CHUNK % STEP == 0, "a chunk is a whole number of steps");

FQ_HD uint32_t popc64(uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popcll(v);
#else
  return (uint32_t)__builtin_popcountll(v);
#endif
}

// bit j: byte j of the little-endian word `w`, which stands at position `at`, is a newline inside [0, hi)
FQ_HD uint32_t newline_bits(uint32_t w, uint64_t at, uint64_t hi) {
  uint32_t b = 0;
  for (uint32_t j = 0; j < 4; j++)
    if (at + j < hi && ((w >> (8 * j)) & 0xffu) == (uint32_t)'\n') b |= 1u << j;
  return b;
}

// m[j]: the lanes whose byte j is a newline (the ballot of bit j of newline_bits)
FQ_HD uint32_t step_count(const uint64_t m[4]) { return popc64(m[0]) + popc64(m[1]) + popc64(m[2]) + popc64(m[3]); }

// how many newlines of the step stand before byte j of lane `lane` (positions run lane-major: 4 * lane + j)
FQ_HD uint32_t step_rank(const uint64_t m[4], uint32_t lane, uint32_t j) {
  const uint64_t below = (1ull << lane) - 1ull;
  uint32_t r = popc64(m[0] & below) + popc64(m[1] & below) + popc64(m[2] & below) + popc64(m[3] & below);
  for (uint32_t k = 0; k < j; k++) r += (uint32_t)((m[k] >> lane) & 1ull);
  return r;
}

// lines of a block with `n_newlines` newlines: a last line without one counts (n > 0)
FQ_HD uint64_t line_count(uint64_t n_newlines, uint8_t last_byte) { return n_newlines + (last_byte != (uint8_t)'\n'); }

// line l without its terminator and without its trailing CRs -- all of them, as the host parser strips: its first byte
// is raw[*at], the return value its length
FQ_HD uint64_t line_extent(const uint8_t* raw, const uint64_t* line_start, uint64_t l, uint64_t* at) {
  const uint64_t s = line_start[l];
  uint64_t e = line_start[l + 1] - 1;
  while (e > s && raw[e - 1] == (uint8_t)'\r') e--;
  *at = s;
  return e - s;
}

struct Record {
  uint64_t name_at, name_len;  // the header line without its '@'
  uint64_t seq_at, seq_len;
  uint64_t qual_at;            // seq_len bytes as well
};

// record r = lines 4r .. 4r+3; false: the block is not device-parsable
FQ_HD bool record_rule(const uint8_t* raw, const uint64_t* line_start, uint64_t r, Record* o) {
  uint64_t at, len;
  len = line_extent(raw, line_start, 4 * r, &at);
  if (len == 0 || raw[at] != (uint8_t)'@') return false;
  o->name_at = at + 1;
  o->name_len = len - 1;
  o->seq_len = line_extent(raw, line_start, 4 * r + 1, &o->seq_at);
  len = line_extent(raw, line_start, 4 * r + 2, &at);
  if (len == 0 || raw[at] != (uint8_t)'+') return false;
  len = line_extent(raw, line_start, 4 * r + 3, &o->qual_at);
  return len == o->seq_len;
}

// lane `lane` of `n_lanes`: its share of dst[0, len) = src[0, len), neighbouring lanes on neighbouring bytes
FQ_HD void copy_bytes(uint8_t* dst, const uint8_t* src, uint64_t len, uint32_t lane, uint32_t n_lanes) {
  for (uint64_t i = lane; i < len; i += n_lanes) dst[i] = src[i];
}

}  // namespace fq
}  // namespace thm
#endif
