// compact_copy.h -- how the 16 lanes of a group move one op stream of the compact stage (kernels_compact.hip): aligned
// dwords on the destination's alignment, each from the two aligned source dwords that hold its bytes, and the up to
// three bytes before the first and behind the last destination dword as single bytes.  A stream's neighbours in ops[]
// belong to other alignments, which other groups write at the same time: nothing outside [dst, dst + len) is written,
// not even with its old value, and nothing outside the source's dwords [src & ~3, (src + len + 3) & ~3) is read.
// No HIP runtime: under hipcc the functions are __host__ __device__, and tests/cpp/compact_copy_main.cpp runs the same
// functions with 16 simulated lanes over a memory that checks every access.
//
// Memory goes through an accessor M with ld32 / ld8 (source) and st32 / st8 (destination), all taking byte offsets from
// two bases that are 4-byte aligned; src and dst below are such offsets.
#ifndef THERMITE_COMPACT_COPY_H
#define THERMITE_COMPACT_COPY_H
#include <cstdint>

#if defined(__HIPCC__)
#define CCOPY_HD __host__ __device__ inline
#else
#define CCOPY_HD inline
#endif

namespace thm {
namespace ccopy {

constexpr int LANES = 16;           // lanes of a group
constexpr int DWORDS_PER_LANE = 4;  // destination dwords a lane holds per trip
constexpr uint32_t TRIP_DWORDS = (uint32_t)(LANES * DWORDS_PER_LANE);  // 256 bytes per trip of the group
constexpr uint32_t NO_BYTE = 0xFFFFFFFFu;
constexpr int TAIL_LANE0 = 8;  // lanes 0..2 store the head bytes, lanes 8..10 the tail bytes

// bytes before the first aligned destination dword (all of a stream that ends before it)
CCOPY_HD uint32_t head_bytes(uint64_t dst, uint32_t len) {
  const uint32_t h = (uint32_t)(0 - dst) & 3u;
  return h < len ? h : len;
}
// whole destination dwords
CCOPY_HD uint32_t body_dwords(uint64_t dst, uint32_t len) { return (len - head_bytes(dst, len)) >> 2; }
// bytes behind the last whole destination dword
CCOPY_HD uint32_t tail_bytes(uint64_t dst, uint32_t len) { return (len - head_bytes(dst, len)) & 3u; }
// trips of the group over a stream: the first one also moves the head and tail bytes
CCOPY_HD uint32_t trips(uint64_t dst, uint32_t len) {
  const uint32_t nd = body_dwords(dst, len);
  return nd ? (nd + TRIP_DWORDS - 1) / TRIP_DWORDS : (len ? 1u : 0u);
}
// the m-th destination dword of a lane in a trip: consecutive lanes, consecutive dwords
CCOPY_HD uint32_t lane_dword(int lane, int m, uint32_t trip) { return trip * TRIP_DWORDS + (uint32_t)m * LANES + (uint32_t)lane; }
// the stream byte a lane moves as a single byte (in trip 0), or NO_BYTE
CCOPY_HD uint32_t edge_byte(int lane, uint64_t dst, uint32_t len) {
  const uint32_t head = head_bytes(dst, len), tail = tail_bytes(dst, len);
  if ((uint32_t)lane < head) return (uint32_t)lane;
  if (lane >= TAIL_LANE0 && (uint32_t)(lane - TAIL_LANE0) < tail) return len - tail + (uint32_t)(lane - TAIL_LANE0);
  return NO_BYTE;
}
// four bytes from byte `shift` (0..3) of the aligned dword lo on; hi is the dword behind it (not looked at for shift 0)
CCOPY_HD uint32_t funnel(uint32_t lo, uint32_t hi, uint32_t shift) { return shift ? (lo >> (8 * shift)) | (hi << (32 - 8 * shift)) : lo; }

// what a lane has loaded for one trip: the source dwords of its destination dwords, and its head or tail byte
struct LaneRegs {
  uint32_t lo[DWORDS_PER_LANE], hi[DWORDS_PER_LANE];
  uint32_t edge;
};

// every load of a lane for one trip; no store of the trip comes before them
template <class M>
CCOPY_HD void lane_load(const M& mem, uint64_t src, uint64_t dst, uint32_t len, uint32_t trip, int lane, LaneRegs& r) {
  const uint32_t head = head_bytes(dst, len), nd = body_dwords(dst, len);
#if defined(__HIPCC__)
  #pragma unroll
#endif
  for (int m = 0; m < DWORDS_PER_LANE; m++) {
    const uint32_t j = lane_dword(lane, m, trip);
    r.lo[m] = r.hi[m] = 0u;
    if (j < nd) {
      const uint64_t s = src + head + 4ull * j;
      r.lo[m] = mem.ld32(s & ~3ull);
      if (s & 3u) r.hi[m] = mem.ld32((s & ~3ull) + 4);
    }
  }
  r.edge = 0u;
  if (trip == 0) {
    const uint32_t e = edge_byte(lane, dst, len);
    if (e != NO_BYTE) r.edge = mem.ld8(src + e);
  }
}

// the stores of the same trip
template <class M>
CCOPY_HD void lane_store(M& mem, uint64_t src, uint64_t dst, uint32_t len, uint32_t trip, int lane, const LaneRegs& r) {
  const uint32_t head = head_bytes(dst, len), nd = body_dwords(dst, len);
  const uint32_t shift = (uint32_t)(src + head) & 3u;  // the same for every dword of the stream
#if defined(__HIPCC__)
  #pragma unroll
#endif
  for (int m = 0; m < DWORDS_PER_LANE; m++) {
    const uint32_t j = lane_dword(lane, m, trip);
    if (j < nd) mem.st32(dst + head + 4ull * j, funnel(r.lo[m], r.hi[m], shift));
  }
  if (trip == 0) {
    const uint32_t e = edge_byte(lane, dst, len);
    if (e != NO_BYTE) mem.st8(dst + e, (uint8_t)r.edge);
  }
}

}  // namespace ccopy
}  // namespace thm
#endif
