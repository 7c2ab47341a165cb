// The op-stream copy of the compact stage (thermite_amd/csrc/compact_copy.h) on the host: 16 simulated lanes run the
// functions of the header in the order the kernel's lanes do (AlnCopy, kernels_compact.hip: every load of a trip by every
// lane, then the stores of the trip; trip 0 first, the further trips of a stream longer than 256 bytes in a loop) over a
// memory that checks every access.  Every (source offset mod 4) x (destination offset mod 4) x length 0..300, 1000 and
// 4099: the destination equals memcpy's, no byte outside [dst, dst + len) is written and none inside twice, no source
// byte outside [src & ~3, (src + len + 3) & ~3) is read, dword accesses are aligned.  Prints the cases and the accesses it
// checked; the first violation is printed and ends the program with status 1.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "compact_copy.h"

using namespace thm;

namespace {

constexpr uint64_t GUARD = 64;  // guard bytes on both sides of either buffer (a multiple of 4)
uint64_t g_checks = 0;
uint64_t g_src = 0, g_dst = 0;
uint32_t g_len = 0;

void require(bool ok, const char* expr, int line) {
  g_checks++;
  if (ok) return;
  fprintf(stderr, "compact_copy_main.cpp:%d: %s\n  at src %" PRIu64 " dst %" PRIu64 " len %u\n", line, expr, g_src, g_dst, g_len);
  exit(1);
}
#define REQUIRE(e) require((e), #e, __LINE__)

// the two buffers behind the accessor of compact_copy.h; offsets are from 4-byte aligned bases
struct CheckedMem {
  const uint8_t* src_buf;
  uint8_t* dst_buf;
  uint8_t* written;  // per destination byte: times written
  uint64_t src, dst;
  uint32_t len;
  uint32_t ld32(uint64_t o) const {
    REQUIRE((o & 3) == 0);
    REQUIRE(o >= (src & ~3ull) && o + 4 <= ((src + len + 3) & ~3ull));
    uint32_t v;
    memcpy(&v, src_buf + o, 4);
    return v;
  }
  uint32_t ld8(uint64_t o) const {
    REQUIRE(o >= src && o < src + len);
    return src_buf[o];
  }
  void st32(uint64_t o, uint32_t v) {
    REQUIRE((o & 3) == 0);
    REQUIRE(o >= dst && o + 4 <= dst + len);
    memcpy(dst_buf + o, &v, 4);
    for (int k = 0; k < 4; k++) written[o + k]++;
  }
  void st8(uint64_t o, uint8_t v) {
    REQUIRE(o >= dst && o < dst + len);
    dst_buf[o] = v;
    written[o]++;
  }
};

uint64_t one_case(uint32_t src_mod, uint32_t dst_mod, uint32_t len, uint32_t seed) {
  const uint64_t size = GUARD + 4 + len + 4 + GUARD;
  // (uint32_t storage: 4-byte aligned bases)
  std::vector<uint32_t> src_store(size / 4 + 4), dst_store(size / 4 + 4);
  uint8_t* src_buf = reinterpret_cast<uint8_t*>(src_store.data());
  uint8_t* dst_buf = reinterpret_cast<uint8_t*>(dst_store.data());
  std::vector<uint8_t> before(size + 8), written(size + 8, 0), expect(size + 8);
  uint32_t x = seed * 2654435761u + 12345u;
  for (uint64_t i = 0; i < size + 8; i++) {
    x = x * 1664525u + 1013904223u;
    src_buf[i] = (uint8_t)(x >> 24);
    dst_buf[i] = before[i] = (uint8_t)(x >> 16) ^ 0x5Au;
  }
  const uint64_t src = GUARD + src_mod, dst = GUARD + dst_mod;
  g_src = src, g_dst = dst, g_len = len;
  expect = before;
  if (len) memcpy(expect.data() + dst, src_buf + src, len);

  // the pure functions against their definitions
  const uint32_t head = ccopy::head_bytes(dst, len), nd = ccopy::body_dwords(dst, len), tail = ccopy::tail_bytes(dst, len);
  REQUIRE(head + 4 * nd + tail == len && head < 4 && tail < 4);
  REQUIRE(nd == 0 || ((dst + head) & 3) == 0);
  REQUIRE(head == len || ((dst + head) & 3) == 0);
  REQUIRE(nd > 0 || len < 7);
  const uint32_t n_trips = ccopy::trips(dst, len);
  REQUIRE((len == 0) == (n_trips == 0));
  REQUIRE(n_trips * ccopy::TRIP_DWORDS >= nd && (n_trips <= 1 || (n_trips - 1) * ccopy::TRIP_DWORDS < nd));
  {  // every dword of the stream belongs to one lane and trip, every head and tail byte to one lane
    std::vector<uint8_t> owner(nd + 1, 0), edge(len + 1, 0);
    for (uint32_t trip = 0; trip < n_trips; trip++)
      for (int lane = 0; lane < ccopy::LANES; lane++)
        for (int m = 0; m < ccopy::DWORDS_PER_LANE; m++) {
          const uint32_t j = ccopy::lane_dword(lane, m, trip);
          if (j < nd) owner[j]++;
        }
    for (uint32_t j = 0; j < nd; j++) REQUIRE(owner[j] == 1);
    for (int lane = 0; lane < ccopy::LANES; lane++) {
      const uint32_t e = ccopy::edge_byte(lane, dst, len);
      if (e != ccopy::NO_BYTE) {
        REQUIRE(e < len && (e < head || e >= head + 4 * nd));
        edge[e]++;
      }
    }
    for (uint32_t e = 0; e < len; e++) REQUIRE(edge[e] == ((e < head || e >= head + 4 * nd) ? 1 : 0));
  }

  // the copy, as the lanes of a group run it
  CheckedMem mem{src_buf, dst_buf, written.data(), src, dst, len};
  ccopy::LaneRegs regs[ccopy::LANES];
  if (len == 0) {  // the kernel runs trip 0 of an empty stream too (an alignment without a transcript stream)
    for (int lane = 0; lane < ccopy::LANES; lane++) ccopy::lane_load(mem, src, dst, len, 0, lane, regs[lane]);
    for (int lane = 0; lane < ccopy::LANES; lane++) ccopy::lane_store(mem, src, dst, len, 0, lane, regs[lane]);
  }
  for (uint32_t trip = 0; trip < n_trips; trip++) {
    for (int lane = 0; lane < ccopy::LANES; lane++) ccopy::lane_load(mem, src, dst, len, trip, lane, regs[lane]);
    for (int lane = 0; lane < ccopy::LANES; lane++) ccopy::lane_store(mem, src, dst, len, trip, lane, regs[lane]);
  }
  REQUIRE(memcmp(dst_buf, expect.data(), size + 8) == 0);
  for (uint64_t i = 0; i < size + 8; i++) REQUIRE(written[i] == ((i >= dst && i < dst + len) ? 1 : 0));
  return 1;
}

}  // namespace

int main() {
  // funnel against bytes
  for (uint32_t shift = 0; shift < 4; shift++) {
    const uint8_t b[8] = {0x10, 0x32, 0x54, 0x76, 0x98, 0xBA, 0xDC, 0xFE};
    uint32_t lo, hi, want;
    memcpy(&lo, b, 4);
    memcpy(&hi, b + 4, 4);
    memcpy(&want, b + shift, 4);
    g_len = shift;
    REQUIRE(ccopy::funnel(lo, hi, shift) == want);
    REQUIRE(shift != 0 || ccopy::funnel(lo, 0xDEADBEEFu, 0) == lo);
  }
  uint64_t cases = 0;
  uint32_t seed = 1;
  for (uint32_t s = 0; s < 4; s++)
    for (uint32_t d = 0; d < 4; d++) {
      for (uint32_t len = 0; len <= 300; len++) cases += one_case(s, d, len, seed++);
      cases += one_case(s, d, 1000, seed++);
      cases += one_case(s, d, 4099, seed++);
    }
  printf("cases %" PRIu64 " checks %" PRIu64 "\n", cases, g_checks);
  return 0;
}
