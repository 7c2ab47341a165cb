// The tagging of single-suffix k-mer table entries (thermite_amd/csrc/lut_direct.h) on the host: the decision whether a
// table may be tagged, the encode / decode round trip at the extreme positions, and that no plain entry of a taggable
// table reads as tagged.  Prints "ok <checks>" and returns 0, or the failed check and 1.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Ithermite_amd/csrc tests/cpp/lut_direct_main.cpp -o lut_direct_asan
#include <cstdio>
#include <cstdint>
#include <vector>

#include "lut_direct.h"

namespace {

int n_checks = 0, n_failed = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    n_checks++;                                                  \
    if (!(cond)) {                                               \
      n_failed++;                                                \
      fprintf(stderr, "line %d: %s\n", __LINE__, #cond);         \
    }                                                            \
  } while (0)

using namespace thm::lutd;

// the device pass and the probe's decode over one entry, as lut_tag_kernel and ms_search do them
template <class C>
struct Entry {
  C lo, hi;
};
template <class C>
void tag(Entry<C>& e, const std::vector<C>& sa) {
  if (single_suffix(e.lo, e.hi) && (uint64_t)e.lo < sa.size()) e.hi = encode(sa[e.lo]);
}

template <class C>
void round_trips(uint64_t n_max) {
  // every stored position is < n <= n_max, n_max = the largest n that can be tagged
  const C last = (C)(n_max - 1);
  for (C pos : {(C)0, (C)1, (C)2, (C)(last / 2), (C)(last - 1), last}) {
    const C stored = encode(pos);
    CHECK(is_tagged(stored));
    CHECK(position(stored) == pos);
    for (C lo : {(C)0, (C)1, (C)(last - 1), last}) {  // lo + 1 <= n_max
      C hi = stored, got = (C)~(C)0;
      CHECK(decode(true, lo, hi, &got));
      CHECK(got == pos && hi == (C)(lo + 1));
      hi = stored;
      got = (C)~(C)0;
      CHECK(!decode(false, lo, hi, &got));  // a plain table is never decoded, whatever its bits
      CHECK(hi == stored && got == (C)~(C)0);
    }
  }
}

template <class C>
void plain_entries_stay_plain(uint64_t n) {
  CHECK(can_tag<C>(n));
  // hi of a genuine entry is at most n: the extremes, with widths 0, 2 and n
  for (uint64_t hi64 : {(uint64_t)0, (uint64_t)2, n - 1, n}) {
    for (uint64_t w : {(uint64_t)0, (uint64_t)2, n}) {
      if (w > hi64) continue;
      C lo = (C)(hi64 - w), hi = (C)hi64, pos = (C)~(C)0;
      CHECK(!is_tagged(hi));
      CHECK(!single_suffix(lo, hi));
      CHECK(!decode(true, lo, hi, &pos));
      CHECK(hi == (C)hi64 && pos == (C)~(C)0);
    }
  }
  // hi == n, one suffix: the last rank.  The plain entry does not read as tagged; the pass rewrites it
  C lo = (C)(n - 1), hi = (C)n, pos = 0;
  CHECK(!is_tagged(hi) && single_suffix(lo, hi));
  CHECK(!decode(true, lo, hi, &pos));
}

}  // namespace

int main() {
  // ---- the decision, 32-bit coordinates
  CHECK(tag_bit<uint32_t>() == 0x80000000u);
  CHECK(can_tag<uint32_t>(0));
  CHECK(can_tag<uint32_t>((1ull << 31) - 1));
  CHECK(!can_tag<uint32_t>(1ull << 31));
  CHECK(!can_tag<uint32_t>((1ull << 32) - 1));
  // ---- 64-bit coordinates: every text that exists
  CHECK(tag_bit<uint64_t>() == 0x8000000000000000ull);
  CHECK(can_tag<uint64_t>(0));
  CHECK(can_tag<uint64_t>((1ull << 31) - 1));
  CHECK(can_tag<uint64_t>(1ull << 31));
  CHECK(can_tag<uint64_t>((1ull << 32) - 1));
  CHECK(can_tag<uint64_t>(1ull << 32));
  CHECK(can_tag<uint64_t>(1ull << 48));
  CHECK(can_tag<uint64_t>((1ull << 63) - 1));
  CHECK(!can_tag<uint64_t>(1ull << 63));

  round_trips<uint32_t>((1ull << 31) - 1);
  round_trips<uint64_t>((1ull << 63) - 1);
  round_trips<uint64_t>(1ull << 32);

  plain_entries_stay_plain<uint32_t>((1ull << 31) - 1);
  plain_entries_stay_plain<uint32_t>(1000);
  plain_entries_stay_plain<uint64_t>((1ull << 31));
  plain_entries_stay_plain<uint64_t>((1ull << 32) - 1);
  plain_entries_stay_plain<uint64_t>((1ull << 63) - 1);

  // ---- a small table through the pass and the decode: text of 12 suffixes, sa = a permutation
  {
    const std::vector<uint32_t> sa = {11, 3, 7, 0, 4, 8, 1, 5, 9, 2, 6, 10};
    std::vector<Entry<uint32_t>> lut = {{0, 1}, {1, 4}, {0, 0}, {4, 5}, {5, 12}, {0, 0}, {11, 12}, {12, 12}};
    const std::vector<Entry<uint32_t>> plain = lut;
    int tagged = 0;
    for (auto& e : lut) tag(e, sa);
    for (size_t i = 0; i < lut.size(); i++) {
      uint32_t hi = lut[i].hi, pos = ~0u;
      const bool t = decode(true, lut[i].lo, hi, &pos);
      CHECK(lut[i].lo == plain[i].lo && hi == plain[i].hi);  // the decoded interval is the plain one
      CHECK(t == (plain[i].hi - plain[i].lo == 1));
      if (t) {
        tagged++;
        CHECK(pos == sa[plain[i].lo]);
      } else {
        CHECK(lut[i].hi == plain[i].hi && pos == ~0u);
      }
    }
    CHECK(tagged == 3);
  }
  if (n_failed) {
    fprintf(stderr, "%d of %d checks failed\n", n_failed, n_checks);
    return 1;
  }
  printf("ok %d\n", n_checks);
  return 0;
}
