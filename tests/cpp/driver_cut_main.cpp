// driver_cut_main.cpp -- thermite_amd/csrc/fastq_cut.h against naive restatements (tests/test_driver_cut_host.py): the
// cut of a block that is not the last, the cut of a mapped plain file and the grouping of BGZF members, exhaustively over
// every string over {'a', '\n'} of length 0 to 12 and every vector of up to 6 member sizes from {0, 1, 5}.  Every string
// stands in a heap block of exactly its length, so that a read behind it is the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "fastq_cut.h"

namespace {

unsigned long long n_cases = 0;

#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      fprintf(stderr, "%s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);               \
      fprintf(stderr, "\n");                      \
      exit(1);                                    \
    }                                             \
  } while (0)

// the position behind the `want`-th newline of s[pos, n), or n where there are fewer; *seen: newlines passed
size_t behind_newline(const char* s, size_t n, size_t pos, unsigned long long want, unsigned long long* seen) {
  *seen = 0;
  size_t p = pos;
  while (p < n && *seen < want) *seen += s[p++] == '\n';
  return p;
}

void check_host_cut(const char* s, size_t n) {
  unsigned long long nl = 0, seen = 0;
  for (size_t i = 0; i < n; i++) nl += s[i] == '\n';
  const unsigned long long want = 4 * (nl / 4);
  const size_t cut = want ? behind_newline(s, n, 0, want, &seen) : 0;
  uint64_t lines = ~0ull;
  const uint64_t got = thm::fastq_host_cut((const uint8_t*)s, n, &lines);
  CHECK(got == cut && lines == want, "fastq_host_cut: length %zu, cut %llu for %zu, lines %llu for %llu", n, (unsigned long long)got, cut,
        (unsigned long long)lines, want);
  n_cases++;
}

void check_mapped_cut(const char* s, size_t n) {
  static const size_t spans[] = {1, 3, 8, (size_t)1 << 20};
  for (size_t pos = 0; pos <= n; pos++)
    for (unsigned long long want = 1; want <= 8; want++) {
      unsigned long long lines = 0;
      const size_t end = behind_newline(s, n, pos, want, &lines);
      if (end == n && end > pos && s[end - 1] != '\n') lines++;
      for (size_t span : spans) {
        uint64_t got_lines = ~0ull;
        const size_t got = span == (size_t)1 << 20 ? thm::mapped_cut(s, n, pos, want, &got_lines) : thm::mapped_cut(s, n, pos, want, &got_lines, span);
        CHECK(got == end && got_lines == lines, "mapped_cut: length %zu from %zu, %llu lines wanted, span %zu: end %zu for %zu, lines %llu for %llu", n, pos,
              want, span, got, end, (unsigned long long)got_lines, lines);
        n_cases++;
      }
    }
}

struct Member {
  uint32_t isize;
};

void check_groups(const std::vector<Member>& tab) {
  const size_t n = tab.size();
  for (size_t k = 0; k < n; k++)
    for (unsigned want = 0; want <= 12; want++) {
      // the first prefix of tab[k, n) of at least one member that reaches the size, or all of it
      size_t end = k + 1;
      unsigned long long have = tab[k].isize;
      while (end < n && have < want) have += tab[end++].isize;
      const size_t got = thm::member_group_end(tab, n, k, (double)want);
      CHECK(got > k && got <= n && got == end, "member_group_end: %zu members from %zu, %u bytes wanted: %zu for %zu", n, k, want, got, end);
      n_cases++;
    }
}

}  // namespace

int main() {
  for (size_t n = 0; n <= 12; n++)
    for (unsigned bits = 0; bits < (1u << n); bits++) {
      std::unique_ptr<char[]> s(new char[n]);
      for (size_t i = 0; i < n; i++) s[i] = (bits >> i) & 1 ? '\n' : 'a';
      check_host_cut(s.get(), n);
      check_mapped_cut(s.get(), n);
    }
  static const uint32_t sizes[] = {0, 1, 5};
  for (size_t n = 1; n <= 6; n++) {
    size_t combos = 1;
    for (size_t i = 0; i < n; i++) combos *= 3;
    for (size_t c = 0; c < combos; c++) {
      std::vector<Member> tab(n);
      size_t x = c;
      for (size_t i = 0; i < n; i++, x /= 3) tab[i].isize = sizes[x % 3];
      check_groups(tab);
    }
  }
  printf("cases %llu\n", n_cases);
  return 0;
}
