// The coordinate sort of BAM records run serially on the host through the functions the kernels spread over threads
// (thermite_amd/csrc/bam_sort_device.h): keys -> std::stable_sort over the bits the device sort looks at -> scan of the
// sorted lengths -> every window of the sorted stream assembled twice, record by record (window_records + clip) and, as
// the gather kernel does it, 16-byte piece by piece (record_at + clip with the piece as the window).
//   bam_sort_model_main <records.bin> <n_sq> <window bytes> <out.bin>
// writes the windows back to back and prints "records N bytes B windows W".  Exit 2: the two assemblies differ.
// Sanitizer build: g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I thermite_amd/csrc tests/cpp/bam_sort_model_main.cpp
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bam_sort_device.h"

using namespace thm;

int main(int argc, char** argv) {
  if (argc != 5) return 64;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 66;
  std::vector<uint8_t> in;
  uint8_t buf[65536];
  for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) in.insert(in.end(), buf, buf + k);
  fclose(f);
  const uint32_t n_sq = (uint32_t)strtoul(argv[2], nullptr, 10);
  const uint64_t window = strtoull(argv[3], nullptr, 10);
  if (window == 0 || window % bsort::PIECE) return 64;
  // records and keys, as the key kernel takes them: key, length, place
  std::vector<uint64_t> key, loc;
  std::vector<uint32_t> len;
  for (uint64_t at = 0; at < in.size();) {
    if (in.size() - at < bsort::MIN_RECORD) return 65;
    const uint64_t n = (uint64_t)bsort::load_le32(&in[at]) + 4;
    if (n < bsort::MIN_RECORD || n > in.size() - at) return 65;
    key.push_back(bsort::record_key(&in[at], n_sq));
    len.push_back((uint32_t)n);
    loc.push_back(at);
    at += n;
  }
  const uint64_t n = key.size();
  // the radix sort sees bits [0, key_bits) only
  const uint32_t bits = bsort::key_bits(n_sq);
  const uint64_t mask = bits >= 64 ? ~0ull : (1ull << bits) - 1;
  std::vector<uint32_t> ord(n);
  for (uint64_t i = 0; i < n; i++) ord[i] = (uint32_t)i;
  std::stable_sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) { return (key[x] & mask) < (key[y] & mask); });
  std::vector<uint64_t> off(n + 1, 0), s_loc(n);
  for (uint64_t r = 0; r < n; r++) {
    off[r + 1] = off[r] + len[ord[r]];
    s_loc[r] = loc[ord[r]];
  }
  const uint64_t total = off[n];
  FILE* o = fopen(argv[4], "wb");
  if (!o) return 73;
  uint64_t n_windows = 0;
  for (uint64_t w0 = 0; w0 < total; w0 += window, n_windows++) {
    const uint64_t w1 = std::min(w0 + window, total);
    std::vector<uint8_t> a(w1 - w0, 0xEE), b(w1 - w0, 0xDD);
    uint64_t first, last;
    bsort::window_records(off.data(), n, w0, w1, &first, &last);
    for (uint64_t r = first; r < last; r++) {
      const bsort::Part q = bsort::clip(off[r], off[r + 1], w0, w1);
      if (q.dst + q.n > a.size() || q.src + q.n > off[r + 1] - off[r]) return 3;
      memcpy(&a[q.dst], &in[s_loc[r] + q.src], q.n);
    }
    for (uint64_t p0 = w0; p0 < w1; p0 += bsort::PIECE) {
      const uint64_t p1 = std::min<uint64_t>(p0 + bsort::PIECE, w1);
      uint64_t r = bsort::record_at(off.data(), n, p0);
      for (uint64_t at = p0; at < p1; r++) {
        const bsort::Part q = bsort::clip(off[r], off[r + 1], p0, p1);
        if (q.n == 0 || q.dst + q.n > p1 - p0) return 3;
        memcpy(&b[p0 - w0 + q.dst], &in[s_loc[r] + q.src], q.n);
        at = off[r + 1];
      }
    }
    if (a != b) return 2;
    if (fwrite(a.data(), 1, a.size(), o) != a.size()) return 74;
  }
  fclose(o);
  printf("records %llu bytes %llu windows %llu\n", (unsigned long long)n, (unsigned long long)total, (unsigned long long)n_windows);
  return 0;
}
