// The rules of the device BGZF inflater (thermite_amd/csrc/inflate_device.h) run serially on the host, in the order of
// inflate.hip and kernels_inflate.hip: the walk of the member chain, then per member inflate_member and copy_out with
// every lane-parallel phase as a loop over the 64 lanes -- what the kernel computes, without a device.
//   inflate_model_main <head_len> <in: gzip members back to back> <out> [<in> <out> ...]
// <out> begins with one line of text:
//   "walk\n"                                the chain is not one the device takes (the host inflater has the bytes)
//   "declined <member> <status> <paths>\n"  the first member that ends with a status word other than 0
//   "ok <members> <paths> <bytes>\n"        followed by the inflated bytes (paths: the P_ bits of all members together)
// The inflated bytes are placed as the device places them, behind head_len bytes, so that member outputs fall on every
// alignment.  Buffers are allocated to the byte: a read or write beyond them is one the sanitizers see.
// tests/test_inflate_device_host.py builds and runs it plainly and as
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Ithermite_amd/csrc
//       tests/cpp/inflate_model_main.cpp -o inflate_model_asan
// over all fixtures, the corrupt ones included (a stand-alone host program: nothing is preloaded).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "inflate_device.h"
using namespace thm::inf;

static int run(uint64_t head_len, const char* in_path, const char* out_path) {
  FILE* f = fopen(in_path, "rb");
  if (!f) return 2;
  fseek(f, 0, SEEK_END);
  const uint64_t n = (uint64_t)ftell(f);
  fseek(f, 0, SEEK_SET);
  // to the next multiple of 4 and no further: the reader takes whole words
  const uint64_t padded = (n + 3) / 4 * 4;
  uint8_t* exact = (uint8_t*)malloc(padded ? padded : 4);  // (malloc's blocks are 16-byte aligned)
  memset(exact, 0, padded ? padded : 4);
  if (n && fread(exact, 1, n, f) != n) return 2;
  fclose(f);
  uint8_t* const members = exact;
  FILE* o = fopen(out_path, "wb");
  if (!o) return 2;
  std::vector<Member> tab;
  uint64_t at = 0, out_off = head_len;
  bool walked = true;
  while (at < n) {
    Member m;
    uint64_t size = 0;
    if (!walk_member(members, n, at, out_off, &m, &size)) {
      walked = false;
      break;
    }
    tab.push_back(m);
    at += size;
    out_off += m.isize;
  }
  if (!walked) {
    fputs("walk\n", o);
    fclose(o);
    free(exact);
    return 0;
  }
  const uint64_t total = out_off;
  uint8_t* block = (uint8_t*)aligned_alloc(16, (total + 15) / 16 * 16 + 16);
  // (the block's end stands where the allocation ends: a store past it is out of bounds)
  uint8_t* const dst0 = block + ((total + 15) / 16 * 16 + 16 - total) / 16 * 16;
  uint32_t* outw = (uint32_t*)malloc((MAX_OUT / 4 + 4) * 4);
  Work* w = (Work*)malloc(sizeof(Work));
  memset(outw, 0xAA, (MAX_OUT / 4 + 4) * 4);
  memset(w, 0xAA, sizeof(Work));
  uint32_t paths = 0;
  for (size_t k = 0; k < tab.size(); k++) {
    const Member& m = tab[k];
    const uint32_t lo = (uint32_t)(m.in_off & 3u);
    const Result r = inflate_member(members + (m.in_off - lo), lo, lo + m.in_len, m.isize, m.crc, outw, *w);
    if (r.status != OK) {
      fprintf(o, "declined %zu %u %u\n", k, r.status, r.paths);
      fclose(o);
      free(exact), free(block), free(outw), free(w);
      return 0;
    }
    paths |= r.paths;
    for (uint32_t lane = 0; lane < LANES; lane++) copy_out(dst0 + m.out_off, outw, m.isize, lane);
  }
  fprintf(o, "ok %zu %u %llu\n", tab.size(), paths, (unsigned long long)(total - head_len));
  if (total > head_len) fwrite(dst0 + head_len, 1, total - head_len, o);
  fclose(o);
  free(exact), free(block), free(outw), free(w);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 4 || (argc - 2) % 2 != 0) {
    fprintf(stderr, "usage: inflate_model_main <head_len> <in> <out> [<in> <out> ...]\n");
    return 2;
  }
  const uint64_t head_len = strtoull(argv[1], nullptr, 10);
  for (int k = 2; k + 1 < argc; k += 2)
    if (int rc = run(head_len, argv[k], argv[k + 1])) return rc;
  return 0;
}
