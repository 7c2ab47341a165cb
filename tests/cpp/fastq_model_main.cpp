// The steps of the device FASTQ parser (thermite_amd/csrc/fastq_device.h) run serially on the host, in the order of
// kernels_fastq.hip and with its walk (chunks of CHUNK bytes, steps of 64 lanes x 4 bytes, one mask per byte position):
// what the kernels compute, without a device.
//   fastq_model_main <in: a block of FASTQ bytes> <out>
// <out> holds "declined\n", or "parsed\n" and the five arrays, each as a u64 byte count and its bytes: names, name_off,
// bases, offsets, quals.  tests/test_fastq_device_host.py builds and runs it plainly; for bounds and undefined behaviour
// build it as
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Ithermite_amd/csrc tests/cpp/fastq_model_main.cpp -o fastq_model_asan
// and run that program over the same inputs (a stand-alone host program: nothing is preloaded).
#include <cstdio>
#include <cstring>
#include <vector>
#include "fastq_device.h"
using namespace thm::fq;
// one step of a wave's walk: the four masks, and every lane's own bits
static void step_masks(const uint8_t* raw, uint64_t at, uint64_t hi, uint64_t m[4], uint32_t mine[64]) {
  m[0] = m[1] = m[2] = m[3] = 0;
  for (uint32_t lane = 0; lane < 64; lane++) {
    const uint64_t i = at + 4ull * lane;
    uint32_t w = 0;
    if (i < hi) memcpy(&w, raw + i, 4);  // (the block is padded, as the device's copy is)
    mine[lane] = newline_bits(w, i, hi);
    for (uint32_t j = 0; j < 4; j++) m[j] |= (uint64_t)((mine[lane] >> j) & 1u) << lane;
  }
}
static void put(FILE* o, const void* p, uint64_t bytes) {
  fwrite(&bytes, 8, 1, o);
  if (bytes) fwrite(p, 1, bytes, o);
}
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> in;
  uint8_t buf[65536];
  size_t got;
  while ((got = fread(buf, 1, sizeof buf, f)) > 0) in.insert(in.end(), buf, buf + got);
  fclose(f);
  const uint64_t n = in.size();
  in.resize(n + 4, 0);
  const uint8_t* raw = in.data();
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  auto declined = [&] {
    fputs("declined\n", o);
    fclose(o);
    return 0;
  };
  if (n == 0) return declined();
  // count, and the scan of the counts
  const uint64_t n_chunks = (n + CHUNK - 1) / CHUNK;
  std::vector<uint64_t> base(n_chunks + 1, 0);
  uint64_t m[4];
  uint32_t mine[64];
  for (uint64_t c = 0; c < n_chunks; c++) {
    const uint64_t lo = c * CHUNK, hi = lo + CHUNK < n ? lo + CHUNK : n;
    uint64_t cnt = 0;
    for (uint64_t at = lo; at < hi; at += STEP) {
      step_masks(raw, at, hi, m, mine);
      cnt += step_count(m);
    }
    base[c + 1] = base[c] + cnt;
  }
  const uint64_t n_newlines = base[n_chunks], n_lines = line_count(n_newlines, raw[n - 1]);
  if (n_lines % 4 != 0) return declined();
  // line starts
  std::vector<uint64_t> ls(n_lines + 1, ~0ull);
  ls[0] = 0;
  if (n_lines > n_newlines) ls[n_lines] = n + 1;
  for (uint64_t c = 0; c < n_chunks; c++) {
    const uint64_t lo = c * CHUNK, hi = lo + CHUNK < n ? lo + CHUNK : n;
    uint64_t k = base[c];
    for (uint64_t at = lo; at < hi; at += STEP) {
      step_masks(raw, at, hi, m, mine);
      for (uint32_t lane = 0; lane < 64; lane++)
        for (uint32_t j = 0; j < 4; j++)
          if ((mine[lane] >> j) & 1u) ls.at(k + step_rank(m, lane, j) + 1) = at + 4ull * lane + j + 1;
      k += step_count(m);
    }
  }
  // the rule per record, the two scans
  const uint64_t nr = n_lines / 4;
  std::vector<uint64_t> name_off(nr + 1, 0), offsets(nr + 1, 0);
  for (uint64_t r = 0; r < nr; r++) {
    Record rec;
    if (!record_rule(raw, ls.data(), r, &rec)) return declined();
    name_off[r + 1] = name_off[r] + rec.name_len;
    offsets[r + 1] = offsets[r] + rec.seq_len;
  }
  // gather, GATHER_LANES lanes a record
  std::vector<uint8_t> names(name_off[nr] + 1), bases(offsets[nr] + 1), quals(offsets[nr] + 1);
  for (uint64_t r = 0; r < nr; r++) {
    uint64_t at;
    (void)line_extent(raw, ls.data(), 4 * r, &at);
    const uint64_t nl = name_off[r + 1] - name_off[r], sl = offsets[r + 1] - offsets[r];
    for (uint32_t lane = 0; lane < GATHER_LANES; lane++) {
      copy_bytes(names.data() + name_off[r], raw + at + 1, nl, lane, GATHER_LANES);
      copy_bytes(bases.data() + offsets[r], raw + ls[4 * r + 1], sl, lane, GATHER_LANES);
      copy_bytes(quals.data() + offsets[r], raw + ls[4 * r + 3], sl, lane, GATHER_LANES);
    }
  }
  fputs("parsed\n", o);
  put(o, names.data(), name_off[nr]);
  put(o, name_off.data(), (nr + 1) * 8);
  put(o, bases.data(), offsets[nr]);
  put(o, offsets.data(), (nr + 1) * 8);
  put(o, quals.data(), offsets[nr]);
  fclose(o);
  return 0;
}
