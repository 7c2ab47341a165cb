// The steps of the device BGZF encoder (thermite_amd/csrc/bgzf_device.h) run serially on the host, in the order and
// with the table discipline of kernels_bgzf.hip: what the kernel computes, without a device.
//   bgzf_model_main <in: bytes> <out: the BGZF members back to back>
// tests/test_bgzf_host.py builds and runs it plainly; for bounds and undefined behaviour build it as
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Ithermite_amd/csrc tests/cpp/bgzf_model_main.cpp -o bgzf_model_asan
// and run that program over the same inputs (a stand-alone host program: nothing is preloaded).
#include <cstdio>
#include <cstring>
#include <vector>
#include "bgzf_device.h"
using namespace thm::bgz;
static size_t encode_block(const uint8_t* src, uint32_t n, uint8_t* out) {
  static Small sm;
  memset(&sm, 0, sizeof sm);
  std::vector<uint8_t> inb(n + 16, 0);
  memcpy(inb.data(), src, n);
  const uint8_t* in = inb.data();
  std::vector<uint32_t> table(1u << HASH_BITS, 0), mt(BLOCK_IN, 0), stage(STAGE_WORDS, 0);
  for (uint32_t t = 0; t < 256; t++) sm.crc_tab[t] = crc_table_entry(t);
  for (uint32_t t0 = 0; t0 < n; t0 += TILE) {
    for (uint32_t p = t0; p < t0 + TILE && p < n; p++) mt[p] = p + 4 <= n ? find_match(in, n, p, table[hash4(load32(in, p))]) : 0;
    for (uint32_t p = t0; p < t0 + TILE && p + 4 <= n; p++) max_word(&table[hash4(load32(in, p))], p + 1);
  }
  const uint32_t n_seg = (n + SEG - 1) / SEG;
  for (uint32_t s = 0; s < n_seg; s++) {
    const uint32_t lo = s * SEG, hi = lo + SEG < n ? lo + SEG : n;
    sm.seg_ntok[s] = parse_segment(in, mt.data(), lo, hi, sm);
    sm.seg_crc[s] = crc_bytes(sm.crc_tab, in, lo, hi);
  }
  sm.lfreq[256] = 1;
  for (uint32_t s = 0; s < 286; s++) rank_symbol(sm.lfreq, 286, s, sm.leaves_l);
  for (uint32_t s = 0; s < 30; s++) rank_symbol(sm.dfreq, 30, s, sm.leaves_d);
  sm.n_leaves_l = count_used(sm.lfreq, 286);
  sm.n_leaves_d = count_used(sm.dfreq, 30);
  build_codes(sm);
  for (uint32_t s = 0; s < n_seg; s++) sm.seg_bits[s] = segment_bits(mt.data() + s * SEG, sm.seg_ntok[s], sm);
  uint32_t off = sm.hdr_bits;
  for (uint32_t s = 0; s < n_seg; s++) { const uint32_t b = sm.seg_bits[s]; sm.seg_bits[s] = off; off += b; }
  sm.total_bits = off + sm.llen[256];
  sm.stored = (sm.total_bits + 7) / 8 >= n + 5;
  sm.crc = crc_combine_segments(sm.seg_crc, n);
  if (!sm.stored) {
    emit_header(sm, stage.data(), off);
    for (uint32_t s = 0; s < n_seg; s++) emit_segment(mt.data() + s * SEG, sm.seg_ntok[s], sm, stage.data(), sm.seg_bits[s]);
  }
  const uint32_t m = member_len(sm, n);
  for (uint32_t k = 0; k < m; k++) out[k] = (uint8_t)member_byte(sm, in, n, stage.data(), k);
  return m;
}
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> in;
  uint8_t buf[65536];
  size_t r;
  while ((r = fread(buf, 1, sizeof buf, f)) > 0) in.insert(in.end(), buf, buf + r);
  fclose(f);
  FILE* o = fopen(argv[2], "wb");
  std::vector<uint8_t> out(SLOT);
  for (size_t at = 0; at < in.size(); at += BLOCK_IN) {
    const uint32_t n = (uint32_t)(in.size() - at < BLOCK_IN ? in.size() - at : BLOCK_IN);
    const size_t m = encode_block(in.data() + at, n, out.data());
    fwrite(out.data(), 1, m, o);
  }
  fclose(o);
  return 0;
}
