// The BAI index of a sorted record stream built serially on the host through the functions the kernels spread over
// threads (thermite_amd/csrc/bai_device.h), pass by pass as kernels_bai.hip and bai.hip run them, with plain loops where
// the device scans and sorts: fields -> run heads, scan, runs -> std::stable_sort over the bits the device sort looks at
// -> chunk and bin heads, scans, chunks -> the linear table's minima and the backward fill -> reference sizes, scan ->
// the bytes.
//   bai_model_main <sorted records.bin> <n_sq> <member sizes.bin: u64 each> <first member offset> <out.bai>
// Exit 3: a record ends beyond 2^29.  4: a CIGAR leaves its record.  5: an emitter wrote outside the file or left a gap.
// Sanitizer build: g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I thermite_amd/csrc tests/cpp/bai_model_main.cpp
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bai_device.h"

using namespace thm;
typedef std::vector<uint64_t> V64;

static std::vector<uint8_t> slurp(const char* path) {
  std::vector<uint8_t> in;
  FILE* f = fopen(path, "rb");
  if (!f) exit(66);
  uint8_t buf[65536];
  for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) in.insert(in.end(), buf, buf + k);
  fclose(f);
  return in;
}

static V64 scan(const V64& in) {  // n -> n + 1 entries
  V64 out(in.size() + 1, 0);
  for (size_t i = 0; i < in.size(); i++) out[i + 1] = out[i] + in[i];
  return out;
}

int main(int argc, char** argv) {
  if (argc != 6) return 64;
  const std::vector<uint8_t> in = slurp(argv[1]), sizes = slurp(argv[3]);
  const uint32_t n_sq = (uint32_t)strtoul(argv[2], nullptr, 10);
  V64 off(1, 0);
  for (uint64_t at = 0; at < in.size();) {
    if (in.size() - at < bsort::MIN_RECORD) return 65;
    const uint64_t len = (uint64_t)bsort::load_le32(&in[at]) + 4;
    if (len < bsort::MIN_RECORD || len > in.size() - at) return 65;
    off.push_back(at += len);
  }
  const uint64_t n = off.size() - 1, total = off[n], n_members = (total + bai::CUT - 1) / bai::CUT;
  if (sizes.size() != n_members * 8) return 65;
  V64 coff(n_members + 1, strtoull(argv[4], nullptr, 10));
  for (uint64_t m = 0; m < n_members; m++) {
    uint64_t s;
    memcpy(&s, &sizes[8 * m], 8);
    coff[m + 1] = coff[m] + s;
  }
  // fields
  V64 key(n), ref_mapped(n_sq, 0), ref_intv(n_sq, 0);
  std::vector<uint32_t> beg(n), end(n);
  for (uint64_t i = 0; i < n; i++) {
    const bai::Fields f = bai::fields(&in[off[i]], off[i + 1] - off[i]);
    if (!f.ok) return 4;
    if (f.ref_id >= 0 && f.end > bai::MAX_END) return 3;
    key[i] = bai::key(f.ref_id, f.ref_id >= 0 ? bai::reg2bin(f.beg, (int64_t)f.end) : 0, n_sq);
    beg[i] = f.beg | (f.mapped ? bai::MAPPED_BIT : 0u);
    end[i] = (uint32_t)f.end;
    if (f.ref_id >= 0 && f.mapped) {
      ref_mapped[f.ref_id]++;
      ref_intv[f.ref_id] = std::max<uint64_t>(ref_intv[f.ref_id], bai::last_window(f.end) + 1);
    }
  }
  const V64 intv_off = scan(ref_intv);
  // run heads, the records of every reference
  V64 flag(n), ref_first(n_sq, 0), ref_end(n_sq, 0);
  uint64_t n_coor = n;
  for (uint64_t i = 0; i <= n; i++) {
    const bool has_prev = i > 0, has_cur = i < n;
    const uint64_t k = has_cur ? key[i] : (uint64_t)n_sq << 16, kp = has_prev ? key[i - 1] : 0;
    if (has_cur) flag[i] = bai::run_head(has_prev, kp, k, n_sq);
    const uint32_t rc = bai::key_ref(k), rp = has_prev ? bai::key_ref(kp) : 0xffffffffu;
    if (rc != rp) {
      if (rc < n_sq)
        ref_first[rc] = i;
      else
        n_coor = i;
      if (has_prev && rp < n_sq) ref_end[rp] = i;
    }
  }
  const V64 idx = scan(flag);
  const uint64_t n_runs = idx[n];
  V64 run_key(n_runs), run_beg(n_runs), run_end(n_runs);
  for (uint64_t i = 0; i <= n; i++) {
    const bool has_prev = i > 0, has_cur = i < n;
    const uint64_t k = has_cur ? key[i] : 0, kp = has_prev ? key[i - 1] : 0;
    if (has_cur && bai::run_head(has_prev, kp, k, n_sq)) {
      run_key[idx[i]] = k;
      run_beg[idx[i]] = off[i];
    }
    if (bai::run_end(has_prev, kp, has_cur, k, n_sq)) run_end[idx[i] - 1] = off[i];
  }
  // the linear table
  V64 table(intv_off[n_sq], bai::NONE);
  for (uint64_t i = 0; i < n_coor; i++) {
    if (!(beg[i] & bai::MAPPED_BIT)) continue;
    const uint32_t b = beg[i] & ~bai::MAPPED_BIT, r = bai::key_ref(key[i]);
    const bool prev_same = i > 0 && bai::key_ref(key[i - 1]) == r && (beg[i - 1] & bai::MAPPED_BIT);
    uint64_t* t = &table[intv_off[r]];
    const uint32_t w0 = bai::first_window(b), w1 = bai::last_window(end[i]);
    if (bai::enters_first_window(prev_same, i > 0 ? beg[i - 1] & ~bai::MAPPED_BIT : 0, b)) t[w0] = std::min(t[w0], off[i]);
    for (uint32_t w = w0 + 1; w <= w1; w++) t[w] = std::min(t[w], off[i]);
  }
  for (uint32_t r = 0; r < n_sq; r++) {
    uint64_t above = bai::NONE;
    for (uint64_t w = intv_off[r + 1]; w > intv_off[r]; w--) above = table[w - 1] = bai::fill(table[w - 1], above);
  }
  // the runs by key, stably, over the bits the radix sort sees
  const uint64_t mask = (1ull << bai::key_bits(n_sq)) - 1;
  std::vector<uint32_t> ord(n_runs);
  for (uint64_t j = 0; j < n_runs; j++) ord[j] = (uint32_t)j;
  std::stable_sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) { return (run_key[x] & mask) < (run_key[y] & mask); });
  V64 skey(n_runs), chunk_flag(n_runs), bin_flag(n_runs);
  for (uint64_t j = 0; j < n_runs; j++) skey[j] = run_key[ord[j]];
  for (uint64_t j = 0; j < n_runs; j++) {
    bool bin = true, chunk = true;
    if (j > 0) {
      bin = skey[j] != skey[j - 1];
      chunk = bin || !bai::merges(run_end[ord[j - 1]], run_beg[ord[j]]);
    }
    bin_flag[j] = bin;
    chunk_flag[j] = chunk;
  }
  const V64 chunk_idx = scan(chunk_flag), bin_idx = scan(bin_flag);
  const uint64_t n_chunks = chunk_idx[n_runs], n_bins = bin_idx[n_runs];
  V64 chunk_beg(n_chunks), chunk_end(n_chunks), chunk_bin(n_chunks), bin_key(n_bins), bin_chunk0(n_bins + 1, 0), ref_bin0(n_sq, 0), ref_bin1(n_sq, 0);
  for (uint64_t j = 0; n_runs && j <= n_runs; j++) {
    const bool has_cur = j < n_runs, has_prev = j > 0;
    const bool chunk = has_cur && chunk_flag[j], bin = has_cur && bin_flag[j];
    const uint64_t c = chunk_idx[j], b = bin_idx[j];
    if (chunk) {
      chunk_beg[c] = run_beg[ord[j]];
      chunk_bin[c] = b + (bin ? 1 : 0) - 1;
    }
    if (has_prev && (!has_cur || chunk)) chunk_end[c - 1] = run_end[ord[j - 1]];
    if (bin) {
      bin_key[b] = skey[j];
      bin_chunk0[b] = c;
    }
    if (!has_cur) bin_chunk0[b] = c;
    const uint32_t rc = has_cur ? bai::key_ref(skey[j]) : 0xfffffffeu, rp = has_prev ? bai::key_ref(skey[j - 1]) : 0xffffffffu;
    if (rc != rp) {
      if (has_cur) ref_bin0[rc] = b;
      if (has_prev) ref_bin1[rp] = b;
    }
  }
  // sizes, places, bytes
  V64 ref_size(n_sq);
  for (uint32_t r = 0; r < n_sq; r++)
    ref_size[r] = bai::ref_bytes(ref_bin1[r] - ref_bin0[r], bin_chunk0[ref_bin1[r]] - bin_chunk0[ref_bin0[r]], ref_end[r] > ref_first[r], ref_intv[r]);
  const V64 ref_at = scan(ref_size);
  const uint64_t n_bytes = bai::file_bytes(ref_at[n_sq]);
  std::vector<uint8_t> out(n_bytes + 16, 0xEE);  // (16 bytes the emitters must leave alone)
  std::vector<uint8_t> seen(n_bytes + 16, 0);
  bool bad = false;
  auto put32 = [&](uint64_t at, uint32_t v) {
    if (at + 4 > n_bytes || (at & 3) || seen[at]) bad = true, at = n_bytes + 8;
    seen[at] = 1;
    bai::put32(out.data(), at, v);
  };
  auto put64 = [&](uint64_t at, uint64_t v) {
    put32(at, (uint32_t)v);
    put32(at + 4, (uint32_t)(v >> 32));
  };
  put32(0, 0x01494142u);
  put32(4, n_sq);
  put64(n_bytes - bai::TAIL_BYTES, n - n_coor);
  for (uint32_t r = 0; r < n_sq; r++) {
    const uint64_t at = bai::HEAD_BYTES + ref_at[r], b0 = ref_bin0[r], b1 = ref_bin1[r], nb = b1 - b0, nc = bin_chunk0[b1] - bin_chunk0[b0];
    const bool has = ref_end[r] > ref_first[r];
    put32(at, (uint32_t)(nb + (has ? 1 : 0)));
    if (has) {
      const uint64_t ps = bai::bin_at(at, nb, nc);
      put32(ps, bai::PSEUDO_BIN);
      put32(ps + 4, 2);
      put64(ps + 8, bai::voff(coff.data(), off[ref_first[r]]));
      put64(ps + 16, bai::voff(coff.data(), off[ref_end[r]]));
      put64(ps + 24, ref_mapped[r]);
      put64(ps + 32, ref_end[r] - ref_first[r] - ref_mapped[r]);
    }
    const uint64_t lin = bai::linear_at(at, nb, nc, has);
    put32(lin, (uint32_t)ref_intv[r]);
    for (uint64_t w = 0; w < ref_intv[r]; w++) put64(lin + 4 + 8 * w, bai::voff(coff.data(), table[intv_off[r] + w]));
  }
  for (uint64_t c = 0; c < n_chunks; c++) {
    const uint64_t b = chunk_bin[c], k = bin_key[b];
    const uint32_t r = bai::key_ref(k);
    const uint64_t b0 = ref_bin0[r], c0 = bin_chunk0[b];
    const uint64_t at = bai::bin_at(bai::HEAD_BYTES + ref_at[r], b - b0, c0 - bin_chunk0[b0]);
    if (c == c0) {
      put32(at, bai::key_bin(k));
      put32(at + 4, (uint32_t)(bin_chunk0[b + 1] - c0));
    }
    put64(bai::chunk_at(at, c - c0), bai::voff(coff.data(), chunk_beg[c]));
    put64(bai::chunk_at(at, c - c0) + 8, bai::voff(coff.data(), chunk_end[c]));
  }
  for (uint64_t at = 0; at < n_bytes; at += 4) bad = bad || !seen[at];
  if (bad) return 5;
  FILE* o = fopen(argv[5], "wb");
  if (!o) return 73;
  if (fwrite(out.data(), 1, n_bytes, o) != n_bytes) return 74;
  fclose(o);
  printf("records %llu runs %llu chunks %llu bins %llu windows %llu bytes %llu\n", (unsigned long long)n, (unsigned long long)n_runs,
         (unsigned long long)n_chunks, (unsigned long long)n_bins, (unsigned long long)intv_off[n_sq], (unsigned long long)n_bytes);
  return 0;
}
