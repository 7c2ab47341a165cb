// bgzf_device.h -- the steps of the device BGZF encoder (kernels_bgzf.hip), each a plain function of the item it works
// on (a position, a segment, the block), so that the kernel is nothing but these functions spread over threads with
// barriers between them.  They compile for the host too: tests/cpp/bgzf_model_main.cpp runs the same steps serially,
// which is how the output format is checked without a device (that file gives the sanitizer build line).
//
// One BGZF block of at most 0xff00 input bytes:
//   match    per position: the longest match among the hash-table candidate (latest earlier-tile position with the same
//            hash of 4 bytes) and the distances 1..N_PROBE, verified byte by byte
//   parse    per segment of SEG bytes: greedy with one step of lazy evaluation, matches clipped at the segment end;
//            tokens overwrite the segment's match entries; symbol histogram
//   codes    the block: code lengths as code_lengths() of io_deflate.cpp builds them (two-queue Huffman, limited on the
//            counts per length), the run-length coded header, canonical codes
//   emit     per segment at its bit offset, or_word() into a zeroed staging area
//   crc      per segment by table, combined with x^(8 len) mod P
#ifndef THERMITE_BGZF_DEVICE_H
#define THERMITE_BGZF_DEVICE_H
#include <cstdint>

#if defined(__HIPCC__)
#define BGZ_M __host__ __device__
#else
#define BGZ_M
#endif
#define BGZ_HD BGZ_M inline

namespace thm {
namespace bgz {

constexpr uint32_t BLOCK_IN = 0xff00;           // input bytes per BGZF block, as bgzf_compress cuts
constexpr uint32_t SLOT = 65536;                // stride of the members before compaction (a member is at most BLOCK_IN + 31)
constexpr uint32_t SEG = 1020, N_SEG = 64;      // parse / emit segments: N_SEG * SEG == BLOCK_IN
constexpr uint32_t TILE = 256;                  // positions looked up, then entered, together
constexpr uint32_t HASH_BITS = 14, N_PROBE = 8;
constexpr uint32_t MAX_DIST = 32768, MAX_MATCH = 258;
constexpr uint32_t STAGE_WORDS = 1u << HASH_BITS;  // the staging area takes the table's place: 64 KiB
static_assert(N_SEG * SEG == BLOCK_IN, "segments tile the block");
static_assert(STAGE_WORDS * 4 >= BLOCK_IN + 8, "a dynamic block that is kept is shorter than the stored one");

// everything of a block that is not the input, the table or the per-position scratch
struct Small {
  uint32_t lfreq[288], dfreq[32], cfreq[20];
  uint32_t w[2 * 288];  // node weights of the Huffman construction
  uint16_t parent[2 * 288], leaves_l[288], leaves_d[32], leaves_c[20];  // leaves: used symbols by (frequency, symbol)
  uint8_t depth[2 * 288];
  uint8_t llen[288], dlen[32], clen[20];
  uint16_t lcode[288], dcode[32], ccode[20];
  uint8_t rl_sym[320], rl_extra[320];
  uint32_t seg_ntok[N_SEG], seg_bits[N_SEG], seg_crc[N_SEG];
  uint32_t crc_tab[256];
  uint32_t n_leaves_l, n_leaves_d, n_rl, hlit, hdist, hclen, hdr_bits, total_bits, stored, crc;
};

// ---- atomics: the device's on shared memory, plain on the host (the model is serial) ----
#if defined(__HIP_DEVICE_COMPILE__)
BGZ_HD void add_word(uint32_t* p, uint32_t v) { atomicAdd(p, v); }
BGZ_HD void or_word(uint32_t* p, uint32_t v) { atomicOr(p, v); }
BGZ_HD void max_word(uint32_t* p, uint32_t v) { atomicMax(p, v); }
#else
BGZ_HD void add_word(uint32_t* p, uint32_t v) { *p += v; }
BGZ_HD void or_word(uint32_t* p, uint32_t v) { *p |= v; }
BGZ_HD void max_word(uint32_t* p, uint32_t v) { if (v > *p) *p = v; }
#endif

BGZ_HD uint32_t load32(const uint8_t* in, uint32_t p) {
  return (uint32_t)in[p] | (uint32_t)in[p + 1] << 8 | (uint32_t)in[p + 2] << 16 | (uint32_t)in[p + 3] << 24;
}
BGZ_HD uint32_t hash4(uint32_t v) { return (v * 2654435761u) >> (32 - HASH_BITS); }
BGZ_HD uint32_t ilog2(uint32_t v) {  // v > 0
  uint32_t k = 0;
  while (v >>= 1) k++;
  return k;
}

// length 3..258 -> symbol - 257, extra bit count, extra value (RFC 1951 section 3.2.5)
BGZ_HD void len_code(uint32_t len, uint32_t* sym, uint32_t* nx, uint32_t* x) {
  const uint32_t l = len - 3;
  if (len == 258) {
    *sym = 28, *nx = 0, *x = 0;
  } else if (l < 8) {
    *sym = l, *nx = 0, *x = 0;
  } else {
    const uint32_t e = ilog2(l) - 2;
    *sym = 4 * e + 4 + ((l >> e) & 3), *nx = e, *x = l & ((1u << e) - 1);
  }
}
// distance 1..32768 -> code, extra bit count, extra value
BGZ_HD void dist_code(uint32_t dist, uint32_t* sym, uint32_t* nx, uint32_t* x) {
  const uint32_t d = dist - 1;
  if (d < 4) {
    *sym = d, *nx = 0, *x = 0;
  } else {
    const uint32_t k = ilog2(d), e = k - 1;
    *sym = 2 * k + ((d >> e) & 1), *nx = e, *x = d & ((1u << e) - 1);
  }
}

// ---- match: entry of position p is len << 16 | (dist - 1), 0 for none.  `cand1` is the table's entry for p's hash as
// it stood before p's tile was entered: a position + 1, or 0 ----
BGZ_HD uint32_t extend(const uint8_t* in, uint32_t p, uint32_t q, uint32_t mx) {
  uint32_t l = 0;
  while (l + 4 <= mx && load32(in, q + l) == load32(in, p + l)) l += 4;
  while (l < mx && in[q + l] == in[p + l]) l++;
  return l;
}
BGZ_HD uint32_t find_match(const uint8_t* in, uint32_t n, uint32_t p, uint32_t cand1) {
  if (p + 4 > n) return 0;
  const uint32_t mx = n - p < MAX_MATCH ? n - p : MAX_MATCH;
  const uint32_t v = load32(in, p);
  uint32_t best = 0, best_d = 0;
  // the nearest sources first: a tile-synchronous table cannot see them (runs of one byte, short periods)
  for (uint32_t d = 1; d <= N_PROBE && d <= p && best < mx; d++) {
    if (load32(in, p - d) != v) continue;
    if (best && in[p - d + best] != in[p + best]) continue;  // cannot be longer
    const uint32_t l = extend(in, p, p - d, mx);
    if (l > best) best = l, best_d = d;
  }
  if (cand1 && best < mx) {
    const uint32_t q = cand1 - 1, d = p - q;  // q lies in an earlier tile: d >= 1
    if (d <= MAX_DIST && load32(in, q) == v && (!best || in[q + best] == in[p + best])) {
      const uint32_t l = extend(in, p, q, mx);
      if (l > best) best = l, best_d = d;
    }
  }
  if (best < 4) return 0;
  return best << 16 | (best_d - 1);
}

// ---- parse of segment [lo, hi): tokens (literal: the byte; match: 1 << 31 | (len - 3) << 16 | (dist - 1)) go to
// mt[lo ..], over the match entries already read; returns their number ----
BGZ_HD uint32_t clipped_len(uint32_t m, uint32_t room) {
  uint32_t len = m >> 16;
  if (len > room) len = room;
  // a clipped match of 3 pays only near by
  if (len < 3 || (len == 3 && (m & 0xFFFF) >= 4096)) return 0;
  return len;
}
BGZ_HD uint32_t parse_segment(const uint8_t* in, uint32_t* mt, uint32_t lo, uint32_t hi, Small& sm) {
  uint32_t i = lo, k = lo;
  uint32_t m = lo < hi ? mt[lo] : 0;
  while (i < hi) {
    const uint32_t m1 = i + 1 < hi ? mt[i + 1] : 0;  // (read before mt[k], k <= i, is written)
    const uint32_t len = clipped_len(m, hi - i);
    if (len && !(i + 1 < hi && clipped_len(m1, hi - i - 1) > len)) {
      uint32_t ls, ds, nx, x;
      len_code(len, &ls, &nx, &x);
      dist_code((m & 0xFFFF) + 1, &ds, &nx, &x);
      add_word(&sm.lfreq[257 + ls], 1);
      add_word(&sm.dfreq[ds], 1);
      mt[k++] = 1u << 31 | (len - 3) << 16 | (m & 0xFFFF);
      i += len;
      m = i < hi ? mt[i] : 0;
    } else {
      add_word(&sm.lfreq[in[i]], 1);
      mt[k++] = in[i];
      i++;
      m = m1;
    }
  }
  return k - lo;
}

// ---- codes ----
// place of symbol s among the used ones, by (frequency, symbol): the sort of code_lengths(), one symbol at a time
BGZ_HD void rank_symbol(const uint32_t* freq, uint32_t n, uint32_t s, uint16_t* leaves) {
  const uint32_t f = freq[s];
  if (!f) return;
  uint32_t r = 0;
  for (uint32_t t = 0; t < n; t++) {
    const uint32_t g = freq[t];
    r += g && (g < f || (g == f && t < s));
  }
  leaves[r] = (uint16_t)s;
}
BGZ_HD uint32_t count_used(const uint32_t* freq, uint32_t n) {
  uint32_t c = 0;
  for (uint32_t t = 0; t < n; t++) c += freq[t] != 0;
  return c;
}
// code_lengths() of io_deflate.cpp from the sorted leaves on
BGZ_HD void build_lengths(const uint32_t* freq, uint32_t n, const uint16_t* leaves, uint32_t n_leaves, uint32_t max_len, uint8_t* len,
                          Small& sm) {
  for (uint32_t i = 0; i < n; i++) len[i] = 0;
  if (n_leaves == 0) return;
  if (n_leaves == 1) {
    len[leaves[0]] = 1;
    return;
  }
  uint32_t* w = sm.w;
  uint16_t* parent = sm.parent;
  uint8_t* depth = sm.depth;
  for (uint32_t i = 0; i < n_leaves; i++) w[i] = freq[leaves[i]];
  uint32_t qa = 0, qb = n_leaves, next = n_leaves;
  while ((n_leaves - qa) + (next - qb) > 1) {
    uint32_t pick[2];
    for (int t = 0; t < 2; t++) pick[t] = (qa < n_leaves && (qb >= next || w[qa] <= w[qb])) ? qa++ : qb++;
    w[next] = w[pick[0]] + w[pick[1]];
    parent[pick[0]] = parent[pick[1]] = (uint16_t)next;
    next++;
  }
  uint32_t bl_count[16];
  for (uint32_t b = 0; b < 16; b++) bl_count[b] = 0;
  int overflow = 0;
  depth[next - 1] = 0;
  for (int i = (int)next - 2; i >= 0; i--) {
    uint32_t b = depth[parent[i]] + 1u;
    if (b > max_len) {
      b = max_len;
      overflow++;
    }
    depth[i] = (uint8_t)b;
    if ((uint32_t)i < n_leaves) bl_count[b]++;
  }
  while (overflow > 0) {
    uint32_t b = max_len - 1;
    while (bl_count[b] == 0) b--;
    bl_count[b]--;
    bl_count[b + 1] += 2;
    bl_count[max_len]--;
    overflow -= 2;
  }
  uint32_t h = 0;
  for (uint32_t b = max_len; b >= 1; b--)
    for (uint32_t k = 0; k < bl_count[b]; k++) len[leaves[h++]] = (uint8_t)b;
}
// canonical codes, bit-reversed for the LSB-first stream
BGZ_HD void make_codes(const uint8_t* len, uint32_t n, uint16_t* code) {
  uint32_t count[16], next[16];
  for (uint32_t l = 0; l < 16; l++) count[l] = 0;
  for (uint32_t i = 0; i < n; i++) count[len[i]]++;
  count[0] = 0;
  uint32_t c = 0;
  next[0] = 0;
  for (uint32_t l = 1; l <= 15; l++) {
    c = (c + count[l - 1]) << 1;
    next[l] = c;
  }
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t l = len[i];
    uint32_t r = 0;
    if (l) {
      const uint32_t v = next[l]++;
      for (uint32_t b = 0; b < l; b++) r |= ((v >> b) & 1u) << (l - 1 - b);
    }
    code[i] = (uint16_t)r;
  }
}
BGZ_HD uint32_t cl_order(uint32_t k) {
  const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  return order[k];
}
// Lengths and codes of the three alphabets, the run-length coded header and its size; the leaves of the literal/length
// and distance alphabets are sorted already (leaves_l, leaves_d, n_leaves_l, n_leaves_d).  One thread.
BGZ_HD void build_codes(Small& sm) {
  build_lengths(sm.lfreq, 286, sm.leaves_l, sm.n_leaves_l, 15, sm.llen, sm);
  build_lengths(sm.dfreq, 30, sm.leaves_d, sm.n_leaves_d, 15, sm.dlen, sm);
  // fewer than two distances in use: a second code of one bit beside the one (or none) in use, so that this code is
  // complete as the others are (a lone 1-bit code is tolerated by inflaters, not required of them)
  if (sm.n_leaves_d == 0) sm.dlen[0] = sm.dlen[1] = 1;
  else if (sm.n_leaves_d == 1) sm.dlen[sm.leaves_d[0] ? 0 : 1] = 1;
  make_codes(sm.llen, 286, sm.lcode);
  make_codes(sm.dlen, 30, sm.dcode);
  uint32_t hlit = 286, hdist = 30;
  while (hlit > 257 && sm.llen[hlit - 1] == 0) hlit--;
  while (hdist > 1 && sm.dlen[hdist - 1] == 0) hdist--;
  const uint32_t n_all = hlit + hdist;
  uint32_t n_rl = 0;
  for (uint32_t k = 0; k < 19; k++) sm.cfreq[k] = 0;
  auto at = [&](uint32_t k) -> uint32_t { return k < hlit ? sm.llen[k] : sm.dlen[k - hlit]; };
  auto put = [&](uint32_t s, uint32_t x) {
    sm.rl_sym[n_rl] = (uint8_t)s;
    sm.rl_extra[n_rl++] = (uint8_t)x;
    sm.cfreq[s]++;
  };
  for (uint32_t k = 0; k < n_all;) {
    const uint32_t v = at(k);
    uint32_t run = 1;
    while (k + run < n_all && at(k + run) == v) run++;
    if (v == 0 && run >= 3) {
      const uint32_t r = run < 138 ? run : 138;
      if (r <= 10) put(17, r - 3);
      else put(18, r - 11);
      k += r;
    } else if (run >= 4) {  // the value once, then repeats of 3..6
      put(v, 0);
      uint32_t left = run - 1;
      k += 1;
      while (left >= 3) {
        const uint32_t r = left < 6 ? left : 6;
        put(16, r - 3);
        left -= r;
        k += r;
      }
    } else {
      put(v, 0);
      k += 1;
    }
  }
  for (uint32_t s = 0; s < 19; s++) rank_symbol(sm.cfreq, 19, s, sm.leaves_c);
  build_lengths(sm.cfreq, 19, sm.leaves_c, count_used(sm.cfreq, 19), 7, sm.clen, sm);
  make_codes(sm.clen, 19, sm.ccode);
  uint32_t hclen = 19;
  while (hclen > 4 && sm.clen[cl_order(hclen - 1)] == 0) hclen--;
  uint32_t bits = 3 + 14 + 3 * hclen;
  for (uint32_t k = 0; k < n_rl; k++) {
    const uint32_t s = sm.rl_sym[k];
    bits += sm.clen[s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0);
  }
  sm.n_rl = n_rl, sm.hlit = hlit, sm.hdist = hdist, sm.hclen = hclen, sm.hdr_bits = bits;
}

// ---- emit ----
struct BitOut {
  uint32_t* w;
  uint64_t buf;
  uint32_t cnt, at;
  BGZ_M BitOut(uint32_t* words, uint32_t bit_off) : w(words), buf(0), cnt(bit_off & 31), at(bit_off >> 5) {}
  BGZ_M void put(uint32_t v, uint32_t n) {  // n <= 32
    buf |= (uint64_t)v << cnt;
    cnt += n;
    if (cnt >= 32) {
      or_word(&w[at++], (uint32_t)buf);
      buf >>= 32;
      cnt -= 32;
    }
  }
  BGZ_M void finish() {
    if (cnt) or_word(&w[at], (uint32_t)buf);
  }
};
// bits the tokens of a segment take
BGZ_HD uint32_t segment_bits(const uint32_t* tok, uint32_t n_tok, const Small& sm) {
  uint32_t bits = 0;
  for (uint32_t k = 0; k < n_tok; k++) {
    const uint32_t t = tok[k];
    if (!(t >> 31)) {
      bits += sm.llen[t];
      continue;
    }
    uint32_t ls, ds, nl, nd, x;
    len_code(((t >> 16) & 0xFF) + 3, &ls, &nl, &x);
    dist_code((t & 0xFFFF) + 1, &ds, &nd, &x);
    bits += sm.llen[257 + ls] + nl + sm.dlen[ds] + nd;
  }
  return bits;
}
BGZ_HD void emit_segment(const uint32_t* tok, uint32_t n_tok, const Small& sm, uint32_t* stage, uint32_t bit_off) {
  BitOut o(stage, bit_off);
  for (uint32_t k = 0; k < n_tok; k++) {
    const uint32_t t = tok[k];
    if (!(t >> 31)) {
      o.put(sm.lcode[t], sm.llen[t]);
      continue;
    }
    uint32_t ls, ds, nl, nd, xl, xd;
    len_code(((t >> 16) & 0xFF) + 3, &ls, &nl, &xl);
    dist_code((t & 0xFFFF) + 1, &ds, &nd, &xd);
    o.put(sm.lcode[257 + ls] | xl << sm.llen[257 + ls], sm.llen[257 + ls] + nl);
    o.put(sm.dcode[ds] | xd << sm.dlen[ds], sm.dlen[ds] + nd);
  }
  o.finish();
}
// block header at bit 0 and the end-of-block code at `eob_off`
BGZ_HD void emit_header(const Small& sm, uint32_t* stage, uint32_t eob_off) {
  BitOut o(stage, 0);
  o.put(1, 1);  // BFINAL
  o.put(2, 2);  // dynamic Huffman
  o.put(sm.hlit - 257, 5);
  o.put(sm.hdist - 1, 5);
  o.put(sm.hclen - 4, 4);
  for (uint32_t k = 0; k < sm.hclen; k++) o.put(sm.clen[cl_order(k)], 3);
  for (uint32_t k = 0; k < sm.n_rl; k++) {
    const uint32_t s = sm.rl_sym[k];
    o.put(sm.ccode[s], sm.clen[s]);
    if (s == 16) o.put(sm.rl_extra[k], 2);
    else if (s == 17) o.put(sm.rl_extra[k], 3);
    else if (s == 18) o.put(sm.rl_extra[k], 7);
  }
  o.finish();
  BitOut e(stage, eob_off);
  e.put(sm.lcode[256], sm.llen[256]);
  e.finish();
}

// ---- CRC-32 (reflected, polynomial 0xEDB88320) ----
BGZ_HD uint32_t crc_table_entry(uint32_t t) {
  uint32_t c = t;
  for (int k = 0; k < 8; k++) c = c & 1 ? 0xEDB88320u ^ (c >> 1) : c >> 1;
  return c;
}
BGZ_HD uint32_t crc_bytes(const uint32_t* tab, const uint8_t* in, uint32_t lo, uint32_t hi) {
  uint32_t c = 0xFFFFFFFFu;
  for (uint32_t i = lo; i < hi; i++) c = tab[(c ^ in[i]) & 0xFF] ^ (c >> 8);
  return ~c;
}
// a(x) * b(x) mod P over GF(2), bit 31 the coefficient of x^0
BGZ_HD uint32_t crc_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t m = 1u << 31; m; m >>= 1) {
    if (a & m) p ^= b;
    b = b & 1 ? (b >> 1) ^ 0xEDB88320u : b >> 1;
  }
  return p;
}
// x^(8 n) mod P
BGZ_HD uint32_t crc_xpow8(uint32_t n) {
  uint32_t r = 1u << 31, base = 1u << 23;  // x^0, x^8
  for (; n; n >>= 1) {
    if (n & 1) r = crc_mul(r, base);
    base = crc_mul(base, base);
  }
  return r;
}
// CRC of the block from the CRCs of its segments (all of SEG bytes but the last)
BGZ_HD uint32_t crc_combine_segments(const uint32_t* seg_crc, uint32_t n) {
  if (n == 0) return 0;
  const uint32_t n_seg = (n + SEG - 1) / SEG, x_full = crc_xpow8(SEG);
  uint32_t c = seg_crc[0];
  for (uint32_t s = 1; s < n_seg; s++) {
    const uint32_t len = (s + 1) * SEG <= n ? SEG : n - s * SEG;
    c = crc_mul(len == SEG ? x_full : crc_xpow8(len), c) ^ seg_crc[s];
  }
  return c;
}

// ---- the member: byte k of header | payload | CRC | ISIZE ----
// payload: `stage` (dynamic, payload_len bytes) or the stored form of in[0, n)
BGZ_HD uint32_t payload_len(const Small& sm, uint32_t n) { return sm.stored ? n + 5 : (sm.total_bits + 7) / 8; }
BGZ_HD uint32_t member_len(const Small& sm, uint32_t n) { return 18 + payload_len(sm, n) + 8; }
BGZ_HD uint32_t member_byte(const Small& sm, const uint8_t* in, uint32_t n, const uint32_t* stage, uint32_t k) {
  const uint32_t plen = payload_len(sm, n), bsize = 18 + plen + 8 - 1;
  if (k < 18) {
    const uint8_t h[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    return k < 16 ? h[k] : (bsize >> (8 * (k - 16))) & 0xFF;
  }
  k -= 18;
  if (k < plen) {
    if (!sm.stored) return (stage[k >> 2] >> (8 * (k & 3))) & 0xFF;
    if (k >= 5) return in[k - 5];
    return k == 0 ? 1 : k == 1 ? n & 0xFF : k == 2 ? n >> 8 : k == 3 ? ~n & 0xFF : (~n >> 8) & 0xFF;
  }
  k -= plen;
  return ((k < 4 ? sm.crc : n) >> (8 * (k & 3))) & 0xFF;
}

}  // namespace bgz
}  // namespace thm
#endif
