// inflate_device.h -- the rules of the device BGZF inflater (kernels_inflate.hip; host side inflate.hip; DESIGN.md
// section 4.13), as functions that compile for the host too: tests/cpp/inflate_model_main.cpp runs the same text
// serially, which is how the decoder is checked -- corrupt streams first of all, under the sanitizers -- before a byte
// of it reaches a device (that file gives the build lines).
//
// One BGZF member is one work item of one wavefront:
//   walk     (host) the member chain: header rule, payload extent, CRC-32 and ISIZE of every member -> Member table
//   inflate  the raw DEFLATE stream into `out`, at most MAX_OUT bytes that live in LDS on the device.  The symbol loop is
//            wave-uniform: bit buffer, positions and table entries are the same in every lane (INF_UNIFORM keeps them in
//            scalar registers); the lanes share the work where there is some to share -- the table build (a lane per
//            symbol), stored and match copies (64 bytes a step, index modulo distance where source and destination
//            overlap), the CRC-32 (a segment per lane, combined with crc_mul / crc_xpow8 of bgzf_device.h)
//   copy_out `out` to its place in the block, 16-byte stores where the destination is aligned
// Lane-parallel phases are written INF_LANES(lane) { ... } with INF_SYNC() between phases that hand data from lane to
// lane: on the device the body runs once in every lane, on the host as a loop over the 64 lanes.
//
// What RFC 1951 says about a block stands here once, for this inflater and for the one of plain gzip (gzip_device.h):
// decode_block<Sink> reads BFINAL / BTYPE, the stored prologue, the fixed or dynamic header (fixed_lengths,
// read_dynamic_header), builds both tables and runs the symbol loop; the bytes go to a sink, a template parameter that
// holds only what the two formats do differently (the list stands at decode_block).  MemberSink is this inflater's;
// inflate_member is the loop over a member's blocks and the checks behind the last one.
//
// Nothing here trusts the stream: compressed bytes are read inside the payload only (behind its end the reader yields
// zeros and the member ends with TRUNCATED), every write is bounded by ISIZE, every match by the bytes produced so far,
// every table index by the table's size, and every turn of every loop takes at least one bit off a stream whose bits
// are counted.  A member ends with a status word, 0 or the reason it is declined for; the host inflater then has the
// last word on the bytes (inflate.hip).
#ifndef THERMITE_INFLATE_DEVICE_H
#define THERMITE_INFLATE_DEVICE_H
#include <cstdint>

#include "bgzf_device.h"

#if defined(__HIPCC__)
#define INF_M __host__ __device__
#else
#define INF_M
#endif
#define INF_HD INF_M inline

#if defined(__HIP_DEVICE_COMPILE__)
#define INF_LANES(lane) for (uint32_t lane = threadIdx.x & 63u, once_ = 1; once_; once_ = 0)
#define INF_SYNC() __syncthreads()
#define INF_UNIFORM(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define INF_LANES(lane) for (uint32_t lane = 0; lane < 64; lane++)
#define INF_SYNC() (void)0
#define INF_UNIFORM(x) ((uint32_t)(x))
#endif

namespace thm {
namespace inf {

constexpr uint32_t LANES = 64;
constexpr uint32_t MAX_OUT = 65536;  // what a BGZF member inflates to at most
constexpr uint32_t LIT_BITS = 10, DIST_BITS = 8, CL_BITS = 7;
// first level plus sub-tables.  Canonical codes ascend with their lengths, so at most four first-level prefixes hold
// codes of mixed lengths and one is filled in part: every other sub-table has as many entries as symbols.  That bounds
// the sub-tables by 286 + 5 * 32 (30 + 5 * 128) entries; a table that still does not fit declines the member.
constexpr uint32_t LIT_ENTRIES = (1u << LIT_BITS) + 512, DIST_ENTRIES = (1u << DIST_BITS) + 768, CL_ENTRIES = 1u << CL_BITS;

// status of a member: 0, or why the device declines it
enum : uint32_t {
  OK = 0,
  TRUNCATED = 1,     // the stream runs past the payload
  BLOCK_TYPE = 2,    // block type 3
  STORED_LEN = 3,    // LEN / NLEN mismatch
  CODE_LENGTHS = 4,  // over-subscribed lengths, a repeat with nothing before it or past the end, too many symbols, no end-of-block code
  BAD_CODE = 5,      // an unassigned literal/length or distance code, symbols 286 / 287, distance codes 30 / 31
  DISTANCE = 6,      // a match that begins before the member's first byte
  OUTPUT = 7,        // more bytes than ISIZE, or fewer
  CRC = 8,
  TABLE_ROOM = 9,    // sub-tables beyond the room above
  TRAILING = 10,     // the stream ends before the payload does
  MEMBER = 11        // a table row the kernel does not take (ISIZE over MAX_OUT)
};
// what a member's decode went through (the model reports it; the tests check that every path is walked)
enum : uint32_t { P_STORED = 1, P_FIXED = 2, P_DYNAMIC = 4, P_SUBTABLE = 8, P_OVERLAP = 16, P_FAR = 32, P_MULTIBLOCK = 64 };

// ---- walk ----
struct Member {
  uint64_t in_off;   // of the raw DEFLATE stream in the members' bytes
  uint32_t in_len;
  uint32_t isize, crc;
  uint32_t pad;
  uint64_t out_off;  // of the member's bytes in the block
};
inline uint32_t le16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
inline uint32_t le32(const uint8_t* p) { return le16(p) | le16(p + 2) << 16; }
// The header rule at the first 18 bytes of a member (or fewer: `avail` of them are readable): 1f 8b 08, FLG exactly 4,
// XLEN, and -- when the whole extra field is within `avail` -- a BC subfield of SLEN 2.  0: not a BGZF header, or the
// BC subfield is not within reach; else the member's size (BSIZE + 1), *xlen set.
inline uint32_t bgzf_header(const uint8_t* p, uint64_t avail, uint32_t* xlen) {
  if (avail < 18 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || p[3] != 4) return 0;
  const uint32_t xl = le16(p + 10);
  if (12ull + xl > avail) return 0;
  for (uint32_t at = 0; at + 4 <= xl;) {
    const uint8_t* f = p + 12 + at;
    const uint32_t slen = le16(f + 2);
    if (f[0] == 'B' && f[1] == 'C' && slen == 2 && at + 6 <= xl) {
      *xlen = xl;
      return le16(f + 4) + 1;
    }
    at += 4 + slen;
  }
  return 0;
}
// member at members[at ..): false when it is not one the device takes.  *size: bytes to the next member.
inline bool walk_member(const uint8_t* members, uint64_t n, uint64_t at, uint64_t out_off, Member* m, uint64_t* size) {
  uint32_t xlen = 0;
  const uint32_t total = bgzf_header(members + at, n - at, &xlen);
  if (!total || total > n - at || total < 12 + xlen + 8 + 1) return false;  // (a DEFLATE stream has a byte at least)
  const uint8_t* trailer = members + at + total - 8;
  m->in_off = at + 12 + xlen;
  m->in_len = total - 12 - xlen - 8;
  m->crc = le32(trailer);
  m->isize = le32(trailer + 4);
  m->pad = 0;
  m->out_off = out_off;
  *size = total;
  return m->isize <= MAX_OUT;
}

// ---- length and distance bases (RFC 1951 section 3.2.5), by rule rather than by table ----
INF_HD void length_base(uint32_t k, uint32_t* base, uint32_t* extra) {  // k = symbol - 257, 0..28
  if (k < 8) *base = 3 + k, *extra = 0;
  else if (k == 28) *base = 258, *extra = 0;
  else {
    const uint32_t e = (k >> 2) - 1;
    *base = 3 + ((4 + (k & 3)) << e), *extra = e;
  }
}
INF_HD void distance_base(uint32_t s, uint32_t* base, uint32_t* extra) {  // s = 0..29
  if (s < 4) *base = 1 + s, *extra = 0;
  else {
    const uint32_t e = (s >> 1) - 1;
    *base = 1 + ((2 + (s & 1)) << e), *extra = e;
  }
}

// ---- table entries: bits 0..3 the code's length (a sub-table pointer: its index bits), 4..7 extra bits, 8..10 the
// kind, 16..31 the literal, the base or the sub-table's first entry.  0 is the unassigned code. ----
enum : uint32_t { K_NONE = 0, K_LIT = 1, K_BASE = 2, K_EOB = 3, K_SUB = 4 };
enum : uint32_t { T_CL = 0, T_LIT = 1, T_DIST = 2 };
INF_HD uint32_t entry(uint32_t kind, uint32_t len, uint32_t extra, uint32_t payload) { return len | extra << 4 | kind << 8 | payload << 16; }
INF_HD uint32_t kind_of(uint32_t e) { return (e >> 8) & 7u; }
INF_HD uint32_t make_entry(uint32_t table, uint32_t sym, uint32_t len) {
  uint32_t base, extra;
  if (table == T_CL) return entry(K_LIT, len, 0, sym);
  if (table == T_LIT) {
    if (sym < 256) return entry(K_LIT, len, 0, sym);
    if (sym == 256) return entry(K_EOB, len, 0, 0);
    if (sym > 285) return 0;
    length_base(sym - 257, &base, &extra);
    return entry(K_BASE, len, extra, base);
  }
  if (sym > 29) return 0;
  distance_base(sym, &base, &extra);
  return entry(K_BASE, len, extra, base);
}
INF_HD uint32_t bitrev(uint32_t c, uint32_t n) {
  uint32_t r = 0;
  for (uint32_t i = 0; i < n; i++) r |= ((c >> i) & 1u) << (n - 1 - i);
  return r;
}

#if defined(__HIP_DEVICE_COMPILE__)
INF_HD uint32_t fetch_add_word(uint32_t* p, uint32_t v) { return atomicAdd(p, v); }
#else
INF_HD uint32_t fetch_add_word(uint32_t* p, uint32_t v) {
  const uint32_t old = *p;
  *p += v;
  return old;
}
#endif

// everything of a member that is not its output (LDS on the device)
struct Work {
  uint32_t lit[LIT_ENTRIES], dist[DIST_ENTRIES], cl[CL_ENTRIES];
  uint32_t count[16], next[16];
  uint32_t used, bad;
  uint32_t crc_tab[256], seg_crc[LANES];
  uint16_t code[320];
  uint16_t lane_cnt[LANES][16];  // per lane and code length: symbols of the lane's run, then those of the lanes before
  uint8_t lens[320], cl_lens[20];
};

// ---- canonical table from code lengths (0 = unused): first level of `root` bits, a sub-table per first-level prefix
// with longer codes under it, sized by the longest of them.  An incomplete code leaves unassigned entries behind.
// OK, CODE_LENGTHS (over-subscribed) or TABLE_ROOM. ----
INF_HD uint32_t build_table(Work& w, const uint8_t* lens, uint32_t n_sym, uint32_t root, uint32_t* table, uint32_t max_entries,
                            uint32_t which) {
  const uint32_t primary = 1u << root;
  INF_LANES(lane) {
    if (lane < 16) w.count[lane] = 0;
    if (lane == 0) w.used = primary, w.bad = 0;
    for (uint32_t i = lane; i < primary; i += LANES) table[i] = 0;
  }
  INF_SYNC();
  INF_LANES(lane) {
    for (uint32_t s = lane; s < n_sym; s += LANES) bgz::add_word(&w.count[lens[s] & 15u], 1);
  }
  INF_SYNC();
  INF_LANES(lane) {
    if (lane == 0) {
      int32_t left = 1;
      uint32_t code = 0, bad = 0;
      w.next[0] = 0;
      for (uint32_t l = 1; l <= 15; l++) {
        left = (left << 1) - (int32_t)w.count[l];
        if (left < 0) {
          bad = 1;
          break;
        }
        code = (code + (l > 1 ? w.count[l - 1] : 0u)) << 1;
        w.next[l] = code;
      }
      w.bad = bad;
    }
  }
  INF_SYNC();
  if (INF_UNIFORM(w.bad)) return CODE_LENGTHS;
  // the code of every symbol: the first of its length plus its rank among the symbols of that length.  Every lane
  // takes a run of neighbouring symbols: its counts per length, their prefix over the lanes (a lane per length), then
  // the ranks from the lane's own row -- linear in the symbols
  const uint32_t per = (n_sym + LANES - 1) / LANES;
  INF_LANES(lane) {
    for (uint32_t l = 0; l < 16; l++) w.lane_cnt[lane][l] = 0;
    const uint32_t hi = (lane + 1) * per < n_sym ? (lane + 1) * per : n_sym;
    for (uint32_t s = lane * per; s < hi; s++) w.lane_cnt[lane][lens[s] & 15u]++;
  }
  INF_SYNC();
  INF_LANES(lane) {
    if (lane < 16) {
      uint32_t run = 0;
      for (uint32_t i = 0; i < LANES; i++) {
        const uint32_t c = w.lane_cnt[i][lane];
        w.lane_cnt[i][lane] = (uint16_t)run;
        run += c;
      }
    }
  }
  INF_SYNC();
  INF_LANES(lane) {
    const uint32_t hi = (lane + 1) * per < n_sym ? (lane + 1) * per : n_sym;
    for (uint32_t s = lane * per; s < hi; s++) {
      const uint32_t l = lens[s] & 15u;
      const uint32_t rank = w.lane_cnt[lane][l]++;
      const uint32_t c = l ? w.next[l] + rank : 0;
      w.code[s] = (uint16_t)c;
      if (l > root) bgz::max_word(&table[bitrev(c, l) & (primary - 1)], l - root);
    }
  }
  INF_SYNC();
  // sub-tables take their room in whatever order the lanes come
  INF_LANES(lane) {
    for (uint32_t pre = lane; pre < primary; pre += LANES) {
      const uint32_t sb = table[pre];
      if (!sb) continue;
      const uint32_t n = 1u << sb, off = fetch_add_word(&w.used, n);
      if (off > max_entries || n > max_entries - off) {
        w.bad = 1;
        table[pre] = 0;
        continue;
      }
      table[pre] = entry(K_SUB, sb, 0, off);
      for (uint32_t i = 0; i < n; i++) table[off + i] = 0;
    }
  }
  INF_SYNC();
  if (INF_UNIFORM(w.bad)) return TABLE_ROOM;
  INF_LANES(lane) {
    for (uint32_t s = lane; s < n_sym; s += LANES) {
      const uint32_t l = lens[s] & 15u;
      if (!l) continue;
      const uint32_t r = bitrev(w.code[s], l), e = make_entry(which, s, l);
      if (l <= root) {
        for (uint32_t i = r; i < primary; i += 1u << l) table[i] = e;
      } else {
        const uint32_t top = table[r & (primary - 1)], sb = top & 15u, off = top >> 16;
        // (the whole code's length stands in the entry: the sub-table is looked up on the unshifted buffer)
        if (kind_of(top) == K_SUB && off + (1u << sb) <= max_entries)
          for (uint32_t i = r >> root; i < (1u << sb); i += 1u << (l - root)) table[off + i] = e;
      }
    }
  }
  INF_SYNC();
  return OK;
}

// ---- bit reader over payload = base[lo, hi): `base` is 4-byte aligned, lo < 4, and the words that overlap the payload
// are readable (their bytes outside it are masked away).  The device keeps a window of 64 words in one register per
// lane and hands them out by lane index; the host reads a word at a time. ----
struct BitIn {
  const uint8_t* base;
  uint32_t lo, hi;
  uint32_t k;    // the next word
  uint64_t bb;
  uint32_t bc;
  uint32_t win, win_k;  // (device) this lane's word of the window, the window's first word
};
INF_HD uint32_t load_word(const BitIn& r, uint32_t k) {
  const uint64_t at = 4ull * k;
  if (at >= r.hi) return 0;
  uint32_t v = *(const uint32_t*)(r.base + at);
  for (uint32_t j = 0; j < 4; j++)
    if (at + j < r.lo || at + j >= r.hi) v &= ~(0xFFu << (8 * j));
  return v;
}
INF_HD uint32_t next_word(BitIn& r) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (r.k - r.win_k >= LANES) {
    r.win_k = r.k;
    r.win = load_word(r, r.k + (threadIdx.x & 63u));
  }
  const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)r.win, (int)INF_UNIFORM(r.k - r.win_k));
#else
  const uint32_t v = load_word(r, r.k);
#endif
  r.k++;
  return v;
}
// a reader over base[lo, hi) that stands nowhere yet: a seek comes next.  (win_k: no word is within 64 of it, so the
// first next_word loads the window.)
INF_HD void open_bits(BitIn& r, const uint8_t* base, uint32_t lo, uint32_t hi) {
  r.base = base, r.lo = lo, r.hi = hi, r.k = 0, r.bb = 0, r.bc = 0, r.win = 0, r.win_k = 0xFFFF0000u;
}
// at byte p of the payload
INF_HD void seek(BitIn& r, uint32_t p) {
  const uint32_t at = r.lo + p;
  r.k = at >> 2;
  const uint32_t sh = 8 * (at & 3u);
  r.bb = (uint64_t)(next_word(r) >> sh);
  r.bc = 32 - sh;
}
INF_HD void refill(BitIn& r) {  // at least 33 bits
  if (r.bc <= 32) {
    r.bb |= (uint64_t)next_word(r) << r.bc;
    r.bc += 32;
  }
}
INF_HD uint32_t take(BitIn& r, uint32_t n) {  // n <= 16
  const uint32_t v = (uint32_t)r.bb & ((1u << n) - 1u);
  r.bb >>= n;
  r.bc -= n;
  return v;
}
INF_HD uint64_t consumed(const BitIn& r) { return 32ull * r.k - r.bc - 8ull * r.lo; }

INF_HD uint32_t lookup(const uint32_t* table, uint32_t root, uint64_t bb, uint32_t* paths) {
  uint32_t e = INF_UNIFORM(table[(uint32_t)bb & ((1u << root) - 1u)]);
  if (kind_of(e) == K_SUB) {
    *paths |= P_SUBTABLE;
    e = INF_UNIFORM(table[(e >> 16) + ((uint32_t)(bb >> root) & ((1u << (e & 15u)) - 1u))]);
  }
  return e;
}

// ---- CRC-32 of out[0, n): a segment of whole words per lane, an odd number of them so that the lanes' reads fall on
// different banks; every segment's CRC is moved to the end of the data (x^(8 * bytes behind it)) and the lot is summed ----
INF_HD void fill_crc_table(uint32_t* tab, uint32_t lane) {  // this lane's share of the 256 entries
  for (uint32_t t = lane; t < 256; t += LANES) tab[t] = bgz::crc_table_entry(t);
}
INF_HD uint32_t fold_seg_crc(const uint32_t* seg_crc) {  // the lanes' pieces, each already moved to the end of the data
  uint32_t c = 0;
  for (uint32_t i = 0; i < LANES; i++) c ^= seg_crc[i];
  return c;
}
INF_HD uint32_t crc_of_output(Work& w, const uint32_t* outw, uint32_t n) {
  INF_SYNC();
  INF_LANES(lane) { fill_crc_table(w.crc_tab, lane); }
  INF_SYNC();
  const uint32_t seg = 4 * ((((n + 3) / 4 + LANES - 1) / LANES) | 1u);
  INF_LANES(lane) {
    const uint32_t lo = lane * seg, hi = lo + seg < n ? lo + seg : n;
    uint32_t c = 0;
    if (lo < n) {
      c = 0xFFFFFFFFu;
      for (uint32_t i = lo; i < hi; i += 4) {
        const uint32_t v = outw[i >> 2];
        for (uint32_t j = 0; j < 4 && i + j < hi; j++) c = w.crc_tab[(c ^ (v >> (8 * j))) & 0xFF] ^ (c >> 8);
      }
      c = bgz::crc_mul(bgz::crc_xpow8(n - hi), ~c);
    }
    w.seg_crc[lane] = c;
  }
  INF_SYNC();
  return INF_UNIFORM(fold_seg_crc(w.seg_crc));
}

// ---- one DEFLATE block, for both inflaters: this one's members and the runs of plain gzip (gzip_device.h) ----
// The header of a dynamic block behind its three first bits: the lengths of both codes into w.lens, *hlit and *hdist
// their counts.  OK, TRUNCATED or CODE_LENGTHS.
INF_HD uint32_t read_dynamic_header(BitIn& r, Work& w, uint64_t total_bits, uint32_t* hlit_out, uint32_t* hdist_out) {
  refill(r);
  const uint32_t hlit = take(r, 5) + 257, hdist = take(r, 5) + 1, hclen = take(r, 4) + 4;
  if (hlit > 286 || hdist > 30) return CODE_LENGTHS;
  INF_SYNC();
  INF_LANES(lane) {
    if (lane < 20) w.cl_lens[lane] = 0;
  }
  INF_SYNC();
  for (uint32_t i = 0; i < hclen; i++) {
    refill(r);
    w.cl_lens[bgz::cl_order(i)] = (uint8_t)take(r, 3);  // (every lane stores the same value)
  }
  if (consumed(r) > total_bits) return TRUNCATED;
  INF_SYNC();
  if (build_table(w, w.cl_lens, 19, CL_BITS, w.cl, CL_ENTRIES, T_CL) != OK) return CODE_LENGTHS;
  uint32_t n = 0, prev = 0;
  while (n < hlit + hdist) {  // each turn takes a bit at least
    refill(r);
    if (consumed(r) > total_bits) return TRUNCATED;
    const uint32_t e = INF_UNIFORM(w.cl[(uint32_t)r.bb & (CL_ENTRIES - 1)]);
    if (kind_of(e) != K_LIT) return CODE_LENGTHS;
    take(r, e & 15u);
    const uint32_t sym = e >> 16;
    if (sym < 16) {
      w.lens[n++] = (uint8_t)sym;
      prev = sym;
      continue;
    }
    uint32_t rep, val = 0;
    if (sym == 16) {
      if (n == 0) return CODE_LENGTHS;
      val = prev;
      rep = 3 + take(r, 2);
    } else if (sym == 17) {
      rep = 3 + take(r, 3);
    } else {
      rep = 11 + take(r, 7);
    }
    if (rep > hlit + hdist - n) return CODE_LENGTHS;
    INF_LANES(lane) {
      for (uint32_t i = lane; i < rep; i += LANES) w.lens[n + i] = (uint8_t)val;
    }
    n += rep;
    prev = val;
  }
  if (consumed(r) > total_bits) return TRUNCATED;
  INF_SYNC();
  if (INF_UNIFORM(w.lens[256]) == 0) return CODE_LENGTHS;
  *hlit_out = hlit, *hdist_out = hdist;
  return OK;
}
// the lengths of the fixed codes into w.lens: 288 literal/length symbols, then 32 distance symbols
INF_HD void fixed_lengths(Work& w) {
  INF_SYNC();
  INF_LANES(lane) {
    for (uint32_t s = lane; s < 320; s += LANES) w.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
  }
}

// The block at the reader's position, its bytes handed to `s`.  OK (*last: the block was final) or why not; *paths
// gains the P_ bits of what the block went through.  A sink is where the two formats differ and nothing else:
//   pos                  bytes it holds so far (wave-uniform, as the reader's state is)
//   room()               bytes it still takes; FULL the status of a block that brings more
//   before_symbol()      a turn of the symbol loop begins
//   literal(b)           one byte                          } room() has been checked,
//   stored(src, len)     len bytes from the input          } pos moves on
//   match(len, dist)     len bytes from dist bytes back    }
//   distance(dist)       OK, or the status of a match that begins before what it may reach
//   DIST_CODE_AT_END     the status of an unassigned distance code whose first bit is past the input's end
template <class Sink>
INF_HD uint32_t decode_block(BitIn& r, Work& w, uint64_t total_bits, Sink& s, uint32_t* last, uint32_t* paths) {
  refill(r);
  *last = take(r, 1);
  const uint32_t type = take(r, 2);
  if (consumed(r) > total_bits) return TRUNCATED;
  if (type == 3) return BLOCK_TYPE;
  if (type == 0) {
    take(r, r.bc & 7u);
    refill(r);
    const uint32_t len = take(r, 16);
    refill(r);
    const uint32_t nlen = take(r, 16);
    if (consumed(r) > total_bits) return TRUNCATED;
    if ((len ^ 0xFFFFu) != nlen) return STORED_LEN;
    const uint32_t p = (uint32_t)(consumed(r) >> 3);
    if (len > r.hi - r.lo - p) return TRUNCATED;
    if (len > s.room()) return Sink::FULL;
    s.stored(r.base + r.lo + p, len);
    seek(r, p + len);
    *paths |= P_STORED;
    return OK;
  }
  uint32_t hlit, hdist;
  if (type == 1) {
    hlit = 288, hdist = 32;
    fixed_lengths(w);
    *paths |= P_FIXED;
  } else {
    const uint32_t status = read_dynamic_header(r, w, total_bits, &hlit, &hdist);
    if (status != OK) return status;
    *paths |= P_DYNAMIC;
  }
  INF_SYNC();
  uint32_t status = build_table(w, w.lens, hlit, LIT_BITS, w.lit, LIT_ENTRIES, T_LIT);
  if (status == OK) status = build_table(w, w.lens + hlit, hdist, DIST_BITS, w.dist, DIST_ENTRIES, T_DIST);
  if (status != OK) return status;
  // symbols: each turn takes a bit at least, and a symbol counts only when all its bits were the input's
  for (;;) {
    s.before_symbol();
    refill(r);
    const uint32_t e = lookup(w.lit, LIT_BITS, r.bb, paths), kind = kind_of(e);
    if (kind != K_BASE) {  // (lengths are told apart first: their turn does not pay for the check below)
      if (kind != K_LIT && kind != K_EOB) return consumed(r) + 1 > total_bits ? TRUNCATED : BAD_CODE;
      // A literal or the end-of-block code: all its bits must be the input's, in both formats.  A member would come to
      // the same word without the check on the end-of-block code: one past the payload's end leaves consumed(r) past
      // it for good, so the next block's three bits, or inflate_member's epilogue behind a final block, end the
      // member TRUNCATED before anything else is written or judged.  A run needs it: decode_run takes a block that
      // ended with OK as a boundary it may stop at or roll back to.
      take(r, e & 15u);
      if (consumed(r) > total_bits) return TRUNCATED;
      if (kind == K_EOB) return OK;
      if (!s.room()) return Sink::FULL;
      s.literal(e >> 16);
      continue;
    }
    take(r, e & 15u);
    const uint32_t len = (e >> 16) + take(r, (e >> 4) & 15u);
    refill(r);
    const uint32_t d = lookup(w.dist, DIST_BITS, r.bb, paths);
    if (kind_of(d) != K_BASE) return consumed(r) + 1 > total_bits ? Sink::DIST_CODE_AT_END : BAD_CODE;
    take(r, d & 15u);
    const uint32_t dist = (d >> 16) + take(r, (d >> 4) & 15u);
    if (consumed(r) > total_bits) return TRUNCATED;
    status = s.distance(dist);
    if (status != OK) return status;
    if (len > s.room()) return Sink::FULL;
    if (dist < len) *paths |= P_OVERLAP;
    if (dist > 16384) *paths |= P_FAR;
    s.match(len, dist);
  }
  // (not reached: every way out of the loop is a return above; no block ends without the check on its last bits)
  return consumed(r) > total_bits ? TRUNCATED : OK;
}

// a member's bytes: out[0, isize) in one flat buffer
struct MemberSink {
  static constexpr uint32_t FULL = OUTPUT, DIST_CODE_AT_END = BAD_CODE;
  uint8_t* out;
  uint32_t isize, pos;
  INF_M uint32_t room() const { return isize - pos; }
  INF_M void before_symbol() {}
  INF_M void literal(uint32_t b) { out[pos++] = (uint8_t)b; }  // (every lane stores the same value)
  INF_M void stored(const uint8_t* src, uint32_t len) {
    INF_LANES(lane) {
      for (uint32_t i = lane; i < len; i += LANES) out[pos + i] = src[i];
    }
    pos += len;
  }
  INF_M uint32_t distance(uint32_t dist) const { return dist > pos ? (uint32_t)DISTANCE : (uint32_t)OK; }
  INF_M void match(uint32_t len, uint32_t dist) {
    // sources lie before `pos` whatever the distance: the lanes need no order among themselves
    INF_SYNC();
    INF_LANES(lane) {
      const uint8_t* src = out + pos - dist;
      for (uint32_t i = lane; i < len; i += LANES) out[pos + i] = src[dist >= len ? i : dist == 1 ? 0 : i % dist];
    }
    pos += len;
  }
};

struct Result {
  uint32_t status, paths;
};

// The raw DEFLATE stream base[lo, hi) -> outw (MAX_OUT bytes and a word of slack), which must come to exactly `isize`
// bytes with CRC-32 `crc`.
INF_HD Result inflate_member(const uint8_t* base, uint32_t lo, uint32_t hi, uint32_t isize, uint32_t crc, uint32_t* outw, Work& w) {
  Result res = {OK, 0};
  if (isize > MAX_OUT || hi < lo) {
    res.status = MEMBER;
    return res;
  }
  BitIn r;
  open_bits(r, base, lo, hi);
  seek(r, 0);
  const uint64_t total_bits = 8ull * (hi - lo);
  MemberSink out = {(uint8_t*)outw, isize, 0};
  uint32_t paths = 0, last = 0, status = OK;
  for (uint32_t n_blocks = 0; status == OK && !last; n_blocks++) {  // each takes 3 bits at least
    // (a further block counts once its three first bits were the payload's)
    if (n_blocks && consumed(r) + 3 <= total_bits) paths |= P_MULTIBLOCK;
    status = decode_block(r, w, total_bits, out, &last, &paths);
  }
  if (status == OK && consumed(r) > total_bits) status = TRUNCATED;
  if (status == OK && (consumed(r) + 7) / 8 != hi - lo) status = TRAILING;
  if (status == OK && out.pos != isize) status = OUTPUT;
  if (status == OK && crc_of_output(w, outw, isize) != crc) status = CRC;
  res.status = status;
  res.paths = paths;
  return res;
}

// ---- out[0, n) to dst, which has any alignment: bytes up to the first 16-byte boundary and behind the last, 16-byte
// stores between them (the words come out of `outw` shifted into place) ----
struct alignas(16) Quad {
  uint32_t v[4];
};
INF_HD void copy_out(uint8_t* dst, const uint32_t* outw, uint32_t n, uint32_t lane) {
  const uint8_t* out = (const uint8_t*)outw;
  uint32_t head = (uint32_t)((16u - ((uintptr_t)dst & 15u)) & 15u);
  if (head > n) head = n;
  for (uint32_t i = lane; i < head; i += LANES) dst[i] = out[i];
  const uint32_t n16 = (n - head) / 16, sh = 8 * (head & 3u), w0 = head >> 2;
  for (uint32_t c = lane; c < n16; c += LANES) {
    Quad q;
    for (uint32_t j = 0; j < 4; j++) {
      const uint32_t a = outw[w0 + 4 * c + j];
      q.v[j] = sh ? a >> sh | outw[w0 + 4 * c + j + 1] << (32 - sh) : a;  // (the word of slack behind MAX_OUT)
    }
    *(Quad*)(dst + head + 16 * c) = q;
  }
  for (uint32_t i = head + 16 * n16 + lane; i < n; i += LANES) dst[i] = out[i];
}

}  // namespace inf
}  // namespace thm
#endif
