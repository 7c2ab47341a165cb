// gzip_device.h -- the rules of the device inflater for plain gzip (kernels_gzip.hip; host side gzip.hip; DESIGN.md
// section 4.14), as functions that compile for the host too: tests/cpp/gzip_model_main.cpp runs the same text serially
// (that file gives the build lines), corrupt streams first of all and under the sanitizers, before a byte of it reaches a
// device.  Bit reader, table build, look-up, the length and distance rules, the decoder of one block (inf::decode_block,
// with the header reader the search uses too) and the CRC arithmetic are those of inflate_device.h / bgzf_device.h;
// what a run does differently with a block's bytes is RingSink below.
//
// An ordinary gzip member is one long DEFLATE stream whose matches reach 32 KiB back across any cut.  The scheme is the
// host inflater's (io_inflate.cpp, "several threads on one gzip file"), one wavefront where that has a thread:
//   search   per chunk of chunk_bytes compressed bytes: the first bit at which a non-final dynamic block's header stands
//            -- 64 bit offsets a step through a lane-private prefilter, survivors one at a time through the header reader
//            with the whole wave.  Chunk 0 starts where the caller's state says and searches nothing.
//   decode   per run (a chunk with a start and the start-less chunks behind it), from its start to the next run's start,
//            into 16-bit symbols: < 256 a byte, 0x8000 | k byte k of the 32 KiB before the run.  The last 32 Ki symbols
//            live in a ring (LDS on the device) that begins as the markers themselves, so that a match source is one ring
//            read wherever it lies; the symbols go to the run's region of global memory FLUSH at a time.
//   chain    in stream order: every run ends exactly on the next one's start, or the whole inflate is declined -- by
//            induction from the known start of chunk 0 every start is then a true one, whatever the search let through;
//            reach of every run into its window against the member's bytes before it; prefix sum of the symbol counts;
//            every run's window from its predecessor's, 32 Ki independent look-ups a step.
//   resolve  every symbol of every run to its byte in the block, CRC-32 pieces per tile folded into their members
//   verify   member CRCs and ISIZEs against the trailers and the incoming state; the outgoing state.
// Lane-parallel phases follow inflate_device.h (INF_LANES / INF_SYNC / INF_UNIFORM); phases of a whole workgroup are
// written GZ_EACH(t, n) { ... }, every t below n once, with GZ_SYNC() between phases.
//
// Nothing here trusts the stream, and the search reads arbitrary bit positions of arbitrary bytes: compressed bytes are
// read inside in[0, n) only (whole words, bytes outside masked away), symbol writes are bounded by the run's region,
// ring indices by the ring, table indices by their tables, member ends by the run's slots, and every turn of every loop
// takes at least one bit off a stream whose bits are counted.  A run ends with a status word, the inflate with one; any
// word other than 0 hands the same bytes to the host inflater, which has the last word (gzip.hip).
#ifndef THERMITE_GZIP_DEVICE_H
#define THERMITE_GZIP_DEVICE_H
#include <cstdint>

#include "inflate_device.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define GZ_EACH(t, n) for (uint32_t t = threadIdx.x; t < (n); t += blockDim.x)
#define GZ_SYNC() __syncthreads()
#else
#define GZ_EACH(t, n) for (uint32_t t = 0; t < (n); t++)
#define GZ_SYNC() (void)0
#endif

namespace thm {
namespace gz {

using namespace inf;

constexpr uint32_t WINDOW = 32768, RING_MASK = WINDOW - 1;
constexpr uint32_t DEFAULT_CHUNK = 32768, MIN_CHUNK = 64;
// A chunk's region holds RATIO symbols per compressed byte and a run's region is the regions of its chunks: a run whose
// blocks inflate beyond that is declined (REGION).  A run of one chunk may begin at the chunk's first bit and end at the
// next chunk's last, so the ratio that is always taken is RATIO / 2.
constexpr uint32_t RATIO = 16;
constexpr uint32_t ENDS_PER_CHUNK = 4;  // member ends a run records per chunk of its own; more declines (MEMBER_CAP)
constexpr uint32_t FLUSH = 4096;        // symbols that wait in the ring before they go to global memory
constexpr uint32_t TILE = 4096;         // output bytes per wavefront of the resolve step
constexpr uint64_t MAX_IN = 64ull << 20;  // compressed bytes one inflate takes (32 x as many bytes of symbol regions)
constexpr uint64_t NONE = ~0ull;
constexpr uint32_t BEFORE = 0xFFFFFFFFu;  // Run::member_start: the member in progress began before the run

// status words beyond those of inflate_device.h
enum : uint32_t {
  NO_MEET = 12,     // a run does not end on the next run's start
  REACH = 13,       // a match reaches further back than the member's bytes before the run
  REGION = 14,      // a run's output over its region, or the block's over the buffer's room
  MEMBER_CAP = 15,  // more member ends in a run than its chunks have slots
  HEADER = 16,      // a member header the device does not take (method, reserved flags, no magic where one must be)
  ISIZE = 17,
  INPUT = 18        // more than MAX_IN bytes, or a state that is not one
};
// what an inflate went through (the model reports it; the tests check that every path is walked)
enum : uint32_t {
  G_MARKER = 1,        // a match source in the window before the run
  G_MARKER_COPY = 2,   // a marker copied from the run's own output
  G_MERGED = 4,        // a start-less chunk merged into a run
  G_WIN_IN_WIN = 8,    // a window that begins inside the predecessor's window
  G_MEMBER_END = 16,   // a member end inside a run
  G_ROLLBACK = 32,     // the last run rolled back to the last block that ended inside the bytes
  G_REACH = 64         // a reach checked against the member's bytes
};

// thm_gzip_state (include/thermite_io.h), field for field
struct State {
  uint8_t window[WINDOW];
  uint32_t window_len, bit_offset, in_member, crc;
  uint64_t member_len, n_members_done, stream_offset;
};

// a state is one: a bit offset only inside a member, and there a window of all the member's bytes that fit one
INF_HD bool state_consistent(const State& st) {
  return st.bit_offset <= 7 && st.window_len <= WINDOW && (st.in_member || st.bit_offset == 0) &&
         (!st.in_member || st.window_len == (st.member_len < WINDOW ? st.member_len : WINDOW));
}

struct Run {
  uint64_t start_bit, end_bit;
  uint64_t sym_off;       // (chain) of the run's first byte in the inflated bytes
  uint32_t status, n_sym;
  uint32_t reach;         // deepest reach into the window before the run, by the member that was in progress at its start
  uint32_t n_ends;
  uint32_t member_start;  // symbol count at which the member in progress at the end began; BEFORE
  uint32_t in_member;     // at end_bit: 1 at a block start inside a member, 0 at a member boundary
  uint32_t at_end;        // 1: the bytes ended at a member boundary; 2: what follows the last member is no member
  uint32_t flags, paths, n_chunks, pad;
  uint64_t header_from;   // the run ends behind a member header, before the member's first block: the header's first bit; NONE
};
struct End {
  uint32_t pos, crc, isize, pad;
};
struct Summary {
  uint32_t status, bad_chunk;
  uint64_t n_out, n_consumed;
  uint32_t n_starts, n_refused, n_ends, flags, paths, bit_offset, in_member, pad;
};

// one inflate: every array lives in global memory
struct Job {
  const uint8_t* in;   // [n], 4-byte aligned, readable up to the next multiple of 4
  uint64_t n;
  uint32_t chunk_bytes, n_chunks, last_block, pad;
  const State* st_in;
  State* st_out;
  uint64_t* cand;      // [n_chunks]
  Run* runs;           // [n_chunks]
  End* ends;           // [n_chunks * ENDS_PER_CHUNK]
  uint16_t* syms;      // [n_chunks * chunk_bytes * RATIO]
  uint8_t* windows;    // [n_chunks * WINDOW]
  uint32_t* run_list;  // [n_chunks]        (chain) the chunks with a start, in order
  uint64_t* run_off;   // [n_chunks + 1]    (chain) sym_off of run_list[r]; n_out behind the last
  uint64_t* end_abs;   // [n_chunks * ENDS_PER_CHUNK] (chain) member ends in the inflated bytes
  uint32_t* end_crc;   // ... their stored CRC-32
  uint32_t* end_isize;
  uint32_t* member_crc;  // [n_chunks * ENDS_PER_CHUNK + 1] (resolve) CRC-32 of what this inflate adds to every member; zeroed
  uint8_t* out;        // [out_cap]
  uint64_t out_cap;
  Summary* sum;
};
INF_HD uint64_t region_syms(const Job& j) { return (uint64_t)j.chunk_bytes * RATIO; }

#if defined(__HIP_DEVICE_COMPILE__)
INF_HD uint64_t ballot_bit(bool p, uint32_t lane) { return __ballot(p); }
INF_HD void xor_word(uint32_t* p, uint32_t v) { atomicXor(p, v); }
#else
INF_HD uint64_t ballot_bit(bool p, uint32_t lane) { return (uint64_t)p << lane; }
INF_HD void xor_word(uint32_t* p, uint32_t v) { *p ^= v; }
#endif

INF_HD uint64_t uniform64(uint64_t v) { return (uint64_t)INF_UNIFORM((uint32_t)v) | (uint64_t)INF_UNIFORM((uint32_t)(v >> 32)) << 32; }

// ---- compressed bytes, wherever a bit offset points: inside in[0, n) or zeros ----
INF_HD uint32_t word_at(const uint8_t* in, uint64_t n, uint64_t k) {
  const uint64_t at = 4 * k;
  if (at >= n) return 0;
  uint32_t v = *(const uint32_t*)(in + at);
  if (n - at < 4) v &= (1u << (8 * (uint32_t)(n - at))) - 1u;
  return v;
}
INF_HD uint32_t byte_at(const uint8_t* in, uint64_t n, uint64_t p) { return p < n ? in[p] : 0u; }
INF_HD uint32_t le32_at(const uint8_t* in, uint64_t n, uint64_t p) {
  return byte_at(in, n, p) | byte_at(in, n, p + 1) << 8 | byte_at(in, n, p + 2) << 16 | byte_at(in, n, p + 3) << 24;
}
INF_HD uint64_t peek64(const uint8_t* in, uint64_t n, uint64_t bit) {
  const uint64_t k = bit >> 5;
  const uint32_t sh = (uint32_t)bit & 31u;
  const uint64_t lo = (uint64_t)word_at(in, n, k) | (uint64_t)word_at(in, n, k + 1) << 32;
  const uint64_t hi = word_at(in, n, k + 2);
  return sh ? lo >> sh | hi << (64 - sh) : lo;
}

// ---- search ----
// lane-private: BFINAL 0, BTYPE 2, HLIT <= 29, HDIST <= 29, the code-length code complete, all of it inside the bytes
INF_HD bool prefilter(const uint8_t* in, uint64_t n, uint64_t bit) {
  const uint64_t v = peek64(in, n, bit);
  if ((v & 7u) != 4u) return false;
  if (((v >> 3) & 31u) > 29u || ((v >> 8) & 31u) > 29u) return false;
  const uint32_t hclen = (uint32_t)((v >> 13) & 15u) + 4;
  if (bit + 17 + 3 * hclen > 8 * n) return false;
  const uint64_t c = peek64(in, n, bit + 17);
  uint32_t kraft = 0;
  for (uint32_t i = 0; i < hclen; i++) {
    const uint32_t l = (uint32_t)(c >> (3 * i)) & 7u;
    if (l) kraft += 128u >> l;
  }
  return kraft == 128u;
}

INF_HD void open_bits(BitIn& r, const uint8_t* in, uint64_t n, uint64_t bit) {
  inf::open_bits(r, in, 0, (uint32_t)n);
  seek(r, (uint32_t)(bit >> 3));
  take(r, (uint32_t)bit & 7u);
}

// Kraft sum of n code lengths in units of 2^-15, and how many are in use
INF_HD uint32_t kraft_sum(const uint8_t* lens, uint32_t n, uint32_t* used) {
  uint32_t sum = 0, u = 0;
  for (uint32_t s = 0; s < n; s++) {
    const uint32_t l = INF_UNIFORM(lens[s]) & 15u;
    if (l) sum += 32768u >> l, u++;
  }
  *used = u;
  return sum;
}

// chunk k's first candidate bit into cand[k] (NONE: none).  The candidate rule: the prefilter, then a header the reader
// takes whose literal/length code is complete and whose distance code is complete or has at most one code.
INF_HD void search_chunk(const Job& j, uint32_t k, Work& w) {
  uint64_t found = NONE;
  if (k == 0) {
    found = j.st_in->bit_offset & 7u;
  } else {
    const uint64_t lo = 8ull * k * j.chunk_bytes, total = 8 * j.n;
    const uint64_t hi = lo + 8ull * j.chunk_bytes < total ? lo + 8ull * j.chunk_bytes : total;
    for (uint64_t base = lo; base < hi && found == NONE; base += LANES) {
      uint64_t mask = 0;
      INF_LANES(lane) {
        const uint64_t bit = base + lane;
        mask |= ballot_bit(bit < hi && prefilter(j.in, j.n, bit), lane);
      }
      mask = uniform64(mask);
      while (mask && found == NONE) {
        const uint64_t bit = base + (uint32_t)__builtin_ctzll(mask);
        mask &= mask - 1;
        BitIn r;
        open_bits(r, j.in, j.n, bit);
        refill(r);
        take(r, 3);
        uint32_t hlit = 0, hdist = 0, used = 0;
        if (read_dynamic_header(r, w, total, &hlit, &hdist) != OK) continue;
        if (kraft_sum(w.lens, hlit, &used) != 32768u) continue;
        const uint32_t kd = kraft_sum(w.lens + hlit, hdist, &used);
        if (kd != 32768u && used > 1) continue;
        found = bit;
      }
    }
  }
  INF_LANES(lane) {
    if (lane == 0) j.cand[k] = found;
  }
}

// ---- decode ----
struct RunWork {
  Work w;
  uint16_t ring[WINDOW];
  uint32_t flags;
};

// A run's symbols, the sink of inf::decode_block: ring[pos & RING_MASK] first, the run's region FLUSH at a time.
struct RingSink {
  static constexpr uint32_t FULL = REGION, DIST_CODE_AT_END = TRUNCATED;
  RunWork& L;
  uint16_t* sym;  // the run's region
  uint32_t region;
  uint32_t member_start;  // as Run's
  uint32_t pos, flushed;
  uint32_t reach;  // as Run's
  INF_M uint32_t room() const { return region - pos; }
  INF_M void flush() {  // ring[flushed, pos) to the region
    INF_SYNC();
    INF_LANES(lane) {
      for (uint32_t i = flushed + lane; i < pos; i += LANES) sym[i] = L.ring[i & RING_MASK];
    }
    INF_SYNC();
    flushed = pos;
  }
  INF_M void before_symbol() {
    if (pos - flushed >= FLUSH) flush();
  }
  INF_M void literal(uint32_t b) { L.ring[pos++ & RING_MASK] = (uint16_t)b; }  // (every lane stores the same value)
  INF_M void stored(const uint8_t* src, uint32_t len) {
    for (uint32_t done = 0; done < len;) {  // (pieces that the ring holds unflushed)
      const uint32_t piece = len - done < FLUSH ? len - done : FLUSH;
      INF_SYNC();
      INF_LANES(lane) {
        for (uint32_t i = lane; i < piece; i += LANES) L.ring[(pos + i) & RING_MASK] = (uint16_t)src[done + i];
      }
      pos += piece, done += piece;
      flush();
    }
  }
  INF_M uint32_t distance(uint32_t dist) {
    if (member_start != BEFORE) return dist > pos - member_start ? (uint32_t)DISTANCE : (uint32_t)OK;
    if (dist > pos) {  // into the window before the run: the chain judges how far is too far
      if (dist - pos > reach) reach = dist - pos;
      bgz::or_word(&L.flags, G_MARKER);
    }
    return OK;
  }
  INF_M void match(uint32_t len, uint32_t dist) {
    // sources lie before `pos` whatever the distance, 64 symbols a step: within a step every source is read before
    // a destination of that step is written, which matters where the ring's slots of both coincide
    INF_SYNC();
    for (uint32_t base = 0; base < len; base += LANES) {
      INF_LANES(lane) {
        const uint32_t i = base + lane;
        if (i < len) {
          const uint32_t o = dist >= len ? i : dist == 1 ? 0 : i % dist;
          const uint16_t s = L.ring[(pos - dist + o) & RING_MASK];
          if ((s & 0x8000u) && dist <= pos + o) bgz::or_word(&L.flags, G_MARKER_COPY);
          L.ring[(pos + i) & RING_MASK] = s;
        }
      }
    }
    pos += len;
  }
};

// the run that begins in chunk k, if one does
INF_HD void decode_run(const Job& j, uint32_t k, RunWork& L) {
  const uint64_t start = j.cand[k];
  if (start == NONE) return;
  uint32_t nxt = k + 1;
  while (nxt < j.n_chunks && j.cand[nxt] == NONE) nxt++;
  const bool last_run = nxt == j.n_chunks;
  const uint64_t total_bits = 8 * j.n, target = last_run ? total_bits : j.cand[nxt];
  const uint64_t room = (uint64_t)(nxt - k) * region_syms(j);
  const uint32_t region = room < 0xFFFF0000ull ? (uint32_t)room : 0xFFFF0000u;
  const uint32_t max_ends = (nxt - k) * ENDS_PER_CHUNK;
  uint16_t* const sym = j.syms + (uint64_t)k * region_syms(j);
  End* const ends = j.ends + (uint64_t)k * ENDS_PER_CHUNK;
  INF_LANES(lane) {
    for (uint32_t i = lane; i < WINDOW; i += LANES) L.ring[i] = (uint16_t)(0x8000u | i);
    if (lane == 0) L.flags = nxt - k > 1 ? (uint32_t)G_MERGED : 0u;
  }
  INF_SYNC();
  struct Mark {
    uint64_t bit;
    uint32_t pos, reach, n_ends, member_start, in_member;
  };
  uint32_t in_member = k == 0 ? (j.st_in->in_member != 0) : 1u;
  uint32_t n_ends = 0, paths = 0, status = OK, at_end = 0, rolled = 0;
  RingSink out = {L, sym, region, BEFORE, 0, 0, 0};
  uint64_t p = start >> 3;  // the byte position while between members
  BitIn r;
  open_bits(r, j.in, j.n, in_member ? start : 0);
  Mark ck = {start, 0, 0, 0, BEFORE, in_member};
  uint64_t end_bit = start, header_from = NONE;
  const bool first_ever = k == 0 && !in_member && j.st_in->n_members_done == 0;
  for (;;) {  // each turn takes a block, a member header with its block, or ends the run
    bool fresh = false;
    if (!in_member) {
      end_bit = 8 * p;
      ck = Mark{end_bit, out.pos, out.reach, n_ends, out.member_start, 0};
      if (!last_run && end_bit >= target) break;
      if (p >= j.n) {
        at_end = 1;
        break;
      }
      if (j.n - p < 10) {
        status = TRUNCATED;
        break;
      }
      if (byte_at(j.in, j.n, p) != 0x1f || byte_at(j.in, j.n, p + 1) != 0x8b) {
        if (first_ever && n_ends == 0) status = HEADER;
        else at_end = 2, end_bit = total_bits;
        break;
      }
      const uint32_t flg = byte_at(j.in, j.n, p + 3);
      if (byte_at(j.in, j.n, p + 2) != 8 || (flg & 0xE0u)) {
        status = HEADER;
        break;
      }
      uint64_t q = p + 10;
      if (flg & 4u) {  // FEXTRA
        if (q + 2 > j.n) status = TRUNCATED;
        else {
          q += 2 + (byte_at(j.in, j.n, q) | byte_at(j.in, j.n, q + 1) << 8);
          if (q > j.n) status = TRUNCATED;
        }
      }
      for (uint32_t f = 8; f <= 16 && status == OK; f <<= 1)  // FNAME, FCOMMENT: zero-terminated
        if (flg & f)
          for (;;) {  // (each turn takes a byte)
            if (q >= j.n) {
              status = TRUNCATED;
              break;
            }
            if (byte_at(j.in, j.n, q++) == 0) break;
          }
      if (status == OK && (flg & 2u)) {  // FHCRC
        q += 2;
        if (q > j.n) status = TRUNCATED;
      }
      if (status != OK) break;
      out.member_start = out.pos;
      in_member = 1;
      header_from = 8 * p;
      fresh = true;  // (the header counts only together with the member's first block)
      seek(r, (uint32_t)q);
    }
    end_bit = consumed(r);
    if (!fresh) ck = Mark{end_bit, out.pos, out.reach, n_ends, out.member_start, 1};
    if (!last_run && end_bit >= target) break;
    uint32_t last = 0;
    // (`paths` also keeps the bit of a dynamic block whose tables then fail to build.  That ends the run with a status
    // other than OK -- not TRUNCATED: the header was inside the input -- and the chain takes no paths from such a run.)
    status = decode_block(r, L.w, total_bits, out, &last, &paths);
    // (a verdict reached on bits behind the input's end is a verdict on zeros: the stream is cut off, whatever it says)
    if (status != OK && consumed(r) > total_bits) status = TRUNCATED;
    if (status != OK) break;
    header_from = NONE;
    if (last) {  // the trailer
      take(r, r.bc & 7u);
      p = consumed(r) >> 3;
      if (p + 8 > j.n) {
        status = TRUNCATED;
        break;
      }
      if (n_ends >= max_ends) {
        status = MEMBER_CAP;
        break;
      }
      const uint32_t crc = le32_at(j.in, j.n, p), isize = le32_at(j.in, j.n, p + 4);
      INF_LANES(lane) {
        if (lane == 0) ends[n_ends] = End{out.pos, crc, isize, 0};
      }
      n_ends++;
      p += 8;
      in_member = 0;
      out.member_start = BEFORE;  // (set again by the next header)
    }
  }
  // the last run of bytes that are not the input's last: what the bytes cut off is not an error, the run ends with the
  // last block that ended inside them
  if (status == TRUNCATED && last_run && !j.last_block) {
    status = OK, rolled = 1, header_from = NONE;
    end_bit = ck.bit, out.pos = ck.pos, out.reach = ck.reach, n_ends = ck.n_ends, out.member_start = ck.member_start, in_member = ck.in_member;
  }
  if (out.flushed > out.pos) out.flushed = out.pos;
  out.flush();
  INF_LANES(lane) {
    if (lane == 0) {
      Run& R = j.runs[k];
      R.start_bit = start, R.end_bit = end_bit, R.sym_off = 0;
      R.status = status, R.n_sym = out.pos, R.reach = out.reach, R.n_ends = n_ends;
      R.member_start = out.member_start, R.in_member = in_member, R.at_end = at_end;
      R.flags = L.flags | (n_ends ? (uint32_t)G_MEMBER_END : 0u) | (rolled ? (uint32_t)G_ROLLBACK : 0u);
      R.paths = paths, R.n_chunks = nxt - k, R.pad = 0;
      R.header_from = status == OK && in_member ? header_from : NONE;
    }
  }
}

// ---- chain ----
// One thread: runs against their neighbours and against the members, offsets, member ends, the summary.
INF_HD void chain_serial(const Job& j) {
  Summary s = {};
  const State& st = *j.st_in;
  uint64_t expect = st.bit_offset & 7u, off = 0, member_before = st.in_member ? st.member_len : 0;
  uint64_t header_from = NONE;  // of the run before
  uint32_t n_runs = 0, n_ends = 0, prev = BEFORE;
  auto decline = [&](uint32_t why, uint32_t k) {
    if (s.status == OK) s.status = why, s.bad_chunk = k;
  };
  if (j.n > MAX_IN || !state_consistent(st)) decline(INPUT, 0);
  for (uint32_t k = 0; k < j.n_chunks && s.status != INPUT; k++) {
    if (j.cand[k] == NONE) continue;
    const Run R = j.runs[k];
    if (R.start_bit != expect) {
      s.n_refused++;
      decline(NO_MEET, k);
    }
    if (R.status != OK) decline(R.status, k);
    if (R.reach) {
      s.flags |= G_REACH;
      if (R.reach > (member_before < WINDOW ? member_before : WINDOW)) decline(REACH, k);
    }
    if (R.n_ends > R.n_chunks * ENDS_PER_CHUNK) decline(MEMBER_CAP, k);
    if (s.status != OK) {  // (what follows a run that is not trusted is only counted)
      expect = R.end_bit;
      n_runs++;
      continue;
    }
    j.runs[k].sym_off = off;
    j.run_list[n_runs] = k;
    j.run_off[n_runs] = off;
    for (uint32_t e = 0; e < R.n_ends; e++) {
      const End& m = j.ends[(uint64_t)k * ENDS_PER_CHUNK + e];
      j.end_abs[n_ends] = off + m.pos, j.end_crc[n_ends] = m.crc, j.end_isize[n_ends] = m.isize;
      n_ends++;
    }
    member_before = !R.in_member ? 0 : R.member_start == BEFORE ? member_before + R.n_sym : R.n_sym - R.member_start;
    if (prev != BEFORE && j.runs[prev].n_sym < WINDOW) s.flags |= G_WIN_IN_WIN;
    s.flags |= R.flags, s.paths |= R.paths;
    off += R.n_sym;
    expect = R.end_bit;
    s.in_member = R.in_member, s.bit_offset = R.in_member ? (uint32_t)R.end_bit & 7u : 0;
    s.n_consumed = R.end_bit >> 3;
    // a run in which no block ended, behind a run that ended on a member header: the header counts only together with
    // its member's first block, so the stream stands before it
    if (R.end_bit == R.start_bit && R.n_sym == 0 && header_from != NONE) s.in_member = 0, s.bit_offset = 0, s.n_consumed = header_from >> 3;
    header_from = R.header_from;
    prev = k;
    n_runs++;
  }
  if (s.status == OK) {
    j.run_off[n_runs] = off;
    if (j.last_block && (s.in_member || s.n_consumed != j.n)) decline(TRUNCATED, prev == BEFORE ? 0 : prev);
    if (off > j.out_cap) decline(REGION, 0);
  }
  s.n_out = off, s.n_starts = n_runs, s.n_ends = n_ends;
  *j.sum = s;
}
// byte t of the window of run r >= 1 (chunks cur, prev): a symbol of the predecessor, or a byte of its window
INF_HD void window_byte(const Job& j, uint32_t cur, uint32_t prev, uint32_t t) {
  const uint32_t ns = j.runs[prev].n_sym;
  const uint8_t* pw = j.windows + (uint64_t)prev * WINDOW;
  uint32_t b;
  if (ns + t >= WINDOW) {
    const uint16_t s = j.syms[(uint64_t)prev * region_syms(j) + (ns + t - WINDOW)];
    b = s & 0x8000u ? pw[s & RING_MASK] : s & 0xFFu;
  } else {
    b = pw[t + ns];
  }
  j.windows[(uint64_t)cur * WINDOW + t] = (uint8_t)b;
}
// ... of run 0: the caller's window, its last byte last
INF_HD void window_byte_first(const Job& j, uint32_t t) {
  const uint32_t wl = j.st_in->window_len <= WINDOW ? j.st_in->window_len : WINDOW;
  j.windows[(uint64_t)j.run_list[0] * WINDOW + t] = t >= WINDOW - wl ? j.st_in->window[t - (WINDOW - wl)] : 0;
}

// ---- resolve ----
struct TileWork {
  uint32_t crc_tab[256], seg_crc[LANES];
  uint8_t bytes[TILE];
};
// tile T of the inflated bytes: symbols to bytes, to out and into the members' CRCs
INF_HD void resolve_tile(const Job& j, uint64_t T, TileWork& L) {
  const Summary& s = *j.sum;
  if (s.status != OK) return;
  const uint64_t a = T * TILE;
  if (a >= s.n_out) return;
  const uint32_t len = s.n_out - a < TILE ? (uint32_t)(s.n_out - a) : TILE;
  // the last run that begins at or before a
  uint32_t lo = 0, hi = s.n_starts;
  while (hi - lo > 1) {  // (run_off[0] == 0)
    const uint32_t mid = lo + (hi - lo) / 2;
    if (j.run_off[mid] <= a) lo = mid;
    else hi = mid;
  }
  const uint32_t r0 = lo;
  INF_LANES(lane) {
    fill_crc_table(L.crc_tab, lane);
    uint32_t r = r0;
    for (uint32_t i = lane; i < len; i += LANES) {
      const uint64_t at = a + i;
      while (r + 1 < s.n_starts && j.run_off[r + 1] <= at) r++;
      const uint32_t k = j.run_list[r];
      const uint16_t sy = j.syms[(uint64_t)k * region_syms(j) + (at - j.run_off[r])];
      const uint8_t b = sy & 0x8000u ? j.windows[(uint64_t)k * WINDOW + (sy & RING_MASK)] : (uint8_t)sy;
      L.bytes[i] = b;
      j.out[at] = b;
    }
  }
  INF_SYNC();
  // pieces of the tile by member: the first member end behind a
  uint32_t e = 0, eh = s.n_ends;
  while (e < eh) {
    const uint32_t mid = e + (eh - e) / 2;
    if (j.end_abs[mid] <= a) e = mid + 1;
    else eh = mid;
  }
  for (uint32_t pa = 0; pa < len;) {  // (each turn takes a byte at least: end_abs[e] > a + pa)
    const uint64_t member_end = e < s.n_ends ? j.end_abs[e] : s.n_out;
    const uint32_t pb = member_end - a < len ? (uint32_t)(member_end - a) : len;
    const uint32_t seg = (pb - pa + LANES - 1) / LANES;
    INF_LANES(lane) {
      const uint32_t l = pa + lane * seg < pb ? pa + lane * seg : pb, h = l + seg < pb ? l + seg : pb;
      uint32_t c = 0;
      if (l < h) c = bgz::crc_mul(bgz::crc_xpow8(pb - h), bgz::crc_bytes(L.crc_tab, L.bytes, l, h));
      L.seg_crc[lane] = c;
    }
    INF_SYNC();
    uint32_t c = fold_seg_crc(L.seg_crc);
    INF_SYNC();
    c = bgz::crc_mul(bgz::crc_xpow8((uint32_t)(member_end - (a + pb))), INF_UNIFORM(c));
    INF_LANES(lane) {
      if (lane == 0) xor_word(&j.member_crc[e], c);
    }
    pa = pb;
    while (e < s.n_ends && j.end_abs[e] <= a + pa) e++;
  }
}

// ---- verify: one thread for the members, then verify_window_byte for every t below the outgoing window_len ----
INF_HD void verify_serial(const Job& j) {
  Summary& s = *j.sum;
  if (s.status != OK) return;
  const State& st = *j.st_in;
  State& o = *j.st_out;
  uint64_t from = 0;
  for (uint32_t e = 0; e < s.n_ends && s.status == OK; e++) {
    const uint64_t to = j.end_abs[e];
    uint32_t crc = j.member_crc[e];
    uint64_t len = to - from;
    if (e == 0 && st.in_member) crc ^= bgz::crc_mul(bgz::crc_xpow8((uint32_t)to), st.crc), len += st.member_len;
    if (crc != j.end_crc[e]) s.status = CRC, s.bad_chunk = e;
    else if ((uint32_t)len != j.end_isize[e]) s.status = ISIZE, s.bad_chunk = e;
    from = to;
  }
  const bool carried = s.n_ends == 0 && st.in_member;
  o.bit_offset = s.bit_offset, o.in_member = s.in_member;
  o.crc = 0, o.member_len = 0;
  if (s.in_member) {
    o.crc = j.member_crc[s.n_ends] ^ (carried ? bgz::crc_mul(bgz::crc_xpow8((uint32_t)s.n_out), st.crc) : 0u);
    o.member_len = s.n_out - from + (carried ? st.member_len : 0);
  }
  o.window_len = (uint32_t)(o.member_len < WINDOW ? o.member_len : WINDOW);
  o.n_members_done = st.n_members_done + s.n_ends;
  o.stream_offset = st.stream_offset + s.n_consumed;
}
INF_HD void verify_window_byte(const Job& j, uint32_t t) {
  const Summary& s = *j.sum;
  const State& st = *j.st_in;
  State& o = *j.st_out;
  if (s.status != OK || t >= o.window_len) return;
  const uint64_t back = o.window_len - 1 - t;  // bytes between this one and the end of the member so far
  o.window[t] = back < s.n_out ? j.out[s.n_out - 1 - back] : st.window[st.window_len - 1 - (uint32_t)(back - s.n_out)];
}

}  // namespace gz
}  // namespace thm
#endif
