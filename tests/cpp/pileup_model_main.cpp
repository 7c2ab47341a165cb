// pileup_model_main.cpp -- the per-item functions of the per-base allele counts (thermite_amd/csrc/pileup_device.h: the
// kind of a byte, the shape and the checks of an alignment, the chunk a lane compares, the key of an event, the row of a
// position) run serially on the host: validate every alignment of a view, walk it as its group of pile::GROUP lanes does
// -- a loop for the lanes, every lane its chunks -- into a list of keys, sort and reduce them into a std::map standing in
// for the sorted table, deposit the blocks into a host difference array, then rows from a serial scan of the depth and
// the table's ranges -- the passes of kernels_pileup.hip with loops for the threads.  tests/test_pileup_host.py builds it
// with -fsanitize=address,undefined and compares its output with the expectation of tests/pileup_common.py.
//
//   pileup_model_main <in> <out>
// in : 6 x u64 (flags, n_refs, n_sq, n_windows, n_views, n_text), ref_sq[n_refs] i32, sq_len[n_sq] u64, tstart[n_sq] u64,
//      text[n_text], windows[n_windows] x 3 u64 (refID, start, n), then per view 5 x u64 (n_reads, n_alns, n_words,
//      has_status, n_bases), off[n_reads + 1] u64, thm_aln[n_alns], thm_aln_digest[n_alns], words[n_words] u32,
//      base_off[n_reads + 1] u64, bases[n_bases], status[n_reads] i32 when has_status
// out: thm_pile_totals, u64 n_events, for min_alt 1, 2, 3 u64 n_sites and thm_pile_site[n_sites], per window thm_pile_site[n]
// exit status 3: a view with an alignment the checks refuse (nothing of it is added, nothing is written)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "pileup_device.h"

using namespace thm;

namespace {

std::vector<uint8_t> slurp(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    perror(path);
    exit(2);
  }
  std::vector<uint8_t> b;
  uint8_t buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + n);
  fclose(f);
  return b;
}

// the next `count` items of type T of the input, copied out (the file's arrays stand at any alignment) into an array
// of exactly that size: a load that leaves it is the sanitiser's to find
template <class T>
std::vector<T> take(const std::vector<uint8_t>& b, size_t& at, uint64_t count) {
  if (count > (b.size() - at) / sizeof(T)) {
    fprintf(stderr, "input cut short at byte %zu\n", at);
    exit(2);
  }
  std::vector<T> v(count);
  if (count) memcpy(v.data(), b.data() + at, count * sizeof(T));
  at += count * sizeof(T);
  return v;
}

// the events of one checked alignment, as the lanes of its group find them
void walk(const thm_aln& al, const thm_aln_digest& d, const uint32_t* words, const uint8_t* text_c, uint64_t g_c, const uint8_t* read, uint64_t read_len,
          std::vector<uint64_t>& keys, uint64_t* n_mismatches) {
  const bool forward = al.strand == 1;
  uint64_t p = al.ystart, q = 0;
  for (uint32_t i = 0; i < d.n_cigar; i++) {
    const uint32_t w = words[i], code = w & 15u;
    const uint64_t len = w >> 4;
    if (code == quant::OP_M) {
      for (uint64_t s0 = 0; s0 < len; s0 += pile::GROUP * pile::CHUNK)
        for (uint32_t lane = 0; lane < pile::GROUP; lane++) {
          const uint64_t c0 = s0 + lane * pile::CHUNK;
          if (c0 >= len) continue;
          uint32_t kinds = 0;
          const uint32_t mask = pile::m_chunk(text_c, read, read_len, forward, p, q, len, c0, &kinds);
          for (uint32_t k = 0; k < pile::CHUNK; k++)
            if (mask >> k & 1u) {
              keys.push_back(pile::key_of(g_c + p + c0 + k, kinds >> (4 * k) & 15u));
              ++*n_mismatches;
            }
        }
      p += len;
      q += len;
    } else if (code == quant::OP_D) {
      for (uint64_t k = 0; k < len; k++) keys.push_back(pile::key_of(g_c + p + k, pile::KIND_DEL));
      p += len;
    } else if (code == quant::OP_N) {
      p += len;
    } else if (code == quant::OP_I) {
      keys.push_back(pile::key_of(g_c + pile::ins_pos(p, al.ystart), pile::KIND_INS));
      q += len;
    } else if (code == quant::OP_S) {
      q += len;
    }
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s <in> <out>\n", argv[0]);
    return 2;
  }
  const std::vector<uint8_t> in = slurp(argv[1]);
  size_t at = 0;
  const std::vector<uint64_t> head = take<uint64_t>(in, at, 6);
  const uint32_t flags = (uint32_t)head[0], n_refs = (uint32_t)head[1], n_sq = (uint32_t)head[2];
  const std::vector<int32_t> ref_sq = take<int32_t>(in, at, n_refs);
  const std::vector<uint64_t> sq_len = take<uint64_t>(in, at, n_sq);
  const std::vector<uint64_t> tstart = take<uint64_t>(in, at, n_sq);
  const std::vector<uint8_t> text = take<uint8_t>(in, at, head[5]);
  const std::vector<uint64_t> windows = take<uint64_t>(in, at, head[3] * 3);
  if (flags & ~THM_PILE_MULTI) return 2;
  std::vector<uint64_t> base(n_sq + 1, 0);
  for (uint32_t s = 0; s < n_sq; s++) base[s + 1] = base[s] + sq_len[s] + 1;
  std::vector<std::vector<uint8_t>> contigs(n_sq);
  for (uint32_t s = 0; s < n_sq; s++) {
    if (tstart[s] > text.size() || sq_len[s] > text.size() - tstart[s]) return 2;
    contigs[s].assign(text.begin() + tstart[s], text.begin() + tstart[s] + sq_len[s]);
  }
  std::vector<uint32_t> diff(base[n_sq], 0);
  std::map<uint64_t, uint32_t> table;
  uint64_t tot[pile::N_TOTALS] = {0};

  for (uint64_t view = 0; view < head[4]; view++) {
    const std::vector<uint64_t> vh = take<uint64_t>(in, at, 5);
    const uint64_t n_reads = vh[0], n_alns = vh[1], n_words = vh[2];
    const std::vector<uint64_t> off = take<uint64_t>(in, at, n_reads + 1);
    const std::vector<thm_aln> alns = take<thm_aln>(in, at, n_alns);
    const std::vector<thm_aln_digest> dig = take<thm_aln_digest>(in, at, n_alns);
    const std::vector<uint32_t> words = take<uint32_t>(in, at, n_words);
    const std::vector<uint64_t> base_off = take<uint64_t>(in, at, n_reads + 1);
    const std::vector<uint8_t> bases = take<uint8_t>(in, at, vh[4]);
    const std::vector<int32_t> status = take<int32_t>(in, at, vh[3] ? n_reads : 0);
    if (n_alns && !n_reads) return 2;
    // ---- count: the checks and the totals; nothing is added yet
    uint64_t bt[pile::N_TOTALS] = {0};
    std::vector<uint8_t> used(n_alns, 0);
    std::vector<uint64_t> aln_read(n_alns, 0);
    bool bad = false;
    for (uint64_t a = 0; a < n_alns; a++) {
      const uint64_t r = quant::read_of(off.data(), n_reads, a);
      const bool multi = off[r + 1] - off[r] > 1, long_run = (dig[a].flags & THM_DIGEST_LONG_RUN) != 0;
      uint32_t sq = 0;
      pile::Shape sh;
      if (!pile::check_aln(alns[a].ref_id, alns[a].ystart, dig[a].cigar_off, dig[a].n_cigar, long_run, words.data(), n_words, ref_sq.data(), n_refs, base.data(), n_sq,
                           base_off[r + 1] - base_off[r], &sq, &sh)) {
        bad = true;
        continue;
      }
      aln_read[a] = r;
      bt[pile::T_ALNS]++;
      if (multi && !(flags & THM_PILE_MULTI)) {
        bt[pile::T_SKIPPED_MULTI]++;
      } else if (long_run) {
        bt[pile::T_LONG_RUN]++;
      } else {
        bt[pile::T_USED]++;
        bt[pile::T_BLOCKS] += sh.n_blocks;
        bt[pile::T_M_BASES] += sh.m_bases;
        bt[pile::T_DEL_BASES] += sh.del_bases;
        bt[pile::T_INS] += sh.ins;
        bt[pile::T_INS_BASES] += sh.ins_bases;
        used[a] = sh.end > alns[a].ystart;
      }
    }
    if (bad) return 3;
    bt[pile::T_READS] = n_reads;
    for (int32_t s : status) bt[pile::T_FAILED] += s != THM_OK;
    // ---- extract, sort, reduce, merge
    std::vector<uint64_t> keys;
    for (uint64_t a = 0; a < n_alns; a++) {
      if (!used[a]) continue;
      const uint32_t sq = (uint32_t)ref_sq[alns[a].ref_id];
      const uint64_t r = aln_read[a];
      // (the contig and the read stand in arrays of their own size: a chunk load that leaves either is reported)
      const std::vector<uint8_t> read(bases.begin() + base_off[r], bases.begin() + base_off[r + 1]);
      walk(alns[a], dig[a], words.data() + dig[a].cigar_off, contigs[sq].data(), base[sq], read.data(), read.size(), keys, &bt[pile::T_MISMATCHES]);
    }
    if (keys.size() != bt[pile::T_MISMATCHES] + bt[pile::T_DEL_BASES] + bt[pile::T_INS]) return 4;
    std::sort(keys.begin(), keys.end());
    for (uint64_t k : keys) {
      if (pile::key_entry(k) >= base[n_sq] || pile::key_kind(k) >= pile::N_KINDS) return 4;
      table[k]++;
    }
    // ---- deposit
    for (uint64_t a = 0; a < n_alns; a++) {
      if (!used[a]) continue;
      uint64_t end = 0;
      const uint64_t g = base[ref_sq[alns[a].ref_id]];
      cov::walk_blocks(words.data() + dig[a].cigar_off, dig[a].n_cigar, alns[a].ystart,
                       [&](uint64_t s, uint64_t e) {
                         diff.at(g + s) += 1;
                         diff.at(g + e) -= 1;
                       },
                       &end);
    }
    for (int k = 0; k < pile::N_TOTALS; k++) tot[k] += bt[k];
  }
  if (at != in.size()) {
    fprintf(stderr, "%zu bytes behind the last view\n", in.size() - at);
    return 2;
  }
  // ---- the table as arrays, the depth by a serial scan
  std::vector<uint64_t> keys;
  std::vector<uint32_t> cnts;
  for (const auto& kv : table) {
    keys.push_back(kv.first);
    cnts.push_back(kv.second);
  }
  std::vector<uint32_t> depth(diff.size(), 0);
  uint32_t run = 0;
  for (size_t g = 0; g < diff.size(); g++) depth[g] = run += diff[g];
  FILE* f = fopen(argv[2], "wb");
  if (!f) {
    perror(argv[2]);
    return 2;
  }
  const uint64_t n_tab = keys.size();
  fwrite(tot, 8, pile::N_TOTALS, f);
  fwrite(&n_tab, 8, 1, f);
  for (uint32_t min_alt = 1; min_alt <= 3; min_alt++) {
    std::vector<thm_pile_site> sites;
    for (uint64_t j = 0; j < n_tab; j++) {
      const bool head = j == 0 || pile::key_entry(keys[j]) != pile::key_entry(keys[j - 1]);
      if (!head || pile::alt_of(keys.data(), cnts.data(), j, n_tab) < min_alt) continue;
      const uint64_t e = pile::key_entry(keys[j]);
      sites.push_back(pile::site_of(keys.data(), cnts.data(), j, n_tab, e, depth.at(e), base.data(), n_sq, tstart.data(), text.data()));
    }
    const uint64_t n = sites.size();
    fwrite(&n, 8, 1, f);
    if (n) fwrite(sites.data(), sizeof(thm_pile_site), n, f);
  }
  for (size_t w = 0; w < windows.size(); w += 3) {
    const uint64_t s = windows[w], start = windows[w + 1], n = windows[w + 2];
    if (s >= n_sq || n > pile::MAX_WINDOW || start > sq_len[s] || n > sq_len[s] - start) return 2;
    const uint64_t lo = pile::lower_bound(keys.data(), 0, n_tab, pile::key_of(base[s] + start, 0)),
                   hi = pile::lower_bound(keys.data(), lo, n_tab, pile::key_of(base[s] + start + n, 0));
    for (uint64_t x = start; x < start + n; x++) {
      const uint64_t e = base[s] + x;
      const thm_pile_site site =
          pile::site_of(keys.data(), cnts.data(), pile::lower_bound(keys.data(), lo, hi, pile::key_of(e, 0)), hi, e, depth.at(e), base.data(), n_sq, tstart.data(), text.data());
      fwrite(&site, sizeof site, 1, f);
    }
  }
  fclose(f);
  return 0;
}
