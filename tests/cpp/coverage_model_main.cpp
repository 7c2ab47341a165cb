// coverage_model_main.cpp -- the per-item functions of the coverage tracks (thermite_amd/csrc/coverage_device.h: the
// track, the block walk, the checks, the layout, the tile arithmetic, the run of a change point) run serially on the
// host: validate every alignment of a view, deposit into host arrays, then per tile of cov::TILE entries the sum and the
// change points with the carry of a serial scan, the runs by pairing change points, and the depth windows from the tile
// sums in front of them -- the passes of kernels_coverage.hip with a loop for the threads.  tests/test_coverage_host.py
// builds it with -fsanitize=address,undefined and compares its output with the expectation of tests/cov_common.py.
//
//   coverage_model_main <in> <out>
// in : 5 x u64 (flags, n_refs, n_sq, n_windows, n_views), ref_sq[n_refs] i32, sq_len[n_sq] u64, windows[n_windows] x 4 u64
//      (track, refID, start, n), then per view 4 x u64 (n_reads, n_alns, n_words, has_status), off[n_reads + 1] u64,
//      thm_aln[n_alns], thm_aln_digest[n_alns], words[n_words] u32, status[n_reads] i32 when has_status
// out: thm_cov_totals, per track u64 n_runs and thm_cov_run[n_runs], per window u32[n]
// exit status 3: a view with an alignment the checks refuse (nothing of it is added, nothing is written)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "coverage_device.h"

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

// the next `count` items of type T of the input, copied out (the file's arrays stand at any alignment)
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

// a std::vector that aborts on an index outside it: every add and every read of the tracks goes through one
struct Track {
  std::vector<uint32_t> d;
  uint32_t& at(uint64_t i) {
    if (i >= d.size()) {
      fprintf(stderr, "entry %llu of %zu\n", (unsigned long long)i, d.size());
      abort();
    }
    return d[i];
  }
};

// per tile of diff[g0, g0 + n): its 32-bit sum and its non-zero entries (the tiles pass)
void tile_pass(Track& tr, uint64_t g0, uint64_t n, std::vector<uint32_t>& sum, std::vector<uint64_t>& cnt) {
  const uint64_t nt = cov::n_tiles(n);
  sum.assign(nt, 0);
  cnt.assign(nt, 0);
  for (uint64_t t = 0; t < nt; t++)
    for (uint64_t x = t * cov::TILE; x < (t + 1) * cov::TILE && x < n; x++) {
      const uint32_t v = tr.at(g0 + x);
      sum[t] += v;
      cnt[t] += v ? 1 : 0;
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
  const std::vector<uint64_t> head = take<uint64_t>(in, at, 5);
  const uint32_t flags = (uint32_t)head[0], n_refs = (uint32_t)head[1], n_sq = (uint32_t)head[2];
  const std::vector<int32_t> ref_sq = take<int32_t>(in, at, n_refs);
  const std::vector<uint64_t> sq_len = take<uint64_t>(in, at, n_sq);
  const std::vector<uint64_t> windows = take<uint64_t>(in, at, head[3] * 4);
  if (flags & ~(THM_COV_STRANDED | THM_COV_MULTI)) return 2;
  std::vector<uint64_t> base(n_sq + 1, 0);
  for (uint32_t s = 0; s < n_sq; s++) base[s + 1] = base[s] + sq_len[s] + 1;
  const uint32_t n_tracks = cov::n_tracks(flags);
  std::vector<Track> tracks(n_tracks);
  for (Track& t : tracks) t.d.assign(base[n_sq], 0);
  uint64_t tot[cov::N_TOTALS] = {0};

  for (uint64_t view = 0; view < head[4]; view++) {
    const std::vector<uint64_t> vh = take<uint64_t>(in, at, 4);
    const uint64_t n_reads = vh[0], n_alns = vh[1], n_words = vh[2];
    const std::vector<uint64_t> off = take<uint64_t>(in, at, n_reads + 1);
    const std::vector<thm_aln> alns = take<thm_aln>(in, at, n_alns);
    const std::vector<thm_aln_digest> dig = take<thm_aln_digest>(in, at, n_alns);
    const std::vector<uint32_t> words = take<uint32_t>(in, at, n_words);
    const std::vector<int32_t> status = take<int32_t>(in, at, vh[3] ? n_reads : 0);
    if (n_alns && !n_reads) return 2;
    // ---- count: the checks and the totals; nothing is added yet
    uint64_t bt[cov::N_TOTALS] = {0};
    std::vector<uint8_t> track_of_aln(n_alns, cov::NO_TRACK);
    for (uint64_t a = 0; a < n_alns; a++) {
      const uint64_t r = quant::read_of(off.data(), n_reads, a);
      if (!(off[r] <= a && a < off[r + 1])) return 4;
      const bool multi = off[r + 1] - off[r] > 1;
      const thm_aln& al = alns[a];
      const thm_aln_digest& d = dig[a];
      const bool long_run = (d.flags & THM_DIGEST_LONG_RUN) != 0;
      uint32_t track = cov::track_of(flags, multi, al.strand == 1), sq = 0, n_blocks = 0;
      uint64_t bases = 0;
      if (!cov::check_aln(al.ref_id, al.ystart, d.cigar_off, d.n_cigar, long_run, words.data(), n_words, ref_sq.data(), n_refs, base.data(), n_sq, &sq, &n_blocks,
                          &bases))
        return 3;
      bt[cov::T_ALNS]++;
      if (track == cov::NO_TRACK) {
        bt[cov::T_SKIPPED_MULTI]++;
      } else if (long_run) {
        bt[cov::T_LONG_RUN]++;
        track = cov::NO_TRACK;
      } else {
        bt[cov::T_TRACK0 + 3 * track]++;
        bt[cov::T_TRACK0 + 3 * track + 1] += n_blocks;
        bt[cov::T_TRACK0 + 3 * track + 2] += bases;
      }
      track_of_aln[a] = (uint8_t)track;
    }
    for (uint64_t r = 0; r < n_reads; r++) {
      bt[cov::T_READS]++;
      if (vh[3] && status[r] != THM_OK) bt[cov::T_FAILED]++;
    }
    if (bt[cov::T_ALNS] > 0xFFFFFFFFull - tot[cov::T_ALNS]) return 3;
    // ---- deposit
    for (uint64_t a = 0; a < n_alns; a++) {
      if (track_of_aln[a] == cov::NO_TRACK) continue;
      Track& tr = tracks[track_of_aln[a]];
      const uint64_t g = base[ref_sq[alns[a].ref_id]];
      uint64_t end = 0;
      (void)cov::walk_blocks(words.data() + dig[a].cigar_off, dig[a].n_cigar, alns[a].ystart,
                             [&](uint64_t s, uint64_t e) {
                               tr.at(g + s) += 1u;
                               tr.at(g + e) += 0xFFFFFFFFu;
                             },
                             &end);
    }
    for (int k = 0; k < cov::N_TOTALS; k++) tot[k] += bt[k];
  }
  if (at != in.size()) {
    fprintf(stderr, "%zu bytes behind the last view\n", in.size() - at);
    return 2;
  }

  FILE* f = fopen(argv[2], "wb");
  if (!f) {
    perror(argv[2]);
    return 2;
  }
  fwrite(tot, 8, cov::N_TOTALS, f);
  // ---- fetch, every track over all contigs
  for (Track& tr : tracks) {
    const uint64_t n = base[n_sq];
    std::vector<uint32_t> sum;
    std::vector<uint64_t> cnt;
    tile_pass(tr, 0, n, sum, cnt);
    std::vector<uint64_t> entry;
    std::vector<uint32_t> depth;
    uint32_t carry = 0;
    for (uint64_t t = 0; t < sum.size(); t++) {  // points: the local scan behind the tile's carry
      uint32_t d = carry;
      const size_t before = entry.size();
      for (uint64_t x = t * cov::TILE; x < (t + 1) * cov::TILE && x < n; x++) {
        const uint32_t v = tr.at(x);
        if (!v) continue;
        d += v;
        entry.push_back(x);
        depth.push_back(d);
      }
      if (entry.size() - before != cnt[t]) abort();
      carry += sum[t];
      if (d != carry) abort();  // the tile's sum is what its scan ends on
    }
    if (carry != 0) abort();  // every block that began has ended
    std::vector<thm_cov_run> runs;
    for (size_t i = 0; i < entry.size(); i++)
      if (depth[i]) runs.push_back(cov::run_of(base.data(), n_sq, entry[i], depth[i], i + 1 < entry.size() ? entry[i + 1] : ~0ull));
    const uint64_t n_runs = runs.size();
    fwrite(&n_runs, 8, 1, f);
    if (n_runs) fwrite(runs.data(), sizeof(thm_cov_run), n_runs, f);
  }
  // ---- depth windows: tiles counted from the contig's first entry, the carry from the tiles in front
  for (size_t w = 0; w < windows.size(); w += 4) {
    const uint64_t track = windows[w], ref = windows[w + 1], start = windows[w + 2], n = windows[w + 3];
    if (track >= n_tracks || ref >= n_sq || n > cov::MAX_DEPTH_WINDOW || start > sq_len[ref] || n > sq_len[ref] - start) return 5;
    if (n == 0) continue;
    Track& tr = tracks[track];
    std::vector<uint32_t> sum, out(n);
    std::vector<uint64_t> cnt;
    tile_pass(tr, base[ref], start + n, sum, cnt);
    uint32_t carry = 0;
    for (uint64_t t = 0; t < sum.size(); t++) {
      if (t >= start / cov::TILE) {
        uint32_t d = carry;
        for (uint64_t x = t * cov::TILE; x < (t + 1) * cov::TILE && x < start + n; x++) {
          d += tr.at(base[ref] + x);
          if (x >= start) out[x - start] = d;
        }
      }
      carry += sum[t];
    }
    fwrite(out.data(), 4, n, f);
  }
  return fclose(f) == 0 ? 0 : 2;
}
