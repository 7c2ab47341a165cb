// The cell rule of the seed stage (thermite_amd/csrc/seed_bounds.h) on the host, against matching statistics computed by
// brute force.  The program models which positions the seed kernels probe (kernels_seed.hip: position 0, the stride-8
// grid and the last position, then the inner positions of grid cells) and what each probe knows, derives the row of match
// ends twice -- straight from MS, and through grid bounds, the header's rule and probes -- and checks that the rows are
// equal, that no position the rule decides starts an SMEM, and that the header's mask lists exactly the positions the
// three cases of the rule leave.  It counts the probes with the rule on and off, which is what thm_debug_seed_stats
// (decided + full) must report for the same reads.
//
//   seed_bounds_main                 named cases and a seeded random sweep over its own text; prints one line per case,
//                                    then "ok <checks>" (exit 0) or the failed checks (exit 1)
//   seed_bounds_main --file F        a batch written by tests/seed_bounds_common.py (text, reads, k, kt); MS from a suffix
//                                    array (the stand-alone run checks that road against brute force); prints
//                                    "probes <rule off> <rule on>"
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Ithermite_amd/csrc tests/cpp/seed_bounds_main.cpp -o seed_bounds_asan
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "seed_bounds.h"

namespace {

int n_checks = 0, n_failed = 0;
#define CHECK(cond)                                                                \
  do {                                                                             \
    n_checks++;                                                                    \
    if (!(cond)) {                                                                 \
      if (n_failed++ < 20) fprintf(stderr, "line %d: %s [%s]\n", __LINE__, #cond, g_what.c_str()); \
    }                                                                              \
  } while (0)

std::string g_what;
using Bytes = std::vector<uint8_t>;
using namespace thm;

constexpr int SHORT_READ_MAX = 255;  // launch.h: longer reads have their cells listed whole

uint8_t sanitize(uint8_t c) {
  if (c >= 'a' && c <= 'z') c = (uint8_t)(c - 32);
  return (c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == 'N') ? c : (uint8_t)0;
}
Bytes revcomp(const Bytes& s) {
  Bytes r(s.rbegin(), s.rend());
  for (auto& c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c;
  return r;
}
// both strands of every contig, each closed by '$', as the index lays the text out
Bytes both_strands(const std::vector<Bytes>& contigs) {
  Bytes t;
  for (const auto& c : contigs) {
    t.insert(t.end(), c.begin(), c.end());
    t.push_back('$');
  }
  for (const auto& c : contigs) {
    const Bytes r = revcomp(c);
    t.insert(t.end(), r.begin(), r.end());
    t.push_back('$');
  }
  return t;
}

int lcp_at(const Bytes& text, size_t t, const uint8_t* q, int cap) {
  int l = 0;
  while (l < cap && t + (size_t)l < text.size() && text[t + l] == q[l]) l++;
  return l;
}
// MS[i] for every position of the (sanitised) read by brute force: the longest byte match of rd[i..L) anywhere
// (every text position that holds the read's byte is tried; `where` lists the positions of each byte value once per text)
std::vector<int> ms_brute(const Bytes& text, const Bytes& rd) {
  static const Bytes* listed = nullptr;
  static std::vector<uint32_t> where[256];
  if (listed != &text) {
    for (auto& w : where) w.clear();
    for (size_t t = 0; t < text.size(); t++) where[text[t]].push_back((uint32_t)t);
    listed = &text;
  }
  const int L = (int)rd.size();
  std::vector<int> ms(L, 0);
  for (int i = 0; i < L; i++) {
    int best = 0;
    for (uint32_t t : where[rd[i]]) best = std::max(best, lcp_at(text, t, rd.data() + i, L - i));
    ms[i] = best;
  }
  return ms;
}
// the same from a suffix array: insertion point of the tail, the better of its two neighbours
struct SuffixArray {
  const Bytes& text;
  std::vector<uint32_t> sa;
  explicit SuffixArray(const Bytes& t) : text(t), sa(t.size()) {
    for (size_t i = 0; i < sa.size(); i++) sa[i] = (uint32_t)i;
    const size_t n = t.size();
    const uint8_t* p = t.data();
    std::sort(sa.begin(), sa.end(), [=](uint32_t a, uint32_t b) {
      const size_t la = n - a, lb = n - b;
      const int c = memcmp(p + a, p + b, std::min(la, lb));
      return c ? c < 0 : la < lb;
    });
  }
  int ms(const uint8_t* q, int cap) const {
    size_t a = 0, b = sa.size();
    while (a < b) {
      const size_t m = a + (b - a) / 2;
      const size_t s = sa[m];
      const int l = lcp_at(text, s, q, cap);
      const bool less = l < cap && (s + (size_t)l >= text.size() || text[s + l] < q[l]);
      if (less)
        a = m + 1;
      else
        b = m;
    }
    int best = 0;
    if (a > 0) best = std::max(best, lcp_at(text, sa[a - 1], q, cap));
    if (a < sa.size()) best = std::max(best, lcp_at(text, sa[a], q, cap));
    return best;
  }
  std::vector<int> ms_all(const Bytes& rd) const {
    const int L = (int)rd.size();
    std::vector<int> out(L);
    for (int i = 0; i < L; i++) out[i] = ms(rd.data() + i, L - i);
    return out;
  }
};

// what ms_search knows after probing `pos` (seed_bounds.h): d and whether the table path found an empty bucket
struct Probe {
  int d;
  bool empty;
};
Probe probe(const Bytes& rd, const std::vector<int>& ms, int pos, int k, int kt) {
  bool table = kt <= k;
  for (int t = 0; table && t < kt; t++) {
    const uint8_t c = rd[pos + t];
    table = c == 'A' || c == 'C' || c == 'G' || c == 'T';
  }
  if (table && ms[pos] < kt) return {0, true};  // no text position starts with the kt-mer
  return {ms[pos], false};
}

struct Counts {
  long probes = 0, decided = 0;
};

// one read through the model of the seed kernels; `bounds`: the rule of seed_bounds.h on (off: the cells rule it replaced)
void run_read(const Bytes& rd, const std::vector<int>& ms, int k, int kt, bool bounds, Counts& cnt) {
  const int L = (int)rd.size();
  if (k > L) return;
  const int npos = L - k + 1;
  std::vector<int> want(npos), row(npos, -1);
  for (int i = 0; i < npos; i++) want[i] = ms[i] >= k ? i + ms[i] : 0;
  for (int i = 0; i + 1 < L; i++) CHECK(i + 1 + ms[i + 1] >= i + ms[i]);  // (M): the match end never decreases
  std::vector<char> was_decided(npos, 0);
  std::vector<int> la(npos, 0), ub(npos, 0);
  auto do_probe = [&](int pos) {
    const Probe pr = probe(rd, ms, pos, k, kt);
    sbd::probe_bound(pos, pr.d, pr.empty, kt, L, la[pos], ub[pos]);
    CHECK(la[pos] <= pos + ms[pos] && pos + ms[pos] <= ub[pos]);
    CHECK(pr.empty || (la[pos] == ub[pos]));
    row[pos] = pr.d >= k ? pos + pr.d : 0;
    cnt.probes++;
  };
  do_probe(0);  // seed_first_kernel
  if (ms[0] >= k && ms[0] == L) return;  // the match spans the read: it leaves the seed stage
  la[0] = sbd::first_lower_bound(row[0]);  // only the stored end of position 0 is left
  if (npos == 1) {
    CHECK(row[0] == want[0]);
    return;
  }
  for (int pos = sbd::STRIDE; pos < npos - 1; pos += sbd::STRIDE) do_probe(pos);
  do_probe(npos - 1);
  const bool rule = bounds && L <= SHORT_READ_MAX;
  for (int a = 0; a < npos - 1; a += sbd::STRIDE) {
    const int b = std::min(a + sbd::STRIDE, npos - 1);
    if (b - a <= 1) continue;
    unsigned mask;
    if (rule) {
      mask = sbd::cell_mask(a, b, la[a], ub[b], k);
      for (int i = a + 1; i < b; i++) {
        // the three cases as the proof states them, position by position
        const bool case1 = ub[b] - i < k, case2 = !case1 && la[a] == ub[b] && (a != 0 || ub[b] - b >= k);  // (first cell: stored ends agree)
        CHECK((((mask >> (i - a)) & 1u) != 0) == (!case1 && !case2));
        if (!((mask >> (i - a)) & 1u)) {
          row[i] = sbd::decided_end(i, la[a], ub[b], k);
          was_decided[i] = 1;
          cnt.decided++;
        }
      }
      CHECK((mask & 1u) == 0 && (mask >> (b - a)) == 0);
    } else if (row[a] != 0 && row[a] == row[b]) {
      mask = 0;
      for (int i = a + 1; i < b; i++) row[i] = row[a];
    } else {
      mask = ((1u << (b - a)) - 1u) & ~1u;
    }
    for (int i = a + 1; i < b; i++)
      if ((mask >> (i - a)) & 1u) do_probe(i);
  }
  for (int i = 0; i < npos; i++) {
    CHECK(row[i] == want[i]);
    if (was_decided[i]) CHECK(!(want[i] != 0 && want[i] > want[i - 1]));  // no SMEM starts at a decided position
  }
}

struct Case {
  std::string name;
  std::vector<Bytes> reads;  // raw
  int k, kt;
};

Bytes sanitized(const Bytes& r) {
  Bytes s(r);
  for (auto& c : s) c = sanitize(c);
  return s;
}

// both settings over a case; MS by brute force, checked against the suffix-array road
void run_case(const Bytes& text, const SuffixArray& sa, const Case& c, bool print) {
  Counts off, on;
  for (size_t r = 0; r < c.reads.size(); r++) {
    g_what = c.name + " read " + std::to_string(r) + " k " + std::to_string(c.k) + " kt " + std::to_string(c.kt);
    const Bytes rd = sanitized(c.reads[r]);
    const std::vector<int> ms = ms_brute(text, rd);
    CHECK(ms == sa.ms_all(rd));
    run_read(rd, ms, c.k, c.kt, false, off);
    run_read(rd, ms, c.k, c.kt, true, on);
  }
  CHECK(on.probes <= off.probes);
  if (print)
    printf("%-22s reads %4zu k %2d kt %2d probes: rule off %6ld, on %6ld (decided without a probe %ld)\n", c.name.c_str(), c.reads.size(),
           c.k, c.kt, off.probes, on.probes, on.decided);
}

const char ACGT[] = "ACGT";
Bytes random_bases(std::mt19937& g, int n) {
  Bytes b(n);
  for (auto& c : b) c = (uint8_t)ACGT[g() & 3];
  return b;
}
uint8_t other(uint8_t a, uint8_t b = 0) {
  for (char c : ACGT)
    if (c && (uint8_t)c != a && (uint8_t)c != b) return (uint8_t)c;
  return 'A';
}
Bytes sub(Bytes r, int p) {
  r[p] = other(r[p]);
  return r;
}
Bytes cut(const Bytes& s, size_t at, size_t n) { return Bytes(s.begin() + at, s.begin() + at + n); }
Bytes cat(const Bytes& a, const Bytes& b) {
  Bytes r(a);
  r.insert(r.end(), b.begin(), b.end());
  return r;
}

int stand_alone() {
  // the text: two contigs; the first holds a 60-base stretch twice (different bases in front and behind) and an N run
  std::mt19937 g(0x5eedb0u);
  constexpr int MAIN = 2600, SECOND = 700, DUP_A = 400, DUP_B = 1500, DUP_LEN = 60, N0 = 2000, N1 = 2040;
  Bytes main_c = random_bases(g, MAIN), second = random_bases(g, SECOND);
  std::copy(main_c.begin() + DUP_A, main_c.begin() + DUP_A + DUP_LEN, main_c.begin() + DUP_B);
  main_c[DUP_B - 1] = other(main_c[DUP_A - 1]);
  main_c[DUP_B + DUP_LEN] = other(main_c[DUP_A + DUP_LEN]);
  std::fill(main_c.begin() + N0, main_c.begin() + N1, (uint8_t)'N');
  const Bytes text = both_strands({main_c, second});
  const SuffixArray sa(text);

  std::vector<Case> cases;
  auto one_sub = [&](int L, int k, int kt, const char* name) {
    Case c{name, {}, k, kt};
    const Bytes w = cut(main_c, 700, L);
    for (int p = 0; p < L; p++) c.reads.push_back(sub(w, p));
    const Bytes v = revcomp(cut(main_c, 1000, L));
    for (int p = 0; p < L; p++) c.reads.push_back(sub(v, p));
    cases.push_back(c);
  };
  one_sub(91, 20, 8, "one_sub_L91");
  one_sub(29, 20, 8, "one_sub_L29");
  one_sub(35, 20, 8, "one_sub_L35");
  one_sub(20, 20, 8, "length_k");
  one_sub(21, 20, 8, "length_k_plus_1");
  one_sub(140, 40, 8, "k40");
  one_sub(50, 8, 8, "k_is_kt");
  one_sub(40, 6, 8, "k_below_kt");
  one_sub(91, 20, 14, "one_sub_kt14");
  {
    Case c{"two_subs", {}, 20, 8};
    const Bytes w = cut(main_c, 1100, 91);
    for (int p = 0; p < 80; p++)
      for (int gap : {19, 20, 21, 29})
        if (p + gap < 91) c.reads.push_back(sub(sub(w, p), p + gap));
    cases.push_back(c);
  }
  {
    // reads that follow one copy of the stretch and leave it: a grid point inside the stretch matches longer at the
    // other copy than along the read's own locus wherever a substitution cuts the own locus short
    Case c{"duplicate", {}, 20, 8};
    for (int at : {DUP_A, DUP_B})
      for (int s = 0; s < 40; s++) {
        Bytes r = cut(main_c, at + s - 20, 91);
        c.reads.push_back(r);
        c.reads.push_back(sub(r, 20 + DUP_LEN - s + 3));  // just behind the stretch
        c.reads.push_back(sub(r, 10));                    // in front of it
      }
    cases.push_back(c);
  }
  {
    // a substitution inside the kt-mer of a grid point: its bucket is (almost surely) empty
    Case c{"empty_bucket", {}, 20, 8};
    const Bytes w = cut(main_c, 100, 91);
    for (int gp : {8, 16, 24, 32, 40, 48, 56, 64})
      for (int j = 0; j < 8; j++) c.reads.push_back(sub(w, gp + j));
    cases.push_back(c);
  }
  {
    Case c{"n_and_contig_end", {}, 20, 8};
    const Bytes w = cut(main_c, 1200, 91);
    for (int p : {0, 7, 8, 33, 45, 70, 90})
      for (char ch : {'N', 'n', 'X', '*', '\0', '$'}) {
        Bytes r = w;
        r[p] = (uint8_t)ch;
        c.reads.push_back(r);
      }
    for (int n : {30, 40, 47, 48, 49, 60}) {
      const Bytes tail = random_bases(g, 91 - n);
      c.reads.push_back(cat(cut(second, SECOND - n, n), tail));   // the match stops at '$'
      c.reads.push_back(cat(cut(main_c, MAIN - n, n), tail));
      c.reads.push_back(cat(cut(main_c, N0 - n, n), tail));       // ... at the N run
      c.reads.push_back(cut(main_c, N0 - n, 91));                 // N against N: the match goes on through the run
      c.reads.push_back(revcomp(cat(tail, cut(second, 0, n))));   // the other strand's contig end
    }
    cases.push_back(c);
  }
  {
    Case c{"indels", {}, 20, 8};
    const Bytes w = cut(main_c, 300, 92);
    for (int p = 4; p < 88; p++) {
      Bytes ins = cat(cut(w, 0, p), Bytes{other(w[p - 1], w[p])});
      c.reads.push_back(cat(ins, cut(w, p, 90 - p)));
      c.reads.push_back(cat(cut(w, 0, p), cut(w, p + 1, 91 - p)));
    }
    cases.push_back(c);
  }
  {
    Case c{"one_long_among_short", {}, 20, 8};
    for (int i = 0; i < 10; i++) c.reads.push_back(sub(cut(main_c, 100 + 97 * i, 91), (7 * i) % 91));
    Bytes w = cut(main_c, 2100, 300);
    for (int p = 17; p < 300; p += 61) w = sub(w, p);
    c.reads.insert(c.reads.begin() + 5, w);
    for (int L : {255, 256}) c.reads.push_back(sub(cut(main_c, 50, L), L / 2));
    cases.push_back(c);
  }
  for (const auto& c : cases) run_case(text, sa, c, true);

  // the one-substitution cases: the rule must remove probes, and the row stays what it was (checked in run_read)
  {
    Counts off, on;
    const Bytes w = cut(main_c, 700, 91);
    g_what = "one substitution saves probes";
    for (int p = 0; p < 91; p++) {
      const Bytes rd = sub(w, p);
      const std::vector<int> ms = ms_brute(text, rd);
      Counts o1, o2;
      run_read(rd, ms, 20, 8, false, o1);
      run_read(rd, ms, 20, 8, true, o2);
      CHECK(o2.probes <= o1.probes);
      off.probes += o1.probes;
      on.probes += o2.probes;
    }
    CHECK(on.probes < off.probes);
  }

  // seeded random sweep: every L from k to 120, 0..4 errors (substitutions, insertions, deletions), k x kt
  long sweep_off = 0, sweep_on = 0, sweep_reads = 0;
  for (int L = 6; L <= 120; L++)
    for (int nerr = 0; nerr <= 4; nerr++) {
      const size_t at = g() % (text.size() - 130);  // anywhere: contig ends, the N run and both strands included
      Bytes r = cut(text, at, L + 4);
      for (int e = 0; e < nerr; e++) {
        const int p = (int)(g() % r.size());
        switch (g() % 3) {
          case 0: r[p] = other(r[p]); break;
          case 1: r.insert(r.begin() + p, (uint8_t)ACGT[g() & 3]); break;
          default:
            if (r.size() > (size_t)L) r.erase(r.begin() + p);
        }
      }
      r.resize(L, 'A');
      const Bytes rd = sanitized(r);  // ('$' of the text becomes 0, as in a real read)
      const std::vector<int> ms = ms_brute(text, rd);
      g_what = "sweep L " + std::to_string(L) + " errors " + std::to_string(nerr);
      CHECK(ms == sa.ms_all(rd));
      for (int k : {6, 8, 20, 40})
        for (int kt : {8, 14}) {
          if (L < k) continue;
          g_what = "sweep L " + std::to_string(L) + " errors " + std::to_string(nerr) + " k " + std::to_string(k) + " kt " + std::to_string(kt);
          Counts off, on;
          run_read(rd, ms, k, kt, false, off);
          run_read(rd, ms, k, kt, true, on);
          CHECK(on.probes <= off.probes);
          sweep_off += off.probes;
          sweep_on += on.probes;
          sweep_reads++;
        }
    }
  printf("%-22s reads %4ld probes: rule off %6ld, on %6ld\n", "random_sweep", sweep_reads, sweep_off, sweep_on);
  if (n_failed) {
    fprintf(stderr, "%d of %d checks failed\n", n_failed, n_checks);
    return 1;
  }
  printf("ok %d\n", n_checks);
  return 0;
}

int from_file(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    return 2;
  }
  char magic[4];
  uint32_t k = 0, kt = 0;
  uint64_t n_text = 0, n_reads = 0;
  bool ok = fread(magic, 1, 4, f) == 4 && memcmp(magic, "SBD1", 4) == 0 && fread(&k, 4, 1, f) == 1 && fread(&kt, 4, 1, f) == 1 &&
            fread(&n_text, 8, 1, f) == 1 && fread(&n_reads, 8, 1, f) == 1 && n_text < (1ull << 31) && n_reads < (1ull << 24);
  std::vector<uint64_t> off;
  Bytes text, bases;
  if (ok) {
    off.resize(n_reads + 1);
    text.resize(n_text);
    ok = fread(off.data(), 8, off.size(), f) == off.size() && (n_text == 0 || fread(text.data(), 1, n_text, f) == n_text);
    ok = ok && off[0] == 0 && std::is_sorted(off.begin(), off.end()) && off.back() < (1ull << 31);
  }
  if (ok) {
    bases.resize(off.back());
    ok = bases.empty() || fread(bases.data(), 1, bases.size(), f) == bases.size();
  }
  fclose(f);
  if (!ok) {
    fprintf(stderr, "%s: not a batch file\n", path);
    return 2;
  }
  const SuffixArray sa(text);
  Counts c_off, c_on;
  for (uint64_t r = 0; r < n_reads; r++) {
    g_what = "read " + std::to_string(r);
    const Bytes rd = sanitized(Bytes(bases.begin() + off[r], bases.begin() + off[r + 1]));
    const std::vector<int> ms = sa.ms_all(rd);
    run_read(rd, ms, (int)k, (int)kt, false, c_off);
    run_read(rd, ms, (int)k, (int)kt, true, c_on);
  }
  if (n_failed) {
    fprintf(stderr, "%d of %d checks failed\n", n_failed, n_checks);
    return 1;
  }
  printf("probes %ld %ld\n", c_off.probes, c_on.probes);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 3 && strcmp(argv[1], "--file") == 0) return from_file(argv[2]);
  if (argc != 1) {
    fprintf(stderr, "usage: %s [--file batch]\n", argv[0]);
    return 2;
  }
  return stand_alone();
}
