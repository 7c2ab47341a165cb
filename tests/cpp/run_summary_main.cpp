// run_summary_main.cpp -- the pure-host parts of thermite_amd/csrc/run_summary.h run on their own: check_cigar_view over
// hand-made views, and the arithmetic of SqLayout (lay_out, len, entries, check_contig).  No HIP call is made: the
// aligner it hands to the checks is an empty one that only carries the index and takes the message.
//
//   run_summary_main cov|pile <n_txs> <n_genes> < input
//
// `input` is what tests/cov_common.py (cov) or tests/pileup_common.py (pile) write with model_input(): the layout and
// the views.  Every view is checked as thm_coverage_add_view (cov) or thm_pileup_add_view (pile) checks it on the host --
// for pile with the read-length check of pileup.hip in the callable, which needs the running read index -- and a line
// "view <k>: <code> <message>" goes to standard output.  tools/run_summary_host_check.py builds it with
// -fsanitize=address,undefined, feeds it the shapes and the bad views of both modules and compares the lines.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pileup_device.h"
#include "run_summary.h"

// fail() also leaves its message where thm_last_error(nullptr) finds it (index.cpp, not linked here)
namespace thm {
void set_global_error(const std::string&) {}
}  // namespace thm

namespace {

std::vector<uint8_t> in;
size_t at = 0;

template <class T>
std::vector<T> take(size_t n) {
  if (n > (in.size() - at) / sizeof(T)) {
    fprintf(stderr, "input ends inside an array of %zu\n", n);
    exit(2);
  }
  std::vector<T> v(n);
  if (n) memcpy(v.data(), in.data() + at, n * sizeof(T));
  at += n * sizeof(T);
  return v;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4 || (strcmp(argv[1], "cov") && strcmp(argv[1], "pile"))) {
    fprintf(stderr, "usage: %s cov|pile n_txs n_genes < input\n", argv[0]);
    return 2;
  }
  const bool pile = !strcmp(argv[1], "pile");
  const char* who = pile ? "thm_pileup_add_view" : "thm_coverage_add_view";
  uint8_t buf[1 << 16];
  for (size_t n; (n = fread(buf, 1, sizeof buf, stdin)) > 0;) in.insert(in.end(), buf, buf + n);

  const std::vector<uint64_t> head = take<uint64_t>(pile ? 6 : 5);
  const uint64_t n_refs = head[1], n_sq = head[2], n_windows = head[3], n_views = head[4];
  thm_index ix;
  ix.refs.resize(n_refs);
  ix.txs.resize(strtoull(argv[2], nullptr, 10));
  ix.genes.resize(strtoull(argv[3], nullptr, 10));
  thm_aligner a;
  a.ix = &ix;
  SqLayout sq;
  sq.h_ref_sq = take<int32_t>(n_refs);
  const std::vector<uint64_t> lens = take<uint64_t>(n_sq);
  if (pile) {
    (void)take<uint64_t>(n_sq);   // tstart
    (void)take<uint8_t>(head[5]);  // the text
  }
  (void)take<uint64_t>(n_windows * (pile ? 3 : 4));
  std::vector<std::pair<std::string, uint64_t>> lines;
  for (uint64_t s = 0; s < n_sq; s++) lines.emplace_back("sq" + std::to_string(s), lens[s]);
  sq.lay_out(lines);
  // the layout's arithmetic: an entry more than bases per contig, the contigs behind one another
  uint64_t sum = 0;
  for (uint32_t s = 0; s < sq.n_sq; s++) {
    if (sq.len(s) != lens[s] || sq.h_base[s] != sum) {
      fprintf(stderr, "contig %u: len %llu of %llu, base %llu of %llu\n", s, (unsigned long long)sq.len(s), (unsigned long long)lens[s],
              (unsigned long long)sq.h_base[s], (unsigned long long)sum);
      return 1;
    }
    sum += lens[s] + 1;
  }
  if (sq.n_sq != n_sq || sq.entries() != sum) {
    fprintf(stderr, "%u contigs with %llu entries, %llu expected\n", sq.n_sq, (unsigned long long)sq.entries(), (unsigned long long)sum);
    return 1;
  }
  printf("layout: %u contigs, %llu entries\n", sq.n_sq, (unsigned long long)sq.entries());

  for (uint64_t k = 0; k < n_views; k++) {
    const std::vector<uint64_t> vh = take<uint64_t>(pile ? 5 : 4);
    const std::vector<uint64_t> off = take<uint64_t>(vh[0] + 1);
    const std::vector<thm_aln> alns = take<thm_aln>(vh[1]);
    const std::vector<thm_aln_digest> dig = take<thm_aln_digest>(vh[1]);
    const std::vector<uint32_t> words = take<uint32_t>(vh[2]);
    std::vector<uint64_t> base_off;
    if (pile) {
      base_off = take<uint64_t>(vh[0] + 1);
      (void)take<uint8_t>(vh[4]);
    }
    const std::vector<int32_t> status = take<int32_t>(vh[3] ? vh[0] : 0);
    // (every array is a heap block of exactly its size: a read past its end is the sanitizer's to see)
    thm_cigar_view v;
    memset(&v, 0, sizeof v);
    v.n_reads = vh[0];
    v.n_alns = vh[1];
    v.n_cigar_words = vh[2];
    v.read_aln_off = vh[0] ? off.data() : nullptr;
    v.alns = alns.empty() ? nullptr : alns.data();
    v.digests = dig.empty() ? nullptr : dig.data();
    v.cigar = words.empty() ? nullptr : words.data();
    v.read_status = status.empty() ? nullptr : status.data();
    a.err.clear();
    uint64_t r = 0;
    const int rc = check_cigar_view(&a, who, &v, sq.h_ref_sq, [&](uint64_t i, const thm_aln& al, const thm_aln_digest& d) {
      if (const int c = sq.check_contig(&a, who, i, al, d.ref_len); c != THM_OK || !pile) return c;
      while (v.read_aln_off[r + 1] <= i) r++;
      if ((d.flags & THM_DIGEST_LONG_RUN) || d.n_cigar == 0) return (int)THM_OK;
      const thm::pile::Shape sh = thm::pile::shape_of(v.cigar + d.cigar_off, d.n_cigar, al.ystart);
      if (sh.qlen != base_off[r + 1] - base_off[r])
        return fail(&a, THM_ERR_INVALID_ARG, "%s: alignment %llu: its M + I + S is %llu, read %llu has %llu bases", who, (unsigned long long)i,
                    (unsigned long long)sh.qlen, (unsigned long long)r, (unsigned long long)(base_off[r + 1] - base_off[r]));
      return (int)THM_OK;
    });
    printf("view %llu: %d %s\n", (unsigned long long)k, rc, a.err.c_str());
  }
  if (at != in.size()) {
    fprintf(stderr, "%zu bytes behind the last view\n", in.size() - at);
    return 2;
  }
  return 0;
}
