// quant_model_main.cpp -- the per-alignment functions of the count tables (thermite_amd/csrc/quant_device.h: the gene
// counter, the walk over the CIGAR words, the key, the row) run serially on the host, a std::map standing in for the
// sorts and the reduce-by-key of kernels_quant.hip.  tests/test_quant_host.py builds it with
// -fsanitize=address,undefined and compares its output with the expectation of tests/quant_common.py.
//
//   quant_model_main <in> <out>
// in : 7 x u64 (n_reads, n_alns, n_words, n_txs, n_genes, n_refs, has_status), off[n_reads + 1] u64, thm_aln[n_alns],
//      thm_aln_digest[n_alns], words[n_words] u32, tx_gene[n_txs] u32, tx_forward[n_txs] u8, ref_sq[n_refs] i32,
//      status[n_reads] i32 when has_status
// out: thm_quant_totals, thm_quant_gene[n_genes], thm_quant_junction[...]
// exit status 3: an alignment with an index out of range
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "quant_device.h"

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

struct Row {
  uint64_t n_unique = 0, n_multi = 0;
  uint32_t overhang = 0;
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s <in> <out>\n", argv[0]);
    return 2;
  }
  const std::vector<uint8_t> in = slurp(argv[1]);
  size_t at = 0;
  const std::vector<uint64_t> head = take<uint64_t>(in, at, 7);
  const uint64_t n_reads = head[0], n_alns = head[1], n_words = head[2], n_txs = head[3], n_genes = head[4], n_refs = head[5];
  const std::vector<uint64_t> off = take<uint64_t>(in, at, n_reads + 1);
  const std::vector<thm_aln> alns = take<thm_aln>(in, at, n_alns);
  const std::vector<thm_aln_digest> dig = take<thm_aln_digest>(in, at, n_alns);
  const std::vector<uint32_t> words = take<uint32_t>(in, at, n_words);
  const std::vector<uint32_t> tx_gene = take<uint32_t>(in, at, n_txs);
  const std::vector<uint8_t> tx_forward = take<uint8_t>(in, at, n_txs);
  const std::vector<int32_t> ref_sq = take<int32_t>(in, at, n_refs);
  const std::vector<int32_t> status = take<int32_t>(in, at, head[6] ? n_reads : 0);

  uint64_t tot[quant::N_TOTALS] = {0};
  std::vector<uint64_t> genes(n_genes * 4, 0);
  std::map<std::pair<uint64_t, uint64_t>, Row> rows;  // ordered by (hi, lo): the order of the two sort passes

  for (uint64_t r = 0; r < n_reads; r++) {
    const uint64_t nh = off[r + 1] - off[r];
    tot[quant::T_READS]++;
    if (head[6] && status[r] != THM_OK)
      tot[quant::T_FAILED]++;
    else if (nh == 0)
      tot[quant::T_UNMAPPED]++;
    else
      tot[nh == 1 ? quant::T_UNIQUE_READS : quant::T_MULTI_READS]++;
  }
  for (uint64_t a = 0; a < n_alns; a++) {
    // the read by the kernels' own lookup
    const uint64_t r = quant::read_of(off.data(), n_reads, a);
    if (!(off[r] <= a && a < off[r + 1])) {
      fprintf(stderr, "read_of(%llu) = %llu\n", (unsigned long long)a, (unsigned long long)r);
      return 4;
    }
    const bool multi = off[r + 1] - off[r] > 1;
    const thm_aln& al = alns[a];
    const thm_aln_digest& d = dig[a];
    const uint32_t c = quant::gene_counter(al.aln_type, al.tx_or_gene_idx, multi, tx_gene.data(), (uint32_t)n_txs, (uint32_t)n_genes);
    if (c == quant::BAD_INDEX || al.ref_id >= n_refs || ref_sq[al.ref_id] < 0 || d.cigar_off > n_words || d.n_cigar > n_words - d.cigar_off) return 3;
    tot[quant::T_ALNS]++;
    if (c == quant::NO_COUNTER)
      tot[multi ? quant::T_INTERGENIC_MULTI : quant::T_INTERGENIC_UNIQUE]++;
    else
      genes[c]++;
    if (d.flags & THM_DIGEST_LONG_RUN) {
      tot[quant::T_LONG_RUN]++;
      continue;
    }
    const uint32_t* w = words.data() + d.cigar_off;
    const uint32_t n_hits = quant::count_hits(w, d.n_cigar);
    if (n_hits == 0) continue;
    if (al.aln_type != THM_ALN_EXONIC) return 3;
    const bool forward = tx_forward[al.tx_or_gene_idx] != 0;
    const uint32_t ref = (uint32_t)ref_sq[al.ref_id];
    uint32_t seen = 0;
    const uint32_t again = quant::walk(w, d.n_cigar, al.ystart, [&](uint32_t k, const quant::Hit& h) {
      if (k != seen++) abort();  // hits come in order
      Row& row = rows[std::make_pair(quant::key_hi(ref, h.start), quant::key_lo(h.end, forward))];
      (multi ? row.n_multi : row.n_unique)++;
      const uint32_t ov = quant::overhang(h);
      row.overhang = ov > row.overhang ? ov : row.overhang;
    });
    if (again != n_hits || seen != n_hits) abort();
    tot[quant::T_SPLICED]++;
    tot[quant::T_HITS] += n_hits;
  }

  FILE* f = fopen(argv[2], "wb");
  if (!f) {
    perror(argv[2]);
    return 2;
  }
  fwrite(tot, 8, quant::N_TOTALS, f);
  if (n_genes) fwrite(genes.data(), 8, genes.size(), f);
  for (const auto& kv : rows) {
    const thm_quant_junction j = quant::row(kv.first.first, kv.first.second, kv.second.n_unique, kv.second.n_multi, kv.second.overhang);
    fwrite(&j, sizeof j, 1, f);
  }
  return fclose(f) == 0 ? 0 : 2;
}
