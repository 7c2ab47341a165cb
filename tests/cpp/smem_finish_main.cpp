// Stand-alone host program over thermite_amd/csrc/smem_finish.h: the finisher's decision, read by read, without a device.
// tests/test_smem_finish_host.py writes the input file (the index's tables as the kernels get them, options, reads and their
// seed hits in align_read's order) and compares what this program prints with the CPU oracle.
//
//   g++ -std=c++17 -O1 -Wall -Wextra -Werror -I thermite_amd/csrc tests/cpp/smem_finish_main.cpp -o smem_finish_main
//   ./smem_finish_main IN OUT
// With sanitizers: add -fsanitize=address,undefined -fno-omit-frame-pointer to the g++ line; the program has its own main and
// needs nothing preloaded.
//
// IN (little endian): u32 magic 'SFIN', u32 coordinate bytes (4 | 8), u32 n_refs, u32 classes; six tables, each u64 byte
// count + bytes padded to 8: ref_bin, ref_recs, exon_grid_off, exon_grid, gene_grid_off, gene_grid; thm_align_opts (32
// bytes); u32 max_read_len, max_bw, cpl, half; u64 n_reads; offsets[n_reads + 1] u64; bases (sanitised, offsets[n_reads]
// bytes, padded to 8); mem_off[n_reads + 1] u64; thm_mem[mem_off[n_reads]].
// OUT: one line per read -- what shape accepted ystart yend ylen tx_ystart tx_yend tx_ylen ops_off tx_ops_off score ref_id
// name_rank type_idx strand aln_type calls window_bytes op_bytes (the record fields are 0 unless accepted).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "smem_finish.h"

using namespace thm;

namespace {

struct Reader {
  std::vector<uint8_t> buf;
  size_t at = 0;
  void need(size_t n) const {
    if (at + n > buf.size()) {
      fprintf(stderr, "input truncated at byte %zu (+%zu of %zu)\n", at, n, buf.size());
      exit(2);
    }
  }
  template <class T>
  T get() {
    need(sizeof(T));
    T v;
    memcpy(&v, buf.data() + at, sizeof(T));
    at += sizeof(T);
    return v;
  }
  template <class T>
  std::vector<T> array(uint64_t bytes) {
    need(bytes);
    if (bytes % sizeof(T)) {
      fprintf(stderr, "table of %llu bytes is no array of %zu-byte elements\n", (unsigned long long)bytes, sizeof(T));
      exit(2);
    }
    std::vector<T> v(bytes / sizeof(T));
    if (bytes) memcpy(v.data(), buf.data() + at, bytes);
    at += (bytes + 7) & ~7ull;
    if (at > buf.size()) at = buf.size();
    return v;
  }
  template <class T>
  std::vector<T> table() {
    return array<T>(get<uint64_t>());
  }
};

template <class C>
int run(Reader& in, uint32_t n_refs, uint32_t classes, FILE* out) {
  const std::vector<uint32_t> ref_bin = in.table<uint32_t>();
  const std::vector<RefRecT<C>> ref_recs = in.table<RefRecT<C>>();
  const std::vector<uint32_t> exon_off = in.table<uint32_t>();
  const std::vector<ExonEntryT<C>> exon_grid = in.table<ExonEntryT<C>>();
  const std::vector<uint32_t> gene_off = in.table<uint32_t>();
  const std::vector<GridEntryT<C>> gene_grid = in.table<GridEntryT<C>>();
  if (ref_recs.size() != n_refs) return 2;
  const thm_align_opts opts = in.get<thm_align_opts>();
  const uint32_t max_read_len = in.get<uint32_t>(), max_bw = in.get<uint32_t>(), cpl = in.get<uint32_t>(), half = in.get<uint32_t>();
  const uint64_t n = in.get<uint64_t>();
  const std::vector<uint64_t> off = in.array<uint64_t>((n + 1) * 8);
  const std::vector<uint8_t> bases = in.array<uint8_t>(off[n]);
  const std::vector<uint64_t> mem_off = in.array<uint64_t>((n + 1) * 8);
  const std::vector<thm_mem> mems = in.array<thm_mem>(mem_off[n] * sizeof(thm_mem));
  fin::Tables<C> tb;
  tb.ref_bin = ref_bin.data();
  tb.ref_recs = ref_recs.data();
  tb.n_refs = n_refs;
  tb.exon_grid_off = exon_off.data();
  tb.exon_grid = exon_grid.data();
  tb.gene_grid_off = gene_off.data();
  tb.gene_grid = gene_grid.data();
  for (uint64_t r = 0; r < n; r++) {
    const uint32_t L = (uint32_t)(off[r + 1] - off[r]);
    const thm_mem* m = mems.data() + mem_off[r];
    const uint32_t n_hits = (uint32_t)(mem_off[r + 1] - mem_off[r]);
    fin::Outcome o;
    memset(&o, 0, sizeof o);
    o.what = fin::LEAVE;
    o.shape = fin::SHAPE_NONE;
    // the kernel's walk: the fast class only; SMEMs from the hits (two hits of one SMEM share position and length in the read)
    if (L > 0 && L <= max_read_len && n_hits >= 1 && n_hits <= 2) {
      const uint32_t smem_cnt = (n_hits == 2 && (m[0].query_idx != m[1].query_idx || m[0].len != m[1].len)) ? 2u : 1u;
      const fin::Setup st = fin::setup(opts, (int)L, max_bw, (int)cpl);
      if ((classes & fin::CLASS_E) && fin::shape_exact(smem_cnt, n_hits, m[0].query_idx, m[0].len, n_hits, L)) {
        o = fin::finish_exact<C>(tb, (C)m[0].ref_idx, (int)L, st, half);
      } else if ((classes & fin::CLASS_S) && smem_cnt == 2) {
        fin::Hit<C> h1, h2;
        h1.hr = (C)m[0].ref_idx;
        h1.q = m[0].query_idx;
        h1.len = m[0].len;
        h2.hr = (C)m[1].ref_idx;
        h2.q = m[1].query_idx;
        h2.len = m[1].len;
        int p = 0;
        C a0 = 0;
        if (fin::shape_subst<C>(smem_cnt, n_hits, 1, 1, h1, h2, L, p, a0))
          o = fin::finish_subst<C>(tb, bases.data() + off[r], h1, h2, (int)L, p, a0, st, half);
      }
    }
    const bool rec = o.what == fin::FINISHED && o.accepted;
    fprintf(out, "%d %d %d %llu %llu %llu %llu %llu %llu %u %u %d %u %u %u %u %u %u %u %u\n", o.what, o.shape, o.what == fin::FINISHED ? o.accepted : 0,
            (unsigned long long)(rec ? o.ystart : 0), (unsigned long long)(rec ? o.yend : 0), (unsigned long long)(rec ? o.ylen : 0),
            (unsigned long long)(rec ? o.tx_ystart : 0), (unsigned long long)(rec ? o.tx_yend : 0), (unsigned long long)(rec ? o.tx_ylen : 0),
            rec ? o.ops_off : 0u, rec ? o.tx_ops_off : 0u, rec ? o.score : 0, rec ? o.ref_id : 0u, rec ? o.name_rank : 0u, rec ? o.type_idx : 0u,
            rec ? (unsigned)o.strand : 0u, rec ? (unsigned)o.aln_type : 0u, o.what == fin::FINISHED ? o.calls : 0u,
            o.what == fin::FINISHED ? o.window_bytes : 0u, rec ? o.op_bytes : 0u);
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
    return 2;
  }
  Reader in;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  fseek(f, 0, SEEK_END);
  const long sz = ftell(f);
  fseek(f, 0, SEEK_SET);
  in.buf.resize((size_t)sz);
  if (sz && fread(in.buf.data(), 1, (size_t)sz, f) != (size_t)sz) return 2;
  fclose(f);
  if (in.get<uint32_t>() != 0x4e494653u) return 2;  // 'SFIN'
  const uint32_t cb = in.get<uint32_t>(), n_refs = in.get<uint32_t>(), classes = in.get<uint32_t>();
  FILE* out = fopen(argv[2], "w");
  if (!out) return 2;
  const int rc = cb == 8 ? run<uint64_t>(in, n_refs, classes, out) : run<uint32_t>(in, n_refs, classes, out);
  fclose(out);
  return rc;
}
