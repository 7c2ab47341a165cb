// cells_model_main.cpp -- the functions of thermite_amd/csrc/cells_device.h run serially over one view: the passes of
// kernels_cells.hip with loops for the threads and a std::map for the sorts and the reduce-by-key.  tests/test_cells_host.py
// builds it with AddressSanitizer and UBSan as this stand-alone program and compares what it writes with the expectation of
// tests/cells_common.py.  Every array of the input stands in an allocation of its own, sized to the byte -- the name pool
// above all -- so a function that reads a byte outside [name_off[0], name_off[n]) is caught here.
//
//   cells_model_main in.bin out.bin      exit 0; 2: bad input; 3: an alignment has a type or an index out of range
//
// in.bin   u64 n_reads, n_alns, n_txs, n_genes, has_status, flags, cb_len, umi_len, min_umis, n_name_bytes; u64
//          offsets[n_reads + 1]; thm_aln alns[n_alns]; u32 tx_gene[n_txs]; u64 name_off[n_reads + 1]; i32 status[n_reads] (with
//          has_status); u8 names[n_name_bytes]
// out.bin  u64 totals[8]; u64 n_molecules, n_barcodes, n_cells_below, n_cells, n_entries; thm_cell cells[n_cells];
//          thm_cell_entry entries[n_entries]; u32 (barcode, gene, umi, reads)[n_molecules] in key order
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <utility>
#include <vector>

#include "cells_device.h"

using namespace thm;

namespace {

struct Input {
  std::vector<unsigned char> bytes;
  size_t at = 0;
  bool ok = true;
  // n elements of T into an allocation of exactly their size
  template <class T>
  std::unique_ptr<T[]> take(size_t n) {
    std::unique_ptr<T[]> out(new T[n]);
    if (at + n * sizeof(T) > bytes.size()) {
      ok = false;
      return out;
    }
    if (n) memcpy(out.get(), bytes.data() + at, n * sizeof(T));
    at += n * sizeof(T);
    return out;
  }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  Input in;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  unsigned char buf[1 << 16];
  for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) in.bytes.insert(in.bytes.end(), buf, buf + n);
  fclose(f);
  const auto head = in.take<uint64_t>(10);
  if (!in.ok) return 2;
  const uint64_t n_reads = head[0], n_alns = head[1], n_txs = head[2], n_genes = head[3], has_status = head[4];
  const uint32_t flags = (uint32_t)head[5], cb_len = (uint32_t)head[6], umi_len = (uint32_t)head[7], min_umis = (uint32_t)head[8];
  const uint64_t n_name_bytes = head[9];
  const auto off = in.take<uint64_t>(n_reads + 1);
  const auto alns = in.take<thm_aln>(n_alns);
  const auto tx_gene = in.take<uint32_t>(n_txs);
  const auto name_off = in.take<uint64_t>(n_reads + 1);
  const auto status = in.take<int32_t>(has_status ? n_reads : 0);
  const auto names = in.take<uint8_t>(n_name_bytes);
  if (!in.ok || in.at != in.bytes.size() || cb_len < 1 || cb_len > 16 || umi_len < 1 || umi_len > 16 || min_umis < 1) return 2;
  if (off[0] != 0 || off[n_reads] != n_alns || name_off[0] != 0 || name_off[n_reads] != n_name_bytes) return 2;

  // classify, and the keys of the counted reads reduced by key: (barcode, lo) -> reads
  uint64_t tot[cells::N_TOTALS] = {0};
  std::map<std::pair<uint32_t, uint64_t>, uint64_t> mol;
  for (uint64_t r = 0; r < n_reads; r++) {
    const uint64_t a0 = off[r], nh = off[r + 1] - a0;
    const bool ok = !has_status || status[r] == THM_OK;
    uint32_t gene = 0;
    int c = nh == 1 && a0 >= n_alns ? (int)cells::BAD_INDEX
                                    : cells::class_before_tag(ok, nh, alns.get() + a0, flags, tx_gene.get(), (uint32_t)n_txs, (uint32_t)n_genes, &gene);
    if (c == cells::BAD_INDEX) return 3;
    if (c == cells::T_COUNTED) {
      const uint64_t nb = name_off[r], ne = name_off[r + 1];
      uint32_t bc = 0, umi = 0;
      if (ne >= nb && cells::parse_tag(names.get(), nb, cells::qname_end(names.get(), nb, ne), cb_len, umi_len, &bc, &umi)) {
        const uint64_t hc = cells::key_hc(bc, 1u), lo = cells::key_lo(gene, umi, umi_len);
        if (cells::gene_of(lo, umi_len) != gene || cells::umi_of(lo, umi_len) != umi || cells::barcode_of(hc) != bc || cells::count_of(hc) != 1) return 2;
        if ((lo >> (cells::gene_bits((uint32_t)n_genes) + 2 * umi_len)) != 0) return 2;  // the sort's bits hold the key
        mol[{bc, lo}]++;
      } else {
        c = cells::T_UNTAGGED;
      }
    }
    tot[cells::T_READS]++;
    tot[c]++;
  }

  // the fetch: the map is the sorted table
  std::vector<thm_cell> cells_out;
  std::vector<thm_cell_entry> entries;
  std::vector<uint32_t> rows;
  uint64_t n_barcodes = 0;
  for (auto it = mol.begin(); it != mol.end();) {
    const uint32_t bc = it->first.first;
    auto end = it;
    uint64_t n_umis = 0;
    while (end != mol.end() && end->first.first == bc) ++end, ++n_umis;
    n_barcodes++;
    const bool keep = n_umis >= min_umis;
    thm_cell cell;
    memset(&cell, 0, sizeof cell);
    cell.barcode = bc;
    cell.n_umis = (uint32_t)n_umis;
    for (; it != end; ++it) {
      const uint32_t gene = cells::gene_of(it->first.second, umi_len);
      rows.insert(rows.end(), {bc, gene, cells::umi_of(it->first.second, umi_len), (uint32_t)it->second});
      if (!keep) continue;
      if (cell.n_genes == 0 || entries.back().gene != gene) {
        entries.push_back(thm_cell_entry{(uint32_t)cells_out.size(), gene, 0, 0});
        cell.n_genes++;
      }
      entries.back().n_umis++;
      entries.back().n_reads += (uint32_t)it->second;
      cell.n_reads += it->second;
    }
    if (keep) cells_out.push_back(cell);
  }
  // (the driver's barcode text, round trip)
  for (const thm_cell& c : cells_out) {
    char text[16];
    cells::unpack_bases(c.barcode, cb_len, text);
    uint32_t back = 0;
    if (!cells::pack_bases((const uint8_t*)text, 0, cb_len, &back) || back != c.barcode) return 2;
  }

  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  const uint64_t counts[5] = {mol.size(), n_barcodes, n_barcodes - cells_out.size(), cells_out.size(), entries.size()};
  fwrite(tot, 8, cells::N_TOTALS, o);
  fwrite(counts, 8, 5, o);
  if (!cells_out.empty()) fwrite(cells_out.data(), sizeof(thm_cell), cells_out.size(), o);
  if (!entries.empty()) fwrite(entries.data(), sizeof(thm_cell_entry), entries.size(), o);
  if (!rows.empty()) fwrite(rows.data(), 4, rows.size(), o);
  return fclose(o) == 0 ? 0 : 2;
}
