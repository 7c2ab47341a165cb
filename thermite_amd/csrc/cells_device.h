// cells_device.h -- what the kernels of the cell-by-gene UMI matrix (kernels_cells.hip) do per read, each a plain function
// of the item it works on: where a name's QNAME ends, the barcode and UMI tag behind it and their packing, the class of a
// read (counted, or the total it falls into) with its gene, and the key of a molecule with what it unpacks to.  They
// compile for the host too: tests/cpp/cells_model_main.cpp drives the same functions serially, a std::map standing in for
// the sorts and the reduce-by-key, which is how the table is checked without a device -- and, under AddressSanitizer with
// name pools allocated to the byte, that no function reads outside the pool.  The contract is in include/thermite_io.h
// above thm_cells_create; DESIGN.md section 4.21 has the passes.
#ifndef THERMITE_CELLS_DEVICE_H
#define THERMITE_CELLS_DEVICE_H
#include <cstdint>

#include "../../include/thermite_io.h"

#if defined(__HIPCC__)
#define CELLS_HD __host__ __device__ inline
#else
#define CELLS_HD inline
#endif

namespace thm {
namespace cells {

// the totals of one batch, in the order of thm_cells_totals; a read's class is the total it counts in
enum { T_READS = 0, T_FAILED, T_UNMAPPED, T_MULTI, T_INTERGENIC, T_INTRONIC_SKIPPED, T_UNTAGGED, T_COUNTED, N_TOTALS };
static_assert(sizeof(thm_cells_totals) == N_TOTALS * 8, "the kernels index thm_cells_totals as an array");
constexpr int BAD_INDEX = -1;  // a class: the read's alignment has a type or an index outside the index's tables

// The end of the QNAME of the name [b, e) of the pool: the place of its first space, or e.  Reads bytes of [b, e) only.
CELLS_HD uint64_t qname_end(const uint8_t* names, uint64_t b, uint64_t e) {
  uint64_t q = b;
  while (q < e && names[q] != ' ') q++;
  return q;
}

// 2 bits of an upper-case base, or 4 for any other byte
CELLS_HD uint32_t base_code(uint8_t c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u; }

// n bases at names[at ...] packed, first base most significant; false where one is no upper-case A C G T
CELLS_HD bool pack_bases(const uint8_t* names, uint64_t at, uint32_t n, uint32_t* out) {
  uint32_t v = 0;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t c = base_code(names[at + i]);
    if (c > 3u) return false;
    v = v << 2 | c;
  }
  *out = v;
  return true;
}

// The tag of the QNAME [b, q): its last cb_len + umi_len + 2 bytes are '_', the barcode, '_', the UMI.  Reads bytes of
// [b, q) only, and none where the QNAME is shorter than a tag.
CELLS_HD bool parse_tag(const uint8_t* names, uint64_t b, uint64_t q, uint32_t cb_len, uint32_t umi_len, uint32_t* barcode, uint32_t* umi) {
  const uint64_t need = (uint64_t)cb_len + umi_len + 2;
  if (q - b < need) return false;
  const uint64_t t = q - need;
  if (names[t] != '_' || names[t + 1 + cb_len] != '_') return false;
  return pack_bases(names, t + 1, cb_len, barcode) && pack_bases(names, t + 2 + cb_len, umi_len, umi);
}

// a packed sequence of n bases back as text (the driver's barcodes.tsv)
CELLS_HD void unpack_bases(uint32_t v, uint32_t n, char* out) {
  for (uint32_t i = 0; i < n; i++) out[i] = "ACGT"[(v >> (2 * (n - 1 - i))) & 3u];
}

// The class of a read in front of its name: one of T_FAILED .. T_INTRONIC_SKIPPED, BAD_INDEX, or T_COUNTED with *gene
// where only the tag decides between T_COUNTED and T_UNTAGGED.  `al` is the read's first alignment (looked at with
// nh == 1 only).
CELLS_HD int class_before_tag(bool status_ok, uint64_t nh, const thm_aln* al, uint32_t flags, const uint32_t* tx_gene, uint32_t n_txs, uint32_t n_genes,
                              uint32_t* gene) {
  if (!status_ok) return T_FAILED;
  if (nh == 0) return T_UNMAPPED;
  if (nh > 1) return T_MULTI;
  const uint32_t type = al->aln_type, idx = al->tx_or_gene_idx;
  uint32_t g;
  if (type == THM_ALN_INTERGENIC) return T_INTERGENIC;
  if (type == THM_ALN_EXONIC) {
    if (idx >= n_txs) return BAD_INDEX;
    g = tx_gene[idx];
  } else if (type == THM_ALN_INTRONIC) {
    g = idx;
  } else {
    return BAD_INDEX;
  }
  if (g >= n_genes) return BAD_INDEX;
  if (type == THM_ALN_INTRONIC && !(flags & THM_CELLS_INTRONIC)) return T_INTRONIC_SKIPPED;
  *gene = g;
  return T_COUNTED;
}

// The key of a molecule, two words.  hc: the barcode in the low half, the row's count of reads in the high half -- rows
// are compared by the low half only.  lo: the gene above the UMI's 2 * umi_len bits.  Rows ascend by (barcode, gene,
// UMI).  The bits in use, for the sorts: the low 2 * cb_len of hc; the low gene_bits + 2 * umi_len (62 at the most) of
// lo.  (The barcode is the low half so that both sorts begin at bit 0: DESIGN.md section 4.21.)
CELLS_HD int gene_bits(uint32_t n_genes) {
  int b = 0;
  while (b < 32 && n_genes > (1ull << b)) b++;
  return b;  // ceil(log2 n_genes): every gene index is below 1 << b
}
CELLS_HD uint64_t key_hc(uint32_t barcode, uint32_t count) { return (uint64_t)count << 32 | barcode; }
CELLS_HD uint64_t key_lo(uint32_t gene, uint32_t umi, uint32_t umi_len) { return (uint64_t)gene << (2 * umi_len) | umi; }
CELLS_HD uint32_t barcode_of(uint64_t hc) { return (uint32_t)hc; }
CELLS_HD uint32_t count_of(uint64_t hc) { return (uint32_t)(hc >> 32); }
CELLS_HD uint32_t gene_of(uint64_t lo, uint32_t umi_len) { return (uint32_t)(lo >> (2 * umi_len)); }
CELLS_HD uint32_t umi_of(uint64_t lo, uint32_t umi_len) { return (uint32_t)(lo & ((1ull << (2 * umi_len)) - 1)); }
CELLS_HD bool same_molecule(uint64_t hc_a, uint64_t lo_a, uint64_t hc_b, uint64_t lo_b) { return barcode_of(hc_a) == barcode_of(hc_b) && lo_a == lo_b; }

}  // namespace cells
}  // namespace thm
#endif
