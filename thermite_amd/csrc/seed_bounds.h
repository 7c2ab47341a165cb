// seed_bounds.h -- which inner positions of a grid cell of the seed stage still need a probe, decided from what the
// probes at the cell's two grid points found (kernels_seed.hip: seed_grid_cells_kernel, seed_fill_kernel).
//
// Terms.  rd[0..L) is the sanitised read (bytes outside ACGTN are 0, lower case is upper case).  "Match" is what lcp_cmp
// computes: byte equality of the read with the text, never past the read's end L.  MS[i] is the longest match of
// rd[i..L) anywhere in the text, E[i] = i + MS[i] its end, k the minimum seed length, kt the width of the k-mer table.
// The row of ends holds ms_end[i] = E[i] where MS[i] >= k and 0 otherwise; position i starts an SMEM iff ms_end[i] != 0
// and ms_end[i] > ms_end[i - 1].
//
// (M) E never decreases.  If rd[i..E[i]) occurs in the text at t and MS[i] >= 1, then rd[i+1..E[i]) occurs at t + 1: a
//     suffix of an occurrence is an occurrence, because the comparison is plain byte equality.  So MS[i+1] >= MS[i] - 1
//     and E[i+1] >= E[i]; with MS[i] = 0, E[i+1] >= i + 1 > E[i].  Nothing here asks for MS >= k.
//
// What a probe knows.  ms_search returns d and the interval [lo, hi).
//   * Empty bucket: the kt-mer rd[pos..pos+kt) is all ACGT, kt <= k, and its table entry is empty (lo == hi).  Then no
//     text position starts with the kt-mer, so MS[pos] < kt, and that is all that is known: d comes back as 0.  Only this
//     case is inexact: pos <= E[pos] <= pos + kt - 1.  It is also the only way ms_search ends with lo == hi: the table
//     path starts from the entry, every other path from [0, n) with n > 0, and no later step empties an interval (each
//     takes the run of suffixes that attain a maximum, or leaves [lo, hi) alone).
//   * Every other return has d == MS[pos] exactly, also below k; by case:
//       - Read end.  A probed position has pos + k <= L and the table path needs kt <= k, so the kt-mer lies inside the
//         read.  Every compare is capped at cap = L - (pos + d): d never counts a byte at or behind L, and where
//         pos + d == L already nothing is compared and d = L - pos, which no match can exceed.
//       - A byte outside ACGTN is 0 in the read and no text byte is 0.  With one suffix left lcp_cmp stops on it; with
//         more, `q[0] != 0` fails and the interval stays at depth d: in both cases d bytes matched and the next cannot.
//       - N against N is byte equality like any other: N is a text symbol, lcp_cmp and the suffix order treat it as one.
//         A kt-mer with an N skips the table (next item), so the table never has to hold it.
//       - '$' (contig ends, the text's end) never occurs in a sanitised read, so every match stops in front of it: it is
//         a mismatch like a substitution, found by the same compare.  The padding behind the text is never reached, the
//         text ends in '$'.
//       - kt > k, or a kt-mer with a byte outside ACGT: the table is not consulted, the search starts from [0, n) at
//         depth 0 and is the plain longest-match search over the whole suffix array -- exact.
//       - One suffix in the interval (from the table entry, with or without the text position kept in it: lut_direct.h):
//         every match of rd[pos..) of kt or more bytes starts with the kt-mer, hence at that suffix; d = kt + lcp.
//       - Up to 8 suffixes: the lcp of each with the query tail is taken (8 bytes, then lcp_cmp for those that agree on
//         all 8), d += the maximum -- the longest match among all text positions that share the first d bytes.
//       - Binary search: the insertion point a of the query tail among the suffixes of [lo, hi) (which agree with the
//         query on d bytes and are sorted by byte order behind them); the longest common prefix of a string with a sorted
//         list is attained at a neighbour of its insertion point, so max(l1, l2) is the maximum over the interval.
//       - MS_DECIDED: d = known_end - pos, shown exact where ms_search takes that return (one suffix in the bucket, the
//         neighbour's match covers the kt-mer).
//   probe_bound() turns (pos, d, empty, kt, L) into la <= E[pos] <= ub, la == ub == E[pos] when exact.
//
// Position 0 is probed by seed_first_kernel, which leaves only ms_end[0]: where that is not 0 it is E[0] (exact), where
// it is 0 the trivial la = 0 <= E[0] is used.  Position 0 is never the right end of a cell, so its ub is not needed.
//
// The rule.  Cell [a, b], both grid points probed, la <= E[a] and E[b] <= ub.  For a < i < b, (M) gives
// la <= E[a] <= E[i] <= E[b] <= ub.
//   1. ub - i < k:  MS[i] = E[i] - i <= ub - i < k, so ms_end[i] = 0.  No SMEM starts at i.
//   2. else la == ub:  E[i] = la, MS[i] = la - i >= k, so ms_end[i] = la.  And E[i - 1] = la too (i - 1 >= a), with
//      MS[i - 1] = MS[i] + 1 >= k, so ms_end[i - 1] = la: no SMEM starts at i and its interval is never read.
//      (ea != 0 && ea == eb, the rule the cells kernels had before, is the case la = ea, ub = eb, ub - b >= k.)
//   3. else i is probed.
// Case 1 holds for every i > ub - k, so the probed positions of a cell are its leftmost ones, a < i <= min(b - 1, ub - k),
// and none when la == ub.  cell_mask() returns them as a bit mask, decided_end() the end of a position that is not in it.
//
// The first cell (a == 0) takes case 2 only in the form the cells kernels had before: both stored ends agree, i.e.
// la == ub and MS[b] >= k as well.  Where position 0 has a match of k or more that ends inside or just behind the cell
// (la == ub, MS[b] < k), its positions i <= ub - k are still probed.  Nothing in the proof asks for this.  Those probes
// are the ones a read of fewer than k + 2 * 8 bases has for the table-entry shortcut of ms_search (the hint is E[0],
// one table read each where the bucket holds one suffix), and tests/test_gpu_seed_infer.py pins that the shortcut
// decides probes of such reads (one_sub_L29).  On 91-base reads it keeps about a quarter of a probe per read.
//
// Plain functions, for the host too: tests/cpp/seed_bounds_main.cpp runs them without a device (that file gives the
// sanitizer build line).
#ifndef THERMITE_SEED_BOUNDS_H
#define THERMITE_SEED_BOUNDS_H
#include <cstdint>

#if defined(__HIPCC__)
#define SBD_HD __host__ __device__ inline
#else
#define SBD_HD inline
#endif

namespace thm {
namespace sbd {

constexpr int STRIDE = 8;  // grid stride of the seed stage (PROBE_STRIDE): a cell has at most STRIDE - 1 inner positions

// la <= E[pos] <= ub from what ms_search returned for pos: its d, and `empty`: the table path found an empty bucket
SBD_HD void probe_bound(int pos, int d, bool empty, int kt, int L, int& la, int& ub) {
  if (empty) {
    la = pos;
    ub = pos + kt - 1 < L ? pos + kt - 1 : L;
  } else {
    la = ub = pos + d;
  }
}
// the same for position 0, of which only the stored end is left (0: MS[0] < k)
SBD_HD int first_lower_bound(int stored_end) { return stored_end; }

// bit j (1 <= j < b - a): position a + j needs a probe.  b - a <= STRIDE.
SBD_HD unsigned cell_mask(int a, int b, int la, int ub, int k) {
  if (la == ub && (a != 0 || ub - b >= k)) return 0u;  // (the first cell: only where the stored ends agree, see above)
  int n = ub - k - a;  // positions a + 1 .. ub - k can still have MS >= k
  if (n > b - a - 1) n = b - a - 1;
  return n > 0 ? ((1u << n) - 1u) << 1 : 0u;
}
// the stored end of an inner position i of the cell that cell_mask() does not list
SBD_HD int decided_end(int i, int la, int ub, int k) { return (ub - i < k) ? 0 : la; }

}  // namespace sbd
}  // namespace thm
#endif
