// lut_direct.h -- the text position kept in single-suffix entries of the device copy of the k-mer prefix table.
//
// An entry {lo, hi} of the table is the suffix-array interval of one kt-mer.  Where the interval holds one suffix, hi is
// lo + 1 and tells nothing, so the device copy keeps TAG | sa[lo] there instead: a probe that lands in such a bucket goes
// from the table entry straight to the text and skips the dependent read of the suffix array (kernels_seed.hip, ms_search).
// TAG is the top bit of the coordinate type.  A genuine hi is at most n, so the table is tagged only when n < TAG: no plain
// entry then has the bit set, and every stored position (< n) fits below it.  A 32-bit table over 2^31 symbols or more
// stays plain; with 64-bit coordinates n < 2^63 always holds.  The host tables, check_lut and the index file keep {lo, hi}.
//
// Plain functions, for the host too: tests/cpp/lut_direct_main.cpp runs them without a device (that file gives the
// sanitizer build line).
#ifndef THERMITE_LUT_DIRECT_H
#define THERMITE_LUT_DIRECT_H
#include <cstdint>

#if defined(__HIPCC__)
#define LUTD_HD __host__ __device__ inline
#else
#define LUTD_HD inline
#endif

namespace thm {
namespace lutd {

template <class C>
LUTD_HD constexpr C tag_bit() {
  return (C)((C)1 << (8 * sizeof(C) - 1));
}
// may the table over a text of n symbols be tagged?
template <class C>
LUTD_HD bool can_tag(uint64_t n) {
  return n < (uint64_t)tag_bit<C>();
}
// is {lo, hi} of the plain table an entry the pass rewrites?
template <class C>
LUTD_HD bool single_suffix(C lo, C hi) {
  return hi > lo && hi - lo == 1;
}
template <class C>
LUTD_HD C encode(C pos) {
  return (C)(tag_bit<C>() | pos);
}
// `hi` of a table that was tagged (never ask this of a plain table: can_tag decided that)
template <class C>
LUTD_HD bool is_tagged(C hi) {
  return (hi & tag_bit<C>()) != 0;
}
template <class C>
LUTD_HD C position(C hi) {
  return (C)(hi & (C)~tag_bit<C>());
}
// what a reader does right after loading {lo, hi}: true and the text position in *pos for a tagged entry, with hi set
// back to lo + 1; false and hi untouched otherwise (and always for a plain table)
template <class C>
LUTD_HD bool decode(bool table_tagged, C lo, C& hi, C* pos) {
  if (!table_tagged || !is_tagged(hi)) return false;
  *pos = position(hi);
  hi = (C)(lo + 1);
  return true;
}

}  // namespace lutd
}  // namespace thm
#endif
