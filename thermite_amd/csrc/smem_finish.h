// smem_finish.h -- reads whose whole result follows from their SMEMs and a few index lookups.
//
// align_read (reference src/aligner.rs:123-190) extends every seed hit with two SwgExtend::extend calls per target.
// For two classes of reads the outcome of all of these calls is known before any of them runs, from the read's SMEMs,
// the contig record of the hit and the entries of the two interval grids:
//
//   class E (exact)   one SMEM, qpos 0, len == L, one occurrence at text position hr.
//   class S (one substitution between two SMEMs)
//                     two SMEMs [0, p) and [p + 1, L), one occurrence each, at rA and rB with rB - rA == p + 1.
//
// The functions below restate what extend_kernel (kernels_extend.hip) computes for such a read -- alignment record,
// op streams, counter increments -- or answer LEAVE, after which the read is extend_kernel's as before.  LEAVE is the
// answer to everything that is not covered by a proof in this file.  They are plain functions of scalars and of
// read-only tables, for the host too: tests/cpp/smem_finish_main.cpp runs them against the CPU oracle without a device.
//
// ---- class E ----
// Both extensions have an empty x.  SwgExtend::extend returns the empty result for an empty x whatever y is
// (src/swg.rs:39-55; swg_extend_wave: broke = true, jmax = 0, no cells, no columns), so with the window clamped inside
// the contig copy ([hr, hr + L) within [ref.start, ref.end - 1), which the rule checks) the genome alignment is
// Match x L, score L, x [0, L), y [hr, hr + L): two calls, seq_end - seq_start window bytes (src/aligner.rs:212-215).
// exon_to_tx.find(hr, hr + L) then yields its entries in pre-order rank.  None: the read is unspliced.  Otherwise the
// first entry is looked at.  If the exon is the first of its transcript that meets the seed (prev_end <= hr) and holds
// the whole read (start <= hr, hr + L <= end), lift_mem_to_tx (src/txome.rs:82-103) moves the seed by the exon's offset
// without cutting it, extend_seed_match finds nothing to add (the seed is the whole read) and both extensions are
// empty again: score L, two more calls, the transcript window's bytes; the loop breaks at score >= L
// (src/aligner.rs:253-257), the read is exonic through this entry (best.score >= gx.score), and lift_tx_to_gx moves the
// ends back by the same offset with no intron (the alignment ends inside the exon, or on its last base with no clip
// behind it: xend == L).  A first entry of any other kind: LEAVE.
//
// ---- class S ----
// Let A = [0, p) at rA and B = [p + 1, L) at rB = rA + p + 1.  The hits are taken in the order of the read's SMEM run
// (the seed stage stores it in align_read's order: longer first, ties as sort_by_key + reverse leave them).
//   Hit A: the left x is empty; the right x is read[p .. L), y starts at text[rA + p].
//   Hit B: the right x is empty; the left x is read[p], read[p - 1], .. read[0], y starts at text[rB - 1] = text[rA + p].
// The non-empty extension of either hit is the shape swg_one_mismatch_shortcut (swg_device.h) answers without DP --
// Subst, Match x (|x| - 1), score |x| - 2, xend = yend = jmax = |x|, broke -- because
//   x[0] != y[0]:  A and B are SMEMs with one occurrence.  Were read[p] == text[rA + p], then [0, p + 1) would match at
//                  rA, and A would not be right-maximal (hit B: [p, L) would match at rB - 1, B not left-maximal).  The
//                  rule asks for read[p] in ACGT, so that the byte comparison of the kernel and the match relation of
//                  the seed stage are the same thing.
//   x[1..] == y[1..|x|):  for hit A this is read[p + 1 .. L) against text[rA + p + 1 .. rA + L) = text[rB .. rB + |B|): B's
//                  match, because the two SMEMs lie on one diagonal.  For hit B it is A's match, backwards.
//   |x| >= 3, |y| >= |x|, x_drop >= 1, x not one repeated base:  checked -- lengths and the contig clamp from the
//                  coordinates ([rA, rA + L) within [ref.start, ref.end - 1) makes L - p symbols available to the right
//                  of A and p + 1 to the left of B, and min(., |x| + bw + 1) never cuts below |x|), the bases from the read.
//                  (A flank of one repeated base cannot in fact have this shape: were read[p .. L) = b^(L-p), then [p, L - 1)
//                  would match at rB too, one diagonal over, a match of |B| bases that B does not contain -- a third SMEM.
//                  The rule checks the bases all the same: two byte compares for almost every read.)
// So both hits give the same alignment: Match x p, Subst, Match x (L - p - 1), score L - 2, x [0, L), y [rA, rA + L).
// Hit 1, if accepted, narrows band and X-drop to min(., L + range - (L - 2)) = min(., 2 + range) >= 1 for range >= 0 given
// x_drop >= 1 before: the shortcut's preconditions hold for hit 2 as well (the rule re-checks x_drop >= 1 per hit).
// Score L - 2 < L: the transcript loop of a hit does not break, every entry exon_to_tx.find yields for the hit's seed is
// evaluated.  Each must be by_coords in extend_kernel's sense -- first exon of its transcript that meets the seed, seed
// uncut, and every column the genome extensions looked at (jmax = |x|, i.e. the whole read) inside the exon -- then the
// transcript extension repeats the genome's: score L - 2, two calls, its window bytes.  The first yielded entry is the best
// (a later one is not strictly better, src/aligner.rs:249).  Any other entry: LEAVE.  An entry that holds the whole read
// overlaps both seeds, so the two hits see the same intervals in the same order; the rule still evaluates both lists and
// answers LEAVE if their sizes or first entries differ.  Both candidates are then accepted or both rejected; retain keeps
// both (equal scores), filter_overlapping's stable sort leaves them in push order and its sweep keeps the first (the second
// starts before max_end and is not strictly better): one alignment, hit 1's.
//
// ---- op streams ----
// Both classes' op streams are windows into one run of bytes, Match x H, Subst, Match x H (H >= the longest read of the
// fast class), kept read-only at the front of the candidate op pool: class E takes [0, L), class S [H - p, H - p + L); a
// reverse-strand contig reverses the genome stream (concat_to_chr_aln, src/aligner.rs:440-447), i.e. mirrors p.
#ifndef THERMITE_SMEM_FINISH_H
#define THERMITE_SMEM_FINISH_H
#include <cstdint>

#include "thermite_internal.h"

#if defined(__HIPCC__)
#define FIN_HD __host__ __device__ inline
#define FIN_UNROLL _Pragma("unroll")
#else
#define FIN_HD inline
#define FIN_UNROLL
#endif

namespace thm {
namespace fin {

constexpr uint32_t CLASS_E = 1u, CLASS_S = 2u;  // which classes a launch finishes
constexpr uint32_t MARK = 0xFFFFFFFFu;          // ReadRecT::len of a finished read: beyond every class, every later kernel passes over it
constexpr uint32_t MAX_GRID = 32;               // candidate entries of one grid query a thread walks; more: LEAVE
constexpr uint32_t MAX_RANGE = 1u << 20;        // multimap_score_range beyond this: LEAVE (the int arithmetic below stays small)

enum : int { LEAVE = 0, FINISHED = 1 };
enum : int { SHAPE_NONE = 0, SHAPE_E = 1, SHAPE_S = 2 };

// bytes of the shared op run for reads up to `half` bases (a multiple of 16: the pool's cursor starts behind it)
FIN_HD uint64_t run_bytes(uint32_t half) { return ((uint64_t)2 * half + 1 + 15) & ~15ull; }

// the complete outcome of a finished read
struct Outcome {
  int what;      // LEAVE | FINISHED
  int shape;     // the class whose SMEM shape the read has (counted as "left" when what == LEAVE)
  int accepted;  // alignments of the read: 0 or 1
  // the candidate (launch.h, Cand), when accepted
  uint64_t ystart, yend, ylen;
  uint64_t tx_ystart, tx_yend, tx_ylen;
  uint32_t ops_off, tx_ops_off;  // windows of the shared run, ops_len == tx_ops_len == L (tx: exonic only)
  int32_t score;
  uint32_t ref_id, name_rank, type_idx;
  uint8_t strand, aln_type;
  // counter increments of the read (reads += 1, aligned / unmapped and alns follow from `accepted`, the type from aln_type)
  uint32_t calls, window_bytes, op_bytes;
};

// thresholds of align_read, src/aligner.rs:130-138 (binary32 product, truncation toward zero), and the state the hit
// loop starts from
struct Setup {
  int min_aln_score, band, x_drop, range;
  bool intron_mode;
  bool ok;  // false: band_bad in extend_kernel's sense (the read gets a status there), or options outside the rules
};
FIN_HD Setup setup(const thm_align_opts& o, int L, uint32_t max_bw, int cpl) {
  Setup s;
  const float prod = o.min_aln_score_percent * (float)L;
  const int ms_pct = (prod != prod) ? 0 : (prod >= 2147483648.0f ? 2147483647 : (prod <= -2147483648.0f ? (-2147483647 - 1) : (int)prod));
  s.min_aln_score = ms_pct > o.min_aln_score ? ms_pct : o.min_aln_score;
  s.band = (s.min_aln_score < 0) ? 0 : (L - s.min_aln_score > 0 ? L - s.min_aln_score : 0);
  s.x_drop = s.band;
  s.range = (int)(o.multimap_score_range > MAX_RANGE ? MAX_RANGE : o.multimap_score_range);
  s.intron_mode = o.intron_mode != 0;
  s.ok = o.multimap_score_range <= MAX_RANGE && !((uint32_t)s.band > max_bw || (cpl > 0 && 2 * s.band + 1 > 64 * cpl));
  return s;
}

// Index::idx_to_ref (src/index.rs:287-290) the way extend_kernel answers it: the contig copy of the bin's first symbol,
// then forward over the boundaries inside the bin
template <class C>
FIN_HD uint32_t ref_of(uint32_t bin_first, const RefRecT<C>* ref_recs, uint32_t n_refs, C idx, RefRecT<C>& r) {
  uint32_t lo = bin_first;  // ref_bin[idx >> GRID_SHIFT], loaded by the caller beside its other first-round loads
  r = ref_recs[lo];
  while (r.end <= idx && lo + 1 < n_refs) {
    lo++;
    r = ref_recs[lo];
  }
  return lo;
}

// Genome window of a hit (hr, len) under band bw, src/aligner.rs:212-215: its bytes for THM_CNT_WINDOW_BYTES.  False:
// the alignment [a0, a0 + L) is not inside the contig copy without its '$' -- a clamp the rules do not cover -- or the
// window arithmetic of the 32-bit kernel would leave its signed range.
template <class C>
FIN_HD bool genome_window(C hr, int len, int L, int bw, const RefRecT<C>& ref, C a0, uint32_t& bytes) {
  if (a0 < ref.start || ref.end < 1 || (uint64_t)a0 + (uint64_t)L > (uint64_t)ref.end - 1) return false;
  if (sizeof(C) == 4 && (uint64_t)hr + (uint64_t)(len + L + bw) > 0x7fffffffull) return false;
  const int64_t h = (int64_t)hr, ext = (int64_t)(L + bw);
  int64_t seq_start = h > ext ? h - ext : 0;
  if (seq_start < (int64_t)ref.start) seq_start = (int64_t)ref.start;
  int64_t seq_end = h + (int64_t)len + ext;
  if (seq_end > (int64_t)ref.end - 1) seq_end = (int64_t)ref.end - 1;
  bytes = (uint32_t)(seq_end - seq_start);
  return true;
}

// extend_kernel's by_coords for a hit whose seed starts at qs and whose genome extensions looked at exactly the columns
// of the alignment [a0, a0 + L): this exon is the first of its transcript that meets the seed, and holds [a0, a0 + L)
// (which contains the seed, so lift_mem_to_tx does not cut it)
template <class C>
FIN_HD bool by_coords(const ExonEntryT<C>& e, C qs, C a0, int L) {
  return e.prev_end <= qs && e.start <= a0 && (uint64_t)a0 + (uint64_t)L <= (uint64_t)e.end;
}
// window of the transcript around the seed (hr, len) lifted through e, [seed - (L + bw), seed end + L + bw + 1) cut to the
// transcript: its bytes for THM_CNT_WINDOW_BYTES (counted whether or not a window is staged)
template <class C>
FIN_HD uint32_t tx_window_bytes(const ExonEntryT<C>& e, C hr, int len, int L, int bw) {
  const int tr = (int)(hr - e.start) + (int)e.txoff, tlen = (int)e.seq_len;
  const int ws = (tr > L + bw) ? tr - (L + bw) : 0;
  const int we = (tlen < tr + len + L + bw + 1) ? tlen : tr + len + L + bw + 1;
  return (uint32_t)(we - ws);
}

// rank of a grid entry in IntervalTree::find's yield order if it overlaps [qs, qe) and is the copy of its interval that
// counts for a query whose first bin is b0, else -1 (extend_device.h, grid_entry_rank)
template <class C>
FIN_HD int grid_rank(C start, C end, uint32_t rank, C qs, C qe, uint32_t b0) {
  const bool overlap = qs < end && start < qe;
  const uint32_t sb = (uint32_t)(start >> GRID_SHIFT), home = b0 > sb ? b0 : sb;
  const bool primary = (rank & 0xffu) == (home & 0xffu);
  return (overlap && primary) ? (int)(rank >> 8) : -1;
}

// The candidate entries of a grid query over [qs, qe): the lists of its first to last bin, side by side (e0, cnt); the two
// offsets are loaded before anything that depends on them, so that callers can ask for several spans and the contig
// record in one round trip.
struct GridSpan {
  uint32_t e0, cnt;
};
template <class C>
FIN_HD GridSpan grid_span(const uint32_t* off, C qs, C qe) {
  const uint32_t b0 = (uint32_t)(qs >> GRID_SHIFT), b1 = (uint32_t)((qe > qs ? qe - 1 : qs) >> GRID_SHIFT);
  GridSpan g;
  g.e0 = off[b0];
  g.cnt = off[b1 + 1] - g.e0;
  return g;
}

// What exon_to_tx.find yields for one seed [qs, qe) inside the alignment [a0, a0 + L), as the rules need it: how many
// entries, the first of them (smallest pre-order rank) with whether it is by_coords and its transcript window bytes, whether
// every entry is by_coords, and the window bytes of them all -- under band bw, and under the band bw_n the hit would see
// after a first accepted hit has narrowed it (class S, second hit).
template <class C>
struct ExonScan {
  C qs, qe;
  uint32_t b0;
  int bw, bw_n;
  uint32_t n, win_all, win_all_n;
  int best;
  bool all_by_coords;
  // the first yielded entry
  bool first_by_coords;
  uint32_t first_win;
  C first_start, first_end;
  uint32_t first_value, first_txoff, first_seq_len;
};
template <class C>
FIN_HD void scan_begin(ExonScan<C>& s, C qs, C qe, int bw, int bw_n) {
  s.qs = qs;
  s.qe = qe;
  s.b0 = (uint32_t)(qs >> GRID_SHIFT);
  s.bw = bw;
  s.bw_n = bw_n;
  s.n = s.win_all = s.win_all_n = 0;
  s.best = 0x7fffffff;
  s.all_by_coords = true;
  s.first_by_coords = false;
  s.first_win = 0;
  s.first_start = s.first_end = 0;
  s.first_value = s.first_txoff = s.first_seq_len = 0;
}
template <class C>
FIN_HD void scan_visit(ExonScan<C>& s, const ExonEntryT<C>& e, C a0, int L) {
  const int r = grid_rank<C>(e.start, e.end, e.rank, s.qs, s.qe, s.b0);
  if (r < 0) return;
  s.n++;
  const bool ok = by_coords<C>(e, s.qs, a0, L);
  const int len = (int)(s.qe - s.qs);
  uint32_t w = 0;
  if (ok) {
    w = tx_window_bytes<C>(e, s.qs, len, L, s.bw);
    s.win_all += w;
    s.win_all_n += tx_window_bytes<C>(e, s.qs, len, L, s.bw_n);
  } else {
    s.all_by_coords = false;
  }
  if (r < s.best) {
    s.best = r;
    s.first_by_coords = ok;
    s.first_win = w;
    s.first_start = e.start;
    s.first_end = e.end;
    s.first_value = e.value;
    s.first_txoff = e.txoff;
    s.first_seq_len = e.seq_len;
  }
}
// One pass over the candidates of the ALIGNMENT's span [a0, a0 + L) serves the seeds of both hits of a class-S read (s2
// null: one seed).  A seed's own bins are among the span's; a copy of an interval listed in another bin is not the copy that
// counts for the seed (grid_rank: its bin is not max(first bin of the seed, bin of the interval's start)), so each seed sees
// exactly what a query of its own would yield.  Four entries are in flight at a time.  False: more candidates than a thread walks.
template <class C>
FIN_HD bool exon_scan(const ExonEntryT<C>* grid, const GridSpan& g, C a0, int L, ExonScan<C>& s1, ExonScan<C>* s2) {
  if (g.cnt > MAX_GRID) return false;
  for (uint32_t i = 0; i < g.cnt; i += 4) {
    ExonEntryT<C> e[4];
    FIN_UNROLL
    for (uint32_t k = 0; k < 4; k++) e[k] = grid[g.e0 + (i + k < g.cnt ? i + k : g.cnt - 1)];
    FIN_UNROLL
    for (uint32_t k = 0; k < 4; k++) {
      if (i + k < g.cnt) {
        scan_visit<C>(s1, e[k], a0, L);
        if (s2) scan_visit<C>(*s2, e[k], a0, L);
      }
    }
  }
  return true;
}
// first interval gene_intervals.find(qs, qe) yields: 1 and its gene, 0 none, -1 more candidates than a thread walks
template <class C>
FIN_HD int gene_first(const GridEntryT<C>* grid, const GridSpan& g, C qs, C qe, uint32_t& gene) {
  if (g.cnt > MAX_GRID) return -1;
  const uint32_t b0 = (uint32_t)(qs >> GRID_SHIFT);
  int best = 0x7fffffff;
  for (uint32_t i = 0; i < g.cnt; i += 4) {
    GridEntryT<C> e[4];
    FIN_UNROLL
    for (uint32_t k = 0; k < 4; k++) e[k] = grid[g.e0 + (i + k < g.cnt ? i + k : g.cnt - 1)];
    FIN_UNROLL
    for (uint32_t k = 0; k < 4; k++) {
      const int r = (i + k < g.cnt) ? grid_rank<C>(e[k].start, e[k].end, e[k].rank, qs, qe, b0) : -1;
      if (r >= 0 && r < best) {
        best = r;
        gene = e[k].value;
      }
    }
  }
  return best != 0x7fffffff ? 1 : 0;
}

// The record of an accepted alignment of the whole read, x [0, L) on y [a0, a0 + L) of the concatenated text, score sc,
// with one Subst at read position p (p < 0: none): concat_to_chr_aln (src/aligner.rs:429-449) on the contig copy `ref`,
// the type from the first exon entry (exonic: through the first entry of scan e, lifted inside the exon) or from the gene grid.
template <class C>
FIN_HD void fill_record(Outcome& o, C a0, int L, int sc, int p, uint32_t half, const RefRecT<C>& ref, uint32_t ref_id,
                        bool exonic, const ExonScan<C>& e, bool have_gene, uint32_t gene) {
  const bool fwd = ref.strand != 0;
  const C cy0 = a0, cy1 = (C)(a0 + (C)L);
  if (fwd) {
    o.ystart = (uint64_t)(C)(cy0 - ref.start);
    o.yend = (uint64_t)(C)(cy1 - ref.start);
  } else {
    o.ystart = (uint64_t)(C)(ref.len - (C)(cy1 - ref.start));
    o.yend = (uint64_t)(C)(ref.len - (C)(cy0 - ref.start));
  }
  o.ylen = ref.len;
  o.score = sc;
  o.ref_id = ref_id;
  o.name_rank = ref.name_rank;
  o.strand = fwd ? 1 : 0;
  const int pg = (p < 0) ? -1 : (fwd ? p : L - 1 - p);  // the Subst's place in the (possibly reversed) genome stream
  o.ops_off = (pg < 0) ? 0u : half - (uint32_t)pg;
  o.tx_ops_off = 0;
  o.tx_ystart = o.tx_yend = o.tx_ylen = 0;
  o.op_bytes = (uint32_t)L;
  if (exonic) {
    o.aln_type = THM_ALN_EXONIC;
    o.type_idx = e.first_value;
    o.tx_ystart = (uint64_t)(a0 - e.first_start) + e.first_txoff;
    o.tx_yend = o.tx_ystart + (uint64_t)L;
    o.tx_ylen = e.first_seq_len;
    o.tx_ops_off = (p < 0) ? 0u : half - (uint32_t)p;
    o.op_bytes = 2u * (uint32_t)L;
  } else if (have_gene) {
    o.aln_type = THM_ALN_INTRONIC;
    o.type_idx = gene;
  } else {
    o.aln_type = THM_ALN_INTERGENIC;
    o.type_idx = THM_NO_IDX;
  }
}

// the tables of the index the rules read (DeviceIndexT's members, or host copies of them)
template <class C>
struct Tables {
  const uint32_t* ref_bin;
  const RefRecT<C>* ref_recs;
  uint32_t n_refs;
  const uint32_t* exon_grid_off;
  const ExonEntryT<C>* exon_grid;
  const uint32_t* gene_grid_off;
  const GridEntryT<C>* gene_grid;
};

// does the read have class E's shape?  (one SMEM over the whole read, one occurrence)
FIN_HD bool shape_exact(uint32_t smem_cnt, uint32_t n_hits, uint32_t qpos0, uint32_t len0, uint64_t occ0, uint32_t L) {
  return smem_cnt == 1 && n_hits == 1 && occ0 == 1 && qpos0 == 0 && len0 == L && L > 0;
}

// ---- class E: hr = the occurrence ----
template <class C>
FIN_HD Outcome finish_exact(const Tables<C>& ix, C hr, int L, const Setup& st, uint32_t half) {
  Outcome o;
  o.what = LEAVE;
  o.shape = SHAPE_E;
  o.accepted = 0;
  o.calls = o.window_bytes = o.op_bytes = 0;
  if (!st.ok || (uint32_t)L > half) return o;
  // first round of loads, all from the hit's position: the contig copy of its bin, the spans of the two grid queries (the
  // gene query is needed for an unspliced read in intron mode only)
  const C qe = (C)(hr + (C)L);
  const uint32_t bin_first = ix.ref_bin[hr >> GRID_SHIFT];
  const GridSpan es = grid_span<C>(ix.exon_grid_off, hr, qe);
  GridSpan gs;
  gs.e0 = gs.cnt = 0;
  if (st.intron_mode) gs = grid_span<C>(ix.gene_grid_off, hr, qe);
  RefRecT<C> ref;
  const uint32_t ref_id = ref_of<C>(bin_first, ix.ref_recs, ix.n_refs, hr, ref);
  ExonScan<C> e;
  scan_begin<C>(e, hr, qe, st.band, st.band);
  if (!exon_scan<C>(ix.exon_grid, es, hr, L, e, nullptr)) return o;
  uint32_t gwin = 0;
  if (!genome_window<C>(hr, L, L, st.band, ref, hr, gwin)) return o;
  o.calls = 2;
  o.window_bytes = gwin;
  const bool exonic = e.n > 0;
  if (exonic) {
    if (!e.first_by_coords) return o;  // the first target needs its window: extend_kernel's
    o.calls += 2;
    o.window_bytes += e.first_win;
  }
  // back in align_read's loop (src/aligner.rs:146-174): score L against min_aln_score (= max_aln_score so far)
  const bool accept = (st.intron_mode || exonic) && L >= st.min_aln_score && L >= st.min_aln_score - st.range;
  uint32_t gene = 0;
  bool have_gene = false;
  if (accept && !exonic) {
    const int g = gene_first<C>(ix.gene_grid, gs, hr, qe, gene);
    if (g < 0) return o;
    have_gene = g > 0;
  }
  o.what = FINISHED;
  if (accept) {
    o.accepted = 1;
    fill_record<C>(o, hr, L, L, -1, half, ref, ref_id, exonic, e, have_gene, gene);
  }
  return o;
}

// one seed hit as align_read meets it
template <class C>
struct Hit {
  C hr;
  uint32_t q, len;
};
// does the read have class S's shape?  (two SMEMs with one occurrence each, [0, p) and [p + 1, L), on one diagonal);
// p and the alignment's start come back
template <class C>
FIN_HD bool shape_subst(uint32_t smem_cnt, uint32_t n_hits, uint64_t occ1, uint64_t occ2, const Hit<C>& h1, const Hit<C>& h2, uint32_t L,
                        int& p, C& a0) {
  if (smem_cnt != 2 || n_hits != 2 || occ1 != 1 || occ2 != 1) return false;
  const bool first_is_a = h1.q == 0;
  const Hit<C>& A = first_is_a ? h1 : h2;
  const Hit<C>& B = first_is_a ? h2 : h1;
  if (A.q != 0 || A.len == 0 || B.q != A.len + 1 || B.len == 0 || B.q + B.len != L) return false;
  if (B.hr <= A.hr || (uint64_t)(B.hr - A.hr) != (uint64_t)A.len + 1) return false;
  p = (int)A.len;
  a0 = A.hr;
  return true;
}
FIN_HD bool is_acgt(uint8_t b) { return b == 'A' || b == 'C' || b == 'G' || b == 'T'; }

// the state align_read carries from hit to hit, and what the hits of a class-S read have added to the counters
struct SubstState {
  int bw, xd, max_score;
  uint32_t calls, win, n_acc;
};
// one hit of a class-S read under the state in force, from the scan of its seed (`narrowed`: the state is what a first
// accepted hit left, the scan's second set of window bytes applies); false: LEAVE
template <class C>
FIN_HD bool subst_hit(const Hit<C>& h, C a0, int L, const RefRecT<C>& ref, const Setup& st, SubstState& ss, const ExonScan<C>& scan, bool narrowed,
                      bool& acc) {
  const int sc = L - 2;
  if (ss.xd < 1) return false;  // the shortcut's precondition; the DP then decides, in extend_kernel
  uint32_t gwin = 0;
  if (!genome_window<C>(h.hr, (int)h.len, L, ss.bw, ref, a0, gwin)) return false;
  if (!scan.all_by_coords) return false;
  ss.calls += 2 + 2 * scan.n;
  ss.win += gwin + (narrowed ? scan.win_all_n : scan.win_all);
  const bool exonic = scan.n > 0;
  acc = (st.intron_mode || exonic) && sc >= st.min_aln_score && sc >= ss.max_score - st.range;
  if (acc) {
    ss.n_acc++;
    const int lim = L + st.range - sc > 0 ? L + st.range - sc : 0;  // src/aligner.rs:162-172
    ss.bw = ss.bw < lim ? ss.bw : lim;
    ss.xd = ss.xd < lim ? ss.xd : lim;
    ss.max_score = ss.max_score > sc ? ss.max_score : sc;
  }
  return true;
}

// ---- class S: h1, h2 in the order of the read's SMEM run; rd = the read's sanitised bases ----
template <class C>
FIN_HD Outcome finish_subst(const Tables<C>& ix, const uint8_t* rd, const Hit<C>& h1, const Hit<C>& h2, int L, int p, C a0, const Setup& st,
                            uint32_t half) {
  Outcome o;
  o.what = LEAVE;
  o.shape = SHAPE_S;
  o.accepted = 0;
  o.calls = o.window_bytes = o.op_bytes = 0;
  if (!st.ok || (uint32_t)L > half) return o;
  // |x| >= 3 for both non-empty extensions: |x| = L - p to the right of A, p + 1 to the left of B
  if (L - p < 3 || p + 1 < 3) return o;
  // the substituted base, and neither x one repeated base: some base of [p + 1, L) and some base of [0, p) differ from it
  const uint8_t c = rd[p];
  if (!is_acgt(c)) return o;
  {
    int t = p + 1;
    while (t < L && rd[t] == c) t++;
    if (t == L) return o;
    t = p - 1;
    while (t >= 0 && rd[t] == c) t--;
    if (t < 0) return o;
  }
  // first round of loads (as in finish_exact), over the alignment's span
  const C ae = (C)(a0 + (C)L);
  const uint32_t bin_first = ix.ref_bin[h1.hr >> GRID_SHIFT];
  const GridSpan es = grid_span<C>(ix.exon_grid_off, a0, ae);
  GridSpan gs;
  gs.e0 = gs.cnt = 0;
  if (st.intron_mode) gs = grid_span<C>(ix.gene_grid_off, a0, ae);
  RefRecT<C> ref;
  const uint32_t ref_id = ref_of<C>(bin_first, ix.ref_recs, ix.n_refs, h1.hr, ref);
  SubstState ss;
  ss.bw = st.band;
  ss.xd = st.x_drop;
  ss.max_score = st.min_aln_score;
  ss.calls = ss.win = ss.n_acc = 0;
  const int sc = L - 2;
  // the band hit 2 sees if hit 1 is accepted (src/aligner.rs:162-172 with score L - 2)
  const int lim = 2 + st.range;
  const int bw_n = st.band < lim ? st.band : lim;
  ExonScan<C> s1, s2;
  scan_begin<C>(s1, h1.hr, (C)(h1.hr + (C)h1.len), st.band, st.band);
  scan_begin<C>(s2, h2.hr, (C)(h2.hr + (C)h2.len), st.band, bw_n);
  if (!exon_scan<C>(ix.exon_grid, es, a0, L, s1, &s2)) return o;
  bool acc1 = false, acc2 = false;
  if (!subst_hit<C>(h1, a0, L, ref, st, ss, s1, false, acc1)) return o;
  if (!subst_hit<C>(h2, a0, L, ref, st, ss, s2, acc1, acc2)) return o;
  const uint32_t n_acc = ss.n_acc;
  // the two hits see the same intervals (see the head of the file); anything else is not this rule's
  if (s1.n != s2.n || acc1 != acc2) return o;
  const bool exonic = s1.n > 0;
  if (exonic && (s1.best != s2.best || s1.first_start != s2.first_start || s1.first_end != s2.first_end || s1.first_value != s2.first_value)) return o;
  uint32_t gene = 0;
  bool have_gene = false;
  if (n_acc && !exonic) {
    const int g = gene_first<C>(ix.gene_grid, gs, a0, ae, gene);
    if (g < 0) return o;
    have_gene = g > 0;
  }
  o.what = FINISHED;
  o.calls = ss.calls;
  o.window_bytes = ss.win;
  if (n_acc) {
    o.accepted = 1;
    fill_record<C>(o, a0, L, sc, p, half, ref, ref_id, exonic, s1, have_gene, gene);
  }
  return o;
}

}  // namespace fin
}  // namespace thm
#endif
