// launch_io.h -- parameter blocks and launch wrappers of the kernels behind the file-level entry points (BAM, BGZF, BAM
// sort, the run summaries, BAI, FASTQ, inflate, gzip): what the alignment pipeline itself never sees.  The pipeline's are in launch.h.
#ifndef THERMITE_LAUNCH_IO_H
#define THERMITE_LAUNCH_IO_H

#include "launch.h"

namespace thm {

// workgroups of 256 threads for n items, a thread each
inline unsigned blocks256(uint64_t n) { return (unsigned)((n + 255) / 256); }

// ---- BAM records on the device (kernels_bam.hip; host side bam.hip) ----
// prep (per read: record count, QNAME length) -> scan -> size (per record: its read, its bytes) -> scan -> emit (one
// wavefront per record) -> offsets (per read: first byte).  `err` collects the conditions that fail the call.
constexpr uint32_t THM_BAM_FLAG_NO_ANNOTATION = 1u;  // THM_BAM_NO_ANNOTATION_TAGS, include/thermite_io.h
constexpr unsigned BAM_ERR_QNAME = 1u, BAM_ERR_CIGAR_WORDS = 2u, BAM_ERR_DIGEST_FLAGS = 4u, BAM_ERR_RANGE = 8u;
struct BamParams {
  uint64_t n_reads, n_rec;
  uint32_t flags;
  uint32_t n_refs, n_txs, n_genes;
  // the batch: raw reads, qualities (null: none), names
  const uint8_t* bases;
  const uint64_t* offsets;
  const uint8_t* quals;
  const uint8_t* names;
  const uint64_t* name_off;
  // the run: compacted records, their digests and CIGAR words
  const uint64_t* aln_off;
  const thm_aln* alns;
  const thm_aln_digest* digests;
  const uint32_t* words;
  uint64_t n_words;
  // the index's names: string pools with offsets, gene of every transcript, @SQ index (BAM refID) of every ref
  const uint8_t *tx_pool, *gid_pool, *gname_pool;
  const uint32_t *tx_off, *gid_off, *gname_off;
  const uint32_t* tx_gene;
  const int32_t* ref_sq;
  // work and results
  uint64_t* rec_cnt;          // [n_reads]      prep
  const uint64_t* rec_first;  // [n_reads + 1]  scan of rec_cnt
  uint32_t* qn;               // [n_reads]      prep
  uint32_t* rec_read;         // [n_rec]        size
  uint64_t* rec_len;          // [n_rec]        size
  const uint64_t* rec_off;    // [n_rec + 1]    scan of rec_len
  uint8_t* out;               // [rec_off[n_rec]]
  uint64_t* read_rec_off;     // [n_reads + 1]
  unsigned int* err;
};
hipError_t launch_bam_prep(const BamParams& p, hipStream_t s);
hipError_t launch_bam_size(const BamParams& p, hipStream_t s);
hipError_t launch_bam_emit(const BamParams& p, bool stage, int n_cu, hipStream_t s);
hipError_t launch_bam_offsets(const BamParams& p, hipStream_t s);

// ---- BGZF members on the device (kernels_bgzf.hip, bgzf_device.h; host side bgzf.hip) ----
// deflate (one workgroup per block of 0xff00 input bytes: a complete member into the block's slot, its size) -> scan of
// the sizes (launch_exclusive_scan_u64) -> compact (the members behind one another).
struct BgzfParams {
  const uint8_t* in;  // [n], 4-byte aligned
  uint64_t n, n_blocks;
  uint32_t* match;      // [bgzf_grid(n_blocks, n_cu) * 0xff00]  per-position scratch of the workgroups
  uint8_t* slots;       // [n_blocks * 65536]
  uint64_t* sizes;      // [n_blocks]      deflate
  const uint64_t* off;  // [n_blocks + 1]  scan of sizes
  uint8_t* out;         // [off[n_blocks]], 4-byte aligned
};
unsigned bgzf_grid(uint64_t n_blocks, int n_cu);
hipError_t launch_bgzf_deflate(const BgzfParams& p, int n_cu, hipStream_t s);
hipError_t launch_bgzf_compact(const BgzfParams& p, int n_cu, hipStream_t s);

// ---- coordinate sort of a run's BAM records (kernels_bam_sort.hip, bam_sort_device.h; host side bam_sort.hip) ----
// keys (one thread per record of the batch just added: its key, length and place in the arena) ... sort of (key, ordinal)
// ... order (lengths and places by sorted ordinal; the caller scans the lengths) ... gather (a window of the sorted
// stream, 16 bytes a lane).
struct BamSortKeysParams {
  const uint8_t* data;  // the batch's records back to back
  const uint64_t* off;  // [n + 1] their offsets in `data`
  uint64_t n;
  uint32_t n_sq;
  uint64_t base;        // global arena offset of data[0]
  uint64_t* key;        // [n]  (the three arrays begin at the batch's first ordinal)
  uint32_t* len;        // [n]
  uint64_t* loc;        // [n]
};
struct BamSortGatherParams {
  const uint64_t* off;        // [n + 1] scan of the sorted lengths
  const uint64_t* loc;        // [n] global arena offset of every sorted record
  uint64_t n;
  const uint64_t* seg_start;  // [n_seg] global offset at which every arena segment begins, ascending from 0
  const uint8_t* const* seg;  // [n_seg] the segments, 4-byte aligned, 16 readable bytes behind their records
  uint32_t n_seg;
  uint64_t w0, w1;            // the window: w0 a multiple of 16, w0 < w1 <= off[n]
  uint8_t* out;               // [w1 - w0], 16-byte aligned
};
hipError_t launch_bam_sort_keys(const BamSortKeysParams& p, hipStream_t s);
hipError_t launch_bam_sort_iota(uint32_t* ord, uint64_t n, hipStream_t s);
hipError_t launch_bam_sort_order(const uint32_t* ord, const uint32_t* len, const uint64_t* loc, uint64_t n, uint64_t* s_len,
                                 uint64_t* s_loc, hipStream_t s);
// by_records: the record-centric shape (a wavefront per record), else the output-centric one (16 bytes a lane)
hipError_t launch_bam_sort_gather(const BamSortGatherParams& p, bool by_records, int n_cu, hipStream_t s);

// ---- what every summary of a run walks (quant, coverage, pileup, cells below; host side run_summary.h) ----
// The alignments of one batch on the device: the compacted records of the batch that is resident after thm_batch_run
// with the digests and words of the CIGAR passes, or the arrays of a caller's thm_cigar_view.  The batch structs of the
// summaries begin with it and add their own tables; they go to the kernels by value.
struct AlnBatch {
  uint64_t n_reads, n_alns, n_words;
  const uint64_t* aln_off;        // [n_reads + 1]
  const thm_aln* alns;            // [n_alns]
  const thm_aln_digest* digests;  // [n_alns]
  const uint32_t* words;          // [n_words]
  const int32_t* status;          // [n_reads]; null: no read failed
  uint32_t n_refs;
  const int32_t* ref_sq;          // [n_refs] BAM refID, -1: none
};

// ---- gene and junction count tables of a run (kernels_quant.hip, quant_device.h; host side quant.hip) ----
// count (per alignment: checks, its hits; per read: the read totals) -> scan -> extract (a row per hit) -> sort by the
// 128-bit key as two stable 64-bit passes over a permutation -> heads, scan, reduce (by key: sums and the maximum) ->
// lookup of the reduced rows in the running table, scan of the new ones -> update (found rows in place, new rows behind
// the table's) -> the same sort over table + new rows -> genes (last, so that a refused batch has added nothing).
struct QuantBatch : AlnBatch {
  uint32_t n_txs, n_genes;
  const uint32_t* tx_gene;        // [n_txs]
  const uint8_t* tx_forward;      // [n_txs] thm_tx::strand
};
// junction rows, one array per field: before the reduce a row is one hit (n_unique + n_multi == 1)
struct QuantRows {
  uint64_t *hi, *lo;  // the key (quant_device.h)
  uint64_t *n_unique, *n_multi;
  uint32_t* overhang;
};
struct QuantCountParams {
  QuantBatch b;
  uint64_t* hit_cnt;           // [n_alns + 1] hits of every alignment, for the scan
  uint8_t* multi;              // [n_alns] NH > 1
  unsigned long long* totals;  // [quant::N_TOTALS] zeroed by the caller
  unsigned long long* bad;     // the first alignment with an index out of range (atomic minimum; ~0: none)
};
struct QuantExtractParams {
  QuantBatch b;
  const uint64_t* hit_off;  // [n_alns + 1]
  const uint8_t* multi;
  QuantRows out;            // [hit_off[n_alns]]
};
struct QuantGenesParams {
  QuantBatch b;
  const uint8_t* multi;
  unsigned long long* genes;  // [n_genes * 4] the running table
};
struct QuantReduceParams {
  QuantRows in;          // [n] unsorted
  const uint32_t* perm;  // [n] sorted position -> row of `in`
  const uint64_t* s_hi;  // [n] the sorted high key words
  uint64_t n;
  uint64_t* flag;        // [n + 1] 1 where a key begins (heads kernel), and its exclusive scan
  const uint64_t* first;  // [n + 1]
  QuantRows out;         // [first[n]] sums and maxima zeroed by the caller
};
struct QuantMergeParams {
  QuantRows tab;   // [n_tab] the running table, sorted
  uint64_t n_tab;
  QuantRows red;   // [n_red] the batch's reduced rows
  uint64_t n_red;
  uint32_t* where;       // [n_red] row of `tab` with the same key, or 0xFFFFFFFF
  uint64_t* is_new;      // [n_red + 1] for the scan
  const uint64_t* new_at;  // [n_red + 1] its scan
  QuantRows cat;   // new rows go to cat[n_tab + new_at[j]]
};
hipError_t launch_quant_count(const QuantCountParams& p, int n_cu, hipStream_t s);
hipError_t launch_quant_extract(const QuantExtractParams& p, hipStream_t s);
hipError_t launch_quant_genes(const QuantGenesParams& p, int n_cu, hipStream_t s);
hipError_t launch_quant_gather(const uint64_t* in, const uint32_t* perm, uint64_t n, uint64_t* out, hipStream_t s);
hipError_t launch_quant_heads(const QuantReduceParams& p, hipStream_t s);
hipError_t launch_quant_reduce(const QuantReduceParams& p, hipStream_t s);
hipError_t launch_quant_lookup(const QuantMergeParams& p, hipStream_t s);
hipError_t launch_quant_update(const QuantMergeParams& p, hipStream_t s);
hipError_t launch_quant_rows(const QuantRows& in, uint64_t n, thm_quant_junction* out, hipStream_t s);

// ---- per-base coverage tracks of a run (kernels_coverage.hip, coverage_device.h; host side coverage.hip) ----
// add:   count (per alignment: its track, the checks, its blocks and bases; per read: the read totals) ... the host
//        reads the totals and the first bad alignment ... deposit (two integer adds per block).
// fetch: tiles (per tile of the range: the sum of its entries and the number of non-zero ones) -> two scans -> points
//        (per tile: a local scan plus the carry is the depth; (entry, depth) per change point) -> scan of the points with
//        a depth -> runs (a thread per change point pairs it with its successor).
// depth: tiles and the scan of the sums -> window (the local scan again, the depths of the window's entries).
struct CovBatch : AlnBatch {
  uint32_t n_sq, flags;           // flags: THM_COV_*
  const uint64_t* base;           // [n_sq + 1] first entry of every contig in a track (coverage_device.h)
};
struct CovCountParams {
  CovBatch b;
  uint8_t* track;              // [n_alns] the track an alignment deposits into, cov::NO_TRACK: none
  unsigned long long* totals;  // [cov::N_TOTALS] zeroed by the caller
  unsigned long long* bad;     // the first alignment that fails a check (atomic minimum; ~0: none)
};
struct CovDepositParams {
  CovBatch b;
  const uint8_t* track;
  uint32_t* diff;              // [n_tracks * track_entries]
  uint64_t track_entries;      // base[n_sq]
};
struct CovTileParams {
  const uint32_t* diff;        // the first entry of the range
  uint64_t n;                  // entries of the range
  uint64_t* tile_sum;          // [n_tiles + 1] tiles: the 32-bit sum of the tile's entries
  uint64_t* tile_cnt;          // [n_tiles + 1] tiles: its non-zero entries
  const uint64_t* carry;       // [n_tiles + 1] scan of tile_sum (its low 32 bits are the depth in front of the tile)
  const uint64_t* point_at;    // [n_tiles + 1] scan of tile_cnt
  uint64_t g0;                 // the range's first entry in the track
  uint64_t* point_entry;       // [n_points] points: the entry (in the track) of every change point
  uint32_t* point_depth;       // [n_points]
  uint64_t* point_live;        // [n_points + 1] 1 where the depth is not 0
};
struct CovRunParams {
  const uint64_t* point_entry;
  const uint32_t* point_depth;
  const uint64_t* run_at;      // [n_points + 1] scan of point_live
  uint64_t n_points;
  const uint64_t* base;
  uint32_t n_sq;
  thm_cov_run* runs;           // [run_at[n_points]]
  unsigned long long* stats;   // [3] zeroed: n_covered, n_bases, max_depth
};
struct CovWindowParams {
  const uint32_t* diff;        // the contig's first entry
  const uint64_t* carry;       // [n_tiles + 1] over the tiles of [0, start + n)
  uint64_t start, n;           // the window
  uint32_t* out;               // [n]
};
hipError_t launch_cov_count(const CovCountParams& p, int n_cu, hipStream_t s);
hipError_t launch_cov_deposit(const CovDepositParams& p, hipStream_t s);
hipError_t launch_cov_tiles(const CovTileParams& p, hipStream_t s);
hipError_t launch_cov_points(const CovTileParams& p, hipStream_t s);
hipError_t launch_cov_runs(const CovRunParams& p, hipStream_t s);
hipError_t launch_cov_window(const CovWindowParams& p, hipStream_t s);

// ---- per-base allele counts of a run (kernels_pileup.hip, pileup_device.h; host side pileup.hip) ----
// add:    count (a group of lanes per alignment: its read, whether it is used, the checks, its blocks, bases and events;
//         per read: the read totals) -> scan of the event counts ... the host reads the totals and the first bad
//         alignment ... extract (the group again: a key per event) -> sort of the keys -> heads, scan, runs (by key: key
//         and count) -> lookup of the reduced rows in the running table, scan of the new ones ... the host checks the cap
//         ... update (found rows in place, new rows behind the table's) -> sort of table + new rows -> deposit (two
//         integer adds per block into the difference array).
// fetch:  bounds (the range's rows) -> keep (the rows that begin a position with enough events) -> scan; coverage's tiles
//         and their scan -> sites (per tile with rows: the depths through LDS, a row per kept position).
// window: bounds, tiles and their scan -> window (per tile of the window: the depths, a row per position).
struct PileBatch : AlnBatch {
  const uint8_t* bases;           // the raw reads: read r is bases[base_off[r], base_off[r + 1])
  const uint64_t* base_off;       // [n_reads + 1]
  uint32_t n_sq, flags;           // flags: THM_PILE_*
  const uint64_t* base;           // [n_sq + 1] first entry of every contig in the layout (coverage_device.h)
  const uint64_t* tstart;         // [n_sq] first byte of every contig's forward copy in the text
  const uint8_t* text;
};
struct PileCountParams {
  PileBatch b;
  uint64_t* ev_cnt;            // [n_alns + 1] events of every alignment, for the scan
  uint64_t* aln_read;          // [n_alns] its read
  uint8_t* used;               // [n_alns] 1: it is walked and deposited
  unsigned long long* totals;  // [pile::N_TOTALS] zeroed by the caller
  unsigned long long* bad;     // the first alignment that fails a check (atomic minimum; ~0: none)
};
struct PileExtractParams {
  PileBatch b;
  const uint64_t* ev_off;      // [n_alns + 1] scan of ev_cnt
  const uint64_t* aln_read;
  const uint8_t* used;
  uint64_t* keys;              // [ev_off[n_alns]]
  uint32_t* diff;              // deposit: the difference array
};
struct PileReduceParams {
  const uint64_t* skey;        // [n] sorted keys
  uint64_t n;
  uint64_t* flag;              // [n + 1] heads: 1 where a key begins
  const uint64_t* first;       // [n + 1] its scan
  uint64_t* head_at;           // [n_keys + 1] runs: where every key begins in skey, and n behind them
  uint64_t* red_key;           // [n_keys]
  uint32_t* red_cnt;           // [n_keys]
  uint64_t n_keys;
};
struct PileMergeParams {
  const uint64_t* tab_key;     // [n_tab] the running table, sorted
  uint64_t n_tab;
  const uint64_t* red_key;     // [n_red] the batch's reduced rows
  const uint32_t* red_cnt;
  uint64_t n_red;
  uint64_t* where;             // [n_red] row of the table with the same key, or ~0
  uint64_t* is_new;            // [n_red + 1] for the scan
  const uint64_t* new_at;      // [n_red + 1] its scan
  uint64_t* dst_key;           // update: found rows add to dst_cnt[where], new rows go to row n_tab + new_at
  uint32_t* dst_cnt;
};
struct PileFetchParams {
  const uint64_t* keys;        // the table
  const uint32_t* cnts;
  uint64_t n_tab;
  uint64_t e0, e1;             // the entries of the range (a window: of the window)
  uint64_t* bounds;            // [2] bounds: the rows of the range, r0 and r1
  uint64_t r0, r1;             // ... read back
  uint32_t min_alt;
  uint64_t* keep;              // [r1 - r0 + 1] keep: 1 where a row begins a position with alt >= min_alt
  const uint64_t* site_at;     // [r1 - r0 + 1] its scan
  uint64_t n_sites;
  const uint32_t* diff;        // sites: the first entry of the range; window: of the contig
  uint64_t n;                  // entries the tiles count from there
  uint64_t g0;                 // that entry in the layout
  const uint64_t* carry;       // [n_tiles + 1] scan of the tile sums
  uint64_t start;              // window: its first position in the contig
  const uint64_t* base;
  const uint64_t* tstart;
  const uint8_t* text;
  uint32_t n_sq;
  thm_pile_site* sites;        // [n_sites]
};
hipError_t launch_pile_count(const PileCountParams& p, int n_cu, hipStream_t s);
hipError_t launch_pile_extract(const PileExtractParams& p, hipStream_t s);
hipError_t launch_pile_deposit(const PileExtractParams& p, hipStream_t s);
hipError_t launch_pile_heads(const PileReduceParams& p, hipStream_t s);
hipError_t launch_pile_runs(const PileReduceParams& p, hipStream_t s);
hipError_t launch_pile_lookup(const PileMergeParams& p, hipStream_t s);
hipError_t launch_pile_update(const PileMergeParams& p, hipStream_t s);
hipError_t launch_pile_bounds(const PileFetchParams& p, hipStream_t s);
hipError_t launch_pile_keep(const PileFetchParams& p, hipStream_t s);
hipError_t launch_pile_sites(const PileFetchParams& p, hipStream_t s);
hipError_t launch_pile_window(const PileFetchParams& p, hipStream_t s);

// ---- cell-by-gene UMI count matrix of a run (kernels_cells.hip, cells_device.h; host side cells.hip) ----
// add:   classify (a thread per read: its class, the tag of its name, its key and a flag; the totals) -> scan of the
//        flags ... the host reads the totals and the first bad alignment ... compact (the counted reads' keys) -> sort,
//        low word then high word, over the bits in use -> heads, scan, head_at, reduce (a row per molecule with its reads)
//        -> the rows go behind the pending ones, or table + pending + rows through the same sort and reduce.
// fetch: (pending rows merged as in add) levels (per row: begins a barcode, begins a (barcode, gene), its reads) -> three
//        scans -> starts (where every barcode and entry begins) -> barcodes (kept or not, its entries) -> two scans ->
//        cells, entries (the rows of the kept ones at their new numbers).
struct CellsBatch : AlnBatch {
  const uint8_t* names;           // read r's name is names[name_off[r], name_off[r + 1])
  const uint64_t* name_off;       // [n_reads + 1]
  uint32_t n_txs, n_genes;
  const uint32_t* tx_gene;        // [n_txs]
  uint32_t flags;                 // THM_CELLS_*
  uint32_t cb_len, umi_len;
};
struct CellsClassifyParams {
  CellsBatch b;
  uint64_t* counted;           // [n_reads + 1] 1: the read is counted, for the scan
  uint64_t *hc, *lo;           // [n_reads] the key of a counted read, its count 1
  unsigned long long* totals;  // [cells::N_TOTALS] zeroed by the caller
  unsigned long long* bad;     // the first alignment with a type or an index out of range (atomic minimum; ~0: none)
};
struct CellsCompactParams {
  uint64_t n_reads;
  const uint64_t* counted;     // [n_reads]
  const uint64_t* at;          // [n_reads + 1] its scan
  const uint64_t *hc, *lo;     // [n_reads]
  uint64_t *out_hc, *out_lo;   // [at[n_reads]]
};
struct CellsReduceParams {
  const uint64_t *hc, *lo;     // [n] sorted rows
  uint64_t n;
  uint64_t* flag;              // [n + 1] heads: 1 where a molecule begins
  const uint64_t* first;       // [n + 1] its scan
  uint64_t* head_at;           // [n_keys + 1] head_at: where every molecule begins, and n behind them
  uint64_t n_keys;
  uint32_t unit;               // 1: every row's count is 1 (a batch's reads): a molecule's count is its run's length
  uint64_t *out_hc, *out_lo;   // [n_keys] reduce
};
struct CellsFetchParams {
  const uint64_t *hc, *lo;     // [n] the table
  uint64_t n;
  uint32_t umi_len, min_umis;
  uint64_t *bflag, *eflag, *cnt;               // [n + 1] levels
  const uint64_t *b_at, *e_at, *pre;           // [n + 1] their scans
  uint64_t n_barcodes, n_all_entries;          // b_at[n], e_at[n]
  uint64_t *bc_start, *ent_start;              // [n_barcodes + 1], [n_all_entries + 1] starts
  uint64_t *keep, *kept_entries;               // [n_barcodes + 1] barcodes
  const uint64_t *cell_at, *ent_at;            // [n_barcodes + 1] their scans
  thm_cell* cells;                             // [cell_at[n_barcodes]]
  thm_cell_entry* entries;                     // [ent_at[n_barcodes]]
};
hipError_t launch_cells_classify(const CellsClassifyParams& p, int n_cu, hipStream_t s);
hipError_t launch_cells_compact(const CellsCompactParams& p, hipStream_t s);
hipError_t launch_cells_heads(const CellsReduceParams& p, hipStream_t s);
hipError_t launch_cells_head_at(const CellsReduceParams& p, hipStream_t s);
hipError_t launch_cells_reduce(const CellsReduceParams& p, hipStream_t s);
hipError_t launch_cells_levels(const CellsFetchParams& p, hipStream_t s);
hipError_t launch_cells_starts(const CellsFetchParams& p, hipStream_t s);
hipError_t launch_cells_barcodes(const CellsFetchParams& p, hipStream_t s);
hipError_t launch_cells_rows(const CellsFetchParams& p, hipStream_t s);

// ---- BAI index of the sorted stream (kernels_bai.hip, bai_device.h; host side bai.hip) ----
// fields (per sorted record: key = refID << 16 | bin, beg, end; per reference the mapped count and n_intv) -> run heads,
// scan, runs (the chunks before merging, raw offsets) -> sort of (key, ordinal) -> chunk and bin heads, two scans, chunks
// -> linear (atomic minima of raw offsets), the backward fill -> reference sizes, scan -> emit (the bytes of the file).
// Offsets are raw offsets of the sorted stream up to the emitter, which translates them with coff[].
struct BaiRecords {          // the sorted records: what thm_bam_sorter_finish left
  const uint64_t* off;       // [n + 1]
  const uint64_t* loc;       // [n]
  uint64_t n;
  const uint64_t* seg_start;
  const uint8_t* const* seg;
  uint32_t n_seg;
  uint32_t n_sq;
};
struct BaiFieldsParams {
  BaiRecords r;
  uint64_t* key;                     // [n]
  uint32_t* beg;                     // [n]  bai::MAPPED_BIT | beg
  uint32_t* end;                     // [n]  (saturated; a record beyond bai::MAX_END is in err[0])
  unsigned long long* ref_mapped;    // [n_sq] zeroed: mapped records
  unsigned long long* ref_intv;      // [n_sq] zeroed: n_intv
  unsigned long long* err;           // [2] all-ones: the first record with end > 2^29; the first whose CIGAR leaves it
};
struct BaiRunParams {
  const uint64_t* key;   // [n]
  const uint64_t* off;   // [n + 1]
  uint64_t n;
  uint32_t n_sq;
  uint64_t* flag;        // [n]      heads: 1 where a run begins
  const uint64_t* idx;   // [n + 1]  runs: scan of flag
  uint64_t *ref_first, *ref_end;  // [n_sq] zeroed: the records of every reference
  uint64_t* n_coor;      // [1] records with a reference
  uint64_t *run_key, *run_beg, *run_end;  // [n_runs]
};
struct BaiChunkParams {
  const uint64_t* skey;  // [n_runs] sorted
  const uint32_t* ord;   // [n_runs] the run each came from
  const uint64_t *run_beg, *run_end;
  uint64_t n_runs;
  uint32_t n_sq;
  uint64_t *chunk_flag, *bin_flag;       // [n_runs]      heads
  const uint64_t *chunk_idx, *bin_idx;   // [n_runs + 1]  chunks: their scans
  uint64_t *chunk_beg, *chunk_end;       // [n_chunks]
  uint32_t* chunk_bin;                   // [n_chunks] which bin (of all, in file order)
  uint64_t* bin_key;                     // [n_bins]
  uint64_t* bin_chunk0;                  // [n_bins + 1] first chunk of every bin
  uint64_t *ref_bin0, *ref_bin1;         // [n_sq] zeroed: the bins of every reference
};
struct BaiLinearParams {
  const uint64_t* key;
  const uint32_t *beg, *end;
  const uint64_t* off;
  uint64_t n;            // the records with a reference
  const uint64_t* intv_off;  // [n_sq + 1] scan of n_intv
  unsigned long long* table; // [intv_off[n_sq]] all-ones
  uint32_t n_sq;
};
struct BaiEmitParams {
  uint32_t n_sq;
  const uint64_t *ref_first, *ref_end, *ref_bin0, *ref_bin1;
  const unsigned long long *ref_mapped, *ref_intv;
  const uint64_t* intv_off;
  const unsigned long long* table;
  uint64_t* ref_size;        // [n_sq]       sizes
  const uint64_t* ref_at;    // [n_sq + 1]   emit: scan of ref_size (bai::HEAD_BYTES to be added)
  const uint64_t *bin_key, *bin_chunk0;
  const uint64_t *chunk_beg, *chunk_end;
  const uint32_t* chunk_bin;
  uint64_t n_chunks;
  const uint64_t* off;       // [n + 1] of the sorted records
  const uint64_t* coff;      // [n_members + 1]
  uint64_t n_no_coor, n_bytes;
  uint8_t* out;              // [n_bytes], 4-byte aligned
};
hipError_t launch_bai_fields(const BaiFieldsParams& p, hipStream_t s);
hipError_t launch_bai_run_heads(const BaiRunParams& p, hipStream_t s);
hipError_t launch_bai_runs(const BaiRunParams& p, hipStream_t s);
hipError_t launch_bai_chunk_heads(const BaiChunkParams& p, hipStream_t s);
hipError_t launch_bai_chunks(const BaiChunkParams& p, hipStream_t s);
hipError_t launch_bai_linear(const BaiLinearParams& p, hipStream_t s);
hipError_t launch_bai_fill(const BaiLinearParams& p, hipStream_t s);
hipError_t launch_bai_ref_sizes(const BaiEmitParams& p, hipStream_t s);
hipError_t launch_bai_emit(const BaiEmitParams& p, hipStream_t s);

// ---- FASTQ blocks parsed on the device (kernels_fastq.hip, fastq_device.h; host side fastq.hip) ----
// count (newlines per chunk) -> scan -> starts (line_start) -> records (the parse rule: lengths, or the flag) -> two
// scans (name_off, offsets) -> gather (names, bases, qualities to their places).
struct FastqParams {
  const uint8_t* raw;  // [n], 4-byte aligned, readable up to n + 4
  uint64_t n, n_chunks;        // n_chunks = ceil(n / fq::CHUNK)
  uint64_t* chunk_cnt;         // [n_chunks]      count
  const uint64_t* chunk_base;  // [n_chunks + 1]  scan of chunk_cnt
  uint64_t n_newlines, n_lines;
  uint64_t* line_start;        // [n_lines + 1]   starts
  uint64_t n_records;          // n_lines / 4
  uint64_t *name_len, *seq_len;  // [n_records]   records
  unsigned* flag;                // 0: every record passed; 1: the block is declined; 2: the line table is inconsistent
  const uint64_t *name_off, *offsets;  // [n_records + 1]  scans of name_len, seq_len
  uint8_t *names, *bases, *quals;      // gather
};
hipError_t launch_fastq_count(const FastqParams& p, int n_cu, hipStream_t s);
hipError_t launch_fastq_starts(const FastqParams& p, int n_cu, hipStream_t s);
hipError_t launch_fastq_records(const FastqParams& p, hipStream_t s);
hipError_t launch_fastq_gather(const FastqParams& p, int n_cu, hipStream_t s);

// ---- BGZF members inflated on the device (kernels_inflate.hip, inflate_device.h; host side inflate.hip) ----
// one wavefront per member of the host's table: its raw DEFLATE stream in `in` -> its isize bytes at out + out_off, and
// a status word (0, or the reason the member is declined for: nothing of `out` is then to be used)
namespace inf {
struct Member;
}
struct InflateParams {
  const uint8_t* in;  // [n_in], 4-byte aligned, readable up to the next multiple of 4
  uint64_t n_in;
  const inf::Member* members;  // [n_members]
  uint64_t n_members;
  uint8_t* out;  // [n_out]
  uint64_t n_out;
  uint32_t* status;  // [n_members]
};
hipError_t launch_bgzf_inflate(const InflateParams& p, hipStream_t s);

// ---- plain gzip inflated on the device (kernels_gzip.hip, gzip_device.h; host side gzip.hip) ----
// search, decode, chain, resolve, verify over one job: its summary, bytes and outgoing state are there when the stream
// has run them.  j.member_crc must be zero.
namespace gz {
struct Job;
}
hipError_t launch_gzip_inflate(const gz::Job& j, hipStream_t s);

}  // namespace thm
#endif
