/*
 * thermite_io.h -- the callers and data formats either side of the hot path
 * (SURVEY.md section 8f, ranks 1-4): reference ingestion + index file, FASTQ
 * batcher, SAM/PAF writer and the whole-file driver.  Same rules as
 * thermite.h: `extern "C"`, plain pointers and sizes, int32 status codes,
 * nothing unwinds.  Each declaration cites the reference interface it stands
 * for (file:line relative to the reference repository root).
 *
 * None of this is on the per-read GPU path: it is host code (C++) that feeds
 * thm_batch_upload / _run / _sync / _fetch and renders their results.
 */
#ifndef THERMITE_AMD_THERMITE_IO_H
#define THERMITE_AMD_THERMITE_IO_H

#include "thermite.h"

#ifdef __cplusplus
extern "C" {
#endif

#define THM_ERR_IO (-8)     /* file cannot be opened / read / written            */
#define THM_ERR_FORMAT (-9) /* malformed FASTA / GTF / FASTQ / index file        */

/* ------------------------------------------------ reference ingestion */

/* Index::create_from_files, src/index.rs:52-223: FASTA (optionally .gz) +
 * GTF -> index.  Text layout src/index.rs:67-101; transcript / exon / gene
 * lifting src/index.rs:126-213.  GTF row semantics follow the `transcriptome`
 * crate (Cargo.lock:1272-1274; not in the reference checkout: parity unpinned,
 * the Python restatement thermite_amd/refdata.py is the cross-check). */
int32_t thm_index_create_from_files(const char* fasta_path, const char* gtf_path, thm_index** out);

/* Names for an index built from in-memory tables; the writer needs
 * Ref::name src/index.rs:392, Tx::id src/txome.rs:19, Gene::{id,name}
 * src/txome.rs:29-33.  contig_names is indexed by thm_ref::name_id. */
int32_t thm_index_set_names(thm_index* ix, const char* const* contig_names, uint32_t n_contigs,
                            const char* const* tx_ids, uint32_t n_txs, const char* const* gene_ids,
                            const char* const* gene_names, uint32_t n_genes);

/* `thermite index -o`, src/main.rs:37-43, and ThermiteAligner::new(index_path),
 * src/wrapper.rs:31-37.  Own little-endian container ("THMIDX01"): the
 * reference's .tai is a bincode dump of bio's FMD index and cannot be read
 * without Rust.  Holds the tables and the suffix array; the k-mer table and
 * the interval grids are rebuilt at load. */
int32_t thm_index_save(const thm_index* ix, const char* path);
int32_t thm_index_load(const char* path, thm_index** out);

/* read-only view of the tables an index holds (pointers live as long as it) */
typedef struct thm_tables_view {
  uint64_t n_text;
  const uint8_t* text;
  uint32_t n_refs;
  const thm_ref* refs;
  uint32_t n_txs;
  const thm_tx* txs;
  uint64_t n_exons;
  const thm_exon* exons;
  uint64_t n_tx_seq;
  const uint8_t* tx_seq;
  uint32_t n_genes;
  const thm_span* genes;
  const uint32_t* name_rank; /* per ref */
  uint32_t n_contigs;        /* 0 when no names were supplied */
} thm_tables_view;
int32_t thm_index_tables(const thm_index* ix, thm_tables_view* out);
const char* thm_index_contig_name(const thm_index* ix, uint32_t name_id); /* NULL when unknown */
const char* thm_index_tx_id(const thm_index* ix, uint32_t tx_idx);
const char* thm_index_gene_id(const thm_index* ix, uint32_t gene_idx);
const char* thm_index_gene_name(const thm_index* ix, uint32_t gene_idx);

/* ------------------------------------------------------- FASTQ batcher */

/* needletail::parse_fastx_file + the record loop of align_reads_from_file,
 * src/aligner.rs:51-56, in batches.  Plain or gzip FASTQ (FASTA records are
 * accepted too and get empty qualities). */
typedef struct thm_fastq thm_fastq;

typedef struct thm_read_batch {
  uint64_t n_reads;
  uint64_t n_bases;
  const uint8_t* bases;     /* record.seq() back to back                  */
  const uint64_t* offsets;  /* [n_reads + 1]                              */
  const uint8_t* quals;     /* record.qual(), same offsets; may be NULL   */
  const uint8_t* names;     /* record.id() (full header line) back to back */
  const uint64_t* name_off; /* [n_reads + 1]                              */
} thm_read_batch;

int32_t thm_fastq_open(const char* path, thm_fastq** out);
/* up to max_reads records; out->n_reads == 0 at end of file.  The view is
 * valid until the next call on the same reader. */
int32_t thm_fastq_next_batch(thm_fastq* r, uint64_t max_reads, thm_read_batch* out);
void thm_fastq_close(thm_fastq* r);

/* ------------------------------------------------- BAM records from the device */

/* The records of the writer loop (src/aligner.rs:54-116) for one aligned batch, BAM-encoded on the device
 * (bam::Writer::write_sam_record, src/aligner.rs:69-76,98-108): back to back, each beginning with its block_size;
 * no BAM header, no BGZF framing.  Byte for byte what thm_writer_format_batch encodes for a BAM writer before it
 * deflates.  The records of read r are data[read_rec_off[r] .. read_rec_off[r+1]): one per alignment, or the unmapped
 * record for a read without alignments (a failed read is one: n_failed_reads / read_status as in thm_batch_view). */
typedef struct thm_bam_view {
  uint64_t n_reads;
  uint64_t n_records;
  uint64_t n_bytes;
  const uint8_t* data;          /* [n_bytes]   */
  const uint64_t* read_rec_off; /* [n_reads+1] */
  uint64_t n_failed_reads;
  const int32_t* read_status;
} thm_bam_view;

/* drops the TX GX GN RE tags: what sam_noodles_to_htslib removes, src/wrapper.rs:134-139 (AS NH HI nM stay) */
#define THM_BAM_NO_ANNOTATION_TAGS 1u

/* thm_batch_upload plus the names and qualities (may be NULL) of the batch in device memory: what thm_batch_fetch_bam
 * needs besides the run's results.  A batch uploaded by plain thm_batch_upload has no names. */
int32_t thm_batch_upload_reads(thm_aligner* a, const thm_read_batch* reads);
/* Stands where thm_batch_fetch / thm_batch_fetch_cigars stand after thm_batch_run: syncs (pool-overflow replays
 * included), runs the CIGAR passes, a size pass, a scan and an emit pass on the aligner's stream and copies back the
 * record bytes, the per-read byte offsets and the statuses only.  Any of the three fetches may follow the others for
 * the same run, in any order.  Results land in two pinned buffer sets of their own, used alternately: a thm_bam_view
 * stays valid until the second-next call on this aligner that returns one, and no other view is invalidated.
 * Counters and the other timings are untouched; THM_T_BAM is set.  The index's name tables go to the device at the
 * first call.  THM_ERR_INVALID_ARG: unknown bits in `flags`, a batch not uploaded by thm_batch_upload_reads, an index
 * without names.  THM_ERR_INTERNAL, with the writer's messages: a QNAME (name up to the first space) over 254 bytes,
 * more than 65535 CIGAR words, a run of 2^28 or more (THM_DIGEST_LONG_RUN). */
int32_t thm_batch_fetch_bam(thm_aligner* a, uint32_t flags, thm_bam_view* out);
/* upload_reads + run + the fetch above */
int32_t thm_align_batch_bam(thm_aligner* a, const thm_read_batch* reads, uint32_t flags, thm_bam_view* out);

/* ------------------------------------------------- BGZF blocks from the device */

/* The same records, BGZF-compressed on the device: the byte stream of a thm_bam_view cut every 0xff00 bytes (as the
 * host writer cuts it; a cut may fall inside a record) and every block deflated there into a complete BGZF member --
 * the 18-byte header with the BC subfield, one raw DEFLATE stream (a dynamic-Huffman block over an LZ77 parse, or a
 * stored block when that is not larger), CRC-32 and ISIZE.  Member b is data[block_off[b] .. block_off[b+1]).  No BAM
 * header and no end-of-file block: thm_writer_header + data + thm_writer_trailer is a valid .bam file.  Inflated, the
 * members give the data of the thm_bam_view of the same run and flags, n_raw_bytes long; no records: n_blocks == 0.
 * The bytes depend on the input bytes only: the same records compress to the same members on every call and aligner. */
typedef struct thm_bgzf_view {
  uint64_t n_reads, n_records;
  uint64_t n_raw_bytes;          /* what the blocks inflate to: thm_bam_view.n_bytes of the same run */
  uint64_t n_blocks, n_bytes;
  const uint8_t* data;           /* [n_bytes]: n_blocks complete BGZF members, back to back */
  const uint64_t* block_off;     /* [n_blocks+1] */
  uint64_t n_failed_reads;
  const int32_t* read_status;
} thm_bgzf_view;
/* Stands where thm_batch_fetch_bam stands and takes its flags, preconditions and errors (same codes and messages, which
 * name thm_batch_fetch_bam: it is that call's record passes that report them); failed reads as there.  Any of the four
 * fetches may follow the others for the same run, in any order.  Only the members, their offsets and the statuses are
 * copied back, into two pinned buffer sets of their own, used alternately: a thm_bgzf_view stays valid until the
 * second-next call on this aligner that returns one, and no other view is invalidated.  Counters and the other
 * timings are untouched; THM_T_BGZF is set.  THM_BAM_LEVEL does not apply. */
int32_t thm_batch_fetch_bgzf(thm_aligner* a, uint32_t flags, thm_bgzf_view* out);
/* upload_reads + run + the fetch above */
int32_t thm_align_batch_bgzf(thm_aligner* a, const thm_read_batch* reads, uint32_t flags, thm_bgzf_view* out);

/* ------------------------------------------------- coordinate-sorted BAM: a whole run's records sorted on the device */

/* The records of every batch of a run stay in device memory (thm_bam_sorter_add in place of a fetch); at the end they
 * are sorted once and handed out in coordinate order, window by window, through the device deflater.  The order, with
 * n_sq the number of @SQ lines (BAM refIDs) of the index and refID, pos, flag the record's fields:
 *     rank = refID >= 0 ? refID : n_sq                              (unmapped last)
 *     key  = rank << 33 | (uint32)(pos + 1) << 1 | (flag >> 4 & 1)  (position, then forward before reverse)
 * Records are ordered by key; records with equal keys keep the order in which they were added (add order, then record
 * order within the batch).  The .bai of the sorted file is built on the device too (thm_bam_sorter_index below).  Not done:
 * spilling to the host when the records exceed device memory, merging across devices, name order. */
typedef struct thm_bam_sorter thm_bam_sorter;

typedef struct thm_bam_sort_info {      /* what one add did, and the totals so far */
  uint64_t n_reads, n_records, n_bytes;            /* this batch */
  uint64_t total_records, total_bytes;             /* held by the sorter */
  uint64_t n_failed_reads; const int32_t* read_status;   /* as in thm_bam_view; valid until the next add */
  float add_ms;                                    /* key kernel + copy, device events */
} thm_bam_sort_info;

typedef struct thm_bam_sorted_view {
  uint64_t total_records, total_raw_bytes;   /* of the whole sorted stream */
  uint64_t raw_offset, n_raw_bytes;          /* this window of it; n_raw_bytes == 0: the stream is exhausted */
  uint64_t n_blocks, n_bytes;
  const uint8_t* data;                       /* BGZF members back to back, or with THM_SORT_RAW the window's record bytes */
  const uint64_t* block_off;                 /* [n_blocks+1]; NULL with THM_SORT_RAW */
  float gather_ms, deflate_ms;
} thm_bam_sorted_view;

#define THM_SORT_RAW 1u

/* A sorter belongs to one aligner: it works on that aligner's device and stream and must be freed before it.
 * max_bytes caps the record bytes held (0: no cap but the device's memory). */
int32_t thm_bam_sorter_create(thm_aligner* a, uint64_t max_bytes, thm_bam_sorter** out);
/* Stands where thm_batch_fetch_bam stands after thm_batch_run and takes its flags, preconditions and errors (same codes
 * and messages): the run's records are encoded on the device and stay there, appended behind those already held (what is
 * held is never copied again); only counts and statuses come back.  It may precede or follow any of the four fetches of
 * the same run and disturbs none of their views, no counter and no timing.  THM_ERR_OOM: the cap would be exceeded, or a
 * device allocation failed (the message names the bytes needed and the cap); the batch is then not added and the sorter
 * stays usable with what it held.  THM_ERR_INVALID_ARG: more than 2^32-1 records in all, or a call after finish. */
int32_t thm_bam_sorter_add(thm_bam_sorter* s, uint32_t bam_flags, thm_bam_sort_info* info);
/* sorts (key, ordinal) pairs and scans the sorted lengths; sort_ms (may be NULL): device events.  Once. */
int32_t thm_bam_sorter_finish(thm_bam_sorter* s, float* sort_ms);
/* The next window of the sorted stream: max_raw_bytes rounded down to a multiple of 0xff00 and at least 0xff00 (0: 256
 * blocks), the last one shorter.  Every window begins on a multiple of 0xff00, so the members of all windows back to
 * back are the sorted stream cut every 0xff00 bytes, whatever the window size and however the records came in batches:
 * thm_writer_header_sorted + all members + thm_writer_trailer is a valid coordinate-sorted .bam.  Two pinned result sets,
 * used alternately: a view stays valid until the second-next call on this sorter.  THM_ERR_INVALID_ARG: before finish,
 * unknown bits in flags.  THM_SORT_GATHER=pieces in the environment when the sorter is created selects the other of the
 * two gather kernels (same bytes). */
int32_t thm_bam_sorter_next(thm_bam_sorter* s, uint64_t max_raw_bytes, uint32_t flags, thm_bam_sorted_view* out);
void thm_bam_sorter_free(thm_bam_sorter* s);

/* The .bai index (SAM specification section 5.2; UCSC binning of section 5.3: min_shift 14, 5 levels, pseudo-bin 37450)
 * of the file thm_writer_header_sorted + all members + thm_writer_trailer, built on the device from the sorted records.
 * These rules are the contract:
 *   Virtual offsets.  F = first_member_offset, the file offset of the first record member (the length of what was written
 *     before it).  coff[m] = F + the compressed sizes of members 0 .. m-1; coff[n_members] is where the trailer goes.  For
 *     a stream offset s:  v(s) = coff[s / 0xff00] << 16 | s % 0xff00.  A record's vbeg is v of its first byte, its vend v
 *     of the offset just past it (for the last record v(total), which points at the trailer member, offset 0, when total
 *     is a multiple of 0xff00).
 *   Per record, from refID, pos, flag, n_cigar_op and the CIGAR words of the record (its bin field is not trusted):
 *     refID < 0: the record counts in n_no_coor and nothing else.  Otherwise beg = max(pos, 0); end = beg + the summed
 *     lengths of its M, D, N, = and X ops, or beg + 1 where that sum is 0 (also with no CIGAR); bin = reg2bin(beg, end);
 *     mapped = !(flag & 4).  A record with refID >= 0 and end > 2^29 makes the call fail with THM_ERR_INVALID_ARG (the
 *     message names its reference and position): BAI cannot address it, and CSI is not written.
 *   Chunks of a bin.  In stream order, a maximal run of consecutive records with one (refID, bin) is a chunk [vbeg of its
 *     first, vend of its last).  Within a bin, in stream order, a chunk is merged into its predecessor when
 *     pred.end >> 16 >= chunk.beg >> 16 (the predecessor's end becomes the chunk's end).  Nothing else is merged or
 *     folded into parent bins.
 *   Per reference, in @SQ order: the bins in ascending bin number, each with its chunks in stream order; then, exactly when
 *     the reference has records, the pseudo-bin 37450 with two chunks, (vbeg of the reference's first record, vend of its
 *     last) and (n_mapped, n_unmapped); it counts in n_bin.  A reference without records has n_bin = 0, n_intv = 0.
 *   Linear index, from mapped records only: n_intv = 1 + max((end - 1) >> 14); ioffset[w] = the smallest vbeg of a mapped
 *     record with beg >> 14 <= w <= (end - 1) >> 14; a window no record overlaps takes the value of the next window above
 *     it that has one (the last window always has one).
 *   Tail: n_no_coor (uint64), always.  An empty sorter gives "BAI\1", n_ref, n_ref x (0, 0), 0. */
typedef struct thm_bai_view {
  uint64_t n_bytes; const uint8_t* data;        /* the finished .bai file */
  uint64_t n_refs, n_bins, n_chunks, n_intervals, n_no_coor;   /* n_bins includes the pseudo-bins; n_chunks: of the other bins */
  float index_ms;                               /* device events, all index kernels */
} thm_bai_view;
/* Valid once thm_bam_sorter_next has returned the exhausted view (n_raw_bytes == 0; an empty sorter is exhausted as soon
 * as it is finished) and every window was taken as BGZF: the sorter keeps every member's compressed size (8 bytes a
 * member, host memory) as it hands the windows out.  THM_ERR_INVALID_ARG with a message: before finish, before the stream
 * is exhausted, after any THM_SORT_RAW window (there are no member sizes then), a record beyond 2^29.  The call may be
 * repeated, also with another first_member_offset: the result depends on the records and that offset only.  The view
 * has a pinned buffer of its own and stays valid until the next index call or the free; no other view, timing or counter
 * changes.  With THM_BAM_SORT=1 and THM_BAM_INDEX=1 thm_align_files writes it to <output_path>.bai. */
int32_t thm_bam_sorter_index(thm_bam_sorter* s, uint64_t first_member_offset, thm_bai_view* out);

/* ------------------------------------------------- gene and splice-junction count tables of a run, built on the device */

/* What a counter reads back out of the run's SAM/BAM records -- per gene the reads (GX + RE + NH), per splice junction the
 * reads that cross it (CIGAR N runs) -- accumulated on the device over any number of batches from what is resident there
 * after thm_batch_run; only the finished tables cross to the host.  These rules are the contract, each phrased as what a
 * pass over the run's SAM records would count.  For an alignment of read r, NH is the number of alignments of r
 * (read_aln_off[r+1] - read_aln_off[r]); the alignment is unique when NH == 1 and multi when NH > 1.
 *   Genes.  One row per gene of the index, in index order: exonic_unique, exonic_multi, intronic_unique, intronic_multi.  An
 *     exonic alignment (RE:A:E) counts in the row of txs[tx_or_gene_idx].gene_idx, an intronic one (RE:A:N) in the row of
 *     tx_or_gene_idx; intergenic alignments count only in the totals.  Counts are per alignment record, not per read.
 *   Junctions.  Every N word of an alignment's genome CIGAR is one junction hit.  With p = ystart plus the lengths of all
 *     M, D and N words before the N word: start = p (0-based first intron base), end = p + len.  ref is the BAM refID of
 *     the alignment's contig (its @SQ index, as in thm_bam_view), strand that of the alignment's transcript (N occurs in
 *     exonic alignments only: lift_tx_to_gx, src/txome.rs:110-160).  A hit has two anchors: left is the summed length of
 *     the M words between the previous N word (or the CIGAR's start) and this one, right the same up to the next N word
 *     (or the end); I, D and S words add nothing and interrupt nothing; overhang = min(left, right).  Two adjacent N
 *     words are two hits, with anchor 0 between them.  The table has one row per distinct (ref, start, end, strand):
 *     n_unique and n_multi (hits from unique / multi alignments) and max_overhang over all its hits.  Rows ascend by ref,
 *     start, end, with forward before reverse.  An alignment whose digest has THM_DIGEST_LONG_RUN has no words: it
 *     contributes no hit and counts in n_long_run_alns.
 *   Totals.  Reads: n_reads = n_failed_reads + n_unmapped_reads + n_unique_reads + n_multi_reads; a failed read is one whose
 *     status is not THM_OK, and is not counted as unmapped.  Alignments: n_alns = the sum of the gene table +
 *     n_intergenic_unique + n_intergenic_multi.  n_spliced_alns: alignments with at least one hit; n_junction_hits = the
 *     sum of n_unique + n_multi over the junction rows. */
typedef struct thm_quant thm_quant;

typedef struct thm_quant_gene {
  uint64_t exonic_unique, exonic_multi, intronic_unique, intronic_multi;
} thm_quant_gene; /* 32 bytes */

typedef struct thm_quant_junction {
  uint32_t ref_id;       /* BAM refID */
  uint32_t strand;       /* 1 = forward, as thm_tx::strand */
  uint64_t start, end;   /* 0-based, half open: the intron's first base, and the base behind its last */
  uint64_t n_unique, n_multi;
  uint32_t max_overhang;
  uint32_t pad_;
} thm_quant_junction; /* 48 bytes */

typedef struct thm_quant_totals {
  uint64_t n_reads, n_failed_reads, n_unmapped_reads, n_unique_reads, n_multi_reads;
  uint64_t n_alns, n_intergenic_unique, n_intergenic_multi;
  uint64_t n_spliced_alns, n_junction_hits, n_long_run_alns;
} thm_quant_totals; /* 88 bytes */

typedef struct thm_quant_info {  /* what one add did, and the table sizes so far */
  thm_quant_totals batch;        /* this batch */
  uint64_t n_junctions;          /* rows of the junction table */
  uint64_t held_bytes;           /* device memory the object holds: both tables and one batch's scratch */
  float add_ms;                  /* device events, all kernels and sorts of the add */
} thm_quant_info;

typedef struct thm_quant_view {
  uint64_t n_genes;
  const thm_quant_gene* genes;          /* [n_genes] */
  uint64_t n_junctions;
  const thm_quant_junction* junctions;  /* [n_junctions] */
  thm_quant_totals totals;
  float fetch_ms;                       /* device events: the row kernel and the copies */
} thm_quant_view;

/* A thm_quant belongs to one aligner, like a thm_bam_sorter: it works on that aligner's device and stream and must be
 * freed before it.  THM_ERR_UNSUPPORTED: a contig of 2^32 bases or more (start and end are 32-bit in the sort key).
 * THM_ERR_INVALID_ARG, with thm_batch_fetch_bam's message: an index without contig / transcript / gene names.  Device
 * memory held is bounded by the distinct junctions, the gene table and one batch's scratch; it does not grow with the run. */
int32_t thm_quant_create(thm_aligner* a, thm_quant** out);
void thm_quant_free(thm_quant* q);
/* Stands where thm_batch_fetch stands after thm_batch_run, and fails as it does before a run or after the next upload.
 * It may precede or follow any fetch or a thm_bam_sorter_add of the same run and disturbs none of their views, no counter
 * and no timing; it runs the CIGAR passes itself.  The batch's hits are extracted, sorted, reduced by key and merged into
 * the running sorted table; the genes are counted last, so that a call that fails has added nothing.  Adding the same run
 * twice counts it twice. */
int32_t thm_quant_add(thm_quant* q, thm_quant_info* info);
/* The same kernels over a caller-supplied view (read_aln_off, alns, digests, cigar, read_status), uploaded by the call:
 * what thm_cigar_encode_batch is to the CIGAR layer.  The host checks the view first -- offsets that start at 0, ascend
 * and end at n_alns; aln_type, tx_or_gene_idx and ref_id in range (a ref_id must have a BAM refID); cigar_off + n_cigar
 * inside the pool; every position below 2^32 -- THM_ERR_INVALID_ARG with a message naming the alignment, and nothing is
 * added. */
int32_t thm_quant_add_view(thm_quant* q, const thm_cigar_view* v, thm_quant_info* info);
/* A snapshot at any time.  The view has a pinned buffer of its own and stays valid until the next fetch, reset or free. */
int32_t thm_quant_fetch(thm_quant* q, thm_quant_view* out);
/* empties both tables and the totals */
int32_t thm_quant_reset(thm_quant* q);

/* ------------------------------------------------- per-base coverage tracks of a run, built on the device */

/* What a depth counter reads back out of the run's SAM/BAM records (samtools depth, bedtools genomecov -bg -split):
 * accumulated on the device over any number of batches from what is resident there after thm_batch_run; only finished
 * runs of equal depth, or a window of depths, cross to the host.  These rules are the contract, each phrased as what a
 * pass over the run's SAM records would compute.
 *   Covered bases.  For an alignment at 0-based p = ystart, over the words (len << 4 | code) of its genome CIGAR: an M or
 *     a D word covers [p, p + len) and advances p; an N word advances p and covers nothing; I and S words do neither.  A
 *     block is a maximal stretch covered by consecutive M / D words (I and S words between them interrupt nothing, an N
 *     word ends it): 3M2D4M is one block of 9, 3M4N4M two blocks.  A stretch of length 0 is no block.  Every alignment
 *     record counts, secondary ones too, with weight 1 (no 1/NH).  An alignment whose digest has THM_DIGEST_LONG_RUN has
 *     no words: it covers nothing and counts in n_long_run_alns.
 *   Tracks, chosen at create by `flags`.  THM_COV_STRANDED: forward alignments (SAM flag 0x10 clear: thm_aln::strand == 1)
 *     and reverse ones are kept apart.  THM_COV_MULTI: alignments with NH > 1 (NH as for thm_quant: the alignments of the
 *     read) get tracks of their own; without it they cover nothing and count in n_skipped_multi.
 *     n_strands = STRANDED ? 2 : 1; n_tracks = n_strands * (MULTI ? 2 : 1); track = cls * n_strands + strand_idx with
 *     cls 0 = unique, 1 = multi and strand_idx 0 = forward, 1 = reverse (always 0 without STRANDED).
 *   Depth.  depth[track][refID][x] = the number of blocks of that track's alignments that cover x, a 32-bit count: an add
 *     that would bring the alignments counted by the object (totals.n_alns) over 2^32 - 1 is refused with
 *     THM_ERR_INVALID_ARG, so no depth can wrap.
 *   Runs: what a fetch returns for a track and a range of @SQ entries -- the maximal intervals of equal, non-zero depth.
 *     A run never crosses a contig; runs ascend by refID, then start; two abutting blocks of equal depth make one run; a
 *     run may end exactly at the contig's length.
 *   Totals.  n_alns = the track n_alns summed + n_skipped_multi + n_long_run_alns (an alignment counts in one of them: a
 *     multi-mapped one without a track in n_skipped_multi, whatever its digest says); per track n_alns (alignments that
 *     went into it), n_blocks and n_bases (the summed block lengths).  Reads: n_reads, and n_failed_reads of them with a
 *     status other than THM_OK. */
typedef struct thm_coverage thm_coverage;

#define THM_COV_STRANDED 1u
#define THM_COV_MULTI 2u

typedef struct thm_cov_run {
  uint32_t ref_id;      /* BAM refID */
  uint32_t depth;
  uint64_t start, end;  /* 0-based, half open */
} thm_cov_run; /* 24 bytes */

typedef struct thm_cov_track_totals {
  uint64_t n_alns, n_blocks, n_bases;
} thm_cov_track_totals;

typedef struct thm_cov_totals {
  uint64_t n_reads, n_failed_reads, n_alns, n_skipped_multi, n_long_run_alns;
  thm_cov_track_totals track[4]; /* [n_tracks] used */
} thm_cov_totals; /* 136 bytes */

typedef struct thm_cov_info {  /* what one add did */
  thm_cov_totals batch;        /* this batch */
  uint64_t held_bytes;         /* device memory the object holds: the difference arrays and the scratch of adds and fetches */
  float add_ms;                /* device events, both kernels of the add */
} thm_cov_info;

typedef struct thm_cov_view {
  uint32_t track, first_ref, n_refs;
  uint32_t max_depth;          /* over the runs; 0 without runs */
  uint64_t n_runs;
  const thm_cov_run* runs;     /* [n_runs] */
  uint64_t n_covered;          /* the sum of end - start over the runs */
  uint64_t n_bases;            /* the sum of (end - start) * depth: over all contigs, the track's n_bases */
  thm_cov_totals totals;       /* of the object so far */
  float fetch_ms;              /* device events: the fetch kernels, scans and the copy */
} thm_cov_view;

typedef struct thm_cov_depth_view {
  uint64_t n;
  const uint32_t* depth;       /* [n] */
  float depth_ms;
} thm_cov_depth_view;

/* A thm_coverage belongs to one aligner, like a thm_quant: it works on that aligner's device and stream and must be freed
 * before it.  It holds n_tracks difference arrays of 4 bytes over every base of every @SQ contig, one more entry behind
 * each contig (where a block that ends on the contig's last base is closed), and a table of 8 bytes per contig.
 * THM_ERR_OOM: those bytes exceed max_bytes (0: no cap but the device's memory) or the allocation fails; the message names
 * the bytes needed and the cap, and nothing is allocated before the cap is checked.  THM_ERR_INVALID_ARG: unknown bits in
 * `flags`; with thm_batch_fetch_bam's message, an index without names. */
int32_t thm_coverage_create(thm_aligner* a, uint32_t flags, uint64_t max_bytes, thm_coverage** out);
void thm_coverage_free(thm_coverage* c);
/* Stands where thm_batch_fetch stands after thm_batch_run, fails as thm_quant_add fails, runs the CIGAR passes itself
 * (THM_T_CIGAR is put back) and disturbs no view, counter or timing.  The device validates every alignment in a pass of
 * its own before any array is touched -- its ref has a refID, cigar_off + n_cigar lies inside the pool, the walk ends
 * inside the contig -- so a call that fails has added nothing and no add can land outside the arrays.  Then every block
 * costs two integer adds, whatever its length: batches in any cut and order give the same bytes.  Adding a run twice
 * doubles every depth. */
int32_t thm_coverage_add(thm_coverage* c, thm_cov_info* info);
/* The same kernels over a caller-supplied view, uploaded by the call.  The host checks it first: what thm_quant_add_view
 * checks of offsets, aln_type, tx_or_gene_idx, ref_id and the CIGAR range, and ystart + digest.ref_len <= the contig's
 * length -- THM_ERR_INVALID_ARG with a message naming the alignment, as for a view the device's pass refuses (a digest
 * whose ref_len is not that of its words), and nothing is added. */
int32_t thm_coverage_add_view(thm_coverage* c, const thm_cigar_view* v, thm_cov_info* info);
/* The runs of `track` on the @SQ entries [first_ref, first_ref + n_refs), built on the device: a snapshot at any time.
 * They arrive in a pinned buffer of the object's own, valid until the next fetch, depth call, reset or free.
 * THM_ERR_INVALID_ARG: no such track, or a range outside the @SQ entries. */
int32_t thm_coverage_fetch(thm_coverage* c, uint32_t track, uint32_t first_ref, uint32_t n_refs, thm_cov_view* out);
/* The depth of every base of [start, start + n) of one contig; valid as the runs are.  THM_ERR_INVALID_ARG: no such track
 * or refID, n over 1 << 24, a window that leaves the contig. */
int32_t thm_coverage_depth(thm_coverage* c, uint32_t track, uint32_t ref_id, uint64_t start, uint64_t n, thm_cov_depth_view* out);
/* empties every track and the totals */
int32_t thm_coverage_reset(thm_coverage* c);

/* ------------------------------------------------- per-base allele counts of a run, built on the device */

/* What a pileup reads back out of the run's SAM records and the FASTA (samtools mpileup without a quality filter, counted
 * per base): accumulated on the device over any number of batches from what is resident there after thm_batch_run -- the
 * raw reads, the alignments, the genome CIGAR words and the index's text, whose forward copy of a contig is its sequence.
 * Only rows of sites cross to the host.  These rules are the contract, each phrased as what a pass over the run's SAM
 * records and the FASTA would compute.
 *   Alignments used.  Every alignment record counts, secondary ones too, with weight 1.  The alignments of a read with
 *     NH > 1 (NH as for thm_quant: the alignments of the read) are left out and count in n_skipped_multi, whatever their
 *     digests say; with THM_PILE_MULTI they count like the others, into the same counts.  An alignment whose digest has
 *     THM_DIGEST_LONG_RUN has no words: it contributes nothing and counts in n_long_run_alns.  The others are the
 *     n_used_alns: n_alns = n_skipped_multi + n_long_run_alns + n_used_alns.
 *   SEQ is what SAM prints: the read for thm_aln::strand == 1, otherwise its reverse complement.  kind(c) of a byte:
 *     upper-cased, A C G T are 0..3 and anything else is 4 (N); the complement of kind 4 is kind 4.
 *   Walk.  From 0-based p = ystart and q = 0 over the words (len << 4 | code) of the genome CIGAR: an M word lets position
 *     p + i observe kind(SEQ[q + i]) for i < len, then p and q advance; a D word lets each of [p, p + len) observe one
 *     `del`, p advances; an N word advances p; an S word advances q; an I word is one `ins` (the word, not its bases)
 *     observed at x = p - 1 if p > ystart, else at x = ystart -- which may be an intron base directly behind an N word --
 *     and q advances.  An alignment that consumes no reference base observes nothing.  M + I + S over the words is the
 *     read's length.
 *   Depth.  depth[x] = the number of used alignments whose M or D words cover x (the blocks of thm_coverage), a 32-bit
 *     count: an add that would bring totals.n_alns over 2^32 - 1 is refused with THM_ERR_INVALID_ARG.
 *   Counts at x.  cnt[0..4] = the M observations of each kind, del and ins as in the walk; depth[x] == cnt[0] + ... +
 *     cnt[4] + del.  An event is an observation whose kind differs from kind(the text's byte at x), or any del or ins;
 *     alt[x] = the events at x.  The reference allele's count is never stored: it is depth minus the rest.  The cap on
 *     n_alns bounds depth, cnt and del below 2^32; ins, of which one alignment can bring several to one position, stays at
 *     2^32 - 1 once it has reached it.
 *   Totals.  n_blocks: the blocks of the used alignments; n_m_bases: their M bases; n_mismatches: the events of kinds
 *     0..4; n_del_bases; n_ins (I words) and n_ins_bases (their summed lengths).  Reads: n_reads, and n_failed_reads of
 *     them with a status other than THM_OK. */
typedef struct thm_pileup thm_pileup;

#define THM_PILE_MULTI 1u

typedef struct thm_pile_site {
  uint32_t ref_id;             /* BAM refID */
  uint8_t ref_base, pad_[3];   /* the text's byte at pos */
  uint64_t pos;                /* 0-based */
  uint32_t depth, cnt[5], del, ins;
} thm_pile_site; /* 48 bytes */

typedef struct thm_pile_totals {
  uint64_t n_reads, n_failed_reads, n_alns, n_skipped_multi, n_long_run_alns, n_used_alns, n_blocks;
  uint64_t n_m_bases, n_mismatches, n_del_bases, n_ins, n_ins_bases;
} thm_pile_totals; /* 96 bytes */

typedef struct thm_pile_info { /* what one add did */
  thm_pile_totals batch;       /* this batch */
  uint64_t n_events;           /* rows of the event table so far: distinct (position, kind) with an event */
  uint64_t held_bytes;         /* device memory the object holds: the difference array, the table and every scratch */
  float add_ms;                /* device events, every pass of the add */
} thm_pile_info;

typedef struct thm_pile_view {
  uint32_t first_ref, n_refs;  /* the range asked for (a window: its refID and 1) */
  uint32_t min_alt, pad_;      /* 0 for a window */
  uint64_t n_sites;
  const thm_pile_site* sites;  /* [n_sites] ascending by ref_id, pos */
  uint64_t n_events;           /* rows of the event table inside the range (a window: inside the window) */
  thm_pile_totals totals;      /* of the object so far */
  float fetch_ms;              /* device events: the kernels, scans and the copy */
} thm_pile_view;

/* A thm_pileup belongs to one aligner, like a thm_coverage: it works on that aligner's device and stream and must be
 * freed before it.  It holds one difference array in thm_coverage's layout -- 4 bytes over every base of every @SQ
 * contig, one more entry behind each contig -- two tables of 8 bytes per contig, and the sorted event table of 12 bytes
 * per row.  max_bytes (0: no cap but the device's memory) bounds the arrays plus the table; the scratch of adds and
 * fetches is not counted against it (held_bytes reports everything).  THM_ERR_OOM: the arrays alone exceed max_bytes, or
 * the allocation fails; the message names the bytes needed and the cap, and nothing is allocated before the cap is
 * checked.  THM_ERR_INVALID_ARG: unknown bits in `flags`; with thm_batch_fetch_bam's message, an index without names. */
int32_t thm_pileup_create(thm_aligner* a, uint32_t flags, uint64_t max_bytes, thm_pileup** out);
void thm_pileup_free(thm_pileup* p);
/* Stands where thm_batch_fetch stands after thm_batch_run, fails as thm_coverage_add fails, runs the CIGAR passes itself
 * (THM_T_CIGAR is put back) and disturbs no view, counter or timing.  The device validates every alignment in a pass of
 * its own before anything is touched -- its ref has a refID, cigar_off + n_cigar lies inside the pool, the walk ends
 * inside the contig, M + I + S is the read's length -- then extracts the events, sorts and reduces them by (position,
 * kind) and merges them into the table; the deposit into the difference array and the swap to the merged table come
 * last, so a call that fails has added nothing.  THM_ERR_OOM: the arrays plus the merged table would exceed max_bytes;
 * the message names the bytes needed and the cap.  Batches in any cut and order give the same rows; adding a run twice
 * doubles every count. */
int32_t thm_pileup_add(thm_pileup* p, thm_pile_info* info);
/* The same kernels over a caller-supplied view and the bytes of its reads (read r is bases[base_off[r], base_off[r + 1])),
 * uploaded by the call.  The host checks first what thm_coverage_add_view checks, that base_off starts at 0 and ascends,
 * and that M + I + S of every alignment with words is its read's length: THM_ERR_INVALID_ARG with a message naming the
 * alignment (or the read), as for a view the device's pass refuses, and nothing is added. */
int32_t thm_pileup_add_view(thm_pileup* p, const thm_cigar_view* v, const uint8_t* bases, const uint64_t* base_off,
                            thm_pile_info* info);
/* One row per position of the @SQ entries [first_ref, first_ref + n_refs) with alt >= min_alt, built on the device: a
 * snapshot at any time.  The rows arrive in a pinned buffer of the object's own, valid until the next fetch, window,
 * reset or free.  THM_ERR_INVALID_ARG: min_alt == 0, or a range outside the @SQ entries. */
int32_t thm_pileup_fetch(thm_pileup* p, uint32_t first_ref, uint32_t n_refs, uint32_t min_alt, thm_pile_view* out);
/* One row for every position of [start, start + n) of one contig, those without events or depth included: what a
 * genotyper of known sites asks for; valid as the fetch's rows are.  THM_ERR_INVALID_ARG: no such refID, n over 1 << 20,
 * a window that leaves the contig. */
int32_t thm_pileup_window(thm_pileup* p, uint32_t ref_id, uint64_t start, uint64_t n, thm_pile_view* out);
/* empties the difference array, the table and the totals */
int32_t thm_pileup_reset(thm_pileup* p);

/* ------------------------------------------------- cell-by-gene UMI count matrix of a run, built on the device */

/* What a single-cell pipeline computes from the run's BAM by parsing every QNAME and sorting by (barcode, gene, UMI): the
 * distinct molecules per cell and gene, accumulated on the device over any number of batches from what is resident there
 * after thm_batch_run -- the alignments with their annotation, the per-read offsets (NH) and the read names.  Only rows
 * of cells and matrix entries cross to the host.  These rules are the contract.
 *   Where barcode and UMI come from (the convention of `umi_tools extract`).  QNAME is the read's name up to its first
 *     space, the BAM layer's rule; a name without a space is all QNAME.  The QNAME carries a tag exactly when its last
 *     cb_len + umi_len + 2 bytes are '_', cb_len bases, '_', umi_len bases, every base one of upper-case A C G T.
 *     Anything else -- an N, lower case, a shorter QNAME, another separator -- means the read has no tag; what follows the
 *     first space is never looked at; the prefix in front of the tag may be empty.  cb_len and umi_len are fixed at create,
 *     each 1..16.  A sequence packs into 32 bits, 2 bits a base, A=0 C=1 G=2 T=3, the first base most significant (a
 *     sequence of L bases fills the low 2 L bits), so integer order is lexicographic order.
 *   Which reads count.  A read is counted exactly when its status is THM_OK, it has a tag, NH == 1 (NH as for thm_quant:
 *     the alignments of the read), and its one alignment is exonic -- its gene is txs[tx_or_gene_idx].gene_idx -- or, only
 *     with THM_CELLS_INTRONIC, intronic -- its gene is tx_or_gene_idx.  Every other read falls into exactly one total,
 *     tested in this order: n_failed_reads (status), n_unmapped_reads (NH == 0), n_multi_reads (NH > 1),
 *     n_intergenic_reads, n_intronic_skipped_reads (intronic without the flag), n_untagged_reads.  n_reads is the sum of
 *     these six and n_counted_reads.  Strand relative to the gene is not considered, as in thm_quant; CIGAR words are not
 *     needed, and an alignment with THM_DIGEST_LONG_RUN counts like any other.
 *   Molecules.  A molecule is a distinct (barcode, gene, UMI); the object keeps one row of 16 bytes per molecule with a
 *     32-bit count of its reads: an add that would bring totals.n_reads over 2^32 - 1 is refused with
 *     THM_ERR_INVALID_ARG.  Batches in any cut and order give the same bytes from a fetch; adding the same run twice
 *     doubles every n_reads and changes no n_umis. */
typedef struct thm_cells thm_cells;

#define THM_CELLS_INTRONIC 1u
#define THM_CELLS_MAX_LEN 16u

typedef struct thm_cell {
  uint64_t n_reads;            /* counted reads of the cell */
  uint32_t barcode;            /* packed */
  uint32_t n_umis;             /* distinct molecules over all genes */
  uint32_t n_genes;            /* genes with a molecule: the cell's entries */
  uint32_t pad_;
} thm_cell; /* 24 bytes */

typedef struct thm_cell_entry {
  uint32_t cell;               /* index into cells[] */
  uint32_t gene;               /* index into the index's genes */
  uint32_t n_umis;             /* distinct UMIs of (cell, gene): the matrix's value */
  uint32_t n_reads;            /* their reads */
} thm_cell_entry; /* 16 bytes */

typedef struct thm_cells_totals {
  uint64_t n_reads, n_failed_reads, n_unmapped_reads, n_multi_reads, n_intergenic_reads, n_intronic_skipped_reads;
  uint64_t n_untagged_reads, n_counted_reads;
} thm_cells_totals; /* 64 bytes */

typedef struct thm_cells_info { /* what one add did */
  thm_cells_totals batch;      /* this batch */
  uint64_t n_molecules;        /* rows the object holds: the sorted table's distinct molecules plus n_pending */
  uint64_t n_pending;          /* rows of batches not yet merged into the table (a molecule of the table, or of two such
                                  batches, has a row in each): 0 when this add merged, and after every fetch */
  uint64_t held_bytes;         /* device memory the object holds: the table, the pending rows and every scratch */
  float add_ms;                /* device events, every pass of the add */
} thm_cells_info;

typedef struct thm_cells_view {
  uint32_t cb_len, umi_len;
  uint32_t min_umis, pad_;
  uint64_t n_cells;
  const thm_cell* cells;          /* [n_cells] ascending by barcode */
  uint64_t n_entries;
  const thm_cell_entry* entries;  /* [n_entries] ascending by (cell, gene) */
  uint64_t n_molecules, n_barcodes;  /* distinct molecules and barcodes of the whole object */
  uint64_t n_cells_below;         /* barcodes with fewer than min_umis molecules: n_barcodes - n_cells */
  thm_cells_totals totals;        /* of the object so far */
  float fetch_ms;                 /* device events: the merge of pending rows, the kernels, scans and the copies */
} thm_cells_view;

/* A thm_cells belongs to one aligner, like a thm_quant: it works on that aligner's device and stream and must be freed
 * before it.  max_bytes (0: no cap but the device's memory) bounds the rows the object keeps, 16 bytes each, the sorted
 * table's and the pending ones; the scratch of adds and fetches is not counted against it (held_bytes reports
 * everything).  THM_ERR_INVALID_ARG: unknown bits in `flags`; cb_len or umi_len outside 1..16; with
 * thm_batch_fetch_bam's message, an index without names.  THM_ERR_UNSUPPORTED: 2^30 genes or more. */
int32_t thm_cells_create(thm_aligner* a, uint32_t flags, uint32_t cb_len, uint32_t umi_len, uint64_t max_bytes, thm_cells** out);
void thm_cells_free(thm_cells* c);
/* Stands where thm_batch_fetch stands after thm_batch_run, fails as thm_quant_add fails, runs the CIGAR passes itself
 * (THM_T_CIGAR is put back) and disturbs no view, counter or timing.  The batch must have its names on the device
 * (thm_batch_upload_reads or a thm_batch_upload_fastq*): otherwise THM_ERR_INVALID_ARG with thm_batch_fetch_bam's message
 * for that.  One pass classifies every read and composes the keys of the counted ones (no byte of the names outside the
 * batch's pool is read); these are compacted, sorted over the bits in use and reduced by key.  The reduced rows wait as
 * pending rows behind those of earlier batches; once there are as many of them as the table has rows, and at every
 * fetch, table and pending rows are sorted and reduced together into the new table, so the cost of an add does not grow
 * with the table at every call.  The totals, the pending count and the swap to a merged table come last: a call that
 * fails has added nothing.  THM_ERR_OOM: the rows held would exceed max_bytes even after a merge; the message names the
 * bytes needed and the cap. */
int32_t thm_cells_add(thm_cells* c, thm_cells_info* info);
/* The same kernels over a caller-supplied view and the names of its reads (read r's is names[name_off[r], name_off[r + 1])),
 * uploaded by the call.  The host checks first what thm_quant_add_view checks of the view's arrays, and that name_off
 * starts at 0 and does not descend: THM_ERR_INVALID_ARG with a message naming the alignment or the read, and nothing is
 * added. */
int32_t thm_cells_add_view(thm_cells* c, const thm_cigar_view* v, const uint8_t* names, const uint64_t* name_off,
                           thm_cells_info* info);
/* The cells with min_umis molecules or more and their matrix entries, built on the device: a snapshot at any time, which
 * changes nothing that a later fetch returns.  Both arrays arrive in a pinned buffer of the object's own, valid until
 * the next fetch, reset or free.  THM_ERR_INVALID_ARG: min_umis == 0. */
int32_t thm_cells_fetch(thm_cells* c, uint32_t min_umis, thm_cells_view* out);
/* empties the table, the pending rows and the totals */
int32_t thm_cells_reset(thm_cells* c);

/* ------------------------------------------------- FASTQ blocks parsed on the device */

typedef struct thm_fastq_upload_info {
  uint64_t n_reads, n_bases, n_name_bytes;
  uint32_t on_device; /* 1: parsed by the device; 0: the block was not device-parsable and went through the host parser */
  float device_ms;    /* HIP-event time of the parse kernels; 0 when on_device == 0 */
} thm_fastq_upload_info;

/* thm_batch_upload_reads for a block of whole FASTQ records as raw bytes (what the file driver cuts its input into):
 * the bytes go up as they are and the device cuts them into names, bases and qualities (needletail's record loop,
 * src/aligner.rs:51-56, for 4-line records).  The device takes the strict form only -- the line count a multiple of 4;
 * with every trailing CR of a line stripped, line 4r non-empty and beginning with '@', line 4r+2 non-empty and beginning
 * with '+', lines 4r+1 and 4r+3 of one length -- and declines everything else; a declined block is parsed on the host,
 * as the driver parses its blocks, and uploaded by thm_batch_upload_reads, or the call returns that parser's
 * THM_ERR_FORMAT and message.  Either way the batch in place, or the error, is what the host parser makes of the bytes.
 * path / first_line (the number of the block's first line in its file) only word error messages; last_block: nothing of
 * the input follows (blank lines are tolerated at its end only).  n == 0: a batch of 0 reads.
 * THM_ERR_INVALID_ARG: null aligner, raw (with n > 0) or info. */
int32_t thm_batch_upload_fastq(thm_aligner* a, const uint8_t* raw, uint64_t n, const char* path, uint64_t first_line,
                               int32_t last_block, thm_fastq_upload_info* info);

/* ------------------------------------------------- BGZF FASTQ inflated and parsed on the device */

typedef struct thm_fastq_bgzf_info {
  uint64_t n_reads, n_bases, n_name_bytes;
  uint64_t n_lines;           /* lines of the block that the batch consumed (a driver's next first_line advances by it) */
  uint64_t n_members;         /* members of the chain as the header walk counts them; 0 where the walk fails (the chain is not
                                 BGZF throughout), whichever side then inflates */
  uint64_t n_inflated_bytes;
  const uint8_t* tail;        /* the block's bytes behind the batch; valid until the next call of this function on `a` */
  uint64_t tail_len;
  uint32_t inflated_on_device, parsed_on_device;
  float inflate_ms, parse_ms; /* HIP-event times; 0 where the host did the step */
} thm_fastq_bgzf_info;

/* thm_batch_upload_fastq for input that is still compressed.  `members` is zero or more whole gzip members back to back
 * and the block is head ++ inflate(members).  With last_block != 0 the batch is the whole block and the tail is empty.
 * Otherwise, with L the block's newline count, the batch is the block's first 4 * (L / 4) lines and the tail is what
 * follows them (the whole block, and a batch of 0 reads, when L < 4).  The batch that ends up uploaded, or the error and
 * its message, is exactly what thm_batch_upload_fastq makes of the batch bytes with the same path, first_line and
 * last_block.  The tail comes back on the host, in one of two buffers used alternately, so that it can be handed in as
 * `head` of the next call on this or any other aligner.
 * The device inflates BGZF only: every member with the header 1f 8b 08, FLG exactly 4 and an extra field with a BC
 * subfield of SLEN 2, BSIZE keeping it inside `members`, the chain ending exactly at n, ISIZE at most 65536, and the raw
 * DEFLATE stream decoding to exactly ISIZE bytes with the trailer's CRC-32.  Anything else -- a plain gzip member, FNAME,
 * a larger ISIZE, a corrupt stream -- is inflated on the host instead, as a whole, and is then that inflater's bytes or
 * its THM_ERR_IO and message: valid gzip the device does not take only costs host time.  The parse step declines to the
 * host parser on its own terms, as in thm_batch_upload_fastq; bytes the device inflated are brought down for it, not
 * inflated again.  THM_ERR_INVALID_ARG: null aligner or info, null members with n > 0, null head with head_len > 0. */
int32_t thm_batch_upload_fastq_bgzf(thm_aligner* a, const uint8_t* head, uint64_t head_len, const uint8_t* members, uint64_t n,
                                    const char* path, uint64_t first_line, int32_t last_block, thm_fastq_bgzf_info* info);

/* ------------------------------------------------- plain gzip FASTQ inflated and parsed on the device */

/* Where a gzip stream stands between two calls: caller-owned, plain data, all zero = the start of a file.  It moves
 * between aligners as the tail does. */
typedef struct thm_gzip_state {
  uint8_t window[32768];  /* the last window_len inflated bytes of the member in progress */
  uint32_t window_len;    /* min(member_len, 32768) while in_member, else 0 */
  uint32_t bit_offset;    /* 0..7: bits of bytes[0] already consumed; 0 when in_member == 0 */
  uint32_t in_member;     /* 1: `bytes` begins (bit_offset bits in) with a DEFLATE block header inside a member;
                             0: `bytes` begins with a gzip member header (or is the end of the input) */
  uint32_t crc;           /* CRC-32 of the member's bytes so far */
  uint64_t member_len;    /* their count */
  uint64_t n_members_done, stream_offset; /* members ended / compressed bytes consumed so far: they only word messages
                             and tell the first member header of a file from what may follow its last member */
} thm_gzip_state;

typedef struct thm_fastq_gzip_info {
  uint64_t n_reads, n_bases, n_name_bytes;
  uint64_t n_lines;           /* as in thm_fastq_bgzf_info */
  uint64_t n_inflated_bytes;
  const uint8_t* tail;        /* the block's bytes behind the batch; valid until the next call of this function on `a` */
  uint64_t tail_len;
  uint32_t inflated_on_device, parsed_on_device;
  float inflate_ms, parse_ms; /* HIP-event times; 0 where the host did the step */
  uint64_t n_consumed_bytes;  /* the next call's `bytes` begins at bytes + n_consumed_bytes */
  uint64_t n_chunks;          /* chunks of compressed bytes the device cut `bytes` into (0 where it was not asked) */
  uint64_t n_starts;          /* ... and the block starts it decoded from, the one the state gives included */
  uint32_t decline_reason;    /* 0, or the status word that sent the inflate to the host */
  uint32_t reserved;
} thm_fastq_gzip_info;

/* thm_batch_upload_fastq_bgzf for ordinary gzip: `bytes` is any n bytes of a gzip stream (RFC 1952 members back to back,
 * each one long DEFLATE stream) that begin where *st says, and need end nowhere in particular.
 * Unit of consumption: the DEFLATE block.  The call consumes every block whose last bit lies inside bytes[0, n) -- a
 * member's final block only together with the 8-byte trailer behind it, a member header only together with its member's
 * first block -- so that between calls the stream stands at a block start inside a member or at a member boundary, which
 * is what *st records.  info->n_consumed_bytes is the byte that holds the next block's first bit (st->bit_offset bits of
 * it are consumed already); the caller presents the stream from there on next time.
 * The block is head ++ the bytes the consumed blocks inflate to; batch, tail, n_lines and the parse step are exactly
 * those of thm_batch_upload_fastq_bgzf for that block, the tail in the same two alternating buffers.
 * A call in which no block ends: n_consumed_bytes == 0, a batch of 0 reads, the head comes back as the tail, *st is
 * unchanged; the caller presents more bytes.
 * last_block != 0: nothing of the input follows bytes[0, n).  Everything must then be consumed and the stream must stand
 * at a member boundary (a stream cut short is the inflater's "truncated stream"); behind the last member may follow
 * what GzInflater accepts there: nothing, or ten bytes or more that do not begin with the gzip magic.
 * Every member's CRC-32 and ISIZE (mod 2^32) are checked, across calls through st->crc / st->member_len.
 * On any error *st is unchanged.
 * The device takes the clean case only (thermite_amd/csrc/gzip_device.h): at most 64 MiB of bytes; a stream in which
 * every decode started at a block start it found ends exactly on the next (so every start was a true one); every such
 * run inflating to at most 16 bytes per byte of its 32 KiB chunks (8 is always taken); at most 4 member ends per
 * chunk; sound members.  Anything else -- a corrupt or odd stream, starts that do not meet, output over the room, more
 * member ends -- declines the inflate as a whole (info->decline_reason) and GzInflater inflates the same bytes by the
 * same rule of consumption: its bytes, or its THM_ERR_IO and message, are then the result.  A stream the device does
 * not take only costs host time.
 * THM_ERR_INVALID_ARG: null aligner, st or info, null bytes with n > 0, null head with head_len > 0, a state whose
 * fields contradict each other. */
int32_t thm_batch_upload_fastq_gzip(thm_aligner* a, thm_gzip_state* st, const uint8_t* head, uint64_t head_len,
                                    const uint8_t* bytes, uint64_t n, const char* path, uint64_t first_line,
                                    int32_t last_block, thm_fastq_gzip_info* info);

/* The uploaded batch back on the host (names, bases as uploaded, qualities -- NULL for a batch uploaded without --, both
 * offset arrays), whichever upload placed it; the view is valid until the next call of this function on the aligner.
 * THM_ERR_INVALID_ARG: no batch with names is uploaded (plain thm_batch_upload carries none). */
int32_t thm_batch_fetch_reads(thm_aligner* a, thm_read_batch* out);

/* -------------------------------------------------------- SAM / PAF writer */

/* OutputFormat, src/aln_writer.rs:16-21 */
enum { THM_FMT_PAF = 0, THM_FMT_SAM = 1, THM_FMT_BAM = 2 };

typedef struct thm_text {
  const uint8_t* data;
  uint64_t len;
} thm_text;

typedef struct thm_writer thm_writer;
/* n_threads formatting threads (0 = hardware concurrency, at most 16; explicit values up to 32) */
int32_t thm_writer_create(const thm_index* ix, int32_t format, uint32_t n_threads, thm_writer** out);
void thm_writer_free(thm_writer* w);
/* build_sam_header, src/aln_writer.rs:256-276 (empty for PAF; for BAM the
 * BGZF-compressed magic + header text + reference list of bam::Writer::write_header
 * / write_reference_sequences, src/aligner.rs:41-46) */
int32_t thm_writer_header(thm_writer* w, thm_text* out);
/* the same with "@HD\tVN:1.6\tSO:coordinate\n" as the first line of the header text (for BAM l_text counts it): the
 * header of a file whose records come from a thm_bam_sorter.  Empty for PAF. */
int32_t thm_writer_header_sorted(thm_writer* w, thm_text* out);
/* what closes the file: the BGZF end-of-file block for BAM, nothing otherwise */
int32_t thm_writer_trailer(thm_writer* w, thm_text* out);
/* aln_to_sam_record / unmapped_sam_record / PafEntry, src/aln_writer.rs:47-253,
 * applied in the order of the writer loop src/aligner.rs:58-115: the records
 * of `reads` rendered from `result` (= what thm_align_batch / thm_batch_fetch
 * returned for exactly these reads).  For BAM the result is a run of complete
 * BGZF blocks (records re-encoded in binary, bam::Writer::write_sam_record,
 * src/aligner.rs:69-76,98-108).  Text valid until the next call on `w`. */
int32_t thm_writer_format_batch(thm_writer* w, const thm_read_batch* reads, const thm_batch_view* result, thm_text* out);
/* The same records from a thm_cigar_view -- thm_batch_fetch_cigars / thm_align_batch_cigars for exactly these reads:
 * byte for byte what thm_writer_format_batch gives for the full view of the same batch.  The CIGAR column and the
 * TX:Z CIGAR (to_noodles_cigar, src/aln_writer.rs:279-323; :176-186) are printed from the words, BAM copies them; nM
 * (:160-168), PafEntry's num_match / num_match_gap (:55-72) and the BAM bin come from the digest.  An alignment whose
 * digest carries a flag (a run of 2^28 or more has no word) cannot be rendered: THM_ERR_INTERNAL. */
int32_t thm_writer_format_batch_cigars(thm_writer* w, const thm_read_batch* reads, const thm_cigar_view* result, thm_text* out);

/* BAM writers only: the records of a thm_bam_view as a run of complete BGZF blocks.  The bytes are cut into read
 * ranges by read_rec_off over the writer's threads, as thm_writer_format_batch cuts the reads, and deflated by the
 * same code (THM_BAM_LEVEL honoured): inflated, the output equals view->data.  THM_ERR_INVALID_ARG: another format,
 * offsets that do not start at 0, descend or end elsewhere than n_bytes.  Text valid until the next call on `w`. */
int32_t thm_writer_wrap_bam(thm_writer* w, const thm_bam_view* view, thm_text* out);

/* ------------------------------------------------------ whole-file driver */

typedef struct thm_run_stats {
  uint64_t n_reads;
  uint64_t n_aligned_reads;
  uint64_t n_records;
  uint64_t n_batches;
  uint64_t n_output_bytes;
  double parse_s;  /* summed over batches; stages overlap, so the sum exceeds wall_s */
  double gpu_s;    /* upload + run + sync + fetch                                    */
  double format_s;
  double write_s;
  double wall_s;
} thm_run_stats;

/* align_reads_from_file, src/aligner.rs:22-120: every record of every FASTQ in
 * order -> output_path ("-" = stdout).  Three overlapped stages (parse | GPU |
 * format+write) over batches of `batch_reads` reads (0 = 250 000).
 * THM_BAM_DEVICE=1 in the environment and THM_FMT_BAM: the records are encoded on the device
 * (thm_batch_upload_reads / thm_batch_fetch_bam) and the formatting stage only deflates (thm_writer_wrap_bam);
 * the file's inflated bytes are the same.
 * THM_BAM_DEVICE=2 and THM_FMT_BAM: the records are encoded and BGZF-compressed on the device (thm_batch_fetch_bgzf)
 * and the formatting stage only passes the members on; the file's inflated bytes are the same again, the compressed
 * ones are the device encoder's (THM_BAM_LEVEL does not apply), and n_output_bytes counts them.
 * THM_FASTQ_DEVICE=1 together with THM_FMT_BAM and THM_BAM_DEVICE=1 or 2 (the modes in which the host needs no read
 * bytes; ignored otherwise): the blocks of 4-line FASTQ input are not parsed by the parser threads but go to the device
 * as they are (thm_batch_upload_fastq); the output file is the same byte for byte.
 * THM_FASTQ_DEVICE=2, in the same two modes: as =1, and an input file that is BGZF throughout -- gzip magic, every member
 * of its chain with the BGZF header, the chain ending exactly at the end of the file, the first member inflating to
 * text that begins with '@' -- is not inflated on the host either: it is mapped, cut into groups of whole members of
 * about batch_reads reads (by the bytes per record of the batches so far, one member at least; a batch may hold more
 * reads than batch_reads) and every group goes to the device compressed (thm_batch_upload_fastq_bgzf), the tail of one
 * batch being the head of the next, across aligners in input order.  The file's inflated bytes are the same; batch
 * boundaries, and with THM_BAM_DEVICE=2 the compressed bytes, may differ.  Every other file takes the path of =1.
 * THM_FASTQ_DEVICE=3, in the same two modes: as =2 (files that are BGZF throughout keep that path), and a gzip file that
 * is not BGZF throughout gets no inflater thread either, provided its first bytes, inflated on the host, begin with '@':
 * it is mapped and goes to the device in slices (thm_batch_upload_fastq_gzip), sized from the bytes per record and the
 * compression ratio of the batches so far, each beginning at the last one's n_consumed_bytes, doubled while nothing of
 * one is consumed, last_block set on the slice that reaches the end of the file; state and tail pass along the same
 * in-order chain of uploads and are reset per file.  The file's inflated bytes are those of the unset run; batch
 * boundaries may differ.  FASTA and input that is not gzip keep the path of =1.
 * THM_BAM_SORT=1 and THM_FMT_BAM (ignored for the other formats): the file is coordinate-sorted.  Batches go up as with
 * THM_BAM_DEVICE=1 (THM_FASTQ_DEVICE=1..3 apply as there) and their records stay on the device (thm_bam_sorter_add);
 * nothing is formatted or written until the input is exhausted.  Then the records are sorted (thm_bam_sorter_finish),
 * thm_writer_header_sorted is written, the windows of thm_bam_sorter_next follow -- window k being written while the
 * device produces window k + 1 -- and the end-of-file block closes the file.  Inflated, the file is the sorted header and
 * the records of the unset run in the order of thm_bam_sorter; the members are the device encoder's.  n_output_bytes
 * counts the file's bytes; the drain's time goes into format_s (sort, gather, deflate, copy) and write_s.  One aligner
 * only: with more, THM_ERR_INVALID_ARG (merging across devices is not done).  Records beyond the device's memory:
 * THM_ERR_OOM from the add that meets it.
 * THM_BAM_INDEX=1 beside THM_BAM_SORT=1: after the end-of-file block, <output_path>.bai is written whole
 * (thm_bam_sorter_index with the length of the sorted header); a failure to write it is THM_ERR_IO with the path.
 * n_output_bytes still counts the BAM only.  THM_FMT_BAM with THM_BAM_INDEX=1 but without THM_BAM_SORT=1, or to standard
 * output, is refused with THM_ERR_INVALID_ARG: only a sorted file has this index.  Ignored for the other formats.
 * THM_QUANT=1, in every format and mode: every aligner keeps a thm_quant and every batch is added to it after its run
 * (thm_quant_add); the output file is the unset run's byte for byte.  At the end two files are written whole:
 * <output_path>.genes.tsv -- the header line gene_id, gene_name, exonic_unique, exonic_multi, intronic_unique,
 * intronic_multi, then one line per gene in index order -- and <output_path>.junctions.tsv -- the header line ref, start,
 * end, strand, unique, multi, max_overhang, then one line per row, start and end the 1-based first and last base of the
 * intron, strand + or -; both tab-separated.  With several aligners their tables are merged on the host by key (counts
 * summed, overhang maximum), so the files do not depend on how the reads were dealt.  A failure to write one is THM_ERR_IO
 * with the path; to standard output the knob is refused with THM_ERR_INVALID_ARG.  thm_run_stats is unchanged.
 * THM_COVERAGE=1, 2 or 3, in every format and mode, beside THM_QUANT or without it: every aligner keeps a thm_coverage and
 * every batch is added to it after its run (thm_coverage_add); the output file is the unset run's byte for byte.
 * THM_COVERAGE=1: the unique alignments, both strands together; =2: THM_COV_STRANDED; =3: THM_COV_STRANDED | THM_COV_MULTI.
 * At the end every track is fetched contig by contig and written whole as <output_path>.cov.<track>.bedgraph, <track> one
 * of unique, unique.fwd, unique.rev, multi, multi.fwd, multi.rev: lines "name<TAB>start<TAB>end<TAB>depth", 0-based and
 * half open, contigs in @SQ order, no line of depth 0, no header.  With several aligners their run lists are merged on
 * the host (depths summed, abutting stretches of equal depth fused), so the files do not depend on how the reads were
 * dealt.  A failure to write one is THM_ERR_IO with the path; to standard output the knob is refused with
 * THM_ERR_INVALID_ARG.  thm_run_stats is unchanged.
 * THM_PILEUP=1 or 2, in every format and mode, beside THM_QUANT / THM_COVERAGE or alone: the aligner keeps a thm_pileup and
 * every batch is added to it after its run (thm_pileup_add); the output file is the unset run's byte for byte.
 * THM_PILEUP=1: the unique alignments; =2: THM_PILE_MULTI; any other value but 0, or a THM_PILEUP_MIN_ALT that is no number of
 * 1 or more, is refused with THM_ERR_INVALID_ARG.  At the end the sites with alt >= THM_PILEUP_MIN_ALT (default
 * 2, at least 1) are fetched and written as <output_path>.pileup.tsv: the header line "#contig pos ref depth A C G T N
 * del ins", then one line per site, tab-separated, pos 1-based, contigs in @SQ order.  A failure to write it is
 * THM_ERR_IO with the path; to standard output, and with more than one aligner (merging needs the depth of one device at
 * the sites of another, which is not done), the knob is refused with THM_ERR_INVALID_ARG.
 * THM_CELLS=1 or 2, in every format and mode, beside the other summaries or alone: the aligner keeps a thm_cells and every
 * batch is added to it after its run (thm_cells_add); every batch goes up with its names (thm_batch_upload_reads where
 * the host formats SAM or PAF), and the output file is the unset run's byte for byte.  THM_CELLS=1: exonic reads only;
 * =2: THM_CELLS_INTRONIC.  THM_CELLS_CB_LEN (default 16) and THM_CELLS_UMI_LEN (default 12) are the tag's lengths, each
 * 1..16; THM_CELLS_MIN_UMIS (default 1, at least 1) is the fetch's min_umis.  Any other THM_CELLS but 0, or one of the
 * three that is no such number, is refused with THM_ERR_INVALID_ARG.  At the end three files are written whole:
 * <output_path>.cells.mtx -- the line "%%MatrixMarket matrix coordinate integer general", the line "n_genes n_cells
 * n_entries", then one line "gene+1 cell+1 n_umis" per entry in the entries' order --, <output_path>.cells.barcodes.tsv
 * -- the unpacked barcode of every cell, a line each -- and <output_path>.cells.features.tsv -- gene_id, gene_name and
 * "Gene Expression", tab-separated, a line per gene in index order.  A failure to write one is THM_ERR_IO with the path;
 * to standard output, and with more than one aligner (the tables of two devices hold reduced counts: their distinct
 * molecules are those of the union of their rows, which is not formed), the knob is refused with THM_ERR_INVALID_ARG.
 * thm_run_stats is unchanged. */
int32_t thm_align_files(thm_aligner* a, const char* const* fastq_paths, uint32_t n_paths, const char* output_path,
                        int32_t format, uint64_t batch_reads, uint32_t n_threads, thm_run_stats* stats);
/* The same over several aligners -- one per GPU of the node, all over one index (the shape of ThermiteAligner: Clone +
 * Send over Arc<Index>, src/wrapper.rs:20-27): batches are dealt to the aligners in input order, each aligner is
 * driven by its own host thread, parsing runs on several threads, and the records still leave in input order
 * (src/aligner.rs:54-115).  thm_align_files is this call with one aligner. */
int32_t thm_align_files_multi(thm_aligner* const* aligners, uint32_t n_aligners, const char* const* fastq_paths, uint32_t n_paths,
                              const char* output_path, int32_t format, uint64_t batch_reads, uint32_t n_threads,
                              thm_run_stats* stats);

#ifdef __cplusplus
}
#endif
#endif
