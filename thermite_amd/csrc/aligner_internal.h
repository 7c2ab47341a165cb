// aligner_internal.h -- host-side state shared by aligner.hip, pipeline.hip and the other host files.
#ifndef THERMITE_ALIGNER_INTERNAL_H
#define THERMITE_ALIGNER_INTERNAL_H
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>
#include <type_traits>
#include <vector>

#include "launch.h"
#include "thermite_internal.h"

// Ownership: a DBuf, an HBuf, an Event and a Stream each free what they hold when they are destroyed, and none of them
// can be copied, so `delete` of the struct that holds them (thm_aligner, thm_index::DevCopy) is the whole clean-up and a
// new member needs no entry anywhere.

// grow-only device buffer
struct DBuf {
  void* p = nullptr;
  size_t cap = 0;
  DBuf() = default;
  DBuf(const DBuf&) = delete;
  DBuf& operator=(const DBuf&) = delete;
  ~DBuf() { release(); }
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    release();
    size_t want = bytes + bytes / 4 + 256;
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const {
    return (T*)p;
  }
};

// a fixed part of another DBuf (the control block's words): same accessors, nothing to grow or free
struct DView {
  void* p = nullptr;
  size_t cap = 0;
  template <class T>
  T* as() const {
    return (T*)p;
  }
};

// grow-only pinned host buffer (results land here: D2H at full PCIe rate, no value-initialisation)
struct HBuf {
  void* p = nullptr;
  size_t cap = 0;
  HBuf() = default;
  HBuf(const HBuf&) = delete;
  HBuf& operator=(const HBuf&) = delete;
  ~HBuf() { release(); }
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    release();
    size_t want = bytes + bytes / 4 + 4096;
    hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const {
    return (T*)p;
  }
};
static_assert(!std::is_copy_constructible_v<DBuf> && !std::is_copy_assignable_v<DBuf>, "one owner per device allocation");
static_assert(!std::is_copy_constructible_v<HBuf> && !std::is_copy_assignable_v<HBuf>, "one owner per pinned allocation");

// an event of the aligner's: made by the first ensure(), passed to the HIP calls as the hipEvent_t it holds
struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() {
    if (e) (void)hipEventDestroy(e);
  }
  hipError_t ensure(bool timed = true) {
    if (e) return hipSuccess;
    return timed ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, hipEventDisableTiming);
  }
  operator hipEvent_t() const { return e; }
};
template <size_t N>
inline hipError_t ensure_events(Event (&ev)[N]) {
  for (Event& e : ev)
    if (hipError_t r = e.ensure(); r != hipSuccess) return r;
  return hipSuccess;
}
// milliseconds from `from` to `to` into *ms, once the stream that recorded them has been synchronised; false, and *ms as
// it was, where HIP cannot tell
inline bool elapsed_ms(const Event& from, const Event& to, float* ms) {
  float t = 0;
  if (hipEventElapsedTime(&t, from, to) != hipSuccess) return false;
  *ms = t;
  return true;
}
// ... of two passes with a synchronisation between them: ev[0] to ev[1] plus ev[2] to ev[3], or false as above
inline bool elapsed_ms(const Event (&ev)[4], float* ms) {
  float m1 = 0, m2 = 0;
  if (!elapsed_ms(ev[0], ev[1], &m1) || !elapsed_ms(ev[2], ev[3], &m2)) return false;
  *ms = m1 + m2;
  return true;
}

// a non-blocking stream of the aligner's, made by create()
struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() {
    if (s) (void)hipStreamDestroy(s);
  }
  hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
  operator hipStream_t() const { return s; }
};

struct thm_index::DevCopy {
  int device = -1;
  DBuf text, sa, lut, refs, name_rank, ref_recs, ref_bin, txs, exons, exon_txoff, tx_seq, exon_grid_off, exon_grid, gene_grid_off, gene_grid;
  bool wide = false;                     // which of the two views is valid (thermite_internal.h, "Coordinate width")
  // lut_direct.h: the pass that runs once behind the upload put text positions into the single-suffix entries of `lut`
  // (THM_LUT_DIRECT=0, or a 32-bit table over 2^31 symbols or more: plain); how many entries it rewrote
  bool lut_direct = false;
  uint64_t lut_tagged = 0;
  DBuf lut_cnt;                          // the pass's counter (one u64)
  thm::DeviceIndexT<uint32_t> view;
  thm::DeviceIndexT<uint64_t> view64;
};

inline void free_dev_copy(thm_index::DevCopy* d) {
  if (!d) return;
  int cur = 0;
  (void)hipGetDevice(&cur);
  (void)hipSetDevice(d->device);
  delete d;
  (void)hipSetDevice(cur);
}

// The opt-in problem-parallel path of the extend stage (pipeline_tpr.hip; kernels_tpr.hip: thread-per-read control kernel
// + wave-per-request DP kernels, in rounds, ahead of the wave-per-read kernels, which take what is left): everything only
// that path uses.  THM_TPR=1 or thm_debug_set_flags turn it on; THM_TPR_ROUNDS = 1..8.
// It holds streams, so thm_aligner declares it among its streams, in front of every buffer and event of its own: the
// aligner's buffers that stream3 and stream4 worked on are freed before this struct is destroyed, and within it the
// streams stand first for the same reason (buffers, then events, then streams go).
struct TprState {
  Stream stream3;  // the wave-per-read and team kernels run beside the rounds
  Stream stream4;  // the thread-per-problem DP kernel of a round runs beside the wave-per-problem one
  Event ev_join3, ev_dpt_fork, ev_dpt_join;  // untimed, made by thm_aligner_create
  DBuf t_memos, t_recs, t_dpops, t_qlist, t_act[2], t_ctl, t_bail, t_queue2, t_trace, t_ttrace, t_hdr, t_sums;
  bool use_tpr = false;  // (until the path is the faster one on the headline workload)
  int tpr_rounds = 8;
};

struct thm_aligner {
  const thm_index* ix = nullptr;
  thm_index::DevCopy* dix = nullptr;
  int device = 0;
  int n_cu = 256;
  // The streams stand in front of every buffer and event: members are destroyed in reverse order, so the streams go last,
  // after what their work may still have touched has been freed (thm_aligner_free synchronises them first).
  Stream stream;
  Stream stream2;  // the team kernel runs beside the wave-per-read kernel
  TprState tpr;    // (two more streams: see the struct)
  Event ev_fork, ev_join;  // untimed, made by thm_aligner_create
  thm_align_opts opts;
  // the options thm_batch_run started the current run with: every replay of that run (thm_batch_sync, after a pool
  // overflow) runs under them again, whatever thm_aligner_set_opts has been given since
  thm_align_opts run_opts;
  std::string err;

  DBuf d_counters;
  // Control block: every word a run of the read-level pipeline wants zeroed when it starts, side by side, so that the
  // run's first kernel zeroes them in one go (launch.h, RunResetParams).  The views below are its parts.
  DBuf d_ctl;
  static constexpr size_t CTL_WORK_COUNTS = 0, CTL_CURSORS = 128, CTL_FAULT = 192, CTL_QUEUE = 256,
                          CTL_QUEUE_EXT = CTL_QUEUE + thm::QUEUE_BYTES, CTL_BYTES = CTL_QUEUE_EXT + thm::QUEUE_BYTES;
  static_assert(CTL_BYTES % 16 == 0 && thm::QUEUE_BYTES % 16 == 0, "the block is zeroed 16 bytes at a time");
  DView d_queue;      // work counters of the seed stage's selection kernel and of the operator-level calls
  DView d_queue_ext;  // ... of the extend stage: its own words, so that one reset serves both stages of a run
  DView d_fault, d_cursors;  // cursors: [0] smem pool head, [1] op pool head (u64 each)
  DView s_work_counts;       // list lengths of the seed stage and of the plan kernel (16 u64)
  DBuf b0, b1, b2, b3, b4, b5, b6, b7, b8;       // operator-level scratch

  // ---- read-level pipeline ----
  DBuf r_bases, r_offsets, r_san;  // raw reads, offsets, upper-cased + sanitised copy (made by every run)
  DBuf r_status;                   // per-read status (i32), zeroed by every run
  uint64_t n_reads = 0, n_bases = 0;
  uint32_t max_read_len = 0;
  // lengths present in the batch, ascending, with their read counts (thm_batch_upload): the length classes of a
  // run (which reads the register-resident kernels take) depend on the options, which may change between runs
  std::vector<std::pair<uint32_t, uint64_t>> len_hist;
  uint64_t n_over = 0;  // reads longer than MAX_READ_LEN (per-read status THM_ERR_UNSUPPORTED)
  bool uploaded = false;
  // seeds
  DBuf s_smems, s_off, s_cnt, s_hits, s_cand_off, scan_tmp, s_ms_end, s_ms_lo, s_ms_hi, s_work_reads, s_work_long, s_work_cells,
      s_sel_scratch, s_heavy, s_slow, s_team, s_fill_keys, s_fill_perm, s_fill_hist;
  uint64_t smem_cap = 0;
  // extension
  DBuf e_heavy, e_rel;  // compact stage: lists of reads with many alignments, op offsets of their alignments
  DBuf e_cands, e_order, e_ops, e_nalns, e_opbytes, e_aln_off, e_ops_off, e_trace, e_slow, e_recs, e_wcnt;
  // e_wcnt (the waves' counter rows) is zero from end to end between runs: launch_counters_reduce zeroes what it read, so
  // only a new allocation is zeroed by the host.  The capacity that is known clean (0 while a run's launches are being
  // enqueued: an enqueue that fails half way leaves rows nobody reduced)
  size_t wcnt_clean_cap = 0;
  uint64_t n_slow_host = 0;     // reads of the slow class in the last enqueue (host count)
  uint32_t fast_max_len = 0, slow_max_len = 0;
  uint64_t cand_cap = 0, cand_ops_cap = 0;
  // compacted outputs
  DBuf o_alns, o_ops, o_mems;
  // out_alns_cap, out_ops_cap: cand_cap and cand_ops_cap as the last enqueued run had them, which is what a fetch checks the
  // batch against (thm_debug_set_pool_caps zeroes those two for the next run while this one's views are still being fetched)
  uint64_t out_alns_cap = 0, out_ops_cap = 0;
  // test hook (thm_debug_set_pool_caps): initial pool sizes instead of the heuristics, to force the grow-and-replay path
  uint64_t dbg_smem_cap = 0, dbg_cand_cap = 0, dbg_ops_cap = 0;
  uint32_t dbg_band_clip = 0;  // test hook (thm_debug_set_band_clip): pretend the fast class holds bands up to this only (0: off)
  // test / tuning hook (thm_debug_set_flags bits 2, 3): seed probes never decided from the table entry and a neighbouring
  // match; seed probes counted (thm_debug_seed_stats)
  bool dbg_seed_noinfer = false, dbg_seed_stats = false;
  // ... bit 6: a probe into a single-suffix bucket reads sa[lo] although the table entry holds the text position
  bool dbg_seed_nodirect = false;
  // The finisher (kernels_finish.hip): classes it takes (thm_debug_set_flags bits 12..15; fin::CLASS_E | fin::CLASS_S), the
  // read-only op run at the front of e_ops (where it was written and for which read length, 0: none; while it exists every
  // run starts the pool's cursor behind it), the classes and workgroups of the last enqueue, its per-workgroup statistics
  uint32_t fin_classes = 3;
  const void* ops_run_ptr = nullptr;
  size_t ops_run_cap = 0;
  uint32_t ops_run_half = 0;
  uint32_t fin_run_classes = 0, fin_blocks = 0;
  DBuf e_finstats;
  uint32_t n_replays = 0;  // pool-overflow replays since the aligner was created
  bool ran = false, synced = false;
  Event ev[6];  // made by thm_aligner_create
  float timings[THM_N_TIMINGS] = {0};

  // host results of the read-level path: two pinned sets used alternately, so that the view
  // thm_batch_fetch returned stays valid while the next batch is uploaded, run and fetched
  HBuf r_off[2], r_alns[2], r_ops[2], r_stat[2];
  int r_cur = 0;
  // host results of the operator- and seed-level calls
  std::vector<uint64_t> h_off;
  std::vector<thm_aln> h_alns;
  std::vector<uint8_t> h_ops;
  std::vector<thm_mem> h_mems;
  std::vector<thm_swg_aln> h_swg;
  std::vector<thm_lr_aln> h_lr;
  // per-hit entry point (seed_hits.hip): device buffers and the host result its view points into
  DBuf sh_bases, sh_san, sh_off, sh_hits, sh_read, sh_bw, sh_xd, sh_list, sh_out, sh_status, sh_ops, sh_ctl, sh_trace, sh_slow;
  std::vector<thm_aln> h_hit_alns;
  std::vector<int32_t> h_hit_status;
  std::vector<uint8_t> h_hit_ops;
  // CIGAR entry points (cigar.hip): per-stream sums and word counts, their scan, digests and words on the device; the
  // uploaded streams of thm_cigar_encode_batch; two pinned host sets of thm_batch_fetch_cigars, used alternately and
  // apart from r_off .. r_stat, so that neither fetch invalidates the other's view
  DBuf c_sums, c_nwords, c_woff, c_scan_tmp, c_flags, c_dig, c_words, c_in_ops, c_in_off;
  HBuf ch_off[2], ch_alns[2], ch_dig[2], ch_words[2], ch_stat[2];
  int c_cur = 0;
  Event ev_cig[4];  // made by the first call
  std::vector<thm_aln_digest> h_cig_dig;
  std::vector<uint32_t> h_cig_words;
  // BAM records on the device (bam.hip): names and qualities of the batch (thm_batch_upload_reads), the index's name
  // tables (uploaded by the first thm_batch_fetch_bam), work arrays of the passes, the records, and two pinned host
  // sets of their own, used alternately
  DBuf bn_names, bn_name_off, bn_quals;
  bool reads_named = false, reads_have_quals = false;  // thm_batch_upload clears reads_named
  DBuf bt_tx_pool, bt_tx_off, bt_gid_pool, bt_gid_off, bt_gname_pool, bt_gname_off, bt_tx_gene, bt_ref_sq;
  bool bam_tables = false;
  DBuf bm_cnt, bm_first, bm_qn, bm_rec_read, bm_len, bm_off, bm_out, bm_read_off, bm_err, bm_scan_tmp;
  HBuf bh_data[2], bh_off[2], bh_stat[2];
  int b_cur = 0;
  int bam_stage = -1;  // emit through LDS and dword stores (1) or byte stores (0); -1: not read from THM_BAM_EMIT yet
  Event ev_bam[4];  // made by the first call
  // BGZF members on the device (bgzf.hip): per-position scratch of the workgroups, the members in their slots, their
  // sizes and the scan, the members behind one another; the bytes thm_debug_bgzf_device uploads; two pinned host sets
  // of their own, used alternately
  DBuf bz_match, bz_slots, bz_sizes, bz_off, bz_out, bz_scan_tmp, bz_dbg_in;
  HBuf zh_data[2], zh_off[2], zh_stat[2];
  int z_cur = 0;
  Event ev_bgzf[2];  // made by the first call
  // FASTQ blocks parsed on the device (fastq.hip): the block's bytes, newline counts per chunk and their scan, the line
  // starts, the records' lengths and the flag word; the offsets come back into fq_h_off for the length classes.  The
  // blocks that went either way since the aligner was created (thm_debug_fastq_device_blocks).  One pinned set behind
  // thm_batch_fetch_reads.
  DBuf fq_raw, fq_cnt, fq_base, fq_lines, fq_name_len, fq_seq_len, fq_flag, fq_scan_tmp;
  HBuf fq_h_off;
  uint64_t fq_on_device = 0, fq_on_host = 0;
  Event ev_fq[6];  // made by the first call
  HBuf fr_bases, fr_off, fr_quals, fr_names, fr_name_off;
  // BGZF members inflated on the device (inflate.hip): the members' bytes, the host's table of them and their status
  // words (the table and the statuses in pinned memory too); the inflated block is built in fq_raw.  Two tail buffers,
  // used alternately; the block on the host where the host inflated or parsed it.  Counts for
  // thm_debug_fastq_bgzf_blocks: inflates on device / on host, parses on device / on host.
  DBuf fz_in, fz_tab, fz_status;
  HBuf fz_h_tab, fz_h_status, fz_tail[2], fz_h_last;
  int fz_cur = 0;
  std::vector<uint8_t> fz_block;
  uint64_t fz_counts[4] = {0, 0, 0, 0};
  Event ev_fz[2];  // made by the first call
  // plain gzip inflated on the device (gzip.hip; the arrays of gz::Job, gzip_device.h): the compressed bytes, both
  // states, candidates, runs, member ends, symbol regions, windows and what the chain derives; summary and outgoing
  // state in pinned memory too.  The inflated block is built in fq_raw and the tail buffers are fz_tail.  Counts for
  // thm_debug_fastq_gzip_blocks, as fz_counts.
  DBuf gz_in, gz_state, gz_cand, gz_runs, gz_ends, gz_syms, gz_windows, gz_run_list, gz_run_off, gz_end_abs, gz_end_crc, gz_end_isize,
      gz_member_crc, gz_sum;
  HBuf gz_h_sum, gz_h_state;
  uint64_t gz_counts[4] = {0, 0, 0, 0};
  Event ev_gz[2];  // made by the first call
};

inline int fail(thm_aligner* a, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (a) a->err = buf;
  thm::set_global_error(buf);
  return code;
}

#define HIPCHK(a, call)                                                                             \
  do {                                                                                              \
    hipError_t e_ = (call);                                                                         \
    if (e_ != hipSuccess)                                                                           \
      return fail(a, e_ == hipErrorOutOfMemory ? THM_ERR_OOM : THM_ERR_HIP, "%s failed: %s (%s:%d)", \
                  #call, hipGetErrorString(e_), __FILE__, __LINE__);                                \
  } while (0)

// cigar.hip: count -> scan -> emit over the streams of `p`; results in c_dig / c_words (synchronises the stream once)
int run_cigar_passes(thm_aligner* a, thm::CigarParams p, uint64_t n_digests, uint64_t* n_words, unsigned* any_flags);
// bam.hip: everything of thm_batch_fetch_bam up to the copies -- after it the records of the run are in bm_out on the
// device and the per-read byte offsets in bm_read_off (both fetches that hand records out start here; the messages name
// thm_batch_fetch_bam whichever it is).  Of the timings only `timing`, the caller's own, is touched: zeroed once the
// arguments have passed; ev_bam[0..3] are left recorded around the size and emit passes.
struct BamOnDevice {
  uint64_t n_reads = 0, n_alns = 0, n_records = 0, n_bytes = 0;
  bool any_failed = false;  // as in BatchSizes
};
int bam_records_on_device(thm_aligner* a, uint32_t flags, int timing, BamOnDevice* r);
// bam.hip: the index's name tables, tx -> gene (bt_tx_gene) and ref -> BAM refID (bt_ref_sq) on the device, once per aligner
// (the aligner's device is current).  THM_ERR_INVALID_ARG: an index without names.  quant.hip counts from the last two.
int bam_tables_on_device(thm_aligner* a);
// bgzf.hip: d_in[0, n) (device, 4-byte aligned) cut every 0xff00 bytes and deflated -> the members back to back in bz_out,
// their offsets in bz_off[0 .. *n_blocks]; synchronises the stream once and sets THM_T_BGZF (bam_sort.hip deflates the
// windows of the sorted stream through it)
int bgzf_range_on_device(thm_aligner* a, const uint8_t* d_in, uint64_t n, uint64_t* n_blocks, uint64_t* n_bytes);
// ---- pipeline.hip: the head and the tail of every fetch entry point (after thm_batch_sync; a new one calls all of them)
struct BatchSizes {
  uint64_t n_alns = 0, n_ops = 0;  // alignments and op bytes of the compacted batch, checked against the pools
  bool any_failed = false;         // a read of the batch may have failed: the statuses are worth copying
};
// One round trip (a single synchronisation of the stream): e_aln_off[n], e_ops_off[n] and the device's count of
// out-of-contract reads.  With `h_off` the whole offsets array comes into it, (n + 2) words with the op bytes last; with
// `d_extra` that device word comes into *extra.
int fetch_batch_sizes(thm_aligner* a, HBuf* h_off, const uint64_t* d_extra, uint64_t* extra, BatchSizes* z);
// r_status on its way into `h_stat` where any_failed says so; after the next synchronisation failed_reads fills the two
// fields of a view from it: the count of reads that failed, and the statuses where there is one (else null)
int enqueue_statuses(thm_aligner* a, bool any_failed, HBuf& h_stat);
void failed_reads(const thm_aligner* a, bool any_failed, const HBuf& h_stat, uint64_t* n_failed, const int32_t** status);
// the two op streams of every alignment in the compacted pool, for run_cigar_passes
thm::CigarParams compacted_cigar_params(const thm_aligner* a, const BatchSizes& z);
// pipeline.hip: what thm_batch_upload derives from the offsets of a batch -- n_reads, n_bases, max_read_len, the length
// classes (len_hist) and n_over -- for every upload path; THM_ERR_INVALID_ARG for offsets that do not start at 0 or descend
int batch_length_classes(thm_aligner* a, const uint64_t* offsets, uint64_t n_reads);
// fastq.hip: the device FASTQ parse (count, starts, records, gather) of a block of n > 0 bytes that stands in fq_raw,
// which the caller has sized to n + 64 -- put there by a copy (thm_batch_upload_fastq) or by the device inflater
// (inflate.hip).  Three synchronisations of the stream, whichever it is.
struct FastqBlock {
  uint64_t n = 0;
  const uint8_t* host = nullptr;  // the block's bytes on the host; null: its last byte comes down with the newline total
  bool whole = true;              // the batch is the whole block; false: its first 4 * (newlines / 4) lines
  const uint32_t* d_status = nullptr;  // status words of an inflate (device), checked at the first synchronisation
  uint64_t n_status = 0;
  HBuf* tail = nullptr;  // where the bytes behind the batch go, in the copy-back the gather ends with (null: not wanted)
  // results
  uint64_t bad_member = 0;  // FQ_NOT_INFLATED: the first member with a status other than 0 (the word is in fz_h_status)
  uint64_t n_newlines = 0;
  uint64_t cut = 0;         // bytes of the batch (valid once the call returns 0 or 1)
  uint64_t n_reads = 0, n_bases = 0, n_name_bytes = 0;
  float ms = 0;
};
enum { FQ_NOT_INFLATED = 2, FQ_NO_RECORD = 3 };  // beside 1 (parsed), 0 (declined: the host parser's) and errors (< 0)
// What an upload entry point (thm_batch_upload_fastq, ..._bgzf, ..._gzip) made of its block; each copies it into its own
// public info struct.
struct FastqOutcome {
  uint64_t n_reads = 0, n_bases = 0, n_name_bytes = 0;
  uint64_t n_lines = 0;  // lines of the block that the batch consumed
  const uint8_t* tail = nullptr;  // the block's bytes behind the batch (in the HBuf handed in)
  uint64_t tail_len = 0;
  uint32_t parsed_on_device = 0;
  float parse_ms = 0;
  // a parse_resident that returned 1
  void take(const FastqBlock& b) {
    n_reads = b.n_reads, n_bases = b.n_bases, n_name_bytes = b.n_name_bytes;
    n_lines = 4 * b.n_reads;
    parse_ms = b.ms;
    tail_len = b.n - b.cut;
  }
};
namespace thm {
int parse_resident(thm_aligner* a, FastqBlock& b);
// fastq.hip, the finish the three entry points share.
// A block that stands on the host: copied into fq_raw and parsed there (parse_resident's codes).  On 1 `o` holds the
// counts and the cut, and the bytes behind it are in `tail` (null: the batch is the whole block).
int parse_host_block(thm_aligner* a, const uint8_t* blk, uint64_t n, bool whole, HBuf* tail, FastqOutcome& o);
// The device parsed the batch: the aligner's batch state, and o.tail.
void batch_parsed_on_device(thm_aligner* a, HBuf* tail, FastqOutcome& o);
// The host parser's batch of a block the device did not parse: the batch bytes -- all of the block for a last block or
// with no `tail`, else up to fastq_host_cut -- through fastq_parse_block and thm_batch_upload_reads, the lines and the
// tail into `o`; *on_host counts a batch that has bytes.  The parser's error goes into a->err and the global error.
int host_parser_batch(thm_aligner* a, const uint8_t* blk, uint64_t n, const std::string& path, uint64_t first_line, bool last_block,
                      HBuf* tail, uint64_t* on_host, FastqOutcome& o);
}
int reset_queue(thm_aligner* a);
inline int grid_blocks(const thm_aligner* a, uint64_t n_items, int waves_per_block, int blocks_per_cu) {
  return thm::grid_blocks(a->n_cu, n_items, waves_per_block, blocks_per_cu);
}
// ---- the extend stage's launches (pipeline.hip, pipeline_tpr.hip) over one run's thm::ExtendPlan ----
// where a launch's waves leave their counters: row `row` of e_wcnt (the plan's row_* offsets)
inline unsigned long long* counter_rows(const thm_aligner* a, uint64_t row) { return a->e_wcnt.as<unsigned long long>() + row * THM_N_COUNTERS; }
// the team kernel's parameter block: `p` over the team list only, with the team's own counter rows and trace slices
template <class C>
thm::ExtendParamsT<C> team_params(const thm_aligner* a, const thm::ExtendPlan& plan, thm::ExtendParamsT<C> p) {
  p.list_only = 1;
  p.wave_counters = counter_rows(a, plan.row_team);
  p.trace_scratch = a->e_trace.as<unsigned long long>() + plan.trace_team_off / 8;
  return p;
}
// pipeline_tpr.hip: the problem-parallel path's launches (plan.tpr), in place of the main and team launches of the default
// path.  `base` is the fast class's parameter block as the main kernel would take it.
int enqueue_tpr_rounds(thm_aligner* a, const thm::ExtendPlan& plan, const thm::ExtendParamsT<uint32_t>& base);
int enqueue_tpr_rounds(thm_aligner* a, const thm::ExtendPlan& plan, const thm::ExtendParamsT<uint64_t>& base);
// pipeline.hip: what THM_SEED_FILL and THM_TEAM_DIV_PER_CU resolved to (read once per process)
uint32_t seed_fill_mode();
unsigned team_div_per_cu();
#endif
