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

// Ownership: a DBuf, an HBuf (and their typed forms DArr<T>, HArr<T>), an Event and a Stream each free what they hold when
// they are destroyed, and none of them can be copied, so `delete` of the struct that holds them (thm_aligner, thm_index::DevCopy) is the whole clean-up and a
// new member needs no entry anywhere.

// grow-only device buffer of bytes: for what holds more than one element type (a DArr otherwise)
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

// a fixed part of another DBuf (the control block's words) of one element type: stands where a T* is wanted, nothing
// to grow or free
template <class T>
struct DView {
  T* p = nullptr;
  size_t cap = 0;  // bytes
  operator T*() const { return p; }
};

// grow-only pinned host buffer of bytes (results land here: D2H at full PCIe rate, no value-initialisation)
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

// A DBuf / an HBuf of one element type: sized in elements, stands where a T* is wanted.  `slack_bytes` is what a kernel may
// read or write behind the last element (the comments at the members say which); it is asked for as it is written, so
// that ensure(count, slack) requests exactly what ensure(count * sizeof(T) + slack) of the byte buffer does.
template <class T, class Bytes>
struct ArrOf {
  Bytes b;
  hipError_t ensure(size_t count, size_t slack_bytes = 0) { return b.ensure(count * sizeof(T) + slack_bytes); }
  void release() { b.release(); }
  T* get() const { return (T*)b.p; }
  operator T*() const { return get(); }
  size_t cap() const { return b.cap; }  // bytes
};
template <class T>
using DArr = ArrOf<T, DBuf>;
template <class T>
using HArr = ArrOf<T, HBuf>;
static_assert(!std::is_copy_constructible_v<DBuf> && !std::is_copy_assignable_v<DBuf>, "one owner per device allocation");
static_assert(!std::is_copy_constructible_v<HBuf> && !std::is_copy_assignable_v<HBuf>, "one owner per pinned allocation");
static_assert(!std::is_copy_constructible_v<DArr<int>> && !std::is_copy_assignable_v<DArr<int>>, "one owner per device allocation");
static_assert(!std::is_copy_constructible_v<HArr<int>> && !std::is_copy_assignable_v<HArr<int>>, "one owner per pinned allocation");

// Two sets of pinned results used alternately, so that the view a fetch returned stays valid while the next batch is
// uploaded, run and fetched: next() is the set that does not back the previous view.
template <class Set>
struct Alternating {
  Set set[2];
  int cur = 0;
  Set& next() { return set[cur ^= 1]; }
  Set& current() { return set[cur]; }
};

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
  DArr<uint8_t> text, tx_seq;
  DArr<thm_ref> refs;
  DArr<thm_tx> txs;
  DArr<thm_exon> exons;
  DArr<uint64_t> exon_txoff;
  DArr<uint32_t> name_rank, ref_bin, exon_grid_off, gene_grid_off;
  DBuf sa, lut, ref_recs, exon_grid, gene_grid;  // of the coordinate type of the valid view
  bool wide = false;                     // which of the two views is valid (thermite_internal.h, "Coordinate width")
  // lut_direct.h: the pass that runs once behind the upload put text positions into the single-suffix entries of `lut`
  // (THM_LUT_DIRECT=0, or a 32-bit table over 2^31 symbols or more: plain); how many entries it rewrote
  bool lut_direct = false;
  uint64_t lut_tagged = 0;
  DArr<unsigned long long> lut_cnt;      // the pass's counter (one u64)
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

namespace thm {
namespace inf {
struct Member;
}
namespace gz {
struct State;
struct Run;
struct End;
struct Summary;
}  // namespace gz
}  // namespace thm

// ---- the aligner's state, a struct per stage, each named after the host file that works on it ----

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
  DArr<thm::ReadMemo> t_memos;
  DArr<thm::DpRec> t_recs;
  DArr<uint32_t> t_qlist, t_act[2];
  DArr<unsigned long long> t_bail;
  DArr<unsigned int> t_queue2;
  DArr<thm::HitHdr> t_hdr;
  DArr<thm::HitSum> t_sums;
  DBuf t_ctl;    // u64 cursors and statistics, then the rounds' u32 work words
  DBuf t_trace;  // sized in bytes per wave
  bool use_tpr = false;  // (until the path is the faster one on the headline workload)
  int tpr_rounds = 8;
};

// pipeline.hip: the batch on the device
struct ReadsState {
  DArr<uint8_t> bases, san;   // raw reads; upper-cased + sanitised copy (made by every run)
  DArr<uint64_t> offsets;
  DArr<int32_t> status;       // per-read status, zeroed by every run
};

// pipeline.hip: the seed stage
struct SeedState {
  DBuf smems, ms_lo, ms_hi;  // of the index's coordinate type
  DArr<uint64_t> off, hits, cand_off;
  DArr<uint32_t> cnt;
  // the pipeline's own scan scratch: plan_pack_kernel reads the tile offsets launch_scan_tiles_sums_u64 leaves in it
  DArr<uint64_t> scan_tmp;
  DArr<uint16_t> ms_end, fill_keys;
  DArr<unsigned long long> work_reads, work_long, work_cells, heavy, slow, team;
  DArr<uint8_t> sel_scratch;
  DArr<uint32_t> fill_perm;
  DArr<unsigned int> fill_hist;
  uint64_t smem_cap = 0;
};

// pipeline.hip: the extend stage and the compact stage's lists
struct ExtendState {
  DArr<uint64_t> heavy;  // compact stage: lists of reads with many alignments ...
  DArr<uint32_t> rel;    // ... and the op offsets of their alignments
  DArr<thm::Cand> cands;
  DArr<uint32_t> order, nalns;
  DArr<uint8_t> ops, slow;
  DArr<uint64_t> opbytes, aln_off, ops_off;
  DBuf trace;  // sized in bytes (the plan's slices)
  DBuf recs;   // ReadRecT of the index's coordinate type
  // wcnt (the waves' counter rows) is zero from end to end between runs: launch_counters_reduce zeroes what it read, so
  // only a new allocation is zeroed by the host.  The capacity that is known clean (0 while a run's launches are being
  // enqueued: an enqueue that fails half way leaves rows nobody reduced)
  DArr<unsigned long long> wcnt;
  size_t wcnt_clean_cap = 0;
  DArr<unsigned long long> finstats;  // the finisher's per-workgroup statistics
  uint64_t cand_cap = 0, cand_ops_cap = 0;
};

// host results of the read-level path (thm_batch_fetch)
struct BatchHost {
  HArr<uint64_t> off;
  HArr<thm_aln> alns;
  HArr<uint8_t> ops;
  HArr<int32_t> stat;
};
// pipeline.hip: the compacted outputs and where thm_batch_fetch lands them
struct OutputState {
  DArr<thm_aln> alns;
  DArr<uint8_t> ops;
  DArr<thm_mem> mems;
  // alns_cap, ops_cap: cand_cap and cand_ops_cap as the last enqueued run had them, which is what a fetch checks the
  // batch against (thm_debug_set_pool_caps zeroes those two for the next run while this one's views are still being fetched)
  uint64_t alns_cap = 0, ops_cap = 0;
  Alternating<BatchHost> host;
};

// per-hit entry point (seed_hits.hip): device buffers
struct SeedHitState {
  DArr<uint8_t> bases, san, ops, slow;
  DArr<uint64_t> off;
  DArr<thm_mem> hits;
  DArr<uint32_t> read, bw, list;
  DArr<int32_t> xd, status;
  DArr<thm_aln> out;
  DArr<unsigned long long> ctl;
  DBuf trace;  // sized in bytes per wave
};

// CIGAR entry points (cigar.hip): per-stream sums and word counts, their scan, digests and words on the device; the
// uploaded streams of thm_cigar_encode_batch; two pinned host sets of thm_batch_fetch_cigars, used alternately and
// apart from OutputState::host, so that neither fetch invalidates the other's view
struct CigarHost {
  HArr<uint64_t> off;
  HArr<thm_aln> alns;
  HArr<thm_aln_digest> dig;
  HArr<uint32_t> words;
  HArr<int32_t> stat;
};
struct CigarState {
  DArr<thm::CigarSum> sums;
  DArr<uint64_t> nwords, woff, in_off;
  DArr<unsigned int> flags;
  DArr<thm_aln_digest> dig;
  DArr<uint32_t> words;
  DArr<uint8_t> in_ops;
  Alternating<CigarHost> host;
  Event ev[4];  // made by the first call
  std::vector<thm_aln_digest> h_dig;
  std::vector<uint32_t> h_words;
};

// BAM records on the device (bam.hip): names and qualities of the batch (thm_batch_upload_reads), the index's name
// tables (uploaded by the first thm_batch_fetch_bam), work arrays of the passes, the records, and two pinned host
// sets of their own, used alternately
struct BytesHost {  // (also the set of BgzfState)
  HArr<uint8_t> data;
  HArr<uint64_t> off;
  HArr<int32_t> stat;
};
struct BamState {
  DArr<uint8_t> names, quals;
  DArr<uint64_t> name_off;
  bool reads_named = false, reads_have_quals = false;  // thm_batch_upload clears reads_named
  DArr<uint8_t> tx_pool, gid_pool, gname_pool;
  DArr<uint32_t> tx_off, gid_off, gname_off, tx_gene;
  DArr<int32_t> ref_sq;
  bool tables = false;
  DArr<uint64_t> cnt, first, len, off, read_off;
  DArr<uint32_t> qn, rec_read;
  DArr<uint8_t> out;
  DArr<unsigned int> err;
  Alternating<BytesHost> host;
  int stage = -1;  // emit through LDS and dword stores (1) or byte stores (0); -1: not read from THM_BAM_EMIT yet
  Event ev[4];  // made by the first call
};

// BGZF members on the device (bgzf.hip): per-position scratch of the workgroups, the members in their slots, their
// sizes and the scan, the members behind one another; the bytes thm_debug_bgzf_device uploads; two pinned host sets
// of their own, used alternately
struct BgzfState {
  DArr<uint32_t> match;
  DArr<uint8_t> slots, out, dbg_in;
  DArr<uint64_t> sizes, off;
  Alternating<BytesHost> host;
  Event ev[2];  // made by the first call
};

// FASTQ blocks parsed on the device (fastq.hip): the block's bytes, newline counts per chunk and their scan, the line
// starts, the records' lengths and the flag word; the offsets come back into h_off for the length classes.  The
// blocks that went either way since the aligner was created (thm_debug_fastq_device_blocks).  One pinned set behind
// thm_batch_fetch_reads.
struct FastqState {
  DBuf raw;  // the block as bytes; the device inflaters build it here (gz::Job::out, InflateParams::out)
  DArr<uint64_t> cnt, base, lines, name_len, seq_len;
  DArr<unsigned int> flag;
  HArr<uint64_t> h_off;
  uint64_t on_device = 0, on_host = 0;
  Event ev[6];  // made by the first call
  struct {
    HArr<uint8_t> bases, quals, names;
    HArr<uint64_t> off, name_off;
  } back;  // thm_batch_fetch_reads
};

// BGZF members inflated on the device (inflate.hip): the members' bytes, the host's table of them and their status
// words (the table and the statuses in pinned memory too); the inflated block is built in fq.raw.  Two tail buffers,
// used alternately; the block on the host where the host inflated or parsed it.  Counts for
// thm_debug_fastq_bgzf_blocks: inflates on device / on host, parses on device / on host.
struct InflateState {
  DArr<uint8_t> in;
  DArr<thm::inf::Member> tab;
  DArr<uint32_t> status;
  HArr<thm::inf::Member> h_tab;
  HArr<uint32_t> h_status;
  HArr<uint8_t> h_last;
  Alternating<HArr<uint8_t>> tail;
  std::vector<uint8_t> block;
  uint64_t counts[4] = {0, 0, 0, 0};
  Event ev[2];  // made by the first call
};

// plain gzip inflated on the device (gzip.hip; the arrays of gz::Job, gzip_device.h): the compressed bytes, both
// states, candidates, runs, member ends, symbol regions, windows and what the chain derives; summary and outgoing
// state in pinned memory too.  The inflated block is built in fq.raw and the tail buffers are fz.tail.  Counts for
// thm_debug_fastq_gzip_blocks, as fz.counts.
struct GzipState {
  DArr<uint8_t> in, windows;
  DArr<thm::gz::State> state;
  DArr<uint64_t> cand, run_off, end_abs;
  DArr<thm::gz::Run> runs;
  DArr<thm::gz::End> ends;
  DArr<uint16_t> syms;
  DArr<uint32_t> run_list, end_crc, end_isize, member_crc;
  DArr<thm::gz::Summary> sum;
  HArr<thm::gz::Summary> h_sum;
  HArr<thm::gz::State> h_state;
  uint64_t counts[4] = {0, 0, 0, 0};
  Event ev[2];  // made by the first call
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

  DArr<unsigned long long> d_counters;  // three rows of THM_N_COUNTERS: the counters, their snapshot, the profile clocks
  // Control block: every word a run of the read-level pipeline wants zeroed when it starts, side by side, so that the
  // run's first kernel zeroes them in one go (launch.h, RunResetParams).  The views below are its parts.
  DBuf d_ctl;
  static constexpr size_t CTL_WORK_COUNTS = 0, CTL_CURSORS = 128, CTL_FAULT = 192, CTL_QUEUE = 256,
                          CTL_QUEUE_EXT = CTL_QUEUE + thm::QUEUE_BYTES, CTL_BYTES = CTL_QUEUE_EXT + thm::QUEUE_BYTES;
  static_assert(CTL_BYTES % 16 == 0 && thm::QUEUE_BYTES % 16 == 0, "the block is zeroed 16 bytes at a time");
  DView<unsigned int> d_queue;      // work counters of the seed stage's selection kernel and of the operator-level calls
  DView<unsigned int> d_queue_ext;  // ... of the extend stage: its own words, so that one reset serves both stages of a run
  DView<int> d_fault;
  DView<unsigned long long> d_cursors;      // cursors: [0] smem pool head, [1] op pool head (u64 each)
  DView<unsigned long long> s_work_counts;  // list lengths of the seed stage and of the plan kernel (16 u64)
  DBuf b0, b1, b2, b3, b4, b5, b6, b7, b8;       // operator-level scratch
  // scratch of the exclusive scans of the stages behind the pipeline (cigar, bam, bgzf, fastq: scan_u64 below), which
  // run on `stream` one after the other
  DArr<uint64_t> stage_scan_tmp;

  // ---- read-level pipeline ----
  ReadsState reads;
  uint64_t n_reads = 0, n_bases = 0;
  uint32_t max_read_len = 0;
  // lengths present in the batch, ascending, with their read counts (thm_batch_upload): the length classes of a
  // run (which reads the register-resident kernels take) depend on the options, which may change between runs
  std::vector<std::pair<uint32_t, uint64_t>> len_hist;
  uint64_t n_over = 0;  // reads longer than MAX_READ_LEN (per-read status THM_ERR_UNSUPPORTED)
  bool uploaded = false;
  SeedState seed;
  ExtendState ext;
  uint64_t n_slow_host = 0;     // reads of the slow class in the last enqueue (host count)
  uint32_t fast_max_len = 0, slow_max_len = 0;
  OutputState out;
  // test hook (thm_debug_set_pool_caps): initial pool sizes instead of the heuristics, to force the grow-and-replay path
  uint64_t dbg_smem_cap = 0, dbg_cand_cap = 0, dbg_ops_cap = 0;
  uint32_t dbg_band_clip = 0;  // test hook (thm_debug_set_band_clip): pretend the fast class holds bands up to this only (0: off)
  // test / tuning hook (thm_debug_set_flags bits 2, 3): seed probes never decided from the table entry and a neighbouring
  // match; seed probes counted (thm_debug_seed_stats)
  bool dbg_seed_noinfer = false, dbg_seed_stats = false;
  // ... bit 6: a probe into a single-suffix bucket reads sa[lo] although the table entry holds the text position
  bool dbg_seed_nodirect = false;
  // (bits 16, 17): grid cells of the seed stage are listed whole, not cut down by the bounds of their grid probes (seed_bounds.h)
  bool dbg_seed_nobounds = false;
  // The finisher (kernels_finish.hip): classes it takes (thm_debug_set_flags bits 12..15; fin::CLASS_E | fin::CLASS_S), the
  // read-only op run at the front of ext.ops (where it was written and for which read length, 0: none; while it exists every
  // run starts the pool's cursor behind it), the classes and workgroups of the last enqueue (its statistics: ext.finstats)
  uint32_t fin_classes = 3;
  const void* ops_run_ptr = nullptr;
  size_t ops_run_cap = 0;
  uint32_t ops_run_half = 0;
  uint32_t fin_run_classes = 0, fin_blocks = 0;
  uint32_t n_replays = 0;  // pool-overflow replays since the aligner was created
  bool ran = false, synced = false;
  Event ev[6];  // made by thm_aligner_create
  float timings[THM_N_TIMINGS] = {0};

  // host results of the operator- and seed-level calls
  std::vector<uint64_t> h_off;
  std::vector<thm_aln> h_alns;
  std::vector<uint8_t> h_ops;
  std::vector<thm_mem> h_mems;
  std::vector<thm_swg_aln> h_swg;
  std::vector<thm_lr_aln> h_lr;
  // per-hit entry point: the host result its view points into
  SeedHitState sh;
  std::vector<thm_aln> h_hit_alns;
  std::vector<int32_t> h_hit_status;
  std::vector<uint8_t> h_hit_ops;
  // ---- the stages behind the pipeline ----
  CigarState cig;
  BamState bam;
  BgzfState bgzf;
  FastqState fq;
  InflateState fz;
  GzipState gz;
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

// ---- the exclusive scan of counts every stage runs: counts -> offsets, the total behind them in out[n]
// `scratch` with room for a scan of n entries (a caller that keeps a scratch of its own sizes it for its longest scan)
inline hipError_t scan_reserve(DArr<uint64_t>& scratch, uint64_t n) { return scratch.ensure(thm::scan_tmp_entries(n + 1), 64); }
// out[0 .. n] = exclusive scan of in[0, n) on `s`, through `scratch`, which grows as the scan needs
inline int scan_u64(thm_aligner* a, DArr<uint64_t>& scratch, const uint64_t* in, uint64_t* out, uint64_t n, hipStream_t s) {
  HIPCHK(a, scan_reserve(scratch, n));
  HIPCHK(a, thm::launch_exclusive_scan_u64(in, out, n, scratch, s));
  return THM_OK;
}
// ... and the total on its way into *h_total, which holds it once the caller has synchronised `s`
template <class W>
inline int scan_u64(thm_aligner* a, DArr<uint64_t>& scratch, const uint64_t* in, uint64_t* out, uint64_t n, hipStream_t s, W* h_total) {
  static_assert(sizeof(W) == 8, "the total is a 64-bit word");
  const int rc = scan_u64(a, scratch, in, out, n, s);
  if (rc != THM_OK) return rc;
  HIPCHK(a, hipMemcpyAsync(h_total, out + n, 8, hipMemcpyDeviceToHost, s));
  return THM_OK;
}

// cigar.hip: count -> scan -> emit over the streams of `p`; results in cig.dig / cig.words (synchronises the stream once)
int run_cigar_passes(thm_aligner* a, thm::CigarParams p, uint64_t n_digests, uint64_t* n_words, unsigned* any_flags);
// bam.hip: everything of thm_batch_fetch_bam up to the copies -- after it the records of the run are in bam.out on the
// device and the per-read byte offsets in bam.read_off (both fetches that hand records out start here; the messages name
// thm_batch_fetch_bam whichever it is).  Of the timings only `timing`, the caller's own, is touched: zeroed once the
// arguments have passed; bam.ev[0..3] are left recorded around the size and emit passes.
struct BamOnDevice {
  uint64_t n_reads = 0, n_alns = 0, n_records = 0, n_bytes = 0;
  bool any_failed = false;  // as in BatchSizes
};
int bam_records_on_device(thm_aligner* a, uint32_t flags, int timing, BamOnDevice* r);
// bam.hip: the index's name tables, tx -> gene (bam.tx_gene) and ref -> BAM refID (bam.ref_sq) on the device, once per aligner
// (the aligner's device is current).  THM_ERR_INVALID_ARG: an index without names.  quant.hip counts from the last two.
int bam_tables_on_device(thm_aligner* a);
// bgzf.hip: d_in[0, n) (device, 4-byte aligned) cut every 0xff00 bytes and deflated -> the members back to back in bgzf.out,
// their offsets in bgzf.off[0 .. *n_blocks]; synchronises the stream once and sets THM_T_BGZF (bam_sort.hip deflates the
// windows of the sorted stream through it)
int bgzf_range_on_device(thm_aligner* a, const uint8_t* d_in, uint64_t n, uint64_t* n_blocks, uint64_t* n_bytes);
// ---- pipeline.hip: the head and the tail of every fetch entry point (after thm_batch_sync; a new one calls all of them)
struct BatchSizes {
  uint64_t n_alns = 0, n_ops = 0;  // alignments and op bytes of the compacted batch, checked against the pools
  bool any_failed = false;         // a read of the batch may have failed: the statuses are worth copying
};
// One round trip (a single synchronisation of the stream): ext.aln_off[n], ext.ops_off[n] and the device's count of
// out-of-contract reads.  With `h_off` the whole offsets array comes into it, (n + 2) words with the op bytes last; with
// `d_extra` that device word comes into *extra.
int fetch_batch_sizes(thm_aligner* a, HArr<uint64_t>* h_off, const uint64_t* d_extra, uint64_t* extra, BatchSizes* z);
// reads.status on its way into `h_stat` where any_failed says so; after the next synchronisation failed_reads fills the two
// fields of a view from it: the count of reads that failed, and the statuses where there is one (else null)
int enqueue_statuses(thm_aligner* a, bool any_failed, HArr<int32_t>& h_stat);
void failed_reads(const thm_aligner* a, bool any_failed, const HArr<int32_t>& h_stat, uint64_t* n_failed, const int32_t** status);
// the two op streams of every alignment in the compacted pool, for run_cigar_passes
thm::CigarParams compacted_cigar_params(const thm_aligner* a, const BatchSizes& z);
// pipeline.hip: what thm_batch_upload derives from the offsets of a batch -- n_reads, n_bases, max_read_len, the length
// classes (len_hist) and n_over -- for every upload path; THM_ERR_INVALID_ARG for offsets that do not start at 0 or descend
int batch_length_classes(thm_aligner* a, const uint64_t* offsets, uint64_t n_reads);
// fastq.hip: the device FASTQ parse (count, starts, records, gather) of a block of n > 0 bytes that stands in fq.raw,
// which the caller has sized to n + 64 -- put there by a copy (thm_batch_upload_fastq) or by the device inflater
// (inflate.hip).  Three synchronisations of the stream, whichever it is.
struct FastqBlock {
  uint64_t n = 0;
  const uint8_t* host = nullptr;  // the block's bytes on the host; null: its last byte comes down with the newline total
  bool whole = true;              // the batch is the whole block; false: its first 4 * (newlines / 4) lines
  const uint32_t* d_status = nullptr;  // status words of an inflate (device), checked at the first synchronisation
  uint64_t n_status = 0;
  HArr<uint8_t>* tail = nullptr;  // where the bytes behind the batch go, in the copy-back the gather ends with (null: not wanted)
  // results
  uint64_t bad_member = 0;  // FQ_NOT_INFLATED: the first member with a status other than 0 (the word is in fz.h_status)
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
  const uint8_t* tail = nullptr;  // the block's bytes behind the batch (in the array handed in)
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
// A block that stands on the host: copied into fq.raw and parsed there (parse_resident's codes).  On 1 `o` holds the
// counts and the cut, and the bytes behind it are in `tail` (null: the batch is the whole block).
int parse_host_block(thm_aligner* a, const uint8_t* blk, uint64_t n, bool whole, HArr<uint8_t>* tail, FastqOutcome& o);
// The device parsed the batch: the aligner's batch state, and o.tail.
void batch_parsed_on_device(thm_aligner* a, HArr<uint8_t>* tail, FastqOutcome& o);
// The host parser's batch of a block the device did not parse: the batch bytes -- all of the block for a last block or
// with no `tail`, else up to fastq_host_cut -- through fastq_parse_block and thm_batch_upload_reads, the lines and the
// tail into `o`; *on_host counts a batch that has bytes.  The parser's error goes into a->err and the global error.
int host_parser_batch(thm_aligner* a, const uint8_t* blk, uint64_t n, const std::string& path, uint64_t first_line, bool last_block,
                      HArr<uint8_t>* tail, uint64_t* on_host, FastqOutcome& o);
}
int reset_queue(thm_aligner* a);
inline int grid_blocks(const thm_aligner* a, uint64_t n_items, int waves_per_block, int blocks_per_cu) {
  return thm::grid_blocks(a->n_cu, n_items, waves_per_block, blocks_per_cu);
}
// ---- the extend stage's launches (pipeline.hip, pipeline_tpr.hip) over one run's thm::ExtendPlan ----
// where a launch's waves leave their counters: row `row` of ext.wcnt (the plan's row_* offsets)
inline unsigned long long* counter_rows(const thm_aligner* a, uint64_t row) { return a->ext.wcnt + row * THM_N_COUNTERS; }
// the team kernel's parameter block: `p` over the team list only, with the team's own counter rows and trace slices
template <class C>
thm::ExtendParamsT<C> team_params(const thm_aligner* a, const thm::ExtendPlan& plan, thm::ExtendParamsT<C> p) {
  p.list_only = 1;
  p.wave_counters = counter_rows(a, plan.row_team);
  p.trace_scratch = a->ext.trace.as<unsigned long long>() + plan.trace_team_off / 8;
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
