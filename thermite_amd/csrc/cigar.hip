// cigar.hip -- host side of the CIGAR entry points (include/thermite.h): thm_batch_fetch_cigars stands where
// thm_batch_fetch stands after a run and hands back what the reference's writer derives from every alignment's
// op list -- to_noodles_cigar (src/aln_writer.rs:279-323), PafEntry's counts (:55-72), nM (:160-168) -- instead of the
// op bytes; thm_cigar_encode_batch is the same two passes (kernels_cigar.hip) over caller-supplied op streams.
#include <hip/hip_runtime.h>

#include <cstring>

#include "aligner_internal.h"

using namespace thm;

// count -> scan -> emit over `n_streams` streams of the pool `p.ops`; device results in cig.dig / cig.words, the number of
// words and the flags met through *n_words / *any_flags (synchronises the stream once between the passes: the word pool
// is sized by the count)
int run_cigar_passes(thm_aligner* a, CigarParams p, uint64_t n_digests, uint64_t* n_words, unsigned* any_flags) {
  hipStream_t s = a->stream;
  HIPCHK(a, ensure_events(a->cig.ev));
  const uint64_t ns = p.n_streams;
  *n_words = 0;
  *any_flags = 0;
  a->timings[THM_T_CIGAR] = 0;
  if (ns == 0) return THM_OK;
  HIPCHK(a, a->cig.sums.ensure(ns));
  HIPCHK(a, a->cig.nwords.ensure(ns + 1));
  HIPCHK(a, a->cig.woff.ensure(ns + 2));
  HIPCHK(a, a->cig.flags.ensure(16));
  HIPCHK(a, a->cig.dig.ensure(n_digests));
  p.sums = a->cig.sums;
  p.n_words = a->cig.nwords;
  p.word_off = a->cig.woff;
  p.digests = a->cig.dig;
  p.any_flags = a->cig.flags;
  p.words = nullptr;
  HIPCHK(a, hipEventRecord(a->cig.ev[0], s));
  HIPCHK(a, hipMemsetAsync(a->cig.flags, 0, 64, s));
  HIPCHK(a, launch_cigar_count(p, a->n_cu, s));
  if (const int rc = scan_u64(a, a->stage_scan_tmp, a->cig.nwords, a->cig.woff, ns, s); rc != THM_OK) return rc;
  HIPCHK(a, hipEventRecord(a->cig.ev[1], s));
  unsigned long long total = 0;
  HIPCHK(a, hipMemcpyAsync(&total, a->cig.woff + ns, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipMemcpyAsync(any_flags, a->cig.flags, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipStreamSynchronize(s));
  HIPCHK(a, a->cig.words.ensure(total, 16));
  p.words = a->cig.words;
  HIPCHK(a, hipEventRecord(a->cig.ev[2], s));
  HIPCHK(a, launch_cigar_emit(p, a->n_cu, s));
  HIPCHK(a, hipEventRecord(a->cig.ev[3], s));
  *n_words = total;
  return THM_OK;
}

extern "C" {

int32_t thm_batch_fetch_cigars(thm_aligner* a, thm_cigar_view* out) {
  if (!a || !out) return THM_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  int rc = thm_batch_sync(a);
  if (rc != THM_OK) return rc;
  HIPCHK(a, hipSetDevice(a->device));
  const uint64_t n = a->n_reads;
  hipStream_t s = a->stream;
  CigarHost& h = a->cig.host.next();  // the other set still backs the previous view
  BatchSizes z;  // offsets, the op-pool size behind them and the count of out-of-contract reads, as thm_batch_fetch takes them
  rc = fetch_batch_sizes(a, &h.off, nullptr, nullptr, &z);
  if (rc != THM_OK) return rc;
  const uint64_t n_alns = z.n_alns;
  HIPCHK(a, h.alns.ensure(n_alns));
  HIPCHK(a, h.dig.ensure(n_alns));
  if (n_alns) HIPCHK(a, hipMemcpyAsync(h.alns, a->out.alns, n_alns * sizeof(thm_aln), hipMemcpyDeviceToHost, s));
  uint64_t n_words = 0;
  unsigned any_flags = 0;
  rc = run_cigar_passes(a, compacted_cigar_params(a, z), n_alns, &n_words, &any_flags);
  if (rc != THM_OK) return rc;
  HIPCHK(a, h.words.ensure(n_words));
  if (n_alns) HIPCHK(a, hipMemcpyAsync(h.dig, a->cig.dig, n_alns * sizeof(thm_aln_digest), hipMemcpyDeviceToHost, s));
  if (n_words) HIPCHK(a, hipMemcpyAsync(h.words, a->cig.words, n_words * 4, hipMemcpyDeviceToHost, s));
  rc = enqueue_statuses(a, z.any_failed, h.stat);
  if (rc != THM_OK) return rc;
  HIPCHK(a, hipStreamSynchronize(s));
  if (n_alns) (void)elapsed_ms(a->cig.ev, &a->timings[THM_T_CIGAR]);
  // the extend kernels write well-formed streams: anything else is a fault of this library, not of the input
  if (any_flags & THM_DIGEST_MALFORMED) return fail(a, THM_ERR_INTERNAL, "malformed op stream in the compacted pool");
  out->n_reads = n;
  out->n_alns = n_alns;
  out->n_cigar_words = n_words;
  out->read_aln_off = h.off;
  out->alns = h.alns;
  out->digests = h.dig;
  out->cigar = h.words;
  failed_reads(a, z.any_failed, h.stat, &out->n_failed_reads, &out->read_status);
  return THM_OK;
}

int32_t thm_align_batch_cigars(thm_aligner* a, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads,
                               thm_cigar_view* out) {
  if (!a || !out) return THM_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  int rc = thm_batch_upload(a, bases, offsets, n_reads);
  if (rc != THM_OK) return rc;
  rc = thm_batch_run(a);
  if (rc != THM_OK) return rc;
  return thm_batch_fetch_cigars(a, out);
}

int32_t thm_cigar_encode_batch(thm_aligner* a, const uint8_t* ops, const uint64_t* off, uint64_t n, thm_cigar_view* out) {
  if (!a || !out) return THM_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  if (n == 0) return THM_OK;
  if (!off || (!ops && off[n] > off[0])) return fail(a, THM_ERR_INVALID_ARG, "thm_cigar_encode_batch: null ops or offsets");
  if (n >= 0xFFFFFFFFull) return fail(a, THM_ERR_UNSUPPORTED, "more than 2^32-1 streams in one call");
  for (uint64_t i = 0; i < n; i++) {
    if (off[i + 1] < off[i]) return fail(a, THM_ERR_INVALID_ARG, "offsets not monotone");
    if (off[i + 1] - off[i] >= (1ull << 32)) return fail(a, THM_ERR_UNSUPPORTED, "stream %llu has 2^32 bytes or more", (unsigned long long)i);
  }
  HIPCHK(a, hipSetDevice(a->device));
  hipStream_t s = a->stream;
  // the pool is uploaded from off[0] on; the offsets travel relative to it
  const uint64_t o0 = off[0], pool = off[n] - o0;
  std::vector<uint64_t> rel(n + 1);
  for (uint64_t i = 0; i <= n; i++) rel[i] = off[i] - o0;
  HIPCHK(a, a->cig.in_ops.ensure(pool, 16));
  HIPCHK(a, a->cig.in_off.ensure(n + 1));
  if (pool) HIPCHK(a, hipMemcpyAsync(a->cig.in_ops, ops + o0, pool, hipMemcpyHostToDevice, s));
  HIPCHK(a, hipMemcpyAsync(a->cig.in_off, rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
  CigarParams p;
  memset(&p, 0, sizeof p);
  p.ops = a->cig.in_ops;
  p.ops_bytes = pool;
  p.n_streams = n;
  p.off = a->cig.in_off;
  uint64_t n_words = 0;
  unsigned any_flags = 0;
  const int rc = run_cigar_passes(a, p, n, &n_words, &any_flags);  // (synchronises: `rel` has been read by then)
  if (rc != THM_OK) return rc;
  a->cig.h_dig.resize(n);
  a->cig.h_words.resize(n_words);
  HIPCHK(a, hipMemcpyAsync(a->cig.h_dig.data(), a->cig.dig, n * sizeof(thm_aln_digest), hipMemcpyDeviceToHost, s));
  if (n_words) HIPCHK(a, hipMemcpyAsync(a->cig.h_words.data(), a->cig.words, n_words * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipStreamSynchronize(s));
  (void)elapsed_ms(a->cig.ev, &a->timings[THM_T_CIGAR]);
  out->n_alns = n;
  out->n_cigar_words = n_words;
  out->digests = a->cig.h_dig.data();
  out->cigar = a->cig.h_words.data();
  return THM_OK;
}

}  // extern "C"
