// cigar.hip -- host side of the CIGAR entry points (include/thermite.h): thm_batch_fetch_cigars stands where
// thm_batch_fetch stands after a run and hands back what the reference's writer derives from every alignment's
// op list -- to_noodles_cigar (src/aln_writer.rs:279-323), PafEntry's counts (:55-72), nM (:160-168) -- instead of the
// op bytes; thm_cigar_encode_batch is the same two passes (kernels_cigar.hip) over caller-supplied op streams.
#include <hip/hip_runtime.h>

#include <cstring>

#include "aligner_internal.h"

using namespace thm;

// count -> scan -> emit over `n_streams` streams of the pool `p.ops`; device results in c_dig / c_words, the number of
// words and the flags met through *n_words / *any_flags (synchronises the stream once between the passes: the word pool
// is sized by the count)
int run_cigar_passes(thm_aligner* a, CigarParams p, uint64_t n_digests, uint64_t* n_words, unsigned* any_flags) {
  hipStream_t s = a->stream;
  HIPCHK(a, ensure_events(a->ev_cig));
  const uint64_t ns = p.n_streams;
  *n_words = 0;
  *any_flags = 0;
  a->timings[THM_T_CIGAR] = 0;
  if (ns == 0) return THM_OK;
  HIPCHK(a, a->c_sums.ensure(ns * sizeof(CigarSum)));
  HIPCHK(a, a->c_nwords.ensure((ns + 1) * 8));
  HIPCHK(a, a->c_woff.ensure((ns + 2) * 8));
  HIPCHK(a, a->c_scan_tmp.ensure(scan_tmp_entries(ns + 1) * 8 + 64));
  HIPCHK(a, a->c_flags.ensure(64));
  HIPCHK(a, a->c_dig.ensure(n_digests * sizeof(thm_aln_digest)));
  p.sums = a->c_sums.as<CigarSum>();
  p.n_words = a->c_nwords.as<uint64_t>();
  p.word_off = a->c_woff.as<uint64_t>();
  p.digests = a->c_dig.as<thm_aln_digest>();
  p.any_flags = a->c_flags.as<unsigned int>();
  p.words = nullptr;
  HIPCHK(a, hipEventRecord(a->ev_cig[0], s));
  HIPCHK(a, hipMemsetAsync(a->c_flags.p, 0, 64, s));
  HIPCHK(a, launch_cigar_count(p, a->n_cu, s));
  HIPCHK(a, launch_exclusive_scan_u64(a->c_nwords.as<uint64_t>(), a->c_woff.as<uint64_t>(), ns, a->c_scan_tmp.as<uint64_t>(), s));
  HIPCHK(a, hipEventRecord(a->ev_cig[1], s));
  unsigned long long total = 0;
  HIPCHK(a, hipMemcpyAsync(&total, a->c_woff.as<uint64_t>() + ns, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipMemcpyAsync(any_flags, a->c_flags.p, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipStreamSynchronize(s));
  HIPCHK(a, a->c_words.ensure(total * 4 + 16));
  p.words = a->c_words.as<uint32_t>();
  HIPCHK(a, hipEventRecord(a->ev_cig[2], s));
  HIPCHK(a, launch_cigar_emit(p, a->n_cu, s));
  HIPCHK(a, hipEventRecord(a->ev_cig[3], s));
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
  const int k = a->c_cur ^= 1;  // the other set still backs the previous view
  HBuf& h_off = a->ch_off[k];
  HBuf& h_alns = a->ch_alns[k];
  HBuf& h_dig = a->ch_dig[k];
  HBuf& h_words = a->ch_words[k];
  HBuf& h_stat = a->ch_stat[k];
  BatchSizes z;  // offsets, the op-pool size behind them and the count of out-of-contract reads, as thm_batch_fetch takes them
  rc = fetch_batch_sizes(a, &h_off, nullptr, nullptr, &z);
  if (rc != THM_OK) return rc;
  const uint64_t n_alns = z.n_alns;
  HIPCHK(a, h_alns.ensure(n_alns * sizeof(thm_aln)));
  HIPCHK(a, h_dig.ensure(n_alns * sizeof(thm_aln_digest)));
  if (n_alns) HIPCHK(a, hipMemcpyAsync(h_alns.p, a->o_alns.p, n_alns * sizeof(thm_aln), hipMemcpyDeviceToHost, s));
  uint64_t n_words = 0;
  unsigned any_flags = 0;
  rc = run_cigar_passes(a, compacted_cigar_params(a, z), n_alns, &n_words, &any_flags);
  if (rc != THM_OK) return rc;
  HIPCHK(a, h_words.ensure(n_words * 4));
  if (n_alns) HIPCHK(a, hipMemcpyAsync(h_dig.p, a->c_dig.p, n_alns * sizeof(thm_aln_digest), hipMemcpyDeviceToHost, s));
  if (n_words) HIPCHK(a, hipMemcpyAsync(h_words.p, a->c_words.p, n_words * 4, hipMemcpyDeviceToHost, s));
  rc = enqueue_statuses(a, z.any_failed, h_stat);
  if (rc != THM_OK) return rc;
  HIPCHK(a, hipStreamSynchronize(s));
  if (n_alns) (void)elapsed_ms(a->ev_cig, &a->timings[THM_T_CIGAR]);
  // the extend kernels write well-formed streams: anything else is a fault of this library, not of the input
  if (any_flags & THM_DIGEST_MALFORMED) return fail(a, THM_ERR_INTERNAL, "malformed op stream in the compacted pool");
  out->n_reads = n;
  out->n_alns = n_alns;
  out->n_cigar_words = n_words;
  out->read_aln_off = h_off.as<uint64_t>();
  out->alns = h_alns.as<thm_aln>();
  out->digests = h_dig.as<thm_aln_digest>();
  out->cigar = h_words.as<uint32_t>();
  failed_reads(a, z.any_failed, h_stat, &out->n_failed_reads, &out->read_status);
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
  HIPCHK(a, a->c_in_ops.ensure(pool + 16));
  HIPCHK(a, a->c_in_off.ensure((n + 1) * 8));
  if (pool) HIPCHK(a, hipMemcpyAsync(a->c_in_ops.p, ops + o0, pool, hipMemcpyHostToDevice, s));
  HIPCHK(a, hipMemcpyAsync(a->c_in_off.p, rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
  CigarParams p;
  memset(&p, 0, sizeof p);
  p.ops = a->c_in_ops.as<uint8_t>();
  p.ops_bytes = pool;
  p.n_streams = n;
  p.off = a->c_in_off.as<uint64_t>();
  uint64_t n_words = 0;
  unsigned any_flags = 0;
  const int rc = run_cigar_passes(a, p, n, &n_words, &any_flags);  // (synchronises: `rel` has been read by then)
  if (rc != THM_OK) return rc;
  a->h_cig_dig.resize(n);
  a->h_cig_words.resize(n_words);
  HIPCHK(a, hipMemcpyAsync(a->h_cig_dig.data(), a->c_dig.p, n * sizeof(thm_aln_digest), hipMemcpyDeviceToHost, s));
  if (n_words) HIPCHK(a, hipMemcpyAsync(a->h_cig_words.data(), a->c_words.p, n_words * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipStreamSynchronize(s));
  (void)elapsed_ms(a->ev_cig, &a->timings[THM_T_CIGAR]);
  out->n_alns = n;
  out->n_cigar_words = n_words;
  out->digests = a->h_cig_dig.data();
  out->cigar = a->h_cig_words.data();
  return THM_OK;
}

}  // extern "C"
