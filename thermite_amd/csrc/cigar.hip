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

int cigar_ensure_events(thm_aligner* a) {
  for (auto& e : a->ev_cig)
    if (!e) HIPCHK(a, hipEventCreate(&e));
  return THM_OK;
}

namespace {

void cigar_timing(thm_aligner* a) {  // after the stream has been synchronised
  float m1 = 0, m2 = 0;
  if (hipEventElapsedTime(&m1, a->ev_cig[0], a->ev_cig[1]) == hipSuccess && hipEventElapsedTime(&m2, a->ev_cig[2], a->ev_cig[3]) == hipSuccess)
    a->timings[THM_T_CIGAR] = m1 + m2;
}

}  // namespace

extern "C" {

int32_t thm_batch_fetch_cigars(thm_aligner* a, thm_cigar_view* out) {
  if (!a || !out) return THM_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  int rc = thm_batch_sync(a);
  if (rc != THM_OK) return rc;
  HIPCHK(a, hipSetDevice(a->device));
  rc = cigar_ensure_events(a);
  if (rc != THM_OK) return rc;
  const uint64_t n = a->n_reads;
  hipStream_t s = a->stream;
  const int k = a->c_cur ^= 1;  // the other set still backs the previous view
  HBuf& h_off = a->ch_off[k];
  HBuf& h_alns = a->ch_alns[k];
  HBuf& h_dig = a->ch_dig[k];
  HBuf& h_words = a->ch_words[k];
  HBuf& h_stat = a->ch_stat[k];
  HIPCHK(a, h_off.ensure((n + 2) * 8));
  // offsets, the op-pool size behind them and the count of out-of-contract reads, as thm_batch_fetch takes them
  HIPCHK(a, hipMemcpyAsync(h_off.p, a->e_aln_off.p, (n + 1) * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipMemcpyAsync(h_off.as<uint64_t>() + n + 1, a->e_ops_off.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, s));
  unsigned long long n_contract = 0;
  HIPCHK(a, hipMemcpyAsync(&n_contract, a->s_work_counts.as<unsigned long long>() + 6, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipStreamSynchronize(s));
  const uint64_t n_alns = h_off.as<uint64_t>()[n];
  const uint64_t n_ops = h_off.as<uint64_t>()[n + 1];
  if (n_alns > a->cand_cap || n_ops > a->cand_ops_cap) return fail(a, THM_ERR_INTERNAL, "compacted batch exceeds its pools");
  HIPCHK(a, h_alns.ensure(n_alns * sizeof(thm_aln)));
  HIPCHK(a, h_dig.ensure(n_alns * sizeof(thm_aln_digest)));
  if (n_alns) HIPCHK(a, hipMemcpyAsync(h_alns.p, a->o_alns.p, n_alns * sizeof(thm_aln), hipMemcpyDeviceToHost, s));
  CigarParams p;
  memset(&p, 0, sizeof p);
  p.ops = a->o_ops.as<uint8_t>();
  p.ops_bytes = n_ops;
  p.n_streams = 2 * n_alns;
  p.alns = a->o_alns.as<thm_aln>();
  uint64_t n_words = 0;
  unsigned any_flags = 0;
  rc = run_cigar_passes(a, p, n_alns, &n_words, &any_flags);
  if (rc != THM_OK) return rc;
  HIPCHK(a, h_words.ensure(n_words * 4));
  if (n_alns) HIPCHK(a, hipMemcpyAsync(h_dig.p, a->c_dig.p, n_alns * sizeof(thm_aln_digest), hipMemcpyDeviceToHost, s));
  if (n_words) HIPCHK(a, hipMemcpyAsync(h_words.p, a->c_words.p, n_words * 4, hipMemcpyDeviceToHost, s));
  uint64_t n_beyond = a->n_over;
  for (const auto& lc : a->len_hist)
    if (lc.first > a->slow_max_len) n_beyond += lc.second;
  const bool any_failed = n_beyond || n_contract;
  if (any_failed) {
    HIPCHK(a, h_stat.ensure((n + 1) * 4));
    HIPCHK(a, hipMemcpyAsync(h_stat.p, a->r_status.p, n * 4, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(a, hipStreamSynchronize(s));
  if (n_alns) cigar_timing(a);
  // the extend kernels write well-formed streams: anything else is a fault of this library, not of the input
  if (any_flags & THM_DIGEST_MALFORMED) return fail(a, THM_ERR_INTERNAL, "malformed op stream in the compacted pool");
  out->n_reads = n;
  out->n_alns = n_alns;
  out->n_cigar_words = n_words;
  out->read_aln_off = h_off.as<uint64_t>();
  out->alns = h_alns.as<thm_aln>();
  out->digests = h_dig.as<thm_aln_digest>();
  out->cigar = h_words.as<uint32_t>();
  out->n_failed_reads = 0;
  out->read_status = nullptr;
  if (any_failed) {
    const int32_t* st = h_stat.as<int32_t>();
    uint64_t bad = 0;
    for (uint64_t i = 0; i < n; i++) bad += st[i] != THM_OK;
    out->n_failed_reads = bad;
    out->read_status = bad ? st : nullptr;
  }
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
  int rc = cigar_ensure_events(a);
  if (rc != THM_OK) return rc;
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
  rc = run_cigar_passes(a, p, n, &n_words, &any_flags);  // (synchronises: `rel` has been read by then)
  if (rc != THM_OK) return rc;
  a->h_cig_dig.resize(n);
  a->h_cig_words.resize(n_words);
  HIPCHK(a, hipMemcpyAsync(a->h_cig_dig.data(), a->c_dig.p, n * sizeof(thm_aln_digest), hipMemcpyDeviceToHost, s));
  if (n_words) HIPCHK(a, hipMemcpyAsync(a->h_cig_words.data(), a->c_words.p, n_words * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipStreamSynchronize(s));
  cigar_timing(a);
  out->n_alns = n;
  out->n_cigar_words = n_words;
  out->digests = a->h_cig_dig.data();
  out->cigar = a->h_cig_words.data();
  return THM_OK;
}

}  // extern "C"
