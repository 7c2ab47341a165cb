// bam.hip -- host side of the BAM entry points (include/thermite_io.h): thm_batch_upload_reads places names and
// qualities beside the reads, thm_batch_fetch_bam stands where thm_batch_fetch / thm_batch_fetch_cigars stand after a
// run and hands back the finished BAM records of the writer loop (reference src/aligner.rs:54-116) -- what
// format_range_bam of io_writer.cpp encodes on the host -- built by kernels_bam.hip from what is resident on the device.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "aligner_internal.h"
#include "io_internal.h"

using namespace thm;

namespace {

// strings back to back with u32 offsets [n + 1]
int upload_pool(thm_aligner* a, const std::vector<std::string>& v, DBuf& pool, DBuf& off) {
  std::vector<uint32_t> o(v.size() + 1, 0);
  std::string all;
  for (size_t i = 0; i < v.size(); i++) {
    all += v[i];
    if (all.size() >= 0xFFFFFFFFull) return fail(a, THM_ERR_UNSUPPORTED, "name table of 4 GiB or more");
    o[i + 1] = (uint32_t)all.size();
  }
  HIPCHK(a, pool.ensure(all.size() + 16));
  HIPCHK(a, off.ensure(o.size() * 4));
  if (!all.empty()) HIPCHK(a, hipMemcpy(pool.p, all.data(), all.size(), hipMemcpyHostToDevice));
  HIPCHK(a, hipMemcpy(off.p, o.data(), o.size() * 4, hipMemcpyHostToDevice));
  return THM_OK;
}

}  // namespace

// the index's name tables, once per aligner
int bam_tables_on_device(thm_aligner* a) {
  if (a->bam_tables) return THM_OK;
  const thm_index* ix = a->ix;
  if (ix->contig_names.empty() || ix->tx_ids.size() != ix->txs.size() || ix->gene_ids.size() != ix->genes.size() ||
      ix->gene_names.size() != ix->genes.size())
    return fail(a, THM_ERR_INVALID_ARG, "thm_batch_fetch_bam needs contig / transcript / gene names: thm_index_set_names or thm_index_create_from_files");
  int rc = upload_pool(a, ix->tx_ids, a->bt_tx_pool, a->bt_tx_off);
  if (rc == THM_OK) rc = upload_pool(a, ix->gene_ids, a->bt_gid_pool, a->bt_gid_off);
  if (rc == THM_OK) rc = upload_pool(a, ix->gene_names, a->bt_gname_pool, a->bt_gname_off);
  if (rc != THM_OK) return rc;
  std::vector<uint32_t> tx_gene(ix->txs.size() + 1, 0);
  for (size_t t = 0; t < ix->txs.size(); t++) tx_gene[t] = ix->txs[t].gene_idx;
  const std::vector<int32_t> sq_of_name = thm::sq_of_name(ix, nullptr);
  std::vector<int32_t> ref_sq(ix->refs.size() + 1, -1);
  for (size_t r = 0; r < ix->refs.size(); r++)
    if (ix->refs[r].name_id < sq_of_name.size()) ref_sq[r] = sq_of_name[ix->refs[r].name_id];
  HIPCHK(a, a->bt_tx_gene.ensure(tx_gene.size() * 4));
  HIPCHK(a, a->bt_ref_sq.ensure(ref_sq.size() * 4));
  HIPCHK(a, hipMemcpy(a->bt_tx_gene.p, tx_gene.data(), tx_gene.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(a, hipMemcpy(a->bt_ref_sq.p, ref_sq.data(), ref_sq.size() * 4, hipMemcpyHostToDevice));
  a->bam_tables = true;
  return THM_OK;
}

extern "C" int32_t thm_batch_upload_reads(thm_aligner* a, const thm_read_batch* reads) {
  if (!a || !reads) return THM_ERR_INVALID_ARG;
  const uint64_t n = reads->n_reads;
  if (!reads->offsets || !reads->name_off || (n && !reads->names && reads->name_off[n] > 0))
    return fail(a, THM_ERR_INVALID_ARG, "thm_batch_upload_reads: null offsets or names");
  if (reads->name_off[0] != 0) return fail(a, THM_ERR_INVALID_ARG, "name_off[0] must be 0");
  for (uint64_t i = 0; i < n; i++)
    if (reads->name_off[i + 1] < reads->name_off[i]) return fail(a, THM_ERR_INVALID_ARG, "name offsets are not monotone");
  int rc = thm_batch_upload(a, reads->bases, reads->offsets, n);
  if (rc != THM_OK) return rc;
  hipStream_t s = a->stream;
  const uint64_t nn = reads->name_off[n], nb = reads->offsets[n];
  HIPCHK(a, a->bn_names.ensure(nn + 16));
  HIPCHK(a, a->bn_name_off.ensure((n + 1) * 8));
  if (nn) HIPCHK(a, hipMemcpyAsync(a->bn_names.p, reads->names, nn, hipMemcpyHostToDevice, s));
  HIPCHK(a, hipMemcpyAsync(a->bn_name_off.p, reads->name_off, (n + 1) * 8, hipMemcpyHostToDevice, s));
  a->reads_have_quals = reads->quals != nullptr;
  if (reads->quals) {
    HIPCHK(a, a->bn_quals.ensure(nb + 16));
    if (nb) HIPCHK(a, hipMemcpyAsync(a->bn_quals.p, reads->quals, nb, hipMemcpyHostToDevice, s));
  }
  HIPCHK(a, hipStreamSynchronize(s));
  a->reads_named = true;
  return THM_OK;
}

int bam_records_on_device(thm_aligner* a, uint32_t flags, int timing, BamOnDevice* r) {
  if (flags & ~(uint32_t)THM_BAM_NO_ANNOTATION_TAGS) return fail(a, THM_ERR_INVALID_ARG, "thm_batch_fetch_bam: unknown flag bits 0x%x", flags);
  if (!a->uploaded || !a->reads_named)
    return fail(a, THM_ERR_INVALID_ARG, "thm_batch_fetch_bam: the batch was not uploaded by thm_batch_upload_reads (no names)");
  int rc = thm_batch_sync(a);
  if (rc != THM_OK) return rc;
  HIPCHK(a, hipSetDevice(a->device));
  rc = bam_tables_on_device(a);
  if (rc != THM_OK) return rc;
  HIPCHK(a, ensure_events(a->ev_bam));
  if (a->bam_stage < 0) {  // THM_BAM_EMIT=bytes: the other form of the emit kernel (DESIGN.md section 4.9 has both times)
    const char* e = getenv("THM_BAM_EMIT");
    a->bam_stage = e && !strcmp(e, "bytes") ? 0 : 1;
  }
  const uint64_t n = a->n_reads;
  hipStream_t s = a->stream;
  a->timings[timing] = 0;
  const thm_index* ix = a->ix;
  BamParams p;
  memset(&p, 0, sizeof p);
  p.n_reads = n;
  p.flags = flags;
  p.n_refs = (uint32_t)ix->refs.size();
  p.n_txs = (uint32_t)ix->txs.size();
  p.n_genes = (uint32_t)ix->genes.size();
  p.bases = a->r_bases.as<uint8_t>();
  p.offsets = a->r_offsets.as<uint64_t>();
  p.quals = a->reads_have_quals ? a->bn_quals.as<uint8_t>() : nullptr;
  p.names = a->bn_names.as<uint8_t>();
  p.name_off = a->bn_name_off.as<uint64_t>();
  p.aln_off = a->e_aln_off.as<uint64_t>();
  p.alns = a->o_alns.as<thm_aln>();
  p.tx_pool = a->bt_tx_pool.as<uint8_t>();
  p.tx_off = a->bt_tx_off.as<uint32_t>();
  p.gid_pool = a->bt_gid_pool.as<uint8_t>();
  p.gid_off = a->bt_gid_off.as<uint32_t>();
  p.gname_pool = a->bt_gname_pool.as<uint8_t>();
  p.gname_off = a->bt_gname_off.as<uint32_t>();
  p.tx_gene = a->bt_tx_gene.as<uint32_t>();
  p.ref_sq = a->bt_ref_sq.as<int32_t>();
  // ---- per read: records and QNAME length; their scan travels with the sizes thm_batch_fetch takes first
  HIPCHK(a, a->bm_cnt.ensure((n + 1) * 8));
  HIPCHK(a, a->bm_first.ensure((n + 2) * 8));
  HIPCHK(a, a->bm_qn.ensure((n + 1) * 4));
  HIPCHK(a, a->bm_read_off.ensure((n + 2) * 8));
  HIPCHK(a, a->bm_err.ensure(64));
  HIPCHK(a, a->bm_scan_tmp.ensure(scan_tmp_entries(n + 1) * 8 + 64));
  p.rec_cnt = a->bm_cnt.as<uint64_t>();
  p.rec_first = a->bm_first.as<uint64_t>();
  p.qn = a->bm_qn.as<uint32_t>();
  p.read_rec_off = a->bm_read_off.as<uint64_t>();
  p.err = a->bm_err.as<unsigned int>();
  HIPCHK(a, hipMemsetAsync(a->bm_err.p, 0, 64, s));
  HIPCHK(a, launch_bam_prep(p, s));
  HIPCHK(a, launch_exclusive_scan_u64(a->bm_cnt.as<uint64_t>(), a->bm_first.as<uint64_t>(), n, a->bm_scan_tmp.as<uint64_t>(), s));
  BatchSizes z;
  uint64_t n_rec = 0;
  rc = fetch_batch_sizes(a, nullptr, a->bm_first.as<uint64_t>() + n, &n_rec, &z);
  if (rc != THM_OK) return rc;
  const uint64_t n_alns = z.n_alns;
  if (n_rec > n_alns + n) return fail(a, THM_ERR_INTERNAL, "more BAM records than alignments and reads");
  // ---- the two CIGAR passes, as thm_batch_fetch_cigars runs them (THM_T_CIGAR belongs to that call)
  uint64_t n_words = 0;
  unsigned any_flags = 0;
  const float t_cigar = a->timings[THM_T_CIGAR];
  rc = run_cigar_passes(a, compacted_cigar_params(a, z), n_alns, &n_words, &any_flags);
  a->timings[THM_T_CIGAR] = t_cigar;
  if (rc != THM_OK) return rc;
  p.n_rec = n_rec;
  p.digests = a->c_dig.as<thm_aln_digest>();
  p.words = a->c_words.as<uint32_t>();
  p.n_words = n_words;
  // ---- size pass and its scan; one synchronisation sizes the output
  HIPCHK(a, a->bm_rec_read.ensure((n_rec + 1) * 4));
  HIPCHK(a, a->bm_len.ensure((n_rec + 1) * 8));
  HIPCHK(a, a->bm_off.ensure((n_rec + 2) * 8));
  HIPCHK(a, a->bm_scan_tmp.ensure(scan_tmp_entries(n_rec + 1) * 8 + 64));
  p.rec_read = a->bm_rec_read.as<uint32_t>();
  p.rec_len = a->bm_len.as<uint64_t>();
  p.rec_off = a->bm_off.as<uint64_t>();
  HIPCHK(a, hipEventRecord(a->ev_bam[0], s));
  HIPCHK(a, launch_bam_size(p, s));
  HIPCHK(a, launch_exclusive_scan_u64(a->bm_len.as<uint64_t>(), a->bm_off.as<uint64_t>(), n_rec, a->bm_scan_tmp.as<uint64_t>(), s));
  HIPCHK(a, hipEventRecord(a->ev_bam[1], s));
  unsigned long long n_bytes = 0;
  unsigned err = 0;
  HIPCHK(a, hipMemcpyAsync(&n_bytes, a->bm_off.as<uint64_t>() + n_rec, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipMemcpyAsync(&err, a->bm_err.p, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipStreamSynchronize(s));
  // what thm_writer_format_batch_cigars reports for the same batch
  if (any_flags & THM_DIGEST_MALFORMED) return fail(a, THM_ERR_INTERNAL, "malformed op stream in the compacted pool");
  if (err & BAM_ERR_QNAME) return fail(a, THM_ERR_INTERNAL, "thm_writer_format_batch: read name longer than 254 bytes cannot be stored in BAM");
  if (err & BAM_ERR_DIGEST_FLAGS) return fail(a, THM_ERR_INTERNAL, "thm_writer_format_batch: a run of 2^28 or more has no CIGAR word");
  if (err & BAM_ERR_CIGAR_WORDS) return fail(a, THM_ERR_INTERNAL, "thm_writer_format_batch: malformed op stream");
  if (err & BAM_ERR_RANGE) return fail(a, THM_ERR_INTERNAL, "thm_writer_format_batch: alignment record out of range");
  // ---- emit and offsets
  HIPCHK(a, a->bm_out.ensure(n_bytes + 16));
  p.out = a->bm_out.as<uint8_t>();
  HIPCHK(a, hipEventRecord(a->ev_bam[2], s));
  HIPCHK(a, launch_bam_emit(p, a->bam_stage == 1, a->n_cu, s));
  HIPCHK(a, hipEventRecord(a->ev_bam[3], s));
  HIPCHK(a, launch_bam_offsets(p, s));
  r->n_reads = n;
  r->n_alns = n_alns;
  r->n_records = n_rec;
  r->n_bytes = n_bytes;
  r->any_failed = z.any_failed;
  return THM_OK;
}

extern "C" {

int32_t thm_batch_fetch_bam(thm_aligner* a, uint32_t flags, thm_bam_view* out) {
  if (!a || !out) return THM_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  BamOnDevice r;
  int rc = bam_records_on_device(a, flags, THM_T_BAM, &r);
  if (rc != THM_OK) return rc;
  const uint64_t n = r.n_reads, n_rec = r.n_records, n_bytes = r.n_bytes;
  hipStream_t s = a->stream;
  // ---- the copies
  const int k = a->b_cur ^= 1;  // the other set still backs the previous view
  HBuf& h_data = a->bh_data[k];
  HBuf& h_off = a->bh_off[k];
  HBuf& h_stat = a->bh_stat[k];
  HIPCHK(a, h_data.ensure(n_bytes));
  HIPCHK(a, h_off.ensure((n + 1) * 8));
  if (n_bytes) HIPCHK(a, hipMemcpyAsync(h_data.p, a->bm_out.p, n_bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipMemcpyAsync(h_off.p, a->bm_read_off.p, (n + 1) * 8, hipMemcpyDeviceToHost, s));
  rc = enqueue_statuses(a, r.any_failed, h_stat);
  if (rc != THM_OK) return rc;
  HIPCHK(a, hipStreamSynchronize(s));
  (void)elapsed_ms(a->ev_bam, &a->timings[THM_T_BAM]);
  out->n_reads = n;
  out->n_records = n_rec;
  out->n_bytes = n_bytes;
  out->data = h_data.as<uint8_t>();
  out->read_rec_off = h_off.as<uint64_t>();
  failed_reads(a, r.any_failed, h_stat, &out->n_failed_reads, &out->read_status);
  return THM_OK;
}

int32_t thm_align_batch_bam(thm_aligner* a, const thm_read_batch* reads, uint32_t flags, thm_bam_view* out) {
  if (!a || !out) return THM_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  int rc = thm_batch_upload_reads(a, reads);
  if (rc != THM_OK) return rc;
  rc = thm_batch_run(a);
  if (rc != THM_OK) return rc;
  return thm_batch_fetch_bam(a, flags, out);
}

}  // extern "C"
