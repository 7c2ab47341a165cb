// bam.hip -- host side of the BAM entry points (include/thermite_io.h): thm_batch_upload_reads places names and
// qualities beside the reads, thm_batch_fetch_bam stands where thm_batch_fetch / thm_batch_fetch_cigars stand after a
// run and hands back the finished BAM records of the writer loop (reference src/aligner.rs:54-116) -- what
// format_range_bam of io_writer.cpp encodes on the host -- built by kernels_bam.hip from what is resident on the device.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "aligner_internal.h"
#include "io_internal.h"
#include "launch_io.h"

using namespace thm;

namespace {

// strings back to back with u32 offsets [n + 1]
int upload_pool(thm_aligner* a, const std::vector<std::string>& v, DArr<uint8_t>& pool, DArr<uint32_t>& off) {
  std::vector<uint32_t> o(v.size() + 1, 0);
  std::string all;
  for (size_t i = 0; i < v.size(); i++) {
    all += v[i];
    if (all.size() >= 0xFFFFFFFFull) return fail(a, THM_ERR_UNSUPPORTED, "name table of 4 GiB or more");
    o[i + 1] = (uint32_t)all.size();
  }
  HIPCHK(a, pool.ensure(all.size(), 16));
  HIPCHK(a, off.ensure(o.size()));
  if (!all.empty()) HIPCHK(a, hipMemcpy(pool, all.data(), all.size(), hipMemcpyHostToDevice));
  HIPCHK(a, hipMemcpy(off, o.data(), o.size() * 4, hipMemcpyHostToDevice));
  return THM_OK;
}

}  // namespace

// the index's name tables, once per aligner
int bam_tables_on_device(thm_aligner* a) {
  if (a->bam.tables) return THM_OK;
  const thm_index* ix = a->ix;
  if (ix->contig_names.empty() || ix->tx_ids.size() != ix->txs.size() || ix->gene_ids.size() != ix->genes.size() ||
      ix->gene_names.size() != ix->genes.size())
    return fail(a, THM_ERR_INVALID_ARG, "thm_batch_fetch_bam needs contig / transcript / gene names: thm_index_set_names or thm_index_create_from_files");
  int rc = upload_pool(a, ix->tx_ids, a->bam.tx_pool, a->bam.tx_off);
  if (rc == THM_OK) rc = upload_pool(a, ix->gene_ids, a->bam.gid_pool, a->bam.gid_off);
  if (rc == THM_OK) rc = upload_pool(a, ix->gene_names, a->bam.gname_pool, a->bam.gname_off);
  if (rc != THM_OK) return rc;
  std::vector<uint32_t> tx_gene(ix->txs.size() + 1, 0);
  for (size_t t = 0; t < ix->txs.size(); t++) tx_gene[t] = ix->txs[t].gene_idx;
  const std::vector<int32_t> sq_of_name = thm::sq_of_name(ix, nullptr);
  std::vector<int32_t> ref_sq(ix->refs.size() + 1, -1);
  for (size_t r = 0; r < ix->refs.size(); r++)
    if (ix->refs[r].name_id < sq_of_name.size()) ref_sq[r] = sq_of_name[ix->refs[r].name_id];
  HIPCHK(a, a->bam.tx_gene.ensure(tx_gene.size()));
  HIPCHK(a, a->bam.ref_sq.ensure(ref_sq.size()));
  HIPCHK(a, hipMemcpy(a->bam.tx_gene, tx_gene.data(), tx_gene.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(a, hipMemcpy(a->bam.ref_sq, ref_sq.data(), ref_sq.size() * 4, hipMemcpyHostToDevice));
  a->bam.tables = true;
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
  HIPCHK(a, a->bam.names.ensure(nn, 16));
  HIPCHK(a, a->bam.name_off.ensure(n + 1));
  if (nn) HIPCHK(a, hipMemcpyAsync(a->bam.names, reads->names, nn, hipMemcpyHostToDevice, s));
  HIPCHK(a, hipMemcpyAsync(a->bam.name_off, reads->name_off, (n + 1) * 8, hipMemcpyHostToDevice, s));
  a->bam.reads_have_quals = reads->quals != nullptr;
  if (reads->quals) {
    HIPCHK(a, a->bam.quals.ensure(nb, 16));
    if (nb) HIPCHK(a, hipMemcpyAsync(a->bam.quals, reads->quals, nb, hipMemcpyHostToDevice, s));
  }
  HIPCHK(a, hipStreamSynchronize(s));
  a->bam.reads_named = true;
  return THM_OK;
}

int bam_records_on_device(thm_aligner* a, uint32_t flags, int timing, BamOnDevice* r) {
  if (flags & ~(uint32_t)THM_BAM_NO_ANNOTATION_TAGS) return fail(a, THM_ERR_INVALID_ARG, "thm_batch_fetch_bam: unknown flag bits 0x%x", flags);
  if (!a->uploaded || !a->bam.reads_named)
    return fail(a, THM_ERR_INVALID_ARG, "thm_batch_fetch_bam: the batch was not uploaded by thm_batch_upload_reads (no names)");
  int rc = thm_batch_sync(a);
  if (rc != THM_OK) return rc;
  HIPCHK(a, hipSetDevice(a->device));
  rc = bam_tables_on_device(a);
  if (rc != THM_OK) return rc;
  HIPCHK(a, ensure_events(a->bam.ev));
  if (a->bam.stage < 0) {  // THM_BAM_EMIT=bytes: the other form of the emit kernel (DESIGN.md section 4.9 has both times)
    const char* e = getenv("THM_BAM_EMIT");
    a->bam.stage = e && !strcmp(e, "bytes") ? 0 : 1;
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
  p.bases = a->reads.bases;
  p.offsets = a->reads.offsets;
  p.quals = a->bam.reads_have_quals ? a->bam.quals : nullptr;
  p.names = a->bam.names;
  p.name_off = a->bam.name_off;
  p.aln_off = a->ext.aln_off;
  p.alns = a->out.alns;
  p.tx_pool = a->bam.tx_pool;
  p.tx_off = a->bam.tx_off;
  p.gid_pool = a->bam.gid_pool;
  p.gid_off = a->bam.gid_off;
  p.gname_pool = a->bam.gname_pool;
  p.gname_off = a->bam.gname_off;
  p.tx_gene = a->bam.tx_gene;
  p.ref_sq = a->bam.ref_sq;
  // ---- per read: records and QNAME length; their scan travels with the sizes thm_batch_fetch takes first
  HIPCHK(a, a->bam.cnt.ensure(n + 1));
  HIPCHK(a, a->bam.first.ensure(n + 2));
  HIPCHK(a, a->bam.qn.ensure(n + 1));
  HIPCHK(a, a->bam.read_off.ensure(n + 2));
  HIPCHK(a, a->bam.err.ensure(16));
  p.rec_cnt = a->bam.cnt;
  p.rec_first = a->bam.first;
  p.qn = a->bam.qn;
  p.read_rec_off = a->bam.read_off;
  p.err = a->bam.err;
  HIPCHK(a, hipMemsetAsync(a->bam.err, 0, 64, s));
  HIPCHK(a, launch_bam_prep(p, s));
  rc = scan_u64(a, a->stage_scan_tmp, a->bam.cnt, a->bam.first, n, s);
  if (rc != THM_OK) return rc;
  BatchSizes z;
  uint64_t n_rec = 0;
  rc = fetch_batch_sizes(a, nullptr, a->bam.first + n, &n_rec, &z);
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
  p.digests = a->cig.dig;
  p.words = a->cig.words;
  p.n_words = n_words;
  // ---- size pass and its scan; one synchronisation sizes the output
  HIPCHK(a, a->bam.rec_read.ensure(n_rec + 1));
  HIPCHK(a, a->bam.len.ensure(n_rec + 1));
  HIPCHK(a, a->bam.off.ensure(n_rec + 2));
  p.rec_read = a->bam.rec_read;
  p.rec_len = a->bam.len;
  p.rec_off = a->bam.off;
  HIPCHK(a, hipEventRecord(a->bam.ev[0], s));
  HIPCHK(a, launch_bam_size(p, s));
  rc = scan_u64(a, a->stage_scan_tmp, a->bam.len, a->bam.off, n_rec, s);
  if (rc != THM_OK) return rc;
  HIPCHK(a, hipEventRecord(a->bam.ev[1], s));
  unsigned long long n_bytes = 0;
  unsigned err = 0;
  HIPCHK(a, hipMemcpyAsync(&n_bytes, a->bam.off + n_rec, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipMemcpyAsync(&err, a->bam.err, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipStreamSynchronize(s));
  // what thm_writer_format_batch_cigars reports for the same batch
  if (any_flags & THM_DIGEST_MALFORMED) return fail(a, THM_ERR_INTERNAL, "malformed op stream in the compacted pool");
  if (err & BAM_ERR_QNAME) return fail(a, THM_ERR_INTERNAL, "thm_writer_format_batch: read name longer than 254 bytes cannot be stored in BAM");
  if (err & BAM_ERR_DIGEST_FLAGS) return fail(a, THM_ERR_INTERNAL, "thm_writer_format_batch: a run of 2^28 or more has no CIGAR word");
  if (err & BAM_ERR_CIGAR_WORDS) return fail(a, THM_ERR_INTERNAL, "thm_writer_format_batch: malformed op stream");
  if (err & BAM_ERR_RANGE) return fail(a, THM_ERR_INTERNAL, "thm_writer_format_batch: alignment record out of range");
  // ---- emit and offsets
  HIPCHK(a, a->bam.out.ensure(n_bytes, 16));
  p.out = a->bam.out;
  HIPCHK(a, hipEventRecord(a->bam.ev[2], s));
  HIPCHK(a, launch_bam_emit(p, a->bam.stage == 1, a->n_cu, s));
  HIPCHK(a, hipEventRecord(a->bam.ev[3], s));
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
  BytesHost& h = a->bam.host.next();  // the other set still backs the previous view
  HIPCHK(a, h.data.ensure(n_bytes));
  HIPCHK(a, h.off.ensure(n + 1));
  if (n_bytes) HIPCHK(a, hipMemcpyAsync(h.data, a->bam.out, n_bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipMemcpyAsync(h.off, a->bam.read_off, (n + 1) * 8, hipMemcpyDeviceToHost, s));
  rc = enqueue_statuses(a, r.any_failed, h.stat);
  if (rc != THM_OK) return rc;
  HIPCHK(a, hipStreamSynchronize(s));
  (void)elapsed_ms(a->bam.ev, &a->timings[THM_T_BAM]);
  out->n_reads = n;
  out->n_records = n_rec;
  out->n_bytes = n_bytes;
  out->data = h.data;
  out->read_rec_off = h.off;
  failed_reads(a, r.any_failed, h.stat, &out->n_failed_reads, &out->read_status);
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
