// bgzf.hip -- host side of thm_batch_fetch_bgzf (include/thermite_io.h): the BAM records of a run, which bam.hip leaves
// in device memory, cut into blocks of 0xff00 bytes as bgzf_compress of io_writer.cpp cuts them and deflated there by
// kernels_bgzf.hip, each block a complete BGZF member; only the members, their offsets and the statuses come back.
#include <hip/hip_runtime.h>

#include <cstring>

#include "aligner_internal.h"
#include "bgzf_device.h"
#include "io_internal.h"
#include "launch_io.h"

using namespace thm;

namespace {

// d_in[0, n) (4-byte aligned) -> members back to back in bgzf.out, their offsets in bgzf.off; synchronises the stream once
// and sets THM_T_BGZF
int bgzf_on_device(thm_aligner* a, const uint8_t* d_in, uint64_t n, uint64_t* n_blocks, uint64_t* n_bytes) {
  hipStream_t s = a->stream;
  HIPCHK(a, ensure_events(a->bgzf.ev));
  a->timings[THM_T_BGZF] = 0;
  const uint64_t nb = (n + bgz::BLOCK_IN - 1) / bgz::BLOCK_IN;
  *n_blocks = nb;
  *n_bytes = 0;
  HIPCHK(a, a->bgzf.off.ensure(nb + 2));
  if (nb == 0) {
    HIPCHK(a, hipMemsetAsync(a->bgzf.off, 0, 8, s));
    HIPCHK(a, hipStreamSynchronize(s));
    return THM_OK;
  }
  BgzfParams p;
  memset(&p, 0, sizeof p);
  HIPCHK(a, a->bgzf.match.ensure((size_t)bgzf_grid(nb, a->n_cu) * bgz::BLOCK_IN));
  HIPCHK(a, a->bgzf.slots.ensure(nb * bgz::SLOT));
  HIPCHK(a, a->bgzf.sizes.ensure(nb + 1));
  HIPCHK(a, a->bgzf.out.ensure(n + nb * 31, 16));  // a member is at most its input + 31 bytes (stored)
  p.in = d_in;
  p.n = n;
  p.n_blocks = nb;
  p.match = a->bgzf.match;
  p.slots = a->bgzf.slots;
  p.sizes = a->bgzf.sizes;
  p.off = a->bgzf.off;
  p.out = a->bgzf.out;
  HIPCHK(a, hipEventRecord(a->bgzf.ev[0], s));
  HIPCHK(a, launch_bgzf_deflate(p, a->n_cu, s));
  if (const int rc = scan_u64(a, a->stage_scan_tmp, a->bgzf.sizes, a->bgzf.off, nb, s); rc != THM_OK) return rc;
  HIPCHK(a, launch_bgzf_compact(p, a->n_cu, s));
  HIPCHK(a, hipEventRecord(a->bgzf.ev[1], s));
  unsigned long long total = 0;
  HIPCHK(a, hipMemcpyAsync(&total, a->bgzf.off + nb, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipStreamSynchronize(s));
  if (total > n + nb * 31 || total < nb * 28) return fail(a, THM_ERR_INTERNAL, "BGZF members of impossible size");
  (void)elapsed_ms(a->bgzf.ev[0], a->bgzf.ev[1], &a->timings[THM_T_BGZF]);
  *n_bytes = total;
  return THM_OK;
}

}  // namespace

int bgzf_range_on_device(thm_aligner* a, const uint8_t* d_in, uint64_t n, uint64_t* n_blocks, uint64_t* n_bytes) {
  return bgzf_on_device(a, d_in, n, n_blocks, n_bytes);
}

int thm::batch_fetch_bgzf(thm_aligner* a, uint32_t flags, thm_bgzf_view* out, uint64_t* n_aligned_reads) {
  if (!a || !out) return THM_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  BamOnDevice r;
  int rc = bam_records_on_device(a, flags, THM_T_BGZF, &r);
  if (rc != THM_OK) return rc;
  uint64_t nb = 0, n_bytes = 0;
  rc = bgzf_on_device(a, a->bam.out, r.n_bytes, &nb, &n_bytes);
  if (rc != THM_OK) return rc;
  hipStream_t s = a->stream;
  const uint64_t n = r.n_reads;
  BytesHost& h = a->bgzf.host.next();  // the other set still backs the previous view
  HIPCHK(a, h.data.ensure(n_bytes));
  HIPCHK(a, h.off.ensure(nb + 1));
  if (n_bytes) HIPCHK(a, hipMemcpyAsync(h.data, a->bgzf.out, n_bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipMemcpyAsync(h.off, a->bgzf.off, (nb + 1) * 8, hipMemcpyDeviceToHost, s));
  rc = enqueue_statuses(a, r.any_failed, h.stat);
  if (rc != THM_OK) return rc;
  HIPCHK(a, hipStreamSynchronize(s));
  out->n_reads = n;
  out->n_records = r.n_records;
  out->n_raw_bytes = r.n_bytes;
  out->n_blocks = nb;
  out->n_bytes = n_bytes;
  out->data = h.data;
  out->block_off = h.off;
  failed_reads(a, r.any_failed, h.stat, &out->n_failed_reads, &out->read_status);
  // a read without alignments has exactly one record, the unmapped one
  if (n_aligned_reads) *n_aligned_reads = n - (r.n_records - r.n_alns);
  return THM_OK;
}

extern "C" {

int32_t thm_batch_fetch_bgzf(thm_aligner* a, uint32_t flags, thm_bgzf_view* out) { return thm::batch_fetch_bgzf(a, flags, out, nullptr); }

int32_t thm_align_batch_bgzf(thm_aligner* a, const thm_read_batch* reads, uint32_t flags, thm_bgzf_view* out) {
  if (!a || !out) return THM_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  int rc = thm_batch_upload_reads(a, reads);
  if (rc != THM_OK) return rc;
  rc = thm_batch_run(a);
  if (rc != THM_OK) return rc;
  return thm_batch_fetch_bgzf(a, flags, out);
}

// test hook: caller bytes through the same kernels and compaction -> *n_blocks members, *n_out bytes in out[0, cap)
int32_t thm_debug_bgzf_device(thm_aligner* a, const uint8_t* in, uint64_t n, uint8_t* out, uint64_t cap, uint64_t* n_out,
                              uint64_t* n_blocks) {
  if (!a || (!in && n) || !out || !n_out || !n_blocks) return THM_ERR_INVALID_ARG;
  HIPCHK(a, hipSetDevice(a->device));
  HIPCHK(a, a->bgzf.dbg_in.ensure(n, 16));
  if (n) HIPCHK(a, hipMemcpyAsync(a->bgzf.dbg_in, in, n, hipMemcpyHostToDevice, a->stream));
  const float t = a->timings[THM_T_BGZF];
  uint64_t nb = 0, n_bytes = 0;
  const int rc = bgzf_on_device(a, a->bgzf.dbg_in, n, &nb, &n_bytes);
  a->timings[THM_T_BGZF] = t;
  if (rc != THM_OK) return rc;
  if (n_bytes > cap) return fail(a, THM_ERR_INVALID_ARG, "thm_debug_bgzf_device: %llu bytes do not fit into %llu", (unsigned long long)n_bytes, (unsigned long long)cap);
  if (n_bytes) HIPCHK(a, hipMemcpy(out, a->bgzf.out, n_bytes, hipMemcpyDeviceToHost));
  *n_out = n_bytes;
  *n_blocks = nb;
  return THM_OK;
}

}  // extern "C"
