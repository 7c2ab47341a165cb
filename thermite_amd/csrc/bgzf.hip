// bgzf.hip -- host side of thm_batch_fetch_bgzf (include/thermite_io.h): the BAM records of a run, which bam.hip leaves
// in device memory, cut into blocks of 0xff00 bytes as bgzf_compress of io_writer.cpp cuts them and deflated there by
// kernels_bgzf.hip, each block a complete BGZF member; only the members, their offsets and the statuses come back.
#include <hip/hip_runtime.h>

#include <cstring>

#include "aligner_internal.h"
#include "bgzf_device.h"
#include "io_internal.h"

using namespace thm;

namespace {

// d_in[0, n) (4-byte aligned) -> members back to back in bz_out, their offsets in bz_off; synchronises the stream once
// and sets THM_T_BGZF
int bgzf_on_device(thm_aligner* a, const uint8_t* d_in, uint64_t n, uint64_t* n_blocks, uint64_t* n_bytes) {
  hipStream_t s = a->stream;
  HIPCHK(a, ensure_events(a->ev_bgzf));
  a->timings[THM_T_BGZF] = 0;
  const uint64_t nb = (n + bgz::BLOCK_IN - 1) / bgz::BLOCK_IN;
  *n_blocks = nb;
  *n_bytes = 0;
  HIPCHK(a, a->bz_off.ensure((nb + 2) * 8));
  if (nb == 0) {
    HIPCHK(a, hipMemsetAsync(a->bz_off.p, 0, 8, s));
    HIPCHK(a, hipStreamSynchronize(s));
    return THM_OK;
  }
  BgzfParams p;
  memset(&p, 0, sizeof p);
  HIPCHK(a, a->bz_match.ensure((size_t)bgzf_grid(nb, a->n_cu) * bgz::BLOCK_IN * 4));
  HIPCHK(a, a->bz_slots.ensure(nb * bgz::SLOT));
  HIPCHK(a, a->bz_sizes.ensure((nb + 1) * 8));
  HIPCHK(a, a->bz_scan_tmp.ensure(scan_tmp_entries(nb + 1) * 8 + 64));
  HIPCHK(a, a->bz_out.ensure(n + nb * 31 + 16));  // a member is at most its input + 31 bytes (stored)
  p.in = d_in;
  p.n = n;
  p.n_blocks = nb;
  p.match = a->bz_match.as<uint32_t>();
  p.slots = a->bz_slots.as<uint8_t>();
  p.sizes = a->bz_sizes.as<uint64_t>();
  p.off = a->bz_off.as<uint64_t>();
  p.out = a->bz_out.as<uint8_t>();
  HIPCHK(a, hipEventRecord(a->ev_bgzf[0], s));
  HIPCHK(a, launch_bgzf_deflate(p, a->n_cu, s));
  HIPCHK(a, launch_exclusive_scan_u64(a->bz_sizes.as<uint64_t>(), a->bz_off.as<uint64_t>(), nb, a->bz_scan_tmp.as<uint64_t>(), s));
  HIPCHK(a, launch_bgzf_compact(p, a->n_cu, s));
  HIPCHK(a, hipEventRecord(a->ev_bgzf[1], s));
  unsigned long long total = 0;
  HIPCHK(a, hipMemcpyAsync(&total, a->bz_off.as<uint64_t>() + nb, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipStreamSynchronize(s));
  if (total > n + nb * 31 || total < nb * 28) return fail(a, THM_ERR_INTERNAL, "BGZF members of impossible size");
  (void)elapsed_ms(a->ev_bgzf[0], a->ev_bgzf[1], &a->timings[THM_T_BGZF]);
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
  rc = bgzf_on_device(a, a->bm_out.as<uint8_t>(), r.n_bytes, &nb, &n_bytes);
  if (rc != THM_OK) return rc;
  hipStream_t s = a->stream;
  const uint64_t n = r.n_reads;
  const int k = a->z_cur ^= 1;  // the other set still backs the previous view
  HBuf& h_data = a->zh_data[k];
  HBuf& h_off = a->zh_off[k];
  HBuf& h_stat = a->zh_stat[k];
  HIPCHK(a, h_data.ensure(n_bytes));
  HIPCHK(a, h_off.ensure((nb + 1) * 8));
  if (n_bytes) HIPCHK(a, hipMemcpyAsync(h_data.p, a->bz_out.p, n_bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipMemcpyAsync(h_off.p, a->bz_off.p, (nb + 1) * 8, hipMemcpyDeviceToHost, s));
  rc = enqueue_statuses(a, r.any_failed, h_stat);
  if (rc != THM_OK) return rc;
  HIPCHK(a, hipStreamSynchronize(s));
  out->n_reads = n;
  out->n_records = r.n_records;
  out->n_raw_bytes = r.n_bytes;
  out->n_blocks = nb;
  out->n_bytes = n_bytes;
  out->data = h_data.as<uint8_t>();
  out->block_off = h_off.as<uint64_t>();
  failed_reads(a, r.any_failed, h_stat, &out->n_failed_reads, &out->read_status);
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
  HIPCHK(a, a->bz_dbg_in.ensure(n + 16));
  if (n) HIPCHK(a, hipMemcpyAsync(a->bz_dbg_in.p, in, n, hipMemcpyHostToDevice, a->stream));
  const float t = a->timings[THM_T_BGZF];
  uint64_t nb = 0, n_bytes = 0;
  const int rc = bgzf_on_device(a, a->bz_dbg_in.as<uint8_t>(), n, &nb, &n_bytes);
  a->timings[THM_T_BGZF] = t;
  if (rc != THM_OK) return rc;
  if (n_bytes > cap) return fail(a, THM_ERR_INVALID_ARG, "thm_debug_bgzf_device: %llu bytes do not fit into %llu", (unsigned long long)n_bytes, (unsigned long long)cap);
  if (n_bytes) HIPCHK(a, hipMemcpy(out, a->bz_out.p, n_bytes, hipMemcpyDeviceToHost));
  *n_out = n_bytes;
  *n_blocks = nb;
  return THM_OK;
}

}  // extern "C"
