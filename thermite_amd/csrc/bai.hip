// bai.hip -- host side of thm_bam_sorter_index (include/thermite_io.h): the .bai of the sorted stream from what
// thm_bam_sorter_finish left on the device (the sorted records' offsets and places) and the members' compressed sizes the
// windows left on the host.  kernels_bai.hip has the passes, bai_device.h the functions they spread over threads;
// DESIGN.md section 4.16.  Every buffer but the pinned result is freed before the call returns.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstring>

#include "aligner_internal.h"
#include "bai_device.h"
#include "bam_sort_internal.h"
#include "io_internal.h"

using namespace thm;

namespace {

const char* const WHO = "thm_bam_sorter_index";

hipError_t zeroed(DBuf& b, size_t bytes, hipStream_t st) {
  hipError_t e = b.ensure(bytes ? bytes : 8);
  return e == hipSuccess ? hipMemsetAsync(b.p, 0, bytes ? bytes : 8, st) : e;
}

int build(thm_bam_sorter* s, uint64_t first_member_offset, thm_bai_view* out) {
  thm_aligner* a = s->a;
  const uint64_t n = s->n_rec, total = s->n_bytes, n_members = (total + bai::CUT - 1) / bai::CUT;
  const uint32_t n_sq = s->n_sq;
  if (s->member_bytes.size() != n_members)
    return fail(a, THM_ERR_INTERNAL, "%s: %llu member sizes for %llu members", WHO, (unsigned long long)s->member_bytes.size(), (unsigned long long)n_members);
  HIPCHK(a, hipSetDevice(a->device));
  hipStream_t st = a->stream;
  HIPCHK(a, ensure_events(s->ev_bai));
  std::vector<uint64_t> coff(n_members + 1);
  coff[0] = first_member_offset;
  for (uint64_t m = 0; m < n_members; m++) coff[m + 1] = coff[m] + s->member_bytes[m];
  if (coff[n_members] >> 48) return fail(a, THM_ERR_INVALID_ARG, "%s: file offset %llu does not fit a virtual offset", WHO, (unsigned long long)coff[n_members]);

  // ---- per record and per reference
  DBuf key, beg, end, d_coff, scal, scan_tmp;
  DBuf ref_mapped, ref_intv, ref_first, ref_end, ref_bin0, ref_bin1, ref_size, ref_at, intv_off;
  HIPCHK(a, key.ensure(n * 8 + 8));
  HIPCHK(a, beg.ensure(n * 4 + 8));
  HIPCHK(a, end.ensure(n * 4 + 8));
  HIPCHK(a, d_coff.ensure(coff.size() * 8));
  HIPCHK(a, scal.ensure(4 * 8));
  const uint64_t scan_n = std::max<uint64_t>(n, n_sq) + 1;
  HIPCHK(a, scan_tmp.ensure(scan_tmp_entries(scan_n) * 8 + 64));
  HIPCHK(a, hipEventRecord(s->ev_bai[0], st));
  for (DBuf* b : {&ref_mapped, &ref_intv, &ref_first, &ref_end, &ref_bin0, &ref_bin1}) HIPCHK(a, zeroed(*b, (size_t)n_sq * 8, st));
  HIPCHK(a, ref_size.ensure((size_t)n_sq * 8 + 8));
  HIPCHK(a, ref_at.ensure(((size_t)n_sq + 1) * 8));
  HIPCHK(a, intv_off.ensure(((size_t)n_sq + 1) * 8));
  HIPCHK(a, hipMemcpyAsync(d_coff.p, coff.data(), coff.size() * 8, hipMemcpyHostToDevice, st));
  HIPCHK(a, hipMemsetAsync(scal.p, 0xff, 4 * 8, st));  // [0], [1]: the error records; [2]: n_coor
  BaiFieldsParams fp;
  fp.r.off = s->s_off.as<uint64_t>();
  fp.r.loc = s->s_loc.as<uint64_t>();
  fp.r.n = n;
  fp.r.seg_start = s->d_seg_start.as<uint64_t>();
  fp.r.seg = s->d_seg_ptr.as<const uint8_t*>();
  fp.r.n_seg = (uint32_t)s->segs.size();
  fp.r.n_sq = n_sq;
  fp.key = key.as<uint64_t>();
  fp.beg = beg.as<uint32_t>();
  fp.end = end.as<uint32_t>();
  fp.ref_mapped = ref_mapped.as<unsigned long long>();
  fp.ref_intv = ref_intv.as<unsigned long long>();
  fp.err = scal.as<unsigned long long>();
  HIPCHK(a, launch_bai_fields(fp, st));
  HIPCHK(a, launch_exclusive_scan_u64(ref_intv.as<uint64_t>(), intv_off.as<uint64_t>(), n_sq, scan_tmp.as<uint64_t>(), st));

  // ---- runs of one (refID, bin): the chunks before merging
  uint64_t n_runs = 0, n_coor = 0, n_table = 0;
  DBuf run_key, run_beg, run_end;
  {
    DBuf flag, idx;
    HIPCHK(a, flag.ensure(n * 8 + 8));
    HIPCHK(a, idx.ensure((n + 1) * 8));
    BaiRunParams rp;
    rp.key = key.as<uint64_t>();
    rp.off = s->s_off.as<uint64_t>();
    rp.n = n;
    rp.n_sq = n_sq;
    rp.flag = flag.as<uint64_t>();
    rp.idx = idx.as<uint64_t>();
    rp.ref_first = ref_first.as<uint64_t>();
    rp.ref_end = ref_end.as<uint64_t>();
    rp.n_coor = scal.as<uint64_t>() + 2;
    rp.run_key = rp.run_beg = rp.run_end = nullptr;
    HIPCHK(a, launch_bai_run_heads(rp, st));
    HIPCHK(a, launch_exclusive_scan_u64(flag.as<uint64_t>(), idx.as<uint64_t>(), n, scan_tmp.as<uint64_t>(), st));
    uint64_t h_scal[4];
    HIPCHK(a, hipMemcpyAsync(h_scal, scal.p, sizeof h_scal, hipMemcpyDeviceToHost, st));
    HIPCHK(a, hipMemcpyAsync(&n_runs, idx.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(a, hipMemcpyAsync(&n_table, intv_off.as<uint64_t>() + n_sq, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(a, hipStreamSynchronize(st));
    n_coor = h_scal[2];
    if (h_scal[1] != bai::NONE)
      return fail(a, THM_ERR_INTERNAL, "%s: the CIGAR of sorted record %llu does not lie inside the record", WHO, (unsigned long long)h_scal[1]);
    if (h_scal[0] != bai::NONE) {
      // the first record BAI cannot address: its reference and position
      uint64_t k = 0;
      uint32_t b = 0;
      HIPCHK(a, hipMemcpy(&k, key.as<uint64_t>() + h_scal[0], 8, hipMemcpyDeviceToHost));
      HIPCHK(a, hipMemcpy(&b, beg.as<uint32_t>() + h_scal[0], 4, hipMemcpyDeviceToHost));
      std::vector<std::pair<std::string, uint64_t>> sq;
      (void)thm::sq_of_name(a->ix, &sq);
      const uint32_t r = bai::key_ref(k);
      return fail(a, THM_ERR_INVALID_ARG, "%s: the record on reference %s (refID %u) at position %u ends beyond 2^29, which a .bai cannot address", WHO,
                  r < sq.size() ? sq[r].first.c_str() : "?", r, b & ~bai::MAPPED_BIT);
    }
    if (n_coor > n || n_runs > n_coor) return fail(a, THM_ERR_INTERNAL, "%s: %llu runs of %llu placed records of %llu", WHO, (unsigned long long)n_runs, (unsigned long long)n_coor, (unsigned long long)n);
    HIPCHK(a, run_key.ensure(n_runs * 8 + 8));
    HIPCHK(a, run_beg.ensure(n_runs * 8 + 8));
    HIPCHK(a, run_end.ensure(n_runs * 8 + 8));
    rp.run_key = run_key.as<uint64_t>();
    rp.run_beg = run_beg.as<uint64_t>();
    rp.run_end = run_end.as<uint64_t>();
    HIPCHK(a, launch_bai_runs(rp, st));
    HIPCHK(a, hipStreamSynchronize(st));  // flag and idx go
  }

  // ---- the linear index: minima of raw offsets, then the backward fill
  DBuf table;
  HIPCHK(a, table.ensure(n_table * 8 + 8));
  HIPCHK(a, hipMemsetAsync(table.p, 0xff, n_table * 8 + 8, st));
  BaiLinearParams lp;
  lp.key = key.as<uint64_t>();
  lp.beg = beg.as<uint32_t>();
  lp.end = end.as<uint32_t>();
  lp.off = s->s_off.as<uint64_t>();
  lp.n = n_coor;
  lp.intv_off = intv_off.as<uint64_t>();
  lp.table = table.as<unsigned long long>();
  lp.n_sq = n_sq;
  HIPCHK(a, launch_bai_linear(lp, st));
  HIPCHK(a, launch_bai_fill(lp, st));

  // ---- the runs by (refID, bin), stably; neighbours merge; chunks, bins, the bins of every reference
  DBuf key2, ord, ord2, tmp, chunk_flag, bin_flag, chunk_idx, bin_idx, chunk_beg, chunk_end, chunk_bin, bin_key, bin_chunk0;
  HIPCHK(a, key2.ensure(n_runs * 8 + 8));
  HIPCHK(a, ord.ensure(n_runs * 4 + 8));
  HIPCHK(a, ord2.ensure(n_runs * 4 + 8));
  HIPCHK(a, chunk_flag.ensure(n_runs * 8 + 8));
  HIPCHK(a, bin_flag.ensure(n_runs * 8 + 8));
  HIPCHK(a, chunk_idx.ensure((n_runs + 1) * 8));
  HIPCHK(a, bin_idx.ensure((n_runs + 1) * 8));
  HIPCHK(a, chunk_beg.ensure(n_runs * 8 + 8));
  HIPCHK(a, chunk_end.ensure(n_runs * 8 + 8));
  HIPCHK(a, chunk_bin.ensure(n_runs * 4 + 8));
  HIPCHK(a, bin_key.ensure(n_runs * 8 + 8));
  HIPCHK(a, zeroed(bin_chunk0, (n_runs + 1) * 8, st));
  uint64_t n_chunks = 0, n_bins = 0;
  if (n_runs) {
    hipcub::DoubleBuffer<uint64_t> dk(run_key.as<uint64_t>(), key2.as<uint64_t>());
    hipcub::DoubleBuffer<uint32_t> dv(ord.as<uint32_t>(), ord2.as<uint32_t>());
    const int bits = (int)bai::key_bits(n_sq);
    size_t tmp_bytes = 0;
    HIPCHK(a, hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, dk, dv, n_runs, 0, bits, st));
    HIPCHK(a, tmp.ensure(tmp_bytes + 16));
    HIPCHK(a, launch_bam_sort_iota(ord.as<uint32_t>(), n_runs, st));
    // least significant digit first, every pass stable: the runs of a bin keep their stream order
    HIPCHK(a, hipcub::DeviceRadixSort::SortPairs(tmp.p, tmp_bytes, dk, dv, n_runs, 0, bits, st));
    BaiChunkParams cp;
    cp.skey = dk.Current();
    cp.ord = dv.Current();
    cp.run_beg = run_beg.as<uint64_t>();
    cp.run_end = run_end.as<uint64_t>();
    cp.n_runs = n_runs;
    cp.n_sq = n_sq;
    cp.chunk_flag = chunk_flag.as<uint64_t>();
    cp.bin_flag = bin_flag.as<uint64_t>();
    cp.chunk_idx = chunk_idx.as<uint64_t>();
    cp.bin_idx = bin_idx.as<uint64_t>();
    cp.chunk_beg = chunk_beg.as<uint64_t>();
    cp.chunk_end = chunk_end.as<uint64_t>();
    cp.chunk_bin = chunk_bin.as<uint32_t>();
    cp.bin_key = bin_key.as<uint64_t>();
    cp.bin_chunk0 = bin_chunk0.as<uint64_t>();
    cp.ref_bin0 = ref_bin0.as<uint64_t>();
    cp.ref_bin1 = ref_bin1.as<uint64_t>();
    HIPCHK(a, launch_bai_chunk_heads(cp, st));
    HIPCHK(a, launch_exclusive_scan_u64(cp.chunk_flag, chunk_idx.as<uint64_t>(), n_runs, scan_tmp.as<uint64_t>(), st));
    HIPCHK(a, launch_exclusive_scan_u64(cp.bin_flag, bin_idx.as<uint64_t>(), n_runs, scan_tmp.as<uint64_t>(), st));
    HIPCHK(a, launch_bai_chunks(cp, st));
    HIPCHK(a, hipMemcpyAsync(&n_chunks, chunk_idx.as<uint64_t>() + n_runs, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(a, hipMemcpyAsync(&n_bins, bin_idx.as<uint64_t>() + n_runs, 8, hipMemcpyDeviceToHost, st));
  }

  // ---- where every reference stands, and the bytes
  BaiEmitParams ep;
  ep.n_sq = n_sq;
  ep.ref_first = ref_first.as<uint64_t>();
  ep.ref_end = ref_end.as<uint64_t>();
  ep.ref_bin0 = ref_bin0.as<uint64_t>();
  ep.ref_bin1 = ref_bin1.as<uint64_t>();
  ep.ref_mapped = ref_mapped.as<unsigned long long>();
  ep.ref_intv = ref_intv.as<unsigned long long>();
  ep.intv_off = intv_off.as<uint64_t>();
  ep.table = table.as<unsigned long long>();
  ep.ref_size = ref_size.as<uint64_t>();
  ep.ref_at = ref_at.as<uint64_t>();
  ep.bin_key = bin_key.as<uint64_t>();
  ep.bin_chunk0 = bin_chunk0.as<uint64_t>();
  ep.chunk_beg = chunk_beg.as<uint64_t>();
  ep.chunk_end = chunk_end.as<uint64_t>();
  ep.chunk_bin = chunk_bin.as<uint32_t>();
  ep.off = s->s_off.as<uint64_t>();
  ep.coff = d_coff.as<uint64_t>();
  ep.n_no_coor = n - n_coor;
  HIPCHK(a, launch_bai_ref_sizes(ep, st));
  HIPCHK(a, launch_exclusive_scan_u64(ref_size.as<uint64_t>(), ref_at.as<uint64_t>(), n_sq, scan_tmp.as<uint64_t>(), st));
  uint64_t all_refs = 0;
  HIPCHK(a, hipMemcpyAsync(&all_refs, ref_at.as<uint64_t>() + n_sq, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(a, hipStreamSynchronize(st));
  // (the sizes the scans gave must add up to what the counts say, before a kernel writes by them)
  uint64_t n_with_records = 0;
  {
    std::vector<uint64_t> f(n_sq), e(n_sq);
    if (n_sq) {
      HIPCHK(a, hipMemcpy(f.data(), ref_first.p, (size_t)n_sq * 8, hipMemcpyDeviceToHost));
      HIPCHK(a, hipMemcpy(e.data(), ref_end.p, (size_t)n_sq * 8, hipMemcpyDeviceToHost));
    }
    for (uint32_t r = 0; r < n_sq; r++) n_with_records += e[r] > f[r];
  }
  const uint64_t want = 8ull * n_sq + 8 * n_bins + 16 * n_chunks + bai::PSEUDO_BYTES * n_with_records + 8 * n_table;
  if (all_refs != want || n_chunks > n_runs || n_bins > n_chunks)
    return fail(a, THM_ERR_INTERNAL, "%s: the references take %llu bytes, the counts give %llu", WHO, (unsigned long long)all_refs, (unsigned long long)want);
  const uint64_t n_bytes = bai::file_bytes(all_refs);
  DBuf d_out;
  HIPCHK(a, d_out.ensure(n_bytes));
  ep.n_chunks = n_chunks;
  ep.n_bytes = n_bytes;
  ep.out = d_out.as<uint8_t>();
  HIPCHK(a, launch_bai_emit(ep, st));
  HIPCHK(a, hipEventRecord(s->ev_bai[1], st));
  HIPCHK(a, s->h_bai.ensure(n_bytes));
  HIPCHK(a, hipMemcpyAsync(s->h_bai.p, d_out.p, n_bytes, hipMemcpyDeviceToHost, st));
  HIPCHK(a, hipStreamSynchronize(st));
  out->n_bytes = n_bytes;
  out->data = s->h_bai.as<uint8_t>();
  out->n_refs = n_sq;
  out->n_bins = n_bins + n_with_records;
  out->n_chunks = n_chunks;
  out->n_intervals = n_table;
  out->n_no_coor = n - n_coor;
  (void)elapsed_ms(s->ev_bai[0], s->ev_bai[1], &out->index_ms);
  return THM_OK;
}

}  // namespace

extern "C" int32_t thm_bam_sorter_index(thm_bam_sorter* s, uint64_t first_member_offset, thm_bai_view* out) {
  if (!s || !out) return THM_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  thm_aligner* a = s->a;
  if (!s->finished) return fail(a, THM_ERR_INVALID_ARG, "%s: thm_bam_sorter_finish has not been called", WHO);
  if (s->raw_taken) return fail(a, THM_ERR_INVALID_ARG, "%s: a window was taken with THM_SORT_RAW, so there are no member sizes", WHO);
  if (!s->exhausted) return fail(a, THM_ERR_INVALID_ARG, "%s: thm_bam_sorter_next has not returned the exhausted view yet", WHO);
  return build(s, first_member_offset, out);
}
