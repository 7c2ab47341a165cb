// bai.hip -- host side of thm_bam_sorter_index (include/thermite_io.h): the .bai of the sorted stream from what
// thm_bam_sorter_finish left on the device (the sorted records' offsets and places) and the members' compressed sizes the
// windows left on the host.  kernels_bai.hip has the passes, bai_device.h the functions they spread over threads;
// DESIGN.md section 4.16.  Every buffer but the pinned result is freed before the call returns.
#include <hip/hip_runtime.h>

#include <cstring>

#include "aligner_internal.h"
#include "bai_device.h"
#include "bam_sort_internal.h"
#include "io_internal.h"
#include "launch_io.h"

using namespace thm;

namespace {

const char* const WHO = "thm_bam_sorter_index";

// n zeroed words (one at least)
template <class T>
hipError_t zeroed(DArr<T>& b, size_t n, hipStream_t st) {
  static_assert(sizeof(T) == 8, "words");
  hipError_t e = b.ensure(n ? n : 1);
  return e == hipSuccess ? hipMemsetAsync(b, 0, (n ? n : 1) * 8, st) : e;
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
  // (everything of this call's own is freed when it returns)
  DArr<uint64_t> key, d_coff, scan_tmp;
  DArr<uint32_t> beg, end;
  DBuf scal;  // [0], [1]: the error records (unsigned long long, for the atomics); [2]: n_coor (uint64_t)
  DArr<unsigned long long> ref_mapped, ref_intv;
  DArr<uint64_t> ref_first, ref_end, ref_bin0, ref_bin1, ref_size, ref_at, intv_off;
  HIPCHK(a, key.ensure(n, 8));
  HIPCHK(a, beg.ensure(n, 8));
  HIPCHK(a, end.ensure(n, 8));
  HIPCHK(a, d_coff.ensure(coff.size()));
  HIPCHK(a, scal.ensure(4 * 8));
  HIPCHK(a, scan_reserve(scan_tmp, std::max<uint64_t>(n, n_sq)));  // (the longest of the scans below)
  HIPCHK(a, hipEventRecord(s->ev_bai[0], st));
  HIPCHK(a, zeroed(ref_mapped, n_sq, st));
  HIPCHK(a, zeroed(ref_intv, n_sq, st));
  for (DArr<uint64_t>* b : {&ref_first, &ref_end, &ref_bin0, &ref_bin1}) HIPCHK(a, zeroed(*b, n_sq, st));
  HIPCHK(a, ref_size.ensure(n_sq, 8));
  HIPCHK(a, ref_at.ensure((size_t)n_sq + 1));
  HIPCHK(a, intv_off.ensure((size_t)n_sq + 1));
  HIPCHK(a, hipMemcpyAsync(d_coff, coff.data(), coff.size() * 8, hipMemcpyHostToDevice, st));
  HIPCHK(a, hipMemsetAsync(scal.p, 0xff, 4 * 8, st));
  BaiFieldsParams fp;
  fp.r.off = s->s_off;
  fp.r.loc = s->s_loc;
  fp.r.n = n;
  fp.r.seg_start = s->d_seg_start;
  fp.r.seg = s->d_seg_ptr;
  fp.r.n_seg = (uint32_t)s->segs.size();
  fp.r.n_sq = n_sq;
  fp.key = key;
  fp.beg = beg;
  fp.end = end;
  fp.ref_mapped = ref_mapped;
  fp.ref_intv = ref_intv;
  fp.err = scal.as<unsigned long long>();
  HIPCHK(a, launch_bai_fields(fp, st));
  int rc = scan_u64(a, scan_tmp, reinterpret_cast<const uint64_t*>(ref_intv.get()), intv_off, n_sq, st);
  if (rc != THM_OK) return rc;

  // ---- runs of one (refID, bin): the chunks before merging
  uint64_t n_runs = 0, n_coor = 0, n_table = 0;
  DArr<uint64_t> run_key, run_beg, run_end;
  {
    DArr<uint64_t> flag, idx;
    HIPCHK(a, flag.ensure(n, 8));
    HIPCHK(a, idx.ensure(n + 1));
    BaiRunParams rp;
    rp.key = key;
    rp.off = s->s_off;
    rp.n = n;
    rp.n_sq = n_sq;
    rp.flag = flag;
    rp.idx = idx;
    rp.ref_first = ref_first;
    rp.ref_end = ref_end;
    rp.n_coor = scal.as<uint64_t>() + 2;
    rp.run_key = rp.run_beg = rp.run_end = nullptr;
    HIPCHK(a, launch_bai_run_heads(rp, st));
    rc = scan_u64(a, scan_tmp, flag, idx, n, st);
    if (rc != THM_OK) return rc;
    uint64_t h_scal[4];
    HIPCHK(a, hipMemcpyAsync(h_scal, scal.p, sizeof h_scal, hipMemcpyDeviceToHost, st));
    HIPCHK(a, hipMemcpyAsync(&n_runs, idx + n, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(a, hipMemcpyAsync(&n_table, intv_off + n_sq, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(a, hipStreamSynchronize(st));
    n_coor = h_scal[2];
    if (h_scal[1] != bai::NONE)
      return fail(a, THM_ERR_INTERNAL, "%s: the CIGAR of sorted record %llu does not lie inside the record", WHO, (unsigned long long)h_scal[1]);
    if (h_scal[0] != bai::NONE) {
      // the first record BAI cannot address: its reference and position
      uint64_t k = 0;
      uint32_t b = 0;
      HIPCHK(a, hipMemcpy(&k, key + h_scal[0], 8, hipMemcpyDeviceToHost));
      HIPCHK(a, hipMemcpy(&b, beg + h_scal[0], 4, hipMemcpyDeviceToHost));
      std::vector<std::pair<std::string, uint64_t>> sq;
      (void)thm::sq_of_name(a->ix, &sq);
      const uint32_t r = bai::key_ref(k);
      return fail(a, THM_ERR_INVALID_ARG, "%s: the record on reference %s (refID %u) at position %u ends beyond 2^29, which a .bai cannot address", WHO,
                  r < sq.size() ? sq[r].first.c_str() : "?", r, b & ~bai::MAPPED_BIT);
    }
    if (n_coor > n || n_runs > n_coor) return fail(a, THM_ERR_INTERNAL, "%s: %llu runs of %llu placed records of %llu", WHO, (unsigned long long)n_runs, (unsigned long long)n_coor, (unsigned long long)n);
    HIPCHK(a, run_key.ensure(n_runs, 8));
    HIPCHK(a, run_beg.ensure(n_runs, 8));
    HIPCHK(a, run_end.ensure(n_runs, 8));
    rp.run_key = run_key;
    rp.run_beg = run_beg;
    rp.run_end = run_end;
    HIPCHK(a, launch_bai_runs(rp, st));
    HIPCHK(a, hipStreamSynchronize(st));  // flag and idx go
  }

  // ---- the linear index: minima of raw offsets, then the backward fill
  DArr<unsigned long long> table;
  HIPCHK(a, table.ensure(n_table, 8));
  HIPCHK(a, hipMemsetAsync(table, 0xff, n_table * 8 + 8, st));
  BaiLinearParams lp;
  lp.key = key;
  lp.beg = beg;
  lp.end = end;
  lp.off = s->s_off;
  lp.n = n_coor;
  lp.intv_off = intv_off;
  lp.table = table;
  lp.n_sq = n_sq;
  HIPCHK(a, launch_bai_linear(lp, st));
  HIPCHK(a, launch_bai_fill(lp, st));

  // ---- the runs by (refID, bin), stably; neighbours merge; chunks, bins, the bins of every reference
  DArr<uint64_t> key2, chunk_flag, bin_flag, chunk_idx, bin_idx, chunk_beg, chunk_end, bin_key, bin_chunk0;
  DArr<uint32_t> ord, ord2, chunk_bin;
  DBuf tmp;
  HIPCHK(a, key2.ensure(n_runs, 8));
  HIPCHK(a, ord.ensure(n_runs, 8));
  HIPCHK(a, ord2.ensure(n_runs, 8));
  HIPCHK(a, chunk_flag.ensure(n_runs, 8));
  HIPCHK(a, bin_flag.ensure(n_runs, 8));
  HIPCHK(a, chunk_idx.ensure(n_runs + 1));
  HIPCHK(a, bin_idx.ensure(n_runs + 1));
  HIPCHK(a, chunk_beg.ensure(n_runs, 8));
  HIPCHK(a, chunk_end.ensure(n_runs, 8));
  HIPCHK(a, chunk_bin.ensure(n_runs, 8));
  HIPCHK(a, bin_key.ensure(n_runs, 8));
  HIPCHK(a, zeroed(bin_chunk0, n_runs + 1, st));
  uint64_t n_chunks = 0, n_bins = 0;
  if (n_runs) {
    // (stable: the runs of a bin keep their stream order)
    uint64_t* skey = nullptr;
    uint32_t* sord = nullptr;
    rc = sort_pairs_u64_u32(a, tmp, run_key, key2, ord, ord2, n_runs, (int)bai::key_bits(n_sq), st, &skey, &sord);
    if (rc != THM_OK) return rc;
    BaiChunkParams cp;
    cp.skey = skey;
    cp.ord = sord;
    cp.run_beg = run_beg;
    cp.run_end = run_end;
    cp.n_runs = n_runs;
    cp.n_sq = n_sq;
    cp.chunk_flag = chunk_flag;
    cp.bin_flag = bin_flag;
    cp.chunk_idx = chunk_idx;
    cp.bin_idx = bin_idx;
    cp.chunk_beg = chunk_beg;
    cp.chunk_end = chunk_end;
    cp.chunk_bin = chunk_bin;
    cp.bin_key = bin_key;
    cp.bin_chunk0 = bin_chunk0;
    cp.ref_bin0 = ref_bin0;
    cp.ref_bin1 = ref_bin1;
    HIPCHK(a, launch_bai_chunk_heads(cp, st));
    rc = scan_u64(a, scan_tmp, cp.chunk_flag, chunk_idx, n_runs, st);
    if (rc == THM_OK) rc = scan_u64(a, scan_tmp, cp.bin_flag, bin_idx, n_runs, st);
    if (rc != THM_OK) return rc;
    HIPCHK(a, launch_bai_chunks(cp, st));
    HIPCHK(a, hipMemcpyAsync(&n_chunks, chunk_idx + n_runs, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(a, hipMemcpyAsync(&n_bins, bin_idx + n_runs, 8, hipMemcpyDeviceToHost, st));
  }

  // ---- where every reference stands, and the bytes
  BaiEmitParams ep;
  ep.n_sq = n_sq;
  ep.ref_first = ref_first;
  ep.ref_end = ref_end;
  ep.ref_bin0 = ref_bin0;
  ep.ref_bin1 = ref_bin1;
  ep.ref_mapped = ref_mapped;
  ep.ref_intv = ref_intv;
  ep.intv_off = intv_off;
  ep.table = table;
  ep.ref_size = ref_size;
  ep.ref_at = ref_at;
  ep.bin_key = bin_key;
  ep.bin_chunk0 = bin_chunk0;
  ep.chunk_beg = chunk_beg;
  ep.chunk_end = chunk_end;
  ep.chunk_bin = chunk_bin;
  ep.off = s->s_off;
  ep.coff = d_coff;
  ep.n_no_coor = n - n_coor;
  HIPCHK(a, launch_bai_ref_sizes(ep, st));
  uint64_t all_refs = 0;
  rc = scan_u64(a, scan_tmp, ref_size, ref_at, n_sq, st, &all_refs);
  if (rc != THM_OK) return rc;
  HIPCHK(a, hipStreamSynchronize(st));
  // (the sizes the scans gave must add up to what the counts say, before a kernel writes by them)
  uint64_t n_with_records = 0;
  {
    std::vector<uint64_t> f(n_sq), e(n_sq);
    if (n_sq) {
      HIPCHK(a, hipMemcpy(f.data(), ref_first, (size_t)n_sq * 8, hipMemcpyDeviceToHost));
      HIPCHK(a, hipMemcpy(e.data(), ref_end, (size_t)n_sq * 8, hipMemcpyDeviceToHost));
    }
    for (uint32_t r = 0; r < n_sq; r++) n_with_records += e[r] > f[r];
  }
  const uint64_t want = 8ull * n_sq + 8 * n_bins + 16 * n_chunks + bai::PSEUDO_BYTES * n_with_records + 8 * n_table;
  if (all_refs != want || n_chunks > n_runs || n_bins > n_chunks)
    return fail(a, THM_ERR_INTERNAL, "%s: the references take %llu bytes, the counts give %llu", WHO, (unsigned long long)all_refs, (unsigned long long)want);
  const uint64_t n_bytes = bai::file_bytes(all_refs);
  DArr<uint8_t> d_out;
  HIPCHK(a, d_out.ensure(n_bytes));
  ep.n_chunks = n_chunks;
  ep.n_bytes = n_bytes;
  ep.out = d_out;
  HIPCHK(a, launch_bai_emit(ep, st));
  HIPCHK(a, hipEventRecord(s->ev_bai[1], st));
  HIPCHK(a, s->h_bai.ensure(n_bytes));
  HIPCHK(a, hipMemcpyAsync(s->h_bai, d_out, n_bytes, hipMemcpyDeviceToHost, st));
  HIPCHK(a, hipStreamSynchronize(st));
  out->n_bytes = n_bytes;
  out->data = s->h_bai;
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
