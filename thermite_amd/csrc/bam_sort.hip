// bam_sort.hip -- host side of thm_bam_sorter (include/thermite_io.h): the BAM records of every batch of a run, which
// bam.hip leaves in device memory, kept there in an arena of segments; at the end one radix sort of (key, ordinal) pairs,
// one scan of the sorted lengths, and then the sorted byte stream window by window: gathered by kernels_bam_sort.hip into
// a staging buffer and deflated from there by the BGZF stage of bgzf.hip.  Only counts, statuses and finished members
// come back to the host.  DESIGN.md section 4.15.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "aligner_internal.h"
#include "bam_sort_device.h"
#include "bam_sort_internal.h"
#include "bgzf_device.h"
#include "io_internal.h"
#include "launch_io.h"

using namespace thm;

namespace {

using Segment = SortSegment;

constexpr uint64_t DEFAULT_WINDOW_BLOCKS = 256;  // 16.7 MB of records a window
constexpr uint64_t MAX_RECORDS = 0xFFFFFFFFull;

}  // namespace

namespace {

// `b` with room for `want` elements, its first `keep` elements kept
template <class T>
int grow(thm_aligner* a, DArr<T>& b, size_t keep, size_t want) {
  if (want * sizeof(T) <= b.cap()) return THM_OK;
  DArr<T> n;
  HIPCHK(a, n.ensure(want));
  if (keep) HIPCHK(a, hipMemcpyAsync(n, b, keep * sizeof(T), hipMemcpyDeviceToDevice, a->stream));
  HIPCHK(a, hipStreamSynchronize(a->stream));
  std::swap(n.b.p, b.b.p);
  std::swap(n.b.cap, b.b.cap);
  return THM_OK;
}

// n records, n_bytes long, that stand back to back in d_data (device) with their offsets in d_off[n + 1]: keys, and the
// bytes into a new segment of the arena.  Nothing is added unless everything succeeded.
int add_resident(thm_bam_sorter* s, const char* who, const uint8_t* d_data, const uint64_t* d_off, uint64_t n, uint64_t n_bytes, float* ms) {
  thm_aligner* a = s->a;
  *ms = 0;
  if (s->n_rec + n > MAX_RECORDS)
    return fail(a, THM_ERR_INVALID_ARG, "%s: %llu records and %llu more are over 2^32-1", who, (unsigned long long)s->n_rec, (unsigned long long)n);
  if (s->max_bytes && s->n_bytes + n_bytes > s->max_bytes)
    return fail(a, THM_ERR_OOM, "%s: %llu bytes of records and the %llu held need %llu bytes, the cap is %llu", who, (unsigned long long)n_bytes,
                (unsigned long long)s->n_bytes, (unsigned long long)(s->n_bytes + n_bytes), (unsigned long long)s->max_bytes);
  if (n == 0) return THM_OK;
  const uint64_t total = s->n_rec + n;
  if (total > s->rec_cap) {
    uint64_t cap = s->rec_cap ? s->rec_cap : 1u << 16;
    while (cap < total) cap *= 2;
    int rc = grow(a, s->key, s->n_rec, cap);
    if (rc == THM_OK) rc = grow(a, s->len, s->n_rec, cap);
    if (rc == THM_OK) rc = grow(a, s->loc, s->n_rec, cap);
    if (rc != THM_OK) return rc;
    s->rec_cap = cap;
  }
  HIPCHK(a, ensure_events(s->ev));
  s->segs.emplace_back();
  Segment& seg = s->segs.back();
  // 16 bytes behind the records: the gather reads whole aligned dwords
  if (hipMalloc(&seg.p, n_bytes + 16) != hipSuccess) {
    (void)hipGetLastError();
    seg.p = nullptr;
    s->segs.pop_back();
    return fail(a, THM_ERR_OOM, "%s: no device memory for %llu bytes of records beside the %llu held (cap %llu)", who, (unsigned long long)n_bytes,
                (unsigned long long)s->n_bytes, (unsigned long long)s->max_bytes);
  }
  hipStream_t st = a->stream;
  BamSortKeysParams p;
  p.data = d_data;
  p.off = d_off;
  p.n = n;
  p.n_sq = s->n_sq;
  p.base = s->n_bytes;
  p.key = s->key + s->n_rec;
  p.len = s->len + s->n_rec;
  p.loc = s->loc + s->n_rec;
  hipError_t e = hipEventRecord(s->ev[0], st);
  if (e == hipSuccess) e = launch_bam_sort_keys(p, st);
  if (e == hipSuccess) e = hipMemcpyAsync(seg.p, d_data, n_bytes, hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync((uint8_t*)seg.p + n_bytes, 0, 16, st);
  if (e == hipSuccess) e = hipEventRecord(s->ev[1], st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    s->segs.pop_back();
    return fail(a, THM_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
  }
  (void)elapsed_ms(s->ev[0], s->ev[1], ms);
  s->seg_start.push_back(s->n_bytes);
  s->n_rec = total;
  s->n_bytes += n_bytes;
  return THM_OK;
}

}  // namespace

extern "C" {

int32_t thm_bam_sorter_create(thm_aligner* a, uint64_t max_bytes, thm_bam_sorter** out) {
  if (!out) return THM_ERR_INVALID_ARG;
  *out = nullptr;
  if (!a) return THM_ERR_INVALID_ARG;
  thm_bam_sorter* s = new thm_bam_sorter();
  s->a = a;
  s->max_bytes = max_bytes;
  std::vector<std::pair<std::string, uint64_t>> sq;
  (void)thm::sq_of_name(a->ix, &sq);
  s->n_sq = (uint32_t)sq.size();
  const char* e = getenv("THM_SORT_GATHER");
  s->by_records = !(e && !strcmp(e, "pieces"));
  *out = s;
  return THM_OK;
}

void thm_bam_sorter_free(thm_bam_sorter* s) {
  if (!s) return;
  int cur = 0;
  (void)hipGetDevice(&cur);
  (void)hipSetDevice(s->a->device);
  (void)hipStreamSynchronize(s->a->stream);
  delete s;
  (void)hipSetDevice(cur);
}

int32_t thm_bam_sorter_add(thm_bam_sorter* s, uint32_t bam_flags, thm_bam_sort_info* info) { return thm::bam_sorter_add(s, bam_flags, info, nullptr); }

}  // extern "C"

int thm::bam_sorter_add(thm_bam_sorter* s, uint32_t bam_flags, thm_bam_sort_info* info, uint64_t* n_aligned_reads) {
  if (!s || !info) return THM_ERR_INVALID_ARG;
  memset(info, 0, sizeof(*info));
  thm_aligner* a = s->a;
  if (s->finished) return fail(a, THM_ERR_INVALID_ARG, "thm_bam_sorter_add: the sorter is finished");
  const float t_bam = a->timings[THM_T_BAM];
  BamOnDevice r;
  int rc = bam_records_on_device(a, bam_flags, THM_T_BAM, &r);
  a->timings[THM_T_BAM] = t_bam;
  if (rc != THM_OK) return rc;
  rc = enqueue_statuses(a, r.any_failed, s->h_stat);  // (first: what can fail after the batch is in must not)
  if (rc != THM_OK) return rc;
  rc = add_resident(s, "thm_bam_sorter_add", a->bam.out, a->bam.off, r.n_records, r.n_bytes, &info->add_ms);
  if (rc != THM_OK) return rc;
  HIPCHK(a, hipStreamSynchronize(a->stream));
  info->n_reads = r.n_reads;
  info->n_records = r.n_records;
  info->n_bytes = r.n_bytes;
  info->total_records = s->n_rec;
  info->total_bytes = s->n_bytes;
  failed_reads(a, r.any_failed, s->h_stat, &info->n_failed_reads, &info->read_status);
  // a read without alignments has exactly one record, the unmapped one
  if (n_aligned_reads) *n_aligned_reads = r.n_reads - (r.n_records - r.n_alns);
  return THM_OK;
}

extern "C" {

int32_t thm_bam_sorter_finish(thm_bam_sorter* s, float* sort_ms) {
  if (!s) return THM_ERR_INVALID_ARG;
  thm_aligner* a = s->a;
  if (sort_ms) *sort_ms = 0;
  if (s->finished) return fail(a, THM_ERR_INVALID_ARG, "thm_bam_sorter_finish: the sorter is finished already");
  const uint64_t n = s->n_rec;
  if (n == 0) {
    s->finished = s->exhausted = true;  // (nothing to hand out: the index may follow at once)
    return THM_OK;
  }
  HIPCHK(a, hipSetDevice(a->device));
  hipStream_t st = a->stream;
  HIPCHK(a, ensure_events(s->ev));
  // (everything of this call's own is freed when it returns)
  DArr<uint64_t> key2, scan_tmp;
  DArr<uint32_t> ord, ord2;
  DBuf tmp;
  HIPCHK(a, key2.ensure(n));
  HIPCHK(a, ord.ensure(n));
  HIPCHK(a, ord2.ensure(n));
  HIPCHK(a, s->s_off.ensure(n + 2));
  HIPCHK(a, s->s_loc.ensure(n));
  HIPCHK(a, scan_reserve(scan_tmp, n));
  // rank n_sq, the unmapped one, must fit: bit_width(n_sq) bits of rank, not log2
  const int bits = (int)bsort::key_bits(s->n_sq);
  uint64_t* s_key = nullptr;
  uint32_t* s_ord = nullptr;
  int rc = sort_pairs_u64_u32(a, tmp, s->key, key2, ord, ord2, n, bits, st, &s_key, &s_ord, s->ev[0]);
  if (rc != THM_OK) return rc;
  // the sorted lengths go where the keys no longer are
  uint64_t* s_len = s_key == s->key.get() ? key2.get() : s->key.get();
  HIPCHK(a, launch_bam_sort_order(s_ord, s->len, s->loc, n, s_len, s->s_loc, st));
  rc = scan_u64(a, scan_tmp, s_len, s->s_off, n, st);
  if (rc != THM_OK) return rc;
  HIPCHK(a, hipEventRecord(s->ev[1], st));
  const uint32_t n_seg = (uint32_t)s->segs.size();
  std::vector<const uint8_t*> ptrs;
  for (const Segment& g : s->segs) ptrs.push_back((const uint8_t*)g.p);
  HIPCHK(a, s->d_seg_start.ensure(n_seg));
  HIPCHK(a, s->d_seg_ptr.ensure(n_seg));
  HIPCHK(a, hipMemcpyAsync(s->d_seg_start, s->seg_start.data(), n_seg * 8, hipMemcpyHostToDevice, st));
  HIPCHK(a, hipMemcpyAsync(s->d_seg_ptr, ptrs.data(), n_seg * sizeof(void*), hipMemcpyHostToDevice, st));
  unsigned long long total = 0;
  HIPCHK(a, hipMemcpyAsync(&total, s->s_off + n, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(a, hipStreamSynchronize(st));
  if (total != s->n_bytes) return fail(a, THM_ERR_INTERNAL, "thm_bam_sorter_finish: the sorted records are %llu bytes, the arena holds %llu", total, (unsigned long long)s->n_bytes);
  if (sort_ms) (void)elapsed_ms(s->ev[0], s->ev[1], sort_ms);
  s->key.release();
  s->len.release();
  s->loc.release();
  s->rec_cap = 0;
  s->finished = true;
  return THM_OK;
}

int32_t thm_bam_sorter_next(thm_bam_sorter* s, uint64_t max_raw_bytes, uint32_t flags, thm_bam_sorted_view* out) {
  if (!s || !out) return THM_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  thm_aligner* a = s->a;
  if (!s->finished) return fail(a, THM_ERR_INVALID_ARG, "thm_bam_sorter_next: thm_bam_sorter_finish has not been called");
  if (flags & ~(uint32_t)THM_SORT_RAW) return fail(a, THM_ERR_INVALID_ARG, "thm_bam_sorter_next: unknown flag bits 0x%x", flags);
  uint64_t window = max_raw_bytes ? max_raw_bytes / bgz::BLOCK_IN * bgz::BLOCK_IN : DEFAULT_WINDOW_BLOCKS * bgz::BLOCK_IN;
  if (window < bgz::BLOCK_IN) window = bgz::BLOCK_IN;
  const uint64_t w0 = s->cursor, left = s->n_bytes - w0, n = left < window ? left : window;
  out->total_records = s->n_rec;
  out->total_raw_bytes = s->n_bytes;
  out->raw_offset = w0;
  if (n == 0) {
    s->exhausted = true;
    return THM_OK;
  }
  HIPCHK(a, hipSetDevice(a->device));
  hipStream_t st = a->stream;
  HIPCHK(a, ensure_events(s->ev));
  HIPCHK(a, s->stage.ensure(n, 64));
  BamSortGatherParams p;
  p.off = s->s_off;
  p.loc = s->s_loc;
  p.n = s->n_rec;
  p.seg_start = s->d_seg_start;
  p.seg = s->d_seg_ptr;
  p.n_seg = (uint32_t)s->segs.size();
  p.w0 = w0;
  p.w1 = w0 + n;
  p.out = s->stage;
  HIPCHK(a, hipEventRecord(s->ev[2], st));
  HIPCHK(a, launch_bam_sort_gather(p, s->by_records, a->n_cu, st));
  HIPCHK(a, hipEventRecord(s->ev[3], st));
  SortHost& h = s->host.next();  // the other set still backs the previous view
  if (flags & THM_SORT_RAW) {
    HIPCHK(a, h.data.ensure(n));
    HIPCHK(a, hipMemcpyAsync(h.data, s->stage, n, hipMemcpyDeviceToHost, st));
    HIPCHK(a, hipStreamSynchronize(st));
    out->n_bytes = n;
    s->raw_taken = true;
  } else {
    const float t_bgzf = a->timings[THM_T_BGZF];
    uint64_t nb = 0, n_bytes = 0;
    const int rc = bgzf_range_on_device(a, s->stage, n, &nb, &n_bytes);
    out->deflate_ms = a->timings[THM_T_BGZF];
    a->timings[THM_T_BGZF] = t_bgzf;
    if (rc != THM_OK) return rc;
    HIPCHK(a, h.data.ensure(n_bytes));
    HIPCHK(a, h.off.ensure(nb + 1));
    HIPCHK(a, hipMemcpyAsync(h.data, a->bgzf.out, n_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(a, hipMemcpyAsync(h.off, a->bgzf.off, (nb + 1) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(a, hipStreamSynchronize(st));
    out->n_blocks = nb;
    out->n_bytes = n_bytes;
    out->block_off = h.off;
    // the index needs every member's compressed size (8 bytes a member, 64 KiB of records each)
    for (uint64_t b = 0; b < nb; b++) s->member_bytes.push_back(out->block_off[b + 1] - out->block_off[b]);
  }
  (void)elapsed_ms(s->ev[2], s->ev[3], &out->gather_ms);
  out->n_raw_bytes = n;
  out->data = h.data;
  s->cursor = w0 + n;
  return THM_OK;
}

// test / tuning hook: which gather the next windows take (0: 16 bytes a lane, 1: a wavefront per record; anything else
// only asks) -> the shape in use before the call
int32_t thm_debug_bam_sorter_gather(thm_bam_sorter* s, int32_t shape) {
  if (!s) return THM_ERR_INVALID_ARG;
  const int32_t was = s->by_records ? 1 : 0;
  if (shape == 0 || shape == 1) s->by_records = shape == 1;
  return was;
}

// test hook: caller-made records (back to back, each beginning with its block_size) through the same key kernel and
// arena as a batch's.  The stream is walked within bounds first.
int32_t thm_debug_bam_sorter_add_records(thm_bam_sorter* s, const uint8_t* bytes, uint64_t n_bytes) {
  if (!s || (!bytes && n_bytes)) return THM_ERR_INVALID_ARG;
  thm_aligner* a = s->a;
  const char* who = "thm_debug_bam_sorter_add_records";
  if (s->finished) return fail(a, THM_ERR_INVALID_ARG, "%s: the sorter is finished", who);
  std::vector<uint64_t> off(1, 0);
  for (uint64_t at = 0; at < n_bytes;) {
    if (n_bytes - at < bsort::MIN_RECORD) return fail(a, THM_ERR_INVALID_ARG, "%s: %llu bytes at offset %llu are no record", who, (unsigned long long)(n_bytes - at), (unsigned long long)at);
    const uint64_t len = (uint64_t)bsort::load_le32(bytes + at) + 4;
    if (len < bsort::MIN_RECORD || len > n_bytes - at)
      return fail(a, THM_ERR_INVALID_ARG, "%s: the record at offset %llu claims %llu bytes", who, (unsigned long long)at, (unsigned long long)len);
    const int32_t ref_id = (int32_t)bsort::load_le32(bytes + at + 4);
    if (ref_id < -1 || ref_id >= (int64_t)s->n_sq)
      return fail(a, THM_ERR_INVALID_ARG, "%s: refID %d of the record at offset %llu is outside [-1, %u)", who, ref_id, (unsigned long long)at, s->n_sq);
    at += len;
    off.push_back(at);
  }
  HIPCHK(a, hipSetDevice(a->device));
  HIPCHK(a, s->dbg_in.ensure(n_bytes, 16));
  HIPCHK(a, s->dbg_off.ensure(off.size()));
  if (n_bytes) HIPCHK(a, hipMemcpy(s->dbg_in, bytes, n_bytes, hipMemcpyHostToDevice));
  HIPCHK(a, hipMemcpy(s->dbg_off, off.data(), off.size() * 8, hipMemcpyHostToDevice));
  float ms = 0;
  return add_resident(s, who, s->dbg_in, s->dbg_off, off.size() - 1, n_bytes, &ms);
}

}  // extern "C"
