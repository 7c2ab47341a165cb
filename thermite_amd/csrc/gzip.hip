// gzip.hip -- host side of thm_batch_upload_fastq_gzip (include/thermite_io.h): bytes of an
// ordinary .fastq.gz go up compressed, wherever they begin and end.  kernels_gzip.hip searches block starts, decodes
// every run into symbols, chains the runs, resolves the symbols into fq.raw behind the head the caller hands in and
// checks the members (gzip_device.h has the rules); the device FASTQ parser (fastq.hip, parse_resident) runs on the
// block where it stands.  The device's summary -- status, bytes out, bytes consumed -- and the outgoing state come down in
// one synchronisation, because the parse cannot be sized before the inflate has ended; the parse brings its own three.
// A summary with a status word other than 0 sends the same bytes to GzInflater::inflate_slice (io_inflate.cpp), which
// consumes by the same rule: the bytes, or the error and its message, are the host inflater's on every input.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "aligner_internal.h"
#include "gzip_device.h"
#include "io_internal.h"
#include "launch_io.h"

using namespace thm;

static_assert(sizeof(gz::State) == sizeof(thm_gzip_state) && offsetof(gz::State, window_len) == offsetof(thm_gzip_state, window_len) &&
                  offsetof(gz::State, member_len) == offsetof(thm_gzip_state, member_len) &&
                  offsetof(gz::State, stream_offset) == offsetof(thm_gzip_state, stream_offset),
              "gz::State is thm_gzip_state");

namespace {

// The inflate of bytes[0, n), n > 0, in chunks of `chunk` on the stream, and one synchronisation: *sum; with status 0
// the bytes stand in fq.raw behind head_len and the outgoing state in gz.h_state.  fq.raw is sized here.
int inflate_on_device(thm_aligner* a, const thm_gzip_state* st, const uint8_t* bytes, uint64_t n, uint32_t chunk, bool last_block,
                      uint64_t head_len, gz::Summary* sum) {
  hipStream_t s = a->stream;
  gz::Job j;
  memset(&j, 0, sizeof j);
  j.n = n, j.chunk_bytes = chunk, j.n_chunks = (uint32_t)((n + chunk - 1) / chunk), j.last_block = last_block ? 1 : 0;
  const uint64_t nc = j.n_chunks, ne = nc * gz::ENDS_PER_CHUNK;
  j.out_cap = nc * gz::region_syms(j);
  HIPCHK(a, ensure_events(a->gz.ev));
  HIPCHK(a, a->fq.raw.ensure(head_len + j.out_cap + 64));
  HIPCHK(a, a->gz.in.ensure(n, 64));
  HIPCHK(a, a->gz.state.ensure(2));
  HIPCHK(a, a->gz.cand.ensure(nc));
  HIPCHK(a, a->gz.runs.ensure(nc));
  HIPCHK(a, a->gz.ends.ensure(ne));
  HIPCHK(a, a->gz.syms.ensure(j.out_cap));
  HIPCHK(a, a->gz.windows.ensure(nc * gz::WINDOW));
  HIPCHK(a, a->gz.run_list.ensure(nc));
  HIPCHK(a, a->gz.run_off.ensure(nc + 1));
  HIPCHK(a, a->gz.end_abs.ensure(ne));
  HIPCHK(a, a->gz.end_crc.ensure(ne));
  HIPCHK(a, a->gz.end_isize.ensure(ne));
  HIPCHK(a, a->gz.member_crc.ensure(ne + 1));
  HIPCHK(a, a->gz.sum.ensure(1));
  HIPCHK(a, a->gz.h_sum.ensure(1));
  HIPCHK(a, a->gz.h_state.ensure(1));
  j.in = a->gz.in;
  j.st_in = a->gz.state;
  j.st_out = a->gz.state + 1;
  j.cand = a->gz.cand, j.runs = a->gz.runs, j.ends = a->gz.ends;
  j.syms = a->gz.syms, j.windows = a->gz.windows;
  j.run_list = a->gz.run_list, j.run_off = a->gz.run_off;
  j.end_abs = a->gz.end_abs, j.end_crc = a->gz.end_crc, j.end_isize = a->gz.end_isize;
  j.member_crc = a->gz.member_crc;
  j.out = a->fq.raw.as<uint8_t>() + head_len;
  j.sum = a->gz.sum;
  HIPCHK(a, hipMemcpyAsync(a->gz.in, bytes, n, hipMemcpyHostToDevice, s));
  HIPCHK(a, hipMemcpyAsync(a->gz.state, st, sizeof(gz::State), hipMemcpyHostToDevice, s));
  HIPCHK(a, hipMemsetAsync(j.st_out, 0, sizeof(gz::State), s));
  HIPCHK(a, hipMemsetAsync(a->gz.member_crc, 0, (ne + 1) * 4, s));
  HIPCHK(a, hipMemsetAsync(a->gz.sum, 0xFF, sizeof(gz::Summary), s));  // (a status no kernel wrote is not 0)
  HIPCHK(a, hipEventRecord(a->gz.ev[0], s));
  HIPCHK(a, launch_gzip_inflate(j, s));
  HIPCHK(a, hipEventRecord(a->gz.ev[1], s));
  HIPCHK(a, hipMemcpyAsync(a->gz.h_sum, a->gz.sum, sizeof(gz::Summary), hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipMemcpyAsync(a->gz.h_state, j.st_out, sizeof(gz::State), hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipStreamSynchronize(s));
  *sum = *a->gz.h_sum;
  if (sum->status == gz::OK && (sum->n_out > j.out_cap || sum->n_consumed > n))
    return fail(a, THM_ERR_INTERNAL, "device gzip inflate: a summary larger than its input");
  return THM_OK;
}

// compressed bytes per chunk: gz::DEFAULT_CHUNK, or THM_GZIP_CHUNK_KB (read once per process; a tuning aid)
uint32_t chunk_bytes() {
  static const uint32_t v = [] {
    const char* e = getenv("THM_GZIP_CHUNK_KB");
    const long kb = e ? atol(e) : 0;
    return kb >= 1 && kb <= 1024 ? (uint32_t)kb << 10 : gz::DEFAULT_CHUNK;
  }();
  return v;
}

bool state_ok(const thm_gzip_state* st) { return gz::state_consistent(*reinterpret_cast<const gz::State*>(st)); }  // (the assert above)

}  // namespace

extern "C" {

int32_t thm_batch_upload_fastq_gzip(thm_aligner* a, thm_gzip_state* st, const uint8_t* head, uint64_t head_len, const uint8_t* bytes,
                                    uint64_t n, const char* path, uint64_t first_line, int32_t last_block, thm_fastq_gzip_info* info) {
  if (!a || !st || !info || (!bytes && n) || (!head && head_len)) return THM_ERR_INVALID_ARG;
  memset(info, 0, sizeof(*info));
  if (!state_ok(st)) return fail(a, THM_ERR_INVALID_ARG, "thm_batch_upload_fastq_gzip: the fields of the state contradict each other");
  HIPCHK(a, hipSetDevice(a->device));
  hipStream_t s = a->stream;
  a->uploaded = a->ran = a->synced = false;
  a->bam.reads_named = false;
  const std::string name = path ? path : "";
  HArr<uint8_t>& tail = a->fz.tail.next();  // (the other one may be this call's head)
  // the state this call leaves, handed over once nothing can fail any more
  std::unique_ptr<thm_gzip_state> next(new thm_gzip_state(*st));
  // ---- the block into fq.raw: inflated there, or inflated here and copied
  bool on_device = n != 0 && n <= gz::MAX_IN;
  if (n > gz::MAX_IN) info->decline_reason = gz::INPUT;
  uint64_t blk_n = head_len, consumed = 0;
  const uint8_t* host_blk = nullptr;  // the block on the host, once it is there
  int d = FQ_NO_RECORD;
  FastqOutcome o;
  if (on_device) {
    gz::Summary sum;
    const int rc = inflate_on_device(a, st, bytes, n, chunk_bytes(), last_block != 0, head_len, &sum);
    if (rc != THM_OK) return rc;
    info->n_chunks = (n + chunk_bytes() - 1) / chunk_bytes();
    info->n_starts = sum.n_starts;
    if (sum.status != gz::OK) {
      info->decline_reason = sum.status;
      on_device = false;
    } else {
      blk_n = head_len + sum.n_out;
      consumed = sum.n_consumed;
      memcpy(next.get(), a->gz.h_state, sizeof(thm_gzip_state));
      a->gz.counts[0]++;
      info->inflated_on_device = 1;
      (void)elapsed_ms(a->gz.ev[0], a->gz.ev[1], &info->inflate_ms);
      if (sum.n_out == 0) {  // nothing new: the block is the head, which the host has
        a->fz.block.assign(head, head + head_len);
        host_blk = a->fz.block.data();
      } else {
        if (head_len) HIPCHK(a, hipMemcpyAsync(a->fq.raw.p, head, head_len, hipMemcpyHostToDevice, s));  // (in front of the inflated bytes)
        FastqBlock b;
        b.n = blk_n;
        b.whole = last_block != 0;
        b.tail = &tail;
        d = parse_resident(a, b);
        if (d < 0) return d;
        if (d == 1) {
          o.take(b);
        } else {  // the parse is the host's: the inflated bytes come down, they are not inflated again
          a->fz.block.resize(blk_n);
          HIPCHK(a, hipMemcpyAsync(a->fz.block.data(), a->fq.raw.p, blk_n, hipMemcpyDeviceToHost, s));
          HIPCHK(a, hipStreamSynchronize(s));
          host_blk = a->fz.block.data();
        }
      }
    }
  }
  if (!on_device) {
    a->fz.block.assign(head, head + head_len);
    const int rc = GzInflater::inflate_slice(next.get(), bytes, (size_t)n, name, last_block != 0, a->fz.block, &consumed, a->err);
    if (rc != THM_OK) {
      set_global_error(a->err);
      return rc;
    }
    if (n) a->gz.counts[1]++;
    blk_n = a->fz.block.size();
    host_blk = a->fz.block.data();
    if (blk_n > head_len && (d = parse_host_block(a, host_blk, blk_n, last_block != 0, &tail, o)) < 0) return d;
  }
  info->n_inflated_bytes = blk_n - head_len;
  info->n_consumed_bytes = consumed;
  if (d == 1) {
    batch_parsed_on_device(a, &tail, o);
    a->gz.counts[2]++;
  } else {
    const int rc = host_parser_batch(a, host_blk, blk_n, name, first_line, last_block != 0, &tail, &a->gz.counts[3], o);
    if (rc != THM_OK) return rc;
  }
  info->n_reads = o.n_reads, info->n_bases = o.n_bases, info->n_name_bytes = o.n_name_bytes;
  info->n_lines = o.n_lines;
  info->tail = o.tail, info->tail_len = o.tail_len;
  info->parsed_on_device = o.parsed_on_device;
  info->parse_ms = o.parse_ms;
  *st = *next;
  return THM_OK;
}

// test hook: the device inflate alone, with no host inflater behind it and in chunks of chunk_bytes (64 or more; 0: the
// default) -- a summary with a status word other than 0 is THM_ERR_UNSUPPORTED (the message names the word and the
// chunk).  *n_out bytes land in out[0, cap), *st moves on, *n_consumed as info->n_consumed_bytes.  counts, when not
// null: n_chunks, n_starts, starts the chain refused, the path flags (G_ of gzip_device.h).
int32_t thm_debug_gzip_inflate(thm_aligner* a, thm_gzip_state* st, const uint8_t* bytes, uint64_t n, uint32_t chunk_bytes, int32_t last_block,
                               uint8_t* out, uint64_t cap, uint64_t* n_out, uint64_t* n_consumed, uint64_t* counts) {
  if (!a || !st || (!bytes && n) || !out || !n_out || !n_consumed) return THM_ERR_INVALID_ARG;
  if (chunk_bytes == 0) chunk_bytes = gz::DEFAULT_CHUNK;
  if (chunk_bytes < gz::MIN_CHUNK || !state_ok(st)) return THM_ERR_INVALID_ARG;
  *n_out = *n_consumed = 0;
  HIPCHK(a, hipSetDevice(a->device));
  if (n == 0) return last_block && st->in_member ? fail(a, THM_ERR_UNSUPPORTED, "thm_debug_gzip_inflate: declined with status %u", gz::TRUNCATED) : THM_OK;
  if (n > gz::MAX_IN) return fail(a, THM_ERR_UNSUPPORTED, "thm_debug_gzip_inflate: declined with status %u", gz::INPUT);
  gz::Summary sum;
  const int rc = inflate_on_device(a, st, bytes, n, chunk_bytes, last_block != 0, 0, &sum);
  if (rc != THM_OK) return rc;
  if (counts) counts[0] = (n + chunk_bytes - 1) / chunk_bytes, counts[1] = sum.n_starts, counts[2] = sum.n_refused, counts[3] = sum.flags;
  if (sum.status != gz::OK)
    return fail(a, THM_ERR_UNSUPPORTED, "thm_debug_gzip_inflate: declined with status %u at chunk %u", sum.status, sum.bad_chunk);
  if (sum.n_out > cap)
    return fail(a, THM_ERR_INVALID_ARG, "thm_debug_gzip_inflate: %llu bytes do not fit into %llu", (unsigned long long)sum.n_out, (unsigned long long)cap);
  if (sum.n_out) HIPCHK(a, hipMemcpy(out, a->fq.raw.p, sum.n_out, hipMemcpyDeviceToHost));
  memcpy(st, a->gz.h_state, sizeof(thm_gzip_state));
  *n_out = sum.n_out;
  *n_consumed = sum.n_consumed;
  return THM_OK;
}

// test hook: what thm_batch_upload_fastq_gzip did since the aligner was created -- counts[0..3] = inflates on the
// device, on the host, batches parsed on the device, parsed on the host (a batch without a record is neither)
int32_t thm_debug_fastq_gzip_blocks(thm_aligner* a, uint64_t* counts) {
  if (!a || !counts) return THM_ERR_INVALID_ARG;
  for (int k = 0; k < 4; k++) counts[k] = a->gz.counts[k];
  return THM_OK;
}

}  // extern "C"
