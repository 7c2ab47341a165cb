// fastq.hip -- host side of thm_batch_upload_fastq / thm_batch_fetch_reads (include/thermite_io.h): a block of whole
// FASTQ records goes up as the bytes it is, and kernels_fastq.hip cuts it into names, bases and qualities where
// thm_batch_upload_reads would have placed them.  The device takes the strict form only (fastq_device.h); a block it
// declines is parsed by fastq_parse_block (io_fastq.cpp) and uploaded the old way, or is that parser's error: what the
// call does is the host parser's doing on every input.  The kernels run on the block where it stands in fq.raw
// (parse_resident), so that a block the device inflated there (inflate.hip, thm_batch_upload_fastq_bgzf) takes the same
// path as one that was copied up.
#include <hip/hip_runtime.h>

#include <cstring>

#include "aligner_internal.h"
#include "fastq_cut.h"
#include "fastq_device.h"
#include "io_internal.h"
#include "launch_io.h"

using namespace thm;

// The parse of a block that stands in fq.raw (FastqBlock, aligner_internal.h): 1: the batch is in place, parsed by the
// device; 0: declined (nothing of the aligner's batch state is valid); < 0: error; FQ_NOT_INFLATED / FQ_NO_RECORD as there
int thm::parse_resident(thm_aligner* a, FastqBlock& b) {
  hipStream_t s = a->stream;
  const uint64_t n = b.n;
  HIPCHK(a, ensure_events(a->fq.ev));
  FastqParams p;
  memset(&p, 0, sizeof p);
  p.n = n;
  p.n_chunks = (n + fq::CHUNK - 1) / fq::CHUNK;
  HIPCHK(a, a->fq.cnt.ensure(p.n_chunks));
  HIPCHK(a, a->fq.base.ensure(p.n_chunks + 2));
  HIPCHK(a, a->fq.flag.ensure(16));
  p.raw = a->fq.raw.as<uint8_t>();
  p.chunk_cnt = a->fq.cnt;
  p.chunk_base = a->fq.base;
  p.flag = a->fq.flag;
  HIPCHK(a, hipMemsetAsync(a->fq.flag, 0, 64, s));
  // ---- newlines: per chunk, their scan; the total sizes the line table
  HIPCHK(a, hipEventRecord(a->fq.ev[0], s));
  HIPCHK(a, launch_fastq_count(p, a->n_cu, s));
  if (const int rc = scan_u64(a, a->stage_scan_tmp, a->fq.cnt, a->fq.base, p.n_chunks, s); rc != THM_OK) return rc;
  HIPCHK(a, hipEventRecord(a->fq.ev[1], s));
  unsigned long long n_nl = 0;
  HIPCHK(a, hipMemcpyAsync(&n_nl, a->fq.base + p.n_chunks, 8, hipMemcpyDeviceToHost, s));
  // a block the host has not seen: its last byte, and the words its inflate left, come down with the total
  if (!b.host) {
    HIPCHK(a, a->fz.h_last.ensure(64));
    HIPCHK(a, hipMemcpyAsync(a->fz.h_last, a->fq.raw.as<uint8_t>() + n - 1, 1, hipMemcpyDeviceToHost, s));
  }
  if (b.n_status) {
    HIPCHK(a, a->fz.h_status.ensure(b.n_status));
    HIPCHK(a, hipMemcpyAsync(a->fz.h_status, b.d_status, b.n_status * 4, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(a, hipStreamSynchronize(s));
  for (uint64_t k = 0; k < b.n_status; k++)
    if (a->fz.h_status[k] != 0) {
      b.bad_member = k;
      return FQ_NOT_INFLATED;
    }
  if (n_nl > n) return fail(a, THM_ERR_INTERNAL, "device FASTQ parse: more newlines than bytes");
  p.n_newlines = n_nl;
  b.n_newlines = n_nl;
  b.cut = n;
  if (b.whole) {
    p.n_lines = fq::line_count(n_nl, b.host ? b.host[n - 1] : a->fz.h_last[0]);
    if (p.n_lines % 4 != 0) return 0;
  } else {
    p.n_lines = 4 * (n_nl / 4);
    if (p.n_lines == 0) return FQ_NO_RECORD;
  }
  const uint64_t nr = p.n_records = p.n_lines / 4;
  if (nr >= 0xFFFFFFF0ull) return 0;  // (the host path words the refusal)
  // ---- line starts, the rule per record, name_off and offsets
  HIPCHK(a, a->fq.lines.ensure((p.n_lines > n_nl ? p.n_lines : n_nl) + 2));
  HIPCHK(a, a->fq.name_len.ensure(nr + 1));
  HIPCHK(a, a->fq.seq_len.ensure(nr + 1));
  HIPCHK(a, a->bam.name_off.ensure(nr + 1));
  HIPCHK(a, a->reads.offsets.ensure(nr + 1));
  HIPCHK(a, a->fq.h_off.ensure(nr + 3));
  p.line_start = a->fq.lines;
  p.name_len = a->fq.name_len;
  p.seq_len = a->fq.seq_len;
  p.name_off = a->bam.name_off;
  p.offsets = a->reads.offsets;
  HIPCHK(a, hipEventRecord(a->fq.ev[2], s));
  HIPCHK(a, launch_fastq_starts(p, a->n_cu, s));
  HIPCHK(a, launch_fastq_records(p, s));
  int rc = scan_u64(a, a->stage_scan_tmp, p.name_len, a->bam.name_off, nr, s);
  if (rc == THM_OK) rc = scan_u64(a, a->stage_scan_tmp, p.seq_len, a->reads.offsets, nr, s);
  if (rc != THM_OK) return rc;
  HIPCHK(a, hipEventRecord(a->fq.ev[3], s));
  // the offsets come down for the length classes (8 bytes a read); the name bytes' total behind them, and behind that
  // the cut of a block that is not the whole batch: where the line behind the batch's last begins
  unsigned flag = 0;
  uint64_t* h_off = a->fq.h_off;
  HIPCHK(a, hipMemcpyAsync(&flag, a->fq.flag, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipMemcpyAsync(h_off, a->reads.offsets, (nr + 1) * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipMemcpyAsync(h_off + nr + 1, a->bam.name_off + nr, 8, hipMemcpyDeviceToHost, s));
  if (!b.whole) HIPCHK(a, hipMemcpyAsync(h_off + nr + 2, p.line_start + p.n_lines, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipStreamSynchronize(s));
  if (flag == 2) return fail(a, THM_ERR_INTERNAL, "device FASTQ parse: inconsistent line table");
  if (!b.whole) {
    if (h_off[nr + 2] > n) return fail(a, THM_ERR_INTERNAL, "device FASTQ parse: a cut behind the block");
    b.cut = h_off[nr + 2];
  }
  if (flag != 0) return 0;
  const uint64_t nb = h_off[nr], nn = h_off[nr + 1];
  if (nn + 2 * nb > b.cut) return fail(a, THM_ERR_INTERNAL, "device FASTQ parse: a parse larger than its block");
  rc = batch_length_classes(a, h_off, nr);
  if (rc != THM_OK) return rc;
  // ---- gather, into the buffers (and with the paddings) of thm_batch_upload / thm_batch_upload_reads
  HIPCHK(a, a->reads.bases.ensure(nb, 64));
  HIPCHK(a, a->bam.names.ensure(nn, 16));
  HIPCHK(a, a->bam.quals.ensure(nb, 16));
  p.names = a->bam.names;
  p.bases = a->reads.bases;
  p.quals = a->bam.quals;
  HIPCHK(a, hipEventRecord(a->fq.ev[4], s));
  HIPCHK(a, launch_fastq_gather(p, a->n_cu, s));
  HIPCHK(a, hipEventRecord(a->fq.ev[5], s));
  if (b.tail && n > b.cut) {
    HIPCHK(a, b.tail->ensure(n - b.cut));
    HIPCHK(a, hipMemcpyAsync(*b.tail, a->fq.raw.as<uint8_t>() + b.cut, n - b.cut, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(a, hipStreamSynchronize(s));
  float ms = 0, sum = 0;
  for (int k = 0; k < 6; k += 2)
    if (hipEventElapsedTime(&ms, a->fq.ev[k], a->fq.ev[k + 1]) == hipSuccess) sum += ms;
  b.n_reads = nr;
  b.n_bases = nb;
  b.n_name_bytes = nn;
  b.ms = sum;
  return 1;
}

// ---- the finish of the three upload entry points (aligner_internal.h)
int thm::parse_host_block(thm_aligner* a, const uint8_t* blk, uint64_t n, bool whole, HArr<uint8_t>* tail, FastqOutcome& o) {
  HIPCHK(a, a->fq.raw.ensure(n + 64));
  HIPCHK(a, hipMemcpyAsync(a->fq.raw.p, blk, n, hipMemcpyHostToDevice, a->stream));
  FastqBlock b;
  b.n = n;
  b.host = blk;
  b.whole = whole;
  const int d = parse_resident(a, b);
  if (d != 1) return d;
  o.take(b);
  if (tail && o.tail_len) {
    HIPCHK(a, tail->ensure(o.tail_len));
    memcpy(*tail, blk + b.cut, o.tail_len);
  }
  return 1;
}

void thm::batch_parsed_on_device(thm_aligner* a, HArr<uint8_t>* tail, FastqOutcome& o) {
  a->bam.reads_have_quals = true;
  a->bam.reads_named = true;
  a->uploaded = true;
  o.parsed_on_device = 1;
  o.tail = tail && o.tail_len ? tail->get() : nullptr;
}

int thm::host_parser_batch(thm_aligner* a, const uint8_t* blk, uint64_t n, const std::string& path, uint64_t first_line, bool last_block,
                           HArr<uint8_t>* tail, uint64_t* on_host, FastqOutcome& o) {
  // (a batch without a record included: nothing is counted as parsed then)
  uint64_t cut = n, n_lines = 0;
  if (tail && !last_block) cut = n ? fastq_host_cut(blk, n, &n_lines) : 0;
  if (cut) ++*on_host;
  HostBatch hb;
  std::string err;
  const int rc = fastq_parse_block((const char*)blk, (size_t)cut, path, first_line, last_block, hb, err);
  if (rc != THM_OK) {
    a->err = err;
    set_global_error(err);
    return rc;
  }
  const thm_read_batch v = hb.view();
  const int urc = thm_batch_upload_reads(a, &v);
  if (urc != THM_OK) return urc;
  o.n_reads = v.n_reads;
  o.n_bases = v.n_bases;
  o.n_name_bytes = v.name_off[v.n_reads];
  if (tail && last_block) {  // every line of the block, counted as fq::line_count counts them
    for (uint64_t i = 0; i < n; i++) n_lines += blk[i] == (uint8_t)'\n';
    if (n && blk[n - 1] != (uint8_t)'\n') n_lines++;
  }
  o.n_lines = n_lines;
  o.tail_len = n - cut;
  if (o.tail_len) {
    HIPCHK(a, tail->ensure(o.tail_len));
    memcpy(*tail, blk + cut, o.tail_len);
    o.tail = *tail;
  }
  return THM_OK;
}

extern "C" {

int32_t thm_batch_upload_fastq(thm_aligner* a, const uint8_t* raw, uint64_t n, const char* path, uint64_t first_line,
                               int32_t last_block, thm_fastq_upload_info* info) {
  if (!a || !info || (!raw && n)) return THM_ERR_INVALID_ARG;
  memset(info, 0, sizeof(*info));
  HIPCHK(a, hipSetDevice(a->device));
  a->uploaded = a->ran = a->synced = false;
  a->bam.reads_named = false;
  FastqOutcome o;
  int d = 0;
  if (n) {  // the block goes up as it is and is parsed where it stands
    d = parse_host_block(a, raw, n, true, nullptr, o);
    if (d < 0) return d;
  }
  if (d == 1) {
    batch_parsed_on_device(a, nullptr, o);
    a->fq.on_device++;
  } else {  // not device-parsable (or empty): the host parser's batch, or its error with its message
    const int rc = host_parser_batch(a, raw, n, path ? path : "", first_line, last_block != 0, nullptr, &a->fq.on_host, o);
    if (rc != THM_OK) return rc;
  }
  info->n_reads = o.n_reads;
  info->n_bases = o.n_bases;
  info->n_name_bytes = o.n_name_bytes;
  info->on_device = o.parsed_on_device;
  info->device_ms = o.parse_ms;
  return THM_OK;
}

int32_t thm_batch_fetch_reads(thm_aligner* a, thm_read_batch* out) {
  if (!a || !out) return THM_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  if (!a->uploaded || !a->bam.reads_named)
    return fail(a, THM_ERR_INVALID_ARG, "thm_batch_fetch_reads: no batch with names is uploaded (thm_batch_upload_reads / thm_batch_upload_fastq)");
  HIPCHK(a, hipSetDevice(a->device));
  hipStream_t s = a->stream;
  const uint64_t n = a->n_reads, nb = a->n_bases;
  HIPCHK(a, a->fq.back.off.ensure(n + 1));
  HIPCHK(a, a->fq.back.name_off.ensure(n + 1));
  HIPCHK(a, hipMemcpyAsync(a->fq.back.off, a->reads.offsets, (n + 1) * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipMemcpyAsync(a->fq.back.name_off, a->bam.name_off, (n + 1) * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipStreamSynchronize(s));
  const uint64_t nn = a->fq.back.name_off[n];
  HIPCHK(a, a->fq.back.bases.ensure(nb + 1));
  HIPCHK(a, a->fq.back.names.ensure(nn + 1));
  if (nb) HIPCHK(a, hipMemcpyAsync(a->fq.back.bases, a->reads.bases, nb, hipMemcpyDeviceToHost, s));
  if (nn) HIPCHK(a, hipMemcpyAsync(a->fq.back.names, a->bam.names, nn, hipMemcpyDeviceToHost, s));
  if (a->bam.reads_have_quals) {
    HIPCHK(a, a->fq.back.quals.ensure(nb + 1));
    if (nb) HIPCHK(a, hipMemcpyAsync(a->fq.back.quals, a->bam.quals, nb, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(a, hipStreamSynchronize(s));
  out->n_reads = n;
  out->n_bases = nb;
  out->bases = a->fq.back.bases;
  out->offsets = a->fq.back.off;
  out->quals = a->bam.reads_have_quals ? a->fq.back.quals : nullptr;
  out->names = a->fq.back.names;
  out->name_off = a->fq.back.name_off;
  return THM_OK;
}

// test hook: the blocks thm_batch_upload_fastq parsed on the device / handed to the host parser since the aligner was created
int32_t thm_debug_fastq_device_blocks(thm_aligner* a, uint64_t* on_device, uint64_t* on_host) {
  if (!a || !on_device || !on_host) return THM_ERR_INVALID_ARG;
  *on_device = a->fq.on_device;
  *on_host = a->fq.on_host;
  return THM_OK;
}

}  // extern "C"
