// inflate.hip -- host side of thm_batch_upload_fastq_bgzf (include/thermite_io.h): a block of
// .fastq.gz input goes up compressed.  The host only walks the chain of BGZF members, header to header, into a table
// (inflate_device.h); kernels_inflate.hip inflates every member to its place in fq.raw, behind the head the caller hands
// in, and the device FASTQ parser (fastq.hip, parse_resident) runs on the block where it stands.  What the device does
// not take -- a chain that is not BGZF throughout, a member that ends with a status word -- is inflated by GzInflater
// (io_inflate.cpp) from memory, as a whole: the bytes, or the error and its message, are the host inflater's on every
// input.  The statuses ride on the parse's first synchronisation, the tail on its last: the call synchronises the
// stream as often as thm_batch_upload_fastq does.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "aligner_internal.h"
#include "fastq_cut.h"
#include "inflate_device.h"
#include "io_internal.h"
#include "launch_io.h"

using namespace thm;

namespace {

// the chain members[0, n) as a table, outputs placed from `out_off` on; false: not BGZF throughout
bool walk_chain(const uint8_t* members, uint64_t n, uint64_t out_off, std::vector<inf::Member>& tab, uint64_t* total) {
  tab.clear();
  uint64_t at = 0, sum = 0;
  while (at < n) {
    inf::Member m;
    uint64_t size = 0;
    if (!inf::walk_member(members, n, at, out_off + sum, &m, &size)) return false;
    tab.push_back(m);
    at += size;
    sum += m.isize;
  }
  *total = sum;
  return true;
}

// members and table up, the kernel on the stream: member k's bytes land at fq.raw + tab[k].out_off, its status word in
// fz.status[k].  fq.raw must hold n_out bytes.  Nothing is synchronised.
int enqueue_inflate(thm_aligner* a, const uint8_t* members, uint64_t n, const std::vector<inf::Member>& tab, uint64_t n_out) {
  hipStream_t s = a->stream;
  const uint64_t nm = tab.size();
  HIPCHK(a, ensure_events(a->fz.ev));
  HIPCHK(a, a->fz.in.ensure(n, 64));
  HIPCHK(a, a->fz.tab.ensure(nm));
  HIPCHK(a, a->fz.status.ensure(nm));
  HIPCHK(a, a->fz.h_tab.ensure(nm));
  memcpy(a->fz.h_tab, tab.data(), nm * sizeof(inf::Member));
  HIPCHK(a, hipMemcpyAsync(a->fz.in, members, n, hipMemcpyHostToDevice, s));
  HIPCHK(a, hipMemcpyAsync(a->fz.tab, a->fz.h_tab, nm * sizeof(inf::Member), hipMemcpyHostToDevice, s));
  InflateParams p;
  p.in = a->fz.in;
  p.n_in = n;
  p.members = a->fz.tab;
  p.n_members = nm;
  p.out = a->fq.raw.as<uint8_t>();
  p.n_out = n_out;
  p.status = a->fz.status;
  HIPCHK(a, hipEventRecord(a->fz.ev[0], s));
  HIPCHK(a, launch_bgzf_inflate(p, s));
  HIPCHK(a, hipEventRecord(a->fz.ev[1], s));
  return THM_OK;
}

// head ++ inflate(members) into `blk` by the host inflater, or its THM_ERR_IO with its message in `err`
int inflate_to(std::vector<uint8_t>& blk, const uint8_t* head, uint64_t head_len, const uint8_t* members, uint64_t n,
               const std::string& path, std::string& err) {
  blk.resize(head_len);
  if (head_len) memcpy(blk.data(), head, head_len);
  if (n == 0) return THM_OK;
  GzInflater z;
  z.open_memory(members, n, path);
  constexpr size_t STEP = 1u << 20, WINDOW = 32768;
  size_t total = head_len;
  for (;;) {
    blk.resize(total + STEP);
    const long k = z.read(blk.data() + total, STEP, std::min<size_t>(total - head_len, WINDOW));
    if (k < 0) {
      err = z.error();
      return THM_ERR_IO;
    }
    if (k == 0) break;
    total += (size_t)k;
  }
  blk.resize(total);
  return THM_OK;
}
int inflate_on_host(thm_aligner* a, const uint8_t* head, uint64_t head_len, const uint8_t* members, uint64_t n, const std::string& path) {
  const int rc = inflate_to(a->fz.block, head, head_len, members, n, path, a->err);
  if (rc != THM_OK) set_global_error(a->err);
  return rc;
}

}  // namespace

int thm::bgzf_block_on_host(const uint8_t* head, uint64_t head_len, const uint8_t* members, uint64_t n, const std::string& path,
                            bool last_block, std::vector<uint8_t>& block, uint64_t* cut, std::string& err) {
  const int rc = inflate_to(block, head, head_len, members, n, path, err);
  if (rc != THM_OK) return rc;
  uint64_t n_lines = 0;
  *cut = last_block || block.empty() ? block.size() : fastq_host_cut(block.data(), block.size(), &n_lines);
  return THM_OK;
}

extern "C" {

int32_t thm_batch_upload_fastq_bgzf(thm_aligner* a, const uint8_t* head, uint64_t head_len, const uint8_t* members, uint64_t n,
                                    const char* path, uint64_t first_line, int32_t last_block, thm_fastq_bgzf_info* info) {
  if (!a || !info || (!members && n) || (!head && head_len)) return THM_ERR_INVALID_ARG;
  memset(info, 0, sizeof(*info));
  HIPCHK(a, hipSetDevice(a->device));
  hipStream_t s = a->stream;
  a->uploaded = a->ran = a->synced = false;
  a->bam.reads_named = false;
  const std::string name = path ? path : "";
  HArr<uint8_t>& tail = a->fz.tail.next();  // (the other one may be this call's head)
  // ---- the block into fq.raw: inflated there, or inflated here and copied
  std::vector<inf::Member> tab;
  uint64_t total = 0;
  bool on_device = n != 0 && walk_chain(members, n, head_len, tab, &total);
  info->n_members = on_device ? tab.size() : 0;
  uint64_t blk_n = head_len + total;
  const uint8_t* host_blk = nullptr;  // the block on the host, once it is there
  int d = FQ_NOT_INFLATED;
  FastqOutcome o;
  if (on_device) {
    HIPCHK(a, a->fq.raw.ensure(blk_n + 64));
    if (head_len) HIPCHK(a, hipMemcpyAsync(a->fq.raw.p, head, head_len, hipMemcpyHostToDevice, s));
    int rc = enqueue_inflate(a, members, n, tab, blk_n);
    if (rc != THM_OK) return rc;
    if (blk_n == 0) {  // (members of no bytes, no head: only the statuses are of interest)
      HIPCHK(a, a->fz.h_status.ensure(tab.size()));
      HIPCHK(a, hipMemcpyAsync(a->fz.h_status, a->fz.status, tab.size() * 4, hipMemcpyDeviceToHost, s));
      HIPCHK(a, hipStreamSynchronize(s));
      d = FQ_NO_RECORD;
      for (size_t k = 0; k < tab.size(); k++)
        if (a->fz.h_status[k] != 0) d = FQ_NOT_INFLATED;
    } else {
      FastqBlock b;
      b.n = blk_n;
      b.whole = last_block != 0;
      b.d_status = a->fz.status;
      b.n_status = tab.size();
      b.tail = &tail;
      d = parse_resident(a, b);
      if (d < 0) return d;
      if (d == 1) o.take(b);
    }
    on_device = d != FQ_NOT_INFLATED;
  }
  if (on_device) {
    a->fz.counts[0]++;
    info->inflated_on_device = 1;
    (void)elapsed_ms(a->fz.ev[0], a->fz.ev[1], &info->inflate_ms);
    if (d != 1 && blk_n) {  // the parse is the host's: the inflated bytes come down, they are not inflated again
      a->fz.block.resize(blk_n);
      HIPCHK(a, hipMemcpyAsync(a->fz.block.data(), a->fq.raw.p, blk_n, hipMemcpyDeviceToHost, s));
      HIPCHK(a, hipStreamSynchronize(s));
      host_blk = a->fz.block.data();
    }
  } else {
    const int rc = inflate_on_host(a, head, head_len, members, n, name);
    if (rc != THM_OK) return rc;
    if (n) a->fz.counts[1]++;
    blk_n = a->fz.block.size();
    host_blk = a->fz.block.data();
    d = FQ_NO_RECORD;
    if (blk_n && (d = parse_host_block(a, host_blk, blk_n, last_block != 0, &tail, o)) < 0) return d;
  }
  info->n_inflated_bytes = blk_n - head_len;
  if (d == 1) {
    batch_parsed_on_device(a, &tail, o);
    a->fz.counts[2]++;
  } else {
    const int rc = host_parser_batch(a, host_blk, blk_n, name, first_line, last_block != 0, &tail, &a->fz.counts[3], o);
    if (rc != THM_OK) return rc;
  }
  info->n_reads = o.n_reads, info->n_bases = o.n_bases, info->n_name_bytes = o.n_name_bytes;
  info->n_lines = o.n_lines;
  info->tail = o.tail, info->tail_len = o.tail_len;
  info->parsed_on_device = o.parsed_on_device;
  info->parse_ms = o.parse_ms;
  return THM_OK;
}

// test hook: the device inflate alone, with no host inflater behind it -- a chain that is not BGZF throughout and a
// member that ends with a status word are THM_ERR_UNSUPPORTED (the message names the member and the word).  *n_out bytes
// land in out[0, cap).
int32_t thm_debug_bgzf_inflate(thm_aligner* a, const uint8_t* members, uint64_t n, uint8_t* out, uint64_t cap, uint64_t* n_out) {
  if (!a || (!members && n) || !out || !n_out) return THM_ERR_INVALID_ARG;
  *n_out = 0;
  HIPCHK(a, hipSetDevice(a->device));
  std::vector<inf::Member> tab;
  uint64_t total = 0;
  if (!walk_chain(members, n, 0, tab, &total)) return fail(a, THM_ERR_UNSUPPORTED, "thm_debug_bgzf_inflate: the chain is not BGZF throughout");
  if (total > cap) return fail(a, THM_ERR_INVALID_ARG, "thm_debug_bgzf_inflate: %llu bytes do not fit into %llu", (unsigned long long)total, (unsigned long long)cap);
  if (tab.empty()) return THM_OK;
  HIPCHK(a, a->fq.raw.ensure(total + 64));
  const int rc = enqueue_inflate(a, members, n, tab, total);
  if (rc != THM_OK) return rc;
  HIPCHK(a, a->fz.h_status.ensure(tab.size()));
  HIPCHK(a, hipMemcpyAsync(a->fz.h_status, a->fz.status, tab.size() * 4, hipMemcpyDeviceToHost, a->stream));
  HIPCHK(a, hipStreamSynchronize(a->stream));
  for (size_t k = 0; k < tab.size(); k++)
    if (const uint32_t st = a->fz.h_status[k])
      return fail(a, THM_ERR_UNSUPPORTED, "thm_debug_bgzf_inflate: member %llu declined with status %u", (unsigned long long)k, st);
  if (total) HIPCHK(a, hipMemcpy(out, a->fq.raw.p, total, hipMemcpyDeviceToHost));
  *n_out = total;
  return THM_OK;
}

// test hook: what thm_batch_upload_fastq_bgzf did since the aligner was created -- counts[0..3] = blocks inflated on
// the device, inflated on the host, batches parsed on the device, parsed on the host (a batch without a record is neither)
int32_t thm_debug_fastq_bgzf_blocks(thm_aligner* a, uint64_t* counts) {
  if (!a || !counts) return THM_ERR_INVALID_ARG;
  for (int k = 0; k < 4; k++) counts[k] = a->fz.counts[k];
  return THM_OK;
}

}  // extern "C"
