// io_internal.h -- shared by the host-side I/O sources (not part of the ABI).
#ifndef THERMITE_IO_INTERNAL_H
#define THERMITE_IO_INTERNAL_H
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/thermite_io.h"

namespace thm {

// one batch of records, owned
struct HostBatch {
  std::vector<uint8_t> bases, quals, names;  // raw storage: the first nb / nq / nn bytes are in use
  size_t nb = 0, nq = 0, nn = 0;
  std::vector<uint64_t> offsets, name_off;
  bool has_quals = true;  // false when a record came without qualities (FASTA input)
  uint64_t n_reads() const { return offsets.empty() ? 0 : offsets.size() - 1; }
  void clear() {
    nb = nq = nn = 0;
    offsets.assign(1, 0);
    name_off.assign(1, 0);
    has_quals = true;
  }
  thm_read_batch view() const {
    thm_read_batch v;
    v.n_reads = n_reads();
    v.n_bases = nb;
    v.bases = bases.data();
    v.offsets = offsets.data();
    v.quals = has_quals ? quals.data() : nullptr;
    v.names = names.data();
    v.name_off = name_off.data();
    return v;
  }
};

// up to max_reads further records of the reader into `b` (cleared first)
int fastq_fill(thm_fastq* r, uint64_t max_reads, HostBatch& b);

// Parallel parsing (the whole-file driver): the reader thread only cuts the byte stream into blocks of whole
// 4-line FASTQ records, parser threads turn blocks into batches.
//   fastq_is_plain_fastq   the input starts with '@' (FASTA and anything else take the sequential parser)
//   fastq_next_raw_block   up to max_reads records as raw bytes (`raw` reused; n_lines = 4 x records, except for a
//                          truncated last record, which the block parser reports); 0 lines at the end of the input
//                          (last_block: nothing follows this block)
//   fastq_parse_block      strict 4-line records (CR LF tolerated, empty lines only at the very end of the input,
//                          i.e. at the end of the block for which last_block is set)
bool fastq_is_plain_fastq(thm_fastq* r);
int fastq_next_raw_block(thm_fastq* r, uint64_t max_reads, std::vector<char>& raw, size_t& raw_len, uint64_t& n_lines,
                         uint64_t& first_line, bool& last_block);
int fastq_parse_block(const char* p, size_t n, const std::string& path, uint64_t first_line, bool last_block, HostBatch& b,
                      std::string& err);
const std::string& fastq_path(const thm_fastq* r);

// gzip input (io_inflate.cpp): a table-driven inflate with CRC-32 / ISIZE checks per member
uint32_t crc32_fast(uint32_t crc, const uint8_t* p, size_t n);
class GzInflater {
 public:
  GzInflater();
  ~GzInflater();
  GzInflater(const GzInflater&) = delete;
  GzInflater& operator=(const GzInflater&) = delete;
  // Takes the descriptor over.  n_threads > 1 and a regular file of some size: the file is mapped and inflated by
  // that many worker threads (io_inflate.cpp, "several threads on one gzip file"); the calling thread only collects.
  void open(int fd, const std::string& path, unsigned n_threads = 1);
  // A memory source in place of a descriptor: the gzip members data[0, n), copied; `path` only words the messages.
  void open_memory(const uint8_t* data, size_t n, const std::string& path);
  // Up to `cap` further bytes of the inflated stream into dst (cap >= 1024; the call stops a few hundred bytes short
  // of cap rather than in the middle of a match).  dst[-history, 0) must hold the `history` bytes that came before
  // (min(bytes so far, 32768) of them: matches reach back there).  0: end of the input; -1: error().
  long read(uint8_t* dst, size_t cap, size_t history);
  const std::string& error() const;
  // A memory source that begins inside a stream: at a block header `bit_offset` bits into data[0], inside a member of
  // which member_len bytes with the CRC-32 `crc` are out already (in_member), or at a member header at data[0];
  // n_members_done members came before.  The first read()'s dst[-history, 0) holds the window.
  void open_memory_at(const uint8_t* data, size_t n, const std::string& path, uint32_t bit_offset, bool in_member, const uint8_t* window,
                      uint32_t crc, uint64_t member_len, uint64_t n_members_done);
  // The host side of thm_batch_upload_fastq_gzip's inflate (include/thermite_io.h has the rule of consumption): the
  // bytes of every unit that ends inside data[0, n) appended to `out`, *st moved on, *n_consumed set.  THM_ERR_IO with
  // the inflater's message in `err` (THM_ERR_INVALID_ARG for a state that is none); *st and `out` are then unchanged.
  static int inflate_slice(thm_gzip_state* st, const uint8_t* data, size_t n, const std::string& path, bool last_block,
                           std::vector<uint8_t>& out, uint64_t* n_consumed, std::string& err);

 private:
  struct Impl;
  struct Par;
  Impl* p_;
  Par* par_ = nullptr;
  bool open_parallel(int fd, const std::string& path, unsigned n_threads);
  long par_read(uint8_t* dst, size_t cap);
  static long serial_read(Impl& s, uint8_t* dst, size_t cap, size_t history);
};

// DEFLATE for the BAM writer's BGZF blocks (io_deflate.cpp): one complete raw DEFLATE stream (a single final block)
// for at most 65280 input bytes; out must hold deflate_block_bound(n) bytes; returns the bytes written
struct DeflateScratch {
  uint32_t tok[0xff00 + 8];
  uint16_t head[1 << 13];
};
size_t deflate_block_bound(size_t n);
size_t deflate_block(const uint8_t* in, size_t n, uint8_t* out, DeflateScratch& sc);

// thm_writer_format_batch without the final concatenation: the text of the batch is
// chunks[0] ++ chunks[1] ++ ... (one chunk per formatting thread, valid until the next call on `w`)
int writer_format_chunks(thm_writer* w, const thm_read_batch* reads, const thm_batch_view* res,
                         std::vector<const std::string*>& chunks);

// thm_writer_wrap_bam without the final concatenation (chunks as above)
int writer_wrap_bam_chunks(thm_writer* w, const thm_bam_view* view, std::vector<const std::string*>& chunks);

// bgzf.hip: thm_batch_fetch_bgzf, which also reports the reads of the batch with at least one alignment (the view
// holds compressed bytes only; the file driver counts them in its statistics); n_aligned_reads may be null
int batch_fetch_bgzf(thm_aligner* a, uint32_t flags, thm_bgzf_view* out, uint64_t* n_aligned_reads);

// bam_sort.hip: thm_bam_sorter_add, which also reports the reads of the batch with at least one alignment (the file
// driver counts them in its statistics); n_aligned_reads may be null
int bam_sorter_add(thm_bam_sorter* s, uint32_t flags, thm_bam_sort_info* info, uint64_t* n_aligned_reads);

// inflate.hip: head ++ inflate(members) by the host inflater into `block` (THM_ERR_IO and `err` as GzInflater words it);
// *cut: bytes of the batch thm_batch_upload_fastq_bgzf takes of it (all of it for a last block)
int bgzf_block_on_host(const uint8_t* head, uint64_t head_len, const uint8_t* members, uint64_t n, const std::string& path,
                       bool last_block, std::vector<uint8_t>& block, uint64_t* cut, std::string& err);

// contig name_id -> index of its @SQ line (the BAM refID), build_sam_header's order (src/aln_writer.rs:256-276);
// `sq`: the lines' (name, length), when asked for
std::vector<int32_t> sq_of_name(const thm_index* ix, std::vector<std::pair<std::string, uint64_t>>* sq);

}  // namespace thm
#endif
