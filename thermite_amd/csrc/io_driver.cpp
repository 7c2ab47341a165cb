// io_driver.cpp -- whole-file driver (include/thermite_io.h): the loop of
// align_reads_from_file, reference src/aligner.rs:22-120, as overlapped stages over
// batches of reads:
//     inflate one thread per gzip input file, a few files at a time: gzip bytes -> blocks of whole FASTQ
//             records, ahead of the file's turn within a memory budget (the records still leave in input order)
//     cut     one thread: mapped file bytes / the inflaters' blocks -> slots, in input order
//     parse   a few threads: block -> batch (names, bases, qualities); with THM_FASTQ_DEVICE=1 the block passes through
//             and the device parses it (thm_batch_upload_fastq)
//             THM_FASTQ_DEVICE=2: a .fastq.gz that is BGZF throughout is not inflated here at all -- the cutter walks its
//             member chain over the mapping and cuts it into groups of whole members, which go to the device
//             compressed (thm_batch_upload_fastq_bgzf); the tail of one batch is the head of the next, so the uploads
//             of such a run are chained in input order across the GPU threads (runs and fetches still overlap)
//             THM_FASTQ_DEVICE=3: ... and an ordinary .fastq.gz is not inflated here either -- it is mapped and goes to the
//             device in slices (thm_batch_upload_fastq_gzip), each beginning where the last one's blocks ended; that
//             is known at the slice's turn in the same chain only, so the cutter cuts such a file one slot at a time
//     GPU     one thread per aligner (= per GPU): upload, run, sync, fetch
//     write   one thread: batches in input order -> formatting threads -> pwrite
// connected by queues over a fixed set of reusable slots, so that the host work either
// side of the hot path hides behind the GPUs (or the other way round: at tens of millions
// of reads per second per GPU the host side is the bottleneck).
// Records leave in input order whatever the number of GPUs.  The stages are the member functions of Run, below.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <utility>
#include <vector>

#include "cells_device.h"
#include "fastq_cut.h"
#include "inflate_device.h"
#include "io_internal.h"
#include "thermite_internal.h"

namespace {

using Clock = std::chrono::steady_clock;
double secs(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double>(b - a).count(); }

// Runs f.  An exception (bad_alloc from a growing buffer, mostly) must not leave a thread body: std::terminate would
// take the host process down, and a thread that simply stopped would leave the others waiting on its queue.  The
// failure goes to fail(code, message) and comes back as the code; the thread goes on with its hand-over protocol.
template <class F, class E>
int guarded(F&& f, E&& fail) {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    fail(THM_ERR_OOM, "out of host memory in the file driver");
    return THM_ERR_OOM;
  } catch (const std::exception& e) {
    fail(THM_ERR_INTERNAL, std::string("file driver: ") + e.what());
    return THM_ERR_INTERNAL;
  } catch (...) {
    fail(THM_ERR_INTERNAL, "file driver: unknown exception");
    return THM_ERR_INTERNAL;
  }
}

// the status of the run: the first failure stays
struct Shared {
  std::mutex mu;
  int rc = THM_OK;
  std::string msg;
  void set(int code, const std::string& m) {
    std::lock_guard<std::mutex> g(mu);
    if (rc == THM_OK) {
      rc = code;
      msg = m;
    }
  }
  bool failed() {
    std::lock_guard<std::mutex> g(mu);
    return rc != THM_OK;
  }
  // one step of a pipeline thread: its failure becomes the run's status
  template <class F>
  int step(F&& f) {
    return guarded(f, [this](int code, const std::string& m) { set(code, m); });
  }
};

// A file mapped read-only, unmapped when the value dies.  Movable, not copyable.
struct Mapping {
  const uint8_t* p = nullptr;
  size_t len = 0;
  Mapping() = default;
  Mapping(Mapping&& o) noexcept : p(o.p), len(o.len) { o.p = nullptr, o.len = 0; }
  Mapping& operator=(Mapping&& o) noexcept {
    if (this != &o) {
      reset();
      p = o.p, len = o.len;
      o.p = nullptr, o.len = 0;
    }
    return *this;
  }
  Mapping(const Mapping&) = delete;
  Mapping& operator=(const Mapping&) = delete;
  ~Mapping() { reset(); }
  explicit operator bool() const { return p != nullptr; }
  void reset() {
    if (p) munmap((void*)p, len);
    p = nullptr, len = 0;
  }
  bool is_gzip() const { return len >= 2 && p[0] == 0x1f && p[1] == 0x8b; }
  // a regular file of min_len bytes or more; `sequential`: it is read front to back
  static Mapping open(const char* path, size_t min_len, bool sequential) {
    Mapping m;
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0) return m;
    struct stat st;
    if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && (size_t)st.st_size >= min_len && st.st_size > 0) {
      void* q = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
      if (q != MAP_FAILED) {
        m.p = (const uint8_t*)q;
        m.len = (size_t)st.st_size;
        if (sequential) (void)madvise(q, m.len, MADV_SEQUENTIAL);
      }
    }
    close(fd);
    return m;
  }
};

// The first text of a compressed file decides whether it goes to the device compressed: 4-line FASTQ begins with '@'
// (FASTA and anything else keep the inflater thread and its parser).  *bytes_per_read: of that text, where it holds a read.
bool first_text_is_fastq(const std::vector<uint8_t>& first, double* bytes_per_read) {
  if (first.empty() || first[0] != '@') return false;
  size_t nl = 0;
  for (uint8_t c : first) nl += c == '\n';
  if (nl >= 4) *bytes_per_read = (double)first.size() / (double)(nl / 4);
  return true;
}

// A gzip input that is BGZF throughout (THM_FASTQ_DEVICE=2): the mapping and its members.  Eligible: gzip magic, every
// member of the chain with the BGZF header (inflate_device.h, the rule the device takes), the chain ending exactly at the
// end of the file, and the first member, inflated on the host, beginning with '@'.
struct BgzfFile {
  Mapping map;
  std::vector<thm::inf::Member> tab;  // in_off - 12 - xlen is not kept: `at` below is
  std::vector<uint64_t> at;           // first byte of every member, and the file's length behind the last
  double bytes_per_read = 256;        // of the first member's text
  bool open(const char* path) {
    map = Mapping::open(path, 28, false);
    if (!map) return false;
    uint64_t p = 0, out = 0;
    bool good = true;
    while (p < map.len && good) {
      thm::inf::Member mb;
      uint64_t size = 0;
      good = thm::inf::walk_member(map.p, map.len, p, out, &mb, &size);
      if (!good) break;
      tab.push_back(mb);
      at.push_back(p);
      p += size;
      out += mb.isize;
    }
    at.push_back(p);
    std::vector<uint8_t> first;
    std::string err;
    uint64_t cut = 0;
    // the first member with text decides, and it must be the file's first
    const bool ok = good && !tab.empty() && tab[0].isize != 0 &&
                    thm::bgzf_block_on_host(nullptr, 0, map.p, at[1], path, true, first, &cut, err) == THM_OK &&
                    first_text_is_fastq(first, &bytes_per_read);
    if (!ok) map.reset();
    return ok;
  }
};

// A gzip input that is not BGZF throughout (THM_FASTQ_DEVICE=3): the mapping.  Eligible: gzip magic, and the first
// bytes, inflated on the host, beginning with '@'.
struct GzipFile {
  Mapping map;
  double bytes_per_read = 256;  // of the first blocks' text
  bool open(const char* path) {
    map = Mapping::open(path, 18, false);
    if (!map) return false;
    bool ok = false;
    // the first blocks that end inside 64 KiB, or inside 1 MiB
    for (size_t take = 65536; !ok; take *= 16) {
      const size_t n = std::min(take, map.len);
      std::unique_ptr<thm_gzip_state> zs(new thm_gzip_state());
      std::vector<uint8_t> first;
      std::string err;
      uint64_t used = 0;
      if (thm::GzInflater::inflate_slice(zs.get(), map.p, n, path, n == map.len, first, &used, err) != THM_OK) break;
      if (!first.empty()) {
        if (!first_text_is_fastq(first, &bytes_per_read)) break;
        ok = true;
      }
      if (n == map.len || take >= (1u << 20)) break;
    }
    if (!ok) map.reset();
    return ok;
  }
};

// what the fetch step made of a batch, whichever fetch it was
struct Fetched {
  uint64_t n_reads = 0;
  const int32_t* read_status = nullptr;
  uint64_t n_failed_reads = 0;
  uint64_t n_records = 0, n_aligned = 0;  // for the statistics (the host-format paths count them when they format)
  const char* span = nullptr;  // bytes that are written as they are (THM_BAM_DEVICE=2: the members), where there are any
  size_t span_len = 0;
};

struct Slot {
  uint64_t seq = 0;  // position of the batch in the input
  std::vector<char> raw;      // block bytes (gzip input: inflated here) ...
  const char* raw_ptr = nullptr;  // ... or a range of the memory-mapped input file (plain input: no copy)
  size_t raw_len = 0;
  uint64_t first_line = 0;
  bool last_block = false;  // nothing of this input file follows the block (blank lines are tolerated at its end)
  std::string path;
  bool zmembers = false;    // raw_ptr / raw_len are whole BGZF members of the mapped input (THM_FASTQ_DEVICE=2) ...
  bool file_first = false;  // ... the first group of its file: the chain of tails starts empty, at line 1
  bool gzslice = false;     // a slice of the mapped plain-gzip input gz_map[0, gz_len) (THM_FASTQ_DEVICE=3): where it begins and
  const uint8_t* gz_map = nullptr;  // how long it is, is known at its turn in the chain of uploads only (file_first as above)
  size_t gz_len = 0;
  bool parsed = false;  // `reads` already holds the batch (sequential parser: FASTA, odd inputs)
  thm::HostBatch reads;
  thm_batch_view res;  // into the pinned result buffers of the aligner that ran it (two sets per aligner, used alternately)
  thm_bam_view bam;    // ... or, with THM_BAM_DEVICE=1, the BAM records encoded on the device (likewise two sets)
  Fetched got;
  bool aligned = false;
  // A slot is reused across files and modes: every per-batch field starts from here (the buffers keep their memory),
  // and a cut sets only what it means.
  void reset(uint64_t seq_, const char* path_) {
    seq = seq_;
    path = path_;
    raw_ptr = nullptr;
    raw_len = 0;
    first_line = 0;
    last_block = false;
    zmembers = file_first = gzslice = parsed = aligned = false;
    gz_map = nullptr;
    gz_len = 0;
    reads.clear();
    memset(&res, 0, sizeof res);
    memset(&bam, 0, sizeof bam);
    got = Fetched();
  }
};

// A gzip FASTQ file on a thread of its own: inflate, cut into blocks of whole records, queue.  The reference reads its
// query files one after the other (src/aligner.rs:51); so does the cutter -- but an inflater decodes only about a
// gigabyte a second, several times less than the stages behind it take, so the inflaters of the next files start
// early and run ahead of their turn until their share of the budget is queued.  (Nothing of this reorders the
// output: the cutter takes the files' blocks strictly in input order.)
struct Ahead {
  struct Block {
    std::vector<char> raw;
    size_t raw_len = 0;
    uint64_t n_lines = 0, first_line = 0;
    bool last_block = false;
    int rc = THM_OK;
    std::string err;
  };
  std::string path;
  uint64_t batch_reads = 0;
  size_t budget = 0;  // bytes this file may hold queued (one more block is cut once the queue is below it)
  thm_fastq* r = nullptr;
  std::thread th;
  std::mutex mu;
  std::condition_variable cv;
  std::deque<Block> ready;
  std::vector<std::vector<char>> spare;
  size_t queued = 0;
  int kind = -1;  // -1 not known yet; 0 not 4-line FASTQ (the cutter runs the sequential parser on `r`); 1 blocks; 2 cannot open
  int open_rc = THM_OK;
  std::string open_err;
  int dead_rc = THM_OK;  // the thread left with an exception: what wait_kind() / next() report once nothing is queued
  bool cancel = false;
  double busy_s = 0;

  void inflate() {
    const auto t0 = Clock::now();
    int rc = thm_fastq_open(path.c_str(), &r);
    bool fast = false;
    if (rc == THM_OK) fast = thm::fastq_is_plain_fastq(r);
    busy_s += secs(t0, Clock::now());
    {
      std::lock_guard<std::mutex> g(mu);
      open_rc = rc;
      if (rc != THM_OK) open_err = thm_last_error(nullptr);
      kind = rc != THM_OK ? 2 : (fast ? 1 : 0);
    }
    cv.notify_all();
    if (!fast) return;
    for (;;) {
      Block b;
      {
        std::unique_lock<std::mutex> g(mu);
        cv.wait(g, [&] { return queued < budget || cancel; });
        if (cancel) return;
        if (!spare.empty()) {
          b.raw.swap(spare.back());
          spare.pop_back();
        }
      }
      const auto t1 = Clock::now();
      try {
        b.rc = thm::fastq_next_raw_block(r, batch_reads, b.raw, b.raw_len, b.n_lines, b.first_line, b.last_block);
        if (b.rc != THM_OK) b.err = thm_last_error(nullptr);
      } catch (const std::bad_alloc&) {
        b.rc = THM_ERR_OOM;
        b.err = "out of host memory inflating " + path;
      }
      busy_s += secs(t1, Clock::now());
      const bool last = b.rc != THM_OK || b.n_lines == 0;
      {
        std::lock_guard<std::mutex> g(mu);
        queued += b.raw_len;
        ready.push_back(std::move(b));
      }
      cv.notify_all();
      if (last) return;
    }
  }
  // The thread body.  An exception anywhere in it (the open, a push into the queue) ends the file with an error in place
  // of the thread: a file whose kind is not known yet cannot be opened, any other ends with a last block that fails, so
  // that wait_kind() and next() always wake.
  void run() {
    (void)guarded([this] { inflate(); return (int)THM_OK; }, [this](int code, const std::string& m) {
      {
        std::lock_guard<std::mutex> g(mu);
        dead_rc = code;
        if (kind < 0) kind = 2, open_rc = code;
        try {
          open_err = m;
        } catch (...) {
        }
      }
      cv.notify_all();
    });
  }
  void start() { th = std::thread(&Ahead::run, this); }
  int wait_kind() {
    std::unique_lock<std::mutex> g(mu);
    cv.wait(g, [&] { return kind >= 0; });
    return kind;
  }
  // the next block of the file (the last one holds no line, or an error); `old` goes back for reuse
  void next(Block& out, std::vector<char>& old) {
    std::unique_lock<std::mutex> g(mu);
    cv.wait(g, [&] { return !ready.empty() || dead_rc != THM_OK; });
    if (ready.empty()) {
      out = Block();
      out.rc = dead_rc;
      out.err = open_err;
      return;
    }
    out = std::move(ready.front());
    ready.pop_front();
    queued -= out.raw_len;
    if (old.capacity()) spare.emplace_back(std::move(old));
    g.unlock();
    cv.notify_all();
  }
  void stop() {
    {
      std::lock_guard<std::mutex> g(mu);
      cancel = true;
    }
    cv.notify_all();
    if (th.joinable()) th.join();
    if (r) thm_fastq_close(r);
    r = nullptr;
  }
};

// blocking queue of slot pointers; nullptr = end of stream
struct Queue {
  std::mutex mu;
  std::condition_variable cv;
  std::deque<Slot*> q;
  void push(Slot* s) {
    {
      std::lock_guard<std::mutex> g(mu);
      q.push_back(s);
    }
    cv.notify_one();
  }
  Slot* pop() {
    std::unique_lock<std::mutex> g(mu);
    cv.wait(g, [&] { return !q.empty(); });
    Slot* s = q.front();
    q.pop_front();
    return s;
  }
};

// The hand-over from the parsers to the GPU threads: slots are put in any order and taken strictly by sequence number
// (parsers may finish out of order; an aligner that ran ahead of a batch it would later have to wait for could block the
// writer for good).
class ToGpu {
  std::mutex mu;
  std::condition_variable cv;
  std::map<uint64_t, Slot*> ready;
  uint64_t next = 0;
  bool closed = false;

 public:
  void put(Slot* s) {
    {
      std::lock_guard<std::mutex> g(mu);
      ready[s->seq] = s;
    }
    cv.notify_all();
  }
  void close() {  // the last parser has left
    {
      std::lock_guard<std::mutex> g(mu);
      closed = true;
    }
    cv.notify_all();
  }
  Slot* take_next() {  // null: the input is exhausted
    Slot* s = nullptr;
    {
      std::unique_lock<std::mutex> g(mu);
      cv.wait(g, [&] { return ready.count(next) || (closed && ready.empty()); });
      auto it = ready.find(next);
      if (it == ready.end()) return nullptr;
      s = it->second;
      ready.erase(it);
      next++;
    }
    cv.notify_all();
    return s;
  }
};

// The hand-over from the GPU threads to the writer: finished batches by sequence number, and how far the writer is.
class ToWriter {
  std::mutex mu;
  std::condition_variable cv;
  std::map<uint64_t, Slot*> done;
  uint64_t next = 0;           // the batch the writer takes next
  uint64_t n_batches_cut = 0;  // set when the cutter has seen the end of the input
  bool cut_done = false;
  uint64_t n_written = 0;  // batches the writer has finished

 public:
  void put(Slot* s) {
    {
      std::lock_guard<std::mutex> g(mu);
      done[s->seq] = s;
    }
    cv.notify_all();
  }
  void close(uint64_t n_batches) {  // the cutter has cut its last batch
    {
      std::lock_guard<std::mutex> g(mu);
      n_batches_cut = n_batches;
      cut_done = true;
    }
    cv.notify_all();
  }
  Slot* take_next() {  // null: the input is exhausted
    std::unique_lock<std::mutex> g(mu);
    cv.wait(g, [&] { return done.count(next) || (cut_done && next >= n_batches_cut); });
    auto it = done.find(next);
    if (it == done.end()) return nullptr;
    Slot* s = it->second;
    done.erase(it);
    next++;
    return s;
  }
  void written(uint64_t seq) {
    {
      std::lock_guard<std::mutex> g(mu);
      n_written = seq + 1;
    }
    cv.notify_all();
  }
  void wait_written(uint64_t seq, Shared& sh) {  // ... or until the run has failed
    std::unique_lock<std::mutex> g(mu);
    cv.wait(g, [&] { return n_written > seq || sh.failed(); });
  }
};

// THM_FASTQ_DEVICE>=2: the chain of uploads.  Every slot of such a run takes its turn in input order for its upload (a
// slot that is not compressed only passes the turn on).  The holder of the turn alone touches the Carry -- the tail that
// is the next head, the line count, where the plain-gzip file of the turn stands -- which wait_turn() hands out; the
// bytes and reads of the batches so far size the next groups and slices, from any thread.
class UploadChain {
 public:
  struct Carry {
    std::vector<uint8_t> tail;
    uint64_t line = 1;
    std::unique_ptr<thm_gzip_state> gz{new thm_gzip_state()};
    uint64_t gz_pos = 0, gz_in = 0, gz_out = 0;  // the position in the file; compressed and inflated bytes so far, for the ratio
    void begin_file() {
      tail.clear();
      line = 1;
      memset(gz.get(), 0, sizeof(thm_gzip_state));
      gz_pos = gz_in = gz_out = 0;
    }
    double ratio() const { return gz_in >= 65536 ? std::max(1.0, (double)gz_out / (double)gz_in) : 4.0; }
  };
  Carry& wait_turn(uint64_t seq) {
    std::unique_lock<std::mutex> g(mu);
    cv.wait(g, [&] { return turn == seq; });
    return carry;
  }
  // file_done: the upload that tells whether its plain-gzip file has another slice found none (or failed)
  void pass_turn(uint64_t seq, bool file_done_) {
    {
      std::lock_guard<std::mutex> g(mu);
      file_done = file_done_;
      turn = seq + 1;
    }
    cv.notify_all();
  }
  // the cutter, behind a slice: until that slice's upload has passed; true: the file has another slice
  bool wait_passed(uint64_t seq) {
    std::unique_lock<std::mutex> g(mu);
    cv.wait(g, [&] { return turn > seq; });
    return !file_done;
  }
  void count(uint64_t bytes, uint64_t reads) {
    est_bytes += bytes;
    est_reads += reads;
  }
  double bytes_per_read(double first_guess) const {
    const uint64_t eb = est_bytes.load(), er = est_reads.load();
    return er >= 64 ? (double)eb / (double)er : first_guess;
  }

 private:
  std::mutex mu;
  std::condition_variable cv;
  uint64_t turn = 0;
  bool file_done = false;
  Carry carry;
  std::atomic<uint64_t> est_bytes{0}, est_reads{0};
};

// what the knobs of the environment ask of a run to `format`
struct Modes {
  bool bam_sort = false;      // THM_BAM_SORT=1: the records of every batch stay on the device (thm_bam_sorter_add, uploads as with
                              // THM_BAM_DEVICE=1); once the input is exhausted they are sorted there and leave window by window
  bool bam_index = false;     // THM_BAM_INDEX=1 (asked for a BAM: valid beside THM_BAM_SORT=1 only): <output_path>.bai behind the sorted file
  bool bgzf_device = false;   // THM_BAM_DEVICE=2: ... and BGZF-compressed there too (thm_batch_fetch_bgzf): the formatting stage passes bytes on
  bool bam_device = false;    // THM_BAM_DEVICE=1: BAM records are encoded on the device (thm_batch_fetch_bam) and only deflated here
  // THM_FASTQ_DEVICE, in those modes only (the host needs no read bytes there):
  bool fastq_device = false;  // =1: blocks of 4-line FASTQ go to the device unparsed (thm_batch_upload_fastq)
  bool fastq_bgzf = false;    // =2: as =1, and input files that are BGZF throughout go to the device compressed
                              // (thm_batch_upload_fastq_bgzf); every other file takes the path of =1
  bool fastq_gzip = false;    // =3: as =2, and gzip files that are not BGZF throughout go to the device compressed too, in slices
                              // (thm_batch_upload_fastq_gzip)
  bool quant = false;         // THM_QUANT=1, any format: every batch is added to its aligner's thm_quant behind its fetch, and
                              // <output_path>.genes.tsv / .junctions.tsv are written at the end
  bool coverage = false;      // THM_COVERAGE=1..3, any format: every batch is added to its aligner's thm_coverage behind its fetch, and
  uint32_t cov_flags = 0;     // <output_path>.cov.<track>.bedgraph are written at the end; =2: THM_COV_STRANDED, =3: ... | THM_COV_MULTI
  bool pileup = false;        // THM_PILEUP=1|2, any format, one aligner: every batch is added to a thm_pileup behind its fetch, and
  uint32_t pile_flags = 0;    // <output_path>.pileup.tsv is written at the end; =2: THM_PILE_MULTI
  uint32_t pile_min_alt = 2;  // THM_PILEUP_MIN_ALT: the events a site needs for a line (at least 1)
  bool pile_bad = false;      // THM_PILEUP is set to something else, or THM_PILEUP_MIN_ALT is no number of 1 or more: the run is refused
  bool cells = false;         // THM_CELLS=1|2, any format, one aligner: every batch goes up with its names and is added to a thm_cells
  uint32_t cells_flags = 0;   // behind its fetch; <output_path>.cells.mtx / .barcodes.tsv / .features.tsv are written at the end; =2: THM_CELLS_INTRONIC
  uint32_t cells_cb_len = 16, cells_umi_len = 12;  // THM_CELLS_CB_LEN, THM_CELLS_UMI_LEN: the tag's lengths, each 1..16
  uint32_t cells_min_umis = 1;                     // THM_CELLS_MIN_UMIS: the molecules a barcode needs to be a cell (at least 1)
  bool cells_bad = false;     // THM_CELLS is set to something else, or one of the three is no such number: the run is refused
  static Modes read(int32_t format) {
    auto is = [](const char* name, const char* v) {
      const char* e = getenv(name);
      return e && !strcmp(e, v);
    };
    Modes m;
    const bool bam = format == THM_FMT_BAM;
    m.bam_sort = bam && is("THM_BAM_SORT", "1");
    m.bam_index = bam && is("THM_BAM_INDEX", "1");
    m.bgzf_device = !m.bam_sort && bam && is("THM_BAM_DEVICE", "2");
    m.bam_device = m.bam_sort || m.bgzf_device || (bam && is("THM_BAM_DEVICE", "1"));
    m.fastq_gzip = m.bam_device && is("THM_FASTQ_DEVICE", "3");
    m.fastq_bgzf = m.fastq_gzip || (m.bam_device && is("THM_FASTQ_DEVICE", "2"));
    m.fastq_device = m.fastq_bgzf || (m.bam_device && is("THM_FASTQ_DEVICE", "1"));
    m.quant = is("THM_QUANT", "1");
    m.coverage = is("THM_COVERAGE", "1") || is("THM_COVERAGE", "2") || is("THM_COVERAGE", "3");
    m.cov_flags = is("THM_COVERAGE", "2") ? THM_COV_STRANDED : is("THM_COVERAGE", "3") ? (THM_COV_STRANDED | THM_COV_MULTI) : 0u;
    m.pileup = is("THM_PILEUP", "1") || is("THM_PILEUP", "2");
    m.pile_flags = is("THM_PILEUP", "2") ? THM_PILE_MULTI : 0u;
    if (const char* e = getenv("THM_PILEUP")) m.pile_bad = *e && strcmp(e, "0") && !m.pileup;
    if (const char* e = getenv("THM_PILEUP_MIN_ALT")) {
      char* end = nullptr;
      const long v = strtol(e, &end, 10);
      if (end == e || *end || v < 1 || v > 0x7FFFFFFFl)
        m.pile_bad = true;
      else
        m.pile_min_alt = (uint32_t)v;
    }
    m.cells = is("THM_CELLS", "1") || is("THM_CELLS", "2");
    m.cells_flags = is("THM_CELLS", "2") ? THM_CELLS_INTRONIC : 0u;
    if (const char* e = getenv("THM_CELLS")) m.cells_bad = *e && strcmp(e, "0") && !m.cells;
    const auto number = [&](const char* name, long most, uint32_t* out) {
      const char* e = getenv(name);
      if (!e) return;
      char* end = nullptr;
      const long v = strtol(e, &end, 10);
      if (end == e || *end || v < 1 || v > most)
        m.cells_bad = true;
      else
        *out = (uint32_t)v;
    };
    number("THM_CELLS_CB_LEN", (long)THM_CELLS_MAX_LEN, &m.cells_cb_len);
    number("THM_CELLS_UMI_LEN", (long)THM_CELLS_MAX_LEN, &m.cells_umi_len);
    number("THM_CELLS_MIN_UMIS", 0x7FFFFFFFl, &m.cells_min_umis);
    return m;
  }
};

// the output file (or stdout): a regular file takes the chunks of a batch at their final offsets from several threads
struct Output {
  int fd = -1;
  bool to_stdout = false, positional = false;
  uint64_t off = 0;  // where the next bytes go (the writer stage's)
  bool open(const char* path) {
    to_stdout = strcmp(path, "-") == 0;
    if (to_stdout) fflush(stdout);
    fd = to_stdout ? 1 : ::open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
    struct stat sb;
    positional = fd >= 0 && !to_stdout && fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode);
    return fd >= 0;
  }
  bool close() {
    const bool ok = to_stdout || fd < 0 || ::close(fd) == 0;
    fd = -1;
    return ok;
  }
  bool write_all(const char* p, size_t n, uint64_t at) const {
    while (n) {
      const ssize_t k = positional ? pwrite(fd, p, n, (off_t)at) : write(fd, p, n);
      if (k <= 0) return false;
      p += k;
      n -= (size_t)k;
      at += (uint64_t)k;
    }
    return true;
  }
};

// what the writer thread writes of one batch; two of them alternate (job k & 1 for batch k)
struct WriteJob {
  Slot* s = nullptr;
  std::vector<const std::string*> chunks;
  std::vector<std::pair<const char*, size_t>> spans;  // what is written: the chunks, or the span the fetch left
  std::vector<uint64_t> at;
};
class WriteJobs {
  std::mutex mu;
  std::condition_variable cv;
  std::deque<WriteJob*> q;  // nullptr = end of stream
  WriteJob jobs[2];
  bool busy[2] = {false, false};

 public:
  WriteJob& job(int k) { return jobs[k]; }  // the formatter's while it is not busy
  void wait_free(int k) {  // job k's previous batch has left
    std::unique_lock<std::mutex> g(mu);
    cv.wait(g, [&] { return !busy[k]; });
  }
  void wait_idle() {
    std::unique_lock<std::mutex> g(mu);
    cv.wait(g, [&] { return !busy[0] && !busy[1]; });
  }
  void submit(int k) {
    {
      std::lock_guard<std::mutex> g(mu);
      busy[k] = true;
      q.push_back(&jobs[k]);
    }
    cv.notify_all();
  }
  void stop() {
    {
      std::lock_guard<std::mutex> g(mu);
      q.push_back(nullptr);
    }
    cv.notify_all();
  }
  WriteJob* take() {
    std::unique_lock<std::mutex> g(mu);
    cv.wait(g, [&] { return !q.empty(); });
    WriteJob* j = q.front();
    q.pop_front();
    return j;
  }
  void finished(WriteJob* j) {
    {
      std::lock_guard<std::mutex> g(mu);
      busy[j - jobs] = false;
    }
    cv.notify_all();
  }
};

// One run of thm_align_files_multi: the state the stages share, and the stages -- cut(), parse(), gpu(gi) and
// format_and_write() with its write_jobs() thread and drain_sorted() -- each on a thread of its own (format_and_write on
// the caller's).  What holds between them, whatever the modes:
//   1. Slots reach the GPU threads strictly in seq order, whichever parser finished first (ToGpu).
//   2. With THM_FASTQ_DEVICE>=2 every slot takes and passes the upload turn in seq order (UploadChain) -- slots that are not
//      compressed, slots of a run that has failed and slots with no read included.
//   3. For a gzip slice, file_done is published before the turn passes (pass_turn does both), and the cutter cuts the next
//      slice of that file only after it (wait_passed).
//   4. A fetch on an aligner waits until that aligner's second-last fetched batch has been written (ToWriter::wait_written):
//      every aligner keeps the results of its last two fetches.
//   5. Batches are formatted and written in seq order (ToWriter::take_next).  Two writer objects alternate, and job k & 1 is
//      reused only after its write has left (WriteJobs).
//   6. After any failure every thread still completes its hand-over protocol: every slot that was cut passes through every
//      stage and back to q_free, so that no thread is left blocked, q_free does not starve and all threads join.
//   7. Every mapping lives until every batch has been written: `maps` dies with the run, after the stages have joined.
struct Run {
  thm_aligner* const* aligners;
  const uint32_t n_aligners;
  const char* const* paths;
  const uint32_t n_paths;
  const int32_t format;
  const uint64_t batch_reads;
  const uint32_t n_threads;
  const unsigned n_parsers;
  const Modes m;
  thm_writer* ws[2];  // used alternately: the chunks of batch k are views into writer k & 1 and are still being written while
                      // batch k + 1 is formatted, so one object cannot stand in for both
  Output& out;
  thm_bam_sorter* sorter;
  thm_quant* const* quants = nullptr;  // THM_QUANT=1: one per aligner
  thm_coverage* const* coverages = nullptr;  // THM_COVERAGE: one per aligner
  thm_pileup* pileup = nullptr;              // THM_PILEUP: the one aligner's
  thm_cells* cells = nullptr;                // THM_CELLS: the one aligner's

  Shared sh;
  thm_run_stats st;
  std::mutex st_mu;  // parse_s / gpu_s / n_reads / n_batches are summed by several threads
  // every aligner keeps the results of its last two fetches: two batches per GPU may be between fetch and write,
  // one more is running; the parsers and the cutter work ahead of that
  std::vector<Slot> slots;
  Queue q_free, q_raw;
  ToGpu to_gpu;
  ToWriter to_writer;
  UploadChain chain;
  WriteJobs wj;
  std::vector<Mapping> maps;  // of the input files that were cut in place (the cutter's, until it has joined)
  std::mutex parsers_mu;
  unsigned parsers_left;

  Run(thm_aligner* const* aligners_, uint32_t n_aligners_, const char* const* paths_, uint32_t n_paths_, int32_t format_, uint64_t batch_reads_,
      uint32_t n_threads_, unsigned n_parsers_, const Modes& m_, thm_writer* w0, thm_writer* w1, Output& out_, thm_bam_sorter* sorter_)
      : aligners(aligners_), n_aligners(n_aligners_), paths(paths_), n_paths(n_paths_), format(format_), batch_reads(batch_reads_),
        n_threads(n_threads_), n_parsers(n_parsers_), m(m_), ws{w0, w1}, out(out_), sorter(sorter_), slots(3 * n_aligners_ + n_parsers_ + 2),
        parsers_left(n_parsers_) {
    memset(&st, 0, sizeof st);
    for (auto& s : slots) q_free.push(&s);
  }

  void add_parse_time(double s) {
    std::lock_guard<std::mutex> g(st_mu);
    st.parse_s += s;
  }
  // a free slot, reset for batch `seq` of `path`; null, and the run has failed, where that throws (the slot is free again)
  Slot* fresh_slot(uint64_t seq, const char* path) {
    Slot* s = q_free.pop();
    if (sh.step([&] { s->reset(seq, path); return (int)THM_OK; }) == THM_OK) return s;
    q_free.push(s);
    return nullptr;
  }
  // header, trailer: bytes of the writer stage's own, at the end of what is written so far
  void append(const thm_text& t) {
    if (!t.len) return;
    if (!out.write_all((const char*)t.data, t.len, out.off)) sh.set(THM_ERR_IO, "short write");
    out.off += t.len;
    st.n_output_bytes += t.len;
  }

  // ---- stage 1: cut the input into blocks of whole records
  void cut();
  void cut_members(BgzfFile& bf, const char* path, uint64_t& seq);
  void cut_slices(GzipFile& gf, const char* path, uint64_t& seq);
  void cut_blocks(const char* path, Ahead* ah, uint64_t& seq);
  // ---- stage 2: parse blocks (several threads)
  void parse();
  // ---- stage 3: one thread per aligner
  void gpu(uint32_t gi);
  int upload_members(thm_aligner* a, Slot* s, UploadChain::Carry& c, bool& have);
  int upload_slice(thm_aligner* a, Slot* s, UploadChain::Carry& c, bool& have, bool& file_done);
  int fetch(thm_aligner* a, Slot* s);
  int fail_by_name(thm_aligner* a, Slot* s, bool raw_up);
  // ---- stage 4: format (the caller's thread, on the formatting threads of the writer) and write (one more thread), in
  // input order, so that batch k + 1 is formatted while batch k is written
  void format_and_write();
  int format_batch(Slot* s, int k);
  void write_jobs();
  void release(Slot* s);
  void drain_sorted();
  void write_index();
  uint64_t first_member_offset = 0;  // where the sorted file's first record member stands: the sorted header's length
  std::string index_path;            // THM_BAM_INDEX=1: <output_path>.bai
};

// groups of whole members of about batch_reads reads, by the bytes per record of the batches so far
void Run::cut_members(BgzfFile& bf, const char* path, uint64_t& seq) {
  const size_t nm = bf.tab.size();
  maps.push_back(std::move(bf.map));  // the run's before the first slot points into it: whatever happens here, it outlives the writes
  const Mapping& map = maps.back();
  for (size_t k = 0; k < nm && !sh.failed();) {
    Slot* s = fresh_slot(seq, path);
    if (!s) break;
    const size_t k1 = thm::member_group_end(bf.tab, nm, k, chain.bytes_per_read(bf.bytes_per_read) * (double)batch_reads);
    s->zmembers = true;
    s->file_first = k == 0;
    s->raw_ptr = (const char*)map.p + bf.at[k];
    s->raw_len = (size_t)(bf.at[k1] - bf.at[k]);
    s->last_block = k1 == nm;
    k = k1;
    seq++;
    q_raw.push(s);
  }
}

// one slot after the other: where a slice begins is known once the one before has gone up
void Run::cut_slices(GzipFile& gf, const char* path, uint64_t& seq) {
  maps.push_back(std::move(gf.map));  // (as in cut_members)
  const Mapping& map = maps.back();
  for (bool first = true, more = true; more && !sh.failed(); first = false) {
    Slot* s = fresh_slot(seq, path);
    if (!s) break;
    s->gzslice = true;
    s->file_first = first;
    s->gz_map = map.p;
    s->gz_len = map.len;
    const uint64_t mine = seq++;
    q_raw.push(s);
    more = chain.wait_passed(mine);
  }
}

// Blocks of text: ranges of the mapping of a plain (not gzip) FASTQ file, which is cut in place; the blocks of the file's
// inflater thread; the blocks of a reader; or, for FASTA and anything that is not plain 4-line FASTQ, batches of the
// sequential parser.
void Run::cut_blocks(const char* path, Ahead* ah, uint64_t& seq) {
  thm_fastq* r = nullptr;
  bool fast = false;
  if (ah) {
    const int kind = ah->wait_kind();
    if (kind == 2) {
      sh.set(ah->open_rc, ah->open_err);
      return;
    }
    fast = kind == 1;
    r = ah->r;  // (the sequential parser's, when the file is not 4-line FASTQ: the inflater thread has left)
  } else {
    const int orc = thm_fastq_open(path, &r);
    if (orc != THM_OK) {
      sh.set(orc, thm_last_error(nullptr));
      return;
    }
    fast = thm::fastq_is_plain_fastq(r);
  }
  const char* map = nullptr;
  size_t map_len = 0;
  if (fast && !ah) {
    Mapping m = Mapping::open(path, 2, true);
    if (m && !m.is_gzip()) {
      map = (const char*)m.p;
      map_len = m.len;
      maps.push_back(std::move(m));  // (as in cut_members)
    }
  }
  size_t map_pos = 0;
  uint64_t map_line = 1;
  for (;;) {
    Slot* s = fresh_slot(seq, path);
    if (!s) break;
    const auto t0 = Clock::now();
    uint64_t n_lines = 0;
    int prc = THM_OK;
    if (map) {
      const size_t p = thm::mapped_cut(map, map_len, map_pos, batch_reads * 4, &n_lines);
      s->raw_ptr = map + map_pos;
      s->raw_len = p - map_pos;
      s->last_block = p == map_len;
      s->first_line = map_line;
      map_line += n_lines;
      map_pos = p;
    } else if (fast && ah) {
      Ahead::Block b;
      prc = sh.step([&] { ah->next(b, s->raw); return (int)THM_OK; });
      if (prc == THM_OK) {
        s->raw.swap(b.raw);
        s->raw_len = b.raw_len;
        s->first_line = b.first_line;
        s->last_block = b.last_block;
        n_lines = b.n_lines;
        prc = b.rc;
        if (prc != THM_OK) thm::set_global_error(b.err);
        s->raw_ptr = s->raw.data();
      }
    } else if (fast) {
      prc = sh.step([&] { return thm::fastq_next_raw_block(r, batch_reads, s->raw, s->raw_len, n_lines, s->first_line, s->last_block); });
      s->raw_ptr = s->raw.data();
    } else {
      prc = sh.step([&] { return thm::fastq_fill(r, batch_reads, s->reads); });
      s->parsed = true;
      n_lines = s->reads.n_reads();
    }
    if (!(fast && ah)) add_parse_time(secs(t0, Clock::now()));  // (an inflater thread counts its own time)
    if (prc != THM_OK || sh.failed() || n_lines == 0) {
      if (prc != THM_OK) sh.set(prc, thm_last_error(nullptr));
      q_free.push(s);
      break;
    }
    seq++;
    q_raw.push(s);
  }
  if (ah) {
    ah->stop();  // (closes the reader)
    add_parse_time(ah->busy_s);
  } else {
    thm_fastq_close(r);
  }
}

void Run::cut() {
  uint64_t seq = 0;
  // gzip inputs get an inflater thread each (Ahead), those of the next few files running ahead of their turn -- unless
  // the file goes to the device compressed: no inflater thread then, it is cut by its members or in slices
  std::vector<std::unique_ptr<Ahead>> ahead(n_paths);
  std::vector<char> is_gz(n_paths, 0);
  std::vector<std::unique_ptr<BgzfFile>> bgzf_files(n_paths);
  std::vector<std::unique_ptr<GzipFile>> gzip_files(n_paths);
  unsigned n_gz = 0;
  (void)sh.step([&] { maps.reserve(n_paths); return (int)THM_OK; });
  for (uint32_t pi = 0; pi < n_paths; pi++) {
    unsigned char magic[2] = {0, 0};
    const int fd = open(paths[pi], O_RDONLY);
    if (fd >= 0) {
      is_gz[pi] = pread(fd, magic, 2, 0) == 2 && magic[0] == 0x1f && magic[1] == 0x8b;
      close(fd);
    }
    if (is_gz[pi] && m.fastq_bgzf) {
      const auto t0 = Clock::now();
      (void)sh.step([&] {
        std::unique_ptr<BgzfFile> bf(new BgzfFile());
        if (bf->open(paths[pi])) {
          bgzf_files[pi] = std::move(bf);
        } else if (m.fastq_gzip) {  // ... or in slices, wherever its blocks end
          std::unique_ptr<GzipFile> gf(new GzipFile());
          if (gf->open(paths[pi])) gzip_files[pi] = std::move(gf);
        }
        if (bgzf_files[pi] || gzip_files[pi]) is_gz[pi] = 0;
        return (int)THM_OK;
      });
      add_parse_time(secs(t0, Clock::now()));
    }
    n_gz += is_gz[pi];
  }
  const unsigned ahead_files = std::max(1u, std::min(n_gz, std::max(2u, n_threads / 4)));
  size_t ahead_bytes = (size_t)768 << 20;  // all inflaters together; THM_INFLATE_AHEAD_MB overrides
  if (const char* e = getenv("THM_INFLATE_AHEAD_MB")) ahead_bytes = (size_t)std::max(1L, atol(e)) << 20;
  auto top_up = [&](uint32_t from) {  // the inflaters of the next `ahead_files` gzip files at or behind `from`
    unsigned running = 0;
    for (uint32_t k = from; k < n_paths && running < ahead_files; k++) {
      if (!is_gz[k]) continue;
      running++;
      if (ahead[k]) continue;
      ahead[k].reset(new Ahead());
      ahead[k]->path = paths[k];
      ahead[k]->batch_reads = batch_reads;
      ahead[k]->budget = ahead_bytes / ahead_files;
      ahead[k]->start();
    }
    return (int)THM_OK;
  };
  for (uint32_t pi = 0; pi < n_paths && !sh.failed(); pi++) {
    if (sh.step([&] { return top_up(pi); }) != THM_OK) break;
    if (sh.step([&] {
          if (bgzf_files[pi]) cut_members(*bgzf_files[pi], paths[pi], seq);
          else if (gzip_files[pi]) cut_slices(*gzip_files[pi], paths[pi], seq);
          else cut_blocks(paths[pi], is_gz[pi] ? ahead[pi].get() : nullptr, seq);
          return (int)THM_OK;
        }) != THM_OK)
      break;
  }
  for (auto& a : ahead)
    if (a) a->stop();  // (inflaters started ahead of a run that failed)
  to_writer.close(seq);
  for (unsigned k = 0; k < n_parsers; k++) q_raw.push(nullptr);
}

void Run::parse() {
  while (Slot* s = q_raw.pop()) {
    if (!s->parsed && !m.fastq_device && !sh.failed()) {  // (with THM_FASTQ_DEVICE the block passes through as it is)
      const auto t0 = Clock::now();
      std::string err;
      const int prc = sh.step([&] { return thm::fastq_parse_block(s->raw_ptr, s->raw_len, s->path, s->first_line, s->last_block, s->reads, err); });
      add_parse_time(secs(t0, Clock::now()));
      if (prc != THM_OK) sh.set(prc, err);
    }
    to_gpu.put(s);
  }
  std::lock_guard<std::mutex> g(parsers_mu);
  if (--parsers_left == 0) to_gpu.close();
}

// a group of members at its turn in the chain: the tail so far is its head
int Run::upload_members(thm_aligner* a, Slot* s, UploadChain::Carry& c, bool& have) {
  if (s->file_first) c.begin_file();
  s->first_line = c.line;
  if (!have) return THM_OK;
  thm_fastq_bgzf_info zi;
  memset(&zi, 0, sizeof zi);
  const int rc = sh.step([&] {
    const size_t head_len = c.tail.size();
    const int r2 = (int)thm_batch_upload_fastq_bgzf(a, c.tail.data(), head_len, (const uint8_t*)s->raw_ptr, s->raw_len, s->path.c_str(), s->first_line,
                                                    s->last_block ? 1 : 0, &zi);
    if (r2 == THM_OK) {
      c.tail.assign(zi.tail, zi.tail + zi.tail_len);
      c.line += zi.n_lines;
      chain.count(head_len + zi.n_inflated_bytes - zi.tail_len, zi.n_reads);
    }
    return r2;
  });
  if (rc == THM_OK && zi.n_reads == 0) have = false;  // (a group without a whole record: all of it is tail)
  return rc;
}

// A slice of a plain-gzip file at its turn in the chain, where the slice before it ended: of about batch_reads reads, by
// the bytes per record and the ratio of the batches so far; doubled while no block ends inside it.  file_done: the file
// has no further slice (a run that has failed cuts none).
int Run::upload_slice(thm_aligner* a, Slot* s, UploadChain::Carry& c, bool& have, bool& file_done) {
  if (s->file_first) c.begin_file();
  s->first_line = c.line;
  file_done = true;
  if (!have) return THM_OK;
  thm_fastq_gzip_info zi;
  memset(&zi, 0, sizeof zi);
  uint64_t want = (uint64_t)(chain.bytes_per_read(256.0) * (double)batch_reads / c.ratio()) + 4096;
  const int rc = sh.step([&] {
    const size_t head_len = c.tail.size();
    for (;;) {
      const uint64_t left = s->gz_len - c.gz_pos, n = std::min<uint64_t>(want, left);
      s->last_block = n == left;
      const int r2 = (int)thm_batch_upload_fastq_gzip(a, c.gz.get(), c.tail.data(), head_len, s->gz_map + c.gz_pos, n, s->path.c_str(), s->first_line,
                                                      s->last_block ? 1 : 0, &zi);
      if (r2 != THM_OK) return r2;
      if (zi.n_consumed_bytes == 0 && !s->last_block) {
        want = 2 * n;
        continue;
      }
      c.gz_pos += zi.n_consumed_bytes;
      c.gz_in += zi.n_consumed_bytes;
      c.gz_out += zi.n_inflated_bytes;
      c.tail.assign(zi.tail, zi.tail + zi.tail_len);
      c.line += zi.n_lines;
      chain.count(head_len + zi.n_inflated_bytes - zi.tail_len, zi.n_reads);
      return (int)THM_OK;
    }
  });
  file_done = rc != THM_OK || s->last_block;
  if (rc == THM_OK && zi.n_reads == 0) have = false;  // (a slice without a whole record: all of it is tail)
  return rc;
}

// the fetch the modes ask for, into s->got (and the view the formatting needs, where the host formats)
int Run::fetch(thm_aligner* a, Slot* s) {
  Fetched& f = s->got;
  int rc;
  if (m.bam_sort) {
    thm_bam_sort_info v;
    memset(&v, 0, sizeof v);
    rc = thm::bam_sorter_add(sorter, 0, &v, &f.n_aligned);
    f.n_reads = v.n_reads, f.read_status = v.read_status, f.n_failed_reads = v.n_failed_reads, f.n_records = v.n_records;
  } else if (m.bgzf_device) {
    thm_bgzf_view v;
    memset(&v, 0, sizeof v);
    rc = thm::batch_fetch_bgzf(a, 0, &v, &f.n_aligned);
    f.n_reads = v.n_reads, f.read_status = v.read_status, f.n_failed_reads = v.n_failed_reads, f.n_records = v.n_records;
    f.span = (const char*)v.data, f.span_len = (size_t)v.n_bytes;
  } else if (m.bam_device) {
    rc = thm_batch_fetch_bam(a, 0, &s->bam);
    f.n_reads = s->bam.n_reads, f.read_status = s->bam.read_status, f.n_failed_reads = s->bam.n_failed_reads;
  } else {
    rc = thm_batch_fetch(a, &s->res);
    f.n_reads = s->res.n_reads, f.read_status = s->res.read_status, f.n_failed_reads = s->res.n_failed_reads;
  }
  return rc;
}

// The reference aligns every read or panics; a read this build cannot take fails the run, by name.  The name is the
// host's where the host parsed the batch; a block that went up raw stands on the device with its names.
int Run::fail_by_name(thm_aligner* a, Slot* s, bool raw_up) {
  const Fetched& f = s->got;
  uint64_t bad = 0;
  while (bad < f.n_reads && f.read_status[bad] == THM_OK) bad++;
  thm_read_batch v = s->reads.view();
  if (raw_up) {
    memset(&v, 0, sizeof v);
    (void)sh.step([&] { return (int)thm_batch_fetch_reads(a, &v); });
  }
  std::string name;
  if (bad < v.n_reads) name.assign((const char*)v.names + v.name_off[bad], (size_t)(v.name_off[bad + 1] - v.name_off[bad]));
  sh.set(f.read_status[bad], "read " + name + (f.read_status[bad] == THM_ERR_UNSUPPORTED
                                                   ? ": longer than 65535 bases, or its DP trace exceeds the device-memory budget"
                                                   : ": hits a condition that panics in the reference (lift_mem_to_tx / lift_tx_to_gx)"));
  return f.read_status[bad];
}

void Run::gpu(uint32_t gi) {
  thm_aligner* a = aligners[gi];
  std::deque<uint64_t> fetched;  // sequence numbers of this aligner's fetched batches, oldest first
  while (Slot* s = to_gpu.take_next()) {
    // a raw block goes up as it is and is parsed there; the slot keeps its bytes (its own buffer, or the mapping) until
    // it is released behind the write
    const bool raw_up = m.fastq_device && !s->parsed;
    bool have = !sh.failed() && (raw_up || s->reads.n_reads() != 0);  // (a blank tail cut into a block of its own holds no read)
    const auto t0 = Clock::now();
    int up_rc = THM_OK;
    if (m.fastq_bgzf) {  // this slot's turn in the chain of uploads
      UploadChain::Carry& c = chain.wait_turn(s->seq);
      bool file_done = false;
      if (s->zmembers) up_rc = upload_members(a, s, c, have);
      if (s->gzslice) up_rc = upload_slice(a, s, c, have, file_done);
      chain.pass_turn(s->seq, file_done);
    }
    if (have && raw_up && !s->zmembers && !s->gzslice) {
      thm_fastq_upload_info fi;
      memset(&fi, 0, sizeof fi);
      up_rc = sh.step([&] {
        return (int)thm_batch_upload_fastq(a, (const uint8_t*)s->raw_ptr, s->raw_len, s->path.c_str(), s->first_line, s->last_block ? 1 : 0, &fi);
      });
      if (up_rc == THM_OK && fi.n_reads == 0) have = false;  // (that blank tail)
    }
    if (have) {
      const thm_read_batch rb = s->reads.view();
      int grc = sh.step([&] {
        int g2 = raw_up ? up_rc : (m.bam_device || m.cells) ? thm_batch_upload_reads(a, &rb) : thm_batch_upload(a, rb.bases, rb.offsets, rb.n_reads);
        if (g2 == THM_OK) g2 = thm_batch_run(a);
        if (g2 == THM_OK) g2 = thm_batch_sync(a);
        return g2;
      });
      const auto t1 = Clock::now();
      // the fetch below reuses the buffers of this aligner's second-last fetch: that batch must have been written
      if (grc == THM_OK && fetched.size() >= 2) to_writer.wait_written(fetched[fetched.size() - 2], sh);
      const auto t2 = Clock::now();
      if (grc == THM_OK) grc = sh.step([&] { return fetch(a, s); });
      if (grc == THM_OK && s->got.n_failed_reads) grc = fail_by_name(a, s, raw_up);
      if (grc == THM_OK && quants) {
        thm_quant_info qi;
        grc = sh.step([&] { return (int)thm_quant_add(quants[gi], &qi); });
      }
      if (grc == THM_OK && coverages) {
        thm_cov_info ci;
        grc = sh.step([&] { return (int)thm_coverage_add(coverages[gi], &ci); });
      }
      if (grc == THM_OK && pileup) {
        thm_pile_info pi;
        grc = sh.step([&] { return (int)thm_pileup_add(pileup, &pi); });
      }
      if (grc == THM_OK && cells) {
        thm_cells_info ci;
        grc = sh.step([&] { return (int)thm_cells_add(cells, &ci); });
      }
      if (grc != THM_OK) {
        sh.set(grc, thm_last_error(a));
      } else {
        s->aligned = true;
        fetched.push_back(s->seq);
        if (fetched.size() > 4) fetched.pop_front();
      }
      std::lock_guard<std::mutex> g(st_mu);
      st.gpu_s += secs(t0, t1) + secs(t2, Clock::now());
      if (grc == THM_OK) {
        st.n_reads += s->got.n_reads;
        st.n_batches += 1;
      }
    }
    to_writer.put(s);
  }
}

void Run::release(Slot* s) {
  to_writer.written(s->seq);
  q_free.push(s);
}

// the writer thread: the spans of a job at their offsets (those of a regular file from several threads)
void Run::write_jobs() {
  while (WriteJob* j = wj.take()) {
    const auto t1 = Clock::now();
    std::vector<char> good(j->spans.size(), 1);
    auto put = [&](size_t c) { good[c] = out.write_all(j->spans[c].first, j->spans[c].second, j->at[c]) ? 1 : 0; };
    if (out.positional && j->spans.size() > 1) {
      std::vector<std::thread> th;
      for (size_t c = 1; c < j->spans.size(); c++) th.emplace_back(put, c);
      put(0);
      for (auto& x : th) x.join();
    } else {
      for (size_t c = 0; c < j->spans.size(); c++) put(c);
    }
    for (char g : good)
      if (!g) sh.set(THM_ERR_IO, "short write");
    st.write_s += secs(t1, Clock::now());
    release(j->s);
    wj.finished(j);
  }
}

// Batch s into job k: the spans to write and their offsets, and the batch's part in the statistics.  Where the fetch
// left a span there is nothing to format: the members leave as one chunk, written from the aligner's pinned set (the GPU
// thread waits for this batch to be written before the fetch that reuses the set).
int Run::format_batch(Slot* s, int k) {
  WriteJob& j = wj.job(k);
  Fetched& f = s->got;
  const auto t0 = Clock::now();
  const thm_read_batch rb = s->reads.view();
  const int wrc = sh.step([&] {
    if (m.bgzf_device) return (int)THM_OK;
    return m.bam_device ? thm::writer_wrap_bam_chunks(ws[k], &s->bam, j.chunks) : thm::writer_format_chunks(ws[k], &rb, &s->res, j.chunks);
  });
  st.format_s += secs(t0, Clock::now());
  if (wrc != THM_OK) {
    sh.set(wrc, thm_last_error(nullptr));
    return wrc;
  }
  j.spans.clear();
  if (m.bgzf_device) j.spans.emplace_back(f.span, f.span_len);
  else
    for (const std::string* c : j.chunks) j.spans.emplace_back(c->data(), c->size());
  j.at.resize(j.spans.size());
  for (size_t c = 0; c < j.spans.size(); c++) {
    j.at[c] = out.off;
    out.off += j.spans[c].second;
    st.n_output_bytes += j.spans[c].second;
  }
  if (m.bgzf_device) return THM_OK;
  if (m.bam_device) {
    // a read is unmapped when its first record carries flag 4 (bytes 18 .. 19 of the record)
    const thm_bam_view& bv = s->bam;
    for (uint64_t r = 0; r < bv.n_reads; r++) f.n_aligned += !(bv.data[bv.read_rec_off[r] + 18] & 4);
    f.n_records = bv.n_records;
  } else {
    const thm_batch_view& v = s->res;
    for (uint64_t r = 0; r < v.n_reads; r++) {
      const uint64_t kk = v.read_aln_off[r + 1] - v.read_aln_off[r];
      f.n_aligned += kk != 0;
      f.n_records += kk ? kk : (format == THM_FMT_PAF ? 0 : 1);
    }
  }
  return THM_OK;
}

void Run::format_and_write() {
  thm_text t;
  // (a sorted file's header is written when the drain begins)
  if (!m.bam_sort && thm_writer_header(ws[0], &t) == THM_OK) append(t);
  std::thread wthread(&Run::write_jobs, this);
  for (;;) {
    Slot* s = to_writer.take_next();
    if (!s) break;  // the input is exhausted
    const int k = (int)(s->seq & 1);
    wj.wait_free(k);  // the writer object (and job) of this parity: its previous batch must have left
    bool queued = false;
    // (after a failure nothing is formatted any more; a sorted run's batch is in the sorter: nothing leaves before the
    // input is exhausted)
    if (!sh.failed() && s->aligned && (m.bam_sort || format_batch(s, k) == THM_OK)) {
      st.n_aligned_reads += s->got.n_aligned;
      st.n_records += s->got.n_records;
      if (!m.bam_sort) {
        wj.job(k).s = s;
        wj.submit(k);
        queued = true;
      }
    }
    if (!queued) {
      // nothing to write for this batch: it still leaves in order behind the writes that are queued
      wj.wait_idle();
      release(s);
    }
  }
  wj.wait_idle();
  wj.stop();
  wthread.join();
  if (m.bam_sort && !sh.failed()) drain_sorted();
  if (!sh.failed() && thm_writer_trailer(ws[0], &t) == THM_OK) append(t);
  if (m.bam_sort && m.bam_index && !sh.failed()) write_index();
}

// the .bai of the sorted file, whole, behind the file's end-of-file block
void Run::write_index() {
  thm_bai_view v;
  const auto t0 = Clock::now();
  const int rc = sh.step([&] { return (int)thm_bam_sorter_index(sorter, first_member_offset, &v); });
  st.format_s += secs(t0, Clock::now());
  if (rc != THM_OK) {
    sh.set(rc, thm_last_error(aligners[0]));
    return;
  }
  const auto t1 = Clock::now();
  Output ix;
  const bool ok = ix.open(index_path.c_str()) && ix.write_all((const char*)v.data, (size_t)v.n_bytes, 0);
  if (!ix.close() || !ok) sh.set(THM_ERR_IO, "cannot write " + index_path);
  st.write_s += secs(t1, Clock::now());
}

// the drain: sort, the sorted header, then window after window -- window k is written (from one of the sorter's two
// pinned sets) while the device gathers and deflates window k + 1
void Run::drain_sorted() {
  struct Write {  // one window on its way out, on a thread of its own
    Run* run;
    thm_bam_sorted_view v;
    uint64_t at = 0;
    bool ok = true;
    std::thread th;
    void go() {
      const auto t2 = Clock::now();
      ok = run->out.write_all((const char*)v.data, (size_t)v.n_bytes, at);
      run->st.write_s += secs(t2, Clock::now());
    }
    void join() {
      if (th.joinable()) th.join();
      if (!ok) run->sh.set(THM_ERR_IO, "short write");
      ok = true;
    }
  } wr;
  wr.run = this;
  thm_text t;
  const auto t0 = Clock::now();
  int drc = sh.step([&] { return (int)thm_bam_sorter_finish(sorter, nullptr); });
  st.format_s += secs(t0, Clock::now());
  if (drc != THM_OK) sh.set(drc, thm_last_error(aligners[0]));
  if (drc == THM_OK && thm_writer_header_sorted(ws[0], &t) == THM_OK) append(t);
  first_member_offset = out.off;
  while (drc == THM_OK && !sh.failed()) {
    thm_bam_sorted_view v;
    const auto t1 = Clock::now();
    drc = sh.step([&] { return (int)thm_bam_sorter_next(sorter, 0, 0, &v); });
    st.format_s += secs(t1, Clock::now());
    wr.join();  // the next call reuses the set the write before last came from
    if (drc != THM_OK) {
      sh.set(drc, thm_last_error(aligners[0]));
      break;
    }
    if (v.n_raw_bytes == 0) break;
    wr.v = v;
    wr.at = out.off;
    out.off += v.n_bytes;
    st.n_output_bytes += v.n_bytes;
    wr.th = std::thread(&Write::go, &wr);
  }
  wr.join();
}

// THM_QUANT=1: the tables of every aligner, merged by key on the host (counts summed, overhang maximum), as
// <output_path>.genes.tsv and <output_path>.junctions.tsv
int write_quant_tables(const thm_index* ix, thm_aligner* const* aligners, thm_quant* const* quants, uint32_t n, const std::string& output_path,
                       std::string& err) {
  std::vector<thm_quant_gene> genes;
  std::map<std::tuple<uint32_t, uint64_t, uint64_t, uint32_t>, thm_quant_junction> rows;  // (ref, start, end, reverse)
  for (uint32_t i = 0; i < n; i++) {
    thm_quant_view v;
    const int rc = thm_quant_fetch(quants[i], &v);
    if (rc != THM_OK) {
      err = thm_last_error(aligners[i]);
      return rc;
    }
    if (genes.empty()) genes.assign(v.n_genes, thm_quant_gene{0, 0, 0, 0});
    for (uint64_t g = 0; g < v.n_genes; g++) {
      genes[g].exonic_unique += v.genes[g].exonic_unique;
      genes[g].exonic_multi += v.genes[g].exonic_multi;
      genes[g].intronic_unique += v.genes[g].intronic_unique;
      genes[g].intronic_multi += v.genes[g].intronic_multi;
    }
    for (uint64_t k = 0; k < v.n_junctions; k++) {
      const thm_quant_junction& j = v.junctions[k];
      auto at = rows.emplace(std::make_tuple(j.ref_id, j.start, j.end, j.strand ? 0u : 1u), j);
      if (at.second) continue;
      thm_quant_junction& have = at.first->second;
      have.n_unique += j.n_unique;
      have.n_multi += j.n_multi;
      have.max_overhang = std::max(have.max_overhang, j.max_overhang);
    }
  }
  std::vector<std::pair<std::string, uint64_t>> sq;
  (void)thm::sq_of_name(ix, &sq);
  std::string g_text = "gene_id\tgene_name\texonic_unique\texonic_multi\tintronic_unique\tintronic_multi\n";
  for (size_t g = 0; g < genes.size(); g++) {
    const char *id = thm_index_gene_id(ix, (uint32_t)g), *name = thm_index_gene_name(ix, (uint32_t)g);
    g_text += std::string(id ? id : "") + "\t" + (name ? name : "") + "\t" + std::to_string(genes[g].exonic_unique) + "\t" + std::to_string(genes[g].exonic_multi) +
              "\t" + std::to_string(genes[g].intronic_unique) + "\t" + std::to_string(genes[g].intronic_multi) + "\n";
  }
  std::string j_text = "ref\tstart\tend\tstrand\tunique\tmulti\tmax_overhang\n";
  for (const auto& kv : rows) {
    const thm_quant_junction& j = kv.second;
    j_text += (j.ref_id < sq.size() ? sq[j.ref_id].first : std::string("*")) + "\t" + std::to_string(j.start + 1) + "\t" + std::to_string(j.end) + "\t" +
              (j.strand ? "+" : "-") + "\t" + std::to_string(j.n_unique) + "\t" + std::to_string(j.n_multi) + "\t" + std::to_string(j.max_overhang) + "\n";
  }
  const std::pair<std::string, const std::string*> files[2] = {{output_path + ".genes.tsv", &g_text}, {output_path + ".junctions.tsv", &j_text}};
  for (const auto& f : files) {
    Output o;
    const bool ok = o.open(f.first.c_str()) && o.write_all(f.second->data(), f.second->size(), 0);
    if (!o.close() || !ok) {
      err = "cannot write " + f.first;
      return THM_ERR_IO;
    }
  }
  return THM_OK;
}

// THM_COVERAGE: every track of every aligner, contig by contig, as <output_path>.cov.<track>.bedgraph.  The run lists of
// several aligners are merged by a sweep over the change points of all of them with the depths summed, so that abutting
// stretches of equal depth fuse: the files do not depend on how the reads were dealt.
int write_coverage_tracks(const thm_index* ix, thm_aligner* const* aligners, thm_coverage* const* coverages, uint32_t n, uint32_t cov_flags,
                          const std::string& output_path, std::string& err) {
  std::vector<std::pair<std::string, uint64_t>> sq;
  (void)thm::sq_of_name(ix, &sq);
  const bool stranded = cov_flags & THM_COV_STRANDED, multi = cov_flags & THM_COV_MULTI;
  std::vector<std::string> tracks;
  for (const char* cls : {"unique", "multi"}) {
    if (cls[0] == 'm' && !multi) continue;
    if (stranded) {
      tracks.push_back(std::string(cls) + ".fwd");
      tracks.push_back(std::string(cls) + ".rev");
    } else {
      tracks.push_back(cls);
    }
  }
  for (uint32_t k = 0; k < tracks.size(); k++) {
    std::string text;
    for (uint32_t s = 0; s < sq.size(); s++) {
      std::map<uint64_t, int64_t> step;  // position -> change of the summed depth there
      for (uint32_t i = 0; i < n; i++) {
        thm_cov_view v;
        const int rc = thm_coverage_fetch(coverages[i], k, s, 1, &v);
        if (rc != THM_OK) {
          err = thm_last_error(aligners[i]);
          return rc;
        }
        for (uint64_t r = 0; r < v.n_runs; r++) {
          step[v.runs[r].start] += (int64_t)v.runs[r].depth;
          step[v.runs[r].end] -= (int64_t)v.runs[r].depth;
        }
      }
      int64_t depth = 0;
      uint64_t from = 0;
      for (const auto& kv : step) {
        if (kv.second == 0) continue;  // two runs abut with equal depths: no change point
        if (depth) text += sq[s].first + "\t" + std::to_string(from) + "\t" + std::to_string(kv.first) + "\t" + std::to_string(depth) + "\n";
        depth += kv.second;
        from = kv.first;
      }
    }
    const std::string path = output_path + ".cov." + tracks[k] + ".bedgraph";
    Output o;
    const bool ok = o.open(path.c_str()) && o.write_all(text.data(), text.size(), 0);
    if (!o.close() || !ok) {
      err = "cannot write " + path;
      return THM_ERR_IO;
    }
  }
  return THM_OK;
}

// The summaries a run was asked for, one quant and one coverage per aligner and the one aligner's pileup and cells: they
// go when their owner does (or at free()), the cells first, then the pileup, the coverages, the quants, all before their
// aligners.
struct Summaries {
  std::vector<thm_quant*> quants;
  std::vector<thm_coverage*> coverages;
  thm_pileup* pileup = nullptr;
  thm_cells* cells = nullptr;
  Summaries() = default;
  Summaries(const Summaries&) = delete;
  Summaries& operator=(const Summaries&) = delete;
  ~Summaries() { free(); }
  void free() {
    thm_cells_free(cells);
    cells = nullptr;
    thm_pileup_free(pileup);
    for (thm_coverage* c : coverages) thm_coverage_free(c);
    for (thm_quant* q : quants) thm_quant_free(q);
    pileup = nullptr;
    coverages.clear();
    quants.clear();
  }
};

// THM_PILEUP: the sites of all contigs with min_alt events or more as <output_path>.pileup.tsv
int write_pileup_sites(const thm_index* ix, thm_aligner* a, thm_pileup* pileup, uint32_t min_alt, const std::string& output_path, std::string& err) {
  std::vector<std::pair<std::string, uint64_t>> sq;
  (void)thm::sq_of_name(ix, &sq);
  thm_pile_view v;
  const int rc = thm_pileup_fetch(pileup, 0, (uint32_t)sq.size(), min_alt, &v);
  if (rc != THM_OK) {
    err = thm_last_error(a);
    return rc;
  }
  std::string text = "#contig\tpos\tref\tdepth\tA\tC\tG\tT\tN\tdel\tins\n";
  for (uint64_t i = 0; i < v.n_sites; i++) {
    const thm_pile_site& s = v.sites[i];
    text += sq[s.ref_id].first + "\t" + std::to_string(s.pos + 1) + "\t" + (char)s.ref_base + "\t" + std::to_string(s.depth);
    for (int k = 0; k < 5; k++) text += "\t" + std::to_string(s.cnt[k]);
    text += "\t" + std::to_string(s.del) + "\t" + std::to_string(s.ins) + "\n";
  }
  const std::string path = output_path + ".pileup.tsv";
  Output o;
  const bool ok = o.open(path.c_str()) && o.write_all(text.data(), text.size(), 0);
  if (!o.close() || !ok) {
    err = "cannot write " + path;
    return THM_ERR_IO;
  }
  return THM_OK;
}

// THM_CELLS: the cells with min_umis molecules or more as <output_path>.cells.mtx, .cells.barcodes.tsv and
// .cells.features.tsv
int write_cells_matrix(const thm_index* ix, thm_aligner* a, thm_cells* cells, uint32_t min_umis, const std::string& output_path, std::string& err) {
  thm_cells_view v;
  const int rc = thm_cells_fetch(cells, min_umis, &v);
  if (rc != THM_OK) {
    err = thm_last_error(a);
    return rc;
  }
  std::string mtx = "%%MatrixMarket matrix coordinate integer general\n";
  mtx += std::to_string(ix->genes.size()) + " " + std::to_string(v.n_cells) + " " + std::to_string(v.n_entries) + "\n";
  for (uint64_t i = 0; i < v.n_entries; i++) {
    const thm_cell_entry& e = v.entries[i];
    mtx += std::to_string(e.gene + 1) + " " + std::to_string(e.cell + 1) + " " + std::to_string(e.n_umis) + "\n";
  }
  std::string barcodes;
  for (uint64_t i = 0; i < v.n_cells; i++) {
    char text[THM_CELLS_MAX_LEN];
    thm::cells::unpack_bases(v.cells[i].barcode, v.cb_len, text);
    barcodes.append(text, v.cb_len);
    barcodes += "\n";
  }
  std::string features;
  for (size_t g = 0; g < ix->genes.size(); g++) {
    const char *id = thm_index_gene_id(ix, (uint32_t)g), *name = thm_index_gene_name(ix, (uint32_t)g);
    features += std::string(id ? id : "") + "\t" + (name ? name : "") + "\tGene Expression\n";
  }
  const std::pair<const char*, const std::string*> files[3] = {{".cells.mtx", &mtx}, {".cells.barcodes.tsv", &barcodes}, {".cells.features.tsv", &features}};
  for (const auto& f : files) {
    const std::string path = output_path + f.first;
    Output o;
    const bool ok = o.open(path.c_str()) && o.write_all(f.second->data(), f.second->size(), 0);
    if (!o.close() || !ok) {
      err = "cannot write " + path;
      return THM_ERR_IO;
    }
  }
  return THM_OK;
}

}  // namespace

extern "C" int32_t thm_align_files_multi(thm_aligner* const* aligners, uint32_t n_aligners, const char* const* fastq_paths,
                                         uint32_t n_paths, const char* output_path, int32_t format, uint64_t batch_reads,
                                         uint32_t n_threads, thm_run_stats* stats) {
  if (!aligners || n_aligners == 0 || !fastq_paths || n_paths == 0 || !output_path) return THM_ERR_INVALID_ARG;
  for (uint32_t i = 0; i < n_paths; i++)
    if (!fastq_paths[i]) return THM_ERR_INVALID_ARG;
  for (uint32_t i = 0; i < n_aligners; i++)
    if (!aligners[i]) return THM_ERR_INVALID_ARG;
  if (batch_reads == 0) batch_reads = 250000;
  const Modes m = Modes::read(format);
  if (m.bam_sort && n_aligners > 1) {
    thm::set_global_error("thm_align_files_multi: THM_BAM_SORT=1 takes one aligner (merging across devices is not done)");
    return THM_ERR_INVALID_ARG;
  }
  if (m.bam_index && (!m.bam_sort || !strcmp(output_path, "-"))) {
    thm::set_global_error("thm_align_files_multi: THM_BAM_INDEX=1 needs THM_BAM_SORT=1 and an output file (only a sorted file has a .bai)");
    return THM_ERR_INVALID_ARG;
  }
  if (m.quant && !strcmp(output_path, "-")) {
    thm::set_global_error("thm_align_files_multi: THM_QUANT=1 needs an output file (the tables are written beside it)");
    return THM_ERR_INVALID_ARG;
  }
  if (m.coverage && !strcmp(output_path, "-")) {
    thm::set_global_error("thm_align_files_multi: THM_COVERAGE needs an output file (the tracks are written beside it)");
    return THM_ERR_INVALID_ARG;
  }
  if (m.pile_bad) {
    thm::set_global_error("thm_align_files_multi: THM_PILEUP must be 1 or 2 (or 0, or unset) and THM_PILEUP_MIN_ALT a number of 1 or more");
    return THM_ERR_INVALID_ARG;
  }
  if (m.pileup && !strcmp(output_path, "-")) {
    thm::set_global_error("thm_align_files_multi: THM_PILEUP needs an output file (the sites are written beside it)");
    return THM_ERR_INVALID_ARG;
  }
  if (m.pileup && n_aligners > 1) {
    thm::set_global_error("thm_align_files_multi: THM_PILEUP takes one aligner (merging across devices is not done)");
    return THM_ERR_INVALID_ARG;
  }
  if (m.cells_bad) {
    thm::set_global_error(
        "thm_align_files_multi: THM_CELLS must be 1 or 2 (or 0, or unset), THM_CELLS_CB_LEN and THM_CELLS_UMI_LEN numbers of 1..16 and THM_CELLS_MIN_UMIS a number of 1 or "
        "more");
    return THM_ERR_INVALID_ARG;
  }
  if (m.cells && !strcmp(output_path, "-")) {
    thm::set_global_error("thm_align_files_multi: THM_CELLS needs an output file (the matrix is written beside it)");
    return THM_ERR_INVALID_ARG;
  }
  if (m.cells && n_aligners > 1) {
    thm::set_global_error(
        "thm_align_files_multi: THM_CELLS takes one aligner (the tables of two devices hold reduced counts: their distinct molecules are those of the union of their rows, "
        "which is not formed)");
    return THM_ERR_INVALID_ARG;
  }
  const thm_index* ix = thm_aligner_index(aligners[0]);
  for (uint32_t i = 1; i < n_aligners; i++)
    if (thm_aligner_index(aligners[i]) != ix) {
      thm::set_global_error("thm_align_files_multi: the aligners must share one index");
      return THM_ERR_INVALID_ARG;
    }
  const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  if (n_threads == 0) n_threads = std::min(hw, 16u);
  // parser threads: a block parses at roughly 10 M records/s per thread; the rest of the budget formats
  const unsigned n_parsers = std::max(1u, std::min(4u, n_threads / 4));
  // ---- the writer, the output and the sorter
  thm_writer* w = nullptr;
  int rc = thm_writer_create(ix, format, n_threads, &w);
  if (rc != THM_OK) return rc;
  Output out;
  if (!out.open(output_path)) {
    thm_writer_free(w);
    thm::set_global_error(std::string("cannot create ") + output_path);
    return THM_ERR_IO;
  }
  thm_bam_sorter* sorter = nullptr;
  if (m.bam_sort && (rc = thm_bam_sorter_create(aligners[0], 0, &sorter)) != THM_OK) {
    (void)out.close();
    thm_writer_free(w);
    return rc;
  }
  Summaries sums;  // (frees what has been created on every return below)
  // a summary that `a` could not create: its message, and what stands so far goes
  const auto not_created = [&](thm_aligner* a) {
    thm::set_global_error(thm_last_error(a));
    sums.free();
    thm_bam_sorter_free(sorter);
    (void)out.close();
    thm_writer_free(w);
    return rc;
  };
  sums.quants.assign(m.quant ? n_aligners : 0, nullptr);
  for (size_t i = 0; i < sums.quants.size(); i++)
    if ((rc = thm_quant_create(aligners[i], &sums.quants[i])) != THM_OK) return not_created(aligners[i]);
  sums.coverages.assign(m.coverage ? n_aligners : 0, nullptr);
  for (size_t i = 0; i < sums.coverages.size(); i++)
    if ((rc = thm_coverage_create(aligners[i], m.cov_flags, 0, &sums.coverages[i])) != THM_OK) return not_created(aligners[i]);
  if (m.pileup && (rc = thm_pileup_create(aligners[0], m.pile_flags, 0, &sums.pileup)) != THM_OK) return not_created(aligners[0]);
  if (m.cells && (rc = thm_cells_create(aligners[0], m.cells_flags, m.cells_cb_len, m.cells_umi_len, 0, &sums.cells)) != THM_OK) return not_created(aligners[0]);
  const auto t_start = Clock::now();
  thm_writer* w2 = nullptr;
  const bool have_w2 = thm_writer_create(ix, format, n_threads, &w2) == THM_OK;
  if (!have_w2) w2 = nullptr;
  Run run(aligners, n_aligners, fastq_paths, n_paths, format, batch_reads, n_threads, n_parsers, m, w, w2 ? w2 : w, out, sorter);
  if (!have_w2) run.sh.set(THM_ERR_OOM, "cannot create the second writer object");
  run.index_path = std::string(output_path) + ".bai";
  if (m.quant) run.quants = sums.quants.data();
  if (m.coverage) run.coverages = sums.coverages.data();
  run.pileup = sums.pileup;
  run.cells = sums.cells;
  // ---- the stages: the cutter, the parsers, a thread per aligner; this thread formats
  std::thread cutter(&Run::cut, &run);
  std::vector<std::thread> parsers, gpus;
  for (unsigned k = 0; k < n_parsers; k++) parsers.emplace_back(&Run::parse, &run);
  for (uint32_t gi = 0; gi < n_aligners; gi++) gpus.emplace_back(&Run::gpu, &run, gi);
  run.format_and_write();
  cutter.join();
  for (auto& x : parsers) x.join();
  for (auto& x : gpus) x.join();
  // ---- tear down: every batch has been written, so the mappings go (inside wall_s, as they always were; the slots go
  // with the run, behind the clock)
  run.maps.clear();
  if (w2) thm_writer_free(w2);
  if (m.quant && run.sh.rc == THM_OK) {
    std::string err;
    const int qrc = run.sh.step([&] { return write_quant_tables(ix, aligners, sums.quants.data(), n_aligners, output_path, err); });
    if (qrc != THM_OK) run.sh.set(qrc, err);
  }
  if (m.coverage && run.sh.rc == THM_OK) {
    std::string err;
    const int crc = run.sh.step([&] { return write_coverage_tracks(ix, aligners, sums.coverages.data(), n_aligners, m.cov_flags, output_path, err); });
    if (crc != THM_OK) run.sh.set(crc, err);
  }
  if (m.pileup && run.sh.rc == THM_OK) {
    std::string err;
    const int prc = run.sh.step([&] { return write_pileup_sites(ix, aligners[0], sums.pileup, m.pile_min_alt, output_path, err); });
    if (prc != THM_OK) run.sh.set(prc, err);
  }
  if (m.cells && run.sh.rc == THM_OK) {
    std::string err;
    const int crc = run.sh.step([&] { return write_cells_matrix(ix, aligners[0], sums.cells, m.cells_min_umis, output_path, err); });
    if (crc != THM_OK) run.sh.set(crc, err);
  }
  sums.free();  // (in front of the sorter and the writer, and inside wall_s, as they always were)
  thm_bam_sorter_free(sorter);
  if (!out.close()) run.sh.set(THM_ERR_IO, std::string("error closing ") + output_path);
  thm_writer_free(w);
  run.st.wall_s = secs(t_start, Clock::now());
  if (stats) *stats = run.st;
  if (run.sh.rc != THM_OK) thm::set_global_error(run.sh.msg);
  return run.sh.rc;
}

extern "C" int32_t thm_align_files(thm_aligner* a, const char* const* fastq_paths, uint32_t n_paths, const char* output_path,
                                   int32_t format, uint64_t batch_reads, uint32_t n_threads, thm_run_stats* stats) {
  if (!a) return THM_ERR_INVALID_ARG;
  thm_aligner* one[1] = {a};
  return thm_align_files_multi(one, 1, fastq_paths, n_paths, output_path, format, batch_reads, n_threads, stats);
}
