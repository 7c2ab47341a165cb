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
// Records leave in input order whatever the number of GPUs.
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
#include <vector>

#include "inflate_device.h"
#include "io_internal.h"
#include "thermite_internal.h"

namespace {

using Clock = std::chrono::steady_clock;
double secs(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double>(b - a).count(); }

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
  std::vector<uint8_t> head;  // ... and the head it went up with (kept for the failed-read message)
  bool gzslice = false;     // a slice of the mapped plain-gzip input gz_map[0, gz_len) (THM_FASTQ_DEVICE=3): where it begins and
  const uint8_t* gz_map = nullptr;  // how long it is, is known at its turn in the chain of uploads only (file_first as above)
  size_t gz_len = 0;
  bool parsed = false;  // `reads` already holds the batch (sequential parser: FASTA, odd inputs)
  thm::HostBatch reads;
  thm_batch_view res;  // into the pinned result buffers of the aligner that ran it (two sets per aligner, used alternately)
  thm_bam_view bam;    // ... or, with THM_BAM_DEVICE=1, the BAM records encoded on the device (likewise two sets)
  thm_bgzf_view bgzf;  // ... or, with THM_BAM_DEVICE=2, their BGZF members deflated there (likewise)
  uint64_t bgzf_aligned = 0;  // reads of the batch with an alignment (the members do not show it)
  thm_bam_sort_info sorted;   // ... or, with THM_BAM_SORT=1, what adding them to the sorter reported (no bytes come back)
  uint64_t sorted_aligned = 0;
  bool aligned = false;
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
  bool cancel = false;
  double busy_s = 0;

  void run() {
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
  void start() {
    th = std::thread([this] { run(); });
  }
  int wait_kind() {
    std::unique_lock<std::mutex> g(mu);
    cv.wait(g, [&] { return kind >= 0; });
    return kind;
  }
  // the next block of the file (the last one holds no line, or an error); `old` goes back for reuse
  void next(Block& out, std::vector<char>& old) {
    std::unique_lock<std::mutex> g(mu);
    cv.wait(g, [&] { return !ready.empty(); });
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

// A gzip input that is BGZF throughout (THM_FASTQ_DEVICE=2): the mapping and its members.  Eligible: gzip magic, every
// member of the chain with the BGZF header (inflate_device.h, the rule the device takes), the chain ending exactly at the
// end of the file, and the first member, inflated on the host, beginning with '@'.
struct BgzfFile {
  const uint8_t* map = nullptr;
  size_t len = 0;
  std::vector<thm::inf::Member> tab;  // in_off - 12 - xlen is not kept: `at` below is
  std::vector<uint64_t> at;           // first byte of every member, and the file's length behind the last
  double bytes_per_read = 256;        // of the first member's text
  bool ok = false;
  BgzfFile() = default;
  BgzfFile(const BgzfFile&) = delete;
  BgzfFile& operator=(const BgzfFile&) = delete;
  ~BgzfFile() {
    if (map) munmap((void*)map, len);  // (a file the run did not get to; otherwise the mapping was handed on)
  }
  void open(const char* path) {
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0) return;
    struct stat st;
    if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size >= 28) {
      void* m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
      if (m != MAP_FAILED) {
        map = (const uint8_t*)m;
        len = (size_t)st.st_size;
      }
    }
    close(fd);
    if (!map) return;
    uint64_t p = 0, out = 0;
    bool good = true;
    while (p < len && good) {
      thm::inf::Member mb;
      uint64_t size = 0;
      good = thm::inf::walk_member(map, len, p, out, &mb, &size);
      if (!good) break;
      tab.push_back(mb);
      at.push_back(p);
      p += size;
      out += mb.isize;
    }
    at.push_back(p);
    if (good && !tab.empty()) {
      std::vector<uint8_t> first;
      std::string err;
      uint64_t cut = 0;
      // the first member with text decides: FASTA and anything else keep today's path
      size_t k = 0;
      while (k + 1 < tab.size() && tab[k].isize == 0) k++;
      if (thm::bgzf_block_on_host(nullptr, 0, map + at[k], at[k + 1] - at[k], path, true, first, &cut, err) == THM_OK && !first.empty() &&
          first[0] == '@' && k == 0) {
        size_t nl = 0;
        for (uint8_t c : first) nl += c == '\n';
        if (nl >= 4) bytes_per_read = (double)first.size() / (double)(nl / 4);
        ok = true;
      }
    }
    if (!ok) {
      munmap((void*)map, len);
      map = nullptr;
      tab.clear();
      at.clear();
    }
  }
};

// A gzip input that is not BGZF throughout (THM_FASTQ_DEVICE=3): the mapping.  Eligible: gzip magic, and the first
// bytes, inflated on the host, beginning with '@' (FASTA and anything else keep the inflater thread and its parser).
struct GzipFile {
  const uint8_t* map = nullptr;
  size_t len = 0;
  double bytes_per_read = 256, ratio = 4;  // of the first blocks' text
  bool ok = false;
  GzipFile() = default;
  GzipFile(const GzipFile&) = delete;
  GzipFile& operator=(const GzipFile&) = delete;
  ~GzipFile() {
    if (map) munmap((void*)map, len);  // (a file the run did not get to; otherwise the mapping was handed on)
  }
  void open(const char* path) {
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0) return;
    struct stat st;
    if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size >= 18) {
      void* m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
      if (m != MAP_FAILED) {
        map = (const uint8_t*)m;
        len = (size_t)st.st_size;
      }
    }
    close(fd);
    if (!map) return;
    // the first blocks that end inside 64 KiB, or inside 1 MiB
    for (size_t take = 65536; !ok; take *= 16) {
      const size_t n = std::min(take, len);
      std::unique_ptr<thm_gzip_state> zs(new thm_gzip_state());
      std::vector<uint8_t> first;
      std::string err;
      uint64_t used = 0;
      if (thm::GzInflater::inflate_slice(zs.get(), map, n, path, n == len, first, &used, err) != THM_OK) break;
      if (!first.empty()) {
        if (first[0] != '@') break;
        size_t nl = 0;
        for (uint8_t c : first) nl += c == '\n';
        if (nl >= 4) bytes_per_read = (double)first.size() / (double)(nl / 4);
        if (used) ratio = std::max(1.0, (double)first.size() / (double)used);
        ok = true;
      }
      if (n == len || take >= (1u << 20)) break;
    }
    if (!ok) {
      munmap((void*)map, len);
      map = nullptr;
    }
  }
};

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
  // Runs one step of a pipeline thread.  An exception (bad_alloc from a growing buffer, mostly) must not leave the
  // thread body: std::terminate would take the host process down, and a thread that simply stopped would leave the
  // others waiting on its queue.  The step's failure becomes the run's status and the thread goes on with its
  // hand-over protocol.
  template <class F>
  int step(F&& f) {
    try {
      return f();
    } catch (const std::bad_alloc&) {
      set(THM_ERR_OOM, "out of host memory in the file driver");
      return THM_ERR_OOM;
    } catch (const std::exception& e) {
      set(THM_ERR_INTERNAL, std::string("file driver: ") + e.what());
      return THM_ERR_INTERNAL;
    } catch (...) {
      set(THM_ERR_INTERNAL, "file driver: unknown exception");
      return THM_ERR_INTERNAL;
    }
  }
};

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
  // THM_BAM_DEVICE=1: BAM records are encoded on the device (thm_batch_fetch_bam) and only deflated here
  const char* bam_dev_env = getenv("THM_BAM_DEVICE");
  // THM_BAM_DEVICE=2: ... and BGZF-compressed there too (thm_batch_fetch_bgzf): the formatting stage passes bytes on
  // THM_BAM_SORT=1: the records of every batch stay on the device (thm_bam_sorter_add, uploads as with THM_BAM_DEVICE=1);
  // once the input is exhausted they are sorted there and leave window by window as finished members
  const char* bam_sort_env = getenv("THM_BAM_SORT");
  const bool bam_sort = format == THM_FMT_BAM && bam_sort_env && !strcmp(bam_sort_env, "1");
  if (bam_sort && n_aligners > 1) {
    thm::set_global_error("thm_align_files_multi: THM_BAM_SORT=1 takes one aligner (merging across devices is not done)");
    return THM_ERR_INVALID_ARG;
  }
  const bool bgzf_device = !bam_sort && format == THM_FMT_BAM && bam_dev_env && !strcmp(bam_dev_env, "2");
  const bool bam_device = bam_sort || bgzf_device || (format == THM_FMT_BAM && bam_dev_env && !strcmp(bam_dev_env, "1"));
  // THM_FASTQ_DEVICE=1, in those two modes only (the host needs no read bytes there): blocks of 4-line FASTQ go to the
  // device unparsed (thm_batch_upload_fastq)
  const char* fq_dev_env = getenv("THM_FASTQ_DEVICE");
  // THM_FASTQ_DEVICE=2: as =1, and input files that are BGZF throughout go to the device compressed
  // (thm_batch_upload_fastq_bgzf); every other file takes the path of =1
  // THM_FASTQ_DEVICE=3: as =2, and gzip files that are not BGZF throughout go to the device compressed too, in slices
  // (thm_batch_upload_fastq_gzip)
  const bool fastq_gzip = bam_device && fq_dev_env && !strcmp(fq_dev_env, "3");
  const bool fastq_bgzf = fastq_gzip || (bam_device && fq_dev_env && !strcmp(fq_dev_env, "2"));
  const bool fastq_device = fastq_bgzf || (bam_device && fq_dev_env && !strcmp(fq_dev_env, "1"));
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
  thm_writer* w = nullptr;
  int rc = thm_writer_create(ix, format, n_threads, &w);
  if (rc != THM_OK) return rc;
  const bool to_stdout = strcmp(output_path, "-") == 0;
  if (to_stdout) fflush(stdout);
  const int fo = to_stdout ? 1 : open(output_path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
  if (fo < 0) {
    thm_writer_free(w);
    thm::set_global_error(std::string("cannot create ") + output_path);
    return THM_ERR_IO;
  }
  // a regular file takes the chunks of a batch at their final offsets from several threads
  struct stat sb;
  const bool positional = !to_stdout && fstat(fo, &sb) == 0 && S_ISREG(sb.st_mode);
  uint64_t file_off = 0;
  auto write_all = [&](const char* p, size_t n, uint64_t off) -> bool {
    while (n) {
      const ssize_t k = positional ? pwrite(fo, p, n, (off_t)off) : write(fo, p, n);
      if (k <= 0) return false;
      p += k;
      n -= (size_t)k;
      off += (uint64_t)k;
    }
    return true;
  };

  thm_bam_sorter* sorter = nullptr;
  if (bam_sort && (rc = thm_bam_sorter_create(aligners[0], 0, &sorter)) != THM_OK) {
    if (!to_stdout) close(fo);
    thm_writer_free(w);
    return rc;
  }
  thm_run_stats st;
  memset(&st, 0, sizeof st);
  std::mutex st_mu;  // parse_s / gpu_s are summed by several threads
  const auto t_start = Clock::now();
  Shared sh;
  // every aligner keeps the results of its last two fetches: two batches per GPU may be between fetch and write,
  // one more is running; the parsers and the cutter work ahead of that
  const unsigned n_slots = 3 * n_aligners + n_parsers + 2;
  std::vector<Slot> slots(n_slots);
  Queue q_free, q_raw;
  for (auto& s : slots) q_free.push(&s);
  // parsed batches are handed to the GPU threads strictly in input order (parsers may finish out of order; an aligner
  // that ran ahead of a batch it would later have to wait for could block the writer for good)
  std::mutex par_mu;
  std::condition_variable par_cv;
  std::map<uint64_t, Slot*> parsed;
  uint64_t next_align = 0;
  bool parse_done = false;
  // finished batches, by sequence number, for the writer
  std::mutex done_mu;
  std::condition_variable done_cv;
  std::map<uint64_t, Slot*> done;
  uint64_t n_batches_cut = 0;  // set when the cutter has seen the end of the input
  bool cut_done = false;
  uint64_t n_written = 0;  // batches the writer has finished (guarded by done_mu)

  // THM_FASTQ_DEVICE=2: the chain of tails.  Every slot of such a run takes its turn in input order for its upload (a
  // slot that is not BGZF only passes the turn on); the holder of the turn alone touches ch_tail and ch_line.  The
  // bytes and reads of the batches so far size the next groups.
  std::mutex ch_mu;
  std::condition_variable ch_cv;
  uint64_t ch_turn = 0;
  std::vector<uint8_t> ch_tail;
  uint64_t ch_line = 1;
  std::atomic<uint64_t> est_bytes{0}, est_reads{0};
  // THM_FASTQ_DEVICE=3: where the plain-gzip file of the turn stands (the holder of the turn alone touches them), and
  // what the cutter waits for before it cuts the next slot of that file: the upload that tells whether there is one
  std::unique_ptr<thm_gzip_state> gz_state(new thm_gzip_state());
  uint64_t gz_pos = 0, gz_in = 0, gz_out = 0;  // the position in the file; compressed and inflated bytes so far, for the ratio
  bool gz_file_done = false;                   // (guarded by ch_mu)
  std::vector<std::pair<const char*, size_t>> maps;
  // ---- stage 1: cut the input into blocks of whole records ----
  std::thread cutter([&] {
    uint64_t seq = 0;
    // gzip inputs get an inflater thread each (Ahead), those of the next few files running ahead of their turn
    std::vector<std::unique_ptr<Ahead>> ahead(n_paths);
    std::vector<char> is_gz(n_paths, 0);
    std::vector<std::unique_ptr<BgzfFile>> bgzf_files(n_paths);
    std::vector<std::unique_ptr<GzipFile>> gzip_files(n_paths);
    unsigned n_gz = 0;
    for (uint32_t pi = 0; pi < n_paths; pi++) {
      unsigned char magic[2] = {0, 0};
      const int fd = open(fastq_paths[pi], O_RDONLY);
      if (fd >= 0) {
        is_gz[pi] = pread(fd, magic, 2, 0) == 2 && magic[0] == 0x1f && magic[1] == 0x8b;
        close(fd);
      }
      if (is_gz[pi] && fastq_bgzf) {  // eligible: no inflater thread, the file is cut by its members
        const auto t0 = Clock::now();
        (void)sh.step([&] {
          std::unique_ptr<BgzfFile> bf(new BgzfFile());
          bf->open(fastq_paths[pi]);
          if (bf->ok) {
            bgzf_files[pi] = std::move(bf);
            is_gz[pi] = 0;
          } else if (fastq_gzip) {  // ... or in slices, wherever its blocks end
            std::unique_ptr<GzipFile> gf(new GzipFile());
            gf->open(fastq_paths[pi]);
            if (gf->ok) {
              gzip_files[pi] = std::move(gf);
              is_gz[pi] = 0;
            }
          }
          return THM_OK;
        });
        std::lock_guard<std::mutex> g(st_mu);
        st.parse_s += secs(t0, Clock::now());
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
        ahead[k]->path = fastq_paths[k];
        ahead[k]->batch_reads = batch_reads;
        ahead[k]->budget = ahead_bytes / ahead_files;
        ahead[k]->start();
      }
    };
    for (uint32_t pi = 0; pi < n_paths && !sh.failed(); pi++) {
      thm_fastq* r = nullptr;
      Ahead* ah = nullptr;
      int prc = THM_OK;
      bool fast = false;
      if (sh.step([&] { top_up(pi); return THM_OK; }) != THM_OK) break;
      if (bgzf_files[pi]) {
        // groups of whole members of about batch_reads reads, by the bytes per record of the batches so far
        BgzfFile& bf = *bgzf_files[pi];
        const size_t nm = bf.tab.size();
        for (size_t k = 0; k < nm && !sh.failed();) {
          Slot* s = q_free.pop();
          const uint64_t eb = est_bytes.load(), er = est_reads.load();
          const double per = er >= 64 ? (double)eb / (double)er : bf.bytes_per_read;
          const double want = per * (double)batch_reads;
          size_t k1 = k;
          double have_bytes = 0;
          do have_bytes += bf.tab[k1++].isize;
          while (k1 < nm && have_bytes < want);
          s->seq = seq++;
          s->parsed = false;
          s->aligned = false;
          s->zmembers = true;
          s->gzslice = false;
          s->file_first = k == 0;
          s->path = fastq_paths[pi];
          s->raw_ptr = (const char*)bf.map + bf.at[k];
          s->raw_len = (size_t)(bf.at[k1] - bf.at[k]);
          s->last_block = k1 == nm;
          s->first_line = 0;
          k = k1;
          q_raw.push(s);
        }
        maps.emplace_back((const char*)bf.map, bf.len);  // unmapped when every batch has been written
        bf.map = nullptr;
        continue;
      }
      if (gzip_files[pi]) {
        // one slot after the other: where a slice begins is known once the one before has gone up
        GzipFile& gf = *gzip_files[pi];
        for (bool first = true, more = true; more && !sh.failed(); first = false) {
          Slot* s = q_free.pop();
          s->seq = seq++;
          s->parsed = false;
          s->aligned = false;
          s->zmembers = false;
          s->gzslice = true;
          s->file_first = first;
          s->path = fastq_paths[pi];
          s->gz_map = gf.map;
          s->gz_len = gf.len;
          s->raw_ptr = nullptr;
          s->raw_len = 0;
          s->last_block = false;
          s->first_line = 0;
          if (first) {
            std::lock_guard<std::mutex> g(ch_mu);
            gz_file_done = false;
          }
          const uint64_t mine = s->seq;
          q_raw.push(s);
          std::unique_lock<std::mutex> g(ch_mu);
          ch_cv.wait(g, [&] { return ch_turn > mine; });
          more = !gz_file_done;
        }
        maps.emplace_back((const char*)gf.map, gf.len);  // unmapped when every batch has been written
        gf.map = nullptr;
        continue;
      }
      if (is_gz[pi]) {
        ah = ahead[pi].get();
        const int kind = ah->wait_kind();
        if (kind == 2) {
          sh.set(ah->open_rc, ah->open_err);
          break;
        }
        fast = kind == 1;
        r = ah->r;  // (the sequential parser's, when the file is not 4-line FASTQ: the inflater thread has left)
      } else {
        prc = thm_fastq_open(fastq_paths[pi], &r);
        if (prc != THM_OK) {
          sh.set(prc, thm_last_error(nullptr));
          break;
        }
        fast = thm::fastq_is_plain_fastq(r);
      }
      // a plain (not gzip) FASTQ file is mapped and cut in place: a block is a range of the mapping
      const char* map = nullptr;
      size_t map_len = 0, map_pos = 0;
      uint64_t map_line = 1;
      if (fast) {
        unsigned char magic[2] = {0, 0};
        const int fd = open(fastq_paths[pi], O_RDONLY);
        struct stat ms;
        if (fd >= 0 && fstat(fd, &ms) == 0 && S_ISREG(ms.st_mode) && ms.st_size > 0 && pread(fd, magic, 2, 0) == 2 &&
            !(magic[0] == 0x1f && magic[1] == 0x8b)) {
          void* m = mmap(nullptr, (size_t)ms.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
          if (m != MAP_FAILED) {
            map = (const char*)m;
            map_len = (size_t)ms.st_size;
            (void)madvise(m, map_len, MADV_SEQUENTIAL);
          }
        }
        if (fd >= 0) close(fd);
      }
      auto count_nl = [](const char* p, size_t n) {
        size_t c = 0;
        for (size_t i = 0; i < n; i++) c += p[i] == '\n';
        return c;
      };
      for (;;) {
        Slot* s = q_free.pop();
        s->seq = seq;
        s->parsed = false;
        s->zmembers = false;
        s->gzslice = false;
        s->aligned = false;
        s->path = fastq_paths[pi];
        const auto t0 = Clock::now();
        uint64_t n_lines = 0;
        s->raw_ptr = nullptr;
        if (map) {
          // the position behind the (4 x batch_reads)-th newline from map_pos, found a span at a time
          const uint64_t want = batch_reads * 4;
          size_t p0 = map_pos, p = map_pos;
          while (p < map_len && n_lines < want) {
            const size_t span = std::min<size_t>(map_len - p, 1u << 20);
            const size_t nl = count_nl(map + p, span);
            if (n_lines + nl < want) {
              n_lines += nl;
              p += span;
              continue;
            }
            const char* q = map + p;
            while (n_lines < want) {
              q = (const char*)memchr(q, '\n', (size_t)(map + p + span - q)) + 1;
              n_lines++;
            }
            p = (size_t)(q - map);
          }
          if (p == map_len && p > p0 && map[p - 1] != '\n') n_lines++;
          s->raw_ptr = map + p0;
          s->raw_len = p - p0;
          s->last_block = p == map_len;
          s->first_line = map_line;
          map_line += n_lines;
          map_pos = p;
          prc = THM_OK;
        } else if (fast && ah) {
          Ahead::Block b;
          ah->next(b, s->raw);
          s->raw.swap(b.raw);
          s->raw_len = b.raw_len;
          s->first_line = b.first_line;
          s->last_block = b.last_block;
          n_lines = b.n_lines;
          prc = b.rc;
          if (prc != THM_OK) thm::set_global_error(b.err);
          s->raw_ptr = s->raw.data();
        } else if (fast) {
          prc = sh.step([&] { return thm::fastq_next_raw_block(r, batch_reads, s->raw, s->raw_len, n_lines, s->first_line, s->last_block); });
          s->raw_ptr = s->raw.data();
        } else {  // FASTA and anything that is not plain 4-line FASTQ: the sequential parser
          prc = sh.step([&] { return thm::fastq_fill(r, batch_reads, s->reads); });
          s->parsed = true;
          n_lines = s->reads.n_reads();
        }
        if (!(fast && ah)) {  // (an inflater thread counts its own time)
          std::lock_guard<std::mutex> g(st_mu);
          st.parse_s += secs(t0, Clock::now());
        }
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
        std::lock_guard<std::mutex> g(st_mu);
        st.parse_s += ah->busy_s;
      } else {
        thm_fastq_close(r);
      }
      if (map) maps.emplace_back(map, map_len);  // unmapped when every batch has been written
    }
    for (auto& a : ahead)
      if (a) a->stop();  // (inflaters started ahead of a run that failed)
    {
      std::lock_guard<std::mutex> g(done_mu);
      n_batches_cut = seq;
      cut_done = true;
    }
    done_cv.notify_all();
    for (unsigned k = 0; k < n_parsers; k++) q_raw.push(nullptr);
  });

  // ---- stage 2: parse blocks (several threads) ----
  std::vector<std::thread> parsers;
  std::mutex parsers_mu;
  unsigned parsers_left = n_parsers;
  for (unsigned k = 0; k < n_parsers; k++)
    parsers.emplace_back([&] {
      for (;;) {
        Slot* s = q_raw.pop();
        if (!s) break;
        if (!s->parsed && !fastq_device && !sh.failed()) {  // (with THM_FASTQ_DEVICE the block passes through as it is)
          const auto t0 = Clock::now();
          std::string err;
          const int prc = sh.step([&] { return thm::fastq_parse_block(s->raw_ptr, s->raw_len, s->path, s->first_line, s->last_block, s->reads, err); });
          {
            std::lock_guard<std::mutex> g(st_mu);
            st.parse_s += secs(t0, Clock::now());
          }
          if (prc != THM_OK) sh.set(prc, err);
        }
        {
          std::lock_guard<std::mutex> g(par_mu);
          parsed[s->seq] = s;
        }
        par_cv.notify_all();
      }
      std::lock_guard<std::mutex> g(parsers_mu);
      if (--parsers_left == 0) {
        {
          std::lock_guard<std::mutex> g2(par_mu);
          parse_done = true;
        }
        par_cv.notify_all();
      }
    });

  // ---- stage 3: one thread per aligner ----
  std::vector<std::thread> gpus;
  for (uint32_t gi = 0; gi < n_aligners; gi++)
    gpus.emplace_back([&, gi] {
      thm_aligner* a = aligners[gi];
      std::deque<uint64_t> fetched;  // sequence numbers of this aligner's fetched batches, oldest first
      for (;;) {
        Slot* s = nullptr;
        {
          std::unique_lock<std::mutex> g(par_mu);
          par_cv.wait(g, [&] { return parsed.count(next_align) || (parse_done && parsed.empty()); });
          auto it = parsed.find(next_align);
          if (it == parsed.end()) break;
          s = it->second;
          parsed.erase(it);
          next_align++;
        }
        par_cv.notify_all();
        // a raw block goes up as it is and is parsed there; the slot keeps its bytes (its own buffer, or the mapping,
        // which lives until every batch is written) until it is released behind the write
        const bool raw_up = fastq_device && !s->parsed;
        bool have = !sh.failed() && (raw_up || s->reads.n_reads() != 0);  // (a blank tail cut into a block of its own holds no read)
        const auto t0 = Clock::now();
        int up_rc = THM_OK;
        if (fastq_bgzf) {  // this slot's turn in the chain of uploads
          std::unique_lock<std::mutex> g(ch_mu);
          ch_cv.wait(g, [&] { return ch_turn == s->seq; });
        }
        if (s->zmembers) {
          if (s->file_first) {
            ch_tail.clear();
            ch_line = 1;
          }
          s->first_line = ch_line;
          if (have) {
            thm_fastq_bgzf_info zi;
            memset(&zi, 0, sizeof zi);
            up_rc = sh.step([&] {
              s->head = ch_tail;
              const int r2 = (int)thm_batch_upload_fastq_bgzf(a, s->head.data(), s->head.size(), (const uint8_t*)s->raw_ptr, s->raw_len,
                                                              s->path.c_str(), s->first_line, s->last_block ? 1 : 0, &zi);
              if (r2 == THM_OK) {
                ch_tail.assign(zi.tail, zi.tail + zi.tail_len);
                ch_line += zi.n_lines;
                est_bytes += s->head.size() + zi.n_inflated_bytes - zi.tail_len;
                est_reads += zi.n_reads;
              }
              return r2;
            });
            if (up_rc == THM_OK && zi.n_reads == 0) have = false;  // (a group without a whole record: all of it is tail)
          }
        }
        if (s->gzslice) {
          if (s->file_first) {
            ch_tail.clear();
            ch_line = 1;
            memset(gz_state.get(), 0, sizeof(thm_gzip_state));
            gz_pos = gz_in = gz_out = 0;
          }
          s->first_line = ch_line;
          bool file_done = !have;  // (a run that has failed cuts no further slot)
          if (have) {
            thm_fastq_gzip_info zi;
            memset(&zi, 0, sizeof zi);
            // a slice of about batch_reads reads, by the bytes per record and the ratio of the batches so far; doubled
            // while no block ends inside it
            const uint64_t eb = est_bytes.load(), er = est_reads.load();
            const double per = er >= 64 ? (double)eb / (double)er : 256.0;
            const double ratio = gz_in >= 65536 ? std::max(1.0, (double)gz_out / (double)gz_in) : 4.0;
            uint64_t want = (uint64_t)(per * (double)batch_reads / ratio) + 4096;
            up_rc = sh.step([&] {
              s->head = ch_tail;
              for (;;) {
                const uint64_t left = s->gz_len - gz_pos, n = std::min<uint64_t>(want, left);
                s->last_block = n == left;
                const int r2 = (int)thm_batch_upload_fastq_gzip(a, gz_state.get(), s->head.data(), s->head.size(), s->gz_map + gz_pos, n,
                                                                s->path.c_str(), s->first_line, s->last_block ? 1 : 0, &zi);
                if (r2 != THM_OK) return r2;
                if (zi.n_consumed_bytes == 0 && !s->last_block) {
                  want = 2 * n;
                  continue;
                }
                gz_pos += zi.n_consumed_bytes;
                gz_in += zi.n_consumed_bytes;
                gz_out += zi.n_inflated_bytes;
                ch_tail.assign(zi.tail, zi.tail + zi.tail_len);
                ch_line += zi.n_lines;
                est_bytes += s->head.size() + zi.n_inflated_bytes - zi.tail_len;
                est_reads += zi.n_reads;
                return (int)THM_OK;
              }
            });
            file_done = up_rc != THM_OK || s->last_block;
            if (up_rc == THM_OK && zi.n_reads == 0) have = false;  // (a slice without a whole record: all of it is tail)
          }
          std::lock_guard<std::mutex> g(ch_mu);
          gz_file_done = file_done;
        }
        if (fastq_bgzf) {
          {
            std::lock_guard<std::mutex> g(ch_mu);
            ch_turn = s->seq + 1;
          }
          ch_cv.notify_all();
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
            int g2 = raw_up ? up_rc : bam_device ? thm_batch_upload_reads(a, &rb) : thm_batch_upload(a, rb.bases, rb.offsets, rb.n_reads);
            if (g2 == THM_OK) g2 = thm_batch_run(a);
            if (g2 == THM_OK) g2 = thm_batch_sync(a);
            return g2;
          });
          const auto t1 = Clock::now();
          // the fetch below reuses the buffers of this aligner's second-last fetch: that batch must have been written
          if (grc == THM_OK && fetched.size() >= 2) {
            const uint64_t must = fetched[fetched.size() - 2];
            std::unique_lock<std::mutex> g(done_mu);
            done_cv.wait(g, [&] { return n_written > must || sh.failed(); });
          }
          const auto t2 = Clock::now();
          if (grc == THM_OK) grc = sh.step([&] {
            if (bam_sort) return thm::bam_sorter_add(sorter, 0, &s->sorted, &s->sorted_aligned);
            if (!bgzf_device) return bam_device ? thm_batch_fetch_bam(a, 0, &s->bam) : thm_batch_fetch(a, &s->res);
            return thm::batch_fetch_bgzf(a, 0, &s->bgzf, &s->bgzf_aligned);
          });
          const uint64_t n_res = bam_sort ? s->sorted.n_reads : bgzf_device ? s->bgzf.n_reads : bam_device ? s->bam.n_reads : s->res.n_reads;
          const int32_t* res_status = bam_sort ? s->sorted.read_status
                                      : bgzf_device ? s->bgzf.read_status : bam_device ? s->bam.read_status : s->res.read_status;
          if (grc == THM_OK && (bam_sort ? s->sorted.n_failed_reads
                                : bgzf_device ? s->bgzf.n_failed_reads : bam_device ? s->bam.n_failed_reads : s->res.n_failed_reads)) {
            // the reference aligns every read or panics; a read this build cannot take fails the run, by name
            uint64_t bad = 0;
            while (bad < n_res && res_status[bad] == THM_OK) bad++;
            thm_read_batch up;  // (the batch as it stands on the device: the host has not seen a byte of a gzip slice)
            memset(&up, 0, sizeof up);
            if (raw_up && s->gzslice) {
              (void)sh.step([&] { return (int)thm_batch_fetch_reads(a, &up); });
            } else if (raw_up && s->zmembers) {  // ... inflate and parse that one block here, for the one message
              std::string perr;
              (void)sh.step([&] {
                std::vector<uint8_t> blk;
                uint64_t cut = 0;
                int r2 = thm::bgzf_block_on_host(s->head.data(), s->head.size(), (const uint8_t*)s->raw_ptr, s->raw_len, s->path, s->last_block, blk, &cut, perr);
                if (r2 == THM_OK) r2 = thm::fastq_parse_block((const char*)blk.data(), (size_t)cut, s->path, s->first_line, s->last_block, s->reads, perr);
                return r2;
              });
            } else if (raw_up) {  // the host has not seen the names of this block: parse it now, for the one message
              std::string perr;
              (void)sh.step([&] { return thm::fastq_parse_block(s->raw_ptr, s->raw_len, s->path, s->first_line, s->last_block, s->reads, perr); });
            }
            const thm_read_batch v = raw_up && s->gzslice ? up : s->reads.view();
            std::string name;
            if (bad < v.n_reads) name.assign((const char*)v.names + v.name_off[bad], (size_t)(v.name_off[bad + 1] - v.name_off[bad]));
            sh.set(res_status[bad], "read " + name + (res_status[bad] == THM_ERR_UNSUPPORTED
                                                           ? ": longer than 65535 bases, or its DP trace exceeds the device-memory budget"
                                                           : ": hits a condition that panics in the reference (lift_mem_to_tx / lift_tx_to_gx)"));
            grc = res_status[bad];
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
            st.n_reads += n_res;
            st.n_batches += 1;
          }
        }
        {
          std::lock_guard<std::mutex> g(done_mu);
          done[s->seq] = s;
        }
        done_cv.notify_all();
      }
    });

  // ---- stage 4: format (this thread, on the formatting threads of the writer) and write (one more thread), in input
  // order; two writer objects are used alternately, so that batch k + 1 is formatted while batch k is written ----
  {
    // two writer objects, used alternately: the chunks of batch k are views into writer k & 1 and are still being
    // written while batch k + 1 is formatted, so one object cannot stand in for both
    thm_writer* w2 = nullptr;
    if (thm_writer_create(ix, format, n_threads, &w2) != THM_OK) {
      w2 = nullptr;
      sh.set(THM_ERR_OOM, "cannot create the second writer object");
    }
    thm_writer* ws[2] = {w, w2 ? w2 : w};  // (after a failure nothing is formatted any more: sh.failed())
    struct WriteJob {
      Slot* s = nullptr;
      uint64_t seq = 0;
      std::vector<const std::string*> chunks;
      std::vector<std::pair<const char*, size_t>> spans;  // what is written: the chunks, or the members of a thm_bgzf_view
      std::vector<uint64_t> at;
      bool stop = false;
    };
    std::mutex wj_mu;
    std::condition_variable wj_cv;
    std::deque<WriteJob*> wj_q;
    WriteJob jobs[2];
    bool job_busy[2] = {false, false};
    thm_text t;
    // (a sorted file's header is written when the drain begins)
    if (!bam_sort && thm_writer_header(w, &t) == THM_OK && t.len) {
      if (!write_all((const char*)t.data, t.len, file_off)) sh.set(THM_ERR_IO, "short write");
      file_off += t.len;
      st.n_output_bytes += t.len;
    }
    auto release = [&](Slot* s, uint64_t seq) {
      {
        std::lock_guard<std::mutex> g(done_mu);
        n_written = seq + 1;
      }
      done_cv.notify_all();
      q_free.push(s);
    };
    std::thread wthread([&] {
      for (;;) {
        WriteJob* j;
        {
          std::unique_lock<std::mutex> g(wj_mu);
          wj_cv.wait(g, [&] { return !wj_q.empty(); });
          j = wj_q.front();
          wj_q.pop_front();
        }
        if (j->stop) break;
        const auto t1 = Clock::now();
        std::vector<char> good(j->spans.size(), 1);
        auto put = [&](size_t c) { good[c] = write_all(j->spans[c].first, j->spans[c].second, j->at[c]) ? 1 : 0; };
        if (positional && j->spans.size() > 1) {
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
        release(j->s, j->seq);
        {
          std::lock_guard<std::mutex> g(wj_mu);
          job_busy[j - jobs] = false;
        }
        wj_cv.notify_all();
      }
    });
    for (uint64_t next = 0;; next++) {
      Slot* s = nullptr;
      {
        std::unique_lock<std::mutex> g(done_mu);
        done_cv.wait(g, [&] { return done.count(next) || (cut_done && next >= n_batches_cut); });
        auto it = done.find(next);
        if (it == done.end()) break;  // the input is exhausted
        s = it->second;
        done.erase(it);
      }
      const int k = (int)(next & 1);
      {  // the writer object (and job) of this parity: its previous batch must have left
        std::unique_lock<std::mutex> g(wj_mu);
        wj_cv.wait(g, [&] { return !job_busy[k]; });
      }
      bool queued = false;
      if (!sh.failed() && s->aligned && bam_sort) {
        // nothing leaves before the input is exhausted: the batch is in the sorter
        st.n_aligned_reads += s->sorted_aligned;
        st.n_records += s->sorted.n_records;
      } else if (!sh.failed() && s->aligned) {
        const auto t0 = Clock::now();
        const thm_read_batch rb = s->reads.view();
        const thm_batch_view& v = s->res;
        WriteJob& j = jobs[k];
        const thm_bam_view& bv = s->bam;
        const int wrc = sh.step([&] {
          // nothing to format: the members leave as one chunk, written from the aligner's pinned set (the GPU thread
          // waits for this batch to be written before the fetch that reuses the set)
          if (bgzf_device) return (int)THM_OK;
          return bam_device ? thm::writer_wrap_bam_chunks(ws[k], &bv, j.chunks) : thm::writer_format_chunks(ws[k], &rb, &v, j.chunks);
        });
        st.format_s += secs(t0, Clock::now());
        if (wrc != THM_OK) {
          sh.set(wrc, thm_last_error(nullptr));
        } else {
          j.spans.clear();
          if (bgzf_device) j.spans.emplace_back((const char*)s->bgzf.data, (size_t)s->bgzf.n_bytes);
          else
            for (const std::string* c : j.chunks) j.spans.emplace_back(c->data(), c->size());
          j.at.resize(j.spans.size());
          for (size_t c = 0; c < j.spans.size(); c++) {
            j.at[c] = file_off;
            file_off += j.spans[c].second;
            st.n_output_bytes += j.spans[c].second;
          }
          if (bgzf_device) {
            st.n_aligned_reads += s->bgzf_aligned;
            st.n_records += s->bgzf.n_records;
          } else if (bam_device) {
            // a read is unmapped when its first record carries flag 4 (bytes 18 .. 19 of the record)
            for (uint64_t r = 0; r < bv.n_reads; r++) st.n_aligned_reads += !(bv.data[bv.read_rec_off[r] + 18] & 4);
            st.n_records += bv.n_records;
          } else {
            for (uint64_t r = 0; r < v.n_reads; r++) {
              const uint64_t kk = v.read_aln_off[r + 1] - v.read_aln_off[r];
              st.n_aligned_reads += kk != 0;
              st.n_records += kk ? kk : (format == THM_FMT_PAF ? 0 : 1);
            }
          }
          j.s = s;
          j.seq = next;
          {
            std::lock_guard<std::mutex> g(wj_mu);
            job_busy[k] = true;
            wj_q.push_back(&j);
          }
          wj_cv.notify_all();
          queued = true;
        }
      }
      if (!queued) {
        // nothing to write for this batch: it still leaves in order behind the writes that are queued
        std::unique_lock<std::mutex> g(wj_mu);
        wj_cv.wait(g, [&] { return !job_busy[0] && !job_busy[1]; });
        g.unlock();
        release(s, next);
      }
    }
    {
      std::unique_lock<std::mutex> g(wj_mu);
      wj_cv.wait(g, [&] { return !job_busy[0] && !job_busy[1]; });
    }
    WriteJob stop;
    stop.stop = true;
    {
      std::lock_guard<std::mutex> g(wj_mu);
      wj_q.push_back(&stop);
    }
    wj_cv.notify_all();
    wthread.join();
    if (bam_sort && !sh.failed()) {
      // the drain: sort, the sorted header, then window after window -- window k is written (from one of the sorter's two
      // pinned sets) while the device gathers and deflates window k + 1
      const auto t0 = Clock::now();
      int drc = sh.step([&] { return (int)thm_bam_sorter_finish(sorter, nullptr); });
      st.format_s += secs(t0, Clock::now());
      if (drc != THM_OK) sh.set(drc, thm_last_error(aligners[0]));
      if (drc == THM_OK && thm_writer_header_sorted(w, &t) == THM_OK && t.len) {
        if (!write_all((const char*)t.data, t.len, file_off)) sh.set(THM_ERR_IO, "short write");
        file_off += t.len;
        st.n_output_bytes += t.len;
      }
      std::thread wr;
      bool wrote = true;
      while (drc == THM_OK && !sh.failed()) {
        thm_bam_sorted_view v;
        const auto t1 = Clock::now();
        drc = sh.step([&] { return (int)thm_bam_sorter_next(sorter, 0, 0, &v); });
        st.format_s += secs(t1, Clock::now());
        if (wr.joinable()) wr.join();  // the next call reuses the set the write before last came from
        if (!wrote) sh.set(THM_ERR_IO, "short write");
        if (drc != THM_OK) {
          sh.set(drc, thm_last_error(aligners[0]));
          break;
        }
        if (v.n_raw_bytes == 0) break;
        const uint64_t at = file_off;
        file_off += v.n_bytes;
        st.n_output_bytes += v.n_bytes;
        wr = std::thread([&, v, at] {
          const auto t2 = Clock::now();
          wrote = write_all((const char*)v.data, (size_t)v.n_bytes, at);
          st.write_s += secs(t2, Clock::now());
        });
      }
      if (wr.joinable()) wr.join();
      if (!wrote) sh.set(THM_ERR_IO, "short write");
    }
    if (!sh.failed() && thm_writer_trailer(w, &t) == THM_OK && t.len) {
      if (!write_all((const char*)t.data, t.len, file_off)) sh.set(THM_ERR_IO, "short write");
      file_off += t.len;
      st.n_output_bytes += t.len;
    }
    if (w2) thm_writer_free(w2);
  }
  cutter.join();
  for (auto& m : maps) munmap((void*)m.first, m.second);
  for (auto& x : parsers) x.join();
  for (auto& x : gpus) x.join();
  thm_bam_sorter_free(sorter);
  bool ok = true;
  if (!to_stdout) ok = close(fo) == 0;
  if (!ok) sh.set(THM_ERR_IO, std::string("error closing ") + output_path);
  thm_writer_free(w);
  st.wall_s = secs(t_start, Clock::now());
  if (stats) *stats = st;
  if (sh.rc != THM_OK) thm::set_global_error(sh.msg);
  return sh.rc;
}

extern "C" int32_t thm_align_files(thm_aligner* a, const char* const* fastq_paths, uint32_t n_paths, const char* output_path,
                                   int32_t format, uint64_t batch_reads, uint32_t n_threads, thm_run_stats* stats) {
  if (!a) return THM_ERR_INVALID_ARG;
  thm_aligner* one[1] = {a};
  return thm_align_files_multi(one, 1, fastq_paths, n_paths, output_path, format, batch_reads, n_threads, stats);
}
