// The rules of the device gzip inflater (thermite_amd/csrc/gzip_device.h) run serially on the host, in the order of
// gzip.hip and kernels_gzip.hip: search per chunk, decode per run, chain, resolve per tile, verify -- every
// lane-parallel phase as a loop over the 64 lanes, what the kernels compute without a device.
//   gzip_model_main <chunk_bytes> <slice_bytes> <last> <in: a gzip file> <out> [<in> <out> ...]
// The file goes through in calls of slice_bytes compressed bytes (0: the whole file in one), each beginning where the
// last one's n_consumed ended with the state it left, a slice doubled when nothing of it was consumed; the call that
// reaches the end of the file has last_block = <last>.  <out> receives the inflated bytes of all calls, <out>.log one
// line of text per call
//   "call <status> <bad> <n> <last_block> <n_out> <n_consumed> <n_chunks> <n_starts> <n_refused> <n_ends> <flags> <paths>\n"
// (the model has no host inflater behind it: a status other than 0 ends the file's run), and <out>.states the state
// after every call that ended with status 0, as the bytes of the struct.
// Buffers are allocated to the byte (the input to the next multiple of 4: the reader takes whole words), so that a read
// or write beyond them is one the sanitizers see.  tests/test_gzip_device_host.py builds and runs it plainly and as
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Ithermite_amd/csrc
//       tests/cpp/gzip_model_main.cpp -o gzip_model_asan
// over all fixtures, the corrupt ones first (a stand-alone host program: nothing is preloaded).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gzip_device.h"
using namespace thm::gz;

template <class T>
static T* exact(size_t n, int fill = 0xAA) {
  T* p = (T*)malloc(n ? n * sizeof(T) : 1);
  memset(p, fill, n ? n * sizeof(T) : 1);
  return p;
}

// one call: in[0, n) with the state *st; the summary, and on status 0 the bytes appended to `bytes` and *st moved on
static Summary inflate_call(const uint8_t* data, uint64_t n, uint32_t chunk_bytes, uint32_t last_block, State* st, std::vector<uint8_t>& bytes) {
  Summary sum = {};
  if (n == 0) {
    if (last_block && st->in_member) sum.status = TRUNCATED;
    return sum;
  }
  if (n > MAX_IN) {
    sum.status = INPUT;
    return sum;
  }
  const uint64_t padded = (n + 3) / 4 * 4;
  uint8_t* in = exact<uint8_t>(padded, 0);  // (malloc's blocks are 16-byte aligned)
  memcpy(in, data, n);
  Job j = {};
  j.in = in, j.n = n, j.chunk_bytes = chunk_bytes, j.n_chunks = (uint32_t)((n + chunk_bytes - 1) / chunk_bytes), j.last_block = last_block;
  const uint64_t nc = j.n_chunks, ne = nc * ENDS_PER_CHUNK;
  State* st_out = exact<State>(1);
  j.st_in = st, j.st_out = st_out;
  j.cand = exact<uint64_t>(nc), j.runs = exact<Run>(nc), j.ends = exact<End>(ne);
  j.syms = exact<uint16_t>(nc * region_syms(j)), j.windows = exact<uint8_t>(nc * WINDOW);
  j.run_list = exact<uint32_t>(nc), j.run_off = exact<uint64_t>(nc + 1);
  j.end_abs = exact<uint64_t>(ne), j.end_crc = exact<uint32_t>(ne), j.end_isize = exact<uint32_t>(ne);
  j.member_crc = exact<uint32_t>(ne + 1, 0);
  j.out_cap = nc * region_syms(j);
  j.out = exact<uint8_t>(j.out_cap);
  j.sum = &sum;
  RunWork* rw = exact<RunWork>(1);
  TileWork* tw = exact<TileWork>(1);
  for (uint32_t k = 0; k < j.n_chunks; k++) search_chunk(j, k, rw->w);
  for (uint32_t k = 0; k < j.n_chunks; k++) decode_run(j, k, *rw);
  chain_serial(j);
  if (sum.status == OK) {
    GZ_EACH(t, WINDOW) window_byte_first(j, t);
    for (uint32_t r = 1; r < sum.n_starts; r++) GZ_EACH(t, WINDOW) window_byte(j, j.run_list[r], j.run_list[r - 1], t);
    for (uint64_t T = 0; T * TILE < sum.n_out; T++) resolve_tile(j, T, *tw);
    verify_serial(j);
    GZ_EACH(t, WINDOW) verify_window_byte(j, t);
  }
  if (sum.status == OK) {
    bytes.insert(bytes.end(), j.out, j.out + sum.n_out);
    memcpy(st->window, st_out->window, st_out->window_len);
    st->window_len = st_out->window_len, st->bit_offset = st_out->bit_offset, st->in_member = st_out->in_member;
    st->crc = st_out->crc, st->member_len = st_out->member_len;
    st->n_members_done = st_out->n_members_done, st->stream_offset = st_out->stream_offset;
  }
  free(in), free(st_out), free(j.cand), free(j.runs), free(j.ends), free(j.syms), free(j.windows), free(j.run_list), free(j.run_off);
  free(j.end_abs), free(j.end_crc), free(j.end_isize), free(j.member_crc), free(j.out), free(rw), free(tw);
  return sum;
}

static int run(uint32_t chunk_bytes, uint64_t slice_bytes, uint32_t last, const char* in_path, const char* out_path) {
  FILE* f = fopen(in_path, "rb");
  if (!f) return 2;
  fseek(f, 0, SEEK_END);
  const uint64_t total = (uint64_t)ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<uint8_t> file(total);
  if (total && fread(file.data(), 1, total, f) != total) return 2;
  fclose(f);
  FILE* o = fopen(out_path, "wb");
  FILE* lg = fopen((std::string(out_path) + ".log").c_str(), "w");
  FILE* sf = fopen((std::string(out_path) + ".states").c_str(), "wb");
  if (!o || !lg || !sf) return 2;
  State* st = exact<State>(1, 0);
  std::vector<uint8_t> bytes;
  uint64_t at = 0, slice = slice_bytes ? slice_bytes : total;
  for (;;) {
    const uint64_t n = slice < total - at ? slice : total - at;
    const bool reaches_end = at + n == total;
    const uint32_t last_block = reaches_end ? last : 0;
    const Summary s = inflate_call(file.data() + at, n, chunk_bytes, last_block, st, bytes);
    fprintf(lg, "call %u %u %llu %u %llu %llu %u %u %u %u %u %u\n", s.status, s.bad_chunk, (unsigned long long)n, last_block,
            (unsigned long long)s.n_out, (unsigned long long)s.n_consumed, n ? (uint32_t)((n + chunk_bytes - 1) / chunk_bytes) : 0,
            s.n_starts, s.n_refused, s.n_ends, s.flags, s.paths);
    if (s.status != OK) break;
    fwrite(st, sizeof(State), 1, sf);
    at += s.n_consumed;
    if (reaches_end) break;
    slice = s.n_consumed == 0 ? slice * 2 : (slice_bytes ? slice_bytes : total);
  }
  if (!bytes.empty()) fwrite(bytes.data(), 1, bytes.size(), o);
  fclose(o), fclose(lg), fclose(sf);
  free(st);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 6 || (argc - 4) % 2 != 0) {
    fprintf(stderr, "usage: gzip_model_main <chunk_bytes> <slice_bytes> <last> <in> <out> [<in> <out> ...]\n");
    return 2;
  }
  const uint32_t chunk = (uint32_t)strtoul(argv[1], nullptr, 10);
  const uint64_t slice = strtoull(argv[2], nullptr, 10);
  const uint32_t last = (uint32_t)strtoul(argv[3], nullptr, 10);
  if (chunk < MIN_CHUNK) return 2;
  for (int k = 4; k + 1 < argc; k += 2)
    if (int rc = run(chunk, slice, last, argv[k], argv[k + 1])) return rc;
  return 0;
}
