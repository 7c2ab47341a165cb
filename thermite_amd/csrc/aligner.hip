// aligner.hip -- host side of the C ABI (include/thermite.h): device upload of
// the index, the per-aligner stream / scratch, and the batch entry points that
// stand where aligner::align_read, Index::all_smems and SwgExtend::extend stand
// in the reference (src/aligner.rs:123, src/index.rs:228, src/swg.rs:31).
//
// There is no CPU fallback: without a HIP device every compute entry point
// fails with THM_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "aligner_internal.h"
#include "lut_direct.h"

namespace thm {
const char* global_error_cstr();
}
using namespace thm;

// tuning knob THM_SWG_BPC = 1..8: resident workgroups per CU of swg_batch_kernel
static int swg_blocks_per_cu() {
  static const int v = [] {
    const char* e = getenv("THM_SWG_BPC");
    const int v = e ? atoi(e) : 4;
    return (v >= 1 && v <= 8) ? v : 4;
  }();
  return v;
}

// knob THM_LUT_DIRECT=0, read when a device copy of an index is made: the k-mer table stays plain (lut_direct.h; A/B runs)
static bool lut_direct_wanted() {
  const char* e = getenv("THM_LUT_DIRECT");
  return !(e && e[0] == '0');
}

// `v` into `b`, which gets 16 bytes at least
template <class T>
static hipError_t upload(DBuf& b, const std::vector<T>& v, hipStream_t s) {
  size_t bytes = std::max<size_t>(v.size() * sizeof(T), 16);
  hipError_t e = b.ensure(bytes);
  if (e != hipSuccess) return e;
  if (!v.empty()) return hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s);
  return hipSuccess;
}
template <class T>
static hipError_t upload(DArr<T>& b, const std::vector<T>& v, hipStream_t s) {
  const size_t bytes = v.size() * sizeof(T);
  hipError_t e = b.ensure(v.size(), bytes < 16 ? 16 - bytes : 0);
  if (e != hipSuccess) return e;
  if (!v.empty()) return hipMemcpyAsync(b, v.data(), bytes, hipMemcpyHostToDevice, s);
  return hipSuccess;
}

static int get_dev_copy(thm_aligner* a) {
  thm_index* ix = const_cast<thm_index*>(a->ix);
  std::lock_guard<std::mutex> g(*(std::mutex*)ix->dev_mu);
  if ((int)ix->dev.size() <= a->device) ix->dev.resize(a->device + 1, nullptr);
  if (!ix->dev[a->device]) {
    auto* d = new thm_index::DevCopy();
    d->device = a->device;
    hipStream_t s = a->stream;
    hipError_t e = hipSuccess;
    auto up = [&](auto& buf, const auto& vec) {
      if (e == hipSuccess) e = upload(buf, vec, s);
    };
    d->wide = ix->wide;
    // the text gets 16 bytes in front (left extensions are read in whole 8-byte words that may begin a few bytes before the
    // first symbol; the window staging of the wave-per-read kernels rounds its addresses down to 16 bytes)
    if (e == hipSuccess) e = d->text.ensure(ix->text.size(), 16 + 16);
    if (e == hipSuccess) e = hipMemsetAsync(d->text, '$', 16, s);
    if (e == hipSuccess && !ix->text.empty())
      e = hipMemcpyAsync(d->text + 16, ix->text.data(), ix->text.size(), hipMemcpyHostToDevice, s);
    if (ix->wide) {
      up(d->sa, ix->sa64);
      up(d->lut, ix->lut64);
    } else {
      up(d->sa, ix->sa);
      up(d->lut, ix->lut);
    }
    up(d->refs, ix->refs);
    up(d->name_rank, ix->name_rank);
    up(d->txs, ix->txs);
    up(d->exons, ix->exons);
    up(d->exon_txoff, ix->exon_txoff);
    // transcript sequences get 16 bytes of front padding: window staging reads whole 16-byte
    // granules and may start up to 15 bytes before a transcript
    if (e == hipSuccess) e = d->tx_seq.ensure(ix->tx_seq.size(), 32);
    if (e == hipSuccess) e = hipMemsetAsync(d->tx_seq, '$', 16, s);
    if (e == hipSuccess && !ix->tx_seq.empty())
      e = hipMemcpyAsync(d->tx_seq + 16, ix->tx_seq.data(), ix->tx_seq.size(), hipMemcpyHostToDevice, s);
    up(d->exon_grid_off, ix->exon_grid_off);
    up(d->gene_grid_off, ix->gene_grid_off);
    up(d->ref_bin, ix->ref_bin);
    if (ix->wide)
      up(d->ref_recs, ix->ref_recs64);
    else
      up(d->ref_recs, ix->ref_recs);
    if (ix->wide) {
      up(d->exon_grid, ix->exon_grid64);
      up(d->gene_grid, ix->gene_grid64);
    } else {
      up(d->exon_grid, ix->exon_grid);
      up(d->gene_grid, ix->gene_grid);
    }
    // text positions into the single-suffix entries of the device table (lut_direct.h): sa and lut are on their way
    // on this stream; the host tables stay as they are
    const bool tag = lut_direct_wanted() && (ix->wide ? lutd::can_tag<uint64_t>(ix->n) : lutd::can_tag<uint32_t>(ix->n)) &&
                     (ix->wide ? !ix->lut64.empty() : !ix->lut.empty());
    if (tag) {
      if (e == hipSuccess) e = d->lut_cnt.ensure(2);
      if (e == hipSuccess) e = hipMemsetAsync(d->lut_cnt, 0, 16, s);
      if (e == hipSuccess)
        e = ix->wide ? launch_lut_tag(d->lut.as<LutEntryT<uint64_t>>(), d->sa.as<uint64_t>(), ix->lut64.size(), ix->n,
                                      d->lut_cnt, s)
                     : launch_lut_tag(d->lut.as<LutEntryT<uint32_t>>(), d->sa.as<uint32_t>(), ix->lut.size(), ix->n,
                                      d->lut_cnt, s);
      if (e == hipSuccess) e = hipMemcpyAsync(&d->lut_tagged, d->lut_cnt, 8, hipMemcpyDeviceToHost, s);
      d->lut_direct = true;
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
      free_dev_copy(d);
      return fail(a, e == hipErrorOutOfMemory ? THM_ERR_OOM : THM_ERR_HIP, "index upload failed: %s",
                  hipGetErrorString(e));
    }
    auto fill_view = [&](auto& v) {
      typedef typename std::remove_reference<decltype(v)>::type::coord_t C;
      v.text = d->text + 16;
      v.sa = d->sa.as<C>();
      v.lut = d->lut.as<LutEntryT<C>>();
      v.refs = d->refs;
      v.name_rank = d->name_rank;
      v.ref_recs = d->ref_recs.as<RefRecT<C>>();
      v.ref_bin = d->ref_bin;
      v.txs = d->txs;
      v.exons = d->exons;
      v.exon_txoff = d->exon_txoff;
      v.tx_seq = d->tx_seq + 16;
      v.exon_grid_off = d->exon_grid_off;
      v.exon_grid = d->exon_grid.as<ExonEntryT<C>>();
      v.gene_grid_off = d->gene_grid_off;
      v.gene_grid = d->gene_grid.as<GridEntryT<C>>();
      v.n = ix->n;
      v.n_refs = (uint32_t)ix->refs.size();
      v.n_txs = (uint32_t)ix->txs.size();
      v.kt = ix->kt;
      v.max_tx_exons = ix->max_tx_exons;
      v.lut_direct = d->lut_direct ? 1u : 0u;
    };
    memset(&d->view, 0, sizeof d->view);
    memset(&d->view64, 0, sizeof d->view64);
    if (ix->wide)
      fill_view(d->view64);
    else
      fill_view(d->view);
    ix->dev[a->device] = d;
  }
  a->dix = ix->dev[a->device];
  return THM_OK;
}

int reset_queue(thm_aligner* a) {
  HIPCHK(a, hipMemsetAsync(a->d_queue, 0, thm::QUEUE_BYTES, a->stream));
  HIPCHK(a, hipMemsetAsync(a->d_fault, 0, 64, a->stream));
  return THM_OK;
}

extern "C" {

const char* thm_version(void) { return "thermite_amd 0.1 (gfx950)"; }

int32_t thm_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

void thm_index_free(thm_index* ix) {
  if (!ix) return;
  for (auto* d : ix->dev) free_dev_copy(d);
  delete (std::mutex*)ix->dev_mu;
  delete ix;
}

const char* thm_last_error(const thm_aligner* a) { return a ? a->err.c_str() : global_error_cstr(); }

int32_t thm_aligner_create(const thm_index* ix, const thm_align_opts* opts, int32_t device_id, thm_aligner** out) {
  if (!out) return THM_ERR_INVALID_ARG;
  *out = nullptr;
  if (!ix || !opts) return fail(nullptr, THM_ERR_INVALID_ARG, "thm_aligner_create: null index or opts");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    return fail(nullptr, THM_ERR_NO_DEVICE, "no HIP device visible: the MI355X path has no CPU fallback");
  if (device_id < 0 || device_id >= n) return fail(nullptr, THM_ERR_NO_DEVICE, "device id %d out of range", device_id);
  thm_aligner* a = new thm_aligner();
  a->ix = ix;
  a->device = device_id;
  a->opts = *opts;
  {
    const char* e = getenv("THM_TPR");  // 0 / 1: the problem-parallel path off / on (A/B measurements)
    if (e && e[0] == '0') a->tpr.use_tpr = false;
    if (e && e[0] == '1') a->tpr.use_tpr = true;
    e = getenv("THM_TPR_ROUNDS");
    if (e && atoi(e) >= 1 && atoi(e) <= TPR_MAX_ROUNDS) a->tpr.tpr_rounds = atoi(e);
  }
  auto bail = [&](int code) {
    thm_aligner_free(a);
    return code;
  };
  if (hipSetDevice(device_id) != hipSuccess) return bail(fail(nullptr, THM_ERR_HIP, "hipSetDevice failed"));
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) a->n_cu = prop.multiProcessorCount;
  if (a->stream.create() != hipSuccess) return bail(fail(nullptr, THM_ERR_HIP, "hipStreamCreate failed"));
  if (ensure_events(a->ev) != hipSuccess) return bail(fail(nullptr, THM_ERR_HIP, "hipEventCreate failed"));
  if (a->stream2.create() != hipSuccess || a->tpr.stream3.create() != hipSuccess || a->tpr.stream4.create() != hipSuccess ||
      a->tpr.ev_dpt_fork.ensure(false) != hipSuccess || a->tpr.ev_dpt_join.ensure(false) != hipSuccess ||
      a->tpr.ev_join3.ensure(false) != hipSuccess || a->ev_fork.ensure(false) != hipSuccess ||
      a->ev_join.ensure(false) != hipSuccess)
    return bail(fail(nullptr, THM_ERR_HIP, "second stream / events: creation failed"));
  if (a->d_counters.ensure(THM_N_COUNTERS * 3) != hipSuccess || a->d_ctl.ensure(thm_aligner::CTL_BYTES) != hipSuccess)
    return bail(fail(nullptr, THM_ERR_OOM, "scratch allocation failed"));
  {
    uint8_t* ctl = a->d_ctl.as<uint8_t>();
    a->s_work_counts = {(unsigned long long*)(ctl + thm_aligner::CTL_WORK_COUNTS), 128};
    a->d_cursors = {(unsigned long long*)(ctl + thm_aligner::CTL_CURSORS), 64};
    a->d_fault = {(int*)(ctl + thm_aligner::CTL_FAULT), 64};
    a->d_queue = {(unsigned int*)(ctl + thm_aligner::CTL_QUEUE), thm::QUEUE_BYTES};
    a->d_queue_ext = {(unsigned int*)(ctl + thm_aligner::CTL_QUEUE_EXT), thm::QUEUE_BYTES};
  }
  (void)hipMemsetAsync(a->d_counters, 0, THM_N_COUNTERS * 8 * 3, a->stream);
  (void)hipMemsetAsync(a->d_ctl.p, 0, thm_aligner::CTL_BYTES, a->stream);
  int rc = get_dev_copy(a);
  if (rc != THM_OK) return bail(rc);
  rc = thm_aligner_set_opts(a, opts);
  if (rc != THM_OK) return bail(rc);
  *out = a;
  return THM_OK;
}

void thm_aligner_free(thm_aligner* a) {
  if (!a) return;
  (void)hipSetDevice(a->device);
  // work may still be in flight; after it every buffer, event and stream frees itself (aligner_internal.h)
  for (const Stream* s : {&a->stream, &a->stream2, &a->tpr.stream3, &a->tpr.stream4})
    if (s->s) (void)hipStreamSynchronize(s->s);
  delete a;
}

int32_t thm_aligner_set_opts(thm_aligner* a, const thm_align_opts* o) {
  if (!a || !o) return THM_ERR_INVALID_ARG;
  if (o->min_seed_len < 1 || o->min_seed_len > 65535) return fail(a, THM_ERR_INVALID_ARG, "min_seed_len out of range");
  if (!(o->min_aln_score_percent >= 0.0f && o->min_aln_score_percent <= 1.0f))
    return fail(a, THM_ERR_INVALID_ARG, "min_aln_score_percent must be within [0,1] (src/main.rs:46-49)");
  // Ranges on which align_read's own arithmetic overflows (src/aligner.rs:156-178; a read has at most 65535 bases here, and
  // max_aln_score lies between min_aln_score and the read's length): read.len() + range in usize, and
  // max_aln_score - (range as i32) in i32 where the cast is negative.
  const int64_t range_i32 = (int64_t)(int32_t)(uint32_t)o->multimap_score_range;
  const int64_t max_score = std::max<int64_t>(65535, o->min_aln_score);
  if (o->multimap_score_range > UINT64_MAX - 65535 || (range_i32 < 0 && max_score - range_i32 > INT32_MAX))
    return fail(a, THM_ERR_OUT_OF_CONTRACT, "multimap_score_range %llu overflows in the reference's align_read",
                (unsigned long long)o->multimap_score_range);
  a->opts = *o;
  return THM_OK;
}

void* thm_aligner_stream(thm_aligner* a) { return a ? (void*)a->stream : nullptr; }

const thm_index* thm_aligner_index(const thm_aligner* a) { return a ? a->ix : nullptr; }

int32_t thm_counters_get(thm_aligner* a, uint64_t out[THM_N_COUNTERS]) {
  if (!a || !out) return THM_ERR_INVALID_ARG;
  HIPCHK(a, hipSetDevice(a->device));
  HIPCHK(a, hipMemcpyAsync(out, a->d_counters, THM_N_COUNTERS * 8, hipMemcpyDeviceToHost, a->stream));
  HIPCHK(a, hipStreamSynchronize(a->stream));
  return THM_OK;
}
int32_t thm_counters_reset(thm_aligner* a) {
  if (!a) return THM_ERR_INVALID_ARG;
  HIPCHK(a, hipSetDevice(a->device));
  HIPCHK(a, hipMemsetAsync(a->d_counters, 0, THM_N_COUNTERS * 8, a->stream));
  return THM_OK;
}
void* thm_counters_device_ptr(thm_aligner* a) { return a ? a->d_counters.get() : nullptr; }

int32_t thm_timings_get(thm_aligner* a, float out[THM_N_TIMINGS]) {
  if (!a || !out) return THM_ERR_INVALID_ARG;
  memcpy(out, a->timings, sizeof(a->timings));
  return THM_OK;
}

// ------------------------------------------------- SwgExtend::extend batch
int32_t thm_swg_extend_batch(thm_aligner* a, const uint8_t* x_bases, const uint64_t* x_off, const uint8_t* y_bases,
                             const uint64_t* y_off, const uint32_t* band_width, const int32_t* x_drop,
                             uint32_t max_band_width, uint64_t n, thm_swg_view* out) {
  if (!a || !out || !x_off || !y_off || !band_width || !x_drop) return THM_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  if (n == 0) return THM_OK;
  if (n >= 0xFFFFFFFFull) return fail(a, THM_ERR_UNSUPPORTED, "more than 2^32-1 problems in one call");
  HIPCHK(a, hipSetDevice(a->device));
  uint32_t bw_max = 0, x_max = 0, y_max = 0;
  std::vector<uint64_t> ops_off(n + 1, 0);
  for (uint64_t i = 0; i < n; i++) {
    if (band_width[i] > max_band_width)  // assert!, src/swg.rs:32
      return fail(a, THM_ERR_OUT_OF_CONTRACT, "problem %llu: band_width %u > max_band_width %u (src/swg.rs:32)",
                  (unsigned long long)i, band_width[i], max_band_width);
    if (x_drop[i] < (int64_t)band_width[i])
      return fail(a, THM_ERR_OUT_OF_CONTRACT, "problem %llu: x_drop < band_width is undefined in the reference",
                  (unsigned long long)i);
    uint64_t xl = x_off[i + 1] - x_off[i], yl = y_off[i + 1] - y_off[i];
    if (x_off[i + 1] < x_off[i] || y_off[i + 1] < y_off[i]) return fail(a, THM_ERR_INVALID_ARG, "offsets not monotone");
    if (xl > MAX_READ_LEN || band_width[i] > 2 * MAX_READ_LEN)
      return fail(a, THM_ERR_UNSUPPORTED, "x longer than %u or band wider than +-%u", MAX_READ_LEN, 2 * MAX_READ_LEN);
    uint64_t cols = std::min<uint64_t>(yl, xl + band_width[i] + 1);
    bw_max = std::max(bw_max, band_width[i]);
    x_max = std::max<uint32_t>(x_max, (uint32_t)xl);
    y_max = std::max<uint32_t>(y_max, (uint32_t)cols);
    ops_off[i + 1] = ops_off[i] + xl + cols + 8;
  }
  int cpl = cells_per_lane(bw_max);
  SwgBatchParams p;
  p.x_cap = (x_max + 15u) & ~15u;
  p.y_cap = (y_max + 15u) & ~15u;
  if (p.x_cap == 0) p.x_cap = 16;
  if (p.y_cap == 0) p.y_cap = 16;
  p.max_bw = bw_max;
  p.scratch = nullptr;
  p.scratch_per_wave = 0;
  // bands over +-127 or problems beyond the LDS budget: the any-width kernel (SwgExtend::new takes any band, src/swg.rs:17-26)
  if (cpl > 4 || swg_batch_lds_bytes(p, cpl) > EXTEND_LDS_LIMIT) cpl = 0;
  const uint64_t xb_n = x_off[n], yb_n = y_off[n], pool = ops_off[n];
  HIPCHK(a, a->b0.ensure(xb_n + 16));
  HIPCHK(a, a->b1.ensure((n + 1) * 8));
  HIPCHK(a, a->b2.ensure(yb_n + 16));
  HIPCHK(a, a->b3.ensure((n + 1) * 8));
  HIPCHK(a, a->b4.ensure(n * 4));
  HIPCHK(a, a->b5.ensure(n * 4));
  HIPCHK(a, a->b6.ensure((n + 1) * 8));
  HIPCHK(a, a->b7.ensure(pool + 16));
  HIPCHK(a, a->b8.ensure(n * sizeof(thm_swg_aln)));
  hipStream_t s = a->stream;
  if (xb_n) HIPCHK(a, hipMemcpyAsync(a->b0.p, x_bases, xb_n, hipMemcpyHostToDevice, s));
  HIPCHK(a, hipMemcpyAsync(a->b1.p, x_off, (n + 1) * 8, hipMemcpyHostToDevice, s));
  if (yb_n) HIPCHK(a, hipMemcpyAsync(a->b2.p, y_bases, yb_n, hipMemcpyHostToDevice, s));
  HIPCHK(a, hipMemcpyAsync(a->b3.p, y_off, (n + 1) * 8, hipMemcpyHostToDevice, s));
  HIPCHK(a, hipMemcpyAsync(a->b4.p, band_width, n * 4, hipMemcpyHostToDevice, s));
  HIPCHK(a, hipMemcpyAsync(a->b5.p, x_drop, n * 4, hipMemcpyHostToDevice, s));
  HIPCHK(a, hipMemcpyAsync(a->b6.p, ops_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
  int rc = reset_queue(a);
  if (rc != THM_OK) return rc;
  p.xb = a->b0.as<uint8_t>();
  p.xo = a->b1.as<uint64_t>();
  p.yb = a->b2.as<uint8_t>();
  p.yo = a->b3.as<uint64_t>();
  p.bw = a->b4.as<uint32_t>();
  p.xd = a->b5.as<int32_t>();
  p.ops_off = a->b6.as<uint64_t>();
  p.ops = a->b7.as<uint8_t>();
  p.out = a->b8.as<thm_swg_aln>();
  p.counters = a->d_counters;
  p.queue = a->d_queue;
  p.fault = a->d_fault;
  p.n = n;
  const int bpc = swg_blocks_per_cu();
  int n_blocks = grid_blocks(a, n, 4, bpc);
  if (cpl == 0) {
    p.scratch_per_wave = (swg_batch_scratch_bytes(p) + 255) & ~255ull;
    const uint64_t budget = 16ull << 30;
    if (p.scratch_per_wave > budget) return fail(a, THM_ERR_UNSUPPORTED, "DP trace of %llu bytes per problem exceeds the device-memory budget",
                                                 (unsigned long long)p.scratch_per_wave);
    n_blocks = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)n_blocks, budget / p.scratch_per_wave / 4));
    HIPCHK(a, a->ext.slow.ensure((size_t)n_blocks * 4 * p.scratch_per_wave, 256));
    p.scratch = a->ext.slow;
  }
  HIPCHK(a, launch_swg_batch(p, cpl, n_blocks, s));
  std::vector<thm_swg_aln> raw(n);
  std::vector<uint8_t> pool_h(pool);
  int fault = 0;
  HIPCHK(a, hipMemcpyAsync(raw.data(), a->b8.p, n * sizeof(thm_swg_aln), hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipMemcpyAsync(pool_h.data(), a->b7.p, pool, hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipMemcpyAsync(&fault, a->d_fault, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipStreamSynchronize(s));
  if (fault) return fail(a, THM_ERR_INTERNAL, "inconsistent trace in swg_batch_kernel");
  // canonical layout: op streams back to back in problem order
  a->h_swg.resize(n);
  a->h_ops.clear();
  for (uint64_t i = 0; i < n; i++) {
    thm_swg_aln r = raw[i];
    uint64_t off = a->h_ops.size();
    a->h_ops.insert(a->h_ops.end(), pool_h.begin() + r.ops_off, pool_h.begin() + r.ops_off + r.ops_len);
    r.ops_off = off;
    a->h_swg[i] = r;
  }
  out->n = n;
  out->n_op_bytes = a->h_ops.size();
  out->alns = a->h_swg.data();
  out->ops = a->h_ops.data();
  return THM_OK;
}

// ------------------------------------------------- extend_left_right batch
int32_t thm_extend_left_right_batch(thm_aligner* a, const uint8_t* x_bases, const uint64_t* x_off, const uint8_t* y_bases,
                                    const uint64_t* y_off, const thm_mem* hits, const uint32_t* band_width,
                                    const int32_t* x_drop, uint32_t max_band_width, uint64_t n, thm_lr_view* out) {
  if (!a || !out || !x_off || !y_off || !hits || !band_width || !x_drop) return THM_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  if (n == 0) return THM_OK;
  if (n >= 0xFFFFFFFFull) return fail(a, THM_ERR_UNSUPPORTED, "more than 2^32-1 problems in one call");
  if ((!x_bases && x_off[n] > 0) || (!y_bases && y_off[n] > 0)) return THM_ERR_INVALID_ARG;
  HIPCHK(a, hipSetDevice(a->device));
  uint32_t bw_max = 0, x_max = 0, y_max = 0;
  std::vector<uint64_t> ops_off(n + 1, 0);
  for (uint64_t i = 0; i < n; i++) {
    if (x_off[i + 1] < x_off[i] || y_off[i + 1] < y_off[i]) return fail(a, THM_ERR_INVALID_ARG, "offsets not monotone");
    const uint64_t xl = x_off[i + 1] - x_off[i], yl = y_off[i + 1] - y_off[i];
    const thm_mem& h = hits[i];
    if (band_width[i] > max_band_width)  // assert!, src/swg.rs:32
      return fail(a, THM_ERR_OUT_OF_CONTRACT, "problem %llu: band_width %u > max_band_width %u (src/swg.rs:32)",
                  (unsigned long long)i, band_width[i], max_band_width);
    if (x_drop[i] < (int64_t)band_width[i])
      return fail(a, THM_ERR_OUT_OF_CONTRACT, "problem %llu: x_drop < band_width is undefined in the reference",
                  (unsigned long long)i);
    if ((uint64_t)h.query_idx + h.len > xl)  // &read[hit.query_idx + hit.len..], src/aligner.rs:360
      return fail(a, THM_ERR_OUT_OF_CONTRACT, "problem %llu: query_idx + len > read length (src/aligner.rs:360)",
                  (unsigned long long)i);
    if (h.ref_idx > yl || h.ref_idx + h.len > yl)  // &ref_seq[hit.ref_idx + hit.len..], src/aligner.rs:361
      return fail(a, THM_ERR_OUT_OF_CONTRACT, "problem %llu: ref_idx + len > reference length (src/aligner.rs:361)",
                  (unsigned long long)i);
    if (xl > MAX_READ_LEN || band_width[i] > 2 * MAX_READ_LEN)
      return fail(a, THM_ERR_UNSUPPORTED, "read longer than %u or band wider than +-%u", MAX_READ_LEN, 2 * MAX_READ_LEN);
    // columns each side can reach: |x| + bw + 1
    const uint64_t xr = xl - (h.query_idx + h.len), xlft = h.query_idx;
    const uint64_t yr = std::min<uint64_t>(yl - (h.ref_idx + h.len), xr + band_width[i] + 1);
    const uint64_t ylft = std::min<uint64_t>(std::min<uint64_t>(h.ref_idx, xl + band_width[i]), xlft + band_width[i] + 1);
    bw_max = std::max(bw_max, band_width[i]);
    x_max = std::max<uint32_t>(x_max, (uint32_t)std::max(xr, xlft));
    y_max = std::max<uint32_t>(y_max, (uint32_t)std::max(yr, ylft));
    ops_off[i + 1] = ops_off[i] + xr + yr + xlft + ylft + h.len + 16;
  }
  int cpl = cells_per_lane(bw_max);
  ElrBatchParams p;
  p.x_cap = (x_max + 15u) & ~15u;
  p.y_cap = (y_max + 15u) & ~15u;
  if (p.x_cap == 0) p.x_cap = 16;
  if (p.y_cap == 0) p.y_cap = 16;
  p.max_bw = bw_max;
  p.scratch = nullptr;
  p.scratch_per_wave = 0;
  // bands over +-127 or problems beyond the LDS budget: the any-width kernel, chosen as thm_swg_extend_batch chooses it
  if (cpl > 4 || elr_batch_lds_bytes(p, cpl) > EXTEND_LDS_LIMIT) cpl = 0;
  const uint64_t xb_n = x_off[n], yb_n = y_off[n], pool = ops_off[n];
  HIPCHK(a, a->b0.ensure(xb_n + 16));
  HIPCHK(a, a->b1.ensure((n + 1) * 8));
  HIPCHK(a, a->b2.ensure(yb_n + 16));
  HIPCHK(a, a->b3.ensure((n + 1) * 8));
  HIPCHK(a, a->b4.ensure(n * 4));
  HIPCHK(a, a->b5.ensure(n * 4));
  HIPCHK(a, a->b6.ensure((n + 1) * 8));
  HIPCHK(a, a->b7.ensure(pool + 16));
  HIPCHK(a, a->b8.ensure(n * sizeof(thm_lr_aln)));
  HIPCHK(a, a->sh.hits.ensure(n));
  hipStream_t s = a->stream;
  if (xb_n) HIPCHK(a, hipMemcpyAsync(a->b0.p, x_bases, xb_n, hipMemcpyHostToDevice, s));
  HIPCHK(a, hipMemcpyAsync(a->b1.p, x_off, (n + 1) * 8, hipMemcpyHostToDevice, s));
  if (yb_n) HIPCHK(a, hipMemcpyAsync(a->b2.p, y_bases, yb_n, hipMemcpyHostToDevice, s));
  HIPCHK(a, hipMemcpyAsync(a->b3.p, y_off, (n + 1) * 8, hipMemcpyHostToDevice, s));
  HIPCHK(a, hipMemcpyAsync(a->b4.p, band_width, n * 4, hipMemcpyHostToDevice, s));
  HIPCHK(a, hipMemcpyAsync(a->b5.p, x_drop, n * 4, hipMemcpyHostToDevice, s));
  HIPCHK(a, hipMemcpyAsync(a->b6.p, ops_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
  HIPCHK(a, hipMemcpyAsync(a->sh.hits, hits, n * sizeof(thm_mem), hipMemcpyHostToDevice, s));
  int rc = reset_queue(a);
  if (rc != THM_OK) return rc;
  p.xb = a->b0.as<uint8_t>();
  p.xo = a->b1.as<uint64_t>();
  p.yb = a->b2.as<uint8_t>();
  p.yo = a->b3.as<uint64_t>();
  p.hits = a->sh.hits;
  p.bw = a->b4.as<uint32_t>();
  p.xd = a->b5.as<int32_t>();
  p.ops_off = a->b6.as<uint64_t>();
  p.ops = a->b7.as<uint8_t>();
  p.out = a->b8.as<thm_lr_aln>();
  p.counters = a->d_counters;
  p.queue = a->d_queue;
  p.fault = a->d_fault;
  p.n = n;
  int n_blocks = grid_blocks(a, n, 4, 4);
  if (cpl == 0) {
    p.scratch_per_wave = (elr_batch_scratch_bytes(p) + 255) & ~255ull;
    const uint64_t budget = 16ull << 30;
    if (p.scratch_per_wave > budget) return fail(a, THM_ERR_UNSUPPORTED, "DP trace of %llu bytes per problem exceeds the device-memory budget",
                                                 (unsigned long long)p.scratch_per_wave);
    n_blocks = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)n_blocks, budget / p.scratch_per_wave / 4));
    HIPCHK(a, a->ext.slow.ensure((size_t)n_blocks * 4 * p.scratch_per_wave, 256));
    p.scratch = a->ext.slow;
  }
  HIPCHK(a, launch_elr_batch(p, cpl, n_blocks, s));
  std::vector<thm_lr_aln> raw(n);
  std::vector<uint8_t> pool_h(pool);
  int fault = 0;
  HIPCHK(a, hipMemcpyAsync(raw.data(), a->b8.p, n * sizeof(thm_lr_aln), hipMemcpyDeviceToHost, s));
  if (pool) HIPCHK(a, hipMemcpyAsync(pool_h.data(), a->b7.p, pool, hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipMemcpyAsync(&fault, a->d_fault, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(a, hipStreamSynchronize(s));
  if (fault) return fail(a, THM_ERR_INTERNAL, "inconsistent trace in elr_batch_kernel");
  // canonical layout: op streams back to back in problem order
  a->h_lr.resize(n);
  a->h_ops.clear();
  for (uint64_t i = 0; i < n; i++) {
    thm_lr_aln r = raw[i];
    const uint64_t off = a->h_ops.size();
    a->h_ops.insert(a->h_ops.end(), pool_h.begin() + r.ops_off, pool_h.begin() + r.ops_off + r.ops_len);
    r.ops_off = off;
    a->h_lr[i] = r;
  }
  out->n = n;
  out->n_op_bytes = a->h_ops.size();
  out->alns = a->h_lr.data();
  out->ops = a->h_ops.data();
  return THM_OK;
}

// tuning hook: per-section shader clocks of the extend kernel (all zero unless built with -DTHM_PROF)
int32_t thm_debug_prof_get(thm_aligner* a, uint64_t out[16], int32_t reset) {
  if (!a || !out) return THM_ERR_INVALID_ARG;
  HIPCHK(a, hipSetDevice(a->device));
  unsigned long long* p = a->d_counters + 2 * THM_N_COUNTERS;
  HIPCHK(a, hipMemcpyAsync(out, p, 16 * 8, hipMemcpyDeviceToHost, a->stream));
  if (reset) HIPCHK(a, hipMemsetAsync(p, 0, 16 * 8, a->stream));
  HIPCHK(a, hipStreamSynchronize(a->stream));
  return THM_OK;
}

// test hook: start the next batches with these pool sizes (entries, entries, bytes; 0 = the usual heuristics) so that
// the grow-and-replay path of thm_batch_sync is exercised; returns the number of replays so far through *n_replays
int32_t thm_debug_set_pool_caps(thm_aligner* a, uint64_t smem_cap, uint64_t cand_cap, uint64_t ops_cap, uint32_t* n_replays) {
  if (!a) return THM_ERR_INVALID_ARG;
  a->dbg_smem_cap = smem_cap;
  a->dbg_cand_cap = cand_cap;
  a->dbg_ops_cap = ops_cap;
  a->seed.smem_cap = a->ext.cand_cap = a->ext.cand_ops_cap = 0;
  if (n_replays) *n_replays = a->n_replays;
  return THM_OK;
}

// test / tuning hook.  flags bit 0: the problem-parallel path (kernels_tpr.hip) off -- every read takes the wave-per-read
// kernels; bit 1: on (the parity tests run both ways); bits 8..11: rounds of requests (0: keep).
// thm_debug_tpr_stats: 32 words of the last run -- [0] reads of the fast class left to the wave-per-read kernel,
// [1..15] why (1 band, 2 grid, 3 lift, 7 other, 8 rounds / requests per round, 9 candidates, 10 ops beside Match, 11 introns,
// 12 request pools, 13 window ends, 14 open targets), [16] DP requests, [17] of them narrow (thread-per-problem kernel),
// [18..21] by band class, [22] reads still waiting when the rounds ran out.
int32_t thm_debug_set_flags(thm_aligner* a, uint32_t flags) {
  if (!a) return THM_ERR_INVALID_ARG;
  if (flags & 1u) a->tpr.use_tpr = false;
  if (flags & 2u) a->tpr.use_tpr = true;
  const int r = (int)((flags >> 8) & 15u);
  if (r >= 1 && r <= TPR_MAX_ROUNDS) a->tpr.tpr_rounds = r;
  // bit 2: the seed probes are never decided from the table entry and a neighbouring match, and store every interval
  // (kernels_seed.hip; for A/B runs), bit 4: they are again; bit 3: the seed kernels count their probes for
  // thm_debug_seed_stats, bit 5: they stop counting.  Neither bit of a pair: keep, as with bits 0 and 1.
  if (flags & 4u) a->dbg_seed_noinfer = true;
  if (flags & 16u) a->dbg_seed_noinfer = false;
  if (flags & 8u) a->dbg_seed_stats = true;
  if (flags & 32u) a->dbg_seed_stats = false;
  // bit 6: a probe into a single-suffix bucket ignores the text position its table entry holds and reads sa[lo] (the
  // table stays as it is; lut_direct.h), bit 7: it uses the position again
  if (flags & 64u) a->dbg_seed_nodirect = true;
  if (flags & 128u) a->dbg_seed_nodirect = false;
  // bit 16: the cells phase of the seed stage decides an inner position only by the rule "both grid points have the same
  // stored end" and leaves every other cell to the fill whole (seed_bounds.h off; for A/B runs), bit 17: bounds again
  if (flags & 0x10000u) a->dbg_seed_nobounds = true;
  if (flags & 0x20000u) a->dbg_seed_nobounds = false;
  // bit 12: the finisher (kernels_finish.hip) leaves class E (whole-read exact matches) to the extend kernel, bit 13: it
  // takes them again; bits 14 / 15: the same for class S (one substitution between two SMEMs).  Default: both on.
  if (flags & 0x1000u) a->fin_classes &= ~1u;
  if (flags & 0x2000u) a->fin_classes |= 1u;
  if (flags & 0x4000u) a->fin_classes &= ~2u;
  if (flags & 0x8000u) a->fin_classes |= 2u;
  return THM_OK;
}
// thm_debug_smem_finish_stats: the finisher in the last batch -- [0] reads of class E it finished, [1] reads with class E's
// SMEM shape it left to the extend kernel, [2] / [3] the same for class S (zeros when it did not run: a class switched
// off is not counted)
int32_t thm_debug_smem_finish_stats(thm_aligner* a, uint64_t stats[4]) {
  if (!a || !stats) return THM_ERR_INVALID_ARG;
  stats[0] = stats[1] = stats[2] = stats[3] = 0;
  if (!a->fin_blocks || !a->ext.finstats.get()) return THM_OK;
  HIPCHK(a, hipSetDevice(a->device));
  HIPCHK(a, hipStreamSynchronize(a->stream));
  std::vector<unsigned long long> rows((size_t)a->fin_blocks * 4);
  HIPCHK(a, hipMemcpy(rows.data(), a->ext.finstats, rows.size() * 8, hipMemcpyDeviceToHost));
  for (size_t b = 0; b < a->fin_blocks; b++)
    for (int k = 0; k < 4; k++) stats[k] += rows[b * 4 + k];
  return THM_OK;
}
// thm_debug_seed_stats: the last batch's seed stage, counted when bit 3 of thm_debug_set_flags is set (else zeros) --
// [0] probes decided from the k-mer table entry alone, [1] probes run in full (position 0 of every read included)
int32_t thm_debug_seed_stats(thm_aligner* a, uint64_t stats[2]) {
  if (!a || !stats) return THM_ERR_INVALID_ARG;
  stats[0] = stats[1] = 0;
  if (!a->s_work_counts.p || a->s_work_counts.cap < 128) return THM_OK;
  HIPCHK(a, hipSetDevice(a->device));
  HIPCHK(a, hipStreamSynchronize(a->stream));
  HIPCHK(a, hipMemcpy(stats, a->s_work_counts + 8, 16, hipMemcpyDeviceToHost));
  return THM_OK;
}
// thm_debug_seed_direct_stats: [0] the device copy of the k-mer table holds text positions (lut_direct.h; 0 under
// THM_LUT_DIRECT=0 or for a 32-bit table over 2^31 symbols or more), [1] entries the pass rewrote; of the last batch,
// counted like thm_debug_seed_stats: [2] full probes that took the text position from the table entry, [3] full probes
// into a single-suffix bucket that read the suffix array
int32_t thm_debug_seed_direct_stats(thm_aligner* a, uint64_t stats[4]) {
  if (!a || !stats) return THM_ERR_INVALID_ARG;
  stats[0] = stats[1] = stats[2] = stats[3] = 0;
  if (!a->dix) return THM_OK;
  stats[0] = a->dix->lut_direct ? 1 : 0;
  stats[1] = a->dix->lut_tagged;
  if (!a->s_work_counts.p || a->s_work_counts.cap < 128) return THM_OK;
  HIPCHK(a, hipSetDevice(a->device));
  HIPCHK(a, hipStreamSynchronize(a->stream));
  HIPCHK(a, hipMemcpy(stats + 2, a->s_work_counts + 10, 16, hipMemcpyDeviceToHost));
  return THM_OK;
}
// test hook: the device copy of the k-mer table as the kernels read it, `bytes` = 4^kt entries of two coordinates
int32_t thm_debug_fetch_lut(thm_aligner* a, void* out, uint64_t bytes) {
  if (!a || !out || !a->dix) return THM_ERR_INVALID_ARG;
  const uint64_t have = a->dix->wide ? a->ix->lut64.size() * sizeof(LutEntryT<uint64_t>) : a->ix->lut.size() * sizeof(LutEntryT<uint32_t>);
  if (bytes != have) return fail(a, THM_ERR_INVALID_ARG, "thm_debug_fetch_lut: the table has %llu bytes", (unsigned long long)have);
  HIPCHK(a, hipSetDevice(a->device));
  HIPCHK(a, hipStreamSynchronize(a->stream));
  if (bytes) HIPCHK(a, hipMemcpy(out, a->dix->lut.p, bytes, hipMemcpyDeviceToHost));
  return THM_OK;
}
// test hook: the register-resident kernels pretend their class holds bands up to `max_bw` only (max_bw + 1 is stored; 0 turns
// the hook off): a read whose band is wider gets the per-read status THM_ERR_INTERNAL and no alignments -- the condition
// the kernels guard against but cannot meet while the classes are cut by read length (src/swg.rs:32 asserts it per call)
int32_t thm_debug_set_band_clip(thm_aligner* a, uint32_t max_bw_plus_1) {
  if (!a) return THM_ERR_INVALID_ARG;
  a->dbg_band_clip = max_bw_plus_1;
  return THM_OK;
}
int32_t thm_debug_tpr_stats(thm_aligner* a, uint64_t stats[32]) {
  if (!a || !stats) return THM_ERR_INVALID_ARG;
  memset(stats, 0, 256);
  if (!a->tpr.t_ctl.p) return THM_OK;
  HIPCHK(a, hipSetDevice(a->device));
  HIPCHK(a, hipStreamSynchronize(a->stream));
  unsigned long long c[40];
  HIPCHK(a, hipMemcpy(c, a->tpr.t_ctl.p, sizeof c, hipMemcpyDeviceToHost));
  for (int k = 0; k < 16; k++) stats[k] = c[TPRC_STATS + k];
  stats[16] = c[TPRC_REC_CUR];
  stats[17] = c[TPRC_Q_CUR];  // class 0: thread-per-problem kernel
  for (int k = 0; k < 4; k++) stats[18 + k] = c[TPRC_Q_CUR + 1 + k];
  stats[22] = c[TPRC_N_ACT + a->tpr.tpr_rounds + 1];
  return THM_OK;
}
// test hook: what the run-time knobs of INTEGRATION.md section 6 resolved to in this process, as the launches will use
// them -- [0] THM_SEED_FILL mode, [1] THM_COMPACT_K, [2] THM_HIT_GL lanes per hit, [3 + 2 * (cpl - 1) + wide] waves per
// SIMD of the wave-per-read extend kernel for cpl = 1..4 cells per lane and 32- / 64-bit coordinates (THM_EXT_MINW,
// THM_EXT_MINW_CPL3, THM_EXT_MINW_WIDE), [11] THM_TEAM_DIV_PER_CU, [12] THM_SWG_BPC, [13] this aligner's use_tpr,
// [14] its tpr_rounds, [15] its n_cu
int32_t thm_debug_knobs(thm_aligner* a, uint32_t out[16]) {
  if (!a || !out) return THM_ERR_INVALID_ARG;
  out[0] = seed_fill_mode();
  out[1] = (uint32_t)compact_k();
  out[2] = (uint32_t)hit_gl();
  for (int cpl = 1; cpl <= 4; cpl++)
    for (int wide = 0; wide < 2; wide++) out[3 + 2 * (cpl - 1) + wide] = (uint32_t)extend_waves_per_simd(cpl, wide != 0);
  out[11] = team_div_per_cu();
  out[12] = (uint32_t)swg_blocks_per_cu();
  out[13] = a->tpr.use_tpr ? 1u : 0u;
  out[14] = (uint32_t)a->tpr.tpr_rounds;
  out[15] = (uint32_t)a->n_cu;
  return THM_OK;
}

// profiling hook (tools/calib_fetch.py): a gather of known size over the index's k-mer table, in the access patterns of the
// hot kernels, so that rocprofv3's FETCH_SIZE can be calibrated against a byte count (launch.h: launch_calib_gather).
// Returns the bytes the lanes ask for through *bytes_requested.
int32_t thm_debug_calib_gather(thm_aligner* a, int32_t pattern, uint64_t n_threads, uint64_t* bytes_requested) {
  if (!a || pattern < 0 || pattern > 2) return THM_ERR_INVALID_ARG;
  HIPCHK(a, hipSetDevice(a->device));
  const uint64_t span = a->dix->lut.cap & ~255ull;
  if (span < 4096) return fail(a, THM_ERR_INVALID_ARG, "k-mer table too small for the calibration gather");
  HIPCHK(a, launch_calib_gather(a->dix->lut.as<uint8_t>(), span, n_threads, pattern, a->d_cursors + 4, a->stream));
  HIPCHK(a, hipStreamSynchronize(a->stream));
  if (bytes_requested) *bytes_requested = n_threads * (pattern == 0 ? 8 : (pattern == 1 ? 4 : 16));
  return THM_OK;
}

// debug hook used by tests/test_gpu_swg.py: wave scan / shift primitives
int32_t thm_debug_wave_prims(thm_aligner* a, const int32_t in[64], int32_t out[384]) {
  if (!a || !in || !out) return THM_ERR_INVALID_ARG;
  HIPCHK(a, hipSetDevice(a->device));
  HIPCHK(a, a->b0.ensure(64 * 4));
  HIPCHK(a, a->b1.ensure(384 * 4));
  HIPCHK(a, hipMemcpyAsync(a->b0.p, in, 64 * 4, hipMemcpyHostToDevice, a->stream));
  HIPCHK(a, launch_wave_prims(a->b0.as<int>(), a->b1.as<int>(), a->stream));
  HIPCHK(a, hipMemcpyAsync(out, a->b1.p, 384 * 4, hipMemcpyDeviceToHost, a->stream));
  HIPCHK(a, hipStreamSynchronize(a->stream));
  return THM_OK;
}

}  // extern "C"
