// kernels_cigar.hip -- run-length CIGARs and alignment summaries from serialised op streams
// (include/thermite.h: thm_aln_digest).  Restates to_noodles_cigar (reference src/aln_writer.rs:279-323) and
// the counts of PafEntry::new (:55-72) and aln_to_sam_record (:160-168) the way csrc/io_writer.cpp restates
// them on the host: Match and Subst -> M, Xclip -> S, Yclip -> N; consecutive equal ops form a run; two
// clips are equal only if their lengths are, and a run of clips is written with the clip's own length.
//
// One op stream per wavefront, 64 bytes per step, one byte per lane.  The only sequential part is finding
// which bytes are tokens: a byte >= 4 at a token position starts a clip and swallows the next four bytes,
// which may themselves be 4 or 5 and may lie in the next step.  That is a scalar loop over the ballot of
// candidate lanes (one turn per clip of the step) which carries 0..4 "payload bytes still to skip" into the
// next step.  Everything else is lane-parallel: a token is a run head when its (kind, clip length) differs
// from the previous token's, run lengths are population counts of the token mask between heads, and the run
// still open at the end of a step is carried as wave-uniform state.
//
// Two passes over the same streams: count (words, counts, flags per stream), an exclusive scan of the word
// counts by the host, emit (BAM words `len << 4 | code` back to back in stream order, and the digests).
#include <hip/hip_runtime.h>

#include "launch.h"

namespace thm {
namespace dev {

constexpr uint32_t CIGAR_NO_KIND = 0xFFu;         // key of "no token yet"
constexpr uint64_t CIGAR_MAX_RUN = 1ull << 28;    // a BAM word holds 28 bits of length
// BAM operation codes of the kinds 0..5 (Match, Subst, Del, Ins, Xclip, Yclip): M M D I S N
__device__ __forceinline__ uint32_t cigar_code(uint32_t kind) { return (0x341200u >> (kind * 4)) & 15u; }

__device__ __forceinline__ uint64_t lanes_below(int l) { return l >= 64 ? ~0ull : ((1ull << l) - 1ull); }

// the stream `s` of the launch: offset and length in the pool; false when it does not lie inside the pool
__device__ __forceinline__ bool cigar_stream(const CigarParams& p, uint64_t s, uint64_t& off, uint64_t& len) {
  if (p.alns) {
    const thm_aln& a = p.alns[s >> 1];
    if (s & 1) {
      off = a.tx_ops_off;
      len = a.aln_type == THM_ALN_EXONIC ? a.tx_ops_len : 0u;
    } else {
      off = a.ops_off;
      len = a.ops_len;
    }
  } else {
    off = p.off[s];
    len = p.off[s + 1] - off;
  }
  return off <= p.ops_bytes && len <= p.ops_bytes - off;
}

template <bool EMIT>
__global__ __launch_bounds__(256) void cigar_kernel(const CigarParams p) {
  const int lane = (int)(threadIdx.x & 63u);
  const uint64_t wave = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
  const uint64_t n_waves = (uint64_t)gridDim.x * 4u;
  const uint64_t below = lanes_below(lane);
  for (uint64_t s = wave; s < p.n_streams; s += n_waves) {
    uint64_t off = 0, len = 0;
    const bool inside = cigar_stream(p, s, off, len);
    uint64_t n_out = 0, w_base = 0;  // EMIT: words this stream has, and where they go
    if (EMIT) {
      n_out = p.n_words[s];
      w_base = p.word_off[s];
      if (lane == 0 && (!p.alns || !(s & 1))) {  // the digest of the alignment (of the stream, without records)
        const uint64_t d = p.alns ? (s >> 1) : s;
        const CigarSum& g = p.sums[s];
        thm_aln_digest o;
        o.cigar_off = w_base;
        o.ref_len = g.ref_len;
        o.n_cigar = (uint32_t)n_out;
        o.n_tx_cigar = p.alns ? (uint32_t)p.n_words[s + 1] : 0u;
        o.n_match = g.n_match;
        o.n_subst = g.n_subst;
        o.n_not_yclip = g.n_not_yclip;
        o.flags = g.flags | (p.alns ? (p.sums[s + 1].flags << 8) : 0u);
        p.digests[d] = o;
      }
      if (n_out == 0) continue;  // empty, malformed or with a run no word can hold
    }
    const uint8_t* src = p.ops + off;
    bool bad = !inside;
    uint32_t skip = 0;                          // payload bytes of a clip that began in an earlier step
    uint32_t open_kind = CIGAR_NO_KIND, open_clip = 0;  // the run still open: its key, its tokens so far
    uint64_t open_cnt = 0;
    uint64_t n_runs = 0, n_match = 0, n_subst = 0, n_yclip = 0, n_tok = 0, n_ref = 0;
    uint64_t yclip_ref = 0;  // per lane: lengths of the Yclip runs whose head the lane held
    bool long_run = false;
    uint32_t nb = (!bad && (uint64_t)lane < len) ? src[lane] : 0u;
    for (uint64_t base = 0; base < len && !bad; base += 64) {
      const uint32_t b = nb;
      const uint64_t pos = base + (uint64_t)lane;
      if (pos + 64 < len) nb = src[pos + 64];  // the next step's byte is on its way while this one is worked on
      const uint64_t left = len - base;
      const uint64_t valid = lanes_below(left >= 64 ? 64 : (int)left);
      // ---- tokens: the scalar walk over the clips of the step
      const uint64_t cand = __ballot(b >= 4u) & valid;
      uint64_t payload = lanes_below((int)skip) & valid;
      uint64_t clips = 0;
      skip = 0;
      for (uint64_t m = cand & ~payload; m;) {
        const int l = __builtin_ctzll(m);
        clips |= 1ull << l;
        if ((uint64_t)l + 5 > left) bad = true;  // a clip cut by the end of the stream
        payload |= (l < 63 ? (0xFull << (l + 1)) : 0ull);
        if (l + 5 > 64) skip = (uint32_t)(l + 5 - 64);
        m = cand & ~payload & ~lanes_below(l + 1);
      }
      payload &= valid;
      const uint64_t tok = valid & ~payload;
      if (__ballot(b > 5u) & tok) bad = true;  // no such kind
      if (bad) break;
      // ---- keys
      const bool is_tok = (tok >> lane) & 1ull;
      const bool is_clip = (clips >> lane) & 1ull;
      uint32_t clip_len = 0;
      if (is_clip) clip_len = (uint32_t)src[pos + 1] | ((uint32_t)src[pos + 2] << 8) | ((uint32_t)src[pos + 3] << 16) | ((uint32_t)src[pos + 4] << 24);
      const uint32_t kind = b == THM_OP_SUBST ? (uint32_t)THM_OP_MATCH : b;
      const uint64_t tok_below = tok & below;
      const int prev_lane = tok_below ? 63 - __builtin_clzll(tok_below) : 0;
      const uint32_t sh_kind = (uint32_t)__shfl((int)kind, prev_lane);
      const uint32_t sh_clip = (uint32_t)__shfl((int)clip_len, prev_lane);
      const uint32_t prev_kind = tok_below ? sh_kind : open_kind;
      const uint32_t prev_clip = tok_below ? sh_clip : open_clip;
      const bool is_head = is_tok && (kind != prev_kind || clip_len != prev_clip);
      const uint64_t heads = __ballot(is_head);
      // ---- counts (wave-uniform)
      n_tok += __builtin_popcountll(tok);
      n_match += __builtin_popcountll(__ballot(is_tok && b == THM_OP_MATCH));
      n_subst += __builtin_popcountll(__ballot(is_tok && b == THM_OP_SUBST));
      n_yclip += __builtin_popcountll(__ballot(is_tok && b == THM_OP_YCLIP));
      n_ref += __builtin_popcountll(__ballot(is_tok && b <= (uint32_t)THM_OP_DEL));
      if (is_head && kind == THM_OP_YCLIP) yclip_ref += clip_len;
      if (__ballot(is_head && is_clip && clip_len >= CIGAR_MAX_RUN)) long_run = true;
      // ---- runs
      if (heads == 0) {
        open_cnt += __builtin_popcountll(tok);
        continue;
      }
      const int first = __builtin_ctzll(heads), last = 63 - __builtin_clzll(heads);
      const int k = __builtin_popcountll(heads);
      if (open_kind != CIGAR_NO_KIND) {  // the first head closes the run carried in
        const uint64_t cnt = open_cnt + __builtin_popcountll(tok & lanes_below(first));
        if (open_kind < THM_OP_XCLIP && cnt >= CIGAR_MAX_RUN) long_run = true;
        if (EMIT && lane == first && n_runs < n_out)
          p.words[w_base + n_runs] = ((open_kind >= THM_OP_XCLIP ? open_clip : (uint32_t)cnt) << 4) | cigar_code(open_kind);
        n_runs++;
      }
      if (EMIT && is_head && lane != last) {  // runs that begin and end inside the step
        const uint64_t above = heads & ~below & ~(1ull << lane);
        const int next = __builtin_ctzll(above);
        const uint32_t cnt = (uint32_t)__builtin_popcountll(tok & ~below & lanes_below(next));
        const uint64_t w = n_runs + (uint64_t)__builtin_popcountll(heads & below);
        if (w < n_out) p.words[w_base + w] = ((kind >= THM_OP_XCLIP ? clip_len : cnt) << 4) | cigar_code(kind);
      }
      n_runs += (uint64_t)(k - 1);
      open_kind = (uint32_t)__shfl((int)kind, last);
      open_clip = (uint32_t)__shfl((int)clip_len, last);
      open_cnt = (uint64_t)__builtin_popcountll(tok & ~lanes_below(last));
    }
    if (!bad && open_kind != CIGAR_NO_KIND) {  // the end of the stream closes the last run
      if (open_kind < THM_OP_XCLIP && open_cnt >= CIGAR_MAX_RUN) long_run = true;
      if (EMIT && lane == 0 && n_runs < n_out)
        p.words[w_base + n_runs] = ((open_kind >= THM_OP_XCLIP ? open_clip : (uint32_t)open_cnt) << 4) | cigar_code(open_kind);
      n_runs++;
    }
    if (!EMIT) {
      for (int o = 32; o; o >>= 1) yclip_ref += (uint64_t)__shfl_xor((long long)yclip_ref, o);
      if (lane == 0) {
        CigarSum g;
        uint32_t flags = 0;
        if (bad) {
          flags = THM_DIGEST_MALFORMED;
          g.ref_len = 0;
          g.n_match = g.n_subst = g.n_not_yclip = 0;
        } else {
          if (long_run) flags = THM_DIGEST_LONG_RUN;
          g.ref_len = n_ref + yclip_ref;
          g.n_match = (uint32_t)n_match;
          g.n_subst = (uint32_t)n_subst;
          g.n_not_yclip = (uint32_t)(n_tok - n_yclip);
        }
        g.flags = flags;
        p.sums[s] = g;
        p.n_words[s] = flags ? 0ull : n_runs;
        if (flags) atomicOr(p.any_flags, flags);
      }
    }
  }
}

}  // namespace dev

static int cigar_blocks(uint64_t n_streams, int n_cu) {
  const uint64_t need = (n_streams + 3) / 4, cap = (uint64_t)(n_cu > 0 ? n_cu : 256) * 8;
  return (int)(need < cap ? (need ? need : 1) : cap);
}

hipError_t launch_cigar_count(const CigarParams& p, int n_cu, hipStream_t s) {
  if (p.n_streams == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::cigar_kernel<false>, dim3((unsigned)cigar_blocks(p.n_streams, n_cu)), dim3(256), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_cigar_emit(const CigarParams& p, int n_cu, hipStream_t s) {
  if (p.n_streams == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::cigar_kernel<true>, dim3((unsigned)cigar_blocks(p.n_streams, n_cu)), dim3(256), 0, s, p);
  return hipGetLastError();
}

}  // namespace thm
