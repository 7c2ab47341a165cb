// kernels_bam.hip -- BAM records of an aligned batch, encoded on the device (include/thermite_io.h: thm_bam_view).
// Restates format_range_bam of csrc/io_writer.cpp byte for byte: the record the reference writes through
// bam::Writer::write_sam_record (src/aligner.rs:69-76,98-108) from aln_to_sam_record / unmapped_sam_record
// (src/aln_writer.rs:118-253), built from what is resident after a run -- raw read bytes, thm_aln records, digests and
// CIGAR words (kernels_cigar.hip) -- plus names, qualities and the index's name tables.
//
// The record index space is the alignments in order plus one record for every read without alignments:
//   prep    one thread per read: records of the read (its alignments, or 1), QNAME length (name up to the first space)
//   (scan)  -> first record of every read
//   size    one thread per record: its read (binary search in the scan), its byte length
//   (scan)  -> byte offset of every record, and the total
//   emit    one wavefront per record: lanes share out the bytes of every part of the record
//   offsets one thread per read: byte offset of its first record
// A read with 60 000 alignments is 60 000 work items of the size pass and 60 000 wavefronts' worth of the emit pass.
//
// Records are byte-packed, so they begin at any byte address.  The emit kernel comes in two forms (template STAGE):
// byte stores straight to global memory -- lane k of a part writes byte k, so a wavefront store covers 64 consecutive
// bytes -- or the record assembled in the wavefront's slice of LDS and written out as aligned dwords with a byte head
// and tail (records beyond the slice take the byte path).  DESIGN.md section 4.9 has the two kernel times.
#include <hip/hip_runtime.h>

#include "bai_device.h"
#include "launch_io.h"

namespace thm {
namespace dev {

constexpr uint32_t BAM_STAGE_BYTES = 1024;  // LDS slice of one wavefront (a 91-base record has some 250 bytes)

// SEQ_CODE of io_writer.cpp: the position in "=ACMGRSVTWYHKDBN", both cases, everything else 15.  Letters by
// (c & 31) = 1 .. 26, four bits each, in two 64-bit constants.
__host__ __device__ constexpr uint64_t seq_code_half(int hi) {
  uint64_t v = 0;
  for (int i = 0; i < 16; i++) {
    const int letter = hi * 16 + i;  // 1 = A
    int code = 15;
    const char* a = "=ACMGRSVTWYHKDBN";
    for (int k = 1; k < 16; k++)
      if (a[k] - 'A' + 1 == letter) code = k;
    v |= (uint64_t)code << (4 * i);
  }
  return v;
}
constexpr uint64_t SEQ_CODE_LO = seq_code_half(0), SEQ_CODE_HI = seq_code_half(1);

__device__ __forceinline__ uint32_t seq_code(uint32_t c) {
  const uint32_t u = c | 32u;
  if (u >= 'a' && u <= 'z') {
    const uint32_t l = c & 31u;
    return (uint32_t)(((l & 16u) ? SEQ_CODE_HI : SEQ_CODE_LO) >> (4u * (l & 15u))) & 15u;
  }
  return c == '=' ? 0u : 15u;
}
// the code of bio's complement (COMP of io_writer.cpp): in the four-bit code A C G T are the bits 1 2 4 8, so the
// complement of any IUPAC code is its bit reversal; '=' (0) and the unknown (15) map to themselves, as there
__device__ __forceinline__ uint32_t seq_code_comp(uint32_t code) { return __brev(code) >> 28; }

__device__ __forceinline__ uint32_t dec_digits(uint64_t v) {
  uint32_t n = 1;
  while (v >= 10) {
    v /= 10;
    n++;
  }
  return n;
}
// digit k (0 = most significant) of v, which has nd digits
__device__ __forceinline__ uint32_t dec_digit_at(uint64_t v, uint32_t nd, uint32_t k) {
  for (uint32_t i = k + 1; i < nd; i++) v /= 10;
  return (uint32_t)(v % 10);
}

// bam_int_tag: the smallest type that holds the value; bytes of the value
__device__ __forceinline__ uint32_t int_tag_bytes(int64_t v) {
  if (v >= 0) return v <= 0xff ? 1u : (v <= 0xffff ? 2u : 4u);
  return v >= -128 ? 1u : (v >= -32768 ? 2u : 4u);
}
__device__ __forceinline__ uint32_t int_tag_type(int64_t v) {
  if (v >= 0) return v <= 0xff ? 'C' : (v <= 0xffff ? 'S' : 'I');
  return v >= -128 ? 'c' : (v >= -32768 ? 's' : 'i');
}

using bai::reg2bin;  // UCSC binning, SAM specification section 5.3 (bai_device.h: io_writer.cpp calls the same)

__device__ __forceinline__ uint32_t multimapq(uint64_t n) {  // io_writer.cpp
  if (n <= 1) return 255;
  if (n >= 5) return 0;
  return n == 2 ? 3u : (n == 3 ? 2u : 1u);
}

// What one mapped record is made of, as both passes see it; false: a table index or the word range is out of range
// (the host reports it as format_range_bam does).
struct BamRec {
  uint64_t a0, multimap;  // first alignment of the read, its number of alignments
  uint64_t cig_off;
  uint32_t n_cig, n_tx;
  uint32_t tx, gene;  // THM_NO_IDX: none
  uint32_t kind;      // 'E' 'N' 'I'
};

__device__ __forceinline__ bool bam_rec(const BamParams& p, uint64_t a, const thm_aln& al, const thm_aln_digest& d, BamRec& o) {
  o.cig_off = d.cigar_off;
  o.n_cig = d.n_cigar;
  o.n_tx = 0;
  o.tx = o.gene = THM_NO_IDX;
  o.kind = 'I';
  if (d.flags) return false;
  if (d.cigar_off > p.n_words || (uint64_t)d.n_cigar + d.n_tx_cigar > p.n_words - d.cigar_off) return false;
  if (al.ref_id >= p.n_refs) return false;
  if (al.aln_type == THM_ALN_EXONIC) {
    if (al.tx_or_gene_idx >= p.n_txs) return false;
    o.tx = al.tx_or_gene_idx;
    o.gene = p.tx_gene[o.tx];
    o.n_tx = d.n_tx_cigar;
    o.kind = 'E';
  } else if (al.aln_type == THM_ALN_INTRONIC) {
    o.gene = al.tx_or_gene_idx;
    o.kind = 'N';
  }
  if (o.gene != THM_NO_IDX && o.gene >= p.n_genes) return false;
  return true;
}

__global__ __launch_bounds__(256) void bam_prep_kernel(const BamParams p) {
  const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (r >= p.n_reads) return;
  const uint64_t k = p.aln_off[r + 1] - p.aln_off[r];
  p.rec_cnt[r] = k ? k : 1;
  // format_read_name: up to the first space
  const uint8_t* nm = p.names + p.name_off[r];
  const uint64_t nl = p.name_off[r + 1] - p.name_off[r];
  uint64_t q = 0;
  while (q < nl && nm[q] != ' ') q++;
  if (q > 254) {
    atomicOr(p.err, BAM_ERR_QNAME);
    q = 254;  // (nothing of this batch is handed out)
  }
  p.qn[r] = (uint32_t)q;
}

__global__ __launch_bounds__(256) void bam_size_kernel(const BamParams p) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= p.n_rec) return;
  // the read whose records hold record i: the last r with rec_first[r] <= i
  uint64_t lo = 0, hi = p.n_reads;
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) >> 1;
    if (p.rec_first[mid] <= i)
      lo = mid;
    else
      hi = mid;
  }
  const uint64_t r = lo;
  p.rec_read[i] = (uint32_t)r;
  const uint64_t L = p.offsets[r + 1] - p.offsets[r];
  uint64_t len = 36 + (uint64_t)p.qn[r] + 1 + (L + 1) / 2 + L;
  const uint64_t a0 = p.aln_off[r], multimap = p.aln_off[r + 1] - a0;
  if (multimap) {
    const uint64_t a = a0 + (i - p.rec_first[r]);
    const thm_aln& al = p.alns[a];
    const thm_aln_digest& d = p.digests[a];
    BamRec rc;
    if (!bam_rec(p, a, al, d, rc)) {
      atomicOr(p.err, d.flags ? BAM_ERR_DIGEST_FLAGS : BAM_ERR_RANGE);
      len = 0;
    } else if (rc.n_cig > 0xffffu) {
      atomicOr(p.err, BAM_ERR_CIGAR_WORDS);
      len = 0;
    } else {
      len += 4ull * rc.n_cig;
      len += 12 + int_tag_bytes(al.score) + int_tag_bytes((int64_t)multimap) + int_tag_bytes((int64_t)(a - a0 + 1)) + int_tag_bytes(d.n_subst);
      if (!(p.flags & THM_BAM_FLAG_NO_ANNOTATION)) {
        if (rc.tx != THM_NO_IDX) {
          uint64_t txt = 1;  // "*"
          if (rc.n_tx) {
            txt = 0;
            const uint32_t* w = p.words + rc.cig_off + rc.n_cig;
            for (uint32_t k = 0; k < rc.n_tx; k++) txt += dec_digits(w[k] >> 4) + 1;
          }
          len += 3 + (p.tx_off[rc.tx + 1] - p.tx_off[rc.tx]) + 2 + dec_digits(al.tx_ystart) + 1 + txt + 1;
        }
        if (rc.gene != THM_NO_IDX)
          len += 3 + (p.gid_off[rc.gene + 1] - p.gid_off[rc.gene]) + 1 + 3 + (p.gname_off[rc.gene + 1] - p.gname_off[rc.gene]) + 1;
        len += 4;
      }
    }
  }
  p.rec_len[i] = len;
}

__global__ __launch_bounds__(256) void bam_offsets_kernel(const BamParams p) {
  const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (r > p.n_reads) return;
  p.read_rec_off[r] = p.rec_off[p.rec_first[r]];
}

// Where the bytes of one record go: the wavefront's LDS slice, or global memory at the record's offset.
template <bool STAGE>
struct BamOut {
  uint8_t* g;
  uint8_t* l;
  bool staged;
  __device__ __forceinline__ void put(uint64_t pos, uint32_t b) const {
    if (STAGE && staged)
      l[pos] = (uint8_t)b;
    else
      g[pos] = (uint8_t)b;
  }
};

// "TT" 'Z' pool[off[i] .. off[i+1]) NUL at `pos`; returns the bytes written
template <bool STAGE>
__device__ __forceinline__ uint64_t put_str_tag(const BamOut<STAGE>& o, uint64_t pos, int lane, uint32_t t0, uint32_t t1,
                                                const uint8_t* s, uint32_t n) {
  for (uint32_t k = (uint32_t)lane; k < n + 4; k += 64) {
    const uint32_t b = k == 0 ? t0 : (k == 1 ? t1 : (k == 2 ? (uint32_t)'Z' : (k < n + 3 ? (uint32_t)s[k - 3] : 0u)));
    o.put(pos + k, b);
  }
  return (uint64_t)n + 4;
}

template <bool STAGE>
__global__ __launch_bounds__(256) void bam_emit_kernel(const BamParams p) {
  __shared__ uint32_t stage[STAGE ? 4 * (BAM_STAGE_BYTES / 4 + 2) : 1];
  const int lane = (int)(threadIdx.x & 63u);
  const uint32_t wib = threadIdx.x >> 6;
  const uint64_t wave = (uint64_t)blockIdx.x * 4u + wib;
  const uint64_t n_waves = (uint64_t)gridDim.x * 4u;
  for (uint64_t i = wave; i < p.n_rec; i += n_waves) {
    const uint64_t base = p.rec_off[i], len = p.rec_off[i + 1] - base;
    if (len == 0) continue;  // (a record the size pass flagged)
    const uint64_t r = p.rec_read[i];
    BamOut<STAGE> o;
    o.g = p.out + base;
    o.l = STAGE ? (uint8_t*)(stage + wib * (BAM_STAGE_BYTES / 4 + 2)) : nullptr;
    o.staged = STAGE && len <= BAM_STAGE_BYTES;
    const uint8_t* seq = p.bases + p.offsets[r];
    const uint64_t L = p.offsets[r + 1] - p.offsets[r];
    const uint8_t* qual = p.quals ? p.quals + p.offsets[r] : nullptr;
    const uint8_t* nm = p.names + p.name_off[r];
    const uint32_t qn = p.qn[r];
    const uint64_t a0 = p.aln_off[r], multimap = p.aln_off[r + 1] - a0;
    const uint64_t a = a0 + (i - p.rec_first[r]);
    thm_aln al;
    thm_aln_digest d;
    BamRec rc;
    rc.n_cig = rc.n_tx = 0;
    rc.cig_off = 0;
    rc.tx = rc.gene = THM_NO_IDX;
    rc.kind = 'I';
    bool forward = true;
    // ---- the 36 fixed bytes: lanes 0 .. 8 hold a dword each
    uint32_t f_ref = 0xFFFFFFFFu, f_pos = 0xFFFFFFFFu, f_mq = 255, f_bin = 4680, f_flag = 4;
    if (multimap) {
      al = p.alns[a];
      d = p.digests[a];
      (void)bam_rec(p, a, al, d, rc);  // (checked by the size pass)
      forward = al.strand != 0;
      const int64_t pos = (int64_t)al.ystart;
      f_ref = (uint32_t)p.ref_sq[al.ref_id];
      f_pos = (uint32_t)(int32_t)pos;
      f_mq = multimapq(multimap);
      f_bin = reg2bin(pos, pos + (int64_t)(d.ref_len > 1 ? d.ref_len : 1));
      f_flag = (al.strand ? 0u : 16u) | (al.primary ? 0u : 256u);
    }
    if (lane < 9) {
      uint32_t v = 0;
      switch (lane) {
        case 0: v = (uint32_t)(len - 4); break;
        case 1: v = f_ref; break;
        case 2: v = f_pos; break;
        case 3: v = ((qn + 1) & 0xffu) | ((f_mq & 0xffu) << 8) | ((f_bin & 0xffffu) << 16); break;
        case 4: v = (rc.n_cig & 0xffffu) | ((f_flag & 0xffffu) << 16); break;
        case 5: v = (uint32_t)L; break;
        case 6: v = 0xFFFFFFFFu; break;  // next refID
        case 7: v = 0xFFFFFFFFu; break;  // next pos
        default: v = 0; break;           // tlen
      }
      for (int j = 0; j < 4; j++) o.put(4 * lane + j, (v >> (8 * j)) & 0xffu);
    }
    uint64_t at = 36;
    // ---- QNAME + NUL
    for (uint32_t k = (uint32_t)lane; k <= qn; k += 64) o.put(at + k, k < qn ? (uint32_t)nm[k] : 0u);
    at += (uint64_t)qn + 1;
    // ---- CIGAR words, copied
    {
      const uint32_t* w = p.words + rc.cig_off;
      const uint32_t nb = 4 * rc.n_cig;
      for (uint32_t k = (uint32_t)lane; k < nb; k += 64) o.put(at + k, (w[k >> 2] >> (8 * (k & 3u))) & 0xffu);
      at += nb;
    }
    // ---- bases, two per byte; complemented and reversed for the reverse strand
    {
      const uint64_t nb = (L + 1) / 2;
      for (uint64_t k = (uint64_t)lane; k < nb; k += 64) {
        const uint64_t i0 = 2 * k, i1 = 2 * k + 1;
        uint32_t c0, c1 = 0;
        if (forward) {
          c0 = seq_code(seq[i0]);
          if (i1 < L) c1 = seq_code(seq[i1]);
        } else {
          c0 = seq_code_comp(seq_code(seq[L - 1 - i0]));
          if (i1 < L) c1 = seq_code_comp(seq_code(seq[L - 1 - i1]));
        }
        o.put(at + k, (c0 << 4) | c1);
      }
      at += nb;
    }
    // ---- qualities
    for (uint64_t k = (uint64_t)lane; k < L; k += 64) o.put(at + k, qual ? (uint32_t)(uint8_t)(qual[forward ? k : L - 1 - k] - 33) : 0xffu);
    at += L;
    if (multimap) {
      // ---- AS NH HI nM: lanes 0 .. 3 write a tag each
      const int64_t tv[4] = {(int64_t)al.score, (int64_t)multimap, (int64_t)(a - a0 + 1), (int64_t)d.n_subst};
      uint32_t tb[4];
      for (int t = 0; t < 4; t++) tb[t] = int_tag_bytes(tv[t]);
      if (lane < 4) {
        uint64_t q = at;
        int64_t v = tv[0];
        uint32_t nb = tb[0], n0 = 'A', n1 = 'S';
        if (lane == 1) q += 3 + tb[0], v = tv[1], nb = tb[1], n0 = 'N', n1 = 'H';
        if (lane == 2) q += 6 + tb[0] + tb[1], v = tv[2], nb = tb[2], n0 = 'H', n1 = 'I';
        if (lane == 3) q += 9 + tb[0] + tb[1] + tb[2], v = tv[3], nb = tb[3], n0 = 'n', n1 = 'M';
        o.put(q, n0);
        o.put(q + 1, n1);
        o.put(q + 2, int_tag_type(v));
        for (uint32_t j = 0; j < nb; j++) o.put(q + 3 + j, (uint32_t)((uint64_t)v >> (8 * j)) & 0xffu);
      }
      at += 12 + tb[0] + tb[1] + tb[2] + tb[3];
      if (!(p.flags & THM_BAM_FLAG_NO_ANNOTATION)) {
        if (rc.tx != THM_NO_IDX) {
          // ---- TX:Z:<tx_id>,+<tx_ystart>,<cigar text> NUL
          const uint8_t* id = p.tx_pool + p.tx_off[rc.tx];
          const uint32_t idn = p.tx_off[rc.tx + 1] - p.tx_off[rc.tx];
          const uint32_t nd = dec_digits(al.tx_ystart);
          const uint32_t head = 3 + idn + 2 + nd + 1;
          for (uint32_t k = (uint32_t)lane; k < head; k += 64) {
            uint32_t b;
            if (k < 3)
              b = k == 0 ? 'T' : (k == 1 ? 'X' : 'Z');
            else if (k < 3 + idn)
              b = id[k - 3];
            else if (k < 5 + idn)
              b = k == 3 + idn ? ',' : '+';
            else if (k < 5 + idn + nd)
              b = '0' + dec_digit_at(al.tx_ystart, nd, k - (5 + idn));
            else
              b = ',';
            o.put(at + k, b);
          }
          at += head;
          if (rc.n_tx == 0) {
            if (lane == 0) o.put(at, '*');
            at += 1;
          } else {
            // one word per lane: its text length, an inclusive scan over the wavefront, its digits and its letter
            const uint32_t* w = p.words + rc.cig_off + rc.n_cig;
            for (uint32_t c = 0; c < rc.n_tx; c += 64) {
              const uint32_t k = c + (uint32_t)lane;
              const uint32_t word = k < rc.n_tx ? w[k] : 0u;
              const uint32_t nd_w = k < rc.n_tx ? dec_digits(word >> 4) : 0u;
              const uint32_t mine = k < rc.n_tx ? nd_w + 1 : 0u;
              uint32_t incl = mine;
              for (int s = 1; s < 64; s <<= 1) {
                const uint32_t up = (uint32_t)__shfl_up((int)incl, s);
                if (lane >= s) incl += up;
              }
              if (k < rc.n_tx) {
                const uint64_t q = at + (incl - mine);
                uint32_t v = word >> 4;
                for (uint32_t j = nd_w; j-- > 0;) {
                  o.put(q + j, '0' + v % 10);
                  v /= 10;
                }
                o.put(q + nd_w, (uint32_t)"MIDNSHP=X???????"[word & 15u]);
              }
              at += (uint32_t)__shfl((int)incl, 63);
            }
          }
          if (lane == 0) o.put(at, 0u);
          at += 1;
        }
        if (rc.gene != THM_NO_IDX) {
          at += put_str_tag<STAGE>(o, at, lane, 'G', 'X', p.gid_pool + p.gid_off[rc.gene], p.gid_off[rc.gene + 1] - p.gid_off[rc.gene]);
          at += put_str_tag<STAGE>(o, at, lane, 'G', 'N', p.gname_pool + p.gname_off[rc.gene], p.gname_off[rc.gene + 1] - p.gname_off[rc.gene]);
        }
        if (lane < 4) o.put(at + lane, lane == 0 ? 'R' : (lane == 1 ? 'E' : (lane == 2 ? 'A' : rc.kind)));
        at += 4;
      }
    }
    if (STAGE && o.staged) {
      // the slice is written and read by this wavefront only: its LDS operations complete in order
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      const uint32_t n = (uint32_t)len;
      uint32_t head = (uint32_t)((4u - (uint32_t)((uintptr_t)o.g & 3u)) & 3u);
      if (head > n) head = n;
      const uint32_t n_dw = (n - head) >> 2, tail = (n - head) & 3u;
      if ((uint32_t)lane < head) o.g[lane] = o.l[lane];
      const uint32_t* lw = (const uint32_t*)o.l;
      uint32_t* gw = (uint32_t*)(o.g + head);
      const uint32_t sh = 8u * head;  // the dwords begin `head` bytes into the slice
      for (uint32_t k = (uint32_t)lane; k < n_dw; k += 64) {
        const uint32_t lo = lw[k], hi = lw[k + 1];
        gw[k] = sh ? (lo >> sh) | (hi << (32u - sh)) : lo;
      }
      if ((uint32_t)lane < tail) o.g[head + 4 * n_dw + lane] = o.l[head + 4 * n_dw + lane];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  // the next record reuses the slice
      __builtin_amdgcn_wave_barrier();
    }
  }
}

}  // namespace dev

hipError_t launch_bam_prep(const BamParams& p, hipStream_t s) {
  if (p.n_reads == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::bam_prep_kernel, dim3(blocks256(p.n_reads)), dim3(256), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_bam_size(const BamParams& p, hipStream_t s) {
  if (p.n_rec == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::bam_size_kernel, dim3(blocks256(p.n_rec)), dim3(256), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_bam_emit(const BamParams& p, bool stage, int n_cu, hipStream_t s) {
  if (p.n_rec == 0) return hipSuccess;
  const uint64_t need = (p.n_rec + 3) / 4, cap = (uint64_t)(n_cu > 0 ? n_cu : 256) * 16;
  const unsigned blocks = (unsigned)(need < cap ? need : cap);
  if (stage)
    hipLaunchKernelGGL(dev::bam_emit_kernel<true>, dim3(blocks), dim3(256), 0, s, p);
  else
    hipLaunchKernelGGL(dev::bam_emit_kernel<false>, dim3(blocks), dim3(256), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_bam_offsets(const BamParams& p, hipStream_t s) {
  hipLaunchKernelGGL(dev::bam_offsets_kernel, dim3(blocks256(p.n_reads + 1)), dim3(256), 0, s, p);
  return hipGetLastError();
}

}  // namespace thm
