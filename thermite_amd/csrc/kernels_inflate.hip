// kernels_inflate.hip -- the device BGZF inflater (host side inflate.hip): the members of a
// block of .fastq.gz input, each an independent raw DEFLATE stream of at most 64 KiB output, inflated to their places in
// the block the device FASTQ parser then reads.  The kernel is inflate_device.h spread over a wavefront:
//   one wavefront per member, one wavefront per workgroup; the member's output is built in LDS (64 KiB) beside the
//   decode tables, the CRC table and the table build's scratch (14.6 KiB): match sources are LDS reads, and no lane reads back global bytes another
//   lane has just stored.  Two workgroups fit the 160 KiB of a CU.
//   The compressed bytes are read-only here; a member's status word is an ordinary store by lane 0.
#include <hip/hip_runtime.h>

#include "inflate_device.h"
#include "launch_io.h"

namespace thm {
namespace dev {

__global__ __launch_bounds__(64) void bgzf_inflate_kernel(const InflateParams p) {
  __shared__ uint32_t outw[inf::MAX_OUT / 4 + 4];
  __shared__ inf::Work w;
  const uint64_t m = blockIdx.x;
  if (m >= p.n_members) return;
  const inf::Member mb = p.members[m];
  uint32_t status = inf::MEMBER;
  // the table is the host's; a row is followed only where it stays inside the two buffers
  if (mb.in_off <= p.n_in && mb.in_len <= p.n_in - mb.in_off && mb.isize <= inf::MAX_OUT && mb.out_off <= p.n_out &&
      mb.isize <= p.n_out - mb.out_off) {
    const uint32_t lo = (uint32_t)(mb.in_off & 3u);
    const inf::Result r = inf::inflate_member(p.in + (mb.in_off - lo), lo, lo + mb.in_len, mb.isize, mb.crc, outw, w);
    status = r.status;
    __syncthreads();
    if (status == inf::OK) inf::copy_out(p.out + mb.out_off, outw, mb.isize, threadIdx.x & 63u);
  }
  if (threadIdx.x == 0) p.status[m] = status;
}

}  // namespace dev

hipError_t launch_bgzf_inflate(const InflateParams& p, hipStream_t s) {
  if (p.n_members == 0) return hipSuccess;
  if (p.n_members > 0x7FFFFFFFull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dev::bgzf_inflate_kernel, dim3((unsigned)p.n_members), dim3(64), 0, s, p);
  return hipGetLastError();
}

}  // namespace thm
