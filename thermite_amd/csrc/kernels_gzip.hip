// kernels_gzip.hip -- the device inflater for plain gzip (host side gzip.hip): gzip_device.h
// spread over wavefronts, five launches on one stream.
//   search   one wavefront per chunk (a workgroup of one): 64 bit offsets a step through the prefilter, the header reader
//            for the survivors; the tables' scratch in LDS (14.6 KiB)
//   decode   one wavefront per chunk, at work where the chunk has a start: the ring of the last 32 Ki symbols in LDS
//            (64 KiB) beside the decode tables -- 78.7 KiB, two workgroups in the 160 KiB of a CU.  Match sources are LDS
//            reads; no lane reads back global symbols another lane has just stored.
//   chain    one workgroup of 1024: thread 0 walks the runs in stream order, then every run's window from its
//            predecessor's, 32 look-ups a thread and step
//   resolve  one wavefront per 4 KiB of inflated bytes; the grid covers the room, tiles behind the bytes leave at once
//   verify   one workgroup: thread 0 compares the members, then the outgoing window
// The compressed bytes are read-only here; status words, counts and CRC pieces are ordinary stores and vector atomics.
#include <hip/hip_runtime.h>

#include "gzip_device.h"
#include "launch_io.h"

namespace thm {
namespace dev {

__global__ __launch_bounds__(64) void gzip_search_kernel(const gz::Job j) {
  __shared__ inf::Work w;
  if (blockIdx.x < j.n_chunks) gz::search_chunk(j, blockIdx.x, w);
}

__global__ __launch_bounds__(64) void gzip_decode_kernel(const gz::Job j) {
  __shared__ gz::RunWork L;
  if (blockIdx.x < j.n_chunks) gz::decode_run(j, blockIdx.x, L);
}

__global__ __launch_bounds__(1024) void gzip_chain_kernel(const gz::Job j) {
  if (threadIdx.x == 0) gz::chain_serial(j);
  __threadfence();
  __syncthreads();
  if (j.sum->status != gz::OK) return;
  const uint32_t n_runs = j.sum->n_starts;
  GZ_EACH(t, gz::WINDOW) gz::window_byte_first(j, t);
  for (uint32_t r = 1; r < n_runs; r++) {
    __threadfence();
    __syncthreads();
    const uint32_t cur = j.run_list[r], prev = j.run_list[r - 1];
    GZ_EACH(t, gz::WINDOW) gz::window_byte(j, cur, prev, t);
  }
}

__global__ __launch_bounds__(64) void gzip_resolve_kernel(const gz::Job j) {
  __shared__ gz::TileWork L;
  gz::resolve_tile(j, blockIdx.x, L);
}

__global__ __launch_bounds__(256) void gzip_verify_kernel(const gz::Job j) {
  if (threadIdx.x == 0) gz::verify_serial(j);
  __threadfence();
  __syncthreads();
  GZ_EACH(t, gz::WINDOW) gz::verify_window_byte(j, t);
}

}  // namespace dev

hipError_t launch_gzip_inflate(const gz::Job& j, hipStream_t s) {
  if (j.n_chunks == 0) return hipSuccess;
  const uint64_t tiles = (j.out_cap + gz::TILE - 1) / gz::TILE;
  if (j.n_chunks > 0x7FFFFFFFu || tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dev::gzip_search_kernel, dim3(j.n_chunks), dim3(64), 0, s, j);
  hipLaunchKernelGGL(dev::gzip_decode_kernel, dim3(j.n_chunks), dim3(64), 0, s, j);
  hipLaunchKernelGGL(dev::gzip_chain_kernel, dim3(1), dim3(1024), 0, s, j);
  if (tiles) hipLaunchKernelGGL(dev::gzip_resolve_kernel, dim3((unsigned)tiles), dim3(64), 0, s, j);
  hipLaunchKernelGGL(dev::gzip_verify_kernel, dim3(1), dim3(256), 0, s, j);
  return hipGetLastError();
}

}  // namespace thm
