// Seeks for the point-read path (slatedb/db.go:291-315 reads through them):
//   block_seek_kernel  block.NewIteratorAtKey (internal/sstable/block/iterator.go:31-82) with
//                      firstFullKey's corrupted-first-key recovery (:117-132) and its warnings,
//                      over blocks decoded by the block decode kernels;
//   index_seek_kernel  sstable.Iterator.firstBlockIncludingOrAfterKey (iterator.go:123-153)
//                      over an SST index's first keys.
// One thread per query: each query is a short dependent chain (a binary search over a
// block's rows or an index), and a batch of point reads supplies the parallelism.
#include "common.h"
#include "kernels.h"
#include "seek_common.h"

namespace slate {

__global__ void block_seek_kernel(const uint8_t* data, const uint64_t* out_off, const slate_block_meta* meta,
                                  const uint32_t* qblock, const uint8_t* qkeys, const uint64_t* qkey_off, uint64_t nq,
                                  slate_seek* res, slate_seek_warn* wout, uint32_t wcap) {
  const uint64_t q = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  seek_one(q, data, out_off, meta, qblock, qkeys, qkey_off, res, wout, wcap);
}

// The point-read form (one workgroup, nq <= 256): the inputs, packed by the host into page-locked
// staging in the device layout, are copied into device memory by the kernel itself -- one burst
// over the link in place of a separate copy call -- then searched as above; the results go straight
// back into the staging through its device address.
// kLds: the staged inputs go to LDS (a point read's block and key: a few KiB), so the search's
// dependent reads are LDS round trips instead of L2 ones; otherwise to device memory at base.
template <bool kLds>
__global__ __launch_bounds__(256) void block_seek_staged_kernel(const uint4* __restrict__ hsrc, uint64_t chunks,
                                                                uint4* __restrict__ base, size_t o_data, size_t o_off,
                                                                size_t o_meta, size_t o_q, size_t o_keys,
                                                                size_t o_koff, uint64_t nq, slate_seek* res,
                                                                slate_seek_warn* wout, uint32_t wcap) {
  extern __shared__ __attribute__((aligned(16))) uint4 stage[];
  uint4* dst = kLds ? stage : base;
  for (uint64_t c = threadIdx.x; c < chunks; c += 4 * blockDim.x) {  // four 16-byte chunks in flight
    uint4 v[4];
#pragma unroll
    for (uint32_t u = 0; u < 4; u++) v[u] = hsrc[min(c + u * blockDim.x, chunks - 1)];
#pragma unroll
    for (uint32_t u = 0; u < 4; u++)
      if (c + u * blockDim.x < chunks) dst[c + u * blockDim.x] = v[u];
  }
  __threadfence_block();
  __syncthreads();
  const uint8_t* b = reinterpret_cast<const uint8_t*>(dst);
  const slate_block_meta* mt = reinterpret_cast<const slate_block_meta*>(b + o_meta);
  if (kLds && nq == 1 && mt[reinterpret_cast<const uint32_t*>(b + o_q)[0]].n_rows <= kSeekWaveRows) {
    // a point read: the wave-cooperative form, its outcome table after the stage
    if (threadIdx.x < 64)
      seek_one_wave(b + o_data, reinterpret_cast<const uint64_t*>(b + o_off),
                    reinterpret_cast<const slate_block_meta*>(b + o_meta), reinterpret_cast<const uint32_t*>(b + o_q),
                    b + o_keys, reinterpret_cast<const uint64_t*>(b + o_koff), res, wout, wcap, threadIdx.x,
                    reinterpret_cast<uint32_t*>(dst + chunks));
    return;
  }
  const uint64_t q = threadIdx.x;
  if (q >= nq) return;
  seek_one(q, b + o_data, reinterpret_cast<const uint64_t*>(b + o_off), reinterpret_cast<const slate_block_meta*>(b + o_meta),
           reinterpret_cast<const uint32_t*>(b + o_q), b + o_keys, reinterpret_cast<const uint64_t*>(b + o_koff), res,
           wout, wcap);
}

__global__ void index_seek_kernel(const uint8_t* keys, const uint64_t* key_off, uint64_t n_blocks, const uint8_t* qkeys,
                                  const uint64_t* qkey_off, uint64_t nq, uint64_t* out) {
  const uint64_t q = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  const uint8_t* key = qkeys + qkey_off[q];
  const uint32_t kl = uint32_t(qkey_off[q + 1] - qkey_off[q]);
  int64_t low = 0, high = int64_t(n_blocks) - 1, found = 0;
  while (low <= high) {
    const int64_t mid = low + (high - low) / 2;
    const int c = cmp_bytes(keys + key_off[mid], uint32_t(key_off[mid + 1] - key_off[mid]), key, kl);
    if (c < 0) {
      low = mid + 1;
      found = mid;
    } else if (c > 0) {
      if (mid > 0) high = mid - 1;
      else break;
    } else {
      found = mid;
      break;
    }
  }
  out[q] = uint64_t(found);
}

hipError_t launch_block_seek(hipStream_t st, const uint8_t* data, const uint64_t* out_off, const slate_block_meta* meta,
                             const uint32_t* qblock, const uint8_t* qkeys, const uint64_t* qkey_off, uint64_t nq,
                             slate_seek* res, slate_seek_warn* warn, uint32_t warn_cap) {
  if (nq == 0) return hipSuccess;
  block_seek_kernel<<<uint32_t((nq + 255) / 256), 256, 0, st>>>(data, out_off, meta, qblock, qkeys, qkey_off, nq, res,
                                                                 warn, warn_cap);
  return hipGetLastError();
}

hipError_t launch_block_seek_staged(hipStream_t st, const void* hsrc_dev, size_t bytes, void* base, size_t o_data,
                                    size_t o_off, size_t o_meta, size_t o_q, size_t o_keys, size_t o_koff, uint64_t nq,
                                    slate_seek* res, slate_seek_warn* warn, uint32_t warn_cap) {
  if (nq == 0) return hipSuccess;
  if (nq > 256 || (reinterpret_cast<uintptr_t>(hsrc_dev) & 15) || (reinterpret_cast<uintptr_t>(base) & 15))
    return hipErrorInvalidValue;
  const uint64_t chunks = (bytes + 15) / 16;
  // LDS: the staged bytes, then (one query) the search's outcome per row
  if (16 * chunks + 4 * kSeekWaveRows <= 65536)
    block_seek_staged_kernel<true><<<1, 256, 16 * chunks + (nq == 1 ? 4 * kSeekWaveRows : 0), st>>>(static_cast<const uint4*>(hsrc_dev), chunks,
                                                                 static_cast<uint4*>(base), o_data, o_off, o_meta, o_q,
                                                                 o_keys, o_koff, nq, res, warn, warn_cap);
  else
    block_seek_staged_kernel<false><<<1, 256, 0, st>>>(static_cast<const uint4*>(hsrc_dev), chunks,
                                                        static_cast<uint4*>(base), o_data, o_off, o_meta, o_q, o_keys,
                                                        o_koff, nq, res, warn, warn_cap);
  return hipGetLastError();
}

hipError_t launch_index_seek(hipStream_t st, const uint8_t* keys, const uint64_t* key_off, uint64_t n_blocks,
                             const uint8_t* qkeys, const uint64_t* qkey_off, uint64_t nq, uint64_t* out) {
  if (nq == 0) return hipSuccess;
  index_seek_kernel<<<uint32_t((nq + 255) / 256), 256, 0, st>>>(keys, key_off, n_blocks, qkeys, qkey_off, nq, out);
  return hipGetLastError();
}

}  // namespace slate
