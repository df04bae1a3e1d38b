// The bloom filter's probe sequence (bloom.go:147-160), shared by the filter build and check
// kernels (encode.hip) and the batched point reads (get.hip).
#pragma once
#include "common.h"

namespace slate {

// bloom.go:147-160 probesForKey in 32-bit arithmetic: every value is below filterBits (< 2^32), so
// the first two reductions are 32-bit and the later ones a conditional subtraction (h + delta <
// 2 filterBits; delta + i below filterBits + i, with the modulo kept for i >= filterBits) -- the
// same values as Go's uint64 % (the probes computed two 64-bit modulos each)
struct BloomProbes {
  uint32_t h, delta, m, k;
  __device__ BloomProbes(uint64_t h64, uint32_t filter_bits) : m(filter_bits), k(0) {
    h = uint32_t(h64) % m;
    delta = uint32_t(h64 >> 32) % m;
  }
  __device__ uint32_t next() {
    const uint64_t d = uint64_t(delta) + k;
    delta = d < m ? uint32_t(d) : (d - m < m ? uint32_t(d - m) : uint32_t(d % m));
    k++;
    const uint32_t p = h;
    const uint64_t hh = uint64_t(h) + delta;
    h = hh < m ? uint32_t(hh) : uint32_t(hh - m);
    return p;
  }
};

}  // namespace slate
