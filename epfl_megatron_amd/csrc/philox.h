// Counter-based Philox-4x32-10 (Salmon et al., SC'11), shared by the dropout
// mask (dropout.hip) and the sampling noise (decode_tail.hip).  Counter =
// (ctr_lo, ctr_hi, offset_lo, offset_hi), key = seed; ops/dropout.py::_philox
// is the NumPy transcription the tests check it against.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace ema {

struct U4 {
  uint32_t x, y, z, w;
};

__device__ __forceinline__ U4 philox(uint64_t ctr, uint64_t offset, uint64_t seed) {
  uint32_t c0 = (uint32_t)ctr, c1 = (uint32_t)(ctr >> 32);
  uint32_t c2 = (uint32_t)offset, c3 = (uint32_t)(offset >> 32);
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {  // Philox-4x32 round
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c0 = n0;
    c1 = n1;
    c2 = n2;
    c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return U4{c0, c1, c2, c3};
}

}  // namespace ema
