// Philox-4x32-10 (Salmon et al., SC'11): the one counter-based generator of the library (the U-Net's
// dropout, unet.hip; the discriminator's augmentation, diffaug.hip) and the one way its 64-bit seed
// becomes the two key words.
#pragma once
#include <hip/hip_runtime.h>

namespace dsg {

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                              unsigned k1, unsigned (&out)[4]) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// key = the seed's low word, then its high word
struct PhiloxKey {
  unsigned k0, k1;
};
static inline PhiloxKey philox_key(long seed) {
  return PhiloxKey{(unsigned)((unsigned long)seed & 0xFFFFFFFFul), (unsigned)((unsigned long)seed >> 32)};
}

}  // namespace dsg
