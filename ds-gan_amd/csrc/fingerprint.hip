// 64-bit fingerprint of a flat buffer of 32-bit words (the resumable-training state check):
//   fp = sum_i mix((i << 32) | bits(word_i))  mod 2^64,  mix = the splitmix64 finaliser.
// Bit patterns, not float values: -0.0 differs from 0.0 and NaN payloads count.  Integer addition
// is associative, so the value depends on neither the grid nor the order of summation.  Two stages
// like dsgan_amp_check (adam.hip): per-block partial sums into the caller's scratch, then one small
// kernel that sums the partials into out.  Read-only on the buffer; no atomics.
#include "common.h"

namespace dsg {
constexpr int FP_PARTS = 1024;
typedef unsigned long long u64;

__device__ __forceinline__ u64 fp_mix(u64 x) {
  u64 z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ u64 fp_term(long i, unsigned w) { return fp_mix(((u64)i << 32) | (u64)w); }

// VEC: the buffer is 16-byte aligned -- each lane loads uint4s, the n % 4 tail words go to the
// first threads.  Otherwise one word per lane (the form dsgan_swap takes for an unaligned pointer).
template <bool VEC>
__global__ __launch_bounds__(256) void fingerprint_kernel(const unsigned* __restrict__ w, long n,
                                                          u64* __restrict__ part) {
  __shared__ u64 sh[4];
  const long tid = blockIdx.x * 256L + threadIdx.x, stride = (long)gridDim.x * 256;
  u64 acc = 0;
  if constexpr (VEC) {
    const long n4 = n >> 2;
    const uint4* w4 = reinterpret_cast<const uint4*>(w);
    for (long i = tid; i < n4; i += stride) {
      const uint4 v = w4[i];
      const long e = i << 2;
      acc += fp_term(e, v.x) + fp_term(e + 1, v.y) + fp_term(e + 2, v.z) + fp_term(e + 3, v.w);
    }
    const long e = (n4 << 2) + tid;
    if (e < n) acc += fp_term(e, w[e]);
  } else {
    for (long e = tid; e < n; e += stride) acc += fp_term(e, w[e]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// out[0] = the sum of the block partials (0 for nparts == 0: the empty buffer)
__global__ __launch_bounds__(64) void fingerprint_sum_kernel(const u64* __restrict__ part, int nparts,
                                                             u64* __restrict__ out) {
  u64 acc = 0;
  for (int i = threadIdx.x; i < nparts; i += 64) acc += part[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (threadIdx.x == 0) out[0] = acc;
}
}  // namespace dsg

using namespace dsg;
extern "C" {
// scratch 64-bit words dsgan_fingerprint needs
long dsgan_fingerprint_parts(void) { return FP_PARTS; }
// out[0] = the fingerprint of n 32-bit words at buf (0 <= n < 2^32); part: part_elems >= dsgan_fingerprint_parts()
int dsgan_fingerprint(const void* buf, long n, unsigned long long* part, long part_elems, unsigned long long* out,
                      hipStream_t st) {
  DSG_REQUIRE(part != nullptr && out != nullptr, "dsgan_fingerprint: part or out is null");
  DSG_REQUIRE(n >= 0 && n < (1L << 32), "dsgan_fingerprint: n = %ld outside [0, 2^32)", n);
  DSG_REQUIRE(buf != nullptr || n == 0, "dsgan_fingerprint: buf is null");
  DSG_REQUIRE(((uintptr_t)buf & 3) == 0, "dsgan_fingerprint: buf is not aligned to its 4-byte words");
  DSG_REQUIRE(part_elems >= FP_PARTS, "dsgan_fingerprint: scratch of %ld words, needs %d", part_elems, FP_PARTS);
  long blocks = 0;
  if (n > 0) {
    blocks = (n + 1023) / 1024;   // four words per lane and trip
    if (blocks > FP_PARTS) blocks = FP_PARTS;
    const unsigned* w = static_cast<const unsigned*>(buf);
    if (((uintptr_t)buf & 15) == 0)
      hipLaunchKernelGGL((fingerprint_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, st, w, n, part);
    else
      hipLaunchKernelGGL((fingerprint_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, st, w, n, part);
  }
  hipLaunchKernelGGL(fingerprint_sum_kernel, dim3(1), dim3(64), 0, st, part, (int)blocks, out);
  DSG_CHECK_LAUNCH();
  return 0;
}
}
