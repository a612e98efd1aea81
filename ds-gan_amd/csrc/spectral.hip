// Spectral normalisation of the discriminator's conv weights (--spectral_norm; Miyato et al., ICLR 2018),
// batched over the layers of one discriminator; the function is restated in dsgan_hip/spectral.py.
//
// A layer is one row of a device descriptor table (SN_FIELDS longs, see SnEnt): W [R][C] in the flat
// parameter buffer, the persistent W_sn, u [R], v [C], sigma [1], the temporaries t [C], a [R],
// part [ceil(R C / SN_CHUNK)], the scratch G [R][C] the weight-grad kernels accumulated into, and dW
// (weight_orig.grad in the flat gradient buffer).  blockIdx.y is the layer; a block past its layer's
// extent returns.  fp32 throughout, whatever the precision mode.
//
// Dependent phases are separate launches; inside a launch no block reads what another one writes:
//   refresh   1. t = W^T u            (skipped with iterate == 0)
//             2. a = W v,  v = t / max(|t|, eps) formed on the fly (iterate) or loaded; block 0 stores v
//             3. u = a / max(|a|, eps) (iterate) or loaded; sigma = u . a; W_sn = W / sigma;
//                block 0 stores u and sigma
//   backward  1. part[b] = <G, W_sn> over chunk b
//             2. s = sum_b part[b];  dW += (G - s u v^T) / sigma;  G <- 0
// Every sum has one fixed order that depends on R and C alone (never on the grid, the batch or the
// launch), and the small norms are recomputed by every block that needs them from the same values by
// the same code: two runs, a batched call and single calls, and iterate == 0 after iterate == 1 all
// give the same bits.  No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"

namespace dsg {

constexpr int SN_FIELDS = 12;     // longs per table row
constexpr int SN_CHUNK = 4096;    // elements of W per block in the elementwise phases
constexpr float SN_EPS = 1e-12f;  // torch.nn.utils.spectral_norm's eps

struct SnEnt {
  const float* W; float* Wsn; float* u; float* v; float* sigma; float* t; float* a; float* part;
  float* G; float* dW;
  int R, C;
};

__device__ __forceinline__ SnEnt sn_entry(const long* __restrict__ desc) {
  const long* d = desc + (long)blockIdx.y * SN_FIELDS;
  SnEnt e;
  e.W = (const float*)d[0]; e.Wsn = (float*)d[1]; e.u = (float*)d[2]; e.v = (float*)d[3];
  e.sigma = (float*)d[4]; e.t = (float*)d[5]; e.a = (float*)d[6]; e.part = (float*)d[7];
  e.G = (float*)d[8]; e.dW = (float*)d[9];
  e.R = (int)d[10]; e.C = (int)d[11];
  return e;
}

// sum_{i = tid, tid + 256, ...} f(i) over [0, n), then the block's fixed-order sum: the same bits in
// every block of every launch
template <typename F>
__device__ __forceinline__ float sn_block_reduce(int n, float* sh, F&& f) {
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += f(i);
  return block_sum<256>(s, sh);
}

// 1. t[c] = sum_r W[r][c] u[r].  A block owns 64 columns (lane = column, coalesced rows); wave w adds
// the rows r = w, w + 4, ... in order, and the four wave sums are added in wave order.
__global__ __launch_bounds__(256) void sn_wtu_kernel(const long* __restrict__ desc) {
  const SnEnt e = sn_entry(desc);
  const int c0 = blockIdx.x * 64;
  if (c0 >= e.C) return;
  __shared__ float sh[4][64];
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, c = c0 + l;
  float s = 0.f;
  if (c < e.C) {
    const float* __restrict__ Wc = e.W + c;
#pragma unroll 4
    for (int r = w; r < e.R; r += 4) s += Wc[(long)r * e.C] * e.u[r];
  }
  sh[w][l] = s;
  __syncthreads();
  if (w == 0 && c < e.C) e.t[c] = ((sh[0][l] + sh[1][l]) + sh[2][l]) + sh[3][l];
}

// 2. a[r] = sum_c W[r][c] v[c]: one wave per row, lane l adds c = l, l + 64, ... in order, then the
// butterfly.  iterate: v[c] = t[c] / max(|t|, eps), |t| recomputed by every block; block 0 stores v.
__global__ __launch_bounds__(256) void sn_wv_kernel(const long* __restrict__ desc, int iterate) {
  const SnEnt e = sn_entry(desc);
  const int r0 = blockIdx.x * 4;
  if (r0 >= e.R) return;
  __shared__ float sh[4];
  const float* __restrict__ src = iterate ? e.t : e.v;
  float den = 1.f;
  if (iterate) {
    const float n2 = sn_block_reduce(e.C, sh, [&](int i) { return src[i] * src[i]; });
    den = fmaxf(sqrtf(n2), SN_EPS);
    if (blockIdx.x == 0)
      for (int c = threadIdx.x; c < e.C; c += 256) e.v[c] = src[c] / den;
  }
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, r = r0 + w;
  if (r >= e.R) return;
  const float* __restrict__ Wr = e.W + (long)r * e.C;
  float s = 0.f;
  if (iterate) {
    for (int c = l; c < e.C; c += 64) s += Wr[c] * (src[c] / den);
  } else {
    for (int c = l; c < e.C; c += 64) s += Wr[c] * src[c];
  }
  s = warp_sum(s);
  if (l == 0) e.a[r] = s;
}

// 3. sigma = u . a with u = a / max(|a|, eps) (iterate) or as stored; W_sn = W / sigma over this
// block's chunk.  Every block recomputes sigma from a[] (R <= a few hundred values).
__global__ __launch_bounds__(256) void sn_scale_kernel(const long* __restrict__ desc, int iterate) {
  const SnEnt e = sn_entry(desc);
  const long total = (long)e.R * e.C;
  const long e0 = (long)blockIdx.x * SN_CHUNK;
  if (e0 >= total) return;
  __shared__ float sh[4];
  float den = 1.f;
  if (iterate) {
    const float n2 = sn_block_reduce(e.R, sh, [&](int i) { return e.a[i] * e.a[i]; });
    den = fmaxf(sqrtf(n2), SN_EPS);
  }
  float sigma;
  if (iterate) sigma = sn_block_reduce(e.R, sh, [&](int i) { return (e.a[i] / den) * e.a[i]; });
  else sigma = sn_block_reduce(e.R, sh, [&](int i) { return e.u[i] * e.a[i]; });
  if (blockIdx.x == 0) {
    // (u is read by no block of this launch when it is written: iterate reads a[] alone)
    if (iterate)
      for (int r = threadIdx.x; r < e.R; r += 256) e.u[r] = e.a[r] / den;
    if (threadIdx.x == 0) e.sigma[0] = sigma;
  }
  const long e1 = e0 + SN_CHUNK < total ? e0 + SN_CHUNK : total;
  const bool vec = ((((uintptr_t)e.W) | ((uintptr_t)e.Wsn)) & 15) == 0 && e1 - e0 == SN_CHUNK;
  if (vec) {
    const float4* __restrict__ s4 = (const float4*)(e.W + e0);
    float4* __restrict__ d4 = (float4*)(e.Wsn + e0);
#pragma unroll
    for (int i = threadIdx.x; i < SN_CHUNK / 4; i += 256) {
      float4 x = s4[i];
      x.x /= sigma; x.y /= sigma; x.z /= sigma; x.w /= sigma;
      d4[i] = x;
    }
  } else {
    for (long i = e0 + threadIdx.x; i < e1; i += 256) e.Wsn[i] = e.W[i] / sigma;
  }
}

// backward 1. part[b] = sum over chunk b of G W_sn (thread-strided, then the block's fixed order)
__global__ __launch_bounds__(256) void sn_dot_kernel(const long* __restrict__ desc) {
  const SnEnt e = sn_entry(desc);
  const long total = (long)e.R * e.C;
  const long e0 = (long)blockIdx.x * SN_CHUNK;
  if (e0 >= total) return;
  __shared__ float sh[4];
  const int n = (int)(e0 + SN_CHUNK < total ? SN_CHUNK : total - e0);
  const float* __restrict__ G = e.G + e0;
  const float* __restrict__ Ws = e.Wsn + e0;
  const float s = sn_block_reduce(n, sh, [&](int i) { return G[i] * Ws[i]; });
  if (threadIdx.x == 0) e.part[blockIdx.x] = s;
}

// backward 2. dW[i] += (G[i] - s u[r] v[c]) / sigma, G[i] <- 0, s = the chunks' parts in order
__global__ __launch_bounds__(256) void sn_project_kernel(const long* __restrict__ desc) {
  const SnEnt e = sn_entry(desc);
  const long total = (long)e.R * e.C;
  const long e0 = (long)blockIdx.x * SN_CHUNK;
  if (e0 >= total) return;
  __shared__ float sh[4];
  const int nparts = (int)((total + SN_CHUNK - 1) / SN_CHUNK);
  const float s = sn_block_reduce(nparts, sh, [&](int i) { return e.part[i]; });
  const float sigma = e.sigma[0];
  const long e1 = e0 + SN_CHUNK < total ? e0 + SN_CHUNK : total;
  for (long i = e0 + threadIdx.x; i < e1; i += 256) {
    const int r = (int)(i / e.C), c = (int)(i - (long)r * e.C);
    e.dW[i] += (e.G[i] - s * e.u[r] * e.v[c]) / sigma;
    e.G[i] = 0.f;
  }
}

static int sn_args_ok(const long* desc, int n, int max_r, int max_c) {
  return desc && n >= 1 && n <= 65535 && max_r >= 1 && max_c >= 1 && (long)max_r * max_c <= (1L << 30);
}

}  // namespace dsg

using namespace dsg;

extern "C" {

int dsgan_sn_fields(void) { return SN_FIELDS; }
long dsgan_sn_parts(int R, int C) { return ((long)R * C + SN_CHUNK - 1) / SN_CHUNK; }

int dsgan_sn_refresh(const long* desc, int n, int max_r, int max_c, int iterate, hipStream_t st) {
  DSG_REQUIRE(sn_args_ok(desc, n, max_r, max_c), "dsgan_sn_refresh: bad args");
  const unsigned chunks = cdiv((long)max_r * max_c, SN_CHUNK);
  if (iterate) hipLaunchKernelGGL(sn_wtu_kernel, dim3(cdiv(max_c, 64), (unsigned)n), dim3(256), 0, st, desc);
  hipLaunchKernelGGL(sn_wv_kernel, dim3(cdiv(max_r, 4), (unsigned)n), dim3(256), 0, st, desc, iterate ? 1 : 0);
  hipLaunchKernelGGL(sn_scale_kernel, dim3(chunks, (unsigned)n), dim3(256), 0, st, desc, iterate ? 1 : 0);
  DSG_CHECK_LAUNCH();
  return 0;
}

int dsgan_sn_backward(const long* desc, int n, int max_r, int max_c, hipStream_t st) {
  DSG_REQUIRE(sn_args_ok(desc, n, max_r, max_c), "dsgan_sn_backward: bad args");
  const unsigned chunks = cdiv((long)max_r * max_c, SN_CHUNK);
  hipLaunchKernelGGL(sn_dot_kernel, dim3(chunks, (unsigned)n), dim3(256), 0, st, desc);
  hipLaunchKernelGGL(sn_project_kernel, dim3(chunks, (unsigned)n), dim3(256), 0, st, desc);
  DSG_CHECK_LAUNCH();
  return 0;
}

}
