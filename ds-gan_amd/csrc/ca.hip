// Channel attention (CA): the per-plane statistics and the shared MLP, forward and backward.
#include "common.h"

namespace dsg {

// ---------------------------------------------------------------------------------------
// CA (DSGAN/models/model/MixConvNeXtML.py:5-22): per-plane avg/max(+argmax), then the tiny
// shared MLP fc2(prelu(fc1(.))) on both, summed, sigmoid.
// ---------------------------------------------------------------------------------------
template <int NT>
__global__ __launch_bounds__(256) void plane_stats_kernel(const float* __restrict__ x, long x_bs,
                                                          float* avg, float* mx, int* amax, int N,
                                                          int C, int HW) {
  __shared__ float shv[4];
  __shared__ int shi[4];
  __shared__ float shs[4];
  const int ppb = 256 / NT;
  const int plane = blockIdx.x * ppb + (NT == 64 ? (threadIdx.x >> 6) : 0);
  const int t = NT == 64 ? (threadIdx.x & 63) : threadIdx.x;
  if (plane >= N * C) return;
  const int n = plane / C, c = plane - n * C;
  const float* xp = x + (long)n * x_bs + (long)c * HW;
  float s = 0.f, best = -INFINITY; int bi = 0x7fffffff;
  for (int i = t; i < HW; i += NT) {
    const float v = xp[i];
    s += v;
    if (v > best || (isnan(v) && !isnan(best))) { best = v; bi = i; }
  }
  // reduce max with smallest index among equal maxima (first occurrence)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    const bool take = (ov > best) || (ov == best && oi < bi) || (isnan(ov) && (!isnan(best) || oi < bi));
    if (take) { best = ov; bi = oi; }
  }
  s = warp_sum(s);
  if (NT == 256) {
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { shv[w] = best; shi[w] = bi; shs[w] = s; }
    __syncthreads();
    if (threadIdx.x == 0) {
      best = shv[0]; bi = shi[0]; s = shs[0];
      for (int i = 1; i < 4; ++i) {
        const bool take = (shv[i] > best) || (shv[i] == best && shi[i] < bi) ||
                          (isnan(shv[i]) && (!isnan(best) || shi[i] < bi));
        if (take) { best = shv[i]; bi = shi[i]; }
        s += shs[i];
      }
    }
  }
  if (t == 0) { avg[plane] = s / (float)HW; mx[plane] = best; amax[plane] = bi; }
}

// One block per sample n.  C <= 1024, R = C/8 <= 128.
__global__ __launch_bounds__(256) void ca_fwd_kernel(const float* avg, const float* mx,
                                                     const float* w1, const float* w2,
                                                     const float* pa, float* att, float* hsave,
                                                     int C, int R) {
  extern __shared__ float sm[];
  float* sa = sm;            // C
  float* sx = sa + C;        // C
  float* hp = sx + C;        // R : prelu(h_avg) + prelu(h_max)
  const int n = blockIdx.x;
  for (int c = threadIdx.x; c < C; c += blockDim.x) { sa[c] = avg[n * C + c]; sx[c] = mx[n * C + c]; }
  __syncthreads();
  const float a = pa[0];
  const int wid = threadIdx.x >> 6, l = threadIdx.x & 63;
  for (int j = wid; j < R; j += blockDim.x / 64) {
    float ha = 0.f, hm = 0.f;
    for (int c = l; c < C; c += 64) { const float w = w1[j * C + c]; ha += w * sa[c]; hm += w * sx[c]; }
    ha = warp_sum(ha); hm = warp_sum(hm);
    if (l == 0) {
      hsave[(n * R + j) * 2 + 0] = ha;
      hsave[(n * R + j) * 2 + 1] = hm;
      hp[j] = (ha >= 0.f ? ha : a * ha) + (hm >= 0.f ? hm : a * hm);
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float o = 0.f;
    for (int j = 0; j < R; ++j) o += w2[c * R + j] * hp[j];
    att[n * C + c] = 1.f / (1.f + __expf(-o));
  }
}

// Backward of CA for one sample per block.  Weight grads go to per-image partials in ws, summed
// over images in a fixed order by launch_split_reduce (deterministic, no atomics).
__global__ __launch_bounds__(256) void ca_bwd_kernel(const float* datt, const float* att,
                                                     const float* avg, const float* mx,
                                                     const float* hsave, const float* w1,
                                                     const float* w2, const float* pa, float* davg,
                                                     float* dmx, float* ws, int want_w1, int want_w2,
                                                     int want_pa, int C, int R) {
  // per-image partials (summed over images in a fixed order by launch_split_reduce):
  // ws = [N][R*C] dw1 | [N][C*R] dw2 | [N] dpa
  extern __shared__ float sm[];
  __shared__ float dal_w[16];
  float* dO = sm;           // C
  float* hp = dO + C;       // R
  float* dha = hp + R;      // R
  float* dhm = dha + R;     // R
  const int n = blockIdx.x;
  const float a = pa[0];
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    const float s = att[n * C + c];
    dO[c] = datt[n * C + c] * s * (1.f - s);
  }
  for (int j = threadIdx.x; j < R; j += blockDim.x) {
    const float ha = hsave[(n * R + j) * 2], hm = hsave[(n * R + j) * 2 + 1];
    hp[j] = (ha >= 0.f ? ha : a * ha) + (hm >= 0.f ? hm : a * hm);
  }
  __syncthreads();
  const int wid = threadIdx.x >> 6, l = threadIdx.x & 63;
  float dal = 0.f;
  for (int j = wid; j < R; j += blockDim.x / 64) {
    float dp = 0.f;
    for (int c = l; c < C; c += 64) dp += w2[c * R + j] * dO[c];
    dp = warp_sum(dp);
    if (l == 0) {
      const float ha = hsave[(n * R + j) * 2], hm = hsave[(n * R + j) * 2 + 1];
      dha[j] = ha > 0.f ? dp : a * dp;
      dhm[j] = hm > 0.f ? dp : a * dp;
      dal += (ha > 0.f ? 0.f : ha * dp) + (hm > 0.f ? 0.f : hm * dp);
    }
  }
  if (l == 0) dal_w[wid] = dal;
  __syncthreads();
  const int N = gridDim.x;
  float* ws_w1 = ws + (long)n * R * C;
  float* ws_w2 = ws + (long)N * R * C + (long)n * C * R;
  if (want_pa && threadIdx.x == 0) {
    float t = 0.f;
    for (int w = 0; w < (int)(blockDim.x / 64); ++w) t += dal_w[w];
    ws[2L * N * R * C + n] = t;
  }
  if (want_w2)
    for (int e = threadIdx.x; e < C * R; e += blockDim.x) ws_w2[e] = dO[e / R] * hp[e % R];
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float ga = 0.f, gm = 0.f;
    const float va = avg[n * C + c], vm = mx[n * C + c];
    for (int j = 0; j < R; ++j) {
      const float w = w1[j * C + c];
      ga += w * dha[j]; gm += w * dhm[j];
      if (want_w1) ws_w1[j * C + c] = dha[j] * va + dhm[j] * vm;
    }
    davg[n * C + c] = ga; dmx[n * C + c] = gm;
  }
}

// dx[n,c,:] += davg/HW ; dx[n,c,argmax] += dmax
// 16-byte forms (HW % 4 == 0, 16-byte aligned planes): each lane walks its float4 groups in increasing
// index order (4 loads in flight), the max / first-argmax update is branch-free with the scalar
// kernel's rule (strict >, NaN wins and sticks), and the cross-lane reduction is the same.
template <int NT>
__global__ __launch_bounds__(256) void plane_stats4_kernel(const float* __restrict__ x, long x_bs, float* avg, float* mx,
                                                           int* amax, int N, int C, int HW) {
  __shared__ float shv[4];
  __shared__ int shi[4];
  __shared__ float shs[4];
  const int ppb = 256 / NT;
  const int plane = blockIdx.x * ppb + (NT == 64 ? (threadIdx.x >> 6) : 0);
  const int t = NT == 64 ? (threadIdx.x & 63) : threadIdx.x;
  if (plane >= N * C) return;
  const int n = plane / C, c = plane - n * C;
  const float4* xp = reinterpret_cast<const float4*>(x + (long)n * x_bs + (long)c * HW);
  const int HW4 = HW >> 2;
  float s = 0.f, best = -INFINITY;
  int bi = 0x7fffffff;
  auto upd = [&](float v, int i) {
    const bool take = v > best || (isnan(v) && !isnan(best));
    best = take ? v : best;
    bi = take ? i : bi;
  };
#pragma unroll 4
  for (int i4 = t; i4 < HW4; i4 += NT) {
    const float4 v = xp[i4];
    s += (v.x + v.y) + (v.z + v.w);
    upd(v.x, 4 * i4); upd(v.y, 4 * i4 + 1); upd(v.z, 4 * i4 + 2); upd(v.w, 4 * i4 + 3);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    const bool take = (ov > best) || (ov == best && oi < bi) || (isnan(ov) && (!isnan(best) || oi < bi));
    if (take) { best = ov; bi = oi; }
  }
  s = warp_sum(s);
  if (NT == 256) {
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { shv[w] = best; shi[w] = bi; shs[w] = s; }
    __syncthreads();
    if (threadIdx.x == 0) {
      best = shv[0]; bi = shi[0]; s = shs[0];
      for (int i = 1; i < 4; ++i) {
        const bool take = (shv[i] > best) || (shv[i] == best && shi[i] < bi) ||
                          (isnan(shv[i]) && (!isnan(best) || shi[i] < bi));
        if (take) { best = shv[i]; bi = shi[i]; }
        s += shs[i];
      }
    }
  }
  if (t == 0) { avg[plane] = s / (float)HW; mx[plane] = best; amax[plane] = bi; }
}

// dx (+)= davg / HW + (i == amax) dmx, four pixels of one plane per thread (HW % 4 == 0, aligned)
__global__ __launch_bounds__(256) void plane_stats_bwd4_kernel(const float* __restrict__ davg, const float* __restrict__ dmx,
                                                               const int* __restrict__ amax, float* __restrict__ dx,
                                                               long dx_bs, int N, int C, int HW) {
  const int HW4 = HW >> 2;
  const long total4 = (long)N * C * HW4;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total4; e += (long)gridDim.x * 256) {
    const long pl = e / HW4;
    const int i4 = (int)(e - pl * HW4);
    const int c = (int)(pl % C), n = (int)(pl / C);
    const float a = davg[pl] / (float)HW, m = dmx[pl];
    const int am = amax[pl] - 4 * i4;
    float4* o = reinterpret_cast<float4*>(dx + (long)n * dx_bs + (long)c * HW) + i4;
    float4 v = *o;
    v.x += am == 0 ? a + m : a; v.y += am == 1 ? a + m : a; v.z += am == 2 ? a + m : a; v.w += am == 3 ? a + m : a;
    *o = v;
  }
}

__global__ void plane_stats_bwd_kernel(const float* davg, const float* dmx, const int* amax,
                                       float* dx, long dx_bs, int N, int C, int HW) {
  const long total = (long)N * C * HW;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int i = e % HW; const long pl = e / HW;
    const int c = pl % C, n = pl / C;
    float v = davg[pl] / (float)HW;
    if (amax[pl] == i) v += dmx[pl];
    dx[(long)n * dx_bs + (long)c * HW + i] += v;
  }
}

}  // namespace dsg

using namespace dsg;

extern "C" {

int dsgan_plane_stats(const float* x, long x_bs, float* avg, float* mx, int* amax, int N, int C,
                      int HW, hipStream_t st) {
  DSG_REQUIRE(x && avg && mx && amax && HW > 0, "dsgan_plane_stats: bad args");
  const int planes = N * C;
  const bool v4 = (HW & 3) == 0 && (x_bs & 3) == 0 && (((uintptr_t)x) & 15) == 0;
  if (v4 && HW <= 4096)
    hipLaunchKernelGGL(plane_stats4_kernel<64>, dim3(cdiv(planes, 4)), dim3(256), 0, st, x, x_bs, avg, mx, amax, N, C, HW);
  else if (v4)
    hipLaunchKernelGGL(plane_stats4_kernel<256>, dim3(planes), dim3(256), 0, st, x, x_bs, avg, mx, amax, N, C, HW);
  else if (HW <= 4096)
    hipLaunchKernelGGL(plane_stats_kernel<64>, dim3(cdiv(planes, 4)), dim3(256), 0, st, x, x_bs, avg, mx, amax, N, C, HW);
  else
    hipLaunchKernelGGL(plane_stats_kernel<256>, dim3(planes), dim3(256), 0, st, x, x_bs, avg, mx, amax, N, C, HW);
  DSG_CHECK_LAUNCH();
  return 0;
}

int dsgan_plane_stats_bwd(const float* davg, const float* dmx, const int* amax, float* dx,
                          long dx_bs, int N, int C, int HW, hipStream_t st) {
  const long total = (long)N * C * HW;
  if ((HW & 3) == 0 && (dx_bs & 3) == 0 && (((uintptr_t)dx) & 15) == 0)
    hipLaunchKernelGGL(plane_stats_bwd4_kernel, dim3(grid_for(total / 4)), dim3(256), 0, st, davg, dmx, amax, dx, dx_bs,
                       N, C, HW);
  else
    hipLaunchKernelGGL(plane_stats_bwd_kernel, dim3(grid_for(total)), dim3(256), 0, st, davg, dmx,
                       amax, dx, dx_bs, N, C, HW);
  DSG_CHECK_LAUNCH();
  return 0;
}

int dsgan_ca_fwd(const float* avg, const float* mx, const float* w1, const float* w2,
                 const float* prelu_a, float* att, float* hsave, int N, int C, int R,
                 hipStream_t st) {
  DSG_REQUIRE(C > 0 && R > 0 && C <= 4096, "dsgan_ca_fwd: bad dims");
  const size_t shm = (2 * C + R) * sizeof(float);
  hipLaunchKernelGGL(ca_fwd_kernel, dim3(N), dim3(256), shm, st, avg, mx, w1, w2, prelu_a, att, hsave, C, R);
  DSG_CHECK_LAUNCH();
  return 0;
}

int dsgan_ca_bwd(const float* datt, const float* att, const float* avg, const float* mx,
                 const float* hsave, const float* w1, const float* w2, const float* prelu_a,
                 float* davg, float* dmx, float* dw1, float* dw2, float* dprelu_a, int N, int C,
                 int R, float* ws, long ws_elems, hipStream_t st) {
  DSG_REQUIRE(N > 0 && C > 0 && R > 0 && C <= 4096, "dsgan_ca_bwd: bad dims");
  DSG_WS((long)N * (2L * R * C + 1), ws, ws_elems, "dsgan_ca_bwd (N*(2*R*C+1) floats)");
  const size_t shm = (C + 3 * R) * sizeof(float);
  hipLaunchKernelGGL(ca_bwd_kernel, dim3(N), dim3(256), shm, st, datt, att, avg, mx, hsave, w1, w2,
                     prelu_a, davg, dmx, ws, dw1 != nullptr, dw2 != nullptr, dprelu_a != nullptr, C, R);
  {   // the three parameter-grad reductions in one launch
    const float* wsv[3];
    int sv[3];
    long mv[3];
    float* dv[3];
    int n = 0;
    if (dw1) { wsv[n] = ws; sv[n] = N; mv[n] = (long)R * C; dv[n] = dw1; ++n; }
    if (dw2) { wsv[n] = ws + (long)N * R * C; sv[n] = N; mv[n] = (long)C * R; dv[n] = dw2; ++n; }
    if (dprelu_a) { wsv[n] = ws + 2L * N * R * C; sv[n] = N; mv[n] = 1; dv[n] = dprelu_a; ++n; }
    if (n) launch_split_reduce_multi(n, wsv, sv, mv, dv, st);
  }
  DSG_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
