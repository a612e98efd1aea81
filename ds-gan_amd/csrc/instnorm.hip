// InstanceNorm (+per-plane scale, +residual, +activation): the scalar, float4, split and 16-bit forms.
//
// InstanceNorm2d(affine=False, eps=1e-5, biased variance) appears 35x in the generator and
// 3x in the PatchGAN D (DSGAN/models/model/MixConvNeXtML.py:54,80,151,158,221,335-420;
// DSGAN/models/networks.py:556,565).  One plane (n,c) is one workgroup (or one wave when the
// plane is small); the activation that follows it (GELU / LeakyReLU(0.2)) and, for MidMLKA
// (:113-116), the CA scaling before it and the residual add after it, are fused in.
#include "common.h"

namespace dsg {

struct INArgs {
  const float* x; long x_bs;
  const float* scale;           // per-plane multiplier [N*C] applied to x first (nullable)
  const float* res; long res_bs;  // residual added after normalisation (nullable)
  float* y; long y_bs;
  float* mean; float* rstd;     // statistics of scale*x, [N*C]
  int N, C, HW, act; float slope, eps;
  int y_bf16;                   // y is 16-bit (1 bf16, 2 fp16; y_bs in elements): the block activation h whose only
                                // consumers are bf16-operand MFMA GEMMs (v4 kernels only)
};

// Plane reduction helper: NT threads per plane (NT = 64: one wave, else the whole block).
template <int NT>
__device__ __forceinline__ float plane_sum(float v, float* sh) {
  if (NT == 64) return warp_sum(v);
  return block_sum<NT>(v, sh);
}

// One plane per workgroup (NT = 256 / 1024) or per wave (NT = 64, 4 planes per 256-thread
// block).  Planes up to NT*CACHE elements are read ONCE into registers (two-pass mean/variance
// from registers); larger planes stream three times.
template <int NT, int CACHE>
__global__ __launch_bounds__(NT == 64 ? 256 : NT) void instnorm_fwd_kernel(INArgs a) {
  __shared__ float sh[16];
  const int planes_per_block = NT == 64 ? 4 : 1;
  const int plane = blockIdx.x * planes_per_block + (NT == 64 ? (threadIdx.x >> 6) : 0);
  const int t = NT == 64 ? (threadIdx.x & 63) : threadIdx.x;
  if (plane >= a.N * a.C) return;  // whole wave / block uniform
  const int n = plane / a.C, c = plane - n * a.C;
  const float* x = a.x + (long)n * a.x_bs + (long)c * a.HW;
  const float s = a.scale ? a.scale[plane] : 1.f;
  float* y = a.y + (long)n * a.y_bs + (long)c * a.HW;
  const float* r = a.res ? a.res + (long)n * a.res_bs + (long)c * a.HW : nullptr;
  const float inv = 1.f / (float)a.HW;
  if (CACHE > 0) {
    float rv[CACHE > 0 ? CACHE : 1];
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < CACHE; ++j) {
      const int i = t + j * NT;
      rv[j] = i < a.HW ? x[i] * s : 0.f;
      sum += rv[j];
    }
    const float mean = plane_sum<NT>(sum, sh) * inv;
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < CACHE; ++j) {
      const float d = rv[j] - mean;
      if (t + j * NT < a.HW) sq += d * d;
    }
    const float rs = 1.f / sqrtf(plane_sum<NT>(sq, sh) * inv + a.eps);
    if (t == 0) { a.mean[plane] = mean; a.rstd[plane] = rs; }
#pragma unroll
    for (int j = 0; j < CACHE; ++j) {
      const int i = t + j * NT;
      if (i < a.HW) {
        float v = (rv[j] - mean) * rs;
        if (r) v += r[i];
        y[i] = act_f(a.act, v, a.slope);
      }
    }
  } else {
    float sum = 0.f;
    for (int i = t; i < a.HW; i += NT) sum += x[i] * s;
    const float mean = plane_sum<NT>(sum, sh) * inv;
    float sq = 0.f;
    for (int i = t; i < a.HW; i += NT) { const float d = x[i] * s - mean; sq += d * d; }
    const float rs = 1.f / sqrtf(plane_sum<NT>(sq, sh) * inv + a.eps);
    if (t == 0) { a.mean[plane] = mean; a.rstd[plane] = rs; }
    for (int i = t; i < a.HW; i += NT) {
      float v = (x[i] * s - mean) * rs;
      if (r) v += r[i];
      y[i] = act_f(a.act, v, a.slope);
    }
  }
}

struct INBwdArgs {
  const float* dy; long dy_bs;
  const float* x; long x_bs;
  const float* scale;
  const float* res; long res_bs;
  const float* mean; const float* rstd;
  float* dx; long dx_bs;
  float* dres; long dres_bs;   // nullable
  float* dscale;               // nullable, [N*C] (written)
  int N, C, HW, act; float slope, eps;
  void* dxh;                   // nullable: dx stored 16-bit (the library half type) here instead of dx
  float* dxsum;                // nullable, [N*C]: per-plane sum of the fp32 dx (before rounding)
  int half;                    // half type of dxh (HALF_BF16 / HALF_F16)
};

// y = act(xhat + res), xhat = (s*x - mean) * rstd
// g = dy * act'(xhat + res);  dres = g;  dxs = rstd * (g - mean(g) - xhat * mean(g * xhat))
// dx = s * dxs;  dscale = sum_p dxs * x.  The sum cancels to O(eps) (IN is scale invariant up to
// eps), so it is evaluated in closed form: sum dxs = 0 and sum xhat^2 = HW*var*rstd^2 give
//   dscale = mean(g*xhat) * HW * eps * rstd^2 / s
// which is what the fp64 reference converges to; the direct fp32 sum loses ~1e-3 relative.
// g is cached in registers (planes <= NT*CACHE); xhat is recomputed from x in the final pass.
template <int NT, int CACHE>
__global__ __launch_bounds__(NT == 64 ? 256 : NT) void instnorm_bwd_kernel(INBwdArgs a) {
  __shared__ float sh[16];
  const int planes_per_block = NT == 64 ? 4 : 1;
  const int plane = blockIdx.x * planes_per_block + (NT == 64 ? (threadIdx.x >> 6) : 0);
  const int t = NT == 64 ? (threadIdx.x & 63) : threadIdx.x;
  if (plane >= a.N * a.C) return;
  const int n = plane / a.C, c = plane - n * a.C;
  const long po = (long)c * a.HW;
  const float* x = a.x + (long)n * a.x_bs + po;
  const float* dy = a.dy + (long)n * a.dy_bs + po;
  const float* r = a.res ? a.res + (long)n * a.res_bs + po : nullptr;
  float* dres = a.dres ? a.dres + (long)n * a.dres_bs + po : nullptr;
  const float s = a.scale ? a.scale[plane] : 1.f;
  const float mean = a.mean[plane], rs = a.rstd[plane];
  float* dx = a.dx + (long)n * a.dx_bs + po;
  auto grad_at = [&](int i, float& xh) -> float {
    xh = (x[i] * s - mean) * rs;
    float g = dy[i];
    if (a.act != ACT_NONE) g *= act_g(a.act, r ? xh + r[i] : xh, a.slope);
    if (dres) dres[i] = g;
    return g;
  };
  const float inv = 1.f / (float)a.HW;
  float sg = 0.f, sgh = 0.f;
  if (CACHE > 0) {
    float gv[CACHE > 0 ? CACHE : 1];
#pragma unroll
    for (int j = 0; j < CACHE; ++j) {
      const int i = t + j * NT;
      gv[j] = 0.f;
      if (i < a.HW) { float xh; gv[j] = grad_at(i, xh); sg += gv[j]; sgh += gv[j] * xh; }
    }
    const float mg = plane_sum<NT>(sg, sh) * inv;
    const float mgh = plane_sum<NT>(sgh, sh) * inv;
#pragma unroll
    for (int j = 0; j < CACHE; ++j) {
      const int i = t + j * NT;
      if (i < a.HW) {
        const float xh = (x[i] * s - mean) * rs;
        dx[i] = s * rs * (gv[j] - mg - xh * mgh);
      }
    }
    if (a.dscale && t == 0) a.dscale[plane] = mgh * (float)a.HW * a.eps * rs * rs / s;
  } else {
    for (int i = t; i < a.HW; i += NT) { float xh; const float g = grad_at(i, xh); sg += g; sgh += g * xh; }
    const float mg = plane_sum<NT>(sg, sh) * inv;
    const float mgh = plane_sum<NT>(sgh, sh) * inv;
    for (int i = t; i < a.HW; i += NT) {
      const float xh = (x[i] * s - mean) * rs;
      float g = dy[i];
      if (a.act != ACT_NONE) g *= act_g(a.act, r ? xh + r[i] : xh, a.slope);
      dx[i] = s * rs * (g - mg - xh * mgh);
    }
    if (a.dscale && t == 0) a.dscale[plane] = mgh * (float)a.HW * a.eps * rs * rs / s;
  }
}

// ---- float4 forms (HW % 4 == 0, 16-byte aligned planes: every G/D plane but PatchGAN's 31x31) ----
// Same math as above with 16-byte accesses: the scalar forms issue 256-byte wave loads and
// reach only 2-4 TB/s on 64K/16K-pixel planes.  C4 float4s per thread are cached in registers
// (C4 == 0: the plane streams, three passes fwd / five bwd); the bwd caches g and, with CX,
// xhat too (x is then read once).
template <int NT>
__device__ __forceinline__ float2 plane_sum2(float u, float v, float* sh) {
  u = warp_sum(u);
  v = warp_sum(v);
  if (NT == 64) return make_float2(u, v);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0) { sh[w] = u; sh[NT / 64 + w] = v; }
  __syncthreads();
  float2 r = make_float2(0.f, 0.f);
#pragma unroll
  for (int i = 0; i < NT / 64; ++i) { r.x += sh[i]; r.y += sh[NT / 64 + i]; }
  return r;
}

__device__ __forceinline__ float hsum4(float4 v) { return (v.x + v.y) + (v.z + v.w); }

// instnorm_fwd_v4's unguarded case: a plane of exactly C4 <= 4 float4s per thread (the kernel and
// dsgan_instnorm_plan both ask this)
__host__ __device__ constexpr bool in_fwd_v4_full(int NT, int C4, int HW4) { return C4 > 0 && C4 <= 4 && HW4 == C4 * NT; }

template <int NT, int C4>
__global__ __launch_bounds__(NT == 64 ? 256 : NT) void instnorm_fwd_v4(INArgs a) {
  __shared__ float sh[32];
  const int plane = blockIdx.x * (NT == 64 ? 4 : 1) + (NT == 64 ? (threadIdx.x >> 6) : 0);
  const int t = NT == 64 ? (threadIdx.x & 63) : threadIdx.x;
  if (plane >= a.N * a.C) return;
  const int n = plane / a.C, c = plane - n * a.C;
  const int HW4 = a.HW >> 2;
  const float4* x = reinterpret_cast<const float4*>(a.x + (long)n * a.x_bs + (long)c * a.HW);
  float4* y = reinterpret_cast<float4*>(a.y + (long)n * a.y_bs + (long)c * a.HW);
  const float4* r = a.res ? reinterpret_cast<const float4*>(a.res + (long)n * a.res_bs + (long)c * a.HW) : nullptr;
  const float s = a.scale ? a.scale[plane] : 1.f;
  const float inv = 1.f / (float)a.HW;
  auto out = [&](int i, float4 v, float mean, float rs) {
    v.x = (v.x - mean) * rs; v.y = (v.y - mean) * rs; v.z = (v.z - mean) * rs; v.w = (v.w - mean) * rs;
    if (r) { const float4 q = r[i]; v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w; }
    v.x = act_f(a.act, v.x, a.slope); v.y = act_f(a.act, v.y, a.slope);
    v.z = act_f(a.act, v.z, a.slope); v.w = act_f(a.act, v.w, a.slope);
    if (a.y_bf16 == 2) {   // fp16 (--precision fp16), round-to-nearest-even like the GEMMs' operand loads
      hx4<_Float16> hv = {(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};
      reinterpret_cast<hx4<_Float16>*>(reinterpret_cast<_Float16*>(a.y) + (long)n * a.y_bs + (long)c * a.HW)[i] = hv;
    } else if (a.y_bf16) {   // bf16, round-to-nearest-even, the same rounding the GEMMs apply to fp32 operands
      hx4<__bf16> hv = {(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w};
      reinterpret_cast<hx4<__bf16>*>(reinterpret_cast<__bf16*>(a.y) + (long)n * a.y_bs + (long)c * a.HW)[i] = hv;
    } else {
      y[i] = v;
    }
  };
  auto ld = [&](int i) -> float4 {
    float4 v = x[i];
    v.x *= s; v.y *= s; v.z *= s; v.w *= s;
    return v;
  };
  if constexpr (C4 > 0) {
    float4 rv[C4];
    float sum = 0.f;
    // a plane of exactly C4 = 4 float4s per thread takes unguarded loads and stores (the same values
    // in the same order: same bits).  Build A/B on two boxes (profiles/r04/in_micro_full*.txt): the
    // 4K-pixel planes of the 256 x 4 form 45 -> 42 us (1024 @ 32^2: 24 -> 22) on both; with C4 = 16
    // the 16K-pixel planes went 108 -> 113 us on one box and the 64K-pixel ones -4 % on one box,
    // +2.5 % on the other, so those keep the guarded loop.
    const bool full = in_fwd_v4_full(NT, C4, HW4);
    if (full) {
#pragma unroll
      for (int j = 0; j < C4; ++j) rv[j] = ld(t + j * NT);
    } else {
#pragma unroll
      for (int j = 0; j < C4; ++j) {
        const int i = t + j * NT;
        rv[j] = i < HW4 ? ld(i) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
#pragma unroll
    for (int j = 0; j < C4; ++j) sum += hsum4(rv[j]);
    const float mean = plane_sum<NT>(sum, sh) * inv;
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < C4; ++j) {
      if (t + j * NT < HW4) {
        const float dx = rv[j].x - mean, dy = rv[j].y - mean, dz = rv[j].z - mean, dw = rv[j].w - mean;
        sq += (dx * dx + dy * dy) + (dz * dz + dw * dw);
      }
    }
    const float rs = 1.f / sqrtf(plane_sum<NT>(sq, sh) * inv + a.eps);
    if (t == 0) { a.mean[plane] = mean; a.rstd[plane] = rs; }
    if (full) {
#pragma unroll
      for (int j = 0; j < C4; ++j) out(t + j * NT, rv[j], mean, rs);
    } else {
#pragma unroll
      for (int j = 0; j < C4; ++j) {
        const int i = t + j * NT;
        if (i < HW4) out(i, rv[j], mean, rs);
      }
    }
  } else {
    float sum = 0.f;
    for (int i0 = t; i0 < HW4; i0 += 4 * NT) {
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = i0 + u * NT < HW4 ? ld(i0 + u * NT) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int u = 0; u < 4; ++u) sum += hsum4(v[u]);
    }
    const float mean = plane_sum<NT>(sum, sh) * inv;
    float sq = 0.f;
    for (int i0 = t; i0 < HW4; i0 += 4 * NT) {
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = i0 + u * NT < HW4 ? ld(i0 + u * NT) : make_float4(mean, mean, mean, mean);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float dx = v[u].x - mean, dy = v[u].y - mean, dz = v[u].z - mean, dw = v[u].w - mean;
        sq += (dx * dx + dy * dy) + (dz * dz + dw * dw);
      }
    }
    const float rs = 1.f / sqrtf(plane_sum<NT>(sq, sh) * inv + a.eps);
    if (t == 0) { a.mean[plane] = mean; a.rstd[plane] = rs; }
    for (int i0 = t; i0 < HW4; i0 += 4 * NT) {
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) if (i0 + u * NT < HW4) v[u] = ld(i0 + u * NT);
#pragma unroll
      for (int u = 0; u < 4; ++u) if (i0 + u * NT < HW4) out(i0 + u * NT, v[u], mean, rs);
    }
  }
}

// XL (> 0 only with !CX): the first XL of a thread's C4 xhat float4s are parked in LDS between the
// statistics pass and the output pass instead of being recomputed from a second read of x.  The
// 64K-pixel planes (NT = 1024, C4 = 16) cannot hold xhat in registers next to g, and a plane of x
// (256 KB) does not stay in the CU's share of L2, so the second read went to HBM: XL = 8 keeps half
// of it in 128 KB of LDS (the workgroup is alone on its CU either way).  Same values, same bits.
// ACTT >= 0: the activation fixed at compile time (the launcher dispatches on a.act), so the cached
// form's loop body has no branches and the scheduler can keep several items' loads in flight.
template <int NT, int C4, bool CX, int XL = 0, int ACTT = -1>
__global__ __launch_bounds__(NT == 64 ? 256 : NT) void instnorm_bwd_v4(INBwdArgs a) {
  static_assert(XL == 0 || (!CX && XL <= C4 && NT > 64), "XL: LDS-parked xhat of the uncached form");
  __shared__ float sh[32];
  __shared__ float4 xl[XL > 0 ? XL * NT : 1];
  const int plane = blockIdx.x * (NT == 64 ? 4 : 1) + (NT == 64 ? (threadIdx.x >> 6) : 0);
  const int t = NT == 64 ? (threadIdx.x & 63) : threadIdx.x;
  if (plane >= a.N * a.C) return;
  const int n = plane / a.C, c = plane - n * a.C;
  const long po = (long)c * a.HW;
  const int HW4 = a.HW >> 2;
  const float4* x = reinterpret_cast<const float4*>(a.x + (long)n * a.x_bs + po);
  const float4* dy = reinterpret_cast<const float4*>(a.dy + (long)n * a.dy_bs + po);
  const float4* r = a.res ? reinterpret_cast<const float4*>(a.res + (long)n * a.res_bs + po) : nullptr;
  float4* dres = a.dres ? reinterpret_cast<float4*>(a.dres + (long)n * a.dres_bs + po) : nullptr;
  float4* dx = reinterpret_cast<float4*>(a.dx + (long)n * a.dx_bs + po);
  const float s = a.scale ? a.scale[plane] : 1.f;
  const float mean = a.mean[plane], rs = a.rstd[plane];
  const float inv = 1.f / (float)a.HW;
  auto xhat = [&](int i) -> float4 {
    float4 v = x[i];
    v.x = (v.x * s - mean) * rs; v.y = (v.y * s - mean) * rs; v.z = (v.z * s - mean) * rs; v.w = (v.w * s - mean) * rs;
    return v;
  };
  auto grad = [&](int i, float4 xh) -> float4 {
    float4 g = dy[i];
    if (a.act != ACT_NONE) {
      float4 z = xh;
      if (r) { const float4 q = r[i]; z.x += q.x; z.y += q.y; z.z += q.z; z.w += q.w; }
      g.x *= act_g(a.act, z.x, a.slope); g.y *= act_g(a.act, z.y, a.slope);
      g.z *= act_g(a.act, z.z, a.slope); g.w *= act_g(a.act, z.w, a.slope);
    }
    if (dres) dres[i] = g;
    return g;
  };
  // 16-bit dx (dxh): its only readers are 16-bit-operand MFMA kernels, which round it the same way
  unsigned short* dxh = a.dxh ? reinterpret_cast<unsigned short*>(a.dxh) + (long)n * a.dx_bs + po : nullptr;
  float dsum = 0.f;
  auto fin = [&](int i, float4 g, float4 xh, float mg, float mgh) {
    const float k = s * rs;
    const float4 v = make_float4(k * (g.x - mg - xh.x * mgh), k * (g.y - mg - xh.y * mgh), k * (g.z - mg - xh.z * mgh),
                                 k * (g.w - mg - xh.w * mgh));
    if (dxh) {
      uint2 u;
      if (a.half == HALF_F16) {
        u.x = (unsigned)f2h<_Float16>(v.x) | ((unsigned)f2h<_Float16>(v.y) << 16);
        u.y = (unsigned)f2h<_Float16>(v.z) | ((unsigned)f2h<_Float16>(v.w) << 16);
      } else {
        u.x = (unsigned)f2h<__bf16>(v.x) | ((unsigned)f2h<__bf16>(v.y) << 16);
        u.y = (unsigned)f2h<__bf16>(v.z) | ((unsigned)f2h<__bf16>(v.w) << 16);
      }
      *reinterpret_cast<uint2*>(dxh + 4 * i) = u;
      dsum += hsum4(v);
    } else {
      dx[i] = v;
    }
  };
  float sg = 0.f, sgh = 0.f;
  float2 m;
  if constexpr (C4 > 0 && NT == 1024) {
    // (64K-pixel planes: the scheduled form below spills at this size's 128-register cap, so the
    // item loop keeps its guarded per-item order; XL parks half of xhat in LDS instead)
    float4 gv[C4];
#pragma unroll
    for (int j = 0; j < C4; ++j) {
      const int i = t + j * NT;
      gv[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (i < HW4) {
        const float4 xh = xhat(i);
        if constexpr (XL > 0) {
          if (j < XL) xl[j * NT + t] = xh;
        }
        gv[j] = grad(i, xh);
        sg += hsum4(gv[j]);
        sgh += (gv[j].x * xh.x + gv[j].y * xh.y) + (gv[j].z * xh.z + gv[j].w * xh.w);
      }
    }
    m = plane_sum2<NT>(sg, sgh, sh);
    m.x *= inv; m.y *= inv;
#pragma unroll
    for (int j = 0; j < C4; ++j) {
      const int i = t + j * NT;
      if (i < HW4) {
        if (XL > 0 && j < XL) fin(i, gv[j], xl[j * NT + t], m.x, m.y);
        else fin(i, gv[j], xhat(i), m.x, m.y);
      }
    }
  } else if constexpr (C4 > 0) {
    // Loads through plane-sized buffer resources (an item past the plane reads 0: no guard, no
    // branch), the activation fixed at compile time, and no global store inside the statistics loop
    // (dres is written afterwards).  A guarded load sits in its own basic block, and a load after a
    // store may not be hoisted above it: each item had waited one memory latency.  Same values and
    // the same summation order (an out-of-plane item adds +0): same bits.
    const int act = ACTT >= 0 ? ACTT : a.act;
    const unsigned prange = (unsigned)a.HW * 4u;
    const __amdgpu_buffer_rsrc_t bx = buf_rsrc(x, prange);
    const __amdgpu_buffer_rsrc_t bd = buf_rsrc(dy, prange);
    const __amdgpu_buffer_rsrc_t br = buf_rsrc(r ? (void*)r : (void*)dy, r ? prange : 0u);
    auto bld4 = [](__amdgpu_buffer_rsrc_t rc, int i) {
      return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rc, i * 16, 0, 0));
    };
    auto bxhat = [&](int i) -> float4 {
      float4 v = bld4(bx, i);
      v.x = (v.x * s - mean) * rs; v.y = (v.y * s - mean) * rs; v.z = (v.z * s - mean) * rs; v.w = (v.w * s - mean) * rs;
      return v;
    };
    float4 gv[C4];
    float4 xv[CX ? C4 : 1];
#pragma unroll
    for (int j = 0; j < C4; ++j) {
      const int i = t + j * NT;
      const float4 xh = bxhat(i);
      float4 g = bld4(bd, i);
      if (act != ACT_NONE) {
        float4 z = xh;
        // (no residual: a zero-range buffer reads 0 and z stays xhat -- no branch, no traffic)
        const float4 q = bld4(br, i);
        z.x += q.x; z.y += q.y; z.z += q.z; z.w += q.w;
        g.x *= act_g(act, z.x, a.slope); g.y *= act_g(act, z.y, a.slope);
        g.z *= act_g(act, z.z, a.slope); g.w *= act_g(act, z.w, a.slope);
      }
      gv[j] = g;
      if constexpr (CX) xv[j] = xh;
      if constexpr (XL > 0) {
        if (j < XL) xl[j * NT + t] = xh;
      }
      sg += hsum4(g);
      sgh += (g.x * xh.x + g.y * xh.y) + (g.z * xh.z + g.w * xh.w);
    }
    if (dres) {
#pragma unroll
      for (int j = 0; j < C4; ++j)
        if (t + j * NT < HW4) dres[t + j * NT] = gv[j];
    }
    m = plane_sum2<NT>(sg, sgh, sh);
    m.x *= inv; m.y *= inv;
    // the recomputed xhat of the uncached items, in groups of FG loaded before their stores
    constexpr int FG = 4;
#pragma unroll
    for (int j0 = 0; j0 < C4; j0 += FG) {
      float4 xq[FG];
      if constexpr (!CX) {
#pragma unroll
        for (int u = 0; u < FG && j0 + u < C4; ++u) {
          const int i = t + (j0 + u) * NT;
          if (!(XL > 0 && j0 + u < XL)) xq[u] = bxhat(i);
        }
      }
#pragma unroll
      for (int u = 0; u < FG && j0 + u < C4; ++u) {
        const int j = j0 + u, i = t + j * NT;
        if (i < HW4) {
          if constexpr (CX) fin(i, gv[j], xv[j], m.x, m.y);
          else if (XL > 0 && j < XL) fin(i, gv[j], xl[j * NT + t], m.x, m.y);
          else fin(i, gv[j], xq[u], m.x, m.y);
        }
      }
    }
  } else {
    for (int i0 = t; i0 < HW4; i0 += 2 * NT) {
      float4 xh[2], g[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) if (i0 + u * NT < HW4) xh[u] = xhat(i0 + u * NT);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (i0 + u * NT < HW4) {
          g[u] = grad(i0 + u * NT, xh[u]);
          sg += hsum4(g[u]);
          sgh += (g[u].x * xh[u].x + g[u].y * xh[u].y) + (g[u].z * xh[u].z + g[u].w * xh[u].w);
        }
      }
    }
    m = plane_sum2<NT>(sg, sgh, sh);
    m.x *= inv; m.y *= inv;
    for (int i0 = t; i0 < HW4; i0 += 2 * NT) {
      float4 xh[2], g[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (i0 + u * NT < HW4) {
          xh[u] = xhat(i0 + u * NT);
          g[u] = dy[i0 + u * NT];
        }
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (i0 + u * NT < HW4) {
          if (a.act != ACT_NONE) {
            float4 z = xh[u];
            if (r) { const float4 q = r[i0 + u * NT]; z.x += q.x; z.y += q.y; z.z += q.z; z.w += q.w; }
            g[u].x *= act_g(a.act, z.x, a.slope); g[u].y *= act_g(a.act, z.y, a.slope);
            g[u].z *= act_g(a.act, z.z, a.slope); g[u].w *= act_g(a.act, z.w, a.slope);
          }
          fin(i0 + u * NT, g[u], xh[u], m.x, m.y);
        }
      }
    }
  }
  if (a.dscale && t == 0) a.dscale[plane] = m.y * (float)a.HW * a.eps * rs * rs / s;
  if (a.dxsum) {   // (uniform branch: every thread of the plane's block reaches the reduction)
    const float2 ds = plane_sum2<NT>(dsum, 0.f, sh);
    if (t == 0) a.dxsum[plane] = ds.x;
  }
}

// xhat float4s per thread parked in LDS by the 64K-pixel backward (instnorm_bwd_v4 XL; A/B in
// profiles/r04/in_micro_xl.txt: 8 of 16, 128 KB of LDS)
constexpr int IN_BWD_XL = 8;

// ---- few-plane forms: one plane split over S workgroups ----
// The generator's 3-channel block (MixConvNeXtML.py:220-221 at dim 3) normalises N*3 = 48 planes
// of 64K pixels: a workgroup per plane keeps 48 of the 256 CUs busy (72.6 us at 0.35 TB/s,
// profiles/r04/launches_c.txt).  Here each plane's S chunks (IN_SPLIT_F4 float4s, 4 per thread)
// are separate workgroups; the plane statistics are summed from per-chunk partials in a fixed
// order, so the result is deterministic (it is not the one-workgroup kernel's summation order).
// fwd: partial sums -> partial squared deviations -> output; bwd: partial (sum g, sum g*xhat) -> dx.
constexpr int IN_SPLIT_F4 = 1024;

static inline int in_split_chunks(long planes, int HW) {
  if ((HW & 3) || planes >= 128 || HW < 16384) return 0;
  return (int)cdiv(HW >> 2, IN_SPLIT_F4);
}

__device__ __forceinline__ float in_split_total(const float* p, int S, int stride) {
  float r = 0.f;
  for (int k = 0; k < S; ++k) r += p[k * stride];
  return r;
}

// PASS 0: ws[plane*S + k] = sum of s*x over chunk k;  PASS 1: ws[P*S + plane*S + k] = sum of (s*x - mean)^2
template <int PASS>
__global__ __launch_bounds__(256) void in_split_stat(INArgs a, float* __restrict__ ws, int S) {
  __shared__ float sh[4];
  const int k = blockIdx.x, plane = blockIdx.y, P = a.N * a.C;
  const int n = plane / a.C, c = plane - n * a.C;
  const int HW4 = a.HW >> 2;
  const float4* x = reinterpret_cast<const float4*>(a.x + (long)n * a.x_bs + (long)c * a.HW);
  const float s = a.scale ? a.scale[plane] : 1.f;
  const float mean = PASS ? in_split_total(ws + (long)plane * S, S, 1) * (1.f / (float)a.HW) : 0.f;
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < IN_SPLIT_F4 / 256; ++j) {
    const int i = k * IN_SPLIT_F4 + j * 256 + threadIdx.x;
    if (i < HW4) {
      float4 v = x[i];
      v.x *= s; v.y *= s; v.z *= s; v.w *= s;
      if (PASS == 0) {
        acc += hsum4(v);
      } else {
        const float dx = v.x - mean, dy = v.y - mean, dz = v.z - mean, dw = v.w - mean;
        acc += (dx * dx + dy * dy) + (dz * dz + dw * dw);
      }
    }
  }
  acc = block_sum<256>(acc, sh);
  if (threadIdx.x == 0) ws[(long)PASS * P * S + (long)plane * S + k] = acc;
}

__global__ __launch_bounds__(256) void in_split_out(INArgs a, const float* __restrict__ ws, int S) {
  const int k = blockIdx.x, plane = blockIdx.y, P = a.N * a.C;
  const int n = plane / a.C, c = plane - n * a.C;
  const int HW4 = a.HW >> 2;
  const long po = (long)c * a.HW;
  const float inv = 1.f / (float)a.HW;
  const float mean = in_split_total(ws + (long)plane * S, S, 1) * inv;
  const float rs = 1.f / sqrtf(in_split_total(ws + (long)P * S + (long)plane * S, S, 1) * inv + a.eps);
  if (k == 0 && threadIdx.x == 0) { a.mean[plane] = mean; a.rstd[plane] = rs; }
  const float4* x = reinterpret_cast<const float4*>(a.x + (long)n * a.x_bs + po);
  const float4* r = a.res ? reinterpret_cast<const float4*>(a.res + (long)n * a.res_bs + po) : nullptr;
  const float s = a.scale ? a.scale[plane] : 1.f;
#pragma unroll
  for (int j = 0; j < IN_SPLIT_F4 / 256; ++j) {
    const int i = k * IN_SPLIT_F4 + j * 256 + threadIdx.x;
    if (i >= HW4) continue;
    float4 v = x[i];
    v.x = (v.x * s - mean) * rs; v.y = (v.y * s - mean) * rs; v.z = (v.z * s - mean) * rs; v.w = (v.w * s - mean) * rs;
    if (r) { const float4 q = r[i]; v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w; }
    v.x = act_f(a.act, v.x, a.slope); v.y = act_f(a.act, v.y, a.slope);
    v.z = act_f(a.act, v.z, a.slope); v.w = act_f(a.act, v.w, a.slope);
    if (a.y_bf16 == 2) {
      hx4<_Float16> hv = {(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};
      reinterpret_cast<hx4<_Float16>*>(reinterpret_cast<_Float16*>(a.y) + (long)n * a.y_bs + po)[i] = hv;
    } else if (a.y_bf16) {
      hx4<__bf16> hv = {(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w};
      reinterpret_cast<hx4<__bf16>*>(reinterpret_cast<__bf16*>(a.y) + (long)n * a.y_bs + po)[i] = hv;
    } else {
      reinterpret_cast<float4*>(a.y + (long)n * a.y_bs + po)[i] = v;
    }
  }
}

// g = dy * act'(xhat + res) (dres = g written here);  ws[(plane*S + k)*2 + {0,1}] = chunk sums of g, g*xhat
__device__ __forceinline__ float4 in_split_g(const INBwdArgs& a, int n, long po, int i, float4 xh) {
  float4 g = reinterpret_cast<const float4*>(a.dy + (long)n * a.dy_bs + po)[i];
  if (a.act != ACT_NONE) {
    float4 z = xh;
    if (a.res) {
      const float4 q = reinterpret_cast<const float4*>(a.res + (long)n * a.res_bs + po)[i];
      z.x += q.x; z.y += q.y; z.z += q.z; z.w += q.w;
    }
    g.x *= act_g(a.act, z.x, a.slope); g.y *= act_g(a.act, z.y, a.slope);
    g.z *= act_g(a.act, z.z, a.slope); g.w *= act_g(a.act, z.w, a.slope);
  }
  return g;
}

template <int PASS>   // 0: partial sums (+ dres);  1: dx (+ dscale)
__global__ __launch_bounds__(256) void in_split_bwd(INBwdArgs a, float* __restrict__ ws, int S) {
  __shared__ float sh[8];
  const int k = blockIdx.x, plane = blockIdx.y;
  const int n = plane / a.C, c = plane - n * a.C;
  const int HW4 = a.HW >> 2;
  const long po = (long)c * a.HW;
  const float4* x = reinterpret_cast<const float4*>(a.x + (long)n * a.x_bs + po);
  const float s = a.scale ? a.scale[plane] : 1.f;
  const float mean = a.mean[plane], rs = a.rstd[plane];
  const float inv = 1.f / (float)a.HW;
  float mg = 0.f, mgh = 0.f;
  if (PASS == 1) {
    mg = in_split_total(ws + (long)plane * S * 2, S, 2) * inv;
    mgh = in_split_total(ws + (long)plane * S * 2 + 1, S, 2) * inv;
  }
  float sg = 0.f, sgh = 0.f;
#pragma unroll
  for (int j = 0; j < IN_SPLIT_F4 / 256; ++j) {
    const int i = k * IN_SPLIT_F4 + j * 256 + threadIdx.x;
    if (i >= HW4) continue;
    float4 xh = x[i];
    xh.x = (xh.x * s - mean) * rs; xh.y = (xh.y * s - mean) * rs; xh.z = (xh.z * s - mean) * rs; xh.w = (xh.w * s - mean) * rs;
    const float4 g = in_split_g(a, n, po, i, xh);
    if (PASS == 0) {
      if (a.dres) reinterpret_cast<float4*>(a.dres + (long)n * a.dres_bs + po)[i] = g;
      sg += hsum4(g);
      sgh += (g.x * xh.x + g.y * xh.y) + (g.z * xh.z + g.w * xh.w);
    } else {
      const float kk = s * rs;
      reinterpret_cast<float4*>(a.dx + (long)n * a.dx_bs + po)[i] =
          make_float4(kk * (g.x - mg - xh.x * mgh), kk * (g.y - mg - xh.y * mgh), kk * (g.z - mg - xh.z * mgh),
                      kk * (g.w - mg - xh.w * mgh));
    }
  }
  if (PASS == 0) {
    const float2 m = plane_sum2<256>(sg, sgh, sh);
    if (threadIdx.x == 0) { ws[((long)plane * S + k) * 2] = m.x; ws[((long)plane * S + k) * 2 + 1] = m.y; }
  } else if (a.dscale && k == 0 && threadIdx.x == 0) {
    a.dscale[plane] = mgh * (float)a.HW * a.eps * rs * rs / s;
  }
}

// the cached IN backward forms instantiated per activation (ACTT, see instnorm_bwd_v4)
template <int NT, int C4, bool CX, int XL = 0>
static void in_bwd_launch(const INBwdArgs& a, dim3 grid, dim3 block, hipStream_t st) {
  switch (a.act) {
    case ACT_NONE: hipLaunchKernelGGL((instnorm_bwd_v4<NT, C4, CX, XL, ACT_NONE>), grid, block, 0, st, a); break;
    case ACT_GELU: hipLaunchKernelGGL((instnorm_bwd_v4<NT, C4, CX, XL, ACT_GELU>), grid, block, 0, st, a); break;
    case ACT_LRELU: hipLaunchKernelGGL((instnorm_bwd_v4<NT, C4, CX, XL, ACT_LRELU>), grid, block, 0, st, a); break;
    case ACT_GELU_FAST:
      hipLaunchKernelGGL((instnorm_bwd_v4<NT, C4, CX, XL, ACT_GELU_FAST>), grid, block, 0, st, a);
      break;
    default: hipLaunchKernelGGL((instnorm_bwd_v4<NT, C4, CX, XL>), grid, block, 0, st, a); break;
  }
}

// ---- launch plans: each plane-size ladder is stated once, and every entry point goes through it ----
// float4 InstanceNorm kernels (16-byte aligned planes); planes up to 64K pixels are cached in
// registers between the statistics and the normalise pass (measured 1.45x faster fwd and bwd
// than streaming them twice).  Unaligned planes take the scalar kernels.
static bool in_fwd_v4_ok(const INArgs& a) {   // (y: fp32 or 16-bit, the test is the same)
  return (a.HW & 3) == 0 && al16(a.x, a.x_bs) && al16(a.y, a.y_bs) && (!a.res || al16(a.res, a.res_bs));
}
static bool in_bwd_v4_ok(const INBwdArgs& a) {   // (dx is NULL in the 16-bit form, which checks dxh itself)
  return (a.HW & 3) == 0 && al16(a.dy, a.dy_bs) && al16(a.x, a.x_bs) && (!a.dx || al16(a.dx, a.dx_bs)) &&
         (!a.res || al16(a.res, a.res_bs)) && (!a.dres || al16(a.dres, a.dres_bs));
}

// The rung of a plane size on the float4 (v4) or the scalar ladder; the scalar ladder has no
// 256 x 16 rung (its 256-thread form caches 16 scalars per thread).
enum InRung : int { IN_WAVE = 0, IN_256x4 = 1, IN_256x16 = 2, IN_1024 = 3, IN_STREAM = 4 };
static int in_rung(int HW, bool v4) {
  if (HW <= 64 * 16) return IN_WAVE;
  if (HW <= 256 * 16) return IN_256x4;
  if (v4) {
    if (HW <= 256 * 64) return IN_256x16;
    if (HW <= 1024 * 64) return IN_1024;
  } else if (HW <= 1024 * 16) {
    return IN_1024;
  }
  return IN_STREAM;
}

// What an entry point launches (dsgan_instnorm_plan returns it, the entry points switch on it):
// bits 0-1 the form (0 scalar, 1 v4, 2 split), bits 2-4 the rung of the one-workgroup forms, bit 5
// instnorm_fwd_v4's unguarded case, bits 8.. the chunks per plane S of the split forms.
enum InForm : int { IN_SCALAR = 0, IN_V4 = 1, IN_SPLIT = 2 };
static int in_plan(long planes, int HW, bool v4_ok, bool bwd, bool ws) {
  const int S = ws && v4_ok ? in_split_chunks(planes, HW) : 0;
  if (S) return IN_SPLIT | (S << 8);
  const int rung = in_rung(HW, v4_ok);
  if (!v4_ok) return IN_SCALAR | (rung << 2);
  const int nt = rung == IN_WAVE ? 64 : rung <= IN_256x16 ? 256 : 1024;
  const int c4 = rung <= IN_256x4 ? 4 : rung == IN_STREAM ? 0 : 16;   // (as in_fwd_v4_launch instantiates)
  const bool full = !bwd && in_fwd_v4_full(nt, c4, HW >> 2);
  return IN_V4 | (rung << 2) | (full ? 32 : 0);
}
static inline int in_plan_form(int plan) { return plan & 3; }
static inline int in_plan_rung(int plan) { return (plan >> 2) & 7; }

static void in_fwd_v4_launch(const INArgs& a, int rung, hipStream_t st) {
  const int planes = a.N * a.C;
  switch (rung) {
    case IN_WAVE: hipLaunchKernelGGL((instnorm_fwd_v4<64, 4>), dim3(cdiv(planes, 4)), dim3(256), 0, st, a); break;
    case IN_256x4: hipLaunchKernelGGL((instnorm_fwd_v4<256, 4>), dim3(planes), dim3(256), 0, st, a); break;
    case IN_256x16: hipLaunchKernelGGL((instnorm_fwd_v4<256, 16>), dim3(planes), dim3(256), 0, st, a); break;
    case IN_1024: hipLaunchKernelGGL((instnorm_fwd_v4<1024, 16>), dim3(planes), dim3(1024), 0, st, a); break;
    default: hipLaunchKernelGGL((instnorm_fwd_v4<1024, 0>), dim3(planes), dim3(1024), 0, st, a); break;
  }
}
static void in_fwd_scalar_launch(const INArgs& a, int rung, hipStream_t st) {
  const int planes = a.N * a.C;
  switch (rung) {
    case IN_WAVE: hipLaunchKernelGGL((instnorm_fwd_kernel<64, 16>), dim3(cdiv(planes, 4)), dim3(256), 0, st, a); break;
    case IN_256x4: hipLaunchKernelGGL((instnorm_fwd_kernel<256, 16>), dim3(planes), dim3(256), 0, st, a); break;
    case IN_1024: hipLaunchKernelGGL((instnorm_fwd_kernel<1024, 16>), dim3(planes), dim3(1024), 0, st, a); break;
    default: hipLaunchKernelGGL((instnorm_fwd_kernel<1024, 0>), dim3(planes), dim3(1024), 0, st, a); break;
  }
}
static void in_bwd_v4_launch(const INBwdArgs& a, int rung, hipStream_t st) {
  const int planes = a.N * a.C;
  switch (rung) {
    case IN_WAVE: in_bwd_launch<64, 4, true>(a, dim3(cdiv(planes, 4)), dim3(256), st); break;
    case IN_256x4: in_bwd_launch<256, 4, true>(a, dim3(planes), dim3(256), st); break;
    case IN_256x16: in_bwd_launch<256, 16, true>(a, dim3(planes), dim3(256), st); break;
    case IN_1024: in_bwd_launch<1024, 16, false, IN_BWD_XL>(a, dim3(planes), dim3(1024), st); break;
    default: hipLaunchKernelGGL((instnorm_bwd_v4<1024, 0, false>), dim3(planes), dim3(1024), 0, st, a); break;
  }
}
static void in_bwd_scalar_launch(const INBwdArgs& a, int rung, hipStream_t st) {
  const int planes = a.N * a.C;
  switch (rung) {
    case IN_WAVE: hipLaunchKernelGGL((instnorm_bwd_kernel<64, 16>), dim3(cdiv(planes, 4)), dim3(256), 0, st, a); break;
    case IN_256x4: hipLaunchKernelGGL((instnorm_bwd_kernel<256, 16>), dim3(planes), dim3(256), 0, st, a); break;
    case IN_1024: hipLaunchKernelGGL((instnorm_bwd_kernel<1024, 16>), dim3(planes), dim3(1024), 0, st, a); break;
    default: hipLaunchKernelGGL((instnorm_bwd_kernel<1024, 0>), dim3(planes), dim3(1024), 0, st, a); break;
  }
}

}  // namespace dsg

using namespace dsg;

extern "C" {

int dsgan_instnorm_fwd(const float* x, long x_bs, const float* scale, const float* res, long res_bs,
                       float* y, long y_bs, float* mean, float* rstd, int N, int C, int HW, int act,
                       float slope, float eps, hipStream_t st) {
  DSG_REQUIRE(x && y && mean && rstd && N > 0 && C > 0 && HW > 0, "dsgan_instnorm_fwd: bad args");
  INArgs a{x, x_bs, scale, res, res_bs, y, y_bs, mean, rstd, N, C, HW, act, slope, eps, 0};
  const int plan = in_plan((long)N * C, HW, in_fwd_v4_ok(a), false, false);
  if (in_plan_form(plan) == IN_V4) in_fwd_v4_launch(a, in_plan_rung(plan), st);
  else in_fwd_scalar_launch(a, in_plan_rung(plan), st);
  DSG_CHECK_LAUNCH();
  return 0;
}

// The launch form of the InstanceNorm entry points for a shape, on the host (no launch): aligned16 =
// every plane operand 16-byte aligned with a batch stride % 4 == 0, bwd = a backward entry point, ws =
// one of the _ws entry points.  Bits 0-1: 0 scalar kernels, 1 float4 kernels, 2 the split forms.
// Bits 2-4, the rung of the one-workgroup forms: 0 a wave per plane, 1 256 threads (4 float4s or 16
// scalars each), 2 256 threads x 16 float4s (float4 kernels only), 3 1024 threads cached, 4 1024
// threads streaming.  Bit 5: the forward float4 kernel's unguarded case (HW = 1024 or 4096).  Bits
// 8 and up: the chunks per plane of the split forms.  -1 for a shape the entry points refuse.
int dsgan_instnorm_plan(int N, int C, int HW, int aligned16, int bwd, int ws) {
  if (N <= 0 || C <= 0 || HW <= 0) return -1;
  return in_plan((long)N * C, HW, aligned16 && (HW & 3) == 0, bwd != 0, ws != 0);
}

// Scratch (fp32 elements) of dsgan_instnorm_{fwd,bwd}_ws for this shape: 0 when the one-workgroup-
// per-plane kernels serve it (>= 128 planes or planes under 16K pixels), else the per-chunk partials
// of the split forms.
long dsgan_instnorm_workspace(int N, int C, int HW) {
  const int S = in_split_chunks((long)N * C, HW);
  return S ? 2L * N * C * S : 0;
}

// dsgan_instnorm_fwd with scratch: few large planes are split over several workgroups each.
int dsgan_instnorm_fwd_ws(const float* x, long x_bs, const float* scale, const float* res, long res_bs,
                          float* y, long y_bs, float* mean, float* rstd, int N, int C, int HW, int act,
                          float slope, float eps, float* ws, long ws_elems, hipStream_t st) {
  DSG_REQUIRE(x && y && mean && rstd && N > 0 && C > 0 && HW > 0, "dsgan_instnorm_fwd_ws: bad args");
  INArgs a{x, x_bs, scale, res, res_bs, y, y_bs, mean, rstd, N, C, HW, act, slope, eps, 0};
  const long planes = (long)N * C;
  const int plan = in_plan(planes, HW, in_fwd_v4_ok(a), false, true);
  const int S = in_plan_form(plan) == IN_SPLIT ? plan >> 8 : 0;
  DSG_WS(S ? 2 * planes * S : 0, ws, ws_elems, "dsgan_instnorm_fwd_ws");
  if (!S) return dsgan_instnorm_fwd(x, x_bs, scale, res, res_bs, y, y_bs, mean, rstd, N, C, HW, act, slope, eps, st);
  const dim3 g(S, (unsigned)planes);
  hipLaunchKernelGGL(in_split_stat<0>, g, dim3(256), 0, st, a, ws, S);
  hipLaunchKernelGGL(in_split_stat<1>, g, dim3(256), 0, st, a, ws, S);
  hipLaunchKernelGGL(in_split_out, g, dim3(256), 0, st, a, ws, S);
  DSG_CHECK_LAUNCH();
  return 0;
}

// y (bf16) = IN(x): the plain InstanceNorm2d(affine=False) of a ConvNeXt block
// (DSGAN/models/model/MixConvNeXtML.py:233), stored bf16 for the block's MLP GEMMs.
int dsgan_instnorm_fwd_bf16(const float* x, long x_bs, void* y, long y_bs, float* mean, float* rstd, int N, int C,
                            int HW, float eps, hipStream_t st) {
  DSG_REQUIRE(x && y && mean && rstd && N > 0 && C > 0 && HW > 0, "dsgan_instnorm_fwd_bf16: bad args");
  // (y has the library's half type: y_bf16 = 1 bf16, 2 fp16)
  INArgs a{x, x_bs, nullptr, nullptr, 0, (float*)y, y_bs, mean, rstd, N, C, HW, ACT_NONE, 0.f, eps,
           half_type() == HALF_F16 ? 2 : 1};
  DSG_REQUIRE(in_fwd_v4_ok(a), "dsgan_instnorm_fwd_bf16: HW %% 4 and 16-byte alignment");
  in_fwd_v4_launch(a, in_plan_rung(in_plan((long)N * C, HW, true, false, false)), st);
  DSG_CHECK_LAUNCH();
  return 0;
}

// Backward with dx stored in the library's 16-bit half type (dxh, batch stride dxh_bs elements)
// plus the per-plane sums of the fp32 dx (dxsum [N*C]; nullable) -- the ConvTranspose backward's
// operand (its data-/weight-grad kernels read it as 16-bit MFMA operands) and its bias grad.
int dsgan_instnorm_bwd_h(const float* dy, long dy_bs, const float* x, long x_bs, const float* res, long res_bs,
                         const float* mean, const float* rstd, void* dxh, long dxh_bs, float* dxsum, float* dres,
                         long dres_bs, int N, int C, int HW, int act, float slope, float eps, hipStream_t st) {
  DSG_REQUIRE(dy && x && mean && rstd && dxh && N > 0 && C > 0 && HW > 0, "dsgan_instnorm_bwd_h: bad args");
  INBwdArgs a{dy, dy_bs, x, x_bs, nullptr, res, res_bs, mean, rstd, nullptr, dxh_bs, dres, dres_bs, nullptr,
              N, C, HW, act, slope, eps, dxh, dxsum, half_type()};
  DSG_REQUIRE(in_bwd_v4_ok(a) && ((uintptr_t)dxh & 7) == 0 && dxh_bs % 4 == 0,
              "dsgan_instnorm_bwd_h: planes must be float4-aligned (HW %% 4 == 0) and dxh 8-byte aligned");
  in_bwd_v4_launch(a, in_plan_rung(in_plan((long)N * C, HW, true, true, false)), st);
  DSG_CHECK_LAUNCH();
  return 0;
}

int dsgan_instnorm_bwd(const float* dy, long dy_bs, const float* x, long x_bs, const float* scale,
                       const float* res, long res_bs, const float* mean, const float* rstd,
                       float* dx, long dx_bs, float* dres, long dres_bs, float* dscale, int N,
                       int C, int HW, int act, float slope, float eps, hipStream_t st) {
  DSG_REQUIRE(dy && x && mean && rstd && dx && N > 0 && C > 0 && HW > 0, "dsgan_instnorm_bwd: bad args");
  INBwdArgs a{dy, dy_bs, x, x_bs, scale, res, res_bs, mean, rstd, dx, dx_bs, dres, dres_bs, dscale,
              N, C, HW, act, slope, eps};
  const int plan = in_plan((long)N * C, HW, in_bwd_v4_ok(a), true, false);
  if (in_plan_form(plan) == IN_V4) in_bwd_v4_launch(a, in_plan_rung(plan), st);
  else in_bwd_scalar_launch(a, in_plan_rung(plan), st);
  DSG_CHECK_LAUNCH();
  return 0;
}

// dsgan_instnorm_bwd with scratch (dsgan_instnorm_workspace): few large planes split as in the forward.
int dsgan_instnorm_bwd_ws(const float* dy, long dy_bs, const float* x, long x_bs, const float* scale,
                          const float* res, long res_bs, const float* mean, const float* rstd,
                          float* dx, long dx_bs, float* dres, long dres_bs, float* dscale, int N,
                          int C, int HW, int act, float slope, float eps, float* ws, long ws_elems, hipStream_t st) {
  DSG_REQUIRE(dy && x && mean && rstd && dx && N > 0 && C > 0 && HW > 0, "dsgan_instnorm_bwd_ws: bad args");
  INBwdArgs a{dy, dy_bs, x, x_bs, scale, res, res_bs, mean, rstd, dx, dx_bs, dres, dres_bs, dscale,
              N, C, HW, act, slope, eps};
  const long planes = (long)N * C;
  const int plan = in_plan(planes, HW, in_bwd_v4_ok(a), true, true);
  const int S = in_plan_form(plan) == IN_SPLIT ? plan >> 8 : 0;
  DSG_WS(S ? 2 * planes * S : 0, ws, ws_elems, "dsgan_instnorm_bwd_ws");
  if (!S)
    return dsgan_instnorm_bwd(dy, dy_bs, x, x_bs, scale, res, res_bs, mean, rstd, dx, dx_bs, dres, dres_bs, dscale,
                              N, C, HW, act, slope, eps, st);
  const dim3 g(S, (unsigned)planes);
  hipLaunchKernelGGL(in_split_bwd<0>, g, dim3(256), 0, st, a, ws, S);
  hipLaunchKernelGGL(in_split_bwd<1>, g, dim3(256), 0, st, a, ws, S);
  DSG_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
