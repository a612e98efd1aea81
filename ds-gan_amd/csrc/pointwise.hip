// The small elementwise / reduction kernels of the DS-GAN step: add_n, the copies, fill, scale, act_bwd,
// channel_sum and the uint8 input pipeline.
#include "common.h"

namespace dsg {

// ---------------------------------------------------------------------------------------
// Elementwise helpers
// ---------------------------------------------------------------------------------------
struct PtrList { const float* p[8]; long bs[8]; };

// out[n, e] = sum_i in_i[n, e]   (per-sample extent E, batch strides per operand)
__global__ void add_n_kernel(PtrList in, int nin, float* out, long out_bs, int N, long E) {
  const long total = (long)N * E;
  for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const int n = t / E; const long e = t - (long)n * E;
    float s = in.p[0][(long)n * in.bs[0] + e];
    for (int i = 1; i < nin; ++i) s += in.p[i][(long)n * in.bs[i] + e];
    out[(long)n * out_bs + e] = s;
  }
}

__global__ void copy_strided_kernel(const float* src, long src_bs, float* dst, long dst_bs, int N, long E) {
  const long total = (long)N * E;
  for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const int n = t / E; const long e = t - (long)n * E;
    dst[(long)n * dst_bs + e] = src[(long)n * src_bs + e];
  }
}

// float4 forms (E, batch strides multiples of 4, 16-byte aligned): blockIdx.y is the sample, so
// no 64-bit division per element (the scalar forms above spend more time in it than in memory).
__global__ __launch_bounds__(256) void add_n4_kernel(PtrList in, int nin, float* out, long out_bs, long E4) {
  const int n = blockIdx.y;
  float4* o = reinterpret_cast<float4*>(out + (long)n * out_bs);
  for (long e = blockIdx.x * 256L + threadIdx.x; e < E4; e += (long)gridDim.x * 256) {
    float4 s = reinterpret_cast<const float4*>(in.p[0] + (long)n * in.bs[0])[e];
    for (int i = 1; i < nin; ++i) {
      const float4 v = reinterpret_cast<const float4*>(in.p[i] + (long)n * in.bs[i])[e];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    o[e] = s;
  }
}

__global__ __launch_bounds__(256) void copy4_kernel(const float* src, long src_bs, float* dst, long dst_bs, long E4) {
  const int n = blockIdx.y;
  const float4* s = reinterpret_cast<const float4*>(src + (long)n * src_bs);
  float4* d = reinterpret_cast<float4*>(dst + (long)n * dst_bs);
  for (long e = blockIdx.x * 256L + threadIdx.x; e < E4; e += (long)gridDim.x * 256) d[e] = s[e];
}

// Up to COPY_MULTI (src, dst) pairs of E floats in one launch (blockIdx.y = pair): the ImagePool's
// per-query gather / scatter (util/image_pool.py) instead of one copy launch per image.
constexpr int COPY_MULTI = 32;
struct CopyPairs {
  const float* src[COPY_MULTI];
  float* dst[COPY_MULTI];
};
__global__ __launch_bounds__(256) void copy_multi4_kernel(CopyPairs pr, long E4) {
  const float4* s = reinterpret_cast<const float4*>(pr.src[blockIdx.y]);
  float4* d = reinterpret_cast<float4*>(pr.dst[blockIdx.y]);
  for (long e = blockIdx.x * 256L + threadIdx.x; e < E4; e += (long)gridDim.x * 256) d[e] = s[e];
}
__global__ __launch_bounds__(256) void copy_multi_kernel(CopyPairs pr, long E) {
  const float* s = pr.src[blockIdx.y];
  float* d = pr.dst[blockIdx.y];
  for (long e = blockIdx.x * 256L + threadIdx.x; e < E; e += (long)gridDim.x * 256) d[e] = s[e];
}

static inline dim3 grid4(int N, long E4) {
  long gx = (E4 + 255) / 256;
  if (gx > 4096) gx = 4096;
  return dim3((unsigned)(gx < 1 ? 1 : gx), (unsigned)N);
}

// Input pipeline (DSGAN/data/aligned_dataset.py:38-86): uint8 HWC crops -> ToTensor (/255) ->
// Normalize(0.5, 0.5) -> horizontal flip (per-sample flag) -> optional RGB->gray
// (0.299/0.587/0.114, evaluated in the reference's order without FMA contraction), NCHW fp32.
// One thread per output pixel, all channels; bit-exact with the torchvision/torch CPU ops.
__global__ void u8_to_image_kernel(const unsigned char* __restrict__ src, const int* __restrict__ flip,
                                   float* __restrict__ dst, int N, int H, int W, int gray) {
#pragma clang fp contract(off)   // hipcc contracts mul+add into FMA by default; torch CPU does not
  const long total = (long)N * H * W;
  for (long t = blockIdx.x * 256L + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const int n = (int)(t / ((long)H * W));
    const int r = (int)(t - (long)n * H * W), h = r / W, w = r - h * W;
    const int ws = flip[n] ? W - 1 - w : w;
    const unsigned char* px = src + (((long)n * H + h) * W + ws) * 3;
    float c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = ((float)px[k] / 255.f - 0.5f) / 0.5f;
    if (gray) {
      dst[(long)n * H * W + r] = (c[0] * 0.299f + c[1] * 0.587f) + c[2] * 0.114f;
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) dst[((long)n * 3 + k) * H * W + r] = c[k];
    }
  }
}

__global__ void scale_kernel(float* p, float a, long n) {
  for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < n; t += (long)gridDim.x * blockDim.x) p[t] *= a;
}

__global__ void fill_kernel(float* p, float v, long n) {
  for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < n; t += (long)gridDim.x * blockDim.x) p[t] = v;
}

// dx = dy * act'(pre)  (+ dx if accumulate)
__global__ void act_bwd_kernel(const float* dy, const float* pre, float* dx, long n, int act, float slope, int accumulate) {
  for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < n; t += (long)gridDim.x * blockDim.x) {
    float v = dy[t] * act_g(act, pre[t], slope);
    dx[t] = accumulate ? dx[t] + v : v;
  }
}

// part[n*C + c] = sum_p dy[n,c,p]   (bias gradient, one plane per NT threads; the sum over n is
// launch_split_reduce's fixed-order pass -- deterministic)
template <int NT>
__global__ __launch_bounds__(256) void channel_sum_kernel(const float* dy, long dy_bs, float* out, int N, int C, int HW) {
  __shared__ float sh[4];
  const int plane = blockIdx.x * (256 / NT) + (NT == 64 ? (threadIdx.x >> 6) : 0);
  const int t = NT == 64 ? (threadIdx.x & 63) : threadIdx.x;
  if (plane >= N * C) return;
  const int n = plane / C, c = plane - n * C;
  const float* p = dy + (long)n * dy_bs + (long)c * HW;
  float s = 0.f;
  if ((HW & 3) == 0 && (((uintptr_t)p) & 15) == 0) {
    const float4* p4 = reinterpret_cast<const float4*>(p);
    const int n4 = HW / 4;
    float s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int i = t;
    for (; i + 3 * NT < n4; i += 4 * NT) {   // four independent 16-byte loads in flight
      const float4 v0 = p4[i], v1 = p4[i + NT], v2 = p4[i + 2 * NT], v3 = p4[i + 3 * NT];
      s += (v0.x + v0.y) + (v0.z + v0.w);
      s1 += (v1.x + v1.y) + (v1.z + v1.w);
      s2 += (v2.x + v2.y) + (v2.z + v2.w);
      s3 += (v3.x + v3.y) + (v3.z + v3.w);
    }
    for (; i < n4; i += NT) { const float4 v = p4[i]; s += (v.x + v.y) + (v.z + v.w); }
    s = (s + s1) + (s2 + s3);
  } else {
    for (int i = t; i < HW; i += NT) s += p[i];
  }
  s = NT == 64 ? warp_sum(s) : block_sum<NT>(s, sh);
  if (t == 0) out[plane] = s;
}

}  // namespace dsg

using namespace dsg;

extern "C" {

int dsgan_add_n(const float* const* ins, const long* in_bs, int nin, float* out, long out_bs, int N,
                long E, hipStream_t st) {
  DSG_REQUIRE(nin >= 1 && nin <= 8 && ins && out, "dsgan_add_n: 1..8 inputs");
  PtrList pl{};
  bool v4 = (E & 3) == 0 && al16(out, out_bs) && N <= 65535;
  for (int i = 0; i < nin; ++i) { pl.p[i] = ins[i]; pl.bs[i] = in_bs[i]; v4 = v4 && al16(ins[i], in_bs[i]); }
  if (v4) {
    hipLaunchKernelGGL(add_n4_kernel, grid4(N, E / 4), dim3(256), 0, st, pl, nin, out, out_bs, E / 4);
    DSG_CHECK_LAUNCH();
    return 0;
  }
  hipLaunchKernelGGL(add_n_kernel, dim3(grid_for((long)N * E)), dim3(256), 0, st, pl, nin, out, out_bs, N, E);
  DSG_CHECK_LAUNCH();
  return 0;
}

int dsgan_copy_strided(const float* src, long src_bs, float* dst, long dst_bs, int N, long E,
                       hipStream_t st) {
  if ((E & 3) == 0 && al16(src, src_bs) && al16(dst, dst_bs) && N <= 65535) {
    hipLaunchKernelGGL(copy4_kernel, grid4(N, E / 4), dim3(256), 0, st, src, src_bs, dst, dst_bs, E / 4);
    DSG_CHECK_LAUNCH();
    return 0;
  }
  hipLaunchKernelGGL(copy_strided_kernel, dim3(grid_for((long)N * E)), dim3(256), 0, st, src, src_bs, dst, dst_bs, N, E);
  DSG_CHECK_LAUNCH();
  return 0;
}

// dst[i][0..E) <- src[i][0..E) for i < count (host arrays of device pointers); pairs must not
// overlap each other (the ImagePool orders its gather and scatter as two calls)
int dsgan_copy_multi(const float* const* src, float* const* dst, int count, long E, hipStream_t st) {
  DSG_REQUIRE(src && dst && count >= 0 && E >= 0, "dsgan_copy_multi: bad args");
  for (int b = 0; b < count; b += COPY_MULTI) {
    const int n = count - b < COPY_MULTI ? count - b : COPY_MULTI;
    CopyPairs pr{};
    bool v4 = (E & 3) == 0;
    for (int i = 0; i < n; ++i) {
      DSG_REQUIRE(src[b + i] && dst[b + i], "dsgan_copy_multi: null pointer in pair %d", b + i);
      pr.src[i] = src[b + i];
      pr.dst[i] = dst[b + i];
      v4 = v4 && al16(src[b + i], 0) && al16(dst[b + i], 0);
    }
    if (v4) hipLaunchKernelGGL(copy_multi4_kernel, grid4(n, E / 4), dim3(256), 0, st, pr, E / 4);
    else hipLaunchKernelGGL(copy_multi_kernel, grid4(n, E), dim3(256), 0, st, pr, E);
    DSG_CHECK_LAUNCH();
  }
  return 0;
}

int dsgan_u8_to_image(const unsigned char* src, const int* flip, float* dst, int N, int H, int W, int gray,
                      hipStream_t st) {
  DSG_REQUIRE(src && flip && dst && N > 0 && H > 0 && W > 0, "dsgan_u8_to_image: bad args");
  hipLaunchKernelGGL(u8_to_image_kernel, dim3(grid_for((long)N * H * W)), dim3(256), 0, st, src, flip, dst, N, H, W,
                     gray);
  DSG_CHECK_LAUNCH();
  return 0;
}

int dsgan_fill(float* p, float v, long n, hipStream_t st) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(fill_kernel, dim3(grid_for(n)), dim3(256), 0, st, p, v, n);
  DSG_CHECK_LAUNCH();
  return 0;
}

int dsgan_scale(float* p, float a, long n, hipStream_t st) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(scale_kernel, dim3(grid_for(n)), dim3(256), 0, st, p, a, n);
  DSG_CHECK_LAUNCH();
  return 0;
}

int dsgan_act_bwd(const float* dy, const float* pre, float* dx, long n, int act, float slope,
                  int accumulate, hipStream_t st) {
  hipLaunchKernelGGL(act_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, st, dy, pre, dx, n, act, slope, accumulate);
  DSG_CHECK_LAUNCH();
  return 0;
}

int dsgan_channel_sum(const float* dy, long dy_bs, float* out, int N, int C, int HW, float* ws, long ws_elems,
                      hipStream_t st) {
  DSG_REQUIRE(dy && out && N > 0 && C > 0 && HW > 0, "dsgan_channel_sum: bad args");
  DSG_WS((long)N * C, ws, ws_elems, "dsgan_channel_sum (N*C floats)");
  if (HW <= 8192)
    hipLaunchKernelGGL(channel_sum_kernel<64>, dim3(cdiv((long)N * C, 4)), dim3(256), 0, st, dy, dy_bs, ws, N, C, HW);
  else
    hipLaunchKernelGGL(channel_sum_kernel<256>, dim3(N * C), dim3(256), 0, st, dy, dy_bs, ws, N, C, HW);
  launch_split_reduce(ws, N, C, out, st);
  DSG_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
