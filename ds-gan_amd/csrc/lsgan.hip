// The LSGAN objective and the multi-scale discriminator's input pyramid (--no_lsgan, quirk q3;
// --which_model_netD multi):
//   sigmoid forward / backward (nn.Sigmoid, the last layer of a use_sigmoid D, DSGAN/models/networks.py:571-572),
//   MSE against a constant label (GANLoss / GANLoss_multi with nn.MSELoss, :148-149, :175-176),
//   AvgPool2d(3, stride=2, padding=1, count_include_pad=False) (MultiscaleDiscriminator.downsample, :675).
// fp32 in every precision mode; no atomics, no host synchronisation, no allocation.
#include "common.h"

namespace dsg {

// ---- sigmoid -------------------------------------------------------------------------------
// The accurate expf: this value is a loss input, not a gate.  expf(-x) overflows to +inf for
// x < -88.7 (y = 0) and underflows to 0 for x > 103 (y = 1): finite either way.
__global__ __launch_bounds__(256) void sigmoid_fwd_kernel(const float* __restrict__ x, long n, float* __restrict__ y) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) y[i] = 1.f / (1.f + expf(-x[i]));
}
__global__ __launch_bounds__(256) void sigmoid_bwd_kernel(const float* __restrict__ y, const float* __restrict__ dy,
                                                          long n, float* dx, int accumulate) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float s = y[i];
    const float v = dy[i] * s * (1.f - s);
    dx[i] = accumulate ? dx[i] + v : v;
  }
}

// ---- MSE against a constant label, mean over n ---------------------------------------------
__global__ __launch_bounds__(256) void mse_fwd_kernel(const float* __restrict__ x, long n, float t,
                                                      float* __restrict__ out) {
  __shared__ float sh[4];
  float s = 0.f;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float d = x[i] - t;
    s = fmaf(d, d, s);
  }
  s = block_sum<256>(s, sh);
  if (threadIdx.x == 0) out[blockIdx.x] = s;   // block partial (launch_final_sum adds them in order)
}
__global__ __launch_bounds__(256) void mse_bwd_kernel(const float* __restrict__ x, long n, float t,
                                                      const float* __restrict__ gout, float coef, float* dx,
                                                      int accumulate) {
  const float g = gout[0] * coef;   // coef = 2 / n
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float v = (x[i] - t) * g;
    dx[i] = accumulate ? dx[i] + v : v;
  }
}

// ---- AvgPool2d(3, 2, 1, count_include_pad=False) -------------------------------------------
// Output (ho, wo) averages the taps of rows 2ho-1..2ho+1 and columns 2wo-1..2wo+1 that lie inside
// the image.  Both forms feed the nine taps (0 where outside) to pool_out in the same order, so
// they agree bitwise.
__device__ __forceinline__ int taps_in(int o, int n) { return 1 + (o > 0 ? 1 : 0) + (2 * o + 1 < n ? 1 : 0); }

__device__ __forceinline__ float pool_out(float a0, float a1, float a2, float b0, float b1, float b2, float c0,
                                          float c1, float c2, int cnt) {
  const float ra = (a0 + a1) + a2, rb = (b0 + b1) + b2, rc = (c0 + c1) + c2;
  return ((ra + rb) + rc) / (float)cnt;
}

// Scalar form: one lane per output, guarded loads.  Any shape, stride and alignment.
__global__ __launch_bounds__(256) void avgpool3s2_fwd_kernel(const float* __restrict__ x, long x_bs,
                                                             float* __restrict__ y, long y_bs, int N, int C, int H,
                                                             int W, int Ho, int Wo) {
  const long per = (long)C * Ho * Wo, total = per * N;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int n = (int)(i / per);
    const long r = i - n * per;
    const int wo = (int)(r % Wo), ho = (int)((r / Wo) % Ho), c = (int)(r / ((long)Wo * Ho));
    const float* p = x + n * x_bs + (long)c * H * W;
    float t[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int h = 2 * ho - 1 + a;
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        const int w = 2 * wo - 1 + b;
        t[a][b] = (h >= 0 && h < H && w >= 0 && w < W) ? p[(long)h * W + w] : 0.f;
      }
    }
    y[n * y_bs + r] = pool_out(t[0][0], t[0][1], t[0][2], t[1][0], t[1][1], t[1][2], t[2][0], t[2][1], t[2][2],
                               taps_in(ho, H) * taps_in(wo, W));
  }
}

constexpr unsigned AP_OOB = 0xFFFFFFF0u;   // past every buffer range: the load returns 0

// Fast form (W % 8 == 0, 16-byte aligned rows on both sides, C*H*W*4 < 2^31): one lane produces 4
// adjacent outputs of a row from three input rows, each row read as two 16-byte loads (columns
// 2wo0 .. 2wo0+7) plus the halo column 2wo0-1.  Rows and the halo column outside the image take
// the out-of-range offset and read 0 through the buffer range check: branch-free, nine loads in
// flight per lane.  (W even: the right-hand tap 2wo+1 <= W-1 is always inside.)
__global__ __launch_bounds__(256) void avgpool3s2_fwd_v4_kernel(const float* __restrict__ x, long x_bs,
                                                                float* __restrict__ y, long y_bs, int N, int C, int H,
                                                                int W, int Ho, int Wo) {
  const int Wq = Wo >> 2;
  const long per = (long)C * Ho * Wq, total = per * N;
  const unsigned range = (unsigned)((long)C * H * W * 4);
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int n = (int)(i / per);
    const long r = i - n * per;
    const int q = (int)(r % Wq), ho = (int)((r / Wq) % Ho), c = (int)(r / ((long)Wq * Ho));
    const __amdgpu_buffer_rsrc_t rx = buf_rsrc(x + n * x_bs, range);
    const int wo0 = 4 * q;
    float4 lo[3], hi[3];
    float hl[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int h = 2 * ho - 1 + a;
      const bool in = h >= 0 && h < H;
      const unsigned off = (unsigned)((((long)c * H + h) * W + 2 * wo0) * 4);
      lo[a] = buf_ld4(rx, in ? off : AP_OOB);
      hi[a] = buf_ld4(rx, in ? off + 16u : AP_OOB);
      hl[a] = buf_ld(rx, in && wo0 > 0 ? off - 4u : AP_OOB);
    }
    const int rc = taps_in(ho, H);
    float4 o;
    o.x = pool_out(hl[0], lo[0].x, lo[0].y, hl[1], lo[1].x, lo[1].y, hl[2], lo[2].x, lo[2].y, rc * taps_in(wo0, W));
    o.y = pool_out(lo[0].y, lo[0].z, lo[0].w, lo[1].y, lo[1].z, lo[1].w, lo[2].y, lo[2].z, lo[2].w, rc * 3);
    o.z = pool_out(lo[0].w, hi[0].x, hi[0].y, lo[1].w, hi[1].x, hi[1].y, lo[2].w, hi[2].x, hi[2].y, rc * 3);
    o.w = pool_out(hi[0].y, hi[0].z, hi[0].w, hi[1].y, hi[1].z, hi[1].w, hi[2].y, hi[2].z, hi[2].w, rc * 3);
    *(float4*)(y + n * y_bs + ((long)c * Ho + ho) * Wo + wo0) = o;
  }
}

// Backward as a gather (no scatter, no atomics): input pixel (h, w) receives dy / taps from output
// row h/2 (h even) or rows (h-1)/2 and (h+1)/2 (h odd; the second only when < Ho), and the same for
// columns: at most four terms, added rows outer, columns inner.
__device__ __forceinline__ float pool_grad(const float* __restrict__ g, int h, int w, int H, int W, int Ho, int Wo) {
  const int oh0 = h >> 1, oh1 = (h & 1) && oh0 + 1 < Ho ? oh0 + 1 : -1;
  const int ow0 = w >> 1, ow1 = (w & 1) && ow0 + 1 < Wo ? ow0 + 1 : -1;
  const int rh0 = taps_in(oh0, H), cw0 = taps_in(ow0, W);
  float v = g[(long)oh0 * Wo + ow0] / (float)(rh0 * cw0);
  if (ow1 >= 0) v += g[(long)oh0 * Wo + ow1] / (float)(rh0 * taps_in(ow1, W));
  if (oh1 >= 0) {
    const int rh1 = taps_in(oh1, H);
    v += g[(long)oh1 * Wo + ow0] / (float)(rh1 * cw0);
    if (ow1 >= 0) v += g[(long)oh1 * Wo + ow1] / (float)(rh1 * taps_in(ow1, W));
  }
  return v;
}

__global__ __launch_bounds__(256) void avgpool3s2_bwd_kernel(const float* __restrict__ dy, long dy_bs, float* dx,
                                                             long dx_bs, int N, int C, int H, int W, int Ho, int Wo,
                                                             int accumulate) {
  const long per = (long)C * H * W, total = per * N;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int n = (int)(i / per);
    const long r = i - n * per;
    const int w = (int)(r % W), h = (int)((r / W) % H), c = (int)(r / ((long)W * H));
    const float v = pool_grad(dy + n * dy_bs + (long)c * Ho * Wo, h, w, H, W, Ho, Wo);
    float* d = dx + n * dx_bs + r;
    *d = accumulate ? *d + v : v;
  }
}
// Four adjacent input pixels per lane and one 16-byte store (W % 4 == 0, dx rows 16-byte aligned);
// the same pool_grad per pixel as the scalar form, so the same bits.
__global__ __launch_bounds__(256) void avgpool3s2_bwd_v4_kernel(const float* __restrict__ dy, long dy_bs, float* dx,
                                                                long dx_bs, int N, int C, int H, int W, int Ho,
                                                                int Wo, int accumulate) {
  const int Wq = W >> 2;
  const long per = (long)C * H * Wq, total = per * N;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int n = (int)(i / per);
    const long r = i - n * per;
    const int q = (int)(r % Wq), h = (int)((r / Wq) % H), c = (int)(r / ((long)Wq * H));
    const float* g = dy + n * dy_bs + (long)c * Ho * Wo;
    const int w0 = 4 * q;
    float4 v;
    v.x = pool_grad(g, h, w0, H, W, Ho, Wo);
    v.y = pool_grad(g, h, w0 + 1, H, W, Ho, Wo);
    v.z = pool_grad(g, h, w0 + 2, H, W, Ho, Wo);
    v.w = pool_grad(g, h, w0 + 3, H, W, Ho, Wo);
    float4* d = (float4*)(dx + n * dx_bs + ((long)c * H + h) * W + w0);
    if (accumulate) {
      const float4 o = *d;
      v.x = o.x + v.x; v.y = o.y + v.y; v.z = o.z + v.z; v.w = o.w + v.w;
    }
    *d = v;
  }
}

static bool ap_fwd_fast_ok(const float* x, long x_bs, const float* y, long y_bs, int C, int H, int W) {
  return W % 8 == 0 && x_bs % 4 == 0 && y_bs % 4 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0 &&
         (long)C * H * W * 4 < (1L << 31);
}
static bool ap_bwd_fast_ok(const float* dx, long dx_bs, int W) {
  return W % 4 == 0 && dx_bs % 4 == 0 && ((uintptr_t)dx & 15) == 0;
}
}  // namespace dsg

using namespace dsg;

extern "C" {

int dsgan_sigmoid_fwd(const float* x, long n, float* y, hipStream_t st) {
  DSG_REQUIRE(x && y && n > 0, "dsgan_sigmoid_fwd: bad args");
  hipLaunchKernelGGL(sigmoid_fwd_kernel, dim3(ew_grid(n)), dim3(256), 0, st, x, n, y);
  DSG_CHECK_LAUNCH();
  return 0;
}
int dsgan_sigmoid_bwd(const float* y, const float* dy, long n, float* dx, int accumulate, hipStream_t st) {
  DSG_REQUIRE(y && dy && dx && n > 0, "dsgan_sigmoid_bwd: bad args");
  hipLaunchKernelGGL(sigmoid_bwd_kernel, dim3(ew_grid(n)), dim3(256), 0, st, y, dy, n, dx, accumulate);
  DSG_CHECK_LAUNCH();
  return 0;
}

int dsgan_mse_const_fwd(const float* x, long n, float target, float* out, float* part, hipStream_t st) {
  DSG_REQUIRE(x && out && part && n > 0, "dsgan_mse_const_fwd: bad args");
  long g = (n + 2047) / 2048;   // <= dsgan_loss_parts() block partials
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(mse_fwd_kernel, dim3((unsigned)g), dim3(256), 0, st, x, n, target, part);
  launch_final_sum(part, (int)g, 1.f / (float)n, out, st);
  DSG_CHECK_LAUNCH();
  return 0;
}
int dsgan_mse_const_bwd(const float* x, long n, float target, const float* gout, float* dx, int accumulate,
                        hipStream_t st) {
  DSG_REQUIRE(x && gout && dx && n > 0, "dsgan_mse_const_bwd: bad args");
  hipLaunchKernelGGL(mse_bwd_kernel, dim3(ew_grid(n)), dim3(256), 0, st, x, n, target, gout, 2.f / (float)n, dx,
                     accumulate);
  DSG_CHECK_LAUNCH();
  return 0;
}

// form: 0 = the fast form where it applies, 1 = the scalar form, 2 = the fast form or an error
int dsgan_avgpool3s2_fast_supported(const float* x, long x_bs, const float* y, long y_bs, int C, int H, int W) {
  return ap_fwd_fast_ok(x, x_bs, y, y_bs, C, H, W) ? 1 : 0;
}
int dsgan_avgpool3s2_fwd(const float* x, long x_bs, float* y, long y_bs, int N, int C, int H, int W, int form,
                         hipStream_t st) {
  DSG_REQUIRE(x && y && N > 0 && C > 0 && H > 0 && W > 0 && form >= 0 && form <= 2, "dsgan_avgpool3s2_fwd: bad args");
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  DSG_REQUIRE(x_bs >= (long)C * H * W && y_bs >= (long)C * Ho * Wo, "dsgan_avgpool3s2_fwd: batch stride below C*H*W");
  const bool fast = ap_fwd_fast_ok(x, x_bs, y, y_bs, C, H, W);
  DSG_REQUIRE(form != 2 || fast, "dsgan_avgpool3s2_fwd: the fast form needs W %% 8 == 0 and 16-byte aligned rows");
  if (fast && form != 1) {
    hipLaunchKernelGGL(avgpool3s2_fwd_v4_kernel, dim3(ew_grid((long)N * C * Ho * (Wo / 4))), dim3(256), 0, st, x, x_bs,
                       y, y_bs, N, C, H, W, Ho, Wo);
  } else {
    hipLaunchKernelGGL(avgpool3s2_fwd_kernel, dim3(ew_grid((long)N * C * Ho * Wo)), dim3(256), 0, st, x, x_bs, y, y_bs,
                       N, C, H, W, Ho, Wo);
  }
  DSG_CHECK_LAUNCH();
  return 0;
}
// dx (+)= the input grad of the pool; H, W are the INPUT's size
int dsgan_avgpool3s2_bwd(const float* dy, long dy_bs, float* dx, long dx_bs, int N, int C, int H, int W, int accumulate,
                         int form, hipStream_t st) {
  DSG_REQUIRE(dy && dx && N > 0 && C > 0 && H > 0 && W > 0 && form >= 0 && form <= 2, "dsgan_avgpool3s2_bwd: bad args");
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  DSG_REQUIRE(dx_bs >= (long)C * H * W && dy_bs >= (long)C * Ho * Wo, "dsgan_avgpool3s2_bwd: batch stride below C*H*W");
  const bool fast = ap_bwd_fast_ok(dx, dx_bs, W);
  DSG_REQUIRE(form != 2 || fast, "dsgan_avgpool3s2_bwd: the fast form needs W %% 4 == 0 and 16-byte aligned rows");
  if (fast && form != 1) {
    hipLaunchKernelGGL(avgpool3s2_bwd_v4_kernel, dim3(ew_grid((long)N * C * H * (W / 4))), dim3(256), 0, st, dy, dy_bs,
                       dx, dx_bs, N, C, H, W, Ho, Wo, accumulate);
  } else {
    hipLaunchKernelGGL(avgpool3s2_bwd_kernel, dim3(ew_grid((long)N * C * H * W)), dim3(256), 0, st, dy, dy_bs, dx, dx_bs,
                       N, C, H, W, Ho, Wo, accumulate);
  }
  DSG_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
