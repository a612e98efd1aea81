// Test-set evaluation kernels (evaluate.py, util/metrics.py EvalMetrics): fp32 / integer / fp64, no MFMA.
//   dsgan_img_metrics_batch  skimage-style SSIM + PSNR of every image pair of a batch (DSGAN/train.py:27-44,
//                            110-124), the per-image definition of losses.hip's img_metrics_kernel
//   dsgan_images_to_u8       [input | result | label] uint8 HWC panels (DSGAN/train.py:110-128)
//   dsgan_ssim_eval          per-image gaussian SSIM (DSGAN/MS_SSIM.py:95-150, size_average=False,
//                            nonnegative_ssim) from losses.hip's ssim_eval_kernel tile partials
// Every reduction adds its partials in a fixed order (no atomics): identical calls give identical bits,
// and an image's values depend neither on its position in the batch nor on the batch size.
#include "common.h"

namespace dsg {

// the reference's uint8 conversion, kept as a float: trunc(clip(((t+1)/2)*255, 0, 255)).  fmaxf returns
// its non-NaN operand, so a NaN pixel becomes 0 (numpy's astype(uint8) of NaN is unspecified).
__device__ __forceinline__ float ev_u8f(float t) {
  const float v = ((t + 1.f) / 2.f) * 255.f;
  return truncf(fminf(fmaxf(v, 0.f), 255.f));
}

// ---- batched SSIM (uniform 7x7, sample covariance, data range 255) + PSNR ---------------------------
// Grid (32x32 tile of the cropped SSIM map, channel, image).  A workgroup stages the 38x38 halo of both
// planes in LDS as the quantised integers (each input pixel converted once), forms the five 7x7 box sums
// separably in int32 -- exact: 49 * 255^2 < 2^22 -- and evaluates S per output pixel in fp64 with
// img_metrics_kernel's expressions, so the per-pixel values are that kernel's.  The squared error is an
// integer sum over the input pixels the tile owns: rows / columns [0, 32) of its halo, and the rest of
// the halo too for the last tile of a direction (its halo reaches the plane's edge: Hc <= oh0 + 32 means
// H <= oh0 + 38), so every input pixel enters exactly once, the 3-pixel border and planes smaller than
// one tile included.  One (sum S, sum err^2) partial per tile; img_metrics_batch_final_kernel adds them.
constexpr int EM_T = 32, EM_K = 7, EM_E = EM_T + EM_K - 1;   // tile, window, halo (38)

__global__ __launch_bounds__(256) void img_metrics_batch_kernel(const float* __restrict__ fake,
                                                                const float* __restrict__ real, int H, int W,
                                                                int tiles_w, int tiles_h, double* __restrict__ part) {
  // pitches 39 and 33 (odd): the column walks of the two passes fall on distinct banks
  __shared__ int xs[EM_E][EM_E + 1], ys[EM_E][EM_E + 1];
  __shared__ int hb[5][EM_E][EM_T + 1];   // vertical 7-sums, [column][row]
  __shared__ double shd[4];
  __shared__ unsigned she[4];
  const int tile = blockIdx.x, tw = tile % tiles_w, th = tile / tiles_w;
  const int oh0 = th * EM_T, ow0 = tw * EM_T;
  const int Hc = H - (EM_K - 1), Wc = W - (EM_K - 1);
  const long plane = (long)blockIdx.z * gridDim.y + blockIdx.y;
  const float* rp = real + plane * H * W;
  const float* fp = fake + plane * H * W;
  const bool last_h = th == tiles_h - 1, last_w = tw == tiles_w - 1;
  unsigned se = 0;   // <= 38 * 38 * 255^2 < 2^27 per tile
  for (int i = threadIdx.x; i < EM_E * EM_E; i += 256) {
    const int r = i / EM_E, q = i - r * EM_E;
    const int h = oh0 + r, w = ow0 + q;
    int x = 0, y = 0;
    if (h < H && w < W) {
      x = (int)ev_u8f(rp[(long)h * W + w]);   // img1 = label, img2 = result
      y = (int)ev_u8f(fp[(long)h * W + w]);
      if ((r < EM_T || last_h) && (q < EM_T || last_w)) se += (unsigned)((x - y) * (x - y));
    }
    xs[r][q] = x; ys[r][q] = y;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < EM_T * EM_E; i += 256) {
    const int r = i / EM_E, q = i - r * EM_E;
    int sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
    for (int k = 0; k < EM_K; ++k) {
      const int x = xs[r + k][q], y = ys[r + k][q];
      sx += x; sy += y; sxx += x * x; syy += y * y; sxy += x * y;
    }
    hb[0][q][r] = sx; hb[1][q][r] = sy; hb[2][q][r] = sxx; hb[3][q][r] = syy; hb[4][q][r] = sxy;
  }
  __syncthreads();
  const double NP = 49.0, cov = NP / (NP - 1.0), C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
  double ssum = 0.0;
  for (int i = threadIdx.x; i < EM_T * EM_T; i += 256) {
    const int r = i >> 5, q = i & 31;
    if (oh0 + r >= Hc || ow0 + q >= Wc) continue;
    int v[5] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < EM_K; ++k) {
#pragma unroll
      for (int j = 0; j < 5; ++j) v[j] += hb[j][q + k][r];
    }
    const double sx = v[0], sy = v[1], sxx = v[2], syy = v[3], sxy = v[4];
    const double ux = sx / NP, uy = sy / NP;
    const double vx = cov * (sxx / NP - ux * ux), vy = cov * (syy / NP - uy * uy), vxy = cov * (sxy / NP - ux * uy);
    ssum += ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
  }
  ssum = warp_sum_d(ssum);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) se += __shfl_xor(se, o, 64);
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { shd[wv] = ssum; she[wv] = se; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* p = part + (plane * gridDim.x + tile) * 2;
    p[0] = (shd[0] + shd[1]) + (shd[2] + shd[3]);
    p[1] = (double)((she[0] + she[1]) + (she[2] + she[3]));
  }
}

// out[n] = (ssim, psnr) of image n from its cnt = C * tiles partials: lane l adds partials l, l + 64, ...
// in order, then the wave's butterfly -- an order fixed by cnt alone.  One wave per image.
__global__ __launch_bounds__(64) void img_metrics_batch_final_kernel(const double* __restrict__ part, int cnt, int C,
                                                                     int H, int W, float* __restrict__ out) {
  const int n = blockIdx.x;
  const double* p = part + (long)n * cnt * 2;
  double s = 0.0, e = 0.0;
  for (int i = threadIdx.x; i < cnt; i += 64) { s += p[2 * i]; e += p[2 * i + 1]; }
  s = warp_sum_d(s);
  e = warp_sum_d(e);   // integers below 2^53: exact in any order
  if (threadIdx.x != 0) return;
  const double ssim = s / ((double)C * (H - 6) * (W - 6));
  const double mse = e / ((double)C * H * W);
  const double psnr = mse / (255.0 * 255.0) < 1e-10 ? 100.0 : 10.0 * log10(255.0 * 255.0 / mse);
  out[2 * n] = (float)ssim;
  out[2 * n + 1] = (float)psnr;
}

// ---- uint8 panels ------------------------------------------------------------------------------------
// out[n][h][j * W + w][c] = u8(img_j[n][Cj == 1 ? 0 : c][h][w]) for the k images present, side by side
// (np.hstack, DSGAN/train.py:128); a one-channel image is repeated to three (DSGAN/util/util.py:16-17).
struct PanelArgs { const float* img[3]; int C[3]; int k; };

// one thread per output pixel (any W)
__global__ void images_to_u8_kernel(PanelArgs a, int N, int H, int W, unsigned char* __restrict__ out) {
  const long HW = (long)H * W, total = (long)N * a.k * HW;
  for (long t = blockIdx.x * 256L + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const int w = (int)(t % W);
    long u = t / W;
    const int j = (int)(u % a.k);
    u /= a.k;
    const int h = (int)(u % H), n = (int)(u / H);
    const int Cj = j == 0 ? a.C[0] : (j == 1 ? a.C[1] : a.C[2]);
    const float* src = (j == 0 ? a.img[0] : (j == 1 ? a.img[1] : a.img[2])) + (long)n * Cj * HW + (long)h * W + w;
    unsigned char* o = out + t * 3;   // t is the pixel's index in [N][H][k*W]
    const unsigned char c0 = (unsigned char)ev_u8f(src[0]);
    o[0] = c0;
    o[1] = Cj == 1 ? c0 : (unsigned char)ev_u8f(src[HW]);
    o[2] = Cj == 1 ? c0 : (unsigned char)ev_u8f(src[2 * HW]);
  }
}
// four pixels per thread (W % 4 == 0, 16-byte aligned planes): float4 loads, three dword stores
__global__ void images_to_u8_v4_kernel(PanelArgs a, int N, int H, int W, unsigned* __restrict__ out) {
  const int W4 = W / 4;
  const long HW = (long)H * W, total = (long)N * a.k * H * W4;
  for (long t = blockIdx.x * 256L + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const int w = (int)(t % W4) * 4;
    long u = t / W4;
    const int j = (int)(u % a.k);
    u /= a.k;
    const int h = (int)(u % H), n = (int)(u / H);
    const int Cj = j == 0 ? a.C[0] : (j == 1 ? a.C[1] : a.C[2]);
    const float* src = (j == 0 ? a.img[0] : (j == 1 ? a.img[1] : a.img[2])) + (long)n * Cj * HW + (long)h * W + w;
    const float4 c0 = *reinterpret_cast<const float4*>(src);
    const float4 c1 = Cj == 1 ? c0 : *reinterpret_cast<const float4*>(src + HW);
    const float4 c2 = Cj == 1 ? c0 : *reinterpret_cast<const float4*>(src + 2 * HW);
    const unsigned r0 = (unsigned)ev_u8f(c0.x), r1 = (unsigned)ev_u8f(c0.y), r2 = (unsigned)ev_u8f(c0.z), r3 = (unsigned)ev_u8f(c0.w);
    const unsigned g0 = (unsigned)ev_u8f(c1.x), g1 = (unsigned)ev_u8f(c1.y), g2 = (unsigned)ev_u8f(c1.z), g3 = (unsigned)ev_u8f(c1.w);
    const unsigned b0 = (unsigned)ev_u8f(c2.x), b1 = (unsigned)ev_u8f(c2.y), b2 = (unsigned)ev_u8f(c2.z), b3 = (unsigned)ev_u8f(c2.w);
    unsigned* o = out + t * 3;   // 12 bytes = the thread's four RGB pixels (little endian)
    o[0] = r0 | (g0 << 8) | (b0 << 16) | (r1 << 24);
    o[1] = g1 | (b1 << 8) | (r2 << 16) | (g2 << 24);
    o[2] = b2 | (r3 << 8) | (g3 << 16) | (b3 << 24);
  }
}

// ---- per-image gaussian SSIM from ssim_eval_kernel's tile partials -----------------------------------
// Per plane the tile sums of S in tile order, / (Ho * Wo), relu when `nonneg` (nonnegative_ssim,
// DSGAN/MS_SSIM.py:144-145); out[n] = the mean over the C planes of image n in channel order (one thread
// per image), out[N] = the mean of out[0..N) in image order.  One workgroup.
__global__ __launch_bounds__(256) void ssim_eval_combine_kernel(const float* __restrict__ tparts, int tiles, int N,
                                                                int C, float inv_cnt, int nonneg,
                                                                float* __restrict__ out) {
  for (int n = threadIdx.x; n < N; n += 256) {
    float acc = 0.f;
    for (int c = 0; c < C; ++c) {
      const float* q = tparts + ((long)n * C + c) * tiles * 2;
      float s = 0.f;
      for (int i = 0; i < tiles; ++i) s += q[2L * i];
      s *= inv_cnt;
      acc += nonneg ? fmaxf(s, 0.f) : s;
    }
    out[n] = acc / (float)C;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
    for (int n = 0; n < N; ++n) tot += out[n];
    out[N] = tot / (float)N;
  }
}

static inline long em_tiles(int H, int W) { return (long)cdiv(H - 6, EM_T) * cdiv(W - 6, EM_T); }

}  // namespace dsg

using namespace dsg;

extern "C" {

// doubles of `part` dsgan_img_metrics_batch needs: one (sum S, sum err^2) pair per (image, channel, tile)
long dsgan_img_metrics_batch_parts(int N, int C, int H, int W) {
  if (N <= 0 || C <= 0 || H <= 6 || W <= 6) return 0;
  return 2L * N * C * em_tiles(H, W);
}

// out[n] = {ssim, psnr} (float [N][2]) of the pairs (fake[n], real[n]), dense [N][C][H][W] in [-1, 1]:
// each value as one dsgan_img_metrics call defines it
int dsgan_img_metrics_batch(const float* fake, const float* real, int N, int C, int H, int W, double* part, float* out,
                            hipStream_t st) {
  DSG_REQUIRE(fake && real && part && out && N > 0 && C > 0 && H > 6 && W > 6 && N <= 65535 && C <= 65535,
              "dsgan_img_metrics_batch: bad args (H, W > 6)");
  const int tw = cdiv(W - 6, EM_T), th = cdiv(H - 6, EM_T);
  hipLaunchKernelGGL(img_metrics_batch_kernel, dim3(tw * th, C, N), dim3(256), 0, st, fake, real, H, W, tw, th, part);
  hipLaunchKernelGGL(img_metrics_batch_final_kernel, dim3(N), dim3(64), 0, st, part, C * tw * th, C, H, W, out);
  DSG_CHECK_LAUNCH();
  return 0;
}

// out uint8 [N][H][k*W][3]: the k non-NULL images of (a, b, c), each dense fp32 [N][Ci][H][W], Ci in {1, 3}
int dsgan_images_to_u8(const float* a, int Ca, const float* b, int Cb, const float* c, int Cc, int N, int H, int W,
                       unsigned char* out, hipStream_t st) {
  PanelArgs p{};
  const float* im[3] = {a, b, c};
  const int ch[3] = {Ca, Cb, Cc};
  bool v4 = W % 4 == 0 && (((uintptr_t)out) & 3) == 0;
  for (int i = 0; i < 3; ++i) {
    if (!im[i]) continue;
    DSG_REQUIRE(ch[i] == 1 || ch[i] == 3, "dsgan_images_to_u8: image %d has %d channels (1 or 3)", i, ch[i]);
    v4 = v4 && (((uintptr_t)im[i]) & 15) == 0;
    p.img[p.k] = im[i]; p.C[p.k] = ch[i]; ++p.k;
  }
  DSG_REQUIRE(out && p.k >= 1 && N > 0 && H > 0 && W > 0, "dsgan_images_to_u8: bad args");
  const long px = (long)N * p.k * H * W, work = v4 ? px / 4 : px;
  long g = (work + 255) / 256;
  if (g > 16384) g = 16384;
  if (v4)   // (H * W % 4 == 0 keeps every plane and row 16-byte aligned)
    hipLaunchKernelGGL(images_to_u8_v4_kernel, dim3((unsigned)g), dim3(256), 0, st, p, N, H, W, (unsigned*)out);
  else
    hipLaunchKernelGGL(images_to_u8_kernel, dim3((unsigned)g), dim3(256), 0, st, p, N, H, W, out);
  DSG_CHECK_LAUNCH();
  return 0;
}

// floats of `part` dsgan_ssim_eval needs: ssim_eval_kernel's (S, cs) pair per (plane, 32x32 output tile)
long dsgan_ssim_eval_parts(int N, int C, int H, int W) {
  if (N <= 0 || C <= 0 || H < 11 || W < 11) return 0;
  return 2L * N * C * cdiv(H - 10, 32) * cdiv(W - 10, 32);
}

// out[n] (n < N) = the SSIM of image n of (a*real+b, a*fake+b): the mean over its channels of the plane
// means of the 11-tap gaussian SSIM map, each relu'd first when nonneg; out[N] = the batch mean
int dsgan_ssim_eval(const float* real, const float* fake, float a, float b, int N, int C, int H, int W,
                    const float* win11, float C1, float C2, int nonneg, float* part, float* out, hipStream_t st) {
  DSG_REQUIRE(real && fake && win11 && part && out && N > 0 && C > 0 && H >= 11 && W >= 11 && (long)N * C <= 65535,
              "dsgan_ssim_eval: bad args (H, W >= 11)");
  const int tiles = launch_ssim_eval_tiles(real, fake, a, b, N * C, H, W, win11, C1, C2, part, st);
  hipLaunchKernelGGL(ssim_eval_combine_kernel, dim3(1), dim3(256), 0, st, part, tiles, N, C,
                     1.f / ((float)(H - 10) * (float)(W - 10)), nonneg, out);
  DSG_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
