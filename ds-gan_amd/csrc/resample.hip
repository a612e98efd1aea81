// Load-time resize (--load_resize, dsgan_hip/resample.py): integers up to the last step, no MFMA.
//   dsgan_u8_resize_crop_to_image   uint8 HWC frames -> Pillow's 8-bit resize to load_h x load_w -> crop of
//                                   fh x fw at per-sample offsets -> flip / normalise / gray -> fp32 NCHW
// Pillow's resampler (Resample.c) per axis: output index i has a window (xmin, n) and n 22-bit fixed-point
// coefficients (resample.pil_coeffs builds the tables on the host, in double, as Pillow does); a pass is
// clip8((2^21 + sum p * k) >> 22) in int32.  The horizontal pass runs first into a uint8 intermediate, the
// vertical pass second; a pass whose axis keeps its size is skipped (k == 0).
//   rs_hpass_kernel   src rows -> tmp uint8 [N][Hs][fw][3]: only the fw columns of the sample's crop window,
//                     and only the source rows the vertical pass of that sample's crop will read
//   rs_vpass_kernel   tmp (or, with the horizontal axis unchanged, src itself at the crop's column offset)
//                     -> the fh crop rows, then u8_to_image_kernel's arithmetic (pointwise.hip) -> dst
// With both axes unchanged the call is rs_vpass_kernel alone on src: crop + convert, dsgan_u8_to_image's bits.
// Both kernels clamp what they read from device arrays -- an offset to [0, load - fine], a window to
// xmin in [0, in - 1], n in [0, min(k, in - xmin)] -- so no content of those arrays can take an access out of
// a frame, a table or tmp.  (Tables that are not pil_coeffs' can make the vertical pass read tmp rows the
// horizontal pass skipped: stale bytes of tmp, never out of it.)
// One wave owns one row (sample and row are wave-uniform: the vertical pass's table reads are scalar loads),
// a thread four consecutive x of it.  12 bytes go as three dwords when aligned, as bytes otherwise (frame
// rows are Ws * 3 bytes apart, often no multiple of 4); fp32 output as float4 when fw % 4 == 0.
#include "common.h"

namespace dsg {

constexpr int RS_BITS = 22;          // Pillow's PRECISION_BITS = 32 - 8 - 2
constexpr int RS_MAXK = 65;          // ceil(2 * 16) * 2 + 1: bicubic at the 16x down-scaling cap
constexpr int RS_MAXDIM = 32768;

__device__ __forceinline__ int rs_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }
__device__ __forceinline__ unsigned rs_clip8(int acc) { return (unsigned)rs_clamp(acc >> RS_BITS, 0, 255); }

__device__ __forceinline__ float rs_norm(unsigned p) {
#pragma clang fp contract(off)
  return ((float)p / 255.f - 0.5f) / 0.5f;
}
__device__ __forceinline__ float rs_gray(float r, float g, float b) {
#pragma clang fp contract(off)   // the reference's order, no FMA (u8_to_image_kernel)
  return (r * 0.299f + g * 0.587f) + b * 0.114f;
}

// 12 bytes at p (cnt * 3 of them valid) -> b[12]
__device__ __forceinline__ void rs_load12(const unsigned char* __restrict__ p, int cnt, unsigned (&b)[12]) {
  if (cnt == 4 && (((uintptr_t)p) & 3) == 0) {
    const unsigned* p4 = reinterpret_cast<const unsigned*>(p);
    const unsigned d0 = p4[0], d1 = p4[1], d2 = p4[2];   // little endian: r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      b[k] = (d0 >> (8 * k)) & 255u; b[4 + k] = (d1 >> (8 * k)) & 255u; b[8 + k] = (d2 >> (8 * k)) & 255u;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k) b[k] = k < 3 * cnt ? p[k] : 0u;
  }
}

// the window of table row i over an axis of `in` samples, clamped: lo in [0, in - 1], n in [0, min(k, in - lo)]
__device__ __forceinline__ void rs_window(const int* __restrict__ bounds, int i, int k, int in, int& lo, int& n) {
  lo = rs_clamp(bounds[2 * i], 0, in - 1);
  n = rs_clamp(bounds[2 * i + 1], 0, min(k, in - lo));
}

// ---- horizontal pass ---------------------------------------------------------------------------------
// grid (x groups of 64 threads, source rows / 4, N); wave w of a block owns source row blockIdx.y * 4 + w.
__global__ __launch_bounds__(256) void rs_hpass_kernel(const unsigned char* __restrict__ src, int Hs, int Ws,
                                                       const int* __restrict__ ybounds, int ky,
                                                       const int* __restrict__ xbounds, const int* __restrict__ xcoef,
                                                       int kx, int load_h, int load_w, const int* __restrict__ off,
                                                       int fh, int fw, unsigned char* __restrict__ tmp) {
  const int n = blockIdx.z;
  const int r = blockIdx.y * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (r >= Hs) return;
  const int h_off = rs_clamp(off[2 * n], 0, load_h - fh), w_off = rs_clamp(off[2 * n + 1], 0, load_w - fw);
  // the source rows the crop's vertical pass reads (windows ascend with the output row)
  int rlo = h_off, rhi = h_off + fh;
  if (ky > 0) {
    int lo, cnt;
    rs_window(ybounds, h_off, ky, Hs, rlo, cnt);
    rs_window(ybounds, h_off + fh - 1, ky, Hs, lo, cnt);
    rhi = lo + cnt;
  }
  if (r < rlo || r >= rhi) return;
  const int x = (blockIdx.x * 64 + (int)(threadIdx.x & 63)) * 4;
  if (x >= fw) return;
  const int cnt = min(4, fw - x);
  const unsigned char* __restrict__ row = src + ((long)n * Hs + r) * Ws * 3;
  unsigned b[12];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int a0 = 1 << (RS_BITS - 1), a1 = a0, a2 = a0;
    if (i < cnt) {
      const int ox = w_off + x + i;
      int lo, nt;
      rs_window(xbounds, ox, kx, Ws, lo, nt);
      const int* __restrict__ k = xcoef + (long)ox * kx;
      const unsigned char* __restrict__ p = row + (long)lo * 3;
      for (int j = 0; j < nt; ++j) {
        const int c = k[j];
        a0 += (int)p[3 * j] * c; a1 += (int)p[3 * j + 1] * c; a2 += (int)p[3 * j + 2] * c;
      }
    }
    b[3 * i] = rs_clip8(a0); b[3 * i + 1] = rs_clip8(a1); b[3 * i + 2] = rs_clip8(a2);
  }
  unsigned char* o = tmp + (((long)n * Hs + r) * fw + x) * 3;
  if (cnt == 4 && (((uintptr_t)o) & 3) == 0) {
    unsigned* o4 = reinterpret_cast<unsigned*>(o);
#pragma unroll
    for (int d = 0; d < 3; ++d) o4[d] = b[4 * d] | (b[4 * d + 1] << 8) | (b[4 * d + 2] << 16) | (b[4 * d + 3] << 24);
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k) if (k < 3 * cnt) o[k] = (unsigned char)b[k];
  }
}

// ---- vertical pass, crop, flip, normalise, gray ------------------------------------------------------
// rows: uint8 rows of `pitch` bytes, Hs of them per sample (`sample` bytes apart).  direct: rows is src, the
// crop's columns start at w_off; otherwise rows is tmp, which holds the crop's columns only.
// grid (x groups of 64 threads, fh / 4, N); wave w of a block owns output row blockIdx.y * 4 + w.
__global__ __launch_bounds__(256) void rs_vpass_kernel(const unsigned char* __restrict__ rows, long sample, long pitch,
                                                       int Hs, int direct, const int* __restrict__ ybounds,
                                                       const int* __restrict__ ycoef, int ky, int load_h, int load_w,
                                                       const int* __restrict__ off, const int* __restrict__ flip,
                                                       int fh, int fw, int gray, float* __restrict__ dst) {
  const int n = blockIdx.z;
  const int y = blockIdx.y * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (y >= fh) return;
  const int h_off = rs_clamp(off[2 * n], 0, load_h - fh), w_off = rs_clamp(off[2 * n + 1], 0, load_w - fw);
  const bool fl = flip[n] != 0;
  const int x = (blockIdx.x * 64 + (int)(threadIdx.x & 63)) * 4;
  if (x >= fw) return;
  const int cnt = min(4, fw - x);
  const int xs = fl ? fw - x - cnt : x;   // the cnt source columns of output columns x .. x + cnt - 1, reversed by a flip
  const unsigned char* __restrict__ col = rows + (long)n * sample + ((long)(direct ? w_off : 0) + xs) * 3;
  unsigned b[12];
  if (ky > 0) {
    int lo, nt;
    rs_window(ybounds, h_off + y, ky, Hs, lo, nt);
    const int* __restrict__ k = ycoef + (long)(h_off + y) * ky;
    int acc[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) acc[i] = 1 << (RS_BITS - 1);
    for (int j = 0; j < nt; ++j) {
      const int c = k[j];
      unsigned q[12];
      rs_load12(col + (long)(lo + j) * pitch, cnt, q);
#pragma unroll
      for (int i = 0; i < 12; ++i) acc[i] += (int)q[i] * c;
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) b[i] = rs_clip8(acc[i]);
  } else {
    rs_load12(col + (long)(h_off + y) * pitch, cnt, b);   // h_off + y < load_h == Hs
  }
  float c[3][4];   // c[ch][i]: source pixel i
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) c[ch][i] = rs_norm(b[3 * i + ch]);
  }
  const long plane = (long)fh * fw;
  float* o = dst + (long)n * (gray ? 1 : 3) * plane + (long)y * fw + x;
  const bool st4 = (fw & 3) == 0 && (((uintptr_t)dst) & 15) == 0;   // then cnt == 4 for every thread
  if (gray) {
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = rs_gray(c[0][i], c[1][i], c[2][i]);
    if (st4) {
      *reinterpret_cast<float4*>(o) = fl ? make_float4(v[3], v[2], v[1], v[0]) : make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) if (i < cnt) o[fl ? cnt - 1 - i : i] = v[i];
    }
  } else {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      if (st4) {
        *reinterpret_cast<float4*>(o + ch * plane) = fl ? make_float4(c[ch][3], c[ch][2], c[ch][1], c[ch][0])
                                                        : make_float4(c[ch][0], c[ch][1], c[ch][2], c[ch][3]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) if (i < cnt) o[ch * plane + (fl ? cnt - 1 - i : i)] = c[ch][i];
      }
    }
  }
}

}  // namespace dsg

using namespace dsg;

extern "C" {

// dst fp32 [N][gray ? 1 : 3][fh][fw] from src uint8 [N][Hs][Ws][3]: every frame resized to load_h x load_w by
// Pillow's 8-bit resampler (tables of resample.pil_coeffs on the device: bounds [load][2], coef [load][k];
// k == 0: that axis keeps its size, no pass), cropped at off[n] = (h_off, w_off), then ((p / 255) - 0.5) / 0.5,
// flipped where flip[n], the reference's gray sum when `gray`.  tmp: N * Hs * fw * 3 bytes when kx > 0.
int dsgan_u8_resize_crop_to_image(const unsigned char* src, int N, int Hs, int Ws, const int* ybounds, const int* ycoef,
                                  int ky, const int* xbounds, const int* xcoef, int kx, int load_h, int load_w,
                                  const int* off, const int* flip, int fh, int fw, int gray, unsigned char* tmp,
                                  long tmp_bytes, float* dst, hipStream_t st) {
  DSG_REQUIRE(src && off && flip && dst, "dsgan_u8_resize_crop_to_image: null src, off, flip or dst");
  DSG_REQUIRE(N > 0 && N <= 65535 && Hs > 0 && Ws > 0 && Hs <= RS_MAXDIM && Ws <= RS_MAXDIM && load_h > 0 &&
                  load_w > 0 && load_h <= RS_MAXDIM && load_w <= RS_MAXDIM && fh > 0 && fw > 0,
              "dsgan_u8_resize_crop_to_image: bad sizes (N %d, source %dx%d, load %dx%d, crop %dx%d)", N, Hs, Ws, load_h,
              load_w, fh, fw);
  DSG_REQUIRE(fh <= load_h && fw <= load_w, "dsgan_u8_resize_crop_to_image: crop %dx%d larger than the load size %dx%d",
              fh, fw, load_h, load_w);
  DSG_REQUIRE(ky >= 0 && ky <= RS_MAXK && kx >= 0 && kx <= RS_MAXK && (ky > 0 ? ybounds && ycoef : Hs == load_h) &&
                  (kx > 0 ? xbounds && xcoef : Ws == load_w),
              "dsgan_u8_resize_crop_to_image: bad tables (ky %d, kx %d of at most %d; source %dx%d, load %dx%d; an axis "
              "without a table must keep its size)", ky, kx, RS_MAXK, Hs, Ws, load_h, load_w);
  const long need = kx > 0 ? (long)N * Hs * fw * 3 : 0;
  DSG_REQUIRE(need == 0 || (tmp && tmp_bytes >= need),
              "dsgan_u8_resize_crop_to_image: tmp of %ld bytes, this call needs %ld", tmp ? tmp_bytes : 0L, need);
  const unsigned gx = cdiv((fw + 3) / 4, 64);
  if (kx > 0) {
    hipLaunchKernelGGL(rs_hpass_kernel, dim3(gx, cdiv(Hs, 4), (unsigned)N), dim3(256), 0, st, src, Hs, Ws, ybounds, ky,
                       xbounds, xcoef, kx, load_h, load_w, off, fh, fw, tmp);
    DSG_CHECK_LAUNCH();
  }
  const unsigned char* rows = kx > 0 ? tmp : src;
  const long pitch = kx > 0 ? (long)fw * 3 : (long)Ws * 3;
  hipLaunchKernelGGL(rs_vpass_kernel, dim3(gx, cdiv(fh, 4), (unsigned)N), dim3(256), 0, st, rows, pitch * Hs, pitch, Hs,
                     kx > 0 ? 0 : 1, ybounds, ycoef, ky, load_h, load_w, off, flip, fh, fw, gray ? 1 : 0, dst);
  DSG_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
