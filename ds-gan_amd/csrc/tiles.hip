// Whole-frame colourisation (evaluate.py --full_frame, dsgan_hip/tiling.py): fp32, element-wise, no MFMA.
//   dsgan_u8_tiles     overlapping th x tw tiles of one uploaded uint8 HWC frame -> fp32 NCHW in [-1, 1]
//                      (u8_to_image_kernel's arithmetic, pointwise.hip, with no flip)
//   dsgan_tiles_blend  the generator's overlapping tiles -> one dense frame, every pixel the weighted mean
//                      of the tiles that cover it
// Tile t = iy * nx + ix has its corner at (oy[iy], ox[ix]); the origin arrays are ascending, every tile
// lies inside the frame (tiling.tile_origins).  Both kernels clamp an origin they read to [0, size - tile],
// so no content of those device arrays can take an access out of the frame or the tile batch.
// The blend gathers: an output pixel visits its tiles in a fixed order (iy, then ix, ascending) and no two
// threads write one address, so identical calls give identical bits.
#include "common.h"

namespace dsg {

constexpr int TL_MAXO = 1024;   // tiles per axis of one frame (the blend stages both origin arrays in LDS)

__device__ __forceinline__ int tl_clamp(int o, int size, int tile) { return min(max(o, 0), size - tile); }

__device__ __forceinline__ float tl_norm(unsigned p) {
#pragma clang fp contract(off)
  return ((float)p / 255.f - 0.5f) / 0.5f;
}
__device__ __forceinline__ float tl_gray(float r, float g, float b) {
#pragma clang fp contract(off)   // the reference's order, no FMA (u8_to_image_kernel)
  return (r * 0.299f + g * 0.587f) + b * 0.114f;
}

// ---- uint8 frame -> tiles ----------------------------------------------------------------------------
// blockIdx.y = tile of the range (its origins are wave-uniform: scalar loads, once per wave); a thread
// owns four consecutive x of one tile row.  Aligned, it reads its 12 bytes as three dwords and writes
// float4; otherwise (frame rows that are no multiple of 4 bytes apart, odd origins, a ragged last group)
// byte loads and scalar stores of the same values.
__global__ __launch_bounds__(256) void u8_tiles_kernel(const unsigned char* __restrict__ src, int H, int W,
                                                       const int* __restrict__ oy, const int* __restrict__ ox, int nx,
                                                       int th, int tw, int t0, int gray, float* __restrict__ dst) {
  const int t = t0 + blockIdx.y, iy = t / nx, ix = t - iy * nx;
  const int y0 = tl_clamp(oy[iy], H, th), x0 = tl_clamp(ox[ix], W, tw);
  const int tw4 = (tw + 3) >> 2, groups = th * tw4;
  const long plane = (long)th * tw;
  float* out = dst + (long)blockIdx.y * (gray ? 1 : 3) * plane;
  const bool st4 = (tw & 3) == 0 && (((uintptr_t)dst) & 15) == 0;
  for (int g = blockIdx.x * 256 + threadIdx.x; g < groups; g += gridDim.x * 256) {
    const int y = g / tw4, x = (g - y * tw4) * 4;
    const int n = min(4, tw - x);
    const unsigned char* px = src + ((long)(y0 + y) * W + (x0 + x)) * 3;
    unsigned b[12];
    if (n == 4 && (((uintptr_t)px) & 3) == 0) {
      const unsigned* p4 = reinterpret_cast<const unsigned*>(px);
      const unsigned d0 = p4[0], d1 = p4[1], d2 = p4[2];   // little endian: r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        b[k] = (d0 >> (8 * k)) & 255u; b[4 + k] = (d1 >> (8 * k)) & 255u; b[8 + k] = (d2 >> (8 * k)) & 255u;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 12; ++k) b[k] = k < 3 * n ? px[k] : 0u;
    }
    float c[3][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) c[ch][k] = tl_norm(b[3 * k + ch]);
    }
    float* o = out + (long)y * tw + x;
    if (gray) {
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = tl_gray(c[0][k], c[1][k], c[2][k]);
      if (st4) {
        *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) if (k < n) o[k] = v[k];
      }
    } else {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        if (st4) {
          *reinterpret_cast<float4*>(o + ch * plane) = make_float4(c[ch][0], c[ch][1], c[ch][2], c[ch][3]);
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) if (k < n) o[ch * plane + k] = c[ch][k];
        }
      }
    }
  }
}

// ---- tiles -> frame ----------------------------------------------------------------------------------
// The 1-D window over the tile offset i in [0, L): min(i + 1, L - i, overlap), 1 with overlap 0.  Integers,
// so the 2-D weight wy * wx <= 2^16 (tiles up to 512) and every sum of at most 9 of them is exact in fp32.
__device__ __forceinline__ int tl_w1(int i, int L, int overlap) {
  return overlap > 0 ? min(min(i + 1, L - i), overlap) : 1;
}
// tile [o, o + len) holds p.  The walks below test both ends, though ascending origins need only the first:
// whatever the arrays hold, an offset into a tile stays inside it.
__device__ __forceinline__ bool tl_covers(int o, int len, int p) { return o <= p && p < o + len; }
// the first i in [0, n) with o[i] + len > p (o ascending); n when there is none
__device__ __forceinline__ int tl_first(const int* o, int n, int len, int p) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (o[mid] + len > p) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// One output pixel, all C channels: num = sum fl(w * v), den = sum w over the covering tiles, iy then ix
// ascending, out = num / den; a pixel that exactly one tile covers takes that tile's value, copied
// ((w * v) / w is not v in fp32).  A pixel no tile covers (origin arrays that are not a plan's) gets 0.
__device__ __forceinline__ void tl_blend_px(const float* __restrict__ tiles, int C, int th, int tw, const int* soy,
                                            int ny, const int* sox, int nx, int overlap, int H, int W, int y, int x,
                                            float* __restrict__ out) {
#pragma clang fp contract(off)
  const long plane = (long)th * tw, HW = (long)H * W;
  const int iy0 = tl_first(soy, ny, th, y), ix0 = tl_first(sox, nx, tw, x);
  int iy1 = iy0, ix1 = ix0;
  while (iy1 < ny && tl_covers(soy[iy1], th, y)) ++iy1;
  while (ix1 < nx && tl_covers(sox[ix1], tw, x)) ++ix1;
  float* o = out + (long)y * W + x;
  const int cnt = (iy1 - iy0) * (ix1 - ix0);
  if (cnt == 0) {
    for (int c = 0; c < C; ++c) o[c * HW] = 0.f;
    return;
  }
  if (cnt == 1) {
    const float* v = tiles + ((long)(iy0 * nx + ix0) * C * th + (y - soy[iy0])) * tw + (x - sox[ix0]);
    for (int c = 0; c < C; ++c) o[c * HW] = v[c * plane];
    return;
  }
  float num[3] = {0.f, 0.f, 0.f}, den = 0.f;
  for (int iy = iy0; iy < iy1; ++iy) {
    const int i = y - soy[iy], wy = tl_w1(i, th, overlap);
    for (int ix = ix0; ix < ix1; ++ix) {
      const int j = x - sox[ix];
      const float w = (float)(wy * tl_w1(j, tw, overlap));
      const float* v = tiles + ((long)(iy * nx + ix) * C * th + i) * tw + j;
      den += w;
#pragma unroll
      for (int c = 0; c < 3; ++c) if (c < C) num[c] += w * v[c * plane];
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) if (c < C) o[c * HW] = num[c] / den;
}

// A thread owns four consecutive x of one frame row.  Vector form: when tw and every origin of a covering
// column are multiples of 4, the four pixels lie in the same tiles at 16-byte aligned offsets, so each
// tile row is one float4 load and the result one float4 store -- per pixel the same operations in the same
// order as tl_blend_px.  Anything else (odd origins or widths, a ragged last group) goes pixel by pixel.
__global__ __launch_bounds__(256) void tiles_blend_kernel(const float* __restrict__ tiles, int C, int th, int tw,
                                                          const int* __restrict__ oy, int ny,
                                                          const int* __restrict__ ox, int nx, int overlap, int H, int W,
                                                          int vec_ok, float* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ int soy[TL_MAXO], sox[TL_MAXO];
  for (int i = threadIdx.x; i < ny; i += 256) soy[i] = tl_clamp(oy[i], H, th);
  for (int i = threadIdx.x; i < nx; i += 256) sox[i] = tl_clamp(ox[i], W, tw);
  __syncthreads();
  const int W4 = (W + 3) >> 2;
  const long groups = (long)H * W4, plane = (long)th * tw, HW = (long)H * W;
  for (long g = blockIdx.x * 256L + threadIdx.x; g < groups; g += (long)gridDim.x * 256) {
    const int y = (int)(g / W4), x = (int)(g - (long)y * W4) * 4;
    const int ix0 = tl_first(sox, nx, tw, x);
    int ix1 = ix0;
    bool vec = vec_ok != 0 && ix0 < nx;
    while (ix1 < nx && tl_covers(sox[ix1], tw, x)) { vec = vec && (sox[ix1] & 3) == 0; ++ix1; }
    // (origins and tw multiples of 4: a tile that covers x covers x + 3, and one that starts after x starts
    // after x + 3 -- but only if it is itself aligned)
    if (vec && ix1 < nx && sox[ix1] < x + 4 && sox[ix1] + tw > x) vec = false;
    if (!vec || ix1 == ix0) {
      for (int k = 0; k < 4 && x + k < W; ++k) tl_blend_px(tiles, C, th, tw, soy, ny, sox, nx, overlap, H, W, y, x + k, out);
      continue;
    }
    const int iy0 = tl_first(soy, ny, th, y);
    int iy1 = iy0;
    while (iy1 < ny && tl_covers(soy[iy1], th, y)) ++iy1;
    float* o = out + (long)y * W + x;
    const int cnt = (iy1 - iy0) * (ix1 - ix0);
    if (cnt == 0) {
      for (int c = 0; c < C; ++c) *reinterpret_cast<float4*>(o + c * HW) = make_float4(0.f, 0.f, 0.f, 0.f);
      continue;
    }
    if (cnt == 1) {
      const float* v = tiles + ((long)(iy0 * nx + ix0) * C * th + (y - soy[iy0])) * tw + (x - sox[ix0]);
      for (int c = 0; c < C; ++c) *reinterpret_cast<float4*>(o + c * HW) = *reinterpret_cast<const float4*>(v + c * plane);
      continue;
    }
    float4 num[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) num[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 den = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int iy = iy0; iy < iy1; ++iy) {
      const int i = y - soy[iy], wy = tl_w1(i, th, overlap);
      for (int ix = ix0; ix < ix1; ++ix) {
        const int j = x - sox[ix];
        const float4 w = make_float4((float)(wy * tl_w1(j, tw, overlap)), (float)(wy * tl_w1(j + 1, tw, overlap)),
                                     (float)(wy * tl_w1(j + 2, tw, overlap)), (float)(wy * tl_w1(j + 3, tw, overlap)));
        const float* v = tiles + ((long)(iy * nx + ix) * C * th + i) * tw + j;
        den.x += w.x; den.y += w.y; den.z += w.z; den.w += w.w;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          if (c < C) {
            const float4 q = *reinterpret_cast<const float4*>(v + c * plane);
            num[c].x += w.x * q.x; num[c].y += w.y * q.y; num[c].z += w.z * q.z; num[c].w += w.w * q.w;
          }
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (c < C)
        *reinterpret_cast<float4*>(o + c * HW) = make_float4(num[c].x / den.x, num[c].y / den.y, num[c].z / den.z, num[c].w / den.w);
    }
  }
}

}  // namespace dsg

using namespace dsg;

extern "C" {

// dst fp32 [T][gray ? 1 : 3][th][tw] = tiles t0 .. t0 + T - 1 (t = iy * nx + ix, corner (oy[iy], ox[ix])) of the
// uint8 frame src [H][W][3]: ((p / 255) - 0.5) / 0.5 per channel, then the reference's gray sum when `gray`;
// bit-exact with dsgan_u8_to_image on host crops of the same windows.  oy (ny ints) and ox (nx ints) are
// device arrays.
int dsgan_u8_tiles(const unsigned char* src, int H, int W, const int* oy, int ny, const int* ox, int nx, int th, int tw,
                   int t0, int T, int gray, float* dst, hipStream_t st) {
  DSG_REQUIRE(src && oy && ox && dst && H > 0 && W > 0 && th > 0 && tw > 0 && th <= H && tw <= W && ny > 0 && nx > 0 &&
                  ny <= TL_MAXO && nx <= TL_MAXO && t0 >= 0 && T > 0 && T <= 65535 && (long)t0 + T <= (long)ny * nx,
              "dsgan_u8_tiles: bad args (frame %dx%d, tile %dx%d, %dx%d tiles, range [%d, %d+%d))", H, W, th, tw, ny, nx,
              t0, t0, T);
  const long groups = (long)th * ((tw + 3) / 4);
  long gx = (groups + 255) / 256;
  if (gx > 4096) gx = 4096;
  hipLaunchKernelGGL(u8_tiles_kernel, dim3((unsigned)gx, (unsigned)T), dim3(256), 0, st, src, H, W, oy, ox, nx, th, tw, t0,
                     gray ? 1 : 0, dst);
  DSG_CHECK_LAUNCH();
  return 0;
}

// out fp32 [C][H][W] from tiles fp32 [ny * nx][C][th][tw], C in {1, 3}, 0 <= overlap <= min(th, tw) / 2:
// per pixel and channel num = sum fl(w * v), den = sum w over the covering tiles (iy, then ix, ascending;
// w = w1(y - oy) * w1(x - ox), w1(i) = min(i + 1, L - i, overlap), 1 with overlap 0), out = num / den in
// fp32 without contraction; a pixel covered by one tile is that tile's value, copied.
int dsgan_tiles_blend(const float* tiles, int C, int th, int tw, const int* oy, int ny, const int* ox, int nx,
                      int overlap, int H, int W, float* out, hipStream_t st) {
  DSG_REQUIRE(tiles && oy && ox && out && (C == 1 || C == 3) && H > 0 && W > 0 && th > 0 && tw > 0 && th <= H &&
                  tw <= W && th <= 32768 && tw <= 32768 && ny > 0 && nx > 0 && ny <= TL_MAXO && nx <= TL_MAXO &&
                  overlap >= 0 && overlap <= th / 2 && overlap <= tw / 2,
              "dsgan_tiles_blend: bad args (C %d, frame %dx%d, tile %dx%d, %dx%d tiles, overlap %d)", C, H, W, th, tw, ny,
              nx, overlap);
  const int vec_ok = (W & 3) == 0 && (tw & 3) == 0 && al16(tiles) && al16(out);
  const long groups = (long)H * ((W + 3) / 4);
  hipLaunchKernelGGL(tiles_blend_kernel, dim3(ew_grid(groups)), dim3(256), 0, st, tiles, C, th, tw, oy, ny, ox, nx,
                     overlap, H, W, vec_ok, out);
  DSG_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
