// Differentiable augmentation of the discriminator's input (--diffaug; Zhao et al., NeurIPS 2020):
//   y = cutout(translation(color(cat(a, b)))) with per-sample parameters drawn from Philox-4x32-10,
//   riding on the pass that forms the channel concatenation; dx = the transpose, for the image half.
// Sample i of call k draws  w = Philox(key = seed, counter = (i, 0, k, stream)),
//                           v = Philox(key = seed, counter = (i, 1, k, stream)):
//   color        b = u24(w0) - 1/2, s = 2 u24(w1), c = u24(w2) + 1/2        (u24(x) = (x >> 8) 2^-24)
//                on the Cb image channels: u = x + b; u' = (u - mean_c u) s + mean_c u;
//                u'' = (u' - M) c + M, M = the sample's mean of u' = mean(x_B) + b
//   translation  tx = mulhi(w3, 2 Sx + 1) - Sx, ty = mulhi(v0, 2 Sy + 1) - Sy, S = floor(size / 8 + 1/2):
//                y[r, q] = x[r - ty, q - tx], 0 outside; one shift for all channels
//   cutout       ch = floor(H / 2 + 1/2), oy = mulhi(v1, H + 1 - ch % 2): rows [oy - ch / 2, oy - ch / 2 + ch)
//                (clipped) x the like columns are 0
// The call counter lives in device memory and is advanced by the forward (replayable from a captured
// graph, as the dropout's); sample n of a launch belongs to call used + n / group with index n % group,
// so one stacked launch draws what several smaller ones draw.  fp32; no atomics: the two per-sample
// means go through block partials in a fixed order and block_sum's fixed tree.
#include "common.h"
#include "philox.h"

namespace dsg {

typedef float f32x4 __attribute__((ext_vector_type(4)));

enum : int { AUG_COLOR = 1, AUG_TRANSLATION = 2, AUG_CUTOUT = 4 };

__device__ __forceinline__ float u24(unsigned x) { return (float)(x >> 8) * 0x1p-24f; }
__device__ __forceinline__ int mulhi(unsigned x, int m) {
  return (int)(((unsigned long long)x * (unsigned long long)(unsigned)m) >> 32);
}

struct Aug {
  float b, s, c;
  int tx, ty, oy, ox;
};

// the draw of sample `i` of call `call` (every word is drawn whatever the policy is)
__device__ __forceinline__ Aug aug_draw(unsigned k0, unsigned k1, unsigned sid, long call, unsigned i, int H, int W) {
  unsigned w[4], v[4];
  philox4x32_10(i, 0u, (unsigned)call, sid, k0, k1, w);
  philox4x32_10(i, 1u, (unsigned)call, sid, k0, k1, v);
  Aug p;
  p.b = u24(w[0]) - 0.5f;
  p.s = 2.f * u24(w[1]);
  p.c = u24(w[2]) + 0.5f;
  const int Sx = (W + 4) >> 3, Sy = (H + 4) >> 3, ch = (H + 1) >> 1, cw = (W + 1) >> 1;
  p.tx = mulhi(w[3], 2 * Sx + 1) - Sx;
  p.ty = mulhi(v[0], 2 * Sy + 1) - Sy;
  p.oy = mulhi(v[1], H + 1 - (ch & 1));
  p.ox = mulhi(v[2], W + 1 - (cw & 1));
  return p;
}

// What a launch needs of a sample's draw: the policy's ops only, the others as the identity.
struct AugGeom {
  float b, s, c;
  int tx, ty, y0, y1, x0, x1;   // the cutout box [y0, y1) x [x0, x1) (empty when off)
};
__device__ __forceinline__ AugGeom aug_geom(const Aug& p, int policy, int H, int W) {
  AugGeom g;
  g.b = p.b; g.s = p.s; g.c = p.c;
  const bool tr = policy & AUG_TRANSLATION, cut = policy & AUG_CUTOUT;
  g.tx = tr ? p.tx : 0;
  g.ty = tr ? p.ty : 0;
  const int ch = (H + 1) >> 1, cw = (W + 1) >> 1;
  g.y0 = cut ? p.oy - (ch >> 1) : 0;
  g.y1 = cut ? g.y0 + ch : 0;
  g.x0 = cut ? p.ox - (cw >> 1) : 0;
  g.x1 = cut ? g.x0 + cw : 0;
  return g;
}

// the partials of one sample: at most 256, so the consumer sums them with one block_sum
static inline unsigned sum_blocks(long E) {
  long g = (E + 4095) / 4096;
  if (g > 256) g = 256;
  if (g < 1) g = 1;
  return (unsigned)g;
}
// sum of a sample's partials: lane t holds part[t], combined by block_sum's fixed tree (all 256 lanes call)
__device__ __forceinline__ float parts_sum(const float* __restrict__ part, int np, float* sh) {
  const float s = (int)threadIdx.x < np ? part[threadIdx.x] : 0.f;
  return block_sum<256>(s, sh);
}

// used[0] <- counter[0], counter[0] += adv (block (0, 0) of the launch that carries it)
__device__ __forceinline__ void aug_advance(long* counter, long* used, long adv) {
  if (counter && threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0) {
    const long c = counter[0];
    used[0] = c;
    counter[0] = c + adv;
  }
}
__global__ void diffaug_advance_kernel(long* counter, long* used, long adv) { aug_advance(counter, used, adv); }

// 16-byte store followed by its wait states (pw_impl.h pw_st128: the data registers stay allocated
// for two wave states after the store)
__device__ __forceinline__ void st128(float* p, f32x4 v) {
  *(f32x4*)p = v;
  asm volatile("s_nop 1" ::"v"(v));
}

template <int V> __device__ __forceinline__ void st_unit(float* p, const float (&v)[V]);
template <> __device__ __forceinline__ void st_unit<1>(float* p, const float (&v)[1]) { p[0] = v[0]; }
template <> __device__ __forceinline__ void st_unit<4>(float* p, const float (&v)[4]) {
  st128(p, f32x4{v[0], v[1], v[2], v[3]});
}

// V source pixels of one row at columns qs .. qs + V - 1, lane j read only where bit j of `m` is set
// (0 elsewhere).  `vec`: the unit is 16-byte aligned and wholly wanted -> one 16-byte load; a shift
// that is no multiple of 4 misaligns the rows, and those units take dword loads.
template <int V>
__device__ __forceinline__ void ld_unit(const float* __restrict__ row, int qs, unsigned m, bool vec, float (&v)[V]) {
  if constexpr (V == 4) {
    if (vec) {
      const f32x4 t = *(const f32x4*)(row + qs);
      v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
      return;
    }
  }
#pragma unroll
  for (int j = 0; j < V; ++j) v[j] = (m >> j) & 1u ? row[qs + j] : 0.f;
}

// ---- per-sample sums ---------------------------------------------------------------------------
// part[n][block] = the block's share of sum over the sample's E = Cb*H*W image elements of x
// (MASKED: of dy where the forward wrote a translated, uncut pixel: the backward's mean).  Block (0, 0)
// also advances the call counter when one is given (the forward: nothing here reads it).
template <bool MASKED>
__global__ __launch_bounds__(256) void diffaug_sum_kernel(const float* __restrict__ x, long x_bs, int E, int H, int W,
                                                          int policy, unsigned k0, unsigned k1, unsigned sid,
                                                          const long* __restrict__ used, int group,
                                                          float* __restrict__ part, long* counter, long* used_w,
                                                          long adv) {
  __shared__ float sh[4];
  aug_advance(counter, used_w, adv);
  const int n = blockIdx.y;
  const float* px = x + (long)n * x_bs;
  AugGeom g = {};
  if (MASKED) g = aug_geom(aug_draw(k0, k1, sid, used[0] + n / group, (unsigned)(n % group), H, W), policy, H, W);
  float s = 0.f;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < E; e += gridDim.x * 256) {
    float v = px[e];
    if (MASKED) {
      const int row = e / W, q = e - row * W, r = row % H;
      const bool cut = r >= g.y0 && r < g.y1 && q >= g.x0 && q < g.x1;
      const int rs = r - g.ty, qs = q - g.tx;
      v = !cut && rs >= 0 && rs < H && qs >= 0 && qs < W ? v : 0.f;
    }
    s += v;
  }
  s = block_sum<256>(s, sh);
  if (threadIdx.x == 0) part[(long)n * gridDim.x + blockIdx.x] = s;
}

// ---- forward -----------------------------------------------------------------------------------
// One lane per unit of V output columns of one row, all Ca + Cb channels of it: the Cb image values of
// a pixel meet in one lane (the saturation's channel mean).  CB > 0: they stay in registers; CB == 0
// (any Cb): the channels are read a second time (a cache hit) once their mean is known.
template <int V, int CB>
__global__ __launch_bounds__(256) void diffaug_fwd_kernel(const float* __restrict__ a, long a_bs,
                                                          const float* __restrict__ b, long b_bs,
                                                          float* __restrict__ y, long y_bs, int Ca, int Cb_rt, int H,
                                                          int W, int policy, unsigned k0, unsigned k1, unsigned sid,
                                                          const long* __restrict__ used, int group,
                                                          const float* __restrict__ part, int np) {
  __shared__ float sh[4];
  const int Cb = CB > 0 ? CB : Cb_rt;
  const int n = blockIdx.y;
  const long HW = (long)H * W;
  const AugGeom g = aug_geom(aug_draw(k0, k1, sid, used[0] + n / group, (unsigned)(n % group), H, W), policy, H, W);
  const bool color = policy & AUG_COLOR;
  float M = 0.f;
  if (color) M = parts_sum(part + (long)n * np, np, sh) / (float)(Cb * HW) + g.b;
  const float inv_cb = 1.f / (float)Cb;
  const float* pa = a ? a + (long)n * a_bs : nullptr;
  const float* pb = b + (long)n * b_bs;
  float* py = y + (long)n * y_bs;
  const int Wq = W / V, units = H * Wq;
  const bool vec_ok = V == 4 && (g.tx & 3) == 0;
  for (int u = blockIdx.x * 256 + threadIdx.x; u < units; u += gridDim.x * 256) {
    const int r = u / Wq, q0 = (u - r * Wq) * V;
    const int rs = r - g.ty, qs0 = q0 - g.tx;
    const bool row_in = rs >= 0 && rs < H, row_cut = r >= g.y0 && r < g.y1;
    unsigned m = 0;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int q = q0 + j, qs = qs0 + j;
      const bool keep = !(row_cut && q >= g.x0 && q < g.x1);
      m |= (unsigned)(keep && row_in && qs >= 0 && qs < W) << j;
    }
    const bool vec = vec_ok && m == 0xFu;
    const long src = (long)rs * W, dst = (long)r * W + q0;
    float v[V];
    if (m == 0) {   // a unit outside the shifted image or inside the cutout: zeros, nothing read
#pragma unroll
      for (int j = 0; j < V; ++j) v[j] = 0.f;
      for (int c = 0; c < Ca + Cb; ++c) st_unit<V>(py + c * HW + dst, v);
      continue;
    }
    for (int c = 0; c < Ca; ++c) {
      ld_unit<V>(pa + c * HW + src, qs0, m, vec, v);
      st_unit<V>(py + c * HW + dst, v);
    }
    float* pyb = py + Ca * HW + dst;
    if (!color) {
      for (int c = 0; c < Cb; ++c) {
        ld_unit<V>(pb + c * HW + src, qs0, m, vec, v);
        st_unit<V>(pyb + c * HW, v);
      }
      continue;
    }
    float mean[V];
#pragma unroll
    for (int j = 0; j < V; ++j) mean[j] = 0.f;
    // u'' of one channel's unit from its x, the pixel's channel mean of u and the sample's M
    auto finish = [&](float (&t)[V]) {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float u1 = (t[j] + g.b - mean[j]) * g.s + mean[j];
        const float u2 = (u1 - M) * g.c + M;
        t[j] = (m >> j) & 1u ? u2 : 0.f;
      }
    };
    if constexpr (CB > 0) {
      float xb[CB][V];
#pragma unroll
      for (int c = 0; c < CB; ++c) {
        ld_unit<V>(pb + c * HW + src, qs0, m, vec, xb[c]);
#pragma unroll
        for (int j = 0; j < V; ++j) mean[j] += xb[c][j] + g.b;
      }
#pragma unroll
      for (int j = 0; j < V; ++j) mean[j] *= inv_cb;
#pragma unroll
      for (int c = 0; c < CB; ++c) {
        finish(xb[c]);
        st_unit<V>(pyb + c * HW, xb[c]);
      }
    } else {
      for (int c = 0; c < Cb; ++c) {
        ld_unit<V>(pb + c * HW + src, qs0, m, vec, v);
#pragma unroll
        for (int j = 0; j < V; ++j) mean[j] += v[j] + g.b;
      }
#pragma unroll
      for (int j = 0; j < V; ++j) mean[j] *= inv_cb;
      for (int c = 0; c < Cb; ++c) {
        ld_unit<V>(pb + c * HW + src, qs0, m, vec, v);
        finish(v);
        st_unit<V>(pyb + c * HW, v);
      }
    }
  }
}

// ---- backward ----------------------------------------------------------------------------------
// dx[c, r, q] for the Cb image channels: g = dy[Ca + c, r + ty, q + tx] where the forward wrote that
// pixel from (r, q) and did not cut it, else 0; g1 = c g + (1 - c) mean_chw g; dx = s g1 + (1 - s) mean_c g1.
template <int V, int CB>
__global__ __launch_bounds__(256) void diffaug_bwd_kernel(const float* __restrict__ dy, long dy_bs,
                                                          float* __restrict__ dx, long dx_bs, int Ca, int Cb_rt, int H,
                                                          int W, int policy, unsigned k0, unsigned k1, unsigned sid,
                                                          const long* __restrict__ used, int group,
                                                          const float* __restrict__ part, int np) {
  __shared__ float sh[4];
  const int Cb = CB > 0 ? CB : Cb_rt;
  const int n = blockIdx.y;
  const long HW = (long)H * W;
  const AugGeom g = aug_geom(aug_draw(k0, k1, sid, used[0] + n / group, (unsigned)(n % group), H, W), policy, H, W);
  const bool color = policy & AUG_COLOR;
  float G = 0.f;
  if (color) G = parts_sum(part + (long)n * np, np, sh) / (float)(Cb * HW);
  const float gc = (1.f - g.c) * G, inv_cb = 1.f / (float)Cb;
  const float* pg = dy + (long)n * dy_bs + Ca * HW;
  float* px = dx + (long)n * dx_bs;
  const int Wq = W / V, units = H * Wq;
  const bool vec_ok = V == 4 && (g.tx & 3) == 0;
  for (int u = blockIdx.x * 256 + threadIdx.x; u < units; u += gridDim.x * 256) {
    const int r = u / Wq, q0 = (u - r * Wq) * V;
    const int rs = r + g.ty, qs0 = q0 + g.tx;   // where the forward put this pixel
    const bool row_in = rs >= 0 && rs < H, row_cut = rs >= g.y0 && rs < g.y1;
    unsigned m = 0;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int qs = qs0 + j;
      const bool keep = !(row_cut && qs >= g.x0 && qs < g.x1);
      m |= (unsigned)(keep && row_in && qs >= 0 && qs < W) << j;
    }
    const bool vec = vec_ok && m == 0xFu;
    const long src = (long)rs * W, dst = (long)r * W + q0;
    float v[V];
    if (!color) {
      for (int c = 0; c < Cb; ++c) {
        ld_unit<V>(pg + c * HW + src, qs0, m, vec, v);
        st_unit<V>(px + c * HW + dst, v);
      }
      continue;
    }
    float mean[V];
#pragma unroll
    for (int j = 0; j < V; ++j) mean[j] = 0.f;
    if constexpr (CB > 0) {
      float gb[CB][V];
#pragma unroll
      for (int c = 0; c < CB; ++c) {
        ld_unit<V>(pg + c * HW + src, qs0, m, vec, gb[c]);
#pragma unroll
        for (int j = 0; j < V; ++j) {
          gb[c][j] = fmaf(g.c, gb[c][j], gc);
          mean[j] += gb[c][j];
        }
      }
#pragma unroll
      for (int j = 0; j < V; ++j) mean[j] *= (1.f - g.s) * inv_cb;
#pragma unroll
      for (int c = 0; c < CB; ++c) {
#pragma unroll
        for (int j = 0; j < V; ++j) gb[c][j] = fmaf(g.s, gb[c][j], mean[j]);
        st_unit<V>(px + c * HW + dst, gb[c]);
      }
    } else {
      for (int c = 0; c < Cb; ++c) {
        ld_unit<V>(pg + c * HW + src, qs0, m, vec, v);
#pragma unroll
        for (int j = 0; j < V; ++j) mean[j] += fmaf(g.c, v[j], gc);
      }
#pragma unroll
      for (int j = 0; j < V; ++j) mean[j] *= (1.f - g.s) * inv_cb;
      for (int c = 0; c < Cb; ++c) {
        ld_unit<V>(pg + c * HW + src, qs0, m, vec, v);
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = fmaf(g.s, fmaf(g.c, v[j], gc), mean[j]);
        st_unit<V>(px + c * HW + dst, v);
      }
    }
  }
}

// out[i][0..7] = (b, s, c, tx, ty, oy, ox, 0) of sample i of call `call`: floats, and int32 bit patterns
__global__ __launch_bounds__(256) void diffaug_params_kernel(float* __restrict__ out, int n, unsigned k0, unsigned k1,
                                                             unsigned sid, long call, int H, int W) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const Aug p = aug_draw(k0, k1, sid, call, (unsigned)i, H, W);
  float* o = out + (long)i * 8;
  o[0] = p.b; o[1] = p.s; o[2] = p.c;
  o[3] = __int_as_float(p.tx); o[4] = __int_as_float(p.ty);
  o[5] = __int_as_float(p.oy); o[6] = __int_as_float(p.ox);
  o[7] = 0.f;
}

static inline unsigned unit_blocks(int H, int Wq) {
  long g = ((long)H * Wq + 255) / 256;
  if (g > 65535) g = 65535;
  if (g < 1) g = 1;
  return (unsigned)g;
}

}  // namespace dsg

using namespace dsg;

// the address ranges of two batches of N per-sample blocks (E elements each, at their batch strides)
// intersect; conservative: the gaps between a strided batch's samples count as its own
static inline bool spans_overlap(const float* p, long p_bs, long pE, const float* q, long q_bs, long qE, int N) {
  const float *p1 = p + (long)(N - 1) * p_bs + pE, *q1 = q + (long)(N - 1) * q_bs + qE;
  return p < q1 && q < p1;
}

static int diffaug_check(const char* who, int N, int Ca, int Cb, int H, int W, int policy, long stream_id, int group) {
  DSG_REQUIRE(N > 0 && N <= 65535 && group >= 1 && Ca >= 0 && Cb >= 1 && H >= 2 && W >= 2 && policy >= 0 && policy < 8 &&
                  stream_id >= 0 && stream_id < (1L << 32) && ((long)Ca + Cb) * H * W < (1L << 30),
              "%s: bad args (N %d, group %d, Ca %d, Cb %d, H %d, W %d, policy %d)", who, N, group, Ca, Cb, H, W, policy);
  return 0;
}

#define DIFFAUG_LAUNCH(KERNEL, V, ...)                                                                        \
  do {                                                                                                        \
    if (Cb == 1) hipLaunchKernelGGL((KERNEL<V, 1>), grid, dim3(256), 0, st, __VA_ARGS__);                     \
    else if (Cb == 3) hipLaunchKernelGGL((KERNEL<V, 3>), grid, dim3(256), 0, st, __VA_ARGS__);                \
    else hipLaunchKernelGGL((KERNEL<V, 0>), grid, dim3(256), 0, st, __VA_ARGS__);                             \
  } while (0)

extern "C" {

// block partials of the per-sample mean (forward: of b; backward: of the masked dy), N * sum_blocks
long dsgan_diffaug_workspace(int N, int Cb, int H, int W) {
  return N > 0 && Cb > 0 && H > 0 && W > 0 ? (long)N * sum_blocks((long)Cb * H * W) : 0;
}

int dsgan_diffaug_fwd(const float* a, long a_bs, const float* b, long b_bs, float* y, long y_bs, int N, int Ca, int Cb,
                      int H, int W, int policy, long seed, long stream_id, long* counter, long* used, int group,
                      float* ws, long ws_elems, hipStream_t st) {
  if (int rc = diffaug_check("dsgan_diffaug_fwd", N, Ca, Cb, H, W, policy, stream_id, group)) return rc;
  DSG_REQUIRE(b && y && counter && used && (a != nullptr) == (Ca > 0), "dsgan_diffaug_fwd: bad args (null pointer)");
  const long HW = (long)H * W;
  DSG_REQUIRE(N == 1 || (y_bs >= (Ca + Cb) * HW && b_bs >= Cb * HW && (!a || a_bs >= Ca * HW)),
              "dsgan_diffaug_fwd: batch stride below C*H*W");
  // a shifted row is read after other lanes may have written it: the destination overlaps no source
  DSG_REQUIRE(!spans_overlap(y, y_bs, (Ca + Cb) * HW, b, b_bs, Cb * HW, N) &&
                  (!a || !spans_overlap(y, y_bs, (Ca + Cb) * HW, a, a_bs, Ca * HW, N)),
              "dsgan_diffaug_fwd: the destination overlaps a source");
  const bool color = policy & AUG_COLOR;
  const unsigned np = sum_blocks(Cb * HW);
  DSG_WS(color ? (long)N * np : 0, ws, ws_elems, "dsgan_diffaug_fwd");
  const PhiloxKey key = philox_key(seed);
  const unsigned k0 = key.k0, k1 = key.k1;
  const unsigned sid = (unsigned)stream_id;
  const long adv = ((long)N + group - 1) / group;
  if (color)
    hipLaunchKernelGGL(diffaug_sum_kernel<false>, dim3(np, (unsigned)N), dim3(256), 0, st, b, b_bs, (int)(Cb * HW), H, W,
                       policy, k0, k1, sid, (const long*)nullptr, group, ws, counter, used, adv);
  else
    hipLaunchKernelGGL(diffaug_advance_kernel, dim3(1), dim3(64), 0, st, counter, used, adv);
  const bool v4 = W % 4 == 0 && al16(y, y_bs) && al16(b, b_bs) && (!a || al16(a, a_bs));
  const long* cused = used;
  if (v4) {
    const dim3 grid(unit_blocks(H, W / 4), (unsigned)N);
    DIFFAUG_LAUNCH(diffaug_fwd_kernel, 4, a, a_bs, b, b_bs, y, y_bs, Ca, Cb, H, W, policy, k0, k1, sid, cused, group,
                   (const float*)ws, (int)np);
  } else {
    const dim3 grid(unit_blocks(H, W), (unsigned)N);
    DIFFAUG_LAUNCH(diffaug_fwd_kernel, 1, a, a_bs, b, b_bs, y, y_bs, Ca, Cb, H, W, policy, k0, k1, sid, cused, group,
                   (const float*)ws, (int)np);
  }
  DSG_CHECK_LAUNCH();
  return 0;
}

// dx [N, Cb, H, W] = the transpose applied to the image channels of dy [N, Ca + Cb, H, W], with the
// draws of the forward whose counter value is used[0]
int dsgan_diffaug_bwd(const float* dy, long dy_bs, float* dx, long dx_bs, int N, int Ca, int Cb, int H, int W,
                      int policy, long seed, long stream_id, const long* used, int group, float* ws, long ws_elems,
                      hipStream_t st) {
  if (int rc = diffaug_check("dsgan_diffaug_bwd", N, Ca, Cb, H, W, policy, stream_id, group)) return rc;
  DSG_REQUIRE(dy && dx && used, "dsgan_diffaug_bwd: bad args (null pointer)");
  const long HW = (long)H * W;
  DSG_REQUIRE(N == 1 || (dy_bs >= (Ca + Cb) * HW && dx_bs >= Cb * HW), "dsgan_diffaug_bwd: batch stride below C*H*W");
  DSG_REQUIRE(!spans_overlap(dx, dx_bs, Cb * HW, dy, dy_bs, (Ca + Cb) * HW, N), "dsgan_diffaug_bwd: dx overlaps dy");
  const bool color = policy & AUG_COLOR;
  const unsigned np = sum_blocks(Cb * HW);
  DSG_WS(color ? (long)N * np : 0, ws, ws_elems, "dsgan_diffaug_bwd");
  const PhiloxKey key = philox_key(seed);
  const unsigned k0 = key.k0, k1 = key.k1;
  const unsigned sid = (unsigned)stream_id;
  if (color)
    hipLaunchKernelGGL(diffaug_sum_kernel<true>, dim3(np, (unsigned)N), dim3(256), 0, st, dy + Ca * HW, dy_bs,
                       (int)(Cb * HW), H, W, policy, k0, k1, sid, used, group, ws, (long*)nullptr, (long*)nullptr, 0L);
  const bool v4 = W % 4 == 0 && al16(dy, dy_bs) && al16(dx, dx_bs);
  if (v4) {
    const dim3 grid(unit_blocks(H, W / 4), (unsigned)N);
    DIFFAUG_LAUNCH(diffaug_bwd_kernel, 4, dy, dy_bs, dx, dx_bs, Ca, Cb, H, W, policy, k0, k1, sid, used, group,
                   (const float*)ws, (int)np);
  } else {
    const dim3 grid(unit_blocks(H, W), (unsigned)N);
    DIFFAUG_LAUNCH(diffaug_bwd_kernel, 1, dy, dy_bs, dx, dx_bs, Ca, Cb, H, W, policy, k0, k1, sid, used, group,
                   (const float*)ws, (int)np);
  }
  DSG_CHECK_LAUNCH();
  return 0;
}

// the test hook: out [n, 8] <- the draws of samples 0 .. n-1 of call `call`
int dsgan_diffaug_params(float* out, int n, long seed, long stream_id, long call, int H, int W, hipStream_t st) {
  DSG_REQUIRE(out && n > 0 && H >= 2 && W >= 2 && stream_id >= 0 && stream_id < (1L << 32) && call >= 0,
              "dsgan_diffaug_params: bad args");
  const PhiloxKey key = philox_key(seed);
  const unsigned k0 = key.k0, k1 = key.k1;
  hipLaunchKernelGGL(diffaug_params_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, out, n, k0, k1, (unsigned)stream_id,
                     call, H, W);
  DSG_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
