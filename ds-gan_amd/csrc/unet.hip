// The glue of the U-Net generator (--which_model_netG unet_128, DSGAN/models/networks.py:445-529):
//   PReLU with one learnable slope over a channel concatenation cat(a, b) (uprelu = nn.PReLU(), :493),
//   dropout from a counter-based generator (nn.Dropout(0.5), :518),
//   tanh (the outermost block's nn.Tanh, :501).
// fp32 in every precision mode; no atomics, no host synchronisation, no allocation.
#include "common.h"
#include "philox.h"

namespace dsg {

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int V> struct vec_of;
template <> struct vec_of<1> { typedef float type; };
template <> struct vec_of<4> { typedef f32x4 type; };
template <int V> __device__ __forceinline__ float& lane_of(typename vec_of<V>::type& v, int j);
template <> __device__ __forceinline__ float& lane_of<1>(float& v, int) { return v; }
template <> __device__ __forceinline__ float& lane_of<4>(f32x4& v, int j) { return ((float*)&v)[j]; }

// One workgroup row per sample (blockIdx.y = n), a grid-stride loop over the sample's E = Ea + Eb
// elements in units of V: no division on the path.  V = 4 needs Ea % 4 == Eb % 4 == 0, batch strides
// % 4 == 0 and 16-byte aligned pointers (a unit never straddles the a/b seam or a sample).
static inline unsigned row_blocks(long E) {
  long g = (E + 4095) / 4096;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  return (unsigned)g;
}

// ---- PReLU over cat(a, b) ------------------------------------------------------------------
// y[n] = prelu(cat(a[n], b[n]), alpha): x > 0 ? x : alpha * x.  alpha is read from device memory (a
// parameter in the flat buffer: Adam changes it under graph replay).  b == nullptr: single input.
template <int V>
__global__ __launch_bounds__(256) void prelu_fwd_kernel(const float* __restrict__ a, long a_bs, long Ea,
                                                        const float* __restrict__ b, long b_bs, long Eb,
                                                        const float* __restrict__ alpha, float* __restrict__ y,
                                                        long y_bs) {
  typedef typename vec_of<V>::type vec;
  const long n = blockIdx.y, E = Ea + Eb;
  const float al = alpha[0];
  const float* pa = a + n * a_bs;
  const float* pb = b ? b + n * b_bs - Ea : nullptr;   // indexed by the concatenation's offset
  float* py = y + n * y_bs;
  for (long r = (blockIdx.x * 256L + threadIdx.x) * V; r < E; r += (long)gridDim.x * 256 * V) {
    vec v = *(const vec*)((r < Ea ? pa : pb) + r);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      float& e = lane_of<V>(v, j);
      e = e > 0.f ? e : al * e;
    }
    *(vec*)(py + r) = v;
  }
}

// da / db = the halves of dy * (x > 0 ? 1 : alpha); part[block] = sum over x <= 0 of x * dy (an exact
// zero adds 0), one partial per workgroup in a fixed order.
template <int V>
__global__ __launch_bounds__(256) void prelu_bwd_kernel(const float* __restrict__ dy, long dy_bs,
                                                        const float* __restrict__ a, long a_bs, long Ea,
                                                        const float* __restrict__ b, long b_bs, long Eb,
                                                        const float* __restrict__ alpha, float* __restrict__ da,
                                                        long da_bs, float* __restrict__ db, long db_bs,
                                                        float* __restrict__ part) {
  typedef typename vec_of<V>::type vec;
  __shared__ float sh[4];
  const long n = blockIdx.y, E = Ea + Eb;
  const float al = alpha[0];
  const float* pa = a + n * a_bs;
  const float* pb = b ? b + n * b_bs - Ea : nullptr;
  const float* pg = dy + n * dy_bs;
  float* qa = da + n * da_bs;
  float* qb = db ? db + n * db_bs - Ea : nullptr;
  float s = 0.f;
  for (long r = (blockIdx.x * 256L + threadIdx.x) * V; r < E; r += (long)gridDim.x * 256 * V) {
    const bool head = r < Ea;
    vec x = *(const vec*)((head ? pa : pb) + r);
    vec g = *(const vec*)(pg + r);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float xe = lane_of<V>(x, j);
      float& ge = lane_of<V>(g, j);
      s += xe > 0.f ? 0.f : xe * ge;
      ge = xe > 0.f ? ge : al * ge;
    }
    *(vec*)((head ? qa : qb) + r) = g;
  }
  s = block_sum<256>(s, sh);
  if (threadIdx.x == 0) part[(long)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// dalpha[0] += sum of the partials: lane t adds part[t], part[t + 256], ... in that order, then the
// lanes are combined by block_sum's fixed tree -- the same bits for the same partials.
__global__ __launch_bounds__(256) void prelu_dalpha_kernel(const float* __restrict__ part, long n, float* dalpha) {
  __shared__ float sh[4];
  float s = 0.f;
  for (long i = threadIdx.x; i < n; i += 256) s += part[i];
  s = block_sum<256>(s, sh);
  if (threadIdx.x == 0) dalpha[0] = dalpha[0] + s;
}

// ---- dropout -------------------------------------------------------------------------------
// Philox-4x32-10 (Salmon et al., SC'11).  key = the 64-bit seed, counter = (group index lo, hi, call
// counter, stream id); the four output words decide the four elements 4g .. 4g+3 of the logical dense
// [N][E] tensor: element kept iff word >= thresh, thresh = round(p * 2^32).
// used[0] <- counter[0], counter[0] += 1: the forward's draw, kept for its backward.
__global__ void dropout_advance_kernel(long* counter, long* used) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const long c = counter[0];
    used[0] = c;
    counter[0] = c + 1;
  }
}

// y[n] = x[n] * (kept ? scale : 0); x == nullptr writes the 0/1 mask itself.  The call counter is
// used[0] when `used` is given (device memory: nothing on the path touches the host), else ctr_val.
template <int V>
__global__ __launch_bounds__(256) void dropout_kernel(const float* __restrict__ x, long x_bs, float* __restrict__ y,
                                                      long y_bs, long E, unsigned k0, unsigned k1, unsigned sid,
                                                      const long* __restrict__ used, long ctr_val, unsigned thresh,
                                                      float scale) {
  typedef typename vec_of<V>::type vec;
  const long n = blockIdx.y;
  const unsigned ctr = (unsigned)(used ? used[0] : ctr_val);
  const float* px = x ? x + n * x_bs : nullptr;
  float* py = y + n * y_bs;
  for (long r = (blockIdx.x * 256L + threadIdx.x) * V; r < E; r += (long)gridDim.x * 256 * V) {
    const unsigned long long e = (unsigned long long)n * (unsigned long long)E + (unsigned long long)r;
    const unsigned long long g = e >> 2;
    unsigned w[4];
    philox4x32_10((unsigned)g, (unsigned)(g >> 32), ctr, sid, k0, k1, w);
    vec v;
    if (px) {
      v = *(const vec*)(px + r);
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) lane_of<V>(v, j) = 1.f;
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const unsigned word = V == 4 ? w[j] : w[(int)(e & 3)];
      float& ve = lane_of<V>(v, j);
      ve = word >= thresh ? ve * scale : 0.f;
    }
    *(vec*)(py + r) = v;
  }
}

// ---- tanh ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tanh_fwd_kernel(const float* __restrict__ x, long n, float* __restrict__ y) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) y[i] = tanhf(x[i]);
}
__global__ __launch_bounds__(256) void tanh_bwd_kernel(const float* __restrict__ y, const float* __restrict__ dy,
                                                       long n, float* dx, int accumulate) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float t = y[i];
    const float v = dy[i] * fmaf(-t, t, 1.f);
    dx[i] = accumulate ? dx[i] + v : v;
  }
}

}  // namespace dsg

using namespace dsg;

extern "C" {

// block partials of dsgan_prelu_bwd for N samples of E elements each
long dsgan_prelu_workspace(int N, long E) { return N > 0 && E > 0 ? (long)N * row_blocks(E) : 0; }

int dsgan_prelu_fwd(const float* a, long a_bs, long Ea, const float* b, long b_bs, long Eb, const float* alpha,
                    float* y, long y_bs, int N, hipStream_t st) {
  DSG_REQUIRE(a && alpha && y && N > 0 && N <= 65535 && Ea > 0 && Eb >= 0 && (b != nullptr) == (Eb > 0),
              "dsgan_prelu_fwd: bad args");
  const long E = Ea + Eb;
  DSG_REQUIRE(N == 1 || (a_bs >= Ea && y_bs >= E && (!b || b_bs >= Eb)), "dsgan_prelu_fwd: batch stride below C*H*W");
  const dim3 grid(row_blocks(E), (unsigned)N);
  const bool v4 = Ea % 4 == 0 && Eb % 4 == 0 && a_bs % 4 == 0 && b_bs % 4 == 0 && y_bs % 4 == 0 && al16(a) &&
                  al16(b) && al16(y);
  if (v4) hipLaunchKernelGGL(prelu_fwd_kernel<4>, grid, dim3(256), 0, st, a, a_bs, Ea, b, b_bs, Eb, alpha, y, y_bs);
  else hipLaunchKernelGGL(prelu_fwd_kernel<1>, grid, dim3(256), 0, st, a, a_bs, Ea, b, b_bs, Eb, alpha, y, y_bs);
  DSG_CHECK_LAUNCH();
  return 0;
}

// dalpha (nullable: a frozen slope) is ACCUMULATED into; db is given exactly when b is
int dsgan_prelu_bwd(const float* dy, long dy_bs, const float* a, long a_bs, long Ea, const float* b, long b_bs, long Eb,
                    const float* alpha, float* da, long da_bs, float* db, long db_bs, float* dalpha, int N,
                    float* ws, long ws_elems, hipStream_t st) {
  DSG_REQUIRE(dy && a && alpha && da && N > 0 && N <= 65535 && Ea > 0 && Eb >= 0 && (b != nullptr) == (Eb > 0) &&
                  (db != nullptr) == (Eb > 0),
              "dsgan_prelu_bwd: bad args");
  const long E = Ea + Eb;
  DSG_REQUIRE(N == 1 || (dy_bs >= E && a_bs >= Ea && da_bs >= Ea && (!b || (b_bs >= Eb && db_bs >= Eb))),
              "dsgan_prelu_bwd: batch stride below C*H*W");
  const dim3 grid(row_blocks(E), (unsigned)N);
  const long parts = (long)grid.x * grid.y;
  DSG_WS(parts, ws, ws_elems, "dsgan_prelu_bwd");
  const bool v4 = Ea % 4 == 0 && Eb % 4 == 0 && dy_bs % 4 == 0 && a_bs % 4 == 0 && b_bs % 4 == 0 && da_bs % 4 == 0 &&
                  db_bs % 4 == 0 && al16(dy) && al16(a) && al16(b) && al16(da) && al16(db);
  if (v4)
    hipLaunchKernelGGL(prelu_bwd_kernel<4>, grid, dim3(256), 0, st, dy, dy_bs, a, a_bs, Ea, b, b_bs, Eb, alpha, da,
                       da_bs, db, db_bs, ws);
  else
    hipLaunchKernelGGL(prelu_bwd_kernel<1>, grid, dim3(256), 0, st, dy, dy_bs, a, a_bs, Ea, b, b_bs, Eb, alpha, da,
                       da_bs, db, db_bs, ws);
  if (dalpha) hipLaunchKernelGGL(prelu_dalpha_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, parts, dalpha);
  DSG_CHECK_LAUNCH();
  return 0;
}

// counter != nullptr: the training forward -- used[0] <- counter[0], counter[0] += 1 on the device
// first, then the mask of (seed, stream_id, used[0]).
static int dropout_launch(const char* who, const float* x, long x_bs, float* y, long y_bs, int N, long E, long seed,
                          long stream_id, long* counter, long* used, long ctr_val, long thresh, float scale,
                          hipStream_t st) {
  DSG_REQUIRE(y && N > 0 && N <= 65535 && E > 0 && thresh >= 0 && thresh < (1L << 32) && stream_id >= 0 &&
                  stream_id < (1L << 32) && (!counter || used),
              "%s: bad args", who);
  DSG_REQUIRE(N == 1 || (y_bs >= E && (!x || x_bs >= E)), "%s: batch stride below C*H*W", who);
  const dim3 grid(row_blocks(E), (unsigned)N);
  const PhiloxKey key = philox_key(seed);
  const unsigned k0 = key.k0, k1 = key.k1;
  const bool v4 = E % 4 == 0 && x_bs % 4 == 0 && y_bs % 4 == 0 && al16(x) && al16(y);
  if (counter) hipLaunchKernelGGL(dropout_advance_kernel, dim3(1), dim3(64), 0, st, counter, used);
  if (v4)
    hipLaunchKernelGGL(dropout_kernel<4>, grid, dim3(256), 0, st, x, x_bs, y, y_bs, E, k0, k1, (unsigned)stream_id,
                       (const long*)used, ctr_val, (unsigned)thresh, scale);
  else
    hipLaunchKernelGGL(dropout_kernel<1>, grid, dim3(256), 0, st, x, x_bs, y, y_bs, E, k0, k1, (unsigned)stream_id,
                       (const long*)used, ctr_val, (unsigned)thresh, scale);
  return 0;
}

// Training forward: y = x * mask * scale with a fresh mask; the call counter lives in device memory
// (`counter`, int64) and is advanced here, the value drawn is left in `used` for the backward.
int dsgan_dropout_fwd(const float* x, long x_bs, float* y, long y_bs, int N, long E, long seed, long stream_id,
                      long* counter, long* used, long thresh, float scale, hipStream_t st) {
  DSG_REQUIRE(x && counter && used, "dsgan_dropout_fwd: bad args");
  if (int rc = dropout_launch("dsgan_dropout_fwd", x, x_bs, y, y_bs, N, E, seed, stream_id, counter, used, 0, thresh,
                              scale, st))
    return rc;
  DSG_CHECK_LAUNCH();
  return 0;
}
// The same mask again for a known draw: the call counter is used[0] (device) when `used` is given,
// else ctr_val.  x == nullptr writes the 0/1 mask itself (scale ignored).  The backward is this call
// on dy with the forward's `used`.
int dsgan_dropout_apply(const float* x, long x_bs, float* y, long y_bs, int N, long E, long seed, long stream_id,
                        const long* used, long ctr_val, long thresh, float scale, hipStream_t st) {
  if (int rc = dropout_launch("dsgan_dropout_apply", x, x_bs, y, y_bs, N, E, seed, stream_id, nullptr, (long*)used,
                              ctr_val, thresh, x ? scale : 1.f, st))
    return rc;
  DSG_CHECK_LAUNCH();
  return 0;
}

int dsgan_tanh_fwd(const float* x, long n, float* y, hipStream_t st) {
  DSG_REQUIRE(x && y && n > 0, "dsgan_tanh_fwd: bad args");
  hipLaunchKernelGGL(tanh_fwd_kernel, dim3(ew_grid(n)), dim3(256), 0, st, x, n, y);
  DSG_CHECK_LAUNCH();
  return 0;
}
// dx (+)= dy * (1 - y^2) from the saved OUTPUT
int dsgan_tanh_bwd(const float* y, const float* dy, long n, float* dx, int accumulate, hipStream_t st) {
  DSG_REQUIRE(y && dy && dx && n > 0, "dsgan_tanh_bwd: bad args");
  hipLaunchKernelGGL(tanh_bwd_kernel, dim3(ew_grid(n)), dim3(256), 0, st, y, dy, n, dx, accumulate);
  DSG_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
