// BatchNorm2d(affine, running statistics) + activation for the PatchGAN under --norm batch
// (DSGAN/models/networks.py:21-30, 533-579): y = act(gamma * (x - mean_c) * rstd_c + beta) with the
// statistics of channel c taken over all N * HW values of the batch (training) or from the running
// buffers (eval), the running-buffer / counter update, and the backward
//   dz = dy * act'(z),  dbeta = sum dz,  dgamma = sum dz * xhat,
//   dx = gamma * rstd * (dz - dbeta / m - xhat * dgamma / m)      (eval: gamma * rstd * dz).
// fp32 in every precision mode; no atomics, no host synchronisation, no allocation.
//
// A channel's m = N * HW values are addressed as one flat range (n = i / HW, p = i % HW), so planes
// of any size and alignment take the same code: 16-byte accesses when HW % 4 == 0 and every operand
// is 16-byte aligned with batch strides % 4 == 0 (VEC = 4), 4-byte accesses otherwise (VEC = 1).
//
// Launch forms (dsgan_batchnorm_plan):
//   0  one workgroup of 1024 threads per channel, the channel held in registers (m <= 16384): one
//      read of x; mean, then the squared deviations from it, each a block sum.
//   1  split: the flat range is cut into S <= 64 slices.  A partial kernel over (slice, channel)
//      writes one partial per slice to scratch -- forward (count, mean, M2) with M2 taken about the
//      partial's own mean from register-held values, backward (sum dz, sum dz * xhat); the apply
//      kernel over the same (slice, channel) grid first combines its channel's S partials in slice
//      order (Chan's pairwise update for the forward), then streams its slice.  The workgroup of
//      slice 0 also writes mean / rstd, the running buffers, the counter and dgamma / dbeta from
//      one lane.  The variance is never formed as E[x^2] - E[x]^2.
// Every summation order is a function of (N, C, HW) and the operands' alignment only.
#include "common.h"

namespace dsg {

constexpr int BN_E = 16;          // values a thread holds per batch
constexpr int BN_ONE_NT = 1024;   // form 0: threads per channel
constexpr int BN_ONE_MAX = BN_ONE_NT * BN_E;
constexpr int BN_NT = 256;        // form 1: threads per workgroup
constexpr int BN_SLICE = BN_NT * BN_E;
constexpr int BN_MAX_S = 64;

static int g_bn_form = 0;   // dsgan_batchnorm_tune key 0: 0 planner, 1 form 0 wherever it fits, 2 form 1 everywhere

struct BNPlan {
  int form;   // 0 one workgroup per channel, 1 split
  int S;      // slices per channel (form 1; also the grid of the eval-mode apply launch)
  long need;  // scratch elements
};

static BNPlan bn_plan(int N, int C, int HW) {
  const long m = (long)N * HW;
  BNPlan p;
  long S = (m + BN_SLICE - 1) / BN_SLICE;
  p.S = (int)(S < 1 ? 1 : S > BN_MAX_S ? BN_MAX_S : S);
  // Form 0 reads x once and saves a launch boundary, but puts a whole channel on one CU: it is
  // taken when a slice would hold the channel anyway (S == 1), or when the channels alone give
  // every other CU a workgroup.
  bool one = m <= BN_ONE_MAX && (m <= BN_SLICE || C >= 128);
  if (g_bn_form == 1) one = m <= BN_ONE_MAX;
  if (g_bn_form == 2) one = false;
  p.form = one ? 0 : 1;
  p.need = one ? 0 : (long)C * p.S * 3;
  return p;
}

struct BNFwdArgs {
  const float* x; long x_bs;
  const float* gamma; const float* beta;
  float* y; long y_bs;
  float* mean; float* rstd;
  float* running_mean; float* running_var; long* nbt;
  int N, C, HW, act;
  float slope, eps, momentum;
  int training;
};

struct BNBwdArgs {
  const float* dy; long dy_bs;
  const float* x; long x_bs;
  const float* gamma; const float* beta;
  const float* mean; const float* rstd;
  float* dx; long dx_bs;
  float* dgamma; float* dbeta;
  int N, C, HW, act;
  float slope;
  int training;
};

// element offset of unit u (VEC values) of a channel whose first plane starts at coff
template <int VEC>
__device__ __forceinline__ long bn_off(int u, int HWv, long bs, long coff) {
  const int n = u / HWv;
  return (long)n * bs + coff + (long)(u - n * HWv) * VEC;
}

// v[j * VEC ..] = unit u0 + j * NT of the channel, j < BN_E / VEC.  Units at or past `end` are read
// from unit end - 1 (a valid address: no branch around the loads) and counted out: the return
// value is the number of valid values, which are v[0 .. count).
template <int VEC, int NT>
__device__ __forceinline__ int bn_load(const float* __restrict__ p, long bs, long coff, int HWv, int u0, int end,
                                       float (&v)[BN_E]) {
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < BN_E / VEC; ++j) {
    const int u = u0 + j * NT;
    const float* q = p + bn_off<VEC>(u < end ? u : end - 1, HWv, bs, coff);
    if constexpr (VEC == 4) {
      const float4 t = *reinterpret_cast<const float4*>(q);
      v[4 * j] = t.x; v[4 * j + 1] = t.y; v[4 * j + 2] = t.z; v[4 * j + 3] = t.w;
    } else {
      v[j] = *q;
    }
    cnt += u < end ? VEC : 0;
  }
  return cnt;
}

template <int VEC, int NT>
__device__ __forceinline__ void bn_store(float* __restrict__ p, long bs, long coff, int HWv, int u0, int end,
                                         const float (&v)[BN_E]) {
#pragma unroll
  for (int j = 0; j < BN_E / VEC; ++j) {
    const int u = u0 + j * NT;
    if (u < end) {
      float* q = p + bn_off<VEC>(u, HWv, bs, coff);
      if constexpr (VEC == 4) *reinterpret_cast<float4*>(q) = make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
      else *q = v[j];
    }
  }
}

// (na, ma, qa) <- the statistics of the union of two disjoint sets (count, mean, sum of squared
// deviations): Chan, Golub & LeVeque's pairwise update.  Empty sets are allowed on either side.
__device__ __forceinline__ void bn_merge(float& na, float& ma, float& qa, float nb, float mb, float qb) {
  const float n = na + nb;
  const float f = n > 0.f ? nb / n : 0.f;
  const float d = mb - ma;
  ma = fmaf(d, f, ma);
  qa = (qa + qb) + (d * d) * (na * f);
  na = n;
}

// the statistics of v[0 .. cnt) about their own mean
__device__ __forceinline__ void bn_batch_stats(const float (&v)[BN_E], int cnt, float& mb, float& qb) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < BN_E; ++i) s += i < cnt ? v[i] : 0.f;
  mb = cnt > 0 ? s / (float)cnt : 0.f;
  qb = 0.f;
#pragma unroll
  for (int i = 0; i < BN_E; ++i) {
    const float d = v[i] - mb;
    qb += i < cnt ? d * d : 0.f;
  }
}

// slice s of a channel of M units, in units: [lo, hi)
__device__ __forceinline__ void bn_slice(int M, int S, int s, int& lo, int& hi) {
  const int L = (M + S - 1) / S;
  lo = s * L < M ? s * L : M;
  hi = lo + L < M ? lo + L : M;
}

// what the forward leaves behind for channel c (one lane)
__device__ __forceinline__ void bn_write_stats(const BNFwdArgs& a, int c, float mean, float q, float rs) {
  a.mean[c] = mean;
  a.rstd[c] = rs;
  if (a.training) {
    const float m = (float)a.N * (float)a.HW;
    a.running_mean[c] = (1.f - a.momentum) * a.running_mean[c] + a.momentum * mean;
    a.running_var[c] = (1.f - a.momentum) * a.running_var[c] + a.momentum * (q / (m - 1.f));
    if (c == 0 && a.nbt) *a.nbt += 1;
  }
}

// ---- form 0: one workgroup per channel -----------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(BN_ONE_NT) void bn_fwd_one(BNFwdArgs a) {
  __shared__ float sh[BN_ONE_NT / 64];
  const int c = blockIdx.x, HWv = a.HW / VEC, M = a.N * HWv;
  const long coff = (long)c * a.HW;
  float v[BN_E];
  const int cnt = bn_load<VEC, BN_ONE_NT>(a.x, a.x_bs, coff, HWv, threadIdx.x, M, v);
  const float m = (float)a.N * (float)a.HW;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < BN_E; ++i) s += i < cnt ? v[i] : 0.f;
  const float mean = block_sum<BN_ONE_NT>(s, sh) / m;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < BN_E; ++i) {
    const float d = v[i] - mean;
    q += i < cnt ? d * d : 0.f;
  }
  q = block_sum<BN_ONE_NT>(q, sh);
  const float rs = 1.f / sqrtf(q / m + a.eps);
  if (threadIdx.x == 0) bn_write_stats(a, c, mean, q, rs);
  const float g = a.gamma[c] * rs, b = a.beta[c];
#pragma unroll
  for (int i = 0; i < BN_E; ++i) v[i] = act_f(a.act, fmaf(v[i] - mean, g, b), a.slope);
  bn_store<VEC, BN_ONE_NT>(a.y, a.y_bs, coff, HWv, threadIdx.x, M, v);
}

template <int VEC>
__global__ __launch_bounds__(BN_ONE_NT) void bn_bwd_one(BNBwdArgs a) {
  __shared__ float sh[BN_ONE_NT / 64];
  const int c = blockIdx.x, HWv = a.HW / VEC, M = a.N * HWv;
  const long coff = (long)c * a.HW;
  float xh[BN_E], dz[BN_E];
  const int cnt = bn_load<VEC, BN_ONE_NT>(a.x, a.x_bs, coff, HWv, threadIdx.x, M, xh);
  bn_load<VEC, BN_ONE_NT>(a.dy, a.dy_bs, coff, HWv, threadIdx.x, M, dz);
  const float mean = a.mean[c], rs = a.rstd[c];
  const float g = a.gamma[c] * rs, b = a.beta[c];
  float sg = 0.f, sgh = 0.f;
#pragma unroll
  for (int i = 0; i < BN_E; ++i) {
    const float d = xh[i] - mean;
    dz[i] = i < cnt ? dz[i] * act_g(a.act, fmaf(d, g, b), a.slope) : 0.f;
    xh[i] = d * rs;
    sg += dz[i];
    sgh = fmaf(dz[i], xh[i], sgh);
  }
  sg = block_sum<BN_ONE_NT>(sg, sh);
  sgh = block_sum<BN_ONE_NT>(sgh, sh);
  if (threadIdx.x == 0 && a.dgamma) { a.dgamma[c] += sgh; a.dbeta[c] += sg; }
  const float inv = 1.f / ((float)a.N * (float)a.HW);
  const float mg = a.training ? sg * inv : 0.f, mgh = a.training ? sgh * inv : 0.f;
#pragma unroll
  for (int i = 0; i < BN_E; ++i) dz[i] = g * (dz[i] - mg - xh[i] * mgh);
  bn_store<VEC, BN_ONE_NT>(a.dx, a.dx_bs, coff, HWv, threadIdx.x, M, dz);
}

// ---- form 1: partials per (slice, channel), then apply -------------------------------------
// ws[(c * S + s) * 3 + {0, 1, 2}] = (count, mean, M2) of slice s of channel c
template <int VEC>
__global__ __launch_bounds__(BN_NT) void bn_fwd_part(BNFwdArgs a, float* __restrict__ ws, int S) {
  __shared__ float sh[3 * BN_NT / 64];
  const int s = blockIdx.x, c = blockIdx.y, HWv = a.HW / VEC, M = a.N * HWv;
  const long coff = (long)c * a.HW;
  int lo, hi;
  bn_slice(M, S, s, lo, hi);
  float n = 0.f, mu = 0.f, q = 0.f;
  for (int base = lo; base < hi; base += BN_NT * (BN_E / VEC)) {
    float v[BN_E], mb, qb;
    const int cnt = bn_load<VEC, BN_NT>(a.x, a.x_bs, coff, HWv, base + threadIdx.x, hi, v);
    bn_batch_stats(v, cnt, mb, qb);
    bn_merge(n, mu, q, (float)cnt, mb, qb);
  }
  // lane l takes in lane l + o; lane 0 ends with the wave's statistics
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float nb = __shfl_down(n, o, 64), mb = __shfl_down(mu, o, 64), qb = __shfl_down(q, o, 64);
    bn_merge(n, mu, q, nb, mb, qb);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sh[3 * w] = n; sh[3 * w + 1] = mu; sh[3 * w + 2] = q; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < BN_NT / 64; ++i) bn_merge(n, mu, q, sh[3 * i], sh[3 * i + 1], sh[3 * i + 2]);
    float* o = ws + ((long)c * S + s) * 3;
    o[0] = n; o[1] = mu; o[2] = q;
  }
}

// S > 0: the channel's statistics from its S partials (training);  S == 0: the running buffers (eval)
template <int VEC>
__global__ __launch_bounds__(BN_NT) void bn_fwd_apply(BNFwdArgs a, const float* __restrict__ ws, int S) {
  const int s = blockIdx.x, c = blockIdx.y, HWv = a.HW / VEC, M = a.N * HWv;
  const long coff = (long)c * a.HW;
  float mean, q = 0.f, rs;
  if (S > 0) {
    const float* p = ws + (long)c * S * 3;
    float n = p[0];
    mean = p[1]; q = p[2];
    for (int i = 1; i < S; ++i) bn_merge(n, mean, q, p[3 * i], p[3 * i + 1], p[3 * i + 2]);
    rs = 1.f / sqrtf(q / ((float)a.N * (float)a.HW) + a.eps);
  } else {
    mean = a.running_mean[c];
    rs = 1.f / sqrtf(a.running_var[c] + a.eps);
  }
  const float g = a.gamma[c] * rs, b = a.beta[c];
  int lo, hi;
  bn_slice(M, gridDim.x, s, lo, hi);
  for (int base = lo; base < hi; base += BN_NT * (BN_E / VEC)) {
    float v[BN_E];
    bn_load<VEC, BN_NT>(a.x, a.x_bs, coff, HWv, base + threadIdx.x, hi, v);
#pragma unroll
    for (int i = 0; i < BN_E; ++i) v[i] = act_f(a.act, fmaf(v[i] - mean, g, b), a.slope);
    bn_store<VEC, BN_NT>(a.y, a.y_bs, coff, HWv, base + threadIdx.x, hi, v);
  }
  // after the stream: in eval mode mean / rstd may not alias the running buffers it reads, and
  // nothing else of this launch reads what is written here
  if (s == 0 && threadIdx.x == 0) bn_write_stats(a, c, mean, q, rs);
}

// dz and xhat of one batch of values (0 past the slice's end)
template <int VEC>
__device__ __forceinline__ void bn_bwd_load(const BNBwdArgs& a, long coff, int HWv, int u0, int end, float mean, float rs,
                                            float g, float b, float (&xh)[BN_E], float (&dz)[BN_E]) {
  const int cnt = bn_load<VEC, BN_NT>(a.x, a.x_bs, coff, HWv, u0, end, xh);
  bn_load<VEC, BN_NT>(a.dy, a.dy_bs, coff, HWv, u0, end, dz);
#pragma unroll
  for (int i = 0; i < BN_E; ++i) {
    const float d = xh[i] - mean;
    dz[i] = i < cnt ? dz[i] * act_g(a.act, fmaf(d, g, b), a.slope) : 0.f;
    xh[i] = d * rs;
  }
}

// ws[(c * S + s) * 2 + {0, 1}] = (sum dz, sum dz * xhat) over slice s of channel c
template <int VEC>
__global__ __launch_bounds__(BN_NT) void bn_bwd_part(BNBwdArgs a, float* __restrict__ ws, int S) {
  __shared__ float sh[BN_NT / 64];
  const int s = blockIdx.x, c = blockIdx.y, HWv = a.HW / VEC, M = a.N * HWv;
  const long coff = (long)c * a.HW;
  const float mean = a.mean[c], rs = a.rstd[c];
  const float g = a.gamma[c] * rs, b = a.beta[c];
  int lo, hi;
  bn_slice(M, S, s, lo, hi);
  float sg = 0.f, sgh = 0.f;
  for (int base = lo; base < hi; base += BN_NT * (BN_E / VEC)) {
    float xh[BN_E], dz[BN_E];
    bn_bwd_load<VEC>(a, coff, HWv, base + threadIdx.x, hi, mean, rs, g, b, xh, dz);
#pragma unroll
    for (int i = 0; i < BN_E; ++i) {
      sg += dz[i];
      sgh = fmaf(dz[i], xh[i], sgh);
    }
  }
  sg = block_sum<BN_NT>(sg, sh);
  sgh = block_sum<BN_NT>(sgh, sh);
  if (threadIdx.x == 0) {
    float* o = ws + ((long)c * S + s) * 2;
    o[0] = sg; o[1] = sgh;
  }
}

// S > 0: the channel sums from its S partials;  S == 0: none (eval mode with frozen parameters)
template <int VEC>
__global__ __launch_bounds__(BN_NT) void bn_bwd_apply(BNBwdArgs a, const float* __restrict__ ws, int S) {
  const int s = blockIdx.x, c = blockIdx.y, HWv = a.HW / VEC, M = a.N * HWv;
  const long coff = (long)c * a.HW;
  const float mean = a.mean[c], rs = a.rstd[c];
  const float g = a.gamma[c] * rs, b = a.beta[c];
  float sg = 0.f, sgh = 0.f;
  for (int i = 0; i < S; ++i) {
    sg += ws[((long)c * S + i) * 2];
    sgh += ws[((long)c * S + i) * 2 + 1];
  }
  if (S > 0 && s == 0 && threadIdx.x == 0 && a.dgamma) { a.dgamma[c] += sgh; a.dbeta[c] += sg; }
  const float inv = 1.f / ((float)a.N * (float)a.HW);
  const float mg = a.training ? sg * inv : 0.f, mgh = a.training ? sgh * inv : 0.f;
  int lo, hi;
  bn_slice(M, gridDim.x, s, lo, hi);
  for (int base = lo; base < hi; base += BN_NT * (BN_E / VEC)) {
    float xh[BN_E], dz[BN_E];
    bn_bwd_load<VEC>(a, coff, HWv, base + threadIdx.x, hi, mean, rs, g, b, xh, dz);
#pragma unroll
    for (int i = 0; i < BN_E; ++i) dz[i] = g * (dz[i] - mg - xh[i] * mgh);
    bn_store<VEC, BN_NT>(a.dx, a.dx_bs, coff, HWv, base + threadIdx.x, hi, dz);
  }
}


}  // namespace dsg

using namespace dsg;

#define BN_LAUNCH(vec4, kern, grid, block, st, ...)                                   \
  do {                                                                                \
    if (vec4) hipLaunchKernelGGL(kern<4>, grid, block, 0, st, __VA_ARGS__);           \
    else hipLaunchKernelGGL(kern<1>, grid, block, 0, st, __VA_ARGS__);                \
  } while (0)

static int bn_check_geo(const char* who, int N, int C, int HW) {
  DSG_REQUIRE(N > 0 && C > 0 && HW > 0, "%s: bad geometry N=%d C=%d HW=%d", who, N, C, HW);
  DSG_REQUIRE(C <= 65535, "%s: C=%d is beyond one launch grid (65535)", who, C);
  DSG_REQUIRE((long)N * HW <= (1L << 30), "%s: N*HW=%ld is beyond 32-bit indexing", who, (long)N * HW);
  return 0;
}

extern "C" {

long dsgan_batchnorm_workspace(int N, int C, int HW) {
  if (N <= 0 || C <= 0 || HW <= 0) return 0;
  return bn_plan(N, C, HW).need;
}

long dsgan_batchnorm_plan(int N, int C, int HW) {
  if (N <= 0 || C <= 0 || HW <= 0) return -1;
  return bn_plan(N, C, HW).form;
}

int dsgan_batchnorm_tune(int key, int val) {
  if (key != 0) return -1;
  const int old = g_bn_form;
  if (val >= 0 && val <= 2) g_bn_form = val;
  return old;
}

int dsgan_batchnorm_fwd(const float* x, long x_bs, const float* gamma, const float* beta, float* y, long y_bs,
                        float* mean, float* rstd, float* running_mean, float* running_var, long* num_batches_tracked,
                        int N, int C, int HW, int act, float slope, float eps, float momentum, int training,
                        float* ws, long ws_elems, hipStream_t stream) {
  if (bn_check_geo("dsgan_batchnorm_fwd", N, C, HW)) return -1;
  DSG_REQUIRE(x && gamma && beta && y && mean && rstd, "dsgan_batchnorm_fwd: null operand");
  DSG_REQUIRE(x_bs >= (long)C * HW && y_bs >= (long)C * HW, "dsgan_batchnorm_fwd: batch stride below C*HW");
  DSG_REQUIRE(running_mean && running_var, "dsgan_batchnorm_fwd: the running buffers are needed in both modes");
  DSG_REQUIRE(!training || (long)N * HW > 1,
              "dsgan_batchnorm_fwd: Expected more than 1 value per channel when training (N*HW == 1)");
  DSG_REQUIRE(training || (mean != running_mean && rstd != running_var),
              "dsgan_batchnorm_fwd: mean / rstd may not alias the running buffers");
  const BNPlan p = bn_plan(N, C, HW);
  DSG_WS(p.need, ws, ws_elems, "dsgan_batchnorm_fwd");
  const bool v4 = HW % 4 == 0 && x_bs % 4 == 0 && y_bs % 4 == 0 && al16(x) && al16(y);
  BNFwdArgs a{x, x_bs, gamma, beta, y, y_bs, mean, rstd, running_mean, running_var, num_batches_tracked,
              N, C, HW, act, slope, eps, momentum, training ? 1 : 0};
  if (!training) {
    BN_LAUNCH(v4, bn_fwd_apply, dim3(p.S, C), dim3(BN_NT), stream, a, (const float*)nullptr, 0);
  } else if (p.form == 0) {
    BN_LAUNCH(v4, bn_fwd_one, dim3(C), dim3(BN_ONE_NT), stream, a);
  } else {
    BN_LAUNCH(v4, bn_fwd_part, dim3(p.S, C), dim3(BN_NT), stream, a, ws, p.S);
    BN_LAUNCH(v4, bn_fwd_apply, dim3(p.S, C), dim3(BN_NT), stream, a, (const float*)ws, p.S);
  }
  DSG_CHECK_LAUNCH();
  return 0;
}

int dsgan_batchnorm_bwd(const float* dy, long dy_bs, const float* x, long x_bs, const float* gamma, const float* beta,
                        const float* mean, const float* rstd, float* dx, long dx_bs, float* dgamma, float* dbeta,
                        int N, int C, int HW, int act, float slope, int training,
                        float* ws, long ws_elems, hipStream_t stream) {
  if (bn_check_geo("dsgan_batchnorm_bwd", N, C, HW)) return -1;
  DSG_REQUIRE(dy && x && gamma && beta && mean && rstd && dx, "dsgan_batchnorm_bwd: null operand");
  DSG_REQUIRE((dgamma == nullptr) == (dbeta == nullptr), "dsgan_batchnorm_bwd: dgamma / dbeta are given as a pair");
  DSG_REQUIRE(dy_bs >= (long)C * HW && x_bs >= (long)C * HW && dx_bs >= (long)C * HW,
              "dsgan_batchnorm_bwd: batch stride below C*HW");
  DSG_REQUIRE(!training || (long)N * HW > 1, "dsgan_batchnorm_bwd: N*HW == 1 in training mode");
  const BNPlan p = bn_plan(N, C, HW);
  DSG_WS(p.need, ws, ws_elems, "dsgan_batchnorm_bwd");
  const bool v4 = HW % 4 == 0 && dy_bs % 4 == 0 && x_bs % 4 == 0 && dx_bs % 4 == 0 && al16(dy) && al16(x) &&
                  al16(dx);
  BNBwdArgs a{dy, dy_bs, x, x_bs, gamma, beta, mean, rstd, dx, dx_bs, dgamma, dbeta,
              N, C, HW, act, slope, training ? 1 : 0};
  if (p.form == 0) {
    BN_LAUNCH(v4, bn_bwd_one, dim3(C), dim3(BN_ONE_NT), stream, a);
  } else if (training || dgamma) {
    BN_LAUNCH(v4, bn_bwd_part, dim3(p.S, C), dim3(BN_NT), stream, a, ws, p.S);
    BN_LAUNCH(v4, bn_bwd_apply, dim3(p.S, C), dim3(BN_NT), stream, a, (const float*)ws, p.S);
  } else {
    BN_LAUNCH(v4, bn_bwd_apply, dim3(p.S, C), dim3(BN_NT), stream, a, (const float*)nullptr, 0);
  }
  DSG_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
