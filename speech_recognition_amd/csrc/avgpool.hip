// AveragePooling1D(pool_size=3, strides=1, padding='same') over act(x), forward and backward: the pool branch of the
// reference's _inception_block (model.py:312-406).  TensorFlow divides by the number of rows that EXIST in a window:
//   n_t = 3 inside a clip, 2 at its two ends, 1 when L = 1
//   fwd  z[b,t,c] = (1 / n_t) * sum over r in {t-1, t, t+1} within [0, L) of act(x[b,r,c]); act = relu6(scale*x + shift) of the
//        table bn [4][C], or the identity without one
//   bwd  dx[b,u,c] (+)= sum over t in {u-1, u, u+1} within [0, L) of dz[b,t,c] / n_t: the gradient wrt act(x) (no gate here)
// Both are HBM-bound single passes: one thread owns a float4 of channels and a run of AP_TT time steps and carries the
// three rows of a window in registers, so a row is loaded once per run (plus the two rows of the halo).  No atomics.
#include "common.h"
#include "internal.h"

namespace {

constexpr int AP_TT = 8;
constexpr int AP_THREADS = 256;

__device__ __forceinline__ float4 ap_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float ap_inv_n(int t, int L) {
  const int n = 1 + (t > 0 ? 1 : 0) + (t + 1 < L ? 1 : 0);
  return n == 3 ? (1.0f / 3.0f) : n == 2 ? 0.5f : 1.0f;
}
// row r of the activated input, zeros outside the clip
__device__ __forceinline__ float4 ap_row(const float* xb, int r, int L, int C, const float4 sc, const float4 sh, bool use_bn) {
  if (r < 0 || r >= L) return make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 v = ap_ld4(xb + (int64_t)r * C);
  if (!use_bn) return v;
  return make_float4(relu6f(fmaf(v.x, sc.x, sh.x)), relu6f(fmaf(v.y, sc.y, sh.y)), relu6f(fmaf(v.z, sc.z, sh.z)),
                     relu6f(fmaf(v.w, sc.w, sh.w)));
}
// row t of dz scaled by 1 / n_t, zeros outside the clip
__device__ __forceinline__ float4 ap_grad_row(const float* dzb, int t, int L, int C) {
  if (t < 0 || t >= L) return make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 v = ap_ld4(dzb + (int64_t)t * C);
  const float inv = ap_inv_n(t, L);
  return make_float4(v.x * inv, v.y * inv, v.z * inv, v.w * inv);
}

__global__ __launch_bounds__(AP_THREADS) void avgpool3_same_fwd_kernel(const float* __restrict__ x, const float* __restrict__ bn,
                                                                       float* __restrict__ z, int64_t n_units, int L, int C,
                                                                       int nchunks) {
  const int64_t i = (int64_t)blockIdx.x * AP_THREADS + threadIdx.x;
  if (i >= n_units) return;
  const int C4 = C >> 2;
  const int c = (int)(i % C4) * 4;
  const int64_t unit = i / C4;
  const int64_t b = unit / nchunks;
  const int t0 = (int)(unit - b * nchunks) * AP_TT;
  const bool use_bn = bn != nullptr;
  float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
  if (use_bn) {
    sc = ap_ld4(bn + c);
    sh = ap_ld4(bn + C + c);
  }
  const float* xb = x + b * L * (int64_t)C + c;
  float* zb = z + b * L * (int64_t)C + c;
  float4 a0 = ap_row(xb, t0 - 1, L, C, sc, sh, use_bn), a1 = ap_row(xb, t0, L, C, sc, sh, use_bn);
#pragma unroll
  for (int k = 0; k < AP_TT; ++k) {
    const int t = t0 + k;
    if (t >= L) break;
    const float4 a2 = ap_row(xb, t + 1, L, C, sc, sh, use_bn);
    const float inv = ap_inv_n(t, L);
    *reinterpret_cast<float4*>(zb + (int64_t)t * C) = make_float4(((a0.x + a1.x) + a2.x) * inv, ((a0.y + a1.y) + a2.y) * inv,
                                                                  ((a0.z + a1.z) + a2.z) * inv, ((a0.w + a1.w) + a2.w) * inv);
    a0 = a1;
    a1 = a2;
  }
}

__global__ __launch_bounds__(AP_THREADS) void avgpool3_same_bwd_kernel(const float* __restrict__ dz, float* __restrict__ dx,
                                                                       int64_t n_units, int L, int C, int nchunks, int accumulate) {
  const int64_t i = (int64_t)blockIdx.x * AP_THREADS + threadIdx.x;
  if (i >= n_units) return;
  const int C4 = C >> 2;
  const int c = (int)(i % C4) * 4;
  const int64_t unit = i / C4;
  const int64_t b = unit / nchunks;
  const int u0 = (int)(unit - b * nchunks) * AP_TT;
  const float* dzb = dz + b * L * (int64_t)C + c;
  float* dxb = dx + b * L * (int64_t)C + c;
  float4 g0 = ap_grad_row(dzb, u0 - 1, L, C), g1 = ap_grad_row(dzb, u0, L, C);
#pragma unroll
  for (int k = 0; k < AP_TT; ++k) {
    const int u = u0 + k;
    if (u >= L) break;
    const float4 g2 = ap_grad_row(dzb, u + 1, L, C);
    float4 v = make_float4((g0.x + g1.x) + g2.x, (g0.y + g1.y) + g2.y, (g0.z + g1.z) + g2.z, (g0.w + g1.w) + g2.w);
    float4* o = reinterpret_cast<float4*>(dxb + (int64_t)u * C);
    if (accumulate) {
      const float4 p = *o;
      v = make_float4(p.x + v.x, p.y + v.y, p.z + v.z, p.w + v.w);
    }
    *o = v;
    g0 = g1;
    g1 = g2;
  }
}

int ap_check(const char* who, int B, int L, int C) {
  KWS_REQUIRE(B > 0 && L >= 1 && C > 0, "%s: B=%d L=%d C=%d must be positive", who, B, L, C);
  KWS_REQUIRE(C % 4 == 0, "%s: C=%d must be a multiple of 4", who, C);
  KWS_REQUIRE(ceil_div64((int64_t)B * ceil_div(L, AP_TT) * (C / 4), AP_THREADS) < (1ll << 31), "%s: tensor too large", who);
  return KWS_OK;
}

}  // namespace

extern "C" {

int kws_avgpool3_same_fwd_f32(const float* x, const float* bn, float* z, int B, int L, int C, void* stream) {
  KWS_TRY(ap_check("avgpool3_same_fwd", B, L, C));
  KWS_REQUIRE(x && z, "avgpool3_same_fwd: NULL pointer");
  const int nchunks = ceil_div(L, AP_TT);
  const int64_t n_units = (int64_t)B * nchunks * (C / 4);
  KwsProfScope prof("avgpool3_same_fwd", 6.0 * B * L * C, 8.0 * B * L * C, (hipStream_t)stream);
  hipLaunchKernelGGL(avgpool3_same_fwd_kernel, dim3((unsigned)ceil_div64(n_units, AP_THREADS)), dim3(AP_THREADS), 0, (hipStream_t)stream,
                     x, bn, z, n_units, L, C, nchunks);
  KWS_LAUNCH_CHECK("avgpool3_same_fwd_kernel");
  return KWS_OK;
}

int kws_avgpool3_same_bwd_f32(const float* dz, float* dx, int accumulate, int B, int L, int C, void* stream) {
  KWS_TRY(ap_check("avgpool3_same_bwd", B, L, C));
  KWS_REQUIRE(dz && dx, "avgpool3_same_bwd: NULL pointer");
  KWS_REQUIRE(accumulate == 0 || accumulate == 1, "avgpool3_same_bwd: accumulate=%d (0 or 1)", accumulate);
  const int nchunks = ceil_div(L, AP_TT);
  const int64_t n_units = (int64_t)B * nchunks * (C / 4);
  KwsProfScope prof("avgpool3_same_bwd", 5.0 * B * L * C, 4.0 * B * L * C * (accumulate ? 3.0 : 2.0), (hipStream_t)stream);
  hipLaunchKernelGGL(avgpool3_same_bwd_kernel, dim3((unsigned)ceil_div64(n_units, AP_THREADS)), dim3(AP_THREADS), 0, (hipStream_t)stream,
                     dz, dx, n_units, L, C, nchunks, accumulate);
  KWS_LAUNCH_CHECK("avgpool3_same_bwd_kernel");
  return KWS_OK;
}

}  // extern "C"
