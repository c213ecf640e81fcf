// MaxPool1D(pool_size=3, strides=2, padding='same') over relu6(bn(y)), forward and backward: the pool of the reference's
// _reduce_conv in conv_1d_multi_time_sliced_model (model.py:1093-1097), where it follows the depthwise block's
// Conv1D(F, 1) + BatchNormalization + relu6 directly.  The contract of pool.hip's VALID pair, with TensorFlow's SAME geometry:
//   Lp = ceil(L / 2); pad_total = 2 (Lp - 1) + 3 - L = 1 (even L) or 2 (odd L); pad_left = pad_total / 2 = 0 (even L) or 1 (odd L)
//   fwd   z[b,t,c] = max over the VALID rows r = 2t - pad_left + j, j < 3, of relu6(scale[c] * y[b,r,c] + shift[c]).  Padding
//         never wins a window (TF pads with -inf); the middle row of every window is a valid one.  The activation comes BEFORE
//         the maximum: a BatchNorm scale may be negative.
//   bwd   gather form: g[b,u,c] = gate(u) * sum of dz[b,t,c] over the (at most two) windows t that u won, where the FIRST
//         maximum among a window's valid rows wins (TF MaxPoolGrad) and gate = relu6'(bn(y[b,u,c])) = [0 < pre <= 6].  Every
//         element of g is written exactly once (every row is in some window here).  In the same pass the per-workgroup
//         BatchNorm partial sums part[row][2][C] = (sum g, sum g * xhat) go out, folded afterwards in a fixed order
//         (bncols.hip gbn_bwd_fin_kernel): no float atomics, bit-reproducible.
// Both are HBM-bound: one thread owns a float4 of channels and a short run of time steps (16-byte loads and stores), and a
// row shared by two windows is read from HBM once (the forward carries it in registers, the backward's re-reads hit L1/L2).
#include <math.h>

#include "common.h"
#include "internal.h"

namespace {

constexpr int PS_FWD_TT = 4;   // outputs per thread (forward): 2 * 4 + 1 input rows
constexpr int PS_BWD_TT = 8;   // input positions per thread (backward), even: a run starts at an even row
constexpr int PS_THREADS = 256;
constexpr int PS_MAXC = 1024;  // C / 4 threads of one time run fit one workgroup

__device__ __forceinline__ float4 ps_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
// activation of row r, or -inf for a row of the padding
__device__ __forceinline__ float4 ps_act(const float* yb, int r, int L, int C, const float4 sc, const float4 sh) {
  if (r < 0 || r >= L) return make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
  const float4 v = ps_ld4(yb + (int64_t)r * C);
  return make_float4(relu6f(fmaf(v.x, sc.x, sh.x)), relu6f(fmaf(v.y, sc.y, sh.y)), relu6f(fmaf(v.z, sc.z, sh.z)),
                     relu6f(fmaf(v.w, sc.w, sh.w)));
}
__device__ __forceinline__ float ps_max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

__global__ __launch_bounds__(PS_THREADS) void pool3s2_same_fwd_kernel(const float* __restrict__ y, const float* __restrict__ bn,
                                                                      float* __restrict__ z, int64_t n_units, int L, int Lp, int C,
                                                                      int nchunks, int pl, int zp) {
  const int64_t i = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x;
  if (i >= n_units) return;
  const int C4 = C >> 2;
  const int c = (int)(i % C4) * 4;
  const int64_t unit = i / C4;
  const int64_t b = unit / nchunks;
  const int t0 = (int)(unit - b * nchunks) * PS_FWD_TT;
  const float4 sc = ps_ld4(bn + c), sh = ps_ld4(bn + C + c);
  const float* yb = y + b * L * (int64_t)C + c;
  float* zb = z + b * Lp * (int64_t)zp + c;   // zp: row pitch of z (C for the public entry point)
  float4 a0 = ps_act(yb, 2 * t0 - pl, L, C, sc, sh);
#pragma unroll
  for (int k = 0; k < PS_FWD_TT; ++k) {
    const int t = t0 + k;
    if (t >= Lp) break;
    const int r = 2 * t - pl;   // rows r, r + 1, r + 2; r + 1 <= L - 1 for every t < Lp
    const float4 a1 = ps_act(yb, r + 1, L, C, sc, sh), a2 = ps_act(yb, r + 2, L, C, sc, sh);
    *reinterpret_cast<float4*>(zb + (int64_t)t * zp) =
        make_float4(ps_max3(a0.x, a1.x, a2.x), ps_max3(a0.y, a1.y, a2.y), ps_max3(a0.z, a1.z, a2.z), ps_max3(a0.w, a1.w, a2.w));
    a0 = a2;
  }
}

// offset (0..2) of the first maximum of a window; a padding row holds -inf and the middle row is valid, so padding never wins
__device__ __forceinline__ int ps_first_max3(float a0, float a1, float a2) {
  int j = 0;
  float m = a0;
  if (a1 > m) { m = a1; j = 1; }
  if (a2 > m) j = 2;
  return j;
}
__device__ __forceinline__ float ps_gate(float pre) { return (pre > 0.f && pre <= 6.f) ? 1.f : 0.f; }

// One thread: float4 of channels x the PS_BWD_TT input rows u0 .. u0 + 7 (u0 even).  PL = pad_left.  The windows that can hand
// a gradient to those rows are t = u0 / 2 - 1 + PL + w, w = 0 .. 4 (rows u0 - 2 + PL + 2w .. u0 + PL + 2w); window w's element j
// is run position 2w - 2 + PL + j.
template <int PL>
__global__ __launch_bounds__(PS_THREADS) void pool3s2_same_bwd_kernel(const float* __restrict__ dz, const float* __restrict__ y,
                                                                      const float* __restrict__ bn, float* __restrict__ g,
                                                                      float* __restrict__ part, int64_t units, int L, int Lp, int C,
                                                                      int nchunks, int R, int zp) {
  __shared__ float red[2][PS_THREADS * 4];
  const int C4 = C >> 2;
  const int tid = threadIdx.x;
  const int r = tid / C4, c4 = tid - r * C4;
  const int c = c4 * 4;
  const int64_t unit = (int64_t)blockIdx.x * R + r;
  float4 sg = make_float4(0.f, 0.f, 0.f, 0.f), sgx = sg;
  if (unit < units) {
    const int64_t b = unit / nchunks;
    const int u0 = (int)(unit - b * nchunks) * PS_BWD_TT;
    const float4 sc = ps_ld4(bn + c), sh = ps_ld4(bn + C + c), mean = ps_ld4(bn + 2 * C + c), rstd = ps_ld4(bn + 3 * C + c);
    const float* yb = y + b * L * (int64_t)C + c;
    const float* dzb = dz + b * Lp * (int64_t)zp + c;   // zp: row pitch of dz
    float4 acc[PS_BWD_TT];
#pragma unroll
    for (int i = 0; i < PS_BWD_TT; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    const int tb = u0 / 2 - 1 + PL;
    float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f);
    bool have0 = false;   // a0 = activation of the first row of the next window (the last row of the one before it)
#pragma unroll
    for (int w = 0; w <= PS_BWD_TT / 2; ++w) {
      const int t = tb + w;
      if (t < 0 || t >= Lp) {
        have0 = false;
        continue;
      }
      const int r0 = 2 * t - PL;
      if (!have0) a0 = ps_act(yb, r0, L, C, sc, sh);
      const float4 a1 = ps_act(yb, r0 + 1, L, C, sc, sh), a2 = ps_act(yb, r0 + 2, L, C, sc, sh);
      const float4 d = ps_ld4(dzb + (int64_t)t * zp);
#define KWS_POOL_SAME_ROUTE(f)                                                                          \
  do {                                                                                                  \
    const int j = ps_first_max3(a0.f, a1.f, a2.f);                                                      \
    if (2 * w - 2 + PL >= 0 && 2 * w - 2 + PL < PS_BWD_TT && j == 0)                                    \
      acc[(2 * w - 2 + PL >= 0 && 2 * w - 2 + PL < PS_BWD_TT) ? 2 * w - 2 + PL : 0].f += d.f;           \
    if (2 * w - 1 + PL >= 0 && 2 * w - 1 + PL < PS_BWD_TT && j == 1)                                    \
      acc[(2 * w - 1 + PL >= 0 && 2 * w - 1 + PL < PS_BWD_TT) ? 2 * w - 1 + PL : 0].f += d.f;           \
    if (2 * w + PL < PS_BWD_TT && j == 2) acc[(2 * w + PL < PS_BWD_TT) ? 2 * w + PL : 0].f += d.f;      \
  } while (0)
      KWS_POOL_SAME_ROUTE(x);
      KWS_POOL_SAME_ROUTE(y);
      KWS_POOL_SAME_ROUTE(z);
      KWS_POOL_SAME_ROUTE(w);
#undef KWS_POOL_SAME_ROUTE
      a0 = a2;
      have0 = true;
    }
#pragma unroll
    for (int i = 0; i < PS_BWD_TT; ++i) {
      const int u = u0 + i;
      if (u >= L) break;
      const float4 yu = ps_ld4(yb + (int64_t)u * C);
      const float4 g0 = make_float4(acc[i].x * ps_gate(fmaf(yu.x, sc.x, sh.x)), acc[i].y * ps_gate(fmaf(yu.y, sc.y, sh.y)),
                                    acc[i].z * ps_gate(fmaf(yu.z, sc.z, sh.z)), acc[i].w * ps_gate(fmaf(yu.w, sc.w, sh.w)));
      *reinterpret_cast<float4*>(g + (b * L + u) * (int64_t)C + c) = g0;
      sg.x += g0.x; sg.y += g0.y; sg.z += g0.z; sg.w += g0.w;
      sgx.x = fmaf(g0.x, (yu.x - mean.x) * rstd.x, sgx.x);
      sgx.y = fmaf(g0.y, (yu.y - mean.y) * rstd.y, sgx.y);
      sgx.z = fmaf(g0.z, (yu.z - mean.z) * rstd.z, sgx.z);
      sgx.w = fmaf(g0.w, (yu.w - mean.w) * rstd.w, sgx.w);
    }
  }
  *reinterpret_cast<float4*>(&red[0][tid * 4]) = sg;
  *reinterpret_cast<float4*>(&red[1][tid * 4]) = sgx;
  __syncthreads();
  for (int o = tid; o < 2 * C; o += blockDim.x) {   // the R time runs of this workgroup, ascending
    const int q = o / C, ch = o - q * C;
    float s = 0.f;
    for (int rr = 0; rr < R; ++rr) s += red[q][rr * C + ch];
    part[((int64_t)blockIdx.x * 2 + q) * C + ch] = s;
  }
}

bool ps_ok(int B, int L, int C) { return B > 0 && L >= 2 && C > 0 && C % 4 == 0 && C <= PS_MAXC; }
struct PsGeom {
  int nchunks, R, block;
  int64_t units, grid;
};
PsGeom ps_geom(int B, int L, int C) {
  PsGeom ge;
  ge.nchunks = ceil_div(L, PS_BWD_TT);
  ge.R = PS_THREADS / (C / 4);
  ge.block = ge.R * (C / 4);
  ge.units = (int64_t)B * ge.nchunks;
  ge.grid = ceil_div64(ge.units, ge.R);
  return ge;
}

}  // namespace

// ---- internal launchers (net_inception.hip): the pooled tensor z / its gradient dz is a column window of a wider tensor ----
// zp = row pitch of z / dz in floats (a multiple of 4, >= C; the pointer names the window's first column, 16-byte aligned).
// With zp = C these are the public entry points, bit for bit.
int kws_pool3s2_same_fwd_pitch(const float* y, const float* bn, float* z, int zp, int B, int L, int C, hipStream_t stream) {
  KWS_REQUIRE(y && bn && z && ps_ok(B, L, C) && zp >= C && zp % 4 == 0, "pool3s2_same_fwd: bad arguments (B=%d L=%d C=%d pitch=%d)", B,
              L, C, zp);
  const int Lp = kws_pool3s2_same_out_len(L);
  const int nchunks = ceil_div(Lp, PS_FWD_TT);
  const int64_t n_units = (int64_t)B * nchunks * (C / 4);
  KWS_REQUIRE(ceil_div64(n_units, PS_THREADS) < (1ll << 31), "pool3s2_same_fwd: tensor too large");
  KwsProfScope prof("pool3s2_same_fwd", 8.0 * B * L * C, 4.0 * ((double)B * L * C + (double)B * Lp * C), stream);
  hipLaunchKernelGGL(pool3s2_same_fwd_kernel, dim3((unsigned)ceil_div64(n_units, PS_THREADS)), dim3(PS_THREADS), 0, stream, y, bn, z,
                     n_units, L, Lp, C, nchunks, L & 1, zp);
  KWS_LAUNCH_CHECK("pool3s2_same_fwd_kernel");
  return KWS_OK;
}

int kws_pool3s2_same_bwd_pitch(const float* dz, int zp, const float* y, const float* bn, float* g, float* part, int B, int L, int C,
                               hipStream_t stream) {
  KWS_REQUIRE(dz && y && bn && g && part && ps_ok(B, L, C) && zp >= C && zp % 4 == 0,
              "pool3s2_same_bwd: bad arguments (B=%d L=%d C=%d pitch=%d)", B, L, C, zp);
  const PsGeom ge = ps_geom(B, L, C);
  KWS_REQUIRE(ge.grid < (1ll << 31), "pool3s2_same_bwd: tensor too large");
  const int Lp = kws_pool3s2_same_out_len(L);
  KwsProfScope prof("pool3s2_same_bwd", 14.0 * B * L * C, 4.0 * (2.0 * B * L * C + (double)B * Lp * C), stream);
  if (L & 1)
    hipLaunchKernelGGL(pool3s2_same_bwd_kernel<1>, dim3((unsigned)ge.grid), dim3((unsigned)ge.block), 0, stream, dz, y, bn, g, part,
                       ge.units, L, Lp, C, ge.nchunks, ge.R, zp);
  else
    hipLaunchKernelGGL(pool3s2_same_bwd_kernel<0>, dim3((unsigned)ge.grid), dim3((unsigned)ge.block), 0, stream, dz, y, bn, g, part,
                       ge.units, L, Lp, C, ge.nchunks, ge.R, zp);
  KWS_LAUNCH_CHECK("pool3s2_same_bwd_kernel");
  return KWS_OK;
}

extern "C" {

int kws_pool3s2_same_out_len(int L) { return L >= 1 ? (L + 1) / 2 : 0; }

int kws_pool3s2_same_fwd_f32(const float* y, const float* bn, float* z, int B, int L, int C, void* stream) {
  return kws_pool3s2_same_fwd_pitch(y, bn, z, C, B, L, C, (hipStream_t)stream);
}

int kws_pool3s2_same_bwd_part_rows(int B, int L, int C) { return ps_ok(B, L, C) ? (int)ps_geom(B, L, C).grid : 0; }

int64_t kws_pool3s2_same_bwd_part_floats(int B, int L, int C) { return (int64_t)kws_pool3s2_same_bwd_part_rows(B, L, C) * 2 * C; }

int kws_pool3s2_same_bwd_f32(const float* dz, const float* y, const float* bn, float* g, float* part, int B, int L, int C,
                             void* stream) {
  return kws_pool3s2_same_bwd_pitch(dz, C, y, bn, g, part, B, L, C, (hipStream_t)stream);
}

}  // extern "C"
