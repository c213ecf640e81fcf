// MaxPool1D(pool_size=3, strides=2, padding='valid') over relu6(bn(y)), forward and backward: the pool of the reference's
// _reduce_conv in conv_1d_time_stacked_model / conv_1d_heavy_model (model.py:271-277, 423-429), where it follows
// Conv1D + BatchNormalization + relu6 directly (no residual join; resblock.hip's block_out3_* are the SAME-padded joins).
//   fwd   z[b,t,c] = max_{j<3} relu6(scale[c] * y[b, 2t+j, c] + shift[c]),  t < Lp = (L - 3) / 2 + 1
//         The activation comes BEFORE the maximum: a BatchNorm scale may be negative, so max(y) normalised is not the same.
//   bwd   gather form: g[b,u,c] = gate(u) * sum of dz[b,t,c] over the (at most two) windows t that u won, where the FIRST
//         maximum of a window wins (TF MaxPoolGrad) and gate = relu6'(bn(y[b,u,c])) = [0 < pre <= 6].  Every element of g
//         is written exactly once; a last row no window covers (even L) gets an exact 0.  In the same pass the per-workgroup
//         BatchNorm partial sums part[row][2][C] = (sum g, sum g * xhat) go out, folded afterwards in a fixed order
//         (bncols.hip gbn_bwd_fin_kernel): no float atomics, bit-reproducible.
// Both are HBM-bound: one thread owns a float4 of channels and a short run of time steps (16-byte loads and stores), and a
// row shared by two windows is read from HBM once (the forward carries it in registers, the backward's re-reads hit L1/L2).
#include "common.h"
#include "internal.h"

namespace {

constexpr int PL_FWD_TT = 4;   // outputs per thread (forward): 2 * 4 + 1 input rows
constexpr int PL_BWD_TT = 8;   // input positions per thread (backward), even: a run starts at an even row
constexpr int PL_THREADS = 256;
constexpr int PL_MAXC = 1024;  // C / 4 threads of one time run fit one workgroup

__device__ __forceinline__ float4 pl_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 pl_act(const float* p, const float4 sc, const float4 sh) {
  const float4 v = pl_ld4(p);
  return make_float4(relu6f(fmaf(v.x, sc.x, sh.x)), relu6f(fmaf(v.y, sc.y, sh.y)), relu6f(fmaf(v.z, sc.z, sh.z)),
                     relu6f(fmaf(v.w, sc.w, sh.w)));
}
__device__ __forceinline__ float pl_max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

__global__ __launch_bounds__(PL_THREADS) void pool3s2_fwd_kernel(const float* __restrict__ y, const float* __restrict__ bn,
                                                                 float* __restrict__ z, int64_t n_units, int L, int Lp, int C,
                                                                 int nchunks) {
  const int64_t i = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x;
  if (i >= n_units) return;
  const int C4 = C >> 2;
  const int c = (int)(i % C4) * 4;
  const int64_t unit = i / C4;
  const int64_t b = unit / nchunks;
  const int t0 = (int)(unit - b * nchunks) * PL_FWD_TT;
  const float4 sc = pl_ld4(bn + c), sh = pl_ld4(bn + C + c);
  const float* yb = y + b * L * (int64_t)C + c;
  float* zb = z + b * Lp * (int64_t)C + c;
  float4 a0 = pl_act(yb + (int64_t)(2 * t0) * C, sc, sh);   // t0 < Lp: rows 2 t0 .. 2 t0 + 2 <= 2 Lp <= L - 1
#pragma unroll
  for (int k = 0; k < PL_FWD_TT; ++k) {
    const int t = t0 + k;
    if (t >= Lp) break;
    const float4 a1 = pl_act(yb + (int64_t)(2 * t + 1) * C, sc, sh), a2 = pl_act(yb + (int64_t)(2 * t + 2) * C, sc, sh);
    *reinterpret_cast<float4*>(zb + (int64_t)t * C) =
        make_float4(pl_max3(a0.x, a1.x, a2.x), pl_max3(a0.y, a1.y, a2.y), pl_max3(a0.z, a1.z, a2.z), pl_max3(a0.w, a1.w, a2.w));
    a0 = a2;
  }
}

// offset (0..2) of the first maximum of a window (resblock.hip first_max3)
__device__ __forceinline__ int pl_first_max3(float a0, float a1, float a2) {
  int j = 0;
  float m = a0;
  if (a1 > m) { m = a1; j = 1; }
  if (a2 > m) j = 2;
  return j;
}
__device__ __forceinline__ float pl_gate(float pre) { return (pre > 0.f && pre <= 6.f) ? 1.f : 0.f; }

// One thread: float4 of channels x the PL_BWD_TT input rows u0 .. u0 + 7 (u0 even).  The windows that can hand a gradient to
// those rows are t = u0 / 2 - 1 + w, w = 0 .. 4 (rows u0 - 2 + 2w .. u0 + 2w); window w's element j is run position 2w - 2 + j.
__global__ __launch_bounds__(PL_THREADS) void pool3s2_bwd_kernel(const float* __restrict__ dz, const float* __restrict__ y,
                                                                 const float* __restrict__ bn, float* __restrict__ g,
                                                                 float* __restrict__ part, int64_t units, int L, int Lp, int C,
                                                                 int nchunks, int R) {
  __shared__ float red[2][PL_THREADS * 4];
  const int C4 = C >> 2;
  const int tid = threadIdx.x;
  const int r = tid / C4, c4 = tid - r * C4;
  const int c = c4 * 4;
  const int64_t unit = (int64_t)blockIdx.x * R + r;
  float4 sg = make_float4(0.f, 0.f, 0.f, 0.f), sgx = sg;
  if (unit < units) {
    const int64_t b = unit / nchunks;
    const int u0 = (int)(unit - b * nchunks) * PL_BWD_TT;
    const float4 sc = pl_ld4(bn + c), sh = pl_ld4(bn + C + c), mean = pl_ld4(bn + 2 * C + c), rstd = pl_ld4(bn + 3 * C + c);
    const float* yb = y + b * L * (int64_t)C + c;
    const float* dzb = dz + b * Lp * (int64_t)C + c;
    float4 acc[PL_BWD_TT];
#pragma unroll
    for (int i = 0; i < PL_BWD_TT; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    const int tb = u0 / 2 - 1;
    float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f);
    bool have0 = false;   // a0 = activation of the first row of the next window (the last row of the one before it)
#pragma unroll
    for (int w = 0; w <= PL_BWD_TT / 2; ++w) {
      const int t = tb + w;
      if (t < 0 || t >= Lp) {
        have0 = false;
        continue;
      }
      if (!have0) a0 = pl_act(yb + (int64_t)(2 * t) * C, sc, sh);
      const float4 a1 = pl_act(yb + (int64_t)(2 * t + 1) * C, sc, sh), a2 = pl_act(yb + (int64_t)(2 * t + 2) * C, sc, sh);
      const float4 d = pl_ld4(dzb + (int64_t)t * C);
#define KWS_POOL_ROUTE(f)                                   \
  do {                                                      \
    const int j = pl_first_max3(a0.f, a1.f, a2.f);          \
    if (w >= 1 && j == 0) acc[w >= 1 ? 2 * w - 2 : 0].f += d.f; \
    if (w >= 1 && j == 1) acc[w >= 1 ? 2 * w - 1 : 0].f += d.f; \
    if (w < PL_BWD_TT / 2 && j == 2) acc[w < PL_BWD_TT / 2 ? 2 * w : 0].f += d.f; \
  } while (0)
      KWS_POOL_ROUTE(x);
      KWS_POOL_ROUTE(y);
      KWS_POOL_ROUTE(z);
      KWS_POOL_ROUTE(w);
#undef KWS_POOL_ROUTE
      a0 = a2;
      have0 = true;
    }
#pragma unroll
    for (int i = 0; i < PL_BWD_TT; ++i) {
      const int u = u0 + i;
      if (u >= L) break;
      const float4 yu = pl_ld4(yb + (int64_t)u * C);
      const float4 g0 = make_float4(acc[i].x * pl_gate(fmaf(yu.x, sc.x, sh.x)), acc[i].y * pl_gate(fmaf(yu.y, sc.y, sh.y)),
                                    acc[i].z * pl_gate(fmaf(yu.z, sc.z, sh.z)), acc[i].w * pl_gate(fmaf(yu.w, sc.w, sh.w)));
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

bool pl_ok(int B, int L, int C) { return B > 0 && L >= 3 && C > 0 && C % 4 == 0 && C <= PL_MAXC; }
struct PlGeom {
  int nchunks, R, block;
  int64_t units, grid;
};
PlGeom pl_geom(int B, int L, int C) {
  PlGeom ge;
  ge.nchunks = ceil_div(L, PL_BWD_TT);
  ge.R = PL_THREADS / (C / 4);
  ge.block = ge.R * (C / 4);
  ge.units = (int64_t)B * ge.nchunks;
  ge.grid = ceil_div64(ge.units, ge.R);
  return ge;
}

}  // namespace

extern "C" {

int kws_pool3s2_out_len(int L) { return L >= 3 ? (L - 3) / 2 + 1 : 0; }

int kws_pool3s2_fwd_f32(const float* y, const float* bn, float* z, int B, int L, int C, void* stream) {
  KWS_REQUIRE(y && bn && z && pl_ok(B, L, C), "pool3s2_fwd: bad arguments (B=%d L=%d C=%d)", B, L, C);
  const int Lp = kws_pool3s2_out_len(L);
  const int nchunks = ceil_div(Lp, PL_FWD_TT);
  const int64_t n_units = (int64_t)B * nchunks * (C / 4);
  KWS_REQUIRE(ceil_div64(n_units, PL_THREADS) < (1ll << 31), "pool3s2_fwd: tensor too large");
  KwsProfScope prof("pool3s2_fwd", 8.0 * B * L * C, 4.0 * ((double)B * L * C + (double)B * Lp * C), (hipStream_t)stream);
  hipLaunchKernelGGL(pool3s2_fwd_kernel, dim3((unsigned)ceil_div64(n_units, PL_THREADS)), dim3(PL_THREADS), 0, (hipStream_t)stream,
                     y, bn, z, n_units, L, Lp, C, nchunks);
  KWS_LAUNCH_CHECK("pool3s2_fwd_kernel");
  return KWS_OK;
}

int kws_pool3s2_bwd_part_rows(int B, int L, int C) { return pl_ok(B, L, C) ? (int)pl_geom(B, L, C).grid : 0; }

int64_t kws_pool3s2_bwd_part_floats(int B, int L, int C) { return (int64_t)kws_pool3s2_bwd_part_rows(B, L, C) * 2 * C; }

int kws_pool3s2_bwd_f32(const float* dz, const float* y, const float* bn, float* g, float* part, int B, int L, int C,
                        void* stream) {
  KWS_REQUIRE(dz && y && bn && g && part && pl_ok(B, L, C), "pool3s2_bwd: bad arguments (B=%d L=%d C=%d)", B, L, C);
  const PlGeom ge = pl_geom(B, L, C);
  KWS_REQUIRE(ge.grid < (1ll << 31), "pool3s2_bwd: tensor too large");
  const int Lp = kws_pool3s2_out_len(L);
  KwsProfScope prof("pool3s2_bwd", 14.0 * B * L * C, 4.0 * (2.0 * B * L * C + (double)B * Lp * C), (hipStream_t)stream);
  hipLaunchKernelGGL(pool3s2_bwd_kernel, dim3((unsigned)ge.grid), dim3((unsigned)ge.block), 0, (hipStream_t)stream, dz, y, bn, g,
                     part, ge.units, L, Lp, C, ge.nchunks, ge.R);
  KWS_LAUNCH_CHECK("pool3s2_bwd_kernel");
  return KWS_OK;
}

}  // extern "C"
