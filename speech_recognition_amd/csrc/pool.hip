// MaxPool1D(pool_size=3, strides=2) over relu6(bn(y)), forward and backward, in both of TensorFlow's paddings, where it follows
// Conv1D + BatchNormalization + relu6 directly (no residual join; resblock.hip's block_out3_* are the SAME-padded joins):
//   'valid'  kws_pool3s2_*       Lp = (L - 3) / 2 + 1  pad_left = 0      _reduce_conv of conv_1d_time_stacked / conv_1d_heavy
//                                                                        (model.py:271-277, 423-429), the inception stem
//   'same'   kws_pool3s2_same_*  Lp = (L + 1) / 2      pad_left = L & 1  conv_1d_multi_time_sliced (model.py:1093-1097), the
//                                                                        inception reduce blocks (pad_total = 2 (Lp - 1) + 3 - L)
// One kernel set runs both: window t covers the rows 2t - pad_left + j, j < 3, a row outside [0, L) holds -inf (TF pads with
// -inf) and the middle row of every window is a valid one, so padding never wins.  VALID never reaches such a row
// and instantiates the row loader without the test (PADDED = false).
//   fwd   z[b,t,c] = max_{j<3} relu6(scale[c] * y[b, 2t - pad_left + j, c] + shift[c]),  t < Lp
//         The activation comes BEFORE the maximum: a BatchNorm scale may be negative, so max(y) normalised is not the same.
//   bwd   gather form: g[b,u,c] = gate(u) * sum of dz[b,t,c] over the (at most two) windows t that u won, where the FIRST
//         maximum of a window wins (TF MaxPoolGrad) and gate = relu6'(bn(y[b,u,c])) = [0 < pre <= 6].  Every element of g
//         is written exactly once; a last row no window covers (VALID, even L) gets an exact 0.  In the same pass the
//         per-workgroup BatchNorm partial sums part[row][2][C] = (sum g, sum g * xhat) go out (part_rows.h), folded afterwards
//         in a fixed order (bncols.hip gbn_bwd_fin_kernel): no float atomics, bit-reproducible.
// Both are HBM-bound: one thread owns a float4 of channels and a short run of time steps (16-byte loads and stores), and a
// row shared by two windows is read from HBM once (the forward carries it in registers, the backward's re-reads hit L1/L2).
#include "common.h"
#include "internal.h"
#include "part_rows.h"

namespace {

using kws_part::gate;
using kws_part::ld4;

constexpr int PL_FWD_TT = 4;   // outputs per thread (forward): 2 * 4 + 1 input rows
constexpr int PL_BWD_TT = 8;   // input positions per thread (backward), even: a run starts at an even row
constexpr int PL_THREADS = kws_part::THREADS;

// activation of row r, or -inf for a row of the padding.  PADDED = false (VALID) skips the test: no window reaches such a row,
// and without it the loads of a run are issued together (measured: the tested loader costs the VALID calls 2 - 20 %)
template <bool PADDED>
__device__ __forceinline__ float4 pl_act(const float* yb, int r, int L, int C, const float4 sc, const float4 sh) {
  if (PADDED && (r < 0 || r >= L)) return make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
  const float4 v = ld4(yb + (int64_t)r * C);
  return make_float4(relu6f(fmaf(v.x, sc.x, sh.x)), relu6f(fmaf(v.y, sc.y, sh.y)), relu6f(fmaf(v.z, sc.z, sh.z)),
                     relu6f(fmaf(v.w, sc.w, sh.w)));
}
__device__ __forceinline__ float pl_max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

template <bool PADDED>
__global__ __launch_bounds__(PL_THREADS) void pool3s2_fwd_kernel(const float* __restrict__ y, const float* __restrict__ bn,
                                                                 float* __restrict__ z, int64_t n_units, int L, int Lp, int C,
                                                                 int nchunks, int pl, int zp) {
  const int64_t i = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x;
  if (i >= n_units) return;
  const int C4 = C >> 2;
  const int c = (int)(i % C4) * 4;
  const int64_t unit = i / C4;
  const int64_t b = unit / nchunks;
  const int t0 = (int)(unit - b * nchunks) * PL_FWD_TT;
  const float4 sc = ld4(bn + c), sh = ld4(bn + C + c);
  const float* yb = y + b * L * (int64_t)C + c;
  float* zb = z + b * Lp * (int64_t)zp + c;   // zp: row pitch of z (C for the public entry points)
  float4 a0 = pl_act<PADDED>(yb, 2 * t0 - pl, L, C, sc, sh);
#pragma unroll
  for (int k = 0; k < PL_FWD_TT; ++k) {
    const int t = t0 + k;
    if (t >= Lp) break;
    const int r = 2 * t - pl;   // rows r, r + 1, r + 2; r + 1 <= L - 1 for every t < Lp
    const float4 a1 = pl_act<PADDED>(yb, r + 1, L, C, sc, sh), a2 = pl_act<PADDED>(yb, r + 2, L, C, sc, sh);
    *reinterpret_cast<float4*>(zb + (int64_t)t * zp) =
        make_float4(pl_max3(a0.x, a1.x, a2.x), pl_max3(a0.y, a1.y, a2.y), pl_max3(a0.z, a1.z, a2.z), pl_max3(a0.w, a1.w, a2.w));
    a0 = a2;
  }
}

// offset (0..2) of the first maximum of a window (resblock.hip first_max3); a padding row holds -inf: it never wins
__device__ __forceinline__ int pl_first_max3(float a0, float a1, float a2) {
  int j = 0;
  float m = a0;
  if (a1 > m) { m = a1; j = 1; }
  if (a2 > m) j = 2;
  return j;
}

// One thread: float4 of channels x the PL_BWD_TT input rows u0 .. u0 + 7 (u0 even).  PL = pad_left.  The windows that can hand
// a gradient to those rows are t = u0 / 2 - 1 + PL + w, w = 0 .. 4 (rows u0 - 2 + PL + 2w .. u0 + PL + 2w); window w's element j
// is run position 2w - 2 + PL + j.  A row no window t < Lp reaches (the last one of an even-L VALID input) keeps acc = 0:
// it is written, as an exact zero.
template <int PL, bool PADDED>
__global__ __launch_bounds__(PL_THREADS) void pool3s2_bwd_kernel(const float* __restrict__ dz, const float* __restrict__ y,
                                                                 const float* __restrict__ bn, float* __restrict__ g,
                                                                 float* __restrict__ part, int64_t units, int L, int Lp, int C,
                                                                 int nchunks, int R, int zp) {
  const int C4 = C >> 2;
  const int tid = threadIdx.x;
  const int r = tid / C4, c4 = tid - r * C4;
  const int c = c4 * 4;
  const int64_t unit = (int64_t)blockIdx.x * R + r;
  float4 sg = make_float4(0.f, 0.f, 0.f, 0.f), sgx = sg;
  if (unit < units) {
    const int64_t b = unit / nchunks;
    const int u0 = (int)(unit - b * nchunks) * PL_BWD_TT;
    const float4 sc = ld4(bn + c), sh = ld4(bn + C + c), mean = ld4(bn + 2 * C + c), rstd = ld4(bn + 3 * C + c);
    const float* yb = y + b * L * (int64_t)C + c;
    const float* dzb = dz + b * Lp * (int64_t)zp + c;   // zp: row pitch of dz
    float4 acc[PL_BWD_TT];
#pragma unroll
    for (int i = 0; i < PL_BWD_TT; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    const int tb = u0 / 2 - 1 + PL;
    float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f);
    bool have0 = false;   // a0 = activation of the first row of the next window (the last row of the one before it)
#pragma unroll
    for (int w = 0; w <= PL_BWD_TT / 2; ++w) {
      const int t = tb + w;
      if (t < 0 || t >= Lp) {
        have0 = false;
        continue;
      }
      const int r0 = 2 * t - PL;
      if (!have0) a0 = pl_act<PADDED>(yb, r0, L, C, sc, sh);
      const float4 a1 = pl_act<PADDED>(yb, r0 + 1, L, C, sc, sh), a2 = pl_act<PADDED>(yb, r0 + 2, L, C, sc, sh);
      const float4 d = ld4(dzb + (int64_t)t * zp);
#define KWS_POOL_ROUTE(f)                                                                               \
  do {                                                                                                  \
    const int j = pl_first_max3(a0.f, a1.f, a2.f);                                                      \
    if (2 * w - 2 + PL >= 0 && 2 * w - 2 + PL < PL_BWD_TT && j == 0)                                    \
      acc[(2 * w - 2 + PL >= 0 && 2 * w - 2 + PL < PL_BWD_TT) ? 2 * w - 2 + PL : 0].f += d.f;           \
    if (2 * w - 1 + PL >= 0 && 2 * w - 1 + PL < PL_BWD_TT && j == 1)                                    \
      acc[(2 * w - 1 + PL >= 0 && 2 * w - 1 + PL < PL_BWD_TT) ? 2 * w - 1 + PL : 0].f += d.f;           \
    if (2 * w + PL < PL_BWD_TT && j == 2) acc[(2 * w + PL < PL_BWD_TT) ? 2 * w + PL : 0].f += d.f;      \
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
      const float4 yu = ld4(yb + (int64_t)u * C);
      const float4 g0 = make_float4(acc[i].x * gate(fmaf(yu.x, sc.x, sh.x)), acc[i].y * gate(fmaf(yu.y, sc.y, sh.y)),
                                    acc[i].z * gate(fmaf(yu.z, sc.z, sh.z)), acc[i].w * gate(fmaf(yu.w, sc.w, sh.w)));
      *reinterpret_cast<float4*>(g + (b * L + u) * (int64_t)C + c) = g0;
      KWS_PART_ACCUMULATE(sg, sgx, g0, yu, mean, rstd);
    }
  }
  kws_part::fold_runs(sg, sgx, part, C, R);
}

// ---- host side: one geometry, one check, one launcher per direction ----
struct PoolPad {
  int Lp, pad_left;
  bool padded;   // some window reaches a row outside [0, L)
};
PoolPad pl_valid(int L) { return {kws_pool3s2_out_len(L), 0, false}; }
PoolPad pl_same(int L) { return {kws_pool3s2_same_out_len(L), L & 1, true}; }
constexpr int PL_VALID_MINL = 3, PL_SAME_MINL = 2;

bool pl_ok(int B, int L, int C, int min_L) { return B > 0 && L >= min_L && kws_part::channels_ok(C); }
// backward: one unit = a run of PL_BWD_TT input rows of one clip
int pl_chunks(int L) { return ceil_div(L, PL_BWD_TT); }
kws_part::Geom pl_geom(int B, int L, int C) { return kws_part::geom((int64_t)B * pl_chunks(L), C); }
int pl_part_rows(int B, int L, int C, int min_L) { return pl_ok(B, L, C, min_L) ? (int)pl_geom(B, L, C).grid : 0; }

// `name` = the profiler family and the prefix of every message; zp = row pitch of z / dz in floats
int pl_fwd(const char* name, PoolPad pp, int min_L, const float* y, const float* bn, float* z, int zp, int B, int L, int C,
           hipStream_t stream) {
  KWS_REQUIRE(y && bn && z && pl_ok(B, L, C, min_L) && zp >= C && zp % 4 == 0, "%s: bad arguments (B=%d L=%d C=%d pitch=%d)", name, B,
              L, C, zp);
  const int nchunks = ceil_div(pp.Lp, PL_FWD_TT);
  const int64_t n_units = (int64_t)B * nchunks * (C / 4);
  KWS_REQUIRE(ceil_div64(n_units, PL_THREADS) < (1ll << 31), "%s: tensor too large", name);
  KwsProfScope prof(name, 8.0 * B * L * C, 4.0 * ((double)B * L * C + (double)B * pp.Lp * C), stream);
  const auto kernel = pp.padded ? pool3s2_fwd_kernel<true> : pool3s2_fwd_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)ceil_div64(n_units, PL_THREADS)), dim3(PL_THREADS), 0, stream, y, bn, z, n_units, L, pp.Lp,
                     C, nchunks, pp.pad_left, zp);
  KWS_LAUNCH_CHECK("pool3s2_fwd_kernel");
  return KWS_OK;
}

int pl_bwd(const char* name, PoolPad pp, int min_L, const float* dz, int zp, const float* y, const float* bn, float* g, float* part,
           int B, int L, int C, hipStream_t stream) {
  KWS_REQUIRE(dz && y && bn && g && part && pl_ok(B, L, C, min_L) && zp >= C && zp % 4 == 0,
              "%s: bad arguments (B=%d L=%d C=%d pitch=%d)", name, B, L, C, zp);
  const kws_part::Geom ge = pl_geom(B, L, C);
  KWS_REQUIRE(ge.grid < (1ll << 31), "%s: tensor too large", name);
  const int nchunks = pl_chunks(L);
  KwsProfScope prof(name, 14.0 * B * L * C, 4.0 * (2.0 * B * L * C + (double)B * pp.Lp * C), stream);
  const auto kernel = !pp.padded    ? pool3s2_bwd_kernel<0, false>   // VALID: pad_left = 0
                      : pp.pad_left ? pool3s2_bwd_kernel<1, true>
                                    : pool3s2_bwd_kernel<0, true>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)ge.grid), dim3((unsigned)ge.block), 0, stream, dz, y, bn, g, part, (int64_t)B * nchunks, L,
                     pp.Lp, C, nchunks, ge.R, zp);
  KWS_LAUNCH_CHECK("pool3s2_bwd_kernel");
  return KWS_OK;
}

}  // namespace

// ---- internal launchers (net_inception.hip): the pooled tensor z / its gradient dz is a column window of a wider tensor ----
// zp = row pitch of z / dz in floats (a multiple of 4, >= C; the pointer names the window's first column, 16-byte aligned).
// With zp = C these are the public entry points, bit for bit.
int kws_pool3s2_same_fwd_pitch(const float* y, const float* bn, float* z, int zp, int B, int L, int C, hipStream_t stream) {
  return pl_fwd("pool3s2_same_fwd", pl_same(L), PL_SAME_MINL, y, bn, z, zp, B, L, C, stream);
}

int kws_pool3s2_same_bwd_pitch(const float* dz, int zp, const float* y, const float* bn, float* g, float* part, int B, int L, int C,
                               hipStream_t stream) {
  return pl_bwd("pool3s2_same_bwd", pl_same(L), PL_SAME_MINL, dz, zp, y, bn, g, part, B, L, C, stream);
}

extern "C" {

int kws_pool3s2_out_len(int L) { return L >= 3 ? (L - 3) / 2 + 1 : 0; }
int kws_pool3s2_same_out_len(int L) { return L >= 1 ? (L + 1) / 2 : 0; }

int kws_pool3s2_fwd_f32(const float* y, const float* bn, float* z, int B, int L, int C, void* stream) {
  return pl_fwd("pool3s2_fwd", pl_valid(L), PL_VALID_MINL, y, bn, z, C, B, L, C, (hipStream_t)stream);
}
int kws_pool3s2_same_fwd_f32(const float* y, const float* bn, float* z, int B, int L, int C, void* stream) {
  return kws_pool3s2_same_fwd_pitch(y, bn, z, C, B, L, C, (hipStream_t)stream);
}

int kws_pool3s2_bwd_part_rows(int B, int L, int C) { return pl_part_rows(B, L, C, PL_VALID_MINL); }
int kws_pool3s2_same_bwd_part_rows(int B, int L, int C) { return pl_part_rows(B, L, C, PL_SAME_MINL); }
int64_t kws_pool3s2_bwd_part_floats(int B, int L, int C) { return (int64_t)kws_pool3s2_bwd_part_rows(B, L, C) * 2 * C; }
int64_t kws_pool3s2_same_bwd_part_floats(int B, int L, int C) { return (int64_t)kws_pool3s2_same_bwd_part_rows(B, L, C) * 2 * C; }

int kws_pool3s2_bwd_f32(const float* dz, const float* y, const float* bn, float* g, float* part, int B, int L, int C,
                        void* stream) {
  return pl_bwd("pool3s2_bwd", pl_valid(L), PL_VALID_MINL, dz, C, y, bn, g, part, B, L, C, (hipStream_t)stream);
}
int kws_pool3s2_same_bwd_f32(const float* dz, const float* y, const float* bn, float* g, float* part, int B, int L, int C,
                             void* stream) {
  return kws_pool3s2_same_bwd_pitch(dz, C, y, bn, g, part, B, L, C, (hipStream_t)stream);
}

}  // extern "C"
