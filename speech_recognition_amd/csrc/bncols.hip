// BatchNorm bookkeeping of the network programs over the columns of a [M, .] matrix of convolution outputs (net_grouped.hip,
// net_dwk.hip, net_mts.hip, net_inception.hip): statistics rows -> tables and moving statistics, inference tables, and the three
// passes of the backward of Activation(relu6) o BatchNormalization.  One kernel set for the two layouts of kws_gbn_cols
// (internal.h): g groups of Ng dense columns with per-group tables bn[g][4][Ng], or one group that is the column window
// [c0, c0 + Ng) of a tensor of row pitch `pitch`, filling its columns of that tensor's table bn[4][pitch].  With g = 1,
// pitch = Ng, c0 = 0 the two are the same thing.
#include "internal.h"

namespace {

constexpr int GFIN_CG = 16, GFIN_RG = 16;   // the 16 x 16 double reduction of the two fin kernels
constexpr int GBWD_ROWS = 64;               // rows per partial-sum chunk of the backward's pass 1

struct Cols {
  int g, Ng;
  int pitch, c0;   // WIN: column c of row m is element m * pitch + c0 + c
};
struct GbnRefs {
  const float* gamma;   // group 0's gamma; group q's at + q * pstride; beta at + boff
  int64_t pstride, boff;
  float* mm;            // group 0's moving mean; group q's at + q * sstride; moving variance at + voff
  int64_t sstride, voff;
};

// Everything the two layouts differ in.  WIN is a template argument of every kernel, not a run-time branch: the kernels are short,
// and a training step measured 0.2 - 0.4 % slower with one run-time form of this arithmetic (profiles/bn_cols_step_times.json).
//   column c -> its group, its column inside the group, its scale entry in the table (shift, mean, rstd follow ts floats apart)
struct Col {
  int grp, n, ts;
  int64_t t;
};
template <bool WIN>
__device__ __forceinline__ Col col_of(const Cols& w, int c) {
  if (WIN) return Col{0, c, w.pitch, (int64_t)w.c0 + c};
  const int grp = c / w.Ng, n = c - grp * w.Ng;
  return Col{grp, n, w.Ng, (int64_t)grp * 4 * w.Ng + n};
}
//   element (row m, column c) of the data
template <bool WIN>
__device__ __forceinline__ int64_t elem_of(const Cols& w, int F, int64_t m, int c) {
  return WIN ? m * w.pitch + w.c0 + c : m * F + c;
}

// part[rows][2][F] -> tables (scale|shift|mean|rstd) and the moving statistics; the arithmetic of bn_stats_finalize_kernel
// (bn.hip): double sums over the rows in a fixed order, biased variance, AssignMovingAvg (r.mm NULL: no update)
template <bool WIN>
__global__ __launch_bounds__(256) void gbn_finalize_kernel(const float* __restrict__ part, int rows, double inv_count, GbnRefs r,
                                                           float eps, float omm, float* __restrict__ bn, Cols w) {
  __shared__ double red[2][GFIN_RG][GFIN_CG];
  const int F = w.g * w.Ng;
  const int cg = threadIdx.x % GFIN_CG, rg = threadIdx.x / GFIN_CG;
  const int c = blockIdx.x * GFIN_CG + cg;
  double s = 0.0, ss = 0.0;
  if (c < F)
    for (int t = rg; t < rows; t += GFIN_RG) {
      s += (double)part[(int64_t)t * 2 * F + c];
      ss += (double)part[(int64_t)t * 2 * F + F + c];
    }
  red[0][rg][cg] = s;
  red[1][rg][cg] = ss;
  __syncthreads();
  if (rg != 0 || c >= F) return;
  s = 0.0;
  ss = 0.0;
  for (int q = 0; q < GFIN_RG; ++q) {
    s += red[0][q][cg];
    ss += red[1][q][cg];
  }
  const Col k = col_of<WIN>(w, c);
  const int n = k.n;
  const double mean = s * inv_count;
  double var = ss * inv_count - mean * mean;
  if (var < 0.0) var = 0.0;
  const float rstd = (float)(1.0 / sqrt(var + (double)eps));
  const float meanf = (float)mean, varf = (float)var;
  const float* ga = r.gamma + (int64_t)k.grp * r.pstride;
  const float scale = ga[n] * rstd;
  float* t = bn + k.t;
  t[0] = scale;
  t[k.ts] = ga[r.boff + n] - meanf * scale;
  t[2 * k.ts] = meanf;
  t[3 * k.ts] = rstd;
  if (r.mm) {
    float* mm = r.mm + (int64_t)k.grp * r.sstride;
    mm[n] = mm[n] - (mm[n] - meanf) * omm;
    mm[r.voff + n] = mm[r.voff + n] - (mm[r.voff + n] - varf) * omm;
  }
}

// inference tables from the moving statistics (bn_infer_prepare_kernel's arithmetic)
template <bool WIN>
__global__ __launch_bounds__(256) void gbn_infer_kernel(GbnRefs r, float eps, float* __restrict__ bn, Cols w) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= w.g * w.Ng) return;
  const Col k = col_of<WIN>(w, c);
  const int n = k.n;
  const float* ga = r.gamma + (int64_t)k.grp * r.pstride;
  const float* mm = r.mm + (int64_t)k.grp * r.sstride;
  const float rstd = 1.0f / sqrtf(mm[r.voff + n] + eps);
  const float scale = ga[n] * rstd;
  float* t = bn + k.t;
  t[0] = scale;
  t[k.ts] = ga[r.boff + n] - mm[n] * scale;
  t[2 * k.ts] = mm[n];
  t[3 * k.ts] = rstd;
}

// backward of Activation(relu6) o BatchNormalization, pass 1: g = dA * relu6'(bn(y)) (+ add: an already gated contribution) in
// place, per-chunk partial sums part[chunk][2][F] of (g, g * xhat); rows of one chunk are added in ascending order.  ADD: `add`
// is there (a template argument: the compiler leaves a run-time test of the pointer inside the row loop)
template <bool WIN, bool ADD>
__global__ __launch_bounds__(256) void gbn_bwd_part_kernel(float* __restrict__ dA, const float* __restrict__ y, const float* __restrict__ bn,
                                                           const float* __restrict__ add, int64_t M, Cols w, float* __restrict__ part) {
  const int F = w.g * w.Ng;
  const int c = blockIdx.y * 256 + threadIdx.x;
  if (c >= F) return;
  const Col k = col_of<WIN>(w, c);
  const float* t = bn + k.t;
  const float sc = t[0], sh = t[k.ts], mean = t[2 * k.ts], rstd = t[3 * k.ts];
  const int64_t m0 = (int64_t)blockIdx.x * GBWD_ROWS;
  const int64_t m1 = m0 + GBWD_ROWS < M ? m0 + GBWD_ROWS : M;
  float s = 0.f, sx = 0.f;
  for (int64_t m = m0; m < m1; ++m) {
    const int64_t i = elem_of<WIN>(w, F, m, c);
    const float yv = y[i];
    const float pre = fmaf(yv, sc, sh);
    float gv = (pre > 0.f && pre <= 6.f) ? dA[i] : 0.f;
    if (ADD) gv += add[i];
    dA[i] = gv;
    s += gv;
    sx += gv * ((yv - mean) * rstd);
  }
  part[(int64_t)blockIdx.x * 2 * F + c] = s;
  part[(int64_t)blockIdx.x * 2 * F + F + c] = sx;
}

// pass 2: dbeta, dgamma (into the flat gradient buffer at the groups' offsets) and coef[2][F] = (sum g / n, sum g xhat / n)
template <bool WIN>
__global__ __launch_bounds__(256) void gbn_bwd_fin_kernel(const float* __restrict__ part, int rows, double inv_count, Cols w,
                                                          float* dgamma0, int64_t pstride, int64_t boff, float* __restrict__ coef) {
  __shared__ double red[2][GFIN_RG][GFIN_CG];
  const int F = w.g * w.Ng;
  const int cg = threadIdx.x % GFIN_CG, rg = threadIdx.x / GFIN_CG;
  const int c = blockIdx.x * GFIN_CG + cg;
  double s = 0.0, sx = 0.0;
  if (c < F)
    for (int t = rg; t < rows; t += GFIN_RG) {
      s += (double)part[(int64_t)t * 2 * F + c];
      sx += (double)part[(int64_t)t * 2 * F + F + c];
    }
  red[0][rg][cg] = s;
  red[1][rg][cg] = sx;
  __syncthreads();
  if (rg != 0 || c >= F) return;
  s = 0.0;
  sx = 0.0;
  for (int q = 0; q < GFIN_RG; ++q) {
    s += red[0][q][cg];
    sx += red[1][q][cg];
  }
  const Col k = col_of<WIN>(w, c);
  float* dg = dgamma0 + (int64_t)k.grp * pstride;
  dg[k.n] = (float)sx;
  dg[boff + k.n] = (float)s;
  coef[c] = (float)(s * inv_count);
  coef[F + c] = (float)(sx * inv_count);
}

// pass 3: dy = scale * (g - c1 - xhat * c2), in place (bn_bwd_apply_kernel's arithmetic with gamma * rstd = scale), one element per
// thread; element e of a dense matrix is e itself
template <bool WIN>
__global__ __launch_bounds__(256) void gbn_bwd_apply_kernel(float* __restrict__ gbuf, const float* __restrict__ y, const float* __restrict__ bn,
                                                            const float* __restrict__ coef, int64_t n_el, Cols w) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_el) return;
  const int F = w.g * w.Ng;
  int c;
  int64_t i;
  if (WIN) {
    const int64_t m = e / F;
    c = (int)(e - m * F);
    i = elem_of<true>(w, F, m, c);
  } else {
    c = (int)(e % F);
    i = e;
  }
  const Col k = col_of<WIN>(w, c);
  const float* t = bn + k.t;
  const float mean = t[2 * k.ts], rstd = t[3 * k.ts];
  gbuf[i] = t[0] * (gbuf[i] - coef[c] - (y[i] - mean) * rstd * coef[F + c]);
}

// a window of a wider tensor is one group: several groups in a window would need a table layout nobody has defined
int cols_of(const kws_gbn_cols* c, const char* who, Cols* w, bool* window) {
  KWS_REQUIRE(c != nullptr && c->g > 0 && c->Ng > 0 && c->c0 >= 0 && (int64_t)c->c0 + (int64_t)c->g * c->Ng <= c->pitch,
              "%s: g=%d Ng=%d c0=%d do not fit the row pitch %d", who, c ? c->g : 0, c ? c->Ng : 0, c ? c->c0 : 0, c ? c->pitch : 0);
  *window = c->pitch != c->g * c->Ng || c->c0 != 0;
  KWS_REQUIRE(!*window || c->g == 1, "%s: a column window (pitch %d, first column %d) of %d groups has no table layout", who, c->pitch,
              c->c0, c->g);
  *w = Cols{c->g, c->Ng, c->pitch, c->c0};
  return KWS_OK;
}

int bwd_finish_launch(float* gbuf, const float* y, const float* bn, int64_t M, const Cols& w, bool window, const float* part, int rows,
                      float* coef, float* dgamma0, int64_t pstride, int64_t boff, hipStream_t st) {
  const int F = w.g * w.Ng;
  hipLaunchKernelGGL(window ? gbn_bwd_fin_kernel<true> : gbn_bwd_fin_kernel<false>, dim3((unsigned)ceil_div(F, GFIN_CG)), dim3(256), 0, st,
                     part, rows, 1.0 / (double)M, w, dgamma0, pstride, boff, coef);
  KWS_LAUNCH_CHECK("gbn_bwd_fin_kernel");
  const int64_t n_el = M * F;
  hipLaunchKernelGGL(window ? gbn_bwd_apply_kernel<true> : gbn_bwd_apply_kernel<false>, dim3((unsigned)ceil_div64(n_el, 256)), dim3(256),
                     0, st, gbuf, y, bn, coef, n_el, w);
  KWS_LAUNCH_CHECK("gbn_bwd_apply_kernel");
  return KWS_OK;
}

}  // namespace

int kws_gbn_finalize(const float* part, int rows, int64_t count, const kws_gbn_cols* c, const kws_gbn_refs* r, float eps, float momentum,
                     float* bn, hipStream_t st) {
  Cols w;
  bool window;
  KWS_TRY(cols_of(c, "gbn_finalize", &w, &window));
  const int F = w.g * w.Ng;
  GbnRefs g{r->gamma, r->pstride, r->boff, r->mm, r->sstride, r->voff};
  KwsProfScope prof("gbn_finalize", 0.0, 8.0 * rows * F, st);
  hipLaunchKernelGGL(window ? gbn_finalize_kernel<true> : gbn_finalize_kernel<false>, dim3((unsigned)ceil_div(F, GFIN_CG)), dim3(256), 0,
                     st, part, rows, 1.0 / (double)count, g, eps, (float)(1.0 - (double)momentum), bn, w);
  KWS_LAUNCH_CHECK("gbn_finalize_kernel");
  return KWS_OK;
}

int kws_gbn_infer(const kws_gbn_cols* c, const kws_gbn_refs* r, float eps, float* bn, hipStream_t st) {
  Cols w;
  bool window;
  KWS_TRY(cols_of(c, "gbn_infer", &w, &window));
  GbnRefs g{r->gamma, r->pstride, r->boff, r->mm, r->sstride, r->voff};
  hipLaunchKernelGGL(window ? gbn_infer_kernel<true> : gbn_infer_kernel<false>, dim3((unsigned)ceil_div(w.g * w.Ng, 256)), dim3(256), 0,
                     st, g, eps, bn, w);
  KWS_LAUNCH_CHECK("gbn_infer_kernel");
  return KWS_OK;
}

int kws_gbn_bwd_rows(int64_t M) { return (int)ceil_div64(M, GBWD_ROWS); }

int kws_gbn_bwd(float* dA, const float* y, const float* bn, const float* add, int64_t M, const kws_gbn_cols* c, float* part, float* coef,
                float* dgamma0, int64_t pstride, int64_t boff, hipStream_t st) {
  Cols w;
  bool window;
  KWS_TRY(cols_of(c, "gbn_bwd", &w, &window));
  const int F = w.g * w.Ng, rows = kws_gbn_bwd_rows(M);
  KwsProfScope prof("gbn_bwd", 0.0, 4.0 * 5.0 * (double)M * F, st);
  const auto pass1 = window ? (add ? gbn_bwd_part_kernel<true, true> : gbn_bwd_part_kernel<true, false>)
                            : (add ? gbn_bwd_part_kernel<false, true> : gbn_bwd_part_kernel<false, false>);
  hipLaunchKernelGGL(pass1, dim3((unsigned)rows, (unsigned)ceil_div(F, 256)), dim3(256), 0, st, dA, y, bn, add, M, w, part);
  KWS_LAUNCH_CHECK("gbn_bwd_part_kernel");
  return bwd_finish_launch(dA, y, bn, M, w, window, part, rows, coef, dgamma0, pstride, boff, st);
}

int kws_gbn_bwd_finish(float* gbuf, const float* y, const float* bn, int64_t M, const kws_gbn_cols* c, const float* part, int rows,
                       float* coef, float* dgamma0, int64_t pstride, int64_t boff, hipStream_t st) {
  Cols w;
  bool window;
  KWS_TRY(cols_of(c, "gbn_bwd_finish", &w, &window));
  KwsProfScope prof("gbn_bwd_finish", 0.0, 4.0 * 3.0 * (double)M * w.g * w.Ng, st);
  return bwd_finish_launch(gbuf, y, bn, M, w, window, part, rows, coef, dgamma0, pstride, boff, st);
}
