// MaxPool2D(pool_size=(2, 2), strides=2, padding='valid') over act(bn(y)), forward and backward: the pool of the reference's
// conv_2d_fast_model (model.py:597-639), where it follows Conv2D + BatchNormalization + relu directly.  kws_pool3s2_*'s
// contract (pool.hip) in two dimensions, with the activation a parameter (relu6 or relu).  y [B, H, W, C] is the RAW convolution
// output, bn its table scale|shift|mean|rstd [4][C]; Hout = H / 2, Wout = W / 2.
//   fwd   z[b,p,q,c] = max_{i,j<2} act(scale[c] * y[b, 2p+i, 2q+j, c] + shift[c]).  The activation comes BEFORE the maximum: a
//         BatchNorm scale may be negative, so max(y) normalised is not the same.
//   bwd   g[b,r,s,c] = act'(bn(y[b,r,s,c])) * dz[b, r/2, s/2, c] where (r, s) is the FIRST maximum of its window in row-major
//         order (TF MaxPoolGrad), else 0.  The windows do not overlap, so one thread owns a 2 x 2 cell of a float4 of channels and
//         writes its (up to) four elements of g exactly once; the cells of a last odd row or column belong to no window and get
//         exact zeros.  In the same pass the per-workgroup BatchNorm partial sums part[row][2][C] = (sum g, sum g * xhat) go out,
//         folded afterwards in a fixed order: no float atomics, bit-reproducible.
// Both are HBM-bound; 16-byte loads and stores.
#include "common.h"
#include "internal.h"
#include "part_rows.h"

namespace {

constexpr int P2_THREADS = kws_part::THREADS;

using kws_part::ld4;

__device__ __forceinline__ float4 p2_pre(const float* p, const float4 sc, const float4 sh) {
  const float4 v = ld4(p);
  return make_float4(fmaf(v.x, sc.x, sh.x), fmaf(v.y, sc.y, sh.y), fmaf(v.z, sc.z, sh.z), fmaf(v.w, sc.w, sh.w));
}
__device__ __forceinline__ float p2_clip(float v, float hi) { return fminf(fmaxf(v, 0.f), hi); }
__device__ __forceinline__ float4 p2_clip4(const float4 v, float hi) {
  return make_float4(p2_clip(v.x, hi), p2_clip(v.y, hi), p2_clip(v.z, hi), p2_clip(v.w, hi));
}
__device__ __forceinline__ float p2_max4(float a, float b, float c, float d) { return fmaxf(fmaxf(a, b), fmaxf(c, d)); }
// index (0..3, row-major) of the first maximum of a window
__device__ __forceinline__ int p2_first_max4(float a0, float a1, float a2, float a3) {
  int j = 0;
  float m = a0;
  if (a1 > m) { m = a1; j = 1; }
  if (a2 > m) { m = a2; j = 2; }
  if (a3 > m) j = 3;
  return j;
}

__global__ __launch_bounds__(P2_THREADS) void pool2x2_fwd_kernel(const float* __restrict__ y, const float* __restrict__ bn,
                                                                 float* __restrict__ z, int64_t n, int H, int W, int Ho, int Wo, int C,
                                                                 float hi) {
  const int64_t i = (int64_t)blockIdx.x * P2_THREADS + threadIdx.x;
  if (i >= n) return;
  const int C4 = C >> 2;
  const int c = (int)(i % C4) * 4;
  int64_t cell = i / C4;
  const int q = (int)(cell % Wo);
  cell /= Wo;
  const int p = (int)(cell % Ho);
  const int64_t b = cell / Ho;
  const float4 sc = ld4(bn + c), sh = ld4(bn + C + c);
  const float* y0 = y + ((b * H + 2 * p) * W + 2 * q) * (int64_t)C + c;   // 2p + 1 <= H - 1 and 2q + 1 <= W - 1
  const float* y1 = y0 + (int64_t)W * C;
  const float4 a0 = p2_clip4(p2_pre(y0, sc, sh), hi), a1 = p2_clip4(p2_pre(y0 + C, sc, sh), hi);
  const float4 a2 = p2_clip4(p2_pre(y1, sc, sh), hi), a3 = p2_clip4(p2_pre(y1 + C, sc, sh), hi);
  *reinterpret_cast<float4*>(z + ((b * Ho + p) * Wo + q) * (int64_t)C + c) =
      make_float4(p2_max4(a0.x, a1.x, a2.x, a3.x), p2_max4(a0.y, a1.y, a2.y, a3.y), p2_max4(a0.z, a1.z, a2.z, a3.z),
                  p2_max4(a0.w, a1.w, a2.w, a3.w));
}

// One thread: a float4 of channels x the cell of rows 2ph, 2ph + 1 and columns 2pw, 2pw + 1 (ph < ceil(H / 2), pw < ceil(W / 2)).
// A cell with all four pixels inside the Ho x Wo windows is a pool window; any other cell lies in the last odd row / column.
__global__ __launch_bounds__(P2_THREADS) void pool2x2_bwd_kernel(const float* __restrict__ dz, const float* __restrict__ y,
                                                                 const float* __restrict__ bn, float* __restrict__ g,
                                                                 float* __restrict__ part, int64_t cells, int H, int W, int Ho, int Wo,
                                                                 int Hc, int Wc, int C, int R, float hi) {
  const int C4 = C >> 2;
  const int tid = threadIdx.x;
  const int r = tid / C4, c4 = tid - r * C4;
  const int c = c4 * 4;
  const int64_t cell = (int64_t)blockIdx.x * R + r;
  float4 sg = make_float4(0.f, 0.f, 0.f, 0.f), sgx = sg;
  if (cell < cells) {
    const int pw = (int)(cell % Wc);
    const int64_t t = cell / Wc;
    const int ph = (int)(t % Hc);
    const int64_t b = t / Hc;
    const int64_t base = ((b * H + 2 * ph) * W + 2 * pw) * (int64_t)C + c;
    const int64_t off[4] = {0, (int64_t)C, (int64_t)W * C, (int64_t)W * C + C};
    if (ph < Ho && pw < Wo) {
      const float4 sc = ld4(bn + c), sh = ld4(bn + C + c), mean = ld4(bn + 2 * C + c), rstd = ld4(bn + 3 * C + c);
      float4 yv[4], pre[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        yv[e] = ld4(y + base + off[e]);
        pre[e] = make_float4(fmaf(yv[e].x, sc.x, sh.x), fmaf(yv[e].y, sc.y, sh.y), fmaf(yv[e].z, sc.z, sh.z), fmaf(yv[e].w, sc.w, sh.w));
      }
      const float4 d = ld4(dz + ((b * Ho + ph) * Wo + pw) * (int64_t)C + c);
      float4 out[4];
#define KWS_POOL2_ROUTE(f)                                                                                              \
  do {                                                                                                                  \
    const int j = p2_first_max4(p2_clip(pre[0].f, hi), p2_clip(pre[1].f, hi), p2_clip(pre[2].f, hi), p2_clip(pre[3].f, hi)); \
    _Pragma("unroll") for (int e = 0; e < 4; ++e) out[e].f = e == j ? d.f * kws_part::gate(pre[e].f, hi) : 0.f;         \
  } while (0)
      KWS_POOL2_ROUTE(x);
      KWS_POOL2_ROUTE(y);
      KWS_POOL2_ROUTE(z);
      KWS_POOL2_ROUTE(w);
#undef KWS_POOL2_ROUTE
#pragma unroll
      for (int e = 0; e < 4; ++e) {   // row-major, as the window is searched
        *reinterpret_cast<float4*>(g + base + off[e]) = out[e];
        KWS_PART_ACCUMULATE(sg, sgx, out[e], yv[e], mean, rstd);
      }
    } else {
      // the last odd row / column: in no window
      const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int rr = 2 * ph + (e >> 1), ss = 2 * pw + (e & 1);
        if (rr < H && ss < W) *reinterpret_cast<float4*>(g + base + off[e]) = zero;
      }
    }
  }
  kws_part::fold_runs(sg, sgx, part, C, R);   // the R cells of this workgroup, ascending
}

bool p2_ok(int B, int H, int W, int C, int act) {
  return B > 0 && H >= 2 && W >= 2 && kws_part::channels_ok(C) && (act == KWS_ACT_RELU6 || act == KWS_ACT_RELU) &&
         (int64_t)B * H * W * C < (1ll << 40);
}
struct P2Geom : kws_part::Geom {
  int Hc, Wc;
  int64_t cells;
};
P2Geom p2_geom(int B, int H, int W, int C) {
  const int Hc = (H + 1) / 2, Wc = (W + 1) / 2;
  const int64_t cells = (int64_t)B * Hc * Wc;
  return P2Geom{kws_part::geom(cells, C), Hc, Wc, cells};
}
float p2_hi(int act) { return act == KWS_ACT_RELU ? INFINITY : 6.f; }

}  // namespace

extern "C" {

int kws_pool2x2_fwd_f32(const float* y, const float* bn, float* z, int B, int H, int W, int C, int act, void* stream) {
  KWS_REQUIRE(y && bn && z && p2_ok(B, H, W, C, act), "pool2x2_fwd: bad arguments (B=%d H=%d W=%d C=%d act=%d)", B, H, W, C, act);
  const int Ho = H / 2, Wo = W / 2;
  const int64_t n = (int64_t)B * Ho * Wo * (C / 4);
  KWS_REQUIRE(ceil_div64(n, P2_THREADS) < (1ll << 31), "pool2x2_fwd: tensor too large");
  KwsProfScope prof("pool2x2_fwd", 8.0 * B * H * W * C, 4.0 * ((double)B * H * W * C + (double)B * Ho * Wo * C), (hipStream_t)stream);
  hipLaunchKernelGGL(pool2x2_fwd_kernel, dim3((unsigned)ceil_div64(n, P2_THREADS)), dim3(P2_THREADS), 0, (hipStream_t)stream, y, bn, z,
                     n, H, W, Ho, Wo, C, p2_hi(act));
  KWS_LAUNCH_CHECK("pool2x2_fwd_kernel");
  return KWS_OK;
}

int kws_pool2x2_bwd_part_rows(int B, int H, int W, int C) {
  if (!p2_ok(B, H, W, C, KWS_ACT_RELU6)) return 0;
  const P2Geom ge = p2_geom(B, H, W, C);
  return ge.grid < (1ll << 31) ? (int)ge.grid : 0;
}

int64_t kws_pool2x2_bwd_part_floats(int B, int H, int W, int C) { return (int64_t)kws_pool2x2_bwd_part_rows(B, H, W, C) * 2 * C; }

int kws_pool2x2_bwd_f32(const float* dz, const float* y, const float* bn, float* g, float* part, int B, int H, int W, int C, int act,
                        void* stream) {
  KWS_REQUIRE(dz && y && bn && g && part && p2_ok(B, H, W, C, act), "pool2x2_bwd: bad arguments (B=%d H=%d W=%d C=%d act=%d)", B, H, W,
              C, act);
  const P2Geom ge = p2_geom(B, H, W, C);
  KWS_REQUIRE(ge.grid < (1ll << 31), "pool2x2_bwd: tensor too large");
  KwsProfScope prof("pool2x2_bwd", 14.0 * B * H * W * C, 4.0 * (2.0 * B * H * W * C + (double)B * (H / 2) * (W / 2) * C),
                    (hipStream_t)stream);
  hipLaunchKernelGGL(pool2x2_bwd_kernel, dim3((unsigned)ge.grid), dim3((unsigned)ge.block), 0, (hipStream_t)stream, dz, y, bn, g, part,
                     ge.cells, H, W, H / 2, W / 2, ge.Hc, ge.Wc, C, ge.R, p2_hi(act));
  KWS_LAUNCH_CHECK("pool2x2_bwd_kernel");
  return KWS_OK;
}

}  // extern "C"
