// Dense NHWC Conv2D (kh x kw taps, stride 1 or 2 and dilation 1 or 2 per axis, zero padding in TensorFlow's SAME geometry or
// none) on f32 MFMA (v_mfma_f32_32x32x2_f32): the convolution of the reference's MFCC-image models (conv_2d_mobile, conv_2d_fast,
// model.py:515-639).  X [B, H, W, Cin], Y / dY [B, Hout, Wout, F], kernel Wt [kh, kw, Cin, F] (Keras layout).  Three operations
// on conv1d.hip's tile (a 128 x 64 output tile per 256-thread workgroup, 4 waves x 32 rows x 64 columns, 16-deep K slabs
// double-buffered through LDS with a register prefetch; every operand loaded element-wise with bounds checks, so Cin = 1 and
// ragged widths need no special case):
//   forward  Y[b,p,q,n] = sum_{i,j,c} act(X[b, p*sh - pad_t + dh*i, q*sw - pad_l + dw*j, c]) * Wt[i,j,c,n]   implicit GEMM,
//            M = B*Hout*Wout, K = kh*kw*Cin walked as (tap, channel).  A tap outside the image contributes 0 - the padding is
//            zeros of the ACTIVATED tensor, not act(0).  act = relu6 or relu of the producer's table, or the identity.  BN partial
//            sums [m_tiles][2][F] go out in the epilogue (128-row tiles, kws_conv1d_fwd_f32's contract)
//   dgrad    dX[b,y,x,c] = sum over the taps (i,j) with (y + pad_t - dh*i) = sh*p and (x + pad_l - dw*j) = sw*q of
//            sum_n dY[b,p,q,n] * Wt[i,j,c,n].  Split by the stride phase (py, px) = ((y + pad_t) mod sh, (x + pad_l) mod sw) the
//            way gconv.hip's dgrad is: the pixels of one phase see the taps i = py + sh*i', j = px + sw*j' only, so each phase is
//            one dense GEMM with K = taps_h(py) * taps_w(px) * F and no tap that cannot hit is visited.  A phase without taps
//            (1 x 1 at stride 2) and pixels past the last window get exact zeros; every element is written once by one thread
//   wgrad    dWt[(i,j,c), n] = sum_m act(X)[m, (i,j,c)] * dY[m, n]; the M range is split into S slabs summed afterwards in a
//            fixed order: no float atomics
// A copy of conv1d.hip's kernel, not a shared template: the row index decomposes into (b, p, q) with two strides, two pads and a
// phase pair, which changes every load and the dgrad epilogue; the two files share only the MFMA loop.
#include <math.h>

#include "common.h"
#include "internal.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int C2_BM = 128, C2_BN = 64, C2_BK = 16;
constexpr int C2_LDP = C2_BM + 4, C2_LDQ = C2_BN + 4;
constexpr int C2_SMEM = C2_BM * (C2_BN + 1);   // epilogue tile of the forward; the pipeline buffers fit in it
static_assert(2 * C2_BK * (C2_LDP + C2_LDQ) <= C2_SMEM, "conv2d LDS");
constexpr int C2_WG_TARGET = 1024;             // weight gradient: workgroups aimed for (tiles x slabs)
constexpr int C2_MAX_KH = 20, C2_MAX_KW = 8;

enum { C2_FWD = 0, C2_DGRAD = 1, C2_WGRAD = 2 };

struct C2Args {
  kws_conv2d_t d;
  const float* X;    // fwd / wgrad: [B, H, W, Cin]
  const float* bn;   // the input's table [4][Cin], or NULL
  const float* W;    // fwd / dgrad: [kh, kw, Cin, F]
  const float* dY;   // dgrad / wgrad: [B, Hout, Wout, F]
  float* out;        // fwd: Y; dgrad: dX; wgrad: slab workspace [S][K][F]
  float* stats;      // fwd (may be NULL)
  int M;             // fwd / wgrad: B * Hout * Wout; dgrad: B * Qh * Qw (pixels of one phase, with slack)
  int K;             // fwd / wgrad: kh * kw * Cin
  int Qh, Qw;        // dgrad: rows / columns of one phase
  int n_tiles;       // wgrad: tiles along F; dgrad: tiles along Cin
  int chunk;         // wgrad: M rows per slab
  float hi;          // upper clip of the activation: 6 (relu6) or +inf (relu)
};

__device__ __forceinline__ float c2_act(float v, float sc, float sh, float hi, bool on) {
  return on ? fminf(fmaxf(fmaf(v, sc, sh), 0.f), hi) : v;
}

template <int MODE>
__global__ __launch_bounds__(256) void conv2d_kernel(C2Args a) {
  __shared__ float smem[C2_SMEM];
  float* sP = smem;                          // [2][BK][LDP]   P[r][kappa] stored kappa-major
  float* sQ = smem + 2 * C2_BK * C2_LDP;     // [2][BK][LDQ]   Q[kappa][c]
  const kws_conv2d_t& d = a.d;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
  const bool use_bn = a.bn != nullptr;
  const int HWo = d.Hout * d.Wout;

  int r0, c0, Kd;
  int mb = 0, me = 0;
  int py = 0, px = 0, th = 0, tw = 0;        // dgrad: the phase and its taps per axis
  if (MODE == C2_WGRAD) {
    const int kt = blockIdx.x / a.n_tiles;
    r0 = kt * C2_BM;
    c0 = (blockIdx.x % a.n_tiles) * C2_BN;
    mb = blockIdx.y * a.chunk;
    me = mb + a.chunk < a.M ? mb + a.chunk : a.M;
    Kd = mb < me ? me - mb : 0;
  } else if (MODE == C2_DGRAD) {
    r0 = blockIdx.x * C2_BM;
    const int ph = blockIdx.y / a.n_tiles;
    c0 = (blockIdx.y % a.n_tiles) * C2_BN;
    py = ph / d.sw;
    px = ph - py * d.sw;
    th = py < d.kh ? (d.kh - py + d.sh - 1) / d.sh : 0;
    tw = px < d.kw ? (d.kw - px + d.sw - 1) / d.sw : 0;
    Kd = th * tw * d.F;
  } else {
    r0 = blockIdx.x * C2_BM;
    c0 = blockIdx.y * C2_BN;
    Kd = a.K;
  }

  // per-thread state that does not change along the reduction
  int64_t rowoff[8];   // fwd: start of the clip in X; dgrad: start of the clip in dY
  int rowh[8];         // fwd: p*sh - pad_t; dgrad: qy
  int roww[8];         // fwd: q*sw - pad_l; dgrad: qx
  bool rowok[8];
  const int kp = tid & 15, rp0 = tid >> 4;         // kappa-fast P mapping (fwd, dgrad)
  const int rp = tid & 127, kp0 = tid >> 7;        // r-fast P mapping (wgrad)
  const int cq = tid & 63, kq0 = tid >> 6;         // c-fast Q mapping (fwd, wgrad)
  const int kq = tid & 15, cq0 = tid >> 4;         // kappa-fast Q mapping (dgrad)
  if (MODE == C2_FWD) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int m = r0 + rp0 + 16 * e;
      rowok[e] = m < a.M;
      const int b = rowok[e] ? m / HWo : 0;
      const int pq = rowok[e] ? m - b * HWo : 0;
      const int p = pq / d.Wout, q = pq - p * d.Wout;
      rowh[e] = p * d.sh - d.pad_t;
      roww[e] = q * d.sw - d.pad_l;
      rowoff[e] = (int64_t)b * d.H * d.W * d.Cin;
    }
  } else if (MODE == C2_DGRAD) {
    const int QQ = a.Qh * a.Qw;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int m = r0 + rp0 + 16 * e;
      rowok[e] = m < a.M;
      const int b = rowok[e] ? m / QQ : 0;
      const int pq = rowok[e] ? m - b * QQ : 0;
      rowh[e] = pq / a.Qw;
      roww[e] = pq - rowh[e] * a.Qw;
      rowoff[e] = (int64_t)b * HWo * d.F;
    }
  }
  // wgrad: this thread's P row is one fixed (tap, channel)
  int w_c = 0, w_dy = 0, w_dx = 0;
  bool w_ok = false;
  float w_sc = 1.f, w_sh = 0.f;
  if (MODE == C2_WGRAD) {
    const int kk = r0 + rp;
    w_ok = kk < a.K;
    const int tap = w_ok ? kk / d.Cin : 0;
    w_c = w_ok ? kk - tap * d.Cin : 0;
    const int i = tap / d.kw, j = tap - i * d.kw;
    w_dy = d.dh * i - d.pad_t;
    w_dx = d.dw * j - d.pad_l;
    if (use_bn && w_ok) {
      w_sc = a.bn[w_c];
      w_sh = a.bn[d.Cin + w_c];
    }
  }

  float rP[8], rQ[4];
  auto load = [&](int k0) {
    if (MODE == C2_FWD) {
      const int kk = k0 + kp;
      const bool okk = kk < Kd;
      const int tap = okk ? kk / d.Cin : 0, c = okk ? kk - tap * d.Cin : 0;
      const int i = tap / d.kw, j = tap - i * d.kw;
      const int dy = d.dh * i, dx = d.dw * j;
      float sc = 1.f, sh = 0.f;
      if (use_bn && okk) {
        sc = a.bn[c];
        sh = a.bn[d.Cin + c];
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int r = rowh[e] + dy, s = roww[e] + dx;
        rP[e] = (okk && rowok[e] && r >= 0 && r < d.H && s >= 0 && s < d.W)
                    ? c2_act(a.X[rowoff[e] + ((int64_t)r * d.W + s) * d.Cin + c], sc, sh, a.hi, use_bn)
                    : 0.f;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int kk2 = k0 + kq0 + 4 * e, n = c0 + cq;
        rQ[e] = (kk2 < Kd && n < d.F) ? a.W[(int64_t)kk2 * d.F + n] : 0.f;
      }
    } else if (MODE == C2_DGRAD) {
      const int kk = k0 + kp;
      const bool okk = kk < Kd;
      const int tap = okk ? kk / d.F : 0, n = okk ? kk - tap * d.F : 0;
      const int i1 = tw > 0 ? tap / tw : 0, j1 = tap - i1 * tw;
      const int dy = d.dh * i1, dx = d.dw * j1;   // dilation > 1 only at stride 1, where i = i1
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int p = rowh[e] - dy, q = roww[e] - dx;
        rP[e] = (okk && rowok[e] && p >= 0 && p < d.Hout && q >= 0 && q < d.Wout)
                    ? a.dY[rowoff[e] + ((int64_t)p * d.Wout + q) * d.F + n]
                    : 0.f;
      }
      const int kk2 = k0 + kq;
      const bool okk2 = kk2 < Kd;
      const int tap2 = okk2 ? kk2 / d.F : 0, n2 = okk2 ? kk2 - tap2 * d.F : 0;
      const int i2 = tw > 0 ? tap2 / tw : 0, j2 = tap2 - i2 * tw;
      const int wi = py + d.sh * i2, wj = px + d.sw * j2;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = c0 + cq0 + 16 * e;
        rQ[e] = (okk2 && c < d.Cin) ? a.W[(((int64_t)wi * d.kw + wj) * d.Cin + c) * d.F + n2] : 0.f;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int m = mb + k0 + kp0 + 2 * e;
        const bool okm = w_ok && m < me;
        const int b = okm ? m / HWo : 0;
        const int pq = okm ? m - b * HWo : 0;
        const int p = pq / d.Wout, q = pq - p * d.Wout;
        const int r = p * d.sh + w_dy, s = q * d.sw + w_dx;
        rP[e] = (okm && r >= 0 && r < d.H && s >= 0 && s < d.W)
                    ? c2_act(a.X[(((int64_t)b * d.H + r) * d.W + s) * d.Cin + w_c], w_sc, w_sh, a.hi, use_bn)
                    : 0.f;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int m = mb + k0 + kq0 + 4 * e;
        const int n = c0 + cq;
        rQ[e] = (m < me && n < d.F) ? a.dY[(int64_t)m * d.F + n] : 0.f;
      }
    }
  };
  auto store = [&](int buf) {
    float* P = sP + buf * C2_BK * C2_LDP;
    float* Qs = sQ + buf * C2_BK * C2_LDQ;
    if (MODE == C2_WGRAD) {
#pragma unroll
      for (int e = 0; e < 8; ++e) P[(kp0 + 2 * e) * C2_LDP + rp] = rP[e];
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) P[kp * C2_LDP + rp0 + 16 * e] = rP[e];
    }
    if (MODE == C2_DGRAD) {
#pragma unroll
      for (int e = 0; e < 4; ++e) Qs[kq * C2_LDQ + cq0 + 16 * e] = rQ[e];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) Qs[(kq0 + 4 * e) * C2_LDQ + cq] = rQ[e];
    }
  };

  f32x16 acc0, acc1;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    acc0[v] = 0.f;
    acc1[v] = 0.f;
  }
  const int stages = (Kd + C2_BK - 1) / C2_BK;
  if (stages > 0) {
    load(0);
    store(0);
  }
  __syncthreads();
  for (int st = 0; st < stages; ++st) {
    const int cur = st & 1;
    if (st + 1 < stages) load((st + 1) * C2_BK);
    const float* P = sP + cur * C2_BK * C2_LDP + wave * 32 + li;
    const float* Qs = sQ + cur * C2_BK * C2_LDQ + li;
#pragma unroll
    for (int s = 0; s < C2_BK / 2; ++s) {
      const float av = P[(2 * s + lh) * C2_LDP];
      const float b0 = Qs[(2 * s + lh) * C2_LDQ], b1 = Qs[(2 * s + lh) * C2_LDQ + 32];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, acc1, 0, 0, 0);
    }
    if (st + 1 < stages) store(cur ^ 1);
    __syncthreads();
  }

  // epilogue: accumulator element v of lane l is row 32*wave + (v&3) + 8*(v>>2) + 4*lh, column li (+32 for acc1)
  if (MODE == C2_FWD) {
    float* tile = smem;   // [BM][BN + 1] (the pipeline buffers are free after the last barrier)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int rl = wave * 32 + (v & 3) + 8 * (v >> 2) + 4 * lh, cl = h * 32 + li;
        const float val = h ? acc1[v] : acc0[v];
        tile[rl * (C2_BN + 1) + cl] = val;
        const int m = r0 + rl;
        const int n = c0 + cl;
        if (m < a.M && n < d.F) a.out[(int64_t)m * d.F + n] = val;
      }
    if (a.stats) {
      __syncthreads();
      if (tid < 2 * C2_BN) {
        const int cl = tid & (C2_BN - 1), sq = tid >> 6;
        float s = 0.f;
        for (int r = 0; r < C2_BM; ++r) {   // rows past M hold exact zeros (their operands were zero)
          const float v = tile[r * (C2_BN + 1) + cl];
          s += sq ? v * v : v;
        }
        const int n = c0 + cl;
        if (n < d.F) a.stats[((int64_t)blockIdx.x * 2 + sq) * d.F + n] = s;
      }
    }
  } else if (MODE == C2_DGRAD) {
    const int QQ = a.Qh * a.Qw;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int m = r0 + wave * 32 + (v & 3) + 8 * (v >> 2) + 4 * lh;   // = (b * Qh + qy) * Qw + qx
      if (m >= a.M) continue;
      const int b = m / QQ, pq = m - b * QQ;
      const int qy = pq / a.Qw, qx = pq - qy * a.Qw;
      const int y = d.sh * qy + py - d.pad_t, x = d.sw * qx + px - d.pad_l;   // the one pixel of this phase at (qy, qx)
      if (y < 0 || y >= d.H || x < 0 || x >= d.W) continue;
      float* o = a.out + (((int64_t)b * d.H + y) * d.W + x) * d.Cin;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int c = c0 + h * 32 + li;
        if (c < d.Cin) o[c] = h ? acc1[v] : acc0[v];
      }
    }
  } else {
    float* ws = a.out + (int64_t)blockIdx.y * a.K * d.F;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int kk = r0 + wave * 32 + (v & 3) + 8 * (v >> 2) + 4 * lh;
        const int n = c0 + h * 32 + li;
        if (kk < a.K && n < d.F) ws[(int64_t)kk * d.F + n] = h ? acc1[v] : acc0[v];
      }
  }
}

// dW[i] = sum over slabs s = 0, 1, ... of ws[s][i] (ascending: the same order in every run)
__global__ __launch_bounds__(256) void conv2d_wgrad_sum_kernel(const float* __restrict__ ws, float* __restrict__ dW, int64_t n, int S) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int k = 0; k < S; ++k) s += ws[k * n + i];
  dW[i] = s;
}

struct C2WgPlan {
  int k_tiles, n_tiles, S;
  int chunk;
};
C2WgPlan c2_wgrad_plan(const kws_conv2d_t* d) {
  C2WgPlan pl;
  const int K = d->kh * d->kw * d->Cin;
  const int64_t M = (int64_t)d->B * d->Hout * d->Wout;
  pl.k_tiles = ceil_div(K, C2_BM);
  pl.n_tiles = ceil_div(d->F, C2_BN);
  const int tiles = pl.k_tiles * pl.n_tiles;
  int64_t S = ceil_div64(C2_WG_TARGET, tiles);
  const int64_t max_s = ceil_div64(M, 4 * C2_BK);   // at least 64 rows per slab
  if (S > max_s) S = max_s;
  if (S < 1) S = 1;
  pl.chunk = (int)(ceil_div64(ceil_div64(M, S), C2_BK) * C2_BK);
  pl.S = (int)ceil_div64(M, pl.chunk);
  return pl;
}

// one axis of the geometry: TensorFlow's SAME (out = ceil(in / s), pad in front = total / 2) or VALID (no padding)
bool c2_axis_ok(int in, int out, int k, int s, int dil, int pad) {
  const int span = dil * (k - 1) + 1;
  const int same_out = (in + s - 1) / s;
  int total = (same_out - 1) * s + span - in;
  if (total < 0) total = 0;
  if (out == same_out && pad == total / 2) return true;
  return pad == 0 && in >= span && out == (in - span) / s + 1;
}

int c2_check_desc(const kws_conv2d_t* d) {
  KWS_REQUIRE(d != nullptr, "conv2d: descriptor is NULL");
  KWS_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0 && d->Hout > 0 && d->Wout > 0 && d->Cin > 0 && d->F > 0,
              "conv2d: B=%d H=%d W=%d Hout=%d Wout=%d Cin=%d F=%d must be positive", d->B, d->H, d->W, d->Hout, d->Wout, d->Cin, d->F);
  KWS_REQUIRE(d->kh >= 1 && d->kh <= C2_MAX_KH && d->kw >= 1 && d->kw <= C2_MAX_KW, "conv2d: window %d x %d (1..%d x 1..%d)", d->kh,
              d->kw, C2_MAX_KH, C2_MAX_KW);
  KWS_REQUIRE((d->sh == 1 || d->sh == 2) && (d->sw == 1 || d->sw == 2), "conv2d: strides (%d, %d) must be 1 or 2", d->sh, d->sw);
  KWS_REQUIRE((d->dh == 1 || d->dh == 2) && (d->dw == 1 || d->dw == 2), "conv2d: dilation (%d, %d) must be 1 or 2", d->dh, d->dw);
  KWS_REQUIRE((d->dh == 1 || d->sh == 1) && (d->dw == 1 || d->sw == 1), "conv2d: dilation (%d, %d) needs stride 1, got (%d, %d)", d->dh,
              d->dw, d->sh, d->sw);
  KWS_REQUIRE(d->act == KWS_ACT_RELU6 || d->act == KWS_ACT_RELU, "conv2d: act=%d (0 relu6, 1 relu)", d->act);
  KWS_REQUIRE(c2_axis_ok(d->H, d->Hout, d->kh, d->sh, d->dh, d->pad_t),
              "conv2d: Hout=%d pad_t=%d do not follow from H=%d kh=%d sh=%d dh=%d (SAME or VALID)", d->Hout, d->pad_t, d->H, d->kh, d->sh,
              d->dh);
  KWS_REQUIRE(c2_axis_ok(d->W, d->Wout, d->kw, d->sw, d->dw, d->pad_l),
              "conv2d: Wout=%d pad_l=%d do not follow from W=%d kw=%d sw=%d dw=%d (SAME or VALID)", d->Wout, d->pad_l, d->W, d->kw, d->sw,
              d->dw);
  KWS_REQUIRE(ceil_div(d->F, C2_BN) <= 16383 && ceil_div(d->Cin, C2_BN) <= 16383 && (int64_t)d->kh * d->kw * d->Cin < (1ll << 30) &&
                  (int64_t)d->kh * d->kw * d->F < (1ll << 30),
              "conv2d: grid too large");
  // row indices are 32-bit: the phase grid of the input gradient is the largest row count (at most (H + kh) * (W + kw) per clip)
  KWS_REQUIRE((int64_t)d->B * (d->H + C2_MAX_KH) * (d->W + C2_MAX_KW) < (1ll << 30) && (int64_t)d->B * d->Hout * d->Wout < (1ll << 30) &&
                  (int64_t)d->B * d->H * d->W * d->Cin < (1ll << 40) && (int64_t)d->B * d->Hout * d->Wout * d->F < (1ll << 40),
              "conv2d: tensor too large");
  return KWS_OK;
}

float c2_hi(const kws_conv2d_t* d) { return d->act == KWS_ACT_RELU ? INFINITY : 6.f; }

}  // namespace

extern "C" {

int kws_conv2d_stats_rows(const kws_conv2d_t* d) {
  return d && d->B > 0 && d->Hout > 0 && d->Wout > 0 ? (int)ceil_div64((int64_t)d->B * d->Hout * d->Wout, C2_BM) : 0;
}

int kws_conv2d_fwd_f32(const float* X, const float* bn, const float* Wt, float* Y, float* stats_part, const kws_conv2d_t* d,
                       void* stream) {
  KWS_TRY(c2_check_desc(d));
  KWS_REQUIRE(X && Wt && Y, "conv2d_fwd: NULL pointer");
  C2Args a{};
  a.d = *d; a.X = X; a.bn = bn; a.W = Wt; a.out = Y; a.stats = stats_part; a.hi = c2_hi(d);
  a.M = d->B * d->Hout * d->Wout; a.K = d->kh * d->kw * d->Cin;
  const double flops = 2.0 * a.M * a.K * d->F;
  KwsProfScope prof("conv2d_fwd", flops, 4.0 * ((double)d->B * d->H * d->W * d->Cin + (double)a.K * d->F + (double)a.M * d->F),
                    (hipStream_t)stream);
  hipLaunchKernelGGL((conv2d_kernel<C2_FWD>), dim3((unsigned)ceil_div(a.M, C2_BM), (unsigned)ceil_div(d->F, C2_BN)), dim3(256), 0,
                     (hipStream_t)stream, a);
  KWS_LAUNCH_CHECK("conv2d_kernel<fwd>");
  return KWS_OK;
}

int kws_conv2d_dgrad_f32(const float* dY, const float* Wt, float* dX, const kws_conv2d_t* d, void* stream) {
  KWS_TRY(c2_check_desc(d));
  KWS_REQUIRE(dY && Wt && dX, "conv2d_dgrad: NULL pointer");
  C2Args a{};
  a.d = *d; a.W = Wt; a.dY = dY; a.out = dX; a.hi = c2_hi(d);
  // the pixels of phase (py, px) are y = sh*qy + py - pad_t, x = sw*qx + px - pad_l; these counts cover every phase (a pixel
  // outside the image is skipped)
  a.Qh = (d->H - 1 + d->pad_t) / d->sh + 1;
  a.Qw = (d->W - 1 + d->pad_l) / d->sw + 1;
  a.M = d->B * a.Qh * a.Qw;
  a.n_tiles = ceil_div(d->Cin, C2_BN);
  const int phases = d->sh * d->sw;
  KWS_REQUIRE((int64_t)phases * a.n_tiles <= 65535, "conv2d_dgrad: grid too large");
  const double flops = 2.0 * d->B * d->Hout * d->Wout * (double)d->kh * d->kw * d->F * d->Cin;
  KwsProfScope prof("conv2d_dgrad", flops,
                    4.0 * ((double)d->B * d->H * d->W * d->Cin + (double)d->kh * d->kw * d->F * d->Cin +
                           (double)d->B * d->Hout * d->Wout * d->F),
                    (hipStream_t)stream);
  hipLaunchKernelGGL((conv2d_kernel<C2_DGRAD>), dim3((unsigned)ceil_div(a.M, C2_BM), (unsigned)(phases * a.n_tiles)), dim3(256), 0,
                     (hipStream_t)stream, a);
  KWS_LAUNCH_CHECK("conv2d_kernel<dgrad>");
  return KWS_OK;
}

int64_t kws_conv2d_wgrad_workspace_floats(const kws_conv2d_t* d) {
  if (c2_check_desc(d) != KWS_OK) return 0;
  const C2WgPlan pl = c2_wgrad_plan(d);
  return (int64_t)pl.S * d->kh * d->kw * d->Cin * d->F;
}

int kws_conv2d_wgrad_f32(const float* X, const float* bn, const float* dY, float* dWt, float* workspace, const kws_conv2d_t* d,
                         void* stream) {
  KWS_TRY(c2_check_desc(d));
  KWS_REQUIRE(X && dY && dWt && workspace, "conv2d_wgrad: NULL pointer");
  const C2WgPlan pl = c2_wgrad_plan(d);
  KWS_REQUIRE(pl.S <= 65535 && (int64_t)pl.k_tiles * pl.n_tiles < (1ll << 31), "conv2d_wgrad: %d slabs", pl.S);
  C2Args a{};
  a.d = *d; a.X = X; a.bn = bn; a.dY = dY; a.out = workspace; a.hi = c2_hi(d);
  a.M = d->B * d->Hout * d->Wout; a.K = d->kh * d->kw * d->Cin; a.n_tiles = pl.n_tiles; a.chunk = pl.chunk;
  const double flops = 2.0 * a.M * a.K * d->F;
  KwsProfScope prof("conv2d_wgrad", flops,
                    4.0 * ((double)d->B * d->H * d->W * d->Cin + (double)a.M * d->F + (double)(pl.S + 1) * a.K * d->F), (hipStream_t)stream);
  hipLaunchKernelGGL((conv2d_kernel<C2_WGRAD>), dim3((unsigned)(pl.k_tiles * pl.n_tiles), (unsigned)pl.S), dim3(256), 0,
                     (hipStream_t)stream, a);
  KWS_LAUNCH_CHECK("conv2d_kernel<wgrad>");
  const int64_t n = (int64_t)a.K * d->F;
  hipLaunchKernelGGL(conv2d_wgrad_sum_kernel, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, (hipStream_t)stream, workspace, dWt, n,
                     pl.S);
  KWS_LAUNCH_CHECK("conv2d_wgrad_sum_kernel");
  return KWS_OK;
}

}  // extern "C"
