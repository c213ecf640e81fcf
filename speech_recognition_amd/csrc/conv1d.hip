// Dense Conv1D (stride 1, k taps, dilation, zero padding on either side) on f32 MFMA (v_mfma_f32_32x32x2_f32), reading a
// column window [x0, x0 + Cin) of a wider input and writing a column window [y0, y0 + F) of a wider output: the convolution
// of the reference's inception blocks (model.py:312-406), whose branches read one joined tensor and write the slices of the
// next one.  Three operations on gconv.hip's tile (a 128 x 64 output tile per 256-thread workgroup, 4 waves x 32 rows x 64
// columns, 16-deep K slabs double-buffered through LDS with a register prefetch; every operand loaded element-wise with
// bounds checks, so no width has to be a multiple of anything):
//   forward  Y[b,t,y0+n] = sum_{j,c} act(X[b, t - pad_l + dil*j, x0+c]) * W[j,c,n]      implicit GEMM, K = k * Cin.  A tap
//            outside [0, L) contributes 0 - the padding is zeros of the ACTIVATED tensor, not act(0) = relu6(shift).  BN
//            partial sums [m_tiles][2][F] go out in the epilogue (128-row tiles, kws_gconv_fwd_f32's contract)
//   dgrad    dX[b,tau,x0+c] (+)= sum_j sum_n dY[b, tau + pad_l - dil*j, y0+n] * W[j,c,n]   one dense GEMM, K = k * F; every
//            element of the window is touched exactly once by one thread (overwrite or add: both bit-reproducible)
//   wgrad    dW[j*Cin+c, n] = sum_m act(X)[m, (j,c)] * dY[m, y0+n]; the M range is split into S slabs summed afterwards in a
//            fixed order: no float atomics
#include "common.h"
#include "internal.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int C1_BM = 128, C1_BN = 64, C1_BK = 16;
constexpr int C1_LDP = C1_BM + 4, C1_LDQ = C1_BN + 4;
constexpr int C1_SMEM = C1_BM * (C1_BN + 1);   // epilogue tile of the forward; the pipeline buffers fit in it
static_assert(2 * C1_BK * (C1_LDP + C1_LDQ) <= C1_SMEM, "conv1d LDS");
constexpr int C1_WG_TARGET = 1024;             // weight gradient: workgroups aimed for (tiles x slabs)
constexpr int C1_MAX_K = 7, C1_MAX_DIL = 4;

enum { C1_FWD = 0, C1_DGRAD = 1, C1_WGRAD = 2 };

struct C1Args {
  kws_conv1d_t d;
  const float* X;    // fwd / wgrad: [B, L, Cx]
  const float* bn;   // the input's table [4][Cx], or NULL
  const float* W;    // fwd / dgrad: [k, Cin, F]
  const float* dY;   // dgrad / wgrad: [B, Lout, Cy]
  float* out;        // fwd: Y; dgrad: dX; wgrad: slab workspace [S][K][F]
  float* stats;      // fwd (may be NULL)
  int64_t M;         // fwd / wgrad: B * Lout; dgrad: B * L
  int K;             // fwd / wgrad: k * Cin; dgrad: k * F
  int n_tiles;       // wgrad: tiles along F
  int64_t chunk;     // wgrad: M rows per slab
  int accumulate;    // dgrad
};

__device__ __forceinline__ float c1_act(float v, float sc, float sh, bool on) { return on ? relu6f(fmaf(v, sc, sh)) : v; }

template <int MODE>
__global__ __launch_bounds__(256) void conv1d_kernel(C1Args a) {
  __shared__ float smem[C1_SMEM];
  float* sP = smem;                          // [2][BK][LDP]   P[r][kappa] stored kappa-major
  float* sQ = smem + 2 * C1_BK * C1_LDP;     // [2][BK][LDQ]   Q[kappa][c]
  const kws_conv1d_t& d = a.d;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
  const bool use_bn = a.bn != nullptr;

  int r0, c0, Kd;
  int64_t mb = 0, me = 0;
  if (MODE == C1_WGRAD) {
    const int kt = blockIdx.x / a.n_tiles;
    r0 = kt * C1_BM;
    c0 = (blockIdx.x % a.n_tiles) * C1_BN;
    mb = (int64_t)blockIdx.y * a.chunk;
    me = mb + a.chunk < a.M ? mb + a.chunk : a.M;
    Kd = mb < me ? (int)(me - mb) : 0;
  } else {
    r0 = blockIdx.x * C1_BM;
    c0 = blockIdx.y * C1_BN;
    Kd = a.K;
  }

  // per-thread state that does not change along the reduction
  int64_t rowoff[8];   // fwd: start of the clip's window columns in X; dgrad: of the clip's window columns in dY
  int rowq[8];         // fwd: t - pad_l; dgrad: tau + pad_l
  bool rowok[8];
  const int kp = tid & 15, rp0 = tid >> 4;         // kappa-fast P mapping (fwd, dgrad)
  const int rp = tid & 127, kp0 = tid >> 7;        // r-fast P mapping (wgrad)
  const int cq = tid & 63, kq0 = tid >> 6;         // c-fast Q mapping (fwd, wgrad)
  const int kq = tid & 15, cq0 = tid >> 4;         // kappa-fast Q mapping (dgrad)
  if (MODE == C1_FWD) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int64_t m = r0 + rp0 + 16 * e;
      rowok[e] = m < a.M;
      const int64_t b = rowok[e] ? m / d.Lout : 0;
      rowq[e] = (rowok[e] ? (int)(m - b * d.Lout) : 0) - d.pad_l;
      rowoff[e] = b * d.L * d.Cx + d.x0;
    }
  } else if (MODE == C1_DGRAD) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int64_t m = r0 + rp0 + 16 * e;
      rowok[e] = m < a.M;
      const int64_t b = rowok[e] ? m / d.L : 0;
      rowq[e] = (rowok[e] ? (int)(m - b * d.L) : 0) + d.pad_l;
      rowoff[e] = b * d.Lout * d.Cy + d.y0;
    }
  }
  // wgrad: this thread's P row is one fixed (tap, channel)
  int w_col = 0, w_shift = 0;
  bool w_ok = false;
  float w_sc = 1.f, w_sh = 0.f;
  if (MODE == C1_WGRAD) {
    const int kk = r0 + rp;
    w_ok = kk < a.K;
    const int j = w_ok ? kk / d.Cin : 0, c = w_ok ? kk - j * d.Cin : 0;
    w_col = d.x0 + c;
    w_shift = d.dil * j - d.pad_l;
    if (use_bn && w_ok) {
      w_sc = a.bn[w_col];
      w_sh = a.bn[d.Cx + w_col];
    }
  }

  float rP[8], rQ[4];
  auto load = [&](int k0) {
    if (MODE == C1_FWD) {
      const int kk = k0 + kp;
      const bool okk = kk < Kd;
      const int j = okk ? kk / d.Cin : 0, c = okk ? kk - j * d.Cin : 0;
      float sc = 1.f, sh = 0.f;
      if (use_bn && okk) {
        sc = a.bn[d.x0 + c];
        sh = a.bn[d.Cx + d.x0 + c];
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int r = rowq[e] + d.dil * j;
        rP[e] = (okk && rowok[e] && r >= 0 && r < d.L) ? c1_act(a.X[rowoff[e] + (int64_t)r * d.Cx + c], sc, sh, use_bn) : 0.f;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int kk2 = k0 + kq0 + 4 * e, n = c0 + cq;
        rQ[e] = (kk2 < Kd && n < d.F) ? a.W[(int64_t)kk2 * d.F + n] : 0.f;
      }
    } else if (MODE == C1_DGRAD) {
      const int kk = k0 + kp;
      const bool okk = kk < Kd;
      const int j = okk ? kk / d.F : 0, n = okk ? kk - j * d.F : 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int t = rowq[e] - d.dil * j;
        rP[e] = (okk && rowok[e] && t >= 0 && t < d.Lout) ? a.dY[rowoff[e] + (int64_t)t * d.Cy + n] : 0.f;
      }
      const int kk2 = k0 + kq;
      const bool okk2 = kk2 < Kd;
      const int j2 = okk2 ? kk2 / d.F : 0, n2 = okk2 ? kk2 - j2 * d.F : 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = c0 + cq0 + 16 * e;
        rQ[e] = (okk2 && c < d.Cin) ? a.W[((int64_t)j2 * d.Cin + c) * d.F + n2] : 0.f;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int64_t m = mb + k0 + kp0 + 2 * e;
        const bool okm = w_ok && m < me;
        const int64_t b = okm ? m / d.Lout : 0;
        const int r = (okm ? (int)(m - b * d.Lout) : 0) + w_shift;
        rP[e] = (okm && r >= 0 && r < d.L) ? c1_act(a.X[(b * d.L + r) * d.Cx + w_col], w_sc, w_sh, use_bn) : 0.f;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t m = mb + k0 + kq0 + 4 * e;
        const int n = c0 + cq;
        rQ[e] = (m < me && n < d.F) ? a.dY[m * d.Cy + d.y0 + n] : 0.f;
      }
    }
  };
  auto store = [&](int buf) {
    float* P = sP + buf * C1_BK * C1_LDP;
    float* Qs = sQ + buf * C1_BK * C1_LDQ;
    if (MODE == C1_WGRAD) {
#pragma unroll
      for (int e = 0; e < 8; ++e) P[(kp0 + 2 * e) * C1_LDP + rp] = rP[e];
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) P[kp * C1_LDP + rp0 + 16 * e] = rP[e];
    }
    if (MODE == C1_DGRAD) {
#pragma unroll
      for (int e = 0; e < 4; ++e) Qs[kq * C1_LDQ + cq0 + 16 * e] = rQ[e];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) Qs[(kq0 + 4 * e) * C1_LDQ + cq] = rQ[e];
    }
  };

  f32x16 acc0, acc1;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    acc0[v] = 0.f;
    acc1[v] = 0.f;
  }
  const int stages = (Kd + C1_BK - 1) / C1_BK;
  if (stages > 0) {
    load(0);
    store(0);
  }
  __syncthreads();
  for (int st = 0; st < stages; ++st) {
    const int cur = st & 1;
    if (st + 1 < stages) load((st + 1) * C1_BK);
    const float* P = sP + cur * C1_BK * C1_LDP + wave * 32 + li;
    const float* Qs = sQ + cur * C1_BK * C1_LDQ + li;
#pragma unroll
    for (int s = 0; s < C1_BK / 2; ++s) {
      const float av = P[(2 * s + lh) * C1_LDP];
      const float b0 = Qs[(2 * s + lh) * C1_LDQ], b1 = Qs[(2 * s + lh) * C1_LDQ + 32];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, acc1, 0, 0, 0);
    }
    if (st + 1 < stages) store(cur ^ 1);
    __syncthreads();
  }

  // epilogue: accumulator element v of lane l is row 32*wave + (v&3) + 8*(v>>2) + 4*lh, column li (+32 for acc1)
  if (MODE == C1_FWD) {
    float* tile = smem;   // [BM][BN + 1] (the pipeline buffers are free after the last barrier)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int rl = wave * 32 + (v & 3) + 8 * (v >> 2) + 4 * lh, cl = h * 32 + li;
        const float val = h ? acc1[v] : acc0[v];
        tile[rl * (C1_BN + 1) + cl] = val;
        const int64_t m = r0 + rl;
        const int n = c0 + cl;
        if (m < a.M && n < d.F) a.out[m * d.Cy + d.y0 + n] = val;
      }
    if (a.stats) {
      __syncthreads();
      if (tid < 2 * C1_BN) {
        const int cl = tid & (C1_BN - 1), sq = tid >> 6;
        float s = 0.f;
        for (int r = 0; r < C1_BM; ++r) {   // rows past M hold exact zeros (their operands were zero)
          const float v = tile[r * (C1_BN + 1) + cl];
          s += sq ? v * v : v;
        }
        const int n = c0 + cl;
        if (n < d.F) a.stats[((int64_t)blockIdx.x * 2 + sq) * d.F + n] = s;
      }
    }
  } else if (MODE == C1_DGRAD) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int64_t m = r0 + wave * 32 + (v & 3) + 8 * (v >> 2) + 4 * lh;   // = b * L + tau
        const int c = c0 + h * 32 + li;
        if (m >= a.M || c >= d.Cin) continue;
        float* o = a.out + m * d.Cx + d.x0 + c;
        const float val = h ? acc1[v] : acc0[v];
        *o = a.accumulate ? *o + val : val;
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
__global__ __launch_bounds__(256) void conv1d_wgrad_sum_kernel(const float* __restrict__ ws, float* __restrict__ dW, int64_t n, int S) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int k = 0; k < S; ++k) s += ws[k * n + i];
  dW[i] = s;
}

struct C1WgPlan {
  int k_tiles, n_tiles, S;
  int64_t chunk;
};
C1WgPlan c1_wgrad_plan(const kws_conv1d_t* d) {
  C1WgPlan pl;
  const int K = d->k * d->Cin;
  const int64_t M = (int64_t)d->B * d->Lout;
  pl.k_tiles = ceil_div(K, C1_BM);
  pl.n_tiles = ceil_div(d->F, C1_BN);
  const int tiles = pl.k_tiles * pl.n_tiles;
  int64_t S = ceil_div64(C1_WG_TARGET, tiles);
  const int64_t max_s = ceil_div64(M, 4 * C1_BK);   // at least 64 rows per slab
  if (S > max_s) S = max_s;
  if (S < 1) S = 1;
  pl.chunk = ceil_div64(ceil_div64(M, S), C1_BK) * C1_BK;
  pl.S = (int)ceil_div64(M, pl.chunk);
  return pl;
}

int c1_check_desc(const kws_conv1d_t* d) {
  KWS_REQUIRE(d != nullptr, "conv1d: descriptor is NULL");
  KWS_REQUIRE(d->B > 0 && d->L > 0 && d->Lout > 0 && d->Cx > 0 && d->Cin > 0 && d->Cy > 0 && d->F > 0,
              "conv1d: B=%d L=%d Lout=%d Cx=%d Cin=%d Cy=%d F=%d must be positive", d->B, d->L, d->Lout, d->Cx, d->Cin, d->Cy, d->F);
  KWS_REQUIRE(d->k >= 1 && d->k <= C1_MAX_K && d->dil >= 1 && d->dil <= C1_MAX_DIL, "conv1d: k=%d (1..%d) dil=%d (1..%d)", d->k,
              C1_MAX_K, d->dil, C1_MAX_DIL);
  const int span = d->dil * (d->k - 1);
  KWS_REQUIRE(d->pad_l >= 0 && d->pad_l <= span, "conv1d: pad_l=%d outside [0, dil*(k-1)=%d]", d->pad_l, span);
  // Lout = L + pad_l + pad_r - dil*(k-1) for some 0 <= pad_r <= dil*(k-1)
  const int pad_r = d->Lout - d->L - d->pad_l + span;
  KWS_REQUIRE(pad_r >= 0 && pad_r <= span, "conv1d: Lout=%d is inconsistent with L=%d pad_l=%d k=%d dil=%d (pad_r would be %d)", d->Lout,
              d->L, d->pad_l, d->k, d->dil, pad_r);
  KWS_REQUIRE(d->x0 >= 0 && (int64_t)d->x0 + d->Cin <= d->Cx, "conv1d: input window [%d, %d + %d) exceeds its pitch Cx=%d", d->x0, d->x0,
              d->Cin, d->Cx);
  KWS_REQUIRE(d->y0 >= 0 && (int64_t)d->y0 + d->F <= d->Cy, "conv1d: output window [%d, %d + %d) exceeds its pitch Cy=%d", d->y0, d->y0,
              d->F, d->Cy);
  KWS_REQUIRE(ceil_div(d->F, C1_BN) <= 65535 && ceil_div(d->Cin, C1_BN) <= 65535 && (int64_t)d->k * d->Cin < (1ll << 30) &&
                  (int64_t)d->k * d->F < (1ll << 30),
              "conv1d: grid too large");
  KWS_REQUIRE((int64_t)d->B * d->L * d->Cx < (1ll << 40) && (int64_t)d->B * d->Lout * d->Cy < (1ll << 40) &&
                  ceil_div64((int64_t)d->B * std::max(d->L, d->Lout), C1_BM) < (1ll << 31),
              "conv1d: tensor too large");
  return KWS_OK;
}

}  // namespace

extern "C" {

int kws_conv1d_stats_rows(const kws_conv1d_t* d) { return d ? (int)ceil_div64((int64_t)d->B * d->Lout, C1_BM) : 0; }

int kws_conv1d_fwd_f32(const float* X, const float* bn, const float* W, float* Y, float* stats_part, const kws_conv1d_t* d,
                       void* stream) {
  KWS_TRY(c1_check_desc(d));
  KWS_REQUIRE(X && W && Y, "conv1d_fwd: NULL pointer");
  C1Args a{};
  a.d = *d; a.X = X; a.bn = bn; a.W = W; a.out = Y; a.stats = stats_part;
  a.M = (int64_t)d->B * d->Lout; a.K = d->k * d->Cin;
  const double flops = 2.0 * a.M * a.K * d->F;
  KwsProfScope prof("conv1d_fwd", flops, 4.0 * ((double)d->B * d->L * d->Cin + (double)a.K * d->F + (double)a.M * d->F),
                    (hipStream_t)stream);
  hipLaunchKernelGGL((conv1d_kernel<C1_FWD>), dim3((unsigned)ceil_div64(a.M, C1_BM), (unsigned)ceil_div(d->F, C1_BN)), dim3(256), 0,
                     (hipStream_t)stream, a);
  KWS_LAUNCH_CHECK("conv1d_kernel<fwd>");
  return KWS_OK;
}

int kws_conv1d_dgrad_f32(const float* dY, const float* W, float* dX, int accumulate, const kws_conv1d_t* d, void* stream) {
  KWS_TRY(c1_check_desc(d));
  KWS_REQUIRE(dY && W && dX, "conv1d_dgrad: NULL pointer");
  KWS_REQUIRE(accumulate == 0 || accumulate == 1, "conv1d_dgrad: accumulate=%d (0 or 1)", accumulate);
  C1Args a{};
  a.d = *d; a.W = W; a.dY = dY; a.out = dX; a.accumulate = accumulate;
  a.M = (int64_t)d->B * d->L; a.K = d->k * d->F;
  const double flops = 2.0 * a.M * a.K * d->Cin;
  KwsProfScope prof("conv1d_dgrad", flops,
                    4.0 * ((double)a.M * d->Cin * (accumulate ? 2.0 : 1.0) + (double)a.K * d->Cin + (double)d->B * d->Lout * d->F),
                    (hipStream_t)stream);
  hipLaunchKernelGGL((conv1d_kernel<C1_DGRAD>), dim3((unsigned)ceil_div64(a.M, C1_BM), (unsigned)ceil_div(d->Cin, C1_BN)), dim3(256), 0,
                     (hipStream_t)stream, a);
  KWS_LAUNCH_CHECK("conv1d_kernel<dgrad>");
  return KWS_OK;
}

int64_t kws_conv1d_wgrad_workspace_floats(const kws_conv1d_t* d) {
  if (c1_check_desc(d) != KWS_OK) return 0;
  const C1WgPlan pl = c1_wgrad_plan(d);
  return (int64_t)pl.S * d->k * d->Cin * d->F;
}

int kws_conv1d_wgrad_f32(const float* X, const float* bn, const float* dY, float* dW, float* workspace, const kws_conv1d_t* d,
                         void* stream) {
  KWS_TRY(c1_check_desc(d));
  KWS_REQUIRE(X && dY && dW && workspace, "conv1d_wgrad: NULL pointer");
  const C1WgPlan pl = c1_wgrad_plan(d);
  KWS_REQUIRE(pl.S <= 65535 && (int64_t)pl.k_tiles * pl.n_tiles < (1ll << 31), "conv1d_wgrad: %d slabs", pl.S);
  C1Args a{};
  a.d = *d; a.X = X; a.bn = bn; a.dY = dY; a.out = workspace;
  a.M = (int64_t)d->B * d->Lout; a.K = d->k * d->Cin; a.n_tiles = pl.n_tiles; a.chunk = pl.chunk;
  const double flops = 2.0 * a.M * a.K * d->F;
  KwsProfScope prof("conv1d_wgrad", flops,
                    4.0 * ((double)d->B * d->L * d->Cin + (double)a.M * d->F + (double)(pl.S + 1) * a.K * d->F), (hipStream_t)stream);
  hipLaunchKernelGGL((conv1d_kernel<C1_WGRAD>), dim3((unsigned)(pl.k_tiles * pl.n_tiles), (unsigned)pl.S), dim3(256), 0,
                     (hipStream_t)stream, a);
  KWS_LAUNCH_CHECK("conv1d_kernel<wgrad>");
  const int64_t n = (int64_t)a.K * d->F;
  hipLaunchKernelGGL(conv1d_wgrad_sum_kernel, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, (hipStream_t)stream, workspace, dW, n,
                     pl.S);
  KWS_LAUNCH_CHECK("conv1d_wgrad_sum_kernel");
  return KWS_OK;
}

}  // extern "C"
