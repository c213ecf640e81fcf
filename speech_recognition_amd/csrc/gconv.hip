// Grouped Conv1D (VALID, k taps, time stride s, g channel groups) on f32 MFMA (v_mfma_f32_32x32x2_f32), the layer
// the reference builds as g separate Keras Conv1D layers over Lambda slices of one input (_grouped_reduce_conv /
// _grouped_context_conv, model.py:651-693 and 1258-1300).  Three operations, each ONE launch for all groups
// (blockIdx.z = group):
//   forward  Y[b,t,g*Ng+n]  = sum_{j,c} act(X[b, s*t+j, g*gs+c]) * W_g[j,c,n]      implicit GEMM, K = k*gs; the producer's
//            BatchNorm scale/shift + ReLU6 is applied on load (act = identity without a table); BN partial sums
//            [m_tiles][2][F] go out in the epilogue (the stats_part contract of kws_gemm_gather_f32, 128-row tiles)
//   dgrad    dX[b,tau,g*gs+c] = sum_{(t,j): s*t+j = tau} sum_n dY[b,t,g*Ng+n] * W_g[j,c,n]; split by phase p = tau mod s
//            so every output row is one dense GEMM over its ceil((k-p)/s) taps (K = taps_p * Ng).  Every element of dX is
//            written exactly once - rows past the last window and channels outside the groups get exact zeros
//   wgrad    dW_g[j*gs+c, n] = sum_m act(X)[m, (j,c)] * dY[m, g*Ng+n]; the M range is split into S slabs (one workgroup
//            per output tile and slab), summed afterwards in a fixed order: bit-reproducible, no float atomics.
// All three run one tile kernel: a 128 x 64 output tile per 256-thread workgroup (4 waves x 32 rows x 64 columns, two
// 32 x 32 accumulators each), 16-deep K slabs double-buffered through LDS with a register prefetch of the next slab.
// Operands are loaded element-wise with bounds checks, so group widths need not be multiples of anything (gs 42, 63,
// 75 ... and Ng 50, 75, 105 ... of the reference models).
// Each group's BatchNorm is its own Keras layer with its own table scale|shift|mean|rstd [4][Ng]: bncols.hip keeps them.
// Also here: the Flatten -> Dense -> softmax tail of the programs that end in one (kws_flat_tail_launch).
#include "common.h"
#include "internal.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int GC_BM = 128, GC_BN = 64, GC_BK = 16;
constexpr int GC_LDP = GC_BM + 4, GC_LDQ = GC_BN + 4;
constexpr int GC_SMEM = GC_BM * (GC_BN + 1);   // epilogue tile of the forward; the pipeline (2 x (16 x 132 + 16 x 68)) fits in it
static_assert(2 * GC_BK * (GC_LDP + GC_LDQ) <= GC_SMEM, "gconv LDS");
constexpr int GC_WG_TARGET = 1024;               // weight gradient: workgroups aimed for (tiles x slabs)

enum { GC_FWD = 0, GC_DGRAD = 1, GC_WGRAD = 2 };

struct GcArgs {
  kws_gconv_t d;
  int64_t wgs;       // floats between consecutive groups' kernels
  const float* X;    // fwd / wgrad: [B, L, C]
  const float* bn;   // producer's BN tables [C / bg][4][bg], or NULL
  int bg;
  const float* W;    // fwd / dgrad
  const float* dY;   // dgrad / wgrad: [B, Lout, F]
  float* out;        // fwd: Y; dgrad: dX; wgrad: slab workspace [S][g][K][Ng]
  float* stats;      // fwd (may be NULL)
  int64_t M;         // fwd / wgrad: B * Lout; dgrad: B * Q
  int K;             // fwd / wgrad: k * gs
  int Q;             // dgrad: ceil(L / s) rows per phase and clip
  int n_tiles;       // tiles along the output columns (Ng for fwd / wgrad, gs for dgrad)
  int64_t chunk;     // wgrad: M rows per slab
};

__device__ __forceinline__ float gc_act(float v, float sc, float sh, bool on) { return on ? relu6f(fmaf(v, sc, sh)) : v; }

template <int MODE>
__global__ __launch_bounds__(256) void gconv_kernel(GcArgs a) {
  __shared__ float smem[GC_SMEM];
  float* sP = smem;                          // [2][BK][LDP]   P[r][kappa] stored kappa-major
  float* sQ = smem + 2 * GC_BK * GC_LDP;     // [2][BK][LDQ]   Q[kappa][c]
  const kws_gconv_t& d = a.d;
  const int grp = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int F = d.g * d.Ng;
  const bool use_bn = a.bn != nullptr;

  int r0, c0, p = 0, Kd;
  int64_t mb = 0, me = 0;
  if (MODE == GC_FWD) {
    r0 = blockIdx.x * GC_BM;
    c0 = blockIdx.y * GC_BN;
    Kd = a.K;
  } else if (MODE == GC_DGRAD) {
    r0 = blockIdx.x * GC_BM;
    p = blockIdx.y / a.n_tiles;
    c0 = (blockIdx.y % a.n_tiles) * GC_BN;
    if (grp == d.g) {
      // channels no group reads: their gradient is exactly 0 (one block per row tile and phase does them all)
      if (c0 != 0) return;
      const int unused = d.C - d.g * d.gs;
      for (int idx = tid; idx < GC_BM * unused; idx += 256) {
        const int64_t m = r0 + idx / unused;
        const int ch = d.g * d.gs + idx % unused;
        if (m >= a.M) continue;
        const int b = (int)(m / a.Q), q = (int)(m % a.Q);
        const int tau = d.stride * q + p;
        if (tau < d.L) a.out[((int64_t)b * d.L + tau) * d.C + ch] = 0.f;
      }
      return;
    }
    const int taps = p < d.k ? (d.k - p + d.stride - 1) / d.stride : 0;
    Kd = taps * d.Ng;
  } else {
    const int kt = blockIdx.x / a.n_tiles;
    r0 = kt * GC_BM;
    c0 = (blockIdx.x % a.n_tiles) * GC_BN;
    mb = (int64_t)blockIdx.y * a.chunk;
    me = mb + a.chunk < a.M ? mb + a.chunk : a.M;
    Kd = mb < me ? (int)(me - mb) : 0;
  }

  // per-thread state that does not change along the reduction
  int64_t rowoff[8];   // fwd: start of the window of row m; dgrad: clip base of dY rows
  int rowq[8];         // dgrad: q of the row (-1: row outside)
  bool rowok[8];
  const int kp = tid & 15, rp0 = tid >> 4;         // kappa-fast P mapping (fwd, dgrad)
  const int rp = tid & 127, kp0 = tid >> 7;        // r-fast P mapping (wgrad)
  const int cq = tid & 63, kq0 = tid >> 6;         // c-fast Q mapping (fwd, wgrad)
  const int kq = tid & 15, cq0 = tid >> 4;         // kappa-fast Q mapping (dgrad)
  if (MODE == GC_FWD) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int64_t m = r0 + rp0 + 16 * e;
      rowok[e] = m < a.M;
      const int64_t b = rowok[e] ? m / d.Lout : 0;
      const int t = rowok[e] ? (int)(m - b * d.Lout) : 0;
      rowoff[e] = (b * d.L + (int64_t)t * d.stride) * d.C + (int64_t)grp * d.gs;
    }
  } else if (MODE == GC_DGRAD) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int64_t m = r0 + rp0 + 16 * e;
      rowok[e] = m < a.M;
      const int64_t b = rowok[e] ? m / a.Q : 0;
      rowq[e] = rowok[e] ? (int)(m - b * a.Q) : -1;
      rowoff[e] = b * d.Lout * F + (int64_t)grp * d.Ng;
    }
  }
  // wgrad: this thread's P row is one fixed (tap, channel)
  int w_off = 0;
  bool w_ok = false;
  float w_sc = 1.f, w_sh = 0.f;
  if (MODE == GC_WGRAD) {
    const int kk = r0 + rp;
    w_ok = kk < a.K;
    const int j = w_ok ? kk / d.gs : 0, c = w_ok ? kk - j * d.gs : 0;
    w_off = j * d.C + grp * d.gs + c;
    if (use_bn && w_ok) {
      const int ch = grp * d.gs + c, l = ch / a.bg, n = ch - l * a.bg;
      w_sc = a.bn[(int64_t)l * 4 * a.bg + n];
      w_sh = a.bn[(int64_t)l * 4 * a.bg + a.bg + n];
    }
  }
  const float* Wg = a.W ? a.W + (int64_t)grp * a.wgs : nullptr;

  float rP[8], rQ[4];
  auto load = [&](int k0) {
    if (MODE == GC_FWD) {
      const int kk = k0 + kp;
      const bool okk = kk < Kd;
      const int j = okk ? kk / d.gs : 0, c = okk ? kk - j * d.gs : 0;
      const int64_t off = (int64_t)j * d.C + c;
      float sc = 1.f, sh = 0.f;
      if (use_bn && okk) {
        const int ch = grp * d.gs + c, l = ch / a.bg, n = ch - l * a.bg;
        sc = a.bn[(int64_t)l * 4 * a.bg + n];
        sh = a.bn[(int64_t)l * 4 * a.bg + a.bg + n];
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) rP[e] = (okk && rowok[e]) ? gc_act(a.X[rowoff[e] + off], sc, sh, use_bn) : 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int kk2 = k0 + kq0 + 4 * e, n = c0 + cq;
        rQ[e] = (kk2 < Kd && n < d.Ng) ? Wg[(int64_t)kk2 * d.Ng + n] : 0.f;
      }
    } else if (MODE == GC_DGRAD) {
      const int kk = k0 + kp;
      const bool okk = kk < Kd;
      const int i = okk ? kk / d.Ng : 0, n = okk ? kk - i * d.Ng : 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int t = rowq[e] - i;
        rP[e] = (okk && rowok[e] && t >= 0 && t < d.Lout) ? a.dY[rowoff[e] + (int64_t)t * F + n] : 0.f;
      }
      const int kk2 = k0 + kq;
      const bool okk2 = kk2 < Kd;
      const int i2 = okk2 ? kk2 / d.Ng : 0, n2 = okk2 ? kk2 - i2 * d.Ng : 0;
      const int j = p + d.stride * i2;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = c0 + cq0 + 16 * e;
        rQ[e] = (okk2 && c < d.gs) ? Wg[((int64_t)j * d.gs + c) * d.Ng + n2] : 0.f;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int64_t m = mb + k0 + kp0 + 2 * e;
        const bool ok = w_ok && m < me;
        const int64_t b = ok ? m / d.Lout : 0;
        const int t = ok ? (int)(m - b * d.Lout) : 0;
        rP[e] = ok ? gc_act(a.X[(b * d.L + (int64_t)t * d.stride) * d.C + w_off], w_sc, w_sh, use_bn) : 0.f;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t m = mb + k0 + kq0 + 4 * e;
        const int n = c0 + cq;
        rQ[e] = (m < me && n < d.Ng) ? a.dY[m * F + (int64_t)grp * d.Ng + n] : 0.f;
      }
    }
  };
  auto store = [&](int buf) {
    float* P = sP + buf * GC_BK * GC_LDP;
    float* Qs = sQ + buf * GC_BK * GC_LDQ;
    if (MODE == GC_WGRAD) {
#pragma unroll
      for (int e = 0; e < 8; ++e) P[(kp0 + 2 * e) * GC_LDP + rp] = rP[e];
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) P[kp * GC_LDP + rp0 + 16 * e] = rP[e];
    }
    if (MODE == GC_DGRAD) {
#pragma unroll
      for (int e = 0; e < 4; ++e) Qs[kq * GC_LDQ + cq0 + 16 * e] = rQ[e];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) Qs[(kq0 + 4 * e) * GC_LDQ + cq] = rQ[e];
    }
  };

  f32x16 acc0, acc1;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    acc0[v] = 0.f;
    acc1[v] = 0.f;
  }
  const int stages = (Kd + GC_BK - 1) / GC_BK;
  if (stages > 0) {
    load(0);
    store(0);
  }
  __syncthreads();
  for (int st = 0; st < stages; ++st) {
    const int cur = st & 1;
    if (st + 1 < stages) load((st + 1) * GC_BK);
    const float* P = sP + cur * GC_BK * GC_LDP + wave * 32 + li;
    const float* Qs = sQ + cur * GC_BK * GC_LDQ + li;
#pragma unroll
    for (int s = 0; s < GC_BK / 2; ++s) {
      const float av = P[(2 * s + lh) * GC_LDP];
      const float b0 = Qs[(2 * s + lh) * GC_LDQ], b1 = Qs[(2 * s + lh) * GC_LDQ + 32];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, acc1, 0, 0, 0);
    }
    if (st + 1 < stages) store(cur ^ 1);
    __syncthreads();
  }

  // epilogue: accumulator element v of lane l is row 32*wave + (v&3) + 8*(v>>2) + 4*lh, column li (+32 for acc1)
  if (MODE == GC_FWD) {
    float* tile = smem;   // [BM][BN + 1] (the pipeline buffers are free after the last barrier)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int rl = wave * 32 + (v & 3) + 8 * (v >> 2) + 4 * lh, cl = h * 32 + li;
        const float val = h ? acc1[v] : acc0[v];
        tile[rl * (GC_BN + 1) + cl] = val;
        const int64_t m = r0 + rl;
        const int n = c0 + cl;
        if (m < a.M && n < d.Ng) a.out[m * F + (int64_t)grp * d.Ng + n] = val;
      }
    if (a.stats) {
      __syncthreads();
      if (tid < 2 * GC_BN) {
        const int cl = tid & (GC_BN - 1), sq = tid >> 6;
        float s = 0.f;
        for (int r = 0; r < GC_BM; ++r) {   // rows past M hold exact zeros (their operands were zero)
          const float v = tile[r * (GC_BN + 1) + cl];
          s += sq ? v * v : v;
        }
        const int n = c0 + cl;
        if (n < d.Ng) a.stats[((int64_t)blockIdx.x * 2 + sq) * F + (int64_t)grp * d.Ng + n] = s;
      }
    }
  } else if (MODE == GC_DGRAD) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int64_t m = r0 + wave * 32 + (v & 3) + 8 * (v >> 2) + 4 * lh;
        const int c = c0 + h * 32 + li;
        if (m >= a.M || c >= d.gs) continue;
        const int b = (int)(m / a.Q), q = (int)(m % a.Q);
        const int tau = d.stride * q + p;
        if (tau < d.L) a.out[((int64_t)b * d.L + tau) * d.C + (int64_t)grp * d.gs + c] = h ? acc1[v] : acc0[v];
      }
  } else {
    float* ws = a.out + ((int64_t)blockIdx.y * d.g + grp) * (int64_t)a.K * d.Ng;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int kk = r0 + wave * 32 + (v & 3) + 8 * (v >> 2) + 4 * lh;
        const int n = c0 + h * 32 + li;
        if (kk < a.K && n < d.Ng) ws[(int64_t)kk * d.Ng + n] = h ? acc1[v] : acc0[v];
      }
  }
}

// dW_g[i] = sum over slabs s = 0, 1, ... of ws[s][g][i] (ascending: the same order in every run)
__global__ __launch_bounds__(256) void gconv_wgrad_sum_kernel(const float* __restrict__ ws, float* __restrict__ dW, int64_t per_group,
                                                             int g, int S, int64_t wgs) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int grp = blockIdx.y;
  if (i >= per_group) return;
  const int64_t slab = (int64_t)g * per_group;
  const float* src = ws + (int64_t)grp * per_group + i;
  float s = 0.f;
  for (int k = 0; k < S; ++k) s += src[k * slab];
  dW[(int64_t)grp * wgs + i] = s;
}

struct WgPlan {
  int k_tiles, n_tiles, S;
  int64_t chunk;
};
WgPlan wgrad_plan(const kws_gconv_t* d) {
  WgPlan pl;
  const int K = d->k * d->gs;
  const int64_t M = (int64_t)d->B * d->Lout;
  pl.k_tiles = ceil_div(K, GC_BM);
  pl.n_tiles = ceil_div(d->Ng, GC_BN);
  const int tiles = pl.k_tiles * pl.n_tiles * d->g;
  int64_t S = ceil_div64(GC_WG_TARGET, tiles);
  const int64_t max_s = ceil_div64(M, 4 * GC_BK);   // at least 64 rows per slab
  if (S > max_s) S = max_s;
  if (S < 1) S = 1;
  pl.chunk = ceil_div64(ceil_div64(M, S), GC_BK) * GC_BK;
  pl.S = (int)ceil_div64(M, pl.chunk);
  return pl;
}

int check_desc(const kws_gconv_t* d) {
  KWS_REQUIRE(d != nullptr, "gconv: descriptor is NULL");
  KWS_REQUIRE(d->B > 0 && d->L > 0 && d->C > 0 && d->Lout > 0 && d->k > 0 && d->stride > 0 && d->g > 0 && d->gs > 0 &&
                  d->Ng > 0,
              "gconv: B=%d L=%d C=%d Lout=%d k=%d stride=%d g=%d gs=%d Ng=%d must be positive", d->B, d->L, d->C, d->Lout,
              d->k, d->stride, d->g, d->gs, d->Ng);
  KWS_REQUIRE((int64_t)d->stride * (d->Lout - 1) + d->k <= d->L, "gconv: Lout=%d windows of %d taps, stride %d, exceed L=%d",
              d->Lout, d->k, d->stride, d->L);
  KWS_REQUIRE((int64_t)d->g * d->gs <= d->C, "gconv: %d groups of %d channels exceed C=%d", d->g, d->gs, d->C);
  KWS_REQUIRE(d->g <= 65535 && d->stride * ceil_div(d->gs, GC_BN) <= 65535, "gconv: grid too large");
  KWS_REQUIRE(d->w_group_stride == 0 || d->w_group_stride >= (int64_t)d->k * d->gs * d->Ng,
              "gconv: w_group_stride %lld < one group's kernel", (long long)d->w_group_stride);
  KWS_REQUIRE((int64_t)d->B * d->L * d->C < (1ll << 40) && ceil_div64((int64_t)d->B * d->Lout, GC_BM) < (1ll << 31),
              "gconv: tensor too large");
  return KWS_OK;
}

int check_bn(const float* bn, int bg, const kws_gconv_t* d) {
  KWS_REQUIRE(bn == nullptr || (bg > 0 && d->C % bg == 0), "gconv: bn_group %d must divide C=%d", bg, d->C);
  return KWS_OK;
}

int64_t wstride(const kws_gconv_t* d) { return d->w_group_stride ? d->w_group_stride : (int64_t)d->k * d->gs * d->Ng; }

// ---- Flatten -> Dropout -> Dense(bias) -> softmax -> keras categorical_crossentropy (conv_1d_fast / conv_1d_spec) ------
// One workgroup per clip.  Features are relu6(bn(y)) of the last grouped block in Keras Flatten order (t * F + f); the
// dropout element index of row r is r * D + i (layer_id 1 unless the caller names another), as in the other tails.  bd may
// be NULL (conv_1d_heavy's Conv1D(num_classes, 1, use_bias=False) head over its [B, 1, 128] features).  Training also writes the dropped
// features fd [B, D], dlogits dl [B, NC] and the gradient wrt the activated block output dA [B, D].
constexpr int FT_MAXD = 8192, FT_MAXNC = 64;
struct FtArgs {
  const float* y; const float* bn; int Ng;   // block output (pre-BN) and its per-group tables
  const float* Wd; const float* bd; const float* labels;
  float* probs; float* fd; float* dl; float* dA; float* per_loss; float* per_correct;
  int B, D, F, NC;
  uint32_t key, thresh; float inv_keep, inv_loss_batch; int64_t row_offset;
};
// RAW (conv_1d_simple's head behind the GRU): the features are y as it is - signed, no table, no dropout
template <bool TRAIN, bool RAW = false>
__global__ __launch_bounds__(256) void flat_tail_kernel(FtArgs a) {
  __shared__ float s_feat[FT_MAXD], s_red[4][FT_MAXNC], s_p[FT_MAXNC], s_dl[FT_MAXNC];
  const int b = blockIdx.x, tid = threadIdx.x, D = a.D, NC = a.NC;
  const uint32_t row = (uint32_t)(a.row_offset + b);
  const float* yb = a.y + (int64_t)b * D;
  for (int i = tid; i < D; i += 256) {
    float f;
    if (RAW) {
      f = yb[i];
    } else {
      const int c = i % a.F, grp = c / a.Ng, n = c - grp * a.Ng;
      const float* t = a.bn + (int64_t)grp * 4 * a.Ng;
      f = relu6f(fmaf(yb[i], t[n], t[a.Ng + n]));
    }
    if (TRAIN) {
      if (!RAW) f = kws_keep(row * (uint32_t)D + (uint32_t)i, a.key, a.thresh) ? f * a.inv_keep : 0.f;
      a.fd[(int64_t)b * D + i] = f;
    }
    s_feat[i] = f;
  }
  __syncthreads();
  {
    const int k = tid & 63, sl = tid >> 6;
    float s = 0.f;
    if (k < NC)
      for (int i = sl; i < D; i += 4) s = fmaf(s_feat[i], a.Wd[(int64_t)i * NC + k], s);
    s_red[sl][k] = s;
    __syncthreads();
    if (tid < NC) {
      const float dot = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
      s_p[tid] = a.bd ? dot + a.bd[tid] : dot;
    }
    __syncthreads();
    if (tid == 0) {
      float mx = s_p[0];
      for (int q = 1; q < NC; ++q) mx = fmaxf(mx, s_p[q]);
      float den = 0.f;
      for (int q = 0; q < NC; ++q) {
        s_p[q] = expf(s_p[q] - mx);
        den += s_p[q];
      }
      for (int q = 0; q < NC; ++q) s_p[q] /= den;
    }
    __syncthreads();
    if (tid < NC) a.probs[(int64_t)b * NC + tid] = s_p[tid];
  }
  if (!TRAIN) return;
  if (tid == 0) {
    // keras categorical_crossentropy: p /= sum(p); clip(eps, 1 - eps); -sum(y log p); gradient back through the softmax
    const float eps = 1e-7f;
    const float* yl = a.labels + (int64_t)b * NC;
    int am_p = 0, am_y = 0;
    float loss = 0.f, S = 0.f, dotp = 0.f;
    for (int q = 0; q < NC; ++q) S += s_p[q];
    for (int q = 0; q < NC; ++q) {
      const float pn = s_p[q] / S;
      const float pc = fminf(fmaxf(pn, eps), 1.f - eps);
      loss -= yl[q] * logf(pc);
      const float inside = (pn >= eps && pn <= 1.f - eps) ? 1.f : 0.f;
      const float dpn = (-yl[q] / pc) * inside * a.inv_loss_batch;
      s_dl[q] = dpn;
      dotp += dpn * s_p[q];
      if (s_p[q] > s_p[am_p]) am_p = q;
      if (yl[q] > yl[am_y]) am_y = q;
    }
    float dot2 = 0.f;
    for (int q = 0; q < NC; ++q) {
      const float dp = s_dl[q] / S - dotp / (S * S);
      s_dl[q] = dp;
      dot2 += dp * s_p[q];
    }
    for (int q = 0; q < NC; ++q) s_dl[q] = s_p[q] * (s_dl[q] - dot2);
    a.per_loss[b] = loss;
    a.per_correct[b] = (am_p == am_y) ? 1.f : 0.f;
  }
  __syncthreads();
  if (tid < NC) a.dl[(int64_t)b * NC + tid] = s_dl[tid];
  for (int i = tid; i < D; i += 256) {
    float dv = 0.f;
    for (int q = 0; q < NC; ++q) dv = fmaf(a.Wd[(int64_t)i * NC + q], s_dl[q], dv);
    a.dA[(int64_t)b * D + i] = RAW ? dv : kws_keep(row * (uint32_t)D + (uint32_t)i, a.key, a.thresh) ? dv * a.inv_keep : 0.f;
  }
}

}  // namespace

// ---- internal launchers (net_grouped.hip) ----------------------------------------------------------------------------------
int kws_flat_tail_launch(const kws_flat_tail_args* t, int training, hipStream_t st) {
  KWS_REQUIRE(t && t->y && (t->bn || t->raw) && t->Wd && t->probs && t->B > 0 && t->D > 0 && t->D <= FT_MAXD && t->F > 0 &&
                  t->D % t->F == 0 && t->Ng > 0 && t->F % t->Ng == 0 && t->NC > 0 && t->NC <= FT_MAXNC,
              "flat_tail: bad arguments (D=%d F=%d NC=%d)", t ? t->D : 0, t ? t->F : 0, t ? t->NC : 0);
  KWS_REQUIRE(!training || (t->labels && t->fd && t->dl && t->dA && t->per_loss && t->per_correct),
              "flat_tail: training needs labels, fd, dl, dA, per_loss, per_correct");
  FtArgs a;
  a.y = t->y; a.bn = t->bn; a.Ng = t->Ng; a.Wd = t->Wd; a.bd = t->bd; a.labels = t->labels;
  a.probs = t->probs; a.fd = t->fd; a.dl = t->dl; a.dA = t->dA; a.per_loss = t->per_loss; a.per_correct = t->per_correct;
  a.B = t->B; a.D = t->D; a.F = t->F; a.NC = t->NC;
  a.key = kws_dropout_key(t->seed, t->step, t->layer_id ? t->layer_id : 1);
  a.thresh = kws_dropout_threshold(t->keep_prob);
  a.inv_keep = (float)(1.0 / (double)t->keep_prob);
  a.inv_loss_batch = 1.0f / (float)(t->loss_batch > 0 ? t->loss_batch : 1);
  a.row_offset = t->row_offset;
  KwsProfScope prof("flat_tail", 2.0 * t->B * t->D * t->NC * (training ? 2.0 : 1.0), 4.0 * (double)t->B * t->D * (training ? 3.0 : 1.0), st);
  if (t->raw && training) hipLaunchKernelGGL((flat_tail_kernel<true, true>), dim3((unsigned)t->B), dim3(256), 0, st, a);
  else if (t->raw) hipLaunchKernelGGL((flat_tail_kernel<false, true>), dim3((unsigned)t->B), dim3(256), 0, st, a);
  else if (training) hipLaunchKernelGGL((flat_tail_kernel<true>), dim3((unsigned)t->B), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((flat_tail_kernel<false>), dim3((unsigned)t->B), dim3(256), 0, st, a);
  KWS_LAUNCH_CHECK("flat_tail_kernel");
  return KWS_OK;
}

extern "C" {

int kws_gconv_stats_rows(const kws_gconv_t* d) { return d ? (int)ceil_div64((int64_t)d->B * d->Lout, GC_BM) : 0; }

int kws_gconv_fwd_f32(const float* X, const float* bn, int bn_group, const float* W, float* Y, float* stats_part,
                      const kws_gconv_t* d, void* stream) {
  KWS_TRY(check_desc(d));
  KWS_TRY(check_bn(bn, bn_group, d));
  KWS_REQUIRE(X && W && Y, "gconv_fwd: NULL pointer");
  GcArgs a{};
  a.d = *d; a.wgs = wstride(d); a.X = X; a.bn = bn; a.bg = bn_group; a.W = W; a.out = Y; a.stats = stats_part;
  a.M = (int64_t)d->B * d->Lout; a.K = d->k * d->gs; a.n_tiles = ceil_div(d->Ng, GC_BN);
  const double flops = 2.0 * a.M * a.K * d->Ng * d->g;
  KwsProfScope prof("gconv_fwd", flops, 4.0 * ((double)d->B * d->L * d->C + (double)a.K * d->Ng * d->g + (double)a.M * d->Ng * d->g),
                    (hipStream_t)stream);
  hipLaunchKernelGGL((gconv_kernel<GC_FWD>), dim3((unsigned)ceil_div64(a.M, GC_BM), (unsigned)a.n_tiles, (unsigned)d->g), dim3(256), 0,
                     (hipStream_t)stream, a);
  KWS_LAUNCH_CHECK("gconv_kernel<fwd>");
  return KWS_OK;
}

int kws_gconv_dgrad_f32(const float* dY, const float* W, float* dX, const kws_gconv_t* d, void* stream) {
  KWS_TRY(check_desc(d));
  KWS_REQUIRE(dY && W && dX, "gconv_dgrad: NULL pointer");
  GcArgs a{};
  a.d = *d; a.wgs = wstride(d); a.W = W; a.dY = dY; a.out = dX;
  a.Q = ceil_div(d->L, d->stride);
  a.M = (int64_t)d->B * a.Q;
  a.n_tiles = ceil_div(d->gs, GC_BN);
  const double flops = 2.0 * d->B * d->Lout * (double)d->k * d->gs * d->Ng * d->g;
  KwsProfScope prof("gconv_dgrad", flops,
                    4.0 * ((double)d->B * d->L * d->C + (double)d->k * d->gs * d->Ng * d->g + (double)d->B * d->Lout * d->Ng * d->g),
                    (hipStream_t)stream);
  const int gz = d->g + (d->C > d->g * d->gs ? 1 : 0);
  hipLaunchKernelGGL((gconv_kernel<GC_DGRAD>), dim3((unsigned)ceil_div64(a.M, GC_BM), (unsigned)(d->stride * a.n_tiles), (unsigned)gz),
                     dim3(256), 0, (hipStream_t)stream, a);
  KWS_LAUNCH_CHECK("gconv_kernel<dgrad>");
  return KWS_OK;
}

int64_t kws_gconv_wgrad_workspace_floats(const kws_gconv_t* d) {
  if (check_desc(d) != KWS_OK) return 0;
  const WgPlan pl = wgrad_plan(d);
  return (int64_t)pl.S * d->g * d->k * d->gs * d->Ng;
}

int kws_gconv_wgrad_f32(const float* X, const float* bn, int bn_group, const float* dY, float* dW, float* workspace,
                        const kws_gconv_t* d, void* stream) {
  KWS_TRY(check_desc(d));
  KWS_TRY(check_bn(bn, bn_group, d));
  KWS_REQUIRE(X && dY && dW && workspace, "gconv_wgrad: NULL pointer");
  const WgPlan pl = wgrad_plan(d);
  GcArgs a{};
  a.d = *d; a.wgs = wstride(d); a.X = X; a.bn = bn; a.bg = bn_group; a.dY = dY; a.out = workspace;
  a.M = (int64_t)d->B * d->Lout; a.K = d->k * d->gs; a.n_tiles = pl.n_tiles; a.chunk = pl.chunk;
  KWS_REQUIRE(pl.S <= 65535, "gconv_wgrad: %d slabs", pl.S);
  const double flops = 2.0 * a.M * a.K * d->Ng * d->g;
  KwsProfScope prof("gconv_wgrad", flops,
                    4.0 * ((double)d->B * d->L * d->C + (double)a.M * d->Ng * d->g + (double)(pl.S + 1) * a.K * d->Ng * d->g),
                    (hipStream_t)stream);
  hipLaunchKernelGGL((gconv_kernel<GC_WGRAD>), dim3((unsigned)(pl.k_tiles * pl.n_tiles), (unsigned)pl.S, (unsigned)d->g), dim3(256), 0,
                     (hipStream_t)stream, a);
  KWS_LAUNCH_CHECK("gconv_kernel<wgrad>");
  const int64_t per_group = (int64_t)a.K * d->Ng;
  hipLaunchKernelGGL(gconv_wgrad_sum_kernel, dim3((unsigned)ceil_div64(per_group, 256), (unsigned)d->g), dim3(256), 0, (hipStream_t)stream,
                     workspace, dW, per_group, d->g, pl.S, a.wgs);
  KWS_LAUNCH_CHECK("gconv_wgrad_sum_kernel");
  return KWS_OK;
}

}  // extern "C"
