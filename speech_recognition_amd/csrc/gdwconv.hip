// Grouped depthwise Conv1D (VALID, k taps, time stride s, g groups over channel WINDOWS of one tensor): the depthwise half of
// the g _depthwise_conv_block calls the reference makes inside _grouped_reduce_conv / _grouped_context_conv of
// conv_1d_top_down_model (model.py:1335-1373).  Group q owns a kernel [k, gs] at w + q * w_group_stride and reads the channels
// [x0 + q * x_step, + gs) of X [B, L, C]; its output is the columns [q * gs, + gs) of Z [B, Lout, g * gs], which a grouped 1x1
// convolution (kws_gconv_* with k = 1) consumes.  x_step = gs is the sliced form (a reduce block: every group its own slice);
// x_step = 0 the shared form (a context block: the reference hands x, not the slice, to every group, so each group filters ALL
// channels with its own kernel).  Channels outside every window are never read.
//   forward   Z[b,t,q*gs+c] = sum_j w_q[j,c] * act(X[b, s*t+j, x0+q*x_step+c]).  One thread per (row, 4 channels): 16-byte loads
//             and stores, adjacent lanes on adjacent vectors.  Shared form: the k input vectors are loaded and activated ONCE
//             and all g groups' outputs come from them.
//   backward  dA[b,u,ch] = sum over the groups q whose window holds ch (ascending), over the taps j (ascending) with
//             s | (u - j), of w_q[j,c] * dZ[b,(u-j)/s,q*gs+c]: the gradient wrt act(X), no gate (kws_gconv_dgrad_f32's contract).
//             One thread per (input row, 4 channels of C) writes its element once: rows no window reaches and channels no
//             group reads come out as exact zeros, without a clearing pass.
//             dw_q[j,c] = sum_{b,t} act(X[b,s*t+j,...]) * dZ[b,t,q*gs+c]: P row chunks x 64-vector column tiles; a block's four
//             row lanes add their rows ascending, are folded 0..3 through LDS into ONE partial row [k + 1][g*gs] (row k: the
//             column sums of dZ), and a fold kernel adds the P rows in one fixed order (16 lanes per element, each its rows ascending, then the lanes
//             ascending) straight into each group's tensor.  In bias mode
//             the same fold gives dbias[ch] = sum_q sum_j w_q[j,c] * colsum(dZ)[q*gs+c] - the column sum of dA, since every
//             (t, j) of a VALID convolution lands on a row of dA.
// act: identity | relu6(scale * x + shift) of the producer's grouped table [C / bn_group][4][bn_group], indexed per channel (a
// 4-channel vector may straddle two table groups) | x + bias[ch].  No atomics anywhere: bit-identical from run to run.
// Weights, tables and biases are read as scalars (they live at arbitrary float offsets of the parameter buffer); X, Z, dZ, dA and
// the workspace must be 16-byte aligned.
#include <algorithm>

#include "common.h"
#include "internal.h"

namespace {

constexpr int GDW_MAXK = 7, GDW_MAXS = 4, GDW_MAXG = 8;
constexpr int GDW_CT = 64;             // column vectors per block of the weight-gradient pass (x 4 row lanes = 256 threads)
constexpr int GDW_WG_TARGET = 1024;    // weight gradient: workgroups aimed for (column tiles x partial rows)
constexpr int GDW_MIN_CHUNK = 16;      // rows per partial row, at least
constexpr unsigned GDW_MAX_GRID = 8192;

struct GdwArgs {
  kws_gdwconv_t d;
  int64_t wgs;        // floats between consecutive groups' kernels
  const float* X;
  const float* tab;   // table (act 1) or bias (act 2)
  const float* w;
  const float* dZ;
  float* out;         // fwd: Z; bwd: dA
  float* part;        // [P][k + 1][g * gs]
  float* dW;
  float* dbias;
  int64_t M;          // B * Lout
  int64_t chunk;      // rows per partial row
  int P;
};

struct GdwAct {
  float sc[4], sh[4];
};

// what act() needs for the channels ch .. ch + 3
__device__ __forceinline__ GdwAct gdw_act_load(const GdwArgs& a, int ch) {
  GdwAct t;
  if (a.d.act == KWS_GDW_ACT_BN_RELU6) {
    const int bg = a.d.bn_group;
    int l = ch / bg, n = ch - l * bg;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      while (n >= bg) {
        n -= bg;
        ++l;
      }
      const float* row = a.tab + (int64_t)l * 4 * bg;
      t.sc[e] = row[n];
      t.sh[e] = row[bg + n];
      ++n;
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      t.sc[e] = 1.f;
      t.sh[e] = a.d.act == KWS_GDW_ACT_BIAS ? a.tab[ch + e] : 0.f;
    }
  }
  return t;
}

__device__ __forceinline__ float4 gdw_act(float4 v, const GdwAct& t, int act) {
  if (act == KWS_GDW_ACT_BN_RELU6) {
    v.x = relu6f(fmaf(v.x, t.sc[0], t.sh[0]));
    v.y = relu6f(fmaf(v.y, t.sc[1], t.sh[1]));
    v.z = relu6f(fmaf(v.z, t.sc[2], t.sh[2]));
    v.w = relu6f(fmaf(v.w, t.sc[3], t.sh[3]));
  } else if (act == KWS_GDW_ACT_BIAS) {
    v.x += t.sh[0];
    v.y += t.sh[1];
    v.z += t.sh[2];
    v.w += t.sh[3];
  }
  return v;
}

__device__ __forceinline__ float4 gdw_fma(const float* w, float4 x, float4 acc) {
  acc.x = fmaf(w[0], x.x, acc.x);
  acc.y = fmaf(w[1], x.y, acc.y);
  acc.z = fmaf(w[2], x.z, acc.z);
  acc.w = fmaf(w[3], x.w, acc.w);
  return acc;
}

__global__ __launch_bounds__(256) void gdw_fwd_kernel(GdwArgs a) {
  const kws_gdwconv_t& d = a.d;
  const int gv = d.gs >> 2, Fz = d.g * d.gs;
  const bool shared = d.x_step == 0;
  const int units = shared ? gv : d.g * gv;   // per output row: a unit is 4 channels of one group (shared: of all groups)
  const int nq = shared ? d.g : 1;
  const int64_t total = a.M * units;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int64_t m = idx / units;
    const int u = (int)(idx - m * units);
    const int64_t b = m / d.Lout;
    const int t = (int)(m - b * d.Lout);
    const int q0 = shared ? 0 : u / gv;
    const int c = (u - q0 * gv) << 2;
    const int ch = d.x0 + q0 * d.x_step + c;
    const GdwAct tb = gdw_act_load(a, ch);
    const float* xp = a.X + (b * d.L + (int64_t)t * d.stride) * d.C + ch;
    float4 xs[GDW_MAXK];
#pragma unroll
    for (int j = 0; j < GDW_MAXK; ++j)
      if (j < d.k) xs[j] = gdw_act(*reinterpret_cast<const float4*>(xp + (int64_t)j * d.C), tb, d.act);
    for (int qq = 0; qq < nq; ++qq) {
      const int q = q0 + qq;
      const float* wq = a.w + (int64_t)q * a.wgs + c;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int j = 0; j < GDW_MAXK; ++j)
        if (j < d.k) acc = gdw_fma(wq + j * d.gs, xs[j], acc);
      *reinterpret_cast<float4*>(a.out + m * Fz + q * d.gs + c) = acc;
    }
  }
}

__global__ __launch_bounds__(256) void gdw_dgrad_kernel(GdwArgs a) {
  const kws_gdwconv_t& d = a.d;
  const int cv = d.C >> 2, Fz = d.g * d.gs;
  const int64_t total = (int64_t)d.B * d.L * cv;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int64_t row = idx / cv;
    const int ch = (int)(idx - row * cv) << 2;
    const int64_t b = row / d.L;
    const int u = (int)(row - b * d.L);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int q = 0; q < d.g; ++q) {
      const int c = ch - (d.x0 + q * d.x_step);
      if (c < 0 || c >= d.gs) continue;
      const float* wq = a.w + (int64_t)q * a.wgs + c;
      const float* dz = a.dZ + b * d.Lout * Fz + q * d.gs + c;
#pragma unroll
      for (int j = 0; j < GDW_MAXK; ++j) {
        const int r = u - j;
        if (j >= d.k || r < 0) continue;
        const int t = r / d.stride;
        if (t * d.stride != r || t >= d.Lout) continue;
        acc = gdw_fma(wq + j * d.gs, *reinterpret_cast<const float4*>(dz + (int64_t)t * Fz), acc);
      }
    }
    *reinterpret_cast<float4*>(a.out + row * d.C + ch) = acc;
  }
}

// grid (column tiles, P): block y adds the rows [y * chunk, (y + 1) * chunk) of its 64 column vectors into partial row y
__global__ __launch_bounds__(256) void gdw_wgrad_part_kernel(GdwArgs a) {
  __shared__ float4 red[3][GDW_CT][GDW_MAXK + 1];
  const kws_gdwconv_t& d = a.d;
  const int gv = d.gs >> 2, Fz = d.g * d.gs, nv = Fz >> 2;
  const int lane = threadIdx.x & (GDW_CT - 1), rl = threadIdx.x / GDW_CT;
  const int v = blockIdx.x * GDW_CT + lane;
  const bool on = v < nv;
  float4 acc[GDW_MAXK + 1];
#pragma unroll
  for (int j = 0; j <= GDW_MAXK; ++j) acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (on) {
    const int q = v / gv, c = (v - q * gv) << 2;
    const int ch = d.x0 + q * d.x_step + c;
    const GdwAct tb = gdw_act_load(a, ch);
    const int64_t m0 = (int64_t)blockIdx.y * a.chunk;
    const int64_t m1 = m0 + a.chunk < a.M ? m0 + a.chunk : a.M;
    for (int64_t m = m0 + rl; m < m1; m += 4) {
      const int64_t b = m / d.Lout;
      const int t = (int)(m - b * d.Lout);
      const float4 dz = *reinterpret_cast<const float4*>(a.dZ + m * Fz + (v << 2));
      const float* xp = a.X + (b * d.L + (int64_t)t * d.stride) * d.C + ch;
#pragma unroll
      for (int j = 0; j < GDW_MAXK; ++j)
        if (j < d.k) {
          const float4 x = gdw_act(*reinterpret_cast<const float4*>(xp + (int64_t)j * d.C), tb, d.act);
          acc[j].x = fmaf(x.x, dz.x, acc[j].x);
          acc[j].y = fmaf(x.y, dz.y, acc[j].y);
          acc[j].z = fmaf(x.z, dz.z, acc[j].z);
          acc[j].w = fmaf(x.w, dz.w, acc[j].w);
        }
      acc[GDW_MAXK].x += dz.x;
      acc[GDW_MAXK].y += dz.y;
      acc[GDW_MAXK].z += dz.z;
      acc[GDW_MAXK].w += dz.w;
    }
  }
  if (rl > 0) {
#pragma unroll
    for (int j = 0; j <= GDW_MAXK; ++j) red[rl - 1][lane][j] = acc[j];
  }
  __syncthreads();
  if (rl == 0 && on) {
    float* prow = a.part + (int64_t)blockIdx.y * (d.k + 1) * Fz + (v << 2);
#pragma unroll
    for (int j = 0; j <= GDW_MAXK; ++j) {
      if (j < d.k || j == GDW_MAXK) {
        float4 s = acc[j];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const float4 o = red[r][lane][j];
          s.x += o.x;
          s.y += o.y;
          s.z += o.z;
          s.w += o.w;
        }
        *reinterpret_cast<float4*>(prow + (int64_t)(j < d.k ? j : d.k) * Fz) = s;
      }
    }
  }
}

// Sum of column i over the P partial rows, by the 16 lanes of one element slot: lane l adds the rows l, l + 16, ... ascending, then
// lane 0 adds the lanes' sums 0 .. 15 ascending - one fixed order whatever P is.  All 64 lanes of the wave call it together.
__device__ __forceinline__ float gdw_fold16(const float* __restrict__ col, int64_t rowf, int P, int lane, bool on) {
  float s = 0.f;
  if (on) {
#pragma unroll 4
    for (int p = lane; p < P; p += 16) s += col[p * rowf];
  }
  float tot = __shfl(s, 0, 16);
#pragma unroll
  for (int l = 1; l < 16; ++l) tot += __shfl(s, l, 16);
  return tot;
}

// blocks [0, dw_blocks): 16 elements of dw each (dw_q[j][c] = the partial rows added in gdw_fold16's order); the blocks behind them,
// when dbias is asked for: 16 channels each, dbias[ch] = sum over the groups holding ch (ascending) of (sum_j w_q[j][c]) * colsum
__global__ __launch_bounds__(256) void gdw_wgrad_fold_kernel(GdwArgs a, int dw_blocks) {
  const kws_gdwconv_t& d = a.d;
  const int Fz = d.g * d.gs;
  const int64_t rowf = (int64_t)(d.k + 1) * Fz;
  const int slot = threadIdx.x >> 4, lane = threadIdx.x & 15;
  if ((int)blockIdx.x < dw_blocks) {
    const int i = blockIdx.x * 16 + slot;
    const bool on = i < d.k * Fz;
    const float s = gdw_fold16(a.part + i, rowf, a.P, lane, on);
    if (on && lane == 0) {
      const int j = i / Fz, col = i - j * Fz;
      const int q = col / d.gs, c = col - q * d.gs;
      a.dW[(int64_t)q * a.wgs + j * d.gs + c] = s;
    }
    return;
  }
  const int ch = ((int)blockIdx.x - dw_blocks) * 16 + slot;
  float db = 0.f;
  for (int q = 0; q < d.g; ++q) {
    const int c = ch - (d.x0 + q * d.x_step);
    const bool on = ch < d.C && c >= 0 && c < d.gs;
    const float s = gdw_fold16(a.part + (int64_t)d.k * Fz + q * d.gs + (on ? c : 0), rowf, a.P, lane, on);
    if (on && lane == 0) {
      float wsum = 0.f;
      for (int j = 0; j < d.k; ++j) wsum += a.w[(int64_t)q * a.wgs + j * d.gs + c];
      db = fmaf(wsum, s, db);
    }
  }
  if (ch < d.C && lane == 0) a.dbias[ch] = db;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

int check_desc(const kws_gdwconv_t* d) {
  KWS_REQUIRE(d != nullptr, "gdwconv: descriptor is NULL");
  KWS_REQUIRE(d->B > 0 && d->L > 0 && d->C > 0 && d->Lout > 0 && d->gs > 0, "gdwconv: B=%d L=%d C=%d Lout=%d gs=%d must be positive", d->B,
              d->L, d->C, d->Lout, d->gs);
  KWS_REQUIRE(d->k >= 1 && d->k <= GDW_MAXK && d->stride >= 1 && d->stride <= GDW_MAXS && d->g >= 1 && d->g <= GDW_MAXG,
              "gdwconv: k=%d (1..%d) stride=%d (1..%d) g=%d (1..%d)", d->k, GDW_MAXK, d->stride, GDW_MAXS, d->g, GDW_MAXG);
  KWS_REQUIRE(d->gs % 4 == 0 && d->C % 4 == 0 && d->x0 >= 0 && d->x0 % 4 == 0 && d->x_step >= 0 && d->x_step % 4 == 0,
              "gdwconv: gs=%d C=%d x0=%d x_step=%d must be multiples of 4", d->gs, d->C, d->x0, d->x_step);
  KWS_REQUIRE((int64_t)d->x0 + (int64_t)(d->g - 1) * d->x_step + d->gs <= d->C, "gdwconv: window %d + %d * %d + %d exceeds C=%d", d->x0,
              d->g - 1, d->x_step, d->gs, d->C);
  KWS_REQUIRE((int64_t)d->stride * (d->Lout - 1) + d->k <= d->L, "gdwconv: Lout=%d windows of %d taps, stride %d, exceed L=%d", d->Lout,
              d->k, d->stride, d->L);
  KWS_REQUIRE(d->act == KWS_GDW_ACT_NONE || d->act == KWS_GDW_ACT_BIAS || (d->act == KWS_GDW_ACT_BN_RELU6 && d->bn_group > 0 &&
                                                                            d->C % d->bn_group == 0),
              "gdwconv: act=%d bn_group=%d (must divide C=%d)", d->act, d->bn_group, d->C);
  KWS_REQUIRE(d->w_group_stride == 0 || d->w_group_stride >= (int64_t)d->k * d->gs, "gdwconv: w_group_stride %lld < one group's kernel",
              (long long)d->w_group_stride);
  KWS_REQUIRE((int64_t)d->B * d->L * d->C < (1ll << 40) && (int64_t)d->B * d->Lout * d->g * d->gs < (1ll << 40), "gdwconv: tensor too large");
  return KWS_OK;
}

int64_t wstride(const kws_gdwconv_t* d) { return d->w_group_stride ? d->w_group_stride : (int64_t)d->k * d->gs; }

struct GdwPlan {
  int col_tiles, P;
  int64_t chunk;
};
GdwPlan wgrad_plan(const kws_gdwconv_t* d) {
  GdwPlan pl;
  const int64_t M = (int64_t)d->B * d->Lout;
  pl.col_tiles = ceil_div(d->g * d->gs / 4, GDW_CT);
  const int64_t max_p = std::max<int64_t>(1, GDW_WG_TARGET / pl.col_tiles);
  pl.chunk = std::max<int64_t>(GDW_MIN_CHUNK, ceil_div64(ceil_div64(M, max_p), 4) * 4);
  pl.P = (int)ceil_div64(M, pl.chunk);
  return pl;
}

unsigned grid_for(int64_t threads) { return (unsigned)std::min<int64_t>(ceil_div64(threads, 256), GDW_MAX_GRID); }

GdwArgs make_args(const kws_gdwconv_t* d) {
  GdwArgs a{};
  a.d = *d;
  a.wgs = wstride(d);
  a.M = (int64_t)d->B * d->Lout;
  return a;
}

}  // namespace

extern "C" {

int kws_gdwconv_fwd_f32(const float* X, const float* tab, const float* w, float* Z, const kws_gdwconv_t* d, void* stream) {
  KWS_TRY(check_desc(d));
  KWS_REQUIRE(X && w && Z && (tab || d->act == KWS_GDW_ACT_NONE), "gdwconv_fwd: NULL pointer");
  KWS_REQUIRE(aligned16(X) && aligned16(Z), "gdwconv_fwd: X and Z must be 16-byte aligned");
  GdwArgs a = make_args(d);
  a.X = X; a.tab = tab; a.w = w; a.out = Z;
  const int windows = d->x_step == 0 ? 1 : d->g;
  const int64_t threads = a.M * windows * (d->gs / 4);
  KwsProfScope prof("gdwconv_fwd", 2.0 * a.M * d->g * d->gs * d->k,
                    4.0 * ((double)d->B * d->L * windows * d->gs + (double)a.M * d->g * d->gs), (hipStream_t)stream);
  hipLaunchKernelGGL(gdw_fwd_kernel, dim3(grid_for(threads)), dim3(256), 0, (hipStream_t)stream, a);
  KWS_LAUNCH_CHECK("gdw_fwd_kernel");
  return KWS_OK;
}

int kws_gdwconv_bwd_part_rows(const kws_gdwconv_t* d) {
  if (check_desc(d) != KWS_OK) return 0;
  return wgrad_plan(d).P;
}

int64_t kws_gdwconv_bwd_workspace_floats(const kws_gdwconv_t* d) {
  if (check_desc(d) != KWS_OK) return 0;
  return (int64_t)wgrad_plan(d).P * (d->k + 1) * d->g * d->gs;
}

int kws_gdwconv_bwd_f32(const float* X, const float* tab, const float* dZ, const float* w, float* dA, float* dW, float* dbias,
                        float* workspace, const kws_gdwconv_t* d, void* stream) {
  KWS_TRY(check_desc(d));
  KWS_REQUIRE(X && dZ && w && dA && dW && workspace && (tab || d->act == KWS_GDW_ACT_NONE), "gdwconv_bwd: NULL pointer");
  KWS_REQUIRE(dbias == nullptr || d->act == KWS_GDW_ACT_BIAS, "gdwconv_bwd: dbias needs the bias mode (act=%d)", d->act);
  KWS_REQUIRE(aligned16(X) && aligned16(dZ) && aligned16(dA) && aligned16(workspace),
              "gdwconv_bwd: X, dZ, dA and the workspace must be 16-byte aligned");
  const GdwPlan pl = wgrad_plan(d);
  GdwArgs a = make_args(d);
  a.X = X; a.tab = tab; a.dZ = dZ; a.w = w; a.out = dA; a.part = workspace; a.dW = dW; a.dbias = dbias;
  a.chunk = pl.chunk; a.P = pl.P;
  const int Fz = d->g * d->gs;
  const int windows = d->x_step == 0 ? 1 : d->g;
  KwsProfScope prof("gdwconv_bwd", 4.0 * a.M * Fz * d->k,
                    4.0 * ((double)d->B * d->L * d->C + (double)d->B * d->L * windows * d->gs + 2.0 * (double)a.M * Fz), (hipStream_t)stream);
  hipLaunchKernelGGL(gdw_dgrad_kernel, dim3(grid_for((int64_t)d->B * d->L * (d->C / 4))), dim3(256), 0, (hipStream_t)stream, a);
  KWS_LAUNCH_CHECK("gdw_dgrad_kernel");
  hipLaunchKernelGGL(gdw_wgrad_part_kernel, dim3((unsigned)pl.col_tiles, (unsigned)pl.P), dim3(256), 0, (hipStream_t)stream, a);
  KWS_LAUNCH_CHECK("gdw_wgrad_part_kernel");
  const int dw_blocks = ceil_div(d->k * Fz, 16);
  hipLaunchKernelGGL(gdw_wgrad_fold_kernel, dim3((unsigned)(dw_blocks + (dbias ? ceil_div(d->C, 16) : 0))), dim3(256), 0,
                     (hipStream_t)stream, a, dw_blocks);
  KWS_LAUNCH_CHECK("gdw_wgrad_fold_kernel");
  return KWS_OK;
}

}  // extern "C"
