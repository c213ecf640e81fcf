// Attention gate in front of a recurrent layer (kws_attn_gate_*): xception_with_attention, reference model.py:973-975
//   attention = _context_conv(x, 1, k, padding='same')   DepthwiseConv2D((1, k)) -> Conv1D(1, 1) -> BatchNormalization -> relu6
//   attention = softmax(attention, axis=1)               over TIME
//   y = x * attention                                    [B, T, C] * [B, T, 1]: the sequence the GRU reads
// Everything here streams x / dy; what orders the passes is the one-channel BatchNorm, whose batch statistics (forward) and
// two batch sums (backward) are reductions over all B T positions: two passes over the tensors each way is the minimum.
//   forward   ag_logits_kernel   reads x once: u [B, T] and the per-clip sums of u                    B T C 4 bytes
//             ag_bn_*_kernel     one workgroup: table [4] = scale | shift | mean | rstd (two-pass variance over u), moving statistics
//             ag_apply_kernel    att = softmax_t(relu6(scale u + shift)); reads x, writes y           2 B T C 4 bytes
//   backward  ag_bwd_gate_kernel reads dy and x: da, softmax backward, ReLU6 mask -> g [B, T]; per-clip (sum g, sum g xhat)   2 B T C 4
//             ag_bwd_fold_kernel one workgroup: dgamma, dbeta, the two means the BatchNorm backward subtracts
//             ag_bwd_dx_kernel   du [T] in LDS; reads dy and x, writes dx; rows [K][C] of S_j[c] = sum du[b, t] x[b, t + j - pl, c]   3 B T C 4
//             ag_bwd_wfold_kernel  fixed-order fold of the rows: dwa[j, c] = Wa[c] S_j[c], dWa[c] = sum_j wa[j, c] S_j[c]
// No atomics; every sum has one order: bit-identical from run to run.
// A wave owns whole time steps where a sum over channels is needed (16-byte loads along C, xor-butterfly reduction); in
// ag_bwd_dx_kernel a thread owns one 16-byte channel vector and walks time, so that S_j stays in its registers.
#include "internal.h"

namespace {

constexpr int AG_MAXT = 128, AG_MAXC = 1024, AG_MAXK = 5;
constexpr int AG_PADL = (AG_MAXK - 1) / 2;
constexpr int AG_MAX_ROWS = 1024;       // partial rows of the depthwise / pointwise weight gradients
constexpr int AG_MAX_RG = 8;            // time-step groups of a workgroup in ag_bwd_dx_kernel
constexpr float AG_BN_EPS = 1e-3f;      // Keras BatchNormalization defaults
constexpr float AG_BN_MOMENTUM = 0.99f;

__device__ __forceinline__ float ag_wave_all_sum(float v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float ag_wave_all_max(float v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float ag_dot4(const float4 a, const float4 b, float acc) {
  return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, fmaf(a.x, b.x, acc))));
}
__device__ __forceinline__ void ag_fma4(float4& acc, float s, const float4 v) {
  acc.x = fmaf(s, v.x, acc.x); acc.y = fmaf(s, v.y, acc.y); acc.z = fmaf(s, v.z, acc.z); acc.w = fmaf(s, v.w, acc.w);
}

// sum of one value per thread over a 1024-thread workgroup, fixed tree; every thread gets the result
__device__ float ag_block_sum(float v, float* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  return red[0];
}

// u[b, t] = sum_j sum_c (Wa[c] wa[j, c]) x[b, t + j - pl, c]: every row of x meets its K folded kernels once
template <int K>
__global__ __launch_bounds__(256) void ag_logits_kernel(const float* __restrict__ x, const float* __restrict__ wa,
                                                        const float* __restrict__ Wa, float* __restrict__ u,
                                                        float* __restrict__ csum, int T, int C) {
  __shared__ float4 ww[K][AG_MAXC / 4];
  __shared__ float v[K][AG_MAXT];
  __shared__ float wsum[2];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C4 = C >> 2;
  const float4* wa4 = reinterpret_cast<const float4*>(wa);
  const float4* Wa4 = reinterpret_cast<const float4*>(Wa);
  for (int i = tid; i < K * C4; i += 256) {
    const int j = i / C4, c4 = i - j * C4;
    const float4 a = wa4[i], w = Wa4[c4];
    ww[j][c4] = make_float4(a.x * w.x, a.y * w.y, a.z * w.z, a.w * w.w);
  }
  __syncthreads();
  const float4* xb = reinterpret_cast<const float4*>(x) + (int64_t)b * T * C4;
  for (int s = wave; s < T; s += 4) {
    float acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j] = 0.f;
    for (int c4 = lane; c4 < C4; c4 += 64) {
      const float4 xv = xb[(int64_t)s * C4 + c4];
#pragma unroll
      for (int j = 0; j < K; ++j) acc[j] = ag_dot4(xv, ww[j][c4], acc[j]);
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const float r = ag_wave_all_sum(acc[j]);
      if (lane == 0) v[j][s] = r;
    }
  }
  __syncthreads();
  constexpr int pl = (K - 1) / 2;
  float uu = 0.f;
  if (tid < T) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const int s = tid + j - pl;
      if (s >= 0 && s < T) uu += v[j][s];
    }
    u[(int64_t)b * T + tid] = uu;
  }
  if (csum) {
    if (wave < 2) {
      const float s = ag_wave_all_sum(tid < T ? uu : 0.f);
      if (lane == 0) wsum[wave] = s;
    }
    __syncthreads();
    if (tid == 0) csum[b] = wsum[0] + wsum[1];
  }
}

// batch statistics of u over N = B T values: the mean from the per-clip sums, the biased variance around it
__global__ __launch_bounds__(1024) void ag_bn_train_kernel(const float* __restrict__ u, const float* __restrict__ csum, int B,
                                                           int64_t N, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float* mm, float* mv,
                                                           float* __restrict__ tab) {
  __shared__ float red[1024];
  const int tid = threadIdx.x;
  float s = 0.f;
  for (int b = tid; b < B; b += 1024) s += csum[b];
  const float mean = ag_block_sum(s, red) / (float)N;
  float q = 0.f;
  for (int64_t i = tid; i < N; i += 1024) {
    const float d = u[i] - mean;
    q = fmaf(d, d, q);
  }
  const float var = ag_block_sum(q, red) / (float)N;
  if (tid == 0) {
    const float rstd = 1.0f / sqrtf(var + AG_BN_EPS);
    const float scale = gamma[0] * rstd;
    tab[0] = scale;
    tab[1] = beta[0] - mean * scale;
    tab[2] = mean;
    tab[3] = rstd;
    if (mm) {   // AssignMovingAvg: m -= (m - batch) * (1 - momentum); biased variance
      const float omm = 1.0f - AG_BN_MOMENTUM;
      mm[0] = mm[0] - (mm[0] - mean) * omm;
      mv[0] = mv[0] - (mv[0] - var) * omm;
    }
  }
}

__global__ void ag_bn_infer_kernel(const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ mm,
                                   const float* __restrict__ mv, float* __restrict__ tab) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float rstd = 1.0f / sqrtf(mv[0] + AG_BN_EPS);
  const float scale = gamma[0] * rstd;
  tab[0] = scale;
  tab[1] = beta[0] - mm[0] * scale;
  tab[2] = mm[0];
  tab[3] = rstd;
}

// att = softmax over time of relu6(scale u + shift), y = x att
__global__ __launch_bounds__(256) void ag_apply_kernel(const float* __restrict__ x, const float* __restrict__ u,
                                                       const float* __restrict__ tab, float* __restrict__ att,
                                                       float* __restrict__ y, int T, int C) {
  __shared__ float att_s[AG_MAXT];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int C4 = C >> 2;
  if (tid < 64) {   // one wave, two time steps per lane
    const float scale = tab[0], shift = tab[1];
    const int t0 = tid, t1 = tid + 64;
    const float p0 = t0 < T ? relu6f(fmaf(u[(int64_t)b * T + t0], scale, shift)) : -INFINITY;
    const float p1 = t1 < T ? relu6f(fmaf(u[(int64_t)b * T + t1], scale, shift)) : -INFINITY;
    const float m = ag_wave_all_max(fmaxf(p0, p1));
    const float e0 = t0 < T ? expf(p0 - m) : 0.f, e1 = t1 < T ? expf(p1 - m) : 0.f;
    const float den = ag_wave_all_sum(e0 + e1);
    if (t0 < T) { att_s[t0] = e0 / den; att[(int64_t)b * T + t0] = e0 / den; }
    if (t1 < T) { att_s[t1] = e1 / den; att[(int64_t)b * T + t1] = e1 / den; }
  }
  __syncthreads();
  const float4* xb = reinterpret_cast<const float4*>(x) + (int64_t)b * T * C4;
  float4* yb = reinterpret_cast<float4*>(y) + (int64_t)b * T * C4;
  for (int s = 0; s < T; ++s) {
    const float a = att_s[s];
    for (int c4 = tid; c4 < C4; c4 += 256) {
      const float4 xv = xb[(int64_t)s * C4 + c4];
      yb[(int64_t)s * C4 + c4] = make_float4(xv.x * a, xv.y * a, xv.z * a, xv.w * a);
    }
  }
}

// da[t] = sum_c dy x -> softmax backward over t -> ReLU6 mask: g [B, T] and the clip's (sum g, sum g xhat)
__global__ __launch_bounds__(256) void ag_bwd_gate_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                          const float* __restrict__ u, const float* __restrict__ att,
                                                          const float* __restrict__ tab, float* __restrict__ g,
                                                          float* __restrict__ part, int T, int C) {
  __shared__ float da[AG_MAXT];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C4 = C >> 2;
  const float4* xb = reinterpret_cast<const float4*>(x) + (int64_t)b * T * C4;
  const float4* db = reinterpret_cast<const float4*>(dy) + (int64_t)b * T * C4;
  for (int s = wave; s < T; s += 4) {
    float acc = 0.f;
    for (int c4 = lane; c4 < C4; c4 += 64) acc = ag_dot4(db[(int64_t)s * C4 + c4], xb[(int64_t)s * C4 + c4], acc);
    acc = ag_wave_all_sum(acc);
    if (lane == 0) da[s] = acc;
  }
  __syncthreads();
  if (tid < 64) {
    const float scale = tab[0], shift = tab[1], mean = tab[2], rstd = tab[3];
    const int t0 = tid, t1 = tid + 64;
    const float a0 = t0 < T ? att[(int64_t)b * T + t0] : 0.f, a1 = t1 < T ? att[(int64_t)b * T + t1] : 0.f;
    const float d0 = t0 < T ? da[t0] : 0.f, d1 = t1 < T ? da[t1] : 0.f;
    const float dot = ag_wave_all_sum(fmaf(a0, d0, a1 * d1));
    const float u0 = t0 < T ? u[(int64_t)b * T + t0] : 0.f, u1 = t1 < T ? u[(int64_t)b * T + t1] : 0.f;
    const float pre0 = fmaf(u0, scale, shift), pre1 = fmaf(u1, scale, shift);
    const float g0 = (t0 < T && pre0 > 0.f && pre0 <= 6.f) ? a0 * (d0 - dot) : 0.f;
    const float g1 = (t1 < T && pre1 > 0.f && pre1 <= 6.f) ? a1 * (d1 - dot) : 0.f;
    if (t0 < T) g[(int64_t)b * T + t0] = g0;
    if (t1 < T) g[(int64_t)b * T + t1] = g1;
    const float sg = ag_wave_all_sum(g0 + g1);
    const float sx = ag_wave_all_sum(fmaf(g0, (u0 - mean) * rstd, g1 * ((u1 - mean) * rstd)));
    if (tid == 0) {
      part[2 * b] = sg;
      part[2 * b + 1] = sx;
    }
  }
}

// dgamma = sum g xhat, dbeta = sum g; coef = (sum g / N, sum g xhat / N) with batch statistics, (0, 0) with moving ones
__global__ __launch_bounds__(1024) void ag_bwd_fold_kernel(const float* __restrict__ part, int B, int64_t N, int training,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                           float* __restrict__ coef) {
  __shared__ float red[1024];
  const int tid = threadIdx.x;
  float sg = 0.f, sx = 0.f;
  for (int b = tid; b < B; b += 1024) {
    sg += part[2 * b];
    sx += part[2 * b + 1];
  }
  sg = ag_block_sum(sg, red);
  sx = ag_block_sum(sx, red);
  if (tid == 0) {
    dgamma[0] = sx;
    dbeta[0] = sg;
    coef[0] = training ? sg / (float)N : 0.f;
    coef[1] = training ? sx / (float)N : 0.f;
  }
}

// du[t] = gamma rstd (g - c1 - xhat c2); dx = dy att + sum_j du[t - j + pl] Wa wa[j]; S_j += du[s - j + pl] x[s]
template <int K>
__global__ __launch_bounds__(256) void ag_bwd_dx_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                        const float* __restrict__ u, const float* __restrict__ att,
                                                        const float* __restrict__ g, const float* __restrict__ tab,
                                                        const float* __restrict__ gamma, const float* __restrict__ coef,
                                                        const float* __restrict__ wa, const float* __restrict__ Wa,
                                                        float* __restrict__ dx, float* __restrict__ part, int B, int T, int C,
                                                        int clips_per) {
  __shared__ float du_p[AG_MAXT + 2 * AG_PADL];
  __shared__ float att_s[AG_MAXT];
  __shared__ float4 sred[K][AG_MAXC / 4];
  constexpr int pl = (K - 1) / 2;
  const int tid = threadIdx.x;
  const int C4 = C >> 2;
  int RG = 256 / C4;
  RG = RG < 1 ? 1 : (RG > AG_MAX_RG ? AG_MAX_RG : RG);
  const int rg = tid / C4, c4 = tid - rg * C4;
  const bool active = rg < RG;
  const float mean = tab[2], rstd = tab[3], c1 = coef[0], c2 = coef[1];
  const float gs = gamma[0] * rstd;
  float4 w[K], S[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    S[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    w[j] = S[j];
    if (active) {
      const float4 a = reinterpret_cast<const float4*>(wa)[j * C4 + c4], p = reinterpret_cast<const float4*>(Wa)[c4];
      w[j] = make_float4(a.x * p.x, a.y * p.y, a.z * p.z, a.w * p.w);
    }
  }
  const int b0 = blockIdx.x * clips_per;
  const int b1 = b0 + clips_per < B ? b0 + clips_per : B;
  for (int b = b0; b < b1; ++b) {
    __syncthreads();
    if (tid < T) {
      const float uu = u[(int64_t)b * T + tid];
      du_p[AG_PADL + tid] = gs * (g[(int64_t)b * T + tid] - c1 - (uu - mean) * rstd * c2);
      att_s[tid] = att[(int64_t)b * T + tid];
    }
    if (tid < AG_PADL) {
      du_p[tid] = 0.f;
      du_p[AG_PADL + T + tid] = 0.f;
    }
    __syncthreads();
    if (active) {
      const float4* xb = reinterpret_cast<const float4*>(x) + (int64_t)b * T * C4;
      const float4* db = reinterpret_cast<const float4*>(dy) + (int64_t)b * T * C4;
      float4* ob = reinterpret_cast<float4*>(dx) + (int64_t)b * T * C4;
      for (int s = rg; s < T; s += RG) {
        const float4 xv = xb[(int64_t)s * C4 + c4];
        const float4 dv = db[(int64_t)s * C4 + c4];
        const float a = att_s[s];
        float4 o = make_float4(dv.x * a, dv.y * a, dv.z * a, dv.w * a);
#pragma unroll
        for (int j = 0; j < K; ++j) {
          const float d = du_p[AG_PADL + s - j + pl];   // index in [AG_PADL - pl, AG_PADL + T - 1 + pl]
          ag_fma4(o, d, w[j]);
          ag_fma4(S[j], d, xv);
        }
        ob[(int64_t)s * C4 + c4] = o;
      }
    }
  }
  // the time-step groups add their sums one after the other: one order
  for (int r = 0; r < RG; ++r) {
    __syncthreads();
    if (active && rg == r) {
#pragma unroll
      for (int j = 0; j < K; ++j) {
        if (r == 0) sred[j][c4] = S[j];
        else kws_add4(sred[j][c4], S[j]);
      }
    }
  }
  __syncthreads();
  float4* prow = reinterpret_cast<float4*>(part) + (int64_t)blockIdx.x * K * C4;
  for (int i = tid; i < K * C4; i += 256) prow[i] = sred[i / C4][i - (i / C4) * C4];
}

// rows [n_rows][K][C] -> dwa [K][C], dWa [C]; 16 channels x 16 slices of rows per workgroup, slices folded in a fixed tree
template <int K>
__global__ __launch_bounds__(256) void ag_bwd_wfold_kernel(const float* __restrict__ part, int n_rows, int C,
                                                           const float* __restrict__ wa, const float* __restrict__ Wa,
                                                           float* __restrict__ dwa, float* __restrict__ dWa) {
  __shared__ float red[K][16][17];
  const int cl = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  float s[K];
#pragma unroll
  for (int j = 0; j < K; ++j) s[j] = 0.f;
  if (c < C)
    for (int r = sl; r < n_rows; r += 16) {
#pragma unroll
      for (int j = 0; j < K; ++j) s[j] += part[((int64_t)r * K + j) * C + c];
    }
#pragma unroll
  for (int j = 0; j < K; ++j) red[j][sl][cl] = s[j];
  __syncthreads();
  for (int o = 8; o > 0; o >>= 1) {
    if (sl < o) {
#pragma unroll
      for (int j = 0; j < K; ++j) red[j][sl][cl] += red[j][sl + o][cl];
    }
    __syncthreads();
  }
  if (sl == 0 && c < C) {
    const float pw = Wa[c];
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const float Sj = red[j][0][cl];
      dwa[(int64_t)j * C + c] = pw * Sj;
      acc = fmaf(wa[(int64_t)j * C + c], Sj, acc);
    }
    dWa[c] = acc;
  }
}

int ag_check(const char* who, int B, int T, int C, int k) {
  KWS_REQUIRE(B >= 1, "%s: B=%d", who, B);
  KWS_REQUIRE(T >= 1 && T <= AG_MAXT, "%s: T=%d (1 .. %d)", who, T, AG_MAXT);
  KWS_REQUIRE(C >= 4 && C <= AG_MAXC && C % 4 == 0, "%s: C=%d (a multiple of 4, 4 .. %d)", who, C, AG_MAXC);
  KWS_REQUIRE(k == 3 || k == 5, "%s: k=%d (3 or 5)", who, k);
  return KWS_OK;
}
bool ag_in_domain(int B, int T, int C, int k) {
  return B >= 1 && T >= 1 && T <= AG_MAXT && C >= 4 && C <= AG_MAXC && C % 4 == 0 && (k == 3 || k == 5);
}
int64_t ag_round(int64_t n) { return (n + 63) / 64 * 64; }
int ag_clips_per(int B) { return ceil_div(B, AG_MAX_ROWS); }
int ag_rows(int B) { return ceil_div(B, ag_clips_per(B)); }

struct AgBwdWs {
  int64_t g, part2, coef, rows, total;
};
AgBwdWs ag_bwd_ws(int B, int T, int C, int k) {
  AgBwdWs w;
  w.g = 0;
  w.part2 = w.g + ag_round((int64_t)B * T);
  w.coef = w.part2 + ag_round((int64_t)2 * B);
  w.rows = w.coef + 64;
  w.total = w.rows + ag_round((int64_t)ag_rows(B) * k * C);
  return w;
}

}  // namespace

extern "C" {

int64_t kws_attn_gate_fwd_floats(int B, int T, int C, int k) { return ag_in_domain(B, T, C, k) ? ag_round(B) : 0; }

int64_t kws_attn_gate_bwd_floats(int B, int T, int C, int k) { return ag_in_domain(B, T, C, k) ? ag_bwd_ws(B, T, C, k).total : 0; }

int kws_attn_gate_fwd_f32(const float* x, const float* wa, const float* Wa, const float* gamma, const float* beta, float* mm,
                          float* mv, float* u, float* table, float* att, float* y, float* workspace, int B, int T, int C, int k,
                          int training, void* stream) {
  KWS_TRY(ag_check("attn_gate_fwd", B, T, C, k));
  KWS_REQUIRE(x && wa && Wa && gamma && beta && mm && mv && u && table && att && y && workspace, "attn_gate_fwd: NULL pointer");
  hipStream_t st = (hipStream_t)stream;
  const double bytes = 4.0 * B * T * C;
  {
    KwsProfScope prof("attn_gate_logits", 2.0 * B * T * C * k, bytes, st);
    if (k == 3) hipLaunchKernelGGL(ag_logits_kernel<3>, dim3((unsigned)B), dim3(256), 0, st, x, wa, Wa, u, training ? workspace : nullptr, T, C);
    else hipLaunchKernelGGL(ag_logits_kernel<5>, dim3((unsigned)B), dim3(256), 0, st, x, wa, Wa, u, training ? workspace : nullptr, T, C);
    KWS_LAUNCH_CHECK("ag_logits_kernel");
  }
  if (training) {
    hipLaunchKernelGGL(ag_bn_train_kernel, dim3(1), dim3(1024), 0, st, u, workspace, B, (int64_t)B * T, gamma, beta, mm, mv, table);
    KWS_LAUNCH_CHECK("ag_bn_train_kernel");
  } else {
    hipLaunchKernelGGL(ag_bn_infer_kernel, dim3(1), dim3(64), 0, st, gamma, beta, mm, mv, table);
    KWS_LAUNCH_CHECK("ag_bn_infer_kernel");
  }
  KwsProfScope prof("attn_gate_apply", 1.0 * B * T * C, 2.0 * bytes, st);
  hipLaunchKernelGGL(ag_apply_kernel, dim3((unsigned)B), dim3(256), 0, st, x, u, table, att, y, T, C);
  KWS_LAUNCH_CHECK("ag_apply_kernel");
  return KWS_OK;
}

int kws_attn_gate_bwd_f32(const float* dy, const float* x, const float* u, const float* att, const float* table, const float* wa,
                          const float* Wa, const float* gamma, float* dx, float* dwa, float* dWa, float* dgamma, float* dbeta,
                          float* workspace, int B, int T, int C, int k, int training, void* stream) {
  KWS_TRY(ag_check("attn_gate_bwd", B, T, C, k));
  KWS_REQUIRE(dy && x && u && att && table && wa && Wa && gamma && dx && dwa && dWa && dgamma && dbeta && workspace,
              "attn_gate_bwd: NULL pointer");
  hipStream_t st = (hipStream_t)stream;
  const AgBwdWs w = ag_bwd_ws(B, T, C, k);
  float* g = workspace + w.g;
  float* part2 = workspace + w.part2;
  float* coef = workspace + w.coef;
  float* rows = workspace + w.rows;
  const double bytes = 4.0 * B * T * C;
  {
    KwsProfScope prof("attn_gate_bwd_gate", 2.0 * B * T * C, 2.0 * bytes, st);
    hipLaunchKernelGGL(ag_bwd_gate_kernel, dim3((unsigned)B), dim3(256), 0, st, dy, x, u, att, table, g, part2, T, C);
    KWS_LAUNCH_CHECK("ag_bwd_gate_kernel");
  }
  hipLaunchKernelGGL(ag_bwd_fold_kernel, dim3(1), dim3(1024), 0, st, part2, B, (int64_t)B * T, training, dgamma, dbeta, coef);
  KWS_LAUNCH_CHECK("ag_bwd_fold_kernel");
  const int cp = ag_clips_per(B), n_rows = ag_rows(B);
  {
    KwsProfScope prof("attn_gate_bwd_dx", 4.0 * B * T * C * k, 3.0 * bytes + 4.0 * n_rows * k * C, st);
    if (k == 3)
      hipLaunchKernelGGL(ag_bwd_dx_kernel<3>, dim3((unsigned)n_rows), dim3(256), 0, st, dy, x, u, att, g, table, gamma, coef, wa, Wa, dx, rows,
                         B, T, C, cp);
    else
      hipLaunchKernelGGL(ag_bwd_dx_kernel<5>, dim3((unsigned)n_rows), dim3(256), 0, st, dy, x, u, att, g, table, gamma, coef, wa, Wa, dx, rows,
                         B, T, C, cp);
    KWS_LAUNCH_CHECK("ag_bwd_dx_kernel");
  }
  if (k == 3) hipLaunchKernelGGL(ag_bwd_wfold_kernel<3>, dim3((unsigned)ceil_div(C, 16)), dim3(256), 0, st, rows, n_rows, C, wa, Wa, dwa, dWa);
  else hipLaunchKernelGGL(ag_bwd_wfold_kernel<5>, dim3((unsigned)ceil_div(C, 16)), dim3(256), 0, st, rows, n_rows, C, wa, Wa, dwa, dWa);
  KWS_LAUNCH_CHECK("ag_bwd_wfold_kernel");
  return KWS_OK;
}

}  // extern "C"
