// Depthwise convolution along time with ANY tap count and stride, channels-last, with the producer's BatchNorm + ReLU6 applied
// on load: the general form of dwconv.hip's 3-tap kernels, for the reference's _depthwise_conv_block as its raw-waveform
// models call it (model.py:34-52; conv_1d_gru_model uses k 63 / 31 / 15 / 7 / 5 / 8 at strides 16 / 4 / 4 / 4 / 2 / 1).
//   fwd   z[b,t,c] = sum_{j<k} w[j,c] * act(y[b, s*t + j - pad_l, c])                        (0 outside [0, L_in))
//   bwd   g[b,u,c] = relu6'(bn(y[b,u,c])) * sum_j w[j,c] * dz[b,(u + pad_l - j)/s,c]          (j with s | u + pad_l - j, t in range)
//         part     = rows [2 + k][C] per workgroup row of (sum g, sum g*xhat, dw_0 .. dw_{k-1})
//   finalize       part -> dw [k, C], dgamma, dbeta, coef = (c1 | c2) for kws_bn_bwd_apply
// Both passes are HBM-bound.  A thread owns one float4 of channels and a run of time steps.  With row u = s*q + r - pad_l (stride
// group q, phase r), row u meets output t = q - m through tap j = s*m + r, m < NA = ceil(k / s): the forward keeps NA output
// accumulators in a register ring and reads every input row once; the backward keeps the NA latest dz rows in the ring and walks
// its run once per phase r, so that the tap gradients of one phase are NA accumulators with compile-time indices.  The k x C
// taps sit in LDS (a workgroup covers a slice of at most 128 channels).  Geometries with NA > 8 (none of the models) take the
// direct kernels, which loop over the taps and leave the re-reads to the caches.  C = 1 (the first layer: [B, 16000] samples)
// is an arm of its own with the lanes along time and the input chunk staged in LDS.
// No atomics: partial rows are folded in a fixed order, results are bit-identical from run to run.
//
// The same file holds the pointwise convolution that follows the one-channel depthwise layer, K = 1 -> N (kws_dwconvk_pw1_*):
// an outer product with the BatchNorm column sums of the GEMMs, and its backward.
#include <string.h>

#include "common.h"
#include "internal.h"

namespace {

constexpr int DK_MAXK = 64, DK_MAXS = 16, DK_MAXC = 1024;
constexpr int DK_CQ = 32;        // channel quads per workgroup slice
constexpr int DK_THREADS = 256;
constexpr int DK_FWD_TT = 32;    // outputs per thread run (forward)
constexpr int DK_BWD_QT = 32;    // stride groups per thread run (backward)
constexpr int DK_MAXNA = 8;      // ring kernels up to this many accumulators
constexpr int DK1_TB = 256;      // C = 1: outputs (forward) / stride groups (backward) per workgroup
constexpr int DK1_SM = DK_MAXS * DK1_TB + DK_MAXK;   // staged input rows of a C = 1 workgroup (upper bound)

__device__ __forceinline__ float4 dk_zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 dk_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void dk_st4(float* p, const float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float4 dk_fma(const float4 a, const float4 b, const float4 c) {
  return make_float4(fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y), fmaf(a.z, b.z, c.z), fmaf(a.w, b.w, c.w));
}
__device__ __forceinline__ float4 dk_act(const float4 v, const float4 sc, const float4 sh) {
  return make_float4(relu6f(fmaf(v.x, sc.x, sh.x)), relu6f(fmaf(v.y, sc.y, sh.y)), relu6f(fmaf(v.z, sc.z, sh.z)),
                     relu6f(fmaf(v.w, sc.w, sh.w)));
}
__device__ __forceinline__ float dk_gate(float pre) { return (pre > 0.f && pre <= 6.f) ? 1.f : 0.f; }
__device__ __forceinline__ float4 dk_gate4(const float4 v, const float4 sc, const float4 sh) {
  return make_float4(dk_gate(fmaf(v.x, sc.x, sh.x)), dk_gate(fmaf(v.y, sc.y, sh.y)), dk_gate(fmaf(v.z, sc.z, sh.z)),
                     dk_gate(fmaf(v.w, sc.w, sh.w)));
}

struct DkArgs {
  const float* y; const float* bn; const float* w; const float* dz;
  float* z; float* g; float* part;
  int B, Lin, Lout, C, k, s, pad_l;
  int cq, R, nruns, Q;
  int64_t units;
};

// taps of this workgroup's channel slice -> LDS rows [k + 1][cq] of float4; row k is zero (what a tap index >= k reads)
__device__ __forceinline__ void dk_load_taps(float4* wl, const DkArgs& a, int slice) {
  const int C4 = a.C >> 2;
  for (int i = threadIdx.x; i < (a.k + 1) * a.cq; i += blockDim.x) {
    const int j = i / a.cq, q4 = i - j * a.cq;
    const int c4 = slice * a.cq + q4;
    wl[i] = (j < a.k && c4 < C4) ? dk_ld4(a.w + (int64_t)j * a.C + c4 * 4) : dk_zero();
  }
  __syncthreads();
}

// ---- forward, C % 4 == 0, NA <= 8 -------------------------------------------------------------------------------------------
// RU = input rows loaded ahead of their use (4 when 4 | s, else 1)
template <int NA, bool HAS_BN, int RU>
__global__ __launch_bounds__(DK_THREADS) void dk_fwd_ring_kernel(DkArgs a) {
  extern __shared__ float4 dk_wl[];
  dk_load_taps(dk_wl, a, (int)blockIdx.y);
  const int C4 = a.C >> 2, cq = a.cq;
  const int rr = threadIdx.x / cq, q4 = threadIdx.x - rr * cq;
  const int c4 = (int)blockIdx.y * cq + q4;
  const int64_t unit = (int64_t)blockIdx.x * a.R + rr;
  if (c4 >= C4 || unit >= a.units) return;
  const int c = c4 * 4, C = a.C, s = a.s, k = a.k;
  const int64_t b = unit / a.nruns;
  const int t0 = (int)(unit - b * a.nruns) * DK_FWD_TT;
  const int t1 = min(t0 + DK_FWD_TT, a.Lout);
  float4 sc = dk_zero(), sh = dk_zero();
  if (HAS_BN) {
    sc = dk_ld4(a.bn + c);
    sh = dk_ld4(a.bn + C + c);
  }
  const float* yb = a.y + b * (int64_t)a.Lin * C + c;
  float* zb = a.z + b * (int64_t)a.Lout * C + c;
  const float4* wq = dk_wl + q4;
  float4 acc[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) acc[i] = dk_zero();
  const int q_end = t1 - 1 + NA - 1;   // output t is complete after stride group t + NA - 1
  for (int qb = t0; qb <= q_end; qb += NA) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int q = qb + i;
      if (q <= q_end) {
        for (int r0 = 0; r0 < s; r0 += RU) {
          float4 v[RU];
          // SAME padding pads the ACTIVATION with zeros: a row outside the clip reads row 0 and is zeroed after the activation
#pragma unroll
          for (int e = 0; e < RU; ++e) {
            const int u = s * q + r0 + e - a.pad_l;
            v[e] = dk_ld4(yb + (int64_t)((u >= 0 && u < a.Lin) ? u : 0) * C);
          }
#pragma unroll
          for (int e = 0; e < RU; ++e) {
            const int r = r0 + e;
            const int u = s * q + r - a.pad_l;
            float4 x = HAS_BN ? dk_act(v[e], sc, sh) : v[e];
            if (!(u >= 0 && u < a.Lin)) x = dk_zero();
#pragma unroll
            for (int m = 0; m < NA; ++m) {
              const int j = s * m + r;
              acc[(i - m + NA) % NA] = dk_fma(wq[(j < k ? j : k) * cq], x, acc[(i - m + NA) % NA]);
            }
          }
        }
        const int t = q - (NA - 1);
        if (t >= t0 && t < t1) dk_st4(zb + (int64_t)t * C, acc[(i + 1) % NA]);
        acc[(i + 1) % NA] = dk_zero();
      }
    }
  }
}

// ---- forward, C % 4 == 0, any k / s: one output row per thread, the taps in a loop ---------------------------------------
template <bool HAS_BN>
__global__ __launch_bounds__(DK_THREADS) void dk_fwd_direct_kernel(DkArgs a) {
  extern __shared__ float4 dk_wl[];
  dk_load_taps(dk_wl, a, (int)blockIdx.y);
  const int C4 = a.C >> 2, cq = a.cq;
  const int rr = threadIdx.x / cq, q4 = threadIdx.x - rr * cq;
  const int c4 = (int)blockIdx.y * cq + q4;
  const int64_t unit = (int64_t)blockIdx.x * a.R + rr;
  if (c4 >= C4 || unit >= a.units) return;
  const int c = c4 * 4, C = a.C;
  const int64_t b = unit / a.nruns;
  const int t0 = (int)(unit - b * a.nruns) * DK_FWD_TT;
  const int t1 = min(t0 + DK_FWD_TT, a.Lout);
  float4 sc = dk_zero(), sh = dk_zero();
  if (HAS_BN) {
    sc = dk_ld4(a.bn + c);
    sh = dk_ld4(a.bn + C + c);
  }
  const float* yb = a.y + b * (int64_t)a.Lin * C + c;
  float* zb = a.z + b * (int64_t)a.Lout * C + c;
  for (int t = t0; t < t1; ++t) {
    float4 acc = dk_zero();
    for (int j = 0; j < a.k; ++j) {
      const int u = a.s * t + j - a.pad_l;
      if (u >= 0 && u < a.Lin) {
        const float4 v = dk_ld4(yb + (int64_t)u * C);
        acc = dk_fma(dk_wl[j * cq + q4], HAS_BN ? dk_act(v, sc, sh) : v, acc);
      }
    }
    dk_st4(zb + (int64_t)t * C, acc);
  }
}

// the R runs of a workgroup, ascending: columns of this slice of part row `row`
__device__ __forceinline__ void dk_fold_row(float* red, const float4 v, const DkArgs& a, int row, int slice) {
  const int cq = a.cq;
  __syncthreads();
  dk_st4(red + threadIdx.x * 4, v);
  __syncthreads();
  for (int o = threadIdx.x; o < cq * 4; o += blockDim.x) {
    const int ch = slice * cq * 4 + o;
    if (ch < a.C) {
      float sum = 0.f;
      for (int r = 0; r < a.R; ++r) sum += red[r * cq * 4 + o];
      a.part[((int64_t)blockIdx.x * (2 + a.k) + row) * a.C + ch] = sum;
    }
  }
}

// ---- backward, C % 4 == 0, NA <= 8 ------------------------------------------------------------------------------------------
template <int NA, bool HAS_BN>
__global__ __launch_bounds__(DK_THREADS) void dk_bwd_ring_kernel(DkArgs a) {
  extern __shared__ float4 dk_wl[];
  __shared__ float red[DK_THREADS * 4];
  dk_load_taps(dk_wl, a, (int)blockIdx.y);
  const int C4 = a.C >> 2, cq = a.cq;
  const int rr = threadIdx.x / cq, q4 = threadIdx.x - rr * cq;
  const int c4 = (int)blockIdx.y * cq + q4;
  const int64_t unit = (int64_t)blockIdx.x * a.R + rr;
  const bool active = c4 < C4 && unit < a.units;
  const int c = active ? c4 * 4 : 0, C = a.C, s = a.s, k = a.k;
  const int64_t b = active ? unit / a.nruns : 0;
  const int q0 = active ? (int)(unit - b * a.nruns) * DK_BWD_QT : 0;
  const int q1 = active ? min(q0 + DK_BWD_QT, a.Q) : 0;
  float4 sc = dk_zero(), sh = dk_zero(), mean = dk_zero(), rstd = dk_zero();
  if (HAS_BN) {
    sc = dk_ld4(a.bn + c);
    sh = dk_ld4(a.bn + C + c);
    mean = dk_ld4(a.bn + 2 * C + c);
    rstd = dk_ld4(a.bn + 3 * C + c);
  }
  const float* yb = a.y + b * (int64_t)a.Lin * C + c;
  const float* dzb = a.dz + b * (int64_t)a.Lout * C + c;
  float* gb = a.g + b * (int64_t)a.Lin * C + c;
  const float4* wq = dk_wl + q4;
  float4 sg = dk_zero(), sgx = dk_zero();
  for (int r = 0; r < s; ++r) {
    float4 dwa[NA], ring[NA];
#pragma unroll
    for (int m = 0; m < NA; ++m) dwa[m] = dk_zero();
    ring[0] = dk_zero();
#pragma unroll
    for (int m = 1; m < NA; ++m) {   // dz rows q0 - 1 .. q0 - NA + 1 ahead of the run
      const int t = q0 - m;
      const float4 d = dk_ld4(dzb + (int64_t)((t >= 0 && t < a.Lout) ? t : 0) * C);
      ring[NA - m] = (active && t >= 0 && t < a.Lout) ? d : dk_zero();
    }
    for (int qb = q0; qb < q1; qb += NA) {
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int q = qb + i;
        if (q < q1) {
          const int u = s * q + r - a.pad_l;
          const bool ok = u >= 0 && u < a.Lin;
          const float4 d0 = dk_ld4(dzb + (int64_t)(q < a.Lout ? q : 0) * C);
          const float4 yv = dk_ld4(yb + (int64_t)(ok ? u : 0) * C);
          ring[i] = q < a.Lout ? d0 : dk_zero();
          float4 x = HAS_BN ? dk_act(yv, sc, sh) : yv;
          if (!ok) x = dk_zero();
          float4 gs = dk_zero();
#pragma unroll
          for (int m = 0; m < NA; ++m) {
            const int j = s * m + r;
            const float4 d = ring[(i - m + NA) % NA];
            gs = dk_fma(wq[(j < k ? j : k) * cq], d, gs);
            dwa[m] = dk_fma(x, d, dwa[m]);
          }
          if (ok) {
            if (HAS_BN) {
              const float4 gt = dk_gate4(yv, sc, sh);
              gs = make_float4(gs.x * gt.x, gs.y * gt.y, gs.z * gt.z, gs.w * gt.w);
              sg.x += gs.x; sg.y += gs.y; sg.z += gs.z; sg.w += gs.w;
              sgx.x = fmaf(gs.x, (yv.x - mean.x) * rstd.x, sgx.x);
              sgx.y = fmaf(gs.y, (yv.y - mean.y) * rstd.y, sgx.y);
              sgx.z = fmaf(gs.z, (yv.z - mean.z) * rstd.z, sgx.z);
              sgx.w = fmaf(gs.w, (yv.w - mean.w) * rstd.w, sgx.w);
            }
            dk_st4(gb + (int64_t)u * C, gs);
          }
        }
      }
    }
#pragma unroll
    for (int m = 0; m < NA; ++m) {
      const int j = s * m + r;   // uniform over the workgroup
      if (j < k) dk_fold_row(red, dwa[m], a, 2 + j, (int)blockIdx.y);
    }
  }
  dk_fold_row(red, sg, a, 0, (int)blockIdx.y);
  dk_fold_row(red, sgx, a, 1, (int)blockIdx.y);
}

// ---- backward, C % 4 == 0, any k / s ----------------------------------------------------------------------------------------
template <bool HAS_BN>
__global__ __launch_bounds__(DK_THREADS) void dk_bwd_direct_kernel(DkArgs a) {
  extern __shared__ float4 dk_wl[];
  __shared__ float red[DK_THREADS * 4];
  dk_load_taps(dk_wl, a, (int)blockIdx.y);
  const int C4 = a.C >> 2, cq = a.cq;
  const int rr = threadIdx.x / cq, q4 = threadIdx.x - rr * cq;
  const int c4 = (int)blockIdx.y * cq + q4;
  const int64_t unit = (int64_t)blockIdx.x * a.R + rr;
  const bool active = c4 < C4 && unit < a.units;
  const int c = active ? c4 * 4 : 0, C = a.C, s = a.s, k = a.k;
  const int64_t b = active ? unit / a.nruns : 0;
  const int q0 = active ? (int)(unit - b * a.nruns) * DK_BWD_QT : 0;
  const int q1 = active ? min(q0 + DK_BWD_QT, a.Q) : 0;
  float4 sc = dk_zero(), sh = dk_zero(), mean = dk_zero(), rstd = dk_zero();
  if (HAS_BN) {
    sc = dk_ld4(a.bn + c);
    sh = dk_ld4(a.bn + C + c);
    mean = dk_ld4(a.bn + 2 * C + c);
    rstd = dk_ld4(a.bn + 3 * C + c);
  }
  const float* yb = a.y + b * (int64_t)a.Lin * C + c;
  const float* dzb = a.dz + b * (int64_t)a.Lout * C + c;
  float* gb = a.g + b * (int64_t)a.Lin * C + c;
  float4 sg = dk_zero(), sgx = dk_zero();
  for (int q = q0; q < q1; ++q)
    for (int r = 0; r < s; ++r) {
      const int u = s * q + r - a.pad_l;
      if (u < 0 || u >= a.Lin) continue;
      float4 gs = dk_zero();
      for (int j = r, t = q; j < k && t >= 0; j += s, --t)
        if (t < a.Lout) gs = dk_fma(dk_wl[j * cq + q4], dk_ld4(dzb + (int64_t)t * C), gs);
      if (HAS_BN) {
        const float4 yv = dk_ld4(yb + (int64_t)u * C);
        const float4 gt = dk_gate4(yv, sc, sh);
        gs = make_float4(gs.x * gt.x, gs.y * gt.y, gs.z * gt.z, gs.w * gt.w);
        sg.x += gs.x; sg.y += gs.y; sg.z += gs.z; sg.w += gs.w;
        sgx.x = fmaf(gs.x, (yv.x - mean.x) * rstd.x, sgx.x);
        sgx.y = fmaf(gs.y, (yv.y - mean.y) * rstd.y, sgx.y);
        sgx.z = fmaf(gs.z, (yv.z - mean.z) * rstd.z, sgx.z);
        sgx.w = fmaf(gs.w, (yv.w - mean.w) * rstd.w, sgx.w);
      }
      dk_st4(gb + (int64_t)u * C, gs);
    }
  dk_fold_row(red, sg, a, 0, (int)blockIdx.y);
  dk_fold_row(red, sgx, a, 1, (int)blockIdx.y);
  for (int j = 0; j < k; ++j) {   // the run's outputs t = q0 .. q1 - 1 (Lout <= Q: every (b, t) belongs to one run)
    float4 acc = dk_zero();
    for (int t = q0; t < q1 && t < a.Lout; ++t) {
      const int u = s * t + j - a.pad_l;
      if (u >= 0 && u < a.Lin) {
        const float4 v = dk_ld4(yb + (int64_t)u * C);
        acc = dk_fma(HAS_BN ? dk_act(v, sc, sh) : v, dk_ld4(dzb + (int64_t)t * C), acc);
      }
    }
    dk_fold_row(red, acc, a, 2 + j, (int)blockIdx.y);
  }
}

// ---- C = 1: lanes along time --------------------------------------------------------------------------------------------------
// LDS index of staged row i: one pad word per 32 rows, so that the stride-s reads of neighbouring lanes spread over the banks
__device__ __forceinline__ int dk1_p(int i) { return i + (i >> 5); }

template <bool HAS_BN>
__global__ __launch_bounds__(DK1_TB) void dk1_fwd_kernel(DkArgs a) {
  __shared__ float sm[DK1_SM + DK1_SM / 32 + 1];
  __shared__ float wl[DK_MAXK];
  const int tid = threadIdx.x, s = a.s, k = a.k;
  const int64_t b = blockIdx.x / a.nruns;
  const int t0 = (int)(blockIdx.x - b * a.nruns) * DK1_TB;
  const float sc = HAS_BN ? a.bn[0] : 0.f, sh = HAS_BN ? a.bn[1] : 0.f;
  const float* yb = a.y + b * (int64_t)a.Lin;
  const int n_in = s * (DK1_TB - 1) + k;
  for (int i = tid; i < n_in; i += DK1_TB) {
    const int u = s * t0 - a.pad_l + i;
    float v = 0.f;
    if (u >= 0 && u < a.Lin) {
      v = yb[u];
      if (HAS_BN) v = relu6f(fmaf(v, sc, sh));
    }
    sm[dk1_p(i)] = v;
  }
  if (tid < k) wl[tid] = a.w[tid];
  __syncthreads();
  const int t = t0 + tid;
  if (t >= a.Lout) return;
  float acc = 0.f;
  for (int j = 0; j < k; ++j) acc = fmaf(wl[j], sm[dk1_p(s * tid + j)], acc);
  a.z[b * (int64_t)a.Lout + t] = acc;
}

// fixed-order sum of one value per thread (256 threads): the tree's shape does not depend on the data
__device__ __forceinline__ float dk1_block_sum(float* red, float v) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = DK1_TB / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

// one workgroup: clip b, stride groups q0 .. q0 + 255 = input rows s*q0 - pad_l .. and the outputs t = q0 .. q0 + 255
template <bool HAS_BN>
__global__ __launch_bounds__(DK1_TB) void dk1_bwd_kernel(DkArgs a, int NA) {
  __shared__ float sm[DK1_SM + DK1_SM / 32 + 1];   // activated input rows
  __shared__ float dzs[DK1_TB + DK_MAXK];          // dz[q0 - NA + 1 .. q0 + 255]
  __shared__ float wl[DK_MAXK];
  __shared__ float red[DK1_TB];
  const int tid = threadIdx.x, s = a.s, k = a.k;
  const int64_t b = blockIdx.x / a.nruns;
  const int q0 = (int)(blockIdx.x - b * a.nruns) * DK1_TB;
  const float sc = HAS_BN ? a.bn[0] : 0.f, sh = HAS_BN ? a.bn[1] : 0.f;
  const float mean = HAS_BN ? a.bn[2] : 0.f, rstd = HAS_BN ? a.bn[3] : 0.f;
  const float* yb = a.y + b * (int64_t)a.Lin;
  const float* dzb = a.dz + b * (int64_t)a.Lout;
  const int n_in = s * (DK1_TB - 1) + k;
  for (int i = tid; i < n_in; i += DK1_TB) {
    const int u = s * q0 - a.pad_l + i;
    float v = 0.f;
    if (u >= 0 && u < a.Lin) {
      v = yb[u];
      if (HAS_BN) v = relu6f(fmaf(v, sc, sh));
    }
    sm[dk1_p(i)] = v;
  }
  for (int i = tid; i < DK1_TB + NA - 1; i += DK1_TB) {
    const int t = q0 - (NA - 1) + i;
    dzs[i] = (t >= 0 && t < a.Lout) ? dzb[t] : 0.f;
  }
  if (tid < k) wl[tid] = a.w[tid];
  __syncthreads();
  float* prow = a.part + (int64_t)blockIdx.x * (2 + k);
  {   // tap gradients: thread (slice p, tap j) adds the outputs t = q0 + p, q0 + p + 4, ...
    const int j = tid & 63, p = tid >> 6;
    float acc = 0.f;
    if (j < k)
      for (int tt = p; tt < DK1_TB; tt += 4) acc = fmaf(sm[dk1_p(s * tt + j)], dzs[NA - 1 + tt], acc);
    red[tid] = acc;
    __syncthreads();
    if (tid < k) prow[2 + tid] = ((red[tid] + red[64 + tid]) + red[128 + tid]) + red[192 + tid];
  }
  float sg = 0.f, sgx = 0.f;
  for (int ii = tid; ii < s * DK1_TB; ii += DK1_TB) {
    const int u = s * q0 - a.pad_l + ii;
    if (u < 0 || u >= a.Lin) continue;
    const int dq = ii / s, r = ii - dq * s;
    float gs = 0.f;
    for (int m = 0, j = r; j < k; ++m, j += s) gs = fmaf(wl[j], dzs[NA - 1 + dq - m], gs);
    if (HAS_BN) {
      const float yv = yb[u];
      gs *= dk_gate(fmaf(yv, sc, sh));
      sg += gs;
      sgx = fmaf(gs, (yv - mean) * rstd, sgx);
    }
    a.g[b * (int64_t)a.Lin + u] = gs;
  }
  const float tg = dk1_block_sum(red, sg);
  const float tgx = dk1_block_sum(red, sgx);
  if (tid == 0) {
    prow[0] = tg;
    prow[1] = tgx;
  }
}

// part[n_parts][2 + k][C] -> dbeta, dgamma, coef, dw[k][C]; 256 threads = 16 channels x 16 row groups (row group r takes rows
// r, r + 16, ...; the groups are combined in order; double), blockIdx.y = row of the [2 + k] block
__global__ __launch_bounds__(256) void dk_finalize_kernel(const float* __restrict__ part, int n_parts, double inv_count, int C, int k,
                                                          float* dw, float* dgamma, float* dbeta, float* coef) {
  __shared__ double red[16][16];
  const int cg = threadIdx.x & 15, rg = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cg, row = blockIdx.y;
  double sum = 0.0;
  if (c < C)
    for (int t = rg; t < n_parts; t += 16) sum += (double)part[((int64_t)t * (2 + k) + row) * C + c];
  red[rg][cg] = sum;
  __syncthreads();
  if (rg == 0 && c < C) {
    double tot = 0.0;
    for (int r = 0; r < 16; ++r) tot += red[r][cg];
    if (row == 0) {
      if (dbeta) dbeta[c] = (float)tot;
      if (coef) coef[c] = (float)(tot * inv_count);
    } else if (row == 1) {
      if (dgamma) dgamma[c] = (float)tot;
      if (coef) coef[C + c] = (float)(tot * inv_count);
    } else if (dw) {
      dw[(int64_t)(row - 2) * C + c] = (float)tot;
    }
  }
}

// ---- pointwise convolution 1 -> N ---------------------------------------------------------------------------------------------
constexpr int PW1_ROWS = 512;   // rows of z per workgroup = per statistics row

struct Pw1Args {
  const float* z; const float* p; const float* dy;
  float* y; float* stats; float* dz; float* ws;
  int64_t M; int N;
};

// y[m, n] = z[m] * p[n]; stats row blockIdx.x = (sum_m y, sum_m y^2) of its rows, the R row lanes folded in order
__global__ __launch_bounds__(DK_THREADS) void pw1_fwd_kernel(Pw1Args a) {
  __shared__ float red[2][DK_THREADS * 4];
  const int N4 = a.N >> 2, R = DK_THREADS / N4;
  const int rr = threadIdx.x / N4, n4 = threadIdx.x - rr * N4;
  const float4 p = dk_ld4(a.p + n4 * 4);
  float4 s1 = dk_zero(), s2 = dk_zero();
  const int64_t m0 = (int64_t)blockIdx.x * PW1_ROWS;
  for (int i = rr; i < PW1_ROWS; i += R) {
    const int64_t m = m0 + i;
    if (m >= a.M) break;
    const float zv = a.z[m];
    const float4 o = make_float4(zv * p.x, zv * p.y, zv * p.z, zv * p.w);
    dk_st4(a.y + m * a.N + n4 * 4, o);
    s1.x += o.x; s1.y += o.y; s1.z += o.z; s1.w += o.w;
    s2 = dk_fma(o, o, s2);
  }
  if (!a.stats) return;
  dk_st4(&red[0][threadIdx.x * 4], s1);
  dk_st4(&red[1][threadIdx.x * 4], s2);
  __syncthreads();
  for (int o = threadIdx.x; o < 2 * a.N; o += DK_THREADS) {
    const int q = o / a.N, ch = o - q * a.N;
    float sum = 0.f;
    for (int r = 0; r < R; ++r) sum += red[q][r * a.N + ch];
    a.stats[((int64_t)blockIdx.x * 2 + q) * a.N + ch] = sum;
  }
}

// dz[m] = sum_n dy[m, n] p[n] (the N / 4 lanes of a row folded by a butterfly of fixed shape); ws row blockIdx.x = this
// workgroup's part of dp[n] = sum_m z[m] dy[m, n]
__global__ __launch_bounds__(DK_THREADS) void pw1_bwd_kernel(Pw1Args a) {
  __shared__ float red[DK_THREADS * 4];
  const int N4 = a.N >> 2, R = DK_THREADS / N4;
  const int rr = threadIdx.x / N4, n4 = threadIdx.x - rr * N4;
  const float4 p = dk_ld4(a.p + n4 * 4);
  float4 dp = dk_zero();
  const int64_t m0 = (int64_t)blockIdx.x * PW1_ROWS;
  for (int i = rr; i < PW1_ROWS; i += R) {   // a row's N4 lanes sit in one wave (N4 is a power of two <= 64) and leave together
    const int64_t m = m0 + i;
    if (m >= a.M) break;
    const float4 d = dk_ld4(a.dy + m * a.N + n4 * 4);
    float dot = fmaf(d.w, p.w, fmaf(d.z, p.z, fmaf(d.y, p.y, d.x * p.x)));
    for (int o = N4 >> 1; o > 0; o >>= 1) dot += __shfl_xor(dot, o);
    if (n4 == 0) a.dz[m] = dot;
    const float zv = a.z[m];
    dp.x = fmaf(zv, d.x, dp.x); dp.y = fmaf(zv, d.y, dp.y); dp.z = fmaf(zv, d.z, dp.z); dp.w = fmaf(zv, d.w, dp.w);
  }
  dk_st4(red + threadIdx.x * 4, dp);
  __syncthreads();
  for (int o = threadIdx.x; o < a.N; o += DK_THREADS) {
    float sum = 0.f;
    for (int r = 0; r < R; ++r) sum += red[r * a.N + o];
    a.ws[(int64_t)blockIdx.x * a.N + o] = sum;
  }
}

// dp[n] = sum over the workspace rows, 16 row groups combined in order (double)
__global__ __launch_bounds__(256) void pw1_fold_kernel(const float* __restrict__ ws, int rows, int N, float* __restrict__ dp) {
  __shared__ double red[16][16];
  const int cg = threadIdx.x & 15, rg = threadIdx.x >> 4;
  const int n = blockIdx.x * 16 + cg;
  double sum = 0.0;
  if (n < N)
    for (int t = rg; t < rows; t += 16) sum += (double)ws[(int64_t)t * N + n];
  red[rg][cg] = sum;
  __syncthreads();
  if (rg == 0 && n < N) {
    double tot = 0.0;
    for (int r = 0; r < 16; ++r) tot += red[r][cg];
    dp[n] = (float)tot;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
bool dk_c_ok(int C) { return C == 1 || (C > 0 && C % 4 == 0 && C <= DK_MAXC); }

int dk_check(const char* who, int B, int L_in, int L_out, int C, int k, int stride, int pad_l) {
  KWS_REQUIRE(B > 0 && L_in > 0 && L_out > 0, "%s: bad shape B=%d L=%d->%d", who, B, L_in, L_out);
  KWS_REQUIRE(dk_c_ok(C), "%s: C=%d (1, or a multiple of 4 up to %d)", who, C, DK_MAXC);
  KWS_REQUIRE(k >= 1 && k <= DK_MAXK, "%s: %d taps (1 .. %d)", who, k, DK_MAXK);
  KWS_REQUIRE(stride >= 1 && stride <= DK_MAXS, "%s: stride %d (1 .. %d)", who, stride, DK_MAXS);
  KWS_REQUIRE(pad_l >= 0 && pad_l < k, "%s: pad_l %d outside [0, %d)", who, pad_l, k);
  KWS_REQUIRE((int64_t)stride * (L_out - 1) + k - pad_l <= (int64_t)L_in + (k - 1), "%s: geometry reads past the padding (L %d->%d k=%d s=%d pad_l=%d)",
              who, L_in, L_out, k, stride, pad_l);
  return KWS_OK;
}

// stride groups that hold an input row for any pad_l < k: the backward's runs (and its partial rows) do not depend on pad_l
int dk_groups(int L_in, int k, int s) { return (L_in + k - 2) / s + 1; }

struct DkGeom {
  int cq, nslices, R, block, nruns;
  int64_t units, grid;
};
DkGeom dk_geom(int B, int C, int steps, int per_run) {
  DkGeom ge;
  const int C4 = C / 4;
  ge.cq = C4 < DK_CQ ? C4 : DK_CQ;
  ge.nslices = ceil_div(C4, ge.cq);
  ge.R = DK_THREADS / ge.cq;
  ge.block = ge.R * ge.cq;
  ge.nruns = ceil_div(steps, per_run);
  ge.units = (int64_t)B * ge.nruns;
  ge.grid = ceil_div64(ge.units, ge.R);
  return ge;
}

template <bool HAS_BN>
void dk_launch_fwd(const DkArgs& a, const DkGeom& ge, int NA, hipStream_t st) {
  const dim3 gr((unsigned)ge.grid, (unsigned)ge.nslices), bl((unsigned)ge.block);
  const size_t lds = (size_t)(a.k + 1) * a.cq * sizeof(float4);
#define DK_FWD(na)                                                                                       \
  do {                                                                                                   \
    if (a.s % 4 == 0) hipLaunchKernelGGL((dk_fwd_ring_kernel<na, HAS_BN, 4>), gr, bl, lds, st, a);        \
    else hipLaunchKernelGGL((dk_fwd_ring_kernel<na, HAS_BN, 1>), gr, bl, lds, st, a);                     \
  } while (0)
  if (NA == 1) DK_FWD(1);
  else if (NA == 2) DK_FWD(2);
  else if (NA == 3) DK_FWD(3);
  else if (NA == 4) DK_FWD(4);
  else if (NA <= 6) DK_FWD(6);
  else if (NA <= DK_MAXNA) DK_FWD(8);
  else hipLaunchKernelGGL((dk_fwd_direct_kernel<HAS_BN>), gr, bl, lds, st, a);
#undef DK_FWD
}

template <bool HAS_BN>
void dk_launch_bwd(const DkArgs& a, const DkGeom& ge, int NA, hipStream_t st) {
  const dim3 gr((unsigned)ge.grid, (unsigned)ge.nslices), bl((unsigned)ge.block);
  const size_t lds = (size_t)(a.k + 1) * a.cq * sizeof(float4);
  if (NA == 1) hipLaunchKernelGGL((dk_bwd_ring_kernel<1, HAS_BN>), gr, bl, lds, st, a);
  else if (NA == 2) hipLaunchKernelGGL((dk_bwd_ring_kernel<2, HAS_BN>), gr, bl, lds, st, a);
  else if (NA == 3) hipLaunchKernelGGL((dk_bwd_ring_kernel<3, HAS_BN>), gr, bl, lds, st, a);
  else if (NA == 4) hipLaunchKernelGGL((dk_bwd_ring_kernel<4, HAS_BN>), gr, bl, lds, st, a);
  else if (NA <= 6) hipLaunchKernelGGL((dk_bwd_ring_kernel<6, HAS_BN>), gr, bl, lds, st, a);
  else if (NA <= DK_MAXNA) hipLaunchKernelGGL((dk_bwd_ring_kernel<8, HAS_BN>), gr, bl, lds, st, a);
  else hipLaunchKernelGGL((dk_bwd_direct_kernel<HAS_BN>), gr, bl, lds, st, a);
}

bool pw1_n_ok(int N) { return N >= 4 && N <= 256 && (N & (N - 1)) == 0; }

}  // namespace

extern "C" {

int kws_dwconvk_fwd_f32(const float* y, const float* bn, const float* w, float* z, int B, int L_in, int L_out, int C, int k,
                        int stride, int pad_l, void* stream) {
  KWS_REQUIRE(y && w && z, "dwconvk_fwd: NULL pointer");
  KWS_TRY(dk_check("dwconvk_fwd", B, L_in, L_out, C, k, stride, pad_l));
  hipStream_t st = (hipStream_t)stream;
  DkArgs a;
  memset(&a, 0, sizeof(a));
  a.y = y; a.bn = bn; a.w = w; a.z = z;
  a.B = B; a.Lin = L_in; a.Lout = L_out; a.C = C; a.k = k; a.s = stride; a.pad_l = pad_l;
  KwsProfScope prof("dwconvk_fwd", 2.0 * k * B * L_out * C, 4.0 * ((double)B * L_in * C + (double)B * L_out * C), st);
  if (C == 1) {
    a.nruns = ceil_div(L_out, DK1_TB);
    const int64_t grid = (int64_t)B * a.nruns;
    KWS_REQUIRE(grid < (1ll << 31), "dwconvk_fwd: tensor too large");
    if (bn) hipLaunchKernelGGL((dk1_fwd_kernel<true>), dim3((unsigned)grid), dim3(DK1_TB), 0, st, a);
    else hipLaunchKernelGGL((dk1_fwd_kernel<false>), dim3((unsigned)grid), dim3(DK1_TB), 0, st, a);
    KWS_LAUNCH_CHECK("dk1_fwd_kernel");
    return KWS_OK;
  }
  const DkGeom ge = dk_geom(B, C, L_out, DK_FWD_TT);
  KWS_REQUIRE(ge.grid < (1ll << 31), "dwconvk_fwd: tensor too large");
  a.cq = ge.cq; a.R = ge.R; a.nruns = ge.nruns; a.units = ge.units;
  const int NA = ceil_div(k, stride);
  if (bn) dk_launch_fwd<true>(a, ge, NA, st);
  else dk_launch_fwd<false>(a, ge, NA, st);
  KWS_LAUNCH_CHECK("dk_fwd_kernel");
  return KWS_OK;
}

int kws_dwconvk_bwd_part_rows(int B, int L_in, int C, int k, int stride) {
  if (B <= 0 || L_in <= 0 || !dk_c_ok(C) || k < 1 || k > DK_MAXK || stride < 1 || stride > DK_MAXS) return 0;
  const int Q = dk_groups(L_in, k, stride);
  const int64_t rows = C == 1 ? (int64_t)B * ceil_div(Q, DK1_TB) : dk_geom(B, C, Q, DK_BWD_QT).grid;
  return rows < (1ll << 31) ? (int)rows : 0;
}

int64_t kws_dwconvk_bwd_part_floats(int B, int L_in, int C, int k, int stride) {
  return (int64_t)kws_dwconvk_bwd_part_rows(B, L_in, C, k, stride) * (2 + k) * C;
}

int kws_dwconvk_bwd_f32(const float* dz, const float* y, const float* bn, const float* w, float* g, float* part, int B, int L_in,
                        int L_out, int C, int k, int stride, int pad_l, void* stream) {
  KWS_REQUIRE(dz && y && w && g && part, "dwconvk_bwd: NULL pointer");
  KWS_TRY(dk_check("dwconvk_bwd", B, L_in, L_out, C, k, stride, pad_l));
  const int rows = kws_dwconvk_bwd_part_rows(B, L_in, C, k, stride);
  KWS_REQUIRE(rows > 0, "dwconvk_bwd: tensor too large");
  hipStream_t st = (hipStream_t)stream;
  DkArgs a;
  memset(&a, 0, sizeof(a));
  a.y = y; a.bn = bn; a.w = w; a.dz = dz; a.g = g; a.part = part;
  a.B = B; a.Lin = L_in; a.Lout = L_out; a.C = C; a.k = k; a.s = stride; a.pad_l = pad_l;
  a.Q = dk_groups(L_in, k, stride);
  const int NA = ceil_div(k, stride);
  KwsProfScope prof("dwconvk_bwd", 4.0 * k * B * L_out * C, 4.0 * (2.0 * B * L_in * C + (double)B * L_out * C), st);
  if (C == 1) {
    a.nruns = ceil_div(a.Q, DK1_TB);
    if (bn) hipLaunchKernelGGL((dk1_bwd_kernel<true>), dim3((unsigned)rows), dim3(DK1_TB), 0, st, a, NA);
    else hipLaunchKernelGGL((dk1_bwd_kernel<false>), dim3((unsigned)rows), dim3(DK1_TB), 0, st, a, NA);
    KWS_LAUNCH_CHECK("dk1_bwd_kernel");
    return KWS_OK;
  }
  const DkGeom ge = dk_geom(B, C, a.Q, DK_BWD_QT);
  a.cq = ge.cq; a.R = ge.R; a.nruns = ge.nruns; a.units = ge.units;
  if (bn) dk_launch_bwd<true>(a, ge, NA, st);
  else dk_launch_bwd<false>(a, ge, NA, st);
  KWS_LAUNCH_CHECK("dk_bwd_kernel");
  return KWS_OK;
}

int kws_dwconvk_bwd_finalize(const float* part, int n_parts, int64_t count, int C, int k, float* dw, float* dgamma, float* dbeta,
                             float* coef, void* stream) {
  KWS_REQUIRE(part && n_parts > 0 && count > 0 && C > 0 && k >= 1 && k <= DK_MAXK, "dwconvk_bwd_finalize: bad arguments (n_parts=%d C=%d k=%d)",
              n_parts, C, k);
  KwsProfScope prof("bn_finalize", 0.0, 4.0 * (2 + k) * (double)n_parts * C, (hipStream_t)stream);
  hipLaunchKernelGGL(dk_finalize_kernel, dim3((unsigned)ceil_div(C, 16), (unsigned)(2 + k)), dim3(256), 0, (hipStream_t)stream, part,
                     n_parts, 1.0 / (double)count, C, k, dw, dgamma, dbeta, coef);
  KWS_LAUNCH_CHECK("dk_finalize_kernel");
  return KWS_OK;
}

int kws_dwconvk_pw1_stats_rows(int64_t M) { return M > 0 && ceil_div64(M, PW1_ROWS) < (1ll << 31) ? (int)ceil_div64(M, PW1_ROWS) : 0; }

int kws_dwconvk_pw1_fwd_f32(const float* z, const float* p, float* y, int64_t M, int N, float* stats_part, void* stream) {
  KWS_REQUIRE(z && p && y, "dwconvk_pw1_fwd: NULL pointer");
  KWS_REQUIRE(M > 0 && kws_dwconvk_pw1_stats_rows(M) > 0 && pw1_n_ok(N), "dwconvk_pw1_fwd: M=%lld N=%d (N a power of two, 4 .. 256)",
              (long long)M, N);
  Pw1Args a;
  memset(&a, 0, sizeof(a));
  a.z = z; a.p = p; a.y = y; a.stats = stats_part; a.M = M; a.N = N;
  KwsProfScope prof("dwconvk_pw1", 3.0 * M * N, 4.0 * ((double)M + (double)M * N), (hipStream_t)stream);
  hipLaunchKernelGGL(pw1_fwd_kernel, dim3((unsigned)kws_dwconvk_pw1_stats_rows(M)), dim3(DK_THREADS), 0, (hipStream_t)stream, a);
  KWS_LAUNCH_CHECK("pw1_fwd_kernel");
  return KWS_OK;
}

int64_t kws_dwconvk_pw1_bwd_workspace_floats(int64_t M, int N) {
  return pw1_n_ok(N) ? (int64_t)kws_dwconvk_pw1_stats_rows(M) * N : 0;
}

int kws_dwconvk_pw1_bwd_f32(const float* dy, const float* z, const float* p, float* dz, float* dp, int64_t M, int N, float* workspace,
                            void* stream) {
  KWS_REQUIRE(dy && z && p && dz && dp && workspace, "dwconvk_pw1_bwd: NULL pointer");
  KWS_REQUIRE(M > 0 && kws_dwconvk_pw1_stats_rows(M) > 0 && pw1_n_ok(N), "dwconvk_pw1_bwd: M=%lld N=%d (N a power of two, 4 .. 256)",
              (long long)M, N);
  Pw1Args a;
  memset(&a, 0, sizeof(a));
  a.z = z; a.p = p; a.dy = dy; a.dz = dz; a.ws = workspace; a.M = M; a.N = N;
  const int rows = kws_dwconvk_pw1_stats_rows(M);
  KwsProfScope prof("dwconvk_pw1", 4.0 * M * N, 4.0 * (2.0 * M + (double)M * N), (hipStream_t)stream);
  hipLaunchKernelGGL(pw1_bwd_kernel, dim3((unsigned)rows), dim3(DK_THREADS), 0, (hipStream_t)stream, a);
  KWS_LAUNCH_CHECK("pw1_bwd_kernel");
  hipLaunchKernelGGL(pw1_fold_kernel, dim3((unsigned)ceil_div(N, 16)), dim3(256), 0, (hipStream_t)stream, workspace, rows, N, dp);
  KWS_LAUNCH_CHECK("pw1_fold_kernel");
  return KWS_OK;
}

}  // extern "C"
