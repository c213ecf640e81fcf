// The first block of a raw-waveform branch whose input view is narrow: conv_1d_multi_time_sliced_model (model.py:1105-1140)
// reshapes the 16000 samples to [4000, 4], [3200, 5] and [640, 25] and runs _depthwise_conv_block on each view.  5 and 25 channels
// are outside kws_dwconvk_* (C = 1 or C % 4 == 0) and outside the GEMMs (K % 4 == 0), so the 3-tap VALID depthwise convolution
// and the pointwise C -> N product are ONE kernel here, for any C = 1 .. 32 and N = 4, 8 .. 64:
//   fwd   y[b,t,n] = sum_c p[c,n] * z[b,t,c],  z[b,t,c] = sum_{j<3} w[j,c] * x[b,t+j,c],  t < L - 2
//         stats_part (may be NULL): kws_stem_stats_rows(B, L) rows [2][N] of (sum y, sum y^2), one per workgroup, for
//         kws_bn_stats_finalize
//   bwd   dp[c,n] = sum_{b,t} z[b,t,c] * dy[b,t,n],  dw[j,c] = sum_{b,t} x[b,t+j,c] * dz[b,t,c],  dz[b,t,c] = sum_n dy[b,t,n] p[c,n]
//         z is recomputed from x (the forward never writes it); no gradient leaves the input.  Each workgroup adds its tiles in
//         ascending order into one partial row [C N + 3 C], the rows are folded in a fixed order: no atomics, bit-reproducible.
// Both directions stream y / dy once (the forward writes B (L - 2) N floats and reads x once) and work out of LDS: a workgroup
// stages a tile of rows of x, the tile of z, and the two small kernels; a thread owns one quad of output columns and up to 8 rows
// (forward), or up to two (c, n-quad) pairs of dp and one (j, c) of dw (backward) - never C N accumulators.
// Rows of x are C floats: for C = 5 or 25 they are not 16-byte aligned, so a tile is loaded as the contiguous run of floats it
// is, with float4 loads where the run starts on a 16-byte boundary.
#include "common.h"
#include "internal.h"

namespace {

constexpr int ST_THREADS = 256;
constexpr int ST_MAXC = 32, ST_MAXN = 64;
constexpr int ST_FWD_TR = 128;     // output rows per forward tile
constexpr int ST_FWD_RPT = 8;      // rows per thread: 8 * (256 / (N / 4)) >= ST_FWD_TR for every N <= 64
constexpr int ST_BWD_TR = 64;      // output rows per backward tile
constexpr int ST_BWD_MAX_ROWS = 1024;   // partial rows (= workgroups) of the backward

// cnt floats from src (global) to dst (LDS); float4 loads when src starts on a 16-byte boundary
__device__ __forceinline__ void st_load_run(const float* __restrict__ src, int64_t base, int cnt, float* dst) {
  const int tid = threadIdx.x;
  if ((base & 3) == 0) {
    const int n4 = cnt >> 2;
    const float4* s4 = reinterpret_cast<const float4*>(src + base);
    for (int i = tid; i < n4; i += ST_THREADS) {
      const float4 v = s4[i];
      dst[4 * i] = v.x; dst[4 * i + 1] = v.y; dst[4 * i + 2] = v.z; dst[4 * i + 3] = v.w;
    }
    for (int i = 4 * n4 + tid; i < cnt; i += ST_THREADS) dst[i] = src[base + i];
  } else {
    for (int i = tid; i < cnt; i += ST_THREADS) dst[i] = src[base + i];
  }
}

// zs[r][c] (row pitch ZS) = sum_j ws[j][c] * xs[r + j][c] for the tile's rows
__device__ __forceinline__ void st_depthwise_tile(const float* xs, const float* ws, float* zs, int rows, int C, int ZS) {
  for (int e = threadIdx.x; e < rows * C; e += ST_THREADS) {
    const int r = e / C, c = e - r * C;
    zs[r * ZS + c] = fmaf(ws[2 * C + c], xs[(r + 2) * C + c], fmaf(ws[C + c], xs[(r + 1) * C + c], ws[c] * xs[r * C + c]));
  }
}

__global__ __launch_bounds__(ST_THREADS) void stem_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ p, float* __restrict__ y,
                                                              float* __restrict__ stats, int L, int Lout, int C, int N, int tpc) {
  __shared__ float xs[(ST_FWD_TR + 2) * ST_MAXC];
  __shared__ float zs[ST_FWD_TR * (ST_MAXC + 1)];
  __shared__ __attribute__((aligned(16))) float ps[ST_MAXC * ST_MAXN];
  __shared__ float ws[3 * ST_MAXC];
  __shared__ __attribute__((aligned(16))) float red[2][ST_THREADS * 4];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x / tpc;
  const int t0 = (int)(blockIdx.x - b * tpc) * ST_FWD_TR;
  const int rows = Lout - t0 < ST_FWD_TR ? Lout - t0 : ST_FWD_TR;
  const int ZS = C | 1;
  st_load_run(x, (b * L + t0) * (int64_t)C, (rows + 2) * C, xs);
  for (int i = tid; i < C * N; i += ST_THREADS) ps[i] = p[i];
  if (tid < 3 * C) ws[tid] = w[tid];
  __syncthreads();
  st_depthwise_tile(xs, ws, zs, rows, C, ZS);
  __syncthreads();
  const int Q = N >> 2, R = ST_THREADS / Q;
  const int q = tid % Q, r0 = tid / Q;
  int nI = (tid < R * Q && r0 < rows) ? (rows - r0 + R - 1) / R : 0;   // this thread's rows: r0, r0 + R, ...
  if (nI > ST_FWD_RPT) nI = ST_FWD_RPT;
  float4 acc[ST_FWD_RPT];
#pragma unroll
  for (int i = 0; i < ST_FWD_RPT; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int c = 0; c < C; ++c) {
    const float4 pv = *reinterpret_cast<const float4*>(&ps[c * N + 4 * q]);
#pragma unroll
    for (int i = 0; i < ST_FWD_RPT; ++i) {
      if (i < nI) {
        const float zv = zs[(r0 + i * R) * ZS + c];
        acc[i].x = fmaf(zv, pv.x, acc[i].x);
        acc[i].y = fmaf(zv, pv.y, acc[i].y);
        acc[i].z = fmaf(zv, pv.z, acc[i].z);
        acc[i].w = fmaf(zv, pv.w, acc[i].w);
      }
    }
  }
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s;
  float* yb = y + (b * Lout + t0) * (int64_t)N + 4 * q;
#pragma unroll
  for (int i = 0; i < ST_FWD_RPT; ++i) {
    if (i < nI) {
      *reinterpret_cast<float4*>(yb + (int64_t)(r0 + i * R) * N) = acc[i];
      s.x += acc[i].x; s.y += acc[i].y; s.z += acc[i].z; s.w += acc[i].w;
      s2.x = fmaf(acc[i].x, acc[i].x, s2.x); s2.y = fmaf(acc[i].y, acc[i].y, s2.y);
      s2.z = fmaf(acc[i].z, acc[i].z, s2.z); s2.w = fmaf(acc[i].w, acc[i].w, s2.w);
    }
  }
  if (stats == nullptr) return;
  *reinterpret_cast<float4*>(&red[0][tid * 4]) = s;
  *reinterpret_cast<float4*>(&red[1][tid * 4]) = s2;
  __syncthreads();
  for (int o = tid; o < 2 * N; o += ST_THREADS) {   // the R thread rows of this workgroup, ascending
    const int k = o / N, n = o - k * N;
    float sum = 0.f;
    for (int rr = 0; rr < R; ++rr) sum += red[k][(rr * Q + (n >> 2)) * 4 + (n & 3)];
    stats[((int64_t)blockIdx.x * 2 + k) * N + n] = sum;
  }
}

// Workgroup g adds the tiles g * tpw .. (g + 1) * tpw - 1 (tile = ST_BWD_TR output rows of one clip) into part[g][C N + 3 C] (row pitch ES: that
// rounded up to 4 floats, so that a row starts on a 16-byte boundary).
__global__ __launch_bounds__(ST_THREADS) void stem_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                              const float* __restrict__ w, const float* __restrict__ p,
                                                              float* __restrict__ part, int L, int Lout, int C, int N, int tpc,
                                                              int64_t tiles, int tpw, int ES) {
  __shared__ float xs[(ST_BWD_TR + 2) * ST_MAXC];
  __shared__ float zs[ST_BWD_TR * (ST_MAXC + 1)];
  __shared__ float dzs[ST_BWD_TR * (ST_MAXC + 1)];
  __shared__ __attribute__((aligned(16))) float dys[ST_BWD_TR * ST_MAXN];
  __shared__ float ps[ST_MAXC * (ST_MAXN + 1)];
  __shared__ float ws[3 * ST_MAXC];
  const int tid = threadIdx.x;
  const int ZS = C | 1, PS = N + 1, Q = N >> 2;
  for (int i = tid; i < C * N; i += ST_THREADS) ps[(i / N) * PS + i % N] = p[i];
  if (tid < 3 * C) ws[tid] = w[tid];
  // this thread's accumulators: pairs (c, n-quad) number tid and tid + 256 of the C Q pairs, and (j, c) = tid of the 3 C taps
  const int pid0 = tid, pid1 = tid + ST_THREADS;
  const bool has0 = pid0 < C * Q, has1 = pid1 < C * Q, has_w = tid < 3 * C;
  const int c0 = has0 ? pid0 / Q : 0, q0 = has0 ? pid0 % Q : 0;
  const int c1 = has1 ? pid1 / Q : 0, q1 = has1 ? pid1 % Q : 0;
  const int jw = has_w ? tid / C : 0, cw = has_w ? tid % C : 0;
  float4 dp0 = make_float4(0.f, 0.f, 0.f, 0.f), dp1 = dp0;
  float dwv = 0.f;
  const int64_t tile0 = (int64_t)blockIdx.x * tpw;
  const int64_t tile1 = tile0 + tpw < tiles ? tile0 + tpw : tiles;
  for (int64_t tile = tile0; tile < tile1; ++tile) {
    const int64_t b = tile / tpc;
    const int t0 = (int)(tile - b * tpc) * ST_BWD_TR;
    const int rows = Lout - t0 < ST_BWD_TR ? Lout - t0 : ST_BWD_TR;
    __syncthreads();   // the previous tile's readers are done (and ps / ws are in place)
    st_load_run(x, (b * L + t0) * (int64_t)C, (rows + 2) * C, xs);
    st_load_run(dy, (b * Lout + t0) * (int64_t)N, rows * N, dys);
    __syncthreads();
    st_depthwise_tile(xs, ws, zs, rows, C, ZS);
    // dz[r][c] = sum_n dy[r][n] p[c][n]: one thread = one c and four consecutive rows
    const int rg = (rows + 3) >> 2;
    for (int e = tid; e < rg * C; e += ST_THREADS) {
      const int g4 = e / C, c = e - g4 * C;
      float a[4] = {0.f, 0.f, 0.f, 0.f};
      for (int n = 0; n < N; n += 4) {
        const float p0 = ps[c * PS + n], p1 = ps[c * PS + n + 1], p2 = ps[c * PS + n + 2], p3 = ps[c * PS + n + 3];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = 4 * g4 + i < rows ? 4 * g4 + i : rows - 1;   // a row of the tile (the duplicate is not stored)
          const float4 d = *reinterpret_cast<const float4*>(&dys[r * N + n]);
          a[i] = fmaf(d.w, p3, fmaf(d.z, p2, fmaf(d.y, p1, fmaf(d.x, p0, a[i]))));
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (4 * g4 + i < rows) dzs[(4 * g4 + i) * ZS + c] = a[i];
    }
    __syncthreads();
    if (has0) {
      for (int r = 0; r < rows; ++r) {
        const float zv = zs[r * ZS + c0];
        const float4 d = *reinterpret_cast<const float4*>(&dys[r * N + 4 * q0]);
        dp0.x = fmaf(zv, d.x, dp0.x); dp0.y = fmaf(zv, d.y, dp0.y); dp0.z = fmaf(zv, d.z, dp0.z); dp0.w = fmaf(zv, d.w, dp0.w);
      }
    }
    if (has1) {
      for (int r = 0; r < rows; ++r) {
        const float zv = zs[r * ZS + c1];
        const float4 d = *reinterpret_cast<const float4*>(&dys[r * N + 4 * q1]);
        dp1.x = fmaf(zv, d.x, dp1.x); dp1.y = fmaf(zv, d.y, dp1.y); dp1.z = fmaf(zv, d.z, dp1.z); dp1.w = fmaf(zv, d.w, dp1.w);
      }
    }
    if (has_w)
      for (int r = 0; r < rows; ++r) dwv = fmaf(xs[(r + jw) * C + cw], dzs[r * ZS + cw], dwv);
  }
  float* out = part + (int64_t)blockIdx.x * ES;
  if (has0) *reinterpret_cast<float4*>(out + 4 * pid0) = dp0;   // pair (c, q) = element c N + 4 q = 4 pid
  if (has1) *reinterpret_cast<float4*>(out + 4 * pid1) = dp1;
  if (has_w) out[C * N + tid] = dwv;
}

// dp[e] / dw[e - C N] = sum over the partial rows, four interleaved chains combined in a fixed order
__global__ __launch_bounds__(ST_THREADS) void stem_bwd_fold_kernel(const float* __restrict__ part, int rows, int CN, int E, int ES,
                                                                   float* __restrict__ dp, float* __restrict__ dw) {
  const int e = blockIdx.x * ST_THREADS + threadIdx.x;
  if (e >= E) return;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int r = 0;
  for (; r + 3 < rows; r += 4) {
    s0 += part[(int64_t)r * ES + e];
    s1 += part[(int64_t)(r + 1) * ES + e];
    s2 += part[(int64_t)(r + 2) * ES + e];
    s3 += part[(int64_t)(r + 3) * ES + e];
  }
  for (; r < rows; ++r) s0 += part[(int64_t)r * ES + e];
  const float s = (s0 + s1) + (s2 + s3);
  if (e < CN) dp[e] = s;
  else dw[e - CN] = s;
}

bool st_ok(int B, int L, int C, int N) {
  return B > 0 && L >= 3 && C >= 1 && C <= ST_MAXC && N >= 4 && N <= ST_MAXN && N % 4 == 0;
}
int st_row_pitch(int C, int N) { return (C * N + 3 * C + 3) & ~3; }
struct StBwdGeom {
  int tpc, tpw, rows;
  int64_t tiles;
};
StBwdGeom st_bwd_geom(int B, int L) {
  StBwdGeom ge;
  ge.tpc = ceil_div(L - 2, ST_BWD_TR);
  ge.tiles = (int64_t)B * ge.tpc;
  ge.tpw = (int)ceil_div64(ge.tiles, ST_BWD_MAX_ROWS);
  ge.rows = (int)ceil_div64(ge.tiles, ge.tpw);
  return ge;
}

}  // namespace

extern "C" {

int kws_stem_stats_rows(int B, int L) {
  if (B <= 0 || L < 3) return 0;
  const int64_t rows = (int64_t)B * ceil_div(L - 2, ST_FWD_TR);
  return rows < (1ll << 31) ? (int)rows : 0;
}

int kws_stem_fwd_f32(const float* x, const float* w, const float* p, float* y, int B, int L, int C, int N, float* stats_part,
                     void* stream) {
  KWS_REQUIRE(x && w && p && y, "stem_fwd: NULL pointer");
  KWS_REQUIRE(st_ok(B, L, C, N) && kws_stem_stats_rows(B, L) > 0, "stem_fwd: B=%d L=%d C=%d N=%d (L >= 3, C 1 .. %d, N %% 4 == 0 up to %d)", B,
              L, C, N, ST_MAXC, ST_MAXN);
  const int Lout = L - 2;
  KwsProfScope prof("stem_fwd", 2.0 * B * Lout * C * (N + 3.0), 4.0 * ((double)B * L * C + (double)B * Lout * N), (hipStream_t)stream);
  hipLaunchKernelGGL(stem_fwd_kernel, dim3((unsigned)kws_stem_stats_rows(B, L)), dim3(ST_THREADS), 0, (hipStream_t)stream, x, w, p, y,
                     stats_part, L, Lout, C, N, ceil_div(Lout, ST_FWD_TR));
  KWS_LAUNCH_CHECK("stem_fwd_kernel");
  return KWS_OK;
}

int64_t kws_stem_bwd_workspace_floats(int B, int L, int C, int N) {
  if (!st_ok(B, L, C, N)) return 0;
  return (int64_t)st_bwd_geom(B, L).rows * st_row_pitch(C, N);
}

int kws_stem_bwd_f32(const float* dy, const float* x, const float* w, const float* p, float* dw, float* dp, int B, int L, int C,
                     int N, float* workspace, void* stream) {
  KWS_REQUIRE(dy && x && w && p && dw && dp && workspace, "stem_bwd: NULL pointer");
  KWS_REQUIRE(st_ok(B, L, C, N), "stem_bwd: B=%d L=%d C=%d N=%d (L >= 3, C 1 .. %d, N %% 4 == 0 up to %d)", B, L, C, N, ST_MAXC, ST_MAXN);
  const int Lout = L - 2;
  const StBwdGeom ge = st_bwd_geom(B, L);
  const int E = C * N + 3 * C;
  KwsProfScope prof("stem_bwd", 2.0 * B * Lout * C * (2.0 * N + 6.0), 4.0 * ((double)B * L * C + (double)B * Lout * N), (hipStream_t)stream);
  hipLaunchKernelGGL(stem_bwd_kernel, dim3((unsigned)ge.rows), dim3(ST_THREADS), 0, (hipStream_t)stream, dy, x, w, p, workspace, L, Lout, C,
                     N, ge.tpc, ge.tiles, ge.tpw, st_row_pitch(C, N));
  KWS_LAUNCH_CHECK("stem_bwd_kernel");
  hipLaunchKernelGGL(stem_bwd_fold_kernel, dim3((unsigned)ceil_div(E, ST_THREADS)), dim3(ST_THREADS), 0, (hipStream_t)stream, workspace,
                     ge.rows, C * N, E, st_row_pitch(C, N), dp, dw);
  KWS_LAUNCH_CHECK("stem_bwd_fold_kernel");
  return KWS_OK;
}

}  // extern "C"
