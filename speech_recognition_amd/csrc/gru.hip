// Bidirectional GRU of Keras 2.1.2 (GRUCell.call, implementation=1; Bidirectional, merge_mode='concat', return_sequences=False):
//   a_g = (x * mx_g) W_g + bias_g                      g in (z, r, h): column blocks of kernel [I, 3H]
//   z = hard_sigmoid(a_z + (h * mh_z) U_z)             hard_sigmoid(v) = clip(0.2 v + 0.5, 0, 1)
//   r = hard_sigmoid(a_r + (h * mh_r) U_r)
//   c = tanh(a_h + (r * h * mh_h) U_h)                 r BEFORE the product (no reset_after in 2.1.2)
//   h' = z h + (1 - z) c
// direction 0 walks t = 0 .. T-1, direction 1 walks t = T-1 .. 0, both from h = 0; the output is [h_fwd(T-1) | h_bwd(0)].
//
// The input projections are the project's f32 GEMMs over B T rows (kws_gru_fwd_f32 below).  The recurrence is ONE launch for
// the whole sequence and both directions: a workgroup of four waves owns 16 batch rows of one direction and all H units and
// loops over time.  Wave w owns the column tiles c = w, w + 4, ... (16 units each) of ALL three gates, so the lane that holds
// element (row, unit) of the z accumulator holds the same element of r, of the candidate and of h: h, z and the lane's mask
// values stay in registers for the whole sequence, and LDS carries only the three left operands of the products
// (h mh_z | h mh_r | r h mh_h, 16 x H each).  U is streamed from L2 as the B operand of mfma_f32_16x16x4f32 every step.
// Two dependent MFMA phases per step (z, r, then the candidate), two workgroup barriers, nothing between workgroups.
// Training saves z, r, c and h of every step; the backward kernel is the same structure run against time, carrying dh in
// registers, with the transposed gate blocks of U as B operands.
#include <algorithm>

#include "internal.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int GRU_ROWS = 16;      // batch rows of a workgroup = the M of one MFMA tile
constexpr int GRU_WAVES = 4;
constexpr int GRU_MAXH = 256;
constexpr int GRU_MAXT = 1024;
constexpr int GRU_HP = GRU_MAXH + 4;   // LDS row pitch
constexpr int GRU_COL_SLICES = 32;

__device__ __forceinline__ float gru_hsig(float v) { return fminf(fmaxf(fmaf(v, 0.2f, 0.5f), 0.f), 1.f); }
__device__ __forceinline__ float gru_hsig_grad(float s) { return (s > 0.f && s < 1.f) ? 0.2f : 0.f; }

struct GruFwdArgs {
  const float* a;                 // pre-activations: element (d, g, b, t, j) at a + d * dir_stride + g * gate_stride + (b T + t) * row_stride + j
  int64_t dir_stride, gate_stride;
  int row_stride;
  const float* U[2];              // [H, 3H]
  const float* bias[2];           // [3H]
  const float* mh;                // [2][3][B][H] or NULL
  float* out;                     // [B, 2H]
  float* save;                    // [2][4: z, r, c, h][B, T, H] or NULL
  int B, T, H;
};

template <int NT>
__global__ __launch_bounds__(GRU_WAVES * 64) void gru_seq_fwd_kernel(GruFwdArgs p) {
  __shared__ float lds[3][GRU_ROWS][GRU_HP];   // 0: h mh_z, 1: h mh_r, 2: r h mh_h
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int d = blockIdx.y, b0 = blockIdx.x * GRU_ROWS;
  const int H = p.H, T = p.T, B = p.B, H3 = 3 * H;
  const int ar = lane & 15, ak = lane >> 4;       // A operand: row ar, k offset ak; B operand: k offset ak, column ar
  const int ntiles = H / 16;
  int tcol[NT];   // first column of the wave's tiles; a wave without tile ti computes tile 0 again and drops the result (no branch in the product loops)
#pragma unroll
  for (int ti = 0; ti < NT; ++ti) tcol[ti] = (wave + GRU_WAVES * ti < ntiles ? wave + GRU_WAVES * ti : 0) * 16;
  const float* __restrict__ U = p.U[d];
  const float* __restrict__ bias = p.bias[d];
  const float* __restrict__ a = p.a + d * p.dir_stride;
  float h[NT][4], mz[NT][4], mr[NT][4], mhh[NT][4], bz[NT], br[NT], bh[NT];
#pragma unroll
  for (int ti = 0; ti < NT; ++ti) {
    const int tile = wave + GRU_WAVES * ti;
    const int col = tile * 16 + ar;
    const bool tv = tile < ntiles;
    bz[ti] = tv ? bias[col] : 0.f;
    br[ti] = tv ? bias[H + col] : 0.f;
    bh[ti] = tv ? bias[2 * H + col] : 0.f;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int b = b0 + 4 * ak + v;
      h[ti][v] = 0.f;
      mz[ti][v] = mr[ti][v] = mhh[ti][v] = 1.f;
      if (p.mh && tv && b < B) {
        const float* m = p.mh + ((int64_t)(d * 3) * B + b) * H + col;
        mz[ti][v] = m[0];
        mr[ti][v] = m[(int64_t)B * H];
        mhh[ti][v] = m[(int64_t)2 * B * H];
      }
    }
  }
  for (int i = threadIdx.x; i < 2 * GRU_ROWS * GRU_HP; i += GRU_WAVES * 64) (&lds[0][0][0])[i] = 0.f;   // h = 0
  __syncthreads();
  for (int s = 0; s < T; ++s) {
    const int t = d ? T - 1 - s : s;
    // this step's pre-activations of the lane's own elements (in flight under the first product)
    float az[NT][4], arr[NT][4], ah[NT][4];
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) {
      const int tile = wave + GRU_WAVES * ti;
      const int col = tile * 16 + ar;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int b = b0 + 4 * ak + v;
        const bool ok = tile < ntiles && b < B;
        const float* q = a + ((int64_t)b * T + t) * p.row_stride + col;
        az[ti][v] = ok ? q[0] : 0.f;
        arr[ti][v] = ok ? q[p.gate_stride] : 0.f;
        ah[ti][v] = ok ? q[2 * p.gate_stride] : 0.f;
      }
    }
    // ---- phase 1: z and r ----
    f32x4 accz[NT], accr[NT];
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) accz[ti] = accr[ti] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (s > 0) {   // h = 0 before the first step: the recurrent term vanishes
      for (int k0 = 0; k0 < H; k0 += 4) {
        const int k = k0 + ak;
        const float fa_z = lds[0][ar][k], fa_r = lds[1][ar][k];
        const float* ub = U + (int64_t)k * H3 + ar;
#pragma unroll
        for (int ti = 0; ti < NT; ++ti) {
          accz[ti] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa_z, ub[tcol[ti]], accz[ti], 0, 0, 0);
          accr[ti] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa_r, ub[H + tcol[ti]], accr[ti], 0, 0, 0);
        }
      }
    }
    float z[NT][4], r[NT][4];
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) {
      const int tile = wave + GRU_WAVES * ti;
      if (tile < ntiles) {
        const int col = tile * 16 + ar;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int row = 4 * ak + v, b = b0 + row;
          z[ti][v] = gru_hsig((az[ti][v] + bz[ti]) + accz[ti][v]);
          r[ti][v] = gru_hsig((arr[ti][v] + br[ti]) + accr[ti][v]);
          lds[2][row][col] = r[ti][v] * (h[ti][v] * mhh[ti][v]);
          if (p.save && b < B) {
            float* sv = p.save + ((int64_t)(d * 4) * B * T + (int64_t)b * T + t) * H + col;
            sv[0] = z[ti][v];
            sv[(int64_t)B * T * H] = r[ti][v];
          }
        }
      }
    }
    __syncthreads();
    // ---- phase 2: the candidate on r h mh_h, then the new state ----
    f32x4 accc[NT];
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) accc[ti] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (s > 0) {
      for (int k0 = 0; k0 < H; k0 += 4) {
        const int k = k0 + ak;
        const float fa = lds[2][ar][k];
        const float* ub = U + (int64_t)k * H3 + 2 * H + ar;
#pragma unroll
        for (int ti = 0; ti < NT; ++ti) accc[ti] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa, ub[tcol[ti]], accc[ti], 0, 0, 0);
      }
    }
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) {
      const int tile = wave + GRU_WAVES * ti;
      if (tile < ntiles) {
        const int col = tile * 16 + ar;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int row = 4 * ak + v, b = b0 + row;
          const float c = tanhf((ah[ti][v] + bh[ti]) + accc[ti][v]);
          const float hn = z[ti][v] * h[ti][v] + (1.f - z[ti][v]) * c;
          h[ti][v] = hn;
          lds[0][row][col] = hn * mz[ti][v];
          lds[1][row][col] = hn * mr[ti][v];
          if (p.save && b < B) {
            float* sv = p.save + ((int64_t)(d * 4 + 2) * B * T + (int64_t)b * T + t) * H + col;
            sv[0] = c;
            sv[(int64_t)B * T * H] = hn;
          }
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int ti = 0; ti < NT; ++ti) {
    const int tile = wave + GRU_WAVES * ti;
    if (tile < ntiles) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int b = b0 + 4 * ak + v;
        if (b < B) p.out[(int64_t)b * 2 * H + d * H + tile * 16 + ar] = h[ti][v];
      }
    }
  }
}

struct GruBwdArgs {
  const float* dout;   // [B, 2H]
  const float* UT;     // [2][3][H][H]: UT[d][g][k][j] = U_d[j][g H + k]
  const float* mh;     // [2][3][B][H] or NULL
  const float* save;   // [2][4][B, T, H]
  float* da;           // [2][3][B T][H] pre-activation gradients, gate-major
  float* lop;          // [2][3][B T][H] the left operands of U (h_prev mh_z | h_prev mh_r | r h_prev mh_h)
  int B, T, H;
};

template <int NT>
__global__ __launch_bounds__(GRU_WAVES * 64) void gru_seq_bwd_kernel(GruBwdArgs p) {
  __shared__ float lds[3][GRU_ROWS][GRU_HP];   // 0: da_h, 1: da_z, 2: da_r
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int d = blockIdx.y, b0 = blockIdx.x * GRU_ROWS;
  const int H = p.H, T = p.T, B = p.B;
  const int ar = lane & 15, ak = lane >> 4;
  const int ntiles = H / 16;
  int tcol[NT];   // first column of the wave's tiles; a wave without tile ti computes tile 0 again and drops the result (no branch in the product loops)
#pragma unroll
  for (int ti = 0; ti < NT; ++ti) tcol[ti] = (wave + GRU_WAVES * ti < ntiles ? wave + GRU_WAVES * ti : 0) * 16;
  const int64_t BTH = (int64_t)B * T * H;
  const float* __restrict__ UTz = p.UT + (int64_t)(d * 3) * H * H;
  const float* __restrict__ UTr = UTz + (int64_t)H * H;
  const float* __restrict__ UTh = UTr + (int64_t)H * H;
  const float* __restrict__ sv = p.save + (int64_t)(d * 4) * BTH;
  float* __restrict__ da = p.da + (int64_t)(d * 3) * BTH;
  float* __restrict__ lop = p.lop + (int64_t)(d * 3) * BTH;
  float dh[NT][4], mz[NT][4], mr[NT][4], mhh[NT][4];
#pragma unroll
  for (int ti = 0; ti < NT; ++ti) {
    const int tile = wave + GRU_WAVES * ti;
    const int col = tile * 16 + ar;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int b = b0 + 4 * ak + v;
      const bool ok = tile < ntiles && b < B;
      dh[ti][v] = ok ? p.dout[(int64_t)b * 2 * H + d * H + col] : 0.f;
      mz[ti][v] = mr[ti][v] = mhh[ti][v] = 1.f;
      if (p.mh && ok) {
        const float* m = p.mh + ((int64_t)(d * 3) * B + b) * H + col;
        mz[ti][v] = m[0];
        mr[ti][v] = m[(int64_t)B * H];
        mhh[ti][v] = m[(int64_t)2 * B * H];
      }
    }
  }
  for (int s = T - 1; s >= 0; --s) {
    const int t = d ? T - 1 - s : s;
    const int tp = d ? t + 1 : t - 1;   // the step that produced h_prev (s > 0)
    float r[NT][4], hp[NT][4], dhp[NT][4], dazv[NT][4];
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) {
      const int tile = wave + GRU_WAVES * ti;
      if (tile < ntiles) {
        const int col = tile * 16 + ar;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int row = 4 * ak + v, b = b0 + row;
          float z = 0.f, c = 0.f, daz = 0.f, dah = 0.f;
          r[ti][v] = 0.f;
          hp[ti][v] = 0.f;
          dhp[ti][v] = 0.f;
          dazv[ti][v] = 0.f;
          if (b < B) {
            const int64_t e = ((int64_t)b * T + t) * H + col;
            z = sv[e];
            r[ti][v] = sv[BTH + e];
            c = sv[2 * BTH + e];
            if (s > 0) hp[ti][v] = sv[3 * BTH + ((int64_t)b * T + tp) * H + col];
            const float g = dh[ti][v];
            dah = (g * (1.f - z)) * (1.f - c * c);
            daz = (g * (hp[ti][v] - c)) * gru_hsig_grad(z);
            dhp[ti][v] = g * z;
            dazv[ti][v] = daz;
            da[e] = daz;
            da[2 * BTH + e] = dah;
            lop[e] = hp[ti][v] * mz[ti][v];
            lop[BTH + e] = hp[ti][v] * mr[ti][v];
            lop[2 * BTH + e] = r[ti][v] * (hp[ti][v] * mhh[ti][v]);
          }
          lds[0][row][col] = dah;   // last read in the previous step's phase A, two barriers ago
        }
      }
    }
    __syncthreads();   // also: every wave has left the previous step's phase B, so lds[1] and lds[2] may be rewritten below
    // ---- phase A: gradient wrt r h_prev mh_h = da_h U_h^T ----
    f32x4 acc[NT];
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) acc[ti] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (s > 0) {   // h_prev = 0 at the first step: nothing flows further back
      for (int k0 = 0; k0 < H; k0 += 4) {
        const int k = k0 + ak;
        const float fa = lds[0][ar][k];
        const float* ub = UTh + (int64_t)k * H + ar;
#pragma unroll
        for (int ti = 0; ti < NT; ++ti) acc[ti] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa, ub[tcol[ti]], acc[ti], 0, 0, 0);
      }
    }
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) {
      const int tile = wave + GRU_WAVES * ti;
      if (tile < ntiles) {
        const int col = tile * 16 + ar;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int row = 4 * ak + v, b = b0 + row;
          const float drh = acc[ti][v];
          const float dar = (drh * (hp[ti][v] * mhh[ti][v])) * gru_hsig_grad(r[ti][v]);
          dhp[ti][v] += drh * (r[ti][v] * mhh[ti][v]);
          lds[1][row][col] = dazv[ti][v];
          lds[2][row][col] = (b < B) ? dar : 0.f;
          if (b < B) da[BTH + ((int64_t)b * T + t) * H + col] = dar;
        }
      }
    }
    __syncthreads();
    // ---- phase B: gradient wrt h_prev mh_z and h_prev mh_r ----
    if (s > 0) {
      f32x4 accz[NT], accr[NT];
#pragma unroll
      for (int ti = 0; ti < NT; ++ti) accz[ti] = accr[ti] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int k0 = 0; k0 < H; k0 += 4) {
        const int k = k0 + ak;
        const float fz = lds[1][ar][k], fr = lds[2][ar][k];
        const float* uz = UTz + (int64_t)k * H + ar;
        const float* ur = UTr + (int64_t)k * H + ar;
#pragma unroll
        for (int ti = 0; ti < NT; ++ti) {
          accz[ti] = __builtin_amdgcn_mfma_f32_16x16x4f32(fz, uz[tcol[ti]], accz[ti], 0, 0, 0);
          accr[ti] = __builtin_amdgcn_mfma_f32_16x16x4f32(fr, ur[tcol[ti]], accr[ti], 0, 0, 0);
        }
      }
#pragma unroll
      for (int ti = 0; ti < NT; ++ti)
#pragma unroll
        for (int v = 0; v < 4; ++v) dh[ti][v] = (dhp[ti][v] + accz[ti][v] * mz[ti][v]) + accr[ti][v] * mr[ti][v];
    }
  }
}

struct GruMaskArgs {
  float* mx; float* mh;
  int B, I, H;
  uint32_t key[12];     // [d][mx_z, mx_r, mx_h, mh_z, mh_r, mh_h]
  uint32_t thresh; float inv_keep; int64_t row_offset;
};

// mask blockIdx.y = d * 6 + q of a direction: q < 3 an input mask [B, I], else a recurrent mask [B, H]; values 0 or 1 / keep
__global__ __launch_bounds__(256) void gru_mask_kernel(GruMaskArgs a) {
  const int q = blockIdx.y % 6, d = blockIdx.y / 6;
  const int n = q < 3 ? a.I : a.H;
  float* out = q < 3 ? a.mx + (int64_t)(d * 3 + q) * a.B * a.I : a.mh + (int64_t)(d * 3 + q - 3) * a.B * a.H;
  const int64_t total = (int64_t)a.B * n;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const uint32_t idx = (uint32_t)(a.row_offset * n + e);   // kws_dropout_fwd's counter
    out[e] = kws_keep(idx, a.key[blockIdx.y], a.thresh) ? a.inv_keep : 0.f;
  }
}

// xm[q][b, t, :] = x[b, t, :] * mx[q][b, :] for the six (direction, gate) masks
__global__ __launch_bounds__(256) void gru_mask_input_kernel(const float* __restrict__ x, const float* __restrict__ mx, float* __restrict__ xm,
                                                             int B, int T, int I) {
  const int64_t total = (int64_t)B * T * I;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int i = (int)(e % I);
  const int64_t b = e / ((int64_t)T * I);
  xm[(int64_t)blockIdx.y * total + e] = x[e] * mx[((int64_t)blockIdx.y * B + b) * I + i];
}

// gate blocks of a [K, 3H] matrix: mode 0 out[g][k][j] = in[k][g H + j]; mode 1 out[g][j][k] = in[k][g H + j] (transposed blocks);
// mode 2 the inverse of mode 0: out[k][g H + j] = in[g][k][j]
__global__ __launch_bounds__(256) void gru_gate_blocks_kernel(const float* __restrict__ in, float* __restrict__ out, int K, int H, int mode) {
  const int64_t total = (int64_t)K * 3 * H;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int k = (int)(e / (3 * H)), gj = (int)(e % (3 * H)), g = gj / H, j = gj % H;
  if (mode == 0) out[((int64_t)g * K + k) * H + j] = in[e];
  else if (mode == 1) out[((int64_t)g * H + j) * K + k] = in[e];
  else out[e] = in[((int64_t)g * K + k) * H + j];
}

// column sums of the three [M, H] gate blocks, fixed order: slice blockIdx.y adds its rows ascending, then the slices are folded
__global__ __launch_bounds__(256) void gru_colsum_part_kernel(const float* __restrict__ da, int64_t M, int H, int64_t rows_per, float* __restrict__ part) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= 3 * H) return;
  const int g = c / H, j = c % H;
  const int64_t m0 = blockIdx.y * rows_per, m1 = m0 + rows_per < M ? m0 + rows_per : M;
  float s = 0.f;
  for (int64_t m = m0; m < m1; ++m) s += da[((int64_t)g * M + m) * H + j];
  part[(int64_t)blockIdx.y * 3 * H + c] = s;
}
__global__ __launch_bounds__(256) void gru_colsum_fold_kernel(const float* __restrict__ part, int slices, int n, float* __restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  float s = 0.f;
  for (int q = 0; q < slices; ++q) s += part[(int64_t)q * n + c];
  out[c] = s;
}

// dx[b, t, i] = sum over the six (direction, gate) products p_q[b, t, i] * mx_q[b, i], q ascending (mx NULL: plain sum)
__global__ __launch_bounds__(256) void gru_dx_kernel(const float* __restrict__ prod, const float* __restrict__ mx, float* __restrict__ dx, int B, int T,
                                                     int I) {
  const int64_t total = (int64_t)B * T * I;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int i = (int)(e % I);
  const int64_t b = e / ((int64_t)T * I);
  float s = 0.f;
  for (int q = 0; q < 6; ++q) s += prod[(int64_t)q * total + e] * (mx ? mx[((int64_t)q * B + b) * I + i] : 1.f);
  dx[e] = s;
}

int gru_check(const char* who, int B, int T, int H) {
  KWS_REQUIRE(B >= 1, "%s: B=%d", who, B);
  KWS_REQUIRE(T >= 1 && T <= GRU_MAXT, "%s: T=%d (1 .. %d)", who, T, GRU_MAXT);
  KWS_REQUIRE(H >= 16 && H <= GRU_MAXH && H % 16 == 0, "%s: H=%d (a multiple of 16, 16 .. %d)", who, H, GRU_MAXH);
  return KWS_OK;
}
int gru_check_in(const char* who, int I) {
  KWS_REQUIRE(I >= 4 && I % 4 == 0, "%s: I=%d (a multiple of 4)", who, I);
  return KWS_OK;
}

int gate_blocks(const float* in, float* out, int K, int H, int mode, hipStream_t st) {
  hipLaunchKernelGGL(gru_gate_blocks_kernel, dim3((unsigned)ceil_div64((int64_t)K * 3 * H, 256)), dim3(256), 0, st, in, out, K, H, mode);
  KWS_LAUNCH_CHECK("gru_gate_blocks_kernel");
  return KWS_OK;
}

struct GruWs {   // float offsets into the caller's workspace
  int64_t a = 0, xm = 0, wg = 0, ut = 0, da = 0, lop = 0, prod = 0, tn = 0, gw = 0, part = 0, total = 0;
};
GruWs gru_ws(int B, int T, int I, int H, bool bwd) {
  GruWs w;
  const int64_t M = (int64_t)B * T;
  int64_t cur = 0;
  auto take = [&](int64_t n) { const int64_t o = cur; cur += (n + 63) / 64 * 64; return o; };
  w.a = take(6 * M * H);
  w.xm = take(6 * M * I);
  w.wg = take((int64_t)6 * I * H);          // forward: the gate blocks of W; backward: their transposes
  if (bwd) {
    w.ut = take((int64_t)6 * H * H);
    w.da = take(6 * M * H);
    w.lop = take(6 * M * H);
    w.prod = take(6 * M * I);
    w.tn = take(std::max(kws_gemm_tn_workspace_floats(M, I, H), kws_gemm_tn_workspace_floats(M, H, H)));
    w.gw = take((int64_t)3 * std::max(I, H) * H);
    w.part = take((int64_t)GRU_COL_SLICES * 3 * H);
  }
  w.total = cur;
  return w;
}

}  // namespace

extern "C" {

int64_t kws_gru_save_floats(int B, int T, int H) {
  if (B < 1 || T < 1 || T > GRU_MAXT || H < 16 || H > GRU_MAXH || H % 16) return 0;
  return (int64_t)8 * B * T * H;
}

int64_t kws_gru_workspace_floats(int B, int T, int I, int H, int backward) {
  if (B < 1 || T < 1 || T > GRU_MAXT || H < 16 || H > GRU_MAXH || H % 16 || I < 4 || I % 4) return 0;
  return gru_ws(B, T, I, H, backward != 0).total;
}

int kws_gru_masks(float* mx, float* mh, int B, int I, int H, float keep_prob, uint64_t seed, uint32_t step, int64_t row_offset,
                  void* stream) {
  KWS_REQUIRE(mx && mh && B >= 1 && I >= 1 && H >= 1 && keep_prob > 0.f && keep_prob <= 1.f && row_offset >= 0,
              "gru_masks: bad arguments (B=%d I=%d H=%d keep_prob=%g)", B, I, H, keep_prob);
  GruMaskArgs a;
  a.mx = mx; a.mh = mh; a.B = B; a.I = I; a.H = H;
  for (int d = 0; d < 2; ++d)
    for (int q = 0; q < 6; ++q) a.key[d * 6 + q] = kws_dropout_key(seed, step, (uint32_t)(16 + 6 * d + q));
  a.thresh = kws_dropout_threshold(keep_prob);
  a.inv_keep = 1.0f / keep_prob;
  a.row_offset = row_offset;
  const int64_t total = (int64_t)B * std::max(I, H);
  const unsigned gx = (unsigned)std::min<int64_t>(ceil_div64(total, 256), 1024);
  hipLaunchKernelGGL(gru_mask_kernel, dim3(gx, 12), dim3(256), 0, (hipStream_t)stream, a);
  KWS_LAUNCH_CHECK("gru_mask_kernel");
  return KWS_OK;
}

int kws_gru_seq_fwd_f32(const float* a, int64_t dir_stride, int64_t gate_stride, int row_stride, const float* U0, const float* U1,
                        const float* bias0, const float* bias1, const float* mh, float* out, float* save, int B, int T, int H,
                        void* stream) {
  KWS_TRY(gru_check("gru_seq_fwd", B, T, H));
  KWS_REQUIRE(a && U0 && U1 && bias0 && bias1 && out, "gru_seq_fwd: NULL pointer");
  KWS_REQUIRE(dir_stride > 0 && gate_stride >= H && row_stride >= H, "gru_seq_fwd: strides %lld %lld %d", (long long)dir_stride,
              (long long)gate_stride, row_stride);
  GruFwdArgs p;
  p.a = a; p.dir_stride = dir_stride; p.gate_stride = gate_stride; p.row_stride = row_stride;
  p.U[0] = U0; p.U[1] = U1; p.bias[0] = bias0; p.bias[1] = bias1; p.mh = mh; p.out = out; p.save = save;
  p.B = B; p.T = T; p.H = H;
  const dim3 grid((unsigned)ceil_div(B, GRU_ROWS), 2), block(GRU_WAVES * 64);
  hipStream_t st = (hipStream_t)stream;
  const double rows = 2.0 * B * T;
  KwsProfScope prof("gru_seq_fwd", 2.0 * rows * H * 3 * H, 4.0 * rows * H * (save ? 7.0 : 3.0), st);
  const int nt = ceil_div(H / 16, GRU_WAVES);
  if (nt == 1) hipLaunchKernelGGL(gru_seq_fwd_kernel<1>, grid, block, 0, st, p);
  else if (nt == 2) hipLaunchKernelGGL(gru_seq_fwd_kernel<2>, grid, block, 0, st, p);
  else if (nt == 3) hipLaunchKernelGGL(gru_seq_fwd_kernel<3>, grid, block, 0, st, p);
  else hipLaunchKernelGGL(gru_seq_fwd_kernel<4>, grid, block, 0, st, p);
  KWS_LAUNCH_CHECK("gru_seq_fwd_kernel");
  return KWS_OK;
}

int kws_gru_seq_bwd_f32(const float* dout, const float* UT, const float* mh, const float* save, float* da, float* lop, int B, int T, int H,
                        void* stream) {
  KWS_TRY(gru_check("gru_seq_bwd", B, T, H));
  KWS_REQUIRE(dout && UT && save && da && lop, "gru_seq_bwd: NULL pointer");
  GruBwdArgs p;
  p.dout = dout; p.UT = UT; p.mh = mh; p.save = save; p.da = da; p.lop = lop; p.B = B; p.T = T; p.H = H;
  const dim3 grid((unsigned)ceil_div(B, GRU_ROWS), 2), block(GRU_WAVES * 64);
  hipStream_t st = (hipStream_t)stream;
  const double rows = 2.0 * B * T;
  KwsProfScope prof("gru_seq_bwd", 2.0 * rows * H * 3 * H, 4.0 * rows * H * 10.0, st);
  const int nt = ceil_div(H / 16, GRU_WAVES);
  if (nt == 1) hipLaunchKernelGGL(gru_seq_bwd_kernel<1>, grid, block, 0, st, p);
  else if (nt == 2) hipLaunchKernelGGL(gru_seq_bwd_kernel<2>, grid, block, 0, st, p);
  else if (nt == 3) hipLaunchKernelGGL(gru_seq_bwd_kernel<3>, grid, block, 0, st, p);
  else hipLaunchKernelGGL(gru_seq_bwd_kernel<4>, grid, block, 0, st, p);
  KWS_LAUNCH_CHECK("gru_seq_bwd_kernel");
  return KWS_OK;
}

int kws_gru_fwd_f32(const float* x, const float* W0, const float* U0, const float* bias0, const float* W1, const float* U1,
                    const float* bias1, const float* mx, const float* mh, float* out, float* save, float* workspace, int B, int T, int I,
                    int H, void* stream) {
  KWS_TRY(gru_check("gru_fwd", B, T, H));
  KWS_TRY(gru_check_in("gru_fwd", I));
  KWS_REQUIRE(x && W0 && U0 && bias0 && W1 && U1 && bias1 && out && workspace, "gru_fwd: NULL pointer");
  hipStream_t st = (hipStream_t)stream;
  const GruWs w = gru_ws(B, T, I, H, false);
  const int64_t M = (int64_t)B * T;
  const float* W[2] = {W0, W1};
  float* a = workspace + w.a;
  if (!mx) {   // one unmasked [B T, I] x [I, 3H] product per direction
    for (int d = 0; d < 2; ++d) KWS_TRY(kws_gemm_nn_f32(x, W[d], a + d * 3 * M * H, M, I, 3 * H, nullptr, stream));
    return kws_gru_seq_fwd_f32(a, 3 * M * H, H, 3 * H, U0, U1, bias0, bias1, mh, out, save, B, T, H, stream);
  }
  // the three masked views of x are materialised per direction and meet the gate blocks of W in one GEMM each
  float* xm = workspace + w.xm;
  float* wg = workspace + w.wg;
  hipLaunchKernelGGL(gru_mask_input_kernel, dim3((unsigned)ceil_div64(M * I, 256), 6), dim3(256), 0, st, x, mx, xm, B, T, I);
  KWS_LAUNCH_CHECK("gru_mask_input_kernel");
  for (int d = 0; d < 2; ++d) {
    KWS_TRY(gate_blocks(W[d], wg + (int64_t)d * 3 * I * H, I, H, 0, st));
    for (int g = 0; g < 3; ++g)
      KWS_TRY(kws_gemm_nn_f32(xm + (int64_t)(d * 3 + g) * M * I, wg + ((int64_t)d * 3 + g) * I * H, a + (int64_t)(d * 3 + g) * M * H, M, I, H,
                              nullptr, stream));
  }
  return kws_gru_seq_fwd_f32(a, 3 * M * H, M * H, H, U0, U1, bias0, bias1, mh, out, save, B, T, H, stream);
}

int kws_gru_bwd_f32(const float* dout, const float* x, const float* W0, const float* U0, const float* W1, const float* U1, const float* mx,
                    const float* mh, const float* save, float* dx, float* dW0, float* dU0, float* dbias0, float* dW1, float* dU1,
                    float* dbias1, float* workspace, int B, int T, int I, int H, void* stream) {
  KWS_TRY(gru_check("gru_bwd", B, T, H));
  KWS_TRY(gru_check_in("gru_bwd", I));
  KWS_REQUIRE(dout && x && W0 && U0 && W1 && U1 && save && dW0 && dU0 && dbias0 && dW1 && dU1 && dbias1 && workspace,
              "gru_bwd: NULL pointer");
  hipStream_t st = (hipStream_t)stream;
  const GruWs w = gru_ws(B, T, I, H, true);
  const int64_t M = (int64_t)B * T;
  const float* W[2] = {W0, W1};
  const float* U[2] = {U0, U1};
  float* dW[2] = {dW0, dW1};
  float* dU[2] = {dU0, dU1};
  float* db[2] = {dbias0, dbias1};
  float* ut = workspace + w.ut;
  float* da = workspace + w.da;
  float* lop = workspace + w.lop;
  float* wt = workspace + w.wg;
  float* xm = workspace + w.xm;
  float* gw = workspace + w.gw;
  for (int d = 0; d < 2; ++d) KWS_TRY(gate_blocks(U[d], ut + (int64_t)d * 3 * H * H, H, H, 1, st));
  KWS_TRY(kws_gru_seq_bwd_f32(dout, ut, mh, save, da, lop, B, T, H, stream));
  if (mx) {
    hipLaunchKernelGGL(gru_mask_input_kernel, dim3((unsigned)ceil_div64(M * I, 256), 6), dim3(256), 0, st, x, mx, xm, B, T, I);
    KWS_LAUNCH_CHECK("gru_mask_input_kernel");
  }
  const int64_t rows_per = ceil_div64(M, GRU_COL_SLICES);
  const int slices = (int)ceil_div64(M, rows_per);
  for (int d = 0; d < 2; ++d) {
    const float* dad = da + (int64_t)d * 3 * M * H;
    // dbias: column sums; dU_g = lop_g^T da_g; dW_g = (x mx_g)^T da_g, each [., H] block merged into its [., 3H] tensor
    hipLaunchKernelGGL(gru_colsum_part_kernel, dim3((unsigned)ceil_div(3 * H, 256), (unsigned)slices), dim3(256), 0, st, dad, M, H, rows_per,
                       workspace + w.part);
    KWS_LAUNCH_CHECK("gru_colsum_part_kernel");
    hipLaunchKernelGGL(gru_colsum_fold_kernel, dim3((unsigned)ceil_div(3 * H, 256)), dim3(256), 0, st, workspace + w.part, slices, 3 * H, db[d]);
    KWS_LAUNCH_CHECK("gru_colsum_fold_kernel");
    for (int g = 0; g < 3; ++g)
      KWS_TRY(kws_gemm_tn_f32(lop + (int64_t)(d * 3 + g) * M * H, dad + (int64_t)g * M * H, gw + (int64_t)g * H * H, M, H, H, workspace + w.tn,
                              stream));
    KWS_TRY(gate_blocks(gw, dU[d], H, H, 2, st));
    for (int g = 0; g < 3; ++g)
      KWS_TRY(kws_gemm_tn_f32(mx ? xm + (int64_t)(d * 3 + g) * M * I : x, dad + (int64_t)g * M * H, gw + (int64_t)g * I * H, M, I, H,
                              workspace + w.tn, stream));
    KWS_TRY(gate_blocks(gw, dW[d], I, H, 2, st));
  }
  if (dx) {   // dx = sum_g (da_g W_g^T) * mx_g over both directions
    for (int d = 0; d < 2; ++d) {
      KWS_TRY(gate_blocks(W[d], wt + (int64_t)d * 3 * H * I, I, H, 1, st));
      for (int g = 0; g < 3; ++g)
        KWS_TRY(kws_gemm_nn_f32(da + (int64_t)(d * 3 + g) * M * H, wt + ((int64_t)d * 3 + g) * H * I, workspace + w.prod + (int64_t)(d * 3 + g) * M * I,
                                M, H, I, nullptr, stream));
    }
    hipLaunchKernelGGL(gru_dx_kernel, dim3((unsigned)ceil_div64(M * I, 256)), dim3(256), 0, st, workspace + w.prod, mx, dx, B, T, I);
    KWS_LAUNCH_CHECK("gru_dx_kernel");
  }
  return KWS_OK;
}

}  // extern "C"
