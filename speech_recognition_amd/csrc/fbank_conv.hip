// Banked strided first convolution of the raw-waveform filterbank front end (reference model.py:1159-1246,
// conv_1d_learned_spec_model: six Conv1D(40, k, strides=160, 'same', no bias) with k = 479 ... 161 on the waveform, concatenated):
//   y[b, t, q*N + n] = sum_{c < ksize[q]} W_q[c, n] * x[b, stride*t + c - pad_l[q]]        (0 outside [0, L))
//   dW_q[c, n]       = sum_{b, t} x[b, stride*t + c - pad_l[q]] * G[b, t, q*N + n]
// Every bank's window lies inside the union window of a row, span = max(ksize - pad_l) + max(pad_l) samples starting max(pad_l)
// in front of sample stride*t (rounded up to an even `pade`, so that the 8-byte staging loads are aligned for any pad parity).
// Bank q's tap c sits at SEGMENT OFFSET off[q] + c of that window, off[q] = pade - pad_l[q]: the banks are one banded product
// over one staged segment, and only the band is multiplied:
//   * a workgroup stages the samples of up to 112 consecutive rows of ONE clip (a whole 100-row clip of the model) as one
//     contiguous LDS segment, read once as consecutive 8-byte pairs, zeros outside [0, L) by address select.  A stride that is a
//     multiple of 32 would put the 16 rows of an MFMA operand on two LDS banks: such a segment is stored with 4 floats of padding
//     per `stride` samples (row pitch 164 for the model: the 16 rows x 4 taps of an operand read hit 64 different banks);
//   * the output columns are cut into tiles of 16 (v_mfma_f32_16x16x4_f32).  A tile's K range is the union of the ranges of the
//     banks it touches, rounded to multiples of 4; a weight outside its own bank's range is a zero by address select.  For the
//     model the tiles multiply 4584 * 16 taps against the 1788 * 40 that exist (+2.5 %; the dense [480, 240] fold: +61 %);
//   * forward: 4 waves; a wave owns every fourth column tile (dealt in a snake, to balance the K ranges) and all 7 row tiles,
//     so a weight is read from global memory (L2) once per workgroup and feeds 7 MFMAs; weights are prefetched 8 K steps ahead;
//   * weight gradient: 16 waves x 18 accumulator tiles [16 offsets x 16 columns] = 288 tiles per workgroup (exactly the model's),
//     more tiles go to further workgroups (grid.y).  The workgroups stride over the clips and write one slab each into the
//     caller's workspace; the fixed-order two-stage slab sum (groups of 16 in place, kws_reduce_slab_groups_f32, then the group
//     sums gathered straight into each bank's dW) finishes it.  No atomics.
#include <algorithm>

#include "internal.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int FB_MAX_BANKS = 8;
constexpr int FB_MAX_N = 64;
constexpr int FB_MAX_SPAN = 512;
constexpr int FB_MAX_STRIDE = 4096;
constexpr int FB_RT = 7;                      // row tiles of 16 per workgroup
constexpr int FB_TM = 16 * FB_RT;             // rows per workgroup at most
constexpr int FB_U = 8;                       // forward: K steps of weights in flight
constexpr int FB_WG_WAVES = 16, FB_TPW = 18;  // weight gradient: waves per workgroup, accumulator tiles per wave
constexpr int FB_TPG = FB_WG_WAVES * FB_TPW;  // accumulator tiles per workgroup
constexpr int FB_WG_SLABS = 256;              // weight-gradient workgroups (= slabs) per tile part at most: one per CU
constexpr int FB_PER_GROUP = 16;              // slabs per group of the two-stage slab sum
constexpr int FB_TAB = 128 + FB_TPG;          // ints of LDS in front of the segment: k0[33] | k1[33] | tile0[33] | .. | wgrad tiles[288]
constexpr int FB_SEG_FLOATS = 36 * 1024;      // LDS floats a segment may take (144 KB of the CU's 160)

struct FbBanks {
  int nbanks, N, F;
  int ksize[FB_MAX_BANKS], off[FB_MAX_BANKS];
  int64_t w_off[FB_MAX_BANKS];
};

struct FbArgs {
  const float* x;
  const float* W;
  float* y;
  const float* G;
  float* ws;
  FbBanks bk;
  int L, Lout, stride;
  int pade;            // samples staged in front of stride * t0 (even)
  int kstage;          // segment offsets staged per row (multiple of 4): the K ranges' and accumulator tiles' reach
  int padw, P;         // padding floats per `stride` samples; LDS row pitch stride + padw
  float inv_stride;
  int R;               // rows per workgroup tile
  int tpc, tiles;      // tiles per clip, B * tpc
  int nct, T;          // column tiles; accumulator tiles of the weight gradient
  int S;               // weight-gradient slabs
  int64_t x_batch_stride;
};

// K range [k0, k1) of column tile ct in segment offsets: the union over the banks whose columns it holds.  The bank loop is
// unrolled over constant indices so that the tables stay in the kernel-argument registers.
__host__ __device__ inline void fb_ct_range(const FbBanks& b, int ct, int* k0, int* k1) {
  const int c0 = ct * 16, c1 = c0 + 16 < b.F ? c0 + 16 : b.F;
  int lo = 1 << 30, hi = 0;
#pragma unroll
  for (int q = 0; q < FB_MAX_BANKS; ++q)
    if (q < b.nbanks && q * b.N < c1 && (q + 1) * b.N > c0) {
      lo = b.off[q] < lo ? b.off[q] : lo;
      hi = b.off[q] + b.ksize[q] > hi ? b.off[q] + b.ksize[q] : hi;
    }
  *k0 = lo & ~3;
  *k1 = (hi + 3) & ~3;
}

__device__ __attribute__((aligned(16))) float g_fb_zero[4] = {0.f, 0.f, 0.f, 0.f};   // frame_conv.hip: g_fc_zero

__device__ __forceinline__ float2 fb_load2(const float* xb, int pos, int L) {
  const bool inside = pos >= 0 && pos + 1 < L;
  float2 v = *reinterpret_cast<const float2*>(inside ? xb + pos : g_fb_zero);
  if (!inside && pos >= 0 && pos < L) v.x = xb[pos];      // an odd L: the pair at L - 1 is half inside (pos is even)
  return v;
}

// LDS address of segment position pos: 4 * padw / 4 floats of padding behind every `stride` samples.  (pos + .5) / stride is
// never within 1 / (2 stride) of an integer, far more than the float product's error (pos < 2^19, stride <= 4096).
__device__ __forceinline__ int fb_at(const FbArgs& p, int pos) {
  return p.padw ? pos + (int)(((float)pos + 0.5f) * p.inv_stride) * p.padw : pos;
}

// k0 | k1 | tile0 of every column tile into LDS (any block size >= 32)
__device__ __forceinline__ void fb_tables(const FbArgs& p, int* sTab) {
  const int tid = threadIdx.x;
  if (tid < p.nct) {
    int k0, k1;
    fb_ct_range(p.bk, tid, &k0, &k1);
    sTab[tid] = k0;
    sTab[33 + tid] = k1;
  }
  __syncthreads();
  if (tid == 0) {
    int t = 0;
    for (int ct = 0; ct < p.nct; ++ct) {
      sTab[66 + ct] = t;
      t += (sTab[33 + ct] - sTab[ct] + 15) >> 4;
    }
    sTab[66 + p.nct] = t;
  }
  __syncthreads();
}

// the samples of the rows t0 .. t0 + nrows - 1 of one clip into sA: segment position s (sample stride * t0 - pade + s) at fb_at(s)
template <int NT>
__device__ __forceinline__ void fb_stage(const FbArgs& p, const float* xb, int t0, int nrows, float* sA) {
  const int s0 = p.stride * t0 - p.pade;                         // even
  const int npairs = ((nrows - 1) * p.stride + p.kstage) >> 1;   // stride and kstage are even: a pair never straddles a padding
#pragma unroll 8
  for (int i = (int)threadIdx.x; i < npairs; i += NT)
    *reinterpret_cast<float2*>(sA + fb_at(p, 2 * i)) = fb_load2(xb, s0 + 2 * i, p.L);
}

// Forward.  Lane (li, lq) = (lane % 16, lane / 16) of an MFMA holds A[row li][k lq] and B[k lq][column li]; result register i is
// row 4 lq + i, column li.
__global__ __launch_bounds__(256) void fbank_conv_fwd_kernel(FbArgs p) {
  extern __shared__ __attribute__((aligned(16))) float fb_smem[];
  int* sTab = reinterpret_cast<int*>(fb_smem);
  float* sA = fb_smem + FB_TAB;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lq = lane >> 4;
  const int b = blockIdx.x / p.tpc, t0 = (blockIdx.x - b * p.tpc) * p.R;
  const int nrows = p.Lout - t0 < p.R ? p.Lout - t0 : p.R;
  fb_stage<256>(p, p.x + b * p.x_batch_stride, t0, nrows, sA);
  fb_tables(p, sTab);                 // (its barriers also publish the segment)
  int rbase[FB_RT];                   // rows past nrows read the last row: finite values, results not stored
#pragma unroll
  for (int rt = 0; rt < FB_RT; ++rt) {
    const int r = rt * 16 + li < nrows ? rt * 16 + li : nrows - 1;
    rbase[rt] = fb_at(p, r * p.stride);
  }
  const int N = p.bk.N;
  // column tiles go to the waves in a snake (0 1 2 3 | 3 2 1 0 | ...): the K ranges shrink from bank to bank, and in plain
  // round-robin order wave 0 would own the longest tile of every round (the model: 1312 against 896 K steps, snake 1220 / 1056)
  for (int round = 0; 4 * round < p.nct; ++round) {
    const int ct = 4 * round + ((round & 1) ? 3 - wave : wave);
    if (ct >= p.nct) continue;
    const int col = ct * 16 + li;
    const bool cvalid = col < p.bk.F;
    int myoff = 0, myks = 0;
    const float* wp = g_fb_zero;
#pragma unroll
    for (int q = 0; q < FB_MAX_BANKS; ++q)
      if (q < p.bk.nbanks && col >= q * N && col < (q + 1) * N) {
        myoff = p.bk.off[q];
        myks = p.bk.ksize[q];
        wp = p.W + p.bk.w_off[q] + (col - q * N);
      }
    const int k0 = __builtin_amdgcn_readfirstlane(sTab[ct]), k1 = __builtin_amdgcn_readfirstlane(sTab[33 + ct]);
    f32x4 acc[FB_RT];
#pragma unroll
    for (int rt = 0; rt < FB_RT; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float wc[FB_U], wn[FB_U];
    auto load_w = [&](float (&w)[FB_U], int kb) {
#pragma unroll
      for (int u = 0; u < FB_U; ++u) {
        const int c = kb + 4 * u + lq - myoff;      // past k1: c >= myks
        const bool ok = cvalid && c >= 0 && c < myks;
        w[u] = *(ok ? wp + (int64_t)c * N : g_fb_zero);
      }
    };
    load_w(wc, k0);
    for (int kk = k0; kk < k1; kk += 4 * FB_U) {
#pragma unroll
      for (int u = 0; u < FB_U; ++u) wn[u] = 0.f;
      if (kk + 4 * FB_U < k1) load_w(wn, kk + 4 * FB_U);
#pragma unroll
      for (int u = 0; u < FB_U; ++u) {
        if (kk + 4 * u < k1) {
          // a row's offset k sits fb_at(r * stride + k) - fb_at(r * stride) = fb_at(k) behind the row's first sample
          const int ka = fb_at(p, kk + 4 * u + lq);
#pragma unroll
          for (int rt = 0; rt < FB_RT; ++rt)
            acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(sA[rbase[rt] + ka], wc[u], acc[rt], 0, 0, 0);
        }
      }
#pragma unroll
      for (int u = 0; u < FB_U; ++u) wc[u] = wn[u];
    }
    if (cvalid) {
      float* yc = p.y + ((int64_t)b * p.Lout + t0) * p.bk.F + col;
#pragma unroll
      for (int rt = 0; rt < FB_RT; ++rt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = rt * 16 + 4 * lq + i;
          if (r < nrows) yc[(int64_t)r * p.bk.F] = acc[rt][i];
        }
    }
  }
}

// Weight gradient.  Accumulator tile j of the T tiles is offsets [ks, ks + 16) x the 16 columns of one column tile; the MFMA's K
// dimension is the row: A[offset li][row lq] = the sample, B[row lq][column li] = G.  Wave w of workgroup part blockIdx.y owns
// the tiles (blockIdx.y * 16 + w) * 18 ... + 17.  Slab layout [S][T][16 offsets][16 columns].
__global__ __launch_bounds__(1024) void fbank_conv_wgrad_kernel(FbArgs p) {
  extern __shared__ __attribute__((aligned(16))) float fb_smem[];
  int* sTab = reinterpret_cast<int*>(fb_smem);
  float* sA = fb_smem + FB_TAB;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lq = lane >> 4;
  fb_tables(p, sTab);
  // the workgroup's tiles (past T: the last one) as column tile << 16 | first offset, looked up once by the first 288 threads
  int* sTile = sTab + 128;
  if (tid < FB_TPG) {
    const int j = (int)blockIdx.y * FB_TPG + tid < p.T ? (int)blockIdx.y * FB_TPG + tid : p.T - 1;
    int ct = 0;
    while (sTab[66 + ct + 1] <= j) ++ct;
    sTile[tid] = ct << 16 | (sTab[ct] + 16 * (j - sTab[66 + ct]));
  }
  __syncthreads();
  const int uwave = __builtin_amdgcn_readfirstlane(wave);
  const int jbase = ((int)blockIdx.y * FB_WG_WAVES + uwave) * FB_TPW;
  int tks[FB_TPW], tct[FB_TPW];       // wave-uniform: first offset and column tile of each owned tile
#pragma unroll
  for (int u = 0; u < FB_TPW; ++u) {
    const int v = __builtin_amdgcn_readfirstlane(sTile[uwave * FB_TPW + u]);
    tct[u] = v >> 16;
    tks[u] = v & 0xffff;
  }
  f32x4 acc[FB_TPW];
#pragma unroll
  for (int u = 0; u < FB_TPW; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    const int b = tile / p.tpc, t0 = (tile - b * p.tpc) * p.R;
    const int nrows = p.Lout - t0 < p.R ? p.Lout - t0 : p.R;
    __syncthreads();                  // the previous tile's operand reads are done
    fb_stage<1024>(p, p.x + b * p.x_batch_stride, t0, nrows, sA);
    __syncthreads();
    const float* Gt = p.G + ((int64_t)b * p.Lout + t0) * p.bk.F;
#pragma unroll 1
    for (int s = 0; 4 * s < nrows; ++s) {
      const int r = 4 * s + lq;
      const bool rok = r < nrows;     // a row past the tile: its sample is the last row's (finite), its G is zero
      const int ra = (rok ? r : nrows - 1) * p.stride + li;   // (the launcher stages without padding)
      const float* Gr = Gt + (int64_t)r * p.bk.F;
      float g = 0.f;
#pragma unroll
      for (int u = 0; u < FB_TPW; ++u) {
        if (u == 0 || tct[u] != tct[u - 1]) {
          const int col = tct[u] * 16 + li;
          g = *(rok && col < p.bk.F ? Gr + col : g_fb_zero);
        }
        const float a = sA[ra + tks[u]];
        acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, g, acc[u], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < FB_TPW; ++u) {
    const int j = jbase + u;
    if (j < p.T) {
      float* dst = p.ws + ((int64_t)blockIdx.x * p.T + j) * 256 + li;
#pragma unroll
      for (int i = 0; i < 4; ++i) dst[(4 * lq + i) * 16] = acc[u][i];
    }
  }
}

// dW_q[c][n] = sum over the slab groups of ws[group][tile of (column q N + n, offset off[q] + c)]: the second stage of the slab
// sum writes every bank's tensor at its own offset.  blockIdx.y = bank.
__global__ __launch_bounds__(256) void fbank_conv_gather_sum_kernel(FbArgs p, float* __restrict__ dW, int groups, int64_t group_stride) {
  __shared__ int sTab[128];
  fb_tables(p, sTab);
  int ks = 0, off = 0;
  int64_t wo = 0;
#pragma unroll
  for (int q = 0; q < FB_MAX_BANKS; ++q)
    if (q == (int)blockIdx.y) {
      ks = p.bk.ksize[q];
      off = p.bk.off[q];
      wo = p.bk.w_off[q];
    }
  const int N = p.bk.N;
  const int i = blockIdx.x * 256 + threadIdx.x;    // c * N + n
  if (i >= ks * N) return;
  const int c = i / N, n = i - c * N;
  const int col = (int)blockIdx.y * N + n, ct = col >> 4, k = off + c - sTab[ct];
  const float* src = p.ws + ((int64_t)(sTab[66 + ct] + (k >> 4)) * 256 + (k & 15) * 16 + (col & 15));
  float s = 0.f;
  for (int g = 0; g < groups; ++g) s += src[(int64_t)g * group_stride];
  dW[wo + i] = s;
}

bool fb_ok(const kws_fbank_conv_t* d) {
  if (!d || d->B <= 0 || d->L <= 0 || d->Lout <= 0) return false;
  if (d->stride < 2 || d->stride % 2 || d->stride > FB_MAX_STRIDE) return false;
  if (d->nbanks < 1 || d->nbanks > FB_MAX_BANKS || d->N < 4 || d->N > FB_MAX_N || d->N % 4) return false;
  if (d->x_batch_stride < d->L || d->x_batch_stride % 2) return false;
  int maxpad = 0, maxtail = 0;
  for (int q = 0; q < d->nbanks; ++q) {
    if (d->ksize[q] < 1 || d->ksize[q] > FB_MAX_SPAN || d->pad_l[q] < 0 || d->pad_l[q] >= d->ksize[q] || d->w_off[q] < 0) return false;
    maxpad = std::max(maxpad, d->pad_l[q]);
    maxtail = std::max(maxtail, d->ksize[q] - d->pad_l[q]);
  }
  if (maxpad + maxtail > FB_MAX_SPAN) return false;
  if ((int64_t)d->stride * (d->Lout - 1) >= (int64_t)d->L + maxpad) return false;   // the last row's union window starts inside the clip
  if ((int64_t)d->B * d->Lout >= (1ll << 31)) return false;
  return true;
}

void fb_fill(FbArgs& a, const kws_fbank_conv_t* d) {
  a.bk.nbanks = d->nbanks; a.bk.N = d->N; a.bk.F = d->nbanks * d->N;
  int maxpad = 0;
  for (int q = 0; q < d->nbanks; ++q) maxpad = std::max(maxpad, d->pad_l[q]);
  a.pade = (maxpad + 1) & ~1;
  for (int q = 0; q < FB_MAX_BANKS; ++q) {
    a.bk.ksize[q] = q < d->nbanks ? d->ksize[q] : 0;
    a.bk.off[q] = q < d->nbanks ? a.pade - d->pad_l[q] : 0;
    a.bk.w_off[q] = q < d->nbanks ? d->w_off[q] : 0;
  }
  a.L = d->L; a.Lout = d->Lout; a.stride = d->stride;
  a.x_batch_stride = d->x_batch_stride;
  a.nct = ceil_div(a.bk.F, 16);
  a.T = 0;
  a.kstage = 0;
  for (int ct = 0; ct < a.nct; ++ct) {
    int k0, k1;
    fb_ct_range(a.bk, ct, &k0, &k1);
    const int nt = (k1 - k0 + 15) / 16;
    a.T += nt;
    a.kstage = std::max(a.kstage, k0 + 16 * nt);
  }
  a.padw = d->stride % 32 == 0 ? 4 : 0;
  a.P = d->stride + a.padw;
  a.inv_stride = 1.f / (float)d->stride;
  // rows per tile: what the segment budget holds (kstage <= 512 + 16 + 2: one row always fits)
  const int64_t fit = 1 + (FB_SEG_FLOATS - a.kstage - (a.kstage / a.stride + 2) * a.padw - 8) / a.P;
  a.R = (int)std::min<int64_t>(std::min(FB_TM, d->Lout), std::max<int64_t>(fit, 1));
  a.tpc = ceil_div(d->Lout, a.R);
  a.tiles = d->B * a.tpc;
  a.S = std::min(a.tiles, FB_WG_SLABS);
}

size_t fb_lds_bytes(const FbArgs& a) {
  const int64_t npos = (int64_t)(a.R - 1) * a.stride + a.kstage;
  return sizeof(float) * (size_t)(FB_TAB + npos + (npos / a.stride + 1) * a.padw + 8);
}

bool fb_aligned(const void* p, int bytes) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(bytes - 1)) == 0; }

double fb_flops(const kws_fbank_conv_t* d) {
  double taps = 0;
  for (int q = 0; q < d->nbanks; ++q) taps += d->ksize[q];
  return 2.0 * d->B * d->Lout * taps * d->N;
}

}  // namespace

extern "C" {

int kws_fbank_conv_fwd_f32(const float* x, const float* W, float* y, const kws_fbank_conv_t* d, void* stream) {
  KWS_REQUIRE(fb_ok(d) && x && W && y && fb_aligned(x, 8), "fbank_conv_fwd: bad arguments or a shape outside the domain");
  FbArgs a{};
  fb_fill(a, d);
  a.x = x; a.W = W; a.y = y;
  const size_t lds = fb_lds_bytes(a);
  KWS_REQUIRE(lds <= 160 * 1024, "fbank_conv_fwd: LDS need %zu B exceeds 160 KiB", lds);
  if (lds > 64 * 1024)
    KWS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&fbank_conv_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds));
  const double M = (double)d->B * d->Lout;
  KwsProfScope prof("fbank_conv_fwd", fb_flops(d), 4.0 * ((double)d->B * d->L + M * a.bk.F + fb_flops(d) / (2.0 * M)),
                    (hipStream_t)stream);
  hipLaunchKernelGGL(fbank_conv_fwd_kernel, dim3((unsigned)a.tiles), dim3(256), lds, (hipStream_t)stream, a);
  KWS_LAUNCH_CHECK("fbank_conv_fwd_kernel");
  return KWS_OK;
}

int64_t kws_fbank_conv_wgrad_workspace_floats(const kws_fbank_conv_t* d) {
  if (!fb_ok(d)) return 0;
  FbArgs a{};
  fb_fill(a, d);
  return (int64_t)a.S * a.T * 256;
}

int kws_fbank_conv_wgrad_f32(const float* x, const float* G, float* dW, float* workspace, const kws_fbank_conv_t* d, void* stream) {
  KWS_REQUIRE(fb_ok(d) && x && G && dW && workspace && fb_aligned(x, 8) && fb_aligned(workspace, 16),
              "fbank_conv_wgrad: bad arguments or a shape outside the domain");
  FbArgs a{};
  fb_fill(a, d);
  a.x = x; a.G = G; a.ws = workspace;
  a.padw = 0;      // an operand read here is 16 consecutive offsets of 4 rows: the padding would buy nothing
  a.P = a.stride;
  const size_t lds = fb_lds_bytes(a);
  KWS_REQUIRE(lds <= 160 * 1024, "fbank_conv_wgrad: LDS need %zu B exceeds 160 KiB", lds);
  if (lds > 64 * 1024)
    KWS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&fbank_conv_wgrad_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds));
  const int64_t n = (int64_t)a.T * 256;
  {
    const double M = (double)d->B * d->Lout;
    KwsProfScope prof("fbank_conv_wgrad", fb_flops(d), 4.0 * ((double)d->B * d->L + M * a.bk.F + (double)a.S * n), (hipStream_t)stream);
    hipLaunchKernelGGL(fbank_conv_wgrad_kernel, dim3((unsigned)a.S, (unsigned)ceil_div(a.T, FB_TPG)), dim3(1024), lds,
                       (hipStream_t)stream, a);
    KWS_LAUNCH_CHECK("fbank_conv_wgrad_kernel");
  }
  // slab sum in two stages: groups of 16 slabs in place (over each group's first slab), then the group sums into the banks
  const int groups = ceil_div(a.S, FB_PER_GROUP);
  KWS_TRY(kws_reduce_slab_groups_f32(workspace, n, a.S, FB_PER_GROUP, (hipStream_t)stream));
  int maxk = 0;
  for (int q = 0; q < d->nbanks; ++q) maxk = std::max(maxk, d->ksize[q]);
  hipLaunchKernelGGL(fbank_conv_gather_sum_kernel, dim3((unsigned)ceil_div(maxk * d->N, 256), (unsigned)d->nbanks), dim3(256), 0,
                     (hipStream_t)stream, a, dW, groups, (int64_t)FB_PER_GROUP * n);
  KWS_LAUNCH_CHECK("fbank_conv_gather_sum_kernel");
  return KWS_OK;
}

}  // extern "C"
