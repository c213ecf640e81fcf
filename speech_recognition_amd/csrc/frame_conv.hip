// Framed first convolution of the raw-waveform nets at NARROW widths (reference model.py:716-772, conv_1d_time_sliced_model:
// overlapping_time_slice_stack(x, 40, 20) + Conv1D(32 * filter_mult, 3, strides=2); conv1.hip is the same layer at exactly 128
// filters).  The frames are never materialised:
//   y[b,t,n]  = sum_{j<taps} sum_{c<ksize} W[j,c,n] * x[b, hop*(stride*t + j) + c - pad_l]        (0 outside [0, L))
//   dW[j,c,n] = sum_{b,t} x[b, hop*(stride*t + j) + c - pad_l] * G[b,t,n]
// The `taps` overlapping taps of a row cover span = hop*(taps-1) + ksize DISTINCT samples, so the product is a Toeplitz GEMM
// over the folded kernel Weff[s] = sum_j W[j][s - hop j] (K = span, padded with zero weights to KP = a multiple of 8), and the
// weight gradient is dWeff = A^T G with every tap row reading the gradient of the sample it multiplies (dW[j][c] =
// dWeff[hop j + c]: overlapping taps each get their own copy, nothing is regrouped).
//
// The layer is HBM-bound (N = 32: 160 B of x and 128 B of y per row at 2 MFLOP per clip), so the kernels are built around the
// memory side:
//   * a workgroup owns 64 consecutive rows of ONE clip.  Consecutive rows overlap (row pitch hop*stride = 40 samples, span
//     80), so the tile's samples are one contiguous SEGMENT of 63 * 40 + 80 samples: it is read once, as consecutive 8-byte
//     pairs over the whole workgroup (hop, pad_l and x_batch_stride are even: every pair is aligned), zero filled outside
//     [0, L), and the MFMA operand of row r is read from the segment at r * pitch.  (Rows that do not overlap - pitch > KP -
//     are staged row by row at pitch KP instead.)
//   * both kernels are persistent and software-pipelined: the next tile's global loads are issued into registers before the
//     current tile's MFMA loop and written to LDS behind it (one LDS buffer, two barriers per tile);
//   * forward: the workgroup folds the kernel once into LDS; a wave owns 32 rows x 32 columns (v_mfma_f32_32x32x2_f32), so a
//     store instruction writes two whole 128-byte row segments; ONE BatchNorm statistics row per workgroup;
//   * weight gradient: wave w owns rows [32 w, 32 w + 32) of dWeff; the tile's G rows go through LDS as 16-byte loads; one
//     slab per workgroup into the caller's workspace, then the fixed-order two-stage slab sum of conv1.hip (groups of 32
//     slabs in place, the group sums straight into the taps of dW).  No atomics.
#include "internal.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int FC_TM = 64;          // rows per tile
constexpr int FC_MAX_SPAN = 128;
constexpr int FC_FWD_WGS = 1024;   // persistent forward workgroups (= statistics rows) at most
constexpr int FC_WG_WGS = 1024;    // persistent weight-gradient workgroups (= slabs) at most: four per CU
constexpr int FC_PER_GROUP = 32;   // slabs per group of the two-stage slab sum

struct FcArgs {
  const float* x;
  const float* W;      // forward: unfolded kernel [taps][ksize][N]
  float* y;            // forward: [B * Lout, N]
  float* stats;        // forward: [grid][2][N] or NULL
  const float* G;      // wgrad: [B * Lout, N]
  float* ws;           // wgrad: [grid][span][N]
  int L, Lout, ksize, hop, pad_l, taps, N;
  int span, KP;        // distinct samples of a row; K extent of the MFMA loop (span rounded up to 8)
  int pitch;           // LDS distance of consecutive rows: stride_t (segment) or KP (row by row)
  int stride_t;        // samples between consecutive rows = hop * stride
  int segment;         // 1: the tile's samples are staged as one contiguous segment
  int tpc;             // tiles per clip
  int tiles;           // B * tpc
  int64_t x_batch_stride;
};

// Samples outside [0, L) read this buffer instead of the clip (an address select, not a branch: a per-load `inside ? load : 0`
// compiles to a branch and a wait per load; conv1.hip).  Not const: a constant-address-space operand makes the selected loads flat.
__device__ __attribute__((aligned(16))) float g_fc_zero[4] = {0.f, 0.f, 0.f, 0.f};

__device__ __forceinline__ float2 fc_load2(const float* xb, int pos, int L) {
  const bool inside = pos >= 0 && pos + 1 < L;
  float2 v = *reinterpret_cast<const float2*>(inside ? xb + pos : g_fc_zero);
  if (!inside && pos >= 0 && pos < L) v.x = xb[pos];      // an odd L: the pair at L - 1 is half inside (pos is even, so never at -1)
  return v;
}

// The samples of the rows t0 .. t0 + nrows - 1 of one clip: first into registers (fc_prefetch: the loads of the NEXT tile are in
// flight while the current one is multiplied), then into sA, element (r, k) at r * pitch + k (fc_commit).  Pair i of the tile
// belongs to thread i % 256: consecutive threads read consecutive 8-byte pairs.
constexpr int FC_MAXP = 16;        // pairs per thread at most: 64 rows x 128 samples / 2 / 256 threads; the kernels are built for
constexpr int FC_FEWP = 8;         // P = 16 and for P = 8 (the model's layer stages 1300 pairs: 6 per thread), to save registers

__device__ __forceinline__ int fc_npairs(const FcArgs& p, int nrows) {
  return p.segment ? ((nrows - 1) * p.stride_t + p.KP) >> 1 : nrows * (p.KP >> 1);
}

template <int P>
__device__ __forceinline__ void fc_prefetch(const FcArgs& p, const float* xb, int t0, int nrows, float2 (&r)[P]) {
  const int s0 = p.stride_t * t0 - p.pad_l;      // even
  const int npairs = fc_npairs(p, nrows), hp = p.KP >> 1;
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const int i = (int)threadIdx.x + j * 256;
    if (j * 256 >= npairs) break;
    if (i < npairs) {
      int pos = s0 + 2 * i;
      if (!p.segment) {
        const int row = i / hp;
        pos = s0 + row * p.stride_t + 2 * (i - row * hp);
      }
      r[j] = fc_load2(xb, pos, p.L);
    }
  }
}

template <int P>
__device__ __forceinline__ void fc_commit(const FcArgs& p, int nrows, const float2 (&r)[P], float* sA) {
  const int npairs = fc_npairs(p, nrows), hp = p.KP >> 1;
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const int i = (int)threadIdx.x + j * 256;
    if (j * 256 >= npairs) break;
    if (i < npairs) {
      int at = 2 * i;
      if (!p.segment) {
        const int row = i / hp;
        at = row * p.KP + 2 * (i - row * hp);
      }
      *reinterpret_cast<float2*>(sA + at) = r[j];
    }
  }
}

struct FcTile {
  int b, t0, nrows;
};
__device__ __forceinline__ FcTile fc_tile(const FcArgs& p, int tile) {
  FcTile t;
  t.b = tile / p.tpc;
  t.t0 = (tile - t.b * p.tpc) * FC_TM;
  t.nrows = p.Lout - t.t0 < FC_TM ? p.Lout - t.t0 : FC_TM;
  return t;
}

// Forward.  256 threads stage; wave (wr, wc) = (wave % 2, wave / 2) with wc < NB computes rows [32 wr, 32 wr + 32) x columns
// [32 wc, 32 wc + 32) of a tile (N = 32: waves 2 and 3 only stage).  K is walked in groups of 8 with lane half lh taking the
// samples 8 q + 4 lh .. + 3 of a group (two 8-byte LDS reads per four MFMAs); the folded kernel is read from LDS in the same order.
template <int NB, int P>
__global__ __launch_bounds__(256) void frame_conv_fwd_kernel(FcArgs p) {
  extern __shared__ __attribute__((aligned(16))) float fc_smem[];
  constexpr int N = 32 * NB;
  float* sW = fc_smem;                 // [KP][N]
  float* sA = fc_smem + p.KP * N;      // the staged rows; the statistics fold reuses it
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 31, lh = lane >> 5;
  const int wr = wave & 1, wc = wave >> 1;
  const bool computes = wc < NB;
  float2 ra[P];
  FcTile cur = fc_tile(p, blockIdx.x);                 // the grid is at most `tiles`
  fc_prefetch(p, p.x + cur.b * p.x_batch_stride, cur.t0, cur.nrows, ra);
  // fold on load, in tap order (fold_taps_kernel's order): Weff[s] = ((0 + W[0][s]) + W[1][s - hop]) + ...
  for (int i = tid; i < p.KP * N; i += 256) {
    const int s = i / N, n = i - s * N;
    float w = 0.f;
    for (int j = 0; j < p.taps; ++j) {
      const int c = s - p.hop * j;
      if (c < 0) break;
      if (c < p.ksize) w += p.W[((int64_t)j * p.ksize + c) * N + n];
    }
    sW[i] = w;
  }
  float st_s = 0.f, st_ss = 0.f;
  for (int tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    fc_commit(p, cur.nrows, ra, sA);
    __syncthreads();
    const int next = tile + gridDim.x;
    FcTile nxt = cur;
    if (next < p.tiles) {
      nxt = fc_tile(p, next);
      fc_prefetch(p, p.x + nxt.b * p.x_batch_stride, nxt.t0, nxt.nrows, ra);
    }
    asm volatile("" ::: "memory");     // the next tile's loads are issued HERE, above the MFMA loop
    if (computes && wr * 32 < cur.nrows) {   // (a clip's ragged last tile: a row block without rows is skipped)
      f32x16 acc;
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[v] = 0.f;
      const float* cA = sA + (wr * 32 + li) * p.pitch + lh * 4;
      const float* cW = sW + (lh * 4) * N + wc * 32 + li;
      const int nq = p.KP >> 3;
      for (int q = 0; q < nq; ++q) {
        const float2 a01 = *reinterpret_cast<const float2*>(cA + q * 8);
        const float2 a23 = *reinterpret_cast<const float2*>(cA + q * 8 + 2);
        const float* w = cW + q * 8 * N;
        const float w0 = w[0], w1 = w[N], w2 = w[2 * N], w3 = w[3 * N];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a01.x, w0, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a01.y, w1, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a23.x, w2, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a23.y, w3, acc, 0, 0, 0);
      }
      // register v of lane (li, lh) = row 32 wr + 4 lh + (v & 3) + 8 (v >> 2), column 32 wc + li.  Rows past nrows were
      // multiplied from whatever LDS held: they are neither stored nor counted.
      const int r0 = wr * 32 + 4 * lh;
      float* yr = p.y + ((int64_t)cur.b * p.Lout + cur.t0 + r0) * N + wc * 32 + li;
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int dr = (v & 3) + 8 * (v >> 2);
        if (r0 + dr < cur.nrows) {
          const float a = acc[v];
          yr[(int64_t)dr * N] = a;
          st_s += a;
          st_ss = fmaf(a, a, st_ss);
        }
      }
    }
    __syncthreads();                   // this tile's operand reads are done: the next commit may overwrite sA
    cur = nxt;
  }
  if (p.stats) {
    float* sRed = sA;                  // [2][2][N]
    const float s = st_s + __shfl_xor(st_s, 32), ss = st_ss + __shfl_xor(st_ss, 32);
    if (computes && lh == 0) {
      sRed[(0 * 2 + wr) * N + wc * 32 + li] = s;
      sRed[(1 * 2 + wr) * N + wc * 32 + li] = ss;
    }
    __syncthreads();
    if (tid < 2 * N) {
      const int q = tid / N, c = tid - q * N;
      p.stats[((int64_t)blockIdx.x * 2 + q) * N + c] = sRed[(q * 2 + 0) * N + c] + sRed[(q * 2 + 1) * N + c];
    }
  }
}

// Weight gradient: dWeff[k][n] += sum over the tile's rows m of A[m][k] G[m][n]; the MFMA's K dimension is the row index, lane
// half lh takes row 2 s + lh of step s.  Wave w owns k in [32 w, 32 w + 32) (waves past the padded span only help staging).  The
// tile's G rows go through registers and LDS like the samples: thread t holds the 16-byte pieces t, t + 256, ...
template <int NB, int P>
__global__ __launch_bounds__(256) void frame_conv_wgrad_kernel(FcArgs p) {
  extern __shared__ __attribute__((aligned(16))) float fc_smem[];
  constexpr int N = 32 * NB;
  constexpr int NG = FC_TM * N / 4 / 256;   // 16-byte pieces of G per thread
  float* sG = fc_smem;                 // [FC_TM][N]
  float* sA = fc_smem + FC_TM * N;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 31, lh = lane >> 5;
  const bool mine = wave * 32 < p.KP;
  f32x16 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[nb][v] = 0.f;
  float2 ra[P];
  float4 rg[NG];
  auto prefetch = [&](const FcTile& t) {
    fc_prefetch(p, p.x + t.b * p.x_batch_stride, t.t0, t.nrows, ra);
    const float4* g4 = reinterpret_cast<const float4*>(p.G + ((int64_t)t.b * p.Lout + t.t0) * N);
#pragma unroll
    for (int j = 0; j < NG; ++j) {     // rows past nrows: zeros (an address select)
      const int i = tid + j * 256;
      rg[j] = i < t.nrows * (N / 4) ? g4[i] : *reinterpret_cast<const float4*>(g_fc_zero);
    }
  };
  FcTile cur = fc_tile(p, blockIdx.x);
  prefetch(cur);
  for (int tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    fc_commit(p, cur.nrows, ra, sA);
#pragma unroll
    for (int j = 0; j < NG; ++j) reinterpret_cast<float4*>(sG)[tid + j * 256] = rg[j];
    __syncthreads();
    const int next = tile + gridDim.x;
    FcTile nxt = cur;
    if (next < p.tiles) {
      nxt = fc_tile(p, next);
      prefetch(nxt);
    }
    asm volatile("" ::: "memory");     // the next tile's loads are issued HERE, above the MFMA loop
    if (mine) {
      const float* cA = sA + lh * p.pitch + wave * 32 + li;
      const float* cG = sG + lh * N + li;
      const int steps = (cur.nrows + 1) >> 1;
      for (int s = 0; s < steps; ++s) {
        const bool ok = 2 * s + lh < cur.nrows;  // the odd last row: A may hold anything there (G is zero)
        const float a = ok ? cA[2 * s * p.pitch] : 0.f;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, cG[2 * s * N + nb * 32], acc[nb], 0, 0, 0);
      }
    }
    __syncthreads();
    cur = nxt;
  }
  if (mine) {
    float* slab = p.ws + (int64_t)blockIdx.x * p.span * N;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int k = wave * 32 + 4 * lh + (v & 3) + 8 * (v >> 2);
      if (k < p.span) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) slab[(int64_t)k * N + nb * 32 + li] = acc[nb][v];
      }
    }
  }
}

// dW[j][c][n] = sum over slab groups of ws[group][hop j + c][n]: the second stage of the slab sum writes the taps directly
__global__ __launch_bounds__(256) void frame_conv_unfold_sum_kernel(const float* __restrict__ ws, float* __restrict__ dW, int groups,
                                                                    int64_t group_stride4, int taps, int ksize, int hop, int N4) {
  const int i = blockIdx.x * 256 + threadIdx.x;   // float4 index into dW[taps][ksize][N]
  if (i >= taps * ksize * N4) return;
  const int n4 = i % N4, jc = i / N4;
  const int j = jc / ksize, c = jc - j * ksize;
  const float4* src = reinterpret_cast<const float4*>(ws) + (int64_t)(hop * j + c) * N4 + n4;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int g = 0; g < groups; ++g) kws_add4(s, src[(int64_t)g * group_stride4]);
  reinterpret_cast<float4*>(dW)[i] = s;
}

bool fc_ok(const kws_frame_conv_t* d) {
  if (!d || d->B <= 0 || d->L <= 0 || d->Lout <= 0 || (d->N != 32 && d->N != 64)) return false;
  if (d->ksize < 1 || d->hop < 1 || d->taps < 1 || (d->stride != 1 && d->stride != 2)) return false;
  if (d->ksize > FC_MAX_SPAN || d->hop > FC_MAX_SPAN || d->taps > FC_MAX_SPAN) return false;
  const int span = d->hop * (d->taps - 1) + d->ksize;
  if (span > FC_MAX_SPAN) return false;
  if (d->hop % 2 || d->pad_l % 2 || d->pad_l < 0 || d->x_batch_stride % 2 || d->x_batch_stride < d->L) return false;
  const int64_t last = (int64_t)d->hop * ((int64_t)d->stride * (d->Lout - 1) + d->taps - 1) + d->ksize - d->pad_l;
  if (last > (int64_t)d->L + span) return false;
  if ((int64_t)d->B * ceil_div(d->Lout, FC_TM) >= (1ll << 31)) return false;
  return true;
}

void fc_fill(FcArgs& a, const kws_frame_conv_t* d) {
  a.L = d->L; a.Lout = d->Lout; a.ksize = d->ksize; a.hop = d->hop; a.pad_l = d->pad_l; a.taps = d->taps; a.N = d->N;
  a.span = d->hop * (d->taps - 1) + d->ksize;
  a.KP = (a.span + 7) / 8 * 8;
  a.stride_t = d->hop * d->stride;
  a.segment = a.stride_t <= a.KP;
  a.pitch = a.segment ? a.stride_t : a.KP;
  a.tpc = ceil_div(d->Lout, FC_TM);
  a.tiles = d->B * a.tpc;
  a.x_batch_stride = d->x_batch_stride;
}

// floats of the staged rows (at most 64 * 128: with the folded kernel [128][64] exactly the 64 KB a launch may ask for)
int fc_a_floats(const FcArgs& a) { return a.segment ? (FC_TM - 1) * a.stride_t + a.KP : FC_TM * a.KP; }

bool fc_aligned(const void* p, int bytes) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(bytes - 1)) == 0; }

}  // namespace

extern "C" {

int kws_frame_conv_stats_rows(const kws_frame_conv_t* d) {
  if (!fc_ok(d)) return 0;
  const int64_t tiles = (int64_t)d->B * ceil_div(d->Lout, FC_TM);
  return (int)(tiles < FC_FWD_WGS ? tiles : FC_FWD_WGS);
}

int kws_frame_conv_fwd_f32(const float* x, const float* W, float* y, float* stats_part, const kws_frame_conv_t* d, void* stream) {
  KWS_REQUIRE(x && W && y && fc_ok(d) && fc_aligned(x, 8), "frame_conv_fwd: bad arguments or a shape outside the domain");
  FcArgs a{};
  fc_fill(a, d);
  a.x = x; a.W = W; a.y = y; a.stats = stats_part;
  const int grid = kws_frame_conv_stats_rows(d);
  int a_floats = fc_a_floats(a);
  if (a_floats < 4 * d->N) a_floats = 4 * d->N;     // the statistics fold
  const size_t lds = sizeof(float) * ((size_t)a.KP * d->N + a_floats);
  const double M = (double)d->B * d->Lout;
  KwsProfScope prof("frame_conv_fwd", 2.0 * M * a.span * d->N, 4.0 * ((double)d->B * d->L + M * d->N + (double)d->taps * d->ksize * d->N),
                    (hipStream_t)stream);
  const bool few = fc_a_floats(a) <= 2 * 256 * FC_FEWP;
  if (d->N == 32 && few) hipLaunchKernelGGL((frame_conv_fwd_kernel<1, FC_FEWP>), dim3(grid), dim3(256), lds, (hipStream_t)stream, a);
  else if (d->N == 32) hipLaunchKernelGGL((frame_conv_fwd_kernel<1, FC_MAXP>), dim3(grid), dim3(256), lds, (hipStream_t)stream, a);
  else if (few) hipLaunchKernelGGL((frame_conv_fwd_kernel<2, FC_FEWP>), dim3(grid), dim3(256), lds, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((frame_conv_fwd_kernel<2, FC_MAXP>), dim3(grid), dim3(256), lds, (hipStream_t)stream, a);
  KWS_LAUNCH_CHECK("frame_conv_fwd_kernel");
  return KWS_OK;
}

int64_t kws_frame_conv_wgrad_workspace_floats(const kws_frame_conv_t* d) {
  if (!fc_ok(d)) return 0;
  const int64_t tiles = (int64_t)d->B * ceil_div(d->Lout, FC_TM);
  const int64_t S = tiles < FC_WG_WGS ? tiles : FC_WG_WGS;
  return S * (d->hop * (d->taps - 1) + d->ksize) * d->N;
}

int kws_frame_conv_wgrad_f32(const float* x, const float* G, float* dW, float* workspace, const kws_frame_conv_t* d, void* stream) {
  KWS_REQUIRE(x && G && dW && workspace && fc_ok(d) && fc_aligned(x, 8) && fc_aligned(G, 16) && fc_aligned(dW, 16) &&
                  fc_aligned(workspace, 16),
              "frame_conv_wgrad: bad arguments or a shape outside the domain");
  FcArgs a{};
  fc_fill(a, d);
  a.x = x; a.G = G; a.ws = workspace;
  const int S = a.tiles < FC_WG_WGS ? a.tiles : FC_WG_WGS;
  // + 32: the last k block reads past the padded span, into rows of dWeff it does not store
  const size_t lds = sizeof(float) * ((size_t)FC_TM * d->N + fc_a_floats(a) + 32);
  const double M = (double)d->B * d->Lout;
  const int64_t n = (int64_t)a.span * d->N;
  {
    KwsProfScope prof("frame_conv_wgrad", 2.0 * M * a.span * d->N, 4.0 * ((double)d->B * d->L + M * d->N + (double)S * n),
                      (hipStream_t)stream);
    const bool few = fc_a_floats(a) <= 2 * 256 * FC_FEWP;
    if (d->N == 32 && few) hipLaunchKernelGGL((frame_conv_wgrad_kernel<1, FC_FEWP>), dim3(S), dim3(256), lds, (hipStream_t)stream, a);
    else if (d->N == 32) hipLaunchKernelGGL((frame_conv_wgrad_kernel<1, FC_MAXP>), dim3(S), dim3(256), lds, (hipStream_t)stream, a);
    else if (few) hipLaunchKernelGGL((frame_conv_wgrad_kernel<2, FC_FEWP>), dim3(S), dim3(256), lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((frame_conv_wgrad_kernel<2, FC_MAXP>), dim3(S), dim3(256), lds, (hipStream_t)stream, a);
    KWS_LAUNCH_CHECK("frame_conv_wgrad_kernel");
  }
  // slab sum in two stages: groups of 32 slabs in place (over each group's first slab), then the group sums into the taps
  const int groups = ceil_div(S, FC_PER_GROUP);
  KWS_TRY(kws_reduce_slab_groups_f32(workspace, n, S, FC_PER_GROUP, (hipStream_t)stream));
  const int n4 = d->taps * d->ksize * (d->N / 4);
  hipLaunchKernelGGL(frame_conv_unfold_sum_kernel, dim3(ceil_div(n4, 256)), dim3(256), 0, (hipStream_t)stream, workspace, dW, groups,
                     (int64_t)FC_PER_GROUP * (n / 4), d->taps, d->ksize, d->hop, d->N / 4);
  KWS_LAUNCH_CHECK("frame_conv_unfold_sum_kernel");
  return KWS_OK;
}

}  // extern "C"
