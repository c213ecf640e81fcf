// GlobalAveragePooling1D over relu6(bn(y)) followed by Dropout, forward and backward: the head of the reference's
// conv_1d_time_sliced_model (model.py:716-772), where the pooled features feed a hidden Dense layer (the pooled tails of
// resblock.hip fuse the pool with ONE Dense + softmax instead).  y [B, T, C] is the RAW output of the last pointwise
// convolution, bn its table scale|shift|mean|rstd [4][C].
//   fwd   feat[b,c] = (1/T) * sum_t relu6(scale[c] * y[b,t,c] + shift[c])   (t ascending, one division)
//         fd[b,c]   = feat[b,c] * mask(b,c) / keep
//   bwd   g[b,t,c]  = relu6'(bn(y[b,t,c])) * dfd[b,c] * mask(b,c) / (keep * T),  relu6' = [0 < pre <= 6]
//         part      = kws_gap_drop_bwd_part_rows() rows [2][C] of (sum g, sum g * xhat), xhat = (y - mean) * rstd: the
//                     BatchNorm backward's reductions, one row per workgroup, to be folded in a fixed order.
// mask = kws_dropout_fwd's counter RNG on element (row_offset + b) * C + c; keep_prob = 1: no mask.  Both kernels are
// HBM-bound: one thread owns a float4 of channels of one clip and walks its T <= 16 rows (16-byte loads and stores).
// No atomics: bit-identical from run to run.
#include "common.h"
#include "internal.h"
#include "part_rows.h"

namespace {

constexpr int GP_THREADS = kws_part::THREADS;
constexpr int GP_MAXT = 16;

using kws_part::gate;
using kws_part::ld4;

// 0 or `inv_keep` for the four channels c .. c + 3 of global row `row` (not masked: `inv_keep` everywhere)
__device__ __forceinline__ float4 gp_mask4(int64_t row, int C, int c, uint32_t key, uint32_t thresh, float inv_keep, int masked) {
  if (!masked) return make_float4(inv_keep, inv_keep, inv_keep, inv_keep);
  const uint32_t idx = (uint32_t)(row * C + c);   // 32-bit counter, wraps like kws_dropout_fwd's
  return make_float4(kws_keep(idx, key, thresh) ? inv_keep : 0.f, kws_keep(idx + 1u, key, thresh) ? inv_keep : 0.f,
                     kws_keep(idx + 2u, key, thresh) ? inv_keep : 0.f, kws_keep(idx + 3u, key, thresh) ? inv_keep : 0.f);
}

__global__ __launch_bounds__(GP_THREADS) void gap_drop_fwd_kernel(const float* __restrict__ y, const float* __restrict__ bn,
                                                                  float* __restrict__ feat, float* __restrict__ fd, int64_t n_units,
                                                                  int T, int C, uint32_t key, uint32_t thresh, float inv_keep,
                                                                  int masked, int64_t row_offset) {
  const int64_t i = (int64_t)blockIdx.x * GP_THREADS + threadIdx.x;
  if (i >= n_units) return;
  const int C4 = C >> 2;
  const int64_t b = i / C4;
  const int c = (int)(i - b * C4) * 4;
  const float4 sc = ld4(bn + c), sh = ld4(bn + C + c);
  const float* yb = y + b * T * (int64_t)C + c;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int t = 0; t < T; ++t) {
    const float4 v = ld4(yb + (int64_t)t * C);
    s.x += relu6f(fmaf(v.x, sc.x, sh.x));
    s.y += relu6f(fmaf(v.y, sc.y, sh.y));
    s.z += relu6f(fmaf(v.z, sc.z, sh.z));
    s.w += relu6f(fmaf(v.w, sc.w, sh.w));
  }
  const float ft = (float)T;
  const float4 f = make_float4(__fdiv_rn(s.x, ft), __fdiv_rn(s.y, ft), __fdiv_rn(s.z, ft), __fdiv_rn(s.w, ft));
  const float4 m = gp_mask4(row_offset + b, C, c, key, thresh, inv_keep, masked);
  *reinterpret_cast<float4*>(feat + b * C + c) = f;
  *reinterpret_cast<float4*>(fd + b * C + c) = make_float4(f.x * m.x, f.y * m.y, f.z * m.z, f.w * m.w);
}

// One workgroup = R clips x C / 4 threads; its part row is the sum over its R clips in ascending order.
__global__ __launch_bounds__(GP_THREADS) void gap_drop_bwd_kernel(const float* __restrict__ dfd, const float* __restrict__ y,
                                                                  const float* __restrict__ bn, float* __restrict__ g,
                                                                  float* __restrict__ part, int B, int T, int C, int R, uint32_t key,
                                                                  uint32_t thresh, float inv_keep_t, int masked, int64_t row_offset) {
  const int C4 = C >> 2;
  const int tid = threadIdx.x;
  const int r = tid / C4, c4 = tid - r * C4;
  const int c = c4 * 4;
  const int64_t b = (int64_t)blockIdx.x * R + r;
  float4 sg = make_float4(0.f, 0.f, 0.f, 0.f), sgx = sg;
  if (b < B) {
    const float4 sc = ld4(bn + c), sh = ld4(bn + C + c), mean = ld4(bn + 2 * C + c), rstd = ld4(bn + 3 * C + c);
    const float4 m = gp_mask4(row_offset + b, C, c, key, thresh, inv_keep_t, masked);   // 0 or 1 / (keep T)
    const float4 d0 = ld4(dfd + b * C + c);
    const float4 d = make_float4(d0.x * m.x, d0.y * m.y, d0.z * m.z, d0.w * m.w);   // what every row of the clip receives
    const float* yb = y + b * T * (int64_t)C + c;
    float* gb = g + b * T * (int64_t)C + c;
    for (int t = 0; t < T; ++t) {
      const float4 yu = ld4(yb + (int64_t)t * C);
      const float4 g0 = make_float4(d.x * gate(fmaf(yu.x, sc.x, sh.x)), d.y * gate(fmaf(yu.y, sc.y, sh.y)),
                                    d.z * gate(fmaf(yu.z, sc.z, sh.z)), d.w * gate(fmaf(yu.w, sc.w, sh.w)));
      *reinterpret_cast<float4*>(gb + (int64_t)t * C) = g0;
      KWS_PART_ACCUMULATE(sg, sgx, g0, yu, mean, rstd);
    }
  }
  kws_part::fold_runs(sg, sgx, part, C, R);   // the R clips of this workgroup, ascending
}

bool gp_ok(int B, int T, int C) { return B > 0 && T >= 1 && T <= GP_MAXT && kws_part::channels_ok(C); }

}  // namespace

extern "C" {

int kws_gap_drop_fwd_f32(const float* y, const float* bn, float* feat, float* fd, int B, int T, int C, float keep_prob, uint64_t seed,
                         uint32_t step, uint32_t layer_id, int64_t row_offset, void* stream) {
  KWS_REQUIRE(y && bn && feat && fd && gp_ok(B, T, C) && keep_prob > 0.f && keep_prob <= 1.f && row_offset >= 0,
              "gap_drop_fwd: bad arguments (B=%d T=%d C=%d keep_prob=%g)", B, T, C, keep_prob);
  const int64_t n_units = (int64_t)B * (C / 4);
  KWS_REQUIRE(ceil_div64(n_units, GP_THREADS) < (1ll << 31), "gap_drop_fwd: tensor too large");
  const int masked = keep_prob < 1.f;
  KwsProfScope prof("gap_drop_fwd", 4.0 * B * T * C, 4.0 * ((double)B * T * C + 2.0 * B * C), (hipStream_t)stream);
  hipLaunchKernelGGL(gap_drop_fwd_kernel, dim3((unsigned)ceil_div64(n_units, GP_THREADS)), dim3(GP_THREADS), 0, (hipStream_t)stream, y,
                     bn, feat, fd, n_units, T, C, kws_dropout_key(seed, step, layer_id), kws_dropout_threshold(keep_prob),
                     1.0f / keep_prob, masked, row_offset);
  KWS_LAUNCH_CHECK("gap_drop_fwd_kernel");
  return KWS_OK;
}

int kws_gap_drop_bwd_part_rows(int B, int T, int C) { return gp_ok(B, T, C) ? (int)kws_part::geom(B, C).grid : 0; }

int kws_gap_drop_bwd_f32(const float* dfd, const float* y, const float* bn, float* g, float* part, int B, int T, int C, float keep_prob,
                         uint64_t seed, uint32_t step, uint32_t layer_id, int64_t row_offset, void* stream) {
  KWS_REQUIRE(dfd && y && bn && g && part && gp_ok(B, T, C) && keep_prob > 0.f && keep_prob <= 1.f && row_offset >= 0,
              "gap_drop_bwd: bad arguments (B=%d T=%d C=%d keep_prob=%g)", B, T, C, keep_prob);
  const kws_part::Geom ge = kws_part::geom(B, C);   // one unit = a clip
  const int masked = keep_prob < 1.f;
  KwsProfScope prof("gap_drop_bwd", 8.0 * B * T * C, 4.0 * (2.0 * B * T * C + (double)B * C), (hipStream_t)stream);
  hipLaunchKernelGGL(gap_drop_bwd_kernel, dim3((unsigned)ge.grid), dim3((unsigned)ge.block), 0, (hipStream_t)stream, dfd, y,
                     bn, g, part, B, T, C, ge.R, kws_dropout_key(seed, step, layer_id), kws_dropout_threshold(keep_prob),
                     1.0f / (keep_prob * (float)T), masked, row_offset);
  KWS_LAUNCH_CHECK("gap_drop_bwd_kernel");
  return KWS_OK;
}

}  // extern "C"
