// The gated-row BatchNorm partial sums of the kernels whose workgroup is R runs x C / 4 threads over the WHOLE channel width
// (pool.hip, pool2d.hip, gap.hip): thread tid = run * (C / 4) + c4 owns the float4 of channels 4 c4 of its run and sums
// (g, g * xhat), xhat = (y - mean) * rstd, over the rows it writes; a workgroup leaves ONE row part[blockIdx.x][2][C], its R runs
// added in ascending order.  kws_gbn_bwd_finish (bncols.hip) folds the rows in a fixed order: no float atomics,
// bit-reproducible.  (resblock.hip's rows are [5][C] over column blocks and dw_bwd_body.h's are grid-strided: not this shape.)
#pragma once
#include <math.h>

#include "common.h"

namespace kws_part {

constexpr int THREADS = 256;   // most threads of a workgroup
constexpr int MAXC = 1024;     // C / 4 threads of one run fit one workgroup

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
// act'(pre) of relu6 (hi = 6) or relu (hi = INFINITY): [0 < pre <= hi]
__device__ __forceinline__ float gate(float pre, float hi = 6.f) { return (pre > 0.f && pre <= hi) ? 1.f : 0.f; }

// One written row: g0 = its four gradients, yu = the raw y they belong to.  A macro, so that the expressions stand in the kernel as
// they always did: as an inlined function the same step moved pool.hip's backward kernels to other code (2 - 6 % slower calls).
#define KWS_PART_ACCUMULATE(sg, sgx, g0, yu, mean, rstd)                 \
  do {                                                                   \
    sg.x += g0.x; sg.y += g0.y; sg.z += g0.z; sg.w += g0.w;              \
    sgx.x = fmaf(g0.x, (yu.x - mean.x) * rstd.x, sgx.x);                 \
    sgx.y = fmaf(g0.y, (yu.y - mean.y) * rstd.y, sgx.y);                 \
    sgx.z = fmaf(g0.z, (yu.z - mean.z) * rstd.z, sgx.z);                 \
    sgx.w = fmaf(g0.w, (yu.w - mean.w) * rstd.w, sgx.w);                 \
  } while (0)

// The end of such a kernel, reached by EVERY thread of the workgroup (a run past the last unit brings zeros).
__device__ __forceinline__ void fold_runs(const float4 sg, const float4 sgx, float* __restrict__ part, int C, int R) {
  __shared__ float red[2][THREADS * 4];
  const int tid = threadIdx.x;
  *reinterpret_cast<float4*>(&red[0][tid * 4]) = sg;
  *reinterpret_cast<float4*>(&red[1][tid * 4]) = sgx;
  __syncthreads();
  for (int o = tid; o < 2 * C; o += blockDim.x) {   // the R runs of this workgroup, ascending
    const int q = o / C, ch = o - q * C;
    float s = 0.f;
    for (int rr = 0; rr < R; ++rr) s += red[q][rr * C + ch];
    part[((int64_t)blockIdx.x * 2 + q) * C + ch] = s;
  }
}

inline bool channels_ok(int C) { return C > 0 && C % 4 == 0 && C <= MAXC; }
struct Geom {
  int R, block;   // runs per workgroup, threads per workgroup
  int64_t grid;   // workgroups = partial rows
};
inline Geom geom(int64_t units, int C) {
  Geom ge;
  ge.R = THREADS / (C / 4);
  ge.block = ge.R * (C / 4);
  ge.grid = ceil_div64(units, ge.R);
  return ge;
}

}  // namespace kws_part
