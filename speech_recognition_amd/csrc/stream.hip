// Keyword spotting in long recordings (kws_stream_*): the window gather in front of the net and the posterior smoothing
// behind it.
//
// frames_kernel: out[w win + i] = scale * (float)src[start + w hop + i], an exact 0.0f where that sample lies outside
// [0, n).  One work item is 4 consecutive outputs of one window = one 16-byte store; the grid strides over the
// (window, group) pairs, so any W is one launch (the pair of the first item comes from one 32-bit division, every later
// one from adding the stride's own (windows, groups) pair - no 64-bit division in the loop).  The source offset of a group
// has any alignment, odd ones included, and it differs from window to window: a group loads the ALIGNED 4-element chunk
// (16 bytes of float, 8 of int16) under its first sample and, when it does not start on that chunk, the chunk behind it,
// and shifts its 4 samples out of the pair.  With hop and start multiples of 4 on an aligned recording (the default: hop
// 320) that is one load per store.  Only a group whose chunks are not wholly inside [0, n) - the first and last windows
// of a recording - reads sample by sample, each one guarded: nothing outside src[0, n) is read, not even the rest of an
// aligned chunk.  The value is ONE float multiply (a lone product: nothing to contract), so the result is defined bit
// for bit.  The windows overlap win / hop times; the re-reads come from L2 / Infinity Cache and the kernel is bound by
// its W win 4 bytes of stores.
//
// gather_kernel: the same gather as a copy of bits into rows of any pitch, out[w pitch + i] = src[start + w hop + i], for
// any win and any float alignment on either side (the windows of a shared feature track, stream.py; the comment at the
// kernel has the chunking).
//
// smooth_kernel: smoothed[w, c] = (probs[lo, c] + ... + probs[w, c]) / (float)(w - lo + 1), lo = max(0, w - A + 1), summed
// in ascending row order in float32 and divided once (the correctly rounded division: no fast-math), top[w] = the lowest
// class that attains the row's maximum, top_score[w] = that maximum.  A row belongs to P = the power of two >= NC (64 at
// the most) neighbouring lanes of one wave, lane l of them to the classes l, l + P, ...; the row's maximum is an xor
// butterfly inside the P lanes.  Every output is the direct A-term sum: no running sum is carried from row to row, so a
// row's bits depend on the A rows under it and on nothing else (not on W, not on how the track was chunked through the
// net).  No atomics.
#include <limits.h>

#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int MAX_BLOCKS = 2048;              // 8 workgroups per compute unit; the rest is the grid stride
constexpr int SMOOTH_MAX_A = 4096, SMOOTH_MAX_NC = 256;
// |start| and n: start + w hop + 4 g with w hop < 2^62 then stays inside int64 for every accepted argument
constexpr int64_t MAX_SAMPLES = (int64_t)1 << 61;

struct FramesArgs {
  const void* src;
  float* out;
  int64_t n, start;
  int hop, win, W, gpw;      // gpw = win / 4 groups per window
  unsigned mis;              // (src / sizeof(T)) mod 4: where the recording starts inside its aligned chunk
  unsigned dw, dg;           // the grid's stride as (windows, groups): gridDim * NT = dw * gpw + dg
  float scale;
};

// the 4 samples from s on, all of [sA, sA + 4) and (a != 0) [sA + 4, sA + 8) inside the recording; sA = s - a is aligned
__device__ __forceinline__ float4 load4_fast(const float* src, int64_t sA, unsigned a) {
  const float4 q0 = *reinterpret_cast<const float4*>(src + sA);
  float4 q1 = q0;
  if (a) q1 = *reinterpret_cast<const float4*>(src + sA + 4);
  float4 v;
  v.x = a == 0 ? q0.x : a == 1 ? q0.y : a == 2 ? q0.z : q0.w;
  v.y = a == 0 ? q0.y : a == 1 ? q0.z : a == 2 ? q0.w : q1.x;
  v.z = a == 0 ? q0.z : a == 1 ? q0.w : a == 2 ? q1.x : q1.y;
  v.w = a == 0 ? q0.w : a == 1 ? q1.x : a == 2 ? q1.y : q1.z;
  return v;
}

__device__ __forceinline__ float4 load4_fast(const int16_t* src, int64_t sA, unsigned a) {
  // sample sA + k sits in bits [16 k, 16 k + 16) of the chunk
  const unsigned long long lo = *reinterpret_cast<const unsigned long long*>(src + sA);
  unsigned long long v = lo;
  if (a) {
    const unsigned long long hi = *reinterpret_cast<const unsigned long long*>(src + sA + 4);
    v = (lo >> (16u * a)) | (hi << (64u - 16u * a));
  }
  float4 r;
  r.x = (float)(int16_t)(v & 0xffffu);
  r.y = (float)(int16_t)((v >> 16) & 0xffffu);
  r.z = (float)(int16_t)((v >> 32) & 0xffffu);
  r.w = (float)(int16_t)(v >> 48);
  return r;
}

template <typename T>
__global__ __launch_bounds__(NT) void frames_kernel(FramesArgs a) {
  const T* src = reinterpret_cast<const T*>(a.src);
  const unsigned i0 = blockIdx.x * NT + threadIdx.x;      // < MAX_BLOCKS * NT
  int64_t w = i0 / (unsigned)a.gpw;
  unsigned g = i0 - (unsigned)w * (unsigned)a.gpw;
  while (w < a.W) {
    const int64_t s = a.start + w * a.hop + 4 * (int64_t)g;
    const unsigned al = (unsigned)((int64_t)a.mis + s) & 3u;
    const int64_t sA = s - al;
    float4 v;
    if (sA >= 0 && sA + (al ? 8 : 4) <= a.n) {
      const float4 x = load4_fast(src, sA, al);
      v.x = a.scale * x.x;
      v.y = a.scale * x.y;
      v.z = a.scale * x.z;
      v.w = a.scale * x.w;
    } else {
      v.x = (s >= 0 && s < a.n) ? a.scale * (float)src[s] : 0.f;
      v.y = (s + 1 >= 0 && s + 1 < a.n) ? a.scale * (float)src[s + 1] : 0.f;
      v.z = (s + 2 >= 0 && s + 2 < a.n) ? a.scale * (float)src[s + 2] : 0.f;
      v.w = (s + 3 >= 0 && s + 3 < a.n) ? a.scale * (float)src[s + 3] : 0.f;
    }
    *reinterpret_cast<float4*>(a.out + w * a.win + 4 * (int64_t)g) = v;
    w += a.dw;
    g += a.dg;
    if (g >= (unsigned)a.gpw) {
      g -= (unsigned)a.gpw;
      ++w;
    }
  }
}

template <typename T>
int frames_launch(const T* src, int64_t n, int64_t start, int hop, int win, float scale, float* out, int W, void* stream) {
  KWS_REQUIRE(out && (src || n == 0), "stream_frames: NULL pointer");
  KWS_REQUIRE(win >= 4 && win % 4 == 0 && hop >= 1 && W >= 1, "stream_frames: win=%d (a multiple of 4, >= 4) hop=%d (>= 1) W=%d (>= 1)",
              win, hop, W);
  KWS_REQUIRE(n >= 0 && n <= MAX_SAMPLES && start >= -MAX_SAMPLES && start <= MAX_SAMPLES, "stream_frames: n=%lld start=%lld",
              (long long)n, (long long)start);
  KWS_REQUIRE(((uintptr_t)out & 15) == 0, "stream_frames: out must be 16-byte aligned");
  KWS_REQUIRE(((uintptr_t)src & (sizeof(T) - 1)) == 0, "stream_frames: src must be aligned to its %d-byte elements", (int)sizeof(T));
  hipStream_t st = (hipStream_t)stream;
  FramesArgs a;
  a.src = src; a.out = out; a.n = n; a.start = start; a.hop = hop; a.win = win; a.W = W; a.gpw = win / 4; a.scale = scale;
  a.mis = (unsigned)(((uintptr_t)src / sizeof(T)) & 3);
  const int64_t items = (int64_t)W * a.gpw;
  const int64_t blocks = ceil_div64(items, NT);
  const unsigned grid = (unsigned)(blocks < MAX_BLOCKS ? blocks : MAX_BLOCKS);
  const unsigned stride = grid * NT;
  a.dw = stride / (unsigned)a.gpw;
  a.dg = stride % (unsigned)a.gpw;
  // every sample under the windows once (the overlaps are cache hits) + one 16-byte store per item
  const int64_t span = (int64_t)(W - 1) * hop + win;
  KwsProfScope prof("stream_frames", (double)items * 4.0, (double)(span < n ? span : n) * sizeof(T) + 16.0 * (double)items, st);
  hipLaunchKernelGGL(frames_kernel<T>, dim3(grid), dim3(NT), 0, st, a);
  KWS_LAUNCH_CHECK("frames_kernel");
  return KWS_OK;
}

struct GatherArgs {
  const unsigned* src;       // the floats as their 32-bit patterns: the kernel moves bits
  unsigned* out;
  int64_t n, start, hop, pitch;
  int64_t live;              // rows w >= live start at or past n: start + w hop is formed for w < live only
  int win, W, cpr;           // cpr = (win + 6) / 4: the most aligned 16-byte chunks one row's destination touches
  unsigned smis, dmis;       // (src / 4) mod 4 and (out / 4) mod 4
  unsigned dw, dc;           // the grid's stride as (rows, chunks): gridDim * NT = dw * cpr + dc
};

// load4_fast on bit patterns
__device__ __forceinline__ uint4 load4_bits(const unsigned* src, int64_t sA, unsigned a) {
  const uint4 q0 = *reinterpret_cast<const uint4*>(src + sA);
  uint4 q1 = q0;
  if (a) q1 = *reinterpret_cast<const uint4*>(src + sA + 4);
  uint4 v;
  v.x = a == 0 ? q0.x : a == 1 ? q0.y : a == 2 ? q0.z : q0.w;
  v.y = a == 0 ? q0.y : a == 1 ? q0.z : a == 2 ? q0.w : q1.x;
  v.z = a == 0 ? q0.z : a == 1 ? q0.w : a == 2 ? q1.x : q1.y;
  v.w = a == 0 ? q0.w : a == 1 ? q1.x : a == 2 ? q1.y : q1.z;
  return v;
}

// out[w pitch + i] = src[start + w hop + i].  One work item is one ALIGNED 16-byte chunk of the destination: chunk c of row w
// holds the row's elements i = 4 c - d .. 4 c - d + 3, d = (out / 4 + w pitch) mod 4 the row's own misalignment (it changes
// from row to row when pitch % 4 != 0).  A chunk wholly inside the row is one 16-byte store; the row's first and last chunk,
// when the row's edge cuts them, store their 1 ... 3 elements one by one - the floats between the rows are never written,
// and never read.  The source side is frames_kernel's: the aligned chunk pair and a shift, sample by sample where a chunk
// is not wholly inside [0, n).
__global__ __launch_bounds__(NT) void gather_kernel(GatherArgs a) {
  const unsigned i0 = blockIdx.x * NT + threadIdx.x;      // < MAX_BLOCKS * NT
  int64_t w = i0 / (unsigned)a.cpr;
  unsigned c = i0 - (unsigned)w * (unsigned)a.cpr;
  while (w < a.W) {
    const unsigned d = (a.dmis + ((unsigned)w & 3u) * ((unsigned)a.pitch & 3u)) & 3u;
    const int64_t i = 4 * (int64_t)c - d;                 // >= -3; the last chunks of a well-aligned row lie behind it
    if (i < a.win) {
      unsigned* o = a.out + w * a.pitch + i;
      const bool live = w < a.live;
      const int64_t s = live ? a.start + w * a.hop + i : 0;
      if (i >= 0 && i + 4 <= a.win) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (live) {
          const unsigned al = (unsigned)((int64_t)a.smis + s) & 3u;
          const int64_t sA = s - al;
          if (sA >= 0 && sA + (al ? 8 : 4) <= a.n) {
            v = load4_bits(a.src, sA, al);
          } else {
            if (s >= 0 && s < a.n) v.x = a.src[s];
            if (s + 1 >= 0 && s + 1 < a.n) v.y = a.src[s + 1];
            if (s + 2 >= 0 && s + 2 < a.n) v.z = a.src[s + 2];
            if (s + 3 >= 0 && s + 3 < a.n) v.w = a.src[s + 3];
          }
        }
        *reinterpret_cast<uint4*>(o) = v;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (i + k >= 0 && i + k < a.win) o[k] = (live && s + k >= 0 && s + k < a.n) ? a.src[s + k] : 0u;
      }
    }
    w += a.dw;
    c += a.dc;
    if (c >= (unsigned)a.cpr) {
      c -= (unsigned)a.cpr;
      ++w;
    }
  }
}

// P lanes per row (a power of two, 1 ... 64), NT / P rows per workgroup
__global__ __launch_bounds__(NT) void smooth_kernel(const float* __restrict__ probs, int W, int NC, int A, int P, float* __restrict__ smoothed,
                                                     int* __restrict__ top, float* __restrict__ top_score) {
  const int rows = NT / P;
  const int l = threadIdx.x & (P - 1), r = threadIdx.x / P;
  for (int64_t w0 = (int64_t)blockIdx.x * rows; w0 < W; w0 += (int64_t)gridDim.x * rows) {   // uniform over the workgroup
    const int64_t w = w0 + r;
    const bool live = w < W;
    float best = -INFINITY;
    int arg = INT_MAX;
    if (live) {
      const int64_t lo = w - A + 1 > 0 ? w - A + 1 : 0;
      const float cnt = (float)(w - lo + 1);
      for (int c = l; c < NC; c += P) {
        const float* p = probs + lo * NC + c;
        float acc = p[0];
#pragma unroll 4   // four loads in flight; the adds stay in row order
        for (int64_t k = 1; k <= w - lo; ++k) acc += p[k * NC];
        const float m = acc / cnt;
        if (smoothed) smoothed[w * NC + c] = m;
        if (m > best || arg == INT_MAX) {   // ascending c: the first maximum stays
          best = m;
          arg = c;
        }
      }
    }
    for (int o = P >> 1; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o);
      const int oa = __shfl_xor(arg, o);
      if (oa != INT_MAX && (arg == INT_MAX || ob > best || (ob == best && oa < arg))) {
        best = ob;
        arg = oa;
      }
    }
    if (live && l == 0) {
      top[w] = arg;
      top_score[w] = best;
    }
  }
}

}  // namespace

extern "C" {

int kws_stream_frames_i16(const int16_t* src, int64_t n, int64_t start, int hop, int win, float scale, float* out, int W,
                          void* stream) {
  return frames_launch<int16_t>(src, n, start, hop, win, scale, out, W, stream);
}

int kws_stream_frames_f32(const float* src, int64_t n, int64_t start, int hop, int win, float scale, float* out, int W,
                          void* stream) {
  return frames_launch<float>(src, n, start, hop, win, scale, out, W, stream);
}

int kws_stream_gather_f32(const float* src, int64_t n, int64_t start, int64_t hop, int win, float* out, int64_t out_pitch, int W,
                          void* stream) {
  KWS_REQUIRE(out && (src || n == 0), "stream_gather: NULL pointer");
  KWS_REQUIRE(win >= 1 && hop >= 1 && W >= 1 && out_pitch >= win, "stream_gather: win=%d (>= 1) hop=%lld (>= 1) W=%d (>= 1) out_pitch=%lld (>= win)",
              win, (long long)hop, W, (long long)out_pitch);
  KWS_REQUIRE(n >= 0 && n <= MAX_SAMPLES && start >= -MAX_SAMPLES && start <= MAX_SAMPLES, "stream_gather: n=%lld start=%lld",
              (long long)n, (long long)start);
  // (W - 1) out_pitch + win floats of output: more than 2^61 of them have no address
  KWS_REQUIRE(W == 1 || out_pitch <= (MAX_SAMPLES - win) / (W - 1), "stream_gather: W=%d rows of pitch %lld exceed 2^61 floats", W,
              (long long)out_pitch);
  KWS_REQUIRE(((uintptr_t)out & 3) == 0 && ((uintptr_t)src & 3) == 0, "stream_gather: src and out must be aligned to their 4-byte elements");
  hipStream_t st = (hipStream_t)stream;
  GatherArgs a;
  a.src = reinterpret_cast<const unsigned*>(src); a.out = reinterpret_cast<unsigned*>(out);
  a.n = n; a.start = start; a.hop = hop; a.pitch = out_pitch; a.win = win; a.W = W;
  // rows that start before n: w hop < n - start <= 2^62, whatever hop is
  const int64_t ahead = n - start;
  a.live = ahead <= 0 ? 0 : (ahead - 1) / hop + 1;
  if (a.live > W) a.live = W;
  a.cpr = (int)(((int64_t)win + 6) / 4);
  a.smis = (unsigned)(((uintptr_t)src / 4) & 3);
  a.dmis = (unsigned)(((uintptr_t)out / 4) & 3);
  const int64_t items = (int64_t)W * a.cpr;
  const int64_t blocks = ceil_div64(items, NT);
  const unsigned grid = (unsigned)(blocks < MAX_BLOCKS ? blocks : MAX_BLOCKS);
  const unsigned stride = grid * NT;
  a.dw = stride / (unsigned)a.cpr;
  a.dc = stride % (unsigned)a.cpr;
  // every source float under the live rows once (overlaps are cache hits) + every row segment stored
  const double span = a.live > 0 ? (double)(a.live - 1) * (double)hop + win : 0.0;
  KwsProfScope prof("stream_gather", 0.0, 4.0 * ((span < (double)n ? span : (double)n) + (double)W * win), st);
  hipLaunchKernelGGL(gather_kernel, dim3(grid), dim3(NT), 0, st, a);
  KWS_LAUNCH_CHECK("gather_kernel");
  return KWS_OK;
}

int kws_stream_smooth_f32(const float* probs, int W, int NC, int A, float* smoothed, int* top, float* top_score, void* stream) {
  KWS_REQUIRE(probs && top && top_score, "stream_smooth: NULL pointer");
  KWS_REQUIRE(W >= 1 && NC >= 1 && NC <= SMOOTH_MAX_NC && A >= 1 && A <= SMOOTH_MAX_A, "stream_smooth: W=%d (>= 1) NC=%d (1 ... %d) A=%d (1 ... %d)",
              W, NC, SMOOTH_MAX_NC, A, SMOOTH_MAX_A);
  hipStream_t st = (hipStream_t)stream;
  int P = 1;
  while (P < NC && P < 64) P <<= 1;
  const int64_t blocks = ceil_div64(W, NT / P);
  const unsigned grid = (unsigned)(blocks < MAX_BLOCKS ? blocks : MAX_BLOCKS);
  const double cells = (double)W * NC;
  KwsProfScope prof("stream_smooth", cells * (W < A ? W : A), 4.0 * cells * (smoothed ? 2.0 : 1.0) + 8.0 * W, st);
  hipLaunchKernelGGL(smooth_kernel, dim3(grid), dim3(NT), 0, st, probs, W, NC, A, P, smoothed, top, top_score);
  KWS_LAUNCH_CHECK("smooth_kernel");
  return KWS_OK;
}

}  // extern "C"
