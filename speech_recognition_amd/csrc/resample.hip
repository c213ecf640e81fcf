// Rational polyphase resampling of wav rows on the device (kws_resample_*): wavs of any sample rate enter the clip
// bank at the model's rate.
//
// The definition is scipy.signal.resample_poly(x, up, down) at its defaults (window ('kaiser', 5.0), constant padding):
//   g = gcd(rate_out, rate_in), up = rate_out / g, down = rate_in / g, mx = max(up, down), half = 10 mx,
//   h[j] = up w[j] fc sinc(fc (j - half)) / S over 2 half + 1 taps, fc = 1 / mx, w = kaiser(2 half + 1, 5), S = the
//   sum of the unscaled windowed taps;
//   y[n] = sum_j h[j] xu[n down + half - j], xu[i up] = x[i] and zero elsewhere, n_out = ceil(n_in up / down).
// With p = n down + half, q = p / up and r = p mod up only the taps j = r + k up meet a sample: x[q - k].  The device
// table is phase major and time reversed, tab[r][t] = h[r + (T - 1 - t) up] (zero where that index passes 2 half),
// T = ceil((2 half + 1) / up), rows padded with zeros to Tp = a multiple of 4 floats, so that
//   y[n] = sum_t tab[r][t] x[q - (T - 1) + t]
// runs over two contiguous ascending sequences.
//
// resample_kernel: a workgroup of NT threads walks tiles of 4 NT consecutive outputs of one row (grid stride over
// (row, tile): a row may be millions of samples long, a batch may hold more tiles than the grid has workgroups).  Per
// tile it stages the input span [lo, hi + 3] the tile needs as floats in LDS, zeros standing in for everything outside
// the row's n_valid samples (nothing past n_valid is read), and every thread forms 4 consecutive outputs, each from Tp / 4
// 16-byte table reads and the Tp samples beside them; the 4 values leave as one 16-byte (f32) / 8-byte (int16) store
// where the output row allows it.  The table sits in LDS beside the tile when both fit in 64 KB (staged once per
// workgroup, not per tile) and is read from global memory (it stays in L2) when they do not.  A tile that lies past the
// row's resampled length writes zeros without staging anything.  Every output element is written exactly once; there
// are no atomics; equal inputs give equal bits whatever the batch around the row (a row's sums do not depend on the
// grid).  Inputs are expected to be finite: a zero tap of a padded table row still multiplies a sample.
// For up = 1 (48 kHz or 32 kHz -> 16 kHz) the 4 outputs of a thread share the one phase: decimate4() reads the union of their
// windows once, 16 bytes at a time, and takes the taps from scalar registers.
// resample_direct_kernel: ratios whose span for the smallest tile (256 outputs) does not fit in LDS (down / up in the
// hundreds) read samples and taps from global memory, one thread per output, the same sum in the same order.
// resample_copy_kernel: equal rates (up = down = 1) copy; the filter is not run (in float it is no identity).
#include <math.h>

#include <vector>

#include "common.h"

struct kws_resample_plan {
  int rate_in = 0, rate_out = 0, up = 1, down = 1, half = 0, T = 0, Tp = 0;
  int cus = 0;
  float* tab = nullptr;  // [up][Tp]
  float* dec = nullptr;  // up = 1: [3 down + ni] the one phase row between zeros, ni = 4 ceil((3 down + T) / 4)
  int ni = 0;
};

namespace {

constexpr int MAX_FACTOR = 65536;        // max(up, down): a prototype of 20 * 65536 + 1 floats (5 MB)
constexpr int LDS_BYTES = 64 * 1024;     // what one workgroup takes at most (tile + table)
constexpr int XS_BYTES = 32 * 1024;      // ... of which the staged input span
constexpr int PER = 4;                   // consecutive outputs per thread

struct Design {
  int up, down, half, T;
};

int64_t gcd64(int64_t a, int64_t b) {
  while (b) {
    const int64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

bool design(int rate_in, int rate_out, Design* d) {
  if (rate_in < 1 || rate_out < 1) return false;
  const int64_t g = gcd64(rate_in, rate_out);
  const int64_t up = rate_out / g, down = rate_in / g, mx = up > down ? up : down;
  if (mx > MAX_FACTOR) return false;
  d->up = (int)up;
  d->down = (int)down;
  d->half = (int)(10 * mx);
  d->T = (int)((2 * (int64_t)d->half + 1 + up - 1) / up);
  return true;
}

// modified Bessel function I0 by its power series (terms (x^2 / 4)^k / (k!)^2; beta = 5 needs about 25 of them)
double bessel_i0(double x) {
  const double y = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 200; ++k) {
    term *= y / ((double)k * (double)k);
    sum += term;
    if (term < 1e-18 * sum) break;
  }
  return sum;
}

// the prototype in double: np.kaiser(2 half + 1, 5.0) * fc * np.sinc(fc * (j - half)), unit sum, times up
void taps_f64(const Design& d, std::vector<double>* h) {
  const int64_t n = 2 * (int64_t)d.half + 1;
  const double mx = d.up > d.down ? d.up : d.down, fc = 1.0 / mx, beta = 5.0, i0b = bessel_i0(beta);
  h->resize((size_t)n);
  double S = 0.0;
  for (int64_t j = 0; j < n; ++j) {
    const double m = (double)(j - d.half);
    const double a = m / (double)d.half;  // (2 j / (n - 1)) - 1
    const double arg = 1.0 - a * a;
    const double w = bessel_i0(beta * sqrt(arg > 0.0 ? arg : 0.0)) / i0b;
    const double z = M_PI * (fc * m);  // np.sinc's argument, bit for bit: at the sinc's zeros the tap IS the rounding of pi (fc m)
    const double s = (j == d.half) ? 1.0 : sin(z) / z;
    (*h)[(size_t)j] = w * fc * s;
    S += (*h)[(size_t)j];
  }
  for (int64_t j = 0; j < n; ++j) (*h)[(size_t)j] = (double)d.up * (*h)[(size_t)j] / S;
}

int64_t out_samples(const Design& d, int64_t n_in) { return (n_in * d.up + d.down - 1) / d.down; }

// floats of LDS a tile of `tile` outputs stages: its span is at most (tile - 1) down / up + 1 + T samples, plus the 3 zeros
// the padded table rows reach, rounded to a multiple of 4 (the table behind it stays 16-byte aligned)
int64_t span_floats(const Design& d, int Tp, int tile) {
  const int64_t s = ((int64_t)(tile - 1) * d.down) / d.up + 1 + Tp + 3;
  return (s + 3) / 4 * 4;
}

struct ResampleArgs {
  const void* x;
  const int32_t* n_valid;
  int16_t* out_i16;
  float* out_f32;
  const float* tab;
  int64_t x_pitch, total_tiles;
  int n_in, B, keep, up, down, half, T, Tp, tiles_per_row, xs_floats, vec_f32, vec_i16;
  unsigned dq, dr;  // down / up, down mod up
  const float* dec;  // up = 1 (kws_resample_plan::dec), else NULL
  int ni;
};

__device__ __forceinline__ int16_t to_i16(float v) { return (int16_t)(int)fminf(fmaxf(rintf(v), -32768.f), 32767.f); }

__device__ __forceinline__ int valid_samples(const ResampleArgs& a, int64_t row) {
  int nv = a.n_valid ? a.n_valid[row] : a.n_in;
  nv = nv < 0 ? 0 : nv;
  return nv > a.n_in ? a.n_in : nv;
}

typedef float rs_v4f __attribute__((ext_vector_type(4)));
typedef short rs_v4s __attribute__((ext_vector_type(4)));

// v[0 .. 4) -> out[row][n .. n + 4), cropped at n1 (the tile's / row's end).  The whole quads leave as ONE non-temporal 16-byte
// (8-byte) store: the output is streamed, and a plain vector store is taken apart again when the compiler merges it with the
// scalar path beside it (3 + 1 dwords in the ISA)
__device__ __forceinline__ void store4(const ResampleArgs& a, int64_t row, int n, int n1, const float (&v)[PER]) {
  const int64_t o = row * a.keep + n;
  const bool full = n + PER <= n1;
  if (a.out_f32) {
    if (full && a.vec_f32) {
      const rs_v4f q = {v[0], v[1], v[2], v[3]};
      __builtin_nontemporal_store(q, reinterpret_cast<rs_v4f*>(a.out_f32 + o));
    } else {
#pragma unroll
      for (int m = 0; m < PER; ++m)
        if (n + m < n1) a.out_f32[o + m] = v[m];
    }
  }
  if (a.out_i16) {
    if (full && a.vec_i16) {
      const rs_v4s q = {to_i16(v[0]), to_i16(v[1]), to_i16(v[2]), to_i16(v[3])};
      __builtin_nontemporal_store(q, reinterpret_cast<rs_v4s*>(a.out_i16 + o));
    } else {
#pragma unroll
      for (int m = 0; m < PER; ++m)
        if (n + m < n1) a.out_i16[o + m] = to_i16(v[m]);
    }
  }
}

// up = 1: the 4 consecutive outputs of a thread share the one phase, and their windows start `down` samples apart from a
// 16-byte-aligned place (4 tid down floats into the tile).  The union of the windows is read ONCE, as float4s, and sample i
// meets tap i - m down of output m: the taps come from the row dec[] = 3 down zeros | tab[0][0 .. T) | zeros, at addresses
// that are the same for every lane - scalar loads, no LDS traffic.  Per output the terms are those of the general loop in
// the same order, between products with zero taps.
typedef const __attribute__((address_space(4))) float* rs_const_f32;
__device__ __forceinline__ void decimate4(const ResampleArgs& a, const float4* xw, float (&acc)[PER]) {
  rs_const_f32 h = (rs_const_f32)(uintptr_t)a.dec + 3 * a.down;
#pragma unroll
  for (int m = 0; m < PER; ++m) acc[m] = 0.f;
  for (int i = 0; i < a.ni; i += 4) {
    const float4 X = xw[i >> 2];
#pragma unroll
    for (int m = 0; m < PER; ++m) {
      rs_const_f32 hm = h + i - m * a.down;
      acc[m] = fmaf(hm[0], X.x, acc[m]);
      acc[m] = fmaf(hm[1], X.y, acc[m]);
      acc[m] = fmaf(hm[2], X.z, acc[m]);
      acc[m] = fmaf(hm[3], X.w, acc[m]);
    }
  }
}

constexpr int TAB_GLOBAL = 0, TAB_LDS = 1, DECIMATE = 2;  // where resample_kernel's taps come from

template <typename TIn, int MODE>
__global__ __launch_bounds__(256) void resample_kernel(ResampleArgs a) {
  extern __shared__ float4 smem4[];
  float* xs = reinterpret_cast<float*>(smem4);
  const float4* tab4 = reinterpret_cast<const float4*>(a.tab);
  const int tid = threadIdx.x, nt = blockDim.x, tile = PER * nt, tp4 = a.Tp >> 2;
  if (MODE == TAB_LDS) {  // visible after the first tile's barrier (a workgroup with no tile to stage never reads it)
    float4* tl = smem4 + (a.xs_floats >> 2);
    for (int i = tid; i < a.up * tp4; i += nt) tl[i] = tab4[i];
    tab4 = tl;
  }
  for (int64_t t = blockIdx.x; t < a.total_tiles; t += gridDim.x) {
    const int64_t row = t / a.tiles_per_row;
    const int n0 = (int)(t - row * a.tiles_per_row) * tile;
    const int n1 = a.keep - n0 < tile ? a.keep : n0 + tile;
    const int nv = valid_samples(a, row);
    const int64_t n_out = ((int64_t)nv * a.up + a.down - 1) / a.down;
    const int n = n0 + PER * tid;
    float v[PER] = {0.f, 0.f, 0.f, 0.f};
    if (n0 < n_out) {  // uniform over the workgroup: the barriers below are met by all of it or by none
      const TIn* x = reinterpret_cast<const TIn*>(a.x) + row * a.x_pitch;
      // p = n down + half of the tile's first output once in 64 bits; everything inside the tile is an offset below 2^27
      const int64_t p0 = (int64_t)n0 * a.down + a.half;
      const int64_t q0 = p0 / a.up;
      const unsigned r0 = (unsigned)(p0 - q0 * a.up);
      const unsigned last = (unsigned)((n1 < n_out ? n1 : (int)n_out) - 1 - n0);
      const int64_t lo = q0 - (a.T - 1);                                           // first sample under the tile
      const int cnt = (int)((r0 + last * (unsigned)a.down) / (unsigned)a.up) + a.T;  // <= xs_floats - 3 (span_floats)
      __syncthreads();                                                             // the previous tile has been read
      // up = 1: every thread with an output reads the ni samples from its first window on (decimate4 below)
      const int stage = MODE == DECIMATE ? (int)(last / PER) * PER * a.down + a.ni : cnt + 3;
      for (int i = tid; i < stage; i += nt) {
        const int64_t g = lo + i;
        xs[i] = ((MODE == DECIMATE || i < cnt) && g >= 0 && g < nv) ? (float)x[g] : 0.f;
      }
      __syncthreads();
      if (MODE == DECIMATE) {
        if (n < n1 && n < n_out) {
          float acc[PER];
          decimate4(a, reinterpret_cast<const float4*>(xs) + tid * a.down, acc);
#pragma unroll
          for (int m = 0; m < PER; ++m)
            if (n + m < n1 && n + m < n_out) v[m] = acc[m];
        }
        if (n < n1) store4(a, row, n, n1, v);
        continue;
      }
      const unsigned s = r0 + (unsigned)(PER * tid) * (unsigned)a.down;
      unsigned q = s / (unsigned)a.up;          // sample under the last tap (t = T - 1), relative to q0: xs[q + t] is under t
      unsigned r = s - q * (unsigned)a.up;      // phase
#pragma unroll
      for (int m = 0; m < PER; ++m) {
        if (n + m < n1 && n + m < n_out) {
          const float* xw = xs + q;
          const float4* w = tab4 + (size_t)r * tp4;
          float acc = 0.f;
          for (int k = 0; k < tp4; ++k) {
            const float4 c = w[k];
            acc = fmaf(c.x, xw[4 * k], acc);
            acc = fmaf(c.y, xw[4 * k + 1], acc);
            acc = fmaf(c.z, xw[4 * k + 2], acc);
            acc = fmaf(c.w, xw[4 * k + 3], acc);
          }
          v[m] = acc;
        }
        q += a.dq;
        r += a.dr;
        if (r >= (unsigned)a.up) {
          r -= a.up;
          ++q;
        }
      }
    }
    if (n < n1) store4(a, row, n, n1, v);
  }
}

// one thread per 4 consecutive outputs, everything from global memory; the sum runs over the same t in the same order
template <typename TIn>
__global__ __launch_bounds__(256) void resample_direct_kernel(ResampleArgs a) {
  const int quads = (a.keep + PER - 1) / PER;
  const int64_t total = (int64_t)a.B * quads;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / quads;
    const int n = (int)(i - row * quads) * PER;
    const int nv = valid_samples(a, row);
    const int64_t n_out = ((int64_t)nv * a.up + a.down - 1) / a.down;
    const TIn* x = reinterpret_cast<const TIn*>(a.x) + row * a.x_pitch;
    float v[PER] = {0.f, 0.f, 0.f, 0.f};
    for (int m = 0; m < PER; ++m) {
      if (n + m < a.keep && n + m < n_out) {
        const int64_t p = (int64_t)(n + m) * a.down + a.half;
        const int64_t q = p / a.up;
        const int r = (int)(p - q * a.up);
        const int64_t g0 = q - (a.T - 1);  // sample under t = 0
        const int t_lo = g0 < 0 ? (int)(-g0 < a.T ? -g0 : a.T) : 0;
        const int t_hi = nv - g0 < a.T ? (int)(nv - g0 > 0 ? nv - g0 : 0) : a.T;
        const float* w = a.tab + (int64_t)r * a.Tp;
        float acc = 0.f;
        for (int t = t_lo; t < t_hi; ++t) acc = fmaf(w[t], (float)x[g0 + t], acc);
        v[m] = acc;
      }
    }
    store4(a, row, n, a.keep, v);
  }
}

template <typename TIn>
__global__ __launch_bounds__(256) void resample_copy_kernel(ResampleArgs a) {
  const int64_t total = (int64_t)a.B * a.keep;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / a.keep;
    const int n = (int)(i - row * a.keep);
    const bool in = n < valid_samples(a, row);
    const TIn* x = reinterpret_cast<const TIn*>(a.x) + row * a.x_pitch;
    if (sizeof(TIn) == 2) {
      const int16_t s = in ? (int16_t)x[n] : (int16_t)0;
      if (a.out_f32) a.out_f32[i] = (float)s;
      if (a.out_i16) a.out_i16[i] = s;
    } else {
      a.out_f32[i] = in ? (float)x[n] : 0.f;
    }
  }
}

template <typename TIn>
int resample_launch(const kws_resample_plan* p, const TIn* x, int64_t x_pitch, const int32_t* n_valid, int n_in, int16_t* out_i16,
                    float* out_f32, int B, int keep, void* stream) {
  KWS_REQUIRE(p && x && (out_i16 || out_f32), "resample: NULL pointer");
  KWS_REQUIRE(B >= 0 && keep >= 0 && n_in >= 0 && x_pitch >= n_in, "resample: B=%d keep=%d n_in=%d x_pitch=%lld", B, keep, n_in,
              (long long)x_pitch);
  if (B == 0 || keep == 0) return KWS_OK;
  hipStream_t st = (hipStream_t)stream;
  ResampleArgs a;
  a.x = x; a.n_valid = n_valid; a.out_i16 = out_i16; a.out_f32 = out_f32; a.tab = p->tab;
  a.x_pitch = x_pitch; a.n_in = n_in; a.B = B; a.keep = keep;
  a.up = p->up; a.down = p->down; a.half = p->half; a.T = p->T; a.Tp = p->Tp;
  a.vec_f32 = keep % 4 == 0 && ((uintptr_t)out_f32 & 15) == 0;
  a.vec_i16 = keep % 4 == 0 && ((uintptr_t)out_i16 & 7) == 0;
  a.tiles_per_row = 0; a.total_tiles = 0; a.xs_floats = 0;
  a.dq = (unsigned)(p->down / p->up); a.dr = (unsigned)(p->down % p->up);
  a.dec = nullptr; a.ni = 0;
  const double bytes = (double)B * ((double)n_in * sizeof(TIn) + (double)keep * ((out_f32 ? 4.0 : 0.0) + (out_i16 ? 2.0 : 0.0)));
  KwsProfScope prof("resample", 2.0 * B * keep * (double)p->T, bytes, st);
  const int cus = p->cus > 0 ? p->cus : 256;
  if (p->up == 1 && p->down == 1) {
    const int64_t blocks = ceil_div64((int64_t)B * keep, 256);
    const unsigned g = (unsigned)(blocks < (int64_t)cus * 8 ? blocks : (int64_t)cus * 8);
    hipLaunchKernelGGL(resample_copy_kernel<TIn>, dim3(g), dim3(256), 0, st, a);
    KWS_LAUNCH_CHECK("resample_copy_kernel");
    return KWS_OK;
  }
  const Design d{p->up, p->down, p->half, p->T};
  int nt = 0;
  for (int c = 256; c >= 64 && !nt; c >>= 1)
    if (span_floats(d, p->Tp, PER * c) * 4 <= XS_BYTES) nt = c;
  if (!nt) {
    const int64_t blocks = ceil_div64((int64_t)B * ceil_div(keep, PER), 256);
    const unsigned g = (unsigned)(blocks < (int64_t)cus * 8 ? blocks : (int64_t)cus * 8);
    hipLaunchKernelGGL(resample_direct_kernel<TIn>, dim3(g), dim3(256), 0, st, a);
    KWS_LAUNCH_CHECK("resample_direct_kernel");
    return KWS_OK;
  }
  a.xs_floats = (int)span_floats(d, p->Tp, PER * nt);
  a.dec = p->dec; a.ni = p->ni;   // (tile - 1) down + ni <= xs_floats: ni <= 3 down + T + 3
  a.tiles_per_row = ceil_div(keep, PER * nt);
  a.total_tiles = (int64_t)B * a.tiles_per_row;
  const int64_t tab_bytes = (int64_t)p->up * p->Tp * 4;
  const bool tab_lds = !p->dec && a.xs_floats * 4 + tab_bytes <= LDS_BYTES;
  const size_t lds = (size_t)a.xs_floats * 4 + (tab_lds ? (size_t)tab_bytes : 0);
  const int64_t cap = (int64_t)cus * 4;
  const unsigned g = (unsigned)(a.total_tiles < cap ? a.total_tiles : cap);
  if (p->dec)
    hipLaunchKernelGGL((resample_kernel<TIn, DECIMATE>), dim3(g), dim3(nt), lds, st, a);
  else if (tab_lds)
    hipLaunchKernelGGL((resample_kernel<TIn, TAB_LDS>), dim3(g), dim3(nt), lds, st, a);
  else
    hipLaunchKernelGGL((resample_kernel<TIn, TAB_GLOBAL>), dim3(g), dim3(nt), lds, st, a);
  KWS_LAUNCH_CHECK("resample_kernel");
  return KWS_OK;
}

}  // namespace

extern "C" {

int kws_resample_design(int rate_in, int rate_out, int* up, int* down, int* half_len, int* taps_per_phase) {
  Design d;
  KWS_REQUIRE(design(rate_in, rate_out, &d), "resample_design: rates %d -> %d (each >= 1, max(up, down) <= %d)", rate_in, rate_out,
              MAX_FACTOR);
  if (up) *up = d.up;
  if (down) *down = d.down;
  if (half_len) *half_len = d.half;
  if (taps_per_phase) *taps_per_phase = d.T;
  return KWS_OK;
}

int kws_resample_taps(int rate_in, int rate_out, float* h, int64_t n) {
  Design d;
  KWS_REQUIRE(design(rate_in, rate_out, &d), "resample_taps: rates %d -> %d (each >= 1, max(up, down) <= %d)", rate_in, rate_out,
              MAX_FACTOR);
  KWS_REQUIRE(h && n == 2 * (int64_t)d.half + 1, "resample_taps: n=%lld, the prototype has %lld taps", (long long)n,
              2 * (long long)d.half + 1);
  std::vector<double> h64;
  taps_f64(d, &h64);
  for (int64_t j = 0; j < n; ++j) h[j] = (float)h64[(size_t)j];
  return KWS_OK;
}

int64_t kws_resample_out_samples(int rate_in, int rate_out, int64_t n_in) {
  Design d;
  KWS_REQUIRE(design(rate_in, rate_out, &d), "resample_out_samples: rates %d -> %d (each >= 1, max(up, down) <= %d)", rate_in,
              rate_out, MAX_FACTOR);
  KWS_REQUIRE(n_in >= 0 && n_in <= INT64_MAX / MAX_FACTOR, "resample_out_samples: n_in=%lld", (long long)n_in);
  return out_samples(d, n_in);
}

int kws_resample_plan_create(int rate_in, int rate_out, kws_resample_plan_t** plan) {
  KWS_REQUIRE(plan, "resample_plan_create: NULL pointer");
  Design d;
  KWS_REQUIRE(design(rate_in, rate_out, &d), "resample_plan_create: rates %d -> %d (each >= 1, max(up, down) <= %d)", rate_in,
              rate_out, MAX_FACTOR);
  kws_resample_plan* p = new kws_resample_plan();
  p->rate_in = rate_in; p->rate_out = rate_out;
  p->up = d.up; p->down = d.down; p->half = d.half; p->T = d.T;
  p->Tp = (d.T + 3) / 4 * 4;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&p->cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) {
    delete p;
    kws_set_error("resample_plan_create: no device");
    return KWS_E_HIP;
  }
  if (d.up > 1 || d.down > 1) {
    std::vector<double> h64;
    taps_f64(d, &h64);
    std::vector<float> tab((size_t)d.up * p->Tp, 0.f);
    for (int r = 0; r < d.up; ++r)
      for (int t = 0; t < d.T; ++t) {
        const int64_t j = r + (int64_t)(d.T - 1 - t) * d.up;
        if (j <= 2 * (int64_t)d.half) tab[(size_t)r * p->Tp + t] = (float)h64[(size_t)j];
      }
    hipError_t e = hipMalloc((void**)&p->tab, tab.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(p->tab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess && d.up == 1) {
      p->ni = (3 * d.down + d.T + 3) / 4 * 4;
      std::vector<float> dec((size_t)3 * d.down + p->ni, 0.f);
      for (int t = 0; t < d.T; ++t) dec[(size_t)3 * d.down + t] = tab[t];
      e = hipMalloc((void**)&p->dec, dec.size() * sizeof(float));
      if (e == hipSuccess) e = hipMemcpy(p->dec, dec.data(), dec.size() * sizeof(float), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
      kws_set_error("resample_plan_create: table upload failed: %s", hipGetErrorString(e));
      kws_resample_plan_destroy(p);
      return KWS_E_HIP;
    }
  }
  *plan = p;
  return KWS_OK;
}

int kws_resample_plan_destroy(kws_resample_plan_t* p) {
  if (!p) return KWS_OK;
  (void)hipFree(p->tab);
  (void)hipFree(p->dec);
  delete p;
  return KWS_OK;
}

int kws_resample_i16(const kws_resample_plan_t* plan, const int16_t* x, int64_t x_pitch, const int32_t* n_valid, int n_in,
                     int16_t* out_i16, float* out_f32, int B, int keep, void* stream) {
  return resample_launch<int16_t>(plan, x, x_pitch, n_valid, n_in, out_i16, out_f32, B, keep, stream);
}

int kws_resample_f32(const kws_resample_plan_t* plan, const float* x, int64_t x_pitch, const int32_t* n_valid, int n_in, float* out,
                     int B, int keep, void* stream) {
  return resample_launch<float>(plan, x, x_pitch, n_valid, n_in, nullptr, out, B, keep, stream);
}

}  // extern "C"
