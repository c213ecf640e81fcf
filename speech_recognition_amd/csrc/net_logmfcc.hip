// Residual-block network programs.  One program class (LmProgram) runs one layer table, and the table is a composition:
//   stem -> [context unit] -> residual blocks -> [plain units] -> head
//   LmUnit   depthwise k 3 -> pointwise -> BatchNorm: the context unit, both halves of a block, a plain unit (unit_fwd / unit_bwd)
//   LmBlock  two units, the shortcut (identity, or a strided 1 x 1 Conv1D + BN), where the stride sits, and the join
//   LmStem   one gathered convolution; LmPaddedStem: on padded copies; LmStem2: two of them, concatenated
//   LmHead   LmAttentionHead (kws_lm_tail_*), LmPoolHead (kws_gp_tail_launch), LmGruHead (attention gate + BiGRU + kws_flat_tail_*)
// A training step is, in stream order: [grads zeroed], stem forward, body forward, the pointwise kernels transposed, the head with its
// backward (it leaves the gradient wrt the last activation in dO), body backward, stem backward; inference is the first, the second
// and the head.  Only the five builders at the end of the file know which model they build: conv_1d_log_mfcc / conv_1d_spectrogram,
// steffeNet, conv_1d_residual, conv_1d_mfcc_and_raw, xception_with_attention.
// Same building blocks as the raw-waveform net (f32-MFMA GEMMs with BN statistics in the epilogue, depthwise kernels applying
// BN + ReLU6 on load, fixed-order partial-slab reductions) plus resblock.hip.  Keras variable names follow per-class auto-numbering
// in layer creation order.
#include "net_internal.h"

namespace {

// depthwise k 3 -> pointwise -> BatchNorm over [Lin, cin] -> [Lout, cout]; whoever reads y applies the table and ReLU6
struct LmUnit {
  int64_t dw, pw;
  BnRef bn;
  int bn_idx, cin, cout, Lin, Lout, stride, pad_l;
  int slot;   // its workspace offsets: LmLayout::u[slot]
};
struct LmUnitWs { int64_t z = 0, y = 0, wt = 0; };   // depthwise output, pointwise output (pre-BN), pointwise kernel transposed (dgrad GEMM)

struct LmBlock {
  int nf, stride, cin, Lin, Lout;
  // where the stride sits: log-mfcc blocks pool after the second pointwise (pool = stride, Lmid = Lin); steffeNet blocks stride
  // their FIRST depthwise convolution (u1.stride = stride, pool = 1, Lmid = Lout)
  int pool, Lmid;
  int pool3 = 0, ppad = 0;  // conv_1d_residual: MaxPool1D(3, stride, 'same') join, window of output t starts at t*stride - ppad
  bool has_short;
  int64_t ws;          // the shortcut Conv1D(nf, 1, strides) over the rows gs gathers, and its BatchNorm
  BnRef bns;
  int bns_idx;
  kws_gather_t gs;
  LmUnit u1, u2;
  int slot;   // LmLayout::b[slot]
};
struct LmBlockWs { int64_t ys = 0, o = 0, wt_ws = 0; };   // shortcut convolution's output, the join's output, the shortcut kernel transposed

constexpr int64_t round64(int64_t floats) { return (floats + 63) / 64 * 64; }

// what the table's layers ask of the shared regions at batch B (floats)
struct LmSizes {
  int B = 0;
  int64_t o = 0, y = 0, z = 0, xs = 64, part = 0, wt = 0, tn = 0;
  int64_t tnq = 0;   // the pointwise weight gradients keep their slabs until one batched sum
  int64_t dwq = 0;   // depthwise backward kernels whose rows hold only a weight gradient: folded at the end
  void parts(int64_t floats) { part = std::max(part, floats); }
  void pw(int64_t M, int K, int N) {   // a GEMM with statistics rows whose weight gradient queues its slabs
    parts((int64_t)kws_gemm_num_row_tiles(M) * 2 * N);
    wt = std::max(wt, (int64_t)K * N);
    tn = std::max(tn, kws_gemm_tn_workspace_floats(M, K, N));
    tnq += round64(kws_gemm_tn_workspace_floats(M, K, N));
  }
  void unit(const LmUnit& u, bool parked) {   // parked: its backward takes the form that parks its rows in DwFinQueue
    z = std::max(z, (int64_t)B * u.Lout * u.cin);
    y = std::max(y, (int64_t)B * u.Lout * u.cout);
    pw((int64_t)B * u.Lout, u.cin, u.cout);
    parts(kws_dwconv_bwd_part_floats(B, u.Lin, u.cin));
    if (parked) dwq += round64(kws_dwconv_bwd_part_floats(B, u.Lin, u.cin));
  }
};

struct LmStemWs {
  int64_t y0 = 0, a0 = 0;                  // raw output(s) of the first convolution(s), the activation the body reads
  int64_t a0m = 0, a0r = 0;                // LmStem2: activated branch outputs before the concatenation
  int64_t xpad = 0, wpad = 0, gwpad = 0;   // LmPaddedStem: re-pitched input, padded kernel and its gradient
};
struct LmHeadWs {
  int64_t u = 0, fd = 0, dl = 0, gu = 0, coef2 = 0, per_loss = 0, per_correct = 0, att = 0;
  // LmGruHead: gate output, gate workspaces, GRU masks / output / saved steps / workspace / output gradient
  int64_t xgy = 0, xagf = 0, xagb = 0, gmx = 0, gmh = 0, gout = 0, gsave = 0, gws = 0, gdout = 0;
};
struct LmLayout {
  int64_t total = 0;
  LmStemWs stem;
  std::vector<LmUnitWs> u;
  std::vector<LmBlockWs> b;
  int64_t ac = 0, alast = 0;               // the context unit's and the last plain unit's activated output
  int64_t bn = 0, bn_stride = 0, part = 0, red = 0, coef = 0, WT = 0, tn = 0, swg = 0;
  int64_t tnq = 0, tnq_floats = 0;         // slabs of the pointwise weight gradients of one backward pass (KwsSlabQueue)
  int64_t dwq = 0, dwq_floats = 0;         // partial rows of the depthwise weight gradients folded by one launch (DwFinQueue)
  int64_t dOa = 0, dOb = 0, G = 0, DZ = 0, DXS = 0;
  LmHeadWs head;
};

// one call: what it received and the program's layout at its batch size
struct LmProgram;
struct Ctx : NetCall {
  LmLayout lo;
  bool ref_schedule;   // gemm mode 1, the A/B reference schedule: no fused depthwise passes, separate input- / weight-gradient launches
  Ctx(const LmProgram& p, const NetCall& n);
  float* bn_at(int idx) const { return ws + lo.bn + lo.bn_stride * idx; }
  float* stats() const { return training ? ws + lo.part : nullptr; }
  float* z(const LmUnit& u) const { return ws + lo.u[u.slot].z; }
  float* y(const LmUnit& u) const { return ws + lo.u[u.slot].y; }
  float* wt(const LmUnit& u) const { return ws + lo.u[u.slot].wt; }
};

// BN statistics -> table (training) or moving statistics -> table (inference)
int bn_table(const Ctx& c, const BnRef& r, int idx, int64_t M, int stat_rows) {
  if (c.training)
    return kws_bn_stats_finalize(c.ws + c.lo.part, stat_rows, M, r.C, c.params + r.gamma, c.params + r.beta, KWS_BN_EPS, KWS_BN_MOMENTUM,
                                 c.state + r.mm, c.state + r.mv, c.bn_at(idx), c.ws + c.lo.red, c.st);
  return kws_bn_infer_prepare(c.params + r.gamma, c.params + r.beta, c.state + r.mm, c.state + r.mv, KWS_BN_EPS, r.C, c.bn_at(idx), c.st);
}

// Depthwise backward kernels that leave ONLY a weight gradient behind (a block's first depthwise convolution, the context unit's, the
// first plain unit's: their input is a materialised activation, no BatchNorm in front): nothing on the dependency chain needs the fold of
// their partial rows, so the rows stay in regions of their own and one launch folds up to KWS_DW_FIN_BATCH layers at the end of the pass.
struct DwFinQueue {
  const float* part[KWS_DW_FIN_BATCH];
  float* dw[KWS_DW_FIN_BATCH];
  int n_parts[KWS_DW_FIN_BATCH], C[KWS_DW_FIN_BATCH];
  int count = 0;
  float* base = nullptr;
  int64_t used = 0, cap = 0;
  hipStream_t st = nullptr;
  int flush() {
    if (count == 0) return KWS_OK;
    const int rc = kws_dw_grad_finalize_batch(part, n_parts, C, dw, count, st);
    count = 0; used = 0;
    return rc;
  }
  // a region for the rows of one depthwise backward launch (floats = kws_dwconv_bwd_part_floats) whose fold writes dW
  int take(int64_t floats, int Cc, float* dW, float** out) {
    const int64_t need = round64(floats);
    if (count == KWS_DW_FIN_BATCH || used + need > cap) KWS_TRY(flush());
    if (need > cap) return KWS_E_WORKSPACE;
    *out = base + used;
    part[count] = base + used; dw[count] = dW; n_parts[count] = (int)(floats / (5 * Cc)); C[count] = Cc;
    used += need; ++count;
    return KWS_OK;
  }
};

// one backward pass: its scratch, the two gradient buffers that trade places layer by layer (dO: wrt the current layer's output) and
// the two queues of deferred weight-gradient sums
struct LmBwd {
  const Ctx& c;
  float *part, *red, *coef, *G, *DZ, *DXS, *dO, *dX;
  KwsSlabQueue sq;
  DwFinQueue dq;
  explicit LmBwd(const Ctx& c_) : c(c_) {
    const LmLayout& lo = c.lo;
    part = c.ws + lo.part; red = c.ws + lo.red; coef = c.ws + lo.coef; G = c.ws + lo.G; DZ = c.ws + lo.DZ; DXS = c.ws + lo.DXS;
    dO = c.ws + lo.dOa; dX = c.ws + lo.dOb;
    sq.base = c.ws + lo.tnq; sq.cap = lo.tnq_floats; sq.allow_pair = !c.ref_schedule;
    dq.base = c.ws + lo.dwq; dq.cap = lo.dwq_floats; dq.st = c.st;
  }
  // join backward + BatchNorm backward in two passes (round 4): reductions, fold (dgamma, dbeta, c1 | c2), then the masked /
  // pool-routed gradient is recomputed and dy written directly - 5 tensor passes instead of the 6 of "kws_block_out_bwd,
  // fold, kws_bn_bwd_apply", <= 256 partial rows (no slice fold), one launch less per join.  `outp` may be `dOin` (pool 1).
  int join_bwd(const float* dOin, const float* yv, const BnRef& r, int bn_idx, float* outp, int L, int C, int pool, int relu) {
    const float* bn = c.bn_at(bn_idx);
    KWS_TRY(kws_block_join_bwd(dOin, yv, bn, nullptr, nullptr, nullptr, part, 1, c.B, L, C, pool, relu, c.st));
    KWS_TRY(kws_dw_bwd_finalize(part, kws_block_join_bwd_parts(c.B, L, C, pool), (int64_t)c.B * L, C, nullptr, c.grads + r.gamma,
                                c.grads + r.beta, coef, red, c.st));
    return kws_block_join_bwd(dOin, yv, bn, c.params + r.gamma, coef, outp, nullptr, 2, c.B, L, C, pool, relu, c.st);
  }
};

// ---- the unit's two steps -----------------------------------------------------------------------------------------------------------
// `prod`: `in` is that unit's raw output, read through its BatchNorm + ReLU6; NULL: a materialised activation.
// z_ready: a fused pass in front wrote the depthwise output already
int unit_fwd(const Ctx& c, const LmUnit& u, const float* in, const LmUnit* prod, bool z_ready = false) {
  const int64_t M = (int64_t)c.B * u.Lout;
  if (!z_ready)
    KWS_TRY(kws_dwconv_fwd_f32(in, prod ? c.bn_at(prod->bn_idx) : nullptr, c.params + u.dw, c.z(u), c.B, u.Lin, u.Lout, u.cin, u.stride,
                               u.pad_l, c.st));
  KWS_TRY(kws_gemm_nn_f32(c.z(u), c.params + u.pw, c.y(u), M, u.cin, u.cout, c.stats(), c.st));
  return bn_table(c, u.bn, u.bn_idx, M, kws_gemm_nn_stats_rows(M, u.cin, u.cout));
}

// a strided block's shortcut branch: its BN (no mask, in place on dO), the 1 x 1 convolution's weight gradient (slabs queued: summed
// with the pass's other weight gradients) and its input gradient on the Lout strided rows, left in DXS
int short_bwd(LmBwd& k, const LmBlock& b, const float* xin) {
  const Ctx& c = k.c;
  const LmBlockWs& w = c.lo.b[b.slot];
  KWS_TRY(k.join_bwd(k.dO, c.ws + w.ys, b.bns, b.bns_idx, k.dO, b.Lout, b.nf, 1, 0));
  KWS_TRY(k.sq.gemm_gather(xin, &b.gs, k.dO, c.grads + b.ws, c.B, b.nf, c.st));
  return kws_gemm_nn_f32(k.dO, c.ws + w.wt_ws, k.DXS, (int64_t)c.B * b.Lout, b.nf, b.cin, nullptr, c.st);
}

// what joins the input gradient while the parked-rows form writes it: nothing; `add`, elementwise (an identity shortcut); or the input
// gradient of block sc's shortcut branch on every sc->stride-th row - that branch then runs here, after the rows are parked
struct LmDxJoin { const float* add = nullptr; const LmBlock* sc = nullptr; };
// k.G = the gradient wrt y -> the pointwise kernel's gradient and dz (one launch where the pair kernel takes the shape), then the
// depthwise backward.  prod != NULL: two passes over dz and the producer's raw output - the producer's BatchNorm backward rides
// along, its masked gradient is never stored, k.G becomes the producer's dy.  prod NULL: k.dX = the gradient wrt `in`.
int unit_bwd(LmBwd& k, const LmUnit& u, const float* in, const LmUnit* prod, const LmDxJoin& j = LmDxJoin()) {
  const Ctx& c = k.c;
  const int B = c.B;
  const float* w = c.params + u.dw;
  KWS_TRY(k.sq.pair(k.G, c.wt(u), k.DZ, c.z(u), c.grads + u.pw, (int64_t)B * u.Lout, u.cin, u.cout, c.st));
  const int64_t rows = kws_dwconv_bwd_part_floats(B, u.Lin, u.cin);
  if (prod) {
    const float* bn = c.bn_at(prod->bn_idx);
    KWS_TRY(kws_dwconv_bwd_bn_f32(k.DZ, in, bn, w, nullptr, nullptr, k.part, 1, B, u.Lin, u.Lout, u.cin, u.stride, u.pad_l, c.st));
    KWS_TRY(kws_dw_bwd_finalize(k.part, (int)(rows / (5 * u.cin)), (int64_t)B * u.Lin, u.cin, c.grads + u.dw, c.grads + prod->bn.gamma,
                                c.grads + prod->bn.beta, k.coef, k.red, c.st));
    return kws_dwconv_bwd_bn_f32(k.DZ, in, bn, w, k.coef, k.G, nullptr, 2, B, u.Lin, u.Lout, u.cin, u.stride, u.pad_l, c.st);
  }
  float* dpart;   // only a weight gradient comes out of these rows: folded with the other layers' at the end of the pass
  KWS_TRY(k.dq.take(rows, u.cin, c.grads + u.dw, &dpart));
  if (j.sc) {
    KWS_TRY(short_bwd(k, *j.sc, in));
    return kws_dwconv_bwd_acc_strided_f32(k.DZ, in, w, k.DXS, j.sc->stride, j.sc->Lout, k.dX, dpart, B, u.Lin, u.Lout, u.cin, u.stride,
                                          u.pad_l, c.st);
  }
  if (j.add) return kws_dwconv_bwd_acc_f32(k.DZ, in, w, j.add, k.dX, dpart, B, u.Lin, u.Lout, u.cin, u.stride, u.pad_l, c.st);
  return kws_dwconv_bwd_f32(k.DZ, in, nullptr, w, k.dX, dpart, B, u.Lin, u.Lout, u.cin, u.stride, u.pad_l, c.st);
}
// a k 3 / stride 1 / 'same' depthwise convolution over exactly [L, C]: the pass that writes that tensor can write its output too
bool dw_follows(const LmUnit& u, int L, int C) { return u.stride == 1 && u.pad_l == 1 && u.Lout == u.Lin && u.Lin == L && u.cin == C; }

// ---- stems ----------------------------------------------------------------------------------------------------------------------------
// The base is the first form: ONE gathered convolution + BN (index 1) + ReLU6 -> a0 [B, L0, C0].
struct LmStem {
  int L0 = 0, C0 = 0;
  int64_t conv1 = 0;
  BnRef bn0;
  kws_gather_t g0;
  virtual ~LmStem() {}
  virtual void sizes(LmSizes* s) const { s->pw((int64_t)s->B * L0, g0.taps * g0.cin, C0); }   // (gathered weight gradients queue their slabs too)
  virtual void take_front(Bump& bp, int B, LmStemWs* w) const { w->y0 = bp.take((int64_t)B * L0 * C0); w->a0 = bp.take((int64_t)B * L0 * C0); }
  virtual void take_back(Bump&, int, LmStemWs*) const {}
  // the pre-BN tensor of BatchNorm `index`, where it is the stem's
  virtual bool view(const LmStemWs& w, int B, int index, int64_t* offset_floats, int64_t* count) const {
    if (index == 1) { *offset_floats = w.y0; *count = (int64_t)B * L0 * C0; }
    return index == 1;
  }
  // the gathered GEMM's operands: the input and the kernel as they are
  virtual int operands(const Ctx& c, const float** x0, const float** w0) const { *x0 = c.x; *w0 = c.params + conv1; return KWS_OK; }
  // dw_next != NULL: the activation pass writes that unit's depthwise output as well (kws_block_out_dw_fwd without a residual: bit-identical)
  virtual int forward(const Ctx& c, const LmUnit* dw_next) const {
    const int64_t M = (int64_t)c.B * L0;
    float *y0 = c.ws + c.lo.stem.y0, *a0 = c.ws + c.lo.stem.a0;
    const float *x0, *w0;
    KWS_TRY(operands(c, &x0, &w0));
    KWS_TRY(kws_gemm_gather_f32(x0, &g0, w0, y0, c.B, C0, c.stats(), c.st));
    KWS_TRY(bn_table(c, bn0, 1, M, kws_gemm_gather_stats_rows(M)));
    if (dw_next) return kws_block_out_dw_fwd(y0, c.bn_at(1), nullptr, nullptr, c.params + dw_next->dw, a0, c.z(*dw_next), c.B, L0, C0, 1, c.st);
    return kws_bn_relu6_apply(y0, c.bn_at(1), a0, M, C0, 1, c.st);
  }
  // k.dO = the gradient wrt a0.  Ends the pass: both queues are flushed, each form in its own stream order
  virtual int backward(LmBwd& k) const {
    const Ctx& c = k.c;
    KWS_TRY(k.dq.flush());     // the depthwise weight gradients whose rows were parked
    KWS_TRY(k.join_bwd(k.dO, c.ws + c.lo.stem.y0, bn0, 1, k.G, L0, C0, 1, 1));
    KWS_TRY(k.sq.gemm_gather(c.x, &g0, k.G, c.grads + conv1, c.B, C0, c.st));   // written in place: the slabs join the pass's batched sum
    return k.sq.flush(c.st);   // the pointwise weight gradients of the whole pass: one sum (two past 16 layers)
  }
};

// rows of F floats -> rows of Fp floats (Fp % 4 == 0), zero filled; one 16-byte store per thread
__global__ __launch_bounds__(256) void repitch_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t rows,
                                                      int F, int Fp) {
  const int q = Fp / 4;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < rows * q; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / q;
    const int f = (int)(i - r * q) * 4;
    const float* src = in + r * F + f;
    float4 v;
    v.x = f + 0 < F ? src[0] : 0.f;
    v.y = f + 1 < F ? src[1] : 0.f;
    v.z = f + 2 < F ? src[2] : 0.f;
    v.w = f + 3 < F ? src[3] : 0.f;
    *reinterpret_cast<float4*>(out + r * Fp + f) = v;
  }
}

// The second form: the gathered GEMM reads 16-byte vectors, so the kernel [taps, K, C0] runs as a zero-padded copy [taps, Kp, C0]
// and the padded weight gradient is copied back without the padding.
//   T0 > 0 (conv_1d_spectrogram, K = 257 bins): the input rows [T0, K] are re-pitched to Kp as well (plain 2-D copies)
//   T0 = 0 (steffeNet, one tap of K = 75 samples): the gather reads Kp = 76 samples per output row of the input as it is
struct LmPaddedStem : LmStem {
  int K = 0, Kp = 0, T0 = 0;
  void take_back(Bump& bp, int B, LmStemWs* w) const override {
    if (T0) w->xpad = bp.take((int64_t)B * T0 * Kp);
    w->wpad = bp.take((int64_t)g0.taps * Kp * C0);
    w->gwpad = bp.take((int64_t)g0.taps * Kp * C0);
  }
  int operands(const Ctx& c, const float** x0, const float** w0) const override {
    float *wp = c.ws + c.lo.stem.wpad, *xp = c.ws + c.lo.stem.xpad;
    *x0 = T0 ? xp : c.x; *w0 = wp;
    if (!T0) {
      KWS_HIP(hipMemcpyAsync(wp, c.params + conv1, (size_t)K * C0 * 4, hipMemcpyDeviceToDevice, c.st));
      KWS_HIP(hipMemsetAsync(wp + (size_t)K * C0, 0, (size_t)(Kp - K) * C0 * 4, c.st));
      return KWS_OK;
    }
    const int64_t rows = (int64_t)c.B * T0, n4 = rows * (Kp / 4);
    hipLaunchKernelGGL(repitch_kernel, dim3((unsigned)std::min<int64_t>(ceil_div64(n4, 256), 8192)), dim3(256), 0, c.st, c.x, xp, rows, K, Kp);
    KWS_LAUNCH_CHECK("repitch_kernel");
    KWS_HIP(hipMemsetAsync(wp, 0, (size_t)g0.taps * Kp * C0 * 4, c.st));
    KWS_HIP(hipMemcpy2DAsync(wp, (size_t)Kp * C0 * 4, c.params + conv1, (size_t)K * C0 * 4, (size_t)K * C0 * 4, g0.taps,
                             hipMemcpyDeviceToDevice, c.st));
    return KWS_OK;
  }
  int backward(LmBwd& k) const override {
    const Ctx& c = k.c;
    float* gw = c.ws + c.lo.stem.gwpad;
    KWS_TRY(k.dq.flush());
    KWS_TRY(k.join_bwd(k.dO, c.ws + c.lo.stem.y0, bn0, 1, k.G, L0, C0, 1, 1));
    KWS_TRY(k.sq.flush(c.st));
    // the gradient of the padded kernel (the forward of this step left the padded input in xpad), then its K rows per tap
    KWS_TRY(kws_gemm_tn_gather_f32(T0 ? c.ws + c.lo.stem.xpad : c.x, &g0, k.G, gw, c.B, C0, c.ws + c.lo.tn, c.st));
    if (!T0) KWS_HIP(hipMemcpyAsync(c.grads + conv1, gw, (size_t)K * C0 * 4, hipMemcpyDeviceToDevice, c.st));
    else KWS_HIP(hipMemcpy2DAsync(c.grads + conv1, (size_t)K * C0 * 4, gw, (size_t)Kp * C0 * 4, (size_t)K * C0 * 4, g0.taps,
                                  hipMemcpyDeviceToDevice, c.st));
    return KWS_OK;
  }
};

// out[r, 0:cols] = in[r, 0:cols] for row pitches ld_in / ld_out (channel concatenation and its backward split)
__global__ __launch_bounds__(256) void copy_cols_kernel(const float* __restrict__ in, int ld_in, float* __restrict__ out,
                                                        int ld_out, int64_t rows, int cols4) {
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < rows * cols4; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / cols4;
    const int c = (int)(i - r * cols4) * 4;
    *reinterpret_cast<float4*>(out + r * ld_out + c) = *reinterpret_cast<const float4*>(in + r * ld_in + c);
  }
}
int copy_cols(const float* in, int ld_in, float* out, int ld_out, int64_t rows, int cols, hipStream_t st) {
  KWS_REQUIRE(cols % 4 == 0 && ld_in % 4 == 0 && ld_out % 4 == 0, "copy_cols: widths must be multiples of 4");
  const int64_t n4 = rows * (cols / 4);
  hipLaunchKernelGGL(copy_cols_kernel, dim3((unsigned)std::min<int64_t>(ceil_div64(n4, 256), 8192)), dim3(256), 0, st, in,
                     ld_in, out, ld_out, rows, cols / 4);
  KWS_LAUNCH_CHECK("copy_cols_kernel");
  return KWS_OK;
}

// The third form (conv_1d_mfcc_and_raw): input rows are [mfcc | raw]; the base's convolution gives Cm channels, a second one
// (BN index 2) Cr, and a0 is their concatenation after BN + ReLU6: C0 = Cm + Cr.  y0 holds [B L0, Cm] then [B L0, Cr].
struct LmStem2 : LmStem {
  int Cm = 0, Cr = 0;
  int64_t conv1r = 0;
  BnRef bn0r;
  kws_gather_t g0r;
  void sizes(LmSizes* s) const override { LmStem::sizes(s); s->pw((int64_t)s->B * L0, g0r.taps * g0r.cin, Cr); }
  void take_front(Bump& bp, int B, LmStemWs* w) const override {
    LmStem::take_front(bp, B, w);
    w->a0m = bp.take((int64_t)B * L0 * Cm); w->a0r = bp.take((int64_t)B * L0 * Cr);
  }
  bool view(const LmStemWs& w, int B, int index, int64_t* offset_floats, int64_t* count) const override {
    if (index > 2) return false;
    *offset_floats = w.y0 + (index == 2 ? (int64_t)B * L0 * Cm : 0);
    *count = (int64_t)B * L0 * (index == 2 ? Cr : Cm);
    return true;
  }
  int forward(const Ctx& c, const LmUnit* dw_next) const override {
    KWS_REQUIRE(!dw_next, "net: the concatenating stem has no fused activation pass");
    const LmStemWs& w = c.lo.stem;
    const int64_t M = (int64_t)c.B * L0;
    float *ws = c.ws, *y0m = ws + w.y0, *y0r = y0m + M * Cm;
    KWS_TRY(kws_gemm_gather_f32(c.x, &g0, c.params + conv1, y0m, c.B, Cm, c.stats(), c.st));
    KWS_TRY(bn_table(c, bn0, 1, M, kws_gemm_gather_stats_rows(M)));
    KWS_TRY(kws_gemm_gather_f32(c.x, &g0r, c.params + conv1r, y0r, c.B, Cr, c.stats(), c.st));
    KWS_TRY(bn_table(c, bn0r, 2, M, kws_gemm_gather_stats_rows(M)));
    KWS_TRY(kws_bn_relu6_apply(y0m, c.bn_at(1), ws + w.a0m, M, Cm, 1, c.st));
    KWS_TRY(kws_bn_relu6_apply(y0r, c.bn_at(2), ws + w.a0r, M, Cr, 1, c.st));
    KWS_TRY(copy_cols(ws + w.a0m, Cm, ws + w.a0, C0, M, Cm, c.st));
    return copy_cols(ws + w.a0r, Cr, ws + w.a0 + Cm, C0, M, Cr, c.st);
  }
  int backward(LmBwd& k) const override {   // split the gradient of the concatenation, then each like a first convolution
    const Ctx& c = k.c;
    const int64_t M = (int64_t)c.B * L0;
    float *y0m = c.ws + c.lo.stem.y0, *dOm = k.dX, *dOr = k.dX + M * Cm;
    KWS_TRY(copy_cols(k.dO, C0, dOm, Cm, M, Cm, c.st));
    KWS_TRY(copy_cols(k.dO + Cm, C0, dOr, Cr, M, Cr, c.st));
    KWS_TRY(k.join_bwd(dOm, y0m, bn0, 1, k.G, L0, Cm, 1, 1));
    KWS_TRY(k.sq.gemm_gather(c.x, &g0, k.G, c.grads + conv1, c.B, Cm, c.st));
    KWS_TRY(k.join_bwd(dOr, y0m + M * Cm, bn0r, 2, k.G, L0, Cr, 1, 1));
    KWS_TRY(k.sq.gemm_gather(c.x, &g0r, k.G, c.grads + conv1r, c.B, Cr, c.st));
    KWS_TRY(k.sq.flush(c.st));
    return k.dq.flush();
  }
};

// ---- heads ----------------------------------------------------------------------------------------------------------------------------
// From the last activation x [B, T, C] to the class probabilities, through a Dense(NC) + softmax over `feat` values per clip.
struct LmHead {
  int T = 0, C = 0, NC = 0, feat = 0;
  int tail_T = 16;           // u / att: [B, tail_T]
  int64_t dk = 0, db = -1;   // dense_1/kernel, dense_1/bias (< 0: none)
  virtual ~LmHead() {}
  void add_dense(kws_net* n, int feat_, bool bias) {
    NC = n->cfg.num_classes; feat = feat_;
    dk = kws_net_add_tensor(n, "dense_1/kernel", {feat, NC}, false, KWS_L2_COEF, feat, NC, 0.f);
    if (bias) db = kws_net_add_tensor(n, "dense_1/bias", {NC}, false, 0.f, 0, 0, 0.f);
  }
  virtual void take(Bump& bp, int B, LmHeadWs* w) const {
    w->u = bp.take((int64_t)B * tail_T); w->fd = bp.take((int64_t)B * feat); w->dl = bp.take((int64_t)B * NC);
    w->gu = bp.take((int64_t)B * 16); w->coef2 = bp.take(4);
    w->per_loss = bp.take(B); w->per_correct = bp.take(B);
    w->att = bp.take((int64_t)B * tail_T);
  }
  // debug views 3 = attention weights, 4 = attention logits u; 1: not one of the head's
  virtual int view(const LmLayout& lo, int B, int training, int what, int64_t* offset_floats, int64_t* count) const {
    if (what != 3 && what != 4) return 1;
    *offset_floats = what == 3 ? lo.head.att : lo.head.u; *count = (int64_t)B * T;
    return KWS_OK;
  }
  virtual int predict(const Ctx& c, const float* x, float* probs) const = 0;
  // probs, metrics, the head's own gradients (the Dense weight gradient launched), and the gradient wrt x in k.dO
  virtual int train(LmBwd& k, const float* x, const float* labels, float* probs, float* metrics, int loss_batch) const = 0;
  int dense_wgrad(const Ctx& c) const {
    return kws_small_wgrad_launch(c.ws + c.lo.head.fd, c.ws + c.lo.head.dl, c.grads + dk, db >= 0 ? c.grads + db : nullptr, c.B, feat, NC,
                                  c.ws + c.lo.swg, c.st);
  }
};
// the attention branch of two heads: a depthwise kernel and a pointwise kernel to one channel, with its BatchNorm
struct LmAttLayers { int64_t dw = 0, pw = 0; BnRef bn; int bn_idx = 0; };

// softmax-over-time attention (depthwise k 3 -> pointwise to 1 channel -> BN), weighted sum over time, Dropout, Dense + softmax, CE
struct LmAttentionHead : LmHead {
  LmAttLayers att;
  float drop_keep = 1.f;
  kws_lm_tail_args args(const Ctx& c, const float* x, float* probs) const {
    kws_lm_tail_args t;
    memset(&t, 0, sizeof(t));
    t.x = x; t.probs = probs;
    t.wa = c.params + att.dw; t.Wa = c.params + att.pw; t.bn_gamma = c.params + att.bn.gamma; t.bn_beta = c.params + att.bn.beta;
    t.mm = c.state + att.bn.mm; t.mv = c.state + att.bn.mv;
    t.Wd = c.params + dk; t.bd = c.params + db;
    t.u = c.ws + c.lo.head.u; t.bn = c.bn_at(att.bn_idx);
    t.B = c.B; t.T = T; t.C = C; t.NC = NC; t.keep_prob = c.training ? drop_keep : 1.f; t.loss_batch = 1;
    return t;
  }
  int predict(const Ctx& c, const float* x, float* probs) const override {
    const kws_lm_tail_args t = args(c, x, probs);
    return kws_lm_tail_fwd(&t, 0, c.st);
  }
  int train(LmBwd& k, const float* x, const float* labels, float* probs, float* metrics, int loss_batch) const override {
    const Ctx& c = k.c;
    const LmHeadWs& w = c.lo.head;
    float* ws = c.ws;
    kws_lm_tail_args t = args(c, x, probs);
    t.labels = labels; t.dX = k.dO; t.fd = ws + w.fd; t.dl = ws + w.dl; t.gu = ws + w.gu;
    t.part = k.part; t.coef = ws + w.coef2; t.d_gamma = c.grads + att.bn.gamma; t.d_beta = c.grads + att.bn.beta;
    t.per_loss = ws + w.per_loss; t.per_correct = ws + w.per_correct; t.att = ws + w.att;
    t.seed = c.seed; t.step = c.step; t.loss_batch = loss_batch; t.row_offset = c.row_offset;
    KWS_TRY(kws_lm_tail_fwd(&t, 1, c.st));
    KWS_TRY(kws_metrics_launch(t.per_loss, t.per_correct, c.B, metrics, c.st));
    KWS_TRY(dense_wgrad(c));
    KWS_TRY(kws_lm_tail_bwd(&t, c.st));
    return kws_dw_bwd_finalize(k.part, c.B, 1, C, c.grads + att.dw, nullptr, c.grads + att.pw, nullptr, k.red, c.st);
  }
};

// GlobalAveragePooling1D, or GlobalMaxPooling1D ++ it, then Dropout, Dense + softmax and the loss (kws_gp_tail_args)
struct LmPoolHead : LmHead {
  bool pool_max = false;
  int loss_kind = 1;       // 0 = label-smoothed CE, 1 = keras categorical_crossentropy
  float label_smoothing = 0.f, drop_keep = 0.5f;
  kws_gp_tail_args args(const Ctx& c, const float* x, float* probs) const {   // inference as it stands
    kws_gp_tail_args g;
    memset(&g, 0, sizeof(g));
    g.x = x; g.Wd = c.params + dk; g.bd = db >= 0 ? c.params + db : nullptr; g.probs = probs;
    g.B = c.B; g.T = T; g.C = C; g.NC = NC;
    g.pool_max = pool_max; g.loss_kind = loss_kind; g.label_smoothing = label_smoothing; g.keep_prob = 1.f; g.loss_batch = 1;
    return g;
  }
  int predict(const Ctx& c, const float* x, float* probs) const override {
    const kws_gp_tail_args g = args(c, x, probs);
    return kws_gp_tail_launch(&g, 0, c.st);
  }
  int train(LmBwd& k, const float* x, const float* labels, float* probs, float* metrics, int loss_batch) const override {
    const Ctx& c = k.c;
    const LmHeadWs& w = c.lo.head;
    kws_gp_tail_args g = args(c, x, probs);
    g.labels = labels; g.dX = k.dO; g.fd = c.ws + w.fd; g.dl = c.ws + w.dl;
    g.per_loss = c.ws + w.per_loss; g.per_correct = c.ws + w.per_correct;
    g.seed = c.seed; g.step = c.step; g.keep_prob = drop_keep; g.loss_batch = loss_batch; g.row_offset = c.row_offset;
    KWS_TRY(kws_gp_tail_launch(&g, 1, c.st));
    KWS_TRY(kws_metrics_launch(g.per_loss, g.per_correct, c.B, metrics, c.st));
    return dense_wgrad(c);
  }
};

constexpr int XC_GATE_K = 5;          // _context_conv(x, 1, 5, padding='same'), model.py:973
constexpr int XC_GRU_UNITS = 192;     // GRU(192, ...), model.py:976
constexpr float XC_GRU_KEEP = 0.8f;   // dropout=0.2, recurrent_dropout=0.2

// xception_with_attention: the attention gate (depthwise kernel [1, 5, C, 1]) over x, a bidirectional GRU of H units on the gated
// sequence as it is, Dense + softmax over its signed [2 H] output (the flat tail's raw arm); the GRU carries the dropout
struct LmGruHead : LmHead {
  LmAttLayers att;
  int H = 0;
  int64_t gW[2] = {0, 0}, gU[2] = {0, 0}, gb[2] = {0, 0};
  void take(Bump& bp, int B, LmHeadWs* w) const override {
    LmHead::take(bp, B, w);
    w->xgy = bp.take((int64_t)B * T * C);
    w->xagf = bp.take(kws_attn_gate_fwd_floats(B, T, C, XC_GATE_K)); w->xagb = bp.take(kws_attn_gate_bwd_floats(B, T, C, XC_GATE_K));
    w->gmx = bp.take((int64_t)6 * B * C); w->gmh = bp.take((int64_t)6 * B * H);
    w->gout = bp.take((int64_t)B * 2 * H); w->gdout = bp.take((int64_t)B * 2 * H);
    w->gsave = bp.take(kws_gru_save_floats(B, T, H));
    w->gws = bp.take(kws_gru_workspace_floats(B, T, C, H, 1));
  }
  // 6 = gate output, 7 = the GRU's saved steps [2][4: z, r, c, h][B, T, H], 8 = GRU output, 9 = attention BN table
  int view(const LmLayout& lo, int B, int training, int what, int64_t* offset_floats, int64_t* count) const override {
    const LmHeadWs& w = lo.head;
    if (what == 6) { *offset_floats = w.xgy; *count = (int64_t)B * T * C; return KWS_OK; }
    KWS_REQUIRE(what != 7 || training, "lm_debug_view: view 7 exists in training only");
    if (what == 7) { *offset_floats = w.gsave; *count = kws_gru_save_floats(B, T, H); return KWS_OK; }
    if (what == 8) { *offset_floats = w.gout; *count = (int64_t)B * 2 * H; return KWS_OK; }
    if (what == 9) { *offset_floats = lo.bn + lo.bn_stride * att.bn_idx; *count = 4; return KWS_OK; }
    return LmHead::view(lo, B, training, what, offset_floats, count);
  }
  int gate_gru_fwd(const Ctx& c, const float* x) const {
    const LmHeadWs& w = c.lo.head;
    float* ws = c.ws;
    const float* p = c.params;
    KWS_TRY(kws_attn_gate_fwd_f32(x, p + att.dw, p + att.pw, p + att.bn.gamma, p + att.bn.beta, c.state + att.bn.mm, c.state + att.bn.mv,
                                  ws + w.u, c.bn_at(att.bn_idx), ws + w.att, ws + w.xgy, ws + w.xagf, c.B, T, C, XC_GATE_K,
                                  c.training ? 1 : 0, c.st));
    if (c.training) KWS_TRY(kws_gru_masks(ws + w.gmx, ws + w.gmh, c.B, C, H, XC_GRU_KEEP, c.seed, c.step, c.row_offset, c.st));
    return kws_gru_fwd_f32(ws + w.xgy, p + gW[0], p + gU[0], p + gb[0], p + gW[1], p + gU[1], p + gb[1], c.training ? ws + w.gmx : nullptr,
                           c.training ? ws + w.gmh : nullptr, ws + w.gout, c.training ? ws + w.gsave : nullptr, ws + w.gws, c.B, T, C, H,
                           c.st);
  }
  kws_flat_tail_args tail_args(const Ctx& c, float* probs) const {
    kws_flat_tail_args t;
    memset(&t, 0, sizeof(t));
    t.y = c.ws + c.lo.head.gout; t.Ng = feat; t.raw = 1;
    t.Wd = c.params + dk; t.bd = c.params + db; t.probs = probs;
    t.B = c.B; t.D = feat; t.F = feat; t.NC = NC; t.keep_prob = 1.f;
    return t;
  }
  int predict(const Ctx& c, const float* x, float* probs) const override {
    KWS_TRY(gate_gru_fwd(c, x));
    const kws_flat_tail_args t = tail_args(c, probs);
    return kws_flat_tail_launch(&t, 0, c.st);
  }
  // ... and back: the GRU's dx (in k.G) is the gate's dy, the gate's dx the last block's dO
  int train(LmBwd& k, const float* x, const float* labels, float* probs, float* metrics, int loss_batch) const override {
    const Ctx& c = k.c;
    const LmHeadWs& w = c.lo.head;
    float *ws = c.ws, *g = c.grads;
    const float* p = c.params;
    KWS_TRY(gate_gru_fwd(c, x));
    kws_flat_tail_args t = tail_args(c, probs);
    KWS_TRY(kws_flat_tail_train(&t, labels, ws + w.fd, ws + w.dl, ws + w.gdout, ws + w.per_loss, ws + w.per_correct, c.seed, c.step,
                                loss_batch, c.row_offset, metrics, c.st));
    KWS_TRY(dense_wgrad(c));
    KWS_TRY(kws_gru_bwd_f32(ws + w.gdout, ws + w.xgy, p + gW[0], p + gU[0], p + gW[1], p + gU[1], ws + w.gmx, ws + w.gmh, ws + w.gsave, k.G,
                            g + gW[0], g + gU[0], g + gb[0], g + gW[1], g + gU[1], g + gb[1], ws + w.gws, c.B, T, C, H, c.st));
    return kws_attn_gate_bwd_f32(k.G, x, ws + w.u, ws + w.att, c.bn_at(att.bn_idx), p + att.dw, p + att.pw, p + att.bn.gamma, k.dO,
                                 g + att.dw, g + att.pw, g + att.bn.gamma, g + att.bn.beta, ws + w.xagb, c.B, T, C, XC_GATE_K, 1, c.st);
  }
};

// ---- the program ----------------------------------------------------------------------------------------------------------------------
struct LmProgram : NetProgram {
  const kws_net* net = nullptr;
  std::unique_ptr<LmStem> stem;
  bool fuse_first_dw = false;   // the stem's activation pass also writes block 0's first depthwise output, where that follows it
  bool has_ctx = false;         // a unit between the stem and the blocks whose activated output is materialised (steffeNet's _context_conv)
  LmUnit ctx;
  std::vector<LmBlock> blocks;
  std::vector<LmUnit> plain;    // units without a residual after the blocks (conv_1d_residual's _reduce_block); the last activation is materialised
  std::unique_ptr<LmHead> head;
  int T = 0, C = 0;             // [T, C]: the running activation while the table is built, the head's input afterwards
  int n_units = 0, n_bn = 0, maxC = 0;   // maxC: the widest BatchNormalization of the table

  void layout(int B, LmLayout* lo) const {
    Bump bp;
    const LmStem& s = *stem;
    LmSizes m;
    m.B = B; m.o = m.y = (int64_t)B * s.L0 * s.C0;
    lo->u.assign(n_units, LmUnitWs());
    lo->b.assign(blocks.size(), LmBlockWs());
    auto take_acts = [&](const LmUnit& u) {
      lo->u[u.slot].z = bp.take((int64_t)B * u.Lout * u.cin);
      lo->u[u.slot].y = bp.take((int64_t)B * u.Lout * u.cout);
    };
    auto take_wt = [&](const LmUnit& u) { lo->u[u.slot].wt = bp.take((int64_t)u.cin * u.cout); };
    s.take_front(bp, B, &lo->stem);
    s.sizes(&m);
    m.parts(kws_block_out_bwd_part_floats(B, s.L0, s.C0, 1));
    if (has_ctx) {
      take_acts(ctx);
      lo->ac = bp.take((int64_t)B * ctx.Lout * ctx.cout);
      m.unit(ctx, true);
    }
    for (const LmBlock& b : blocks) {
      LmBlockWs& w = lo->b[b.slot];
      if (b.has_short) w.ys = bp.take((int64_t)B * b.Lout * b.nf);
      take_acts(b.u1); take_acts(b.u2);
      w.o = bp.take((int64_t)B * b.Lout * b.nf);
      m.o = std::max(m.o, std::max((int64_t)B * b.Lout * b.nf, (int64_t)B * b.Lin * b.cin));
      m.xs = std::max(m.xs, (int64_t)B * b.Lout * b.cin);
      m.unit(b.u1, true); m.unit(b.u2, false);
      if (b.has_short) m.pw((int64_t)B * b.Lout, b.cin, b.nf);
      m.parts(b.pool3 ? kws_block_out3_bwd_part_floats(B, b.Lmid, b.nf) : kws_block_out_bwd_part_floats(B, b.Lmid, b.nf, b.pool));
      m.parts(kws_block_out_bwd_part_floats(B, b.Lout, b.nf, 1));
    }
    for (size_t j = 0; j < plain.size(); ++j) {
      const LmUnit& q = plain[j];
      take_acts(q);
      m.o = std::max(m.o, std::max((int64_t)B * q.Lin * q.cin, (int64_t)B * q.Lout * q.cout));
      m.unit(q, j == 0);
      m.parts(kws_block_out_bwd_part_floats(B, q.Lout, q.cout, 1));
    }
    if (!plain.empty()) lo->alast = bp.take((int64_t)B * T * C);
    m.parts((int64_t)B * 5 * C);
    lo->bn_stride = 4 * maxC;
    lo->bn = bp.take(lo->bn_stride * (n_bn + 1));
    lo->part = bp.take(m.part);
    lo->red = bp.take((int64_t)KWS_REDUCE_SLICES * 5 * maxC);
    lo->coef = bp.take(2 * maxC);
    lo->WT = bp.take(m.wt);
    for (const LmBlock& b : blocks) {
      take_wt(b.u1); take_wt(b.u2);
      if (b.has_short) lo->b[b.slot].wt_ws = bp.take((int64_t)b.cin * b.nf);
    }
    for (const LmUnit& q : plain) take_wt(q);
    if (has_ctx) take_wt(ctx);
    lo->tn = bp.take(m.tn);
    lo->tnq_floats = m.tnq; lo->tnq = bp.take(m.tnq);
    lo->dwq_floats = m.dwq; lo->dwq = bp.take(m.dwq);
    lo->swg = bp.take((int64_t)KWS_SMALL_WGRAD_SLICES * head->feat * head->NC);
    lo->dOa = bp.take(m.o); lo->dOb = bp.take(m.o);
    lo->G = bp.take(m.y); lo->DZ = bp.take(m.z); lo->DXS = bp.take(m.xs);
    head->take(bp, B, &lo->head);
    s.take_back(bp, B, &lo->stem);
    lo->total = bp.cur * 4;
  }

  // block 0's first unit where the stem's activation pass writes its depthwise output
  const LmUnit* fused_first_dw(const Ctx& c) const {
    if (!fuse_first_dw || c.ref_schedule || blocks.empty()) return nullptr;
    return dw_follows(blocks[0].u1, stem->L0, stem->C0) ? &blocks[0].u1 : nullptr;
  }

  // from the stem's activation a0 to the last activation *x_last
  int body_forward(const Ctx& c, const float** x_last) const {
    const LmLayout& lo = c.lo;
    float* ws = c.ws;
    const int B = c.B;
    const float* xin = ws + lo.stem.a0;
    if (has_ctx) {
      KWS_TRY(unit_fwd(c, ctx, xin, nullptr));
      KWS_TRY(kws_bn_relu6_apply(c.y(ctx), c.bn_at(ctx.bn_idx), ws + lo.ac, (int64_t)B * ctx.Lout, ctx.cout, 1, c.st));
      xin = ws + lo.ac;
    }
    bool z1_ready = fused_first_dw(c) != nullptr;   // the first block's first depthwise output already written by the stem
    for (size_t i = 0; i < blocks.size(); ++i) {
      const LmBlock& b = blocks[i];
      const LmBlockWs& w = lo.b[i];
      if (b.has_short) {
        // the shortcut convolution (1 x 1, stride s): over an even-length input it is every s-th ROW of the block input - a plain GEMM
        // with a row pitch on the wave-specialised kernel (round 6); the gathered kernel otherwise
        const int64_t Ms = (int64_t)B * b.Lout;
        int lda = 0, srows = kws_gemm_gather_stats_rows(Ms);
        int rs = 1;
        if (kws_gather_strided_rows(&b.gs, &lda)) {
          rs = kws_gemm_nn_strided_f32(xin, lda, c.params + b.ws, ws + w.ys, Ms, b.gs.cin, b.nf, c.stats(), c.st);
          if (rs < 0) return rs;
          if (rs == 0 && c.training) srows = kws_gemm_nn_stats_rows(Ms, b.gs.cin, b.nf);
        }
        if (rs != 0) KWS_TRY(kws_gemm_gather_f32(xin, &b.gs, c.params + b.ws, ws + w.ys, B, b.nf, c.stats(), c.st));
        KWS_TRY(bn_table(c, b.bns, b.bns_idx, Ms, srows));
      }
      KWS_TRY(unit_fwd(c, b.u1, xin, nullptr, z1_ready));   // (z1_ready: written by the previous block's join, below)
      KWS_TRY(unit_fwd(c, b.u2, c.y(b.u1), &b.u1));
      const float* y2 = c.y(b.u2);
      const float* bn2 = c.bn_at(b.u2.bn_idx);
      const float* res = b.has_short ? ws + w.ys : xin;
      const float* res_bn = b.has_short ? c.bn_at(b.bns_idx) : nullptr;
      // round 6: the join writes the NEXT block's first depthwise output too where that is a k 3 / stride 1 / 'same' convolution over this
      // block's output (every log-mfcc block): one tensor pass and one launch less per block, bit-identical (not in the reference schedule)
      const LmUnit* nx = i + 1 < blocks.size() ? &blocks[i + 1].u1 : nullptr;
      z1_ready = !b.pool3 && nx && !c.ref_schedule && dw_follows(*nx, b.Lout, b.nf);
      if (b.pool3) KWS_TRY(kws_block_out3_fwd(y2, bn2, res, res_bn, ws + w.o, B, b.Lmid, b.Lout, b.nf, b.stride, b.ppad, c.st));
      else if (z1_ready) KWS_TRY(kws_block_out_dw_fwd(y2, bn2, res, res_bn, c.params + nx->dw, ws + w.o, c.z(*nx), B, b.Lmid, b.nf, b.pool, c.st));
      else KWS_TRY(kws_block_out_fwd(y2, bn2, res, res_bn, ws + w.o, B, b.Lmid, b.nf, b.pool, c.st));
      xin = ws + w.o;
    }
    for (size_t j = 0; j < plain.size(); ++j) {
      KWS_TRY(unit_fwd(c, plain[j], j ? c.y(plain[j - 1]) : xin, j ? &plain[j - 1] : nullptr));
      if (j + 1 == plain.size()) {
        KWS_TRY(kws_bn_relu6_apply(c.y(plain[j]), c.bn_at(plain[j].bn_idx), ws + lo.alast, (int64_t)B * T, C, 1, c.st));
        xin = ws + lo.alast;
      }
    }
    *x_last = xin;
    return KWS_OK;
  }

  // every pointwise kernel transposed for its dgrad GEMM, KWS_TRANSPOSE_BATCH matrices per launch
  int transpose_pointwise(const Ctx& c) const {
    std::vector<const float*> tin;
    std::vector<float*> tout;
    std::vector<int> trows, tcols;
    auto add = [&](int64_t src, float* dst, int rows, int cols) {
      tin.push_back(c.params + src); tout.push_back(dst); trows.push_back(rows); tcols.push_back(cols);
    };
    auto add_unit = [&](const LmUnit& u) { add(u.pw, c.wt(u), u.cin, u.cout); };
    for (const LmBlock& b : blocks) {
      add_unit(b.u1); add_unit(b.u2);
      if (b.has_short) add(b.ws, c.ws + c.lo.b[b.slot].wt_ws, b.cin, b.nf);
    }
    for (const LmUnit& q : plain) add_unit(q);
    if (has_ctx) add_unit(ctx);
    for (size_t o = 0; o < tin.size(); o += KWS_TRANSPOSE_BATCH) {
      const int nbat = (int)std::min<size_t>(KWS_TRANSPOSE_BATCH, tin.size() - o);
      KWS_TRY(kws_transpose_batch_f32(tin.data() + o, tout.data() + o, trows.data() + o, tcols.data() + o, nbat, c.st));
    }
    return KWS_OK;
  }

  // k.dO = the gradient wrt the last activation -> k.dO = the gradient wrt the stem's activation a0
  int body_backward(LmBwd& k) const {
    const Ctx& c = k.c;
    const LmLayout& lo = c.lo;
    float* ws = c.ws;
    const int B = c.B;
    // ---- plain units, last to first: dO is the gradient wrt the materialised activation; below it k.G carries dy from unit to unit
    for (int j = (int)plain.size() - 1; j >= 0; --j) {
      const LmUnit& q = plain[j];
      if (j + 1 == (int)plain.size()) KWS_TRY(k.join_bwd(k.dO, c.y(q), q.bn, q.bn_idx, k.G, q.Lout, q.cout, 1, 1));
      KWS_TRY(unit_bwd(k, q, j ? c.y(plain[j - 1]) : ws + lo.b[blocks.size() - 1].o, j ? &plain[j - 1] : nullptr));
      if (j == 0) std::swap(k.dO, k.dX);
    }
    // ---- residual blocks, last to first ----
    for (int i = (int)blocks.size() - 1; i >= 0; --i) {
      const LmBlock& b = blocks[i];
      const float* xin = i ? ws + lo.b[i - 1].o : has_ctx ? ws + lo.ac : ws + lo.stem.a0;
      // main branch: join backward (maxpool routing + ReLU6 mask) -> BN2, then the second unit and the first
      if (b.pool3) {   // the 3-wide SAME join keeps the one-pass form (an input position collects up to three windows)
        const int64_t M = (int64_t)B * b.Lmid;
        const float* bn2 = c.bn_at(b.u2.bn_idx);
        KWS_TRY(kws_block_out3_bwd(k.dO, c.y(b.u2), bn2, k.G, k.part, B, b.Lmid, b.Lout, b.nf, b.stride, b.ppad, c.st));
        const int np = (int)(kws_block_out3_bwd_part_floats(B, b.Lmid, b.nf) / (5 * b.nf));
        KWS_TRY(kws_dw_bwd_finalize(k.part, np, M, b.nf, nullptr, c.grads + b.u2.bn.gamma, c.grads + b.u2.bn.beta, k.coef, k.red, c.st));
        KWS_TRY(kws_bn_bwd_apply(k.G, c.y(b.u2), bn2, c.params + b.u2.bn.gamma, k.coef, M, b.nf, c.st));
      } else {
        KWS_TRY(k.join_bwd(k.dO, c.y(b.u2), b.u2.bn, b.u2.bn_idx, k.G, b.Lmid, b.nf, b.pool, 1));
      }
      KWS_TRY(unit_bwd(k, b.u2, c.y(b.u1), &b.u1));
      // round 6: with a strided shortcut whose rows sit at whole multiples of the stride, the shortcut branch runs FIRST and its input
      // gradient joins the depthwise input gradient inside that kernel (same single addition per element: bit-identical) instead of an
      // add_strided pass afterwards; the reference schedule keeps the order and the launches of rounds 3 - 5
      const bool short_first = b.has_short && !c.ref_schedule && b.stride >= 2 && (int64_t)(b.Lout - 1) * b.stride < b.Lin;
      if (!b.has_short) {   // identity shortcut: the join's other gradient is added while the depthwise input gradient is written
        KWS_TRY(unit_bwd(k, b.u1, xin, nullptr, LmDxJoin{k.dO, nullptr}));
      } else if (short_first) {
        KWS_TRY(unit_bwd(k, b.u1, xin, nullptr, LmDxJoin{nullptr, &b}));
      } else {
        KWS_TRY(unit_bwd(k, b.u1, xin, nullptr));
        KWS_TRY(short_bwd(k, b, xin));   // residual branch
        KWS_TRY(kws_add_strided_f32(k.dX, k.DXS, B, b.Lin, b.Lout, b.cin, b.stride, c.st));
      }
      std::swap(k.dO, k.dX);
    }
    if (has_ctx) {   // dO is the gradient wrt the context unit's activated output
      KWS_TRY(k.join_bwd(k.dO, c.y(ctx), ctx.bn, ctx.bn_idx, k.G, ctx.Lout, ctx.cout, 1, 1));
      KWS_TRY(unit_bwd(k, ctx, ws + lo.stem.a0, nullptr));
      std::swap(k.dO, k.dX);
    }
    return KWS_OK;
  }

  int64_t workspace_bytes(int B, int) const override {
    LmLayout lo;
    layout(B, &lo);
    return lo.total;
  }
  // what: 0 = pre-BN tensor of BN `index` (1-based Keras numbering), 2 = BN table of BN `index`, 5 = the last block's output,
  //       the rest are the head's
  int debug_view(int B, int training, int what, int index, int64_t* offset_floats, int64_t* count) const override {
    LmLayout lo;
    layout(B, &lo);
    if (what == 2) {
      KWS_REQUIRE(index >= 1 && index <= n_bn, "lm_debug_view: bn index %d", index);
      *offset_floats = lo.bn + lo.bn_stride * index; *count = 4 * maxC;
      return KWS_OK;
    }
    if (what == 5) { *offset_floats = lo.b[blocks.size() - 1].o; *count = (int64_t)B * T * C; return KWS_OK; }
    const int rc = head->view(lo, B, training, what, offset_floats, count);
    if (rc != 1) return rc;
    auto unit_view = [&](const LmUnit& u) {
      if (index == u.bn_idx) { *offset_floats = lo.u[u.slot].y; *count = (int64_t)B * u.Lout * u.cout; }
      return index == u.bn_idx;
    };
    if (what == 0) {
      if (stem->view(lo.stem, B, index, offset_floats, count) || (has_ctx && unit_view(ctx))) return KWS_OK;
      for (const LmUnit& q : plain)
        if (unit_view(q)) return KWS_OK;
      for (const LmBlock& b : blocks) {
        if (b.has_short && index == b.bns_idx) { *offset_floats = lo.b[b.slot].ys; *count = (int64_t)B * b.Lout * b.nf; return KWS_OK; }
        if (unit_view(b.u1) || unit_view(b.u2)) return KWS_OK;
      }
    }
    kws_set_error("lm_debug_view: unknown view %d/%d", what, index);
    return KWS_E_INVALID;
  }
  int predict(const float* params, const float* state, const float* x, int B, float* probs, float* ws, int64_t ws_bytes,
              hipStream_t st) const override {
    const Ctx c(*this, NetCall{params, const_cast<float*>(state), x, B, false, nullptr, ws, 0, 0, 0, st});   // state is only read
    KWS_TRY(kws_workspace_check("net_predict", c.lo.total, ws_bytes, B));
    const float* x_last = nullptr;
    KWS_TRY(stem->forward(c, fused_first_dw(c)));
    KWS_TRY(body_forward(c, &x_last));
    return head->predict(c, x_last, probs);
  }
  int train(const float* params, float* state, const float* x, const float* y_onehot, int B, float* grads, float* probs, float* metrics,
            uint64_t seed, uint32_t step, int64_t row_offset, int loss_batch, float* ws, int64_t ws_bytes, hipStream_t st) const override {
    const Ctx c(*this, NetCall{params, state, x, B, true, grads, ws, seed, step, row_offset, st});
    KWS_TRY(kws_workspace_check("net_train_fwd_bwd", c.lo.total, ws_bytes, B));
    KWS_HIP(hipMemsetAsync(grads, 0, (size_t)net->n_params * 4, st));
    const float* x_last = nullptr;
    KWS_TRY(stem->forward(c, fused_first_dw(c)));
    KWS_TRY(body_forward(c, &x_last));
    KWS_TRY(transpose_pointwise(c));
    LmBwd k(c);
    KWS_TRY(head->train(k, x_last, y_onehot, probs, metrics, loss_batch));   // leaves the gradient wrt x_last in k.dO
    KWS_TRY(body_backward(k));
    return stem->backward(k);
  }
};

Ctx::Ctx(const LmProgram& p, const NetCall& n) : NetCall(n), ref_schedule(kws_net_get_gemm_mode(p.net) == 1) { p.layout(B, &lo); }

// ---- what the builders share ----------------------------------------------------------------------------------------------------------
// Where a residual block's stride sits (LmBlock::pool / Lmid / pool3 / ppad and its first unit's stride follow from it)
enum LmStridePlace {
  LM_POOL_AFTER,   // MaxPool1D(stride, stride) after the second pointwise convolution (conv_1d_log_mfcc)
  LM_STRIDED_DW,   // the block's first depthwise convolution is strided, 'same' (steffeNet)
  LM_POOL3_SAME,   // MaxPool1D(3, stride, 'same') after the second pointwise (conv_1d_residual, conv_1d_mfcc_and_raw)
};

// Installs the program with its stem (L0 and C0 set): the running activation is the stem's [L0, C0]
LmProgram* lm_new(kws_net* n, LmStem* stem) {
  LmProgram* p = new LmProgram();
  n->program.reset(p);   // freed with the net when the builder fails
  p->net = n; p->stem.reset(stem);
  p->T = stem->L0; p->C = p->maxC = stem->C0;
  return p;
}

// Creates one unit's layers (Keras creation order: depthwise, pointwise, BatchNormalization) for the given geometry
LmUnit lm_unit(KerasNames& kn, LmProgram* p, int cin, int cout, int Lin, int Lout, int stride, int pad_l) {
  LmUnit u;
  u.cin = cin; u.cout = cout; u.Lin = Lin; u.Lout = Lout; u.stride = stride; u.pad_l = pad_l;
  u.dw = kn.dw(cin); u.pw = kn.conv(1, cin, cout, KWS_L2_COEF);
  u.bn = kn.bn(cout, &u.bn_idx);
  u.slot = p->n_units++;
  p->maxC = std::max(p->maxC, cout);
  return u;
}

// Appends one residual block of nf filters over the running activation [p->T, p->C] and moves that on to the block's
// output.  Keras creation order: shortcut Conv1D + BN (strided blocks only), then the two units.
int lm_add_block(KerasNames& kn, LmProgram* p, LmStridePlace place, int nf, int stride) {
  const int cin = p->C, L = p->T;
  LmBlock b{};
  b.nf = nf; b.stride = stride; b.cin = cin; b.Lin = L; b.pool = stride; b.Lmid = L;
  b.Lout = (L + stride - 1) / stride;   // Keras 'same' whichever layer carries the stride: ceil(L / stride)
  int s1 = 1, pad1 = 1;
  if (place == LM_STRIDED_DW) {
    kws_same_pad(L, 3, stride, &b.Lout, &pad1);
    s1 = stride; b.pool = 1; b.Lmid = b.Lout;
  } else if (place == LM_POOL3_SAME) {
    b.pool3 = 1;
    kws_same_pad(L, 3, stride, &b.Lout, &b.ppad);
  }
  b.has_short = stride != 1;
  if (b.has_short) {
    b.ws = kn.conv(1, cin, nf, 0.f);  // the shortcut Conv1D(nf, 1, strides) has no kernel_regularizer (model.py:1431-1432, 1692-1693)
    b.bns = kn.bn(nf, &b.bns_idx);
    b.gs.L_out = b.Lout; b.gs.cin = cin; b.gs.taps = 1; b.gs.stride_t = stride * cin; b.gs.stride_j = 0;
    b.gs.base_off = 0; b.gs.x_len = L * cin; b.gs.x_batch_stride = (int64_t)L * cin;
  } else {
    KWS_REQUIRE(cin == nf, "net: identity shortcut needs cin == nf");
  }
  b.u1 = lm_unit(kn, p, cin, nf, L, b.Lmid, s1, pad1);
  b.u2 = lm_unit(kn, p, nf, nf, b.Lmid, b.Lmid, 1, 1);
  b.slot = (int)p->blocks.size();
  p->blocks.push_back(b);
  p->C = nf; p->T = b.Lout;
  return KWS_OK;
}

// Appends a unit without a residual: _reduce_conv (strides 2, 'same') or _context_conv ('valid')
int lm_add_plain(KerasNames& kn, LmProgram* p, int cout, int stride) {
  int Lout = p->T - 2, pad_l = 0;
  if (stride != 1) kws_same_pad(p->T, 3, stride, &Lout, &pad_l);
  KWS_REQUIRE(Lout >= 1, "net: conv_1d_residual input too short");
  p->plain.push_back(lm_unit(kn, p, p->C, cout, p->T, Lout, stride, pad_l));
  p->C = cout; p->T = Lout;
  return KWS_OK;
}

// Closes the table with head h over the running activation; feat: the width of the dense layer's input
void lm_add_head(KerasNames& kn, LmProgram* p, LmHead* h, int feat, bool bias) {
  p->head.reset(h);
  h->T = p->T; h->C = p->C;
  h->add_dense(kn.n, feat, bias);
  p->n_bn = kn.n_bn;
}
LmPoolHead* lm_add_pool_head(KerasNames& kn, LmProgram* p, bool pool_max, bool bias, float drop_keep) {
  LmPoolHead* h = new LmPoolHead();
  h->pool_max = pool_max; h->drop_keep = drop_keep;
  lm_add_head(kn, p, h, pool_max ? 2 * p->C : p->C, bias);
  return h;
}
// the attention branch over the running activation: a k-wide depthwise kernel, Conv1D(1, 1) and its BatchNormalization
LmAttLayers lm_att_layers(KerasNames& kn, const LmProgram* p, int k) {
  LmAttLayers a;
  a.dw = kn.dwk(k, p->C); a.pw = kn.conv(1, p->C, 1, KWS_L2_COEF);
  a.bn = kn.bn(1, &a.bn_idx);
  return a;
}

// overlapping_time_slice_stack(x, 40, 20) SAME fused with Conv1D(64 fm, 3, strides=2) (model.py:881-884, 957-960), as the
// raw-waveform net's first convolution: the stem of conv_1d_residual and xception_with_attention
LmStem* time_slice_stem(KerasNames& kn, int input_size, int fm) {
  LmStem* s = new LmStem();
  int Lf, plf;
  kws_same_pad(input_size, 40, 20, &Lf, &plf);
  s->C0 = 64 * fm; s->L0 = (Lf - 3) / 2 + 1;
  s->conv1 = kn.conv(3, 40, s->C0, KWS_L2_COEF);
  s->bn0 = kn.bn(s->C0);
  kws_gather_t& g0 = s->g0;
  g0.L_out = s->L0; g0.cin = 40; g0.taps = 3; g0.stride_t = 2 * 20; g0.stride_j = 20; g0.base_off = -plf;
  g0.x_len = input_size; g0.x_batch_stride = input_size;
  return s;
}

}  // namespace

// conv_1d_log_mfcc_model (reference model.py:1400-1479; SURVEY 8a row a19, layer table Appendix B.2): Conv1D(64, 3) + BN + ReLU6 on
// [98, 40] features, 10 residual blocks, softmax-over-time attention, Dropout(.2), Dense(num_classes) + softmax, categorical
// cross-entropy.  conv_1d_spectrogram_model (model.py:1482-1561) is the same table on 257-bin input, its stem on re-pitched copies.
int lm_build(kws_net* n) {
  const kws_net_config_t& c = n->cfg;
  KWS_REQUIRE(c.spectrogram_length >= 19 && c.num_features >= 4 && c.input_size == c.spectrogram_length * c.num_features,
              "net: log-mfcc input %d != %d x %d", c.input_size, c.spectrogram_length, c.num_features);
  KerasNames kn{n};
  const int T0 = c.spectrogram_length, F = c.num_features;
  const int Fp = (F + 3) & ~3;   // F rounded up to the 16-byte vectors of the gathered GEMM (spectrogram input: 257 -> 260)
  LmPaddedStem* ps = Fp != F ? new LmPaddedStem() : nullptr;
  if (ps) { ps->K = F; ps->Kp = Fp; ps->T0 = T0; }
  LmStem* s = ps ? ps : new LmStem();
  s->C0 = 64; s->L0 = T0 - 2;
  LmProgram* p = lm_new(n, s);
  s->conv1 = kn.conv(3, F, s->C0, KWS_L2_COEF);
  s->bn0 = kn.bn(s->C0);
  kws_gather_t& g0 = s->g0;
  g0.L_out = s->L0; g0.cin = Fp; g0.taps = 3; g0.stride_t = Fp; g0.stride_j = Fp; g0.base_off = 0;
  g0.x_len = T0 * Fp; g0.x_batch_stride = T0 * Fp;
  p->fuse_first_dw = true;   // (round 6) block 0 starts with a k 3 / stride 1 / 'same' depthwise convolution over the stem's activation
  // any length: the strided blocks are Keras 'same' layers - MaxPool1D(2, 2) and Conv1D(nf, 1, strides=2) both give
  // ceil(L / 2), e.g. the function's own default spectrogram_length = 65 -> 63 -> 32 -> 16 -> 8 (model.py:1410)
  static const int spec[10][2] = {{64, 1}, {64, 1}, {128, 2}, {128, 1}, {192, 2}, {192, 1}, {192, 1}, {256, 2},
                                  {256, 1}, {256, 1}};  // model.py:1453-1462
  for (const int* b : spec) KWS_TRY(lm_add_block(kn, p, LM_POOL_AFTER, b[0], b[1]));
  KWS_REQUIRE(p->T <= 16, "net: %d time steps at the tail (max 16)", p->T);
  LmAttentionHead* h = new LmAttentionHead();
  h->drop_keep = 0.8f;   // Dropout(0.2), model.py:1471
  h->att = lm_att_layers(kn, p, 3);
  lm_add_head(kn, p, h, p->C, true);
  return KWS_OK;
}

// steffeNet, reference model.py:1663-1726
int steffe_build(kws_net* n) {
  const kws_net_config_t& c = n->cfg;
  KWS_REQUIRE(c.input_size >= 3200 && c.input_size % 2 == 0, "net: steffeNet input_size %d", c.input_size);
  KerasNames kn{n};
  // Conv1D(256, 75, strides=50, padding='same', use_bias=False): no kernel_regularizer (model.py:1705); its 75 taps on one channel are
  // gathered as ONE tap of 76 samples against a zero-padded kernel
  LmPaddedStem* s = new LmPaddedStem();
  s->K = 75; s->Kp = 76; s->C0 = 256;
  int pl0;
  kws_same_pad(c.input_size, s->K, 50, &s->L0, &pl0);
  LmProgram* p = lm_new(n, s);
  KWS_REQUIRE(pl0 % 2 == 0, "net: steffeNet left padding %d must be even (8-byte gather loads)", pl0);
  s->conv1 = kn.conv(s->K, 1, s->C0, 0.f);
  s->bn0 = kn.bn(s->C0);
  kws_gather_t& g0 = s->g0;
  g0.L_out = s->L0; g0.cin = s->Kp; g0.taps = 1; g0.stride_t = 50; g0.stride_j = 0; g0.base_off = -pl0;
  g0.x_len = c.input_size; g0.x_batch_stride = c.input_size;
  p->has_ctx = true;   // _context_conv(x, 256, 3, padding='same'), model.py:1708
  p->ctx = lm_unit(kn, p, s->C0, s->C0, s->L0, s->L0, 1, 1);
  static const int widths[6] = {320, 384, 512, 768, 1024, 1536};  // model.py:1709
  for (int nf : widths)
    for (int stride = 2; stride >= 1; --stride) KWS_TRY(lm_add_block(kn, p, LM_STRIDED_DW, nf, stride));
  KWS_REQUIRE(p->T >= 1 && p->T <= 64, "net: %d time steps at the tail", p->T);
  // GlobalMaxPooling1D ++ GlobalAveragePooling1D -> Dropout(0.5) -> Dense(use_bias=False), model.py:1712-1718; loss: model.py:1722-1724
  LmPoolHead* h = lm_add_pool_head(kn, p, true, false, 0.5f);
  h->loss_kind = 0; h->label_smoothing = 0.1f;
  return KWS_OK;
}

// conv_1d_residual_model, reference model.py:841-908
int residual_build(kws_net* n) {
  const kws_net_config_t& c = n->cfg;
  KWS_REQUIRE(c.input_size >= 4000 && c.input_size % 2 == 0, "net: conv_1d_residual input_size %d", c.input_size);
  const int fm = c.filter_mult > 0 ? c.filter_mult : 1;
  KerasNames kn{n};
  LmProgram* p = lm_new(n, time_slice_stem(kn, c.input_size, fm));
  static const int spec[13][2] = {{128, 2}, {256, 2}, {256, 1}, {256, 1}, {256, 1}, {256, 1}, {256, 1}, {256, 1},
                                  {256, 1}, {256, 1}, {512, 2}, {728, 2}, {728, 2}};  // model.py:888-894
  for (const int* b : spec) KWS_TRY(lm_add_block(kn, p, LM_POOL3_SAME, b[0] * fm, b[1]));
  // _reduce_block(x, 1024, 3): _reduce_conv (strides 2, 'same') then _context_conv ('valid'), model.py:895
  KWS_TRY(lm_add_plain(kn, p, 1024 * fm, 2));
  KWS_TRY(lm_add_plain(kn, p, 1024 * fm, 1));
  KWS_REQUIRE(p->T <= 64, "net: %d time steps at the tail", p->T);
  lm_add_pool_head(kn, p, false, true, 0.5f);   // GlobalAveragePooling1D -> Dropout(0.5) -> Dense, model.py:898-905
  return KWS_OK;
}

// xception_with_attention_model, reference model.py:911-983: conv_1d_residual's stem, eleven of its blocks, attention gate, BiGRU
int xception_build(kws_net* n) {
  const kws_net_config_t& c = n->cfg;
  KWS_REQUIRE(c.input_size >= 4000 && c.input_size % 2 == 0, "net: xception_with_attention input_size %d", c.input_size);
  const int fm = c.filter_mult > 0 ? c.filter_mult : 1;
  KerasNames kn{n};
  LmProgram* p = lm_new(n, time_slice_stem(kn, c.input_size, fm));
  static const int spec[11][2] = {{128, 2}, {256, 2}, {256, 1}, {256, 1}, {256, 1}, {256, 1}, {256, 1}, {256, 1},
                                  {256, 1}, {256, 1}, {384, 2}};  // model.py:964-968
  for (const int* b : spec) KWS_TRY(lm_add_block(kn, p, LM_POOL3_SAME, b[0] * fm, b[1]));
  KWS_REQUIRE(kws_attn_gate_fwd_floats(1, p->T, p->C, XC_GATE_K) > 0, "net: xception_with_attention tail [%d, %d] is outside the attention gate's domain",
              p->T, p->C);
  LmGruHead* h = new LmGruHead();
  h->tail_T = p->T;
  h->att = lm_att_layers(kn, p, XC_GATE_K);   // _context_conv(x, 1, 5, padding='same'), model.py:973
  h->H = XC_GRU_UNITS;
  const int H = h->H;
  for (int d = 0; d < 2; ++d) {   // kernel_regularizer=l2(1e-5) reaches `kernel` only; recurrent_kernel: Orthogonal, drawn by the host
    const std::string base = std::string("bidirectional_1/") + (d ? "backward" : "forward") + "_gru_1/";
    h->gW[d] = kws_net_add_tensor(n, base + "kernel", {p->C, 3 * H}, false, KWS_L2_COEF, p->C, 3 * H, 0.f);
    h->gU[d] = kws_net_add_tensor(n, base + "recurrent_kernel", {H, 3 * H}, false, 0.f, 0, 0, 0.f);
    h->gb[d] = kws_net_add_tensor(n, base + "bias", {3 * H}, false, 0.f, 0, 0, 0.f);
  }
  lm_add_head(kn, p, h, 2 * H, true);   // no Dropout layer: the GRU carries the model's dropout
  return KWS_OK;
}

// conv_1d_mfcc_and_raw_model, reference model.py:1563-1660.  Input rows: [mfcc T*F | raw L].
int mfcc_raw_build(kws_net* n) {
  const kws_net_config_t& c = n->cfg;
  const int T = c.spectrogram_length, F = c.num_features;
  KWS_REQUIRE(T >= 19 && F >= 4 && F % 4 == 0 && c.input_size > T * F, "net: mfcc_and_raw input %d, features %d x %d",
              c.input_size, T, F);
  const int Lraw = c.input_size - T * F;
  const int frame_len = 480, frame_step = 160;   // window_size_samples / window_stride_samples of prepare_model_settings
  KWS_REQUIRE(1 + (Lraw - frame_len) / frame_step == T && (T * F) % 4 == 0 && Lraw % 2 == 0,
              "net: mfcc_and_raw needs 1 + (raw %d - 480) / 160 == spectrogram_length %d", Lraw, T);
  KerasNames kn{n};
  LmStem2* s = new LmStem2();
  s->Cm = 64; s->Cr = 96; s->C0 = s->Cm + s->Cr; s->L0 = T - 2;
  LmProgram* p = lm_new(n, s);
  s->conv1 = kn.conv(3, F, s->Cm, KWS_L2_COEF);            // model.py:1615
  s->bn0 = kn.bn(s->Cm);
  s->conv1r = kn.conv(3, frame_len, s->Cr, KWS_L2_COEF);   // model.py:1625
  s->bn0r = kn.bn(s->Cr);
  kws_gather_t g;
  g.L_out = s->L0; g.cin = F; g.taps = 3; g.stride_t = F; g.stride_j = F; g.base_off = 0;
  g.x_len = T * F; g.x_batch_stride = c.input_size;
  s->g0 = g;
  // overlapping_time_slice_stack(x, 480, 160, 'VALID') fused with Conv1D(96, 3): row t reads 3 frames 160 apart
  g.cin = frame_len; g.stride_t = frame_step; g.stride_j = frame_step; g.base_off = T * F; g.x_len = c.input_size;
  s->g0r = g;
  static const int spec[10][2] = {{160, 1}, {160, 1}, {192, 2}, {192, 1}, {256, 2}, {256, 1}, {320, 2}, {320, 1},
                                  {384, 2}, {384, 1}};  // model.py:1632-1641
  for (const int* b : spec) KWS_TRY(lm_add_block(kn, p, LM_POOL3_SAME, b[0], b[1]));
  lm_add_pool_head(kn, p, false, true, 0.7f);   // GlobalAveragePooling1D -> Dropout(0.3) -> Dense, model.py:1648
  return KWS_OK;
}
