// Shared between the network programs.  A model kind runs on one NetProgram: a layer table built once by kws_net_create
// (the switch there maps a kind to its builder) plus the launch sequences over it.  Each family keeps its program class in
// its own file and exports only its builder(s):
//   net.hip          conv_1d_time_sliced_with_attention
//   net_logmfcc.hip  the residual-block family (LmProgram: a stem, units of depthwise k 3 -> pointwise -> BN, residual blocks, a head):
//                    conv_1d_log_mfcc / conv_1d_spectrogram, steffeNet, conv_1d_residual, conv_1d_mfcc_and_raw, xception_with_attention
//   net_grouped.hip  conv_1d_fast, conv_1d_spec, conv_1d_time_stacked, conv_1d_heavy, conv_1d_learned_spec, conv_1d_top_down
//   net_dwk.hip      conv_1d_gru, conv_1d_simple
//   net_time_sliced.hip  conv_1d_time_sliced
//   net_dw3ladder.hip  no builder of its own: the 3-tap depthwise ladder (Dw3Ladder) under net.hip and net_time_sliced.hip
//   net_mts.hip      conv_1d_multi_time_sliced
//   net_inception.hip  inception_d1
//   net_conv2d.hip   conv_2d_mobile, conv_2d_fast
// The five programs whose head is the flat tail (kws_flat_tail_*) - those of net_grouped.hip, net_dwk.hip, net_time_sliced.hip,
// net_mts.hip and net_inception.hip (GcProgram, DkProgram, TslProgram, MtProgram, IncProgram) - derive from FlatTailProgram
// below: it owns workspace_bytes, predict and the order of a training step, and a program supplies its layout, forward,
// tail_args and backward.  net.hip (attention tail, split step), net_logmfcc.hip (three heads behind its own LmHead; it shares NetCall
// and kws_flat_tail_train) and net_conv2d.hip (another tail) implement NetProgram directly.
// The BatchNorm bookkeeping all but net.hip and net_logmfcc.hip share is bncols.hip (kws_gbn_*, declared in internal.h).
// Not part of the public C ABI.
#pragma once
#include <string.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <string>
#include <vector>

#include "internal.h"

constexpr float KWS_BN_EPS = 1e-3f;
constexpr float KWS_BN_MOMENTUM = 0.99f;
constexpr float KWS_L2_COEF = 1e-5f;

struct BnRef {
  int64_t gamma, beta;  // param offsets
  int64_t mm, mv;       // state offsets
  int C;
};
// bncols.hip's launchers for ONE BatchNorm layer r (g = 1) over the columns c: its parameters / state, and its gradients in `grads`
inline kws_gbn_refs kws_gbn_layer_refs(const BnRef& r, const float* params, float* state) {
  return kws_gbn_refs{params + r.gamma, 0, r.beta - r.gamma, state + r.mm, 0, r.mv - r.mm};
}
inline int kws_gbn_layer_bwd(float* dA, const float* y, const float* bn, const float* add, int64_t M, const kws_gbn_cols& c, float* part,
                             float* coef, float* grads, const BnRef& r, hipStream_t st) {
  return kws_gbn_bwd(dA, y, bn, add, M, &c, part, coef, grads + r.gamma, 0, r.beta - r.gamma, st);
}
inline int kws_gbn_layer_bwd_finish(float* g, const float* y, const float* bn, int64_t M, const kws_gbn_cols& c, const float* part, int rows,
                                    float* coef, float* grads, const BnRef& r, hipStream_t st) {
  return kws_gbn_bwd_finish(g, y, bn, M, &c, part, rows, coef, grads + r.gamma, 0, r.beta - r.gamma, st);
}

// One model's layer table and its launch sequences on one HIP stream.  The public entry points of net.hip check their
// arguments and make one of these calls; `ws` is the caller's workspace of `ws_bytes` bytes.
struct NetProgram {
  virtual ~NetProgram() {}
  virtual int64_t workspace_bytes(int B, int training) const = 0;
  virtual int debug_view(int B, int training, int what, int index, int64_t* offset_floats, int64_t* count) const = 0;
  virtual int predict(const float* params, const float* state, const float* x, int B, float* probs, float* ws, int64_t ws_bytes,
                      hipStream_t st) const = 0;
  virtual int train(const float* params, float* state, const float* x, const float* y_onehot, int B, float* grads, float* probs,
                    float* metrics, uint64_t seed, uint32_t step, int64_t row_offset, int loss_batch, float* ws, int64_t ws_bytes,
                    hipStream_t st) const = 0;
};

struct kws_net {
  kws_net_config_t cfg;
  std::vector<kws_tensor_info_t> tensors;
  int64_t n_params = 0, n_state = 0;
  std::unique_ptr<NetProgram> program;  // installed by the kind's builder (also when it fails half way: freed with the net)
  // arithmetic of the pointwise GEMMs (kws_net_set_gemm_mode): 0 = f32 MFMA, 2 = fp16 x 2 split products (A/B arm)
  std::atomic<int> gemm_mode{0};
};

// Appends a Keras-named tensor to the flat parameter (or state) buffer; returns its float offset.
int64_t kws_net_add_tensor(kws_net* n, const std::string& name, std::vector<int64_t> shape, bool is_state, float l2,
                           int fan_in, int fan_out, float init);
BnRef kws_net_add_bn(kws_net* n, int idx, int C);
// Keras padding='same': output length and left padding of a k-wide window at stride s (TF puts the odd sample on the right)
void kws_same_pad(int L, int k, int s, int* Lout, int* pl);

// Keras names a layer by its class and a per-class counter in creation order, and those names are the checkpoint format.
// One KerasNames per table: the builders create their layers through it, in model.py's order.
struct KerasNames {
  kws_net* n;
  int n_conv = 0, n_bn = 0, n_dw = 0;
  int64_t conv(int k, int cin, int cout, float l2);  // conv1d_<n>/kernel [k, cin, cout]
  BnRef bn(int C, int* idx = nullptr);               // batch_normalization_<n>/...; *idx = n
  int64_t dw(int C);                                 // depthwise_conv2d_<n>/depthwise_kernel [1, 3, C, 1], l2
  int64_t dwk(int k, int C);                         // depthwise_conv2d_<n>/depthwise_kernel [1, k, C, 1], l2
};

struct Bump {
  int64_t cur = 0;  // in floats
  int64_t take(int64_t floats) {
    const int64_t o = cur;
    cur += (floats + 63) / 64 * 64;  // 256-B granules
    return o;
  }
};

// ---- the builders: each installs its program on the net and appends the net's tensors (net.hip keeps its own local) ------
int lm_build(kws_net* n);        // net_logmfcc.hip
int steffe_build(kws_net* n);
int residual_build(kws_net* n);
int mfcc_raw_build(kws_net* n);
int xception_build(kws_net* n);
int gc_build(kws_net* n);        // net_grouped.hip
int dk_build(kws_net* n);        // net_dwk.hip
int mt_build(kws_net* n);        // net_mts.hip
int inc_build(kws_net* n);       // net_inception.hip
int c2n_build(kws_net* n);       // net_conv2d.hip
int tsl_build(kws_net* n);       // net_time_sliced.hip

// ---- pieces the programs share (net.hip) -------------------------------------------------------------------------------
// KWS_E_WORKSPACE with its message when the caller's workspace is too small; who = "net_predict" / "net_train_fwd_bwd"
int kws_workspace_check(const char* who, int64_t need_bytes, int64_t ws_bytes, int B);
// The training step of a flat tail: t comes filled for inference; adds the training fields, launches the tail with
// training = 1 (probs, loss, fd, dl, dA) and then the batch metrics
int kws_flat_tail_train(kws_flat_tail_args* t, const float* labels, float* fd, float* dl, float* dA, float* per_loss,
                        float* per_correct, uint64_t seed, uint32_t step, int loss_batch, int64_t row_offset, float* metrics,
                        hipStream_t st);

// ---- the skeleton of the programs that end in the flat tail (kws_flat_tail_*: Dropout -> Dense + softmax -> loss) ------------
// the tail's training regions: dropped features [B, D], dlogits [B, NC], the per-clip loss and hit, the weight-gradient slices
struct FlatTailWs {
  int64_t fd = 0, dl = 0, per_loss = 0, per_correct = 0, swg = 0;
  void take(Bump& bp, int B, int D, int NC) {
    fd = bp.take((int64_t)B * D);
    dl = bp.take((int64_t)B * NC);
    per_loss = bp.take(B);
    per_correct = bp.take(B);
    swg = bp.take((int64_t)KWS_SMALL_WGRAD_SLICES * D * NC);
  }
};
// what every forward / backward pass of one call receives (predict: training false, grads NULL, seed = step = row_offset = 0)
struct NetCall {
  const float* params;
  float* state;   // training: moving statistics are updated
  const float* x;
  int B;
  bool training;
  float* grads;
  float* ws;
  uint64_t seed;
  uint32_t step;
  int64_t row_offset;
  hipStream_t st;
};
// the Dense + softmax layer the tail ends in: its kernel and bias in params / grads (bias < 0: none), its input width, the classes
struct FlatTailDense {
  int64_t kernel = 0, bias = -1;
  int D = 0, NC = 0;
};
// workspace_bytes, predict and train of such a program.  Layout: the program's workspace offsets, with `total` (bytes) and
// `tail` (a FlatTailWs, taken in training).  One training step is, in stream order: [grads zeroed], forward, the tail with its
// backward, the Dense layer's weight gradient, backward.
template <class Layout>
struct FlatTailProgram : NetProgram {
  const kws_net* net = nullptr;
  FlatTailDense dense;
  bool zero_grads = false;   // train zeroes the net's n_params gradients in front of the forward pass

  virtual void layout(int B, bool training, Layout* lo) const = 0;
  virtual int forward(const Layout& lo, const NetCall& c) const = 0;
  virtual kws_flat_tail_args tail_args(const Layout& lo, const NetCall& c, float* probs) const = 0;   // filled for inference
  virtual int64_t tail_grad(const Layout& lo) const = 0;   // where the tail leaves the gradient wrt its input (float offset)
  virtual int backward(const Layout& lo, const NetCall& c) const = 0;   // from that gradient down to the first layer

  int64_t workspace_bytes(int B, int training) const override {
    Layout lo;
    layout(B, training != 0, &lo);
    return lo.total;
  }
  int predict(const float* params, const float* state, const float* x, int B, float* probs, float* ws, int64_t ws_bytes,
              hipStream_t st) const override {
    Layout lo;
    layout(B, false, &lo);
    KWS_TRY(kws_workspace_check("net_predict", lo.total, ws_bytes, B));
    const NetCall c{params, const_cast<float*>(state), x, B, false, nullptr, ws, 0, 0, 0, st};   // state is only read
    KWS_TRY(forward(lo, c));
    const kws_flat_tail_args t = tail_args(lo, c, probs);
    return kws_flat_tail_launch(&t, 0, st);
  }
  int train(const float* params, float* state, const float* x, const float* y_onehot, int B, float* grads, float* probs, float* metrics,
            uint64_t seed, uint32_t step, int64_t row_offset, int loss_batch, float* ws, int64_t ws_bytes, hipStream_t st) const override {
    Layout lo;
    layout(B, true, &lo);
    KWS_TRY(kws_workspace_check("net_train_fwd_bwd", lo.total, ws_bytes, B));
    const NetCall c{params, state, x, B, true, grads, ws, seed, step, row_offset, st};
    if (zero_grads) KWS_HIP(hipMemsetAsync(grads, 0, (size_t)net->n_params * 4, st));
    KWS_TRY(forward(lo, c));
    kws_flat_tail_args t = tail_args(lo, c, probs);
    const FlatTailWs& w = lo.tail;
    KWS_TRY(kws_flat_tail_train(&t, y_onehot, ws + w.fd, ws + w.dl, ws + tail_grad(lo), ws + w.per_loss, ws + w.per_correct, seed, step,
                                loss_batch, row_offset, metrics, st));
    KWS_TRY(kws_small_wgrad_launch(ws + w.fd, ws + w.dl, grads + dense.kernel, dense.bias >= 0 ? grads + dense.bias : nullptr, B, dense.D,
                                   dense.NC, ws + w.swg, st));
    return backward(lo, c);
  }
};

// ---- the hidden Dense layer of conv_1d_gru and conv_1d_time_sliced (net_dwk.hip) ------------------------------------------
constexpr int DK_BIAS_SLICES = 32;
// tab [4][n] = 1 | bias (0 without one) | 0 | 1: what the flat tail reads as a BatchNorm table over the layer's output
int dk_bias_table(const float* bias, int n, float* tab, hipStream_t st);
// gradient wrt relu6(h + bias) -> gradient wrt h, in place on d [B, n]; bias and dbias may be NULL; part: DK_BIAS_SLICES * n floats
int dk_bias_relu6_bwd(float* d, const float* h, const float* bias, float* dbias, int B, int n, float* part, hipStream_t st);
// the whole layer h = in W (+ bias) backwards: d [B, H] = gradient wrt relu6(h + bias) -> wrt h (in place), dW [D, H] and dbias,
// out [B, D] = gradient wrt in.  Scratch: WT D * H floats, tn kws_gemm_tn_workspace_floats(B, D, H), part as above
struct DkDenseBwdScratch {
  float *WT, *tn, *part;
};
int dk_dense_bwd(float* d, const float* h, const float* in, const float* W, const float* bias, float* dW, float* dbias, float* out, int B,
                 int D, int H, const DkDenseBwdScratch& s, hipStream_t st);

// ---- the k-wide depthwise-separable block of net_dwk.hip and net_mts.hip (net_sepblock.hip) ------------------------------
// DepthwiseConv2D((1, k), strides) -> Conv1D(cout, 1) -> BatchNormalization -> relu6
struct SepBlock {
  int Lin = 0, Lout = 0, k = 0, stride = 1, pad_l = 0, cin = 0, cout = 0;
  int64_t dw = 0, pw = 0;  // param offsets
  BnRef bn;                // BN behind the pointwise convolution
};
// scratch of one backward pass: transposed pointwise kernel, gradient wrt the depthwise output, weight-gradient GEMM
// workspace, depthwise-backward partial rows, the producer's BatchNorm backward coefficients
struct SepBwdScratch {
  float *WT, *DZ, *tn, *part, *coef;
};
// z = dwk(in) - in read through the table bn_in (BN + ReLU6 on load) or, bn_in NULL, as it is - then y = z W with the BN
// partial sums in stats (NULL: none).  Returns the number of statistics rows, or a negative KWS_E_* code.
int kws_sep_fwd(const SepBlock& b, const float* params, const float* in, const float* bn_in, float* z, float* y, float* stats, int B,
                hipStream_t st);
// the block's table bn [4][cout]: from `rows` statistics rows over M rows (training: moving averages updated) or from the
// moving statistics
int kws_sep_bn_table(const SepBlock& b, const float* params, float* state, const float* stats, int rows, int64_t M, bool training,
                     float* bn, float* red, hipStream_t st);
// dz (s.DZ) -> the depthwise kernel's gradient and out = the gradient wrt the block's input.  prod != NULL: the input is
// the producer's raw output read through bn_in; the producer's BatchNorm backward rides along (its dgamma / dbeta, out
// becomes its dy).  prod NULL: out stays the gradient wrt the input as read.
int kws_sep_dw_bwd(const SepBlock& b, const float* params, float* grads, const float* in, const float* bn_in, const BnRef* prod,
                   float* out, const SepBwdScratch& s, int B, hipStream_t st);
// dy [B * Lout, cout] -> the pointwise kernel's gradient (z: the block's depthwise output), dz, then kws_sep_dw_bwd
int kws_sep_bwd(const SepBlock& b, const float* params, float* grads, const float* dy, const float* z, const float* in,
                const float* bn_in, const BnRef* prod, float* out, const SepBwdScratch& s, int B, hipStream_t st);

// ---- the 3-tap depthwise ladder of net.hip and net_time_sliced.hip (net_dw3ladder.hip) -----------------------------------
// A first convolution's raw output y[0] [B, L1, C1] with its BatchNorm bn1, then blocks of
//   z[i] = dw3_i( relu6(bn_i(y[i])) )      BN + ReLU6 of the producer applied on load, never materialised
//   y[i + 1] = z[i] W_i                    f32 MFMA GEMM, the statistics of bn_{i+1} in its epilogue
// The programs keep their first convolution, their head, their other buffers and the order of their workspace.
struct Dw3Block {   // depthwise k 3 -> pointwise -> BN -> relu6
  int stride, pad_l, cin, cout, Lin, Lout;
  int64_t dw, pw;  // param offsets
  BnRef bn;        // BN behind the pointwise convolution
};
struct Dw3Sizes {   // over y[0] and the blocks at one batch size, in floats
  int64_t max_y = 0, max_z = 0;
  int64_t max_part = 0;    // statistics rows of the pointwise GEMMs
  int64_t max_dwpart = 0;  // partial rows of depthwise-backward pass 1
  int maxC = 0;
};
struct Dw3Offsets {   // float offsets into the workspace
  std::vector<int64_t> y, z;  // y[0] = first convolution, y[i + 1] / z[i] = pointwise / depthwise output of block i
  std::vector<int64_t> WT;    // transposed pointwise kernel of block i (input-gradient GEMM operand)
  int64_t bn = 0, bn_stride = 0;  // table l (scale|shift|mean|rstd of the BN behind y[l]) at bn + l * bn_stride
};
struct Dw3Run {   // one call's buffers
  const Dw3Offsets* o;
  const float* params;
  float* state;   // training: moving statistics are updated
  float* grads;   // backward only
  float* ws;
  int B;
  float *red, *part, *coef, *DZ;   // reduce scratch; backward: pass-1 partial rows, the producer's coefficients, gradient wrt z[i]
  hipStream_t st;
  float* y(int l) const { return ws + o->y[l]; }
  float* z(int i) const { return ws + o->z[i]; }
  float* WT(int i) const { return ws + o->WT[i]; }
  float* bn_at(int l) const { return ws + o->bn + o->bn_stride * l; }
};
struct Dw3Ladder {
  int L1 = 0, C1 = 0;   // set, with bn1, before build()
  BnRef bn1;
  std::vector<Dw3Block> blocks;
  int nb() const { return (int)blocks.size(); }
  // spec[i] = {stride, filters}: stride 2 is a SAME block (_reduce_conv), stride 1 a VALID one (_context_conv); creates the layers
  int build(KerasNames& kn, const int (*spec)[2], int n, int fm, int input_size);
  Dw3Sizes sizes(int B) const;
  // workspace pieces, each taken where the program's own order has it.  Activations: one y / z per block in training, two
  // y buffers and one z buffer (ping-pong) in inference
  void take_acts(Bump& bp, int B, bool training, const Dw3Sizes& s, Dw3Offsets* o) const;
  void take_bn(Bump& bp, int maxC, Dw3Offsets* o) const;   // nb + 1 tables, each wide enough for maxC channels
  void take_WT(Bump& bp, Dw3Offsets* o) const;
  // what = 0: y[index], 1: z[index], 2: BatchNorm table index
  int debug_view(const Dw3Offsets& o, int B, int what, int index, int64_t* offset_floats, int64_t* count) const;
  int infer_tables(const Dw3Run& r) const;    // the nb + 1 inference tables from the moving statistics, one launch
  int transpose_all(const Dw3Run& r) const;   // every pointwise kernel [cin][cout] -> WT [cout][cin], one launch
  // the steps of block i.  amax (may be NULL): a slot group that receives the |x| maximum of the tensor the step writes
  int fwd_dw(int i, const Dw3Run& r, unsigned* amax) const;                       // y[i] -> z[i]
  int stats_finalize(int i, const Dw3Run& r, const float* stats, int rows) const;   // statistics rows of y[i + 1] -> table i + 1
  int fwd_block_f32(int i, const Dw3Run& r, float* stats, unsigned* amax) const;  // both around the f32 GEMM; stats NULL: no table
  // r.DZ = gradient wrt z[i] -> the depthwise kernel's gradient, the producing BN's dgamma / dbeta, and dy = gradient wrt y[i]
  int bwd_block_input(int i, const Dw3Run& r, float* dy, unsigned* amax) const;
};

// ---- residual-block / log-mfcc tail launchers (resblock.hip) ------------------------------------------
// o = maxpool_P(relu6(bn(y))) + (res_bn ? res_bn.scale*res + res_bn.shift : res)
int kws_block_out_fwd(const float* y, const float* bn, const float* res, const float* res_bn, float* o, int B,
                      int L, int C, int pool, hipStream_t st);
// resblock.hip (round 6): that join and the NEXT block's first depthwise convolution (k 3, stride 1, pad (1, 1); kernel w [3, C]) in one pass
int kws_block_out_dw_fwd(const float* y, const float* bn, const float* res, const float* res_bn, const float* w, float* o, float* z, int B,
                         int L, int C, int pool, hipStream_t st);
// g[b,u,c] = [u wins its pool window] * dO[b,u/P,c] * (relu ? relu6'(bn(y)) : 1); part = [blocks][5][C] sums of
// (g, g*xhat, 0, 0, 0)
// two-pass join backward + BatchNorm backward (resblock.hip block_join_bwd_kernel): pass 1 leaves kws_block_join_bwd_parts()
// partial rows [5][C] (<= 256 per launch: no slice fold in front of kws_dw_bwd_finalize), pass 2 writes dy directly
int kws_block_join_bwd_parts(int B, int L, int C, int pool);
int kws_block_join_bwd(const float* dO, const float* y, const float* bn, const float* gamma, const float* coef, float* out,
                       float* part, int pass, int B, int L, int C, int pool, int relu, hipStream_t st);
int64_t kws_block_out_bwd_part_floats(int B, int L, int C, int pool);
int kws_block_out_bwd(const float* dO, const float* y, const float* bn, float* g, float* part, int B, int L, int C,
                      int pool, int relu, hipStream_t st);
int kws_block_out3_fwd(const float* y, const float* bn, const float* res, const float* res_bn, float* o, int B, int L,
                       int Lo, int C, int stride, int pad_l, hipStream_t st);
int64_t kws_block_out3_bwd_part_floats(int B, int L, int C);
int kws_block_out3_bwd(const float* dO, const float* y, const float* bn, float* g, float* part, int B, int L, int Lo,
                       int C, int stride, int pad_l, hipStream_t st);
int kws_add_f32(const float* a, const float* b, float* out, int64_t n, hipStream_t st);
// out[b, stride*t, :] += in[b, t, :]
int kws_add_strided_f32(float* out, const float* in, int B, int L_out, int L_in, int C, int stride, hipStream_t st);

struct kws_lm_tail_args {
  const float* x;       // [B, T, C] block-stack output
  const float* wa;      // [3, C] attention depthwise kernel
  const float* Wa;      // [C]    attention pointwise kernel (C -> 1)
  const float* bn_gamma; const float* bn_beta; float* mm; float* mv;   // attention BN (1 channel)
  const float* Wd;      // [C, NC]
  const float* bd;      // [NC]
  const float* labels;  // [B, NC]
  float* probs;         // [B, NC]
  float* u;             // [B, T] attention logits (pre-BN)
  float* bn;            // [4] scale|shift|mean|rstd of the attention BN
  float* dX;            // [B, T, C] gradient wrt x (train)
  float* fd;            // [B, C] dropped features
  float* dl;            // [B, NC]
  float* gu;            // [B, T] masked gradient wrt the attention BN output
  float* part;          // [B][5][C] per-clip partials (dWa | 0 | dwa taps)
  float* coef;          // [2]
  float* d_gamma; float* d_beta;   // grads of the attention BN
  float* per_loss; float* per_correct; float* att;
  int B, T, C, NC; uint64_t seed; uint32_t step; float keep_prob; int loss_batch; int64_t row_offset;
};
// Global-pooling tails; training also writes dX, the dropped features and dlogits (for the dense wgrad).
//   steffeNet (model.py:1712-1718, 1722-1724): GlobalMaxPooling1D ++ GlobalAveragePooling1D -> Dropout -> Dense(no
//     bias) + softmax -> label-smoothed CE: pool_max = 1, bd = NULL, loss_kind = 0
//   conv_1d_residual (model.py:898-905): GlobalAveragePooling1D -> Dropout -> Dense + softmax -> keras
//     categorical_crossentropy: pool_max = 0, loss_kind = 1
struct kws_gp_tail_args {
  const float* x;       // [B, T, C] block-stack output
  const float* Wd;      // [F, NC], F = 2C (max ++ avg) or C (avg)
  const float* bd;      // [NC] or NULL
  int pool_max, loss_kind;
  const float* labels;  // [B, NC]
  float* probs;         // [B, NC]
  float* dX;            // [B, T, C]
  float* fd;            // [B, F]
  float* dl;            // [B, NC]
  float* per_loss;
  float* per_correct;
  int B, T, C, NC;
  uint64_t seed; uint32_t step; float keep_prob; float label_smoothing; int loss_batch; int64_t row_offset;
};
int kws_gp_tail_launch(const kws_gp_tail_args* a, int training, hipStream_t st);
int kws_lm_tail_fwd(const kws_lm_tail_args* a, int training, hipStream_t st);   // logits -> BN stats -> probs (+ tail backward when training)
int kws_lm_tail_bwd(const kws_lm_tail_args* a, hipStream_t st);                 // attention BN backward + dX accumulation + per-clip partials
