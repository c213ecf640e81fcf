// Network programs of the two grouped-Conv1D models:
//   KWS_NET_CONV_1D_FAST  conv_1d_fast_model (reference model.py:642-713): raw waveform -> Conv1D(252, 479, strides=160, VALID,
//                         no bias, l2 1e-4) with no BN and no activation -> grouped reduce blocks (300, k15, g6 on 252 channels),
//                         (360, k7, g5 on 300) -> Flatten -> Dropout(.3) -> Dense + softmax; RMSprop(3e-3), categorical CE
//   KWS_NET_CONV_1D_SPEC  conv_1d_spec_model (model.py:1249-1323): the 'spec' output [98, 257] -> four reduce / context pairs,
//                         k 3, reduce g 4 stride 2, context g 3 -> Flatten -> Dropout(.3) -> Dense + softmax; RMSprop(2e-3)
// A grouped block is g Keras Conv1D layers over the slices x[:, :, q*gs : (q+1)*gs] (gs from the block's num_channels
// argument: channels past g*gs are never read), each followed by its own BatchNormalization and relu6, concatenated.
// On the device a block is one kws_gconv_fwd_f32 launch (BN partial sums in its epilogue) and one grouped BN finalise; the
// normalise + ReLU6 is applied on load by the next block (or the tail), the project's convention.  The 479-tap front
// convolution is the gathered GEMM on ONE tap of 480 samples against a kernel padded with a zero row (as steffeNet pads 75
// to 76).
// The same program runs the reference's plain dense-Conv1D ladders, a block with ONE group and, on every second layer, a
// MaxPool1D(3, strides=2, 'valid') behind the activation (kws_pool3s2_*: the pooled tensor is materialised ACTIVATED, the next
// block reads it without a table):
//   KWS_NET_CONV_1D_TIME_STACKED  conv_1d_time_stacked_model (model.py:257-309): raw waveform as [800, 20] -> Conv1D(32, 1) ->
//                         six reduce (k 3, pooled) / context (k 3) pairs of 48 ... 256 filters, l2 1e-5 -> Dropout(.3) ->
//                         Conv1D(num_classes, 5, softmax, bias) over the 5 remaining steps = the flat tail with D = 1280; Adam(3e-4)
//   KWS_NET_CONV_1D_HEAVY conv_1d_heavy_model (model.py:409-467): [1600, 10], seven pairs up to 320 filters -> Dropout(.3) ->
//                         Conv1D(128, 5, no bias) -> BatchNormalization (over the B rows) + relu6 -> Dropout(.1) ->
//                         Conv1D(num_classes, 1, softmax, no bias).  The 1600 -> 128 product is one more block of this program
//                         whose input is the materialised dropped features; what follows it is the flat tail with D = 128,
//                         dropout layer 2 and no bias.
// And the filterbank sibling of conv_1d_fast / conv_1d_spec:
//   KWS_NET_CONV_1D_LEARNED_SPEC  conv_1d_learned_spec_model (model.py:1159-1246): raw waveform -> six Conv1D(40, k, strides=160,
//                         SAME, no bias, l2 1e-4), k = 479 ... 161, concatenated to [ceil(L / 160), 240] with no BN and no activation
//                         (ONE kws_fbank_conv_fwd_f32 launch) -> four reduce (g 3, stride 2) / context (g 2) pairs, k 3 ->
//                         Flatten -> Dropout(.3) -> Dense + softmax; RMSprop(2e-3).  Its second block slices 360 channels of a
//                         300-channel tensor in two, so its groups read 180 and 120 channels (Keras clips the slice): a RAGGED
//                         block, run as two kws_conv1d_* column-window convolutions over the producer's table repacked from the
//                         grouped layout [g][4][Ng] to the flat [4][C] one those kernels index.
//   KWS_NET_CONV_1D_TOP_DOWN  conv_1d_top_down_model (model.py:1326-1397): raw waveform -> Conv1D(480, 479, strides=160, VALID, WITH
//                         bias; no BN, no activation) -> four reduce (g 3, stride 2) / context (g 2) pairs whose groups are
//                         depthwise-separable blocks (DepthwiseConv2D((1, 3)) -> Conv1D(F / g, 1) -> BatchNormalization -> relu6, l2
//                         1e-5) -> Flatten -> Dropout(.05) -> Dense + softmax; RMSprop(3e-3).  A SEPARABLE block of this program: a
//                         block is one kws_gdwconv_fwd_f32 launch for all groups' depthwise halves (the front bias or the producer's
//                         table applied on load; the context groups all read the whole input), one kws_gconv_fwd_f32 with k = 1 over
//                         its output and the grouped BN finalise.  The front bias is a per-channel constant in front of block 1's
//                         BatchNormalization on batch statistics (depthwise and 1x1 keep it one), so it cancels in a training step:
//                         its gradient is written as exact 0, as the Conv2D program does for its biases in front of a BatchNorm.
// So a block has one of four forms - plain, pooled, ragged, separable - and everything around the blocks (the two 479-tap fronts,
// the banked front, the tables, the gradient ping-pong, the flat tail through FlatTailProgram) is written once.
#include "net_internal.h"

namespace {

struct GcBlock {
  kws_gconv_t d;            // B filled in per call
  int F;
  int64_t w0;               // group 0's kernel (params); group q's at + q * pstride
  int64_t gamma0, beta_off; // group 0's gamma (params); beta at gamma + beta_off
  int64_t mm0, mv_off;      // group 0's moving mean (state); variance at mm + mv_off
  int64_t pstride, sstride;
  int bn_idx0;              // 0-based Keras index of group 0's BatchNormalization
  bool pool;                // MaxPool1D(3, strides=2, 'valid') behind the activation: Lp rows per clip leave the block
  int Lp;
  bool ragged;              // two groups of different input widths: rc[q] (B filled in per call), group q's kernel at rw[q]
  kws_conv1d_t rc[2];
  int64_t rw[2];
  bool sep;                 // a depthwise half (k 3) in front: d is the k = 1 pointwise descriptor over its output [B, Lout, g * gs]
  bool dw_shared;           // its groups all read the whole input (_grouped_context_conv), else group q the slice [q * gs, + gs)
  kws_gdwconv_t dw;         // B, act and bn_group filled in per call
  int64_t dw0;              // group 0's depthwise kernel (params); group q's at + q * pstride
};

struct GcLayout {
  int64_t total = 0;
  int64_t w0p = 0, y0 = 0;
  std::vector<int64_t> y, bn, z, dwo;   // z: the pooled activated output of a pooled block; dwo: a separable block's depthwise output
  int64_t fa = 0, fd1 = 0;         // head2: activated / dropped features [B, Dd]
  int64_t stats = 0, dA[2] = {0, 0}, part = 0, coef = 0, wws = 0, dwws = 0, tnws = 0, dw0p = 0;
  FlatTailWs tail;
  int64_t bnflat = 0, fbws = 0;    // a ragged block's input table as [4][C]; the banked front's weight-gradient workspace
  int64_t rstats = 0;              // distance of the two groups' statistics rows of a ragged block
};

struct GcProgram : FlatTailProgram<GcLayout> {
  bool front = false;       // conv_1d_fast, conv_1d_top_down: the 479-tap front convolution
  int L_in = 0, C_in = 0;   // the input seen as [L_in, C_in]
  int64_t conv0 = 0, bias0 = -1;   // its kernel; conv_1d_top_down: its bias, applied on load by block 1
  int K0 = 0, K0p = 0, L0 = 0, C0 = 0;
  kws_gather_t g0{};
  bool fbank = false;       // conv_1d_learned_spec: the six-bank front convolution (w_off: the kernels' offsets in params / grads)
  kws_fbank_conv_t fb{};
  bool has_front() const { return front || fbank; }
  std::vector<GcBlock> blocks;
  float keep = 0.7f;
  bool head2 = false;       // conv_1d_heavy: the last block is the Conv1D(128, 5) head over the dropped features [B, Dd]
  int Dd = 0;
  float keep2 = 1.f;        // Dropout(0.1) between that block and the softmax convolution (dropout layer 2)

  void layout(int B, bool training, GcLayout* lo) const override;
  int forward(const GcLayout& lo, const NetCall& c) const override;
  kws_flat_tail_args tail_args(const GcLayout& lo, const NetCall& c, float* probs) const override;
  int64_t tail_grad(const GcLayout& lo) const override { return lo.dA[0]; }
  int backward(const GcLayout& lo, const NetCall& c) const override;
  int debug_view(int B, int training, int what, int index, int64_t* offset_floats, int64_t* count) const override;
};

constexpr float GC_DROP_KEEP = 0.7f;      // Dropout(0.3), model.py:710 / 1318
constexpr float GC_FRONT_L2 = 1e-4f;      // kernel_regularizer=l2(0.0001), model.py:700
constexpr float GC_HEAD2_KEEP = 0.9f;     // Dropout(0.1), model.py:458
constexpr float GC_TOP_DOWN_KEEP = 0.95f; // Dropout(0.05), model.py:1389

enum GcDw { GC_NO_DW, GC_DW_SLICED, GC_DW_SHARED };

// A grouped block of F filters and k taps over g slices of num_channels / g channels.  dw: the groups are depthwise-separable
// (DepthwiseConv2D((1, k)) -> Conv1D(F / g, 1)), group q reading its slice (_grouped_reduce_conv) or, shared, all C channels
// (_grouped_context_conv); the layers of a group in the reference's order: [depthwise,] convolution, BatchNorm
int add_block(KerasNames& kn, GcProgram* p, int L, int C, int F, int k, int g, int num_channels, int stride, float l2 = 0.f,
              bool pool = false, GcDw dw = GC_NO_DW) {
  KWS_REQUIRE(num_channels % g == 0 && F % g == 0 && num_channels <= C, "net: grouped block F=%d g=%d num_channels=%d C=%d", F, g,
              num_channels, C);
  KWS_REQUIRE(L >= k, "net: grouped block input length %d < %d taps", L, k);
  GcBlock b;
  memset(&b, 0, sizeof(b));
  const int gs = dw == GC_DW_SHARED ? C : num_channels / g, Ng = F / g, Lout = (L - k) / stride + 1;
  b.sep = dw != GC_NO_DW;
  b.dw_shared = dw == GC_DW_SHARED;
  if (b.sep) {
    b.dw.L = L; b.dw.C = C; b.dw.k = k; b.dw.stride = stride; b.dw.g = g; b.dw.gs = gs; b.dw.Lout = Lout;
    b.dw.x0 = 0; b.dw.x_step = b.dw_shared ? 0 : gs;
    b.d.L = Lout; b.d.C = g * gs; b.d.k = 1; b.d.stride = 1;
  } else {
    b.d.L = L; b.d.C = C; b.d.k = k; b.d.stride = stride;
  }
  b.d.Lout = Lout; b.d.g = g; b.d.gs = gs; b.d.Ng = Ng;
  b.F = F;
  b.pool = pool;
  KWS_REQUIRE(!pool || (g == 1 && !b.sep && Lout >= 3), "net: pooled block needs one group and >= 3 rows (g=%d Lout=%d)", g, Lout);
  b.Lp = pool ? kws_pool3s2_out_len(Lout) : Lout;
  b.bn_idx0 = kn.n_bn;
  int64_t prev_first = 0, prev_m = 0;
  for (int q = 0; q < g; ++q) {
    const int64_t dwk = b.sep ? kn.dwk(k, gs) : -1;
    const int64_t w = kn.conv(b.d.k, gs, Ng, l2);
    const BnRef r = kn.bn(Ng);
    const int64_t first = b.sep ? dwk : w;   // the group's first tensor
    if (q == 0) {
      b.dw0 = first; b.w0 = w; b.gamma0 = r.gamma; b.beta_off = r.beta - r.gamma; b.mm0 = r.mm; b.mv_off = r.mv - r.mm;
    } else {
      // every group has the same tensors in the same order: one stride per buffer
      if (q == 1) {
        b.pstride = first - prev_first;
        b.sstride = r.mm - prev_m;
      }
      KWS_REQUIRE(first - prev_first == b.pstride && r.mm - prev_m == b.sstride && w - first == b.w0 - b.dw0 &&
                      r.gamma - w == b.gamma0 - b.w0,
                  "net: grouped block layout is not uniform");
    }
    prev_first = first;
    prev_m = r.mm;
  }
  if (g == 1) {
    b.pstride = b.sep ? 0 : (int64_t)k * gs * Ng;
    b.sstride = 0;
  }
  b.d.w_group_stride = b.pstride;
  b.dw.w_group_stride = b.pstride;
  p->blocks.push_back(b);
  return KWS_OK;
}

// Conv1D(C0, 479, strides=160, VALID) over the raw waveform, no BN and no activation behind it, as the gathered GEMM on ONE tap
// of 480 samples (the 480th weight is a zero row): window t starts at 160 t and ends at 160 t + 479 < input_size
void add_front(KerasNames& kn, GcProgram* p, int input_size, int C0, float l2, bool bias) {
  p->front = true;
  p->K0 = 479; p->K0p = 480; p->C0 = C0;
  p->L0 = (input_size - p->K0) / 160 + 1;
  p->conv0 = kn.conv(p->K0, 1, C0, l2);
  if (bias) p->bias0 = kws_net_add_tensor(kn.n, "conv1d_1/bias", {C0}, false, 0.f, 0, 0, 0.f);
  p->g0.L_out = p->L0; p->g0.cin = p->K0p; p->g0.taps = 1; p->g0.stride_t = 160; p->g0.stride_j = 0; p->g0.base_off = 0;
  p->g0.x_len = input_size; p->g0.x_batch_stride = input_size;
  p->L_in = input_size; p->C_in = 1;
}

// _grouped_context_conv(x, F, k, 2, num_channels) with num_channels > C: Keras clips the second slice, so group 0 reads
// num_channels / 2 channels and group 1 the C - num_channels / 2 that are left
int add_ragged_block(KerasNames& kn, GcProgram* p, int L, int C, int F, int k, int num_channels) {
  const int gs = num_channels / 2, Ng = F / 2;
  KWS_REQUIRE(num_channels % 2 == 0 && F % 2 == 0 && gs < C && C < num_channels && L >= k,
              "net: ragged block F=%d num_channels=%d C=%d L=%d", F, num_channels, C, L);
  GcBlock b;
  memset(&b, 0, sizeof(b));
  b.d.L = L; b.d.C = C; b.d.k = k; b.d.stride = 1; b.d.g = 2; b.d.gs = gs; b.d.Ng = Ng;
  b.d.Lout = L - k + 1;
  b.F = F;
  b.Lp = b.d.Lout;
  b.ragged = true;
  b.bn_idx0 = kn.n_bn;
  for (int q = 0; q < 2; ++q) {
    const int cin = q == 0 ? gs : C - gs;
    b.rw[q] = kn.conv(k, cin, Ng, 0.f);
    const BnRef r = kn.bn(Ng);
    if (q == 0) {
      b.w0 = b.rw[0]; b.gamma0 = r.gamma; b.beta_off = r.beta - r.gamma; b.mm0 = r.mm; b.mv_off = r.mv - r.mm;
    } else {
      b.pstride = r.gamma - b.gamma0;
      b.sstride = r.mm - b.mm0;
      KWS_REQUIRE(r.beta - r.gamma == b.beta_off && r.mv - r.mm == b.mv_off, "net: ragged block layout is not uniform");
    }
    kws_conv1d_t& c = b.rc[q];
    c.L = L; c.Lout = b.d.Lout; c.k = k; c.dil = 1; c.pad_l = 0;
    c.Cx = C; c.x0 = q * gs; c.Cin = cin;
    c.Cy = F; c.y0 = q * Ng; c.F = Ng;
  }
  b.d.w_group_stride = b.rw[1] - b.rw[0];
  p->blocks.push_back(b);
  return KWS_OK;
}

void GcProgram::layout(int B, bool training, GcLayout* lo) const {
  const GcProgram& p = *this;
  Bump bp;
  const int nb = (int)p.blocks.size();
  int64_t max_act = 64, max_stats = 64, max_part = 64, max_coef = 64, max_wws = 64, max_dwws = 0;
  if (p.front) {
    lo->w0p = bp.take((int64_t)p.K0p * p.C0);
    lo->y0 = bp.take((int64_t)B * p.L0 * p.C0);
    max_act = std::max(max_act, (int64_t)B * p.L0 * p.C0);
  }
  if (p.fbank) {
    lo->y0 = bp.take((int64_t)B * p.L0 * p.C0);
    max_act = std::max(max_act, (int64_t)B * p.L0 * p.C0);
  }
  lo->y.assign(nb, 0);
  lo->bn.assign(nb, 0);
  lo->z.assign(nb, 0);
  lo->dwo.assign(nb, 0);
  for (int i = 0; i < nb; ++i) {
    kws_gconv_t d = p.blocks[i].d;
    d.B = B;
    const int64_t M = (int64_t)B * d.Lout;
    if (p.blocks[i].sep) {
      kws_gdwconv_t dw = p.blocks[i].dw;
      dw.B = B;
      lo->dwo[i] = bp.take(M * d.C);
      max_act = std::max(max_act, (int64_t)B * dw.L * dw.C);
      max_dwws = std::max(std::max(max_dwws, (int64_t)64), kws_gdwconv_bwd_workspace_floats(&dw));
    }
    lo->y[i] = bp.take(M * p.blocks[i].F);
    lo->bn[i] = bp.take((int64_t)4 * p.blocks[i].F);
    if (p.blocks[i].pool) {
      lo->z[i] = bp.take((int64_t)B * p.blocks[i].Lp * p.blocks[i].F);
      max_part = std::max(max_part, kws_pool3s2_bwd_part_floats(B, d.Lout, p.blocks[i].F));
    }
    max_act = std::max(max_act, std::max(M * p.blocks[i].F, (int64_t)B * d.L * d.C));
    max_part = std::max(max_part, (int64_t)kws_gbn_bwd_rows(M) * 2 * p.blocks[i].F);
    max_coef = std::max(max_coef, (int64_t)2 * p.blocks[i].F);
    if (p.blocks[i].ragged) {
      lo->bnflat = bp.take((int64_t)4 * d.C);
      for (int q = 0; q < 2; ++q) {
        kws_conv1d_t c = p.blocks[i].rc[q];
        c.B = B;
        lo->rstats = std::max(lo->rstats, ((int64_t)kws_conv1d_stats_rows(&c) * 2 * c.F + 63) / 64 * 64);
        max_wws = std::max(max_wws, kws_conv1d_wgrad_workspace_floats(&c));
      }
      max_stats = std::max(max_stats, 2 * lo->rstats);
      continue;
    }
    max_stats = std::max(max_stats, (int64_t)kws_gconv_stats_rows(&d) * 2 * p.blocks[i].F);
    max_wws = std::max(max_wws, kws_gconv_wgrad_workspace_floats(&d));
  }
  lo->stats = bp.take(max_stats);
  if (training) {
    if (p.head2) {
      lo->fa = bp.take((int64_t)B * p.Dd);
      lo->fd1 = bp.take((int64_t)B * p.Dd);
    }
    lo->dA[0] = bp.take(max_act);
    lo->dA[1] = bp.take(max_act);
    lo->part = bp.take(max_part);
    lo->coef = bp.take(max_coef);
    lo->wws = bp.take(max_wws);
    if (max_dwws) lo->dwws = bp.take(max_dwws);
    if (p.front) {
      lo->tnws = bp.take(kws_gemm_tn_workspace_floats((int64_t)B * p.L0, p.K0p, p.C0));
      lo->dw0p = bp.take((int64_t)p.K0p * p.C0);
    }
    if (p.fbank) {
      kws_fbank_conv_t fb = p.fb;
      fb.B = B;
      lo->fbws = bp.take(kws_fbank_conv_wgrad_workspace_floats(&fb));
    }
    lo->tail.take(bp, B, dense.D, dense.NC);
  }
  lo->total = bp.cur * 4;
}

kws_gbn_refs refs_of(const GcBlock& b, const float* params, float* state) {
  kws_gbn_refs r;
  r.gamma = params + b.gamma0; r.pstride = b.pstride; r.boff = b.beta_off;
  r.mm = state ? state + b.mm0 : nullptr; r.sstride = b.sstride; r.voff = b.mv_off;
  return r;
}

// what block i convolves: the raw output of the block before it with that block's table (applied on load), its pooled
// activated output without one, the network input, or (head2's last block, training) the dropped features
struct GcInput {
  const float* in;
  const float* bn;
  int bg;
};
GcInput gc_input(const GcProgram& p, const GcLayout& lo, int i, const NetCall& c) {
  const float* ws = c.ws;
  if (i == 0) return {p.has_front() ? ws + lo.y0 : c.x, nullptr, 0};
  if (p.head2 && c.training && i + 1 == (int)p.blocks.size()) return {ws + lo.fd1, nullptr, 0};
  if (p.blocks[i - 1].pool) return {ws + lo.z[i - 1], nullptr, 0};
  return {ws + lo.y[i - 1], ws + lo.bn[i - 1], p.blocks[i - 1].d.Ng};
}

// the depthwise half of separable block i over that input: its descriptor with what it applies on load - the producer's table,
// or (block 1 behind a front with a bias) that bias - and the table
struct GcDwInput {
  kws_gdwconv_t d;
  const float* tab;
};
GcDwInput gc_dw_input(const GcProgram& p, int i, const GcInput& gi, const NetCall& c) {
  GcDwInput r{p.blocks[i].dw, gi.bn};
  r.d.B = c.B;
  if (gi.bn) {
    r.d.act = KWS_GDW_ACT_BN_RELU6;
    r.d.bn_group = gi.bg;
  } else if (i == 0 && p.bias0 >= 0) {
    r.d.act = KWS_GDW_ACT_BIAS;
    r.tab = c.params + p.bias0;
  }
  return r;
}

// the producer's grouped table [g][4][Ng] as the flat [4][C] one of kws_conv1d_* (C = g * Ng)
int gc_flat_table(const float* bn, int g, int Ng, float* flat, hipStream_t st) {
  for (int q = 0; q < g; ++q)
    KWS_HIP(hipMemcpy2DAsync(flat + (int64_t)q * Ng, sizeof(float) * g * Ng, bn + (int64_t)q * 4 * Ng, sizeof(float) * Ng,
                             sizeof(float) * Ng, 4, hipMemcpyDeviceToDevice, st));
  return KWS_OK;
}

kws_gbn_refs ragged_refs(const GcBlock& b, int q, const float* params, float* state) {
  kws_gbn_refs r;
  r.gamma = params + b.gamma0 + q * b.pstride; r.pstride = 0; r.boff = b.beta_off;
  r.mm = state ? state + b.mm0 + q * b.sstride : nullptr; r.sstride = 0; r.voff = b.mv_off;
  return r;
}

// a ragged block (i >= 1, behind an unpooled grouped block): two column-window convolutions, each with its own BatchNorm layer,
// whose tables land in the grouped layout [2][4][Ng] the next block reads
int gc_ragged_forward(const GcProgram& p, const GcLayout& lo, int i, const NetCall& c) {
  const float* params = c.params;
  float* state = c.state;
  float* ws = c.ws;
  const int B = c.B;
  const bool training = c.training;
  hipStream_t st = c.st;
  const GcBlock& b = p.blocks[i];
  const GcBlock& pb = p.blocks[i - 1];
  KWS_TRY(gc_flat_table(ws + lo.bn[i - 1], pb.d.g, pb.d.Ng, ws + lo.bnflat, st));
  const kws_gbn_cols cols = kws_gbn_grouped(1, b.d.Ng);
  for (int q = 0; q < 2; ++q) {
    kws_conv1d_t cv = b.rc[q];
    cv.B = B;
    float* stats = training ? ws + lo.stats + q * lo.rstats : nullptr;
    KWS_TRY(kws_conv1d_fwd_f32(ws + lo.y[i - 1], ws + lo.bnflat, params + b.rw[q], ws + lo.y[i], stats, &cv, st));
    const kws_gbn_refs r = ragged_refs(b, q, params, state);
    float* bn = ws + lo.bn[i] + (int64_t)q * 4 * b.d.Ng;
    if (training)
      KWS_TRY(kws_gbn_finalize(stats, kws_conv1d_stats_rows(&cv), (int64_t)B * cv.Lout, &cols, &r, KWS_BN_EPS, KWS_BN_MOMENTUM, bn, st));
    else
      KWS_TRY(kws_gbn_infer(&cols, &r, KWS_BN_EPS, bn, st));
  }
  return KWS_OK;
}

// forward through the blocks; training: batch statistics (moving averages updated), else the moving statistics
int GcProgram::forward(const GcLayout& lo, const NetCall& c) const {
  const GcProgram& p = *this;
  const float* params = c.params;
  float* state = c.state;
  const float* x = c.x;
  float* ws = c.ws;
  const int B = c.B;
  const bool training = c.training;
  hipStream_t st = c.st;
  if (p.front) {
    KWS_HIP(hipMemcpyAsync(ws + lo.w0p, params + p.conv0, sizeof(float) * p.K0 * p.C0, hipMemcpyDeviceToDevice, st));
    KWS_HIP(hipMemsetAsync(ws + lo.w0p + (int64_t)p.K0 * p.C0, 0, sizeof(float) * (p.K0p - p.K0) * p.C0, st));
    KWS_TRY(kws_gemm_gather_f32(x, &p.g0, ws + lo.w0p, ws + lo.y0, B, p.C0, nullptr, st));
  }
  if (p.fbank) {
    kws_fbank_conv_t fb = p.fb;
    fb.B = B;
    KWS_TRY(kws_fbank_conv_fwd_f32(x, params, ws + lo.y0, &fb, st));
  }
  for (size_t i = 0; i < p.blocks.size(); ++i) {
    const GcBlock& b = p.blocks[i];
    kws_gconv_t d = b.d;
    d.B = B;
    GcInput gi = gc_input(p, lo, (int)i, c);
    const kws_gbn_refs r = refs_of(b, params, state);
    const kws_gbn_cols cols = kws_gbn_grouped(d.g, d.Ng);
    if (b.ragged) {
      KWS_TRY(gc_ragged_forward(p, lo, (int)i, c));
      continue;
    }
    if (b.sep) {   // all groups' depthwise halves in one launch; the k = 1 convolution reads their output as it is
      const GcDwInput di = gc_dw_input(p, (int)i, gi, c);
      KWS_TRY(kws_gdwconv_fwd_f32(gi.in, di.tab, params + b.dw0, ws + lo.dwo[i], &di.d, st));
      gi = {ws + lo.dwo[i], nullptr, 0};
    }
    if (training) {
      if (p.head2 && i + 1 == p.blocks.size()) {   // Dropout(.3) over the activated ladder output, materialised for the head's GEMMs
        const GcBlock& pb = p.blocks[i - 1];
        KWS_TRY(kws_bn_relu6_apply(ws + lo.y[i - 1], ws + lo.bn[i - 1], ws + lo.fa, (int64_t)B * pb.d.Lout, pb.F, 1, st));
        KWS_TRY(kws_dropout_fwd(ws + lo.fa, ws + lo.fd1, B, p.Dd, p.keep, c.seed, c.step, 1, c.row_offset, st));
      }
      KWS_TRY(kws_gconv_fwd_f32(gi.in, gi.bn, gi.bg, params + b.w0, ws + lo.y[i], ws + lo.stats, &d, st));
      KWS_TRY(kws_gbn_finalize(ws + lo.stats, kws_gconv_stats_rows(&d), (int64_t)B * d.Lout, &cols, &r, KWS_BN_EPS, KWS_BN_MOMENTUM,
                               ws + lo.bn[i], st));
    } else {
      KWS_TRY(kws_gconv_fwd_f32(gi.in, gi.bn, gi.bg, params + b.w0, ws + lo.y[i], nullptr, &d, st));
      KWS_TRY(kws_gbn_infer(&cols, &r, KWS_BN_EPS, ws + lo.bn[i], st));
    }
    if (b.pool) KWS_TRY(kws_pool3s2_fwd_f32(ws + lo.y[i], ws + lo.bn[i], ws + lo.z[i], B, d.Lout, b.F, st));
  }
  return KWS_OK;
}

kws_flat_tail_args GcProgram::tail_args(const GcLayout& lo, const NetCall& c, float* probs) const {
  const GcBlock& last = blocks.back();
  kws_flat_tail_args t;
  memset(&t, 0, sizeof(t));
  t.y = c.ws + lo.y.back(); t.bn = c.ws + lo.bn.back(); t.Ng = last.d.Ng;
  t.Wd = c.params + dense.kernel; t.bd = dense.bias >= 0 ? c.params + dense.bias : nullptr;
  t.probs = probs;
  t.B = c.B; t.D = dense.D; t.F = last.F; t.NC = dense.NC;
  t.keep_prob = head2 ? keep2 : keep;
  t.layer_id = head2 ? 2 : 1;
  return t;
}

}  // namespace

int gc_build(kws_net* n) {
  const kws_net_config_t& c = n->cfg;
  GcProgram* p = new GcProgram();
  n->program.reset(p);
  p->net = n;
  const int NC = p->dense.NC = c.num_classes;
  p->keep = GC_DROP_KEEP;
  KerasNames kn{n};
  // the ladder of conv_1d_spec, conv_1d_learned_spec and conv_1d_top_down: four reduce / context pairs, k 3, over [L, C]
  struct Row { int F, g, nch, stride; };
  const Row* spec = nullptr;
  int L = 0, C = 0;
  if (c.kind == KWS_NET_CONV_1D_FAST) {
    KWS_REQUIRE(c.input_size >= 479 && c.input_size % 2 == 0, "net: conv_1d_fast input_size %d (even, >= 479)", c.input_size);
    add_front(kn, p, c.input_size, 252, GC_FRONT_L2, false);
    KWS_TRY(add_block(kn, p, p->L0, p->C0, 300, 15, 6, 252, 2));
    const GcBlock& b1 = p->blocks.back();
    KWS_TRY(add_block(kn, p, b1.d.Lout, b1.F, 360, 7, 5, 300, 2));
  } else if (c.kind == KWS_NET_CONV_1D_TOP_DOWN) {
    // the ladder's lengths are 45, 43, 21, 19, 9, 7, 3, 1 at 91 rows, the fewest that leave one: 14879 samples.  The gathered GEMM
    // loads pairs of samples, so clips must start on even offsets (conv_1d_fast's rule): the first size it takes is 14880
    KWS_REQUIRE(c.input_size >= 14879 && c.input_size % 2 == 0,
                "net: conv_1d_top_down input_size %d (even, >= 14879: the ladder needs 91 rows of 160 samples)", c.input_size);
    p->keep = GC_TOP_DOWN_KEEP;
    add_front(kn, p, c.input_size, 480, 0.f, true);
    static const Row rows[8] = {{420, 3, 480, 2}, {420, 2, 420, 1}, {360, 3, 300, 2}, {360, 2, 360, 1},
                                {300, 3, 360, 2}, {300, 2, 300, 1}, {240, 3, 300, 2}, {240, 2, 240, 1}};
    spec = rows; L = p->L0; C = p->C0;
  } else if (c.kind == KWS_NET_CONV_1D_TIME_STACKED || c.kind == KWS_NET_CONV_1D_HEAVY) {
    const bool heavy = c.kind == KWS_NET_CONV_1D_HEAVY;
    KWS_REQUIRE(c.input_size == 16000, "net: conv_1d_%s input_size %d (the reference reshapes 16000 samples)",
                heavy ? "heavy" : "time_stacked", c.input_size);
    p->L_in = heavy ? 1600 : 800; p->C_in = heavy ? 10 : 20;   // Reshape([800, 20]) / Reshape([1600, 10])
    KWS_TRY(add_block(kn, p, p->L_in, p->C_in, 32, 1, 1, p->C_in, 1, KWS_L2_COEF));
    const int widths[7] = {48, 96, 128, 160, 192, 256, 320};
    for (int i = 0; i < (heavy ? 7 : 6); ++i)
      for (int half = 0; half < 2; ++half) {   // _reduce_conv (pooled; its strides argument goes to the pool only), _context_conv
        const GcBlock& pb = p->blocks.back();
        KWS_TRY(add_block(kn, p, pb.Lp, pb.F, widths[i], 3, 1, pb.F, 1, KWS_L2_COEF, half == 0));
      }
    const GcBlock& top = p->blocks.back();
    KWS_REQUIRE(top.d.Lout == 5, "net: ladder ends with %d rows, the head convolves 5", top.d.Lout);
    if (heavy) {
      p->head2 = true;
      p->Dd = top.d.Lout * top.F;
      p->keep2 = GC_HEAD2_KEEP;
      KWS_TRY(add_block(kn, p, top.d.Lout, top.F, 128, 5, 1, top.F, 1));
      const GcBlock& head = p->blocks.back();
      p->dense.D = head.F;
      p->dense.kernel = kn.conv(1, head.F, NC, 0.f);
    } else {
      p->dense.D = top.d.Lout * top.F;
      p->dense.kernel = kn.conv(top.d.Lout, top.F, NC, 0.f);   // [5, 256, NC] = the Dense kernel [1280, NC] over the t-major flatten
      p->dense.bias = kws_net_add_tensor(n, "conv1d_" + std::to_string(kn.n_conv) + "/bias", {NC}, false, 0.f, 0, 0, 0.f);
    }
    return KWS_OK;
  } else if (c.kind == KWS_NET_CONV_1D_LEARNED_SPEC) {
    const int ks[6] = {479, 383, 319, 255, 191, 161};
    kws_fbank_conv_t& fb = p->fb;
    fb.L = c.input_size; fb.stride = 160; fb.nbanks = 6; fb.N = 40;
    fb.Lout = (c.input_size + 159) / 160;
    // the ladder's lengths are 49, 47, 23, 21, 10, 8, 3, 1 at 100 rows: 91 rows are the fewest that leave one
    KWS_REQUIRE(c.input_size > 0 && c.input_size % 2 == 0 && fb.Lout >= 91,
                "net: conv_1d_learned_spec input_size %d (even, >= 14402: the ladder needs 91 rows of 160 samples)", c.input_size);
    for (int q = 0; q < 6; ++q) {
      int Lout = 0;
      fb.ksize[q] = ks[q];
      kws_same_pad(c.input_size, ks[q], 160, &Lout, &fb.pad_l[q]);
      fb.w_off[q] = kn.conv(ks[q], 1, fb.N, GC_FRONT_L2);
    }
    fb.x_batch_stride = c.input_size;
    fb.B = 1;
    KWS_REQUIRE(kws_fbank_conv_wgrad_workspace_floats(&fb) > 0, "net: input_size %d is outside the front convolution's domain",
                c.input_size);
    p->fbank = true;
    p->L_in = c.input_size; p->C_in = 1;
    p->L0 = fb.Lout; p->C0 = fb.nbanks * fb.N;
    static const Row rows[8] = {{300, 3, 240, 2}, {300, 2, 360, 1}, {360, 3, 300, 2}, {360, 2, 360, 1},
                                {420, 3, 240, 2}, {420, 2, 420, 1}, {480, 3, 420, 2}, {480, 2, 480, 1}};
    spec = rows; L = p->L0; C = p->C0;
  } else {
    p->L_in = 98; p->C_in = 257;   // Input(shape=[98 * 257]) -> Reshape([98, 257]); input_size is not consulted
    static const Row rows[8] = {{300, 4, 252, 2}, {300, 3, 300, 1}, {360, 4, 300, 2}, {360, 3, 360, 1},
                                {420, 4, 360, 2}, {420, 3, 360, 1}, {480, 4, 420, 2}, {480, 3, 480, 1}};
    spec = rows; L = p->L_in; C = p->C_in;
  }
  const bool sep = c.kind == KWS_NET_CONV_1D_TOP_DOWN;   // its groups are depthwise-separable, l2 1e-5 on the 1x1 kernels
  for (int i = 0; spec && i < 8; ++i) {
    const Row& s = spec[i];
    if (s.nch > C) KWS_TRY(add_ragged_block(kn, p, L, C, s.F, 3, s.nch));
    else KWS_TRY(add_block(kn, p, L, C, s.F, 3, s.g, s.nch, s.stride, sep ? KWS_L2_COEF : 0.f, false,
                           !sep ? GC_NO_DW : s.stride == 1 ? GC_DW_SHARED : GC_DW_SLICED));
    L = p->blocks.back().d.Lout;
    C = p->blocks.back().F;
  }
  const GcBlock& last = p->blocks.back();
  p->dense.D = last.d.Lout * last.F;
  p->dense.kernel = kws_net_add_tensor(n, "dense_1/kernel", {p->dense.D, NC}, false, 0.f, p->dense.D, NC, 0.f);
  p->dense.bias = kws_net_add_tensor(n, "dense_1/bias", {NC}, false, 0.f, 0, 0, 0.f);
  return KWS_OK;
}

namespace {

int GcProgram::debug_view(int B, int training, int what, int index, int64_t* offset_floats, int64_t* count) const {
  const GcProgram& p = *this;
  GcLayout lo;
  layout(B, training != 0, &lo);
  const int nb = (int)p.blocks.size();
  if (what == 0) {   // pre-BN output of conv stage `index` (conv_1d_fast: 0 = the front convolution)
    const int i = index - (p.has_front() ? 1 : 0);
    KWS_REQUIRE(index >= 0 && i < nb, "net_debug_view: y index %d", index);
    if (i < 0) {
      *offset_floats = lo.y0;
      *count = (int64_t)B * p.L0 * p.C0;
    } else {
      *offset_floats = lo.y[i];
      *count = (int64_t)B * p.blocks[i].d.Lout * p.blocks[i].F;
    }
  } else if (what == 1) {   // depthwise output of conv stage `index`, which must be a separable block
    const int i = index - (p.has_front() ? 1 : 0);
    KWS_REQUIRE(i >= 0 && i < nb && p.blocks[i].sep, "net_debug_view: z index %d", index);
    *offset_floats = lo.dwo[i];
    *count = (int64_t)B * p.blocks[i].d.Lout * p.blocks[i].d.C;
  } else if (what == 2) {   // table of batch_normalization_{index+1}
    for (int i = 0; i < nb; ++i) {
      const GcBlock& b = p.blocks[i];
      if (index >= b.bn_idx0 && index < b.bn_idx0 + b.d.g) {
        *offset_floats = lo.bn[i] + (int64_t)(index - b.bn_idx0) * 4 * b.d.Ng;
        *count = 4 * b.d.Ng;
        return KWS_OK;
      }
    }
    kws_set_error("net_debug_view: bn index %d", index);
    return KWS_E_INVALID;
  } else {
    kws_set_error("net_debug_view: unknown view %d", what);
    return KWS_E_INVALID;
  }
  return KWS_OK;
}

// dA[cur] = gradient wrt the activated output of block i, from the tail's down to the front convolution
int GcProgram::backward(const GcLayout& lo, const NetCall& c) const {
  const GcProgram& p = *this;
  const float* params = c.params;
  const float* x = c.x;
  float* grads = c.grads;
  float* ws = c.ws;
  const int B = c.B;
  hipStream_t st = c.st;
  int cur = 0;
  for (int i = (int)p.blocks.size() - 1; i >= 0; --i) {
    const GcBlock& b = p.blocks[i];
    kws_gconv_t d = b.d;
    d.B = B;
    const int64_t M = (int64_t)B * d.Lout;
    const kws_gbn_cols cols = kws_gbn_grouped(d.g, d.Ng);
    if (b.pool) {   // dA[cur] = gradient wrt the pooled output: route it to the winners, gate it, BN sums in the same pass
      KWS_TRY(kws_pool3s2_bwd_f32(ws + lo.dA[cur], ws + lo.y[i], ws + lo.bn[i], ws + lo.dA[cur ^ 1], ws + lo.part, B, d.Lout, b.F, st));
      cur ^= 1;
      KWS_TRY(kws_gbn_bwd_finish(ws + lo.dA[cur], ws + lo.y[i], ws + lo.bn[i], M, &cols, ws + lo.part,
                                 kws_pool3s2_bwd_part_rows(B, d.Lout, b.F), ws + lo.coef, grads + b.gamma0, b.pstride, b.beta_off, st));
    } else {
      KWS_TRY(kws_gbn_bwd(ws + lo.dA[cur], ws + lo.y[i], ws + lo.bn[i], nullptr, M, &cols, ws + lo.part, ws + lo.coef, grads + b.gamma0,
                          b.pstride, b.beta_off, st));
    }
    float* dy = ws + lo.dA[cur];
    if (b.ragged) {   // the windows [0, gs) and [gs, C) together cover dA[cur ^ 1]: the gradient wrt the activated input
      for (int q = 0; q < 2; ++q) {
        kws_conv1d_t cv = b.rc[q];
        cv.B = B;
        KWS_TRY(kws_conv1d_wgrad_f32(ws + lo.y[i - 1], ws + lo.bnflat, dy, grads + b.rw[q], ws + lo.wws, &cv, st));
        KWS_TRY(kws_conv1d_dgrad_f32(dy, params + b.rw[q], ws + lo.dA[cur ^ 1], 0, &cv, st));
      }
      cur ^= 1;
      continue;
    }
    const GcInput gi = gc_input(p, lo, i, c);
    if (b.sep) {   // the pointwise kernels' gradients and dz, then the depthwise kernels' and the gradient wrt the activated input
      const GcDwInput di = gc_dw_input(p, i, gi, c);
      KWS_TRY(kws_gconv_wgrad_f32(ws + lo.dwo[i], nullptr, 0, dy, grads + b.w0, ws + lo.wws, &d, st));
      KWS_TRY(kws_gconv_dgrad_f32(dy, params + b.w0, ws + lo.dA[cur ^ 1], &d, st));
      KWS_TRY(kws_gdwconv_bwd_f32(gi.in, di.tab, ws + lo.dA[cur ^ 1], params + b.dw0, ws + lo.dA[cur], grads + b.dw0, nullptr,
                                  ws + lo.dwws, &di.d, st));
      continue;
    }
    KWS_TRY(kws_gconv_wgrad_f32(gi.in, gi.bn, gi.bg, dy, grads + b.w0, ws + lo.wws, &d, st));
    if (p.head2 && i + 1 == (int)p.blocks.size()) {   // back through Dropout(.3): the gradient wrt the activated ladder output
      KWS_TRY(kws_gconv_dgrad_f32(dy, params + b.w0, ws + lo.fa, &d, st));
      KWS_TRY(kws_dropout_bwd(ws + lo.fa, ws + lo.dA[cur], B, p.Dd, p.keep, c.seed, c.step, 1, c.row_offset, st));
    } else if (i > 0 || p.has_front()) {
      KWS_TRY(kws_gconv_dgrad_f32(dy, params + b.w0, ws + lo.dA[cur ^ 1], &d, st));
      cur ^= 1;
    }
  }
  // a front bias cancels in block 1's BatchNorm on batch statistics: its gradient is exactly 0, not the float32 residue (1e-5)
  // that the column sum of dA[cur] would leave
  if (p.bias0 >= 0) KWS_HIP(hipMemsetAsync(grads + p.bias0, 0, sizeof(float) * p.C0, st));
  if (p.front) {   // dA[cur] = gradient wrt the front convolution's output (no BN, no activation in between)
    KWS_TRY(kws_gemm_tn_gather_f32(x, &p.g0, ws + lo.dA[cur], ws + lo.dw0p, B, p.C0, ws + lo.tnws, st));
    KWS_HIP(hipMemcpyAsync(grads + p.conv0, ws + lo.dw0p, sizeof(float) * p.K0 * p.C0, hipMemcpyDeviceToDevice, st));
  }
  if (p.fbank) {   // likewise; the six kernels' gradients land at their own offsets in grads
    kws_fbank_conv_t fb = p.fb;
    fb.B = B;
    KWS_TRY(kws_fbank_conv_wgrad_f32(x, ws + lo.dA[cur], grads, ws + lo.fbws, &fb, st));
  }
  return KWS_OK;
}

}  // namespace
