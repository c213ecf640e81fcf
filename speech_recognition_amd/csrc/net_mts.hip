// Network program of the three-branch raw-waveform net:
//   KWS_NET_CONV_1D_MULTI_TIME_SLICED  conv_1d_multi_time_sliced_model (reference model.py:1080-1156): the 16000 samples viewed as
//                        [4000, 4], [3200, 5] and [640, 25], each view a ladder of _depthwise_conv_block (DepthwiseConv2D((1, k),
//                        VALID, l2 1e-5) -> Conv1D(F, 1, l2 1e-5) -> BatchNormalization -> relu6); a _reduce_conv is a block followed
//                        by MaxPool1D(3, strides=2, 'same'), a _context_conv a bare block.  Five one-step branch ends of 64 channels
//                        are concatenated -> Dropout(.1) -> _context_conv(128, 1) -> Dropout(.1) -> Conv1D(num_classes, 1, softmax,
//                        bias); RMSprop(3e-3), categorical CE.  32 blocks, in the reference's creation order (= Keras numbering):
//                          xs4   1 - 7 reduce (16 .. 160), 8 context (160, 3) [28 steps, TWO consumers], 9 context (64, 28) = end xs4a,
//                                10 reduce (192), 11 context (192, 3), 12 context (64, 11) = end xs4b
//                          xs5   13 - 24, the same ladder on 3200 steps (22 steps at the fork; ends k 22 and k 8)
//                          xs25  25 - 29 reduce (32 .. 128), 30 context (128, 3), 31 context (64, 17) = end xs25
//                          head  32 context (128, 1) over the 320 concatenated features
// Data flow (training):
//   stem (blocks 1, 13, 25)   y = kws_stem_fwd_f32(x): depthwise + pointwise in one kernel, 4 / 5 / 25 input channels
//   other blocks              net_sepblock.hip's: z = dwk(input), y = z W (f32 MFMA GEMM with the BN statistics in its epilogue)
//   reduce block              a = kws_pool3s2_same_fwd_f32(y, table): the pooled tensor is materialised ACTIVATED, its consumer
//                             reads it without a table
//   fork (blocks 8, 20)       a = relu6(bn(y)) materialised once (at most [B, 28, 160]); both consumers read it without a table
//   context behind context    BN + ReLU6 applied on load by the consumer's depthwise kernel (blocks 12, 24, 31)
//   branch end                its activated output goes to its 64 columns of the feature buffer [B, 320]
//   head                      Dropout (layer 1) -> one-tap depthwise -> GEMM -> BN table; bias, relu6, Dropout (layer 2), the
//                             classifier and the loss run inside the flat tail over (y, table), as conv_1d_heavy's head does
// The backward walks the blocks in descending order on ONE stream.  At a fork the two consumers' gradients wrt the materialised
// activation are added before the fork's single BatchNorm backward.  The three ladders reuse the same gradient buffers.
#include "net_internal.h"

namespace {

struct MtBlock : SepBlock {   // all VALID at stride 1
  int src = -1;          // producing block, -1 = the raw input (stem)
  int Lp = 0;            // rows per clip that leave the block (behind the pool, if any)
  bool pool = false;     // _reduce_conv: SAME pool behind the block
  bool fork = false;     // the activated output is materialised for two consumers
  bool onload = false;   // reads its producer's raw output through the producer's table
  int end_col = -1;      // branch end: first column in the feature buffer
};

struct MtLayout {
  int64_t total = 0;
  std::vector<int64_t> z, y, bn, a;   // depthwise output, raw pointwise output, table, materialised activation (pool / fork)
  int64_t stats = 0, red = 0, feat = 0, featd = 0;
  int64_t G[2] = {0, 0}, FG = 0, DZ = 0, part = 0, coef = 0, tn = 0, WT = 0, stem = 0;
  FlatTailWs tail;
};

struct MtProgram : FlatTailProgram<MtLayout> {
  std::vector<MtBlock> blocks;   // blocks.back() is the head's context block
  int D = 0, H = 0;              // concatenated features, head width (the classifier is `dense`)
  float keep = 0.9f;

  void layout(int B, bool training, MtLayout* lo) const override;
  int forward(const MtLayout& lo, const NetCall& c) const override;
  kws_flat_tail_args tail_args(const MtLayout& lo, const NetCall& c, float* probs) const override;
  int64_t tail_grad(const MtLayout& lo) const override { return lo.G[0]; }
  int backward(const MtLayout& lo, const NetCall& c) const override;
  int debug_view(int B, int training, int what, int index, int64_t* offset_floats, int64_t* count) const override;
};

constexpr float MT_DROP_KEEP = 0.9f;   // Dropout(0.1), model.py:1144, 1146
constexpr int MT_END_WIDTH = 64, MT_HEAD_WIDTH = 128;

// feat[b, col0 + c] = relu6(scale[c] * y[b, c] + shift[c]): a branch end's activated output at its place in the concatenation
__global__ __launch_bounds__(256) void mt_end_act_kernel(const float* __restrict__ y, const float* __restrict__ bn, float* __restrict__ feat,
                                                         int B, int C, int pitch, int col0) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * C) return;
  const int b = i / C, c = i - b * C;
  feat[(int64_t)b * pitch + col0 + c] = relu6f(fmaf(y[i], bn[c], bn[C + c]));
}

// out[b, c] = in[b, col0 + c]: the gradient of one branch end out of the concatenation's
__global__ __launch_bounds__(256) void mt_cols_kernel(const float* __restrict__ in, float* __restrict__ out, int B, int C, int pitch,
                                                      int col0) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * C) return;
  const int b = i / C, c = i - b * C;
  out[i] = in[(int64_t)b * pitch + col0 + c];
}

void MtProgram::layout(int B, bool training, MtLayout* lo) const {
  const MtProgram& p = *this;
  Bump bp;
  const int nb = (int)p.blocks.size();
  int64_t max_g = 64, max_z = 64, max_stats = 64, max_part = 64, max_tn = 64, max_w = 64, max_fork = 64, max_stem = 64;
  int maxC = 4;
  lo->z.assign(nb, 0);
  lo->y.assign(nb, 0);
  lo->bn.assign(nb, 0);
  lo->a.assign(nb, 0);
  for (int i = 0; i < nb; ++i) {
    const MtBlock& b = p.blocks[i];
    const int64_t M = (int64_t)B * b.Lout;
    if (b.src >= 0 || i == nb - 1) lo->z[i] = bp.take(M * b.cin);
    lo->y[i] = bp.take(M * b.cout);
    lo->bn[i] = bp.take((int64_t)4 * b.cout);
    if (b.pool) lo->a[i] = bp.take((int64_t)B * b.Lp * b.cout);
    if (b.fork) lo->a[i] = bp.take(M * b.cout);
    maxC = std::max(maxC, b.cout);
    max_g = std::max(max_g, std::max(M * b.cout, (int64_t)B * b.Lin * b.cin));
    max_part = std::max(max_part, (int64_t)kws_gbn_bwd_rows(M) * 2 * b.cout);
    if (b.pool) max_part = std::max(max_part, kws_pool3s2_same_bwd_part_floats(B, b.Lout, b.cout));
    if (b.fork) max_fork = std::max(max_fork, M * b.cout);
    if (b.src < 0 && i != nb - 1) {
      max_stats = std::max(max_stats, (int64_t)2 * b.cout * kws_stem_stats_rows(B, b.Lin));
      max_stem = std::max(max_stem, kws_stem_bwd_workspace_floats(B, b.Lin, b.cin, b.cout));
    } else {
      max_z = std::max(max_z, M * b.cin);
      max_stats = std::max(max_stats, (int64_t)2 * b.cout * kws_gemm_num_row_tiles(M));
      max_part = std::max(max_part, kws_dwconvk_bwd_part_floats(B, b.Lin, b.cin, b.k, 1));
      max_tn = std::max(max_tn, kws_gemm_tn_workspace_floats(M, b.cin, b.cout));
      max_w = std::max(max_w, (int64_t)b.cin * b.cout);
    }
  }
  lo->stats = bp.take(max_stats);
  lo->red = bp.take((int64_t)KWS_REDUCE_SLICES * 2 * maxC);
  lo->feat = bp.take((int64_t)B * p.D);
  if (training) {
    lo->featd = bp.take((int64_t)B * p.D);
    lo->G[0] = bp.take(max_g);
    lo->G[1] = bp.take(max_g);
    lo->FG = bp.take(max_fork);
    lo->DZ = bp.take(max_z);
    lo->part = bp.take(max_part);
    lo->coef = bp.take((int64_t)2 * std::max(maxC, p.D));
    lo->tn = bp.take(max_tn);
    lo->WT = bp.take(max_w);
    lo->stem = bp.take(max_stem);
    lo->tail.take(bp, B, p.H, dense.NC);
  }
  lo->total = bp.cur * 4;
}

// what block i's depthwise layer reads: (tensor, table or NULL)
void mt_input(const MtProgram& p, const MtLayout& lo, int i, float* ws, const float** in, const float** bn) {
  const MtBlock& b = p.blocks[i];
  if (b.onload) {
    *in = ws + lo.y[b.src];
    *bn = ws + lo.bn[b.src];
  } else {
    *in = ws + lo.a[b.src];
    *bn = nullptr;
  }
}

// forward through the 31 branch blocks, the concatenation and the head's block; training: batch statistics and dropout
int MtProgram::forward(const MtLayout& lo, const NetCall& c) const {
  const MtProgram& p = *this;
  const float* params = c.params;
  float* state = c.state;
  float* ws = c.ws;
  const int B = c.B;
  const bool training = c.training;
  hipStream_t st = c.st;
  const int nb = (int)p.blocks.size();
  float* stats = training ? ws + lo.stats : nullptr;
  for (int i = 0; i + 1 < nb; ++i) {
    const MtBlock& b = p.blocks[i];
    const int64_t M = (int64_t)B * b.Lout;
    int rows;
    if (b.src < 0) {
      KWS_TRY(kws_stem_fwd_f32(c.x, params + b.dw, params + b.pw, ws + lo.y[i], B, b.Lin, b.cin, b.cout, stats, st));
      rows = kws_stem_stats_rows(B, b.Lin);
    } else {
      const float *in, *bn_in;
      mt_input(p, lo, i, ws, &in, &bn_in);
      rows = kws_sep_fwd(b, params, in, bn_in, ws + lo.z[i], ws + lo.y[i], stats, B, st);
      if (rows < 0) return rows;
    }
    KWS_TRY(kws_sep_bn_table(b, params, state, stats, rows, M, training, ws + lo.bn[i], ws + lo.red, st));
    if (b.pool) KWS_TRY(kws_pool3s2_same_fwd_f32(ws + lo.y[i], ws + lo.bn[i], ws + lo.a[i], B, b.Lout, b.cout, st));
    if (b.fork) KWS_TRY(kws_bn_relu6_apply(ws + lo.y[i], ws + lo.bn[i], ws + lo.a[i], M, b.cout, 1, st));
    if (b.end_col >= 0) {
      hipLaunchKernelGGL(mt_end_act_kernel, dim3((unsigned)ceil_div(B * b.cout, 256)), dim3(256), 0, st, ws + lo.y[i], ws + lo.bn[i],
                         ws + lo.feat, B, b.cout, p.D, b.end_col);
      KWS_LAUNCH_CHECK("mt_end_act_kernel");
    }
  }
  // Dropout(.1) -> _context_conv(128, 1): a one-tap depthwise layer (a per-channel scale) and the 320 -> 128 GEMM
  const MtBlock& h = p.blocks[nb - 1];
  const float* feat = ws + lo.feat;
  if (training) {
    KWS_TRY(kws_dropout_fwd(ws + lo.feat, ws + lo.featd, B, p.D, p.keep, c.seed, c.step, 1, c.row_offset, st));
    feat = ws + lo.featd;
  }
  const int rows = kws_sep_fwd(h, params, feat, nullptr, ws + lo.z[nb - 1], ws + lo.y[nb - 1], stats, B, st);
  if (rows < 0) return rows;
  return kws_sep_bn_table(h, params, state, stats, rows, B, training, ws + lo.bn[nb - 1], ws + lo.red, st);
}

// relu6(bn(.)) of the head's block, Dropout (layer 2), Conv1D(num_classes, 1) + bias + softmax (+ loss and its backward)
kws_flat_tail_args MtProgram::tail_args(const MtLayout& lo, const NetCall& c, float* probs) const {
  const int nb = (int)blocks.size();
  kws_flat_tail_args t;
  memset(&t, 0, sizeof(t));
  t.y = c.ws + lo.y[nb - 1]; t.bn = c.ws + lo.bn[nb - 1]; t.Ng = H;
  t.Wd = c.params + dense.kernel; t.bd = c.params + dense.bias;
  t.probs = probs;
  t.B = c.B; t.D = H; t.F = H; t.NC = dense.NC;
  t.keep_prob = keep;
  t.layer_id = 2;
  return t;
}

}  // namespace

int mt_build(kws_net* n) {
  const kws_net_config_t& c = n->cfg;
  KWS_REQUIRE(c.input_size == 16000, "net: conv_1d_multi_time_sliced input_size %d (the reference reshapes exactly 16000 samples)",
              c.input_size);
  MtProgram* p = new MtProgram();
  n->program.reset(p);
  p->net = n;
  p->dense.NC = c.num_classes;
  p->zero_grads = true;
  p->keep = MT_DROP_KEEP;
  KerasNames kn{n};
  int cur = -1, L = 0, C = 0, col = 0;   // the tensor the next block reads
  bool fail = false;
  auto add = [&](int F, int k, bool pool) {
    MtBlock b;
    b.src = cur; b.Lin = L; b.k = k; b.cin = C; b.cout = F; b.pool = pool;
    b.Lout = L - k + 1;
    if (b.Lout < 1 || (pool && b.Lout < 2)) fail = true;
    b.Lp = pool ? kws_pool3s2_same_out_len(b.Lout) : b.Lout;
    b.onload = cur >= 0 && !p->blocks[cur].pool && !p->blocks[cur].fork;
    b.dw = kn.dwk(k, C);
    b.pw = kn.conv(1, C, F, KWS_L2_COEF);
    b.bn = kn.bn(F);
    p->blocks.push_back(b);
    cur = (int)p->blocks.size() - 1;
    L = b.Lp;
    C = F;
    return cur;
  };
  auto end = [&](int from, int k) {   // _context_conv(64, k) over the whole remaining length of block `from`'s output
    const int keep_cur = cur, keep_L = L, keep_C = C;
    cur = from; L = p->blocks[from].Lp; C = p->blocks[from].cout;
    const int e = add(MT_END_WIDTH, k, false);
    if (p->blocks[e].Lout != 1) fail = true;
    p->blocks[e].end_col = col;
    col += MT_END_WIDTH;
    cur = keep_cur; L = keep_L; C = keep_C;
  };
  static const int wide[7] = {16, 32, 48, 64, 96, 128, 160};
  for (int view = 0; view < 2; ++view) {   // xs4 = [4000, 4], xs5 = [3200, 5] (model.py:1105-1131)
    cur = -1; L = view == 0 ? 4000 : 3200; C = view == 0 ? 4 : 5;
    for (int i = 0; i < 7; ++i) add(wide[i], 3, true);
    const int f = add(160, 3, false);
    p->blocks[f].fork = true;
    end(f, view == 0 ? 28 : 22);
    cur = f;
    add(192, 3, true);
    const int g = add(192, 3, false);
    end(g, view == 0 ? 11 : 8);
  }
  {   // xs25 = [640, 25] (model.py:1133-1140)
    static const int w25[5] = {32, 48, 64, 96, 128};
    cur = -1; L = 640; C = 25;
    for (int i = 0; i < 5; ++i) add(w25[i], 3, true);
    const int g = add(128, 3, false);
    end(g, 17);
  }
  KWS_REQUIRE(!fail && col == 5 * MT_END_WIDTH, "net: conv_1d_multi_time_sliced ladders do not end in five one-step tensors");
  p->D = col;
  p->H = p->dense.D = MT_HEAD_WIDTH;
  cur = -1; L = 1; C = p->D;
  add(p->H, 1, false);   // _context_conv(128, 1) over the concatenation
  p->blocks.back().onload = false;
  p->dense.kernel = kn.conv(1, p->H, c.num_classes, 0.f);
  p->dense.bias = kws_net_add_tensor(n, "conv1d_" + std::to_string(kn.n_conv) + "/bias", {c.num_classes}, false, 0.f, 0, 0, 0.f);
  return KWS_OK;
}

namespace {

int MtProgram::debug_view(int B, int training, int what, int index, int64_t* offset_floats, int64_t* count) const {
  const MtProgram& p = *this;
  MtLayout lo;
  layout(B, training != 0, &lo);
  KWS_REQUIRE(index >= 0 && index < (int)p.blocks.size(), "net_debug_view: block index %d", index);
  const MtBlock& b = p.blocks[index];
  if (what == 0) {          // raw pointwise output of block `index` (creation order)
    *offset_floats = lo.y[index];
    *count = (int64_t)B * b.Lout * b.cout;
  } else if (what == 2) {   // table of batch_normalization_{index+1}
    *offset_floats = lo.bn[index];
    *count = (int64_t)4 * b.cout;
  } else {
    kws_set_error("net_debug_view: unknown view %d", what);
    return KWS_E_INVALID;
  }
  return KWS_OK;
}

// the head's context block, then the 31 branch blocks
int MtProgram::backward(const MtLayout& lo, const NetCall& c) const {
  const MtProgram& p = *this;
  const float* params = c.params;
  const float* x = c.x;
  float* grads = c.grads;
  float* ws = c.ws;
  const int B = c.B;
  hipStream_t st = c.st;
  const int nb = (int)p.blocks.size();
  float* G[2] = {ws + lo.G[0], ws + lo.G[1]};
  float* FG = ws + lo.FG;
  float* part = ws + lo.part;
  float* coef = ws + lo.coef;
  const SepBwdScratch scratch = {ws + lo.WT, ws + lo.DZ, ws + lo.tn, part, coef};
  float* dcat = ws + lo.featd;   // gradient wrt the concatenated features [B, 320], over the dropped features once they are spent
  {
    const MtBlock& h = p.blocks[nb - 1];
    // G[0] = gradient wrt relu6(bn(y)) [B, 128] -> dy; the GEMM's two gradients; the one-tap depthwise layer; Dropout (layer 1)
    KWS_TRY(kws_gbn_layer_bwd(G[0], ws + lo.y[nb - 1], ws + lo.bn[nb - 1], nullptr, B, kws_gbn_grouped(1, h.cout), part, coef, grads,
                              h.bn, st));
    KWS_TRY(kws_sep_bwd(h, params, grads, G[0], ws + lo.z[nb - 1], ws + lo.featd, nullptr, nullptr, G[0], scratch, B, st));
    KWS_TRY(kws_dropout_bwd(G[0], dcat, B, p.D, p.keep, c.seed, c.step, 1, c.row_offset, st));
  }
  // ---- the 31 branch blocks, descending: `grad` = what arrives at block i, wrt its output (is_dy false) or its raw y (true) ----
  float* grad = nullptr;
  bool is_dy = false, fork_filled = false;
  for (int i = nb - 2; i >= 0; --i) {
    const MtBlock& b = p.blocks[i];
    const int64_t M = (int64_t)B * b.Lout;
    if (b.end_col >= 0) {
      grad = G[0];
      is_dy = false;
      hipLaunchKernelGGL(mt_cols_kernel, dim3((unsigned)ceil_div(B * b.cout, 256)), dim3(256), 0, st, dcat, grad, B, b.cout, p.D,
                         b.end_col);
      KWS_LAUNCH_CHECK("mt_cols_kernel");
    } else if (b.fork) {
      grad = FG;   // the sum of its two consumers' gradients
      is_dy = false;
      fork_filled = false;
    }
    float* dy = grad;
    if (!is_dy) {
      if (b.pool) {   // route the pooled gradient to the winners, gate it, BN sums in the same pass
        dy = grad == G[0] ? G[1] : G[0];
        KWS_TRY(kws_pool3s2_same_bwd_f32(grad, ws + lo.y[i], ws + lo.bn[i], dy, part, B, b.Lout, b.cout, st));
        KWS_TRY(kws_gbn_layer_bwd_finish(dy, ws + lo.y[i], ws + lo.bn[i], M, kws_gbn_grouped(1, b.cout), part,
                                         kws_pool3s2_same_bwd_part_rows(B, b.Lout, b.cout), coef, grads, b.bn, st));
      } else {
        KWS_TRY(kws_gbn_layer_bwd(dy, ws + lo.y[i], ws + lo.bn[i], nullptr, M, kws_gbn_grouped(1, b.cout), part, coef, grads, b.bn,
                                  st));
      }
    }
    if (b.src < 0) {   // stem: both kernels' gradients from dy and x; no gradient leaves the input
      KWS_TRY(kws_stem_bwd_f32(dy, x, params + b.dw, params + b.pw, grads + b.dw, grads + b.pw, B, b.Lin, b.cin, b.cout, ws + lo.stem,
                               st));
      continue;
    }
    const MtBlock& pb = p.blocks[b.src];
    const bool to_fork = pb.fork;
    float* out = (to_fork && !fork_filled) ? FG : (dy == G[0] ? G[1] : G[0]);
    const float *in, *bn_in;
    mt_input(p, lo, i, ws, &in, &bn_in);
    // onload: the producer's BatchNorm backward rides on this pass and out becomes the producer's dy
    KWS_TRY(kws_sep_bwd(b, params, grads, dy, ws + lo.z[i], in, bn_in, b.onload ? &pb.bn : nullptr, out, scratch, B, st));
    is_dy = b.onload;
    if (to_fork) {
      if (fork_filled) KWS_TRY(kws_add_f32(FG, out, FG, (int64_t)B * b.Lin * b.cin, st));
      fork_filled = true;
    }
    grad = out;
  }
  return KWS_OK;
}

}  // namespace
