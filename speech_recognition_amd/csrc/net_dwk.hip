// Network programs of the general depthwise ladder:
//   KWS_NET_CONV_1D_GRU  conv_1d_gru_model (reference model.py:470-512; Keras model name 'conv_1d_bigru', no recurrent layer):
//                        raw waveform as [16000, 1] -> six _depthwise_conv_block (DepthwiseConv2D((1, k), strides=s, l2 1e-5) ->
//                        Conv1D(F, 1, l2 1e-5) -> BatchNormalization -> relu6) with k 63 / 31 / 15 / 7 / 5 SAME at strides
//                        16 / 4 / 4 / 4 / 2 and k 8 VALID, F = 128 / 256 / 384 / 448 / 512 / 512 -> Flatten (one time step) ->
//                        Dropout(.3) -> Dense(256) -> relu6 -> Dropout(.3) -> Dense + softmax; RMSprop(1e-3), categorical CE
//   KWS_NET_CONV_1D_SIMPLE  conv_1d_simple_model (reference model.py:116-156; Keras model name 'conv_1d_time_stacked'): raw waveform as
//                        [16000, 1] -> fourteen such blocks, all VALID: k 31 at stride 16, then k 3 at strides 1, 2, 1, 2, 1, ...;
//                        F = 32, 32, 64, 64, 96, 96 .. 224, 224; ends at [B, 10, 224] -> Bidirectional(GRU(128, dropout=.2,
//                        recurrent_dropout=.2)) (gru.hip) -> Dense + softmax; Adam(1e-3), categorical CE.  No l2 on the GRU or the Dense
//                        layer.  The activated ladder output is materialised for the GRU's GEMMs (kws_bn_relu6_apply), its masked
//                        views by kws_gru_fwd_f32; the head is the flat tail's raw arm over the signed [B, 256] GRU output.
// The blocks and their data flow are net_sepblock.hip's.  Block 1 has one input channel: its depthwise layer is the C = 1 arm and
// its pointwise layer the outer product kws_dwconvk_pw1_* (K = 1 is outside the GEMM).
// The hidden Dense layer is a GEMM over the materialised dropped features; its bias, relu6 and Dropout run inside the flat tail,
// which reads (h, table) with the table scale = 1 | shift = bias (fmaf(h, 1, b) = h + b exactly).
#include "net_internal.h"

namespace {

struct DkProgram : NetProgram {
  const kws_net* net = nullptr;
  std::vector<SepBlock> blocks;
  int NC = 0, D = 0, H = 0;          // features into the head, hidden width
  int64_t d1k = 0, d1b = -1, d2k = 0, d2b = 0;
  float keep = 0.7f;
  // KWS_NET_CONV_1D_SIMPLE: the ladder ends in gT steps of D channels, a bidirectional GRU of gH units follows (H = 0: no hidden Dense)
  bool gru = false;
  int gT = 0, gH = 0;
  int64_t gW[2] = {0, 0}, gU[2] = {0, 0}, gb[2] = {0, 0};

  int64_t workspace_bytes(int B, int training) const override;
  int debug_view(int B, int training, int what, int index, int64_t* offset_floats, int64_t* count) const override;
  int predict(const float* params, const float* state, const float* x, int B, float* probs, float* ws, int64_t ws_bytes,
              hipStream_t st) const override;
  int train(const float* params, float* state, const float* x, const float* y_onehot, int B, float* grads, float* probs, float* metrics,
            uint64_t seed, uint32_t step, int64_t row_offset, int loss_batch, float* ws, int64_t ws_bytes, hipStream_t st) const override;
};

constexpr float DK_DROP_KEEP = 0.7f;   // Dropout(0.3), model.py:502, 504
constexpr int DK_HIDDEN = 256;         // Dense(256), model.py:503
constexpr int DK_GRU_UNITS = 128;      // GRU(128, ...), model.py:148
constexpr float DK_GRU_KEEP = 0.8f;    // dropout=0.2, recurrent_dropout=0.2

// tab [4][n] = 1 | bias (0 without one) | 0 | 1: what the flat tail reads as a BatchNorm table
__global__ __launch_bounds__(256) void dk_bias_table_kernel(const float* __restrict__ bias, int n, float* __restrict__ tab) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  tab[i] = 1.f;
  tab[n + i] = bias ? bias[i] : 0.f;
  tab[2 * n + i] = 0.f;
  tab[3 * n + i] = 1.f;
}

// d[b, i] *= relu6'(h[b, i] + bias[i]) in place; slice blockIdx.y adds its rows of the result, ascending, into part[slice][n]
__global__ __launch_bounds__(256) void dk_bias_relu6_bwd_kernel(float* __restrict__ d, const float* __restrict__ h,
                                                                const float* __restrict__ bias, int B, int n, int rows_per,
                                                                float* __restrict__ part) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float bi = bias ? bias[i] : 0.f;
  const int b0 = blockIdx.y * rows_per;
  const int b1 = b0 + rows_per < B ? b0 + rows_per : B;
  float sum = 0.f;
  for (int b = b0; b < b1; ++b) {
    const float pre = h[(int64_t)b * n + i] + bi;
    const float v = (pre > 0.f && pre <= 6.f) ? d[(int64_t)b * n + i] : 0.f;
    d[(int64_t)b * n + i] = v;
    sum += v;
  }
  part[(int64_t)blockIdx.y * n + i] = sum;
}

__global__ __launch_bounds__(256) void dk_bias_grad_fold_kernel(const float* __restrict__ part, int slices, int n,
                                                                float* __restrict__ dbias) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float sum = 0.f;
  for (int s = 0; s < slices; ++s) sum += part[(int64_t)s * n + i];
  dbias[i] = sum;
}

}  // namespace

// (declared in net_internal.h: net_time_sliced.hip's head is this one without the bias)
int dk_bias_table(const float* bias, int n, float* tab, hipStream_t st) {
  hipLaunchKernelGGL(dk_bias_table_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, bias, n, tab);
  KWS_LAUNCH_CHECK("dk_bias_table_kernel");
  return KWS_OK;
}

// the hidden layer's backward through bias + relu6: gradient wrt relu6(h + bias) -> gradient wrt h, in place; dbias may be NULL
// (a hidden layer without bias: conv_1d_time_sliced has this head with use_bias=False)
int dk_bias_relu6_bwd(float* d, const float* h, const float* bias, float* dbias, int B, int n, float* part, hipStream_t st) {
  const int rows_per = ceil_div(B, DK_BIAS_SLICES);
  const int slices = ceil_div(B, rows_per);
  hipLaunchKernelGGL(dk_bias_relu6_bwd_kernel, dim3((unsigned)ceil_div(n, 256), (unsigned)slices), dim3(256), 0, st, d, h, bias, B, n,
                     rows_per, part);
  KWS_LAUNCH_CHECK("dk_bias_relu6_bwd_kernel");
  if (dbias) {
    hipLaunchKernelGGL(dk_bias_grad_fold_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, part, slices, n, dbias);
    KWS_LAUNCH_CHECK("dk_bias_grad_fold_kernel");
  }
  return KWS_OK;
}

namespace {

struct DkLayout {
  int64_t total = 0;
  std::vector<int64_t> z, y, bn;
  int64_t stats = 0, red = 0, fa = 0, fd1 = 0, h = 0, tab = 0;
  int64_t G[2] = {0, 0}, DZ = 0, part = 0, coef = 0, tn = 0, WT = 0, pw1ws = 0;
  int64_t fd = 0, dl = 0, per_loss = 0, per_correct = 0, swg = 0, bpart = 0;
  int64_t gmx = 0, gmh = 0, gout = 0, gsave = 0, gws = 0, gdout = 0;   // KWS_NET_CONV_1D_SIMPLE
};

void dk_layout(const DkProgram& p, int B, bool training, DkLayout* lo) {
  Bump bp;
  const int nb = (int)p.blocks.size();
  int64_t max_y = 64, max_z = 64, max_stats = 64, max_part = 64, max_tn = 64, max_w = 64;
  int maxC = 4;
  lo->z.assign(nb, 0);
  lo->y.assign(nb, 0);
  lo->bn.assign(nb, 0);
  for (int i = 0; i < nb; ++i) {
    const SepBlock& b = p.blocks[i];
    const int64_t M = (int64_t)B * b.Lout;
    lo->z[i] = bp.take(M * b.cin);
    lo->y[i] = bp.take(M * b.cout);
    lo->bn[i] = bp.take((int64_t)4 * b.cout);
    max_y = std::max(max_y, std::max(M * b.cout, (int64_t)B * b.Lin * b.cin));
    max_z = std::max(max_z, M * b.cin);
    maxC = std::max(maxC, b.cout);
    max_stats = std::max(max_stats, (int64_t)2 * b.cout * (i == 0 ? kws_dwconvk_pw1_stats_rows(M) : kws_gemm_num_row_tiles(M)));
    max_part = std::max(max_part, kws_dwconvk_bwd_part_floats(B, b.Lin, b.cin, b.k, b.stride));
    if (i > 0) {
      max_tn = std::max(max_tn, kws_gemm_tn_workspace_floats(M, b.cin, b.cout));
      max_w = std::max(max_w, (int64_t)b.cin * b.cout);
    }
  }
  if (p.gru) {
    const int T = p.gT, I = p.D, H = p.gH;
    max_part = std::max(max_part, (int64_t)kws_gbn_bwd_rows((int64_t)B * T) * 2 * I);
    lo->stats = bp.take(max_stats);
    lo->red = bp.take((int64_t)KWS_REDUCE_SLICES * 2 * maxC);
    lo->fa = bp.take((int64_t)B * T * I);
    lo->gout = bp.take((int64_t)B * 2 * H);
    lo->gws = bp.take(kws_gru_workspace_floats(B, T, I, H, training ? 1 : 0));
    if (training) {
      lo->gmx = bp.take((int64_t)6 * B * I);
      lo->gmh = bp.take((int64_t)6 * B * H);
      lo->gsave = bp.take(kws_gru_save_floats(B, T, H));
      lo->gdout = bp.take((int64_t)B * 2 * H);
      lo->G[0] = bp.take(max_y);
      lo->G[1] = bp.take(max_y);
      lo->DZ = bp.take(max_z);
      lo->part = bp.take(max_part);
      lo->coef = bp.take((int64_t)2 * maxC);
      lo->tn = bp.take(max_tn);
      lo->WT = bp.take(max_w);
      lo->pw1ws = bp.take(kws_dwconvk_pw1_bwd_workspace_floats((int64_t)B * p.blocks[0].Lout, p.blocks[0].cout));
      lo->fd = bp.take((int64_t)B * 2 * H);
      lo->dl = bp.take((int64_t)B * p.NC);
      lo->per_loss = bp.take(B);
      lo->per_correct = bp.take(B);
      lo->swg = bp.take((int64_t)KWS_SMALL_WGRAD_SLICES * 2 * H * p.NC);
    }
    lo->total = bp.cur * 4;
    return;
  }
  max_stats = std::max(max_stats, (int64_t)2 * p.H * kws_gemm_num_row_tiles(B));
  max_part = std::max(max_part, (int64_t)kws_gbn_bwd_rows(B) * 2 * p.D);
  max_tn = std::max(max_tn, kws_gemm_tn_workspace_floats(B, p.D, p.H));
  max_w = std::max(max_w, (int64_t)p.D * p.H);
  lo->stats = bp.take(max_stats);
  lo->red = bp.take((int64_t)KWS_REDUCE_SLICES * 2 * maxC);
  lo->fa = bp.take((int64_t)B * p.D);
  lo->h = bp.take((int64_t)B * p.H);
  lo->tab = bp.take((int64_t)4 * p.H);
  if (training) {
    lo->fd1 = bp.take((int64_t)B * p.D);
    lo->G[0] = bp.take(max_y);
    lo->G[1] = bp.take(max_y);
    lo->DZ = bp.take(max_z);
    lo->part = bp.take(max_part);
    lo->coef = bp.take((int64_t)2 * maxC);
    lo->tn = bp.take(max_tn);
    lo->WT = bp.take(max_w);
    lo->pw1ws = bp.take(kws_dwconvk_pw1_bwd_workspace_floats((int64_t)B * p.blocks[0].Lout, p.blocks[0].cout));
    lo->fd = bp.take((int64_t)B * p.H);
    lo->dl = bp.take((int64_t)B * p.NC);
    lo->per_loss = bp.take(B);
    lo->per_correct = bp.take(B);
    lo->swg = bp.take((int64_t)KWS_SMALL_WGRAD_SLICES * p.H * p.NC);
    lo->bpart = bp.take((int64_t)DK_BIAS_SLICES * p.H);
  }
  lo->total = bp.cur * 4;
}

// forward through the blocks and the hidden Dense product; training: batch statistics (moving averages updated) and dropout
int dk_forward(const DkProgram& p, const DkLayout& lo, const float* params, float* state, const float* x, int B, bool training, float* ws,
               uint64_t seed, uint32_t step, int64_t row_offset, hipStream_t st) {
  const int nb = (int)p.blocks.size();
  for (int i = 0; i < nb; ++i) {
    const SepBlock& b = p.blocks[i];
    const int64_t M = (int64_t)B * b.Lout;
    const float* in = i == 0 ? x : ws + lo.y[i - 1];
    const float* bn_in = i == 0 ? nullptr : ws + lo.bn[i - 1];
    float* stats = training ? ws + lo.stats : nullptr;
    int rows;
    if (i == 0) {
      KWS_TRY(kws_dwconvk_fwd_f32(in, bn_in, params + b.dw, ws + lo.z[i], B, b.Lin, b.Lout, b.cin, b.k, b.stride, b.pad_l, st));
      KWS_TRY(kws_dwconvk_pw1_fwd_f32(ws + lo.z[i], params + b.pw, ws + lo.y[i], M, b.cout, stats, st));
      rows = kws_dwconvk_pw1_stats_rows(M);
    } else {
      rows = kws_sep_fwd(b, params, in, bn_in, ws + lo.z[i], ws + lo.y[i], stats, B, st);
      if (rows < 0) return rows;
    }
    KWS_TRY(kws_sep_bn_table(b, params, state, stats, rows, M, training, ws + lo.bn[i], ws + lo.red, st));
  }
  if (p.gru) {   // the activated ladder output [B, T, I] is materialised for the GRU's GEMMs; masks only in training
    const int T = p.gT, I = p.D, H = p.gH;
    KWS_TRY(kws_bn_relu6_apply(ws + lo.y[nb - 1], ws + lo.bn[nb - 1], ws + lo.fa, (int64_t)B * T, I, 1, st));
    if (training) KWS_TRY(kws_gru_masks(ws + lo.gmx, ws + lo.gmh, B, I, H, DK_GRU_KEEP, seed, step, row_offset, st));
    return kws_gru_fwd_f32(ws + lo.fa, params + p.gW[0], params + p.gU[0], params + p.gb[0], params + p.gW[1], params + p.gU[1],
                           params + p.gb[1], training ? ws + lo.gmx : nullptr, training ? ws + lo.gmh : nullptr, ws + lo.gout,
                           training ? ws + lo.gsave : nullptr, ws + lo.gws, B, T, I, H, st);
  }
  // Flatten (one time step) -> Dropout -> Dense(H): the features are materialised for the GEMMs
  KWS_TRY(kws_bn_relu6_apply(ws + lo.y[nb - 1], ws + lo.bn[nb - 1], ws + lo.fa, B, p.D, 1, st));
  const float* feat = ws + lo.fa;
  if (training) {
    KWS_TRY(kws_dropout_fwd(ws + lo.fa, ws + lo.fd1, B, p.D, p.keep, seed, step, 1, row_offset, st));
    feat = ws + lo.fd1;
  }
  KWS_TRY(kws_gemm_nn_f32(feat, params + p.d1k, ws + lo.h, B, p.D, p.H, nullptr, st));
  return dk_bias_table(p.d1b >= 0 ? params + p.d1b : nullptr, p.H, ws + lo.tab, st);
}

// bias + relu6 + Dropout (layer 2) of the hidden layer, Dense + softmax (+ loss and its backward): the flat tail over (h, table)
kws_flat_tail_args dk_tail_args(const DkProgram& p, const DkLayout& lo, const float* params, float* ws, int B, float* probs) {
  kws_flat_tail_args t;
  memset(&t, 0, sizeof(t));
  if (p.gru) {   // Dense + softmax over the signed GRU output: the raw arm
    t.y = ws + lo.gout; t.Ng = 2 * p.gH; t.raw = 1;
    t.Wd = params + p.d2k; t.bd = params + p.d2b;
    t.probs = probs;
    t.B = B; t.D = 2 * p.gH; t.F = 2 * p.gH; t.NC = p.NC;
    t.keep_prob = 1.f;
    return t;
  }
  t.y = ws + lo.h; t.bn = ws + lo.tab; t.Ng = p.H;
  t.Wd = params + p.d2k; t.bd = params + p.d2b;
  t.probs = probs;
  t.B = B; t.D = p.H; t.F = p.H; t.NC = p.NC;
  t.keep_prob = p.keep;
  t.layer_id = 2;
  return t;
}

// conv_1d_simple: _reduce_conv(x, 32, 31, strides=16), _context_conv(x, 32, 3), then for F in 64 .. 224: _reduce_conv(x, F, 3) (stride 2),
// _context_conv(x, F, 3), all padding='valid' (model.py:142-146) -> Bidirectional(GRU(128)) -> Dense
int dk_build_simple(kws_net* n) {
  const kws_net_config_t& c = n->cfg;
  KWS_REQUIRE(c.input_size == 16000, "net: conv_1d_simple input_size %d (the reference's ladder ends in 10 time steps for 16000 samples)",
              c.input_size);
  DkProgram* p = new DkProgram();
  n->program.reset(p);
  p->net = n;
  p->NC = c.num_classes;
  p->gru = true;
  KerasNames kn{n};
  int L = c.input_size, cin = 1;
  for (int i = 0; i < 14; ++i) {
    SepBlock b;
    b.Lin = L; b.k = i == 0 ? 31 : 3; b.stride = i == 0 ? 16 : (i % 2 == 0 ? 2 : 1); b.cin = cin; b.cout = i < 2 ? 32 : 32 * (i / 2 + 1);
    KWS_REQUIRE(L >= b.k, "net: block %d input length %d < %d taps", i, L, b.k);
    b.Lout = (L - b.k) / b.stride + 1;
    b.pad_l = 0;
    b.dw = kn.dwk(b.k, cin);
    b.pw = kn.conv(1, cin, b.cout, KWS_L2_COEF);
    b.bn = kn.bn(b.cout);
    p->blocks.push_back(b);
    L = b.Lout;
    cin = b.cout;
  }
  KWS_REQUIRE(L == 10 && cin == 224, "net: conv_1d_simple ladder ends at [%d, %d], the GRU reads [10, 224]", L, cin);
  p->D = cin;
  p->gT = L;
  p->gH = DK_GRU_UNITS;
  const int H = p->gH;
  for (int d = 0; d < 2; ++d) {   // recurrent_kernel: Keras's Orthogonal initialiser, drawn by the host (fan_in = 0 here)
    const std::string base = std::string("bidirectional_1/") + (d ? "backward" : "forward") + "_gru_1/";
    p->gW[d] = kws_net_add_tensor(n, base + "kernel", {p->D, 3 * H}, false, 0.f, p->D, 3 * H, 0.f);
    p->gU[d] = kws_net_add_tensor(n, base + "recurrent_kernel", {H, 3 * H}, false, 0.f, 0, 0, 0.f);
    p->gb[d] = kws_net_add_tensor(n, base + "bias", {3 * H}, false, 0.f, 0, 0, 0.f);
  }
  p->d2k = kws_net_add_tensor(n, "dense_1/kernel", {2 * H, p->NC}, false, 0.f, 2 * H, p->NC, 0.f);
  p->d2b = kws_net_add_tensor(n, "dense_1/bias", {p->NC}, false, 0.f, 0, 0, 0.f);
  return KWS_OK;
}

}  // namespace

int dk_build(kws_net* n) {
  const kws_net_config_t& c = n->cfg;
  if (c.kind == KWS_NET_CONV_1D_SIMPLE) return dk_build_simple(n);
  KWS_REQUIRE(c.input_size == 16000, "net: conv_1d_gru input_size %d (the reference's ladder ends in one time step for 16000 samples)",
              c.input_size);
  DkProgram* p = new DkProgram();
  n->program.reset(p);
  p->net = n;
  p->NC = c.num_classes;
  p->keep = DK_DROP_KEEP;
  KerasNames kn{n};
  // _reduce_conv(x, F, k, strides) padding='same' x 5, _context_conv(x, 512, 8) padding='valid' (model.py:495-500)
  static const struct { int F, k, s; bool same; } spec[6] = {{128, 63, 16, true}, {256, 31, 4, true}, {384, 15, 4, true},
                                                             {448, 7, 4, true},   {512, 5, 2, true},  {512, 8, 1, false}};
  int L = c.input_size, cin = 1;
  for (int i = 0; i < 6; ++i) {
    SepBlock b;
    b.Lin = L; b.k = spec[i].k; b.stride = spec[i].s; b.cin = cin; b.cout = spec[i].F;
    if (spec[i].same) {
      kws_same_pad(L, b.k, b.stride, &b.Lout, &b.pad_l);
    } else {
      KWS_REQUIRE(L >= b.k, "net: block %d input length %d < %d taps", i, L, b.k);
      b.Lout = (L - b.k) / b.stride + 1;
      b.pad_l = 0;
    }
    b.dw = kn.dwk(b.k, cin);
    b.pw = kn.conv(1, cin, b.cout, KWS_L2_COEF);
    b.bn = kn.bn(b.cout);
    p->blocks.push_back(b);
    L = b.Lout;
    cin = b.cout;
  }
  KWS_REQUIRE(L == 1, "net: conv_1d_gru ladder ends with %d time steps, the head flattens 1", L);
  p->D = cin;
  p->H = DK_HIDDEN;
  p->d1k = kws_net_add_tensor(n, "dense_1/kernel", {p->D, p->H}, false, 0.f, p->D, p->H, 0.f);
  p->d1b = kws_net_add_tensor(n, "dense_1/bias", {p->H}, false, 0.f, 0, 0, 0.f);
  p->d2k = kws_net_add_tensor(n, "dense_2/kernel", {p->H, p->NC}, false, 0.f, p->H, p->NC, 0.f);
  p->d2b = kws_net_add_tensor(n, "dense_2/bias", {p->NC}, false, 0.f, 0, 0, 0.f);
  return KWS_OK;
}

namespace {

int64_t DkProgram::workspace_bytes(int B, int training) const {
  DkLayout lo;
  dk_layout(*this, B, training != 0, &lo);
  return lo.total;
}

int DkProgram::debug_view(int B, int training, int what, int index, int64_t* offset_floats, int64_t* count) const {
  const DkProgram& p = *this;
  DkLayout lo;
  dk_layout(p, B, training != 0, &lo);
  const int nb = (int)p.blocks.size();
  if (p.gru && what == 5) {   // the GRU's saved steps [2][4: z, r, c, h][B, T, H] (training)
    KWS_REQUIRE(training, "net_debug_view: view 5 exists in training only");
    *offset_floats = lo.gsave;
    *count = kws_gru_save_floats(B, p.gT, p.gH);
    return KWS_OK;
  }
  if (p.gru && what == 6) {   // the GRU output [B, 2H]
    *offset_floats = lo.gout;
    *count = (int64_t)B * 2 * p.gH;
    return KWS_OK;
  }
  if (what == 4 && !p.gru) {   // the hidden Dense layer's output before its bias [B, H]
    *offset_floats = lo.h;
    *count = (int64_t)B * p.H;
    return KWS_OK;
  }
  KWS_REQUIRE(index >= 0 && index < nb, "net_debug_view: block index %d", index);
  const SepBlock& b = p.blocks[index];
  if (what == 0) {          // raw pointwise output of block `index`
    *offset_floats = lo.y[index];
    *count = (int64_t)B * b.Lout * b.cout;
  } else if (what == 1) {   // depthwise output of block `index`
    *offset_floats = lo.z[index];
    *count = (int64_t)B * b.Lout * b.cin;
  } else if (what == 2) {   // table of batch_normalization_{index+1}
    *offset_floats = lo.bn[index];
    *count = (int64_t)4 * b.cout;
  } else {
    kws_set_error("net_debug_view: unknown view %d", what);
    return KWS_E_INVALID;
  }
  return KWS_OK;
}

int DkProgram::predict(const float* params, const float* state, const float* x, int B, float* probs, float* ws, int64_t ws_bytes,
                       hipStream_t st) const {
  DkLayout lo;
  dk_layout(*this, B, false, &lo);
  KWS_TRY(kws_workspace_check("net_predict", lo.total, ws_bytes, B));
  KWS_TRY(dk_forward(*this, lo, params, const_cast<float*>(state), x, B, false, ws, 0, 0, 0, st));
  kws_flat_tail_args t = dk_tail_args(*this, lo, params, ws, B, probs);
  return kws_flat_tail_launch(&t, 0, st);
}

int DkProgram::train(const float* params, float* state, const float* x, const float* y_onehot, int B, float* grads, float* probs,
                     float* metrics, uint64_t seed, uint32_t step, int64_t row_offset, int loss_batch, float* ws, int64_t ws_bytes,
                     hipStream_t st) const {
  const DkProgram& p = *this;
  DkLayout lo;
  dk_layout(p, B, true, &lo);
  KWS_TRY(kws_workspace_check("net_train_fwd_bwd", lo.total, ws_bytes, B));
  const int nb = (int)p.blocks.size();
  KWS_HIP(hipMemsetAsync(grads, 0, (size_t)net->n_params * 4, st));   // the padding behind a tensor of 63 taps stays zero
  KWS_TRY(dk_forward(p, lo, params, state, x, B, true, ws, seed, step, row_offset, st));
  float* G[2] = {ws + lo.G[0], ws + lo.G[1]};
  float* part = ws + lo.part;
  float* coef = ws + lo.coef;
  const SepBwdScratch scratch = {ws + lo.WT, ws + lo.DZ, ws + lo.tn, part, coef};
  // ---- head ----
  kws_flat_tail_args t = dk_tail_args(p, lo, params, ws, B, probs);
  KWS_TRY(kws_flat_tail_train(&t, y_onehot, ws + lo.fd, ws + lo.dl, p.gru ? ws + lo.gdout : G[0], ws + lo.per_loss, ws + lo.per_correct,
                              seed, step, loss_batch, row_offset, metrics, st));
  int cur = 0;   // G[cur] = gradient wrt the activated output of the last block [B, T, D]
  if (p.gru) {
    const int T = p.gT, I = p.D, H = p.gH;
    const SepBlock& b = p.blocks[nb - 1];
    KWS_TRY(kws_small_wgrad_launch(ws + lo.fd, ws + lo.dl, grads + p.d2k, grads + p.d2b, B, 2 * H, p.NC, ws + lo.swg, st));
    KWS_TRY(kws_gru_bwd_f32(ws + lo.gdout, ws + lo.fa, params + p.gW[0], params + p.gU[0], params + p.gW[1], params + p.gU[1], ws + lo.gmx,
                            ws + lo.gmh, ws + lo.gsave, G[0], grads + p.gW[0], grads + p.gU[0], grads + p.gb[0], grads + p.gW[1],
                            grads + p.gU[1], grads + p.gb[1], ws + lo.gws, B, T, I, H, st));
    KWS_TRY(kws_gbn_layer_bwd(G[cur], ws + lo.y[nb - 1], ws + lo.bn[nb - 1], nullptr, (int64_t)B * T, kws_gbn_grouped(1, b.cout), part,
                              coef, grads, b.bn, st));
  } else {
    KWS_TRY(kws_small_wgrad_launch(ws + lo.fd, ws + lo.dl, grads + p.d2k, grads + p.d2b, B, p.H, p.NC, ws + lo.swg, st));
    // G[0] = gradient wrt relu6(h + b1) [B, H] -> wrt h; dense_1's gradients; back through Dropout(.3) onto the activated features
    KWS_TRY(dk_bias_relu6_bwd(G[0], ws + lo.h, p.d1b >= 0 ? params + p.d1b : nullptr, p.d1b >= 0 ? grads + p.d1b : nullptr, B, p.H,
                              ws + lo.bpart, st));
    KWS_TRY(kws_gemm_tn_f32(ws + lo.fd1, G[0], grads + p.d1k, B, p.D, p.H, ws + lo.tn, st));
    KWS_TRY(kws_transpose_f32(params + p.d1k, ws + lo.WT, p.D, p.H, st));
    KWS_TRY(kws_gemm_nn_f32(G[0], ws + lo.WT, G[1], B, p.H, p.D, nullptr, st));
    KWS_TRY(kws_dropout_bwd(G[1], G[0], B, p.D, p.keep, seed, step, 1, row_offset, st));
    const SepBlock& b = p.blocks[nb - 1];
    KWS_TRY(kws_gbn_layer_bwd(G[cur], ws + lo.y[nb - 1], ws + lo.bn[nb - 1], nullptr, B, kws_gbn_grouped(1, b.cout), part, coef, grads,
                              b.bn, st));
  }
  // ---- blocks: G[cur] = dy of block i's pointwise output ----
  for (int i = nb - 1; i >= 1; --i) {
    const SepBlock& b = p.blocks[i];
    KWS_TRY(kws_sep_bwd(b, params, grads, G[cur], ws + lo.z[i], ws + lo.y[i - 1], ws + lo.bn[i - 1], &p.blocks[i - 1].bn, G[cur ^ 1],
                        scratch, B, st));
    cur ^= 1;
  }
  {   // block 1: the outer product's backward, then the taps of the one-channel depthwise layer (no gradient leaves the input)
    const SepBlock& b = p.blocks[0];
    const int64_t M = (int64_t)B * b.Lout;
    KWS_TRY(kws_dwconvk_pw1_bwd_f32(G[cur], ws + lo.z[0], params + b.pw, scratch.DZ, grads + b.pw, M, b.cout, ws + lo.pw1ws, st));
    KWS_TRY(kws_sep_dw_bwd(b, params, grads, x, nullptr, nullptr, G[cur ^ 1], scratch, B, st));
  }
  return KWS_OK;
}

}  // namespace
