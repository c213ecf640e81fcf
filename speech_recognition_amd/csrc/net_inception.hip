// Network program of KWS_NET_INCEPTION_D1: conv_inception_d1_model (reference model.py:312-406).
//   raw waveform as [800, 20] -> Conv1D(32, 1) -> three pairs of a stride-1 _reduce_conv (k 3 VALID + MaxPool1D(3, 2, 'valid')) and
//   a _context_conv (k 3 VALID), 64 / 128 / 256 filters -> [93, 256]
//   -> _inception_block x 2 (dilation 2) -> _reduce_inception_block -> [47, 496] -> blocks (2), (1) -> reduce -> [24, 496]
//   -> blocks (1), (1) -> reduce -> [12, 496] -> blocks (1), (1) -> reduce -> [6, 496]
//   -> Dropout(.2) -> Conv1D(num_classes, 6, softmax, bias) = the flat tail with D = 2976.  Adam(1e-3), categorical CE.
// Every convolution is use_bias=False, l2 1e-5, followed by its own BatchNormalization and relu6.
//
// The program is a list of operations over a list of tensors, run forwards and then backwards:
//   * a tensor is [B, L, C] in the workspace.  A RAW tensor holds convolution outputs before their BatchNorm and carries one
//     table [4][C] (scale|shift|mean|rstd) that its consumers apply on load - the project's convention; the output of an
//     inception block is such a tensor whose four column slices were written by four convolutions (kws_conv1d_*'s y0 window),
//     each BatchNorm filling its columns of the composite table.  An ACTIVATED tensor (the output of a pool; the output of a
//     reduce block, whose three slices all come out of max pools) is read as it is.
//   * the stem is the one-group kws_gconv_* ladder with kws_pool3s2_*; the blocks run kws_conv1d_* (SAME, dilation 1 or 2),
//     kws_avgpool3_same_* and kws_pool3s2_same_* (through the pitch launchers: the pooled rows are a slice of the joined tensor).
//   * backward: every tensor has a gradient buffer of its shape holding the gradient wrt its ACTIVATED value.  The consumers of
//     a tensor add into it in the reverse of the forward order, which is fixed: the first overwrites, the others accumulate
//     (one thread per element, no atomics).  The relu6 gate and the BatchNorm backward are applied once, by the convolution that
//     produced the columns, in place on its window (kws_gbn_bwd), or by the max pool behind a pooled convolution
//     (kws_pool3s2*_bwd gates and leaves the BatchNorm sums; kws_gbn_bwd_finish ends it).  The SAME max pool that reads a block's
//     raw input hands back an already gated gradient: it goes to a buffer of its own and is added behind the gate.
// The three sibling 1x1 convolutions of a block stay three launches, each writing where its consumer reads.
#include "net_internal.h"

namespace {

constexpr float INC_DROP_KEEP = 0.8f;   // Dropout(0.2), model.py:397
constexpr int INC_BASE = 32;            // base_num of every block

// the table of an activated tensor for a consumer that wants one (the flat tail): relu6(1 * v + 0) = v for v in [0, 6]
__global__ __launch_bounds__(256) void inc_identity_table_kernel(float* __restrict__ bn, int C) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  bn[c] = 1.f;
  bn[C + c] = 0.f;
  bn[2 * C + c] = 0.f;
  bn[3 * C + c] = 1.f;
}

// ---- the program --------------------------------------------------------------------------------------------------------------
struct IncTensor {
  int L, C;
  bool raw;    // convolution outputs before their BatchNorm: read through the table [4][C]
  bool gadd;   // a SAME max pool reads this raw tensor: its gated gradient arrives in a buffer of its own
};

enum { OP_GCONV, OP_CONV, OP_MAXV, OP_MAXS, OP_AVG };

struct IncOp {
  int kind;
  int in, out;           // tensor ids
  int y0, F;             // the column window of `out` this operation writes (pools: F = the input's channels)
  int k, dil, pad_l;     // convolutions
  int64_t w;             // kernel (params)
  BnRef bn;
  int prod;              // max pools: the convolution operation whose output they pool (-1: a block's input)
  bool pooled;           // convolutions: a max pool follows and does the gate and the BatchNorm sums
  bool acc, need_dx;     // backward: adds to the input's gradient (another consumer wrote it first) / has one to write
};

struct IncLayout {
  int64_t total = 0;
  std::vector<int64_t> buf, bn, grad, gadd;
  int64_t stats = 0, part = 0, coef = 0, wws = 0, ident = 0;
  FlatTailWs tail;
};

struct IncProgram : FlatTailProgram<IncLayout> {
  std::vector<IncTensor> tensors;   // 0 = the network input [800, 20]
  std::vector<IncOp> ops;
  std::vector<int> convs;           // operation of Conv1D i (Keras creation order; BatchNormalization i + 1 is behind it)
  int top = 0;                      // the tensor the tail reads

  kws_gconv_t gdesc(const IncOp& o, int B) const;
  kws_conv1d_t cdesc(const IncOp& o, int B) const;
  void layout(int B, bool training, IncLayout* lo) const override;
  int forward(const IncLayout& lo, const NetCall& c) const override;
  kws_flat_tail_args tail_args(const IncLayout& lo, const NetCall& c, float* probs) const override;
  int64_t tail_grad(const IncLayout& lo) const override { return lo.grad[top]; }
  int backward(const IncLayout& lo, const NetCall& c) const override;
  int debug_view(int B, int training, int what, int index, int64_t* offset_floats, int64_t* count) const override;
};

kws_gconv_t IncProgram::gdesc(const IncOp& o, int B) const {
  kws_gconv_t d;
  memset(&d, 0, sizeof(d));
  d.B = B; d.L = tensors[o.in].L; d.C = tensors[o.in].C; d.Lout = tensors[o.out].L; d.k = o.k; d.stride = 1;
  d.g = 1; d.gs = d.C; d.Ng = o.F;
  return d;
}

kws_conv1d_t IncProgram::cdesc(const IncOp& o, int B) const {
  kws_conv1d_t d;
  d.B = B; d.L = tensors[o.in].L; d.Lout = tensors[o.out].L; d.k = o.k; d.dil = o.dil; d.pad_l = o.pad_l;
  d.Cx = tensors[o.in].C; d.x0 = 0; d.Cin = d.Cx;
  d.Cy = tensors[o.out].C; d.y0 = o.y0; d.F = o.F;
  return d;
}

void IncProgram::layout(int B, bool training, IncLayout* lo) const {
  Bump bp;
  const int nt = (int)tensors.size();
  lo->buf.assign(nt, 0);
  lo->bn.assign(nt, 0);
  lo->grad.assign(nt, 0);
  lo->gadd.assign(nt, 0);
  for (int i = 1; i < nt; ++i) {
    const int64_t n = (int64_t)B * tensors[i].L * tensors[i].C;
    lo->buf[i] = bp.take(n);
    if (tensors[i].raw) lo->bn[i] = bp.take((int64_t)4 * tensors[i].C);
    if (training) {
      lo->grad[i] = bp.take(n);
      if (tensors[i].gadd) lo->gadd[i] = bp.take(n);
    }
  }
  int64_t max_stats = 64, max_part = 64, max_coef = 64, max_wws = 64;
  for (const IncOp& o : ops) {
    const IncTensor& ti = tensors[o.in];
    if (o.kind == OP_GCONV || o.kind == OP_CONV) {
      const int64_t M = (int64_t)B * tensors[o.out].L;
      max_stats = std::max(max_stats, ceil_div64(M, 128) * 2 * o.F);
      max_part = std::max(max_part, (int64_t)kws_gbn_bwd_rows(M) * 2 * o.F);
      max_coef = std::max(max_coef, (int64_t)2 * o.F);
      if (o.kind == OP_GCONV) {
        const kws_gconv_t d = gdesc(o, B);
        max_wws = std::max(max_wws, kws_gconv_wgrad_workspace_floats(&d));
      } else {
        const kws_conv1d_t d = cdesc(o, B);
        max_wws = std::max(max_wws, kws_conv1d_wgrad_workspace_floats(&d));
      }
    } else if (o.kind == OP_MAXV) {
      max_part = std::max(max_part, kws_pool3s2_bwd_part_floats(B, ti.L, ti.C));
    } else if (o.kind == OP_MAXS) {
      max_part = std::max(max_part, kws_pool3s2_same_bwd_part_floats(B, ti.L, ti.C));
    }
  }
  lo->stats = bp.take(max_stats);
  lo->ident = bp.take((int64_t)4 * tensors[top].C);
  if (training) {
    lo->part = bp.take(max_part);
    lo->coef = bp.take(max_coef);
    lo->wws = bp.take(max_wws);
    lo->tail.take(bp, B, dense.D, dense.NC);
  }
  lo->total = bp.cur * 4;
}

int IncProgram::forward(const IncLayout& lo, const NetCall& c) const {
  const float* params = c.params;
  float* state = c.state;
  const float* x = c.x;
  float* ws = c.ws;
  const int B = c.B;
  const bool training = c.training;
  hipStream_t st = c.st;
  for (const IncOp& o : ops) {
    const IncTensor& ti = tensors[o.in];
    const IncTensor& to = tensors[o.out];
    const float* in = o.in == 0 ? x : ws + lo.buf[o.in];
    const float* bn_in = ti.raw ? ws + lo.bn[o.in] : nullptr;
    float* out = ws + lo.buf[o.out];
    // the BatchNorm behind a convolution fills its columns of the output tensor's table from the rows of sums in lo.stats
    const auto bn_table = [&](int stats_rows) {
      const kws_gbn_cols w = kws_gbn_window(to.C, o.y0, o.F);
      const kws_gbn_refs r = kws_gbn_layer_refs(o.bn, params, state);
      if (!training) return kws_gbn_infer(&w, &r, KWS_BN_EPS, ws + lo.bn[o.out], st);
      return kws_gbn_finalize(ws + lo.stats, stats_rows, (int64_t)B * to.L, &w, &r, KWS_BN_EPS, KWS_BN_MOMENTUM, ws + lo.bn[o.out], st);
    };
    switch (o.kind) {
      case OP_GCONV: {
        const kws_gconv_t d = gdesc(o, B);
        KWS_TRY(kws_gconv_fwd_f32(in, bn_in, d.C, params + o.w, out, training ? ws + lo.stats : nullptr, &d, st));
        KWS_TRY(bn_table(kws_gconv_stats_rows(&d)));
        break;
      }
      case OP_CONV: {
        const kws_conv1d_t d = cdesc(o, B);
        KWS_TRY(kws_conv1d_fwd_f32(in, bn_in, params + o.w, out, training ? ws + lo.stats : nullptr, &d, st));
        KWS_TRY(bn_table(kws_conv1d_stats_rows(&d)));
        break;
      }
      case OP_MAXV:
        KWS_TRY(kws_pool3s2_fwd_f32(in, bn_in, out, B, ti.L, ti.C, st));
        break;
      case OP_MAXS:
        KWS_TRY(kws_pool3s2_same_fwd_pitch(in, bn_in, out + o.y0, to.C, B, ti.L, ti.C, st));
        break;
      case OP_AVG:
        KWS_TRY(kws_avgpool3_same_fwd_f32(in, bn_in, out, B, ti.L, ti.C, st));
        break;
    }
  }
  hipLaunchKernelGGL(inc_identity_table_kernel, dim3((unsigned)ceil_div(tensors[top].C, 256)), dim3(256), 0, st, ws + lo.ident,
                     tensors[top].C);
  KWS_LAUNCH_CHECK("inc_identity_table_kernel");
  return KWS_OK;
}

kws_flat_tail_args IncProgram::tail_args(const IncLayout& lo, const NetCall& c, float* probs) const {
  kws_flat_tail_args t;
  memset(&t, 0, sizeof(t));
  t.y = c.ws + lo.buf[top]; t.bn = c.ws + lo.ident; t.Ng = tensors[top].C;
  t.Wd = c.params + dense.kernel; t.bd = c.params + dense.bias;
  t.probs = probs;
  t.B = c.B; t.D = dense.D; t.F = tensors[top].C; t.NC = dense.NC;
  t.keep_prob = INC_DROP_KEEP;
  t.layer_id = 1;
  return t;
}

// ---- the table builder ---------------------------------------------------------------------------------------------------------
struct IncBuilder {
  IncProgram* p;
  KerasNames kn;

  int tensor(int L, int C, bool raw) {
    p->tensors.push_back(IncTensor{L, C, raw, false});
    return (int)p->tensors.size() - 1;
  }
  // Conv1D(F, k, dilation_rate=dil, padding, use_bias=False, l2 1e-5) + BatchNormalization (+ relu6 on load) from tensor `in`
  // into the columns [y0, y0 + F) of `out` (-1: a tensor of its own)
  int conv(int kind, int in, int out, int y0, int F, int k, int dil, bool same, bool pooled = false) {
    const IncTensor ti = p->tensors[in];
    const int span = dil * (k - 1);
    const int Lout = same ? ti.L : ti.L - span;
    if (out < 0) out = tensor(Lout, F, true);
    IncOp o;
    memset(&o, 0, sizeof(o));
    o.kind = kind; o.in = in; o.out = out; o.y0 = y0; o.F = F; o.k = k; o.dil = dil;
    o.pad_l = same ? span / 2 : 0;   // TF SAME at stride 1: dil * (k - 1) zeros in all, the smaller half in front
    o.w = kn.conv(k, ti.C, F, KWS_L2_COEF);
    o.bn = kn.bn(F);
    o.prod = -1;
    o.pooled = pooled;
    p->convs.push_back((int)p->ops.size());
    p->ops.push_back(o);
    return out;
  }
  // MaxPool1D(3, 2, 'valid' / 'same') of tensor `in` into the columns from y0 of `out` (-1: a tensor of its own)
  int maxpool(int kind, int in, int out, int y0, int prod) {
    const IncTensor ti = p->tensors[in];
    if (out < 0) out = tensor(kind == OP_MAXV ? kws_pool3s2_out_len(ti.L) : kws_pool3s2_same_out_len(ti.L), ti.C, false);
    IncOp o;
    memset(&o, 0, sizeof(o));
    o.kind = kind; o.in = in; o.out = out; o.y0 = y0; o.F = ti.C; o.prod = prod;
    if (prod < 0) p->tensors[in].gadd = true;
    p->ops.push_back(o);
    return out;
  }
  int last_conv() const { return p->convs.back(); }

  int inception_block(int x, int dil) {
    const int L = p->tensors[x].L, b = INC_BASE;
    const int J = tensor(L, 2 * b + 2 * b + 3 * b + b, true);
    conv(OP_CONV, x, J, 0, 2 * b, 1, 1, true);                       // branch1x1
    int h = conv(OP_CONV, x, -1, 0, 3 * b / 2, 1, 1, true);          // branch5x5: 1x1 -> 3 taps, dilation 2 (always)
    conv(OP_CONV, h, J, 2 * b, 2 * b, 3, 2, true);
    h = conv(OP_CONV, x, -1, 0, 2 * b, 1, 1, true);                  // branch3x3dbl
    h = conv(OP_CONV, h, -1, 0, 3 * b, 3, dil, true);
    conv(OP_CONV, h, J, 4 * b, 3 * b, 3, dil, true);
    const int z = tensor(L, p->tensors[x].C, false);                 // branch_pool
    IncOp o;
    memset(&o, 0, sizeof(o));
    o.kind = OP_AVG; o.in = x; o.out = z; o.F = p->tensors[x].C; o.prod = -1;
    p->ops.push_back(o);
    conv(OP_CONV, z, J, 7 * b, b, 1, 1, true);
    return J;
  }
  int reduce_block(int x) {
    const IncTensor tx = p->tensors[x];
    const int b = INC_BASE, Lp = kws_pool3s2_same_out_len(tx.L);
    const int J = tensor(Lp, 6 * b + 3 * b / 2 + tx.C, false);
    int y = conv(OP_CONV, x, -1, 0, 6 * b, 3, 1, true, true);        // branch3x3
    maxpool(OP_MAXS, y, J, 0, last_conv());
    int h = conv(OP_CONV, x, -1, 0, b, 1, 1, true);                  // branch3x3dbl
    h = conv(OP_CONV, h, -1, 0, 3 * b / 2, 3, 1, true);
    y = conv(OP_CONV, h, -1, 0, 3 * b / 2, 3, 1, true, true);
    maxpool(OP_MAXS, y, J, 6 * b, last_conv());
    maxpool(OP_MAXS, x, J, 6 * b + 3 * b / 2, -1);                   // branch_pool
    return J;
  }
};

}  // namespace

int inc_build(kws_net* n) {
  const kws_net_config_t& c = n->cfg;
  IncProgram* p = new IncProgram();
  n->program.reset(p);
  p->net = n;
  KWS_REQUIRE(c.input_size == 16000, "net: inception_d1 input_size %d (the reference reshapes 16000 samples)", c.input_size);
  const int NC = p->dense.NC = c.num_classes;
  IncBuilder b{p, KerasNames{n}};
  int x = b.tensor(800, 20, false);   // Reshape([800, 20])
  x = b.conv(OP_GCONV, x, -1, 0, 32, 1, 1, false);
  const int widths[3] = {64, 128, 256};
  for (int i = 0; i < 3; ++i) {       // _reduce_conv (stride 1; its strides argument goes to the pool only), _context_conv
    x = b.conv(OP_GCONV, x, -1, 0, widths[i], 3, 1, false, true);
    x = b.maxpool(OP_MAXV, x, -1, 0, b.last_conv());
    x = b.conv(OP_GCONV, x, -1, 0, widths[i], 3, 1, false);
  }
  const int dils[4][2] = {{2, 2}, {2, 1}, {1, 1}, {1, 1}};
  for (int s = 0; s < 4; ++s) {
    x = b.inception_block(x, dils[s][0]);
    x = b.inception_block(x, dils[s][1]);
    KWS_REQUIRE(p->tensors[x].raw, "net: a reduce block pools a raw tensor");
    x = b.reduce_block(x);
  }
  p->top = x;
  const IncTensor& top = p->tensors[x];
  KWS_REQUIRE(top.L == 6 && top.C == 496, "net: inception_d1 ends with [%d, %d], the head convolves [6, 496]", top.L, top.C);
  p->dense.D = top.L * top.C;
  p->dense.kernel = b.kn.conv(top.L, top.C, NC, 0.f);   // [6, 496, NC] = the Dense kernel [2976, NC] over the t-major flatten
  p->dense.bias = kws_net_add_tensor(n, "conv1d_" + std::to_string(b.kn.n_conv) + "/bias", {NC}, false, 0.f, 0, 0, 0.f);
  // backward plan: the consumers of a tensor write its gradient in the reverse of the forward order; the first overwrites
  std::vector<char> written(p->tensors.size(), 0);
  for (int i = (int)p->ops.size() - 1; i >= 0; --i) {
    IncOp& o = p->ops[i];
    o.need_dx = o.in != 0;
    if (!o.need_dx || (o.kind == OP_MAXS && o.prod < 0)) continue;   // (that pool's gradient goes to the tensor's second buffer)
    o.acc = written[o.in] != 0;
    written[o.in] = 1;
    KWS_REQUIRE(!o.acc || o.kind == OP_CONV || o.kind == OP_AVG, "net: operation %d cannot accumulate", i);
  }
  for (size_t t = 1; t < p->tensors.size(); ++t)
    KWS_REQUIRE(written[t] || (int)t == p->top, "net: tensor %d has no consumer", (int)t);
  return KWS_OK;
}

namespace {

int IncProgram::debug_view(int B, int training, int what, int index, int64_t* offset_floats, int64_t* count) const {
  IncLayout lo;
  layout(B, training != 0, &lo);
  KWS_REQUIRE(what == 0 || what == 2 || what == 3, "net_debug_view: unknown view %d", what);
  KWS_REQUIRE(index >= 0 && index < (int)convs.size(), "net_debug_view: Conv1D index %d", index);
  const IncOp& o = ops[convs[index]];
  const IncTensor& t = tensors[o.out];
  if (what == 0) {          // raw output of Conv1D `index`: a column window, from its first to its last element
    *offset_floats = lo.buf[o.out] + o.y0;
    *count = ((int64_t)B * t.L - 1) * t.C + o.F;
  } else if (what == 2) {   // table of batch_normalization_{index+1}: four rows one pitch apart
    *offset_floats = lo.bn[o.out] + o.y0;
    *count = (int64_t)3 * t.C + o.F;
  } else {                  // geometry: row pitch, filters
    *offset_floats = t.C;
    *count = o.F;
  }
  return KWS_OK;
}

// the operations in descending order
int IncProgram::backward(const IncLayout& lo, const NetCall& c) const {
  const float* params = c.params;
  const float* x = c.x;
  float* grads = c.grads;
  float* ws = c.ws;
  const int B = c.B;
  hipStream_t st = c.st;
  float* part = ws + lo.part;
  float* coef = ws + lo.coef;
  for (int i = (int)ops.size() - 1; i >= 0; --i) {
    const IncOp& o = ops[i];
    const IncTensor& ti = tensors[o.in];
    const IncTensor& to = tensors[o.out];
    const float* in = o.in == 0 ? x : ws + lo.buf[o.in];
    const float* bn_in = ti.raw ? ws + lo.bn[o.in] : nullptr;
    float* d_in = o.need_dx ? ws + lo.grad[o.in] : nullptr;
    float* d_out = ws + lo.grad[o.out];
    const int64_t M = (int64_t)B * to.L;
    switch (o.kind) {
      case OP_GCONV:
      case OP_CONV: {
        // d_out's window: the gradient wrt the activated output, or (pooled) dy already
        if (!o.pooled)
          KWS_TRY(kws_gbn_layer_bwd(d_out, ws + lo.buf[o.out], ws + lo.bn[o.out], to.gadd ? ws + lo.gadd[o.out] : nullptr, M,
                                    kws_gbn_window(to.C, o.y0, o.F), part, coef, grads, o.bn, st));
        if (o.kind == OP_GCONV) {
          const kws_gconv_t d = gdesc(o, B);
          KWS_TRY(kws_gconv_wgrad_f32(in, bn_in, d.C, d_out, grads + o.w, ws + lo.wws, &d, st));
          if (o.need_dx) KWS_TRY(kws_gconv_dgrad_f32(d_out, params + o.w, d_in, &d, st));
        } else {
          const kws_conv1d_t d = cdesc(o, B);
          KWS_TRY(kws_conv1d_wgrad_f32(in, bn_in, d_out, grads + o.w, ws + lo.wws, &d, st));
          if (o.need_dx) KWS_TRY(kws_conv1d_dgrad_f32(d_out, params + o.w, d_in, o.acc ? 1 : 0, &d, st));
        }
        break;
      }
      case OP_MAXV:
      case OP_MAXS: {
        // route the pooled gradient to the winners and gate it; a pooled convolution's BatchNorm backward ends here
        float* g = o.prod >= 0 ? d_in : ws + lo.gadd[o.in];
        int rows;
        if (o.kind == OP_MAXV) {
          KWS_TRY(kws_pool3s2_bwd_f32(d_out, in, bn_in, g, part, B, ti.L, ti.C, st));
          rows = kws_pool3s2_bwd_part_rows(B, ti.L, ti.C);
        } else {
          KWS_TRY(kws_pool3s2_same_bwd_pitch(d_out + o.y0, to.C, in, bn_in, g, part, B, ti.L, ti.C, st));
          rows = kws_pool3s2_same_bwd_part_rows(B, ti.L, ti.C);
        }
        if (o.prod >= 0) {
          KWS_TRY(kws_gbn_layer_bwd_finish(g, in, bn_in, (int64_t)B * ti.L, kws_gbn_grouped(1, ti.C), part, rows, coef, grads,
                                           ops[o.prod].bn, st));
        }
        break;
      }
      case OP_AVG:
        KWS_TRY(kws_avgpool3_same_bwd_f32(d_out, d_in, o.acc ? 1 : 0, B, ti.L, ti.C, st));
        break;
    }
  }
  return KWS_OK;
}

}  // namespace
