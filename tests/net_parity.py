"""The harness of the GPU parity files.  A plain module like grouped_oracle.py: no fixtures, and no checker has default bars.

What every family shares: the weight perturbation of an oracle / device pair (perturb, device_pair), the waveform batch, the
read-back of the device's ReLU6 decisions and pool winners (relu_masks, gates_and_winners), one training step as plain host data
(device_step) and its comparison with the oracle (check_train_step), and the CPU files' read-out of a net's native tensor table.
The ten family model files (test_{grouped,stacked,dwk,gru,time_sliced,mts,learned_spec,xception,inception,conv2d}_models_gpu.py)
also share their bars (FAMILY_BARS) and the smaller comparisons below; each keeps its oracle, its net kind, its own read-back, its
parametrisations and its mutations.

One comparison, two entrances.  check_train_step works on plain data, so tests/test_net_parity_cpu.py can show without a device
that it refuses what it should.  The residual-family files (test_logmfcc_gpu, test_steffe_gpu, test_residual_gpu,
test_mfcc_and_raw_gpu) enter through check_residual_step: their oracles' gradients carry the L2 term, which the device leaves
to its optimizer, they check the moving means only, and each file states its own bars; the adapter takes the L2 term out, names
those bars and hands the step to the same comparison."""
import ctypes

import numpy as np

import pool_oracle

# predict: probabilities; train_probs / loss: one training step's probabilities and mean loss; grad: every gradient relative to
# its tensor's maximum; moving_mean / moving_variance: (atol, rtol) of the updated statistics.  Indices and counts are exact.
FAMILY_BARS = {'predict': 2e-5, 'train_probs': 5e-5, 'loss': 1e-4, 'grad': 2e-4,
               'moving_mean': (5e-6, 1e-5), 'moving_variance': (5e-6, 1e-5)}
MUTATED_ORACLE_BAR = 1e-2      # what the device's gradients miss a deliberately wrong oracle by, at the least
BN_MOMENTUM_STEP = 0.01        # moving' = moving - (moving - batch) * 0.01


def native_table(kind, nc=12, input_size=16000, filter_mult=1, spectrogram_length=0, num_features=0):
    """The tensor table (a list of _lib.TensorInfo) of a net created for this configuration and destroyed again"""
    from speech_recognition_amd import _lib
    lib = _lib.load()
    cfg = _lib.NetConfig(kind, nc, filter_mult, input_size, spectrogram_length, num_features)
    h = ctypes.c_void_p()
    _lib.check(lib.kws_net_create(ctypes.byref(cfg), ctypes.byref(h)), "kws_net_create")
    out = []
    try:
        for i in range(lib.kws_net_num_tensors(h)):
            ti = _lib.TensorInfo()
            _lib.check(lib.kws_net_tensor_info(h, i, ctypes.byref(ti)), "kws_net_tensor_info")
            out.append(ti)
    finally:
        lib.kws_net_destroy(h)
    return out


def perturb(ora, seed, negative_fraction=0.0, beta=(0.0, 0.1), bias=0.1, state=True, bias_names=None):
    """Moves BN scales (1 + 0.1 n, about a negative_fraction of them negative - asserted), shifts (beta[0] + beta[1] n), biases
    (bias n; None: left alone; bias_names: only those) and, with `state`, the moving statistics off their initial 1 / 0 so that a
    mix-up shows."""
    rng = np.random.RandomState(seed)
    for k in ora.params:
        shape = ora.params[k].shape
        if k.endswith('gamma'):
            g = 1.0 + 0.1 * rng.randn(*shape)
            if negative_fraction:
                g = g * np.where(rng.rand(*shape) < negative_fraction, -1.0, 1.0)
            ora.params[k] = g.astype(np.float32)
        if k.endswith('beta'):
            ora.params[k] = (beta[0] + beta[1] * rng.randn(*shape)).astype(np.float32)
        if k.endswith('bias') and bias is not None and (bias_names is None or k in bias_names):
            ora.params[k] = (bias * rng.randn(*shape)).astype(np.float32)
    for k in ora.state if state else ():
        if k.endswith('moving_mean'):
            ora.state[k] = (0.05 * rng.randn(*ora.state[k].shape)).astype(np.float32)
        else:
            ora.state[k] = (1.0 + 0.2 * rng.rand(*ora.state[k].shape)).astype(np.float32)
    if negative_fraction:
        assert any((v < 0).any() for k, v in ora.params.items() if k.endswith('gamma'))


def device_pair(ora, kind, num_classes=12, **config):
    """(ora, a DeviceNet of this kind and configuration holding the oracle's parameters and state)"""
    from speech_recognition_amd.net import DeviceNet
    net = DeviceNet(kind, num_classes, **config)
    net.set_weights(dict(ora.params, **ora.state))
    return ora, net


def waveform_batch(B, nc, seed, L=16000):
    """Noise at the data set's level plus a sine whose frequency names the label: ([B, L] f32, one-hot [B, nc] f32)."""
    rng = np.random.RandomState(seed)
    lab = rng.randint(0, nc, B)
    t = np.arange(L) / 16000.0
    x = rng.randn(B, L) * 0.0774 + 0.05 * np.sin(2 * np.pi * 200.0 * (1 + lab)[:, None] * t[None, :])
    return x.astype(np.float32), np.eye(nc, dtype=np.float32)[lab]


def relu_masks(net, B, shapes, y_views=None):
    """ReLU6 masks per BN index from the device tensors of the last training pass, in the f32 math of the kernels
    (pre = fmaf(y, scale, shift)).  shapes {bn index: (B, L, C)} names the activated BatchNorms; a layer's input y is
    debug_view(B, 0, idx) unless y_views[idx] = (what, index) says otherwise.  Returns (masks, pre-activations)."""
    masks, pre_of = {}, {}
    for idx, shp in shapes.items():
        C = shp[2]
        bn = net.debug_view(B, 2, idx)
        y = net.debug_view(B, *(y_views or {}).get(idx, (0, idx))).reshape(shp)
        pre = (y.astype(np.float64) * bn[:C].astype(np.float64) + bn[C:2 * C].astype(np.float64)).astype(np.float32)
        masks[idx] = ((pre > 0) & (pre <= 6)).astype(np.float64)
        pre_of[idx] = pre
    return masks, pre_of


def gates_and_winners(net, B, layers):
    """The ReLU6 gates and MaxPool1D(3, 2) winners of nets whose layer `idx` (1-based) has views idx - 1.  layers: (idx, Lout,
    F, pool) with pool None or (windows, pad_left).  -> (masks, winners), keyed by idx as the oracles take them."""
    masks, pre = relu_masks(net, B, {idx - 1: (B, Lout, F) for idx, Lout, F, _ in layers})
    inds = {idx: pool_oracle.argmax(np.clip(pre[idx - 1], 0, 6).astype(np.float64), *pool) for idx, _, _, pool in layers if pool}
    return {i + 1: m for i, m in masks.items()}, inds


def device_step(net, x, y, seed, step, row_offset=0):
    """One net.train_fwd_bwd as plain host data: probabilities, metrics, gradients and weights as NumPy.  The net's debug views
    are those of this step afterwards."""
    import torch
    probs = net.train_fwd_bwd(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), seed=seed, step=step, row_offset=row_offset)
    torch.cuda.synchronize()
    return host_step(net, probs)


def host_step(net, probs):
    return {'probs': probs.cpu().numpy(), 'metrics': net.metrics.cpu().numpy(), 'grads': net.grads_dict(), 'weights': net.get_weights()}


def grad_errors(g, grads):
    """max |g - reference| of every reference tensor, relative to that tensor's maximum (floor 1e-7)"""
    return {k: np.abs(np.asarray(g[k], np.float64) - np.asarray(r, np.float64).reshape(np.shape(g[k]))).max() /
            max(np.abs(r).max(), 1e-7) for k, r in grads.items()}


def check_train_step(dev, y, ref, ora, bars, tag, lead=''):
    """dev = device_step(...) against ref = (loss, p, grads, cache) = ora.loss_and_grads(...) taken on the device's own decisions:
    probabilities and their argmax, mean loss, the correct count, every gradient relative to its tensor's maximum, and each
    moving statistic that `bars` names, from ora.state and the batch statistics in cache.  Prints one line; -> the gradient
    errors."""
    loss, p, grads, cache = ref
    B = y.shape[0]
    got, m = dev['probs'], dev['metrics']
    errs = grad_errors(dev['grads'], grads)
    worst = max(errs, key=errs.get)
    print("train %s: %sprobs %.3g, loss %.3g, worst gradient %s %.3g" %
          (tag, lead, np.abs(got - p).max(), abs(m[0] / B - loss), worst, errs[worst]))
    assert np.abs(got - p).max() < bars['train_probs']
    assert np.array_equal(got.argmax(1), p.argmax(1))
    assert abs(m[0] / B - loss) < bars['loss']
    assert m[1] == (p.argmax(1) == y.argmax(1)).sum()
    for k, err in errs.items():
        assert err < bars['grad'], (k, err)
    for idx, stats in cache['batch_stats'].items():
        for nm, batch in zip(('moving_mean', 'moving_variance'), stats):
            if nm in bars:
                name = 'batch_normalization_%d/%s' % (idx, nm)
                old = ora.state[name].astype(np.float64)
                np.testing.assert_allclose(dev['weights'][name], old - (old - batch) * BN_MOMENTUM_STEP, atol=bars[nm][0],
                                           rtol=bars[nm][1], err_msg=name)
    return errs


def check_residual_step(ora, net, probs, y, ref, *, probs_atol, loss_atol, grad_rtol, moving_mean_atol):
    """check_train_step for the residual family: the device keeps L2 out of its gradients, so the oracle's L2 term is taken
    out first; the moving means only, at assert_allclose's own rtol.  Every bar is the caller's."""
    loss, p, grads, cache = ref
    grads = {k: r - 2e-5 * ora.params[k].astype(np.float64) if k in ora.l2_names else r for k, r in grads.items()}
    bars = {'train_probs': probs_atol, 'loss': loss_atol, 'grad': grad_rtol, 'moving_mean': (moving_mean_atol, 1e-7)}
    check_train_step(host_step(net, probs), y, (loss, p, grads, cache), ora, bars, 'residual-family step B=%d' % y.shape[0])


def check_predict(p, ref, bars, tag):
    print("predict %s: max |p - oracle| = %.3g" % (tag, np.abs(p - ref).max()))
    assert np.abs(p - ref).max() < bars['predict']
    assert np.array_equal(p.argmax(1), ref.argmax(1))


def check_shard(dev, ref, bars):
    """A data-parallel shard's step against the oracle run at the shard's drop_offset: probabilities and every gradient."""
    assert np.abs(dev['probs'] - ref[1]).max() < bars['train_probs']
    assert max(grad_errors(dev['grads'], ref[2]).values()) < bars['grad']


def check_mutated_oracle(g, good, bad, bars, far):
    """Negative control: the device's gradients g meet the bar against the oracle's, and miss the mutated oracle's by `far`."""
    assert max(grad_errors(g, good).values()) < bars['grad']
    assert max(grad_errors(g, bad).values()) > far


def check_tensor_table(ora, net, shapes=False):
    assert [s.name for s in net.tensors.values() if not s.is_state] == list(ora.params.keys())
    assert [s.name for s in net.tensors.values() if s.is_state] == list(ora.state.keys())
    if shapes:
        for k, v in list(ora.params.items()) + list(ora.state.items()):
            assert net.tensors[k].shape == v.shape, k
    assert net.count_params() == ora.count_params()


def assert_bit_reproducible(net, x, y):
    """The same step twice from the same moving statistics: the same bits in probabilities, gradients and state."""
    import torch
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    state0 = net.state.clone()
    p1 = net.train_fwd_bwd(xd, yd, seed=1, step=0)
    g1, s1 = net.grads.clone(), net.state.clone()
    net.state.copy_(state0)
    p2 = net.train_fwd_bwd(xd, yd, seed=1, step=0)
    assert torch.equal(g1, net.grads) and torch.equal(s1, net.state) and torch.equal(p1, p2)


def check_checkpoint_round_trip(new_model, batches, path, slots, iterations=False):
    """save -> load -> one more step equals the uninterrupted run bit for bit: weights, moving statistics and the optimizer's
    `slots` (net attributes: 'slots', and 'slots2' for Adam; non-zero when saved), with `iterations` the optimizer's step count."""
    import torch

    def same():
        return all(torch.equal(getattr(a.net, s), getattr(b.net, s)) for s in ('params', 'state') + tuple(slots))

    a = new_model()
    for xb, yb in batches[:-1]:
        a.train_on_batch(xb, yb)
    assert all(float(getattr(a.net, s).abs().max()) > 0 for s in slots)
    a.save(path)
    b = new_model()
    b.load_weights(path)
    assert not iterations or b.optimizer.iterations == len(batches) - 1
    wa, wb = a.net.get_weights(), b.net.get_weights()
    assert list(wa) == list(wb) and all(np.array_equal(wa[k], wb[k]) for k in wa)
    assert same()
    la, lb = a.train_on_batch(*batches[-1]), b.train_on_batch(*batches[-1])
    assert la == lb
    assert same()


def generator_model(model_type, representation, repo_root, dct=80, mel=60, settings_to_model=True):
    """A model as train.py drives it: AudioProcessor on the synthetic bank -> data_gen (batches of 64) -> speech_model.
    -> (generator, model, settings)"""
    import sys
    import torch
    sys.path.insert(0, repo_root)
    import bench
    from speech_recognition_amd.input_data import AudioProcessor, prepare_words_list
    from speech_recognition_amd.model import prepare_model_settings, speech_model
    from speech_recognition_amd.utils import data_gen
    dev = torch.device("cuda", 0)
    settings = prepare_model_settings(label_count=len(prepare_words_list(bench.WANTED)), sample_rate=16000,
                                      clip_duration_ms=1000, window_size_ms=30.0, window_stride_ms=10.0,
                                      dct_coefficient_count=dct, num_log_mel_features=mel, output_representation=representation)
    proc = AudioProcessor(bench.build_synthetic(dev, 8192, seed=59185), 13.0, 60.0, bench.WANTED, 10.0, 0.0, settings,
                          output_representation=representation, device=dev)
    np.random.seed(1234)
    gen = data_gen(proc, None, batch_size=64, mode='training')
    model = speech_model(model_type, settings['fingerprint_size'], num_classes=settings['label_count'],
                         **(settings if settings_to_model else {}))
    return gen, model, settings


def check_workspace_refusal(net, x, y, training):
    """A step in a workspace of exactly workspace_bytes leaves the guard bands around it alone; one byte less is KWS_E_WORKSPACE
    with a message, and nothing runs."""
    import torch
    from speech_recognition_amd import _lib
    lib, B, guard = net.lib, x.shape[0], 4096
    need = int(lib.kws_net_workspace_bytes(net.handle, B, training))
    assert need > 0 and need % 4 == 0
    buf = torch.full((need // 4 + 2 * guard,), float('nan'), dtype=torch.float32, device="cuda")
    ws = buf[guard:guard + need // 4]
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    probs = torch.full(y.shape, float('nan'), dtype=torch.float32, device="cuda")

    def run(nbytes):
        if training:
            return lib.kws_net_train_fwd_bwd(net.handle, _lib.ptr(net.params), _lib.ptr(net.state), _lib.ptr(xd), _lib.ptr(yd), B,
                                             _lib.ptr(net.grads), _lib.ptr(probs), _lib.ptr(net.metrics), ctypes.c_uint64(1),
                                             ctypes.c_uint32(0), 0, B, _lib.ptr(ws), nbytes, _lib.stream_ptr())
        return lib.kws_net_predict(net.handle, _lib.ptr(net.params), _lib.ptr(net.state), _lib.ptr(xd), B, _lib.ptr(probs), _lib.ptr(ws),
                                   nbytes, _lib.stream_ptr())

    assert run(need - 1) == -3                                   # KWS_E_WORKSPACE
    assert b'workspace' in lib.kws_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(probs).all()) and bool(torch.isnan(buf).all())
    assert run(need) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[-guard:]).all())
    p = probs.cpu().numpy()
    assert np.isfinite(p).all() and np.abs(p.sum(1) - 1).max() < 1e-5
