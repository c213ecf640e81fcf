"""What the residual-family GPU parity files (test_logmfcc_gpu, test_steffe_gpu, test_residual_gpu, test_mfcc_and_raw_gpu)
share: the weight perturbation of their oracle / device pairs, the waveform batch, the read-back of the device's ReLU6
decisions, and the comparison of one training step against the oracle; and what the CPU files of every family share: the
perturbation again and the read-out of a net's native tensor table.  A plain module like grouped_oracle.py: no fixtures."""
import ctypes

import numpy as np


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


def perturb(ora, seed, negative_fraction=0.0, beta=(0.0, 0.1), bias=0.1, state=True):
    """Moves BN scales (1 + 0.1 n, about a negative_fraction of them negative), shifts (beta[0] + beta[1] n), biases (bias n;
    None: left alone) and, with `state`, the moving statistics off their initial 1 / 0 so that a mix-up shows."""
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
        if k.endswith('bias') and bias is not None:
            ora.params[k] = (bias * rng.randn(*shape)).astype(np.float32)
    for k in ora.state if state else ():
        if k.endswith('moving_mean'):
            ora.state[k] = (0.05 * rng.randn(*ora.state[k].shape)).astype(np.float32)
        else:
            ora.state[k] = (1.0 + 0.2 * rng.rand(*ora.state[k].shape)).astype(np.float32)


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


def check_step(ora, net, probs, y, ref, *, probs_atol, loss_atol, grad_rtol, moving_mean_atol):
    """One net.train_fwd_bwd against ref = ora.loss_and_grads(...) taken on the device's own decisions: probabilities and
    their argmax, mean loss, the correct count, every gradient relative to its tensor's maximum (the device keeps L2 out
    of its gradients), the moving means.  Every bar is the caller's: none has a default."""
    loss, p, grads, cache = ref
    B = y.shape[0]
    got = probs.cpu().numpy()
    assert np.abs(got - p).max() < probs_atol
    assert np.array_equal(got.argmax(1), p.argmax(1))
    m = net.metrics.cpu().numpy()
    assert abs(m[0] / B - loss) < loss_atol
    assert m[1] == (p.argmax(1) == y.argmax(1)).sum()
    g = net.grads_dict()
    for k, r in grads.items():
        if k in ora.l2_names:
            r = r - 2e-5 * ora.params[k].astype(np.float64)
        r = r.reshape(g[k].shape)
        err = np.abs(g[k] - r).max() / max(np.abs(r).max(), 1e-7)
        assert err < grad_rtol, (k, err)
    w = net.get_weights()
    for idx, (mean, var) in cache['batch_stats'].items():
        name = 'batch_normalization_%d/moving_mean' % idx
        mm = ora.state[name].astype(np.float64)
        np.testing.assert_allclose(w[name], mm - (mm - mean) * 0.01, atol=moving_mean_atol)
