#!/usr/bin/env python
"""Layer structure of the reference's conv_1d_time_sliced_model (model.py:716-772) for filter_mult 1 and 2, recorded BY RUNNING
the reference's own model builder.

Build container only (needs the reference checkout):   python tests/golden/make_golden_time_sliced.py

The recording stand-ins for keras are make_golden_grouped.py's and make_golden_dwk.py's (every layer class records its
constructor arguments when it is created and computes its output shape when it is called on a stand-in tensor), plus what this
model adds: tensorflow.extract_image_patches on a [1, W, 1] tensor (SAME: ceil(W / stride) patches of ksize samples, TensorFlow's
left padding recorded next to them) with the K.int_shape / K.reshape calls around it, GlobalAveragePooling1D, and a Dense that
records its kernel_regularizer.  Names follow Keras 2.1's per-class auto-numbering in creation order.  No reference source text
is stored: tests/golden/time_sliced_models.json holds the recorded structure only.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_dwk as md  # noqa: E402
import make_golden_grouped as mg  # noqa: E402

_patches = []


def int_shape(x):
    return (None,) + tuple(x.shape)


def reshape(x, shape):
    assert shape[0] == -1
    n = 1
    for d in x.shape:
        n *= d
    m = 1
    for d in shape[1:]:
        m *= d
    assert n == m
    return mg.T(shape[1:])


def extract_image_patches(x, ksizes, strides, rates, padding):
    assert len(x.shape) == 3 and x.shape[0] == 1 and x.shape[2] == 1 and padding == 'SAME'
    assert ksizes[0] == ksizes[1] == ksizes[3] == 1 and strides[0] == strides[1] == strides[3] == 1 and list(rates) == [1, 1, 1, 1]
    W, k, s = x.shape[1], ksizes[2], strides[2]
    n = -(-W // s)
    total = max((n - 1) * s + k - W, 0)
    _patches.append({'class': 'extract_image_patches', 'ksize': k, 'stride': s, 'padding': padding, 'input_length': W,
                     'pad_left': total // 2, 'output': [n, k]})
    return mg.T((1, n, k))


class Lambda(md.Lambda):
    def __call__(self, x):
        before = len(_patches)
        out = md.Lambda.__call__(self, x)
        if len(_patches) > before:
            self.rec['patches'] = _patches[-1]
        return out


class GlobalAveragePooling1D(mg.Layer):
    def out_shape(self, x):
        self.rec.update({'input': list(x.shape), 'output': [x.shape[-1]]})
        return (x.shape[-1],)


class Dense(mg.Dense):
    def out_shape(self, x):
        out = mg.Dense.out_shape(self, x)
        self.rec['kernel_regularizer'] = self.kwargs.get('kernel_regularizer')
        return out


def install_stubs():
    md.install_stubs()
    kl = sys.modules['keras.layers']
    kl.Lambda = Lambda
    kl.Dense = Dense
    kl.GlobalAveragePooling1D = GlobalAveragePooling1D
    kl.__all__ = list(kl.__all__) + ['GlobalAveragePooling1D']
    kb = sys.modules['keras.backend']
    kb.int_shape, kb.reshape = int_shape, reshape
    sys.modules['tensorflow'].extract_image_patches = extract_image_patches


def record(builder, input_size, num_classes, filter_mult):
    mg._counts.clear()
    del mg._layers[:]
    del _patches[:]
    model = builder(input_size=input_size, num_classes=num_classes, filter_mult=filter_mult)
    weights = []
    for r in mg._layers:
        l2 = (r.get('kernel_regularizer') or {}).get('l2', 0.0)
        if r['class'] == 'DepthwiseConv2D':
            weights.append({'name': r['name'] + '/depthwise_kernel', 'shape': r['kernel'], 'l2': l2})
            assert not r['use_bias']
        elif r['class'] == 'Conv1D':
            weights.append({'name': r['name'] + '/kernel', 'shape': r['kernel'], 'l2': l2})
            assert not r['use_bias']
        elif r['class'] == 'BatchNormalization':
            for w in ('gamma', 'beta', 'moving_mean', 'moving_variance'):
                weights.append({'name': '%s/%s' % (r['name'], w), 'shape': [r['channels']], 'l2': 0.0,
                                'state': w.startswith('moving')})
        elif r['class'] == 'Dense':
            weights.append({'name': r['name'] + '/kernel', 'shape': r['kernel'], 'l2': l2})
            assert not r['use_bias']
    return {'model_name': model.name, 'optimizer': model.optimizer.kind, 'lr': model.optimizer.lr, 'loss': model.loss,
            'input_size': input_size, 'num_classes': num_classes, 'filter_mult': filter_mult, 'output_shape': list(model.output_shape),
            'layers': [{k: v for k, v in r.items() if k != 'kernel_regularizer'} for r in mg._layers], 'weights': weights}


def main():
    install_stubs()
    sys.path.insert(0, mg.REF)
    import model as ref_model
    out = {'conv_1d_time_sliced_fm%d' % fm: record(ref_model.conv_1d_time_sliced_model, 16000, 12, fm) for fm in (1, 2)}
    path = os.path.join(mg.OUT, 'time_sliced_models.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print('wrote', path)


if __name__ == '__main__':
    main()
