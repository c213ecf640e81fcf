#!/usr/bin/env python
"""Layer structure of the reference's conv_1d_simple_model (model.py:116-156), recorded BY RUNNING the reference's own model builder.

Build container only (needs the reference checkout):   python tests/golden/make_golden_gru.py

The recording stand-ins for keras are make_golden_dwk.py's (the depthwise blocks) plus what this model adds: a GRU that records its
units and both dropout rates, a Bidirectional wrapper that records its merge mode, the three weight shapes of each direction
(kernel [I, 3 units], recurrent_kernel [units, 3 units], bias [3 units]) and its output shape, and Adam.  Weight names follow Keras
2.1's Bidirectional: bidirectional_<n>/forward_<gru name>/... then bidirectional_<n>/backward_<gru name>/...  No reference source
text is stored: tests/golden/gru_models.json holds the recorded structure only.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_grouped as mg  # noqa: E402
import make_golden_dwk as md  # noqa: E402
from make_golden_stacked import Adam  # noqa: E402


class GRU(mg.Layer):
    """Recorded when created; shapes are filled in by the Bidirectional wrapper that calls it."""

    def __init__(self, *args, **kwargs):
        mg.Layer.__init__(self, *args, **kwargs)
        self.rec.update({'units': args[0], 'dropout': kwargs.get('dropout', 0.0), 'recurrent_dropout': kwargs.get('recurrent_dropout', 0.0),
                         'return_sequences': kwargs.get('return_sequences', False), 'use_bias': kwargs.get('use_bias', True),
                         'activation': kwargs.get('activation', 'tanh'),
                         'recurrent_activation': kwargs.get('recurrent_activation', 'hard_sigmoid'),
                         'implementation': kwargs.get('implementation', 1)})


class Bidirectional(mg.Layer):
    def out_shape(self, x):
        inner = self.args[0]
        units = inner.rec['units']
        T, I = x.shape
        merge = self.kwargs.get('merge_mode', 'concat')
        assert merge == 'concat' and not inner.rec['return_sequences']
        self.rec.update({'layer': inner.name, 'merge_mode': merge, 'units': units, 'dropout': inner.rec['dropout'],
                         'recurrent_dropout': inner.rec['recurrent_dropout'], 'input': [T, I], 'kernel': [I, 3 * units],
                         'recurrent_kernel': [units, 3 * units], 'bias': [3 * units], 'output': [2 * units]})
        return (2 * units,)


def install_stubs():
    md.install_stubs()
    kl = sys.modules['keras.layers']
    kl.GRU, kl.Bidirectional = GRU, Bidirectional
    kl.__all__ = list(kl.__all__) + ['GRU', 'Bidirectional']
    sys.modules['keras.optimizers'].Adam = Adam


def record(builder, input_size, num_classes):
    rec = md.record(builder, input_size, num_classes)
    # md.record does not know the recurrent layer: its weights go between the last BatchNormalization and the Dense layer
    weights = [w for w in rec['weights'] if not w['name'].startswith('dense_')]
    for r in mg._layers:
        if r['class'] == 'Bidirectional':
            for d in ('forward', 'backward'):
                for w in ('kernel', 'recurrent_kernel', 'bias'):
                    weights.append({'name': '%s/%s_%s/%s' % (r['name'], d, r['layer'], w), 'shape': r[w], 'l2': 0.0})
    weights += [w for w in rec['weights'] if w['name'].startswith('dense_')]
    rec['weights'] = weights
    return rec


def main():
    install_stubs()
    sys.path.insert(0, mg.REF)
    import model as ref_model
    out = {'conv_1d_simple': record(ref_model.conv_1d_simple_model, 16000, 12)}
    path = os.path.join(mg.OUT, 'gru_models.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print('wrote', path)


if __name__ == '__main__':
    main()
