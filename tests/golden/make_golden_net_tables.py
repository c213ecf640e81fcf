#!/usr/bin/env python
"""Tensor tables of every net kind, recorded from the built library:   python tests/golden/make_golden_net_tables.py

The Keras tensor names, their order and their offsets in the flat parameter / state buffers ARE the checkpoint format
(DeviceNet.set_weights, the .npz checkpoints, the buffer RCCL all-reduces), so tests/golden/net_tensor_tables.json pins
them: tests/test_net_tables_cpu.py compares the library's tables with it row by row.  The file was recorded at the commit
before the residual-family builders were put on one shared block planner; re-record it only when a table is MEANT to
change, and say so in that commit.  The last six configs were added later, recorded at the commit before the flat-tail
programs were put on one skeleton; the entries recorded earlier came out byte for byte as they were.

One row per tensor: [name, shape, offset, is_state, l2, fan_in, fan_out, init] (l2 and init as the shortest decimal that
gives the float32 back)."""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from speech_recognition_amd import _lib  # noqa: E402

COLUMNS = ['name', 'shape', 'offset', 'is_state', 'l2', 'fan_in', 'fan_out', 'init']
# id -> (kind, num_classes, filter_mult, input_size, spectrogram_length, num_features)
CONFIGS = {
    'ts_attention': (_lib.KWS_NET_TS_ATTENTION, 12, 1, 16000, 0, 0),
    'ts_attention_32_x2': (_lib.KWS_NET_TS_ATTENTION, 32, 2, 16000, 0, 0),
    'log_mfcc_32': (_lib.KWS_NET_LOG_MFCC, 32, 1, 98 * 40, 98, 40),
    'log_mfcc_65x40': (_lib.KWS_NET_LOG_MFCC, 12, 1, 65 * 40, 65, 40),
    'spectrogram': (_lib.KWS_NET_LOG_MFCC, 12, 1, 98 * 257, 98, 257),
    'steffe': (_lib.KWS_NET_STEFFE, 12, 1, 16000, 0, 0),
    'residual': (_lib.KWS_NET_RESIDUAL, 12, 1, 16000, 0, 0),
    'residual_x2': (_lib.KWS_NET_RESIDUAL, 12, 2, 16000, 0, 0),
    'mfcc_and_raw': (_lib.KWS_NET_MFCC_AND_RAW, 12, 1, 98 * 40 + 16000, 98, 40),
    'conv_1d_fast': (_lib.KWS_NET_CONV_1D_FAST, 12, 1, 16000, 0, 0),
    'conv_1d_spec': (_lib.KWS_NET_CONV_1D_SPEC, 12, 1, 98 * 257, 0, 0),
    'conv_1d_time_stacked': (_lib.KWS_NET_CONV_1D_TIME_STACKED, 12, 1, 16000, 0, 0),
    'conv_1d_heavy': (_lib.KWS_NET_CONV_1D_HEAVY, 12, 1, 16000, 0, 0),
    'conv_1d_gru': (_lib.KWS_NET_CONV_1D_GRU, 12, 1, 16000, 0, 0),
    'conv_1d_simple': (_lib.KWS_NET_CONV_1D_SIMPLE, 12, 1, 16000, 0, 0),
    'conv_1d_multi_time_sliced': (_lib.KWS_NET_CONV_1D_MULTI_TIME_SLICED, 12, 1, 16000, 0, 0),
    'conv_1d_time_sliced': (_lib.KWS_NET_CONV_1D_TIME_SLICED, 12, 1, 16000, 0, 0),
    'conv_1d_time_sliced_x2': (_lib.KWS_NET_CONV_1D_TIME_SLICED, 12, 2, 12000, 0, 0),
    'xception_with_attention': (_lib.KWS_NET_XCEPTION_ATTENTION, 12, 1, 16000, 0, 0),
    'inception_d1': (_lib.KWS_NET_INCEPTION_D1, 12, 1, 16000, 0, 0),
    'conv_2d_mobile': (_lib.KWS_NET_CONV_2D_MOBILE, 12, 1, 98 * 40, 0, 0),
    'conv_2d_fast': (_lib.KWS_NET_CONV_2D_FAST, 12, 1, 98 * 40, 0, 0),
    'conv_1d_learned_spec': (_lib.KWS_NET_CONV_1D_LEARNED_SPEC, 12, 1, 16000, 0, 0),
    'conv_1d_top_down': (_lib.KWS_NET_CONV_1D_TOP_DOWN, 12, 1, 16000, 0, 0),
}


def _f32(v):
    return float(str(np.float32(v)))


def table(config):
    """The library's tensor table for one config: (rows, num_params, num_state)."""
    lib = _lib.load()
    cfg = _lib.NetConfig(*config)
    h = ctypes.c_void_p()
    _lib.check(lib.kws_net_create(ctypes.byref(cfg), ctypes.byref(h)), "kws_net_create")
    try:
        rows = []
        for i in range(lib.kws_net_num_tensors(h)):
            t = _lib.TensorInfo()
            _lib.check(lib.kws_net_tensor_info(h, i, ctypes.byref(t)), "kws_net_tensor_info")
            rows.append([t.name.decode(), [int(t.shape[k]) for k in range(t.ndim)], int(t.offset), int(t.is_state), _f32(t.l2),
                         int(t.fan_in), int(t.fan_out), _f32(t.init)])
        return rows, int(lib.kws_net_num_params(h)), int(lib.kws_net_num_state(h))
    finally:
        lib.kws_net_destroy(h)


def main():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'net_tensor_tables.json')
    with open(path, 'w') as f:
        f.write('{"columns": %s,\n "tables": {' % json.dumps(COLUMNS))
        for k, (name, config) in enumerate(CONFIGS.items()):
            rows, n_params, n_state = table(config)
            f.write('%s\n"%s": {"config": %s, "num_params": %d, "num_state": %d, "rows": [\n' %
                    (',' if k else '', name, json.dumps(list(config)), n_params, n_state))
            f.write(',\n'.join(json.dumps(r, separators=(',', ':')) for r in rows))
            f.write(']}')
        f.write('}}\n')
    print('wrote', path)


if __name__ == '__main__':
    main()
