"""The tensor table of every net kind against tests/golden/net_tensor_tables.json (recorded by
tests/golden/make_golden_net_tables.py before the residual-family builders moved onto one shared block planner).  The
Keras names, their order and the offsets in the flat buffers are the checkpoint format: nothing in a table may move unless
a commit means it to and re-records the file."""
import copy
import json
import os

import numpy as np
import pytest

from net_parity import native_table

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'net_tensor_tables.json')
with open(GOLDEN) as _f:
    _GOLD = json.load(_f)
TABLES = _GOLD['tables']
# the counts at the recorded commit, written down apart from the file: a truncated fixture does not pass
N_TENSORS = {'ts_attention': 74, 'ts_attention_32_x2': 74, 'log_mfcc_32': 148, 'log_mfcc_65x40': 148, 'spectrogram': 148,
             'steffe': 186, 'residual': 200, 'residual_x2': 200, 'mfcc_and_raw': 152, 'conv_1d_fast': 58, 'conv_1d_spec': 142,
             'conv_1d_time_stacked': 67, 'conv_1d_heavy': 81, 'conv_1d_gru': 40, 'conv_1d_simple': 92,
             'conv_1d_multi_time_sliced': 194, 'conv_1d_time_sliced': 85, 'conv_1d_time_sliced_x2': 85,
             'xception_with_attention': 166, 'inception_d1': 397, 'conv_2d_mobile': 50, 'conv_2d_fast': 26,
             'conv_1d_learned_spec': 108, 'conv_1d_top_down': 124}


def _row(t):
    """A TensorInfo in the fixture's columns; l2 and init stay float32."""
    return [t.name.decode(), [int(t.shape[k]) for k in range(t.ndim)], int(t.offset), int(t.is_state), np.float32(t.l2),
            int(t.fan_in), int(t.fan_out), np.float32(t.init)]


def _mismatches(table, gold_rows):
    """Every difference between the library's table and the recorded rows, as readable strings (empty: equal)."""
    out = []
    if len(table) != len(gold_rows):
        out.append('%d tensors, %d recorded' % (len(table), len(gold_rows)))
    for i, (t, g) in enumerate(zip(table, gold_rows)):
        got = _row(t)
        want = g[:4] + [np.float32(g[4])] + g[5:7] + [np.float32(g[7])]
        if got != want:
            out.append('row %d: %r != recorded %r' % (i, got, want))
    return out


def test_fixture_is_complete():
    assert _GOLD['columns'] == ['name', 'shape', 'offset', 'is_state', 'l2', 'fan_in', 'fan_out', 'init']
    assert {k: len(v['rows']) for k, v in TABLES.items()} == N_TENSORS


@pytest.mark.parametrize("name", sorted(N_TENSORS))
def test_tensor_table_matches_recorded(name):
    gold = TABLES[name]
    kind, nc, fm, input_size, T, F = gold['config']
    table = native_table(kind, nc, input_size, fm, T, F)
    assert _mismatches(table, gold['rows']) == []
    # the buffer sizes: the end of the last tensor of each buffer, rounded up to the 16-byte granule
    for state, total in ((0, gold['num_params']), (1, gold['num_state'])):
        last = max((t for t in table if t.is_state == state), key=lambda t: t.offset)
        assert last.offset + (last.size + 3) // 4 * 4 == total


@pytest.mark.parametrize("name", ['log_mfcc_32', 'steffe', 'residual', 'mfcc_and_raw', 'ts_attention', 'conv_1d_fast'])
def test_comparison_reports_a_renumbered_name_and_a_swapped_pair(name):
    """Negative control: the comparison above is not vacuous."""
    gold = TABLES[name]
    kind, nc, fm, input_size, T, F = gold['config']
    table = native_table(kind, nc, input_size, fm, T, F)
    rows = gold['rows']
    # a Keras counter off by one on one layer (what a change in creation order does)
    i = next(k for k, r in enumerate(rows) if r[0] == 'batch_normalization_3/gamma')
    renumbered = copy.deepcopy(rows)
    renumbered[i][0] = 'batch_normalization_4/gamma'
    bad = _mismatches(table, renumbered)
    assert len(bad) == 1 and bad[0].startswith('row %d:' % i)
    # two neighbouring tensors created in the other order (names, shapes and offsets travel with their rows)
    j = next(k for k, r in enumerate(rows) if r[0].startswith('depthwise_conv2d_') or r[0] == 'conv1d_2/kernel')
    swapped = copy.deepcopy(rows)
    swapped[j], swapped[j + 1] = swapped[j + 1], swapped[j]
    bad = _mismatches(table, swapped)
    assert [b.split(':')[0] for b in bad] == ['row %d' % j, 'row %d' % (j + 1)]
    # a row dropped from the end
    assert _mismatches(table, rows[:-1]) == ['%d tensors, %d recorded' % (len(rows), len(rows) - 1)]
