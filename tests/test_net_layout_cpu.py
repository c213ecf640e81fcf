"""The workspace layout of every net kind against tests/golden/net_workspace_layout.json (recorded by
tests/golden/make_golden_net_layout.py before the network programs were put behind one interface): the bytes
kws_net_workspace_bytes asks for, the set of (what, index) pairs kws_net_debug_view accepts, and the offset and count of
each.  All of it is host arithmetic over the layer table, so no GPU is needed.  The programs keep every intermediate at
these offsets: nothing may move unless a commit means it to and re-records the file."""
import copy
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('make_golden_net_layout', os.path.join(HERE, 'golden', 'make_golden_net_layout.py'))
_rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_rec)

with open(os.path.join(HERE, 'golden', 'net_workspace_layout.json')) as _f:
    _GOLD = json.load(_f)
LAYOUTS = _GOLD['layouts']
# accepted views (training, inference) at the recorded commit, written down apart from the file: a truncated fixture does not pass
N_VIEWS = {'ts_attention': (99, 35), 'ts_attention_32_x2': (99, 35), 'log_mfcc_32': (241, 241), 'log_mfcc_65x40': (241, 241),
           'spectrogram': (241, 241), 'steffe': (256, 256), 'residual': (260, 260), 'residual_x2': (260, 260),
           'mfcc_and_raw': (245, 245), 'conv_1d_fast': (14, 14), 'conv_1d_spec': (36, 36), 'conv_1d_time_stacked': (26, 26),
           'conv_1d_heavy': (32, 32), 'conv_1d_gru': (82, 82), 'conv_1d_simple': (170, 106), 'conv_1d_multi_time_sliced': (64, 64),
           'conv_1d_time_sliced': (105, 105), 'conv_1d_time_sliced_x2': (105, 105),
           'xception_with_attention': (309, 309), 'inception_d1': (192, 192), 'conv_2d_mobile': (32, 32), 'conv_2d_fast': (16, 16),
           'conv_1d_learned_spec': (29, 29), 'conv_1d_top_down': (37, 37)}


def _mismatches(got, gold):
    """Every difference between the library's layout and the recorded one, as readable strings (empty: equal)."""
    out = []
    for B in sorted(set(got['workspace_bytes']) | set(gold['workspace_bytes']), key=int):
        if got['workspace_bytes'].get(B) != gold['workspace_bytes'].get(B):
            out.append('workspace_bytes B=%s: %r != recorded %r' % (B, got['workspace_bytes'].get(B), gold['workspace_bytes'].get(B)))
    for t in ('1', '0'):
        have = {(r[0], r[1]): r[2:] for r in got['views'][t]}
        want = {(r[0], r[1]): r[2:] for r in gold['views'][t]}
        for key in sorted(set(have) | set(want)):
            if have.get(key) != want.get(key):
                out.append('training=%s view %d/%d: %r != recorded %r' % ((t,) + key + (have.get(key), want.get(key))))
    return out


def test_fixture_is_complete():
    assert _GOLD['batches'] == [1, 5, 64] == list(_rec.BATCHES) and _GOLD['view_batch'] == 5 == _rec.VIEW_BATCH
    assert (list(_rec.WHATS), list(_rec.INDICES)) == (list(range(7)), list(range(64)))
    assert {k: (len(v['views']['1']), len(v['views']['0'])) for k, v in LAYOUTS.items()} == N_VIEWS
    for v in LAYOUTS.values():
        assert sorted(v['workspace_bytes']) == ['1', '5', '64'] and all(len(s) == 2 and min(s) > 0 for s in v['workspace_bytes'].values())
    with open(os.path.join(HERE, 'golden', 'net_tensor_tables.json')) as f:
        assert {k: v['config'] for k, v in json.load(f)['tables'].items()} == {k: v['config'] for k, v in LAYOUTS.items()}


@pytest.mark.parametrize("name", sorted(N_VIEWS))
def test_workspace_layout_matches_recorded(name):
    gold = LAYOUTS[name]
    assert _mismatches(_rec.layout(gold['config']), gold) == []


def test_comparison_reports_a_moved_offset():
    """Negative control: one offset moved by one 256-byte granule is reported, at that entry only."""
    gold = LAYOUTS['conv_1d_multi_time_sliced']
    got = _rec.layout(gold['config'])
    moved = copy.deepcopy(gold)
    row = moved['views']['1'][7]
    row[2] += 64
    assert _mismatches(got, moved) == ['training=1 view %d/%d: %r != recorded %r' % (row[0], row[1], [row[2] - 64, row[3]], row[2:])]
