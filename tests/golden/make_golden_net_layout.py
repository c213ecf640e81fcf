#!/usr/bin/env python
"""Workspace layout of every net kind, recorded from the built library:   python tests/golden/make_golden_net_layout.py

kws_net_workspace_bytes and kws_net_debug_view are host arithmetic over the layer table (no GPU is touched), and the
offsets they hand out are where the network programs keep every intermediate tensor.  tests/golden/net_workspace_layout.json
pins them for the configs of net_tensor_tables.json: tests/test_net_layout_cpu.py asks the library for the same numbers.
The file was recorded at the commit before the network programs were put behind one interface; re-record it only when a
layout is MEANT to change, and say so in that commit.

Per config: "workspace_bytes" maps a batch to [inference, training] bytes; "views" maps training (1, 0) to one row
[what, index, offset_floats, count] for every (what, index) the library accepts at batch VIEW_BATCH."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from speech_recognition_amd import _lib  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
BATCHES = (1, 5, 64)
VIEW_BATCH = 5
WHATS, INDICES = range(7), range(64)


def layout(config):
    """The library's workspace sizes and accepted debug views for one config, in the fixture's form."""
    lib = _lib.load()
    cfg = _lib.NetConfig(*config)
    h = ctypes.c_void_p()
    _lib.check(lib.kws_net_create(ctypes.byref(cfg), ctypes.byref(h)), "kws_net_create")
    try:
        sizes = {str(B): [int(lib.kws_net_workspace_bytes(h, B, training)) for training in (0, 1)] for B in BATCHES}
        views = {}
        for training in (1, 0):
            rows = []
            for what in WHATS:
                for index in INDICES:
                    off, cnt = ctypes.c_int64(-1), ctypes.c_int64(-1)
                    if lib.kws_net_debug_view(h, VIEW_BATCH, training, what, index, ctypes.byref(off), ctypes.byref(cnt)) == 0:
                        rows.append([what, index, off.value, cnt.value])
            views[str(training)] = rows
        return {"workspace_bytes": sizes, "views": views}
    finally:
        lib.kws_net_destroy(h)


def main():
    with open(os.path.join(HERE, 'net_tensor_tables.json')) as f:
        configs = {name: t['config'] for name, t in json.load(f)['tables'].items()}
    path = os.path.join(HERE, 'net_workspace_layout.json')
    with open(path, 'w') as f:
        f.write('{"batches": %s, "view_batch": %d, "view_columns": ["what", "index", "offset_floats", "count"],\n "layouts": {' %
                (json.dumps(list(BATCHES)), VIEW_BATCH))
        for k, (name, config) in enumerate(configs.items()):
            lo = layout(config)
            f.write('%s\n"%s": {"config": %s, "workspace_bytes": %s, "views": {' %
                    (',' if k else '', name, json.dumps(config), json.dumps(lo['workspace_bytes'])))
            f.write(',\n'.join('"%s": [\n%s]' % (t, ',\n'.join(json.dumps(r, separators=(',', ':')) for r in lo['views'][t]))
                               for t in ('1', '0')))
            f.write('}}')
        f.write('}}\n')
    print('wrote', path)


if __name__ == '__main__':
    main()
