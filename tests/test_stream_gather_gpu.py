"""kws_stream_gather_f32 (csrc/stream.hip) through ctypes against stream_feature_cases.gather_ref, compared as uint32: the
kernel copies bits.  The source is arbitrary 32-bit patterns (NaNs of every payload, -0.0, denormals); the output lies inside
a poisoned buffer with guard bands, and every float outside the row segments - the gaps between rows, the bands before and
after - must still hold the poison afterwards.  Every case runs twice into the same buffer."""
import ctypes

import numpy as np
import pytest
import torch

import stream_feature_cases as FC
from speech_recognition_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 64                      # poisoned floats before and after the rows
SOURCE_WORDS = 1 << 20          # more than the largest n of the tables (GATHER_WRAP's) + 4


@pytest.fixture(scope="module")
def source():
    u = FC.gather_source(SOURCE_WORDS, 7)
    return u, torch.from_numpy(u.view(np.int32)).cuda().view(torch.float32)


def _gather(src_t, c, out_t):
    """The C call on slices: src = src_t[soff : soff + n], out = out_t[GUARD + doff :] -> rc."""
    lib = _lib.load()
    src_ptr = ctypes.c_void_p(src_t.data_ptr() + 4 * c['soff']) if c['n'] else None
    return lib.kws_stream_gather_f32(src_ptr, c['n'], c['start'], c['hop'], c['win'],
                                     ctypes.c_void_p(out_t.data_ptr() + 4 * (GUARD + c['doff'])), c['out_pitch'], c['W'],
                                     _lib.stream_ptr())


def _check(source, c):
    u, src_t = source
    assert c['soff'] + c['n'] <= len(u)
    words = GUARD + c['doff'] + (c['W'] - 1) * c['out_pitch'] + c['win'] + GUARD
    poisoned = np.full(words, FC.POISON, dtype=np.uint32)
    out_t = torch.from_numpy(poisoned.view(np.int32)).cuda().view(torch.float32)
    assert out_t.data_ptr() % 16 == 0 and src_t.data_ptr() % 16 == 0       # so soff / doff ARE the offsets mod 4
    for _ in range(2):
        assert _gather(src_t, c, out_t) == 0, (c, _lib.load().kws_last_error())
    got = out_t.view(torch.int32).cpu().numpy().view(np.uint32)
    want = FC.gather_ref(u[c['soff']:c['soff'] + c['n']], c['n'], c['start'], c['hop'], c['win'], poisoned, c['out_pitch'],
                         c['W'], GUARD + c['doff'])
    if got.tobytes() != want.tobytes():
        bad = np.nonzero(got != want)[0]
        rel = bad - (GUARD + c['doff'])
        pytest.fail("%r: %d words differ, first at row %d element %d (got %08x, want %08x)" %
                    (c, len(bad), rel[0] // c['out_pitch'], rel[0] % c['out_pitch'], got[bad[0]], want[bad[0]]))


@pytest.mark.parametrize("win", FC.GATHER_WINS)
def test_gather_is_a_copy_of_bits_at_every_alignment_pitch_hop_and_edge(source, win):
    n_cases = 0
    for c in FC.gather_cases(win):
        _check(source, c)
        n_cases += 1
    assert n_cases >= 4 * 4 * 5 * 16


def test_more_chunks_than_one_pass_of_the_grid(source):
    c = FC.GATHER_WRAP
    assert c['W'] * -(-c['win'] // 4) > FC.GATHER_GRID_THREADS
    _check(source, c)


def test_composite_rows_from_two_calls(source):
    """Rows [3 features | 5 samples] at pitch 8 + 1 by two calls with one out_pitch: each leaves the other's half and the
    spare float alone."""
    u, src_t = source
    W, pitch = 6, 9
    poisoned = np.full(GUARD + W * pitch + GUARD, FC.POISON, dtype=np.uint32)
    out_t = torch.from_numpy(poisoned.view(np.int32)).cuda().view(torch.float32)
    a = dict(n=40, start=0, hop=2, win=3, out_pitch=pitch, W=W, soff=3, doff=0)
    b = dict(n=50, start=-2, hop=7, win=5, out_pitch=pitch, W=W, soff=100, doff=3)
    assert _gather(src_t, a, out_t) == 0 and _gather(src_t, b, out_t) == 0
    want = FC.gather_ref(u[3:43], 40, 0, 2, 3, poisoned, pitch, W, GUARD)
    want = FC.gather_ref(u[100:150], 50, -2, 7, 5, want, pitch, W, GUARD + 3)
    got = out_t.view(torch.int32).cpu().numpy().view(np.uint32)
    assert got.tobytes() == want.tobytes()
    assert (got.reshape(-1)[GUARD:GUARD + W * pitch].reshape(W, pitch)[:, 8] == FC.POISON).all()


@pytest.mark.parametrize("change", [
    dict(win=0), dict(win=-4), dict(hop=0), dict(hop=-1), dict(W=0), dict(W=-1), dict(out_pitch=7), dict(n=-1),
    dict(n=(1 << 61) + 1), dict(start=(1 << 61) + 1), dict(start=-(1 << 61) - 1), dict(out_pitch=1 << 61, W=3),
    dict(null_out=True), dict(null_src=True), dict(out_bytes=2), dict(src_bytes=1),
])
def test_refused_arguments_write_nothing(source, change):
    _, src_t = source
    c = dict(win=8, hop=3, W=4, out_pitch=8, n=100, start=0)
    flags = {k: change[k] for k in ('null_out', 'null_src', 'out_bytes', 'src_bytes') if k in change}
    c.update({k: v for k, v in change.items() if k not in flags})
    poisoned = np.full(GUARD + 64 + GUARD, FC.POISON, dtype=np.uint32)
    out_t = torch.from_numpy(poisoned.view(np.int32)).cuda().view(torch.float32)
    src_ptr = None if flags.get('null_src') else ctypes.c_void_p(src_t.data_ptr() + flags.get('src_bytes', 0))
    out_ptr = None if flags.get('null_out') else ctypes.c_void_p(out_t.data_ptr() + 4 * GUARD + flags.get('out_bytes', 0))
    lib = _lib.load()
    rc = lib.kws_stream_gather_f32(src_ptr, c['n'], c['start'], c['hop'], c['win'], out_ptr, c['out_pitch'], c['W'],
                                   _lib.stream_ptr())
    assert rc == -1                                                       # KWS_E_INVALID
    assert b"stream_gather" in lib.kws_last_error()
    torch.cuda.synchronize()
    assert (out_t.view(torch.int32).cpu().numpy().view(np.uint32) == FC.POISON).all()


def test_accepted_extremes(source):
    """n = 0 with a NULL source, the largest accepted n / start (rows wholly outside: zeros, nothing read), a hop beyond 2^62."""
    u, src_t = source
    for c in (dict(n=0, start=0, hop=1, win=5, out_pitch=6, W=3, soff=0, doff=1),
              dict(n=0, start=-(1 << 61), hop=1, win=5, out_pitch=5, W=3, soff=0, doff=0),
              dict(n=100, start=1 << 61, hop=4, win=7, out_pitch=9, W=3, soff=2, doff=3),
              dict(n=100, start=-(1 << 61), hop=1 << 40, win=7, out_pitch=7, W=4, soff=1, doff=0),
              dict(n=100, start=-3, hop=(1 << 63) - 1, win=9, out_pitch=12, W=4, soff=1, doff=2)):
        words = GUARD + c['doff'] + (c['W'] - 1) * c['out_pitch'] + c['win'] + GUARD
        poisoned = np.full(words, FC.POISON, dtype=np.uint32)
        out_t = torch.from_numpy(poisoned.view(np.int32)).cuda().view(torch.float32)
        assert _gather(src_t, c, out_t) == 0, (c, _lib.load().kws_last_error())
        got = out_t.view(torch.int32).cpu().numpy().view(np.uint32)
        # Python integers: the indices of these cases leave int64 in the restatement's own arithmetic
        want = poisoned.copy()
        for w in range(c['W']):
            for i in range(c['win']):
                s = c['start'] + w * c['hop'] + i
                want[GUARD + c['doff'] + w * c['out_pitch'] + i] = u[c['soff'] + s] if 0 <= s < c['n'] else 0
        assert got.tobytes() == want.tobytes(), c
