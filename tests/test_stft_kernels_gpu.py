"""kws_stft_mel_f32 on every dispatch path and frame edge, against float64 (cases, references and bars: tests/stft_cases.py,
checked on the CPU by tests/test_stft_cases_cpu.py).

Every case first asks the library which kernel it launches (kws_stft_mel_kernel) and compares the answer with the case table,
then runs the three output kinds (1 magnitudes, 2 log-mel, 0 features) twice into sentinel-guarded outputs - the input sits
between NaN guards too - and asserts: bit-identical runs, every element written and finite, the bars of stft_cases against
oracle.features in float64, and two float64 replays FROM THE DEVICE'S OWN intermediate results that place an error in one
stage (log-mel from the device's magnitudes; the generic kernel's DCT chain from the device's log-mel rows).

Paths that no other test launches: stft4's full-width instances (shapes 2 and 4), the host clamp of a tap window at the
Nyquist end of the magnitude row and the table image's shift of the weights (P7, P5), an empty mel band, the generic kernel's
DCT with n_out > 64, n_mel % 4 != 0, an odd frame_len, a 65-bin band and 128 bands, F = 1, 2, 3, 4, 5, 14 (7-wave form), 15
(ragged second workgroup) and 28, DCT groups that mix the quads of two clips, a persistent grid with an uneven quad split.

Worst measured error / bar per plan and stage on an MI355X (`pytest -s` prints every case's figures as `stft-err` lines;
`logmel|mag` = log-mel against float64 from the device's magnitudes, `dct|logmel` = features against float64 from the
device's log-mel rows, generic kernel only; the MFCC and chain bars are per case, the one shown is the worst case's).
The log-mel column is the worst element among the 99.97 % that carry the flat bar:

  plan  mag / 2.3e-6   logmel / 5e-6   logmel|mag / 5e-6   mfcc / bar            dct|logmel / bar
  P1    1.26e-6        1.98e-6         1.14e-6             4.69e-5 / 1.05e-4
  P2    8.5e-7         1.15e-6         1.14e-6             2.56e-5 / 9.67e-5
  P3    1.22e-6        2.29e-6         2.29e-6             5.33e-5 / 1.04e-4
  P4    9.0e-7         1.15e-6         1.14e-6             1.42e-5 / 7.04e-5
  P5    1.31e-6        2.29e-6         2.29e-6             5.33e-5 / 1.04e-4
  P6    8.2e-7         1.35e-6         1.18e-6             4.69e-5 / 1.05e-4
  P7    9.1e-7         1.15e-6         1.14e-6             2.52e-5 / 7.42e-5
  G1    1.21e-6        1.86e-6         1.14e-6             1.63e-5 / 1.05e-4     1.09e-6 / 6.46e-5
  G2    1.04e-6        1.26e-6         1.14e-6             3.10e-5 / 1.04e-4     1.67e-5 / 8.02e-4
  G3    1.19e-6        4.22e-6         1.14e-6             1.63e-5 / 1.05e-4     9.3e-7 / 6.03e-5
  G4    1.11e-6        1.15e-6         1.14e-6             7.85e-6 / 4.69e-5     9.8e-7 / 1.36e-5
  G5    9.8e-7         1.59e-6         1.15e-6             6.41e-5 / 1.33e-4     4.58e-5 / 1.69e-3

Nearly empty bands.  At 0.03 % of the elements a band's mel sum in one frame is so small (a narrow low band that happens to
cancel, or the row scaled by 2^-10) that half an ulp of the frame's largest bin, through d log(s) = ds / s, is already more
than 5e-6 of log-mel; there the bar is 5e-6 plus exactly that (stft_cases.logmel_bar has the float64 argument, the CPU
test bounds the share).  Six cases have such an element over the flat 5e-6, error / element bar:
  P1-L1120-B7      1.07e-5 / 6.09e-5 at clip 2 (first 60 % silent) frame 4 band 1,  mel sum 5.8e-3
  P1-L1120-B1600   1.10e-5 / 6.89e-5 at clip 1220 frame 2 band 1,                   mel sum 4.2e-3
  P6-L1362-B7      8.50e-6 / 2.07e-5 at clip 3 (x 2^-10) frame 4 band 2,            mel sum 1.7e-5
  G1-L2720-B3      6.77e-6 / 1.41e-5 at clip 2 (x 2^-10) frame 11 band 8,           mel sum 3.7e-5
  G1-L4800-B7      6.71e-6 / 3.56e-5 at clip 5 frame 21 band 1,                     mel sum 1.1e-2
  G5-L480-B13      5.31e-6 / 1.86e-5 at clip 0 frame 0 band 15,                     mel sum 2.4e-2
Magnitudes and the mel / log stage are inside their flat bars at all of them (columns 1 and 3): the device's magnitude error
there is 1e-10 - 1.3e-7, and scipy's complex64 rfft gives 1.45e-5 on the first.
What the cases exposed and this suite now pins: a clip of NaN samples came out as the features of silence on a plan with a log
floor (fmaxf drops the NaN; both kernels), and the generic kernel's DCT, one fma chain, drifted by 1.8e-4 on a silent clip's
constant row at 128 bands (over the MFCC bar of 1.33e-4; four interleaved chains: 6.4e-5)."""
import ctypes

import numpy as np
import pytest
import torch

import stft_cases as SC
from speech_recognition_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 4096                       # words on each side (16-byte lines: the window's alignment is its offset's)
SENT = 0x7FC0DEAD                  # a quiet-NaN payload no kernel produces (the method of tests/test_grouped_conv_gpu.py)

# plan -> stage -> (error, bar): the worst (by error / bar) over the plan's cases of this run, for whoever prints it
WORST = {}


class Guarded(object):
    """n floats between two runs of GUARD sentinel words (NaN as floats); the window starts `off` floats past a 16-byte line"""

    def __init__(self, n, init=None, off=0):
        self.n = n
        self.buf = torch.empty(n + 2 * GUARD + 4, dtype=torch.int32, device="cuda")
        self.buf.fill_(SENT)
        self.lo = GUARD + off
        self.view = self.buf[self.lo:self.lo + n].view(torch.float32)
        assert self.view.data_ptr() % 16 == 4 * off
        if init is not None:
            self.view.copy_(torch.from_numpy(np.array(init, dtype=np.float32).reshape(-1)).cuda())   # (a copy: the shared references are read-only)

    def ptr(self):
        return ctypes.c_void_p(self.view.data_ptr())

    def bits(self):
        torch.cuda.synchronize()
        return self.view.view(torch.int32).cpu().numpy().copy()

    def guards_intact(self):
        torch.cuda.synchronize()
        return bool((self.buf[:self.lo] == SENT).all()) and bool((self.buf[self.lo + self.n:] == SENT).all())

    def check(self, what):
        assert self.guards_intact(), "%s wrote outside its output" % what
        w = self.bits() != SENT
        assert w.all(), "%s left %d output elements unwritten" % (what, int((~w).sum()))

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf == SENT).all())


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return _lib.load()


def _create(lib, frame_len, step, fft_len, n_mel, n_out, tables):
    win = np.ascontiguousarray(tables["window"], dtype=np.float32)
    mel = np.ascontiguousarray(tables["mel"], dtype=np.float32)
    dct = np.ascontiguousarray(tables["dct"], dtype=np.float32)
    h = ctypes.c_void_p()
    rc = lib.kws_stft_plan_create(frame_len, step, fft_len, n_mel, n_out, win.ctypes.data_as(ctypes.c_void_p),
                                  mel.ctypes.data_as(ctypes.c_void_p), dct.ctypes.data_as(ctypes.c_void_p),
                                  tables["log_offset"], tables["log_floor"], ctypes.byref(h))
    return rc, h


@pytest.fixture(scope="module")
def plans(lib):
    """name -> plan handle, created on first use, destroyed with the module"""
    made = {}

    def get(name):
        if name not in made:
            p = SC.plan(name)
            rc, h = _create(lib, p["frame_len"], p["step"], 512, p["n_mel"], p["n_out"], p["tables"])
            assert rc == 0, lib.kws_last_error()
            made[name] = h
        return made[name]

    yield get
    torch.cuda.synchronize()
    for h in made.values():
        lib.kws_stft_plan_destroy(h)


def _width(p, kind):
    return {0: p["n_out"], 1: SC.NBINS, 2: p["n_mel"]}[kind]


def _run(lib, p, h, x, B, L, kind):
    """one launch into a fresh guarded output -> Guarded [B, F, width]"""
    F = lib.kws_stft_num_frames(h, L)
    assert F == SC.num_frames(p, L)
    out = Guarded(B * F * _width(p, kind))
    rc = lib.kws_stft_mel_f32(h, x.ptr(), B, L, out.ptr(), kind, _lib.stream_ptr())
    assert rc == 0, "kws_stft_mel_f32 failed (%d): %s" % (rc, lib.kws_last_error())
    out.check("kws_stft_mel_f32(kind=%d)" % kind)
    return out


def _f32(bits, B, p, kind):
    return bits.view(np.float32).reshape(B, -1, _width(p, kind))


def _note(name, case, figures):
    """print one case's figures; keep the worst per plan"""
    print("stft-err %-22s %s" % (case, "  ".join("%s %.3g/%.3g" % (k, v, bar) for k, (v, bar) in figures.items())))
    worst = WORST.setdefault(name, {})
    for k, (v, bar) in figures.items():
        if k not in worst or v / bar > worst[k][0] / worst[k][1]:
            worst[k] = (v, bar)


def _check_case(lib, plans, name, L, B, off):
    p, h = SC.plan(name), plans(name)
    r = SC.reference(name, L, B)
    x = Guarded(B * L, init=r["x"], off=off)
    x_bits = x.bits()
    got = {}
    for kind in (1, 2, 0):
        assert lib.kws_stft_mel_kernel(h, x.ptr(), L, kind) == SC.expected_kernel(p, L, kind, off == 0), (name, L, kind)
        first, second = _run(lib, p, h, x, B, L, kind).bits(), _run(lib, p, h, x, B, L, kind).bits()
        assert np.array_equal(first, second), "two runs of kind %d differ" % kind
        got[kind] = _f32(first, B, p, kind)
        assert got[kind].shape == {0: r["mfcc"], 1: r["mag"], 2: r["logmel"]}[kind].shape
        assert np.isfinite(got[kind]).all(), "kind %d" % kind
    assert x.guards_intact() and np.array_equal(x.bits(), x_bits)
    rows = SC.special_rows(B)
    if SC.NEGATED in rows:
        assert np.array_equal(got[1][rows[SC.NEGATED]].view(np.int32), got[1][0].view(np.int32)), "|X| of -x differs from |X| of x"
    # log-mel: the bar is per element (SC.logmel_bar: the flat LOGMEL_BAR but for the nearly empty bands); the figure is
    # the element closest to its bar
    lm_err, lm_bar = np.abs(got[2] - r["logmel"]), SC.logmel_bar(p, r)
    b, f, m = np.unravel_index((lm_err / lm_bar).argmax(), lm_err.shape)
    flat = lm_bar == SC.LOGMEL_BAR
    fig = {
        "mag": (np.abs(got[1] - r["mag"]).max(), SC.MAG_BAR),
        "logmel": (lm_err[b, f, m], lm_bar[b, f, m]),
        "logmel(flat)": (lm_err[flat].max(), SC.LOGMEL_BAR),
        # stage isolation: the mel + log stage alone, from the magnitudes the device itself stored
        "logmel|mag": (np.abs(got[2] - SC.logmel_of_mag(p, got[1])).max(), SC.LOGMEL_BAR),
        "mfcc": (np.abs(got[0] - r["mfcc"]).max(), SC.mfcc_bar(p["tables"], r["logmel"])),
    }
    if not p["shape"]:
        # the generic kernel's kind 0 is an fma chain over the very log-mel row its kind 2 stores
        replay = got[2].astype(np.float64) @ SC.tables32(p)[2]
        fig["dct|logmel"] = (np.abs(got[0] - replay).max(), SC.chain_bar(p, got[2]))
    _note(name, SC.case_id((name, L, B, off)), fig)
    # the log multiplies a magnitude error by 1 / (mel sum): say where the log-mel figure was taken
    where = "log-mel element closest to its bar: clip %d frame %d band %d, mel sum %.3g" % (b, f, m, np.exp(r["logmel"][b, f, m]))
    assert (lm_err <= lm_bar).all(), "%s: %d log-mel elements over their bars (%s)" % (
        SC.case_id((name, L, B, off)), int((lm_err > lm_bar).sum()), where)
    for k, (v, bar) in fig.items():
        assert v <= bar, "%s: %s error %.4g over its bar %.4g (%s)" % (SC.case_id((name, L, B, off)), k, v, bar, where)


@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_features_match_float64(case, lib, plans):
    _check_case(lib, plans, *case)


def test_features_match_float64_on_the_persistent_grid(lib, plans):
    """3200 quads on 256 workgroups: 12.5 quads each, so q_lo / q_hi alternate between 12 and 13 and every DCT group at a
    workgroup's end is partial"""
    name, L, B = SC.PERSISTENT
    _check_case(lib, plans, name, L, B, 0)


# ---------------------------------------------------------------------------------------------------------------------------
# clip isolation
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1120, 1122])
@pytest.mark.parametrize("name", SC.ISOLATION_PLANS)
def test_a_clip_in_a_batch_is_the_clip_alone(name, L, lib, plans):
    """B = 7, F = 5: 14 quads, so stft4's DCT groups hold quads of two or three clips, and the generic kernel's workgroups one
    clip each.  The splits use fixed power-of-two scales and the rows of a matrix product are independent: a clip's features
    do not depend on its neighbours, bit for bit - nor on NaN neighbours, nor on NaN words before and after the batch."""
    p, h = SC.plan(name), plans(name)
    B = 7
    xh = SC.inputs(name, L, B)
    x = Guarded(B * L, init=xh)
    batch = dict((kind, _f32(_run(lib, p, h, x, B, L, kind).bits(), B, p, kind)) for kind in (0, 1, 2))
    for kind in (0, 1, 2):
        assert np.isfinite(batch[kind]).all()
    for b in range(B):
        off = ((x.view.data_ptr() + 4 * b * L) % 16) // 4           # the same alignment as inside the batch
        alone = Guarded(L, init=xh[b], off=off)
        for kind in (0, 1, 2):
            assert lib.kws_stft_mel_kernel(h, alone.ptr(), L, kind) == lib.kws_stft_mel_kernel(h, x.ptr(), L, kind)
            one = _f32(_run(lib, p, h, alone, 1, L, kind).bits(), 1, p, kind)
            assert np.array_equal(one[0].view(np.int32), batch[kind][b].view(np.int32)), "clip %d, kind %d" % (b, kind)
    bad = (2, 5)
    xn = xh.copy()
    xn[list(bad)] = np.nan
    x2 = Guarded(B * L, init=xn)
    for kind in (0, 1, 2):
        g = _f32(_run(lib, p, h, x2, B, L, kind).bits(), B, p, kind)
        for b in range(B):
            if b in bad:
                assert np.isnan(g[b]).all(), "kind %d: rows of the NaN clip %d are not all NaN" % (kind, b)
            else:
                assert np.array_equal(g[b].view(np.int32), batch[kind][b].view(np.int32)), "clip %d, kind %d" % (b, kind)
    assert x.guards_intact() and x2.guards_intact()


# ---------------------------------------------------------------------------------------------------------------------------
# refusals, frame counts
# ---------------------------------------------------------------------------------------------------------------------------
def test_refused_arguments_leave_the_output_alone(lib, plans):
    p, h = SC.plan("P1"), plans("P1")
    x = Guarded(3 * 1122, init=np.zeros(3 * 1122, np.float32))
    out = Guarded(3 * 5 * SC.NBINS)
    S = _lib.stream_ptr()
    for B, L, kind in ((3, 1121, 0), (3, 478, 0), (3, 478, 1), (0, 1120, 0), (3, 1120, 3), (3, 1120, -1)):
        assert lib.kws_stft_mel_f32(h, x.ptr(), B, L, out.ptr(), kind, S) != 0, (B, L, kind)
        assert out.untouched()
        assert lib.kws_stft_mel_kernel(h, x.ptr(), L, kind) == (13 if (L, kind) == (1120, 0) else -1)   # (the query has no B)
    assert lib.kws_stft_mel_f32(h, None, 3, 1120, out.ptr(), 0, S) != 0 and lib.kws_stft_mel_kernel(h, None, 1120, 0) == -1
    assert lib.kws_stft_mel_kernel(None, x.ptr(), 1120, 0) == -1
    assert out.untouched()
    # plan creation: odd frame_step, fft_len != 512, n_mel = 129, n_out = n_mel + 129
    t = p["tables"]
    big = dict(t, mel=np.zeros((SC.NBINS, 129), np.float32), dct=np.zeros((129, 258), np.float32))
    for args in ((480, 161, 512, 80, 60, t), (480, 160, 256, 80, 60, t), (480, 160, 1024, 80, 60, t), (480, 160, 512, 129, 60, big),
                 (480, 160, 512, 80, 80 + 129, big)):
        rc, hh = _create(lib, *args)
        assert rc != 0 and not hh.value, args[:5]
    assert lib.kws_stft_mel_f32(h, x.ptr(), 3, 1120, out.ptr(), 0, S) == 0      # the plan still works


@pytest.mark.parametrize("name", ["P1", "P6", "G3"])
def test_num_frames(name, lib, plans):
    p, h = SC.plan(name), plans(name)
    for L480, F in SC.L_480:
        L = SC.length_for(p, L480)
        assert lib.kws_stft_num_frames(h, L) == 1 + (L - p["frame_len"]) // p["step"] == F
    for L in (16000, 16002, p["frame_len"], p["frame_len"] + p["step"] - 1, p["frame_len"] + p["step"]):
        assert lib.kws_stft_num_frames(h, L) == 1 + (L - p["frame_len"]) // p["step"]
    for L in (p["frame_len"] - 1, p["frame_len"] - 2, 1, 0):
        assert lib.kws_stft_num_frames(h, L) == 0
