"""CPU checks of tests/stft_cases.py: the case table of tests/test_stft_kernels_gpu.py lands every plan on the kernel it is
in the table for (the host dispatch of csrc/stft.hip / csrc/stft4.hip replayed in NumPy), reaches the table corners it claims,
and its float64 reference agrees with a direct O(N^2) DFT."""
import numpy as np
import pytest

import stft_cases as SC
from oracle import features as OF


@pytest.mark.parametrize("name", SC.PLANS)
def test_every_plan_lands_on_the_kernel_the_table_says(name):
    p = SC.plan(name)
    rp = SC.replay_plan(p)
    for L480, F in SC.L_480:
        L = SC.length_for(p, L480)
        assert SC.num_frames(p, L) == F
        for aligned in (True, False):
            for kind in (0, 1, 2):
                got = SC.replay_kernel(p, L, kind, aligned, rp)
                assert got == SC.expected_kernel(p, L, kind, aligned), (name, L, kind, aligned)
                if kind:                                   # the other output kinds always run the generic kernel
                    assert got == (1 if F % 14 == 0 else 0)
    if p["shape"]:
        assert rp["shape"] == p["shape"] and rp["lds_bytes"] <= SC.LDS_CAP
        # both load widths of the instance are in the table
        codes = set(SC.expected_kernel(p, c[1], 0, c[3] == 0) for c in SC.CASES if c[0] == name)
        assert codes == {10 + 2 * p["shape"], 11 + 2 * p["shape"]}


def test_the_plans_are_generic_for_the_reason_the_table_gives():
    rp = dict((n, SC.replay_plan(SC.plan(n))) for n in SC.PLANS)
    # G1, G2, G3 have tables stft4 would serve (shape 1): only n_out, n_mel % 4 and the odd frame_len keep them off it
    for n in ("G1", "G2", "G3"):
        assert rp[n]["shape"] == 1
    assert SC.plan("G1")["n_out"] > 64 and SC.plan("G2")["n_mel"] % 4 != 0 and SC.plan("G3")["frame_len"] % 2 == 1
    assert rp["G4"]["mel_mc"] == [17] and rp["G4"]["mel_maxw"] == 0 and rp["G4"]["band_cnt"].max() == 65
    assert SC.plan("G5")["n_mel"] == 128 and len(rp["G5"]["mel_mc"]) == 8 and rp["G5"]["shape"] == 0
    # the never-launched instances
    assert rp["P2"]["mel_mc"] == [2, 2, 3, 4, 4] and rp["P4"]["mel_mc"] == [3, 7, 8]
    assert SC.plan("P2")["n_mel"] % 16 != 0
    last = rp["P2"]["band_start"][-1] + rp["P2"]["band_cnt"][-1] - 1
    assert last == 255                                      # every shipped table ends at bin 243 or 127


def test_p7_takes_the_host_clamp_has_an_empty_band_and_weight_on_the_nyquist_bin():
    p = SC.plan("P7")
    rp = SC.replay_plan(p)
    mel = np.asarray(p["tables"]["mel"], np.float32)
    assert rp["mel_mc"] == [2, 8, 2] and rp["mel_maxw"] == 32 and rp["shape"] == 4
    assert rp["clamped"] == [38, 39]
    for m in rp["clamped"]:                                 # the band sits later in its (moved) window
        assert rp["mel_ws"][m] == SC.MAGF - 32 < rp["band_start"][m]
        assert rp["band_start"][m] + rp["band_cnt"][m] <= rp["mel_ws"][m] + 32
    assert rp["band_cnt"][5] == 0 and not mel[:, 5].any()
    assert mel[256, 39] > 0 and rp["band_start"][39] == 250 and rp["band_cnt"][39] == 7
    assert rp["band_cnt"][20] == 29


def test_p5_takes_the_shift_of_the_table_image():
    """a band of lane group 2 whose plan window (mel_maxw taps from mel_ws) stays inside the 260-float row - no host clamp -
    while the 32 taps the kernel instance reads from there run past it: stft4_tables moves the window back and shifts the
    weights (stft4.hip: `win = ws0 + taps <= MAGF ? ws0 : MAGF - taps`)"""
    p = SC.plan("P5")
    rp = SC.replay_plan(p)
    assert rp["shape"] == 3 and rp["mel_maxw"] == 28 and not rp["clamped"]
    shifted = [m for m in range(32, 40) if rp["mel_ws"][m] + SC.kernel_taps(3, m) > SC.MAGF]
    assert shifted and SC.kernel_taps(3, 39) == 32
    for m in shifted:
        assert rp["mel_ws"][m] + rp["mel_maxw"] <= SC.MAGF
        assert rp["band_cnt"][m] > 0                        # ... and the shifted weights are not all zero
    # no other plan of the table takes it: P5 is the case that would notice
    for n in SC.PLANS:
        q = SC.plan(n)
        if q["shape"] and n != "P5":
            rq = SC.replay_plan(q)
            assert not [m for m in range(q["n_mel"]) if m not in rq["clamped"] and
                        rq["mel_ws"][m] + SC.kernel_taps(q["shape"], m) > SC.MAGF]


def test_frame_counts_and_batches_cover_the_edges():
    F = set(SC.F_LIST)
    assert {f % 4 for f in F} == {0, 1, 2, 3} and {1, 14, 15} <= F
    assert any(L % 4 == 2 for L, _ in SC.L_480)
    for name in SC.PLANS:
        mine = [c for c in SC.CASES if c[0] == name]
        p = SC.plan(name)
        fs = set(SC.num_frames(p, c[1]) for c in mine)
        assert {f % 4 for f in fs} == {0, 1, 2, 3} and {1, 14, 15} <= fs
        assert any(c[3] for c in mine)                      # one unaligned batch
        assert (name, SC.length_for(p, 480), 13, 0) in mine and (name, SC.length_for(p, 1120), 7, 0) in mine
        if name in SC.FULL_GRID:
            assert len(mine) == len(SC.L_480) * len(SC.BATCHES) + 1
    assert set(c[2] for c in SC.CASES) == set(SC.BATCHES)
    # the persistent grid: more quads than 12 x 256, dealt unevenly
    name, L, B = SC.PERSISTENT
    quads = B * ((SC.num_frames(SC.plan(name), L) + 3) // 4)
    assert quads > 12 * 256 and quads % 256 != 0
    assert len(set(SC.case_id(c) for c in SC.CASES)) == len(SC.CASES)


def test_inputs_hold_the_special_rows():
    x = SC.inputs("P1", 1120, 7)
    r = SC.special_rows(7)
    assert not x[r[SC.SILENT]].any()
    assert not x[r[SC.HALF_SILENT], :672].any() and x[r[SC.HALF_SILENT], 672:].all()
    assert np.abs(x[r[SC.SMALL]]).max() < 1e-3 and np.array_equal(x[r[SC.NEGATED]], -x[0])
    assert np.abs(x).max() < 0.5                            # no full-scale rows
    assert sorted(SC.special_rows(3)) == [SC.SILENT, SC.HALF_SILENT, SC.SMALL] and not SC.special_rows(1)
    assert np.array_equal(x, SC.inputs("P1", 1120, 7)) and not np.array_equal(x[0], SC.inputs("P3", 1120, 7)[0])


def test_the_log_mel_bar_is_the_flat_one_almost_everywhere():
    """logmel_bar() leaves LOGMEL_BAR in place except at nearly empty bands: the exceptions stay a sliver of the table and of every
    case, never go below the flat bar, and hold no silent frame (nothing to amplify there)"""
    total = wide = 0
    for name, L, B, _ in SC.CASES + [SC.PERSISTENT + (0,)]:
        r = SC.reference(name, L, B)
        bar = SC.logmel_bar(SC.plan(name), r)
        assert bar.shape == r["logmel"].shape and (bar >= SC.LOGMEL_BAR).all() and np.isfinite(bar).all()
        w = bar > SC.LOGMEL_BAR
        assert w.mean() <= 0.01, (name, L, B, w.mean())
        assert not w[r["mag"].max(-1) == 0].any()
        total, wide = total + bar.size, wide + int(w.sum())
    assert 0 < wide <= 5e-4 * total, (wide, total)


@pytest.mark.parametrize("name", ["P1", "P3", "P6", "G3"])
def test_reference_agrees_with_a_direct_dft(name):
    """oracle.features against the definition X[k] = sum_n w[n] x[n] e^{-2 pi i k n / 512} summed in float64, on one 3-frame clip"""
    p = SC.plan(name)
    t = p["tables"]
    L = SC.length_for(p, 800)
    x = SC.inputs(name, L, 1)[0].astype(np.float64)
    mag, logmel, mfcc = OF.features(x[None], t, p["step"], dtype=np.float64, return_all=True)
    assert mag.shape == (1, 3, 257)
    n = np.arange(p["frame_len"])
    k = np.arange(257)
    E = np.exp(-2j * np.pi * ((k[:, None] * n[None, :]) % 512) / 512.0)
    win = np.asarray(t["window"], np.float64)
    for f in range(3):
        X = E @ (x[f * p["step"]:f * p["step"] + p["frame_len"]] * win)
        assert np.abs(np.abs(X) - mag[0, f]).max() < 1e-12
        mel = np.abs(X) @ np.asarray(t["mel"], np.float64) + t["log_offset"]
        if t["log_floor"] > 0:
            mel = np.maximum(mel, t["log_floor"])
        assert np.abs(np.log(mel) - logmel[0, f]).max() < 1e-10
        assert np.abs(np.log(mel) @ np.asarray(t["dct"], np.float64) - mfcc[0, f]).max() < 1e-9


def test_mfcc_bar_reproduces_the_bar_of_the_shipped_shapes():
    """the formula gives test_stft_mel_features' 1.1e-4 to within 15 % on both shipped shapes, on that test's inputs"""
    L = 16000
    tt = np.arange(L) / 16000.0
    for tables, seed in ((OF.tables_path_b(480, 80, 60), 80 + 480), (OF.tables_path_a(480, 16000, 40, 40), 40 + 480)):
        rng = np.random.RandomState(seed)
        x = (rng.randn(5, L) * 0.0774 + 0.05 * np.sin(2 * np.pi * 440 * tt)[None]).astype(np.float32)
        x[1] = 0.0
        _, lm, _ = OF.features(x.astype(np.float64), tables, 160, dtype=np.float64, return_all=True)
        bar = SC.mfcc_bar(tables, lm)
        assert 0.85 * 1.1e-4 <= bar <= 1.1e-4, bar
