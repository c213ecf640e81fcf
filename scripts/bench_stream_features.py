"""Keyword spotting with the feature-input models over a ten-minute recording: overlapping windows on shared STFT frames
(stream.Features.rows, the default of stream.spot(features=)) against every window's own feature step (share_frames=False):
python scripts/bench_stream_features.py [minutes] [out.json]

The recording is synthetic and made here from a seed (int16 noise plus planted tone bursts); the models keep their fresh
initialisation (the timing does not depend on the weights).  hop 320, batch 1024, conv_1d_log_mfcc (rows of 98 x 40) and
conv_1d_spec (98 x 257).  Reported, per model:
  spot       wall time of the whole stream.spot, shared and per window taking turns run by run in the same process (host clock
             around a call that ends in a device synchronise; median, minimum and maximum of `SPOT_RUNS` runs after a warm-up),
             and whether the two posterior tracks are equal bit for bit;
  pass       device time of one pass over the recording - feature step and net for every chunk, no host synchronisation -
             both ways, and of the feature step alone both ways (device events around a pass, the compared passes taking
             turns, median of `ROUNDS`).
And for kws_stream_gather_f32 alone, against a device-to-device copy and a device fill of the same output bytes (device events
around `REPS` launches, the three taking turns, median of `ROUNDS`): 1024 dense rows of 98 x 40 out of a track, 1024 rows of
98 x 257 (25186 floats: the rows' alignment rotates), and 1024 composite rows [98 x 40 | 16000] by its two calls."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from speech_recognition_amd import stream  # noqa: E402
from speech_recognition_amd.model import prepare_model_settings, speech_model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINUTES = float(sys.argv[1]) if len(sys.argv) > 1 else 10.0
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "stream_features_bench.json")
RATE, WIN, HOP, BATCH = 16000, 16000, 320, 1024
SPOT_RUNS, REPS, ROUNDS = 5, 10, 7
MODELS = (('conv_1d_log_mfcc', 'mfcc'), ('conv_1d_spec', 'spec'))


def recording(minutes, seed=1234, planted=300):
    """int16 samples: noise at a quiet level and `planted` one-second tone bursts, evenly spread with a seeded jitter."""
    rng = np.random.RandomState(seed)
    n = int(minutes * 60 * RATE)
    x = rng.normal(0.0, 300.0, n)
    planted = min(planted, max(n // (2 * RATE) - 1, 0))
    t = np.arange(RATE) / float(RATE)
    env = np.hanning(RATE)
    for k in range(planted):
        at = int((k + 0.5) * n / planted) - RATE // 2 + int(rng.randint(-2000, 2001))
        at = min(max(at, 0), n - RATE)
        x[at:at + RATE] += 8000.0 * env * np.sin(2 * np.pi * (200.0 + 150.0 * (2 + k % 10)) * t)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def events_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def alternate(fns, reps=REPS, rounds=ROUNDS, warm=3):
    """{name: (median, min, max) us per call}: the calls compared take turns, round by round."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(events_us(fn, reps))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in out.items()}


def spread(prefix, t, row):
    row[prefix + "_us"], row[prefix + "_us_min"], row[prefix + "_us_max"] = (round(v, 2) for v in t)


def bench_model(name, rep, x, xd, res):
    s = prepare_model_settings(12, RATE, 1000, 30.0, 10.0, 40, 40, output_representation=rep)
    model = speech_model(name, s['fingerprint_size'], num_classes=12, **s)
    net = model.net
    f = stream.Features(s, output_representation=rep)
    n = len(x)
    W = stream.plan_windows(n, WIN, HOP)
    chunks = [(w0, min(w0 + BATCH, W)) for w0 in range(0, W, BATCH)]
    _, J, r = stream.plan_rows(BATCH, HOP, WIN, f.frame_len, f.step)
    row = {"representation": rep, "row_floats": f.row, "windows": W, "chunks": len(chunks),
           "frames_per_full_chunk": {"per_window": BATCH * f.F, "shared": J, "ratio": round(BATCH * f.F / float(J), 1)}}

    # ---- the whole spot, the two ways taking turns ------------------------------------------------------------------------------
    got = {}
    for share in (True, False):
        got[share] = stream.spot(model, x, hop=HOP, batch=BATCH, features=f, share_frames=share)      # warm-up
    row["probs_equal_bit_for_bit"] = got[True].probs.tobytes() == got[False].probs.tobytes()
    row["detections_equal"] = got[True].detections == got[False].detections
    walls = {True: [], False: []}
    for _ in range(SPOT_RUNS):
        for share in (True, False):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stream.spot(model, x, hop=HOP, batch=BATCH, features=f, share_frames=share)
            walls[share].append((time.perf_counter() - t0) * 1e3)
    for share, key in ((True, "shared"), (False, "per_window")):
        v = walls[share]
        row["spot_wall_ms_" + key] = round(statistics.median(v), 2)
        row["spot_wall_ms_" + key + "_min"], row["spot_wall_ms_" + key + "_max"] = round(min(v), 2), round(max(v), 2)
    row["spot_wall_per_window_over_shared"] = round(row["spot_wall_ms_per_window"] / row["spot_wall_ms_shared"], 3)
    row["recording_seconds_per_wall_second_shared"] = round(n / float(RATE) / (row["spot_wall_ms_shared"] * 1e-3), 1)

    # ---- one pass on the device: feature step + net, and the feature step alone ------------------------------------------------
    rows_buf = torch.empty((BATCH, f.row), dtype=torch.float32, device="cuda")
    win_buf = torch.empty((BATCH, WIN), dtype=torch.float32, device="cuda")
    probs = torch.empty((W, 12), dtype=torch.float32, device="cuda")

    def shared_features(predict=False):
        for w0, w1 in chunks:
            rows = f.rows(xd, HOP, 0, w0, w1 - w0, out=rows_buf)
            if predict:
                net.predict(rows, out=probs[w0:w1])

    def window_features(predict=False):
        for w0, w1 in chunks:
            rows = f.windows(stream.frames(xd, WIN, HOP, first=w0, count=w1 - w0, out=win_buf), out=rows_buf)
            if predict:
                net.predict(rows, out=probs[w0:w1])

    t = alternate({"pass_shared": lambda: shared_features(True), "pass_per_window": lambda: window_features(True),
                   "features_shared": shared_features, "features_per_window": window_features}, reps=1, warm=2)
    for k, v in t.items():
        spread(k, v, row)
    row["pass_per_window_over_shared"] = round(t["pass_per_window"][0] / t["pass_shared"][0], 3)
    row["features_per_window_over_shared"] = round(t["features_per_window"][0] / t["features_shared"][0], 2)
    row["features_share_of_pass_shared"] = round(t["features_shared"][0] / t["pass_shared"][0], 4)
    row["features_share_of_pass_per_window"] = round(t["features_per_window"][0] / t["pass_per_window"][0], 4)
    res["models"][name] = row
    print("%s: spot %.1f ms shared (%.1f - %.1f), %.1f ms per window (%.1f - %.1f); one pass on the device %.0f against %.0f us; "
          "the feature step alone %.0f against %.0f us (%.1f x); probs equal: %s"
          % (name, row["spot_wall_ms_shared"], row["spot_wall_ms_shared_min"], row["spot_wall_ms_shared_max"],
             row["spot_wall_ms_per_window"], row["spot_wall_ms_per_window_min"], row["spot_wall_ms_per_window_max"],
             t["pass_shared"][0], t["pass_per_window"][0], t["features_shared"][0], t["features_per_window"][0],
             row["features_per_window_over_shared"], row["probs_equal_bit_for_bit"]))
    f.close()


def bench_gather(res):
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    F, frames_in_track = 98, (BATCH - 1) * 2 + 98
    cases = {}
    for name, width in (("dense_98x40", 40), ("spectrogram_98x257", 257)):
        track = torch.randn(frames_in_track * width, generator=g, device="cuda")
        out = torch.empty(BATCH * F * width, dtype=torch.float32, device="cuda")
        cases[name] = (out, lambda track=track, out=out, width=width: stream.gather(track, track.numel(), 0, 2 * width, F * width, out,
                                                                                  F * width, BATCH))
    track = torch.randn(frames_in_track * 40, generator=g, device="cuda")
    P = torch.randn((BATCH - 1) * HOP + WIN, generator=g, device="cuda")
    pitch = F * 40 + WIN
    comp = torch.empty(BATCH * pitch, dtype=torch.float32, device="cuda")

    def composite():
        stream.gather(track, track.numel(), 0, 80, F * 40, comp, pitch, BATCH)
        stream.gather(P, P.numel(), 0, HOP, WIN, comp, pitch, BATCH, out_offset=F * 40)

    cases["composite_98x40_and_16000"] = (comp, composite)
    for name, (out, fn) in cases.items():
        other = torch.empty_like(out)
        t = alternate({"gather": fn, "copy": lambda: out.copy_(other), "fill": lambda: out.fill_(1.0)})
        row = {"rows": BATCH, "out_bytes": 4 * out.numel(), "launches": 2 if name.startswith("composite") else 1}
        for k, v in t.items():
            spread(k, v, row)
        row["gather_over_copy"] = round(t["gather"][0] / t["copy"][0], 3)
        row["gather_over_fill"] = round(t["gather"][0] / t["fill"][0], 3)
        row["gather_out_gb_per_s"] = round(4 * out.numel() / t["gather"][0] / 1e3, 1)
        res["gather"][name] = row
        print("gather %s: %.1f us (%.0f GB/s of stores); copy %.1f us, fill %.1f us: %.2f x the copy, %.2f x the fill"
              % (name, t["gather"][0], row["gather_out_gb_per_s"], t["copy"][0], t["fill"][0], row["gather_over_copy"],
                 row["gather_over_fill"]))


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_stream_features: no GPU (this measurement has no CPU form)")
    x = recording(MINUTES)
    xd = torch.from_numpy(x).cuda()
    res = {"device": torch.cuda.get_device_name(0), "recording_seconds": len(x) / float(RATE), "samples": len(x), "hop": HOP,
           "win": WIN, "batch": BATCH, "models": {}, "gather": {},
           "note": "spot: host clock around stream.spot of the host int16 recording, shared and per-window runs taking turns, "
                   "median of %d after a warm-up; pass_* / features_*: device events around one pass over the recording in "
                   "chunks of %d, median of %d rounds, the compared passes taking turns; gather: device events around %d "
                   "launches, median of %d rounds, gather / copy / fill taking turns" % (SPOT_RUNS, BATCH, ROUNDS, REPS, ROUNDS)}
    for name, rep in MODELS:
        bench_model(name, rep, x, xd, res)
    bench_gather(res)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
