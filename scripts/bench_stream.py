"""Keyword spotting over a ten-minute recording with the headline model (stream.spot, hop 320):
python scripts/bench_stream.py [minutes] [out.json]

The recording is synthetic and made here from a seed: int16 noise plus a few hundred planted one-second tone bursts at known
offsets.  The model keeps its fresh initialisation (the timing does not depend on the weights, the detections mean nothing).
Reported:
  spot       wall time of the whole stream.spot (upload, windows, net, smoothing, the copy back and the host state machine;
             host clock around a call that ends in a device synchronise; median of `SPOT_RUNS` runs after a warm-up), as recording
             seconds per wall second;
  frames     kws_stream_frames_i16 alone at batch 1024 and 4096 windows of 16000 samples, against a device fill and a
             device-to-device copy of the same output bytes: device events around `REPS` launches, the three kinds of launch
             alternating window by window in the same run, median of `ROUNDS` windows each; the ratios are the figures to keep;
  smooth     the one kws_stream_smooth_f32 launch over the whole track;
  shares     device time of the three stages of one pass over the recording in chunks of 1024 (each stage's launches alone
             between device events) - the share of the net."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from speech_recognition_amd import _lib, stream  # noqa: E402
from speech_recognition_amd.model import speech_model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINUTES = float(sys.argv[1]) if len(sys.argv) > 1 else 10.0
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "stream_bench.json")
RATE, WIN, HOP, BATCH = 16000, 16000, 320, 1024
SPOT_RUNS, REPS, ROUNDS = 7, 10, 9


def recording(minutes, seed=1234, planted=300):
    """(int16 samples, [(class, end sample)]): noise at a quiet level and `planted` one-second tone bursts, evenly spread
    with a seeded jitter, whose frequency names a class."""
    rng = np.random.RandomState(seed)
    n = int(minutes * 60 * RATE)
    x = rng.normal(0.0, 300.0, n)
    planted = min(planted, max(n // (2 * RATE) - 1, 0))
    truth = []
    t = np.arange(RATE) / float(RATE)
    env = np.hanning(RATE)
    for k in range(planted):
        at = int((k + 0.5) * n / planted) - RATE // 2 + int(rng.randint(-2000, 2001))
        at = min(max(at, 0), n - RATE)
        c = 2 + k % 10
        x[at:at + RATE] += 8000.0 * env * np.sin(2 * np.pi * (200.0 + 150.0 * c) * t)
        truth.append((c, at + RATE))
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16), truth


def events_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def alternate(fns, reps=REPS, rounds=ROUNDS):
    """{name: (median, min, max) us per launch}: the launches compared take turns, window by window."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(events_us(fn, reps))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in out.items()}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_stream: no GPU (this measurement has no CPU form)")
    model = speech_model('conv_1d_time_sliced_with_attention', WIN, 12)
    net = model.net
    x, truth = recording(MINUTES)
    n = len(x)
    W = stream.plan_windows(n, WIN, HOP)
    res = {"device": torch.cuda.get_device_name(0), "model": "conv_1d_time_sliced_with_attention (fresh initialisation)",
           "recording_seconds": n / float(RATE), "samples": n, "planted_bursts": len(truth), "hop": HOP, "win": WIN, "windows": W,
           "batch": BATCH,
           "note": "spot: host clock around stream.spot of the host int16 recording, median of %d runs after 2 warm-up runs; "
                   "frames / fill / copy / smooth / shares: device events around %d launches (shares: around one pass), median "
                   "of %d windows, the compared launches alternating" % (SPOT_RUNS, REPS, ROUNDS)}

    # ---- the whole spot -------------------------------------------------------------------------------------------------------
    for _ in range(2):
        r = stream.spot(model, x, hop=HOP, batch=BATCH)
    walls = []
    for _ in range(SPOT_RUNS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = stream.spot(model, x, hop=HOP, batch=BATCH)
        walls.append(time.perf_counter() - t0)
    wall = statistics.median(walls)
    res["spot"] = {"wall_ms": round(wall * 1e3, 2), "wall_ms_min": round(min(walls) * 1e3, 2), "wall_ms_max": round(max(walls) * 1e3, 2),
                   "recording_seconds_per_wall_second": round(n / float(RATE) / wall, 1),
                   "windows_per_second": round(W / wall, 0), "average_windows": r.average_windows,
                   "detections": len(r.detections)}
    print("spot: %.1f s of audio, %d windows in %.1f ms (%.1f - %.1f): %.0f recording seconds per wall second"
          % (n / float(RATE), W, wall * 1e3, min(walls) * 1e3, max(walls) * 1e3, n / float(RATE) / wall))

    # ---- the gather alone against a fill and a copy of its output bytes ----------------------------------------------------------
    xd = torch.from_numpy(x).cuda()
    s = _lib.stream_ptr()
    res["frames"] = {}
    for batch in (1024, 4096):
        cnt = min(batch, W)
        buf = torch.empty((cnt, WIN), dtype=torch.float32, device="cuda")
        other = torch.empty_like(buf)

        def gather():
            _lib.call("kws_stream_frames_i16", _lib.ptr(xd), n, 0, HOP, WIN, stream.INT16_SCALE, _lib.ptr(buf), cnt, s)

        t = alternate({"frames": gather, "fill": lambda: buf.fill_(1.0), "copy": lambda: buf.copy_(other)})
        nbytes = 4 * cnt * WIN
        row = {"windows": cnt, "out_bytes": nbytes}
        for k, (med, lo, hi) in t.items():
            row[k + "_us"], row[k + "_us_min"], row[k + "_us_max"] = round(med, 2), round(lo, 2), round(hi, 2)
            row[k + "_out_gb_per_s"] = round(nbytes / med / 1e3, 1)
        row["frames_over_fill"] = round(t["frames"][0] / t["fill"][0], 3)
        row["frames_over_copy"] = round(t["frames"][0] / t["copy"][0], 3)
        row["frames_rate_over_fill_rate"] = round(t["fill"][0] / t["frames"][0], 3)
        res["frames"][str(batch)] = row
        print("frames batch %d: %.1f us (%.0f GB/s of stores); fill %.1f us, copy %.1f us: %.2f x the fill, %.2f x the copy"
              % (batch, t["frames"][0], row["frames_out_gb_per_s"], t["fill"][0], t["copy"][0], row["frames_over_fill"],
                 row["frames_over_copy"]))
        del buf, other

    # ---- the smoothing launch and the stages' shares ----------------------------------------------------------------------------
    probs = torch.from_numpy(r.probs).cuda()
    A = r.average_windows
    med, lo, hi = alternate({"smooth": lambda: stream.smooth(probs, A)})["smooth"]
    res["smooth"] = {"us": round(med, 2), "us_min": round(lo, 2), "us_max": round(hi, 2), "W": W, "NC": 12, "A": A}
    print("smooth [%d, 12], A = %d: %.1f us" % (W, A, med))

    buf = torch.empty((BATCH, WIN), dtype=torch.float32, device="cuda")
    out = torch.empty((W, 12), dtype=torch.float32, device="cuda")
    chunks = [(w0, min(w0 + BATCH, W)) for w0 in range(0, W, BATCH)]

    def all_frames():
        for w0, w1 in chunks:
            stream.frames(xd, WIN, HOP, first=w0, count=w1 - w0, out=buf)

    def all_net():
        for w0, w1 in chunks:
            net.predict(buf[:w1 - w0], out=out[w0:w1])

    t = alternate({"frames": all_frames, "net": all_net, "smooth": lambda: stream.smooth(out, A)}, reps=1)
    total = sum(v[0] for v in t.values())
    res["shares"] = {"chunks": len(chunks), "device_us": {k: round(v[0], 1) for k, v in t.items()}, "device_us_total": round(total, 1),
                     "net_share": round(t["net"][0] / total, 3), "frames_share": round(t["frames"][0] / total, 3),
                     "smooth_share": round(t["smooth"][0] / total, 3),
                     "device_total_over_spot_wall": round(total / (wall * 1e6), 3)}
    print("one pass: frames %.0f us, net %.0f us, smooth %.0f us: the net is %.1f %% of the device time, the device time %.1f %% "
          "of spot's wall time" % (t["frames"][0], t["net"][0], t["smooth"][0], 100 * res["shares"]["net_share"],
                                   100 * res["shares"]["device_total_over_spot_wall"]))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
