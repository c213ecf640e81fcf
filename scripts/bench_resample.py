"""Resampling kernel timing at B one-second clips per source rate -> 16 kHz (int16 in, int16 out: the ingest launch):
python scripts/bench_resample.py [B] [out.json]

Per rate: microseconds per kws_resample_i16 launch (device events around `reps` launches, median of `rounds` windows), the
launch's in + out bytes, and those bytes over the copy rate measured in the same run (a device-to-device copy of the same
number of bytes, read + write counted like the launch's in + out).  Where scipy is importable, also the wall time of
scipy.signal.resample_poly on the same batch on the host; null otherwise."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from speech_recognition_amd import _lib  # noqa: E402
from speech_recognition_amd import resample as rs  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                         "resample_bench_b%d.json" % B)
RATES = (48000, 44100, 22050, 8000)
RATE_OUT = 16000


def window_us(fn, reps, rounds=7):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return statistics.median(out), min(out), max(out)


def main():
    try:
        from scipy import signal
        import scipy
        scipy_version = scipy.__version__
    except ImportError:
        signal, scipy_version = None, None
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    res = {"B": B, "rate_out": RATE_OUT, "device": torch.cuda.get_device_name(0), "scipy": scipy_version,
           "note": "int16 in, int16 out, one-second clips; us = median of 7 windows of `reps` launches between device events; "
                   "copy = torch device-to-device copy of (in + out) / 2 bytes (it reads and writes them: in + out bytes of traffic)"
                   + ("" if signal else "; scipy is not importable on this machine: scipy_ms is null"),
           "rates": {}}
    for rate in RATES:
        n_in = rate
        keep = rs.resampled_samples(n_in, rate, RATE_OUT)
        x = torch.randint(-32768, 32768, (B, n_in), generator=g, device="cuda", dtype=torch.int32).to(torch.int16)
        out = torch.empty((B, keep), dtype=torch.int16, device="cuda")
        plan = rs._plan(rate, RATE_OUT)
        s = _lib.stream_ptr()

        def launch():
            _lib.call("kws_resample_i16", plan, _lib.ptr(x), n_in, None, n_in, _lib.ptr(out), None, B, keep, s)

        nbytes = 2 * B * (n_in + keep)
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        us, lo, hi = window_us(launch, 50)
        cus, clo, chi = window_us(lambda: dst.copy_(src), 50)
        up, down, half, T = rs.design(rate, RATE_OUT)
        row = {"up": up, "down": down, "taps_per_output": T, "us": round(us, 2), "us_min": round(lo, 2), "us_max": round(hi, 2),
               "bytes_in_out": nbytes, "gb_per_s": round(nbytes / us / 1e3, 1), "copy_us": round(cus, 2),
               "copy_gb_per_s": round(nbytes / cus / 1e3, 1), "time_over_copy": round(us / cus, 2),
               "gflop_per_s": round(2.0 * B * keep * T / us / 1e3, 1), "scipy_ms": None}
        if signal is not None:
            xh = x.cpu().numpy().astype(np.float64)
            t0 = time.perf_counter()
            yh = signal.resample_poly(xh, up, down, axis=1)
            row["scipy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            got = out.cpu().numpy()[:64].astype(np.float64)
            row["max_abs_diff_vs_scipy_first_64_rows"] = float(np.abs(got - np.clip(np.rint(yh[:64, :keep]), -32768, 32767)).max())
        res["rates"][str(rate)] = row
        print("%d -> %d  B=%d: %.1f us (%.1f - %.1f)  %.0f GB/s in+out; copy of the same bytes %.1f us (%.0f GB/s): x%.2f;  scipy %s ms"
              % (rate, RATE_OUT, B, us, lo, hi, row["gb_per_s"], cus, row["copy_gb_per_s"], row["time_over_copy"], row["scipy_ms"]))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
