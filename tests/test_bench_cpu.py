"""Host-side pieces of bench.py that need no GPU: the preflight watchdog of N > 1 runs."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(code, **env):
    e = dict(os.environ, **env)
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def test_watchdog_reports_and_kills_a_rank_that_hangs_in_its_first_collective():
    code = ("import sys, time; sys.argv = ['bench.py']; import bench\n"
            "dog = bench.PreflightWatchdog(sys.stdout, 8)\n"
            "dog.say('start')\n"
            "time.sleep(60)\n"
            "print('not reached')\n")
    res = _run(code, KWS_BENCH_PREFLIGHT_TIMEOUT="1")
    assert res.returncode == -9                         # SIGKILL from the fresh child, never an exec of the hung process
    lines = [l for l in res.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1, lines
    out = json.loads(lines[0])
    assert out["value"] is None and out["n_gpus"] == 8 and out["stage"] == "preflight all-reduce" and "watchdog" in out["error"]


def test_watchdog_covers_the_rendezvous_too_and_is_silent_when_all_is_well():
    hang_in_init = ("import sys, time; sys.argv = ['bench.py']; import bench\n"
                    "dog = bench.PreflightWatchdog(sys.stdout, 2)\n"
                    "time.sleep(60)\n")
    res = _run(hang_in_init, KWS_BENCH_INIT_TIMEOUT="1")
    assert res.returncode == -9 and json.loads(res.stdout.decode().strip())["stage"] == "init_process_group"
    fine = ("import sys, time; sys.argv = ['bench.py']; import bench\n"
            "dog = bench.PreflightWatchdog(sys.stdout, 2)\n"
            "dog.say('start'); time.sleep(0.2); dog.done()\n"
            "time.sleep(1.5)\n")                        # well past the limit: the watchdog has gone
    res = _run(fine, KWS_BENCH_PREFLIGHT_TIMEOUT="1")
    assert res.returncode == 0 and not res.stdout.strip(), (res.stdout, res.stderr)
    dies_by_itself = ("import sys; sys.argv = ['bench.py']; import bench\n"
                      "dog = bench.PreflightWatchdog(sys.stdout, 2)\n"
                      "raise SystemExit(5)\n")          # the rank ends on its own (it printed its own reason): pipe closes, no line
    res = _run(dies_by_itself, KWS_BENCH_PREFLIGHT_TIMEOUT="1")
    assert res.returncode == 5 and not res.stdout.strip()


def test_plain_run_turns_every_leg_beyond_the_headline_off():
    """Without --full the checker legs are off whatever else is asked; --full runs them unless a --no-* option says otherwise."""
    code = ("import sys, json; sys.argv = ['bench.py']; import bench\n"
            "keys = ('full', 'no_cpu_baseline', 'no_ab', 'no_configs', 'no_val_acc', 'profile_steps')\n"
            "for argv in ([], ['--profile-steps', '3'], ['--full'], ['--full', '--no-ab']):\n"
            "    a = bench.parse_args(argv)\n"
            "    print(json.dumps([getattr(a, k) for k in keys]))\n")
    res = _run(code)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    got = [json.loads(l) for l in res.stdout.decode().split("\n") if l.strip()]
    assert got == [[False, True, True, True, True, 5], [False, True, True, True, True, 3],
                   [True, False, False, False, False, 5], [True, False, True, False, False, 5]]


def test_dump_outputs_writes_float32_arrays_of_the_last_step(tmp_path):
    """--dump-outputs: one DIR/<name>.npy per array the timed path hands back, float32, values unchanged."""
    code = ("import sys, types, json, torch; d = sys.argv[1]; sys.argv = ['bench.py']; import bench\n"
            "g = torch.Generator().manual_seed(0)\n"
            "net = types.SimpleNamespace(params=torch.randn(1000, generator=g), state=torch.randn(40, generator=g),\n"
            "                            grads=torch.randn(1000, generator=g), slots=torch.rand(1000, generator=g))\n"
            "rows = torch.randn(7, 4, generator=g)\n"
            "names = bench.dump_outputs(d, net, rows)\n"
            "torch.save(dict(net.__dict__, metrics_per_step=rows), d + '/expected.pt')\n"
            "print(json.dumps(names))\n")
    d = str(tmp_path / "out")
    res = subprocess.run([sys.executable, "-c", code, d], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    names = json.loads(res.stdout.decode().strip().splitlines()[-1])
    assert names == ["params", "bn_state", "grads", "rmsprop_slots", "metrics_per_step"]
    import numpy as np
    import torch
    exp = torch.load(os.path.join(d, "expected.pt"))
    for name, key in zip(names, ["params", "state", "grads", "slots", "metrics_per_step"]):
        a = np.load(os.path.join(d, name + ".npy"))
        assert a.dtype == np.float32 and np.array_equal(a, exp[key].numpy()), name


def test_dump_outputs_limit_ends_every_rank_and_only_rank0_writes(tmp_path):
    """Off rank 0 (write=False) nothing is written, and an output over the limit raises on every rank alike, before a collective."""
    code = ("import sys, types, torch; d = sys.argv[1]; sys.argv = ['bench.py']; import bench\n"
            "net = types.SimpleNamespace(params=torch.zeros(10), state=torch.zeros(2), grads=torch.zeros(10), slots=torch.zeros(10))\n"
            "assert bench.dump_outputs(d, net, torch.zeros(3, 4), write=False) is None\n"
            "big = types.SimpleNamespace(params=torch.zeros(17 << 20), state=torch.zeros(2), grads=torch.zeros(10), slots=torch.zeros(10))\n"
            "for write in (False, True):\n"
            "    try:\n"
            "        bench.dump_outputs(d, big, torch.zeros(3, 4), write=write)\n"
            "    except SystemExit as e:\n"
            "        assert 'limit' in str(e)\n"
            "    else:\n"
            "        raise AssertionError('no limit')\n")
    d = str(tmp_path / "out")
    res = subprocess.run([sys.executable, "-c", code, d], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    assert not os.path.exists(d)
