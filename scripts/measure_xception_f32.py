"""xception_with_attention: the float64 oracle net (tests/xception_oracle.py) run in float32 against itself in float64 on the CPU, at
the two cases of tests/test_xception_models_gpu.py - the figures that test's bars are checked against (a bar stands while the
figure is under half of it).  No GPU needed.
usage: python3 scripts/measure_xception_f32.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from xception_oracle import net_float32_figures  # noqa: E402

if __name__ == '__main__':
    for B, input_size in ((8, 16000), (40, 4000)):
        print(json.dumps(dict(net_float32_figures(B, input_size), batch=B, input_size=input_size)))
