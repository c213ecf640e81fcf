"""CPU check of the module-level drop-in: every name the reference's train.py / make_submission.py
import resolves through dropin/ (their import statements are stored in tests/golden/k9_script_imports.json,
made by tests/golden/make_golden_imports.py)."""
import importlib
import json
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'k9_script_imports.json')
STDLIB_OR_THIRD_PARTY = {'glob', 'os', 'numpy', 'pandas', 'tqdm', '__future__'}


@pytest.mark.parametrize("script", ["train.py", "make_submission.py"])
def test_reference_script_imports_resolve(script, repo_root, monkeypatch):
    monkeypatch.syspath_prepend(repo_root)
    monkeypatch.syspath_prepend(os.path.join(repo_root, 'dropin'))
    for m in ('tensorflow', 'keras', 'keras.backend', 'keras.callbacks', 'keras.models', 'IPython', 'input_data',
              'model', 'utils', 'classes', 'callbacks', 'audio'):
        sys.modules.pop(m, None)
    with open(GOLDEN) as f:
        imports = json.load(f)['scripts'][script]
    checked = 0
    for entry in imports:
        if entry[0] == 'from' and entry[1] not in STDLIB_OR_THIRD_PARTY:
            mod = importlib.import_module(entry[1])
            for name in entry[2]:
                assert hasattr(mod, name), (script, entry[1], name)
                checked += 1
        elif entry[0] == 'import' and entry[1] not in STDLIB_OR_THIRD_PARTY:
            importlib.import_module(entry[1])
            checked += 1
    assert checked >= 8
    assert 'dropin' in sys.modules['input_data'].__file__
