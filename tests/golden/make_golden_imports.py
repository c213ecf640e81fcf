#!/usr/bin/env python
"""Golden fixture k9_script_imports.json: the import statements of the reference's train.py and make_submission.py.

Run in the build container only (needs /root/reference):
    python tests/golden/make_golden_imports.py

Stores, per script and in ast.walk order, only what its import statements name: ["from", module, [names]] for
`from module import names` and ["import", name] for `import name`.  No other source text is stored.
tests/test_dropin_cpu.py resolves every entry through dropin/."""
import ast
import json
import os

REF = '/root/reference'
OUT = os.path.dirname(os.path.abspath(__file__))
SCRIPTS = ("train.py", "make_submission.py")


def script_imports(path):
    out = []
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.ImportFrom):
            out.append(["from", node.module, [a.name for a in node.names]])
        elif isinstance(node, ast.Import):
            out.extend(["import", a.name] for a in node.names)
    return out


def main():
    if not os.path.isdir(REF):
        raise SystemExit('reference checkout not found at %s' % REF)
    scripts = {s: script_imports(os.path.join(REF, s)) for s in SCRIPTS}
    with open(os.path.join(OUT, 'k9_script_imports.json'), 'w') as f:       # one import statement per line
        f.write('{"note": "import statements of the reference scripts (see make_golden_imports.py)",\n "scripts": {\n')
        f.write(',\n'.join('  %s: [\n%s\n  ]' % (json.dumps(s), ',\n'.join('   ' + json.dumps(e) for e in scripts[s]))
                           for s in SCRIPTS))
        f.write('\n }\n}\n')


if __name__ == '__main__':
    main()
