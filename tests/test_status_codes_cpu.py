"""CPU tests of how the package treats the C ABI's status codes (no GPU): an entry point that declines a shape returns E_NOKERNEL and
leaves its outputs unwritten, so no call site may drop that status on the floor."""
import ast
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _discarded_checks():
    """(file, line) of every `_lib.check(...)` / `check(...)` whose result is thrown away (a bare expression statement)."""
    sites = []
    for base, _, files in os.walk(os.path.join(ROOT, 'afcm_amd')):
        for name in sorted(files):
            if not name.endswith('.py'):
                continue
            path = os.path.join(base, name)
            with open(path) as f:
                tree = ast.parse(f.read(), path)
            for node in ast.walk(tree):
                if isinstance(node, ast.Expr) and isinstance(node.value, ast.Call):
                    fn = node.value.func
                    called = fn.attr if isinstance(fn, ast.Attribute) else getattr(fn, 'id', None)
                    if called == 'check':
                        sites.append(f'{os.path.relpath(path, ROOT)}:{node.lineno}')
    return sites


def test_no_call_site_discards_a_status():
    """`_lib.check` passes E_NOKERNEL through; a caller that ignores its result would use an uninitialised output.  Sites with no
    fallback call `_lib.launched`, the others branch on the returned code."""
    sites = _discarded_checks()
    assert not sites, 'status of a C-ABI call thrown away (use _lib.launched, or branch on the code):\n  ' + '\n  '.join(sites)


def test_launched_raises_on_a_declined_launch():
    from afcm_amd import _lib
    assert _lib.launched(0, 'op') == 0
    assert _lib.check(_lib.E_NOKERNEL, 'op') == _lib.E_NOKERNEL
    with pytest.raises(RuntimeError, match='op: no kernel'):
        _lib.launched(_lib.E_NOKERNEL, 'op')
    with pytest.raises(RuntimeError, match='HIP error'):
        _lib.launched(1000 + 7, 'op')
