"""A piece of a test in a fresh process.  The A/B switches of the backend library are read once per process, so a test that needs a
result under another setting runs that piece in a child and compares.  Every such child is started here, one way:
  * a fresh interpreter (never an exec of this process), under a time limit the caller must state;
  * the repository root and tests/ on sys.path, torch imported before anything loads the backend library (the load order of
    tests/conftest.py), the calling test module imported as `t`;
  * the value of one expression over `t` comes back pickled through a temporary file: stdout and stderr stay free for the library's
    banners and counters, and stderr is handed to the caller;
  * a child that fails or outlives its limit fails the calling test at once, with the end of its stderr in the message.  Nothing is
    tried again and nothing else is started: a caller runs its child before its own GPU work."""
import os
import pickle
import subprocess
import sys
import tempfile

import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)

_CHILD = """import importlib, pickle, sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
try:
    import torch
except Exception:
    torch = None
t = importlib.import_module(sys.argv[3])
value = eval(sys.argv[4])
with open(sys.argv[5], "wb") as f:
    pickle.dump(value, f)
"""


def _text(x):
    return x.decode(errors="replace") if isinstance(x, bytes) else (x or "")


def run_child(module, expr, *, env=None, unset=(), timeout, cwd=None):
    """(value of `expr`, the child's stderr).  module: the name of the test module the child imports as `t`; expr: an expression over
    `t` (and `torch`); env: variables added to a copy of this process's environment, unset: variables taken out of it; timeout: seconds"""
    child_env = dict(os.environ, **(env or {}))
    for v in unset:
        child_env.pop(v, None)
    with tempfile.TemporaryDirectory() as tmp:
        result = os.path.join(tmp, "value.pickle")
        cmd = [sys.executable, "-c", _CHILD, TESTS, ROOT, module, expr, result]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=child_env, cwd=cwd)  # (kills and reaps at the limit)
        except subprocess.TimeoutExpired as e:
            pytest.fail(f"child process `{module}: {expr}`: the time limit of {timeout} s expired, the child was killed; "
                        f"its stderr ended:\n{_text(e.stderr)[-2000:]}", pytrace=False)
        if p.returncode != 0:
            pytest.fail(f"child process `{module}: {expr}` ended with return code {p.returncode}; its stderr ended:\n{p.stderr[-2000:]}", pytrace=False)
        with open(result, "rb") as f:
            return pickle.load(f), p.stderr
