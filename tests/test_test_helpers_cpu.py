"""The helpers the GPU tests stand on, without a GPU: tests/child_process.py (a piece of a test in a fresh process) and the parts of
tests/icp_search_harness.py that need no device.  The children here import this module, which loads no backend library."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_search_harness as harness  # noqa: E402
from child_process import run_child  # noqa: E402

ME = "test_test_helpers_cpu"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _report(names):
    """(child side) the named variables as the child sees them, after a line on stderr"""
    print("a banner on stdout")
    print("child speaking", file=sys.stderr)
    return {n: os.environ.get(n) for n in names}, list(sys.path)


def _exit_three():
    print("about to give up", file=sys.stderr)
    sys.exit(3)


def test_value_stderr_and_environment(monkeypatch):
    monkeypatch.setenv("O3DS_HELPER_TEST_KEEP", "kept")
    monkeypatch.setenv("O3DS_HELPER_TEST_DROP", "dropped")
    monkeypatch.delenv("O3DS_HELPER_TEST_NEW", raising=False)
    before = dict(os.environ)
    names = ("O3DS_HELPER_TEST_KEEP", "O3DS_HELPER_TEST_DROP", "O3DS_HELPER_TEST_NEW")
    (seen, path), err = run_child(ME, f"t._report({names!r})", env={"O3DS_HELPER_TEST_NEW": "1"}, unset=("O3DS_HELPER_TEST_DROP",), timeout=120)
    assert seen == {"O3DS_HELPER_TEST_KEEP": "kept", "O3DS_HELPER_TEST_DROP": None, "O3DS_HELPER_TEST_NEW": "1"}
    assert "child speaking" in err and "a banner" not in err
    here = os.path.dirname(os.path.abspath(__file__))
    assert here in path and os.path.dirname(here) in path, "tests/ and the repository root are on the child's sys.path"
    assert dict(os.environ) == before, "env or unset leaked into this process"


def test_a_failing_child_fails_the_test_with_its_stderr():
    with pytest.raises(pytest.fail.Exception) as e:
        run_child(ME, "t._exit_three()", timeout=120)
    assert "return code 3" in str(e.value) and "about to give up" in str(e.value)


def test_a_child_beyond_its_limit_is_killed():
    t0 = time.monotonic()
    with pytest.raises(pytest.fail.Exception) as e:
        run_child(ME, "__import__('time').sleep(30)", timeout=1)
    assert time.monotonic() - t0 < 10.0, "the child was waited for, not killed"
    assert "time limit of 1 s expired" in str(e.value)


def test_the_limit_has_no_default():
    with pytest.raises(TypeError):
        run_child(ME, "1")


def test_parse_stats_finds_every_pass_of_every_recorded_line():
    loop = harness.load_parent_record(os.path.join(GOLDEN, "icp_scan_loop_parent.npz"))[1]
    lines = [ln for s in sorted(loop) for ln in loop[s]] + [str(x) for x in np.load(os.path.join(GOLDEN, "icp_lane_exchange_parent.npz"))["end_stats"]]
    assert sorted(loop) == ["f32", "f64"] and len(lines) > 50
    for ln in lines:
        passes = harness.parse_stats(ln)
        assert len(passes) == ln.count("[") > 0 and all(sorted(p) == ["f", "k", "s", "v"] for p in passes), ln
    assert harness.parse_stats("icp stats (n_src 80): [0 v0 s80 k0 f3] [1 v7 s73 k80 f0]") == [dict(v=0, s=80, k=0, f=3), dict(v=7, s=73, k=80, f=0)]
    with pytest.raises(AssertionError):
        harness.parse_stats("icp stats (n_src 80): [0 v0 s80 k0 f3] [1 v7 s73 k80]")


def test_pack_keeps_the_recorded_order():
    T = np.arange(16.0).reshape(4, 4)
    f, i = harness.pack(dict(transformation=T, fitness=0.25, inlier_rmse=0.5, iterations=3, n_corr=77, extra="ignored"))
    assert f.dtype == np.float64 and f.tolist() == list(range(16)) + [0.25, 0.5]
    assert i.dtype == np.int64 and i.tolist() == [3, 77]
    harness.assert_bits(f, np.array(list(range(16)) + [0.25, 0.5]), "packed floats")
    with pytest.raises(AssertionError):
        harness.assert_bits(np.array([0.0]), np.array([-0.0]), "zero and minus zero are equal numbers, other bits")
