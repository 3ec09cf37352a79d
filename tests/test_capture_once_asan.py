"""CycleGraph (algebraic-multigrid_amd/csrc/capture_once.hpp), the owner of every captured cycle graph,
under AddressSanitizer + UndefinedBehaviorSanitizer against stand-ins for the HIP calls: capture once and
replay, the four failure paths, reset and scope exit.  A stand-alone host program, no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cycle_graph_under_asan_and_ubsan():
    d = os.path.join(ROOT, "tests", "sanitize")
    subprocess.check_call(["make", "-C", d, "capture_once_asan"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([os.path.join(d, "capture_once_asan")], capture_output=True, text=True, timeout=60, env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "capture_once_asan ok" in p.stdout and "runtime error" not in p.stderr
