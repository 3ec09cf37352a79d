"""bench.py end to end on the GPU at a small grid: a plain run reports the headline only, --full
adds the checks and figures of its own runs, and both time exactly --steps cycles and dump the
same solution."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--grid", "256",
           "--steps", "7", "--warmup", "2", "--dump-outputs", str(out_dir), *extra]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_plain_and_full_runs(tmp_path):
    plain = _bench(tmp_path / "plain")
    full = _bench(tmp_path / "full", "--full", "--cpu-cycles", "1")
    for d in (plain, full):
        assert d["metric"].startswith("V-cycles/sec, 2D Poisson N=256^2")
        assert d["unit"] == "V-cycles/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
        assert d["steps"] == 7 and d["warmup"] == 2 and d["n_gpus"] == 1
        assert d["ms_per_step"] > 0 and abs(d["value"] * d["ms_per_step"] - 1e3) < 1e-6
    assert "roofline" not in plain and "cpu_baseline" not in plain
    assert "whole_cycle" not in plain["config"] and "rss_after_steps" not in plain["config"]
    assert full["roofline"]["achieved"] > 0 and full["cpu_baseline"]["value"] > 0
    assert full["config"]["rss_after_steps"] < full["config"]["rss_after_warmup"]
    assert "whole_cycle" in full["config"]
    u_plain = np.load(tmp_path / "plain" / "u.npy")
    u_full = np.load(tmp_path / "full" / "u.npy")
    assert u_plain.dtype == np.float64 and u_plain.shape == (256 * 256,)
    assert np.all(np.isfinite(u_plain)) and np.any(u_plain != 0)
    assert np.array_equal(u_plain, u_full)   # the rss check of --full leaves the cycles alone
