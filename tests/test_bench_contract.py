"""CPU-side checks of bench.py's reporting contract (no GPU, no compute): the metric string
follows --grid, PMC traffic records are only quoted for the build they were measured on, and
the multi-GPU default transport set cannot hang."""
import glob
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_metric_string_and_level_choice():
    import bench
    assert "N=4096^2" in bench.metric_string(4096)
    assert "N=2048^2" in bench.metric_string(2048)          # was hard-coded
    assert bench.n_levels_for(4096) == 16 and bench.n_levels_for(1024) == 12
    assert "3D" in bench.metric_string(512, 3) and "N=512^3" in bench.metric_string(512, 3)
    assert bench.n_levels_for(512, dim=3) == 19             # BASELINE config 5: 134 M -> 511 dofs
    assert bench.HBM_PEAK_GBS == 8000.0
    assert len(bench.CPU_FLAGS) == 2 and "-O3 -march=native" in bench.CPU_FLAGS[1]


def test_pmc_records_are_keyed_to_the_source_hash(tmp_path, monkeypatch):
    import bench
    sha = bench.source_sha16()
    assert len(sha) == 16 and int(sha, 16) >= 0 and sha == bench.source_sha16()
    # a record of another build must not be quoted; one of this build must
    prof = tmp_path / "profiles"
    prof.mkdir()
    rec = {"source": "test", "n": 4096, "source_sha16": "0" * 16,
           "kernels": {"patch_down_kernel<5, true, true>@L0": {"traffic_bytes": 123.0}}}
    (prof / "zz_pmc_traffic.json").write_text(json.dumps(rec))
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    val, src = bench.pmc_traffic("patch_down_kernel", 4096)
    assert val is None and "no PMC record for this build" in src
    rec["source_sha16"] = sha
    (prof / "zz_pmc_traffic.json").write_text(json.dumps(rec))
    val, src = bench.pmc_traffic("patch_down_kernel", 4096)
    assert val == 123.0 and "zz_pmc_traffic" in src
    assert bench.pmc_traffic("patch_down_kernel", 2048)[0] is None      # other grid
    assert bench.pmc_traffic("sell_kernel", 4096)[0] is None            # other kernel


def test_committed_pmc_records_are_well_formed():
    import bench
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r0[2-9]*_pmc_traffic.json")))   # round 2 on
    assert files
    fresh = 0
    for f in files:
        rec = json.load(open(f))
        assert rec.get("n") == 4096 and rec.get("kernels")
        for k, v in rec["kernels"].items():
            assert "@L" in k and v["traffic_bytes"] > 0
        fresh += rec.get("source_sha16") == bench.source_sha16()
    if not fresh:   # bench.py then reports traffic = null: legal, but worth knowing
        warnings.warn("no committed PMC record matches the current device sources")


def test_multi_gpu_default_is_the_safe_transport_set():
    import bench
    argv = sys.argv
    try:
        sys.argv = ["bench.py"]
        import argparse
        ap_main = bench.main.__code__.co_consts      # the parser is built inside main()
        assert any(isinstance(c, str) and c == "safe" for c in ap_main)
    finally:
        sys.argv = argv
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert 'choices=["safe", "auto", "p2p", "slab", "window", "library", "ipc", "graph"], default="safe"' in src


def test_dump_outputs_writes_the_whole_solution_or_a_fixed_sample(tmp_path):
    import numpy as np
    import bench

    class FakeSolver:
        def __init__(self, n):
            self.u = np.arange(n, dtype=np.float64) * 0.5

        def get_soln(self, level=0):
            assert level == 0
            return self.u.copy()

    small = FakeSolver(1000)
    bench.dump_outputs(small, str(tmp_path / "small"))
    u = np.load(tmp_path / "small" / "u.npy")
    assert u.dtype == np.float64 and np.array_equal(u, small.u)

    big = FakeSolver(bench.DUMP_MAX_VALUES * 2 + 3)
    for d in ("a", "b"):
        bench.dump_outputs(big, str(tmp_path / d))
    a, b = np.load(tmp_path / "a" / "u.npy"), np.load(tmp_path / "b" / "u.npy")
    assert a.dtype == np.float64 and a.size == bench.DUMP_MAX_VALUES and a.nbytes <= 64 * 2 ** 20
    assert np.array_equal(a, b)                                  # the same sample every run
    idx = (a * 2).astype(np.int64)
    assert np.all(np.diff(idx) > 0) and idx[-1] < big.u.size   # distinct entries, in order
