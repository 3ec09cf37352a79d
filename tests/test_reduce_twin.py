"""tests/reduce_twin.py on the CPU: the vectorised twin is the tree it says it is, it is a sum, and the
data of the GPU comparison (tests/test_gpu_reductions.py) can see a kernel that sums something else.

  emulation   a pure-Python restatement (one loop per thread, one per lane, Python floats) gives the same
              bits at every size up to 1023 and at 262401
  accuracy    relative distance from math.fsum of the same terms <= reduce_twin.bound(n)
  conditions  on uniform [1, 2) data the twin's value changes when the last element is dropped, when the
              ragged last workgroup is dropped, when everything past the first stride is dropped; and the
              sequential sum differs from the tree on at least one of the four seeds of every size >= 63
These are conditions on the data, not measurements: a kernel that made one of these mistakes would give
another float64 than the twin on the very vectors the GPU tests use."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import reduce_twin as RT  # noqa: E402

SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 262143, 262144, 262145, 262401, 524291]
SEEDS = [0, 1, 2, 3]
STRIDE = 262144       # 1024 workgroups x 256 threads: the first size with a second grid-stride pass is 262145
KINDS = ["sum", "sumsq", "dot"]

_DATA = {}


def data(n, seed):
    """(x, y): two read-only vectors of n entries drawn uniformly from [1, 2), made once"""
    if (n, seed) not in _DATA:
        rng = np.random.default_rng([seed, n])
        x, y = 1.0 + rng.random(n), 1.0 + rng.random(n)
        x.setflags(write=False)
        y.setflags(write=False)
        _DATA[(n, seed)] = (x, y)
    return _DATA[(n, seed)]


def twin(kind, x, y):
    return {"sum": lambda: RT.sum(x), "sumsq": lambda: RT.sumsq(x), "dot": lambda: RT.dot(x, y)}[kind]()


def terms(kind, x, y):
    return {"sum": x, "sumsq": x * x, "dot": x * y}[kind]


def bits(v):
    return np.float64(v).view(np.uint64)


# ---- the independent emulation: Python floats, no numpy arithmetic, no code of the twin ---------------
def emulate_launch(t, groups):
    """one launch of `groups` workgroups of 256 threads over the list of terms t: the list of partials"""
    n = len(t)
    threads = 256 * groups
    out = []
    for wg in range(groups):
        waves = []
        for w in range(4):
            lane = []
            for l in range(64):
                i = wg * 256 + w * 64 + l
                s = 0.0
                while i < n:
                    s = s + t[i]
                    i += threads
                lane.append(s)
            off = 32
            while off > 0:
                old = list(lane)
                for l in range(64):
                    lane[l] = old[l] + (old[l + off] if l + off < 64 else old[l])
                off //= 2
            waves.append(lane[0])
        out.append(((waves[0] + waves[1]) + waves[2]) + waves[3])
    return out


def emulate(t):
    n = len(t)
    groups = (n + 255) // 256
    groups = 1024 if groups > 1024 else groups
    groups = 1 if groups < 1 else groups
    return emulate_launch(emulate_launch(t, groups), 1)[0]


def py_terms(kind, x, y):
    xs, ys = x.tolist(), y.tolist()
    if kind == "sum":
        return xs
    if kind == "sumsq":
        return [a * a for a in xs]
    return [a * b for a, b in zip(xs, ys)]


@pytest.mark.parametrize("n", [n for n in SIZES if n <= 1023])
def test_twin_equals_the_scalar_emulation(n):
    for seed in SEEDS:
        x, y = data(n, seed)
        for kind in KINDS:
            assert bits(twin(kind, x, y)) == bits(emulate(py_terms(kind, x, y))), (n, seed, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_twin_equals_the_scalar_emulation_past_one_stride(kind):
    """262401 = 262144 + 257: 1024 workgroups, 257 threads with a second element"""
    for seed in SEEDS:
        x, y = data(262401, seed)
        assert bits(twin(kind, x, y)) == bits(emulate(py_terms(kind, x, y))), seed


@pytest.mark.parametrize("n", [1, 63, 257, 1023])
def test_block_twin_is_the_twin_per_column_and_the_emulation(n):
    """every panel width of block_sum_kernel<KP>, zero columns (the padding) included"""
    for kp in (1, 2, 4, 8, 16):
        rng = np.random.default_rng([kp, n])
        X, Y = 1.0 + rng.random((n, kp)), 1.0 + rng.random((n, kp))
        if kp > 2:
            X[:, kp - 1] = 0.0
        s, d = RT.block(X), RT.block(X, Y)
        assert s.shape == d.shape == (kp,) and s.dtype == d.dtype == np.float64
        for j in range(kp):
            xj, yj = np.ascontiguousarray(X[:, j]), np.ascontiguousarray(Y[:, j])
            assert bits(s[j]) == bits(RT.sum(xj)) == bits(emulate(xj.tolist())), (n, kp, j)
            assert bits(d[j]) == bits(RT.dot(xj, yj)) == bits(emulate(py_terms("dot", xj, yj))), (n, kp, j)
        if kp > 2:
            assert bits(s[kp - 1]) == bits(0.0) and bits(d[kp - 1]) == bits(0.0)


def test_grid_and_depth():
    assert [RT.grid(n) for n in (0, 1, 256, 257, 262144, 262145, 524291)] == \
        [(1, 256), (1, 256), (1, 256), (2, 512), (1024, STRIDE), (1024, STRIDE), (1024, STRIDE)]
    assert RT.depth(1) == 1 + 9 + 1 + 9 and RT.depth(262144) == 1 + 9 + 4 + 9 and RT.depth(524291) == 3 + 9 + 4 + 9
    assert RT.rss(np.array([3.0, 4.0])) == 25.0 and RT.sum(np.zeros(0)) == 0.0 and bits(RT.sumsq(np.zeros(0))) == bits(0.0)


@pytest.mark.parametrize("n", SIZES)
def test_twin_is_a_sum_within_the_bound(n):
    worst = 0.0
    for seed in SEEDS:
        x, y = data(n, seed)
        for kind in KINDS:
            exact = math.fsum(terms(kind, x, y).tolist())
            got = twin(kind, x, y)
            if n == 0:
                assert got == 0.0 == exact
                continue
            rel = abs(got - exact) / exact
            worst = max(worst, rel)
            assert rel <= RT.bound(n), (n, seed, kind, rel, RT.bound(n))
    print(f"\nn = {n}: largest relative distance from fsum {worst:.3e}, bound {RT.bound(n):.3e}")


@pytest.mark.parametrize("n", [n for n in SIZES if n >= 2])
def test_data_sees_a_dropped_last_element(n):
    for seed in SEEDS:
        x, y = data(n, seed)
        for kind in KINDS:
            assert bits(twin(kind, x, y)) != bits(twin(kind, x[:-1], y[:-1])), (n, seed, kind)


@pytest.mark.parametrize("n", [n for n in SIZES if n > 256 and n % 256])
def test_data_sees_a_dropped_ragged_workgroup(n):
    keep = n - n % 256
    for seed in SEEDS:
        x, y = data(n, seed)
        for kind in KINDS:
            assert bits(twin(kind, x, y)) != bits(twin(kind, x[:keep], y[:keep])), (n, seed, kind)


@pytest.mark.parametrize("n", [n for n in SIZES if n > STRIDE])
def test_data_sees_a_loop_that_stops_after_one_stride(n):
    for seed in SEEDS:
        x, y = data(n, seed)
        for kind in KINDS:
            assert bits(twin(kind, x, y)) != bits(twin(kind, x[:STRIDE], y[:STRIDE])), (n, seed, kind)


@pytest.mark.parametrize("n", [n for n in SIZES if n >= 63])
def test_data_sees_the_sequential_order(n):
    """np.add.accumulate adds one element after the other.  A sum good to an ulp often rounds alike in two
    orders, so the condition is on the four seeds of a size together, per kind of reduction."""
    for kind in KINDS:
        differ = 0
        for seed in SEEDS:
            x, y = data(n, seed)
            seq = np.add.accumulate(terms(kind, x, y))[-1]
            differ += int(bits(seq) != bits(twin(kind, x, y)))
        assert differ >= 1, (n, kind)
