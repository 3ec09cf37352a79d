"""tests/pcg_twin.py on the CPU: with the oracle's V-cycle as M^-1 it is the oracle's textbook PCG up to the
order of the dot products (the device's tree against a sequential sum), so it takes the same number of
iterations and ends within rounding of the same x; and its trajectory does not depend on max_iters."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pcg_twin as PT  # noqa: E402


@pytest.mark.parametrize("smoother", ["spgs", "jacobi"])
def test_twin_is_the_oracles_pcg_up_to_the_order_of_the_dots(oracle, smoother):
    n, L = 48, 3
    A, b = oracle.laplacian(n), oracle.rhs(n)
    kw = dict(smoother=oracle.SM_TRUE_JACOBI, smoother_iters=2, omega=0.6) if smoother == "jacobi" else {}
    ref = oracle.Multigrid(A, b, L, **kw)
    x, it, rel, trace = PT.pcg(A, b, np.zeros(n * n), ref.apply, 1e-10, 200)
    xr, itr, relr = oracle.Multigrid(A, b, L, **kw).pcg(1e-10, 200)
    assert it == itr and len(trace) == it and rel <= 1e-10
    assert abs(rel - relr) <= 1e-6 * relr
    assert np.linalg.norm(x - xr) <= 1e-12 * np.linalg.norm(xr)
    assert trace[-1][1] is None and all(t[1] is not None for t in trace[:-1])
    assert np.linalg.norm(oracle.residual(A, x, b)) <= 1.01e-10 * np.linalg.norm(b)


def test_trajectory_does_not_depend_on_the_iteration_limit(oracle):
    n, L = 48, 3
    A, b = oracle.laplacian(n), oracle.rhs(n)
    ref = oracle.Multigrid(A, b, L)
    x0 = np.random.default_rng(1).standard_normal(n * n)
    _, it, _, full = PT.pcg(A, b, x0, ref.apply, 0.0, 5, keep_iterates=True)
    assert it == 5
    for k in (0, 1, 3):
        x, itk, rel, trace = PT.pcg(A, b, x0, ref.apply, 0.0, k)
        assert itk == k
        if k == 0:
            assert np.array_equal(x, x0) and trace == []
        else:
            assert np.array_equal(x, full[k - 1][3]) and rel == full[k - 1][2]
            assert [t[0] for t in trace] == [t[0] for t in full[:k]]


def test_edge_cases(oracle):
    n, L = 24, 3
    A, b = oracle.laplacian(n), oracle.rhs(n)
    ref = oracle.Multigrid(A, b, L)
    zero = np.zeros(n * n)
    x, it, rel, _ = PT.pcg(A, zero, zero, ref.apply, 1e-10, 50)
    assert it == 0 and rel == 0.0 and not x.any()
    bad = b.copy()
    bad[7] = np.nan
    x, it, rel, _ = PT.pcg(A, bad, zero, ref.apply, 1e-10, 50)      # NaN leaves the loop after one iteration
    assert it == 1 and np.isnan(rel)
