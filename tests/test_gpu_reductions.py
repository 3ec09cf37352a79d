"""The device's reductions (kernels.hip: K-SumSq sum_kernel, K-PCG dot_kernel, block_sum_kernel<KP>) and
what the solver decides on them, bit for bit against tests/reduce_twin.py.  Every comparison is `==` on
the float64 bits; every result is also within reduce_twin.bound(n) of math.fsum of the same terms, which
says that it is a sum at all, independently of the twin.  tests/test_reduce_twin.py shows on the CPU that
the data used here tells the device's order from a dropped last element, a dropped ragged workgroup, a
grid-stride loop that stops after one pass, and the sequential order.

  amg_hip_dev_sumsq   n = 0 .. 524291 (both sides of the 1024-workgroup cap at 262144, ragged tails), four
                      seeds of uniform [1, 2) data, NaN-filled scratch and output, both streams
  amg_hip_rss         Poisson 40^2 and 513^2, a 1-D three-point matrix of 262145 rows, knn(1600, 4, 1);
                      level 0 in CSR, SELL and the dictionary layout (knn does not fit the dictionary: that
                      request runs in SELL, and the test prints the layout it got); u after two cycles and
                      a random u
  amg_hip_solve       96^2, a check every 2 of 6 cycles: last_rss is the twin's, `converged` follows
  amg_hip_block_rss   k = 1, 2, 3, 4, 7, 8, 9, 16 at 40^2 and 513^2: every block_sum_kernel<KP>
  dot_kernel          amg_hip_pcg with max_iters = 0: relres = sqrt(r.r) / sqrt(b.b), and sqrt(r.r) for b = 0

The order of amg_hip_rss's terms: the row kernel (CSR_RSSQ) forms d = b_i - bhat_i with bhat = A u summed
from zero in ascending column order, then d * d (common.hpp:22-26 of the reference; DESIGN.md, K-SumSq).
That is b - oracle.spmv(A, u).  It is NOT oracle.residual(A, u, b), which starts from b_i and subtracts
entry by entry (the cycle's residual, CSR_RESID) and rounds differently in some rows; each rss test
prints in how many.  The PCG residual is CSR_RESID and is compared with oracle.residual."""
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sp = pytest.importorskip("scipy.sparse")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import irregular_mats as im  # noqa: E402
import reduce_twin as RT  # noqa: E402
from test_reduce_twin import SEEDS, SIZES, data  # noqa: E402

pytestmark = pytest.mark.gpu

JAC = dict(smoother=3, smoother_iters=2, omega=0.6)
LAYOUTS = [im.LAYOUT_CSR, im.LAYOUT_SELL, im.LAYOUT_DICT]


def csc(A):
    return A.colptr, A.rowind, A.val


def dev(a):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


def bits(v):
    return np.float64(v).view(np.uint64)


def is_a_sum(got, terms, what):
    """within the tree's bound of the correctly rounded sum of the (non-negative) terms"""
    exact = math.fsum(np.asarray(terms).tolist())
    assert abs(got - exact) <= RT.bound(len(terms)) * exact, (what, got, exact)


# ---- amg_hip_dev_sumsq ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_dev_sumsq_has_the_twins_bits(amg, n):
    lib = amg.lib()
    side = torch.cuda.Stream()
    for seed in SEEDS:
        x = data(n, seed)[0]
        want = RT.sumsq(x)
        xd = dev(x) if n else torch.zeros(1, dtype=torch.float64, device="cuda")
        for stream in (None, side):
            scratch = torch.full((1024,), float("nan"), dtype=torch.float64, device="cuda")
            out = torch.full((8,), float("nan"), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            handle = None if stream is None else stream.cuda_stream
            assert lib.amg_hip_dev_sumsq(n, xd.data_ptr(), out[3:].data_ptr(), scratch.data_ptr(), handle) == 0
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert bits(got[3]) == bits(want), (n, seed, stream is not None, got[3], want)
            assert np.isnan(np.delete(got, 3)).all()              # one double written
            g = RT.grid(n)[0]
            part = scratch.cpu().numpy()
            assert not np.isnan(part[:g]).any() and np.isnan(part[g:]).all()   # g partials, no slot more
            is_a_sum(float(got[3]), x * x, (n, seed))


# ---- amg_hip_rss ------------------------------------------------------------------------------------
_OPS = {}


def operator(oracle, name):
    """(oracle CSC, b, levels, constructor options), made once"""
    if name not in _OPS:
        if name in ("lap40", "lap513"):
            n = int(name[3:])
            _OPS[name] = (oracle.laplacian(n), oracle.rhs(n), 3, {})
        elif name == "line262145":   # 1-D three-point matrix: one row in the second grid-stride pass
            n = 262145
            M = sp.diags([-np.ones(n - 1), 2.0 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1], format="csc")
            M.sort_indices()
            b = 1.0 + np.random.default_rng(3).random(n)
            _OPS[name] = (oracle.CSC(n, n, M.indptr, M.indices, M.data), b, 2, {})
        else:
            assert name == "knn"
            S = im.knn(1600, 4, 1).tocsc()
            S.sort_indices()
            b = np.random.default_rng(7).standard_normal(1600)
            _OPS[name] = (oracle.CSC(1600, 1600, S.indptr, S.indices, S.data), b, None, {})
    return _OPS[name]


def rss_difference(oracle, A, u, b):
    """the vector amg_hip_rss squares: b - A u with A u summed from zero (see the module's docstring)"""
    return np.subtract(b, oracle.spmv(A, u))


def build(amg, oracle, name, **kw):
    A, b, levels, _ = operator(oracle, name)
    if levels is None:
        return amg.Multigrid.ruge_stueben(*csc(A), b, 12, 0.25, 40, **JAC, **kw)
    return amg.Multigrid(*csc(A), b, levels, **JAC, **kw)


@pytest.mark.parametrize("layout", LAYOUTS, ids=[im.LAYOUT_NAME[l] for l in LAYOUTS])
@pytest.mark.parametrize("name", ["lap40", "lap513", "line262145", "knn"])
def test_rss_has_the_twins_bits(amg, oracle, name, layout):
    A, b, _, _ = operator(oracle, name)
    mg = build(amg, oracle, name, layout=layout)
    try:
        got_layout = mg.level_layout(0)[0]
        if name.startswith("lap"):
            assert got_layout == layout          # the 5-point stencil fits every layout
        mg.vcycle(2)
        starts = [("two cycles", mg.get_soln(0)),
                  ("random", np.random.default_rng(11).standard_normal(A.rows))]
        for what, u in starts:
            mg.set_vec(0, "u", u)
            got = mg.rss()
            d = rss_difference(oracle, A, u, b)
            want = RT.rss(d)
            other = oracle.residual(A, u, b)
            print(f"\n{name} {im.LAYOUT_NAME[got_layout]} {what}: rss {got!r}, twin {want!r}; b - A u differs from the "
                  f"cycle's residual in {int(np.count_nonzero(d != other))} of {A.rows} rows; sequential {oracle.rss(A, u, b)!r}")
            assert bits(got) == bits(want), (name, layout, what, got, want)
            is_a_sum(got, d * d, (name, layout, what))
            assert np.array_equal(mg.get_soln(0), u) and np.array_equal(mg.get_rhs(0), b)
    finally:
        mg.close()


# ---- amg_hip_solve ----------------------------------------------------------------------------------
def test_solve_decides_on_the_twins_rss(amg, oracle, capsys):
    n, L = 96, 4
    # the right-hand side scaled by a power of two, so that every check value lies below the 100 that
    # solve() starts its loop from (multigrid.hpp:313)
    A, b = oracle.laplacian(n), oracle.rhs(n) * 2.0 ** -4
    kw = dict(JAC, exact_coarse_solve=True, compute_error_every_n_iters=2, n_iters=6)
    mg = amg.Multigrid(*csc(A), b, L, **kw)
    checks, us = [], []
    for _ in range(3):                      # what solve() runs between two checks
        mg.vcycle(2)
        us.append(mg.get_soln(0))
        checks.append(RT.rss(rss_difference(oracle, A, us[-1], b)))
    mg.close()
    assert 100.0 > checks[0] > checks[1] > checks[2] > 0.0, checks
    # (tolerance, checks taken, converged): between the first and the second check value, between the
    # second and the third, and one that is never met
    for tol, taken, conv in ((math.sqrt(checks[0] * checks[1]), 2, True), (math.sqrt(checks[1] * checks[2]), 3, True),
                             (0.5 * checks[2], 3, False)):
        assert tol < checks[taken - 2] and (checks[taken - 1] <= tol) == conv
        mg =amg.Multigrid(*csc(A), b, L, tolerance=tol, **kw)
        try:
            u, iters, converged, last = mg.solve()
            assert iters == 2 * taken and converged is conv
            assert np.array_equal(u, us[taken - 1])
            assert bits(last) == bits(RT.rss(rss_difference(oracle, A, u, b))) == bits(checks[taken - 1])
            assert converged == (last <= tol)
        finally:
            mg.close()
    capsys.readouterr()


# ---- amg_hip_block_rss ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lap40", "lap513"])
def test_block_rss_has_the_twins_bits_in_every_column(amg, oracle, name):
    A, b, _, _ = operator(oracle, name)
    mg = build(amg, oracle, name)
    try:
        for k in (1, 2, 3, 4, 7, 8, 9, 16):
            rng = np.random.default_rng([k, A.rows])
            U, F = rng.standard_normal((A.rows, k)), rng.standard_normal((A.rows, k))
            got = mg.block_rss(dev(U), dev(F))
            torch.cuda.synchronize()
            assert got.shape == (k,)
            for j in range(k):
                d = rss_difference(oracle, A, np.ascontiguousarray(U[:, j]), np.ascontiguousarray(F[:, j]))
                assert bits(got[j]) == bits(RT.rss(d)), (name, k, j, got[j], RT.rss(d))
                is_a_sum(float(got[j]), d * d, (name, k, j))
    finally:
        mg.close()


# ---- the dot product alone --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lap40", "lap513", "line262145"])
def test_pcg_without_iterations_is_two_dot_products(amg, oracle, name):
    A, b, _, _ = operator(oracle, name)
    mg = build(amg, oracle, name)
    try:
        u = np.random.default_rng(5).standard_normal(A.rows)
        for rhs in (b, np.zeros(A.rows)):
            mg.set_vec(0, "f", rhs)
            mg.set_vec(0, "u", u)
            x, iters, rel = mg.pcg(1e-10, 0)
            r = oracle.residual(A, u, rhs)
            rr, bb = RT.dot(r, r), RT.dot(rhs, rhs)
            want = math.sqrt(rr) / math.sqrt(bb) if rhs.any() else math.sqrt(rr)
            assert bb > 0.0 or not rhs.any()
            assert iters == 0 and bits(rel) == bits(want), (name, rel, want)
            # a quotient of two roots of sums: half the tree's bound from each, and three roundings
            exact = math.sqrt(math.fsum((r * r).tolist()))
            exact = exact / math.sqrt(math.fsum((rhs * rhs).tolist())) if rhs.any() else exact
            assert abs(rel - exact) <= (RT.bound(A.rows) + 4 * RT.U) * exact, (name, rel, exact)
            assert np.array_equal(x, u) and np.array_equal(mg.get_soln(0), u)
            assert np.array_equal(mg.get_rhs(0), rhs)
    finally:
        mg.close()
