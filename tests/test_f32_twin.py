"""tests/f32_twin.py without a GPU: the float32 restatement of the single-precision cycle is as accurate
as the project's scipy float32 twin, its padded row walk is the plain per-row loop bit for bit (empty
rows, rows without a diagonal, every width from 0 to 25), a reversed row order shows in the bits, and
everything it returns is float32."""
import os
import sys

import numpy as np
import pytest

sp = pytest.importorskip("scipy.sparse")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import f32_twin as FT  # noqa: E402
import irregular_mats as im  # noqa: E402
import mixed_twin as MT  # noqa: E402

_H = {}


def hierarchy(grid, smoother):
    """f32_twin.Hierarchy on tensor_twin.Twin's matrices and transfers, scipy's LU as the coarse solve;
    smoother "jacobi" (2+2, omega 0.8) or "cheb" (degree 2 on ChebTwin's intervals)."""
    key = (grid, smoother)
    if key not in _H:
        tw = MT.operator(grid)[4]
        if smoother == "jacobi":
            sm = ("jacobi", 0.8, 2)
        else:
            ct = MT.cheb_twin(grid)
            bounds = []
            for M, (alpha, beta) in zip(ct.A[:-1], ct.coefs):
                G = float(np.max(np.asarray(abs(M).sum(axis=1)).ravel() / np.abs(M.diagonal())))
                bounds.append((0.3 * G, 1.0 * G))
                assert FT.cheb_twin.cheb_coefs(*bounds[-1], 2) == (alpha, beta)  # ChebTwin's own intervals
            sm = ("cheb", 2, 1, bounds)
        _H[key] = FT.Hierarchy(tw.A, tw.P, tw.R, sm, tw.coarse.solve)
    return _H[key]


@pytest.mark.parametrize("smoother", ["jacobi", "cheb"])
@pytest.mark.parametrize("grid", sorted(MT.GRIDS))
def test_the_cycle_is_as_accurate_as_the_scipy_float32_twin(grid, smoother):
    """within max(8 e32, 1e-6 ||z||) of the longdouble cycle, e32 = the scipy float32 cycle's distance
    (the bound of test_gpu_mixed.py)"""
    v = MT.operator(grid)[3]
    tw = MT.operator(grid)[4] if smoother == "jacobi" else MT.cheb_twin(grid)
    H = hierarchy(grid, smoother)
    u, f, r = FT.cycle(H, v)
    zero = np.zeros(v.size)
    ref = tw.vcycle(zero, v, np.longdouble)[0][0]
    z32 = tw.vcycle(zero.astype(np.float32), v.astype(np.float32), np.float32)[0][0]
    e32 = float(np.linalg.norm(np.asarray(z32, np.longdouble) - ref))
    dist = float(np.linalg.norm(np.asarray(u[0], np.longdouble) - ref))
    bound = max(8.0 * e32, 1e-6 * float(np.linalg.norm(u[0])))
    print(f"\nf32 twin {grid} {smoother}: distance {dist:.3e}, e32 {e32:.3e}, ratio {dist / e32:.2f}, "
          f"bound {bound:.3e}")
    assert np.all(np.isfinite(u[0])) and np.linalg.norm(u[0]) > 0
    assert dist <= bound
    # what cycle() returns: float32 on every level, the zero guess replaced, r from the down-leg
    assert len(u) == len(f) == len(r) == H.nl and r[-1] is None
    for l in range(H.nl):
        for a in (u[l], f[l]) + ((r[l],) if l < H.nl - 1 else ()):
            assert a.dtype == np.float32 and a.shape == (H.n[l],)
    assert FT.same_bits(f[0], v.astype(np.float32))


def test_the_padded_walk_is_the_per_row_loop_bit_for_bit():
    """irregular_mats.staircase(): row widths 0 .. 25, empty rows, rows without a diagonal"""
    M = im.staircase()
    cnt = np.diff(M.indptr)
    assert cnt.min() == 0 and cnt.max() == 25 and np.any(M.diagonal()[cnt > 0] == 0.0)
    n = M.shape[0]
    rng = np.random.default_rng(3)
    x, f, d = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    R = FT.Rows(M)
    alpha, beta = 0.37, 1.21
    got = {
        "resid": FT.residual(R, x, f),
        "spmv": FT.spmv(R, x),
        "spmv_add": FT.spmv_add(R, x, f),
        "jacobi": FT.jacobi(R, x, f, 0.8),
    }
    want = {
        "resid": FT.loop(M, "resid", x, f),
        "spmv": FT.loop(M, "spmv", x),
        "spmv_add": FT.loop(M, "spmv_add", x, f),
        "jacobi": FT.loop(M, "jacobi", x, f, omega=0.8),
    }
    for first in (True, False):
        got[f"cheb first={first}"] = FT.cheb_step(R, x, f, None if first else d, alpha, beta, first)
        want[f"cheb first={first}"] = FT.loop(M, "cheb", x, f, d=d, alpha=alpha, beta=beta, first=first)
    for name in want:
        g, w = got[name], want[name]
        for a, b in zip(g if isinstance(g, tuple) else (g,), w if isinstance(w, tuple) else (w,)):
            assert a.dtype == np.float32
            assert FT.same_bits(a, b), name
    # rows without a diagonal keep x in the two sweeps; empty rows give f, 0, f
    nodiag = M.diagonal() == 0.0
    assert FT.same_bits(got["jacobi"][nodiag], x[nodiag])
    assert FT.same_bits(got["cheb first=True"][0][nodiag], x[nodiag])
    empty = cnt == 0
    assert FT.same_bits(got["resid"][empty], f[empty]) and not np.any(got["spmv"][empty])
    print(f"\nstaircase: {n} rows, widths {cnt.min()} .. {cnt.max()}, {int(empty.sum())} empty, "
          f"{int((nodiag & ~empty).sum())} without a diagonal: 6 row modes bit for bit")


def test_a_reversed_row_order_shows_in_the_bits():
    """33x20: the residual summed in descending column order differs in at least one bit"""
    A = MT.operator("33x20")[2]
    rng = np.random.default_rng(5)
    x, f = (rng.standard_normal(A.shape[0]).astype(np.float32) for _ in range(2))
    up = FT.residual(FT.Rows(A), x, f)
    down = FT.residual(FT.Rows(A, descending=True), x, f)
    differ = int(np.count_nonzero(up.view(np.uint32) != down.view(np.uint32)))
    print(f"\n33x20 residual, ascending against descending columns: {differ} of {up.size} entries differ")
    assert differ >= 1
    assert np.allclose(up, down, rtol=0, atol=1e-4)  # the same sum, another order


def test_a_level_that_is_not_symmetric_walks_two_matrices():
    A = MT.operator("33x20")[2].copy()
    B = sp.csr_matrix(A + sp.diags([0.25], [1], shape=A.shape))
    ident = sp.identity(A.shape[0], format="csr")
    assert FT.Hierarchy([A, A], [ident], [ident], ("jacobi", 0.8, 1), None).symmetric(0)
    H = FT.Hierarchy([B, B], [ident], [ident], ("jacobi", 0.8, 1), None)
    assert not H.symmetric(0)
    rng = np.random.default_rng(6)
    x, f = (rng.standard_normal(A.shape[0]).astype(np.float32) for _ in range(2))
    # the sweep walks B transposed, the residual B
    assert FT.same_bits(H.smooth(0, x, f), FT.jacobi(FT.Rows(B.T), x, f, 0.8))
    assert FT.same_bits(H.resid(0, x, f), FT.residual(FT.Rows(B), x, f))
    assert not FT.same_bits(H.smooth(0, x, f), FT.jacobi(FT.Rows(B), x, f, 0.8))
