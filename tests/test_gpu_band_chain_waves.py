"""K-BandChain as a four-wave workgroup (kernels.hip: band_chain_kernel, 256 threads around a
recurrence that wave 0 walks): staging, the scaling by D^-1, the store of x and the fused
prolongation are spread over all threads in rounds of 256, so the sizes below sit on the edges of
a wave (64), of a 256-thread round, of the 512-row entry round, of the 16-step chunk padding and
of band_chain_ok (2048 rows).  Every comparison is numpy.array_equal against the CPU oracle and
against the one-wave K-Band path (set_band_chain(False)): same operations on the same operands in
the same order, so the same bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048]


def csc(A):
    return A.colptr, A.rowind, A.val


def banded(oracle, n, w):
    """test_band_chain_bit_exact's random banded matrix and right-hand side"""
    import scipy.sparse as sp
    rng = np.random.default_rng(100 * n + w)
    diags = [-(4.0 + rng.random(n))]
    offs = [0]
    for d in range(1, w + 1):
        v = 0.5 + 0.5 * rng.random(n - d)
        diags += [v, v]
        offs += [d, -d]
    M = sp.diags(diags, offs, format="csc") if n > 1 else sp.csc_matrix(np.array([[-4.5]]))
    M.sort_indices()
    return oracle.CSC(n, n, M.indptr, M.indices, M.data), rng.standard_normal(n)


@pytest.mark.parametrize("n", SIZES)
def test_standalone_solve_bit_exact(amg, oracle, n):
    """amg_hip_coarse_solve on w = 1, 2, 3 (capped at n - 1).  n = 2048, w = 3 needs 115 KB for both
    operand sets: the backward operands go over the forward ones between the passes (pre == 0); so
    do n >= 849 at w = 3, n >= 1201 at w = 2 and n >= 2033 at w = 1."""
    try:
        for w in sorted({min(w, max(n - 1, 0)) for w in (1, 2, 3)}):
            A, f = banded(oracle, n, w)
            want, w_ref = oracle.band_solve(A, f)
            got = {}
            for on in (True, False):
                amg.set_band_chain(on)
                got[on], wg = amg.coarse_solve(*csc(A), f)
                assert wg == w_ref == w, (n, w, on)
            assert np.array_equal(got[True], want), (n, w)
            assert np.array_equal(got[False], want), (n, w)
    finally:
        amg.set_band_chain(True)


JAC22 = dict(smoother_iters=2, omega=0.6)

# Multigrid.poisson(n, L), true Jacobi 2+2: rows and half-bandwidth of the coarsest level, which the
# chain solves and prolongs into level L-2 (2 x rows + 1 fine rows, two pairs per thread and round of
# 1024 fine rows): (n, L, coarsest rows, half-bandwidth)
HIERARCHIES = [
    (32, 5, 63, 3),        # 127 fine rows: one partial round
    (128, 8, 127, 2),
    (512, 10, 511, 2),     # the headline's coarsest shape: 1023 fine rows, one round, one pair idle
    (256, 8, 511, 3),
    (512, 9, 1023, 3),     # 2047 fine rows: two rounds; backward operands over the forward ones
    (1024, 10, 2047, 3),   # 4095 fine rows: four rounds
]


def run_device(amg, n, L, chain, use_graph):
    amg.set_band_chain(chain)
    mg = amg.Multigrid.poisson(n, L, smoother=amg.SM_JACOBI, use_graph=use_graph, **JAC22)
    kind = mg.coarse_solve_kind()
    rows = mg.get_n_dofs(L - 1)
    mg.vcycle(3)
    mg.sync()
    out = [mg.get_soln(l) for l in range(L)]
    mg.close()
    return kind, rows, out


@pytest.mark.parametrize("n,L,rows,w", HIERARCHIES)
def test_fused_prolongation_bit_exact(amg, oracle, n, L, rows, w):
    """After 3 cycles every level vector equals the K-Band run and the oracle; captured-graph and
    eager runs are equal."""
    ref = oracle.Multigrid(oracle.laplacian(n), oracle.rhs(n), L, smoother=oracle.SM_TRUE_JACOBI, **JAC22)
    assert ref.n_dofs(L - 1) == rows and ref.coarse_halfbw() == w
    for _ in range(3):
        ref.vcycle()
    want = [ref.get_vec(l, "u") for l in range(L)]
    try:
        kind, got_rows, chain = run_device(amg, n, L, True, True)
        assert "band-chain" in kind and got_rows == rows
        _, _, eager = run_device(amg, n, L, True, False)
        kind_off, _, band = run_device(amg, n, L, False, True)
        assert "band-chain" not in kind_off
    finally:
        amg.set_band_chain(True)
    for l in range(L):
        assert np.array_equal(chain[l], want[l]), l
        assert np.array_equal(eager[l], chain[l]), l
        assert np.array_equal(band[l], chain[l]), l


def test_block_cycle_chain_on_off(amg, oracle):
    """cols = 3 right-hand sides, one workgroup each (cstride): chain on against chain off"""
    torch = pytest.importorskip("torch")
    n, L = 128, 8
    rng = np.random.default_rng(17)
    got = {}
    try:
        for on in (True, False):
            amg.set_band_chain(on)
            mg = amg.Multigrid.poisson(n, L, smoother=amg.SM_JACOBI, **JAC22)
            assert ("band-chain" in mg.coarse_solve_kind()) == on
            n0 = mg.get_n_dofs(0)
            if on:
                U0, F0 = rng.standard_normal((n0, 3)), rng.standard_normal((n0, 3))
            U = torch.from_numpy(U0.copy()).cuda()
            mg.block_vcycles(U, torch.from_numpy(F0.copy()).cuda(), n=2)
            torch.cuda.synchronize()
            got[on] = U.cpu().numpy()
            mg.close()
    finally:
        amg.set_band_chain(True)
    assert not np.array_equal(got[True], U0)
    for j in range(3):
        assert np.array_equal(got[True][:, j], got[False][:, j]), j
