"""K-Patch hand-over between two consecutive K-Patch levels (amg_hip_set_patch_xf): the down-leg of
the coarser level forms its first from-zero Jacobi sweep from the f it loads anyway, and the finer
level's down-leg stores f_H alone.  Same expression on the same bits as the stored form, so the
bar is bitwise: switch on against switch off, and both against the oracle twin, on every level
vector -- on the Poisson hierarchy, on an anisotropic box with ragged lines and several row types,
with coarse rows that have no diagonal, under graph replay, and over the line ranges of the slab
and window forms.  cycle_must_move() proves that the new path ran."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "algebraic-multigrid_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

OMEGA = 0.6


@pytest.fixture
def patch_everywhere(amg):
    amg.set_patch_min_rows(0)          # every level whose band has a 2-D pitch >= 128
    yield
    amg.set_patch_min_rows(amg.PATCH_MIN_ROWS_DEFAULT)


def _to_csc(oracle, n, rows, cols, vals):
    order = np.lexsort((rows, cols))
    colptr = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(cols, minlength=n), out=colptr[1:])
    return oracle.CSC(n, n, colptr, rows[order].astype(np.int32), vals[order].astype(np.float64))


def box2d(oracle, nx, ny):
    """The anisotropic box of tests/test_gpu_round2.py: the x coupling alternates with the column
    parity and the y coupling with the line parity, the diagonal is 0.125 larger on odd lines."""
    n = nx * ny
    r = np.arange(n, dtype=np.int64)
    i, j = r % nx, r // nx
    wx = np.where(i % 2 == 0, -1.0, -0.75)
    wy = np.where(j % 2 == 0, -0.375, -0.5)
    ox, oy = i < nx - 1, j < ny - 1
    rows = np.concatenate([r[ox], r[ox] + 1, r[oy], r[oy] + nx, r])
    cols = np.concatenate([r[ox] + 1, r[ox], r[oy] + nx, r[oy], r])
    vals = np.concatenate([wx[ox], wx[ox], wy[oy], wy[oy], 4.0 + 0.125 * (j % 2)])
    return _to_csc(oracle, n, rows, cols, vals)


def box2d_no_diag(oracle, nx, ny, no_diag):
    """5-point box with x coupling -1, y coupling -0.375 and diagonal 4; the rows `no_diag` (odd
    flat index 2c + 1, not at a line end) have no diagonal entry.  The Galerkin diagonal of the
    coarse row c is then 0.25 * 4 + 0.25 * 4 + 2 * 0.5 * (-1) + 2 * 0.5 * (-1) = 0 exactly."""
    n = nx * ny
    r = np.arange(n, dtype=np.int64)
    i, j = r % nx, r // nx
    ox, oy = i < nx - 1, j < ny - 1
    keep = np.ones(n, bool)
    keep[list(no_diag)] = False
    rows = np.concatenate([r[ox], r[ox] + 1, r[oy], r[oy] + nx, r[keep]])
    cols = np.concatenate([r[ox] + 1, r[ox], r[oy] + nx, r[oy], r[keep]])
    vals = np.concatenate([np.full(int(ox.sum()), -1.0)] * 2 + [np.full(int(oy.sum()), -0.375)] * 2 +
                          [np.full(int(keep.sum()), 4.0)])
    return _to_csc(oracle, n, rows, cols, vals)


NO_DIAG_ROWS = (7 * 256 + 101, 30 * 256 + 33, 45 * 256 + 201)   # lines of both tile rows of 256 x 50


def _problem(oracle, shape):
    """(A, b, levels, index of the first level that is no K-Patch level)"""
    if shape == "lap512":       # pitches 512, 256, 128 are patch levels; 64 is too narrow
        return oracle.laplacian(512), oracle.rhs(512), 7, 3
    if shape == "box1024x300":  # pitches 1024 .. 128
        A = box2d(oracle, 1024, 300)
        return A, np.sin(0.001 * np.arange(A.rows)) + 1.5, 9, 4
    assert shape == "nodiag256x50"   # pitches 256, 128
    A = box2d_no_diag(oracle, 256, 50, NO_DIAG_ROWS)
    return A, np.sin(0.001 * np.arange(A.rows)) + 1.5, 4, 2


def _csc(A):
    return A.colptr, A.rowind, A.val


_ORACLE = {}


def _oracle_levels(oracle, shape, cycles=3):
    """u, f, r of every level after each cycle of the oracle twin; computed once per shape"""
    if shape not in _ORACLE:
        A, b, L, _ = _problem(oracle, shape)
        ref = oracle.Multigrid(A, b, L, smoother=oracle.SM_TRUE_JACOBI, smoother_iters=2, omega=OMEGA)
        out = []
        for _ in range(cycles):
            ref.vcycle()
            out.append([(ref.get_vec(l, "u"), ref.get_vec(l, "f"), ref.get_vec(l, "r")) for l in range(L)])
        _ORACLE[shape] = (out, ref.rss())
    return _ORACLE[shape]


def _solver(amg, oracle, shape, xf, keep, **extra):
    A, b, L, _ = _problem(oracle, shape)
    amg.set_patch_xf(xf)
    try:
        return amg.Multigrid(*_csc(A), b, L, smoother=amg.SM_JACOBI, smoother_iters=2, omega=OMEGA,
                             keep_residual=keep, exact_coarse_solve=True, **extra)
    finally:
        amg.set_patch_xf(1)


def _levels(mg, L, keep):
    return [(mg.get_soln(l), mg.get_rhs(l), mg.get_residual(l) if keep else None) for l in range(L)]


def _assert_same(a, b, tag):
    for l, (x, y) in enumerate(zip(a, b)):
        for name, p, q in zip("ufr", x, y):
            if p is not None and q is not None:
                assert np.array_equal(p, q), (tag, l, name)


@pytest.mark.parametrize("shape", ["lap512", "box1024x300", "nodiag256x50"])
def test_xf_on_off_bitwise_and_bytes(amg, oracle, patch_everywhere, shape):
    """3 cycles from a random non-zero start, residual kept: every level's u, f, r and rss() equal
    with the switch on and off.  Per pair of consecutive K-Patch levels (l, l+1) the "on" cycle has to
    move 16 n_{l+1} bytes less (8 for the store, 8 for the load) and, under the tiles that do not get
    the coarse diagonal as a kernel argument, the 8 bytes per coarse row of that diagonal: between 16
    and 24 n_{l+1}, which only a cycle that took the new path on every such pair reaches
    (test_xf_bytes_exact_without_tile_flags pins the figure exactly)."""
    A, b, L, npatch = _problem(oracle, shape)
    u0 = np.random.default_rng(11).standard_normal(A.rows)
    got = {}
    for xf in (1, 0):
        mg = _solver(amg, oracle, shape, xf, True)
        try:
            assert mg.profile_fine_sweep(1)[3].startswith("patch_down_kernel")
            rows = [mg.get_n_dofs(l) for l in range(L)]
            mg.set_vec(0, "u", u0)
            mg.vcycle(3)
            got[xf] = (_levels(mg, L, True), mg.rss(), mg.cycle_must_move())
        finally:
            mg.close()
    _assert_same(got[1][0], got[0][0], shape)
    assert got[1][1] == got[0][1]
    assert npatch >= 2
    pairs = float(sum(rows[l + 1] for l in range(npatch - 1)))
    assert 16.0 * pairs <= got[0][2] - got[1][2] <= 24.0 * pairs, (got[0][2], got[1][2], pairs)


@pytest.mark.parametrize("shape", ["lap512", "nodiag256x50"])
def test_xf_bytes_exact_without_tile_flags(amg, oracle, patch_everywhere, shape):
    """Without the per-tile flags every stored-form down-leg reads the coarse diagonal for every coarse
    row: the cycle then has to move exactly 24 n_{l+1} bytes more per pair of K-Patch levels than the
    new form (first sweep stored, first sweep loaded, coarse diagonal).  No cycle is run: the figure
    is summed while the graph is captured."""
    _, _, L, npatch = _problem(oracle, shape)
    mm = {}
    amg.set_patch_tile_flags(False)
    try:
        for xf in (1, 0):
            mg = _solver(amg, oracle, shape, xf, False)
            try:
                rows = [mg.get_n_dofs(l) for l in range(L)]
                mm[xf] = mg.cycle_must_move()
            finally:
                mg.close()
    finally:
        amg.set_patch_tile_flags(True)
    assert mm[0] - mm[1] == 24.0 * sum(rows[l + 1] for l in range(npatch - 1)), mm


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("shape", ["lap512", "box1024x300", "nodiag256x50"])
def test_xf_against_oracle(amg, oracle, patch_everywhere, shape, keep):
    """every level vector equals the oracle twin's bit for bit after each of 3 cycles"""
    _, _, L, _ = _problem(oracle, shape)
    ref, ref_rss = _oracle_levels(oracle, shape)
    mg = _solver(amg, oracle, shape, 1, keep)
    try:
        for c in range(3):
            mg.vcycle()
            for l in range(L):
                if l < L - 1 or keep:      # the coarsest level's u is the direct solve either way
                    assert np.array_equal(mg.get_soln(l), ref[c][l][0]), (c, l, "u")
                assert np.array_equal(mg.get_rhs(l), ref[c][l][1]), (c, l, "f")
                if keep:
                    assert np.array_equal(mg.get_residual(l), ref[c][l][2]), (c, l, "r")
        assert abs(mg.rss() - ref_rss) <= 1e-11 * ref_rss
    finally:
        mg.close()


def test_no_diag_case_has_coarse_rows_without_diagonal(amg, oracle):
    """the hierarchy the d == 0 guard is tested on really has it: the level-1 rows under the fine
    rows without a diagonal have a diagonal of exactly 0 (and nothing else on level 1 does)"""
    A, b, L, _ = _problem(oracle, "nodiag256x50")
    h = amg.Multigrid(*_csc(A), b, L, smoother=amg.SM_JACOBI, smoother_iters=2, omega=OMEGA, host_only=True)
    try:
        cp, ri, v = h.get_coefficient_matrix(1)
        n1 = cp.size - 1
        diag = np.zeros(n1)
        for c in range(n1):
            s = slice(cp[c], cp[c + 1])
            hit = ri[s] == c
            if hit.any():
                diag[c] = v[s][hit][0]
        assert sorted(np.flatnonzero(diag == 0.0).tolist()) == sorted((r - 1) // 2 for r in NO_DIAG_ROWS)
    finally:
        h.close()


def test_xf_graph_and_eager_bitwise(amg, oracle, patch_everywhere):
    got = []
    for use_graph in (True, False):
        mg = _solver(amg, oracle, "lap512", 1, True, use_graph=use_graph)
        try:
            mg.vcycle(3)
            got.append((_levels(mg, 7, True), mg.rss()))
        finally:
            mg.close()
    _assert_same(got[0][0], got[1][0], "graph/eager")
    assert got[0][1] == got[1][1]


# ---- ranged launches: the slab and window forms use the hand-over too ----
def _single_poisson(amg, n, L, cycles):
    mg = amg.Multigrid.poisson(n, L, smoother=amg.SM_JACOBI, smoother_iters=2, omega=OMEGA)
    try:
        mg.vcycle(cycles)
        return mg.get_soln(0)
    finally:
        mg.close()


@pytest.mark.parametrize("max_levels", [-1, 2])
def test_xf_slab_two_ranks_on_off(amg, patch_everywhere, max_levels):
    """slab_setup(rank, 2) on 1024^2 / 9 levels (the slab tests' shape), switch on and off, against
    the single-solver cycle; max_levels = 2 cuts between two K-Patch levels, so the replicated rest
    begins with a level that forms its own first sweep."""
    import torch
    import slab_vcycle
    from test_gpu_slab import _assemble, _cycle
    n, L, cycles = 1024, 9, 3
    u_ref = _single_poisson(amg, n, L, cycles)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    torch.cuda.set_stream(st)
    for xf in (1, 0):
        amg.set_patch_xf(xf)
        try:
            engs = [slab_vcycle.HipSlabEngine(amg, dev, st, n, L, OMEGA, 2, r, 2, max_levels) for r in range(2)]
        finally:
            amg.set_patch_xf(1)
        try:
            assert int(engs[0].info.levels) == (4 if max_levels < 0 else max_levels)
            for _ in range(cycles):
                _cycle(engs, poison=True)
            st.synchronize()
            assert np.array_equal(_assemble(engs), u_ref), xf
        finally:
            for e in engs:
                e.close()


def test_xf_window_two_ranks_on_off(amg, patch_everywhere):
    """two windows of 1024^2 with three window levels (the window tests' shape), switch on and off"""
    from test_gpu_window import JAC, _sharded
    n, L, k, cycles = 1024, 10, 3, 3
    u_ref = _single_poisson(amg, n, L, cycles)
    for xf in (1, 0):
        amg.set_patch_xf(xf)
        try:
            res = _sharded(amg, 2, n, L, k, 2, JAC, 2, OMEGA, cycles)
        finally:
            amg.set_patch_xf(1)
        assert np.array_equal(res[0][0], u_ref), xf
