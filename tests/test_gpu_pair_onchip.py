"""The pair kernels of the small levels (dict_pair_down_kernel / dict_pair_up_kernel) load every
operand at kernel entry -- tables, the window of `a` the first sweep gathers from, f and the row
types (or code words) of the window rows into LDS, the tail's operand into registers -- and run
both steps from LDS.  The arithmetic does not move, so the bar is bitwise: u, f and r of every level
after each of three cycles against the oracle twin and against the same solver without fusion,
on the shapes at which each branch of the memory phase runs:
  laplacian(256), 9 levels   levels 2-7 are pair levels with half-bandwidths 65 (the window at its
                             capacity), 33, 17, 9, 5, 3; level 7 has two tiles, the second holding a
                             single row; every first tile starts before row 0, every last tile runs
                             past n
  the same, no row types     code words staged instead of row types, one and two words per row
  box2d(300, 50), 7 levels   ragged lines, several row types per wave, n no multiple of 510; levels
                             3-5 are pair levels
  zero-diagonal box, 5 lvls  level 2 (a pair level under the pair level 1) holds rows whose Galerkin
                             diagonal is exactly 0: the d == 0 guard of the down tail on a preloaded
                             coarse diagonal, and the no-diagonal branch of the row walk
cycle_must_move() shows which levels took the pair form."""
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
CYCLES = 3


def _to_csc(oracle, n, rows, cols, vals):
    order = np.lexsort((rows, cols))
    colptr = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(cols, minlength=n), out=colptr[1:])
    return oracle.CSC(n, n, colptr, rows[order].astype(np.int32), vals[order].astype(np.float64))


def box2d(oracle, nx, ny):
    """The anisotropic box of tests/test_gpu_patch_xf.py: the x coupling alternates with the column
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


# Fine rows 4 c + 3 (weight 1 in the coarse point c of level 2, not at a line end) whose diagonal is
# -2 instead of 4: the level-2 diagonal of an interior row of the plain box is 6 and the fine
# diagonal enters it with weight 1, so these level-2 rows get 6 - 4 - 2 = 0 exactly.
ZERO_DIAG_FINE = (7 * 128 + 43, 30 * 128 + 99, 45 * 128 + 19)
ZERO_DIAG_LEVEL = 2
ZERO_DIAG_ROWS = tuple((i - 3) // 4 for i in ZERO_DIAG_FINE)


def box2d_zero_diag(oracle, nx, ny, rows_m2):
    """5-point box with x coupling -1, y coupling -0.375 and diagonal 4, -2 on the rows `rows_m2`"""
    n = nx * ny
    r = np.arange(n, dtype=np.int64)
    i, j = r % nx, r // nx
    ox, oy = i < nx - 1, j < ny - 1
    diag = np.full(n, 4.0)
    diag[list(rows_m2)] = -2.0
    rows = np.concatenate([r[ox], r[ox] + 1, r[oy], r[oy] + nx, r])
    cols = np.concatenate([r[ox] + 1, r[ox], r[oy] + nx, r[oy], r])
    vals = np.concatenate([np.full(int(ox.sum()), -1.0)] * 2 + [np.full(int(oy.sum()), -0.375)] * 2 + [diag])
    return _to_csc(oracle, n, rows, cols, vals)


# shape -> levels, and the levels that take the pair form: half-bandwidth <= 65, at least 256 rows,
# neither the finest nor the coarsest level
LEVELS = {"lap256": 9, "box300x50": 7, "zerodiag128x50": 5}
# (box300x50: half-bandwidths 300, 151, 76, 39, 20, 11, 6 on 15000, 7499, 3749, 1874, 936, 467, 233 rows)
PAIR_LEVELS = {"lap256": (2, 3, 4, 5, 6, 7), "box300x50": (3, 4, 5), "zerodiag128x50": (1, 2, 3)}

_PROBLEM = {}
_ORACLE = {}


def _problem(oracle, shape):
    if shape not in _PROBLEM:
        if shape == "lap256":
            A, b = oracle.laplacian(256), oracle.rhs(256)
        elif shape == "box300x50":
            A = box2d(oracle, 300, 50)
            b = np.sin(0.001 * np.arange(A.rows)) + 1.5
        else:
            assert shape == "zerodiag128x50"
            A = box2d_zero_diag(oracle, 128, 50, ZERO_DIAG_FINE)
            b = np.sin(0.001 * np.arange(A.rows)) + 1.5
        _PROBLEM[shape] = (A, b, LEVELS[shape])
    return _PROBLEM[shape]


def _oracle_twin(oracle, shape):
    """the oracle twin (kept for its level matrices) and u, f, r of every level after each cycle;
    computed once per shape"""
    if shape not in _ORACLE:
        A, b, L = _problem(oracle, shape)
        ref = oracle.Multigrid(A, b, L, smoother=oracle.SM_TRUE_JACOBI, smoother_iters=2, omega=OMEGA)
        out = []
        for _ in range(CYCLES):
            ref.vcycle()
            out.append([(ref.get_vec(l, "u"), ref.get_vec(l, "f"), ref.get_vec(l, "r")) for l in range(L)])
        _ORACLE[shape] = (ref, out)
    return _ORACLE[shape]


def _solver(amg, oracle, shape, keep, **extra):
    A, b, L = _problem(oracle, shape)
    return amg.Multigrid(A.colptr, A.rowind, A.val, b, L, smoother=amg.SM_JACOBI, smoother_iters=2,
                         omega=OMEGA, keep_residual=keep, exact_coarse_solve=True, **extra)


def _run(amg, oracle, shape, keep, **extra):
    """u, f, r (None unless kept) of every level after each cycle, and cycle_must_move()"""
    L = LEVELS[shape]
    mg = _solver(amg, oracle, shape, keep, **extra)
    try:
        out = []
        for _ in range(CYCLES):
            mg.vcycle()
            out.append([(mg.get_soln(l), mg.get_rhs(l), mg.get_residual(l) if keep else None) for l in range(L)])
        return out, mg.cycle_must_move()
    finally:
        mg.close()


def _assert_same(a, b, tag, skip_coarsest_u=False):
    assert len(a) == len(b) == CYCLES
    for c, (la, lb) in enumerate(zip(a, b)):
        for l, (x, y) in enumerate(zip(la, lb)):
            for name, p, q in zip("ufr", x, y):
                if p is None or q is None or (skip_coarsest_u and name == "u" and l == len(la) - 1):
                    continue
                assert np.array_equal(p, q), (tag, "cycle", c, "level", l, name)


def _check(amg, oracle, shape, keep):
    """fused cycle against the oracle twin and against the same solver built with no_fusion"""
    _, ref = _oracle_twin(oracle, shape)
    got, _ = _run(amg, oracle, shape, keep)
    # without the residual kept the coarsest level's u is the direct solve either way, not the oracle's vector
    _assert_same(got, ref, (shape, "oracle"), skip_coarsest_u=not keep)
    plain, _ = _run(amg, oracle, shape, keep, no_fusion=True)
    _assert_same(got, plain, (shape, "no_fusion"))


@pytest.fixture
def no_row_types(amg):
    amg.set_row_types(False)
    try:
        yield
    finally:
        amg.set_row_types(True)


@pytest.mark.parametrize("keep", [False, True])
def test_pair_poisson_bitwise(amg, oracle, keep):
    _check(amg, oracle, "lap256", keep)


@pytest.mark.parametrize("keep", [False, True])
def test_pair_poisson_code_words_bitwise(amg, oracle, no_row_types, keep):
    """rtype == nullptr: the code words of the window rows are staged; levels of one word per row
    (<= 8 entries) and of two occur in this hierarchy"""
    _check(amg, oracle, "lap256", keep)


@pytest.mark.parametrize("keep", [False, True])
def test_pair_box_bitwise(amg, oracle, keep):
    _check(amg, oracle, "box300x50", keep)


@pytest.mark.parametrize("keep", [False, True])
def test_pair_zero_diagonal_bitwise(amg, oracle, keep):
    _check(amg, oracle, "zerodiag128x50", keep)


def test_zero_diagonal_case_has_the_rows(oracle):
    """the oracle's level 2 of the zero-diagonal box has a diagonal of exactly 0 in the rows
    ZERO_DIAG_ROWS and nowhere else, and its half-bandwidth and those of levels 1 and 3 fit the pair
    window (test_pair_levels_by_bytes shows that the solver runs levels 1-3 in pair form)"""
    ref, _ = _oracle_twin(oracle, "zerodiag128x50")
    for l in PAIR_LEVELS["zerodiag128x50"]:
        M = ref.level_matrix(l)
        col = np.repeat(np.arange(M.rows), np.diff(M.colptr))
        nz = M.val != 0.0
        assert M.rows >= 256 and int(np.abs(M.rowind[nz] - col[nz]).max()) <= 65, l
        diag = np.zeros(M.rows)
        on = (M.rowind == col)
        diag[col[on]] = M.val[on]
        zero = np.flatnonzero(diag == 0.0).tolist()
        assert zero == (sorted(ZERO_DIAG_ROWS) if l == ZERO_DIAG_LEVEL else []), (l, zero)


@pytest.mark.parametrize("shape", ["lap256", "box300x50", "zerodiag128x50"])
def test_pair_levels_by_bytes(amg, oracle, shape):
    """Which levels took the pair form, from the bytes the cycle has to move.  A pair level l accounts
    mat + 24 n + 24 n_H on the way down and mat + 24 n + 16 n_F on the way up.  With one row per
    lane (set_dict_rows(1)) no level qualifies and the same level runs the second pre-sweep
    (mat + 24 n) and the fused residual + restriction (mat + 16 n + 24 n_H) on the way down, a sweep
    (mat + 24 n) and the sweep that prolongs (mat + 24 n + 16 n_F) on the way up: 2 mat + 40 n more
    per pair level, where mat is the matrix stream of one application (level_layout).
    set_dict_rows is the library's switch for the pair form (dict_pair_ok asks for two rows per lane)
    and changes nothing else in the accounting, so the difference isolates the pair branches; against
    no_fusion every other fusion of the cycle would be in it too."""
    L = LEVELS[shape]
    mm = {}
    for rows_per_lane in (2, 1):
        amg.set_dict_rows(rows_per_lane)
        try:
            mg = _solver(amg, oracle, shape, False)
            try:
                n = [mg.get_n_dofs(l) for l in range(L)]
                mat = [mg.level_layout(l)[1] for l in range(L)]
                mm[rows_per_lane] = mg.cycle_must_move()
            finally:
                mg.close()
        finally:
            amg.set_dict_rows(2)
    want = float(sum(2 * mat[l] + 40 * n[l] for l in PAIR_LEVELS[shape]))
    print(f"\n{shape}: rows {n}, must move {mm[2]:.0f} (pair) / {mm[1]:.0f} (one row per lane), want {want:.0f} less")
    assert mm[1] - mm[2] == want, (mm, want)


def test_pair_graph_and_eager_bitwise(amg, oracle):
    graph, _ = _run(amg, oracle, "lap256", True)
    eager, _ = _run(amg, oracle, "lap256", True, use_graph=False)
    _assert_same(graph, eager, "graph/eager")
