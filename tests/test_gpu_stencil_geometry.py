"""GPU tests of the fused stencil kernels on anisotropic, non-cubic operators: K-March (both Jacobi
sweeps of a 3-D 7-point level in one plane-marching launch) and the wave-uniform stencil rows
(dict_rows_stencil), on box operators whose six neighbour weights differ, some of them nonsymmetric,
with perturbed row classes and with couplings that wrap across a line or plane edge.

Every operator is built here with numpy and replayed by the oracle twin; true Jacobi with the exact
coarse solve is bit-exact against it, so u and f of every level (and r where it is kept) are compared
bitwise.  Every case also asserts which level-0 kernel ran, so that a silent fallback cannot make a
case vacuous.  Nothing here reads the reference tree."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# x, y, z couplings of the symmetric anisotropic box; the convection part of the nonsymmetric one
W_SYM = (-1.0, -0.375, -1.625)
W_CONV = (0.25, 0.125, 0.3125)


def box3d(nx, ny, nz, nonsym=False, diag_mod=0, no_diag=(), wrap=()):
    """7-point operator on an nx x ny x nz box (dof = k*nx*ny + j*nx + i) as (colptr, rowind, val).

    Six neighbour weights: w(-1) = wx - cx, w(+1) = wx + cx, and so on, c = 0 unless nonsym.  The
    diagonal is 0.5 above the sum of the neighbour magnitudes, plus 0.0625 * (k % diag_mod) when
    diag_mod > 0 (bounded row classes by plane).  no_diag: rows without a diagonal entry.  wrap:
    extra (row, col, value) entries, e.g. couplings across a line end."""
    n = nx * ny * nz
    r = np.arange(n, dtype=np.int64)
    i, j, k = r % nx, (r // nx) % ny, r // (nx * ny)
    c = W_CONV if nonsym else (0.0, 0.0, 0.0)
    rows, cols, vals = [], [], []
    for (dim, lo, step), (w, cc) in zip(((i, nx, 1), (j, ny, nx), (k, nz, nx * ny)), zip(W_SYM, c)):
        for sgn, ok in ((-1, dim > 0), (1, dim < lo - 1)):
            rows.append(r[ok])
            cols.append(r[ok] + sgn * step)
            vals.append(np.full(int(ok.sum()), w + sgn * cc))
    diag = 2.0 * sum(abs(w) for w in W_SYM) + 2.0 * sum(c) + 0.5
    d = np.full(n, diag)
    if diag_mod:
        d += 0.0625 * (k % diag_mod)
    keep = np.ones(n, bool)
    keep[list(no_diag)] = False
    rows.append(r[keep])
    cols.append(r[keep])
    vals.append(d[keep])
    for (a, b, v) in wrap:
        rows.append(np.array([a]))
        cols.append(np.array([b]))
        vals.append(np.array([v]))
    return to_csc(n, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals))


def band(n, offsets, weights, diag):
    """A band with every offset present on every row where the column is in range (no box edges)."""
    r = np.arange(n, dtype=np.int64)
    rows, cols, vals = [r], [r], [np.full(n, diag)]
    for o, w in zip(offsets, weights):
        ok = (r + o >= 0) & (r + o < n)
        rows.append(r[ok])
        cols.append(r[ok] + o)
        vals.append(np.full(int(ok.sum()), w))
    return to_csc(n, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals))


def to_csc(n, rows, cols, vals):
    order = np.lexsort((rows, cols))
    rows, cols, vals = rows[order], cols[order], vals[order]
    colptr = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(cols, minlength=n), out=colptr[1:])
    return colptr, rows.astype(np.int32), vals.astype(np.float64)


def rhs_for(n):
    return np.sin(0.001 * np.arange(n)) + 1.5


def levels_for(n, coarse=1500):
    """levels such that the coarsest band solve stays small (the linear coarsening halves n)"""
    L = 2
    while n // 2 ** (L - 1) > coarse:
        L += 1
    return L


def snapshot(mg, L, keep):
    return ([mg.get_soln(l) for l in range(L)], [mg.get_rhs(l) for l in range(L)],
            [mg.get_residual(l) for l in range(L)] if keep else [])


def assert_equal_to_oracle(mg, ref, L, keep, tag):
    for l in range(L):
        if l < L - 1 or keep:  # the coarsest level's u is the direct solve either way
            assert np.array_equal(mg.get_soln(l), ref.get_vec(l, "u")), (tag, l, "u")
        assert np.array_equal(mg.get_rhs(l), ref.get_vec(l, "f")), (tag, l, "f")
        if keep:
            assert np.array_equal(mg.get_residual(l), ref.get_vec(l, "r")), (tag, l, "r")


def run_against_oracle(amg, oracle, op, L, cycles, keep, expect_march, **extra):
    """true Jacobi 2 sweeps (omega 0.6), dictionary layout: every level against the oracle after
    every cycle; returns the final snapshot and rss"""
    cp, ri, v = op
    n = cp.size - 1
    b = rhs_for(n)
    ref = oracle.Multigrid(oracle.CSC(n, n, cp, ri, v), b, L, smoother=oracle.SM_TRUE_JACOBI,
                           smoother_iters=2, omega=0.6)
    mg = amg.Multigrid(cp, ri, v, b, L, smoother=amg.SM_JACOBI, smoother_iters=2, omega=0.6,
                       layout=amg.LAYOUT_DICT, keep_residual=keep, exact_coarse_solve=True, **extra)
    try:
        name = mg.fine_sweep_info()[0]
        for c in range(cycles):
            ref.vcycle()
            mg.vcycle()
            assert_equal_to_oracle(mg, ref, L, keep, c)
        assert abs(mg.rss() - ref.rss()) <= 1e-11 * ref.rss()
        assert (name == "march_kernel") == expect_march, name
        return snapshot(mg, L, keep), mg.rss()
    finally:
        mg.close()


# ------------------------------------------------------------------------- B: K-March vs oracle
# (nx, ny, nz): launch_march tiles 64 columns x 16 lines, chunks = max(1, min(nz / 8, ceil(512 / tiles))),
# chunk_planes = ceil(nz / chunks)
MARCH_SHAPES = [
    (64, 16, 3),      # 1 tile, 1 chunk of 3 planes: the smallest box K-March takes
    (64, 16, 37),     # 1 tile, 4 chunks of 10, 10, 10, 7 planes (ragged last chunk)
    (192, 16, 130),   # 3 column tiles, 15 chunks: 14 of 9 planes + one of 4
    (128, 48, 17),    # 2 column x 3 line tiles, 2 chunks of 9 and 8 planes
    (1024, 512, 4),   # 16 x 32 = 512 tiles: one chunk spans all 4 planes
]


@pytest.mark.parametrize("nonsym", [False, True], ids=["sym", "nonsym"])
@pytest.mark.parametrize("shape", MARCH_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_march_anisotropic_box_against_oracle_and_no_fusion(amg, oracle, shape, nonsym):
    """K-March on an anisotropic box (six distinct neighbour weights when nonsymmetric, then the
    smoother's columns and the residual's rows differ; the residual is kept there): u, f (and r) of
    every level equal the oracle bitwise after each of 3 cycles, and equal no_fusion (two launches of
    the dictionary sweep per leg)."""
    op = box3d(*shape, nonsym=nonsym)
    n = op[0].size - 1
    L = levels_for(n)
    keep = nonsym
    got, rss = run_against_oracle(amg, oracle, op, L, 3, keep, True)
    b = rhs_for(n)
    mg = amg.Multigrid(*op, b, L, smoother=amg.SM_JACOBI, smoother_iters=2, omega=0.6, layout=amg.LAYOUT_DICT,
                       keep_residual=keep, exact_coarse_solve=True, no_fusion=True)
    try:
        assert mg.fine_sweep_info()[0] != "march_kernel"
        mg.vcycle(3)
        want = snapshot(mg, L, keep)
        for a, c in zip(got, want):
            for l, (x, y) in enumerate(zip(a, c)):
                assert np.array_equal(x, y), l
        assert mg.rss() == rss
    finally:
        mg.close()


@pytest.mark.parametrize("shape,diag_mod,marches", [((64, 16, 37), 5, True), ((64, 16, 37), 7, False),
                                                    ((128, 48, 17), 5, True)])
def test_march_row_type_budget(amg, oracle, shape, diag_mod, marches):
    """Diagonal shifted by plane index mod 5: 9 in-plane classes x (first plane, 5 residues, last
    plane) = 63 row types, within K-March's 64, so the level still marches; mod 7 gives 81 types and
    the level falls back to the dictionary sweep.  Nonsymmetric; both equal the oracle bitwise."""
    op = box3d(*shape, nonsym=True, diag_mod=diag_mod)
    run_against_oracle(amg, oracle, op, levels_for(op[0].size - 1), 2, False, marches)


def test_march_rows_without_diagonal(amg, oracle):
    """A few rows without a diagonal entry (the sweep keeps their value): still marched, still
    equal to the oracle bitwise."""
    nx, ny, nz = 128, 16, 9
    op = box3d(nx, ny, nz, no_diag=(5 * nx * ny + 3 * nx + 7, 7 * nx * ny + 9 * nx + 100))
    run_against_oracle(amg, oracle, op, levels_for(op[0].size - 1), 2, True, True)


@pytest.mark.parametrize("shape", [(96, 16, 8), (64, 24, 8), (65, 16, 8)], ids=["nx96", "ny24", "nx65"])
def test_march_refuses_shapes_off_its_tiles(amg, oracle, shape):
    """nx not a multiple of 64, ny not a multiple of 16, odd nx (which also turns off the paired
    loads of the stencil rows): march_ok refuses, and the cycle still equals the oracle bitwise."""
    op = box3d(*shape, nonsym=True)
    run_against_oracle(amg, oracle, op, levels_for(op[0].size - 1), 2, True, False)


# --------------------------------------------------------------- D: couplings across box edges
def test_march_refuses_flat_band_with_line_wrap(amg, oracle):
    """Offsets +-1, +-64, +-1024 on every row where the column exists (n = 1024 * 8): the offset
    pattern of a 64 x 16 x 8 box, but the rows at a line end couple to the next line.  K-March would
    drop those products; it must not take the level, and the cycle equals the oracle bitwise."""
    op = band(1024 * 8, (-1024, -64, -1, 1, 64, 1024), (-1.5, -0.5, -1.0, -1.0, -0.5, -1.5), 7.0)
    run_against_oracle(amg, oracle, op, 5, 2, True, False)


def test_march_refuses_single_wrap_couplings(amg, oracle):
    """A true 64 x 16 x 8 box, except that one row at column nx-1 couples to the next line's first
    column and one row at line ny-1 to the next plane's first line (rows only: A != A^T, so the
    smoother's column walk sees them at column 0 / line 0).  Not marched, equal to the oracle."""
    nx, ny, nz = 64, 16, 8
    r1 = 3 * nx * ny + 5 * nx + nx - 1
    r2 = 4 * nx * ny + (ny - 1) * nx + 17
    op = box3d(nx, ny, nz, wrap=((r1, r1 + 1, -0.125), (r2, r2 + nx, -0.0625)))
    run_against_oracle(amg, oracle, op, 5, 2, True, False)


# ------------------------------------------------------------- E: buffer roles of K-March
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "stream"])
def test_march_on_a_single_level_keeps_its_buffers(amg, oracle, use_graph):
    """n_levels = 1: K-March sweeps the only level on the down-leg alone, then the direct solve.  u
    and the kept r equal the oracle after every one of 3 cycles (graph replays included), and the
    level-0 u buffer is the same one before the first cycle and after the third."""
    op = box3d(64, 16, 4, nonsym=True)
    cp, ri, v = op
    n = cp.size - 1
    b = rhs_for(n)
    ref = oracle.Multigrid(oracle.CSC(n, n, cp, ri, v), b, 1, smoother=oracle.SM_TRUE_JACOBI,
                           smoother_iters=2, omega=0.6)
    mg = amg.Multigrid(cp, ri, v, b, 1, smoother=amg.SM_JACOBI, smoother_iters=2, omega=0.6,
                       layout=amg.LAYOUT_DICT, keep_residual=True, exact_coarse_solve=True,
                       use_graph=use_graph)
    try:
        assert mg.fine_sweep_info()[0] == "march_kernel"
        p0 = mg.vec_dev_ptr(0, "u")
        for c in range(3):
            ref.vcycle()
            mg.vcycle()
            assert np.array_equal(mg.get_soln(0), ref.get_vec(0, "u")), c
            assert np.array_equal(mg.get_residual(0), ref.get_vec(0, "r")), c
        assert mg.vec_dev_ptr(0, "u") == p0
    finally:
        mg.close()


# ------------------------------------------------- C: wave-uniform stencil rows, anisotropic 3-D
@pytest.mark.parametrize("kind", ["jacobi2", "jacobi1", "cheb2"])
def test_stencil_rows_anisotropic_box_bit_neutral(amg, kind):
    """The paired-load stencil rows (dict_rows_stencil) against plain dict_rows on a symmetric
    anisotropic 256 x 32 x 15 box: level 0 is a 7-point level with three different weights, the
    Galerkin levels below it 15-point patterns with unequal weights.  True Jacobi (2 sweeps: level 0
    marches; 1 sweep: level 0 takes the stencil rows too) and Chebyshev of degree 2 (the CSR_CHEB
    mode): every level vector bitwise after 3 cycles, same rss."""
    op = box3d(256, 32, 15)
    n = op[0].size - 1
    L = levels_for(n)
    b = rhs_for(n)
    kw = {"jacobi2": dict(smoother=amg.SM_JACOBI, smoother_iters=2, omega=0.6),
          "jacobi1": dict(smoother=amg.SM_JACOBI, smoother_iters=1, omega=0.6),
          "cheb2": dict(smoother=amg.SM_CHEBYSHEV, smoother_iters=1, cheb_degree=2)}[kind]
    out = []
    for on in (1, 0):
        amg.set_dict_stencil(on)
        try:
            mg = amg.Multigrid(*op, b, L, layout=amg.LAYOUT_DICT, keep_residual=True, **kw)
            try:
                assert (mg.fine_sweep_info()[0] == "march_kernel") == (kind == "jacobi2")
                mg.vcycle(3)
                out.append((snapshot(mg, L, True), mg.rss()))
            finally:
                mg.close()
        finally:
            amg.set_dict_stencil(1)
    for a, c in zip(out[0][0], out[1][0]):
        for l, (x, y) in enumerate(zip(a, c)):
            assert np.array_equal(x, y), (kind, l)
    assert out[0][1] == out[1][1]
