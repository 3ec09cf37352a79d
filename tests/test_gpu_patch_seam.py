"""K-Patch seam (amg_hip_set_patch_seam): vcycle(n >= 2) runs the level-0 up-leg of one cycle and the
level-0 down-leg of the next as one launch (patch_seam_kernel), so the level-0 vector between two
cycles is neither stored nor loaded.  Same expressions on the same bits as the two launches, so the
bar is bitwise on every level vector: vcycle(n) against n single cycles, against the switch off and
against the oracle twin; graph against eager; both parities of n followed by further calls on the same
solver; tiles with ragged last rows; the shapes of the hand-over tests; and every configuration in
which the seam has to step aside.  patch_leg_lines(0, 2) and cycle_must_move(4) prove which path ran."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "algebraic-multigrid_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from test_gpu_patch_xf import OMEGA, _csc, _problem as _xf_problem, box2d  # noqa: E402

SEAM_LINES = 38      # output lines of a seam tile: 48 held lines less five halo rings above and below


@pytest.fixture
def patch_everywhere(amg):
    amg.set_patch_min_rows(0)          # every level whose band has a 2-D pitch >= 128
    yield
    amg.set_patch_min_rows(amg.PATCH_MIN_ROWS_DEFAULT)


def _problem(oracle, shape):
    """(A, b, levels); "box256xN": the anisotropic box on N lines of 256 (patch levels 0 and 1);
    "lap512small": Poisson 512^2 with the right-hand side scaled by 2^-40, so that its rss lies below
    the 100 that solve() starts from"""
    if shape == "lap512small":
        A, b, L = _xf_problem(oracle, "lap512")[:3]
        return A, b * 2.0 ** -40, L
    if shape.startswith("box256x"):
        A = box2d(oracle, 256, int(shape[len("box256x"):]))
        return A, np.sin(0.001 * np.arange(A.rows)) + 1.5, 4
    return _xf_problem(oracle, shape)[:3]


_ORACLE = {}


def _oracle_levels(oracle, shape, cycles):
    """[(u, f) of every level] after each cycle of the oracle twin; computed once per shape"""
    if shape not in _ORACLE or len(_ORACLE[shape]) < cycles:
        A, b, L = _problem(oracle, shape)
        ref = oracle.Multigrid(A, b, L, smoother=oracle.SM_TRUE_JACOBI, smoother_iters=2, omega=OMEGA)
        out = []
        for _ in range(cycles):
            ref.vcycle()
            out.append([(ref.get_vec(l, "u"), ref.get_vec(l, "f")) for l in range(L)])
        _ORACLE[shape] = out
    return _ORACLE[shape]


def _solver(amg, oracle, shape, seam, **extra):
    A, b, L = _problem(oracle, shape)
    amg.set_patch_seam(seam)
    try:
        return amg.Multigrid(*_csc(A), b, L, smoother=amg.SM_JACOBI, smoother_iters=2, omega=OMEGA,
                             exact_coarse_solve=True, **extra)
    finally:
        amg.set_patch_seam(1)


def _levels(mg, L):
    return [(mg.get_soln(l), mg.get_rhs(l)) for l in range(L)]


def _assert_same(a, b, tag, skip_coarsest_u=False):
    assert len(a) == len(b)
    for l, (x, y) in enumerate(zip(a, b)):
        for name, p, q in zip("uf", x, y):
            if skip_coarsest_u and name == "u" and l == len(a) - 1:
                continue   # the oracle's coarsest u is the direct solve of a smoothed level either way
            assert np.array_equal(p, q), (tag, l, name)


def _run(amg, oracle, shape, seam, calls, expect_seam=None, **extra):
    """the level vectors after vcycle(c) for c in calls on one solver"""
    L = _problem(oracle, shape)[2]
    mg = _solver(amg, oracle, shape, seam, **extra)
    try:
        if expect_seam is not None:
            assert mg.patch_leg_lines(0, 2) == (SEAM_LINES if expect_seam else 0)
        for c in calls:
            mg.vcycle(c)
        return _levels(mg, L)
    finally:
        mg.close()


@pytest.mark.parametrize("n", [2, 3, 4, 7])
def test_seam_against_single_cycles_switch_off_and_oracle(amg, oracle, patch_everywhere, n):
    """Poisson 512^2 (14 tile rows of 38 lines, the last one ragged): vcycle(n) with the seam == n single
    cycles == vcycle(n) without it == the oracle twin after n cycles, on every level vector"""
    on = _run(amg, oracle, "lap512", 1, [n], expect_seam=True)
    singles = _run(amg, oracle, "lap512", 1, [1] * n)
    off = _run(amg, oracle, "lap512", 0, [n], expect_seam=False)
    _assert_same(on, singles, "singles")
    _assert_same(on, off, "off")
    _assert_same(on, _oracle_levels(oracle, "lap512", 7)[n - 1], "oracle", skip_coarsest_u=True)


@pytest.mark.parametrize("n", [3, 4])
def test_seam_graph_and_eager_bitwise(amg, oracle, patch_everywhere, n):
    graph = _run(amg, oracle, "lap512", 1, [n], expect_seam=True, use_graph=True)
    eager = _run(amg, oracle, "lap512", 1, [n], expect_seam=True, use_graph=False)
    _assert_same(graph, eager, "graph/eager")


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("use_graph", [True, False])
def test_seam_both_parities_then_further_calls(amg, oracle, patch_everywhere, n, use_graph):
    """vcycle(n), vcycle(1), vcycle(2) on the same solver: every buffer is where a stand-alone cycle
    expects it whatever the parity of n (the handed-over vector alternates between two buffers)"""
    got = _run(amg, oracle, "lap512", 1, [n, 1, 2], expect_seam=True, use_graph=use_graph)
    _assert_same(got, _oracle_levels(oracle, "lap512", 7)[n + 2], "oracle", skip_coarsest_u=True)


@pytest.mark.parametrize("lines", [SEAM_LINES, SEAM_LINES + 1, 2 * SEAM_LINES, 2 * SEAM_LINES + 1])
def test_seam_line_counts_at_the_tile_height(amg, oracle, patch_everywhere, lines):
    """one and two full tile rows, and each with one line more (a last tile row of a single line)"""
    shape = "box256x%d" % lines
    on = _run(amg, oracle, shape, 1, [3], expect_seam=True)
    off = _run(amg, oracle, shape, 0, [3], expect_seam=False)
    _assert_same(on, off, "off")
    _assert_same(on, _oracle_levels(oracle, shape, 3)[2], "oracle", skip_coarsest_u=True)


@pytest.mark.parametrize("shape", ["box1024x300", "nodiag256x50"])
def test_seam_on_the_hand_over_shapes(amg, oracle, patch_everywhere, shape):
    """the anisotropic box with several row types, and the box whose level-1 rows have a zero Galerkin diagonal"""
    on = _run(amg, oracle, shape, 1, [3], expect_seam=True)
    off = _run(amg, oracle, shape, 0, [3], expect_seam=False)
    _assert_same(on, off, "off")
    _assert_same(on, _oracle_levels(oracle, shape, 3)[2], "oracle", skip_coarsest_u=True)


@pytest.mark.parametrize("nx", [200, 192])
def test_width_that_is_no_multiple_of_the_tile_falls_back(amg, oracle, patch_everywhere, nx):
    """K-Patch tiles are 64 columns wide and a level's pitch has to be a multiple of that, so a width
    of 200 is no K-Patch level at all and one of 192 has a level 1 (pitch 96) that is none: no ragged
    tile column exists, the seam steps aside and the cycles are the two-launch ones"""
    A = box2d(oracle, nx, 60)
    b = np.sin(0.001 * np.arange(A.rows)) + 1.5
    got = []
    for seam in (1, 0):
        amg.set_patch_seam(seam)
        try:
            mg = amg.Multigrid(*_csc(A), b, 4, smoother=amg.SM_JACOBI, smoother_iters=2, omega=OMEGA,
                               exact_coarse_solve=True)
        finally:
            amg.set_patch_seam(1)
        try:
            assert mg.patch_leg_lines(0, 2) == 0
            mg.vcycle(3)
            got.append(_levels(mg, 4))
        finally:
            mg.close()
    _assert_same(got[0], got[1], "off")


def test_non_five_point_level_0_falls_back(amg, oracle, patch_everywhere):
    """only the 5-point kind of the seam kernel is instantiated: a 9-point level 0 (level 1 of the
    Poisson hierarchy as a problem of its own) keeps the two launches and stays identical"""
    A0, b0, _ = _problem(oracle, "lap512")
    A = oracle.Multigrid(A0, b0, 2).level_matrix(1)
    b = np.sin(0.001 * np.arange(A.rows)) + 1.5
    got = []
    for seam in (1, 0):
        amg.set_patch_seam(seam)
        try:
            mg = amg.Multigrid(*_csc(A), b, 5, smoother=amg.SM_JACOBI, smoother_iters=2, omega=OMEGA,
                               exact_coarse_solve=True)
        finally:
            amg.set_patch_seam(1)
        try:
            assert mg.patch_leg_lines(0, 0) > 0 and mg.patch_leg_lines(1, 0) > 0   # K-Patch levels ...
            assert mg.patch_leg_lines(0, 2) == 0                                   # ... without a seam
            mg.vcycle(3)
            got.append(_levels(mg, 5))
        finally:
            mg.close()
    _assert_same(got[0], got[1], "off")


def test_seam_without_tile_flags(amg, oracle, patch_everywhere):
    amg.set_patch_tile_flags(False)
    try:
        on = _run(amg, oracle, "lap512", 1, [3], expect_seam=True)
    finally:
        amg.set_patch_tile_flags(True)
    _assert_same(on, _oracle_levels(oracle, "lap512", 7)[2], "oracle", skip_coarsest_u=True)


def test_seam_steps_aside_without_the_hand_over(amg, oracle, patch_everywhere):
    amg.set_patch_xf(0)
    try:
        on = _run(amg, oracle, "lap512", 1, [3], expect_seam=False)
    finally:
        amg.set_patch_xf(1)
    _assert_same(on, _oracle_levels(oracle, "lap512", 7)[2], "oracle", skip_coarsest_u=True)


def test_seam_with_tall_legs_off(amg, oracle, patch_everywhere):
    """the legs around the seam launch (head, finish, levels >= 1) on 42-line tiles"""
    amg.set_patch_tall(0)
    try:
        on = _run(amg, oracle, "lap512", 1, [3], expect_seam=True)
    finally:
        amg.set_patch_tall(1)
    _assert_same(on, _oracle_levels(oracle, "lap512", 7)[2], "oracle", skip_coarsest_u=True)


@pytest.mark.parametrize("opt", ["keep_residual", "no_fusion"])
def test_options_that_switch_the_seam_off(amg, oracle, patch_everywhere, opt):
    on = _run(amg, oracle, "lap512", 1, [3], expect_seam=False, **{opt: True})
    off = _run(amg, oracle, "lap512", 0, [3], expect_seam=False, **{opt: True})
    _assert_same(on, off, opt)
    _assert_same(on, _oracle_levels(oracle, "lap512", 7)[2], "oracle", skip_coarsest_u=True)


def _solve(amg, oracle, shape, seam, every, n_iters, tol):
    mg = _solver(amg, oracle, shape, seam, compute_error_every_n_iters=every, n_iters=n_iters, tolerance=tol)
    try:
        u, iters, conv, last = mg.solve()
        return u, iters, conv, last
    finally:
        mg.close()


@pytest.mark.parametrize("every", [1, 2, 3])
def test_solve_runs_the_cycles_between_two_checks_as_one_call(amg, oracle, patch_everywhere, every):
    """n_iters = 7 is no multiple of 2 or 3: same iteration count, last_rss and solution as with the
    switch off -- when the tolerance is never met (7 cycles, the oracle's solution after 7), and when it
    is met at the second check (2 `every` cycles)"""
    u1, it1, conv1, last1 = _solve(amg, oracle, "lap512", 1, every, 7, 1e-300)
    u0, it0, conv0, last0 = _solve(amg, oracle, "lap512", 0, every, 7, 1e-300)
    assert it1 == it0 == 7 and not conv1 and not conv0 and last1 == last0
    assert np.array_equal(u1, u0)
    assert np.array_equal(u1, _oracle_levels(oracle, "lap512", 7)[6][0][0])
    mg = _solver(amg, oracle, "lap512small", 0)
    try:
        mg.vcycle(every)
        rss_first = mg.rss()
        mg.vcycle(every)
        tol = 1.5 * mg.rss()
    finally:
        mg.close()
    assert tol < rss_first and tol < 100.0    # not met at the first check, nor by solve()'s initial 100
    u1, it1, conv1, last1 = _solve(amg, oracle, "lap512small", 1, every, 7, tol)
    u0, it0, conv0, last0 = _solve(amg, oracle, "lap512small", 0, every, 7, tol)
    assert it1 == it0 == 2 * every and conv1 and conv0 and last1 == last0
    assert np.array_equal(u1, u0)


def test_steady_state_bytes_query(amg, oracle, patch_everywhere):
    """part 4 = the stand-alone cycle less the up-leg and the down-leg of level 0 (25 n0 + 8 n1 each) plus
    the seam launch (25 n0 + 16 n1): 25 n0 less; parts 0 and the fine-sweep figures do not move"""
    got = {}
    for seam in (1, 0):
        mg = _solver(amg, oracle, "lap512", seam)
        try:
            n0 = mg.get_n_dofs(0)
            got[seam] = (mg.cycle_must_move(0), mg.cycle_must_move(4), mg.fine_sweep_info())
            mg.vcycle(3)
            assert (mg.cycle_must_move(0), mg.cycle_must_move(4)) == got[seam][:2]
        finally:
            mg.close()
    assert got[1][0] == got[0][0] and got[1][2] == got[0][2]
    assert got[0][1] == got[0][0]
    assert got[1][1] == got[1][0] - 25.0 * n0


def test_slab_and_window_plans_run_as_before(amg, patch_everywhere):
    """the sharded forms run by parts (ranged launches), never through the seam: two slab ranks and two
    windows on 1024^2, switch on and off, against the single-solver cycles (which take the seam)"""
    import torch
    import slab_vcycle
    from test_gpu_slab import _assemble, _cycle
    from test_gpu_window import JAC, _sharded
    n, cycles = 1024, 3
    ref = {}
    for L in (9, 10):
        mg = amg.Multigrid.poisson(n, L, smoother=amg.SM_JACOBI, smoother_iters=2, omega=OMEGA)
        try:
            assert mg.patch_leg_lines(0, 2) == SEAM_LINES
            mg.vcycle(cycles)
            ref[L] = mg.get_soln(0)
        finally:
            mg.close()
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    torch.cuda.set_stream(st)
    for seam in (1, 0):
        amg.set_patch_seam(seam)
        try:
            engs = [slab_vcycle.HipSlabEngine(amg, dev, st, n, 9, OMEGA, 2, r, 2, -1) for r in range(2)]
            try:
                for _ in range(cycles):
                    _cycle(engs, poison=True)
                st.synchronize()
                assert np.array_equal(_assemble(engs), ref[9]), seam
            finally:
                for e in engs:
                    e.close()
            res = _sharded(amg, 2, n, 10, 3, 2, JAC, 2, OMEGA, cycles)
            assert np.array_equal(res[0][0], ref[10]), seam
        finally:
            amg.set_patch_seam(1)
