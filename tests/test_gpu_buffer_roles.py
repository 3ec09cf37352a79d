"""Buffer roles belong to the cycle plan: no cycle and no level operation moves a level's vectors.

K-March used to trade u and tmp of a level while the cycle was enqueued, and the level operations traded
them for the length of a call; both now read the roles from the plan.  What must hold from outside:
  the device pointers of u, f and r of every level are the same before and after every cycle and every
  level operation (eager and from the graph), and the u pointer is where get_soln reads;
  a level operation on and around a coarse K-Patch level (which rests in its second buffer) gives the
  bits of the solver without K-Patch levels there (which rests in u)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "algebraic-multigrid_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import test_gpu_pair_duo as D  # noqa: E402
import test_gpu_pair_onchip as P  # noqa: E402
import test_gpu_patch_seam as S  # noqa: E402
import test_gpu_stencil_geometry as G  # noqa: E402


def _patch_solver(amg, oracle, min_rows, **extra):
    """lap512 of tests/test_gpu_patch_seam.py; min_rows = 0: levels 0 .. 2 are K-Patch levels"""
    amg.set_patch_min_rows(min_rows)
    try:
        return S._solver(amg, oracle, "lap512", 1, **extra)
    finally:
        amg.set_patch_min_rows(amg.PATCH_MIN_ROWS_DEFAULT)


def _march_solver(amg, shape, levels, **extra):
    op = G.box3d(*shape)
    n = op[0].size - 1
    return amg.Multigrid(*op, G.rhs_for(n), levels or G.levels_for(n), smoother=amg.SM_JACOBI, smoother_iters=2,
                         omega=0.6, layout=amg.LAYOUT_DICT, exact_coarse_solve=True, **extra)


SOLVERS = {
    # the finer level of every duo rests in tmp
    "lap256_duo": lambda amg, oracle, **kw: P._solver(amg, oracle, "lap256", False, **kw),
    # coarse K-Patch levels rest in tmp; vcycle(3) runs the seam sequence
    "lap512_patch": lambda amg, oracle, **kw: _patch_solver(amg, oracle, 0, **kw),
    # K-March on both legs of level 0
    "march64x16x3": lambda amg, oracle, **kw: _march_solver(amg, G.MARCH_SHAPES[0], 0, **kw),
    # K-March on the down-leg alone, then the copy home
    "march64x16x4_single": lambda amg, oracle, **kw: _march_solver(amg, (64, 16, 4), 1, keep_residual=True, **kw),
}


def _pointers(mg, L):
    return [tuple(mg.vec_dev_ptr(l, w)[0] for w in "ufr") for l in range(L)]


def _u_is_where_get_soln_reads(mg, L, tag):
    """bit for bit (before the first cycle a second buffer holds whatever the allocation left there)"""
    for l in range(L):
        want = mg.get_soln(l).view(np.uint64)
        by_copy, by_ptr = D._dev_copy(mg, l, mg.get_n_dofs(l))
        assert np.array_equal(by_copy.view(np.uint64), want) and np.array_equal(by_ptr.view(np.uint64), want), (tag, l)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("name", list(SOLVERS))
def test_pointers_do_not_move(amg, oracle, name, use_graph):
    """vec_dev_ptr of u, f, r on every level: before the first cycle, after vcycle(), after vcycle(3),
    after every level operation.  All records are equal (a level the plan rests in tmp -- a coarse
    K-Patch level, the finer level of a duo -- hands out tmp from the start, because the accessors
    answer from the plan the first cycle will run), and at every point u is the buffer get_soln reads."""
    mg = SOLVERS[name](amg, oracle, use_graph=use_graph)
    try:
        L = mg.n_levels
        if name.startswith("march"):
            assert mg.fine_sweep_info()[0] == "march_kernel"
        before = _pointers(mg, L)
        _u_is_where_get_soln_reads(mg, L, "before")
        mg.vcycle()
        mg.sync()
        first = _pointers(mg, L)
        _u_is_where_get_soln_reads(mg, L, "vcycle()")
        # (before the first cycle the accessors answer from the plan that cycle runs: nothing may differ)
        assert before == first, "vcycle()"
        mg.vcycle(3)
        mg.sync()
        assert _pointers(mg, L) == first, "vcycle(3)"
        if name == "lap512_patch":  # it ran as head, two seam cycles and finish, which move less than three cycles
            assert mg.patch_leg_lines(0, 2) == S.SEAM_LINES
            assert mg.cycle_must_move(4) < mg.cycle_must_move(0)
        _u_is_where_get_soln_reads(mg, L, "vcycle(3)")
        for l in range(L):
            for op in ((0, 1, 2, 3) if l + 1 < L else (4,)):
                mg.level_op(l, op)
                mg.sync()
                assert _pointers(mg, L) == first, ("level_op", l, op)
        _u_is_where_get_soln_reads(mg, L, "level ops")
        mg.vcycle()
        mg.sync()
        assert _pointers(mg, L) == first, "a cycle after the level operations"
    finally:
        mg.close()


def test_level_ops_on_a_coarse_patch_level(amg, oracle):
    """set_vec, one level operation, get_vec on the last K-Patch level l >= 1 of lap512 and on levels
    l - 1 and l + 1: smoothing, residual, restriction (which zeroes the coarser u) and prolongation give
    the bits of the solver made with patch_min_rows at its default, which has no K-Patch level there and
    rests everywhere in u (the scheme of test_duo_level_ops_work_on_the_resting_buffer)."""
    got = {}
    for min_rows in (0, amg.PATCH_MIN_ROWS_DEFAULT):
        mg = _patch_solver(amg, oracle, min_rows, keep_residual=True)
        try:
            L = mg.n_levels
            mg.vcycle()
            patch = [l for l in range(1, L) if mg.leg_form(l)[0] == "patch"]
            if min_rows:
                assert not patch
            else:
                assert patch and patch[-1] + 2 < L
                levels = (patch[-1] - 1, patch[-1], patch[-1] + 1)
            rng = np.random.default_rng(7)
            out = []
            for l in levels:
                n, nc = mg.get_n_dofs(l), mg.get_n_dofs(l + 1)
                for op in (0, 1, 2, 3):
                    mg.set_vec(l, "u", rng.standard_normal(n))
                    mg.set_vec(l, "f", rng.standard_normal(n))
                    mg.set_vec(l + 1, "u", rng.standard_normal(nc))
                    mg.level_op(l, op)
                    mg.sync()
                    out.append((l, op, mg.get_soln(l), mg.get_residual(l), mg.get_soln(l + 1), mg.get_rhs(l + 1)))
            got[min_rows] = out
        finally:
            mg.close()
    for a, b in zip(got[0], got[amg.PATCH_MIN_ROWS_DEFAULT]):
        assert a[:2] == b[:2]
        for k in range(2, 6):
            assert np.array_equal(a[k], b[k]), ("level", a[0], "op", a[1], "vector", k)
