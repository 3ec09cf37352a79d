"""The cycle plan: one decision per level and leg, read by the enqueue and by every
accessor.  A coarse K-Patch level leaves its solution in its second buffer, as the finer level of a K-Duo
pair does; these tests are the K-Patch counterparts of the two K-Duo accessor tests in
tests/test_gpu_pair_duo.py, on Poisson 512^2, 7 levels, with K-Patch on levels 0 .. 2:
  - get_vec, copy_vec_dev and vec_dev_ptr hand out the same bits on every level, and copy_vec_dev into the
    solver and zero_vec are read back through get_vec;
  - set_vec, one level operation, get_vec give the bits of a solver without a K-Patch level, whose levels
    all rest in u;
  - the K-Duo pairing announced before the first cycle is the one read after it.
Before the plan, the device accessors and level_op knew only the K-Duo case, so the first two failed on
levels 1 and 2."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "algebraic-multigrid_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import test_gpu_patch_seam as S  # noqa: E402

SHAPE = "lap512"
PATCH_LEVELS = (0, 1, 2)


@pytest.fixture
def patch_everywhere(amg):
    amg.set_patch_min_rows(0)          # every level whose band has a 2-D pitch >= 128
    yield
    amg.set_patch_min_rows(amg.PATCH_MIN_ROWS_DEFAULT)


def _solver(amg, oracle, patch, **extra):
    """patch: K-Patch on levels 0 .. 2; else the default threshold, under which this problem has none"""
    amg.set_patch_min_rows(0 if patch else amg.PATCH_MIN_ROWS_DEFAULT)
    try:
        mg = S._solver(amg, oracle, SHAPE, 1, **extra)
    finally:
        amg.set_patch_min_rows(0)      # the fixture's value
    L = S._problem(oracle, SHAPE)[2]
    got = [l for l in range(L) if mg.patch_leg_lines(l, 1) > 0]
    assert got == (list(PATCH_LEVELS) if patch else []), got
    return mg, L


def _dev_copy(mg, level, n):
    """the level's u through amg_hip_copy_vec_dev and through the pointer of amg_hip_vec_dev_ptr"""
    import torch
    from window_vcycle import _DevArray
    buf = torch.empty(n, dtype=torch.float64, device="cuda")
    mg.copy_vec_dev(level, "u", buf.data_ptr(), False)
    mg.sync()
    ptr, m = mg.vec_dev_ptr(level, "u")
    assert m == n
    view = torch.as_tensor(_DevArray(ptr, n), device="cuda")
    return buf.cpu().numpy(), view.cpu().numpy().copy()


def test_patch_device_accessors_follow_the_resting_buffer(amg, oracle, patch_everywhere):
    import torch
    mg, L = _solver(amg, oracle, True)
    try:
        mg.vcycle()
        mg.vcycle()
        bad = []
        for l in range(L):
            n = mg.get_n_dofs(l)
            want = mg.get_soln(l)
            by_copy, by_ptr = _dev_copy(mg, l, n)
            print("level", l, "copy_vec_dev == get_soln:", np.array_equal(by_copy, want),
                  " vec_dev_ptr == get_soln:", np.array_equal(by_ptr, want))
            if not (np.array_equal(by_copy, want) and np.array_equal(by_ptr, want)):
                bad.append(l)
        assert not bad, ("levels whose device accessors disagree with get_soln", bad)
        rng = np.random.default_rng(11)
        for l in range(L):
            n = mg.get_n_dofs(l)
            x = rng.standard_normal(n)
            xd = torch.from_numpy(x).cuda()
            torch.cuda.synchronize()
            mg.copy_vec_dev(l, "u", xd.data_ptr(), True)
            mg.sync()
            assert np.array_equal(mg.get_soln(l), x), (l, "copy in")
            mg.zero_vec(l, "u")
            mg.sync()
            assert not mg.get_soln(l).any(), (l, "zero")
    finally:
        mg.close()


def test_patch_level_ops_work_on_the_resting_buffer(amg, oracle, patch_everywhere):
    got = {}
    for patch in (True, False):
        mg, L = _solver(amg, oracle, patch, keep_residual=True)
        try:
            mg.vcycle()
            rng = np.random.default_rng(7)
            out = []
            for l in PATCH_LEVELS:
                n, nc = mg.get_n_dofs(l), mg.get_n_dofs(l + 1)
                for op in (0, 1, 2, 3):
                    mg.set_vec(l, "u", rng.standard_normal(n))
                    mg.set_vec(l, "f", rng.standard_normal(n))
                    mg.set_vec(l + 1, "u", rng.standard_normal(nc))
                    mg.level_op(l, op)
                    mg.sync()
                    out.append((l, op, mg.get_soln(l), mg.get_residual(l), mg.get_soln(l + 1), mg.get_rhs(l + 1)))
            got[patch] = out
        finally:
            mg.close()
    bad = []
    for a, b in zip(got[True], got[False]):
        assert a[:2] == b[:2]
        for k, name in zip(range(2, 6), ("u", "r", "u_coarse", "f_coarse")):
            same = np.array_equal(a[k], b[k])
            print("level", a[0], "op", a[1], name, "same" if same else "DIFFERENT")
            if not same:
                bad.append((a[0], a[1], name))
    assert not bad, ("(level, op, vector) that differ from the solver without a K-Patch level", bad)


def test_pairing_announced_before_the_first_cycle(amg, oracle, patch_everywhere):
    """K-Patch on levels 0 .. 2 above the duo (4, 5), vcycle(3) through the seam"""
    mg, L = _solver(amg, oracle, True)
    try:
        before = [mg.pair_duo_partner(l) for l in range(L)]
        mg.vcycle(3)
        after = [mg.pair_duo_partner(l) for l in range(L)]
    finally:
        mg.close()
    want = [-1] * L
    want[4], want[5] = 5, 4
    assert before == after == want, (before, after)
