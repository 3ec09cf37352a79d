"""K-Duo (dict_duo_down_kernel / dict_duo_up_kernel): two consecutive pair levels (l, l+1) run their
down-legs as one launch and their up-legs as one.  Same row arithmetic and the same transfer
expressions as the four pair launches, so the bar is bitwise: u, f and r of every level after each of
three cycles against the oracle twin, against the same solver with the switch off and against
no_fusion, on the three problems of tests/test_gpu_pair_onchip.py:
  laplacian(256), 9 levels   duos (2,3), (4,5), (6,7): half-bandwidths 65 over 33 (the windows at their
                             capacity) down to 5 over 3, rows of two code words over rows of one; level
                             6 has three tiles, the last with three rows and one coarse row
  box2d(300, 50), 7 levels   duo (3,4), level 5 single: ragged lines, several row types per wave, tiles
                             whose first coarse row is odd
  zero-diagonal box, 5 lvls  duo (1,2), level 3 single: the first sweep of level 2, formed in LDS, meets
                             d == 0; rows of one code word over rows of two
The finer level of a duo rests in its second buffer and is read through the normal getter."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "algebraic-multigrid_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import test_gpu_pair_onchip as P  # noqa: E402
import test_gpu_patch_seam as S  # noqa: E402

DUOS = {"lap256": ((2, 3), (4, 5), (6, 7)), "box300x50": ((3, 4),), "zerodiag128x50": ((1, 2),)}
SHAPES = tuple(DUOS)


def _partners(shape_levels, duos):
    want = [-1] * shape_levels
    for a, b in duos:
        want[a], want[b] = b, a
    return want


def _run(amg, oracle, shape, keep, duo, **extra):
    """u, f, r of every level after each cycle, the duo partner of every level, cycle_must_move()"""
    L = P.LEVELS[shape]
    amg.set_pair_duo(duo)
    try:
        mg = P._solver(amg, oracle, shape, keep, **extra)
    finally:
        amg.set_pair_duo(1)
    try:
        before = [mg.pair_duo_partner(l) for l in range(L)]
        out = []
        for _ in range(P.CYCLES):
            mg.vcycle()
            out.append([(mg.get_soln(l), mg.get_rhs(l), mg.get_residual(l) if keep else None) for l in range(L)])
        partner = [mg.pair_duo_partner(l) for l in range(L)]
        assert partner == before, "the pairing a cycle runs is the one announced before it"
        return out, partner, mg.cycle_must_move()
    finally:
        mg.close()


def _check(amg, oracle, shape, keep):
    _, ref = P._oracle_twin(oracle, shape)
    L = P.LEVELS[shape]
    on, partner, mm_on = _run(amg, oracle, shape, keep, 1)
    assert partner == _partners(L, DUOS[shape]), (shape, partner)
    P._assert_same(on, ref, (shape, "oracle"), skip_coarsest_u=not keep)
    off, partner_off, mm_off = _run(amg, oracle, shape, keep, 0)
    assert partner_off == [-1] * L
    P._assert_same(on, off, (shape, "switch off"))
    assert mm_on == mm_off, "a duo accounts what the pair launches of its two levels would have moved"
    plain, partner_plain, _ = _run(amg, oracle, shape, keep, 1, no_fusion=True)
    assert partner_plain == [-1] * L
    P._assert_same(on, plain, (shape, "no_fusion"))


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_duo_bitwise(amg, oracle, shape, keep):
    _check(amg, oracle, shape, keep)


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_duo_code_words_bitwise(amg, oracle, shape, keep):
    """row types off: the code words of the windows of both levels are staged"""
    amg.set_row_types(False)
    try:
        _check(amg, oracle, shape, keep)
    finally:
        amg.set_row_types(True)


@pytest.mark.parametrize("shape", SHAPES)
def test_duo_graph_and_eager_bitwise(amg, oracle, shape):
    graph, pg, _ = _run(amg, oracle, shape, True, 1)
    eager, pe, _ = _run(amg, oracle, shape, True, 1, use_graph=False)
    assert pg == pe == _partners(P.LEVELS[shape], DUOS[shape])
    P._assert_same(graph, eager, (shape, "graph/eager"))


def test_duo_one_row_per_lane_runs_no_duo(amg, oracle):
    """set_dict_rows(1): no level is a pair level, so none is paired"""
    amg.set_dict_rows(1)
    try:
        _, partner, _ = _run(amg, oracle, "box300x50", False, 1)
    finally:
        amg.set_dict_rows(2)
    assert partner == [-1] * P.LEVELS["box300x50"]


def test_duo_beside_tail_fusion(amg, oracle):
    """Poisson 512^2, 10 levels, with K-Tail on: the levels K-Tail takes are not paired, a duo above
    them hands over to it, and every level vector has the bits of the run without either"""
    n, L = 512, 10
    kw = dict(smoother=amg.SM_JACOBI, smoother_iters=2, omega=0.6)
    runs = {}
    for name, duo, tail in (("plain", 0, 0), ("duo", 1, 0), ("duo+tail", 1, 1)):
        amg.set_pair_duo(duo)
        amg.set_tail_fusion(tail)
        try:
            mg = amg.Multigrid.poisson(n, L, **kw)
            try:
                rows = [mg.get_n_dofs(l) for l in range(L)]
                chain = int(amg.lib().amg_hip_coarse_solve_kind(mg._h)) == 3
                mg.vcycle(3)
                mg.sync()
                partner = [mg.pair_duo_partner(l) for l in range(L)]
                runs[name] = ([mg.get_soln(l) for l in range(L)], [mg.get_rhs(l) for l in range(L)], partner)
            finally:
                mg.close()
        finally:
            amg.set_pair_duo(1)
            amg.set_tail_fusion(0)
    assert runs["plain"][2] == [-1] * L
    # pair levels: half-bandwidth <= 65, i.e. levels 3 .. 8; greedy from the finest
    assert runs["duo"][2] == _partners(L, ((3, 4), (5, 6), (7, 8))), runs["duo"][2]
    pt = runs["duo+tail"][2]
    assert all(p == -1 or p == q for p, q in zip(pt, runs["duo"][2])), "K-Tail only takes duos away"
    # K-Tail runs on this solver (its solve is K-BandChain's) and takes the deepest levels of at most 4095 rows
    assert chain and rows[L - 2] <= 4095 and pt[L - 2] == -1, (chain, pt)
    assert pt[3] == 4 and pt[4] == 3, pt
    for name in ("duo", "duo+tail"):
        for l in range(L):
            assert np.array_equal(runs[name][0][l], runs["plain"][0][l]), (name, "u", l)
            assert np.array_equal(runs[name][1][l], runs["plain"][1][l]), (name, "f", l)


@pytest.fixture
def patch_everywhere(amg):
    amg.set_patch_min_rows(0)
    yield
    amg.set_patch_min_rows(amg.PATCH_MIN_ROWS_DEFAULT)


def test_duo_under_the_patch_seam(amg, oracle, patch_everywhere):
    """Poisson 512^2, 7 levels, K-Patch on levels 0 .. 2 and vcycle(3) through the seam: level 3 prolongs
    into a K-Patch level and stays single, levels (4,5) are a duo; against the switch off"""
    L = S._problem(oracle, "lap512")[2]
    got = {}
    for duo in (1, 0):
        amg.set_pair_duo(duo)
        try:
            mg = S._solver(amg, oracle, "lap512", 1)
        finally:
            amg.set_pair_duo(1)
        try:
            assert mg.patch_leg_lines(0, 2) == S.SEAM_LINES
            mg.vcycle(3)
            got[duo] = (S._levels(mg, L), [mg.pair_duo_partner(l) for l in range(L)])
        finally:
            mg.close()
    assert got[1][1] == _partners(L, ((4, 5),)) and got[0][1] == [-1] * L, (got[1][1], got[0][1])
    S._assert_same(got[1][0], got[0][0], "switch off")


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


@pytest.mark.parametrize("shape", ["lap256", "zerodiag128x50"])
def test_duo_device_accessors_follow_the_resting_buffer(amg, oracle, shape):
    """after a cycle, copy_vec_dev and vec_dev_ptr hand out what get_vec does on every level (the finer
    level of a duo rests in its second buffer); copy_vec_dev into the solver and zero_vec are read back
    through get_vec"""
    import torch
    L = P.LEVELS[shape]
    mg = P._solver(amg, oracle, shape, False)
    try:
        mg.vcycle()
        mg.vcycle()
        rng = np.random.default_rng(11)
        for l in range(L):
            n = mg.get_n_dofs(l)
            want = mg.get_soln(l)
            by_copy, by_ptr = _dev_copy(mg, l, n)
            assert np.array_equal(by_copy, want) and np.array_equal(by_ptr, want), (shape, l)
        for l in sorted({a for a, _ in DUOS[shape]} | {b for _, b in DUOS[shape]}):
            n = mg.get_n_dofs(l)
            x = rng.standard_normal(n)
            xd = torch.from_numpy(x).cuda()
            torch.cuda.synchronize()
            mg.copy_vec_dev(l, "u", xd.data_ptr(), True)
            mg.sync()
            assert np.array_equal(mg.get_soln(l), x), (shape, l, "copy in")
            mg.zero_vec(l, "u")
            mg.sync()
            assert not mg.get_soln(l).any(), (shape, l, "zero")
    finally:
        mg.close()


@pytest.mark.parametrize("shape", ["lap256", "zerodiag128x50"])
def test_duo_level_ops_work_on_the_resting_buffer(amg, oracle, shape):
    """set_vec, one level operation, get_vec on and around the levels of a duo: smoothing, residual,
    restriction (which zeroes the coarser u) and prolongation give the bits of the solver with the switch
    off, whose levels all rest in u"""
    L = P.LEVELS[shape]
    first = DUOS[shape][0][0]
    levels = [l for l in (first - 1, first, first + 1) if l >= 0]
    got = {}
    for duo in (1, 0):
        amg.set_pair_duo(duo)
        try:
            mg = P._solver(amg, oracle, shape, True)
        finally:
            amg.set_pair_duo(1)
        try:
            assert mg.pair_duo_partner(first) == (first + 1 if duo else -1)
            mg.vcycle()
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
            got[duo] = out
        finally:
            mg.close()
    for a, b in zip(got[1], got[0]):
        assert a[:2] == b[:2]
        for k in range(2, 6):
            assert np.array_equal(a[k], b[k]), (shape, "level", a[0], "op", a[1], "vector", k)
