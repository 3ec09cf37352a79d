"""K-Patch tall legs (amg_hip_set_patch_tall): the Jacobi legs that run two dependent stencil stages
on the data they load -- every up-leg, the down-legs of the levels >= 1 -- use tiles of 44 lines with
two halo rings instead of 42 with three.  Every output row is computed by the expressions that
computed it before, only by another workgroup, so the bar is bitwise everywhere: switch on against
switch off and against the oracle twin on every level vector, on shapes whose last tile row is
ragged, which have several row types and rows without a diagonal, and on the smallest line counts
at which the new cut differs (one tall tile row exactly, one line more, two rows, two and a line);
under graph replay, combined with the other K-Patch switches, and over the line ranges of the slab
and window forms.  amg_hip_patch_leg_lines proves which geometry ran."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "algebraic-multigrid_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import test_gpu_patch_xf as XF                                     # noqa: E402
from test_gpu_patch_xf import OMEGA, patch_everywhere, box2d      # noqa: E402,F401

BIG = ["lap512", "box1024x300", "nodiag256x50"]       # 13 / 12, 8 / 7 and 2 / 2 tile rows of 42 / 44 lines
SMALL = ["box256x44", "box256x45", "box256x88", "box256x89"]
SHAPES = BIG + SMALL


def _problem(oracle, shape):
    """(A, b, levels, index of the first level that is no K-Patch level)"""
    if shape in BIG:
        return XF._problem(oracle, shape)
    A = box2d(oracle, 256, int(shape[len("box256x"):]))   # pitches 256 and 128 are K-Patch levels
    return A, np.sin(0.001 * np.arange(A.rows)) + 1.5, 4, 2


_ORACLE = {}


def _oracle_levels(oracle, shape, cycles=3):
    """u, f, r of every level after each cycle of the oracle twin; computed once per shape"""
    if shape in BIG:
        return XF._oracle_levels(oracle, shape, cycles)
    if shape not in _ORACLE:
        A, b, L, _ = _problem(oracle, shape)
        ref = oracle.Multigrid(A, b, L, smoother=oracle.SM_TRUE_JACOBI, smoother_iters=2, omega=OMEGA)
        out = []
        for _ in range(cycles):
            ref.vcycle()
            out.append([(ref.get_vec(l, "u"), ref.get_vec(l, "f"), ref.get_vec(l, "r")) for l in range(L)])
        _ORACLE[shape] = (out, ref.rss())
    return _ORACLE[shape]


def _solver(amg, oracle, shape, tall, keep, xf=1, flags=True, **extra):
    A, b, L, _ = _problem(oracle, shape)
    amg.set_patch_tall(tall)
    amg.set_patch_xf(xf)
    amg.set_patch_tile_flags(flags)
    try:
        return amg.Multigrid(*XF._csc(A), b, L, smoother=amg.SM_JACOBI, smoother_iters=2, omega=OMEGA,
                             keep_residual=keep, exact_coarse_solve=True, **extra)
    finally:
        amg.set_patch_tall(1)
        amg.set_patch_xf(1)


def _run(amg, oracle, shape, u0=None, cycles=3, **kw):
    """(level vectors, rss, must-move bytes) after `cycles` cycles; the tile-flag switch is read at
    launch, so it stays as set until the cycles have run"""
    _, _, L, _ = _problem(oracle, shape)
    try:
        mg = _solver(amg, oracle, shape, kw.pop("tall", 1), True, **kw)
        try:
            if u0 is not None:
                mg.set_vec(0, "u", u0)
            mg.vcycle(cycles)
            return XF._levels(mg, L, True), mg.rss(), mg.cycle_must_move()
        finally:
            mg.close()
    finally:
        amg.set_patch_tile_flags(True)


_DEFAULT = {}


def _default_run(amg, oracle, shape):
    """the all-default run (tall on) from the shape's random start; computed once per shape"""
    if shape not in _DEFAULT:
        A = _problem(oracle, shape)[0]
        _DEFAULT[shape] = _run(amg, oracle, shape, u0=np.random.default_rng(11).standard_normal(A.rows))
    return _DEFAULT[shape]


@pytest.mark.parametrize("shape", SHAPES)
def test_tall_on_off_bitwise(amg, oracle, patch_everywhere, shape):
    """3 cycles from a random non-zero start, residual kept: u, f, r of every level and rss() equal
    with the switch on and off"""
    A = _problem(oracle, shape)[0]
    on = _default_run(amg, oracle, shape)
    off = _run(amg, oracle, shape, u0=np.random.default_rng(11).standard_normal(A.rows), tall=0)
    XF._assert_same(on[0], off[0], shape)
    assert on[1] == off[1]
    assert on[2] == off[2]


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_tall_against_oracle(amg, oracle, patch_everywhere, shape, keep):
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


@pytest.mark.parametrize("shape", ["lap512", "box256x45"])
def test_tall_path_ran(amg, oracle, patch_everywhere, shape):
    """on: 42 lines for the level-0 down-leg, 44 for its up-leg and both legs of every other K-Patch
    level, 0 on the other levels; off: 42 on every K-Patch leg.  The bytes a cycle has to move do not
    depend on the tile height."""
    _, _, L, npatch = _problem(oracle, shape)
    mm = {}
    for tall in (1, 0):
        mg = _solver(amg, oracle, shape, tall, False)
        try:
            for l in range(L):
                want = (0, 0) if l >= npatch else ((42, 42) if not tall else ((42, 44) if l == 0 else (44, 44)))
                assert (mg.patch_leg_lines(l, 0), mg.patch_leg_lines(l, 1)) == want, (tall, l)
            assert mg.patch_leg_lines(L, 0) == 0 and mg.patch_leg_lines(-1, 1) == 0
            mm[tall] = mg.cycle_must_move()
        finally:
            mg.close()
    assert mm[1] == mm[0] and mm[1] > 0.0


def test_tall_graph_and_eager_bitwise(amg, oracle, patch_everywhere):
    got = []
    for use_graph in (True, False):
        mg = _solver(amg, oracle, "lap512", 1, True, use_graph=use_graph)
        try:
            mg.vcycle(3)
            got.append((XF._levels(mg, 7, True), mg.rss()))
        finally:
            mg.close()
    XF._assert_same(got[0][0], got[1][0], "graph/eager")
    assert got[0][1] == got[1][1]


@pytest.mark.parametrize("shape", ["lap512", "nodiag256x50", "box256x89"])
@pytest.mark.parametrize("combo", ["xf_off", "flags_off"])
def test_tall_with_other_switches(amg, oracle, patch_everywhere, shape, combo):
    """tall legs with the stored-form down-legs (XF off: two-ring legs too) and without the per-tile
    flags (every workgroup on the general path), each against the all-default run"""
    A = _problem(oracle, shape)[0]
    kw = {"xf": 0} if combo == "xf_off" else {"flags": False}
    ref = _default_run(amg, oracle, shape)
    got = _run(amg, oracle, shape, u0=np.random.default_rng(11).standard_normal(A.rows), **kw)
    XF._assert_same(got[0], ref[0], (shape, combo))
    assert got[1] == ref[1]


# ---- ranged launches: the down- and the up-leg of a level round a line range to different tiles ----
@pytest.mark.parametrize("max_levels", [-1, 2])
def test_tall_slab_two_ranks_on_off(amg, patch_everywhere, max_levels):
    """slab_setup(rank, 2) on 1024^2 / 9 levels (the slab tests' shape), switch on and off, against
    the single-solver cycle; max_levels = 2 cuts between two K-Patch levels"""
    import torch
    import slab_vcycle
    from test_gpu_slab import _assemble, _cycle
    n, L, cycles = 1024, 9, 3
    u_ref = XF._single_poisson(amg, n, L, cycles)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    torch.cuda.set_stream(st)
    for tall in (1, 0):
        amg.set_patch_tall(tall)
        try:
            engs = [slab_vcycle.HipSlabEngine(amg, dev, st, n, L, OMEGA, 2, r, 2, max_levels) for r in range(2)]
        finally:
            amg.set_patch_tall(1)
        try:
            assert int(engs[0].info.levels) == (4 if max_levels < 0 else max_levels)
            for _ in range(cycles):
                _cycle(engs, poison=True)
            st.synchronize()
            assert np.array_equal(_assemble(engs), u_ref), tall
        finally:
            for e in engs:
                e.close()


def test_tall_window_two_ranks_on_off(amg, patch_everywhere):
    """two windows of 1024^2 with three window levels (the window tests' shape), switch on and off"""
    from test_gpu_window import JAC, _sharded
    n, L, k, cycles = 1024, 10, 3, 3
    u_ref = XF._single_poisson(amg, n, L, cycles)
    for tall in (1, 0):
        amg.set_patch_tall(tall)
        try:
            res = _sharded(amg, 2, n, L, k, 2, JAC, 2, OMEGA, cycles)
        finally:
            amg.set_patch_tall(1)
        assert np.array_equal(res[0][0], u_ref), tall
