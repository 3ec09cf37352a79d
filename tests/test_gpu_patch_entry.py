"""K-Patch prologue: a workgroup issues every load of its tile at entry -- before its tile flag is
known, so with the clamped rows of the general path -- reads the flag as a byte of an aligned
32-bit word through a scalar load, waits for f only inside the first stage, and stages the
per-lane tables only where a wave can read them.  Nothing of this may change a bit: every test runs
2 cycles and compares every level vector with the oracle twin and with the unfused kernels
(no_fusion).

The 384 x 100 box has 18 tiles on level 0 and 9 on level 1 (6 and 3 tile columns, 3 tile rows
for both the 42- and the 44-line tiles): the flag bytes sit at every position of a word and the
last word is partial; its tiles touch all four edges of the matrix, so the early loads run on
clamped rows."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "algebraic-multigrid_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import test_gpu_patch_xf as XF  # noqa: E402  (the boxes are built the way that file builds its own)

OMEGA = XF.OMEGA
CYCLES = 2
patch_everywhere = XF.patch_everywhere


def _problem(oracle, shape):
    """(A, b, levels)"""
    if shape == "box384x100":      # pitches 384, 192 are K-Patch levels; 96 is too narrow
        A = XF.box2d(oracle, 384, 100)
        return A, np.sin(0.001 * np.arange(A.rows)) + 1.5, 6
    if shape == "nodiag256x50":    # the XF test's box: rows without a diagonal
        return XF._problem(oracle, shape)[:3]
    assert shape == "lap512"       # pitches 512, 256, 128
    return oracle.laplacian(512), oracle.rhs(512), 7


_REF = {}


def _oracle_levels(oracle, shape):
    """u, f, r of every level after CYCLES cycles of the true-Jacobi oracle twin; once per shape"""
    if ("oracle", shape) not in _REF:
        A, b, L = _problem(oracle, shape)
        ref = oracle.Multigrid(A, b, L, smoother=oracle.SM_TRUE_JACOBI, smoother_iters=2, omega=OMEGA)
        for _ in range(CYCLES):
            ref.vcycle()
        _REF["oracle", shape] = [(ref.get_vec(l, "u"), ref.get_vec(l, "f"), ref.get_vec(l, "r")) for l in range(L)]
    return _REF["oracle", shape]


def _jacobi_levels(amg, oracle, shape, keep, **extra):
    A, b, L = _problem(oracle, shape)
    mg = amg.Multigrid(A.colptr, A.rowind, A.val, b, L, smoother=amg.SM_JACOBI, smoother_iters=2, omega=OMEGA,
                       keep_residual=keep, exact_coarse_solve=True, **extra)
    try:
        assert mg.fine_sweep_info()[0].startswith("patch_down_kernel") != bool(extra.get("no_fusion"))
        mg.vcycle(CYCLES)
        return [(mg.get_soln(l), mg.get_rhs(l), mg.get_residual(l) if keep else None) for l in range(L)]
    finally:
        mg.close()


def _unfused_levels(amg, oracle, shape, keep):
    """the same cycles by the unfused kernels (no K-Patch launch); once per shape and keep"""
    if ("unfused", shape, keep) not in _REF:
        _REF["unfused", shape, keep] = _jacobi_levels(amg, oracle, shape, keep, no_fusion=True)
    return _REF["unfused", shape, keep]


def _assert_levels(got, oracle_lv, unfused_lv, keep, tag):
    L = len(got)
    for l in range(L):
        for name, p, q, o in zip("ufr", got[l], unfused_lv[l], oracle_lv[l]):
            if p is None:
                continue
            assert np.array_equal(p, q), (tag, "no_fusion", l, name)
            if name == "u" and l == L - 1 and not keep:
                continue               # the coarsest level's u is the direct solve either way
            assert np.array_equal(p, o), (tag, "oracle", l, name)


def _check(amg, oracle, shape, keep, tag, **extra):
    got = _jacobi_levels(amg, oracle, shape, keep, **extra)
    _assert_levels(got, _oracle_levels(oracle, shape), _unfused_levels(amg, oracle, shape, keep), keep, tag)
    return got


def test_entry_box(amg, oracle, patch_everywhere):
    _check(amg, oracle, "box384x100", False, "box")


def test_entry_box_without_tile_flags(amg, oracle, patch_everywhere):
    """null flag pointers: every tile takes the path with row-type loads and staged tables"""
    amg.set_patch_tile_flags(False)
    try:
        _check(amg, oracle, "box384x100", False, "no flags")
    finally:
        amg.set_patch_tile_flags(True)


def test_entry_box_graph_and_eager(amg, oracle, patch_everywhere):
    a = _check(amg, oracle, "box384x100", False, "graph", use_graph=True)
    b = _check(amg, oracle, "box384x100", False, "eager", use_graph=False)
    for l, (x, y) in enumerate(zip(a, b)):
        for p, q in zip(x[:2], y[:2]):
            assert np.array_equal(p, q), l


def test_entry_box_keep_residual(amg, oracle, patch_everywhere):
    _check(amg, oracle, "box384x100", True, "keep_residual")


def test_entry_box_without_diagonal_rows(amg, oracle, patch_everywhere):
    """256 x 50 with rows that have no diagonal: they take the branch of the sweep that never reads
    f, so the deferred wait for f is not reached on that path"""
    for keep in (False, True):
        _check(amg, oracle, "nodiag256x50", keep, "no diagonal")


class _BoxSlabEngine:
    """slab_vcycle.HipSlabEngine for a solver of a user matrix (that class builds Poisson solvers)"""

    def __init__(self, amg, torch, slab_vcycle, dev, st, A, b, L, rank, world):
        self.mg = amg.Multigrid(A.colptr, A.rowind, A.val, b, L, smoother=amg.SM_JACOBI, smoother_iters=2,
                                omega=OMEGA, exact_coarse_solve=True, device=dev.index, stream=st.cuda_stream)
        try:
            self.info = i = self.mg.slab_setup(rank, world, -1)
        except Exception:
            self.mg.close()
            raise
        cap = int(i.chunk_lines) * world
        self.u0 = torch.as_tensor(slab_vcycle._DevArray(i.u0, cap * int(i.pitch0)), device=dev)
        self.fg = torch.as_tensor(slab_vcycle._DevArray(i.f_gather, cap * int(i.gather_pitch)), device=dev)

    def run(self, part):
        self.mg.slab_run(part)

    def close(self):
        self.u0 = self.fg = None
        self.mg.close()


@pytest.mark.parametrize("world", [2, 3])
def test_entry_box_slab_line_ranges(amg, oracle, patch_everywhere, world):
    """The box cut into line ranges, slab form on one GPU: the launches of the later ranges start at
    a tile row py0 != 0, which enters the flag index (two ranges: the up-legs; three: the down-legs
    too).  What a sharded cycle leaves assembled is level 0's u: compared with the oracle's and the
    unfused kernels'."""
    import torch
    import slab_vcycle
    from test_gpu_slab import _assemble, _cycle
    A, b, L = _problem(oracle, "box384x100")
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    torch.cuda.set_stream(st)
    engs = []
    try:
        for r in range(world):
            engs.append(_BoxSlabEngine(amg, torch, slab_vcycle, dev, st, A, b, L, r, world))
        last = engs[-1].info
        assert int(last.levels) == 2                     # levels 0 and 1 are K-Patch levels
        assert int(last.up_lo[0]) // 44 >= 1 and int(last.up_lo[1]) // 44 >= 1
        assert world < 3 or (int(last.down_lo[0]) // 42 >= 1 and int(last.down_lo[1]) // 44 >= 1)
        for _ in range(CYCLES):
            _cycle(engs, poison=True)
        st.synchronize()
        u = _assemble(engs)
    finally:
        for e in engs:
            e.close()
    assert np.array_equal(u, _oracle_levels(oracle, "box384x100")[0][0])
    assert np.array_equal(u, _unfused_levels(amg, oracle, "box384x100", False)[0][0])


def test_entry_multicolor_512(amg, oracle, patch_everywhere):
    """512^2, multicolour smoother: patch_rb_kernel shares the prologue"""
    A, b, L = _problem(oracle, "lap512")
    got = {}
    for nf in (False, True):
        mg = amg.Multigrid(A.colptr, A.rowind, A.val, b, L, smoother=amg.SM_MULTICOLOR_GS, smoother_iters=1,
                           exact_coarse_solve=True, keep_residual=True, no_fusion=nf)
        try:
            assert mg.fine_sweep_info()[0].startswith("patch_rb_kernel") != nf
            if not nf:
                colors = [mg.get_colors(l) for l in range(L)]
            mg.vcycle(CYCLES)
            got[nf] = [(mg.get_soln(l), mg.get_rhs(l), mg.get_residual(l)) for l in range(L)]
        finally:
            mg.close()
    ref = oracle.Multigrid(A, b, L, smoother=oracle.SM_MULTICOLOR, smoother_iters=1)
    for l, (col, nc) in enumerate(colors):
        ref.set_colors(l, col, nc)
    for _ in range(CYCLES):
        ref.vcycle()
    ref_lv = [(ref.get_vec(l, "u"), ref.get_vec(l, "f"), ref.get_vec(l, "r")) for l in range(L)]
    _assert_levels(got[False], ref_lv, got[True], False, "multicolour")
