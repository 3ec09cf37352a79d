"""K-Patch column-typed tiles (amg_hip_set_patch_coltype): a tile whose held rows all lie inside the
matrix and whose every held column has one row type over all held lines -- the tiles at the two ends
of the grid lines -- gets the tile flag 254 at set-up and is evaluated with a sliding 3 x 3 window and
the weights of the lane's type (patch_eval_c) instead of the per-entry tables.  Nothing of this may
change a bit: after 2 cycles every level vector equals the oracle twin's, the unfused kernels'
(no_fusion) and the same solver's with the switch off.

amg_hip_patch_tile_classes counts the tiles by class; the expected counts are derived here, in numpy,
from the oracle's level matrices (a row type = its (offset, value) pattern, exact zeros pruned).

Shapes: lap512 (pitches 512 / 256 / 128; at pitch 128 every tile is an edge tile); the 256 x 50 box
with single rows without a diagonal (two tile rows, both at the matrix edge: no column-typed tile, and a
single such row breaks its column's type anyway); a 256 x 150 box in which two whole COLUMNS have no
diagonal (and the coarse columns under them the Galerkin diagonal 0), so that lanes of column-typed
tiles take the keep-the-value branch; the anisotropic boxes, whose coefficients alternate with the line
parity -- no tile of theirs may be column-typed; boxes of 44 / 45 / 88 / 89 lines (one and two tile
rows of 44 lines, whole and ragged: a column-typed tile needs a tile row above and below it, which of
these only the 42-line tiles of 89 lines have)."""
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
import test_gpu_patch_entry as ENTRY                               # noqa: E402
from test_gpu_patch_xf import OMEGA, patch_everywhere              # noqa: E402,F401

CYCLES = 2
LAP_LINES = ["lap256x44", "lap256x45", "lap256x88", "lap256x89"]   # constant coefficients: edge tiles are column-typed
ALTERNATING = ["box384x100", "box1024x300"]                        # coefficients alternate with the line parity


def lap2d(oracle, nx, ny):
    """5-point box with constant coefficients (x coupling -1, y coupling -0.375, diagonal 4)"""
    return XF.box2d_no_diag(oracle, nx, ny, ())


def _problem(oracle, shape):
    """(A, b, levels, pitch of level 0, index of the first level that is no K-Patch level)"""
    if shape in ("lap512", "box1024x300", "nodiag256x50"):
        A, b, L, k = XF._problem(oracle, shape)
        return A, b, L, {"lap512": 512, "box1024x300": 1024, "nodiag256x50": 256}[shape], k
    if shape == "box384x100":
        A, b, L = ENTRY._problem(oracle, shape)
        return A, b, L, 384, 2
    if shape == "nodiagcol256x150":  # columns 33 and 201 (odd, not at a line end, in the first / last tile column)
        nd = [j * 256 + c for j in range(150) for c in (33, 201)]
        A = XF.box2d_no_diag(oracle, 256, 150, nd)
        return A, np.sin(0.001 * np.arange(A.rows)) + 1.5, 4, 256, 2
    assert shape in LAP_LINES
    A = lap2d(oracle, 256, int(shape[len("lap256x"):]))            # pitches 256 and 128 are K-Patch levels
    return A, np.sin(0.001 * np.arange(A.rows)) + 1.5, 4, 256, 2


_REF = {}


def _oracle_twin(oracle, shape):
    if ("twin", shape) not in _REF:
        A, b, L = _problem(oracle, shape)[:3]
        _REF["twin", shape] = [oracle.Multigrid(A, b, L, smoother=oracle.SM_TRUE_JACOBI, smoother_iters=2, omega=OMEGA), 0, {}]
    return _REF["twin", shape]


def _oracle_levels(oracle, shape, cycles=CYCLES):
    """u, f, r of every level after `cycles` cycles of the true-Jacobi oracle twin; each state computed once"""
    tw = _oracle_twin(oracle, shape)
    L = _problem(oracle, shape)[2]
    while tw[1] < cycles:
        tw[0].vcycle()
        tw[1] += 1
        tw[2][tw[1]] = [(tw[0].get_vec(l, "u"), tw[0].get_vec(l, "f"), tw[0].get_vec(l, "r")) for l in range(L)]
    return tw[2][cycles]


def _run(amg, oracle, shape, keep=False, coltype=1, tall=1, xf=1, flags=True, cycles=CYCLES, **extra):
    """level vectors after vcycle(cycles).  The coltype, tall and xf switches are read when the solver is
    created; the tile-flag switch at launch, so it stays as set until the cycles have run."""
    A, b, L = _problem(oracle, shape)[:3]
    amg.set_patch_coltype(coltype)
    amg.set_patch_tall(tall)
    amg.set_patch_xf(xf)
    amg.set_patch_tile_flags(flags)
    try:
        mg = amg.Multigrid(*XF._csc(A), b, L, smoother=amg.SM_JACOBI, smoother_iters=2, omega=OMEGA,
                           keep_residual=keep, exact_coarse_solve=True, **extra)
        try:
            assert mg.fine_sweep_info()[0].startswith("patch_down_kernel") != bool(extra.get("no_fusion"))
            mg.vcycle(cycles)
            return XF._levels(mg, L, keep)
        finally:
            mg.close()
    finally:
        amg.set_patch_coltype(1)
        amg.set_patch_tall(1)
        amg.set_patch_xf(1)
        amg.set_patch_tile_flags(True)


def _unfused(amg, oracle, shape, keep, cycles=CYCLES):
    if ("unfused", shape, keep, cycles) not in _REF:
        _REF["unfused", shape, keep, cycles] = _run(amg, oracle, shape, keep, cycles=cycles, no_fusion=True)
    return _REF["unfused", shape, keep, cycles]


def _check(amg, oracle, shape, keep=False, cycles=CYCLES, **kw):
    """switch on against the oracle twin, the unfused kernels and the switch off (same other switches)"""
    on = _run(amg, oracle, shape, keep, coltype=1, cycles=cycles, **kw)
    off = _run(amg, oracle, shape, keep, coltype=0, cycles=cycles, **kw)
    ENTRY._assert_levels(on, _oracle_levels(oracle, shape, cycles), _unfused(amg, oracle, shape, keep, cycles), keep,
                         (shape, keep, cycles, kw))
    XF._assert_same(on, off, (shape, "switch off", kw))
    return on


# ---- the tile classes, derived from the oracle's level matrices ---------------------------------
def _row_type_ids(A):
    """id of every row's (offset, value) pattern, exact zeros pruned; -1 = empty row"""
    n = A.rows
    cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(A.colptr))
    rows, vals = A.rowind.astype(np.int64), A.val
    nz = vals != 0.0
    rows, offs, vals = rows[nz], (cols - rows)[nz], vals[nz]
    order = np.lexsort((offs, rows))
    rows, offs, vals = rows[order], offs[order], vals[order]
    cnt = np.bincount(rows, minlength=n)
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    pos = np.arange(rows.size) - start[rows]
    W = int(cnt.max())
    key = np.zeros((n, 2 * W + 1))
    key[:, 0] = cnt
    key[rows, 1 + pos] = offs
    key[rows, 1 + W + pos] = vals
    ids = np.unique(key, axis=0, return_inverse=True)[1].reshape(n).astype(np.int64)
    ids[cnt == 0] = -1
    return ids


def _expected_classes(ids, m, rings):
    """(one type, column-typed, general) over the tiles of the launches with `rings` halo rings: 48 held lines,
    columns [-4, 68) -- the seam's frame (5 rings): [-6, 70) -- of the flat index around 64 output columns"""
    n = ids.size
    EH, (EC, CL) = 48, ((76, 6) if rings == 5 else (72, 4))
    th, lines = EH - 2 * rings, (n + m - 1) // m
    out = [0, 0, 0]
    le, c = np.arange(EH)[:, None], np.arange(EC)[None, :]
    for py in range((lines + th - 1) // th):
        for px in range(m // 64):
            idx = (py * th - rings) * m + px * 64 - CL + le * m + c
            if idx[0, 0] < 0 or idx[-1, -1] >= n:
                out[2] += 1
                continue
            t = ids[idx]
            if (t < 0).any():
                out[2] += 1
            elif (t == t[0, 0]).all():
                out[0] += 1
            elif (t == t[0:1, :]).all():
                out[1] += 1
            else:
                out[2] += 1
    return tuple(out)


@pytest.mark.parametrize("shape", ["lap512", "nodiag256x50", "nodiagcol256x150", "lap256x89"] + ALTERNATING)
def test_coltype_tile_classes(amg, oracle, patch_everywhere, shape):
    """the query against counts derived from the oracle's level matrices; off: no column-typed tile, the
    one-type count unchanged"""
    A, b, L, pitch, k = _problem(oracle, shape)
    tw = _oracle_twin(oracle, shape)[0]
    got = {}
    for on in (1, 0):
        amg.set_patch_coltype(on)
        try:
            mg = amg.Multigrid(*XF._csc(A), b, L, smoother=amg.SM_JACOBI, smoother_iters=2, omega=OMEGA,
                               exact_coarse_solve=True)
        finally:
            amg.set_patch_coltype(1)
        try:
            got[on] = {(l, r): mg.patch_tile_classes(l, r) for l in range(k) for r in ((2, 3, 5) if l == 0 else (2, 3))}
            with pytest.raises(ValueError):
                mg.patch_tile_classes(k, 3)          # no K-Patch level
            with pytest.raises(ValueError):
                mg.patch_tile_classes(0, 4)          # no such geometry
        finally:
            mg.close()
    some = 0
    for l in range(k):
        ids = _row_type_ids(tw.level_matrix(l))
        for r in ((2, 3, 5) if l == 0 else (2, 3)):
            want = _expected_classes(ids, pitch >> l, r)
            print(shape, "level", l, "rings", r, "one type / column-typed / general:", got[1][l, r], "expected", want)
            assert got[1][l, r] == want, (l, r)
            assert got[0][l, r] == (want[0], 0, want[1] + want[2]), (l, r)
            some += want[1]
    if shape in ("lap512", "nodiagcol256x150"):
        assert some > 0
    elif shape in ALTERNATING:  # the types alternate with the line: no column has one type
        assert some == 0


def test_coltype_smallest_pitch_all_edge_tiles(amg, oracle, patch_everywhere):
    """pitch 128, the smallest legal one: two tile columns, both at a line end -- no tile has one type"""
    ids = _row_type_ids(_oracle_twin(oracle, "lap512")[0].level_matrix(2))
    one, col, gen = _expected_classes(ids, 128, 2)
    assert one == 0 and col > 0


# ---- same bits ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["lap512", "nodiag256x50", "nodiagcol256x150"] + ALTERNATING + LAP_LINES)
def test_coltype_bitwise(amg, oracle, patch_everywhere, shape):
    _check(amg, oracle, shape)


@pytest.mark.parametrize("shape", ["lap512", "nodiag256x50", "nodiagcol256x150", "lap256x89"])
def test_coltype_keep_residual(amg, oracle, patch_everywhere, shape):
    _check(amg, oracle, shape, keep=True)


@pytest.mark.parametrize("combo", ["flags_off", "xf_off", "tall_off"])
@pytest.mark.parametrize("shape", ["lap512", "nodiagcol256x150"])
def test_coltype_with_other_switches(amg, oracle, patch_everywhere, shape, combo):
    """without tile flags (no flag is read: the general path everywhere), with the stored-form down-legs
    (the non-XF instantiations) and with 42-line tiles on three rings everywhere"""
    kw = {"flags_off": {"flags": False}, "xf_off": {"xf": 0}, "tall_off": {"tall": 0}}[combo]
    _check(amg, oracle, shape, **kw)


def test_coltype_graph_and_eager(amg, oracle, patch_everywhere):
    a = _check(amg, oracle, "lap512", use_graph=True)
    b = _check(amg, oracle, "lap512", use_graph=False)
    XF._assert_same(a, b, "graph / eager")


@pytest.mark.parametrize("n", [2, 3, 4])
def test_coltype_vcycles_seam(amg, oracle, patch_everywhere, n):
    """vcycle(n): the seam launch runs n - 1 times on level 0 (its own flag and column-type arrays)"""
    _check(amg, oracle, "lap512", cycles=n)


def test_coltype_slab_two_ranks(amg, patch_everywhere):
    """slab_setup(rank, 2) on 1024^2 / 9 levels (the slab tests' shape): the later rank's launches start at
    a tile row py0 != 0, which enters the index of the flag and of the column types"""
    import torch
    import slab_vcycle
    from test_gpu_slab import _assemble, _cycle
    n, L, cycles = 1024, 9, 2
    u_ref = XF._single_poisson(amg, n, L, cycles)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    torch.cuda.set_stream(st)
    for on in (1, 0):
        amg.set_patch_coltype(on)
        try:
            engs = [slab_vcycle.HipSlabEngine(amg, dev, st, n, L, OMEGA, 2, r, 2, -1) for r in range(2)]
        finally:
            amg.set_patch_coltype(1)
        try:
            for _ in range(cycles):
                _cycle(engs, poison=True)
            st.synchronize()
            assert np.array_equal(_assemble(engs), u_ref), on
        finally:
            for e in engs:
                e.close()


def test_coltype_window_two_ranks(amg, patch_everywhere):
    """two windows of 1024^2 with three window levels (the window tests' shape)"""
    from test_gpu_window import JAC, _sharded
    n, L, k, cycles = 1024, 10, 3, 2
    u_ref = XF._single_poisson(amg, n, L, cycles)
    for on in (1, 0):
        amg.set_patch_coltype(on)
        try:
            res = _sharded(amg, 2, n, L, k, 2, JAC, 2, OMEGA, cycles)
        finally:
            amg.set_patch_coltype(1)
        assert np.array_equal(res[0][0], u_ref), on


def test_coltype_multicolor_512(amg, oracle, patch_everywhere):
    """the multicolour kernel reads the same flag arrays and takes a flag 254 for 255: unchanged, against the
    oracle and the unfused kernels (the entry test's check, with the switch on) and against the switch off"""
    amg.set_patch_coltype(1)
    ENTRY.test_entry_multicolor_512(amg, oracle, None)
    A, b, L = _problem(oracle, "lap512")[:3]
    got = {}
    for on in (1, 0):
        amg.set_patch_coltype(on)
        try:
            mg = amg.Multigrid(*XF._csc(A), b, L, smoother=amg.SM_MULTICOLOR_GS, smoother_iters=1, exact_coarse_solve=True,
                               keep_residual=True)
        finally:
            amg.set_patch_coltype(1)
        try:
            assert mg.fine_sweep_info()[0].startswith("patch_rb_kernel")
            assert (mg.patch_tile_classes(0, 3)[1] > 0) == bool(on)
            mg.vcycle(CYCLES)
            got[on] = XF._levels(mg, L, True)
        finally:
            mg.close()
    XF._assert_same(got[1], got[0], "multicolour on / off")
