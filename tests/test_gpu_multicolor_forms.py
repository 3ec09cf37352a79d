"""The four device forms of the multicolour smoother -- patch colour stages (patch_rb_kernel), K-Strip
(mc_strip_kernel), the one-workgroup pass (dict_gs_sweep_kernel, levels of at most 8192 rows) and one
launch per colour (dict_gs_color_kernel) -- off the square 5-point Laplacian: on the operators of
tests/mc_ops.py (coefficients that vary by column and line parity, odd pitches, 4 to 9 colours on
wider stencils, 1-D bands whose levels need 15 stages or shrink to 3 rows, a nonsymmetric box).

Every case builds (a) the fused solver, (b) the same with no_fusion and (c) the oracle twin with
(a)'s colouring replayed, starts all three from the same seeded u and compares u and f (r where it
is kept) of every level bit for bit after EACH of 2 cycles; the coarsest u is the direct solve
either way and is compared with the oracle only where r is kept.  Before the first cycle the case
asserts the launch form of every level and leg through leg_form(), and the strip geometry through
strip_geometry(): a case cannot fall back to another form and still pass.  A plain level runs the
one-workgroup pass when it has at most ONE_LAUNCH_ROWS rows (and fusion is on), else the colour
launches; the helper asserts which from the level's row count.

Shapes that differ from the first plan of these cases, and why:
  - box5(542,130), level 1: the first-fit colouring gives 5 colours, not 4 (the level is refused
    either way: one half-bandwidth of 272 rows times 10 does not fit the window)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "algebraic-multigrid_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import mc_ops as M  # noqa: E402

CYCLES = 2
ONE_LAUNCH_ROWS = 8192     # solver.cpp: mc_one_launch_max_rows
STRIP_WMAX = 4608          # kernels.hip: rows of a strip's LDS window
STRIP, PATCH, PLAIN = "mc_strip", "mc_patch", "plain"

OPS = {
    "box5_96x40": lambda: M.box5(96, 40),
    "box5_97x41": lambda: M.box5(97, 41),
    "box9_96x40": lambda: M.box9(96, 40),
    "box13_96x40": lambda: M.box13(96, 40),
    "band1025": lambda: M.band(*M.BAND1025),
    "band257": lambda: M.band(*M.BAND257),
    "box5_542x130": lambda: M.box5(542, 130),
    "box5_520x260": lambda: M.box5(520, 260),
    "box5_544x125": lambda: M.box5(544, 125),
    "box5_160x60": lambda: M.box5(160, 60),
    "conv_96x40": lambda: M.box5_conv(96, 40),
    "box5_384x100": lambda: M.box5(384, 100),
    "box9_384x100": lambda: M.box9(384, 100),
}
_MAT = {}
_ORACLE = {}
_UNFUSED = {}


@pytest.fixture
def patch_everywhere(amg):
    amg.set_patch_min_rows(0)          # every level whose band has a 2-D pitch >= 128
    yield
    amg.set_patch_min_rows(amg.PATCH_MIN_ROWS_DEFAULT)


def _matrix(op):
    if op not in _MAT:
        _MAT[op] = OPS[op]()
    return _MAT[op]


def _snapshot(mg, L, keep):
    return [(mg.get_soln(l), mg.get_rhs(l), mg.get_residual(l) if keep else None) for l in range(L)]


def _device_cycles(amg, op, L, iters, keep, **extra):
    """a device solver of the case before its first cycle, level 0 holding the seeded start vector"""
    cp, ri, v = _matrix(op)
    n = cp.size - 1
    mg = amg.Multigrid(cp, ri, v, M.rhs(n), L, smoother=amg.SM_MULTICOLOR_GS, smoother_iters=iters, omega=1.0,
                       exact_coarse_solve=True, keep_residual=keep, **extra)
    mg.set_vec(0, "u", M.start(n))
    return mg


def _cycles(mg, L, keep):
    out = []
    for _ in range(CYCLES):
        mg.vcycle()
        out.append(_snapshot(mg, L, keep))
    return out


def _unfused(amg, op, L, iters, keep, stencil_transfers):
    """(b): the same cycles by the unfused kernels; every level but the coarsest is plain.  Once per key"""
    key = (op, L, iters, keep, stencil_transfers)
    if key not in _UNFUSED:
        mg = _device_cycles(amg, op, L, iters, keep, no_fusion=True, stencil_transfers=stencil_transfers)
        try:
            forms = [mg.leg_form(l) for l in range(L)]
            assert forms == [(PLAIN, PLAIN)] * (L - 1) + [(PLAIN if keep else "none", "none")], forms
            _UNFUSED[key] = _cycles(mg, L, keep)
        finally:
            mg.close()
    return _UNFUSED[key]


def _oracle_cycles(oracle, op, L, iters, colors):
    """(c): u, f, r of every level after each cycle of the oracle twin on the solver's colouring.  Once
    per (operator, levels, passes); the colouring is a function of the hierarchy alone"""
    key = (op, L, iters)
    if key not in _ORACLE:
        cp, ri, v = _matrix(op)
        n = cp.size - 1
        ref = oracle.Multigrid(oracle.CSC(n, n, cp, ri, v), M.rhs(n), L, smoother=oracle.SM_MULTICOLOR,
                               smoother_iters=iters, omega=1.0)
        for l, (col, nc) in enumerate(colors):
            ref.set_colors(l, col, nc)
        ref.set_vec(0, "u", M.start(n))
        out = []
        for _ in range(CYCLES):
            ref.vcycle()
            out.append([(ref.get_vec(l, "u"), ref.get_vec(l, "f"), ref.get_vec(l, "r")) for l in range(L)])
        _ORACLE[key] = (out, [(c.copy(), k) for c, k in colors])
    out, kept = _ORACLE[key]
    for (c, k), (c2, k2) in zip(colors, kept):
        assert k == k2 and np.array_equal(c, c2)
    return out


def _expected_forms(L, forms, keep):
    """forms: one name per level but the coarsest (the same on both legs)"""
    assert len(forms) == L - 1
    return [(f, f) for f in forms] + [(PLAIN if keep else "none", "none")]


def _run(amg, oracle, op, L, forms, geometry=None, iters=1, keep=False, one_launch=None, **extra):
    """forms: the expected form of every level but the coarsest; geometry: {level: (T, tiles, stages,
    halo_down, halo_up)} of every strip level; one_launch: {level: bool} of every plain level (True:
    the one-workgroup pass, False: one launch per colour).  Returns (a)'s levels after each cycle."""
    geometry = geometry or {}
    one_launch = one_launch or {}
    tag = (op, L, iters, keep, tuple(sorted(extra.items())))
    mg = _device_cycles(amg, op, L, iters, keep, **extra)
    try:
        got = [mg.leg_form(l) for l in range(L)]
        print(tag, "forms", got)
        geo = {}
        for l in range(L):
            if got[l][0] == STRIP:
                geo[l] = tuple(mg.strip_geometry(l))
            else:
                with pytest.raises(ValueError, match="no K-Strip level"):
                    mg.strip_geometry(l)
        print(tag, "strips", geo)
        rows = [mg.get_n_dofs(l) for l in range(L)]
        assert got == _expected_forms(L, forms, keep), (tag, got)
        assert geo == {l: tuple(g) for l, g in geometry.items()}, (tag, geo)
        assert sorted(geometry) == [l for l in range(L - 1) if forms[l] == STRIP]
        for T, tiles, stages, halo_down, halo_up in geo.values():
            assert T + 2 * halo_down + 2 <= STRIP_WMAX and halo_up < halo_down
        # which launches a plain level runs is a function of its rows (enqueue_multicolor)
        assert sorted(one_launch) == [l for l in range(L - 1) if forms[l] == PLAIN], tag
        for l, one in one_launch.items():
            assert (rows[l] <= ONE_LAUNCH_ROWS) == one, (tag, l, rows[l])
        colors = [mg.get_colors(l) for l in range(L)]
        a = _cycles(mg, L, keep)
        assert [mg.leg_form(l) for l in range(L)] == got       # the plan that ran is the one announced
    finally:
        mg.close()
    b = _unfused(amg, op, L, iters, keep, extra.get("stencil_transfers", True))
    c = _oracle_cycles(oracle, op, L, iters, colors)
    for k in range(CYCLES):
        for l in range(L):
            for name, p, q, o in zip("ufr", a[k][l], b[k][l], c[k][l]):
                if p is None:
                    continue
                assert np.array_equal(p, q), (tag, "no_fusion", "cycle", k, "level", l, name)
                if name == "u" and l == L - 1 and not keep:
                    continue               # the coarsest level's u is the direct solve either way
                assert np.array_equal(p, o), (tag, "oracle", "cycle", k, "level", l, name)
    return a


# ---- 1, 6: strips on varying coefficients ------------------------------------------------------
GEO_BOX5_96 = {0: (256, 15, 3, 384, 288), 1: (256, 8, 7, 400, 350), 2: (256, 4, 7, 208, 182),
               3: (256, 2, 7, 112, 98), 4: (256, 1, 7, 64, 56)}


def test_strips_varying_coefficients_graph_and_eager(amg, oracle):
    """box5(96,40), 6 levels: levels 0-4 are strips of 256 rows, 15, 8, 4, 2, 1 tiles"""
    g = _run(amg, oracle, "box5_96x40", 6, [STRIP] * 5, GEO_BOX5_96, use_graph=True)
    e = _run(amg, oracle, "box5_96x40", 6, [STRIP] * 5, GEO_BOX5_96, use_graph=False)
    for k in range(CYCLES):
        for l in range(6):
            for p, q in zip(g[k][l][:2], e[k][l][:2]):
                assert np.array_equal(p, q), (k, l)


def test_strips_varying_coefficients_keep_residual(amg, oracle):
    _run(amg, oracle, "box5_96x40", 6, [STRIP] * 5, GEO_BOX5_96, keep=True)


# ---- 2: odd pitch, odd and even n ----------------------------------------------------------------
def test_strips_odd_pitch(amg, oracle):
    """box5(97,41), 5 levels: n = 3977, 1988, 993, 496 (247 is solved)"""
    _run(amg, oracle, "box5_97x41", 5, [STRIP] * 4,
         {0: (256, 16, 3, 392, 294), 1: (256, 8, 7, 400, 350), 2: (256, 4, 7, 208, 182), 3: (256, 2, 7, 112, 98)})


# ---- 3: four colours on the finest level ---------------------------------------------------------
def test_strips_four_colours_on_level_0(amg, oracle):
    _run(amg, oracle, "box9_96x40", 5, [STRIP] * 4,
         {0: (256, 15, 7, 784, 686), 1: (256, 8, 7, 400, 350), 2: (256, 4, 7, 208, 182), 3: (256, 2, 7, 112, 98)})


# ---- 4, 6: many colours ----------------------------------------------------------------------------
GEO_BAND1025 = {0: (256, 5, 7, 96, 84), 1: (256, 2, 15, 128, 120), 2: (256, 1, 9, 40, 36), 3: (256, 1, 7, 32, 28)}


@pytest.mark.parametrize("keep", [False, True], ids=["", "keep_residual"])
def test_strips_many_colours(amg, oracle, keep):
    """band(1025): 4, 8, 5, 4 colours = 7, 15, 9, 7 stages (15: the most one pass reaches); the fifth
    tile of level 0 holds row 1024 alone"""
    _run(amg, oracle, "band1025", 5, [STRIP] * 4, GEO_BAND1025, keep=keep)


# ---- 5: down to three rows ---------------------------------------------------------------------------
@pytest.mark.parametrize("keep", [False, True], ids=["", "keep_residual"])
def test_strips_down_to_three_rows(amg, oracle, keep):
    """band(257), 8 levels: n = 257 (a one-row last tile), 128, 63, 31, 15, 7, 3 -> 1.  Row 256 has no
    coarse row of its own: of what its tile computes beyond u, only the kept r is stored"""
    tail = (256, 1, 5, 12, 10)
    _run(amg, oracle, "band257", 8, [STRIP] * 7,
         {0: (256, 2, 3, 32, 24), 1: (256, 1, 9, 40, 36), 2: (256, 1, 7, 32, 28), 3: tail, 4: tail, 5: tail, 6: tail},
         keep=keep)


# ---- 7: more passes -------------------------------------------------------------------------------------
def test_strips_two_passes(amg, oracle):
    """smoother_iters = 2: 5, 13, 13 stages"""
    _run(amg, oracle, "box5_96x40", 4, [STRIP] * 3,
         {0: (256, 15, 5, 576, 480), 1: (256, 8, 13, 700, 650), 2: (256, 4, 13, 364, 338)}, iters=2)


def test_strips_three_passes_refuse_19_stages(amg, oracle):
    """smoother_iters = 3: level 0 has 7 stages; levels 1-2 would need 19 > 16 and run the
    one-workgroup pass three times"""
    _run(amg, oracle, "box5_96x40", 4, [STRIP, PLAIN, PLAIN], {0: (256, 15, 7, 768, 672)}, iters=3,
         one_launch={1: True, 2: True})


# ---- 8: window limits ---------------------------------------------------------------------------------------
def test_strip_window_exactly_full(amg, oracle):
    """box5(542,130): level 0 runs T = T_max = 270 and its down-leg window is the whole LDS window;
    level 1 (half-bandwidth 272) is refused and runs one launch per colour"""
    geo = {0: (270, 261, 3, 4 * 542, 3 * 542)}
    assert geo[0][0] + 2 * geo[0][3] + 2 == STRIP_WMAX
    _run(amg, oracle, "box5_542x130", 3, [STRIP, PLAIN], geo, one_launch={1: False})


def test_strip_rows_clamped_and_unclamped(amg, oracle):
    """box5(520,260): level 0 T = 446 (clamped from 530), 304 tiles; level 1 T = 266 (its own n / 256,
    above the floor of 256 and below its T_max of 414)"""
    _run(amg, oracle, "box5_520x260", 3, [STRIP, STRIP], {0: (446, 304, 3, 2080, 1560), 1: (266, 255, 7, 2096, 1834)})


def test_strip_refused_below_256_rows(amg, oracle):
    """box5(544,125): T_max = 254 on level 0: refused; levels 0 and 1 run one launch per colour"""
    _run(amg, oracle, "box5_544x125", 3, [PLAIN, PLAIN], one_launch={0: False, 1: False})


# ---- 9: fallbacks -----------------------------------------------------------------------------------------------
def test_plain_one_workgroup_pass_7_and_9_colours(amg, oracle):
    """box13(96,40): 7 colours at half-bandwidth 192 fit no strip, 9 colours are 17 stages"""
    _run(amg, oracle, "box13_96x40", 4, [PLAIN] * 3, one_launch={0: True, 1: True, 2: True})


def test_plain_colour_launches_two_passes(amg, oracle):
    """box5(160,60), 9600 rows, without stencil transfers: level 0 runs one launch per colour, the
    second pass without its colour 0 (it directly follows colour 0 of the first)"""
    _run(amg, oracle, "box5_160x60", 3, [PLAIN, PLAIN], iters=2, stencil_transfers=False,
         one_launch={0: False, 1: True})


def test_plain_nonsymmetric(amg, oracle):
    _run(amg, oracle, "conv_96x40", 5, [PLAIN] * 4, one_launch={l: True for l in range(4)})


# ---- 10: patch colour stages off the Laplacian -----------------------------------------------------------------
GEO_384_L2 = {2: (256, 38, 7, 784, 686)}


@pytest.mark.parametrize("keep", [False, True], ids=["", "keep_residual"])
@pytest.mark.parametrize("op", ["box5_384x100", "box9_384x100"])
def test_patch_colour_stages(amg, oracle, patch_everywhere, op, keep):
    """pitches 384 and 192 (19 199 rows: a ragged last line) run patch colour stages -- box5: the
    checkerboard, then the 4-colour product colouring; box9: 4 colours from level 0 -- and pitch 96 a strip"""
    _run(amg, oracle, op, 4, [PATCH, PATCH, STRIP], GEO_384_L2, keep=keep)


def test_patch_colour_stages_two_passes(amg, oracle, patch_everywhere):
    _run(amg, oracle, "box5_384x100", 4, [PATCH, PATCH, STRIP], {2: (256, 38, 13, 1372, 1274)}, iters=2)


# ---- 11: level-0 reporting ----------------------------------------------------------------------------------------
def test_level_0_strip_is_reported_and_profiled(amg):
    """Poisson 512^2 at the default K-Patch threshold: level 0 is a strip (2 colours, half-bandwidth
    512, T = T_max = 510).  fine_sweep_info names the launch, profile_fine_sweep runs it and leaves
    the solver as it was: the next cycle gives the bits of a solver that was never profiled."""
    L = 6
    kw = dict(smoother=amg.SM_MULTICOLOR_GS, smoother_iters=1, exact_coarse_solve=True)
    mg = amg.Multigrid.poisson(512, L, **kw)
    ref = amg.Multigrid.poisson(512, L, **kw)
    try:
        forms = [mg.leg_form(l) for l in range(L)]
        print("lap512 forms", forms, [tuple(mg.strip_geometry(l)) for l in range(L) if forms[l][0] == STRIP])
        assert forms == _expected_forms(L, [STRIP] * 5, False), forms
        n, nH = mg.get_n_dofs(0), mg.get_n_dofs(1)
        geo = mg.strip_geometry(0)
        assert tuple(geo) == (510, (n + 509) // 510, 3, 4 * 512, 3 * 512)
        name, stages, nbytes = mg.fine_sweep_info()
        assert name.startswith("mc_strip_kernel<") and name.endswith("false, true>"), name
        assert stages == geo.stages == 3 and nbytes == 26.0 * n + 16.0 * nH
        with pytest.raises(ValueError):
            mg.leg_form(L)
        with pytest.raises(ValueError):
            mg.leg_form(-1)
        mg.vcycle()
        ref.vcycle()
        u = mg.get_soln(0)
        avg, mn, k, pname, pbytes = mg.profile_fine_sweep(3)
        assert (pname, k, pbytes) == (name, stages, nbytes) and 0.0 < mn <= avg
        assert np.array_equal(mg.get_soln(0), u)
        mg.vcycle()
        ref.vcycle()
        for l in range(L):
            assert np.array_equal(mg.get_soln(l), ref.get_soln(l)), l
            assert np.array_equal(mg.get_rhs(l), ref.get_rhs(l)), l
    finally:
        mg.close()
        ref.close()
