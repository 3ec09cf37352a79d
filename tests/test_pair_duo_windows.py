"""K-Duo windows (amg_hip_duo_windows, host only).  A duo tile owns T rows of level l, the rows c of
level l+1 with 2c in the tile and the rows cc of level l+2 with 4cc in it, and recomputes everything else
it needs from wider windows of what it loads.  Here the owned outputs are marked and "needed" is walked
backwards through every step -- +- hb for a sweep or a residual, fine rows 2c .. 2c + 2 for the
restriction, the coarse rows of a fine row for the prolongation -- and every needed row has to lie in
the window the library returns for that stage, and every window within the capacity it returns.  The
prolongation is walked with the kernel's stencil (linear_prolong_add2_kernel: row 2j takes u_H[j - 1]
and u_H[j], row 2j + 1 takes u_H[j]) together with floor(i / 2) and ceil(i / 2), the superset of both
ways of writing it."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILES = (510, 254)   # the tile heights the launchers use: under a wide band, under a narrow one

# indices into the 31 numbers (include/amg_hip.h): (rows before the base, rows) per window, then capacities
D_R1, D_U1, D_M1, D_R0, D_M0, D_A0, U_S1, U_M1, U_A1, U_S0, U_M0, U_A0 = range(0, 24, 2)
CAP_D_M1, CAP_D_M0, CAP_D_A0, CAP_U_M1, CAP_U_A1, CAP_U_M0, CAP_U_A0 = range(24, 31)
CAP_OF = {D_R1: CAP_D_M1, D_U1: CAP_D_M1, D_M1: CAP_D_M1, D_R0: CAP_D_M0, D_M0: CAP_D_M0, D_A0: CAP_D_A0,
          U_S1: CAP_U_M1, U_M1: CAP_U_M1, U_A1: CAP_U_A1, U_S0: CAP_U_M0, U_M0: CAP_U_M0, U_A0: CAP_U_A0}

HB = (1, 2, 3, 5, 9, 17, 33, 65)
CASES = sorted({(h, (h + 2) // 2) for h in HB} | {(h, h) for h in HB})   # ceil((h + 1) / 2), and h' = h


def _grow(rows, h, n):
    """rows +- h, inside [0, n)"""
    if not rows:
        return set()
    out = set()
    for r in rows:
        out.update(range(max(0, r - h), min(n, r + h + 1)))
    return out


def _fine_of(coarse, n):
    """rows 2c .. 2c + 2 of the finer level that the restriction to the rows `coarse` reads"""
    return {i for c in coarse for i in (2 * c, 2 * c + 1, 2 * c + 2) if 0 <= i < n}


def _coarse_of(fine, n):
    """coarse rows the prolongation into the rows `fine` reads (see the module's docstring)"""
    out = set()
    for i in fine:
        out.update((i // 2 - 1, i // 2) if i % 2 == 0 else (i // 2, (i + 1) // 2))
        out.add(i // 2)
    return {c for c in out if 0 <= c < n}


def _owned(amg, t0, n0, n1, n2, T):
    """the rows of the three levels that the tile starting at t0 owns: the library's ranges
    (amg_hip_duo_owned, the function the kernels call), clipped to the levels' sizes"""
    assert t0 % T == 0
    (a0, b0), (a1, b1), (a2, b2) = amg.duo_owned(t0 // T, T)
    assert (a0, b0) == (t0, t0 + T)
    o0 = set(range(a0, min(b0, n0)))
    o1 = set(range(a1, min(b1, n1)))
    o2 = set(range(a2, min(b2, n2)))
    # the rule: c belongs to the tile that owns fine row 2c, cc to the one that owns row 4cc
    assert all(t0 <= 2 * c < t0 + T for c in range(a1, b1)) and all(t0 <= 4 * c < t0 + T for c in range(a2, b2))
    return o0, o1, o2


def _inside(rows, w, which, base, tag):
    lo = base - int(w[which])
    hi = lo + int(w[which + 1])
    bad = [r for r in rows if not lo <= r < hi]
    assert not bad, (tag, "window", (lo, hi), "misses", bad[:4])


def _windows(amg, h0, h1, T):
    fits, w = amg.duo_windows(h0, h1, T)
    within = all(int(w[k + 1]) <= int(w[CAP_OF[k]]) for k in CAP_OF)
    assert fits == within, (h0, h1, w)
    return fits, w


@pytest.mark.parametrize("T", TILES)
@pytest.mark.parametrize("h0,h1", CASES)
def test_windows_hold_what_the_steps_need(amg, h0, h1, T):
    fits, w = _windows(amg, h0, h1, T)
    if h1 == (h0 + 2) // 2:
        assert fits, "the half-bandwidths of two consecutive Galerkin levels have to fit"
    if not fits:
        return   # the library keeps the pair form for such a pair of levels (65 over 65)
    for k in CAP_OF:
        assert int(w[k]) % 2 == 0 and int(w[k + 1]) % 2 == 0, "pairs never straddle a window end"
    n0 = 4 * T + 7                      # four full tiles and a ragged last one of 7 rows
    n1, n2, nf = (n0 - 1) // 2, ((n0 - 1) // 2 - 1) // 2, 2 * n0 + 1
    tiles = (n0 + T - 1) // T
    for tile in (0, 1, tiles - 2, tiles - 1):
        t0 = tile * T
        ce = (t0 // 2) & ~1
        o0, o1, o2 = _owned(amg, t0, n0, n1, n2, T)
        tag = (h0, h1, T, "tile", tile)
        # down-leg, backwards from f_{l+2} and its first sweep on the owned rows
        r1 = _fine_of(o2, n1) | o1                    # residual of l+1 (stored on owned rows when kept)
        u1 = _grow(r1, h1, n1) | o1                   # second sweep of l+1
        m1 = _grow(u1, h1, n1) | o1                   # f_{l+1} and the first sweep from zero
        r0 = _fine_of(m1, n0) | o0                    # residual of l
        u0 = _grow(r0, h0, n0) | o0                   # second sweep of l
        a0 = _grow(u0, h0, n0)                        # tmp_l
        _inside(r1, w, D_R1, ce, tag + ("r1",))
        _inside(u1, w, D_U1, ce, tag + ("u1",))
        _inside(m1, w, D_M1, ce, tag + ("m1",))
        _inside(r0, w, D_R0, 2 * ce, tag + ("r0",))
        _inside(u0, w, D_M0, 2 * ce, tag + ("u0",))
        _inside(a0, w, D_A0, 2 * ce, tag + ("a0",))
        # up-leg, backwards from the prolongation into level l-1: the tile prolongs the points
        # t0 + 1 .. t0 + T (t0 too in the first tile; n0 is the virtual point) and stores its owned rows
        pts = [j for j in range(t0 + (1 if tile else 0), t0 + T + 1) if j <= n0]
        s0 = {i for j in pts for i in (j - 1, j) if 0 <= i < n0} | o0
        m0 = _grow(s0, h0, n0)                        # first sweep of l
        p0 = _grow(m0, h0, n0)                        # u_l + P u_{l+1}
        s1 = _coarse_of(p0, n1) | o1                  # second sweep of l+1
        mm1 = _grow(s1, h1, n1)                       # first sweep of l+1
        a1 = _grow(mm1, h1, n1)                       # tmp_{l+1}
        _inside(s0, w, U_S0, t0, tag + ("s0",))
        _inside(m0, w, U_M0, t0, tag + ("m0",))
        _inside(p0, w, U_A0, t0, tag + ("p0",))
        _inside(s1, w, U_S1, ce, tag + ("s1",))
        _inside(mm1, w, U_M1, ce, tag + ("m1 up",))
        _inside(a1, w, U_A1, ce, tag + ("a1",))


def test_the_issue_s_figures(amg):
    """T = 510 over half-bandwidths 65 / 33: the sweep window of level l still fits two passes of 512"""
    fits, w = _windows(amg, 65, 33, 510)
    assert fits and int(w[D_M0 + 1]) <= 1024 and int(w[CAP_D_M0]) == 1024
    assert not _windows(amg, 65, 65, 510)[0]
    assert not amg.duo_windows(66, 3, 510)[0] and not amg.duo_windows(3, 2, 511)[0] and not amg.duo_windows(3, 2, 512)[0]
    # half-bandwidths 33 over 17 on tiles of 254 rows: every stage is one pass of 256 lanes x 2 rows
    fits, w = _windows(amg, 33, 17, 254)
    assert fits and max(int(w[k + 1]) for k in CAP_OF if k not in (D_A0, U_A0, U_A1)) <= 512


@pytest.mark.parametrize("T", TILES)
@pytest.mark.parametrize("n0", [256, 509, 510, 511, 1021, 4095])
def test_every_row_is_owned_once(amg, n0, T):
    for n1 in ((n0 - 1) // 2, (n0 + 1) // 2):
        for n2 in ((n1 - 1) // 2, (n1 + 1) // 2):
            cnt = [np.zeros(n, int) for n in (n0, n1, n2)]
            for tile in range((n0 + T - 1) // T):
                for c, o in zip(cnt, _owned(amg, tile * T, n0, n1, n2, T)):
                    c[sorted(o)] += 1
            for lev, c in enumerate(cnt):
                assert (c == 1).all(), (n0, n1, n2, "level +%d" % lev, np.flatnonzero(c != 1)[:4])


def test_tile_heights_the_launchers_use(amg):
    """254 rows where the half-window of level l is at most 34 rows, 510 above; both are in TILES"""
    assert [amg.duo_tile_rows(h) for h in (0, 1, 17, 33, 34, 35, 65)] == [254, 254, 254, 254, 254, 510, 510]
    assert set(amg.duo_tile_rows(h) for h in range(66)) == set(TILES)
    with pytest.raises(ValueError):
        amg.duo_owned(0, 511)
