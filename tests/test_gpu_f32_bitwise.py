"""The single-precision V-cycle (amg_hip_apply_f32; kernels.hip: K-F32) bit for bit against its float32
restatement tests/f32_twin.py, step by step on random data through the test hooks amg_hip_f32_set_vec /
amg_hip_f32_level_op / amg_hip_f32_get_vec, and as a whole cycle (every level's u, f and r, captured
and eager, first and replayed call).  Equality is on view(np.uint32) everywhere.

The twin takes the level matrices and transfers from the solver's getters, rounds them with
astype(float32) and walks them in row order; the only thing it borrows from the device is the DOUBLE
coarsest solve (amg_hip_level_op 4 on the solver's own double vectors, pinned by the double tests),
which the float cycle runs between two roundings.

Cases (the smallest shapes that reach each path; layout SELL unless stated, true Jacobi 2+2 omega 0.8
unless stated):
  t33, t64          mixed_twin.operator: tensor_dev 33x20 / 3 levels, tensor 64x64 / 5.  The odd line 33:
                    restriction pairs that are not aligned, a last panel that is partial
  t33-i32, t33-csr  t33 with 32-bit SELL indices; with layout CSR (csr_f32_kernel's row modes)
  t33-it1, t33-it3  smoother_iters 1 and 3: an odd pass count, the copy home from the second buffer
  box               tensor_dev 17x12x9 / 3: 27-entry rows on level 1 (the w > 9 loop), 3-D transfers
  cheb1 .. cheb3    t33 with Chebyshev degree 1, 2, 3, one application: the four step modes, d written
                    and read, odd passes for degree 1 and 3; cheb3 also in CSR and on 32-bit indices,
                    cheb2 also with two applications
  nat-all, nat-xlow natural_twin.diffusion 33x20 / 3: every side natural and singular; Dirichlet on
                    x-low only.  Weight 1 at fine point 0 and at the last point of the odd axis
  per-*             periodic_twin.diffusion: (32, 20) / 4 masks (3, 3, 1) periodic xy; (32, 21) / 4
                    periodic x; (16, 12, 8) / 3 periodic xyz; (6, 4) / 2 periodic xy (the seam beside the
                    first coarse point)
  semi2, semi3      semi_twin.case((33, 20), (1, 1e-3)) and ((17, 12, 9), (1e-3, 1, 1e-3)), automatic
                    masks: axes that are not coarsened
  rs48              ruge_stueben on the 48^2 Laplacian, min_coarse 100: CSR transfers in float
  knn, knn-csr      irregular_mats.knn(1600, 4, 1), ruge_stueben(12, 0.25, 40), omega 0.6: ragged
                    panels, wide rows
  lin63, lin64      Multigrid on the 63^2 / 64^2 Laplacian, 3 levels: the flat stride-2 transfers, odd
                    and even n_h
  nonsym            33x20 diffusion plus first-order upwind convection (an M-matrix that is not
                    symmetric), Multigrid.tensor: Jacobi on the column walk, the residual on the rows"""
import os
import sys

import numpy as np
import pytest

sp = pytest.importorskip("scipy.sparse")
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import f32_twin as FT  # noqa: E402
import irregular_mats as im  # noqa: E402
import mixed_twin as MT  # noqa: E402
import natural_twin as N  # noqa: E402
import periodic_twin as PT  # noqa: E402
import semi_twin as S  # noqa: E402

pytestmark = pytest.mark.gpu

DICT, SELL, CSR = 3, 2, 1
JAC = dict(smoother=3, smoother_iters=2, omega=0.8)


def cheb(degree, iters=1):
    return dict(smoother=5, smoother_iters=iters, cheb_degree=degree)


def _csc(A):
    Ac = sp.csc_matrix(A)
    Ac.sort_indices()
    return Ac.indptr.astype(np.int32), Ac.indices.astype(np.int32), Ac.data.copy()


def _csr(A):
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy()


_MATS = {}


def upwind():
    """mixed_twin.diffusion on 33x20 plus a first-order upwind convection term, velocity (3, 1.5): row i
    gains c on its diagonal and -c on its upstream neighbour along each axis.  Off-diagonals stay <= 0
    and the rows stay diagonally dominant (an M-matrix); the matrix is not symmetric."""
    if "upwind" not in _MATS:
        nx, ny = 33, 20
        A = MT.diffusion((nx, ny), seed=2)
        sx = sp.kron(sp.identity(ny), sp.eye(nx, k=-1))
        sy = sp.kron(sp.eye(ny, k=-1), sp.identity(nx))
        ident = sp.identity(nx * ny)
        B = sp.csr_matrix(A + 3.0 * (ident - sx) + 1.5 * (ident - sy))
        B.sort_indices()
        _MATS["upwind"] = B
    return _MATS["upwind"]


def _mixed(amg, grid, dev, **kw):
    dims, levels, A, b, _ = MT.operator(grid)
    if dev:
        return amg.Multigrid.tensor_dev(*_csr(A), b.copy(), dims, levels, **kw)
    return amg.Multigrid.tensor(*_csc(A), b, dims, levels, **kw)


def _t33(**over):
    """t33 with other options; a case that names its smoother takes none of JAC"""
    def make(amg, oracle, **kw):
        base = dict(layout=SELL) if "smoother" in over else dict(JAC, layout=SELL)
        return _mixed(amg, "33x20", True, **dict(base, **over), **kw)
    return make


def _natural(dirichlet):
    def make(amg, oracle, **kw):
        A = N.diffusion((33, 20), dirichlet)
        b = N.rhs(A.shape[0], dirichlet)
        sides = 15 & ~dirichlet
        return amg.Multigrid.tensor(*_csc(A), b, (33, 20), 3, natural_sides=sides, singular=(dirichlet == 0),
                                    layout=SELL, **JAC, **kw)
    return make


def _periodic(dims, nl, masks, per):
    def make(amg, oracle, **kw):
        dirichlet = PT.open_sides(len(dims), per)
        A = PT.diffusion(dims, per, dirichlet)
        b = PT.rhs(A.shape[0], dirichlet == 0)
        return amg.Multigrid.tensor_periodic(*_csc(A), b, dims, nl, per, axis_masks=masks, natural_sides=0,
                                             singular=(dirichlet == 0), layout=SELL, **JAC, **kw)
    return make


def _semi(dims, eps):
    def make(amg, oracle, **kw):
        A, b, _ = S.case(dims, eps)
        return amg.Multigrid.tensor_semi(*_csc(A), b, dims, S.MAX_LEVELS, theta=S.THETA, min_coarse=S.MIN_COARSE,
                                         layout=SELL, **JAC, **kw)
    return make


def _rs48(amg, oracle, **kw):
    Ao = oracle.laplacian(48)
    b = np.random.default_rng(7).standard_normal(48 * 48)
    return amg.Multigrid.ruge_stueben(Ao.colptr, Ao.rowind, Ao.val, b, min_coarse=100, layout=SELL, **JAC, **kw)


def _knn(layout):
    def make(amg, oracle, **kw):
        if "knn" not in _MATS:
            _MATS["knn"] = im.knn(1600, 4, 1)
        b = np.random.default_rng(7).standard_normal(1600)
        return amg.Multigrid.ruge_stueben(*_csc(_MATS["knn"]), b, 12, 0.25, 40, layout=layout, smoother=3,
                                          smoother_iters=2, omega=0.6, **kw)
    return make


def _lin(n):
    def make(amg, oracle, **kw):
        Ao = oracle.laplacian(n)
        b = np.random.default_rng(7).standard_normal(n * n)
        return amg.Multigrid(Ao.colptr, Ao.rowind, Ao.val, b, 3, layout=SELL, **JAC, **kw)
    return make


def _nonsym(amg, oracle, **kw):
    A = upwind()
    b = np.random.default_rng(7).standard_normal(A.shape[0])
    return amg.Multigrid.tensor(*_csc(A), b, (33, 20), 3, layout=SELL, **JAC, **kw)


# name -> (constructor, what the getters must say).  layout: of every level with a float matrix;
# kind: level_transfer_kind of every level; idx32: 32-bit SELL indices; the rest is named per key below
CASES = {
    "t33": (_t33(), dict(layout=SELL, kind=2, passes=2)),
    "t64": (lambda amg, oracle, **kw: _mixed(amg, "64x64", False, **dict(JAC, layout=SELL), **kw),
            dict(layout=SELL, kind=2, passes=2, levels=5)),
    "t33-i32": (_t33(), dict(layout=SELL, kind=2, idx32=True)),
    "t33-csr": (_t33(layout=CSR), dict(layout=CSR, kind=2)),
    "t33-it1": (_t33(smoother_iters=1), dict(layout=SELL, kind=2, passes=1)),
    "t33-it3": (_t33(smoother_iters=3), dict(layout=SELL, kind=2, passes=3)),
    "box": (lambda amg, oracle, **kw: _mixed(amg, "17x12x9", True, **dict(JAC, layout=SELL), **kw),
            dict(layout=SELL, kind=2, width=27)),
    "cheb1": (_t33(**cheb(1)), dict(layout=SELL, kind=2, passes=1)),
    "cheb2": (_t33(**cheb(2)), dict(layout=SELL, kind=2, passes=2)),
    "cheb3": (_t33(**cheb(3)), dict(layout=SELL, kind=2, passes=3)),
    "cheb3-csr": (_t33(**cheb(3), layout=CSR), dict(layout=CSR, kind=2, passes=3)),
    "cheb3-i32": (_t33(**cheb(3)), dict(layout=SELL, kind=2, passes=3, idx32=True)),
    "cheb2-it2": (_t33(**cheb(2, 2)), dict(layout=SELL, kind=2, passes=4)),
    "nat-all": (_natural(0), dict(layout=SELL, kind=2, sides=15)),
    "nat-xlow": (_natural(1), dict(layout=SELL, kind=2, sides=14)),
    "per-xy": (_periodic((32, 20), 4, (3, 3, 1), 3), dict(layout=SELL, kind=2, periodic=3, axes=[3, 3, 1])),
    "per-x": (_periodic((32, 21), 4, None, 1), dict(layout=SELL, kind=2, periodic=1, axes=[3, 3, 3])),
    "per-xyz": (_periodic((16, 12, 8), 3, None, 7), dict(layout=SELL, kind=2, periodic=7, axes=[7, 7])),
    "per-small": (_periodic((6, 4), 2, None, 3), dict(layout=SELL, kind=2, periodic=3, axes=[3])),
    "semi2": (_semi((33, 20), (1.0, 1e-3)), dict(layout=SELL, kind=2, semi=((33, 20), (1.0, 1e-3)))),
    "semi3": (_semi((17, 12, 9), (1e-3, 1.0, 1e-3)), dict(layout=SELL, kind=2, semi=((17, 12, 9), (1e-3, 1.0, 1e-3)))),
    "rs48": (_rs48, dict(layout=SELL, kind=0)),
    "knn": (_knn(SELL), dict(layout=SELL, kind=0, ragged=True)),
    "knn-csr": (_knn(CSR), dict(layout=CSR, kind=0, ragged=True)),
    "lin63": (_lin(63), dict(layout=SELL, kind=1, n0=63 * 63)),
    "lin64": (_lin(64), dict(layout=SELL, kind=1, n0=64 * 64)),
    "nonsym": (_nonsym, dict(layout=SELL, kind=2, unsym0=True)),
}


def make(amg, oracle, case, **kw):
    ctor, want = CASES[case]
    if want.get("idx32"):
        amg.set_index16(0)
    try:
        return ctor(amg, oracle, **kw)
    finally:
        amg.set_index16(1)  # the library's default; the switch has no getter


def _jac(omega, iters):
    return lambda mg: ("jacobi", omega, iters)


def _cheb(degree, iters=1):
    return lambda mg: ("cheb", degree, iters, [mg.cheb_bounds(l) for l in range(mg.n_levels - 1)])


SMOOTHERS = {name: _jac(0.8, 2) for name in CASES}
SMOOTHERS.update({"t33-it1": _jac(0.8, 1), "t33-it3": _jac(0.8, 3), "knn": _jac(0.6, 2), "knn-csr": _jac(0.6, 2),
                  "cheb1": _cheb(1), "cheb2": _cheb(2), "cheb3": _cheb(3), "cheb3-csr": _cheb(3),
                  "cheb3-i32": _cheb(3), "cheb2-it2": _cheb(2, 2)})


def device_coarse(mg):
    """the solver's own double coarsest solve: float64 -> float64"""
    last = mg.n_levels - 1

    def solve(f64):
        mg.set_vec(last, "f", f64)
        mg.level_op(last, 4)
        return mg.get_soln(last)
    return solve


_HIER = {}


def hierarchy(mg, case):
    """f32_twin.Hierarchy of the solver's level matrices and transfers (its getters), made once per case
    -- every solver of a case has the same hierarchy -- with this solver's coarse solve."""
    if case not in _HIER:
        nl = mg.n_levels
        n = [mg.get_n_dofs(l) for l in range(nl)]
        A, P, R = [], [], []
        for l in range(nl):
            colptr, rowind, val = mg.get_coefficient_matrix(l)
            A.append(sp.csc_matrix((val, rowind, colptr), shape=(n[l], n[l])))
        for l in range(nl - 1):
            colptr, rowind, val = mg.get_transfer(l, "P")
            P.append(sp.csc_matrix((val, rowind, colptr), shape=(n[l], n[l + 1])))
            colptr, rowind, val = mg.get_transfer(l, "R")
            R.append(sp.csc_matrix((val, rowind, colptr), shape=(n[l + 1], n[l])))
        _HIER[case] = (FT.Hierarchy(A, P, R, SMOOTHERS[case](mg), None), A)
    H, A = _HIER[case]
    H.coarse = device_coarse(mg)
    return H, A


def check_path(amg, mg, case, H, A):
    """the path the case is named for was taken, by the getters that exist"""
    want = CASES[case][1]
    nl = mg.n_levels
    assert nl >= 2 and nl == want.get("levels", nl)
    said = []
    for l in range(nl - 1):
        layout, stream = mg.level_layout(l)
        assert layout == want["layout"], (case, l, layout)
        assert mg.level_transfer_kind(l) == want["kind"], (case, l)
        if layout == SELL:  # the index width shows in the bytes of the matrix stream: 8 + w per slot
            panels = (A[l].shape[0] + 63) // 64
            w = 4 if want.get("idx32") else 2
            slots, rest = divmod(stream - 8 * panels, 8 + w)
            assert rest == 0 and slots % 64 == 0, (case, l, stream, panels)
            if l == 0:  # the caller's matrix: no exact zeros, so the slot count is known
                assert slots == im.sell_slots(im.pruned(sp.csr_matrix(A[0]))), (case, stream, slots, panels)
    said.append(f"layout {im.LAYOUT_NAME[want['layout']]}" + (" 32-bit indices" if want.get("idx32") else ""))
    said.append(f"transfer kind {want['kind']}")
    if "passes" in want:
        assert H.passes() == want["passes"]
        said.append(f"{want['passes']} passes per smoothing")
    if "width" in want:
        assert max(R.w for R in H.rows) == want["width"]
        said.append(f"rows of up to {want['width']} entries")
    unsym = [l for l in range(nl - 1) if not H.symmetric(l)]  # no getter says it: printed, not required
    said.append(f"levels that are not bitwise symmetric: {unsym}")
    if want.get("unsym0"):
        csr = sp.csr_matrix(A[0])
        csr.sort_indices()
        assert not (np.array_equal(csr.indptr, A[0].indptr) and np.array_equal(csr.indices, A[0].indices) and
                    np.array_equal(csr.data, A[0].data))
        assert not H.symmetric(0)
        said.append("level 0 not symmetric: the CSC and CSR arrays differ")
    if "sides" in want:
        assert mg.natural_sides() == want["sides"]
        said.append(f"natural sides {want['sides']}")
    if "periodic" in want:
        assert mg.periodic_axes() == want["periodic"]
        assert [mg.level_axes(l) for l in range(nl - 1)] == want["axes"]
        assert all(want["periodic"] & a for a in want["axes"])  # a seam on every level
        said.append(f"periodic axes {want['periodic']}, level axes {want['axes']}")
    if "semi" in want:
        tw = S.case(*want["semi"])[2]
        axes = [mg.level_axes(l) for l in range(nl - 1)]
        full = S.full_mask(len(want["semi"][0]))
        assert nl == tw.nl and axes == tw.masks and any(a != full for a in axes)
        said.append(f"level axes {axes}")
    if want.get("ragged"):
        cnt = np.diff(sp.csr_matrix(A[0]).indptr)
        assert cnt.min() < cnt.max() and cnt.max() > 9
        said.append(f"row widths {cnt.min()} .. {cnt.max()}")
    if "n0" in want:
        assert mg.get_n_dofs(0) == want["n0"]
        said.append(f"n_h = {want['n0']} ({'odd' if want['n0'] & 1 else 'even'})")
    return ", ".join(said)


def rnd(rng, n):
    return rng.standard_normal(n).astype(np.float32)


def bits_equal(got, want, what):
    assert got.dtype == np.float32 and want.dtype == np.float32, what
    assert np.all(np.isfinite(want)), what
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (f"{what}: {bad.size} of {got.size} entries differ, first at {int(bad[0])}: "
                           f"device {got[bad[0]]!r} twin {want[bad[0]]!r}")


# ---- a. single steps on random data -----------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
def test_single_steps_have_the_twins_bits(amg, oracle, case):
    mg = make(amg, oracle, case)
    try:
        H, A = hierarchy(mg, case)
        path = check_path(amg, mg, case, H, A)
        nl = mg.n_levels
        rng = np.random.default_rng(nl * 1000 + H.n[0])
        done = []
        for l in range(nl - 1):
            u, f = rnd(rng, H.n[l]), rnd(rng, H.n[l])
            mg.f32_set_vec(l, "u", u)
            mg.f32_set_vec(l, "f", f)
            bits_equal(mg.f32_get_vec(l, "u"), u, (case, l, "set / get"))
            mg.f32_level_op(l, 0)
            u1 = H.smooth(l, u, f)
            bits_equal(mg.f32_get_vec(l, "u"), u1, (case, l, "op 0: u after the smoother"))
            bits_equal(mg.f32_get_vec(l, "f"), f, (case, l, "op 0: f unchanged"))
            assert not FT.same_bits(u1, u)
            mg.f32_level_op(l, 1)
            r = H.resid(l, u1, f)
            bits_equal(mg.f32_get_vec(l, "r"), r, (case, l, "op 1: r"))
            bits_equal(mg.f32_get_vec(l, "u"), u1, (case, l, "op 1: u unchanged"))
            mg.f32_set_vec(l + 1, "u", rnd(rng, H.n[l + 1]))  # op 2 has to zero it
            mg.f32_level_op(l, 2)
            bits_equal(mg.f32_get_vec(l + 1, "f"), H.restrict(l, r), (case, l, "op 2: f of the coarser level"))
            assert not np.any(mg.f32_get_vec(l + 1, "u").view(np.uint32)), (case, l, "op 2: u of the coarser level is +0.0")
            uH = rnd(rng, H.n[l + 1])
            mg.f32_set_vec(l + 1, "u", uH)
            mg.f32_level_op(l, 3)
            bits_equal(mg.f32_get_vec(l, "u"), H.prolong_add(l, uH, u1), (case, l, "op 3: u"))
            bits_equal(mg.f32_get_vec(l + 1, "u"), uH, (case, l, "op 3: u of the coarser level unchanged"))
            done.append(l)
        fL = rnd(rng, H.n[-1])
        mg.f32_set_vec(nl - 1, "f", fL)
        mg.f32_level_op(nl - 1, 4)
        bits_equal(mg.f32_get_vec(nl - 1, "u"), H.coarse_solve(fL), (case, nl - 1, "op 4: u"))
        bits_equal(mg.f32_get_vec(nl - 1, "f"), fL, (case, nl - 1, "op 4: f unchanged"))
        print(f"\n{case}: {path}; n = {H.n}; ops 0 1 2 3 bit for bit on levels {done}, op 4 on level {nl - 1}")
    finally:
        mg.close()


# ---- b. the whole cycle -----------------------------------------------------------------------------
def _apply(mg, v):
    dv = torch.from_numpy(np.array(v)).cuda()
    dz = torch.empty_like(dv)
    mg.apply_f32(dv.data_ptr(), dz.data_ptr())
    mg.sync()
    return dz.cpu().numpy()


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_cycle_leaves_the_twins_bits_on_every_level(amg, oracle, case):
    said = []
    for graph in (True, False):
        mg = make(amg, oracle, case, use_graph=graph)
        try:
            H, A = hierarchy(mg, case)
            check_path(amg, mg, case, H, A)
            nl = mg.n_levels
            v = np.random.default_rng(7).standard_normal(H.n[0])
            u, f, r = FT.cycle(H, v)
            assert np.linalg.norm(u[0]) > 0
            for call in ("first", "second"):
                z = _apply(mg, v)
                where = (case, "graph" if graph else "eager", call)
                for l in range(nl):
                    bits_equal(mg.f32_get_vec(l, "u"), u[l], where + (l, "u"))
                    bits_equal(mg.f32_get_vec(l, "f"), f[l], where + (l, "f"))
                    if l < nl - 1:
                        bits_equal(mg.f32_get_vec(l, "r"), r[l], where + (l, "r"))
                assert z.dtype == np.float64 and np.array_equal(z.view(np.uint64), u[0].astype(np.float64).view(np.uint64))
            said.append(f"{'graph' if graph else 'eager'}: u f r of levels 0 .. {nl - 2}, u f of level {nl - 1}, "
                        "z = widen(u_0), first and replayed call")
        finally:
            mg.close()
    print(f"\n{case}: " + "; ".join(said))


def test_the_comparison_sees_a_reversed_row_order(amg, oracle):
    """control: the device's residual on t33 has the ascending sum's bits and NOT the descending one's,
    so the bitwise comparison above would catch a kernel that summed a row the other way round"""
    mg = make(amg, oracle, "t33")
    try:
        H, A = hierarchy(mg, "t33")
        rng = np.random.default_rng(5)
        u, f = rnd(rng, H.n[0]), rnd(rng, H.n[0])
        mg.f32_set_vec(0, "u", u)
        mg.f32_set_vec(0, "f", f)
        mg.f32_level_op(0, 1)
        got = mg.f32_get_vec(0, "r")
        bits_equal(got, H.resid(0, u, f), "ascending")
        down = FT.residual(FT.Rows(sp.csr_matrix(A[0]), descending=True), u, f)
        differ = int(np.count_nonzero(got.view(np.uint32) != down.view(np.uint32)))
        print(f"\nt33 level 0 residual: the descending sum differs from the device in {differ} of {got.size} entries")
        assert differ >= 1
    finally:
        mg.close()


# ---- the hooks' own contract ------------------------------------------------------------------------
def test_the_hooks_refuse_what_a_level_does_not_have(amg, oracle):
    mg = make(amg, oracle, "t33")
    try:
        nl = mg.n_levels
        bad = [lambda: mg.f32_get_vec(nl - 1, "r"),
               lambda: mg.f32_set_vec(nl - 1, "r", np.zeros(mg.get_n_dofs(nl - 1), np.float32)),
               lambda: mg.f32_level_op(nl, 0), lambda: mg.f32_level_op(-1, 0), lambda: mg.f32_level_op(0, 5),
               lambda: mg.f32_level_op(0, 4)]
        bad += [lambda op=op: mg.f32_level_op(nl - 1, op) for op in range(4)]
        for call in bad:
            with pytest.raises(amg.AmgHipError) as err:
                call()
            assert err.value.status == amg.EINVAL
        with pytest.raises(ValueError):
            mg.f32_set_vec(0, "u", np.zeros(mg.get_n_dofs(0)))  # float64: the wrapper does not round
        # the solver's own vectors are not the float ones
        u0 = mg.get_soln(0)
        mg.f32_set_vec(0, "u", np.ones(mg.get_n_dofs(0), np.float32))
        assert np.array_equal(mg.get_soln(0), u0)
    finally:
        mg.close()
    # amg_hip_apply_f32's checks come first: a smoother without a float form, a dictionary level
    Ao = oracle.laplacian(64)
    spgs = amg.Multigrid(Ao.colptr, Ao.rowind, Ao.val, oracle.rhs(64), 3, layout=SELL)
    dct = amg.Multigrid(Ao.colptr, Ao.rowind, Ao.val, oracle.rhs(64), 3, layout=DICT, **JAC)
    try:
        assert dct.level_layout(0)[0] == DICT
        for m in (spgs, dct):
            for call in (lambda: m.f32_get_vec(0, "u"), lambda: m.f32_set_vec(0, "u", np.zeros(64 * 64, np.float32)),
                         lambda: m.f32_level_op(0, 0)):
                with pytest.raises(amg.AmgHipError) as err:
                    call()
                assert err.value.status == amg.EUNSUPPORTED
            # a bad argument is refused first
            for call in (lambda: m.f32_level_op(0, 7), lambda: m.f32_level_op(2, 0), lambda: m.f32_get_vec(2, "r")):
                with pytest.raises(amg.AmgHipError) as err:
                    call()
                assert err.value.status == amg.EINVAL
    finally:
        spgs.close()
        dct.close()
