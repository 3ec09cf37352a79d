"""Operator-dependent interpolation on tensor hierarchies (amg_hip_create_tensor_opdep), the parts that
need no GPU: on host_only solvers P against the weight rule of the numpy twin (tests/opdep_twin.py)
bit for bit, pattern and values, the level matrices against amg_hip_create_custom on the returned P / R
bit for bit, the automatic masks, the compact weights, every argument error -- and, on the twin alone,
the conditions that make the feature worth having: on coefficients that jump, the PCG count is at most
half of full coarsening's and of geometric interpolation's on the same masks."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "algebraic-multigrid_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import opdep_twin as O  # noqa: E402
import semi_twin as S  # noqa: E402
import tensor_twin as T  # noqa: E402

JAC = dict(smoother_iters=2, omega=0.8)
GRIDS = ((33, 20), (64, 48), (17, 12, 9), (2, 5), (3, 4), (5, 4, 3))
OPERATORS = ("jump", "diffusion", "nonsymmetric")


def csc(A):
    A = sp.csc_matrix(A)
    A.sort_indices()
    return A


def _same_triple(got, want):
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and
            np.array_equal(np.asarray(got[2]).view(np.uint64), np.asarray(want[2]).view(np.uint64)))


def operator(kind, dims):
    if kind == "jump":
        return O.jump(dims, contrast=4, seed=5)
    eps = (1.0, 1e-2, 0.3)[:len(dims)]
    A = S.diffusion(dims, eps, seed=7)
    return O.nonsymmetric(A, dims) if kind == "nonsymmetric" else A


def make(amg, A, b, dims, n_levels, masks=None, min_coarse=O.MIN_COARSE, **kw):
    A = csc(A)
    kw.setdefault("smoother", amg.SM_JACOBI)
    kw.setdefault("host_only", True)
    for k, v in JAC.items():
        kw.setdefault(k, v)
    return amg.Multigrid.tensor_opdep(A.indptr, A.indices, A.data, b, dims, n_levels, axis_masks=masks,
                                      min_coarse=min_coarse, **kw)


def level_matrix(mg, l):
    n = mg.get_n_dofs(l)
    return T.csr_of(*mg.get_coefficient_matrix(l), n, n)


def P_of_weights(dims, dim, mask, W):
    """The CSC triple of P from the compact weights, in plain loops (x fastest)."""
    d = T.dims3(dims)
    axis = O.axis_of(mask)
    m = d[axis]
    cd = S.coarse_dims(d, dim, mask)
    ed = list(d)
    ed[axis] = m - m // 2
    W = np.asarray(W).reshape(-1, 2)
    ptr, idx, val = [0], [], []
    for K in range(cd[2]):
        for J in range(cd[1]):
            for I in range(cd[0]):
                H = [I, J, K]
                for t in range(3):
                    f = list(H)
                    f[axis] = 2 * H[axis] + t
                    if f[axis] >= m:
                        continue
                    idx.append((f[2] * d[1] + f[1]) * d[0] + f[0])
                    if t == 1:
                        val.append(1.0)
                    else:
                        e = list(H)
                        e[axis] = H[axis] + t // 2
                        val.append(W[(e[2] * ed[1] + e[1]) * ed[0] + e[0], 1 - t // 2])
                ptr.append(len(idx))
    return np.array(ptr, np.int32), np.array(idx, np.int32), np.array(val, np.float64)


def check_against_the_rule(amg, mg, A, b, dims):
    """Every level's P / R are the rule applied to that level's own matrix, the compact weights round-trip
    into P, and the level matrices are amg_hip_create_custom's on these P / R, bit for bit."""
    dim, nl = len(dims), mg.n_levels
    transfers = []
    for l in range(nl - 1):
        mask = mg.level_axes(l)
        d = mg.level_dims(l)
        P, W = O.opdep_P(level_matrix(mg, l), d, dim, mask)
        got = mg.get_transfer(l, "P")
        assert _same_triple(got, (P.indptr, P.indices, P.data)), (l, "P")
        # the pattern is the semi-coarsening P's for the same mask
        G = S.semi_P(d, dim, mask)
        assert np.array_equal(got[0], G.indptr) and np.array_equal(got[1], G.indices), l
        R = sp.csc_matrix((got[2], got[1], got[0]), shape=P.shape).T.tocsc()
        R.sort_indices()
        assert _same_triple(mg.get_transfer(l, "R"), (R.indptr, R.indices, R.data)), (l, "R")
        Wl = mg.axis_weights(l)
        assert Wl.shape == (mg.get_n_dofs(l) - mg.get_n_dofs(l + 1), 2)
        assert np.array_equal(Wl.view(np.uint64), W.view(np.uint64)), l
        assert _same_triple(P_of_weights(d, dim, mask, Wl), got), (l, "weights -> P")
        assert mg.level_dims(l + 1) == S.coarse_dims(d, dim, mask)
        transfers.append((got, mg.get_transfer(l, "R")))
    with pytest.raises(ValueError):
        mg.axis_weights(nl - 1)
    A0 = csc(A)
    cu = amg.Multigrid(A0.indptr, A0.indices, A0.data, b, nl, smoother=amg.SM_JACOBI, transfers=transfers,
                       host_only=True, **JAC)
    for l in range(nl):
        assert cu.get_n_dofs(l) == mg.get_n_dofs(l), l
        assert _same_triple(mg.get_coefficient_matrix(l), cu.get_coefficient_matrix(l)), l
    cu.close()


def single_axis_chains(dims):
    """Every single axis alone, and the longest chain that cycles through the axes (down to a level of 3
    rows: amg_hip_create_custom, the yardstick of the level matrices, coarsens no level of 2 rows)."""
    dim = len(dims)
    out = [(1 << a,) for a in range(dim)]
    d, chain, a, idle = list(dims), [], 0, 0
    while idle < dim and len(chain) < 8 and int(np.prod(d)) >= 3:
        if d[a] >= 2:
            chain.append(1 << a)
            d[a] //= 2
            idle = 0
        else:
            idle += 1
        a = (a + 1) % dim
    return out + [tuple(chain)]


@pytest.mark.parametrize("kind", OPERATORS)
@pytest.mark.parametrize("dims", GRIDS)
def test_explicit_masks_against_the_twin(amg, dims, kind):
    A = operator(kind, dims)
    b = S.rhs(A.shape[0], seed=8)
    for masks in single_axis_chains(dims):
        mg = make(amg, A, b, dims, len(masks) + 1, masks, min_coarse=0)  # min_coarse is ignored
        assert mg.n_levels == len(masks) + 1
        assert [mg.level_axes(l) for l in range(len(masks))] == list(masks)
        assert [mg.level_transfer_kind(l) for l in range(len(masks))] == [3] * len(masks)
        check_against_the_rule(amg, mg, A, b, dims)
        # level 0 of the twin is bit for bit the library's (deeper levels follow scipy's product order)
        tw = O.OpdepTwin(A, dims, masks=masks[:1])
        assert _same_triple(mg.get_transfer(0, "P"), T.csc_triple(tw.P[0]))
        mg.close()
    k0 = make(amg, A, b, dims, 2, (1,), stencil_transfers=False)
    assert k0.level_transfer_kind(0) == 0
    k0.close()


@pytest.mark.parametrize("kind", OPERATORS)
@pytest.mark.parametrize("dims", GRIDS)
def test_automatic_rule_against_the_twin(amg, dims, kind):
    A = operator(kind, dims)
    b = S.rhs(A.shape[0], seed=8)
    mg = make(amg, A, b, dims, O.MAX_LEVELS)
    tw = O.OpdepTwin(A, dims)
    assert mg.n_levels == tw.nl
    assert [mg.level_axes(l) for l in range(tw.nl - 1)] == tw.masks
    assert [mg.level_dims(l) for l in range(tw.nl)] == tw.dims
    # the rule on the library's own level matrices, so that no rounding of the twin's products enters
    for l in range(mg.n_levels - 1):
        d = mg.level_dims(l)
        assert mg.level_axes(l) == O.auto_mask(d, len(dims), S.axis_strength(level_matrix(mg, l), d)), l
    check_against_the_rule(amg, mg, A, b, dims)
    for l in range(tw.nl):  # the twin's hierarchy is the library's up to the rounding of the products
        M, Tm = level_matrix(mg, l), tw.A[l]
        assert abs(M - Tm).max() <= 1e-12 * abs(Tm).max(), l
    ex = make(amg, A, b, dims, tw.nl, tw.masks)  # the same hierarchy as the explicit constructor
    for l in range(tw.nl):
        assert _same_triple(mg.get_coefficient_matrix(l), ex.get_coefficient_matrix(l)), l
    ex.close()
    mg.close()


NAMES = {1: "x", 2: "y", 4: "z"}


def test_automatic_masks_where_they_are_known(amg, oracle):
    # isotropic square: x first (the lowest axis on the tie), then y, and every further pair of levels
    # coarsens each axis once.  Strict alternation x y x y does not follow from the rule: after x and y
    # the interior couplings tie (0.5 each), but w is a maximum over ALL rows and the rows next to the
    # Dirichlet sides decide it (w = 0.5, 0.546875 on level 2 of this grid), so level 2 takes y, level 3 x.
    L = oracle.laplacian(16)
    A = T.csr_of(L.colptr, L.rowind, L.val, 256, 256)
    mg = amg.Multigrid.tensor_opdep(L.colptr, L.rowind, L.val, oracle.rhs(16), (16, 16), 16, min_coarse=4,
                                    host_only=True, smoother=amg.SM_JACOBI, **JAC)
    got = "".join(NAMES[mg.level_axes(l)] for l in range(mg.n_levels - 1))
    assert got == "xyyxxy" and mg.get_n_dofs(mg.n_levels - 1) == 4, got
    assert all(sorted(got[k:k + 2]) == ["x", "y"] for k in range(0, len(got), 2))
    # on amg.laplacian the P of level 0 is semi_P of the same mask bit for bit on every grid line but the
    # two next to the y sides: there the Dirichlet term stays on the diagonal, the collapsed s_0 is
    # -3 h^-2 instead of -2 h^-2, and the rule gives 1 / 3 where P1 has 1 / 2 (pattern unchanged)
    assert _same_triple((L.colptr, L.rowind, L.val), amg.laplacian(16))
    got, geo = mg.get_transfer(0, "P"), T.csc_triple(S.semi_P((16, 16), 2, 1))
    assert np.array_equal(got[0], geo[0]) and np.array_equal(got[1], geo[1])
    side = np.isin(got[1] // 16, (0, 15))
    assert np.array_equal(got[2][~side].view(np.uint64), geo[2][~side].view(np.uint64))
    third = np.float64(72.25) / np.float64(216.75)
    assert set(got[2][side]) == {1.0, third} and np.count_nonzero(got[2][side] == third) == 30
    assert O.OpdepTwin(A, (16, 16), min_coarse=4).masks == [mg.level_axes(l) for l in range(mg.n_levels - 1)]
    mg.close()
    # the strong axis first on the anisotropic cases
    for dims, eps, first in (((64, 48), (1.0, 1e-2), "xxxx"), ((17, 12, 9), (1e-3, 1.0, 1e-3), "yyy")):
        A = S.diffusion(dims, eps)
        mg = make(amg, A, S.rhs(A.shape[0]), dims, O.MAX_LEVELS)
        got = "".join(NAMES[mg.level_axes(l)] for l in range(mg.n_levels - 1))
        assert got.startswith(first), got
        assert [mg.level_axes(l) for l in range(mg.n_levels - 1)] == O.OpdepTwin(A, dims).masks
        mg.close()
    # min_coarse and n_levels end the hierarchy
    A = O.jump((33, 20))
    mg = make(amg, A, np.ones(660), (33, 20), 16, min_coarse=200)
    assert [mg.get_n_dofs(l) for l in range(mg.n_levels)] == [660, 320, 160]
    mg.close()
    mg = make(amg, A, np.ones(660), (33, 20), 2)
    assert mg.n_levels == 2
    mg.close()
    one = amg.Multigrid.tensor_opdep(np.array([0, 1], np.int32), np.array([0], np.int32), np.array([2.0]),
                                     np.ones(1), (1, 1), 5, min_coarse=1, host_only=True)
    assert one.n_levels == 1
    one.close()


def test_weights_are_what_the_issue_says(amg):
    """P1 in the interior of a constant-coefficient operator, 1.0 at a side without a Dirichlet term, and
    k- / (k- + k+), k+ / (k- + k+) across a jump."""
    mg = make(amg, O.jump((24, 3), block=8, contrast=3, seed=11, natural=True, shift=1e-3), np.ones(72), (24, 3), 2, (1,))
    W = mg.axis_weights(0).reshape(3, 12, 2)
    kb = O.jump((24, 3), block=8, contrast=3, seed=11, natural=True)
    for j in range(3):
        row = j * 24
        assert W[j, 0, 0] == 0.0 and abs(W[j, 0, 1] - 1.0) < 1e-3  # the natural low side
        for q in range(1, 12):
            c = 2 * q
            km, kp = -kb[row + c, row + c - 1], -kb[row + c, row + c + 1]
            assert abs(W[j, q, 0] - km / (km + kp)) < 1e-3 and abs(W[j, q, 1] - kp / (km + kp)) < 1e-3
    mg.close()


def _raw(amg, A, b, dim, dims3, levels, masks, min_coarse=32, window=0, **opt):
    A = csc(A)
    o = amg.Options()
    amg.lib().amg_hip_default_options(C.byref(o))
    o.host_only = 1
    o.window = window
    for k, v in opt.items():
        setattr(o, k, v)
    h = C.c_void_p()
    d = np.array(dims3, np.int64)
    i32, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    cp, ri, v, b = (np.ascontiguousarray(A.indptr, np.int32), np.ascontiguousarray(A.indices, np.int32),
                    np.ascontiguousarray(A.data, np.float64), np.ascontiguousarray(b, np.float64))
    m = None if masks is None else np.ascontiguousarray(masks, np.int32)
    st = amg.lib().amg_hip_create_tensor_opdep(A.shape[0], cp.ctypes.data_as(i32), ri.ctypes.data_as(i32),
                                               v.ctypes.data_as(f64), b.ctypes.data_as(f64), dim,
                                               d.ctypes.data_as(C.POINTER(C.c_int64)), levels,
                                               None if m is None else m.ctypes.data_as(i32), min_coarse,
                                               C.byref(o), C.byref(h))
    msg = amg.lib().amg_hip_last_error().decode()
    if st == 0:
        amg.lib().amg_hip_destroy(h)
    return st, msg


def test_argument_errors(amg, oracle):
    A = O.jump((12, 10))
    b = np.ones(120)
    A3 = O.jump((4, 3, 2))
    b3 = np.ones(24)
    assert _raw(amg, A, b, 2, (12, 10, 1), 3, [1, 2])[0] == 0
    for masks, level, word in (([0, 1], 0, "no axis"), ([1, 0], 1, "no axis"), ([4, 1], 0, "z"),
                               ([3, 1], 0, "several"), ([1, 3], 1, "several"), ([8, 1], 0, "bits"),
                               ([-1, 1], 0, "bits"), ([2, 6], 1, "z")):
        st, msg = _raw(amg, A, b, 2, (12, 10, 1), 3, masks)
        assert st == amg.EINVAL and f"level {level}" in msg and word in msg, (masks, msg)
        assert "amg_hip_create_tensor_opdep" in msg
    for masks, level in (([5, 1], 0), ([1, 6], 1), ([7, 1], 0)):
        st, msg = _raw(amg, A3, b3, 3, (4, 3, 2), 3, masks)
        assert st == amg.EINVAL and f"level {level}" in msg and "several" in msg, (masks, msg)
    # a masked axis shorter than 2: y of 10 -> 5 -> 2 -> 1
    st, msg = _raw(amg, A, b, 2, (12, 10, 1), 5, [2, 2, 2, 2])
    assert st == amg.EINVAL and "level 3" in msg and "axis y" in msg, msg
    st, msg = _raw(amg, A3, b3, 3, (4, 3, 2), 3, [4, 4])
    assert st == amg.EINVAL and "level 1" in msg and "axis z" in msg, msg
    # the automatic rule's parameter; explicit masks ignore it
    st, msg = _raw(amg, A, b, 2, (12, 10, 1), 3, None, min_coarse=0)
    assert st == amg.EINVAL and "min_coarse" in msg
    assert _raw(amg, A, b, 2, (12, 10, 1), 3, None, min_coarse=1)[0] == 0
    assert _raw(amg, A, b, 2, (12, 10, 1), 3, [1, 2], min_coarse=0)[0] == 0
    # the grid, in the words of amg_hip_create_tensor_semi
    assert _raw(amg, A, b, 2, (12, 11, 1), 2, [1])[0] == amg.EINVAL
    assert _raw(amg, A, b, 2, (12, 5, 2), 2, [1])[0] == amg.EINVAL
    assert _raw(amg, A, b, 4, (12, 10, 1), 2, [1])[0] == amg.EINVAL
    assert _raw(amg, A, b, 2, (12, 10, 1), 0, None)[0] == amg.EINVAL
    st, msg = _raw(amg, A, b, 2, (12, 10, 1), 2, [1], window=1)
    assert st == amg.EUNSUPPORTED and "amg_hip_create_tensor_opdep" in msg
    # natural_sides is validated and reported; singular needs every side
    st, msg = _raw(amg, A, b, 2, (12, 10, 1), 2, [1], natural_sides=16)
    assert st == amg.EINVAL and "natural_sides" in msg
    st, msg = _raw(amg, A, b, 2, (12, 10, 1), 2, [1], natural_sides=3, singular=1)
    assert st == amg.EINVAL and "singular" in msg
    N = O.jump((12, 10), natural=True)
    assert _raw(amg, N, b, 2, (12, 10, 1), 3, [1, 2], natural_sides=15, singular=1)[0] == 0
    M = csc(N)
    mg = amg.Multigrid.tensor_opdep(M.indptr, M.indices, M.data, b, (12, 10), 3, natural_sides=5, host_only=True)
    assert mg.natural_sides() == 5
    mg.close()
    # a row whose collapsed s_0 is zero: row 14 = (x 2, y 1); collapsed onto x, its entries in the
    # columns 2, 14, 26 (added in that order) cancel
    def entry(i, j, v):
        Z = sp.csr_matrix(A, copy=True)
        Z.sort_indices()
        k = Z.indptr[i] + int(np.searchsorted(Z.indices[Z.indptr[i]:Z.indptr[i + 1]], j))
        assert Z.indices[k] == j
        Z.data[k] = v
        return Z
    st, msg = _raw(amg, entry(14, 14, -(A[14, 2] + A[14, 26])), b, 2, (12, 10, 1), 3, [1, 2])
    assert st == amg.EINVAL and "level 0" in msg and "row 14" in msg and "s_0" in msg, msg
    # ... and on level 1: a diagonal matrix on the 4 x 2 grid, masks x then y.  Row 1 = (x 1, y 0) has an
    # odd x, carries no weights on level 0 and becomes row 0 of the 2 x 2 level 1, where y = 0 is even
    D = sp.csr_matrix((np.array([2.0, 0.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0]), np.arange(8), np.arange(9)), shape=(8, 8))
    st, msg = _raw(amg, D, np.ones(8), 2, (4, 2, 1), 3, [1, 2])
    assert st == amg.EINVAL and "level 1" in msg and "row 0" in msg and "s_0" in msg, msg
    # collapsed onto y, the columns 13, 14, 15 of row 14 hold s_0; row 14 has the odd y = 1 and carries
    # no weights along y, so the same matrix passes with the mask y
    assert _raw(amg, entry(14, 14, -(A[14, 13] + A[14, 15])), b, 2, (12, 10, 1), 2, [2])[0] == 0
    # a weight that is not finite
    st, msg = _raw(amg, entry(14, 15, np.inf), b, 2, (12, 10, 1), 2, [1])
    assert st == amg.EINVAL and "level 0" in msg and "row 14" in msg and "w_hi" in msg, msg
    st, msg = _raw(amg, entry(14, 14, np.nan), b, 2, (12, 10, 1), 2, [1])
    assert st == amg.EINVAL and "level 0" in msg and "row 14" in msg and "s_0" in msg, msg
    # every smoother builds, the alternating line smoother included (the level grids are known)
    M = csc(A)
    for sm in (amg.SM_SPGS, amg.SM_REF_JACOBI, amg.SM_SOR, amg.SM_JACOBI, amg.SM_MULTICOLOR_GS,
               amg.SM_CHEBYSHEV, amg.SM_LINE_JACOBI, amg.SM_LINE_ALT):
        mg = amg.Multigrid.tensor_opdep(M.indptr, M.indices, M.data, b, (12, 10), 4, axis_masks=(1, 1, 1),
                                        host_only=True, smoother=sm, omega=0.7)
        assert mg.level_dims(3) == (1, 10, 1)
        if sm == amg.SM_LINE_ALT:
            assert mg.line_directions(0) == [1, 12] and mg.line_directions(3) == [1]
        mg.close()
    with pytest.raises(ValueError, match="n_levels - 1"):
        amg.Multigrid.tensor_opdep(M.indptr, M.indices, M.data, b, (12, 10), 4, axis_masks=(1, 1), host_only=True)
    # the weights belong to these solvers
    semi = amg.Multigrid.tensor_semi(M.indptr, M.indices, M.data, b, (12, 10), 2, axis_masks=(1,), host_only=True)
    with pytest.raises(ValueError, match="amg_hip_create_tensor_opdep"):
        semi.axis_weights(0)
    semi.close()
    # the stand-alone transfers check their grid and axis before they look for a device
    for axis in (-1, 2, 3):
        with pytest.raises(ValueError):
            amg.axis_restrict((12, 10), axis, np.zeros(2 * 60), np.ones(120))
    with pytest.raises(ValueError, match="axis x"):
        amg.axis_prolong_add((1, 10), 0, np.zeros(20), np.ones(0), np.ones(10))


def test_the_switch_selects_kind_0(amg):
    A = O.jump((12, 10))
    try:
        amg.set_axis_stencil(False)
        mg = make(amg, A, np.ones(120), (12, 10), 3, (1, 2))
        assert [mg.level_transfer_kind(l) for l in range(2)] == [0, 0]
        mg.close()
    finally:
        amg.set_axis_stencil(True)
    mg = make(amg, A, np.ones(120), (12, 10), 3, (1, 2))
    assert [mg.level_transfer_kind(l) for l in range(2)] == [3, 3]
    mg.close()


def test_twin_opdep_halves_the_pcg_count_on_jumps():
    """Conditions on the inputs, on the twin alone (true Jacobi 0.8, 2 + 2, PCG to 1e-8).  Measured:
    jump((128, 128), 4): opdep 15, geometric weights on the same masks 51, full coarsening 59, operator
    complexity 2.62; jump((64, 48), 4): opdep 10."""
    A, b, tw = O.case((128, 128))
    op = tw.pcg(b, 1e-8)[1]
    geo = O.OpdepTwin(A, (128, 128), masks=tw.masks, geometric=True).pcg(b, 1e-8)[1]
    full = S.full_twin(A, (128, 128)).pcg(b, 1e-8)[1]
    print("128^2: opdep", op, "geometric", geo, "full", full, "complexity", tw.complexity())
    assert 2 * op <= full and 2 * op <= geo, (op, geo, full)
    A, b, tw = O.case((64, 48))
    op = tw.pcg(b, 1e-8)[1]
    print("64x48: opdep", op)
    assert op <= 12, op


@pytest.mark.parametrize("dims,eps", (((64, 48), (1.0, 1e-2)), ((17, 12, 9), (1e-3, 1.0, 1e-3))))
def test_twin_opdep_is_no_worse_than_semi_coarsening_on_smooth_coefficients(dims, eps):
    """Measured: (64, 48) opdep 6 against semi 11; (17, 12, 9) opdep 6 against semi 11."""
    A, b, semi = S.case(dims, eps)
    op = O.OpdepTwin(A, dims).pcg(b, 1e-8)[1]
    se = semi.pcg(b, 1e-8)[1]
    print(dims, "opdep", op, "semi", se)
    assert op <= se, (op, se)


DROPIN_SRC = r"""
#include <cstdlib>
#include <iostream>
#include <amg/grid.hpp>
#include <amg/interpolator.hpp>
#include <amg/multigrid.hpp>
#include <amg/smoother.hpp>

int main(int argc, char** argv) {
  AMG::OpdepTensorInterpolator<double> rule(12, 10);
  if (!rule.masks().empty() || rule.min_coarse() != 32 || rule.dim() != 2) return 2;
  int threw = 0;
  try { rule.make_operators(120, 60, 0); } catch (const std::logic_error&) { ++threw; }
  if (threw != 1) return 3;
  if (argc < 2) { std::cout << "constructed" << std::endl; return 0; }  // CPU: no device
  const int N = std::atoi(argv[1]);
  Eigen::SparseMatrix<double> A = AMG::Grid<double>::laplacian(N);
  Eigen::VectorXd b = AMG::Grid<double>::rhs(N);
  AMG::OpdepTensorInterpolator<double> interp(N, N, 1, {1, 2, 1, 2});
  AMG::TrueJacobi<double> jac(0.8, 2);
  AMG::Multigrid<double> mg(&interp, &jac, A, b, 5, 1e-9, 5, 50);
  const int32_t want[4] = {1, 2, 1, 2};
  for (int l = 0; l < 4; ++l) {
    int32_t kind = -1, mask = -1;
    if (amg_hip_level_transfer_kind(mg.native_handle(), l, &kind) != AMG_HIP_OK || kind != 3) return 4;
    if (amg_hip_get_level_axes(mg.native_handle(), l, &mask) != AMG_HIP_OK || mask != want[l]) return 5;
  }
  if (mg.get_n_levels() != 5 || (long)interp.get_P(0).rows() != (long)N * N ||
      (long)interp.get_P(0).cols() != (long)(N / 2) * N || (long)interp.get_P(1).cols() != (long)(N / 2) * (N / 2) ||
      (long)mg.get_n_dofs(4) != (long)(N / 4) * (N / 4))
    return 6;
  bool refused = false;
  try {
    AMG::OpdepTensorInterpolator<double> bad(N, N, 1, {1, 3});
    AMG::Multigrid<double> no(&bad, &jac, A, b, 3, 1e-9, 5, 50);
  } catch (const std::invalid_argument&) { refused = true; }
  if (!refused) return 7;
  const double r0 = AMG::rss(A, mg.get_soln(0), b);
  for (int i = 0; i < 6; ++i) mg.vcycle();
  const double r6 = AMG::rss(A, mg.get_soln(0), b);
  std::cout.precision(17);
  std::cout << "drop6 " << r6 / r0 << std::endl;
  return r6 < 1e-4 * r0 ? 0 : 1;
}
"""


def build_dropin(amg, tmp_path):
    src = tmp_path / "opdep_dropin.cpp"
    src.write_text(DROPIN_SRC)
    exe = tmp_path / "opdep_dropin"
    pkg = os.path.dirname(amg.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe), "-L" + pkg, "-lamg_hip", "-Wl,-rpath," + pkg,
                           "-Wl,-rpath,/opt/rocm/lib"])
    return str(exe)


def test_dropin_opdep_interpolator_compiles_and_constructs(amg, tmp_path):
    exe = build_dropin(amg, tmp_path)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "constructed" in p.stdout, p.stdout + p.stderr
