"""Periodic axes of the tensor hierarchies (amg_hip_create_tensor_periodic), the parts that need no
GPU: on host_only solvers level dims, masks and P / R against the Kronecker products of the scipy twin
(tests/periodic_twin.py) entry for entry, the level matrices against amg_hip_create_custom on the
twin's operators bit for bit, P 1 = 1 on all-periodic boxes, periodic_axes = 0 against
Multigrid.tensor / tensor_semi, the getter, and every refusal with the argument's name in the
message."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "algebraic-multigrid_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import natural_twin as N  # noqa: E402
import periodic_twin as PT  # noqa: E402
import semi_twin as S  # noqa: E402
import tensor_twin as T  # noqa: E402

JAC = dict(smoother_iters=2, omega=0.8)

# (dims, periodic axes, natural sides, masks or None, levels): the sides of the axes that are not
# periodic are Dirichlet unless named in `natural sides`
CHAINS = [((4, 4), 3, 0, None, 2), ((6, 4), 3, 0, None, 2), ((8, 6), 3, 0, None, 2), ((8, 6), 1, 0, (1, 1), 3),
          ((5, 4), 2, 0, None, 2), ((5, 4), 2, 3, None, 2), ((33, 20), 2, 2, None, 3), ((33, 20), 2, 2, (2, 3, 1), 4),
          ((64, 48), 3, 0, None, 5), ((64, 48), 1, 12, None, 5), ((64, 48), 1, 0, None, 5),
          ((4, 4, 4), 7, 0, None, 2), ((6, 4, 3), 3, 0, None, 2), ((6, 4, 3), 3, 48, (3,), 2),
          ((16, 12, 8), 7, 0, None, 3), ((16, 12, 8), 5, 12, (5, 7), 3), ((16, 12, 9), 3, 48, None, 3)]


def csc(A):
    A = sp.csc_matrix(A)
    A.sort_indices()
    return A


def _same_triple(got, want):
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and
            np.array_equal(np.asarray(got[2]).view(np.uint64), np.asarray(want[2]).view(np.uint64)))


def problem(dims, per, sides):
    """(A, b, singular): Dirichlet on the sides that are neither periodic nor natural."""
    dim = len(dims)
    dirichlet = PT.open_sides(dim, per) & ~sides
    A = PT.diffusion(dims, per, dirichlet)
    return A, PT.rhs(A.shape[0], dirichlet == 0), dirichlet == 0


def make(amg, A, b, dims, n_levels, per, masks=None, **kw):
    A = csc(A)
    kw.setdefault("smoother", amg.SM_JACOBI)
    for k, v in JAC.items():
        kw.setdefault(k, v)
    return amg.Multigrid.tensor_periodic(A.indptr, A.indices, A.data, b, dims, n_levels, per, axis_masks=masks,
                                         host_only=True, **kw)


def test_P1per_is_the_definition():
    for m in (4, 6, 8, 20):
        P = PT.P1per(m).toarray()
        want = np.zeros((m, m // 2))
        for j in range(m // 2):
            want[2 * j, j], want[2 * j + 1, j], want[(2 * j + 2) % m, j] = 0.5, 1.0, 0.5
        assert np.array_equal(P, want)
        assert np.array_equal(P.sum(axis=1), np.ones(m))
        extra = P - T.P1(m).toarray()
        assert np.count_nonzero(extra) == 1 and extra[0, m // 2 - 1] == 0.5


@pytest.mark.parametrize("dims,per,sides,masks,nl", CHAINS)
def test_hierarchy_equals_the_twin_and_create_custom(amg, dims, per, sides, masks, nl):
    """Dims, masks, transfers (both transfer kinds) and level matrices of the whole chain, the matrices
    bit for bit with amg_hip_create_custom on the twin's P and R."""
    dim = len(dims)
    A, b, singular = problem(dims, per, sides)
    tw = PT.PeriodicTwin(A, dims, nl, masks=masks, sides=sides, periodic=per, singular=singular)
    transfers = []
    for st in (True, False):
        mg = make(amg, A, b, dims, nl, per, masks, natural_sides=sides, singular=singular, stencil_transfers=st)
        assert mg.n_levels == nl and mg.periodic_axes() == per and mg.natural_sides() == sides
        assert [mg.level_dims(l) for l in range(nl)] == tw.dims
        for l in range(nl - 1):
            assert mg.level_axes(l) == tw.masks[l] and mg.level_transfer_kind(l) == (2 if st else 0)
            P = PT.periodic_P(tw.dims[l], dim, tw.masks[l], sides, per)
            assert set(np.unique(P.data)) <= {2.0 ** -k for k in range(dim + 1)}
            got = mg.get_transfer(l, "P")
            for c in range(P.shape[1]):  # the rows of every column ascend: the wrapped row comes first
                assert np.all(np.diff(got[1][got[0][c]:got[0][c + 1]]) > 0), (l, c)
            assert _same_triple(got, T.csc_triple(P)), (l, st, "P")
            assert _same_triple(mg.get_transfer(l, "R"), T.csc_triple(P.T)), (l, st, "R")
            if st:
                transfers.append((T.csc_triple(P), T.csc_triple(P.T)))
        if st:
            keep = mg
        else:
            for l in range(nl):
                assert _same_triple(mg.get_coefficient_matrix(l), keep.get_coefficient_matrix(l)), l
            mg.close()
    mg = keep
    A0 = csc(A)
    cu = amg.Multigrid(A0.indptr, A0.indices, A0.data, b, nl, smoother=amg.SM_JACOBI, transfers=transfers,
                       host_only=True, **JAC)
    assert cu.periodic_axes() == 0
    for l in range(nl):
        assert cu.get_n_dofs(l) == mg.get_n_dofs(l) == tw.n[l], l
        assert _same_triple(mg.get_coefficient_matrix(l), cu.get_coefficient_matrix(l)), l
        M = mg.get_coefficient_matrix(l)
        got = sp.csc_matrix((M[2], M[1], M[0]), shape=(tw.n[l], tw.n[l]))
        # the twin's product adds in scipy's order: rounding relative to the entries that went in
        assert abs(got - tw.A[l]).max() <= 1e-13 * max(abs(tw.A[k]).max() for k in range(l + 1)), l
    if singular:  # the constants stay in the null space of every level
        M = mg.get_coefficient_matrix(nl - 1)
        Ac = sp.csc_matrix((M[2], M[1], M[0]), shape=(tw.n[-1], tw.n[-1]))
        assert np.abs(Ac @ np.ones(tw.n[-1])).max() <= 1e-12 * abs(tw.A[0]).max()
    cu.close()
    mg.close()


@pytest.mark.parametrize("dims,nl", [((4, 4), 2), ((6, 4), 2), ((8, 6), 2), ((64, 48), 5), ((4, 4, 4), 2),
                                     ((16, 12, 8), 3)])
def test_P_reproduces_the_constants_on_periodic_boxes(amg, dims, nl):
    dim = len(dims)
    per = PT.all_axes(dim)
    A, b, singular = problem(dims, per, 0)
    assert singular
    mg = make(amg, A, b, dims, nl, per, singular=True)
    for l in range(nl - 1):
        cp, ri, v = mg.get_transfer(l, "P")
        P = sp.csc_matrix((v, ri, cp), shape=(mg.get_n_dofs(l), mg.get_n_dofs(l + 1)))
        assert np.array_equal(P @ np.ones(P.shape[1]), np.ones(P.shape[0])), l
    mg.close()


@pytest.mark.parametrize("dims,masks,nl,sides", [((33, 20), None, 4, 0), ((33, 20), None, 4, 6),
                                                 ((17, 12, 9), (3, 6, 5), 4, 0), ((17, 12, 9), (3, 6, 5), 4, 63)])
def test_mask_zero_is_the_tensor_constructors_solver(amg, dims, masks, nl, sides):
    dim = len(dims)
    A = csc(N.diffusion(dims, N.all_sides(dim) & ~sides))
    b = N.rhs(A.shape[0], N.all_sides(dim) & ~sides)
    kw = dict(host_only=True, smoother=amg.SM_JACOBI, natural_sides=sides, singular=sides == N.all_sides(dim), **JAC)
    if masks is None:
        old = amg.Multigrid.tensor(A.indptr, A.indices, A.data, b, dims, nl, **kw)
    else:
        old = amg.Multigrid.tensor_semi(A.indptr, A.indices, A.data, b, dims, nl, axis_masks=masks, **kw)
    new = amg.Multigrid.tensor_periodic(A.indptr, A.indices, A.data, b, dims, nl, 0, axis_masks=masks, **kw)
    assert old.periodic_axes() == new.periodic_axes() == 0 and new.n_levels == old.n_levels == nl
    for l in range(nl):
        assert old.level_dims(l) == new.level_dims(l)
        assert _same_triple(old.get_coefficient_matrix(l), new.get_coefficient_matrix(l)), l
    for l in range(nl - 1):
        assert old.level_axes(l) == new.level_axes(l)
        for which in "PR":
            assert _same_triple(old.get_transfer(l, which), new.get_transfer(l, which)), (l, which)
    old.close()
    new.close()


def _raw(amg, ctor, dims, per, n_levels=2, masks=None, natural_sides=0, singular=0, window=0, n=None):
    """status and message of the periodic constructor `ctor` ("host" / "dev"), host_only.  The _dev
    form gets fake device pointers: the argument errors return before any device call."""
    i32, i64, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
    dim = len(dims)
    A = csc(PT.diffusion(dims, 0, N.all_sides(dim)) if min(dims) >= 2 else sp.identity(int(np.prod(dims))))
    nn =A.shape[0] if n is None else n
    b = np.ones(A.shape[0])
    o = amg.Options()
    L = amg.lib()
    L.amg_hip_default_options(C.byref(o))
    o.host_only = 1
    o.smoother, o.smoother_iters, o.omega = amg.SM_JACOBI, 2, 0.8
    o.natural_sides, o.singular, o.window = natural_sides, singular, window
    h = C.c_void_p()
    d = np.array(T.dims3(dims), np.int64)
    cp, ri, v = (np.ascontiguousarray(A.indptr, np.int32), np.ascontiguousarray(A.indices, np.int32),
                 np.ascontiguousarray(A.data, np.float64))
    m = None if masks is None else np.ascontiguousarray(masks, np.int32)
    mp = None if m is None else m.ctypes.data_as(i32)
    if ctor == "host":
        st = L.amg_hip_create_tensor_periodic(nn, cp.ctypes.data_as(i32), ri.ctypes.data_as(i32),
                                              v.ctypes.data_as(f64), b.ctypes.data_as(f64), dim,
                                              d.ctypes.data_as(i64), per, n_levels, mp, C.byref(o), C.byref(h))
    else:
        fake = (C.c_void_p(8),) * 4
        st = L.amg_hip_create_tensor_periodic_dev(nn, *fake, dim, d.ctypes.data_as(i64), per, n_levels, mp,
                                                  C.byref(o), C.byref(h))
    msg = L.amg_hip_last_error().decode()
    if st == 0:
        L.amg_hip_destroy(h)
    return st, msg


@pytest.mark.parametrize("ctor", ("host", "dev"))
def test_refusals_name_the_argument(amg, ctor):
    E = amg.EINVAL
    # periodic_axes itself
    for dims, bad in (((8, 6), 4), ((8, 6), 7), ((8, 6), -1), ((8, 6), 8), ((8, 6, 4), 8), ((8, 6, 4), -8)):
        st, msg = _raw(amg, ctor, dims, bad)
        assert st == E and "periodic_axes" in msg, (dims, bad, msg)
    # a coarsened periodic axis that is odd or shorter than 4, the level in the message
    for dims, per, nl, masks, lvl in (((5, 4), 1, 2, None, 0), ((8, 3), 2, 2, None, 0), ((8, 2), 2, 2, None, 0),
                                      ((8, 6), 2, 3, None, 1), ((8, 6), 2, 3, (3, 2), 1), ((8, 8, 6), 4, 3, None, 1),
                                      ((64, 48), 3, 6, None, 4), ((12, 8), 1, 4, (1, 1, 1), 2)):
        st, msg = _raw(amg, ctor, dims, per, nl, masks)
        assert st == E and "periodic_axes" in msg and f"level {lvl}" in msg, (dims, per, nl, masks, msg)
    st, msg = _raw(amg, ctor, (64, 48), 3, 6)
    assert "axis y" in msg and "3 points" in msg, msg
    # ... but a periodic axis that a level does not coarsen may have any length
    if ctor == "host":
        assert _raw(amg, ctor, (8, 3), 2, 3, (1, 1))[0] == 0
        assert _raw(amg, ctor, (64, 48), 3, 5)[0] == 0
    # a periodic axis has no sides
    for dims, per, sides in (((8, 6), 1, 1), ((8, 6), 1, 2), ((8, 6), 2, 4), ((8, 6), 3, 8), ((8, 6, 4), 4, 16),
                             ((8, 6, 4), 5, 32 | 12)):
        st, msg = _raw(amg, ctor, dims, per, natural_sides=sides)
        assert st == E and "natural_sides" in msg and "periodic" in msg, (dims, per, sides, msg)
    # natural_sides out of range, in the tensor constructors' words
    st, msg = _raw(amg, ctor, (8, 6), 1, natural_sides=16)
    assert st == E and "natural_sides" in msg and "has bits other than" in msg, msg
    # singular needs the sides of every axis that is not periodic, and only those
    for dims, per, sides in (((8, 6), 1, 0), ((8, 6), 1, 4), ((8, 6), 2, 1), ((8, 6, 4), 3, 16), ((8, 6, 4), 5, 0)):
        st, msg = _raw(amg, ctor, dims, per, natural_sides=sides, singular=1)
        assert st == E and "singular" in msg, (dims, per, sides, msg)
    for sing in (2, -1):
        st, msg = _raw(amg, ctor, (8, 6), 3, singular=sing)
        assert st == E and "singular" in msg, msg
    st, msg = _raw(amg, ctor, (8, 6), 3, n_levels=1, singular=1)
    assert st == E and "singular" in msg and "2 levels" in msg, msg
    if ctor == "host":
        for dims, per, sides in (((8, 6), 3, 0), ((8, 6), 1, 12), ((8, 6), 2, 3), ((8, 6, 4), 7, 0), ((8, 6, 4), 5, 12)):
            st, msg = _raw(amg, ctor, dims, per, natural_sides=sides, singular=1)
            assert st == 0, (dims, per, sides, msg)
    # what amg_hip_create_tensor / _tensor_semi check
    st, msg = _raw(amg, ctor, (8, 6), 1, n=47)
    assert st == E and "`n` = 47" in msg, msg
    st, msg = _raw(amg, ctor, (8, 6), 1, n_levels=0)
    assert st == E and "n_levels" in msg, msg
    st, msg = _raw(amg, ctor, (8, 6), 0, n_levels=4)  # 8x6 -> 4x3 -> 2x1: the rule's own refusal
    assert st == E and "level 2" in msg, msg
    for mask, word in ((0, "coarsens no axis"), (4, "coarsens z"), (8, "has bits other than")):
        st, msg = _raw(amg, ctor, (8, 6), 1, 2, (mask,))
        assert st == E and word in msg and "level 0" in msg, (mask, msg)
    st, msg = _raw(amg, ctor, (8, 1), 1, 2, (2,))
    assert st == E and "axis y" in msg, msg
    st, msg = _raw(amg, ctor, (8, 6), 1, window=1)
    assert st == amg.EUNSUPPORTED and "window" in msg, msg


def test_python_front_end_raises(amg):
    A = csc(PT.diffusion((8, 6), 3))
    b = PT.rhs(48, True)
    with pytest.raises(ValueError, match="periodic_axes"):
        amg.Multigrid.tensor_periodic(A.indptr, A.indices, A.data, b, (8, 6), 2, 4, host_only=True)
    with pytest.raises(ValueError, match="level 1"):
        amg.Multigrid.tensor_periodic(A.indptr, A.indices, A.data, b, (8, 6), 3, 3, host_only=True)
    with pytest.raises(ValueError, match="axis_masks"):
        amg.Multigrid.tensor_periodic(A.indptr, A.indices, A.data, b, (8, 6), 3, 3, axis_masks=(1,), host_only=True)


def test_existing_constructors_refusals_are_unchanged(amg):
    """The rule of amg_hip_create_tensor / _tensor_semi for `singular` and its words."""
    A = csc(N.diffusion((6, 5)))
    b = N.rhs(30)
    kw = dict(host_only=True, smoother=amg.SM_JACOBI, **JAC)
    for sides in (0, 3, 12):
        with pytest.raises(ValueError, match=r"`singular` = 1 needs every side natural: `natural_sides` = 15, got "
                                             + str(sides)):
            amg.Multigrid.tensor(A.indptr, A.indices, A.data, b, (6, 5), 2, natural_sides=sides, singular=True, **kw)
        with pytest.raises(ValueError, match="`singular` = 1 needs every side natural"):
            amg.Multigrid.tensor_semi(A.indptr, A.indices, A.data, b, (6, 5), 2, axis_masks=(1,),
                                      natural_sides=sides, singular=True, **kw)
    with pytest.raises(ValueError, match="has bits other than the 4 sides of a 2-D grid"):
        amg.Multigrid.tensor(A.indptr, A.indices, A.data, b, (6, 5), 2, natural_sides=16, **kw)
    with pytest.raises(ValueError, match="only the tensor constructors"):
        _flat_sides(amg, A, b)


def _flat_sides(amg, A, b):
    """amg_hip_create with natural_sides = 1 through the C interface."""
    i32, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    o = amg.Options()
    L = amg.lib()
    L.amg_hip_default_options(C.byref(o))
    o.host_only, o.natural_sides = 1, 1
    h = C.c_void_p()
    cp, ri, v = (np.ascontiguousarray(A.indptr, np.int32), np.ascontiguousarray(A.indices, np.int32),
                 np.ascontiguousarray(A.data, np.float64))
    st = L.amg_hip_create(A.shape[0], cp.ctypes.data_as(i32), ri.ctypes.data_as(i32), v.ctypes.data_as(f64),
                          b.ctypes.data_as(f64), 2, C.byref(o), C.byref(h))
    assert st == amg.EINVAL
    raise ValueError(L.amg_hip_last_error().decode())


def test_standalone_transfers_check_the_periodic_mask(amg):
    """Before they look for a device."""
    r, uH = np.ones(120), np.ones(30)
    for per in (4, -1, 8):
        with pytest.raises(ValueError, match="periodic_axes"):
            amg.tensor_restrict((12, 10), r, periodic_axes=per)
        with pytest.raises(ValueError, match="periodic_axes"):
            amg.tensor_prolong_add((12, 10), uH, r, periodic_axes=per)
    with pytest.raises(ValueError, match="periodic_axes"):  # 5 points along a coarsened periodic x
        amg.tensor_restrict((5, 4), np.ones(20), periodic_axes=1)
    with pytest.raises(ValueError, match="periodic_axes"):  # 2 points
        amg.tensor_prolong_add((8, 2), np.ones(4), np.ones(16), periodic_axes=2)
    with pytest.raises(ValueError, match="natural_sides"):
        amg.tensor_restrict((12, 10), r, natural_sides=1, periodic_axes=1)
    with pytest.raises(ValueError, match="natural_sides"):
        amg.tensor_prolong_add((12, 10), uH, r, natural_sides=8, periodic_axes=2)
    for mask in (0, 4, 8):  # the _axes checks stay
        with pytest.raises(ValueError):
            amg.tensor_restrict((12, 10), r, axes=mask, periodic_axes=1)
    # the _per entry point itself with mask 0 (the wrappers take it for a non-zero mask only): the _bc
    # form's checks, and no refusal of the mask
    i64, f64 = C.POINTER(C.c_int64), C.POINTER(C.c_double)
    d3, out = np.array((12, 10, 1), np.int64), np.empty(30)
    L = amg.lib()
    for sides, word in ((16, "natural_sides"), (-1, "natural_sides")):
        st = L.amg_hip_tensor_restrict_per(2, d3.ctypes.data_as(i64), 3, sides, 0, r.ctypes.data_as(f64),
                                           out.ctypes.data_as(f64))
        assert st == amg.EINVAL and word in L.amg_hip_last_error().decode()
    st = L.amg_hip_tensor_restrict_per(2, d3.ctypes.data_as(i64), 0, 0, 0, r.ctypes.data_as(f64), out.ctypes.data_as(f64))
    assert st == amg.EINVAL and "coarsens no axis" in L.amg_hip_last_error().decode()
    st = L.amg_hip_tensor_restrict_per(2, d3.ctypes.data_as(i64), 3, 5, 0, r.ctypes.data_as(f64), out.ctypes.data_as(f64))
    assert st != amg.EINVAL, L.amg_hip_last_error().decode()  # accepted: runs, or EHIP for want of a device


def test_getter_on_other_solvers(amg):
    cp, ri, v = amg.laplacian(16)
    flat = amg.Multigrid(cp, ri, v, amg.rhs(16), 3, host_only=True)
    assert flat.periodic_axes() == 0
    flat.close()
    A = csc(N.diffusion((6, 5), 15))
    t = amg.Multigrid.tensor(A.indptr, A.indices, A.data, np.ones(30), (6, 5), 2, host_only=True)
    assert t.periodic_axes() == 0
    t.close()


def test_twin_counts_do_not_grow_with_periodic_transfers():
    """A condition on the inputs, on the twin alone: the fully periodic operator at (64, 48) / 5 levels
    takes 9 PCG iterations with the periodic transfers and 13 with the best hierarchy the tensor
    constructors offer without them (every side natural, singular)."""
    A = PT.diffusion((64, 48), 3)
    b = PT.rhs(A.shape[0], True)
    per = PT.PeriodicTwin(A, (64, 48), 5, periodic=3, singular=True).pcg(b, 1e-8)[1]
    nat = N.NaturalTwin(A, (64, 48), 5, sides=15, singular=True).pcg(b, 1e-8)[1]
    assert (per, nat) == (9, 13), (per, nat)
