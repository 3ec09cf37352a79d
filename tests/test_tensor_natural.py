"""Natural boundary sides of the tensor hierarchies (amg_hip_options.natural_sides / .singular), the
parts that need no GPU: on host_only solvers P / R against the Kronecker products of the scipy twin
(tests/natural_twin.py) entry for entry, the level matrices against amg_hip_create_custom on the
twin's operators bit for bit, the getter, mask 0 against a solver made without the fields, and every
argument error with the field's name in the message."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "algebraic-multigrid_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import natural_twin as N  # noqa: E402
import semi_twin as S  # noqa: E402
import tensor_twin as T  # noqa: E402

JAC = dict(smoother_iters=2, omega=0.8)

# axis lengths 2, 3, 4, 5, 20 and 33; every side mask on the grids of at most 5 points per axis
SMALL = ((2, 3), (4, 5), (5, 2), (3, 4), (2, 3, 4), (5, 4, 3), (3, 5, 2), (5, 5, 5))
LARGE = ((33, 20), (20, 33), (33, 20, 4), (5, 20, 33))


def csc(A):
    A = sp.csc_matrix(A)
    A.sort_indices()
    return A


def _same_triple(got, want):
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and
            np.array_equal(np.asarray(got[2]).view(np.uint64), np.asarray(want[2]).view(np.uint64)))


def side_masks(dims):
    dim = len(dims)
    if max(dims) <= 5:
        return range(1 << (2 * dim))
    return (N.all_sides(dim), N.low_sides(dim), N.high_sides(dim), 0b000110 if dim == 2 else 0b100110)


def axis_masks(dims):
    """The full mask and every semi mask whose axes have 2 points."""
    dim = len(dims)
    return [m for m in range(1, 1 << dim) if S.mask_error(dims, dim, m) is None]


def make(amg, A, b, dims, n_levels, masks=None, **kw):
    A = csc(A)
    kw.setdefault("smoother", amg.SM_JACOBI)
    for k, v in JAC.items():
        kw.setdefault(k, v)
    if masks is None:
        return amg.Multigrid.tensor(A.indptr, A.indices, A.data, b, dims, n_levels, host_only=True, **kw)
    return amg.Multigrid.tensor_semi(A.indptr, A.indices, A.data, b, dims, n_levels, axis_masks=masks,
                                     host_only=True, **kw)


@pytest.mark.parametrize("dims", SMALL + LARGE)
def test_transfers_equal_the_twin(amg, dims):
    """One level pair per (axis mask, side mask): P and R entry for entry, through the matrix-free
    kind (rebuilt for the getter) and through stencil_transfers = 0."""
    dim = len(dims)
    A = N.diffusion(dims)
    b = N.rhs(A.shape[0])
    full = S.full_mask(dim)
    for am, sides in itertools.product(axis_masks(dims), side_masks(dims)):
        P = N.natural_P(dims, dim, am, sides)
        assert set(np.unique(P.data)) <= {2.0 ** -k for k in range(dim + 1)}
        assert P.nnz == S.semi_P(dims, dim, am).nnz  # the pattern is P1's
        for st in ((True, False) if max(dims) <= 5 else (True,)):
            mg = make(amg, A, b, dims, 2, None if am == full else (am,), natural_sides=sides,
                      stencil_transfers=st)
            assert mg.natural_sides() == sides
            assert mg.level_axes(0) == am and mg.level_transfer_kind(0) == (2 if st else 0)
            assert _same_triple(mg.get_transfer(0, "P"), T.csc_triple(P)), (am, sides, st, "P")
            assert _same_triple(mg.get_transfer(0, "R"), T.csc_triple(P.T)), (am, sides, st, "R")
            mg.close()
    # all sides natural: P reproduces the constants
    P = N.natural_P(dims, dim, full, N.all_sides(dim))
    assert np.array_equal(P @ np.ones(P.shape[1]), np.ones(P.shape[0]))


CHAINS = [((33, 20), None, 5), ((20, 33), (2, 3, 1, 3), 5), ((5, 20, 33), None, 3), ((33, 20, 4), (5, 2, 7), 4),
          ((5, 4), None, 3), ((5, 5, 5), None, 3), ((17, 12, 9), (3, 6, 5), 4)]


@pytest.mark.parametrize("dims,masks,nl", CHAINS)
def test_level_matrices_equal_create_custom(amg, dims, masks, nl):
    """The same side mask on every level: dims, transfers and level matrices of the whole chain, the
    matrices bit for bit with amg_hip_create_custom on the twin's P and R; also for a singular
    solver, whose getters return the true operators."""
    dim = len(dims)
    for sides, dirichlet in ((N.all_sides(dim), 0), (N.all_sides(dim) & ~1, 1), (N.high_sides(dim), N.low_sides(dim))):
        A = N.diffusion(dims, dirichlet)
        b = N.rhs(A.shape[0], dirichlet)
        tw = N.NaturalTwin(A, dims, nl, masks=masks, sides=sides, singular=dirichlet == 0)
        mg = make(amg, A, b, dims, nl, masks, natural_sides=sides, singular=dirichlet == 0)
        assert mg.n_levels == nl and mg.natural_sides() == sides
        assert [mg.level_dims(l) for l in range(nl)] == tw.dims
        transfers = []
        for l in range(nl - 1):
            P = N.natural_P(tw.dims[l], dim, tw.masks[l], sides)
            assert _same_triple(mg.get_transfer(l, "P"), T.csc_triple(P)), (l, "P")
            assert _same_triple(mg.get_transfer(l, "R"), T.csc_triple(P.T)), (l, "R")
            transfers.append((T.csc_triple(P), T.csc_triple(P.T)))
        A0 = csc(A)
        cu = amg.Multigrid(A0.indptr, A0.indices, A0.data, b, nl, smoother=amg.SM_JACOBI, transfers=transfers,
                           host_only=True, **JAC)
        assert cu.natural_sides() == 0
        for l in range(nl):
            assert cu.get_n_dofs(l) == mg.get_n_dofs(l) == tw.n[l], l
            assert _same_triple(mg.get_coefficient_matrix(l), cu.get_coefficient_matrix(l)), l
            M = mg.get_coefficient_matrix(l)
            got = sp.csc_matrix((M[2], M[1], M[0]), shape=(tw.n[l], tw.n[l]))
            # the twin's product adds in scipy's order: rounding relative to the entries that went in
            # (a singular chain ends in entries that cancel to rounding)
            assert abs(got - tw.A[l]).max() <= 1e-13 * max(abs(tw.A[k]).max() for k in range(l + 1)), l
        if dirichlet == 0:  # the constants stay in the null space of every level
            M = mg.get_coefficient_matrix(nl - 1)
            Ac = sp.csc_matrix((M[2], M[1], M[0]), shape=(tw.n[-1], tw.n[-1]))
            assert np.abs(Ac @ np.ones(tw.n[-1])).max() <= 1e-12 * abs(tw.A[0]).max()
        cu.close()
        mg.close()


@pytest.mark.parametrize("dims,masks,nl", [((33, 20), None, 4), ((17, 12, 9), (3, 6, 5), 4)])
def test_mask_zero_is_the_solver_without_the_fields(amg, dims, masks, nl):
    A = S.diffusion(dims, (1.0,) * len(dims))
    b = S.rhs(A.shape[0])
    old = make(amg, A, b, dims, nl, masks)
    new = make(amg, A, b, dims, nl, masks, natural_sides=0, singular=False)
    assert old.natural_sides() == new.natural_sides() == 0
    for l in range(nl):
        assert _same_triple(old.get_coefficient_matrix(l), new.get_coefficient_matrix(l)), l
    for l in range(nl - 1):
        P = S.semi_P(old.level_dims(l), len(dims), old.level_axes(l))
        for which in "PR":
            assert _same_triple(old.get_transfer(l, which), new.get_transfer(l, which)), (l, which)
        assert _same_triple(new.get_transfer(l, "P"), T.csc_triple(P)), l
    old.close()
    new.close()


def test_default_options_zero_both_fields(amg):
    o = amg.Options()
    o.natural_sides, o.singular = 63, 1
    amg.lib().amg_hip_default_options(C.byref(o))
    assert o.natural_sides == 0 and o.singular == 0
    assert [f[0] for f in amg.Options._fields_][-2:] == ["natural_sides", "singular"]


def _raw(amg, ctor, dims, natural_sides, singular, masks=None, n_levels=2):
    """status and message of constructor `ctor` with the two fields set, host_only.  The _dev
    constructors get fake device pointers: callers pass them valid options only when no device is
    present (argument errors return before any device call)."""
    i32, i64, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
    dim = len(dims)
    A = csc(N.diffusion(dims, 1))
    n = A.shape[0]
    b = np.ones(n)
    o = amg.Options()
    L = amg.lib()
    L.amg_hip_default_options(C.byref(o))
    o.host_only = 1
    o.smoother, o.smoother_iters, o.omega = amg.SM_JACOBI, 2, 0.8
    o.natural_sides, o.singular = natural_sides, singular
    h = C.c_void_p()
    d = np.array(T.dims3(dims), np.int64)
    cp, ri, v = (np.ascontiguousarray(A.indptr, np.int32), np.ascontiguousarray(A.indices, np.int32),
                 np.ascontiguousarray(A.data, np.float64))
    mat = (n, cp.ctypes.data_as(i32), ri.ctypes.data_as(i32), v.ctypes.data_as(f64), b.ctypes.data_as(f64))
    fake = (n,) + (C.c_void_p(8),) * 4  # device arrays: not read by the argument checks
    m = None if masks is None else np.ascontiguousarray(masks, np.int32)
    mp = None if m is None else m.ctypes.data_as(i32)
    grid = (dim, d.ctypes.data_as(i64), n_levels)
    if ctor == "create":
        st = L.amg_hip_create(*mat, 2, C.byref(o), C.byref(h))
    elif ctor == "custom":
        P = T.csc_triple(S.semi_P(dims, dim, S.full_mask(dim)))
        R = T.csc_triple(S.semi_P(dims, dim, S.full_mask(dim)).T)
        tabs = []
        for a in (P[0], P[1], P[2], R[0], R[1], R[2]):
            t = ((f64 if a.dtype == np.float64 else i32) * 1)()
            t[0] = a.ctypes.data_as(f64 if a.dtype == np.float64 else i32)
            tabs.append(t)
        st = L.amg_hip_create_custom(*mat, 2, *tabs, C.byref(o), C.byref(h))
    elif ctor == "rs":
        st = L.amg_hip_create_rs(*mat, 3, 0.25, 4, C.byref(o), C.byref(h))
    elif ctor == "poisson":
        st = L.amg_hip_create_poisson(2, 8, 2, C.byref(o), C.byref(h))
    elif ctor == "poisson_window":
        st = L.amg_hip_create_poisson_window(2, 8, 0, 4, 2, C.byref(o), C.byref(h))
    elif ctor == "poisson_tensor":
        st = L.amg_hip_create_poisson_tensor(2, 8, 2, C.byref(o), C.byref(h))
    elif ctor == "tensor":
        st = L.amg_hip_create_tensor(*mat, *grid, C.byref(o), C.byref(h))
    elif ctor == "tensor_semi":
        st = L.amg_hip_create_tensor_semi(*mat, *grid, mp, 0.5, 1, C.byref(o), C.byref(h))
    elif ctor == "tensor_dev":
        st = L.amg_hip_create_tensor_dev(*fake, *grid, C.byref(o), C.byref(h))
    elif ctor == "tensor_semi_dev":
        st = L.amg_hip_create_tensor_semi_dev(*fake, *grid, mp, 0.5, 1, C.byref(o), C.byref(h))
    else:
        raise AssertionError(ctor)
    msg = L.amg_hip_last_error().decode()
    if st == 0:
        L.amg_hip_destroy(h)
    return st, msg


TENSOR_CTORS = ("tensor", "tensor_semi", "tensor_dev", "tensor_semi_dev")
FLAT_CTORS = ("create", "custom", "rs", "poisson", "poisson_window", "poisson_tensor")


@pytest.mark.parametrize("ctor", TENSOR_CTORS)
def test_tensor_constructors_check_the_fields(amg, ctor):
    host = ctor in ("tensor", "tensor_semi")
    # the _dev constructors copy the caller's device arrays once the checks pass: accepted options go
    # to them with fake pointers only where no device is present (the refusal is then EHIP); with real
    # device arrays tests/test_gpu_tensor_natural.py covers acceptance
    no_device = amg.device_count() == 0
    for dims in ((6, 5), (4, 3, 2)):
        dim = len(dims)
        top = 1 << (2 * dim)
        for bad in (top, top + 1, 1 << 6, 1 << 20, -1, -top):
            st, msg = _raw(amg, ctor, dims, bad, 0)
            assert st == amg.EINVAL and "natural_sides" in msg, (dims, bad, msg)
        for sides in (0, 1, top - 2, N.low_sides(dim)):
            st, msg = _raw(amg, ctor, dims, sides, 1)
            assert st == amg.EINVAL and "singular" in msg, (dims, sides, msg)
        for sing in (2, -1, 7):
            st, msg = _raw(amg, ctor, dims, top - 1, sing)
            assert st == amg.EINVAL and "singular" in msg, (dims, sing, msg)
        for sides, sing in ((0, 0), (top - 1, 0), (top - 1, 1), (5, 0)):
            if host:
                st, msg = _raw(amg, ctor, dims, sides, sing)
                assert st == 0, (dims, sides, sing, msg)
            elif no_device:  # past the argument checks: refused for want of a device
                st, msg = _raw(amg, ctor, dims, sides, sing)
                assert st == amg.EHIP and "natural_sides" not in msg and "singular" not in msg, msg
        # singular needs a coarser level: a one-level solver would solve on the caller's own b
        st, msg = _raw(amg, ctor, dims, top - 1, 1, n_levels=1)
        assert st == amg.EINVAL and "singular" in msg and "2 levels" in msg, msg
        if host:
            assert _raw(amg, ctor, dims, top - 1, 0, n_levels=1)[0] == 0
    # 2-D: the z bits are out of range
    st, msg = _raw(amg, ctor, (6, 5), 16, 0)
    assert st == amg.EINVAL and "natural_sides" in msg, msg


@pytest.mark.parametrize("ctor", FLAT_CTORS)
def test_other_constructors_refuse_the_fields(amg, ctor):
    for sides in (1, 15, 63, -1):
        st, msg = _raw(amg, ctor, (6, 5), sides, 0)
        assert st == amg.EINVAL and "natural_sides" in msg, (sides, msg)
    st, msg = _raw(amg, ctor, (6, 5), 0, 1)
    assert st == amg.EINVAL and "singular" in msg, msg
    st, msg = _raw(amg, ctor, (6, 5), 0, 2)
    assert st == amg.EINVAL and "singular" in msg, msg


def test_standalone_transfers_check_the_side_mask(amg):
    """Before they look for a device."""
    for sides in (16, 64, -1):
        with pytest.raises(ValueError, match="natural_sides"):
            amg.tensor_restrict((12, 10), np.ones(120), natural_sides=sides)
        with pytest.raises(ValueError, match="natural_sides"):
            amg.tensor_prolong_add((12, 10), np.ones(30), np.ones(120), natural_sides=sides)
    with pytest.raises(ValueError, match="natural_sides"):
        amg.tensor_restrict((4, 3, 2), np.ones(24), axes=3, natural_sides=64)
    # the _axes checks stay
    for mask in (0, 4, 8):
        with pytest.raises(ValueError):
            amg.tensor_restrict((12, 10), np.ones(120), axes=mask, natural_sides=15)
    with pytest.raises(ValueError, match="axis x"):
        amg.tensor_prolong_add((1, 10), np.ones(0), np.ones(10), axes=1, natural_sides=3)


def test_automatic_rule_that_stops_at_level_0_refuses_singular(amg):
    """n_levels is a maximum under the automatic semi rule: a hierarchy that ends at level 0 is the
    one-level case and refuses singular = 1 like an explicit n_levels = 1."""
    A = csc(N.diffusion((6, 5)))
    b = N.rhs(30)
    kw = dict(theta=0.5, min_coarse=64, host_only=True, smoother=amg.SM_JACOBI, natural_sides=15, **JAC)
    one = amg.Multigrid.tensor_semi(A.indptr, A.indices, A.data, b, (6, 5), 4, **kw)
    assert one.n_levels == 1
    one.close()
    with pytest.raises(ValueError, match="singular"):
        amg.Multigrid.tensor_semi(A.indptr, A.indices, A.data, b, (6, 5), 4, singular=True, **kw)


def test_getter_on_other_solvers(amg):
    cp, ri, v = amg.laplacian(16)
    flat = amg.Multigrid(cp, ri, v, amg.rhs(16), 3, host_only=True)
    assert flat.natural_sides() == 0
    flat.close()


def test_twin_counts_do_not_grow_with_natural_sides():
    """A condition on the inputs, on the twin alone: with no Dirichlet side the PCG count at (64, 48) /
    5 levels is 25 with mask 0 and 10 with the natural sides and the pinned solve."""
    A = N.diffusion((64, 48))
    b = N.rhs(A.shape[0])
    today = N.NaturalTwin(A, (64, 48), 5).pcg(b, 1e-8)[1]
    fixed = N.NaturalTwin(A, (64, 48), 5, sides=15, singular=True).pcg(b, 1e-8)[1]
    assert (today, fixed) == (25, 10), (today, fixed)
