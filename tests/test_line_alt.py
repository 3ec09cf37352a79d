"""Alternating-direction line smoother (AMG_HIP_SM_LINE_ALT), the parts that need no GPU: the
constant and the symbols, the directions of every level of host_only tensor hierarchies, the
refusals, and the argument checks of the stand-alone call."""
import os
import sys

import numpy as np
import pytest

sp = pytest.importorskip("scipy.sparse")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import line_alt_twin as AT  # noqa: E402

SM = 7  # AMG_HIP_SM_LINE_ALT
KW = dict(smoother=SM, smoother_iters=1, omega=0.8, host_only=True)


def laplacian(dims):
    """2 d-point Laplacian on the grid `dims` (x fastest), Dirichlet; (CSC arrays, b)."""
    A = None
    for m in dims:
        T = sp.diags([-np.ones(m - 1), 2.0 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1]) if m > 1 else sp.eye(1) * 2.0
        A = T if A is None else sp.kron(sp.eye(m), A) + sp.kron(T, sp.eye(A.shape[0]))
    A = sp.csc_matrix(A)
    A.sort_indices()
    return (A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy()), np.ones(A.shape[0])


def test_constant_and_symbols(amg):
    assert amg.SM_LINE_ALT == 7
    L = amg.lib()
    assert hasattr(L, "amg_hip_line_directions") and hasattr(L, "amg_hip_smooth_line_alt")
    with open(os.path.join(os.path.dirname(__file__), "..", "include", "amg_hip.h")) as h:
        text = h.read()
    assert "AMG_HIP_SM_LINE_ALT = 7" in text
    assert "amg_hip_line_directions(" in text and "amg_hip_smooth_line_alt(" in text


@pytest.mark.parametrize("dims,levels", [((12, 10), 3), ((9, 2), 2), ((2, 9), 2), ((6, 5, 4), 3), ((8, 2, 5), 2)])
def test_line_directions_on_every_level(amg, dims, levels):
    """The strides of the axes of length >= 2 of each level's own grid, down to the last level; levels
    where an axis reached length 1 drop it ((9, 2) -> (4, 1), (6, 5, 4) -> (3, 2, 2) -> (1, 1, 1))."""
    A, b = laplacian(dims)
    mg = amg.Multigrid.tensor(*A, b, dims, levels, **KW)
    seen_short = False
    for l in range(mg.n_levels):
        d = mg.level_dims(l)
        want = [s for s, _ in AT.directions(d)]
        assert mg.line_directions(l) == want, (l, d)
        seen_short |= len(want) < len(dims)
    if dims in ((9, 2), (2, 9), (6, 5, 4), (8, 2, 5)):
        assert seen_short
    with pytest.raises(ValueError, match="level out of range"):
        mg.line_directions(mg.n_levels)
    mg.close()


def test_line_directions_values(amg):
    A, b = laplacian((12, 10))
    mg = amg.Multigrid.tensor(*A, b, (12, 10), 3, **KW)
    assert [mg.line_directions(l) for l in range(3)] == [[1, 12], [1, 6], [1, 3]]
    mg.close()
    A, b = laplacian((6, 5, 4))
    mg = amg.Multigrid.tensor(*A, b, (6, 5, 4), 3, **KW)
    assert [mg.level_dims(l) for l in range(3)] == [(6, 5, 4), (3, 2, 2), (1, 1, 1)]
    assert [mg.line_directions(l) for l in range(3)] == [[1, 6, 30], [1, 3, 6], []]
    mg.close()
    A, b = laplacian((9, 2))
    mg = amg.Multigrid.tensor(*A, b, (9, 2), 2, **KW)
    assert [mg.line_directions(l) for l in range(2)] == [[1, 9], [1]]
    mg.close()
    A, b = laplacian((2, 9))
    mg = amg.Multigrid.tensor(*A, b, (2, 9), 2, **KW)
    assert [mg.line_directions(l) for l in range(2)] == [[1, 2], [1]]      # (1, 4): the stride of y is nx = 1
    mg.close()


def test_line_directions_needs_the_smoother(amg):
    A, b = laplacian((12, 10))
    mg = amg.Multigrid.tensor(*A, b, (12, 10), 2, smoother=amg.SM_LINE_JACOBI, omega=0.7, host_only=True)
    with pytest.raises(ValueError, match="not AMG_HIP_SM_LINE_ALT"):
        mg.line_directions(0)
    mg.close()
    alt = amg.Multigrid.tensor(*A, b, (12, 10), 2, **KW)
    with pytest.raises(ValueError, match="not AMG_HIP_SM_LINE_JACOBI"):
        alt.line_stride(0)
    alt.close()


def test_non_tensor_constructors_refuse(amg, oracle):
    """EINVAL, 'unknown smoother kind' kept, and the pointer to amg_hip_create_tensor."""
    A, b = oracle.laplacian(16), oracle.rhs(16)
    msg = "unknown smoother kind.*level grids of amg_hip_create_tensor"
    with pytest.raises(ValueError, match=msg):
        amg.Multigrid(A.colptr, A.rowind, A.val, b, 3, **KW)
    with pytest.raises(ValueError, match=msg):                     # not host_only: still before the device
        amg.Multigrid(A.colptr, A.rowind, A.val, b, 3, smoother=SM, omega=0.8)
    with pytest.raises(ValueError, match=msg):
        amg.Multigrid.ruge_stueben(A.colptr, A.rowind, A.val, b, 12, 0.25, 30, **KW)
    with pytest.raises(ValueError, match=msg):                     # amg_hip_create_poisson has no host_only form
        amg.Multigrid.poisson(16, 3, smoother=SM, omega=0.8)
    with pytest.raises(ValueError, match=msg):
        amg.Multigrid.poisson_window(64, 0, 32, 3, **KW)
    with pytest.raises(ValueError, match="unknown smoother kind"):   # the next value is still unknown everywhere
        amg.Multigrid(A.colptr, A.rowind, A.val, b, 3, smoother=8, host_only=True)
    with pytest.raises(ValueError, match="unknown smoother kind"):
        A2, b2 = laplacian((12, 10))
        amg.Multigrid.tensor(*A2, b2, (12, 10), 2, smoother=8, host_only=True)


def test_custom_constructor_refuses(amg, oracle):
    import ctypes as C
    A, b = oracle.laplacian(8), oracle.rhs(8)
    o = amg.Options()
    amg.lib().amg_hip_default_options(C.byref(o))
    o.host_only, o.smoother, o.omega = 1, SM, 0.8
    h = C.c_void_p()
    p32, p64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    cp, ri, v = (np.ascontiguousarray(A.colptr, np.int32), np.ascontiguousarray(A.rowind, np.int32),
                 np.ascontiguousarray(A.val, np.float64))
    st = amg.lib().amg_hip_create_custom(64, cp.ctypes.data_as(p32), ri.ctypes.data_as(p32), v.ctypes.data_as(p64),
                                         np.ascontiguousarray(b).ctypes.data_as(p64), 1, None, None, None, None,
                                         None, None, C.byref(o), C.byref(h))
    assert st == amg.EINVAL
    msg = amg.lib().amg_hip_last_error().decode()
    assert "unknown smoother kind" in msg and "amg_hip_create_tensor" in msg


def test_tensor_constructor_checks(amg):
    A, b = laplacian((12, 10))
    for omega in (0.0, 2.0, -1.0, 2.5, float("nan")):
        with pytest.raises(ValueError, match=r"`omega` must lie in \(0, 2\)"):
            amg.Multigrid.tensor(*A, b, (12, 10), 2, smoother=SM, omega=omega, host_only=True)
    with pytest.raises(amg.AmgHipError) as e:
        amg.Multigrid.tensor(*A, b, (12, 10), 2, window=True, **KW)
    assert e.value.status == amg.EUNSUPPORTED
    with pytest.raises(ValueError, match="smoother_iters"):
        amg.Multigrid.tensor(*A, b, (12, 10), 2, **dict(KW, smoother_iters=-1))


def test_bad_pivot_names_level_direction_and_row(amg):
    (cp, ri, v), b = laplacian((12, 10))
    # row 36 is the first row of the x line y = 3: its pivot is its diagonal
    v = laplacian((12, 10))[0][2].copy()
    at = [p for p in range(cp[36], cp[37]) if ri[p] == 36][0]
    v[at] = 0.0
    with pytest.raises(ValueError, match=r"level 0 direction x row 36 .*pivot"):
        amg.Multigrid.tensor(cp, ri, v, b, (12, 10), 2, **KW)
    # y direction: a diagonal matrix with one bad entry on a grid whose x axis has length 1
    D = sp.identity(9, format="csc") * 2.0
    d = D.data.copy()
    d[0] = 0.0
    with pytest.raises(ValueError, match=r"level 0 direction y row 0 .*pivot"):
        amg.Multigrid.tensor(D.indptr.astype(np.int32), D.indices.astype(np.int32), d, np.ones(9), (1, 9), 1, **KW)
    d[0] = float("inf")
    with pytest.raises(ValueError, match=r"direction y row 0 .*pivot"):
        amg.Multigrid.tensor(D.indptr.astype(np.int32), D.indices.astype(np.int32), d, np.ones(9), (1, 9), 1, **KW)


def test_host_only_solver_refusals(amg):
    """Where AMG_HIP_SM_LINE_JACOBI is refused with EUNSUPPORTED, so is this smoother."""
    A, b = laplacian((12, 10))
    mg = amg.Multigrid.tensor(*A, b, (12, 10), 2, **KW)
    for call in (lambda: mg.slab_setup(0, 2), lambda: mg.fine_sweep_info(), lambda: mg.profile_fine_sweep(1),
                 lambda: mg.block_must_move(2), lambda: mg.f32_must_move(), lambda: mg.pcg_mixed(1e-8, 5),
                 lambda: mg.apply_f32(8, 16)):  # never dereferenced: the smoother is refused first
        with pytest.raises(amg.AmgHipError) as e:
            call()
        assert e.value.status == amg.EUNSUPPORTED, amg.lib().amg_hip_last_error()
    mg.close()


def test_smooth_line_alt_argument_errors(amg):
    (cp, ri, v), b = laplacian((6, 5))
    u = np.zeros(30)
    with pytest.raises(ValueError, match="is not the 6 x 4 x 1 grid"):
        amg.smooth_line_alt(cp, ri, v, u, b, (6, 4))
    with pytest.raises(ValueError, match="dim"):
        amg.smooth_line_alt(cp, ri, v, u, b, (30,))
    with pytest.raises(ValueError, match="dims"):
        amg.smooth_line_alt(cp, ri, v, u, b, (6, 5, 0))
    for omega in (0.0, 2.0, float("nan")):
        with pytest.raises(ValueError, match=r"`omega` must lie in \(0, 2\)"):
            amg.smooth_line_alt(cp, ri, v, u, b, (6, 5), omega=omega)
    with pytest.raises(ValueError, match="`iters` must be >= 0"):
        amg.smooth_line_alt(cp, ri, v, u, b, (6, 5), iters=-1)
    bad = v.copy()
    bad[[p for p in range(cp[12], cp[13]) if ri[p] == 12][0]] = 0.0     # first row of the line y = 2
    with pytest.raises(ValueError, match=r"direction x row 12 .*pivot"):
        amg.smooth_line_alt(cp, ri, bad, u, b, (6, 5))


def test_twin_directions_and_line_ends():
    """The twin itself: T_x of the flat 1-D Laplacian seen as a 16 x 8 grid has no entry across a line
    end, and the application is the adjoint of its reverse for a symmetric operator."""
    n = 128
    A = sp.diags([-np.ones(n - 1), 2.0 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1], format="csr")
    dl, dd, du = AT.tridiagonal_part(A, 1, 16)
    assert np.all(dl[::16] == 0) and np.all(du[15::16] == 0) and np.count_nonzero(dl) == n - 8
    assert AT.directions((16, 8, 1)) == [(1, 16), (16, 8)] and AT.directions((1, 9, 1)) == [(1, 9)]
    rng = np.random.default_rng(0)
    B = AT.split_anisotropy(8, 6, 1e-3)
    v, w = rng.standard_normal(48), rng.standard_normal(48)
    z = np.zeros(48)
    fwd = AT.apply(B, z, v, (8, 6, 1), 0.8)
    bwd = AT.apply(B, z, w, (8, 6, 1), 0.8, reverse=True)
    assert abs(fwd @ w - v @ bwd) <= 1e-12 * np.linalg.norm(v) * np.linalg.norm(bwd)
