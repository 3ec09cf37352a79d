"""amg_hip_create_tensor_periodic_dev with amg_hip_set_periodic_device_setup(1): the hierarchy is built
on the device by K-TensorGalerkin's periodic form, and every level, transfer, cycle and solve equals
the host constructor's bit for bit (the host product is spgemm_csr on tensor_P with the mask).

Every test turns the switch on through the fixture `on` and back to 0 in its teardown; no test sets the
environment variable.  setup_on_device == 1 is a condition of every comparison: a silent fall-back to
the host constructor would compare the host product with itself."""
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
import periodic_twin as PT  # noqa: E402
import semi_twin as S  # noqa: E402
import tensor_twin as T  # noqa: E402

pytestmark = pytest.mark.gpu

JAC = dict(smoother=3, smoother_iters=2, omega=0.8)

# (dims, levels, masks, periodic axes, natural sides), as in tests/test_gpu_tensor_periodic.py
XY = ((64, 48), 5, None, 3, 0)
X_DIR = ((32, 21), 4, None, 1, 0)
XYZ = ((16, 12, 8), 3, None, 7, 0)
FORMS = ((32, 20), 4, (3, 3, 1), 3, 0)
# down to coarse length 2 through Galerkin operators: 16 -> 8 -> 4 -> 2 and 8 -> 4 -> 2 on every axis
DEEP2 = ((16, 16), 4, None, 3, 0)
DEEP3 = ((8, 8, 8), 3, None, 7, 0)


@pytest.fixture
def on(amg):
    amg.set_periodic_device_setup(1)
    yield amg
    amg.set_periodic_device_setup(0)


_OPS = {}


def op(dims, per, sides=0):
    """(A as CSR, A as CSC, b, singular) of periodic_twin.diffusion / rhs: built once, never modified."""
    key = (tuple(dims), per, sides)
    if key not in _OPS:
        dirichlet = PT.open_sides(len(dims), per) & ~sides
        A = PT.diffusion(dims, per, dirichlet)
        b = PT.rhs(A.shape[0], dirichlet == 0)
        _OPS[key] = frozen(A, b) + (dirichlet == 0,)
    return _OPS[key]


def frozen(A, b):
    A = sp.csr_matrix(A)
    A.sort_indices()
    Ac = transposed_arrays(A)
    for a in (A.data, A.indices, A.indptr, Ac.data, Ac.indices, Ac.indptr, b):
        a.setflags(write=False)
    return A, Ac, b


def transposed_arrays(A):
    """CSC of a CSR matrix with its stored zeros kept (scipy's own conversion keeps them too; this one
    does not depend on that)."""
    n = A.shape[0]
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    order = np.lexsort((rows, A.indices))
    ptr = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(A.indices, minlength=n), out=ptr[1:])
    return sp.csc_matrix((A.data[order], rows[order].astype(np.int32), ptr), shape=A.shape)


def dev_arrays(A, b):
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy(), np.array(b)


def pair(amg, A, Ac, b, dims, nl, per, masks=None, sides=0, singular=False, **kw):
    """(device-built, host-built) solvers of one operator; setup_on_device is 1 and 0."""
    kw = dict(JAC, **kw)
    dev = amg.Multigrid.tensor_periodic_dev(*dev_arrays(A, b), dims, nl, per, axis_masks=masks, natural_sides=sides,
                                            singular=singular, **kw)
    host = amg.Multigrid.tensor_periodic(Ac.indptr, Ac.indices, Ac.data, b, dims, nl, per, axis_masks=masks,
                                         natural_sides=sides, singular=singular, **kw)
    assert dev.setup_on_device == 1, "the device path fell back to the host constructor"
    assert host.setup_on_device == 0
    return dev, host


def case_pair(amg, case, **kw):
    dims, nl, masks, per, sides = case
    A, Ac, b, singular = op(dims, per, sides)
    return pair(amg, A, Ac, b, dims, nl, per, masks, sides, singular, **kw)


def bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def same_triple(a, c):
    return np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1]) and bits(a[2], c[2])


def state(mg):
    mg.sync()
    return [(mg.get_soln(l), mg.get_rhs(l)) for l in range(mg.n_levels)]


def same_state(a, b):
    return len(a) == len(b) and all(bits(x[0], y[0]) and bits(x[1], y[1]) for x, y in zip(a, b))


def assert_same_hierarchy(dev, host, what):
    nl = host.n_levels
    assert dev.n_levels == nl and dev.periodic_axes() == host.periodic_axes(), what
    assert dev.natural_sides() == host.natural_sides(), what
    for l in range(nl):
        assert dev.level_dims(l) == host.level_dims(l), (what, l)
        assert same_triple(dev.get_coefficient_matrix(l), host.get_coefficient_matrix(l)), (what, l)
    for l in range(nl - 1):
        assert dev.level_axes(l) == host.level_axes(l), (what, l)
        assert dev.level_transfer_kind(l) == 2 and host.level_transfer_kind(l) == 2, (what, l)
        for w in "PR":
            assert same_triple(dev.get_transfer(l, w), host.get_transfer(l, w)), (what, l, w)


def assert_same_cycles(dev, host, what, n=2):
    dev.vcycle(n)
    host.vcycle(n)
    got, ref = state(dev), state(host)
    assert all(np.all(np.isfinite(u)) for u, _ in ref) and np.linalg.norm(ref[0][0]) > 0, what
    assert same_state(got, ref), what


def side_masks(dims, per):
    """tests/test_gpu_tensor_periodic.py: side masks on the axes that are not periodic -- every subset
    on the small 2-D grids, else none, all, the low and the high ones."""
    dim = len(dims)
    free = PT.open_sides(dim, per)
    if dim == 2 and max(dims) <= 8:
        return sorted({s & free for s in range(1 << (2 * dim))})
    return sorted({0, free, free & N.low_sides(dim), free & N.high_sides(dim)})


# ---- 1. one product, every legal mask triple ---------------------------------------------------------
@pytest.mark.parametrize("dims", [(4, 4), (6, 4), (8, 6), (5, 4), (8, 5), (4, 4, 4), (6, 4, 3), (5, 6, 4), (8, 4, 6)])
def test_one_product_every_mask_triple(on, dims):
    """Two levels, one explicit axis mask: level 1 of the device-built solver against level 1 of
    tensor_periodic(host_only=True), pattern exactly and values bit for bit, for every non-zero periodic
    mask, every axis mask that is legal with it -- among them those that leave a periodic axis alone, where
    only the wrap entries of A cross the seam -- and the side masks on the open axes.  Lengths 4 and 6
    give coarse lengths 2 and 3: the left and the right coarse neighbour are one column, or the three
    offsets cover the axis.  The 5- / 7-point rows reach at most 9 / 27 coarse columns of the 16 / 32 a
    lane group holds, so setup_on_device == 1 is asserted on every triple."""
    amg = on
    dim = len(dims)
    axes = [m for m in range(1, 1 << dim) if S.mask_error(dims, dim, m) is None]
    count = seams = alone = 0
    for am, per in itertools.product(axes, range(1, 1 << dim)):
        if PT.level_error(dims, dim, am, per) is not None:
            continue
        for sides in side_masks(dims, per):
            A, Ac, b, singular = op(dims, per, sides)
            what = (dims, am, per, sides)
            dev = amg.Multigrid.tensor_periodic_dev(*dev_arrays(A, b), dims, 2, per, axis_masks=(am,),
                                                    natural_sides=sides, singular=singular, **JAC)
            assert dev.setup_on_device == 1, what
            host = amg.Multigrid.tensor_periodic(Ac.indptr, Ac.indices, Ac.data, b, dims, 2, per, axis_masks=(am,),
                                                 natural_sides=sides, singular=singular, host_only=True, **JAC)
            assert dev.n_levels == host.n_levels == 2, what
            assert dev.level_dims(0) == host.level_dims(0) and dev.level_dims(1) == host.level_dims(1), what
            assert dev.level_axes(0) == host.level_axes(0) == am, what
            got, want = dev.get_coefficient_matrix(1), host.get_coefficient_matrix(1)
            dev.close()
            host.close()
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what
            assert bits(got[2], want[2]), what
            count += 1
            seams += bool(per & am)
            alone += bool(per & ~am)
    print(f"\n{dims}: {count} (axis mask, periodic mask, side mask) triples bitwise on the device, {seams} with a "
          f"coarsened seam, {alone} with a periodic axis that is not coarsened")
    assert seams > 0 and alone > 0


# ---- 2. deep hierarchies ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", [DEEP2, DEEP3, XY, X_DIR, FORMS, XYZ],
                         ids=["16x16-4", "8x8x8-3", "64x48-xy", "32x21-x", "32x20-masks", "16x12x8-xyz"])
def test_deep_hierarchy_equals_host_constructor(on, case):
    """Every level, transfer, two V-cycles and PCG to 1e-8 against the host constructor.  16 x 16 / 4 and
    8 x 8 x 8 / 3 end on coarse length 2 after products on 9- / 27-point Galerkin levels whose wraps
    and neighbours meet."""
    amg = on
    dev, host = case_pair(amg, case)
    assert dev.n_levels == case[1]
    assert_same_hierarchy(dev, host, case)
    assert_same_cycles(dev, host, case)
    n = dev.get_n_dofs(0)
    out = []
    for mg in (dev, host):
        mg.set_vec(0, "u", np.zeros(n))
        out.append(mg.pcg(1e-8, 100))
    dev.close()
    host.close()
    (x, it, rel), (xh, ith, relh) = out
    print(f"\n{case[0]}/{case[1]} periodic {case[3]}: PCG {it} iterations, relres {rel:.3e} (host-built {ith}, {relh:.3e})")
    assert relh <= 1e-8
    assert it == ith and rel == relh and bits(x, xh), case


# ---- 3. forms that read the lazily rebuilt P / R or the float copies ---------------------------------
def test_forms_on_a_device_built_solver(on):
    torch = pytest.importorskip("torch")
    amg = on
    dims, nl, masks, per, _ = FORMS
    _, _, b, _ = op(dims, per)
    n = b.size
    for name, sm in (("chebyshev(2) 1+1", dict(smoother=amg.SM_CHEBYSHEV, smoother_iters=1, cheb_degree=2)),
                     ("line Jacobi 1+1", dict(smoother=amg.SM_LINE_JACOBI, smoother_iters=1, omega=0.7))):
        dev, host = case_pair(amg, FORMS, **sm)
        assert_same_hierarchy(dev, host, name)
        assert_same_cycles(dev, host, name)
        dev.close()
        host.close()
    dev, host = case_pair(amg, FORMS)
    out = []
    for mg in (dev, host):
        mg.set_vec(0, "u", np.zeros(n))
        out.append(mg.pcg_mixed(1e-8, 100))
    (x, it, rel), (xh, ith, relh) = out
    print(f"\n{dims}/{nl}: pcg_mixed {it} iterations, relres {rel:.3e} (host-built {ith}, {relh:.3e})")
    assert relh <= 1e-8 and it == ith and rel == relh and bits(x, xh)
    rng = np.random.default_rng(11)
    B = rng.standard_normal((n, 3))
    B -= B.mean(axis=0)
    out = []
    for mg in (dev, host):
        X, itb, relb = mg.block_pcg(torch.from_numpy(np.ascontiguousarray(B)).cuda(), rtol=1e-8, max_iters=100)
        torch.cuda.synchronize()
        out.append((X.cpu().numpy(), np.array(itb), np.array(relb)))
    dev.close()
    host.close()
    (X, itb, relb), (Xh, itbh, relbh) = out
    print(f"  block_pcg on 3 columns: {itb.tolist()} iterations (host-built {itbh.tolist()})")
    assert np.all(relbh <= 1e-8)
    assert np.array_equal(itb, itbh) and bits(relb, relbh) and bits(X, Xh)


# ---- 4. operators that stress the order of the sum --------------------------------------------------
def upwind(dims, per, sides=0, c=(3.0, 1.5, 0.75)):
    """periodic_twin.diffusion plus a first-order upwind term c . grad u, c > 0 on every axis: +c_a on the
    diagonal and -c_a on the lower neighbour along axis a (the wrapped one on a periodic axis; none at a
    low boundary).  The pattern is the diffusion's; the operator is not symmetric."""
    dirichlet = PT.open_sides(len(dims), per) & ~sides
    A = sp.lil_matrix(PT.diffusion(dims, per, dirichlet))
    d3 = T.dims3(dims)
    stride = (1, d3[0], d3[0] * d3[1])
    for i in range(A.shape[0]):
        co = (i % d3[0], (i // d3[0]) % d3[1], i // (d3[0] * d3[1]))
        for a in range(len(dims)):
            if co[a] > 0:
                j = i - stride[a]
            elif (per >> a) & 1:
                j = i + (d3[a] - 1) * stride[a]
            else:
                j = None
            A[i, i] += c[a]
            if j is not None:
                assert A[i, j] != 0.0
                A[i, j] -= c[a]
    return sp.csr_matrix(A), PT.rhs(A.shape[0], False)


def stored_zeros(dims, per):
    """periodic_twin.diffusion with every second wrap entry along x (rows and columns on even grid
    lines) set to 0.0 and kept in the pattern, in both triangles."""
    A = sp.csr_matrix(PT.diffusion(dims, per, PT.open_sides(len(dims), per)))
    A.sort_indices()
    nx = dims[0]
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    wrap = (np.abs(A.indices % nx - rows % nx) == nx - 1) & ((rows // nx) % 2 == 0)
    assert wrap.sum() > 0
    A.data[wrap] = 0.0
    assert A.nnz == rows.size and np.count_nonzero(A.data == 0.0) == wrap.sum()
    return A, PT.rhs(A.shape[0], False)


def test_nonsymmetric_operator(on):
    """Diffusion plus upwind convection on 32 x 21, periodic in x, and on 8 x 8 x 8, periodic in x and y
    (Dirichlet on the other sides): the levels are not symmetric, the device path takes K-Transpose for
    the column form, and the sums keep the host's order."""
    amg = on
    for dims, nl, per in (((32, 21), 4, 1), ((8, 8, 8), 3, 3)):
        A, b = upwind(dims, per)
        assert abs(A - A.T).max() > 1.0
        A, Ac, b = frozen(A, b)
        dev, host = pair(amg, A, Ac, b, dims, nl, per)
        assert_same_hierarchy(dev, host, dims)
        assert_same_cycles(dev, host, dims)
        dev.close()
        host.close()


def test_stored_exact_zeros(on):
    amg = on
    dims, nl, per = (16, 12), 3, 1
    A, b = stored_zeros(dims, per)
    A, Ac, b = frozen(A, b)
    assert Ac.nnz == A.nnz
    for kw in (dict(), dict(keep_structural_zeros=True)):
        dev, host = pair(amg, A, Ac, b, dims, nl, per, **kw)
        assert_same_hierarchy(dev, host, kw)
        assert_same_cycles(dev, host, kw)
        dev.close()
        host.close()


def test_layouts(on):
    amg = on
    for layout in (amg.LAYOUT_AUTO, amg.LAYOUT_CSR, amg.LAYOUT_SELL):
        dev, host = case_pair(amg, XY, layout=layout)
        assert [dev.level_layout(l) for l in range(XY[1])] == [host.level_layout(l) for l in range(XY[1])], layout
        assert_same_hierarchy(dev, host, layout)
        assert_same_cycles(dev, host, layout)
        dev.close()
        host.close()


# ---- 5. the switch ----------------------------------------------------------------------------------
def test_switch_off_is_the_host_path_and_the_same_solver(on):
    amg = on
    dims, nl, masks, per, sides = XY
    A, Ac, b, singular = op(dims, per, sides)
    dev, host = case_pair(amg, XY)
    amg.set_periodic_device_setup(0)
    off = amg.Multigrid.tensor_periodic_dev(*dev_arrays(A, b), dims, nl, per, axis_masks=masks, natural_sides=sides,
                                            singular=singular, **JAC)
    amg.set_periodic_device_setup(1)
    assert off.setup_on_device == 0
    assert_same_hierarchy(dev, off, "switch off")
    assert_same_hierarchy(dev, host, "host")
    dev.vcycle(2)
    off.vcycle(2)
    assert same_state(state(dev), state(off))
    for mg in (dev, off, host):
        mg.close()


def test_malformed_arrays_are_refused_with_the_switch_on(on):
    amg = on
    dims, nl, masks, per, sides = X_DIR
    A, _, b, singular = op(dims, per, sides)
    arrs = dev_arrays(A, b)
    bad = arrs[1].copy()
    bad[3] = -1
    with pytest.raises(ValueError, match="malformed"):
        amg.Multigrid.tensor_periodic_dev(arrs[0], bad, arrs[2], arrs[3], dims, nl, per, axis_masks=masks,
                                          natural_sides=sides, singular=singular, **JAC)


def test_wide_operator_falls_back_silently(on):
    """A 13-point operator (couplings at distance 1 and 2 along both periodic axes and the four diagonal
    neighbours) on 16 x 16: a coarse row reaches 5 x 5 coarse columns, more than the 16 a lane group holds.
    The product is refused as a whole and the host constructor builds the same solver."""
    amg = on
    dims, per = (16, 16), 3
    n = 256
    i = np.arange(n)
    x, y = i % 16, i // 16
    rows, cols, vals = [i], [i], [np.full(n, 6.0)]
    for dx, dy, w in [(s * d, 0, w) for d, w in ((1, -1.0), (2, -0.25)) for s in (1, -1)] + \
                     [(0, s * d, w) for d, w in ((1, -1.0), (2, -0.25)) for s in (1, -1)] + \
                     [(sx, sy, -0.125) for sx in (1, -1) for sy in (1, -1)]:
        rows.append(i)
        cols.append(((y + dy) % 16) * 16 + (x + dx) % 16)
        vals.append(np.full(n, w))
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    assert np.all(np.diff(A.indptr) == 13)
    A, Ac, b = frozen(A, PT.rhs(n, False))
    dev = amg.Multigrid.tensor_periodic_dev(*dev_arrays(A, b), dims, 2, per, **JAC)
    host = amg.Multigrid.tensor_periodic(Ac.indptr, Ac.indices, Ac.data, b, dims, 2, per, **JAC)
    assert dev.setup_on_device == 0 and host.setup_on_device == 0
    assert_same_hierarchy(dev, host, "13-point")
    assert np.diff(host.get_coefficient_matrix(1)[0]).max() > 16  # the rows themselves are too long as well
    dev.close()
    host.close()
