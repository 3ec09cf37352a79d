"""amg_hip_create_tensor_opdep_dev: operator-dependent interpolation with the set-up on the device
(K-AxisWeights, K-AxisGalerkin) against the host constructor amg_hip_create_tensor_opdep on the same
matrix, bit for bit: axes, dims, transfer kinds, the compact weights, P, R and every level matrix --
values compared as uint64 words, so that -0.0 and +0.0 differ -- then the cycle, amg_hip_apply and the
PCG drivers.  The operators are tests/opdep_twin.py's.

Grids: the smallest at which the index rules differ -- an axis of 2 points (one coarse point, fine
point 0 with a high neighbour only), of 3, odd lengths (the last fine point has a low neighbour only)
and even ones, an axis that cannot be coarsened any more, every axis, more than one workgroup (64 x 48:
3072 / 16 coarse rows per 16-row workgroup; 17 x 12 x 9), and levels whose rows are not their columns
(nonsymmetric: K-Transpose).  The structural rule is pinned by an operator cut along a plane, whose
weights across the cut are stored zeros, once with the cut entries absent and once stored as 0.0."""
import os
import sys

import numpy as np
import pytest

sp = pytest.importorskip("scipy.sparse")
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import opdep_twin as O  # noqa: E402
import semi_twin as S  # noqa: E402
from test_gpu_tensor_opdep import TWIN_PCG  # noqa: E402

pytestmark = pytest.mark.gpu

JAC = dict(smoother=3, smoother_iters=2, omega=0.8)
SMOOTHERS = {"jacobi": JAC, "chebyshev": dict(smoother=5, smoother_iters=1, cheb_degree=2),
             "line_alt": dict(smoother=7, smoother_iters=1, omega=0.8)}
SELL = 2
GRIDS = [(7, 5), (8, 3), (2, 9), (3, 2), (33, 20), (64, 48), (5, 4, 3), (17, 12, 9)]
HOST, DEV = "amg_hip_create_tensor_opdep: ", "amg_hip_create_tensor_opdep_dev: "


def csr_arrays(A):
    M = sp.csr_matrix(A, dtype=np.float64)
    M.sort_indices()
    return M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.astype(np.float64)


def csc_arrays(A):
    """CSC by hand: the stored entries of the CSR form, explicit zeros included, sorted by (column, row)"""
    rp, ci, v = csr_arrays(A)
    n = rp.size - 1
    row = np.repeat(np.arange(n, dtype=np.int32), np.diff(rp))
    order = np.lexsort((row, ci))
    cp = np.zeros(n + 1, np.int64)
    np.add.at(cp, ci.astype(np.int64) + 1, 1)
    return np.cumsum(cp).astype(np.int32), row[order], v[order]


def chain(dims):
    """x, y, (z,) x, ... down to the last possible level: an axis of one point is passed over"""
    d, dim, masks, a, idle = list(dims), len(dims), [], 0, 0
    while idle < dim:
        if d[a] >= 2:
            masks.append(1 << a)
            d[a] //= 2
            idle = 0
        else:
            idle += 1
        a = (a + 1) % dim
    return masks


def levels_of(masks):
    return O.MAX_LEVELS if masks is None else len(masks) + 1


def host(amg, A, b, dims, masks=None, **kw):
    opts = dict(JAC)
    opts.update(kw)
    return amg.Multigrid.tensor_opdep(*csc_arrays(A), b, dims, opts.pop("n_levels", levels_of(masks)), axis_masks=masks,
                                      min_coarse=O.MIN_COARSE, **opts)


def dev(amg, A, b, dims, masks=None, **kw):
    opts = dict(JAC)
    opts.update(kw)
    return amg.Multigrid.tensor_opdep_dev(*csr_arrays(A), np.array(b), dims, opts.pop("n_levels", levels_of(masks)),
                                          axis_masks=masks, min_coarse=O.MIN_COARSE, **opts)


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def same_matrix(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2].shape == b[2].shape and
            np.array_equal(bits(a[2]), bits(b[2])))


def state(mg):
    mg.sync()
    return [(mg.get_soln(l), mg.get_rhs(l)) for l in range(mg.n_levels)]


def same_state(a, b):
    return len(a) == len(b) and all(np.array_equal(bits(x[0]), bits(y[0])) and np.array_equal(bits(x[1]), bits(y[1]))
                                    for x, y in zip(a, b))


def compare(hs, dv, what, on_device=1, kind=3):
    """comparison 1 of the module: the two hierarchies, then one V-cycle on both"""
    assert hs.setup_on_device == 0 and dv.setup_on_device == on_device, what
    nl = hs.n_levels
    assert dv.n_levels == nl, (what, nl, dv.n_levels)
    assert [tuple(dv.level_dims(l)) for l in range(nl)] == [tuple(hs.level_dims(l)) for l in range(nl)], what
    assert [dv.level_axes(l) for l in range(nl - 1)] == [hs.level_axes(l) for l in range(nl - 1)], what
    assert [dv.level_transfer_kind(l) for l in range(nl - 1)] == [kind] * (nl - 1), what
    assert [hs.level_transfer_kind(l) for l in range(nl - 1)] == [kind] * (nl - 1), what
    for l in range(nl):
        assert same_matrix(hs.get_coefficient_matrix(l), dv.get_coefficient_matrix(l)), (what, "A", l)
    for l in range(nl - 1):
        Wh, Wd = hs.axis_weights(l), dv.axis_weights(l)
        assert Wh.shape == Wd.shape and np.array_equal(bits(Wh), bits(Wd)), (what, "W", l)
        for which in ("P", "R"):
            assert same_matrix(hs.get_transfer(l, which), dv.get_transfer(l, which)), (what, which, l)
    hs.vcycle(1)
    dv.vcycle(1)
    got, ref = state(dv), state(hs)
    assert all(np.all(np.isfinite(u)) for u, _ in ref) and np.linalg.norm(ref[0][0]) > 0, what
    assert same_state(got, ref), (what, "V-cycle")


def pair(amg, A, b, dims, masks, what, on_device=1, kind=3, **kw):
    hs = host(amg, A, b, dims, masks, **kw)
    dv = dev(amg, A, b, dims, masks, **kw)
    try:
        compare(hs, dv, what, on_device, kind)
    finally:
        hs.close()
        dv.close()


# ---- 1. set-up parity, explicit masks ---------------------------------------------------------------
@pytest.mark.parametrize("operator", ["jump", "nonsymmetric"])
@pytest.mark.parametrize("dims", GRIDS)
def test_setup_parity_with_explicit_masks(amg, dims, operator):
    A = O.jump(dims, contrast=4)
    if operator == "nonsymmetric":
        A = O.nonsymmetric(A, dims)
    b = S.rhs(A.shape[0])
    masks = chain(dims)
    assert masks[:2] == [1, 2] and len(masks) == sum(int(m).bit_length() - 1 for m in dims)
    pair(amg, A, b, dims, masks, (dims, operator))


# ---- 2. the structural rule --------------------------------------------------------------------------
def cut(A, dims, store_zero):
    """every coupling across the plane between the x-coordinates 4 and 5 cut, the diagonal unchanged: the cut
    entries stored as 0.0, or absent from the pattern"""
    nx = dims[0]
    rp, ci, v = csr_arrays(A)
    n = rp.size - 1
    row = np.repeat(np.arange(n), np.diff(rp))
    rx, cx = row % nx, ci % nx
    k = ((rx <= 4) & (cx >= 5)) | ((rx >= 5) & (cx <= 4))
    assert k.any() and not (row[k] == ci[k]).any()
    if store_zero:
        v = v.copy()
        v[k] = 0.0
        return sp.csr_matrix((v, ci, rp), shape=(n, n))
    keep = ~k
    ptr = np.zeros(n + 1, np.int64)
    np.add.at(ptr, row[keep] + 1, 1)
    return sp.csr_matrix((v[keep], ci[keep], np.cumsum(ptr).astype(np.int32)), shape=(n, n))


@pytest.mark.parametrize("store_zero", [False, True], ids=["absent", "stored-zero"])
@pytest.mark.parametrize("dims", [(12, 10), (9, 8, 6)])
def test_structure_is_geometric_not_numeric(amg, dims, store_zero):
    A = cut(O.jump(dims, contrast=4), dims, store_zero)
    assert (A.data == 0.0).any() == store_zero
    b = S.rhs(A.shape[0])
    masks = [1, 2, 1] if len(dims) == 2 else [1, 2, 4, 1]
    hs = host(amg, A, b, dims, masks)
    try:  # else the case shows nothing
        assert (hs.get_transfer(0, "P")[2] == 0.0).any(), "no stored zero weight in P_0"
        assert (hs.get_coefficient_matrix(1)[2] == 0.0).any(), "no stored exact zero in A_1"
    finally:
        hs.close()
    pair(amg, A, b, dims, masks, (dims, store_zero))


# ---- 3. automatic masks ------------------------------------------------------------------------------
@pytest.mark.parametrize("smoother", ["jacobi", "chebyshev"])
@pytest.mark.parametrize("dims", [(64, 48), (24, 20, 16)])
def test_automatic_masks(amg, dims, smoother):
    A, b, tw = O.case(dims)
    hs = host(amg, A, b, dims, None, **SMOOTHERS[smoother])
    dv = dev(amg, A, b, dims, None, **SMOOTHERS[smoother])
    try:
        assert [dv.level_axes(l) for l in range(dv.n_levels - 1)] == [hs.level_axes(l) for l in range(hs.n_levels - 1)]
        assert [hs.level_axes(l) for l in range(hs.n_levels - 1)] == tw.masks
        compare(hs, dv, (dims, smoother))
    finally:
        hs.close()
        dv.close()


# ---- 4. smoothers and solvers on a device-built hierarchy -------------------------------------------
def apply_once(mg, b):
    dv = torch.from_numpy(np.array(b)).cuda()
    dz = torch.empty_like(dv)
    mg.apply_dev(dv.data_ptr(), dz.data_ptr())
    mg.sync()
    return dz.cpu().numpy()


@pytest.mark.parametrize("smoother", sorted(SMOOTHERS))
@pytest.mark.parametrize("dims", [(33, 20), (17, 12, 9)])
def test_apply_and_pcg_equal_the_host_built_solver(amg, dims, smoother):
    A, b, tw = O.case(dims)
    kw = SMOOTHERS[smoother]
    out = {}
    for name, make in (("host", host), ("dev", dev)):
        mg = make(amg, A, b, dims, None, **kw)
        assert mg.setup_on_device == (name == "dev") and mg.n_levels == tw.nl
        z = apply_once(mg, b)
        x, it, rel = mg.pcg(1e-8, 200)
        out[name] = (z, x, it, rel)
        mg.close()
    (zh, xh, ith, relh), (zd, xd, itd, reld) = out["host"], out["dev"]
    print(f"\n{dims} {smoother}: PCG {ith} (host-built) / {itd} (device-built) iterations, relres {relh:.2e}")
    assert np.all(np.isfinite(zh)) and np.linalg.norm(zh) > 0 and relh <= 1e-8
    assert np.array_equal(bits(zd), bits(zh)), "amg_hip_apply"
    assert itd == ith and np.array_equal(bits(xd), bits(xh)) and reld == relh, "amg_hip_pcg"


@pytest.mark.parametrize("dims", [(33, 20), (17, 12, 9)])
def test_block_and_mixed_pcg_use_the_lazy_csr_transfers(amg, dims):
    """block_pcg (k = 3) and pcg_mixed take the CSR kernels on kind-3 levels: CSR(P), CSR(R) of a device-built
    level are made from the downloaded weights at that moment."""
    A, b, _ = O.case(dims)
    B0 = np.random.default_rng(11).standard_normal((b.size, 3))
    B0[:, 0] = b
    out = {}
    for name, make in (("host", host), ("dev", dev)):
        mg = make(amg, A, b, dims, None)
        X, it, rel = mg.block_pcg(torch.from_numpy(np.ascontiguousarray(B0)).cuda(), None, 1e-8, 100)
        torch.cuda.synchronize()
        blk = (X.cpu().numpy(), list(it))
        mg.close()
        mg = make(amg, A, b, dims, None, layout=SELL)  # the float cycle's layout
        assert mg.setup_on_device == (name == "dev")
        x32, it32, rel32 = mg.pcg_mixed(1e-8, 200)
        mg.close()
        out[name] = (blk, x32, it32, rel32)
    (bh, xh, ith, relh), (bd, xd, itd, reld) = out["host"], out["dev"]
    assert bd[1] == bh[1] and np.array_equal(bits(bd[0]), bits(bh[0])), "amg_hip_block_pcg"
    assert relh <= 1e-8 and itd == ith and reld == relh and np.array_equal(bits(xd), bits(xh)), "amg_hip_pcg_mixed"


@pytest.mark.parametrize("dims", [(64, 48), (24, 20, 16)])
def test_pcg_counts_on_a_device_built_hierarchy(amg, dims):
    """the float64 twin's counts of tests/test_gpu_tensor_opdep.py: 10 at (64, 48), 9 at (24, 20, 16)"""
    A, b, tw = O.case(dims)
    mg = dev(amg, A, b, dims, None)
    assert mg.setup_on_device == 1 and mg.n_levels == tw.nl
    x, it, rel = mg.pcg(1e-8, 200)
    mg.close()
    true = float(np.linalg.norm(b - A @ x) / np.linalg.norm(b))
    print(f"\n{dims}: PCG {it} iterations (twin {TWIN_PCG[dims]}), relres {rel:.2e}, true {true:.2e}")
    assert rel <= 1e-8 and true <= 2e-8
    assert it == TWIN_PCG[dims]


# ---- 5. singular ---------------------------------------------------------------------------------------
def test_singular_system_with_the_mean_projection(amg):
    dims = (64, 48)
    A = O.jump(dims, contrast=4, natural=True, shift=0.0)
    b = S.rhs(A.shape[0])
    out = {}
    for name, make in (("host", host), ("dev", dev)):
        mg = make(amg, A, b, dims, None, natural_sides=15, singular=True)
        assert mg.setup_on_device == (name == "dev") and mg.natural_sides() == 15
        mg.set_mean_projection(1)
        out[name] = mg.pcg(1e-8, 200)
        mg.close()
    (xh, ith, relh), (xd, itd, reld) = out["host"], out["dev"]
    print(f"\nsingular {dims}: PCG {ith} / {itd} iterations, relres {relh:.2e}")
    assert relh <= 1e-8 and np.all(np.isfinite(xh))
    assert itd == ith and reld == relh and np.array_equal(bits(xd), bits(xh))


# ---- 6. fallbacks --------------------------------------------------------------------------------------
def test_fallbacks_take_the_host_constructor(amg):
    dims = (12, 10)
    A = O.jump(dims, contrast=4)
    b = S.rhs(A.shape[0])
    masks = [1, 2, 1]
    pair(amg, A, b, dims, masks, "stencil_transfers = 0", on_device=0, kind=0, stencil_transfers=False)
    try:
        amg.set_axis_stencil(False)
        pair(amg, A, b, dims, masks, "set_axis_stencil(0)", on_device=0, kind=0)
    finally:
        amg.set_axis_stencil(True)
    pair(amg, A, b, dims, masks, "smoother 0", on_device=0, smoother=0, smoother_iters=1, omega=1.0)
    pair(amg, A, b, dims, [], "one level", on_device=0, n_levels=1)
    A2 = sp.csr_matrix(A @ A)  # 13-point: the box of a coarse row holds 5 x 5 = 25 columns, the lane group 16
    A2.sort_indices()
    assert np.diff(A2.indptr).max() == 13
    pair(amg, A2, b, dims, masks, "box overflow", on_device=0)
    pair(amg, A, b, dims, masks, "the device path, for contrast", on_device=1)


# ---- 7. refusals ---------------------------------------------------------------------------------------
def five_point(dims):
    nx, ny = dims
    T = lambda m: sp.diags([-np.ones(m - 1), np.zeros(m), -np.ones(m - 1)], [-1, 0, 1])  # noqa: E731
    A = (sp.kron(sp.identity(ny), T(nx)) + sp.kron(T(ny), sp.identity(nx)) + 4.0 * sp.identity(nx * ny)).tolil()
    return A


def refusal(make, amg, A, b, dims, masks):
    with pytest.raises(ValueError) as e:
        make(amg, sp.csr_matrix(A), b, dims, masks).close()
    return str(e.value)


def test_refusals_are_worded_by_the_host_constructor(amg):
    dims = (8, 6)
    b = np.ones(48)
    row = lambda x, y: y * dims[0] + x  # noqa: E731
    # s_0 of an even-x row, collapsed onto x: the diagonal and the two y-neighbours, 2 - 1 - 1 = 0 exactly
    A = five_point(dims)
    A[row(4, 2), row(4, 2)] = 2.0
    mh, md = refusal(host, amg, A, b, dims, [1]), refusal(dev, amg, A, b, dims, [1])
    print("\n" + md)
    assert md == mh.replace(HOST, DEV) and md.startswith(DEV + "level 0: row 20: the diagonal sum s_0 is 0")
    # a second such row earlier in the matrix: the smaller row is the one named
    A[row(2, 1), row(2, 1)] = 2.0
    mh, md = refusal(host, amg, A, b, dims, [1]), refusal(dev, amg, A, b, dims, [1])
    print(md)
    assert md == mh.replace(HOST, DEV) and "level 0: row 10: " in md
    # every entry finite, w_lo = (-s_m) / s_0 = -1e308 / 1e-10 overflows
    A = five_point(dims)
    A[row(4, 2), row(3, 2)] = 1e308
    A[row(4, 2), row(4, 2)] = 2.0 + 1e-10
    mh, md = refusal(host, amg, A, b, dims, [1]), refusal(dev, amg, A, b, dims, [1])
    print(md)
    assert md == mh.replace(HOST, DEV) and "level 0: row 20: the weight w_lo is " in md and "inf" in md
    # a mask chain whose level 1 is impossible: y has 3 points, then 1
    A = five_point((8, 3))
    mh, md = refusal(host, amg, A, np.ones(24), (8, 3), [2, 2]), refusal(dev, amg, A, np.ones(24), (8, 3), [2, 2])
    print(md)
    assert md == mh.replace(HOST, DEV) and md.startswith(DEV) and "level 1" in md
