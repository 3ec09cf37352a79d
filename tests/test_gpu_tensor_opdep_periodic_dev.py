"""amg_hip_create_tensor_opdep_periodic_dev with amg_hip_set_periodic_device_setup(1): the hierarchy is built on
the device by the seam forms of K-AxisWeights and K-AxisGalerkin, and equals the host constructor
amg_hip_create_tensor_opdep_periodic on the same matrix bit for bit.  The comparison is the `compare` of
tests/test_gpu_tensor_opdep_dev.py (n_levels, dims, axes, transfer kinds, the compact weights, P, R and every
level matrix as uint64 words, then one V-cycle), with the periodic mask, amg_hip_apply and amg_hip_pcg on top.

Every test turns the switch on through the fixture `on` and back to 0 in its teardown.  setup_on_device == 1 is
a condition of every comparison of the device path -- on a library without the seam kernels those assertions fail,
for a silent fall-back would compare the host product with itself.

Grids (tests/opdep_periodic_dev_cases.py): the smallest at which the seam can go wrong -- coarse length 2, where
the left and the right coarse neighbour of a coarse row are one column; one line; a periodic y with an odd open
x, both rules in one chain; 3-D; more than one workgroup with a partial last one on a coarser level.  The masks
alternate x, y, (z,) ..., so that every periodic axis is also seen on a level that does not coarsen it: its wrap
entries then exercise the cyclic box.  That the nonsymmetric operator tells a wrong seam from a right one is
shown without a GPU in tests/test_tensor_opdep_periodic_dev_seam.py."""
import os
import sys

import numpy as np
import pytest

sp = pytest.importorskip("scipy.sparse")
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import opdep_periodic_dev_cases as K  # noqa: E402
import opdep_periodic_twin as OP  # noqa: E402
import opdep_twin as O  # noqa: E402
from test_gpu_tensor_opdep_dev import (JAC, SELL, apply_once, bits, compare, csc_arrays, csr_arrays,  # noqa: E402
                                       same_matrix)
from test_gpu_tensor_opdep_dev import dev as open_dev  # noqa: E402
from test_gpu_tensor_opdep_periodic import TWIN_PCG  # noqa: E402

pytestmark = pytest.mark.gpu

SMOOTHERS = {"jacobi": JAC, "chebyshev": dict(smoother=5, smoother_iters=1, cheb_degree=2),
             "line": dict(smoother=6, smoother_iters=1, omega=0.8), "line_alt": dict(smoother=7, smoother_iters=1, omega=0.8)}
HOST, DEV = "amg_hip_create_tensor_opdep_periodic: ", "amg_hip_create_tensor_opdep_periodic_dev: "


@pytest.fixture
def on(amg):
    amg.set_periodic_device_setup(1)
    try:
        yield amg
    finally:
        amg.set_periodic_device_setup(0)


def levels_of(masks):
    return O.MAX_LEVELS if masks is None else len(masks) + 1


def host(amg, A, b, dims, per, masks, **kw):
    opts = dict(JAC)
    opts.update(kw)
    return amg.Multigrid.tensor_opdep_periodic(*csc_arrays(A), b, dims, opts.pop("n_levels", levels_of(masks)), per,
                                               axis_masks=masks, min_coarse=O.MIN_COARSE, **opts)


def dev(amg, A, b, dims, per, masks, **kw):
    opts = dict(JAC)
    opts.update(kw)
    return amg.Multigrid.tensor_opdep_periodic_dev(*csr_arrays(A), np.array(b), dims,
                                                   opts.pop("n_levels", levels_of(masks)), per, axis_masks=masks,
                                                   min_coarse=O.MIN_COARSE, **opts)


def compare_all(hs, dv, b, per, what, on_device=1, kind=3):
    """the hierarchies and one V-cycle (compare), then amg_hip_apply and amg_hip_pcg"""
    assert hs.periodic_axes() == per and dv.periodic_axes() == per, what
    compare(hs, dv, what, on_device, kind)
    zh, zd = apply_once(hs, b), apply_once(dv, b)
    assert np.all(np.isfinite(zh)) and np.linalg.norm(zh) > 0, what
    assert np.array_equal(bits(zd), bits(zh)), (what, "amg_hip_apply")
    (xh, ith, relh), (xd, itd, reld) = hs.pcg(1e-8, 60), dv.pcg(1e-8, 60)
    assert itd == ith and np.array_equal(bits(xd), bits(xh)) and bits(reld) == bits(relh), (what, "amg_hip_pcg")


def pair(amg, A, b, dims, per, masks, what, on_device=1, kind=3, **kw):
    hs = host(amg, A, b, dims, per, masks, **kw)
    dv = dev(amg, A, b, dims, per, masks, **kw)
    try:
        compare_all(hs, dv, b, per, what, on_device, kind)
    finally:
        hs.close()
        dv.close()


# ---- 1. set-up parity, explicit masks ---------------------------------------------------------------------
@pytest.mark.parametrize("operator", ["jump", "nonsymmetric"])
@pytest.mark.parametrize("dims,per", K.GRIDS)
def test_setup_parity_with_explicit_masks(on, dims, per, operator):
    A, b, singular = K.case(operator, dims, per)
    masks = K.chain(dims, per)
    seen = {m: [l for l, k in enumerate(masks) if k == m] for m in set(masks)}
    assert any(m & per for m in masks), "no level coarsens a periodic axis"
    print(f"\n{dims} per {per}: masks {masks}, levels per axis {seen}")
    pair(on, A, b, dims, per, masks, (dims, per, operator), singular=singular)


@pytest.mark.parametrize("operator", ["jump", "nonsymmetric"])
def test_y_coarsened_twice_while_x_wraps(on, operator):
    dims, per, masks = (32, 16), 1, [2, 2, 1]
    A, b, singular = K.case(operator, dims, per)
    pair(on, A, b, dims, per, masks, (dims, per, operator), singular=singular)


# ---- 2. the structural rule at the seam ---------------------------------------------------------------------
@pytest.mark.parametrize("store_zero", [False, True], ids=["absent", "stored-zero"])
@pytest.mark.parametrize("dims,per", [((8, 6), 1), ((8, 4, 4), 5)])
def test_zero_seam_weights_are_kept_as_entries(on, dims, per, store_zero):
    """no coupling across the seam of x: w_lo of fine 0, the one weight that crosses it, comes out +-0.0 on every
    line and stays an entry of W, of P and -- coarse row m / 2 - 1, column 0 -- of the level matrix"""
    A = K.without_wrap(K.case("jump", dims, per)[0], dims, 0, store_zero)
    assert (A.data == 0.0).any() == store_zero
    b = K.S.rhs(A.shape[0])
    masks = K.chain(dims, per)
    assert masks[0] == 1
    hs = host(on, A, b, dims, per, masks)
    try:  # else the case shows nothing
        W = hs.axis_weights(0)
        assert np.all(W[::dims[0] // 2, 0] == 0.0) and np.count_nonzero(W == 0.0) == W.shape[0] // (dims[0] // 2), \
            "the seam weights, and only they, are zero"
        P = hs.get_transfer(0, "P")
        assert np.all(np.diff(P[0]) == 3) and (P[2] == 0.0).any(), "a zero weight left P_0"
        assert (hs.get_coefficient_matrix(1)[2] == 0.0).any(), "no stored exact zero in A_1"
    finally:
        hs.close()
    pair(on, A, b, dims, per, masks, (dims, per, store_zero))


# ---- 3. automatic masks ------------------------------------------------------------------------------------
def ineligible_before_the_end(mg, per):
    """levels l that still coarsen on which a periodic axis is odd or shorter than 4"""
    out = []
    for l in range(mg.n_levels - 1):
        d = mg.level_dims(l)
        if any((per >> a) & 1 and (d[a] < 4 or d[a] % 2) for a in range(3)):
            out.append(l)
    return out


@pytest.mark.parametrize("smoother", ["jacobi", "chebyshev"])
@pytest.mark.parametrize("dims,per", [((64, 48), 3), ((24, 20, 16), 7)])
def test_automatic_masks(on, dims, per, smoother):
    """(24, 20, 16) per 7 (host_only, on the CPU): masks 1 2 4 4 2 1 4 1; y reaches 5 on level 5 and the rule goes on
    with x and z, z reaches 2 on level 7 and x is still coarsened.  (64, 48) per 3 ends at (8, 3) with 24 rows <=
    min_coarse: no axis becomes ineligible before that."""
    A, b, singular = K.case("jump", dims, per)
    hs = host(on, A, b, dims, per, None, singular=singular, **SMOOTHERS[smoother])
    dv = dev(on, A, b, dims, per, None, singular=singular, **SMOOTHERS[smoother])
    try:
        if dims == (24, 20, 16):
            assert [hs.level_axes(l) for l in range(hs.n_levels - 1)] == [1, 2, 4, 4, 2, 1, 4, 1]
            assert ineligible_before_the_end(hs, per) == [5, 6, 7]
        compare_all(hs, dv, b, per, (dims, per, smoother))
    finally:
        hs.close()
        dv.close()


# ---- 4. smoothers and solvers on a device-built hierarchy ------------------------------------------------
@pytest.mark.parametrize("smoother", sorted(SMOOTHERS))
@pytest.mark.parametrize("dims,per,nl", [((32, 24), 3, 5), ((16, 16, 16), 7, 7)])
def test_every_smoother_of_the_device_path(on, dims, per, nl, smoother):
    A, b, tw = OP.case(dims, per, nl)
    hs = host(on, A, b, dims, per, tw.masks, singular=True, **SMOOTHERS[smoother])
    dv = dev(on, A, b, dims, per, tw.masks, singular=True, **SMOOTHERS[smoother])
    try:
        compare_all(hs, dv, b, per, (dims, per, smoother))
        x, it, rel = dv.pcg(1e-8, 200)
        print(f"\n{dims} per {per} {smoother}: PCG {it} iterations, relres {rel:.2e}")
        assert rel <= 1e-8 and np.all(np.isfinite(x))
    finally:
        hs.close()
        dv.close()


def test_block_and_mixed_pcg_use_the_lazy_csr_transfers(on):
    """block_pcg (k = 3) and pcg_mixed take the CSR kernels on kind-3 levels: CSR(P), CSR(R) of a device-built level
    are made from the downloaded weights at that moment, in the periodic form"""
    dims, per, nl = (32, 24), 3, 5
    A, b, tw = OP.case(dims, per, nl)
    B0 = np.random.default_rng(11).standard_normal((b.size, 3))
    B0 -= B0.mean(axis=0)
    B0[:, 0] = b
    out = {}
    for name, make in (("host", host), ("dev", dev)):
        mg = make(on, A, b, dims, per, tw.masks, singular=True)
        assert mg.setup_on_device == (name == "dev")
        X, it, rel = mg.block_pcg(torch.from_numpy(np.ascontiguousarray(B0)).cuda(), None, 1e-8, 100)
        torch.cuda.synchronize()
        blk = (X.cpu().numpy(), list(it))
        mg.close()
        mg = make(on, A, b, dims, per, tw.masks, singular=True, layout=SELL)  # the float cycle's layout
        assert mg.setup_on_device == (name == "dev")
        x32, it32, rel32 = mg.pcg_mixed(1e-8, 200)
        mg.close()
        out[name] = (blk, x32, it32, rel32)
    (bh, xh, ith, relh), (bd, xd, itd, reld) = out["host"], out["dev"]
    assert np.all(np.isfinite(bh[0])) and bd[1] == bh[1] and np.array_equal(bits(bd[0]), bits(bh[0])), "amg_hip_block_pcg"
    assert relh <= 1e-8 and itd == ith and reld == relh and np.array_equal(bits(xd), bits(xh)), "amg_hip_pcg_mixed"


def test_mean_projected_pcg_on_the_singular_case(on):
    dims, per, nl = (64, 48), 3, 7
    A, b, tw = OP.case(dims, per, nl)
    out = {}
    for name, make in (("host", host), ("dev", dev)):
        mg = make(on, A, b + 1e-6, dims, per, tw.masks, singular=True)
        assert mg.setup_on_device == (name == "dev")
        mg.set_mean_projection(1)
        out[name] = mg.pcg(1e-8, 200)
        mg.close()
    (xh, ith, relh), (xd, itd, reld) = out["host"], out["dev"]
    print(f"\n{dims} per {per}, b + 1e-6: PCG {ith} / {itd} iterations, relres {relh:.2e}")
    assert relh <= 1e-8 and ith == TWIN_PCG[(dims, per, nl)]
    assert itd == ith and reld == relh and np.array_equal(bits(xd), bits(xh))


@pytest.mark.parametrize("dims,per,nl", sorted(TWIN_PCG))
def test_pcg_counts_on_a_device_built_hierarchy(on, dims, per, nl):
    """the float64 twin's counts of tests/test_gpu_tensor_opdep_periodic.py"""
    A, b, tw = OP.case(dims, per, nl)
    mg = dev(on, A, b, dims, per, tw.masks, singular=K.all_periodic(dims, per))
    assert mg.setup_on_device == 1 and mg.n_levels == nl
    assert [mg.level_transfer_kind(l) for l in range(nl - 1)] == [3] * (nl - 1)
    x, it, rel = mg.pcg(1e-8, 200)
    mg.close()
    true = float(np.linalg.norm(b - A @ x) / np.linalg.norm(b))
    print(f"\n{dims} per {per}: PCG {it} iterations (twin {TWIN_PCG[(dims, per, nl)]}), relres {rel:.2e}, true {true:.2e}")
    assert rel <= 1e-8 and true <= 2e-8
    assert it == TWIN_PCG[(dims, per, nl)]


# ---- 5. paths ---------------------------------------------------------------------------------------------
def same_hierarchy(hs, dv):
    nl = hs.n_levels
    assert dv.n_levels == nl and [dv.level_axes(l) for l in range(nl - 1)] == [hs.level_axes(l) for l in range(nl - 1)]
    for l in range(nl):
        assert same_matrix(hs.get_coefficient_matrix(l), dv.get_coefficient_matrix(l)), ("A", l)
    for l in range(nl - 1):
        assert np.array_equal(bits(hs.axis_weights(l)), bits(dv.axis_weights(l))), ("W", l)
        for which in ("P", "R"):
            assert same_matrix(hs.get_transfer(l, which), dv.get_transfer(l, which)), (which, l)


def test_the_switch_and_the_fallbacks(amg):
    dims, per = (12, 8), 3
    A, b, singular = K.case("jump", dims, per)
    masks = K.chain(dims, per)
    assert masks == [1, 2, 1, 2]  # 12 -> 6 -> 3 and 8 -> 4 -> 2
    amg.set_periodic_device_setup(0)
    pair(amg, A, b, dims, per, masks, "switch off", on_device=0, singular=singular)
    try:
        amg.set_periodic_device_setup(1)
        pair(amg, A, b, dims, per, masks, "switch on", on_device=1, singular=singular)
        pair(amg, A, b, dims, per, masks, "multicolour", on_device=0, singular=singular, smoother=amg.SM_MULTICOLOR_GS,
             smoother_iters=1, omega=1.0)
        pair(amg, A, b, dims, per, masks, "stencil_transfers = 0", on_device=0, kind=0, singular=singular,
             stencil_transfers=False)
        try:
            amg.set_axis_stencil(False)
            pair(amg, A, b, dims, per, masks, "set_axis_stencil(0)", on_device=0, kind=0, singular=singular)
        finally:
            amg.set_axis_stencil(True)
        hs = host(amg, A, b, dims, per, masks, singular=singular, host_only=True)
        dv = dev(amg, A, b, dims, per, masks, singular=singular, host_only=True)
        try:
            assert hs.setup_on_device == 0 and dv.setup_on_device == 0
            same_hierarchy(hs, dv)
        finally:
            hs.close()
            dv.close()
    finally:
        amg.set_periodic_device_setup(0)


@pytest.mark.parametrize("dims", [(7, 5), (12, 10), (5, 4, 3)])
def test_no_periodic_axis_is_tensor_opdep_dev(on, dims):
    A = O.nonsymmetric(O.jump(dims, contrast=4), dims)
    b = K.S.rhs(A.shape[0])
    masks = K.chain(dims, 0)
    dv = dev(on, A, b, dims, 0, masks)
    od = open_dev(on, A, b, dims, masks)
    try:
        assert dv.setup_on_device == 1 and od.setup_on_device == 1 and dv.periodic_axes() == 0
        nl = od.n_levels
        assert [dv.level_transfer_kind(l) for l in range(nl - 1)] == [3] * (nl - 1)
        same_hierarchy(od, dv)
        zo, zd = apply_once(od, b), apply_once(dv, b)
        assert np.linalg.norm(zo) > 0 and np.array_equal(bits(zd), bits(zo))
    finally:
        dv.close()
        od.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------
def five_point_x_periodic(dims):
    nx, ny = dims
    Tx = sp.diags([-np.ones(nx - 1), np.zeros(nx), -np.ones(nx - 1)], [-1, 0, 1]).tolil()
    Tx[0, nx - 1] = Tx[nx - 1, 0] = -1.0
    Ty = sp.diags([-np.ones(ny - 1), np.zeros(ny), -np.ones(ny - 1)], [-1, 0, 1])
    return (sp.kron(sp.identity(ny), Tx) + sp.kron(Ty, sp.identity(nx)) + 4.0 * sp.identity(nx * ny)).tolil()


def refusal(make, amg, A, b, dims, per, masks):
    with pytest.raises(ValueError) as e:
        make(amg, sp.csr_matrix(A), b, dims, per, masks).close()
    return str(e.value)


def test_refusals_are_worded_by_the_host_constructor(on):
    dims, per = (8, 6), 1
    b = np.ones(48)
    row = lambda x, y: y * dims[0] + x  # noqa: E731
    # s_0 of an even-x row, collapsed onto x: the diagonal and the two y-neighbours, 2 - 1 - 1 = 0 exactly
    A = five_point_x_periodic(dims)  # the seam row: fine coordinate 0
    A[row(0, 2), row(0, 2)] = 2.0
    mh, md = refusal(host, on, A, b, dims, per, [1]), refusal(dev, on, A, b, dims, per, [1])
    print("\n" + md)
    assert md == mh.replace(HOST, DEV) and md.startswith(DEV + "level 0: row 16: the diagonal sum s_0 is 0")
    A = five_point_x_periodic(dims)  # an interior even row
    A[row(4, 2), row(4, 2)] = 2.0
    mh, md = refusal(host, on, A, b, dims, per, [1]), refusal(dev, on, A, b, dims, per, [1])
    print(md)
    assert md == mh.replace(HOST, DEV) and md.startswith(DEV + "level 0: row 20: the diagonal sum s_0 is 0")
    A[row(0, 2), row(0, 2)] = 2.0  # both: the smaller row is the one named
    mh, md = refusal(host, on, A, b, dims, per, [1]), refusal(dev, on, A, b, dims, per, [1])
    print(md)
    assert md == mh.replace(HOST, DEV) and "level 0: row 16: " in md
    # a masked periodic axis of odd length: refused before the device is touched, in the host constructor's words
    A = five_point_x_periodic((7, 6))
    mh, md = refusal(host, on, A, np.ones(42), (7, 6), 1, [1]), refusal(dev, on, A, np.ones(42), (7, 6), 1, [1])
    print(md)
    assert md == mh.replace(HOST, DEV) and md.startswith(DEV) and "even length of at least 4" in md
