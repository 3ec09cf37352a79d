"""Operator-dependent interpolation on periodic axes (amg_hip_create_tensor_opdep_periodic) on the device.

The PER forms of K-AxisRestrict / K-AxisProlong against amg_hip_spmv on the R / P their weights stand for,
bit for bit, on the smallest grids that can go wrong: m = 4 (both neighbours of a coarse point are the same
two points), one line, odd nx along y / z (the half pair at the line end, lines at odd offsets), more than
one block, vectors 8 bytes past a 16-byte boundary.  The weights are RANDOM in [-0.5, 1.5] with zeros and
negative zeros among them: every product rounds, so only the order of the CSR SpMV gives its bits -- and
that order changes at the seam.  Then the solver on the jump operator with wrap edges
(tests/opdep_periodic_twin.py): cycle, amg_hip_apply and PCG bit for bit across transfer kinds 3 and 0; one
V-cycle against the longdouble twin; PCG counts against the float64 twin; the _dev constructor; block,
mixed and mean-projected PCG; the C++ drop-in."""
import os
import subprocess
import sys

import numpy as np
import pytest

sp = pytest.importorskip("scipy.sparse")
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import opdep_periodic_twin as OP  # noqa: E402
import opdep_twin as O  # noqa: E402
import tensor_twin as T  # noqa: E402
from test_gpu_tensor_opdep import SMOOTHERS, JAC, SELL, _run, mixed_pcg_count, projected_pcg, same, state  # noqa: E402
from test_tensor_opdep import P_of_weights  # noqa: E402
from test_tensor_opdep_periodic import all_periodic, build_dropin, csc  # noqa: E402

pytestmark = pytest.mark.gpu

# (axis, grid): the coarsened axis is periodic
TRANSFER_GRIDS = ([(0, g) for g in ((4, 3), (6, 5), (8, 1), (130, 3))] +
                  [(1, g) for g in ((3, 4), (5, 6), (8, 4), (129, 8))] +
                  [(2, g) for g in ((3, 5, 4), (6, 4, 8), (1, 1, 4), (65, 3, 6))])
# (dims, periodic mask, levels with the masks x, y, (z,) x, ...)
CYCLE_CASES = (((32, 24), 3, 5), ((16, 16, 16), 7, 7))
# PCG to 1e-8 on the float64 twin, true Jacobi 0.8 2 + 2 (numpy, nothing measured on a GPU)
TWIN_PCG = {((64, 48), 1, 7): 10, ((64, 48), 3, 7): 10, ((32, 24), 3, 5): 8, ((24, 20, 16), 4, 7): 9,
            ((16, 16, 16), 7, 7): 9}


def ctor(amg, A, b, dims, per, masks, dev=False, **kw):
    opts = dict(JAC)
    opts.update(kw)
    opts.setdefault("singular", all_periodic(dims, per))
    if dev:
        M = sp.csr_matrix(A)
        M.sort_indices()
        return amg.Multigrid.tensor_opdep_periodic_dev(M.indptr.astype(np.int32), M.indices.astype(np.int32),
                                                       M.data, np.array(b), dims, len(masks) + 1, per,
                                                       axis_masks=masks, **opts)
    Ac = csc(A)
    return amg.Multigrid.tensor_opdep_periodic(Ac.indptr, Ac.indices, Ac.data, b, dims, len(masks) + 1, per,
                                               axis_masks=masks, **opts)


def random_weights(rng, rows):
    W = rng.uniform(-0.5, 1.5, size=(rows, 2))
    flat = W.reshape(-1)
    k = rng.permutation(flat.size)
    flat[k[:max(1, flat.size // 8)]] = 0.0
    flat[k[max(1, flat.size // 8):max(2, flat.size // 4)]] = -0.0
    return W


@pytest.mark.parametrize("axis,dims", TRANSFER_GRIDS)
def test_seam_transfers_equal_spmv_bitwise(amg, axis, dims):
    dim = len(dims)
    n_h = int(np.prod(dims))
    n_H = n_h // 2
    rng = np.random.default_rng(1000 * n_h + axis)
    W = random_weights(rng, n_h - n_H)
    if W.size >= 32:
        assert (W == 0.0).any() and (W < 0.0).any() and np.signbit(W[W == 0.0]).any()
    P = OP.P_of_weights_per(dims, dim, 1 << axis, W)
    assert P.nnz == 3 * n_H  # every column holds three rows, explicit zeros kept
    R = P.T.tocsc()
    R.sort_indices()
    assert R.nnz == P.nnz
    r, uH, uh = rng.standard_normal(n_h), rng.standard_normal(n_H), rng.standard_normal(n_h)
    want_r = amg.spmv(n_H, n_h, R.indptr, R.indices, R.data, r)
    want_p = uh + amg.spmv(n_h, n_H, P.indptr, P.indices, P.data, uH)
    for shift in (0, 1):
        got = amg.axis_restrict(dims, axis, W, r, periodic=True, vec_shift=shift)
        assert np.array_equal(got, want_r), (dims, axis, shift, "restrict")
        got = amg.axis_prolong_add(dims, axis, W, uH, uh, periodic=True, vec_shift=shift)
        assert np.array_equal(got, want_p), (dims, axis, shift, "prolong")


@pytest.mark.parametrize("dims", ((7, 5), (8, 3), (5, 4, 3)))
def test_periodic_0_is_the_open_pair(amg, dims):
    dim = len(dims)
    for axis in range(dim):
        n_h = int(np.prod(dims))
        n_H = n_h // dims[axis] * (dims[axis] // 2)
        rng = np.random.default_rng(n_h + axis)
        W = rng.uniform(-0.5, 1.5, size=(n_h - n_H, 2))
        r, uH, uh = rng.standard_normal(n_h), rng.standard_normal(n_H), rng.standard_normal(n_h)
        want_r = amg.axis_restrict(dims, axis, W, r)
        want_p = amg.axis_prolong_add(dims, axis, W, uH, uh)
        Pc = P_of_weights(dims, dim, 1 << axis, W)
        assert np.array_equal(want_p, uh + amg.spmv(n_h, n_H, Pc[0], Pc[1], Pc[2], uH))
        for shift in (0, 1):
            assert np.array_equal(amg.axis_restrict(dims, axis, W, r, periodic=False, vec_shift=shift), want_r)
            assert np.array_equal(amg.axis_prolong_add(dims, axis, W, uH, uh, periodic=False, vec_shift=shift), want_p)


@pytest.mark.parametrize("smoother", sorted(SMOOTHERS))
@pytest.mark.parametrize("dims,per,nl", CYCLE_CASES)
def test_cycle_apply_and_pcg_across_transfer_kinds(amg, dims, per, nl, smoother):
    A, b, tw = OP.case(dims, per, nl)
    kw = SMOOTHERS[smoother]
    for what in ("vcycle", "apply", "pcg"):
        mg = ctor(amg, A, b, dims, per, tw.masks, **kw)
        assert mg.n_levels == nl and mg.periodic_axes() == per
        assert [mg.level_transfer_kind(l) for l in range(nl - 1)] == [3] * (nl - 1)
        ref = _run(mg, b, what)
        mg.close()
        assert all(np.all(np.isfinite(u)) for u, _ in ref) and np.linalg.norm(ref[0][0]) > 0
        csr = ctor(amg, A, b, dims, per, tw.masks, stencil_transfers=False, **kw)
        assert [csr.level_transfer_kind(l) for l in range(nl - 1)] == [0] * (nl - 1)
        assert same(_run(csr, b, what), ref), (dims, smoother, what, "stencil_transfers = 0")
        csr.close()
        try:
            amg.set_axis_stencil(False)
            off = ctor(amg, A, b, dims, per, tw.masks, **kw)
        finally:
            amg.set_axis_stencil(True)
        assert [off.level_transfer_kind(l) for l in range(nl - 1)] == [0] * (nl - 1)
        assert same(_run(off, b, what), ref), (dims, smoother, what, "set_axis_stencil(0)")
        off.close()
    # the level operation at the seam: restrict zeroes u_H and equals the SpMV with the solver's own R
    mg = ctor(amg, A, b, dims, per, tw.masks, **kw)
    mg.set_vec(1, "u", np.full(mg.get_n_dofs(1), np.nan))
    r = np.random.default_rng(5).standard_normal(mg.get_n_dofs(0))
    mg.set_vec(0, "r", r)
    mg.level_op(0, 2)
    mg.sync()
    R = mg.get_transfer(0, "R")
    assert np.array_equal(mg.get_soln(1), np.zeros(mg.get_n_dofs(1)))
    assert np.array_equal(mg.get_rhs(1), amg.spmv(mg.get_n_dofs(1), mg.get_n_dofs(0), R[0], R[1], R[2], r))
    mg.close()


@pytest.mark.parametrize("dims,per,nl", CYCLE_CASES + (((64, 48), 1, 7),))
def test_one_vcycle_against_the_twin(amg, dims, per, nl):
    """The measure of test_gpu_tensor_opdep.py::test_one_vcycle_against_the_twin: the distance to the
    longdouble twin within tensor_twin.within of the float64 twin's own distance."""
    A, b, tw = OP.case(dims, per, nl)
    mg = ctor(amg, A, b, dims, per, tw.masks)
    assert tw.n[-1] <= 256
    mg.vcycle(1)
    got = state(mg)[0][0]
    mg.close()
    zero = np.zeros(b.size)
    u64 = tw.vcycle(zero, b)[0][0]
    uld = tw.vcycle(zero.astype(np.longdouble), b, np.longdouble)[0][0]
    e64 = float(np.linalg.norm(u64.astype(np.longdouble) - uld))
    ok, dist, bound, ratio = T.within(got, uld, e64, np.linalg.norm(got))
    print(f"\n{dims} per {per}: distance {dist:.3e}, e64 {e64:.3e}, ratio {ratio:.2f}, bound {bound:.3e}")
    assert np.all(np.isfinite(got)) and np.linalg.norm(got) > 0
    assert ok, (dims, dist, bound, ratio)


@pytest.mark.parametrize("dims,per,nl", sorted(TWIN_PCG))
def test_pcg_counts_are_the_twins(amg, dims, per, nl):
    """amg_hip_pcg takes the float64 twin's count, through the host and the _dev constructor (which builds
    on the host, always: setup_on_device = 0)."""
    A, b, tw = OP.case(dims, per, nl)
    want = tw.pcg(b, 1e-8)[1]
    for dev in (False, True):
        mg = ctor(amg, A, b, dims, per, tw.masks, dev=dev)
        assert mg.n_levels == nl and mg.setup_on_device == 0 and mg.periodic_axes() == per
        assert [mg.level_transfer_kind(l) for l in range(nl - 1)] == [3] * (nl - 1)
        x, it, rel = mg.pcg(1e-8, 200)
        true = float(np.linalg.norm(b - A @ x) / np.linalg.norm(b))
        if dev:
            assert np.array_equal(x, x_host) and it == it_host
        x_host, it_host = x, it
        mg.close()
        print(f"\n{dims} per {per}{' (_dev)' if dev else ''}: PCG {it} iterations (twin {want}), relres {rel:.2e}, "
              f"true {true:.2e}")
        assert want == TWIN_PCG[(dims, per, nl)]
        assert rel <= 1e-8 and true <= 2e-8
        assert it == want


def test_block_pcg_columns_have_the_bits_of_the_single_path(amg):
    dims, per, nl = CYCLE_CASES[0]
    A, b, tw = OP.case(dims, per, nl)
    mg = ctor(amg, A, b, dims, per, tw.masks)
    n0, k = b.size, 3
    B0 = np.random.default_rng(11).standard_normal((n0, k))
    B0 -= B0.mean(axis=0)
    B0[:, 0] = b
    want, its = np.empty_like(B0), []
    for j in range(k):
        one = ctor(amg, A, B0[:, j], dims, per, tw.masks)
        x, it, _ = one.pcg(1e-8, 100)
        want[:, j] = x
        its.append(it)
        one.close()
    X, it, rel = mg.block_pcg(torch.from_numpy(np.ascontiguousarray(B0)).cuda(), None, 1e-8, 100)
    torch.cuda.synchronize()
    got = X.cpu().numpy()
    assert list(it) == its
    for j in range(k):
        assert np.array_equal(got[:, j], want[:, j]), j
    mg.close()


def test_mixed_pcg_takes_the_float_cycle_count(amg):
    dims, per, nl = (64, 48), 3, 7
    A, b, tw = OP.case(dims, per, nl)
    mg = ctor(amg, A, b, dims, per, tw.masks, layout=SELL)
    x32, it32, rel32 = mg.pcg_mixed(1e-8, 200)
    true32 = float(np.linalg.norm(b - A @ x32) / np.linalg.norm(b))
    mg.close()
    want32 = mixed_pcg_count(tw, A, b, 1e-8)
    print(f"\n{dims} per {per}: mixed PCG {it32} iterations (twin with a float32 cycle {want32}), true {true32:.2e}")
    assert abs(it32 - want32) <= 1 and true32 <= 2e-8


def test_inconsistent_rhs_with_the_mean_projection(amg):
    """b + 1e-6 is not in the range of the fully periodic operator; with amg_hip_set_mean_projection(1) the
    solve takes the count of the consistent system (the twin's, 10) and returns a zero-mean solution."""
    dims, per, nl = (64, 48), 3, 7
    A, b, tw = OP.case(dims, per, nl)
    consistent = tw.pcg(b, 1e-8)[1]
    want = projected_pcg(tw, A, b + 1e-6, 1e-8)[1]
    mg = ctor(amg, A, b + 1e-6, dims, per, tw.masks)
    mg.set_mean_projection(1)
    x, it, rel = mg.pcg(1e-8, 200)
    true = float(np.linalg.norm(b - A @ x) / np.linalg.norm(b))
    mg.close()
    print(f"\n{dims} per {per}, b + 1e-6: PCG {it} iterations (consistent {consistent}, projected twin {want}), "
          f"relres {rel:.2e}, true {true:.2e}")
    assert consistent == TWIN_PCG[(dims, per, nl)] and want == consistent
    assert it == consistent and rel <= 1e-8 and true <= 2e-8
    assert abs(float(x.mean())) <= 1e-12 * float(np.abs(x).max())


def test_dropin_runs_with_periodic_axes(amg, tmp_path):
    """AMG::Multigrid with AMG::OpdepTensorInterpolator(..., periodic_axes = 3) on the shifted 48^2 torus:
    the mask, transfer kind 3 and the seam column are checked inside; six cycles bring rss down by more
    than 1e-4."""
    exe = build_dropin(amg, tmp_path)
    p = subprocess.run([exe, "48"], capture_output=True, text=True, timeout=120)
    print("\n" + p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
