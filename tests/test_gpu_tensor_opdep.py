"""Operator-dependent interpolation on tensor hierarchies (amg_hip_create_tensor_opdep) on the device.

Shapes of the stand-alone transfers: odd and even axis lengths, axes of 2 and 3 points (one coarse
point), odd nx (fine lines start at odd offsets: the unaligned branches of K-AxisRestrict /
K-AxisProlong), more than one block (64 x 48), every axis.  The weights there are RANDOM in [-0.5, 1.5]:
every product rounds, so only the order of operations of the CSR SpMV gives its bits.  Checked on the
jump operator (tests/opdep_twin.py): one V-cycle, amg_hip_apply and three PCG iterations bit for bit
across transfer kind 3, kind 0 (stencil_transfers = 0) and amg_hip_set_axis_stencil(0); the cycle against
the longdouble twin within tensor_twin.within; a poisoned coarse u; PCG counts against the float64
twin within +-1, as tests/test_gpu_tensor_semi.py compares its counts; the float and block forms; a
singular system with the mean projection; the bytes the transfers must move.

PCG to 1e-8, float64 twin (numpy, nothing measured on a GPU), true Jacobi 0.8 2 + 2: jump((64, 48), 4) 10;
jump((128, 128), 4) 15 (full coarsening 59); jump((24, 20, 16), 4) 9; the singular jump((64, 48), 4,
natural) with the projection 12."""
import os
import subprocess
import sys

import numpy as np
import pytest

sp = pytest.importorskip("scipy.sparse")
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import opdep_twin as O  # noqa: E402
import semi_twin as S  # noqa: E402
import tensor_twin as T  # noqa: E402
from test_tensor_opdep import P_of_weights, build_dropin  # noqa: E402

pytestmark = pytest.mark.gpu

JAC = dict(smoother=3, smoother_iters=2, omega=0.8)
SMOOTHERS = {"jacobi": JAC, "chebyshev": dict(smoother=5, smoother_iters=1, cheb_degree=2),
             "line_alt": dict(smoother=7, smoother_iters=1, omega=0.8)}
SELL = 2
TRANSFER_GRIDS = [(7, 5), (8, 3), (2, 9), (3, 2), (64, 48), (5, 4, 3), (17, 12, 9)]
CYCLE_GRIDS = [(33, 20), (17, 12, 9)]
TWIN_PCG = {(64, 48): 10, (128, 128): 15, (24, 20, 16): 9}


def ctor(amg, A, b, dims, n_levels=O.MAX_LEVELS, masks=None, **kw):
    Ac = A.tocsc()
    Ac.sort_indices()
    opts = dict(JAC)
    opts.update(kw)
    return amg.Multigrid.tensor_opdep(Ac.indptr, Ac.indices, Ac.data, b, dims, n_levels, axis_masks=masks,
                                      min_coarse=O.MIN_COARSE, **opts)


def state(mg):
    mg.sync()
    return [(mg.get_soln(l), mg.get_rhs(l)) for l in range(mg.n_levels)]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
                                    for x, y in zip(a, b))


@pytest.mark.parametrize("dims", TRANSFER_GRIDS)
def test_axis_transfers_equal_spmv_bitwise(amg, dims):
    dim = len(dims)
    for axis in range(dim):
        n_h = int(np.prod(dims))
        n_H = n_h // dims[axis] * (dims[axis] // 2)
        rng = np.random.default_rng(n_h + axis)
        W = rng.uniform(-0.5, 1.5, size=(n_h - n_H, 2))
        Pc = P_of_weights(dims, dim, 1 << axis, W)
        P = sp.csc_matrix((Pc[2], Pc[1], Pc[0]), shape=(n_h, n_H))
        R = P.T.tocsc()
        R.sort_indices()
        assert P.nnz == Pc[2].size and R.nnz == P.nnz
        r, uH, uh = rng.standard_normal(n_h), rng.standard_normal(n_H), rng.standard_normal(n_h)
        got = amg.axis_restrict(dims, axis, W, r)
        want = amg.spmv(n_H, n_h, R.indptr, R.indices, R.data, r)
        assert np.array_equal(got, want), (dims, axis, "restrict")
        got = amg.axis_prolong_add(dims, axis, W, uH, uh)
        want = uh + amg.spmv(n_h, n_H, P.indptr, P.indices, P.data, uH)
        assert np.array_equal(got, want), (dims, axis, "prolong")


def _run(mg, b, what):
    """the states after one V-cycle / the result of amg_hip_apply / of three PCG iterations"""
    if what == "vcycle":
        mg.vcycle(1)
        return state(mg)
    if what == "apply":
        dv = torch.from_numpy(np.array(b)).cuda()
        dz = torch.empty_like(dv)
        mg.apply_dev(dv.data_ptr(), dz.data_ptr())
        mg.sync()
        return [(dz.cpu().numpy(), np.array(b))]
    x, it, rel = mg.pcg(1e-30, 3)
    assert it == 3
    return [(x, np.array([rel]))]


@pytest.mark.parametrize("smoother", sorted(SMOOTHERS))
@pytest.mark.parametrize("dims", CYCLE_GRIDS)
def test_cycle_apply_and_pcg_across_transfer_kinds(amg, dims, smoother):
    A, b, tw = O.case(dims)
    kw = SMOOTHERS[smoother]
    for what in ("vcycle", "apply", "pcg"):
        mg = ctor(amg, A, b, dims, **kw)
        nl = mg.n_levels
        assert nl == tw.nl and [mg.level_axes(l) for l in range(nl - 1)] == tw.masks
        assert [mg.level_transfer_kind(l) for l in range(nl - 1)] == [3] * (nl - 1)
        ref = _run(mg, b, what)
        mg.close()
        assert all(np.all(np.isfinite(u)) for u, _ in ref) and np.linalg.norm(ref[0][0]) > 0
        csr = ctor(amg, A, b, dims, stencil_transfers=False, **kw)
        assert [csr.level_transfer_kind(l) for l in range(nl - 1)] == [0] * (nl - 1)
        assert same(_run(csr, b, what), ref), (dims, smoother, what, "stencil_transfers = 0")
        csr.close()
        try:
            amg.set_axis_stencil(False)
            off = ctor(amg, A, b, dims, **kw)
        finally:
            amg.set_axis_stencil(True)
        assert [off.level_transfer_kind(l) for l in range(nl - 1)] == [0] * (nl - 1)
        assert same(_run(off, b, what), ref), (dims, smoother, what, "set_axis_stencil(0)")
        off.close()
    # the cycle zeroes u_H where it relies on it: a poisoned coarse u changes nothing
    mg = ctor(amg, A, b, dims, **kw)
    mg.vcycle(1)
    ref = state(mg)
    mg.close()
    mg = ctor(amg, A, b, dims, **kw)
    for l in range(1, mg.n_levels):
        mg.set_vec(l, "u", np.full(mg.get_n_dofs(l), np.nan))
    mg.vcycle(1)
    assert same(state(mg), ref), (dims, smoother, "poisoned coarse u")
    # the level operations: restrict zeroes u_H, prolong adds
    mg.set_vec(1, "u", np.full(mg.get_n_dofs(1), np.nan))
    r = np.random.default_rng(5).standard_normal(mg.get_n_dofs(0))
    mg.set_vec(0, "r", r)
    mg.level_op(0, 2)
    mg.sync()
    R = mg.get_transfer(0, "R")
    assert np.array_equal(mg.get_soln(1), np.zeros(mg.get_n_dofs(1)))
    assert np.array_equal(mg.get_rhs(1), amg.spmv(mg.get_n_dofs(1), mg.get_n_dofs(0), R[0], R[1], R[2], r))
    mg.close()


@pytest.mark.parametrize("dims", CYCLE_GRIDS)
def test_one_vcycle_against_the_twin(amg, dims):
    A, b, tw = O.case(dims)
    mg = ctor(amg, A, b, dims)
    assert tw.n[-1] <= 256
    mg.vcycle(1)
    got = state(mg)[0][0]
    mg.close()
    zero = np.zeros(b.size)
    u64 = tw.vcycle(zero, b)[0][0]
    uld = tw.vcycle(zero.astype(np.longdouble), b, np.longdouble)[0][0]
    e64 = float(np.linalg.norm(u64.astype(np.longdouble) - uld))
    ok, dist, bound, ratio = T.within(got, uld, e64, np.linalg.norm(got))
    print(f"\n{dims}: distance {dist:.3e}, e64 {e64:.3e}, ratio {ratio:.2f}, bound {bound:.3e}")
    assert np.all(np.isfinite(got)) and np.linalg.norm(got) > 0
    assert ok, (dims, dist, bound, ratio)


def mixed_pcg_count(tw, A, b, rtol, max_iters=200):
    """tensor_twin.Twin.pcg with the V-cycle in float32 and everything else in float64 (amg_hip_pcg_mixed)."""
    x = np.zeros(b.size)
    r = b.copy()
    bnorm = np.linalg.norm(b)

    def apply(r):
        return tw.vcycle(np.zeros(r.size, np.float32), r.astype(np.float32), np.float32)[0][0].astype(np.float64)
    z = apply(r)
    p, rz, it = z.copy(), r @ z, 0
    while it < max_iters:
        q = A @ p
        a = rz / (p @ q)
        x, r, it = x + a * p, r - a * q, it + 1
        if not np.linalg.norm(r) / bnorm > rtol:
            break
        z = apply(r)
        rzn = r @ z
        p, rz = z + (rzn / rz) * p, rzn
    return it


@pytest.mark.parametrize("dims", sorted(TWIN_PCG))
def test_pcg_counts_on_the_jump_operator(amg, dims):
    """amg_hip_pcg within +-1 of the float64 twin's count (module docstring); amg_hip_pcg_mixed within
    +-1 of the twin's count with a float32 cycle (SELL, as the float cycle requires); on 128^2 at most
    half the count of Multigrid.tensor (full coarsening) on the same matrix."""
    A, b, tw = O.case(dims)
    mg = ctor(amg, A, b, dims, layout=SELL)
    assert mg.n_levels == tw.nl and [mg.level_axes(l) for l in range(tw.nl - 1)] == tw.masks
    x, it, rel = mg.pcg(1e-8, 200)
    true = float(np.linalg.norm(b - A @ x) / np.linalg.norm(b))
    mg.zero_vec(0, "u")
    x32, it32, rel32 = mg.pcg_mixed(1e-8, 200)
    true32 = float(np.linalg.norm(b - A @ x32) / np.linalg.norm(b))
    mg.close()
    want = TWIN_PCG[dims]
    print(f"\n{dims}: PCG {it} iterations (twin {want}), relres {rel:.2e}, true {true:.2e}; "
          f"mixed {it32} iterations, true {true32:.2e}")
    assert tw.pcg(b, 1e-8)[1] == want
    assert rel <= 1e-8 and true <= 2e-8
    assert abs(it - want) <= 1
    want32 = mixed_pcg_count(tw, A, b, 1e-8)
    print(f"twin with a float32 cycle: {want32}")
    assert abs(it32 - want32) <= 1 and true32 <= 2e-8
    if dims == (128, 128):
        Ac = A.tocsc()
        Ac.sort_indices()
        nl = S.full_twin(A, dims).nl
        full = amg.Multigrid.tensor(Ac.indptr, Ac.indices, Ac.data, b, dims, nl, **JAC)
        itf = full.pcg(1e-8, 400)[1]
        full.close()
        print(f"full coarsening: {itf} iterations")
        assert 2 * it <= itf, (it, itf)


@pytest.mark.parametrize("dims", CYCLE_GRIDS)
def test_block_pcg_columns_have_the_bits_of_the_single_path(amg, dims):
    A, b, tw = O.case(dims)
    mg = ctor(amg, A, b, dims)
    n0, k = b.size, 3
    B0 = np.random.default_rng(11).standard_normal((n0, k))
    B0[:, 0] = b
    want, its = np.empty_like(B0), []
    for j in range(k):
        one = ctor(amg, A, B0[:, j], dims)
        x, it, _ = one.pcg(1e-8, 100)
        want[:, j] = x
        its.append(it)
        one.close()
    X, it, rel = mg.block_pcg(torch.from_numpy(np.ascontiguousarray(B0)).cuda(), None, 1e-8, 100)
    torch.cuda.synchronize()
    got = X.cpu().numpy()
    assert [mg.level_transfer_kind(l) for l in range(mg.n_levels - 1)] == [3] * (mg.n_levels - 1)
    assert list(it) == its
    for j in range(k):
        assert np.array_equal(got[:, j], want[:, j]), (dims, j)
    # the double cycle still runs its own kernels after the block copies were made
    mg.vcycle(1)
    ref = ctor(amg, A, b, dims)
    ref.vcycle(1)
    assert same(state(mg), state(ref))
    ref.close()
    mg.close()


def projected_pcg(tw, A, b, rtol, max_iters=200):
    """tensor_twin.Twin.pcg with b, every preconditioned residual and the result projected onto the
    complement of the constants (amg_hip_set_mean_projection)."""
    def proj(v):
        return v - v.mean()
    b = proj(b)
    x = np.zeros(b.size)
    r = b.copy()
    bnorm = np.linalg.norm(b)
    z = proj(tw.vcycle(np.zeros_like(r), r)[0][0])
    p, rz, it = z.copy(), r @ z, 0
    while it < max_iters:
        q = A @ p
        a = rz / (p @ q)
        x, r, it = x + a * p, r - a * q, it + 1
        if not np.linalg.norm(r) / bnorm > rtol:
            break
        z = proj(tw.vcycle(np.zeros_like(r), r)[0][0])
        rzn = r @ z
        p, rz = z + (rzn / rz) * p, rzn
    return proj(x), it


def test_singular_system_with_the_mean_projection(amg):
    dims = (64, 48)
    A = O.jump(dims, contrast=4, natural=True, shift=0.0)
    b = S.rhs(A.shape[0])
    tw = O.OpdepTwin(A, dims, pin=True)
    want = projected_pcg(tw, A, b, 1e-8)[1]
    mg = ctor(amg, A, b, dims, natural_sides=15, singular=True)
    assert mg.n_levels == tw.nl and mg.natural_sides() == 15
    mg.set_mean_projection(1)
    x, it, rel = mg.pcg(1e-8, 200)
    bp = b - b.mean()
    true = float(np.linalg.norm(bp - A @ x) / np.linalg.norm(bp))
    mg.close()
    print(f"\nsingular {dims}: PCG {it} iterations (twin {want}), relres {rel:.2e}, true {true:.2e}")
    assert want == 12
    assert rel <= 1e-8 and true <= 2e-8 and abs(float(x.mean())) <= 1e-12 * float(np.abs(x).max())
    assert abs(it - want) <= 1


def test_must_move_follows_the_byte_formula(amg):
    """Restrict: 8 n_l + 16 (n_l - n_{l+1}) + 8 n_{l+1} (+ 8 n_{l+1} where u_H is zeroed); prolong:
    16 n_l + 16 (n_l - n_{l+1}) + 8 n_{l+1}.  Kind 0 moves 12 nnz + 4 rows for the CSR arrays instead of
    the weights, the vectors being the same; the test sums the difference over the levels."""
    dims = (33, 20)
    A, b, _ = O.case(dims)
    kw = SMOOTHERS["chebyshev"]
    k3 = ctor(amg, A, b, dims, **kw)
    k0 = ctor(amg, A, b, dims, stencil_transfers=False, **kw)
    n = [k3.get_n_dofs(l) for l in range(k3.n_levels)]
    diff = 0.0
    for l in range(k3.n_levels - 1):
        nnz = k3.get_transfer(l, "P")[2].size
        w = 16.0 * (n[l] - n[l + 1])
        diff += (12.0 * nnz + 4.0 * n[l + 1] - w) + (12.0 * nnz + 4.0 * n[l] - w)
    m3, m0 = k3.cycle_must_move(), k0.cycle_must_move()
    assert m0 - m3 == diff and diff > 0, (m0, m3, diff)
    # the transfers alone, kind 3 against kind 0: about 1.5 x fewer bytes
    t3 = sum(24.0 * n[l] + 32.0 * (n[l] - n[l + 1]) + 24.0 * n[l + 1] for l in range(len(n) - 1))
    assert 1.3 < (t3 + diff) / t3 < 1.8
    c3, c0 = k3.cycle_bytes()[0], k0.cycle_bytes()[0]
    assert c0 > c3
    k3.close()
    k0.close()


def test_dropin_runs_operator_dependent_interpolation(amg, tmp_path):
    """AMG::Multigrid with AMG::OpdepTensorInterpolator and explicit masks x, y, x, y on the 48^2 model
    problem: masks, transfer kind 3 and operator shapes are checked inside; six cycles bring rss down by
    more than 1e-4."""
    exe = build_dropin(amg, tmp_path)
    p = subprocess.run([exe, "48"], capture_output=True, text=True, timeout=120)
    print("\n" + p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
