"""Semi-coarsening tensor hierarchies (amg_hip_create_tensor_semi / _semi_dev) on the device.

Shapes: the smallest at which the index arithmetic of the masked kernels can go wrong -- odd and even
lengths, axes of 2 and 3 points (one coarse point), odd nx without x-coarsening (fine lines start at
odd offsets: the unaligned branches of K-TensorRestrict / K-TensorProlong), every mask 1..3 in 2-D and
1..7 in 3-D.  Checked: the stand-alone transfers against amg_hip_spmv on the getter's R / P (bitwise);
one V-cycle across transfer kinds 2 and 0 and against amg_hip_create_custom on the same operators
(bitwise) and against the longdouble twin (tests/semi_twin.py) within tensor_twin.within, i.e. 8 x the
float64 twin's own distance; PCG counts on the anisotropic cases; the block and the float forms; the
device set-up against the host constructor (bitwise), fallback included.

PCG to 1e-8 on the anisotropic cases, float64 twin (numpy, nothing measured on a GPU), semi / full
coarsening: 33x20 (1, 1e-3) 12 / 68; 33x20 (1e-3, 1) 12 / 50; 64x48 (1, 1e-2) 11 / 50;
17x12x9 (1, 1, 1e-3) 9 / 31; 17x12x9 (1e-3, 1, 1e-3) 11 / 38; 48x40x24 (1, 1e-2, 1) 9 / 48.  The device
must take the twin's semi count within +-1."""
import os
import subprocess
import sys

import numpy as np
import pytest

sp = pytest.importorskip("scipy.sparse")
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import semi_twin as S  # noqa: E402
import tensor_twin as T  # noqa: E402
from test_tensor_semi import build_dropin  # noqa: E402

pytestmark = pytest.mark.gpu

JAC = dict(smoother=3, smoother_iters=2, omega=0.8)
SELL = 2
SHAPES = [(7, 5), (8, 6), (2, 3), (33, 20), (7, 5, 3), (8, 6, 4), (2, 3, 2), (17, 12, 9)]
TWIN_PCG = {((33, 20), (1.0, 1e-3)): 12, ((33, 20), (1e-3, 1.0)): 12, ((64, 48), (1.0, 1e-2)): 11,
            ((17, 12, 9), (1.0, 1.0, 1e-3)): 9, ((17, 12, 9), (1e-3, 1.0, 1e-3)): 11,
            ((48, 40, 24), (1.0, 1e-2, 1.0)): 9}


def masks_of(dims):
    return range(1, 4 if len(dims) == 2 else 8)


def chain(dims, m):
    """the hierarchy a mask is tried in: two levels, one full-coarsening level more on the two larger
    grids so that the twin's longdouble cycle solves its coarsest level (<= 256 rows) in longdouble"""
    return (m, S.full_mask(len(dims))) if int(np.prod(dims)) > 256 else (m,)


_OPS = {}


def op(dims):
    """(A as scipy CSR, A as sorted CSC, b): mildly anisotropic diffusion, made once per shape"""
    if dims not in _OPS:
        A = S.diffusion(dims, (1.0, 0.3, 0.05)[:len(dims)], seed=7)
        Ac = A.tocsc()
        Ac.sort_indices()
        b = S.rhs(A.shape[0], seed=8)
        for a in (A.data, Ac.data, b):
            a.setflags(write=False)
        _OPS[dims] = (A, Ac, b)
    return _OPS[dims]


def host_ctor(amg, Ac, b, dims, n_levels, masks=None, **kw):
    return amg.Multigrid.tensor_semi(Ac.indptr, Ac.indices, Ac.data, b, dims, n_levels, axis_masks=masks,
                                     theta=S.THETA, min_coarse=S.MIN_COARSE, **dict(JAC, **kw))


def dev_ctor(amg, A, b, dims, n_levels, masks=None, **kw):
    return amg.Multigrid.tensor_semi_dev(A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy(),
                                         np.array(b), dims, n_levels, axis_masks=masks, theta=S.THETA,
                                         min_coarse=S.MIN_COARSE, **dict(JAC, **kw))


def state(mg):
    mg.sync()
    return [(mg.get_soln(l), mg.get_rhs(l)) for l in range(mg.n_levels)]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
                                    for x, y in zip(a, b))


def same_triple(got, want):
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and
            np.array_equal(np.asarray(got[2]).view(np.uint64), np.asarray(want[2]).view(np.uint64)))


@pytest.mark.parametrize("dims", SHAPES)
def test_axes_transfers_equal_spmv_bitwise(amg, dims):
    dim = len(dims)
    for m in masks_of(dims):
        P = S.semi_P(dims, dim, m)
        R = P.T.tocsc()
        R.sort_indices()
        n_h, n_H = P.shape
        rng = np.random.default_rng(n_h + m)
        r, uH, uh = rng.standard_normal(n_h), rng.standard_normal(n_H), rng.standard_normal(n_h)
        got = amg.tensor_restrict(dims, r, axes=m)
        want = amg.spmv(n_H, n_h, R.indptr, R.indices, R.data, r)
        assert np.array_equal(got, want), (dims, m, "restrict")
        got = amg.tensor_prolong_add(dims, uH, uh, axes=m)
        want = uh + amg.spmv(n_h, n_H, P.indptr, P.indices, P.data, uH)
        assert np.array_equal(got, want), (dims, m, "prolong")
    # the full mask is the entry point without one
    full = S.full_mask(dim)
    r = np.random.default_rng(3).standard_normal(int(np.prod(dims)))
    assert np.array_equal(amg.tensor_restrict(dims, r, axes=full), amg.tensor_restrict(dims, r))


@pytest.mark.parametrize("dims", SHAPES)
def test_one_vcycle_across_paths_and_against_the_twin(amg, dims):
    A, Ac, b = op(dims)
    print()
    for m in masks_of(dims):
        masks = chain(dims, m)
        nl = len(masks) + 1
        mg = host_ctor(amg, Ac, b, dims, nl, masks)
        assert [mg.level_transfer_kind(l) for l in range(nl - 1)] == [2] * (nl - 1)
        assert [mg.level_axes(l) for l in range(nl - 1)] == list(masks)
        tw = S.SemiTwin(A, dims, masks=masks)
        assert [mg.level_dims(l) for l in range(nl)] == tw.dims and tw.n[-1] <= 256
        transfers = [(mg.get_transfer(l, "P"), mg.get_transfer(l, "R")) for l in range(nl - 1)]
        for l in range(nl - 1):
            assert same_triple(transfers[l][0], T.csc_triple(S.semi_P(tw.dims[l], tw.dim, masks[l])))
        mg.vcycle(1)
        ref = state(mg)
        mg.close()
        csr = host_ctor(amg, Ac, b, dims, nl, masks, stencil_transfers=False)
        assert [csr.level_transfer_kind(l) for l in range(nl - 1)] == [0] * (nl - 1)
        csr.vcycle(1)
        assert same(state(csr), ref), (dims, masks, "CSR transfers")
        csr.close()
        cu = amg.Multigrid(Ac.indptr, Ac.indices, Ac.data, b, nl, transfers=transfers, **JAC)
        cu.vcycle(1)
        assert same(state(cu), ref), (dims, masks, "amg_hip_create_custom")
        cu.close()
        zero = np.zeros(b.size)
        u64 = tw.vcycle(zero, b)[0][0]
        uld = tw.vcycle(zero.astype(np.longdouble), b, np.longdouble)[0][0]
        e64 = float(np.linalg.norm(u64.astype(np.longdouble) - uld))
        got = ref[0][0]
        ok, dist, bound, ratio = T.within(got, uld, e64, np.linalg.norm(got))
        print(f"  {dims} masks {masks}: distance {dist:.3e}, e64 {e64:.3e}, ratio {ratio:.2f}, bound {bound:.3e}")
        assert np.all(np.isfinite(got)) and np.linalg.norm(got) > 0
        assert ok, (dims, masks, dist, bound, ratio)


@pytest.mark.parametrize("dims,eps", S.ANISO)
def test_pcg_counts_on_the_anisotropic_cases(amg, dims, eps):
    """amg_hip_pcg within +-1 of the float64 twin's count (module docstring); amg_hip_pcg_mixed takes
    amg_hip_pcg's iterations; the layout is SELL, as the float cycle requires."""
    A, b, tw = S.case(dims, eps)
    Ac = A.tocsc()
    Ac.sort_indices()
    mg = host_ctor(amg, Ac, b, dims, S.MAX_LEVELS, layout=SELL)
    assert mg.n_levels == tw.nl and [mg.level_axes(l) for l in range(tw.nl - 1)] == tw.masks
    x, it, rel = mg.pcg(1e-8, 100)
    true = float(np.linalg.norm(b - A @ x) / np.linalg.norm(b))
    mg.zero_vec(0, "u")
    x32, it32, rel32 = mg.pcg_mixed(1e-8, 100)
    true32 = float(np.linalg.norm(b - A @ x32) / np.linalg.norm(b))
    want = TWIN_PCG[(dims, eps)]
    print(f"\n{dims} eps {eps}: PCG {it} iterations (twin {want}), relres {rel:.2e}, true {true:.2e}; "
          f"mixed {it32} iterations, true {true32:.2e}")
    assert tw.pcg(b, 1e-8)[1] == want
    assert rel <= 1e-8 and true <= 2e-8
    assert abs(it - want) <= 1
    assert it32 == it and true32 <= 2e-8
    mg.close()


AUTO = [((33, 20), (1.0, 1e-3)), ((17, 12, 9), (1e-3, 1.0, 1e-3))]


@pytest.mark.parametrize("dims,eps", AUTO)
def test_block_columns_have_the_bits_of_the_single_cycle(amg, dims, eps):
    A, b, tw = S.case(dims, eps)
    Ac = A.tocsc()
    Ac.sort_indices()
    mg = host_ctor(amg, Ac, b, dims, S.MAX_LEVELS)
    n0, k = b.size, 3
    rng = np.random.default_rng(11)
    U0, F0 = rng.standard_normal((n0, k)), rng.standard_normal((n0, k))
    want = np.empty_like(U0)
    for j in range(k):
        mg.set_vec(0, "u", U0[:, j])
        mg.set_vec(0, "f", F0[:, j])
        mg.vcycle(2)
        mg.sync()
        want[:, j] = mg.get_soln(0)
    U = torch.from_numpy(np.ascontiguousarray(U0)).cuda()
    mg.block_vcycles(U, torch.from_numpy(np.ascontiguousarray(F0)).cuda(), n=2)
    torch.cuda.synchronize()
    got = U.cpu().numpy()
    for j in range(k):
        assert np.array_equal(got[:, j], want[:, j]), (dims, j)
    mg.close()


@pytest.mark.parametrize("dims,eps", AUTO)
def test_float_cycle_against_the_twin(amg, dims, eps):
    """tests/test_gpu_mixed.py's bound: within max(8 e32, 1e-6 ||z||) of the longdouble cycle, e32 = the
    float32 twin's distance; odd nx without x-coarsening on both cases' deeper levels"""
    A, b, tw = S.case(dims, eps)
    Ac = A.tocsc()
    Ac.sort_indices()
    mg = host_ctor(amg, Ac, b, dims, S.MAX_LEVELS, layout=SELL)
    dv = torch.from_numpy(np.array(b)).cuda()
    dz = torch.empty_like(dv)
    mg.apply_f32(dv.data_ptr(), dz.data_ptr())
    mg.sync()
    z = dz.cpu().numpy()
    zero = np.zeros(b.size)
    small = tw.n[-1] <= 256
    ref = tw.vcycle(zero.astype(np.longdouble), b, np.longdouble)[0][0]
    z32 = tw.vcycle(zero.astype(np.float32), b.astype(np.float32), np.float32)[0][0]
    e32 = float(np.linalg.norm(np.asarray(z32, np.longdouble) - ref))
    dist = float(np.linalg.norm(np.asarray(z, np.longdouble) - ref))
    bound = max(8.0 * e32, 1e-6 * float(np.linalg.norm(z)))
    print(f"\nfloat cycle {dims} eps {eps}: distance {dist:.3e}, e32 {e32:.3e}, ratio {dist / e32:.2f}, "
          f"bound {bound:.3e}")
    assert small and np.all(np.isfinite(z)) and np.linalg.norm(z) > 0
    assert dist <= bound
    mg.close()


def _compare_setups(amg, A, Ac, b, dims, n_levels, masks, on, **kw):
    host = host_ctor(amg, Ac, b, dims, n_levels, masks, **kw)
    dev = dev_ctor(amg, A, b, dims, n_levels, masks, **kw)
    what = (dims, masks, kw)
    assert dev.setup_on_device == on and host.setup_on_device == 0, what
    nl = host.n_levels
    assert dev.n_levels == nl, what
    assert [dev.level_dims(l) for l in range(nl)] == [host.level_dims(l) for l in range(nl)], what
    assert [dev.level_axes(l) for l in range(nl - 1)] == [host.level_axes(l) for l in range(nl - 1)], what
    assert [dev.level_transfer_kind(l) for l in range(nl - 1)] == [host.level_transfer_kind(l) for l in range(nl - 1)], what
    for l in range(nl):
        assert same_triple(dev.get_coefficient_matrix(l), host.get_coefficient_matrix(l)), (what, l)
    host.vcycle(1)
    dev.vcycle(1)
    assert same(state(dev), state(host)), what
    masks_found = [host.level_axes(l) for l in range(nl - 1)]
    host.close()
    dev.close()
    return masks_found


@pytest.mark.parametrize("dims", SHAPES)
def test_device_setup_equals_host_setup_on_every_mask(amg, dims):
    A, Ac, b = op(dims)
    for m in masks_of(dims):
        masks = chain(dims, m)
        assert _compare_setups(amg, A, Ac, b, dims, len(masks) + 1, masks, 1) == list(masks)


@pytest.mark.parametrize("dims,eps", AUTO + [((64, 48), (1.0, 1e-2))])
def test_device_setup_with_automatic_masks(amg, dims, eps):
    A, b, tw = S.case(dims, eps)
    Ac = A.tocsc()
    Ac.sort_indices()
    assert _compare_setups(amg, A, Ac, b, dims, S.MAX_LEVELS, None, 1) == tw.masks
    assert _compare_setups(amg, A, Ac, b, dims, S.MAX_LEVELS, None, 1, smoother=5, smoother_iters=1,
                           cheb_degree=2) == tw.masks


def test_device_setup_falls_back_to_the_host(amg):
    """a lexicographic smoother needs host structures: the host constructor builds, same solver"""
    dims, eps = AUTO[0]
    A, b, tw = S.case(dims, eps)
    Ac = A.tocsc()
    Ac.sort_indices()
    assert _compare_setups(amg, A, Ac, b, dims, S.MAX_LEVELS, None, 0, smoother=0, smoother_iters=1,
                           omega=1.0) == tw.masks
    assert _compare_setups(amg, A, Ac, b, dims, 3, (1, 2), 0, stencil_transfers=False) == [1, 2]
    with pytest.raises(ValueError, match="level 1"):
        dev_ctor(amg, A, b, dims, 3, (1, 4))


def test_dropin_runs_semi_coarsening(amg, tmp_path):
    """AMG::Multigrid with AMG::SemiTensorInterpolator and explicit masks x, y, xy on the 48^2 model
    problem: masks, transfer kind 2 and operator shapes are checked inside; six cycles bring rss down
    by more than 1e-4."""
    exe = build_dropin(amg, tmp_path)
    p = subprocess.run([exe, "48"], capture_output=True, text=True, timeout=120)
    print("\n" + p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
