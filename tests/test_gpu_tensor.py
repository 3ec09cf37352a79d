"""Full-coarsening tensor-product hierarchies (amg_hip_create_tensor) on the device: the matrix-free
transfer kernels against the CSR SpMV with R / P (bitwise), whole V-cycles across transfer paths, cycle
paths, fusion switches, layouts and smoothers (bitwise), the cycle against the scipy twin
(tests/tensor_twin.py), convergence counts against the twin's, the C++ drop-in, PCG, the block entry
points and the byte accounting.

The bound of every comparison with the twin comes from the reference side: with e64 the 2-norm
distance of the twin's float64 cycle from its longdouble cycle on the same inputs, the device must lie
within max(8 e64, 1e-14 ||u||) of the longdouble cycle.  Every test prints the ratio it found."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "algebraic-multigrid_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tensor_twin as T  # noqa: E402
from test_tensor_hierarchy import build_dropin, grid_laplacian  # noqa: E402

pytestmark = pytest.mark.gpu

JAC = dict(smoother=3, smoother_iters=2, omega=0.8)
CHEB = dict(smoother=5, smoother_iters=1, cheb_degree=2)
MCGS = dict(smoother=4, smoother_iters=1)


def tensor_mg(amg, dims, levels, seed=5, **kw):
    A = grid_laplacian(dims)
    b = np.random.default_rng(seed).standard_normal(A.shape[0])
    return A, b, amg.Multigrid.tensor(A.indptr, A.indices, A.data, b, dims, levels, **kw)


@pytest.mark.parametrize("dims", [(7, 5), (64, 64), (255, 256), (256, 255), (2, 2), (9, 8, 7), (33, 33, 33),
                                  (16, 2, 5)])
def test_transfer_kernels_equal_spmv_bitwise(amg, dims):
    dim = len(dims)
    P = T.tensor_P(dims, dim)
    R = P.T.tocsc()
    R.sort_indices()
    n_h, n_H = P.shape
    rng = np.random.default_rng(n_h)
    r, uH, uh = rng.standard_normal(n_h), rng.standard_normal(n_H), rng.standard_normal(n_h)
    got = amg.tensor_restrict(dims, r)
    want = amg.spmv(n_H, n_h, R.indptr, R.indices, R.data, r)
    assert np.array_equal(got, want), dims
    got = amg.tensor_prolong_add(dims, uH, uh)
    want = uh + amg.spmv(n_h, n_H, P.indptr, P.indices, P.data, uH)
    assert np.array_equal(got, want), dims
    assert np.array_equal(amg.tensor_prolong_add(dims, np.zeros(n_H), uh), uh)


def test_transfer_refusals(amg):
    with pytest.raises(ValueError):
        amg.tensor_restrict((7, 1), np.zeros(7))
    with pytest.raises(ValueError):
        amg.tensor_restrict((4, 4, 1), np.zeros(16))


def _state(mg):
    return [(mg.get_soln(l), mg.get_rhs(l)) for l in range(mg.n_levels)]


def _cycles(mg, k=3):
    mg.vcycle(k)
    mg.sync()
    st = _state(mg)
    mg.close()
    return st


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
                                    for x, y in zip(a, b))


@pytest.mark.parametrize("sm", [JAC, CHEB, MCGS], ids=["jacobi", "chebyshev", "multicolor"])
@pytest.mark.parametrize("dims,levels", [((255, 255), 6), ((256, 256), 6), ((33, 33, 33), 4)])
def test_vcycles_bit_identical_across_paths(amg, dims, levels, sm):
    ref_mg = tensor_mg(amg, dims, levels, **sm)[2]
    assert [ref_mg.level_transfer_kind(l) for l in range(levels - 1)] == [2] * (levels - 1)
    ref = _cycles(ref_mg)
    assert all(np.all(np.isfinite(u)) for u, _ in ref) and np.linalg.norm(ref[0][0]) > 0
    variants = [dict(stencil_transfers=False), dict(use_graph=False), dict(no_fusion=True),
                dict(stencil_transfers=False, use_graph=False, no_fusion=True),
                dict(layout=amg.LAYOUT_SELL), dict(layout=amg.LAYOUT_CSR),
                dict(layout=amg.LAYOUT_CSR, stencil_transfers=False)]
    for v in variants:
        mg = tensor_mg(amg, dims, levels, **sm, **v)[2]
        if not v.get("stencil_transfers", True):
            assert [mg.level_transfer_kind(l) for l in range(levels - 1)] == [0] * (levels - 1)
        assert _same(_cycles(mg), ref), (dims, sm, v)


def test_level_ops_match_the_cycle_paths(amg):
    """amg_hip_level_op ops 2 and 3 dispatch on the transfer kind: same bits as the CSR path."""
    out = []
    for st in (True, False):
        mg = tensor_mg(amg, (100, 100), 4, stencil_transfers=st, **JAC)[2]
        rng = np.random.default_rng(2)
        mg.set_vec(0, "u", rng.standard_normal(10000))
        mg.level_op(0, 1)
        mg.level_op(0, 2)
        mg.set_vec(1, "u", rng.standard_normal(2500))
        mg.level_op(0, 3)
        mg.sync()
        out.append((mg.get_rhs(1), mg.get_soln(0)))
        mg.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def check(got, ref, e64, scale, what):
    ok, dist, bound, ratio = T.within(got, ref, e64, scale)
    print(f"  {what}: distance {dist:.3e}, e64 {e64:.3e}, ratio {ratio:.2f}, bound {bound:.3e}")
    assert ok, (what, dist, bound, ratio)
    return ratio


@pytest.mark.parametrize("dims,levels", [((255, 255), 6), ((256, 256), 6), ((100, 100), 5), ((33, 33, 33), 4),
                                         ((48, 20), 4)])
def test_vcycles_equal_twin(amg, dims, levels):
    A, b, mg = tensor_mg(amg, dims, levels, **JAC)
    tw = T.Twin(A, dims, levels, 0.8, 2)
    assert tw.n[-1] <= 256      # the twin's longdouble cycle solves the coarsest level in longdouble
    u64, uld = np.zeros(b.size), np.zeros(b.size, np.longdouble)
    print()
    done = 0
    for k in (1, 3):
        while done < k:
            u64 = tw.vcycle(u64, b)[0][0]
            uld = tw.vcycle(uld, b, np.longdouble)[0][0]
            mg.vcycle(1)
            done += 1
        mg.sync()
        got = mg.get_soln(0)
        e64 = float(np.linalg.norm(u64.astype(np.longdouble) - uld))
        check(got, uld, e64, np.linalg.norm(got), f"{dims}/{levels}: level-0 u after {k} V-cycle(s)")
    mg.close()


def _device_cycles_to(mg, f, tol=1e-8, max_cycles=40):
    mg.set_vec(0, "f", f)
    mg.set_vec(0, "u", np.zeros(f.size))
    mg.sync()
    r0 = mg.rss()
    hist = [1.0]
    for k in range(1, max_cycles + 1):
        mg.vcycle(1)
        hist.append((mg.rss() / r0) ** 0.5)
        if hist[-1] <= tol:
            return k, hist
    return None, hist


@pytest.mark.parametrize("N,levels", [(255, 7), (256, 7), (1023, 9)])
def test_cycles_to_1e8_equal_twin_count(amg, N, levels):
    A, _, mg = tensor_mg(amg, (N, N), levels, **JAC)
    tw = T.Twin(A, (N, N), levels, 0.8, 2)
    f = np.random.default_rng(0).standard_normal(N * N)
    kt, ht = tw.cycles_to(f, 1e-8, 30)
    k, hist = _device_cycles_to(mg, f)
    print(f"\n{N}^2/{levels} true Jacobi omega 0.8 2+2 to ||r||/||r0|| <= 1e-8: device {k} cycles, twin {kt}; "
          f"late factor {hist[-1] / hist[-2]:.3f} (twin {ht[-1] / ht[-2]:.3f})")
    assert k is not None and kt is not None and abs(k - kt) <= 1
    mg.close()


def test_dropin_runs_on_the_matrix_free_path(amg, tmp_path):
    """AMG::Multigrid with AMG::TensorInterpolator: transfer kind 2 on every level (checked inside),
    cycles to 1e-8 within one of the twin's, rss down by more than 1e-4 over six cycles."""
    exe = build_dropin(amg, tmp_path)
    N, levels = 255, 7
    f = np.random.default_rng(0).standard_normal(N * N)
    path = tmp_path / "rhs.bin"
    f.tofile(path)
    p = subprocess.run([exe, str(N), str(levels), str(path)], capture_output=True, text=True, timeout=300)
    print("\n" + p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    cp, ri, v = amg.laplacian(N)
    import scipy.sparse as sp
    A = sp.csc_matrix((v, ri, cp), shape=(N * N, N * N))
    kt, _ = T.Twin(A, (N, N), levels, 0.8, 2).cycles_to(f, 1e-8, 30)
    words = p.stdout.split()
    k, drop6 = int(words[words.index("cycles") + 1]), float(words[words.index("drop6") + 1])
    print(f"drop-in: {k} cycles, twin {kt}; rss ratio after six cycles {drop6:.3e}")
    assert abs(k - kt) <= 1 and drop6 < 1e-4


def test_pcg_on_the_tensor_hierarchy(amg):
    N, levels = 1024, 9
    mg = amg.Multigrid.poisson_tensor(N, levels, **JAC)
    b = mg.get_rhs(0)
    kc, _ = _device_cycles_to(mg, b)
    mg.set_vec(0, "u", np.zeros(b.size))
    _, it, rel = mg.pcg(1e-8, 100)
    cp, ri, v = amg.laplacian(N)
    import scipy.sparse as sp
    A = sp.csc_matrix((v, ri, cp), shape=(N * N, N * N))
    tw = T.Twin(A, (N, N), levels, 0.8, 2)
    _, itt, relt = tw.pcg(b, 1e-8, 100)
    print(f"\npoisson_tensor({N}, {levels}) to 1e-8: {kc} V-cycles, PCG {it} iterations (relres {rel:.2e}); "
          f"numpy PCG on the twin cycle {itt} ({relt:.2e})")
    assert rel <= 1e-8 and kc is not None and it <= kc
    assert abs(it - itt) <= 1
    mg.close()


@pytest.mark.parametrize("sm", [JAC, CHEB], ids=["jacobi", "chebyshev"])
@pytest.mark.parametrize("dims,levels", [((255, 256), 6), ((33, 33, 33), 4)])
def test_block_entry_points_equal_single_vector_path(amg, dims, levels, sm):
    torch = pytest.importorskip("torch")

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()

    for use_graph in (True, False):
        mg = tensor_mg(amg, dims, levels, use_graph=use_graph, **sm)[2]
        n0 = mg.get_n_dofs(0)
        rng = np.random.default_rng(11)
        U0, F0 = rng.standard_normal((n0, 8)), rng.standard_normal((n0, 8))
        want = np.empty_like(U0)
        rss = []
        for j in range(8):
            mg.set_vec(0, "u", U0[:, j])
            mg.set_vec(0, "f", F0[:, j])
            rss.append(mg.rss())
            mg.vcycle(2)
            want[:, j] = mg.get_soln(0)
        for k in (3, 8):
            U = dev(U0[:, :k])
            got_rss = mg.block_rss(U, dev(F0[:, :k]))
            assert [got_rss[j] for j in range(k)] == rss[:k]
            mg.block_vcycles(U, dev(F0[:, :k]), n=2)
            torch.cuda.synchronize()
            got = U.cpu().numpy()
            for j in range(k):
                assert np.array_equal(got[:, j], want[:, j]), (dims, sm, k, j)
        # PCG per column against amg_hip_pcg
        xs, its, rels = [], [], []
        for j in range(3):
            mg.set_vec(0, "f", F0[:, j])
            mg.set_vec(0, "u", np.zeros(n0))
            x, it, rel = mg.pcg(1e-8, 50)
            xs.append(x), its.append(it), rels.append(rel)
        for k in (3, 8):
            X, it, rel = mg.block_pcg(dev(F0[:, :k]), rtol=1e-8, max_iters=50)
            torch.cuda.synchronize()
            got = X.cpu().numpy()
            for j in range(3):
                assert np.array_equal(got[:, j], xs[j]) and it[j] == its[j] and rel[j] == rels[j], (k, j)
        mg.close()


def test_cycle_must_move_by_hand(amg):
    """64^2, 4 levels (64^2, 32^2, 16^2, 8^2; the 8 x 8 level is solved).  Without smoothing sweeps a
    cycle is, per level l < 3: the residual (matrix + f, u, r = 24 n), K-TensorRestrict (8 n_h + 8 n_H,
    and 8 n_H more for the zero-filled u_H) and K-TensorProlong (16 n_h + 8 n_H); then the banded solve
    of the 64 rows (half-bandwidth 9: 16 n w + 24 n).  With the CSR transfers instead: R and P of
    nnz = (3 m / 2 - 1)^2 entries at 12 B, 4 B per row, and the same vectors."""
    bare = tensor_mg(amg, (64, 64), 4, smoother=3, smoother_iters=0, omega=0.8)[2]
    n = [4096, 1024, 256, 64]
    assert [bare.get_n_dofs(l) for l in range(4)] == n and bare.coarse_halfbw() == 9
    hand = 0.0
    for l in range(3):
        hand += bare.level_layout(l)[1] + 24 * n[l]
        hand += 8 * n[l] + 16 * n[l + 1]
        hand += 16 * n[l] + 8 * n[l + 1]
    hand += 16 * 64 * 9 + 24 * 64
    assert bare.cycle_must_move() == pytest.approx(hand, rel=1e-12)
    csr = tensor_mg(amg, (64, 64), 4, smoother=3, smoother_iters=0, omega=0.8, stencil_transfers=False)[2]
    extra = 0.0
    for l, m in enumerate((64, 32, 16)):
        nnz = (3 * m // 2 - 1) ** 2
        assert nnz == bare.get_transfer(l, "P")[2].size
        extra += 2 * 12 * nnz + 4 * n[l + 1] + 4 * n[l]
    assert csr.cycle_must_move() - bare.cycle_must_move() == pytest.approx(extra, rel=1e-12)
    # the 2 + 2 cycle: zero-fill is dead (the first coarse sweep starts from f), 8 n_H less per level
    full = tensor_mg(amg, (64, 64), 4, **JAC)[2]
    full_csr = tensor_mg(amg, (64, 64), 4, stencil_transfers=False, **JAC)[2]
    assert full_csr.cycle_must_move() - full.cycle_must_move() == pytest.approx(extra, rel=1e-12)
    for mg in (bare, csr, full, full_csr):
        mg.close()
