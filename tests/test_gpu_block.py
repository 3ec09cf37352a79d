"""Block (multi-right-hand-side) V-cycle, rss and PCG on an MI355X: column j of every block
result must have the bits of the single-vector path on column j (include/amg_hip.h:
amg_hip_block_vcycles), on every hierarchy kind, smoother and coarse-solve kind the block cycle
supports; the solver's own vectors are left alone; the refusals leave the state as it was."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BAND, SPIKE, WIDE, CHAIN = 0, 1, 2, 3


def csc(A):
    return A.colptr, A.rowind, A.val


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def kind(amg, mg):
    return int(amg.lib().amg_hip_coarse_solve_kind(mg._h))


def nonsym_band(oracle):
    """test_vcycle_nonsymmetric_operator's convection-diffusion-like band matrix"""
    n = 5000
    cp = np.zeros(n + 1, dtype=np.int32)
    ri, va = [], []
    for j in range(n):
        for i, v in ((j - 70, -1.0), (j - 1, -1.5), (j, 5.0), (j + 1, -0.5), (j + 70, -1.0)):
            if 0 <= i < n:
                ri.append(i)
                va.append(v + (0.125 if i == j and j % 3 == 0 else 0.0))
        cp[j + 1] = len(ri)
    return oracle.CSC(n, n, cp, np.array(ri, dtype=np.int32), np.array(va)), np.sin(0.01 * np.arange(n)) + 2.0


def custom_transfers(oracle, n, L):
    """perturbed copies of the linear pair (test_custom_interpolator_galerkin_on_device_matches_host)"""
    ref = oracle.Multigrid(oracle.laplacian(n), oracle.rhs(n), L)
    rng = np.random.default_rng(8)
    tr = []
    for l in range(L - 1):
        P, R = ref.transfer(l, "P"), ref.transfer(l, "R")
        pv = P.val * (1.0 + 0.1 * rng.random(P.val.size))
        rv = R.val * (1.0 + 0.1 * rng.random(R.val.size))
        tr.append(((P.colptr, P.rowind, pv), (R.colptr, R.rowind, rv)))
    return tr


JAC22 = dict(smoother=3, smoother_iters=2, omega=0.6)
JAC11 = dict(smoother=3, smoother_iters=1, omega=0.8)


def cheb(degree, iters):
    return dict(smoother=5, cheb_degree=degree, smoother_iters=iters)


# name -> (builder(amg, oracle, use_graph, **smoother), expected coarse kind or None, smoothers)
def _hierarchies():
    def p513_8(amg, O, g, **kw):
        return amg.Multigrid.poisson(513, 8, use_graph=g, exact_coarse_solve=True, **kw)

    def p513_9(amg, O, g, **kw):
        return amg.Multigrid.poisson(513, 9, use_graph=g, **kw)

    def p33_3d(amg, O, g, **kw):
        return amg.Multigrid.poisson(33, 4, dim=3, use_graph=g, exact_coarse_solve=True, **kw)

    def p1024_6(amg, O, g, **kw):
        return amg.Multigrid.poisson(1024, 6, use_graph=g, fast_coarse_solve=True, **kw)

    def host255(amg, O, g, **kw):
        return amg.Multigrid(*csc(O.laplacian(255)), O.rhs(255), 6, use_graph=g, exact_coarse_solve=True, **kw)

    def rs96(amg, O, g, **kw):
        return amg.Multigrid.ruge_stueben(*csc(O.laplacian(96)), O.rhs(96), 25, 0.25, 50, use_graph=g,
                                          exact_coarse_solve=True, **kw)

    def custom150(amg, O, g, **kw):
        return amg.Multigrid(*csc(O.laplacian(150)), O.rhs(150), 5, transfers=custom_transfers(O, 150, 5),
                             use_graph=g, exact_coarse_solve=True, **kw)

    def nonsym(amg, O, g, **kw):
        A, b = nonsym_band(O)
        return amg.Multigrid(*csc(A), b, 4, use_graph=g, exact_coarse_solve=True, **kw)

    return {
        "poisson513x8": (p513_8, BAND, [JAC22, cheb(3, 1)]),
        "poisson513x9": (p513_9, CHAIN, [JAC22, JAC11]),
        "poisson33-3d": (p33_3d, WIDE, [JAC22, cheb(2, 1)]),
        "poisson1024x6": (p1024_6, SPIKE, [JAC22]),
        "host255x6": (host255, BAND, [JAC22, JAC11, cheb(1, 2)]),
        "rs96": (rs96, None, [JAC22, cheb(2, 2)]),
        "custom150": (custom150, None, [JAC22, cheb(3, 2)]),
        "nonsym5000": (nonsym, None, [JAC22, cheb(1, 1)]),
    }


HIER = _hierarchies()


def single_columns(mg, U0, F0, n):
    """column j = the solver's own level-0 solution after set_vec(u, U0[:, j]), set_vec(f, F0[:, j]),
    vcycle(n)"""
    out = np.empty_like(U0)
    for j in range(U0.shape[1]):
        mg.set_vec(0, "u", U0[:, j])
        mg.set_vec(0, "f", F0[:, j])
        mg.vcycle(n)
        out[:, j] = mg.get_soln(0)
    return out


@pytest.mark.parametrize("name", list(HIER))
def test_block_vcycle_equals_single_vcycle_per_column(amg, oracle, name):
    build, want_kind, smoothers = HIER[name]
    rng = np.random.default_rng(11)
    for sm in smoothers:
        ref = build(amg, oracle, True, **sm)
        if want_kind is not None:
            assert kind(amg, ref) == want_kind, (name, ref.coarse_solve_kind())
        else:
            assert kind(amg, ref) != SPIKE
        n0 = ref.get_n_dofs(0)
        U0 = rng.standard_normal((n0, 16))
        F0 = rng.standard_normal((n0, 16))
        want = single_columns(ref, U0, F0, 3)
        eager = build(amg, oracle, False, **sm)
        for mg in (ref, eager):
            for k in (1, 3, 8, 16):
                U = dev(U0[:, :k])
                mg.block_vcycles(U, dev(F0[:, :k]), n=3)
                torch.cuda.synchronize()
                got = U.cpu().numpy()
                for j in range(k):
                    assert np.array_equal(got[:, j], want[:, j]), (name, sm, k, j)
        if name == "nonsym5000" and sm is JAC22:  # and against the CPU oracle directly
            A, b = nonsym_band(oracle)
            o = oracle.Multigrid(A, b, 4, smoother=oracle.SM_TRUE_JACOBI, smoother_iters=2, omega=0.6)
            for j in range(3):
                o.set_vec(0, "u", U0[:, j])
                o.set_vec(0, "f", F0[:, j])
                for _ in range(3):
                    o.vcycle()
                assert np.array_equal(o.get_vec(0, "u"), want[:, j]), j
        ref.close()
        eager.close()


def test_every_coarse_solve_kind_is_covered(amg, oracle):
    kinds = {want for _, want, _ in HIER.values() if want is not None}
    assert kinds == {BAND, SPIKE, WIDE, CHAIN}


def test_block_vcycle_full_size_bench_object(amg, oracle):
    """the bench.py object (K-Patch and the other fusions on in the single path), k = 4"""
    mg = amg.Multigrid.poisson(4096, 16, smoother=amg.SM_JACOBI, smoother_iters=2, omega=0.6)
    n0 = mg.get_n_dofs(0)
    rng = np.random.default_rng(5)
    U0 = rng.standard_normal((n0, 4))
    F0 = rng.standard_normal((n0, 4))
    U = dev(U0)
    mg.block_vcycles(U, dev(F0), n=2)
    torch.cuda.synchronize()
    got = U.cpu().numpy()
    want = single_columns(mg, U0, F0, 2)
    for j in range(4):
        assert np.array_equal(got[:, j], want[:, j]), j
    mg.close()


def test_block_calls_leave_the_solver_state_alone(amg, oracle):
    A, b = oracle.laplacian(128), oracle.rhs(128)
    mk = lambda: amg.Multigrid(*csc(A), b, 4, exact_coarse_solve=True, **JAC22)
    mg, twin = mk(), mk()
    mg.vcycle(2)
    twin.vcycle(2)
    u_before, f_before = mg.get_soln(0), mg.get_rhs(0)
    rng = np.random.default_rng(3)
    n0 = mg.get_n_dofs(0)
    U = dev(rng.standard_normal((n0, 5)))
    mg.block_vcycles(U, dev(rng.standard_normal((n0, 5))), n=2)
    mg.block_pcg(dev(rng.standard_normal((n0, 5))), rtol=1e-8, max_iters=20)
    mg.block_rss(U, dev(rng.standard_normal((n0, 5))))
    assert np.array_equal(mg.get_soln(0), u_before)
    assert np.array_equal(mg.get_rhs(0), f_before)
    mg.vcycle()
    twin.vcycle()
    assert np.array_equal(mg.get_soln(0), twin.get_soln(0))
    mg.close()
    twin.close()


@pytest.mark.parametrize("name", ["host255x6", "rs96"])
def test_block_rss_equals_rss_per_column(amg, oracle, name):
    build, _, _ = HIER[name]
    for sm in (JAC22, cheb(2, 1)):
        mg = build(amg, oracle, True, **sm)
        n0 = mg.get_n_dofs(0)
        rng = np.random.default_rng(4)
        U0, F0 = rng.standard_normal((n0, 5)), rng.standard_normal((n0, 5))
        got = mg.block_rss(dev(U0), dev(F0))
        for j in range(5):
            mg.set_vec(0, "u", U0[:, j])
            mg.set_vec(0, "f", F0[:, j])
            assert got[j] == mg.rss(), (name, j)
        mg.close()


def _pcg_case(amg, mg, rtol, max_iters):
    n0 = mg.get_n_dofs(0)
    rng = np.random.default_rng(9)
    b0 = mg.get_rhs(0)
    # a converged solution of b0: restarting from it stops at once
    mg.set_vec(0, "u", np.zeros(n0))
    xs, _, rel_s = mg.pcg(rtol, max_iters)
    assert rel_s <= rtol
    B0 = np.stack([np.zeros(n0), b0, 1e-6 * b0, 1e6 * b0, rng.standard_normal(n0), rng.standard_normal(n0)], 1)
    X0 = np.zeros_like(B0)
    X0[:, 1] = xs
    X0[:, 5] = rng.standard_normal(n0)
    X = dev(X0)
    X, it, rel = mg.block_pcg(dev(B0), X, rtol=rtol, max_iters=max_iters)
    torch.cuda.synchronize()
    got = X.cpu().numpy()
    assert it[0] == 0 and it[1] == 0
    assert rel[1] <= rtol
    for j in range(B0.shape[1]):
        mg.set_vec(0, "f", B0[:, j])
        mg.set_vec(0, "u", X0[:, j])
        x, it_s, rel_s = mg.pcg(rtol, max_iters)
        assert it[j] == it_s, (j, it[j], it_s)
        assert rel[j] == rel_s, j
        assert np.array_equal(got[:, j], x), j
    assert len(set(it.tolist())) > 1  # the columns really stopped at different times


def test_block_pcg_equals_pcg_per_column_strength_based(amg, oracle):
    A = oracle.laplacian(1024)
    mg = amg.Multigrid.ruge_stueben(*csc(A), oracle.rhs(1024), 25, 0.25, 500, **JAC22)
    _pcg_case(amg, mg, 1e-9, 60)
    mg.close()


def test_block_pcg_equals_pcg_per_column_chebyshev(amg, oracle):
    A = oracle.laplacian(96)
    mg = amg.Multigrid(*csc(A), oracle.rhs(96), 4, exact_coarse_solve=True, **cheb(2, 1))
    _pcg_case(amg, mg, 1e-9, 80)
    mg.close()


def _expected_must_move(mg, k, iters, w):
    nl = mg.n_levels
    n = [mg.get_n_dofs(l) for l in range(nl)]
    nnz = [int(amg_lib_nnz(mg, l)) for l in range(nl)]
    mat = 0.0
    vec = 0.0
    for l in range(nl - 1):
        mat += (2 * iters + 1) * (12.0 * nnz[l] + 4.0 * (n[l] + 1))   # sweeps + residual
        vec += 2 * iters * 24.0 * n[l] + (2 * 16.0 * n[l] if iters % 2 else 0.0)
        vec += 24.0 * n[l]                                          # residual
        vec += 8.0 * n[l] + 16.0 * n[l + 1]                         # restriction + zeroed u_H
        vec += 8.0 * n[l + 1] + 16.0 * n[l]                         # prolongation + add
    nc = n[nl - 1]
    mat += 16.0 * nc * max(w, 1)                                    # banded factor
    vec += 24.0 * nc + 32.0 * nc                                    # f, u; the column reorderings
    return mat + k * vec


def amg_lib_nnz(mg, l):
    import amg_ctypes
    return amg_ctypes.lib().amg_hip_get_level_nnz(mg._h, l)


@pytest.mark.parametrize("iters", [1, 2])
def test_block_must_move_matches_the_level_sizes(amg, oracle, iters):
    A, b = oracle.laplacian(128), oracle.rhs(128)
    mg = amg.Multigrid(*csc(A), b, 4, smoother=amg.SM_JACOBI, smoother_iters=iters, omega=0.6,
                       keep_structural_zeros=True, exact_coarse_solve=True)
    assert kind(amg, mg) == BAND
    for k in (1, 8):
        want = _expected_must_move(mg, k, iters, mg.coarse_halfbw())
        assert mg.block_must_move(k) == pytest.approx(want, rel=1e-12), k
    mg.close()


def test_block_refusals_leave_the_state_unchanged(amg, oracle):
    A, b = oracle.laplacian(64), oracle.rhs(64)
    n0 = 64 * 64
    U, F = dev(np.ones((n0, 4))), dev(np.ones((n0, 4)))
    for mk in (lambda: amg.Multigrid(*csc(A), b, 3, smoother=amg.SM_SPGS),
               lambda: amg.Multigrid(*csc(A), b, 3, smoother=amg.SM_MULTICOLOR_GS)):
        mg = mk()
        mg.vcycle()
        u, f = mg.get_soln(0), mg.get_rhs(0)
        for call in (lambda: mg.block_vcycles(U, F), lambda: mg.block_rss(U, F), lambda: mg.block_pcg(F),
                     lambda: mg.block_must_move(4)):
            with pytest.raises(amg.AmgHipError) as e:
                call()
            assert e.value.status == amg.EUNSUPPORTED
        assert np.array_equal(mg.get_soln(0), u) and np.array_equal(mg.get_rhs(0), f)
        mg.close()
    w = amg.Multigrid.poisson_window(256, 32, 128, 3)
    with pytest.raises(amg.AmgHipError) as e:
        w.block_must_move(2)
    assert e.value.status == amg.EUNSUPPORTED
    w.close()
    mg = amg.Multigrid(*csc(A), b, 3, **JAC22)
    mg.vcycle()
    u, f = mg.get_soln(0), mg.get_rhs(0)
    L = amg.lib()
    for k in (0, 17):
        assert L.amg_hip_block_vcycles(mg._h, k, F.data_ptr(), U.data_ptr(), 1) == amg.EINVAL
    big = torch.zeros(n0 * 4 + 1, dtype=torch.float64, device="cuda")
    odd = big[1:].view(n0, 4)  # contiguous, 8 bytes off a 16-byte boundary
    with pytest.raises(amg.AmgHipError) as e:
        mg.block_vcycles(odd, F)
    assert e.value.status == amg.EINVAL
    U_before = U.clone()
    mg.block_vcycles(U, F, n=0)  # no cycle: U unchanged
    torch.cuda.synchronize()
    assert torch.equal(U, U_before)
    assert np.array_equal(mg.get_soln(0), u) and np.array_equal(mg.get_rhs(0), f)
    mg.close()
