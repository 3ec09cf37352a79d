"""Chebyshev polynomial smoother (AMG_HIP_SM_CHEBYSHEV) on the device: per-level smoothing and whole
V-cycles against the numpy / scipy twin (tests/cheb_twin.py), degree 1 against true Jacobi bit for
bit, bit-identity across layouts and cycle paths, PCG, convergence against true Jacobi, and the
byte accounting / measurement hooks."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "algebraic-multigrid_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cheb_twin as T  # noqa: E402

pytestmark = pytest.mark.gpu
SM = 5  # AMG_HIP_SM_CHEBYSHEV


def csc(A):
    return A.colptr, A.rowind, A.val


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def make(amg, oracle, kind, degree=2, iters=1, **kw):
    kw = dict(smoother=SM, smoother_iters=iters, cheb_degree=degree, **kw)
    if kind == "poisson-513":
        return amg.Multigrid.poisson(513, 8, **kw)
    if kind == "poisson3d-33":
        return amg.Multigrid.poisson(33, 4, dim=3, **kw)
    if kind == "host-255":
        A, b = oracle.laplacian(255), oracle.rhs(255)
        return amg.Multigrid(*csc(A), b, 6, **kw)
    if kind == "rs-96":
        A, b = oracle.laplacian(96), oracle.rhs(96)
        return amg.Multigrid.ruge_stueben(*csc(A), b, 12, 0.25, 50, **kw)
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["poisson-513", "poisson3d-33", "host-255", "rs-96"])
@pytest.mark.parametrize("degree,iters", [(1, 1), (2, 1), (3, 1), (1, 2), (2, 2), (3, 2)])
def test_level_smoothing_equals_twin(amg, oracle, kind, degree, iters):
    mg = make(amg, oracle, kind, degree, iters)
    tw = T.Twin(mg, degree, 0.3, 1.0, iters)
    rng = np.random.default_rng(degree * 10 + iters)
    for l in range(mg.n_levels):
        assert mg.cheb_bounds(l) == pytest.approx(tw.bounds[l], rel=1e-15)
        n = mg.get_n_dofs(l)
        u, f = rng.standard_normal(n), rng.standard_normal(n)
        mg.set_vec(l, "u", u)
        mg.set_vec(l, "f", f)
        mg.level_op(l, 0)
        mg.sync()
        got = mg.get_soln(l)
        assert rel(got, tw.smooth(l, u, f)) <= 1e-12, (kind, l)
        assert np.array_equal(mg.get_rhs(l), f)
    mg.close()


def test_degree1_is_true_jacobi_bit_for_bit(amg, oracle):
    A, b = oracle.laplacian(100), oracle.rhs(100)
    mats = [csc(A)]
    # a symmetric matrix with a non-trivial bound: an RS coarse level, symmetrised bitwise
    rs = amg.Multigrid.ruge_stueben(*csc(oracle.laplacian(64)), oracle.rhs(64), 4, 0.25, 50, smoother=SM,
                                    host_only=True)
    n1 = rs.get_n_dofs(1)
    B = T.csr_of(*rs.get_coefficient_matrix(1), n1, n1)
    S = ((B + B.T) / 2).tocsc()
    S.sort_indices()
    mats.append((S.indptr, S.indices, S.data))
    rs.close()
    rng = np.random.default_rng(3)
    for cp, ri, v in mats:
        n = len(cp) - 1
        u0, f = rng.standard_normal(n), rng.standard_normal(n)
        G = T.gershgorin(T.csr_of(cp, ri, v, n, n))
        lo, hi = 0.3 * G, 1.0 * G
        uc = amg.smooth_chebyshev(cp, ri, v, u0, f, degree=1, lower=0.3, upper=1.0, n_iters=2)
        uj, _, _ = amg.smooth(amg.SM_JACOBI, cp, ri, v, u0, f, n_iters=2, omega=2 / (lo + hi))
        assert np.array_equal(uc, uj)
        # and the stand-alone call is the twin
        u3 = amg.smooth_chebyshev(cp, ri, v, u0, f, degree=3, lower=0.3, upper=1.0, n_iters=2)
        assert rel(u3, T.cheb_smooth(T.csr_of(cp, ri, v, n, n), u0, f, lo, hi, 3, 2)) <= 1e-12


def _state(mg):
    return [(mg.get_soln(l), mg.get_rhs(l)) for l in range(mg.n_levels)]


def _same(a, b):
    return all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


def _cycles(mg, k):
    mg.vcycle(k)
    mg.sync()
    st = _state(mg)
    mg.close()
    return st


def test_layouts_row_types_index16_nontemporal_bit_identical(amg, oracle):
    A, b = oracle.laplacian(511), oracle.rhs(511)
    Ar, br = oracle.laplacian(128), oracle.rhs(128)
    for deg in (2, 3):
        ref = ref_rs = None
        try:
            for lay in (amg.LAYOUT_CSR, amg.LAYOUT_SELL, amg.LAYOUT_DICT):
                for rt, i16, nt in ((1, 1, 1), (0, 0, 0), (1, 0, 1), (0, 1, 0)):
                    amg.set_row_types(rt)
                    amg.set_index16(i16)
                    amg.set_nontemporal(nt)
                    st = _cycles(amg.Multigrid(*csc(A), b, 7, smoother=SM, cheb_degree=deg, layout=lay), 5)
                    ref = ref or st
                    assert _same(st, ref), (deg, lay, rt, i16, nt)
                    st = _cycles(amg.Multigrid.ruge_stueben(*csc(Ar), br, 12, 0.25, 50, smoother=SM,
                                                            cheb_degree=deg, layout=lay), 5)
                    ref_rs = ref_rs or st
                    assert _same(st, ref_rs), ("rs", deg, lay, rt, i16, nt)
        finally:
            amg.set_row_types(1)
            amg.set_index16(1)
            amg.set_nontemporal(1)


def test_large_level_sell_nontemporal_equals_dict(amg):
    # 2048^2: the SELL-64 matrix of level 0 is beyond the non-temporal threshold (~210 MB)
    base = _cycles(amg.Multigrid.poisson(2048, 12, smoother=SM, cheb_degree=3), 2)
    sell = amg.Multigrid.poisson(2048, 12, smoother=SM, cheb_degree=3, layout=amg.LAYOUT_SELL)
    assert sell.level_layout(0)[0] == amg.LAYOUT_SELL
    assert _same(_cycles(sell, 2), base)


@pytest.mark.parametrize("deg,iters", [(2, 1), (3, 1), (1, 1), (2, 2)])
def test_graph_fusion_and_setup_paths_bit_identical(amg, oracle, deg, iters):
    kw = dict(smoother=SM, cheb_degree=deg, smoother_iters=iters)
    ref = _cycles(amg.Multigrid.poisson(1024, 10, **kw), 5)
    assert _same(_cycles(amg.Multigrid.poisson(1024, 10, use_graph=False, **kw), 5), ref)
    assert _same(_cycles(amg.Multigrid.poisson(1024, 10, no_fusion=True, **kw), 5), ref)
    A, b = oracle.laplacian(1024), oracle.rhs(1024)
    host = amg.Multigrid(*csc(A), b, 10, **kw)
    dev = amg.Multigrid.poisson(1024, 10, **kw)
    for l in range(host.n_levels):
        assert host.cheb_bounds(l) == dev.cheb_bounds(l), l      # host sum vs device kernel: same bits
    dev.close()
    assert _same(_cycles(host, 5), ref)


def _twin_cycles(mg, tw, k, tol):
    b = mg.get_rhs(0)
    u = np.zeros(b.size)
    for _ in range(k):
        u = tw.vcycle(u, b)[0][0]
    mg.vcycle(k)
    mg.sync()
    got = mg.get_soln(0)
    assert rel(got, u) <= tol, rel(got, u)


@pytest.mark.parametrize("kind", ["poisson-1024", "rs-1024", "poisson3d-64"])
def test_vcycles_equal_twin(amg, oracle, kind):
    if kind == "poisson-1024":
        mg = amg.Multigrid.poisson(1024, 6, smoother=SM)
    elif kind == "poisson3d-64":
        mg = amg.Multigrid.poisson(64, 6, dim=3, smoother=SM, cheb_degree=3)
    else:
        A, b = oracle.laplacian(1024), oracle.rhs(1024)
        mg = amg.Multigrid.ruge_stueben(*csc(A), b, 25, 0.25, 500, smoother=SM)
    deg = 3 if kind == "poisson3d-64" else 2
    _twin_cycles(mg, T.Twin(mg, deg, 0.3, 1.0, 1), 4, 1e-10)
    mg.close()


def test_full_size_4096_vcycles_equal_twin(amg):
    mg = amg.Multigrid.poisson(4096, 16, smoother=SM)
    _twin_cycles(mg, T.Twin(mg, 2, 0.3, 1.0, 1), 2, 1e-10)
    mg.close()


def _rs_1024(amg, oracle, **kw):
    A, b = oracle.laplacian(1024), oracle.rhs(1024)
    return amg.Multigrid.ruge_stueben(*csc(A), b, 25, 0.25, 500, **kw)


def test_pcg_matches_twin_iterations(amg, oracle):
    mg = _rs_1024(amg, oracle, smoother=SM)
    tw = T.Twin(mg, 2, 0.3, 1.0, 1)
    _, it_t, rel_t = tw.pcg(mg.get_rhs(0), 1e-8)
    _, it, r = mg.pcg(1e-8, 200)
    print(f"\nRS 1024^2 PCG to 1e-8, Chebyshev(2) 1+1: device {it} iterations (relres {r:.3e}), twin {it_t}")
    assert r <= 1e-8 and abs(it - it_t) <= 1
    mg.close()


def test_contraction_beats_true_jacobi_at_equal_passes(amg, oracle):
    def contraction(mg):
        mg.vcycle(5)
        r5 = mg.rss()
        mg.vcycle(5)
        r10 = mg.rss()
        mg.close()
        return (r10 / r5) ** (1 / 10)   # rss is a sum of squares
    ch = contraction(_rs_1024(amg, oracle, smoother=SM, cheb_degree=2, smoother_iters=1))
    jac = contraction(_rs_1024(amg, oracle, smoother=amg.SM_JACOBI, omega=0.6, smoother_iters=2))
    print(f"\nRS 1024^2 residual contraction per V-cycle (cycles 5-10): Chebyshev(2) 1+1 {ch:.4f}, "
          f"true Jacobi 2+2 omega=0.6 {jac:.4f}")
    assert ch < jac


@pytest.mark.parametrize("deg,iters", [(1, 1), (2, 1), (3, 1), (4, 2), (3, 3)])
def test_must_move_and_profile_hooks(amg, deg, iters):
    mg = amg.Multigrid.poisson(1024, 8, smoother=SM, cheb_degree=deg, smoother_iters=iters)
    bare = amg.Multigrid.poisson(1024, 8, smoother=SM, cheb_degree=deg, smoother_iters=0)
    predicted = 0.0
    for l in range(mg.n_levels - 1):      # pre- and post-smoothing; the coarsest level is solved
        n, mat = mg.get_n_dofs(l), mg.level_layout(l)[1]
        steps = [mat + 24 * n + (0 if j == 0 else 8 * n) + (0 if j == deg - 1 else 8 * n) for j in range(deg)]
        leg = iters * sum(steps) + (16 * n if (iters * deg) % 2 else 0)
        predicted += 2 * leg
    assert mg.cycle_must_move() - bare.cycle_must_move() == pytest.approx(predicted, rel=1e-12)
    avg, mn, sweeps, name, nbytes = mg.profile_fine_sweep(5)
    assert avg > 0 and mn > 0 and sweeps == 1
    mode = 16 if deg >= 3 else (17 if deg == 2 else 19)        # middle step, else step 0
    assert name.startswith(f"dict_kernel<{mode},"), name
    n, mat = mg.get_n_dofs(0), mg.level_layout(0)[1]
    assert nbytes == mat + 24 * n + {16: 16 * n, 17: 8 * n, 19: 0}[mode]
    before = mg.get_soln(0)
    mg.profile_fine_sweep(3)
    assert np.array_equal(mg.get_soln(0), before)               # u is not written
    mg.close()
    bare.close()


def test_dropin_chebyshev_runs(amg, tmp_path):
    import subprocess
    from test_chebyshev import build_dropin
    exe = build_dropin(amg, tmp_path)
    p = subprocess.run([exe, "run"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
