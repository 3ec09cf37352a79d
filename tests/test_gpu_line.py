"""Line smoother (AMG_HIP_SM_LINE_JACOBI) on the device: per-level sweeps, the stand-alone call and
whole V-cycles against the numpy twin (tests/line_twin.py), bit-identity across layouts, cycle paths
and constructors, convergence against the twin's cycle counts (4096^2 included), PCG against true
Jacobi, and the byte accounting.

The bound of every comparison with the twin comes from the reference side: with e64 the 2-norm
distance of the twin's float64 result from its longdouble result on the same inputs, the device must
lie within max(8 e64, 1e-14 ||u||) of the longdouble result.  Every test prints the ratio it found."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "algebraic-multigrid_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import line_twin as T  # noqa: E402

pytestmark = pytest.mark.gpu
SM = 6  # AMG_HIP_SM_LINE_JACOBI
OMEGA = 0.7


def csc(A):
    return A.colptr, A.rowind, A.val


def make(amg, oracle, kind, iters=1, **kw):
    kw = dict(smoother=SM, smoother_iters=iters, omega=OMEGA, **kw)
    if kind == "poisson-513":
        return amg.Multigrid.poisson(513, 8, **kw)
    if kind == "poisson-1024":
        return amg.Multigrid.poisson(1024, 12, **kw)
    if kind == "poisson3d-33":
        return amg.Multigrid.poisson(33, 4, dim=3, **kw)
    if kind == "host-255":
        A, b = oracle.laplacian(255), oracle.rhs(255)
        return amg.Multigrid(*csc(A), b, 6, **kw)
    if kind == "rs-96":
        A, b = oracle.laplacian(96), oracle.rhs(96)
        return amg.Multigrid.ruge_stueben(*csc(A), b, 12, 0.25, 50, **kw)
    raise KeyError(kind)


def check(got, ref, e64, scale, what):
    ok, dist, bound, ratio = T.within(got, ref, e64, scale)
    print(f"  {what}: distance {dist:.3e}, e64 {e64:.3e}, ratio {ratio:.2f}, bound {bound:.3e}")
    assert ok, (what, dist, bound, ratio)
    return ratio


@pytest.mark.parametrize("kind", ["poisson-513", "poisson-1024", "poisson3d-33", "host-255", "rs-96"])
@pytest.mark.parametrize("iters", [1, 2])
def test_level_sweep_equals_twin(amg, oracle, kind, iters):
    mg = make(amg, oracle, kind, iters)
    tw = T.Twin(mg, OMEGA, iters)
    rng = np.random.default_rng(10 + iters)
    worst = 0.0
    print()
    for l in range(mg.n_levels):
        assert mg.line_stride(l) == tw.stride[l], (kind, l)
        n = mg.get_n_dofs(l)
        u, f = rng.standard_normal(n), rng.standard_normal(n)
        mg.set_vec(l, "u", u)
        mg.set_vec(l, "f", f)
        mg.level_op(l, 0)
        mg.sync()
        got = mg.get_soln(l)
        ref, e64 = T.sweep_bound(tw.A[l], u, f, tw.stride[l], OMEGA, iters)
        worst = max(worst, check(got, ref, e64, np.linalg.norm(got), f"{kind} iters {iters} level {l} "
                                 f"(n {n}, stride {tw.stride[l]})"))
        assert np.array_equal(mg.get_rhs(l), f)
    print(f"  {kind} iters {iters}: largest ratio {worst:.2f}")
    mg.close()


def _banded(n, rng):
    """symmetric, strictly diagonally dominant, entries at offsets 1, 2, 63, 64, 65 and n - 1"""
    offs = [1, 2, 63, 64, 65, n - 1]
    bands = [-(0.2 + rng.random(n - o)) for o in offs]
    A = sp.diags(bands + bands, offs + [-o for o in offs], format="csr")
    A = A + sp.diags(np.asarray(abs(A).sum(axis=1)).ravel() + 0.5 + rng.random(n))
    A = sp.csc_matrix(A)
    A.sort_indices()
    return A


@pytest.mark.parametrize("n", [2117, 64 * 33])
def test_smooth_line_explicit_strides(amg, n):
    rng = np.random.default_rng(n)
    A = _banded(n, rng)
    Ar = sp.csr_matrix(A)
    u, f = rng.standard_normal(n), rng.standard_normal(n)
    print()
    assert T.stride_rule(Ar) in (1, 2, 63, 64, 65, n - 1)
    got = amg.smooth_line(A.indptr, A.indices, A.data, u, f, stride=0, omega=OMEGA, iters=1)
    ref, e64 = T.sweep_bound(Ar, u, f, T.stride_rule(Ar), OMEGA, 1)
    check(got, ref, e64, np.linalg.norm(got), f"n {n} automatic stride {T.stride_rule(Ar)}")
    for s in (1, 2, 63, 64, 65, n - 1, n, n + 7):
        for iters in (1, 2):
            got = amg.smooth_line(A.indptr, A.indices, A.data, u, f, stride=s, omega=OMEGA, iters=iters)
            ref, e64 = T.sweep_bound(Ar, u, f, s, OMEGA, iters)
            check(got, ref, e64, np.linalg.norm(got), f"n {n} stride {s} iters {iters}")
            if s >= n:      # every row its own chain: weighted Jacobi
                uj, _, _ = amg.smooth(amg.SM_JACOBI, A.indptr, A.indices, A.data, u, f, n_iters=iters, omega=OMEGA)
                check(uj, ref, e64, np.linalg.norm(uj), f"n {n} true Jacobi iters {iters} against the same reference")


def test_smooth_line_huge_strides_equal_stride_n(amg):
    """Every stride >= n means the same thing (each row its own chain): 2^31, 2^60 and INT64_MAX must
    give the bits of stride = n (products of a position and such a stride would overflow int64)."""
    n = 2117
    rng = np.random.default_rng(11)
    A = _banded(n, rng)
    u, f = rng.standard_normal(n), rng.standard_normal(n)
    for iters in (1, 2):
        ref = amg.smooth_line(A.indptr, A.indices, A.data, u, f, stride=n, omega=OMEGA, iters=iters)
        assert not np.array_equal(ref, u) and np.all(np.isfinite(ref))
        for s in (n + 1, 2 ** 31, 2 ** 60, 2 ** 63 // 31, 2 ** 63 - 1):
            got = amg.smooth_line(A.indptr, A.indices, A.data, u, f, stride=s, omega=OMEGA, iters=iters)
            assert np.array_equal(got, ref), (s, iters)


@pytest.mark.parametrize("n,s", [(50021, 1), (2 * 40000 + 1, 2)])
def test_smooth_line_long_chains_cross_the_lds_chunks(amg, n, s):
    """Few long chains with more than 1024 separators each (1563 and 1250, no multiple of 1024): the
    reduced system is walked in several LDS chunks with the recurrence carried between them."""
    assert (n // s) // 32 > 1024 and ((n // s) // 32) % 1024 != 0
    rng = np.random.default_rng(n)
    offs = [s, 3 * s + 1]
    bands = [-(0.9 + 0.2 * rng.random(n - offs[0])), -0.05 * rng.random(n - offs[1])]
    A = sp.diags(bands + bands, offs + [-o for o in offs], format="csr")
    A = sp.csc_matrix(A + sp.diags(np.asarray(abs(A).sum(axis=1)).ravel() + 0.01 + 0.05 * rng.random(n)))
    A.sort_indices()
    Ar = sp.csr_matrix(A)
    assert T.stride_rule(Ar) == s
    u, f = rng.standard_normal(n), rng.standard_normal(n)
    print()
    for stride, iters in ((0, 1), (s, 2)):      # the automatic rule and the explicit stride
        got = amg.smooth_line(A.indptr, A.indices, A.data, u, f, stride=stride, omega=OMEGA, iters=iters)
        ref, e64 = T.sweep_bound(Ar, u, f, s, OMEGA, iters)
        check(got, ref, e64, np.linalg.norm(got), f"n {n} stride {stride or 'auto'} iters {iters}")


def test_dropin_line_jacobi_runs(amg, tmp_path):
    import subprocess
    from test_line_smoother import build_dropin
    exe = build_dropin(amg, tmp_path)
    p = subprocess.run([exe, "run"], capture_output=True, text=True, timeout=300)
    print("\n" + p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr


def _state(mg):
    return [(mg.get_soln(l), mg.get_rhs(l)) for l in range(mg.n_levels)]


def _same(a, b):
    return all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


def _sweep_then_cycles(mg, k=3):
    """one sweep on every level from seeded vectors, then k V-cycles from u = 0; the states of both"""
    rng = np.random.default_rng(4)
    b = mg.get_rhs(0)
    sweeps = []
    for l in range(mg.n_levels):
        n = mg.get_n_dofs(l)
        mg.set_vec(l, "u", rng.standard_normal(n))
        mg.set_vec(l, "f", rng.standard_normal(n))
        mg.level_op(l, 0)
        mg.sync()
        sweeps.append(mg.get_soln(l))
    mg.set_vec(0, "f", b)
    mg.set_vec(0, "u", np.zeros(b.size))
    mg.vcycle(k)
    mg.sync()
    st = _state(mg)
    mg.close()
    return sweeps, st


def _equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and _same(a[1], b[1])


def test_layouts_bit_identical(amg, oracle):
    A, b = oracle.laplacian(511), oracle.rhs(511)
    Ar, br = oracle.laplacian(128), oracle.rhs(128)
    ref = ref_rs = None
    for lay in (amg.LAYOUT_DICT, amg.LAYOUT_SELL, amg.LAYOUT_CSR):
        st = _sweep_then_cycles(amg.Multigrid(*csc(A), b, 12, smoother=SM, omega=OMEGA, layout=lay))
        ref = ref or st
        assert _equal(st, ref), lay
        st = _sweep_then_cycles(amg.Multigrid.ruge_stueben(*csc(Ar), br, 12, 0.25, 50, smoother=SM, omega=OMEGA,
                                                          layout=lay))
        ref_rs = ref_rs or st
        assert _equal(st, ref_rs), ("rs", lay)


@pytest.mark.parametrize("iters", [1, 2])
def test_graph_eager_and_setup_paths_bit_identical(amg, oracle, iters):
    kw = dict(smoother=SM, omega=OMEGA, smoother_iters=iters)
    ref = _sweep_then_cycles(amg.Multigrid.poisson(1024, 12, **kw))
    assert _equal(_sweep_then_cycles(amg.Multigrid.poisson(1024, 12, use_graph=False, **kw)), ref)
    assert _equal(_sweep_then_cycles(amg.Multigrid.poisson(1024, 12, no_fusion=True, **kw)), ref)
    A, b = oracle.laplacian(1024), oracle.rhs(1024)
    host = amg.Multigrid(*csc(A), b, 12, **kw)
    dev = amg.Multigrid.poisson(1024, 12, **kw)
    assert [host.line_stride(l) for l in range(12)] == [dev.line_stride(l) for l in range(12)]
    dev.close()
    assert _equal(_sweep_then_cycles(host), ref)


@pytest.mark.parametrize("kind", ["poisson-256-16", "host-127-12", "poisson3d-33-14"])
def test_vcycles_equal_twin(amg, oracle, kind):
    kw = dict(smoother=SM, omega=OMEGA)
    if kind == "poisson-256-16":
        mg = amg.Multigrid.poisson(256, 16, **kw)
    elif kind == "host-127-12":
        A, b = oracle.laplacian(127), oracle.rhs(127)
        mg = amg.Multigrid(*csc(A), b, 12, **kw)
    else:
        mg = amg.Multigrid.poisson(33, 14, dim=3, **kw)
    tw = T.Twin(mg, OMEGA, 1)
    assert tw.n[-1] <= 256                  # the twin's longdouble cycle solves the coarsest level in longdouble
    b = mg.get_rhs(0)
    u64, uld = np.zeros(b.size), np.zeros(b.size, np.longdouble)
    for _ in range(3):
        u64 = tw.vcycle(u64, b)[0][0]
        uld = tw.vcycle(uld, b, np.longdouble)[0][0]
    e64 = float(np.linalg.norm(u64.astype(np.longdouble) - uld))
    mg.vcycle(3)
    mg.sync()
    got = mg.get_soln(0)
    print()
    check(got, uld, e64, np.linalg.norm(got), f"{kind}: level-0 u after 3 V-cycles")
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


def test_convergence_256_equals_twin_count(amg):
    mg = amg.Multigrid.poisson(256, 16, smoother=SM, omega=OMEGA)
    tw = T.Twin(mg, OMEGA, 1)
    f = np.random.default_rng(0).standard_normal(256 * 256)
    kt, _ = tw.cycles_to(f, 1e-8, 30)
    k, hist = _device_cycles_to(mg, f)
    print(f"\n256^2/16 line Jacobi omega 0.7 1+1 to ||r||/||r0|| <= 1e-8: device {k} cycles, twin {kt}; "
          f"late factor {hist[-1] / hist[-2]:.3f}")
    assert k is not None and kt is not None and abs(k - kt) <= 1
    mg.close()


def test_convergence_4096_within_twin_512_plus_three(amg, oracle):
    """The count at full size must not exceed the twin's count at 512^2 / 18 levels (recomputed here;
    15) plus three.  Measured on MI355X: 15 cycles, ||r|| / ||r0|| 1.08e-8 after 14 and 3.94e-9 after
    15 ("Line smoother"); the count found is printed."""
    A, b = oracle.laplacian(512), oracle.rhs(512)
    small = amg.Multigrid(*csc(A), b, 18, smoother=SM, omega=OMEGA, host_only=True)
    tw = T.Twin(small, OMEGA, 1)
    kt, _ = tw.cycles_to(np.random.default_rng(0).standard_normal(512 * 512), 1e-8, 30)
    small.close()
    assert kt is not None
    mg = amg.Multigrid.poisson(4096, 16, smoother=SM, omega=OMEGA)
    assert [mg.line_stride(l) for l in range(16)] == [4096 >> l for l in range(12)] + [1] * 4
    f = np.random.default_rng(1).standard_normal(4096 * 4096)
    k, hist = _device_cycles_to(mg, f)
    print(f"\n4096^2/16 line Jacobi omega 0.7 1+1 to ||r||/||r0|| <= 1e-8: device {k} cycles "
          f"(twin at 512^2/18: {kt}); history {' '.join(f'{h:.2e}' for h in hist)}")
    assert k is not None and k <= kt + 3
    mg.close()


def test_pcg_beats_true_jacobi(amg):
    line = amg.Multigrid.poisson(1024, 12, smoother=SM, omega=OMEGA, smoother_iters=1)
    jac = amg.Multigrid.poisson(1024, 12, smoother=amg.SM_JACOBI, omega=0.6, smoother_iters=2)
    xl, itl, rl = line.pcg(1e-8, 500)
    xj, itj, rj = jac.pcg(1e-8, 500)
    print(f"\npoisson(1024, 12) PCG to 1e-8: line 1+1 {itl} iterations (relres {rl:.2e}), true Jacobi 2+2 {itj} "
          f"({rj:.2e})")
    assert rl <= 1e-8 and rj <= 1e-8 and itl < itj
    assert np.linalg.norm(xl - xj) <= 1e-6 * np.linalg.norm(xj)
    line.close()
    jac.close()


def test_must_move_bytes(amg):
    """Per sweep: the residual (matrix + f, u, r = 24 n) and K-Line: 80 B per interior row, 96 B per
    separator row ("Line smoother").  64^2, 4 levels, by hand: level 0 has n = 4096,
    s = 64, 64 positions per chain, separators at positions 31 and 63 -> 128 separator rows."""
    mg = amg.Multigrid.poisson(64, 4, smoother=SM, omega=OMEGA, smoother_iters=1)
    bare = amg.Multigrid.poisson(64, 4, smoother=SM, omega=OMEGA, smoother_iters=0)
    predicted = 0.0
    for l in range(mg.n_levels - 1):        # pre- and post-smoothing; the coarsest level is solved
        n, mat, s = mg.get_n_dofs(l), mg.level_layout(l)[1], mg.line_stride(l)
        sep = int(np.count_nonzero((np.arange(n) // s) % 32 == 31))
        if l == 0:
            assert (n, s, sep) == (4096, 64, 128)
        predicted += 2 * (mat + 24 * n + 80 * (n - sep) + 96 * sep)
    assert mg.cycle_must_move() - bare.cycle_must_move() == pytest.approx(predicted, rel=1e-12)
    with pytest.raises(amg.AmgHipError):
        mg.profile_fine_sweep(3)
    mg.close()
    bare.close()
