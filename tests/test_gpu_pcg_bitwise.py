"""The three PCG drivers (solver.cpp: pcg_run behind amg_hip_pcg and amg_hip_pcg_mixed, amg_hip_block_pcg)
bit for bit against tests/pcg_twin.py: np.array_equal on x, `==` on the iteration count and on relres.

PCG corrects itself: a dot product that drops a tail, an update with a stale alpha or the r.z of the wrong
iteration still converges to a true solution, usually in the same number of iterations.  So the comparison
is on the TRAJECTORY: the device's iterate after max_iters = 1, 2, 3, 4, 6 (rtol = 0) is the twin's after as
many iterations.  Before any of that, amg_hip_apply (amg_hip_apply_f32) on the twin's first residual has
the bits of the twin's preconditioner, so a later difference points at the Krylov kernels, not the cycle.

  double   true Jacobi 2+2 omega 0.6 on Poisson 96^2 / 4 levels, captured and eager; the same on 513^2 / 8
           levels (263169 rows: the dot products take a second grid-stride pass with a ragged tail),
           max_iters <= 3; symmetric Gauss-Seidel with exact_gs on 96^2; the Ruge-Stueben hierarchy of
           knn(1600, 4, 1); the K-Patch hierarchy of Poisson 512^2 / 7 levels after vcycle(3) through the seam,
           max_iters <= 3.  Run to rtol = 1e-10 on 96^2 and knn.  Edge cases on 96^2.
  mixed    t64 and t33 of tests/test_gpu_f32_bitwise.py (full-coarsening tensor hierarchies, M^-1 = the
           float32 twin's cycle): max_iters = 1, 2, 3 and the run to rtol = 1e-8.
           With line smoothers (amg_hip_set_f32_lines) the float cycle has no bitwise twin: K-Line solves a
           line in segments with a Schur complement and is held to 8 e32 of a longdouble reference
           (tests/test_gpu_f32_lines.py), not to bits.  On that case the twin BORROWS M^-1 from the device
           (amg_hip_apply_f32 on the same solver); the dot products, updates, alpha, beta and the stopping
           rule are still the twin's own, the attribution check on that case only says that amg_hip_apply_f32
           gives the same bits twice.
  block    k = 3 and k = 16 on 96^2, columns that stop after different counts: every column against the
           TWIN, so that single == twin and block == twin close the chain from both ends."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sp = pytest.importorskip("scipy.sparse")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "algebraic-multigrid_amd"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import f32_twin as FT  # noqa: E402
import pcg_twin as PT  # noqa: E402
import test_gpu_cycle_irregular as CI  # noqa: E402
import test_gpu_f32_bitwise as FB  # noqa: E402
import test_gpu_f32_lines as FL  # noqa: E402
from test_gpu_patch_seam import SEAM_LINES, patch_everywhere  # noqa: E402,F401
from test_gpu_patch_xf import _problem as patch_problem  # noqa: E402

pytestmark = pytest.mark.gpu

JAC = dict(smoother=3, smoother_iters=2, omega=0.6)


def csc(A):
    return A.colptr, A.rowind, A.val


def dev(a):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


def apply_on_device(mg, v, f32=False):
    dv = dev(v)
    dz = torch.full_like(dv, float("nan"))
    (mg.apply_f32 if f32 else mg.apply_dev)(dv.data_ptr(), dz.data_ptr())
    mg.sync()
    return dz.cpu().numpy()


# ---- the double configurations: name -> (A, b, oracle twin, solver, largest max_iters) ----------------
def _poisson(n, L, spgs=False):
    def make(amg, oracle, **kw):
        A, b = oracle.laplacian(n), oracle.rhs(n)
        if spgs:
            ref = oracle.Multigrid(A, b, L)
            mg = amg.Multigrid(*csc(A), b, L, exact_coarse_solve=True, exact_gs=True, **kw)
        else:
            ref = oracle.Multigrid(A, b, L, smoother=oracle.SM_TRUE_JACOBI, smoother_iters=2, omega=0.6)
            mg = amg.Multigrid(*csc(A), b, L, exact_coarse_solve=True, **JAC, **kw)
        return A, b, ref, mg
    return make


def _knn(amg, oracle, **kw):
    M, A, b, Ps = CI.setup(oracle, "knn")
    ref = oracle.Multigrid(A, b, len(Ps) + 1, transfers=Ps, smoother=oracle.SM_TRUE_JACOBI, smoother_iters=2, omega=0.6)
    return A, np.array(b), ref, CI.solver(amg, oracle, "knn", **JAC, **kw)


def _patch(amg, oracle, **kw):
    """Poisson 512^2 with set_patch_min_rows(0) (the test's fixture): K-Patch on levels 0 .. 2, and the
    solver has just run vcycle(3) through the seam when the first preconditioner call comes"""
    A, b, L = patch_problem(oracle, "lap512")[:3]
    ref = oracle.Multigrid(A, b, L, smoother=oracle.SM_TRUE_JACOBI, smoother_iters=2, omega=0.6)
    mg = amg.Multigrid(*csc(A), b, L, exact_coarse_solve=True, **JAC, **kw)
    assert mg.patch_leg_lines(0, 2) == SEAM_LINES
    mg.vcycle(3)
    return A, b, ref, mg


CONFIGS = {
    "jac96-graph": (_poisson(96, 4), dict(use_graph=True), 6),
    "jac96-eager": (_poisson(96, 4), dict(use_graph=False), 6),
    "jac513": (_poisson(513, 8), {}, 3),
    "spgs96": (_poisson(96, 4, spgs=True), {}, 6),
    "knn-rs": (_knn, {}, 6),
    "patch512": (_patch, {}, 3),
}
STEPS = (1, 2, 3, 4, 6)


def check_run(mg, run, b, x0, rtol, max_iters, want, what):
    """one device run from x0 against the twin's (x, iters, relres)"""
    mg.set_vec(0, "u", x0)
    x, it, rel = run(rtol, max_iters)
    assert it == want[1], (what, it, want[1])
    assert np.float64(rel).view(np.uint64) == np.float64(want[2]).view(np.uint64), (what, rel, want[2])
    bad = np.flatnonzero(x.view(np.uint64) != want[0].view(np.uint64))
    assert bad.size == 0, (f"{what}: {bad.size} of {x.size} entries of x differ, first at {int(bad[0])}: "
                           f"device {x[bad[0]]!r} twin {want[0][bad[0]]!r}")
    assert np.array_equal(mg.get_rhs(0), b), what          # f is b again


def check_trajectory(mg, run, A, b, x0, apply, steps, what):
    top = max(steps)
    _, it, _, trace = PT.pcg(A, b, x0, apply, 0.0, top, keep_iterates=True)
    assert it == top and len(trace) == top
    assert all(np.isfinite(t[0]) and np.isfinite(t[2]) for t in trace)
    assert not np.array_equal(trace[0][3], x0)
    for k in steps:
        _, _, rel, xk = trace[k - 1]
        check_run(mg, run, b, x0, 0.0, k, (xk, k, rel), (what, "max_iters", k))
    print(f"\n{what}: n = {A.rows}, iterates 1 .. {top} bit for bit; relres " + " ".join(f"{t[2]:.3e}" for t in trace))


def _trajectory(amg, oracle, name):
    ctor, kw, top = CONFIGS[name]
    A, b, ref, mg = ctor(amg, oracle, **kw)
    try:
        x0 = 1e-3 * np.random.default_rng(4).standard_normal(A.rows)
        r0 = PT.first_residual(A, b, x0)
        # attribution: the cycle first
        assert np.array_equal(apply_on_device(mg, r0), ref.apply(r0)), (name, "amg_hip_apply on the first residual")
        check_trajectory(mg, mg.pcg, A, b, x0, ref.apply, [k for k in STEPS if k <= top], name)
    finally:
        mg.close()


@pytest.mark.parametrize("name", sorted(set(CONFIGS) - {"patch512"}))
def test_pcg_trajectory_has_the_twins_bits(amg, oracle, name):
    _trajectory(amg, oracle, name)


def test_pcg_trajectory_on_the_patch_hierarchy_has_the_twins_bits(amg, oracle, patch_everywhere):
    _trajectory(amg, oracle, "patch512")


@pytest.mark.parametrize("name", ["jac96-graph", "knn-rs"])
def test_pcg_run_to_tolerance_has_the_twins_bits(amg, oracle, name):
    ctor, kw, _ = CONFIGS[name]
    A, b, ref, mg = ctor(amg, oracle, **kw)
    try:
        x0 = np.zeros(A.rows)
        want = PT.pcg(A, b, x0, ref.apply, 1e-10, 200)
        assert 2 <= want[1] < 200 and want[2] <= 1e-10
        check_run(mg, mg.pcg, b, x0, 1e-10, 200, want, name)
        print(f"\n{name}: {want[1]} iterations, relres {want[2]!r}")
    finally:
        mg.close()


def test_pcg_edge_cases_have_the_twins_bits(amg, oracle):
    A, b, ref, mg = _poisson(96, 4)(amg, oracle)
    try:
        n = A.rows
        x0 = 1e-3 * np.random.default_rng(4).standard_normal(n)
        # no iteration allowed
        want = PT.pcg(A, b, x0, ref.apply, 1e-10, 0)
        assert want[1] == 0 and np.array_equal(want[0], x0)
        check_run(mg, mg.pcg, b, x0, 1e-10, 0, want, "max_iters = 0")
        # a start that is converged already: no iteration, x untouched
        xs = PT.pcg(A, b, np.zeros(n), ref.apply, 1e-12, 200)[0]
        want = PT.pcg(A, b, xs, ref.apply, 1e-10, 200)
        assert want[1] == 0 and 0.0 < want[2] <= 1e-10 and np.array_equal(want[0], xs)
        check_run(mg, mg.pcg, b, xs, 1e-10, 200, want, "converged start")
        # b = 0 from x = 0: relres 0, no iteration, nothing NaN
        zero = np.zeros(n)
        mg.set_vec(0, "f", zero)
        want = PT.pcg(A, zero, zero, ref.apply, 1e-10, 50)
        assert want[1] == 0 and want[2] == 0.0 and not want[0].any()
        check_run(mg, mg.pcg, zero, zero, 1e-10, 50, want, "b = 0")
        assert not np.isnan(mg.get_soln(0)).any()
        mg.set_vec(0, "f", b)
        # a second call after plain cycles: the work vectors are reused, x starts where the cycles left u
        mg.set_vec(0, "u", x0)
        mg.vcycle(2)
        x1 = mg.get_soln(0)
        want = PT.pcg(A, b, x1, ref.apply, 1e-10, 200)
        assert want[1] >= 2
        check_run(mg, mg.pcg, b, x1, 1e-10, 200, want, "after vcycle(2)")
    finally:
        mg.close()


# ---- amg_hip_pcg_mixed ------------------------------------------------------------------------------
def level0_matrix(oracle, mg):
    n = mg.get_n_dofs(0)
    colptr, rowind, val = mg.get_coefficient_matrix(0)
    return oracle.CSC(n, n, colptr, rowind, val)


@pytest.mark.parametrize("case", ["t33", "t64"])
def test_pcg_mixed_has_the_twins_bits(amg, oracle, case):
    mg = FB.make(amg, oracle, case)
    try:
        H, _ = FB.hierarchy(mg, case)
        A = level0_matrix(oracle, mg)
        b = mg.get_rhs(0)

        def apply(v):
            return FT.cycle(H, v)[0][0].astype(np.float64)

        x0 = 1e-3 * np.random.default_rng(4).standard_normal(A.rows)
        r0 = PT.first_residual(A, b, x0)
        assert np.array_equal(apply_on_device(mg, r0, f32=True), apply(r0)), (case, "amg_hip_apply_f32")
        check_trajectory(mg, mg.pcg_mixed, A, b, x0, apply, (1, 2, 3), case)
        want = PT.pcg(A, b, np.zeros(A.rows), apply, 1e-8, 200)
        assert 2 <= want[1] < 200 and want[2] <= 1e-8
        check_run(mg, mg.pcg_mixed, b, np.zeros(A.rows), 1e-8, 200, want, (case, "rtol 1e-8"))
        print(f"\n{case}: {want[1]} iterations to relres {want[2]!r}")
    finally:
        mg.close()


def test_pcg_mixed_with_line_smoothers_has_the_twins_krylov_bits(amg, oracle):
    """M^-1 borrowed from the device (see the module's docstring): the Krylov steps around it are the twin's"""
    amg.set_f32_lines(1)
    try:
        mg, _, b = FL._mixed33(amg, oracle)
        try:
            A = level0_matrix(oracle, mg)
            b = np.array(b, np.float64)

            def apply(v):
                return apply_on_device(mg, v, f32=True)

            x0 = 1e-3 * np.random.default_rng(4).standard_normal(A.rows)
            r0 = PT.first_residual(A, b, x0)
            z0 = apply(r0)
            assert np.isfinite(z0).all() and z0.any() and np.array_equal(z0, apply(r0))
            check_trajectory(mg, mg.pcg_mixed, A, b, x0, apply, (1, 2, 3), "mixed33 with lines")
            want = PT.pcg(A, b, np.zeros(A.rows), apply, 1e-8, 200)
            assert 2 <= want[1] < 200 and want[2] <= 1e-8
            check_run(mg, mg.pcg_mixed, b, np.zeros(A.rows), 1e-8, 200, want, "mixed33 with lines, rtol 1e-8")
        finally:
            mg.close()
    finally:
        amg.set_f32_lines(0)


# ---- amg_hip_block_pcg ------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 16])
def test_block_pcg_has_the_twins_bits_in_every_column(amg, oracle, k):
    """the recipe of tests/test_gpu_block.py: a zero column, a column that starts converged, scaled copies
    of b, random right-hand sides, a random start"""
    A, b, ref, mg = _poisson(96, 4)(amg, oracle)
    try:
        n = A.rows
        rtol, cap = 1e-9, 80
        rng = np.random.default_rng(9)
        xs = PT.pcg(A, b, np.zeros(n), ref.apply, 1e-12, 200)[0]
        cols = [np.zeros(n), b, rng.standard_normal(n)] if k == 3 else \
            [np.zeros(n), b, 1e-6 * b, 1e6 * b] + [rng.standard_normal(n) for _ in range(12)]
        B0 = np.stack(cols, 1)
        X0 = np.zeros_like(B0)
        X0[:, 1] = xs
        X0[:, k - 1] = rng.standard_normal(n)
        # attribution: one block cycle from zero on the first residuals is the twin's M^-1 per column
        R0 = np.stack([PT.first_residual(A, B0[:, j], X0[:, j]) for j in range(k)], 1)
        Z = mg.block_vcycles(dev(np.zeros_like(R0)), dev(R0), 1)
        torch.cuda.synchronize()
        Z = Z.cpu().numpy()
        for j in range(k):
            assert np.array_equal(Z[:, j], ref.apply(np.ascontiguousarray(R0[:, j]))), (k, j, "block cycle")
        X, it, rel = mg.block_pcg(dev(B0), dev(X0), rtol=rtol, max_iters=cap)
        torch.cuda.synchronize()
        got = X.cpu().numpy()
        for j in range(k):
            want = PT.pcg(A, B0[:, j], X0[:, j], ref.apply, rtol, cap)
            assert it[j] == want[1], (k, j, it[j], want[1])
            assert np.float64(rel[j]).view(np.uint64) == np.float64(want[2]).view(np.uint64), (k, j, rel[j], want[2])
            assert np.array_equal(got[:, j], want[0]), (k, j)
        assert it[0] == 0 and it[1] == 0 and len(set(it.tolist())) > 1   # the columns stopped at different times
        print(f"\nk = {k}: iterations per column {it.tolist()}")
    finally:
        mg.close()
