"""Mean projection of the PCG drivers (amg_hip_set_mean_projection; K-Center) bit for bit against
tests/pcg_project_twin.py, by the method of tests/test_gpu_pcg_bitwise.py: the device's iterate after
max_iters = 1, 2, 3 (rtol = 0) and the run to rtol = 1e-8 equal the twin's x (np.array_equal), iteration count
and relres bits.  M^-1 is BORROWED from the device through amg_hip_apply / amg_hip_apply_f32, which the switch
does not touch, as that file does for the line smoothers: the dot products, the centring, the updates, alpha,
beta and the stopping rule are the twin's own, so a difference points at K-Center and the driver, not at the
cycle.  The attribution check says that the borrowed cycle gives the same bits twice.

  single   pure-Neumann variable-coefficient diffusion (natural_twin.diffusion, all sides natural, singular,
           true Jacobi omega 0.8 2+2, built on the device) on 33 x 20 / 3 levels (660 rows: three workgroups and
           a ragged tail), 64 x 48 / 4 (3072 rows: twelve full workgroups) and 17 x 12 x 9 / 3; the fully periodic
           `per` operator of tests/dict_cases.py; 513 x 513 / 6 (263169 rows > 1024 * 256: the first stage of
           the sums takes a second grid-stride pass with a tail), max_iters <= 2.  Each with b and b + 1e-6,
           from x0 = 1e-3 standard_normal.
  mixed    amg_hip_pcg_mixed on 33 x 20 with layout = SELL
  block    amg_hip_block_pcg, k = 3: columns b, b + 1e-3 and zeros, every column against the single-vector twin;
           k = 1, 2, 8, 16 (the other panel widths of the block kernels), two iterations
  edges    max_iters = 0 and a converged start return centre(x0); b = 0 gives relres 0 and no NaN
  off      with the switch off the singular solver's trajectory has pcg_twin.pcg's bits
  centre   amg_hip_center_vec has the twin's bits on levels 0 and 1
After every run with the switch on get_rhs(0) is the caller's b bit for bit (check_run asserts it)."""
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

import dict_cases as DC  # noqa: E402
import pcg_project_twin as PP  # noqa: E402
import pcg_twin as PT  # noqa: E402
import test_gpu_pcg_bitwise as PB  # noqa: E402
import test_gpu_tensor_natural as TN  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL, CAP = 1e-8, 60
SINGLE = {"33x20": ((33, 20), 3, (1, 2, 3)), "64x48": ((64, 48), 4, (1, 2, 3)), "17x12x9": ((17, 12, 9), 3, (1, 2, 3)),
          "per": (None, 4, (1, 2, 3)), "513x513": ((513, 513), 6, (1, 2))}


def make(amg, oracle, name, host=False, **kw):
    """(solver, b) of a single-vector case"""
    dims, nl, _ = SINGLE[name]
    if name == "per":
        return DC.make(amg, oracle, "per", **kw), np.array(DC.operator("per")[1])
    ctor = TN.host_ctor if host else TN.dev_ctor
    mg = ctor(amg, dims, nl, 0, natural_sides=TN.N.all_sides(len(dims)), singular=True, **kw)
    return mg, np.array(TN.op(dims)[2])


def start(n):
    return 1e-3 * np.random.default_rng(4).standard_normal(n)


def borrowed(mg, f32=False):
    def apply(v):
        return PB.apply_on_device(mg, v, f32=f32)
    return apply


def check_attribution(mg, A, b, x0, apply, what):
    r0 = PT.first_residual(A, PP.centre(b), x0)
    z0 = apply(r0)
    assert np.isfinite(z0).all() and z0.any() and np.array_equal(z0, apply(r0)), what


def check_trajectory(mg, run, A, b, x0, apply, steps, what, project=True):
    top = max(steps)
    _, it, _, trace = PP.pcg(A, b, x0, apply, 0.0, top, project=project, keep_iterates=True)
    assert it == top and len(trace) == top
    assert all(np.isfinite(t[0]) and np.isfinite(t[2]) for t in trace)
    assert not np.array_equal(trace[0][3], x0)
    for k in steps:
        PB.check_run(mg, run, b, x0, 0.0, k, (trace[k - 1][3], k, trace[k - 1][2]), (what, "max_iters", k))
    print(f"\n{what}: n = {A.rows}, iterates 1 .. {top} bit for bit; relres " + " ".join(f"{t[2]:.3e}" for t in trace))


def check_to_tolerance(mg, run, A, b, x0, apply, what):
    want = PP.pcg(A, b, x0, apply, RTOL, CAP, project=True)
    assert 2 <= want[1] < CAP and want[2] <= RTOL, (what, want[1], want[2])
    PB.check_run(mg, run, b, x0, RTOL, CAP, want, (what, "rtol 1e-8"))
    print(f"{what}: {want[1]} iterations to relres {want[2]!r}")


@pytest.mark.parametrize("shift", [0.0, 1e-6], ids=["b", "b+1e-6"])
@pytest.mark.parametrize("name", sorted(SINGLE))
def test_projected_pcg_has_the_twins_bits(amg, oracle, name, shift):
    mg, b = make(amg, oracle, name)
    try:
        assert mg.mean_projection == 0
        mg.set_mean_projection(1)
        assert mg.mean_projection == 1
        A = PB.level0_matrix(oracle, mg)
        b = b + shift
        mg.set_vec(0, "f", b)
        x0 = start(A.rows)
        apply = borrowed(mg)
        check_attribution(mg, A, b, x0, apply, name)
        check_trajectory(mg, mg.pcg, A, b, x0, apply, SINGLE[name][2], (name, shift))
        if name != "513x513":
            check_to_tolerance(mg, mg.pcg, A, b, x0, apply, (name, shift))
    finally:
        mg.close()


def test_projected_pcg_mixed_has_the_twins_bits(amg, oracle):
    mg, b = make(amg, oracle, "33x20", host=True, layout=amg.LAYOUT_SELL)
    try:
        mg.set_mean_projection(1)
        A = PB.level0_matrix(oracle, mg)
        x0 = start(A.rows)
        apply = borrowed(mg, f32=True)
        for shift in (0.0, 1e-6):
            bs = b + shift
            mg.set_vec(0, "f", bs)
            check_attribution(mg, A, bs, x0, apply, ("mixed", shift))
            check_trajectory(mg, mg.pcg_mixed, A, bs, x0, apply, (1, 2, 3), ("mixed 33x20", shift))
            check_to_tolerance(mg, mg.pcg_mixed, A, bs, x0, apply, ("mixed 33x20", shift))
    finally:
        mg.close()


def test_projected_block_pcg_has_the_twins_bits_in_every_column(amg, oracle):
    mg, b = make(amg, oracle, "33x20")
    try:
        mg.set_mean_projection(1)
        A = PB.level0_matrix(oracle, mg)
        n = A.rows
        apply = borrowed(mg)
        B0 = np.stack([b, b + 1e-3, np.zeros(n)], 1)
        X0 = np.zeros_like(B0)
        X0[:, 0] = start(n)
        dB = PB.dev(B0)
        X, it, rel = mg.block_pcg(dB, PB.dev(X0), rtol=RTOL, max_iters=CAP)
        torch.cuda.synchronize()
        got = X.cpu().numpy()
        assert np.array_equal(dB.cpu().numpy(), B0)          # B is not written
        for j in range(3):
            want = PP.pcg(A, np.ascontiguousarray(B0[:, j]), np.ascontiguousarray(X0[:, j]), apply, RTOL, CAP, project=True)
            assert it[j] == want[1], (j, it[j], want[1])
            assert np.float64(rel[j]).view(np.uint64) == np.float64(want[2]).view(np.uint64), (j, rel[j], want[2])
            assert np.array_equal(got[:, j], want[0]), j
        assert it[2] == 0 and rel[2] == 0.0 and not got[:, 2].any()
        assert 2 <= it[0] < CAP and 2 <= it[1] < CAP and max(rel) <= RTOL
        print(f"\nblock k = 3, rtol 1e-8: iterations per column {[int(i) for i in it]}")
        # a short run: columns stopped by the cap, the centring of the last iterate in every column
        X, it, rel = mg.block_pcg(dB, PB.dev(X0), rtol=0.0, max_iters=2)
        torch.cuda.synchronize()
        got = X.cpu().numpy()
        for j in range(2):
            want = PP.pcg(A, np.ascontiguousarray(B0[:, j]), np.ascontiguousarray(X0[:, j]), apply, 0.0, 2, project=True)
            assert it[j] == 2 and np.array_equal(got[:, j], want[0]), j
            assert np.float64(rel[j]).view(np.uint64) == np.float64(want[2]).view(np.uint64), j
    finally:
        mg.close()


@pytest.mark.parametrize("k", [1, 2, 8, 16])
def test_projected_block_pcg_at_every_panel_width(amg, oracle, k):
    """the other instantiations of the block K-Center kernels (kp = 1, 2, 8, 16): two iterations, column j with
    b + j 1e-3 from a start of its own"""
    mg, b = make(amg, oracle, "33x20")
    try:
        mg.set_mean_projection(1)
        A = PB.level0_matrix(oracle, mg)
        n = A.rows
        apply = borrowed(mg)
        B0 = np.stack([b + 1e-3 * j for j in range(k)], 1)
        X0 = 1e-3 * np.random.default_rng(5).standard_normal((n, k)) + 0.25
        X, it, rel = mg.block_pcg(PB.dev(B0), PB.dev(X0), rtol=0.0, max_iters=2)
        torch.cuda.synchronize()
        got = X.cpu().numpy()
        for j in range(k):
            want = PP.pcg(A, np.ascontiguousarray(B0[:, j]), np.ascontiguousarray(X0[:, j]), apply, 0.0, 2, project=True)
            assert it[j] == 2 and want[1] == 2, (k, j, it[j])
            assert np.float64(rel[j]).view(np.uint64) == np.float64(want[2]).view(np.uint64), (k, j, rel[j], want[2])
            assert np.array_equal(got[:, j], want[0]), (k, j)
    finally:
        mg.close()


def test_projected_edge_cases_have_the_twins_bits(amg, oracle):
    mg, b = make(amg, oracle, "33x20")
    try:
        mg.set_mean_projection(1)
        A = PB.level0_matrix(oracle, mg)
        n = A.rows
        apply = borrowed(mg)
        x0 = 1.0 + start(n)                                 # a start with a mean worth removing
        # no iteration allowed: centre(x0)
        want = PP.pcg(A, b, x0, apply, RTOL, 0, project=True)
        assert want[1] == 0 and np.array_equal(want[0], PP.centre(x0)) and not np.array_equal(want[0], x0)
        PB.check_run(mg, mg.pcg, b, x0, RTOL, 0, want, "max_iters = 0")
        # a start that is converged already, shifted by a constant: no iteration, centre(x0)
        xs = PP.pcg(A, b, np.zeros(n), apply, 1e-12, 200, project=True)[0] + 0.5
        want = PP.pcg(A, b, xs, apply, RTOL, CAP, project=True)
        assert want[1] == 0 and 0.0 < want[2] <= RTOL and np.array_equal(want[0], PP.centre(xs))
        PB.check_run(mg, mg.pcg, b, xs, RTOL, CAP, want, "converged start")
        # b = 0 from x = 0: relres 0, no iteration, nothing NaN
        zero = np.zeros(n)
        mg.set_vec(0, "f", zero)
        want = PP.pcg(A, zero, zero, apply, RTOL, 50, project=True)
        assert want[1] == 0 and want[2] == 0.0 and not want[0].any()
        PB.check_run(mg, mg.pcg, zero, zero, RTOL, 50, want, "b = 0")
        assert not np.isnan(mg.get_soln(0)).any()
    finally:
        mg.close()


def test_switch_off_keeps_the_unprojected_bits(amg, oracle):
    mg, b = make(amg, oracle, "33x20")
    try:
        A = PB.level0_matrix(oracle, mg)
        x0 = start(A.rows)
        apply = borrowed(mg)

        def off():
            _, it, _, trace = PT.pcg(A, b, x0, apply, 0.0, 3, keep_iterates=True)
            assert it == 3
            for k in (1, 2, 3):
                PB.check_run(mg, mg.pcg, b, x0, 0.0, k, (trace[k - 1][3], k, trace[k - 1][2]), ("off", k))
        off()                                               # never switched on
        mg.set_mean_projection(1)
        check_trajectory(mg, mg.pcg, A, b, x0, apply, (1,), "on")
        mg.set_mean_projection(0)
        assert mg.mean_projection == 0
        off()                                               # switched on and off again
    finally:
        mg.close()


def test_center_vec_has_the_twins_bits(amg, oracle):
    mg, b = make(amg, oracle, "33x20")
    try:
        rng = np.random.default_rng(12)
        for level in (0, 1):
            n = mg.get_n_dofs(level)
            for which, get in (("u", mg.get_soln), ("f", mg.get_rhs)):
                other, get_other = ("f", mg.get_rhs) if which == "u" else ("u", mg.get_soln)
                v = 3.0 + rng.standard_normal(n)
                w = rng.standard_normal(n)
                mg.set_vec(level, which, v)
                mg.set_vec(level, other, w)
                mg.center_vec(level, which)
                mg.sync()
                got = get(level)
                assert np.array_equal(got, PP.centre(v)), (level, which)
                assert not np.array_equal(got, v)
                assert np.array_equal(get_other(level), w), (level, which, "the other vector")
        assert mg.mean_projection == 0                      # amg_hip_center_vec does not need the switch
    finally:
        mg.close()
