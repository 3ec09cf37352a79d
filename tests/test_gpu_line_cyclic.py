"""Cyclic line solves of the alternating line smoother on periodic axes, on the device
(opts->cyclic_lines, amg_hip_smooth_line_alt_per, K-LineSeam): the stand-alone operation, the level
operation and the V-cycle against the numpy twin (tests/line_cyclic_twin.py), exactness on operators
that are nothing but cyclic lines, the bit identities across replay paths, constructors and layouts,
the PCG counts, the symmetry of the preconditioner and the byte accounting.

The bound of every comparison with the twin is line_twin.within: with e64 the distance of the twin's
float64 result from its longdouble result, the device lies within max(8 e64, 1e-14 ||u||) of the
longdouble result.  Every test prints the figures it found."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "algebraic-multigrid_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import line_cyclic_twin as CT  # noqa: E402
import line_twin as LT  # noqa: E402
import periodic_twin as PT  # noqa: E402

pytestmark = pytest.mark.gpu
SM = 7  # AMG_HIP_SM_LINE_ALT
OMEGA = 0.8
ALT = dict(smoother=SM, smoother_iters=1, omega=OMEGA)


def check(got, ref, e64, scale, what):
    ok, dist, bound, ratio = LT.within(got, ref, e64, scale)
    print(f"  {what}: distance {dist:.3e}, e64 {e64:.3e}, ratio {ratio:.2f}, bound {bound:.3e}")
    assert ok, (what, dist, bound, ratio)
    return ratio


def csc(A):
    Ac = sp.csc_matrix(A)
    Ac.sort_indices()
    return Ac.indptr.astype(np.int32), Ac.indices.astype(np.int32), Ac.data.copy()


def diffusion(dims, per):
    """periodic_twin.diffusion, Dirichlet on both sides of the axes that are not periodic."""
    return PT.diffusion(dims, per, PT.open_sides(len(dims), per))


def standalone(amg, A, dims, per, what, seed=0):
    """iters 1 and 2, reverse 0 and 1 of amg_hip_smooth_line_alt_per against the twin."""
    rng = np.random.default_rng(seed)
    n = A.shape[0]
    u, f = rng.standard_normal(n), rng.standard_normal(n)
    Ac = csc(A)
    for iters in (1, 2):
        for rev in (False, True):
            got = amg.smooth_line_alt(*Ac, u, f, dims, omega=OMEGA, iters=iters, reverse=rev, periodic_axes=per)
            ref, e64 = CT.sweep_bound(A, u, f, dims, per, OMEGA, iters, rev)
            check(got, ref, e64, np.linalg.norm(got), f"{what} per {per} iters {iters} reverse {int(rev)}")


@pytest.mark.parametrize("nx", [3, 4, 21, 22, 32, 33, 63, 64, 65, 129])
def test_x_periodic(amg, nx):
    """ny = 5: line lengths on either side of every lane width 4 .. 64 of the packed form, at and above
    a wave, and more than one pass."""
    print()
    standalone(amg, diffusion((nx, 5), 1), (nx, 5), 1, f"{nx} x 5", seed=nx)


@pytest.mark.parametrize("ny", [3, 4, 64, 65])
def test_y_periodic(amg, ny):
    print()
    standalone(amg, diffusion((5, ny), 2), (5, ny), 2, f"5 x {ny}", seed=ny)


@pytest.mark.parametrize("dims", [(6, 5), (66, 3)])
def test_both_periodic(amg, dims):
    print()
    standalone(amg, diffusion(dims, 3), dims, 3, " x ".join(map(str, dims)), seed=1)


@pytest.mark.parametrize("dims,per", [((6, 5, 4), m) for m in range(1, 8)] + [((4, 3, 66), 4)])
def test_three_dimensions(amg, dims, per):
    print()
    standalone(amg, diffusion(dims, per), dims, per, " x ".join(map(str, dims)), seed=per)


@pytest.mark.parametrize("dims", [(4097, 3), (7, 1000)])
def test_long_and_many_lines(amg, dims):
    """3 lines of 4097 rows (65 columns to a lane, the last pass of one column); 1000 lines of 7 rows
    (8 to a wave, 125 waves, the last workgroup partial)."""
    print()
    standalone(amg, diffusion(dims, 1), dims, 1, " x ".join(map(str, dims)), seed=2)


@pytest.mark.parametrize("dims,per", [((33, 6), 1), ((6, 5, 4), 1), ((6, 5, 4), 6)])
def test_nonsymmetric_operator(amg, dims, per):
    """0.3 times a first-order upwind difference along every periodic axis: alpha != beta, and p comes
    from the factors of T'^T."""
    A = diffusion(dims, per)
    for a in range(len(dims)):
        if (per >> a) & 1:
            A = A + 0.3 * CT.upwind(dims, a, per)
    A = sp.csr_matrix(A)
    assert abs(A - A.T).nnz > 0
    print()
    standalone(amg, A, dims, per, "upwind " + " x ".join(map(str, dims)), seed=4)


def nine_point(nx, ny, seed):
    """Symmetric, diagonally dominant 9-point operator on nx x ny, periodic in x: every point couples to
    its 8 neighbours, x taken modulo nx."""
    rng = np.random.default_rng(seed)
    idx = np.arange(nx * ny).reshape(ny, nx)
    rows, cols, vals = [], [], []
    for dy, dx in ((0, 1), (1, -1), (1, 0), (1, 1)):
        src = idx[:ny - dy, :].ravel()
        dst = np.roll(idx, -dx, axis=1)[dy:, :].ravel()
        w = -(0.1 + rng.random(src.size)) * (1.0 if dx == 0 or dy == 0 else 0.25)
        rows += [src, dst]
        cols += [dst, src]
        vals += [w, w]
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(nx * ny,) * 2).tocsr()
    A = sp.csr_matrix(A + sp.diags(np.asarray(abs(A).sum(axis=1)).ravel() + 0.05))
    A.sort_indices()
    return A


def test_cross_seam_diagonal_neighbours_stay_out_of_tx(amg):
    """9-point operator on 8 x 6, x periodic: row i0 of line y also couples to the LAST rows of the lines
    y - 1 and y + 1 (flat neighbours i0 - 1 and i1 + 8).  Those entries wrap to a different line and
    stay in A only: the device equals the twin, whose T_x holds A[i0, i1] and A[i1, i0] alone, and an
    independent application with the explicitly assembled T_x by sparse LU; a change of f on line 1
    leaves the x sub-sweep of every other line alone."""
    nx, ny = 8, 6
    A = nine_point(nx, ny, 3)
    n = nx * ny
    i0 = np.arange(1, ny) * nx
    assert np.all(A[i0, i0 - 1].A1 != 0) and np.all(A[i0[:-1], i0[:-1] + 2 * nx - 1].A1 != 0)  # across the seam
    print()
    standalone(amg, A, (nx, ny), 1, "9-point 8 x 6")
    rng = np.random.default_rng(5)
    f = rng.standard_normal(n)
    f2 = f.copy()
    f2[nx:2 * nx] += 1.0
    Ac = csc(A)
    Tx = spla.splu(sp.csc_matrix(CT.cyclic_T(A, 1, nx)))
    dl, dd, du = CT.at.tridiagonal_part(A, nx, ny)
    Ty = spla.splu(sp.csc_matrix(sp.diags([dl[nx:], dd, du[:n - nx]], [-nx, 0, nx])))
    for rhs, what in ((f, "f"), (f2, "f shifted on line 1")):
        got = amg.smooth_line_alt(*Ac, np.zeros(n), rhs, (nx, ny), omega=1.0, iters=1, periodic_axes=1)
        ref, e64 = CT.sweep_bound(A, np.zeros(n), rhs, (nx, ny), 1, 1.0, 1)
        check(got, ref, e64, np.linalg.norm(got), f"9-point, {what}")
        ux = Tx.solve(rhs)
        lu = ux + Ty.solve(rhs - A @ ux)
        rel = np.linalg.norm(got - lu) / np.linalg.norm(lu)
        print(f"  against sparse LU with the assembled T_x: {rel:.2e}")
        assert rel <= 1e-12
    # T_x is block diagonal over the lines: the x solve of f2 - f lives on line 1 alone
    d = Tx.solve(f2 - f)
    assert np.all(d[:nx] == 0) and np.all(d[2 * nx:] == 0) and np.all(d[nx:2 * nx] != 0)


@pytest.mark.parametrize("dims", [(64, 4), (5, 3)])
def test_exact_on_decoupled_cyclic_lines(amg, dims):
    """A = the cyclic (-1, 2, -1) operator on every x line plus 0.5 I, nothing across lines: T_x = A, so
    one application with omega = 1 from u = 0 solves the system; the open lines do not."""
    nx, ny = dims
    A = sp.csr_matrix(sp.kron(sp.identity(ny), CT.scaled_diffusion((nx,), (1.0,), 1)) + 0.5 * sp.identity(nx * ny))
    f = np.random.default_rng(7).standard_normal(nx * ny)
    u = amg.smooth_line_alt(*csc(A), np.zeros(f.size), f, dims, omega=1.0, iters=1, periodic_axes=1)
    res = np.linalg.norm(f - A @ u) / np.linalg.norm(f)
    uo = amg.smooth_line_alt(*csc(A), np.zeros(f.size), f, dims, omega=1.0, iters=1, periodic_axes=0)
    reso = np.linalg.norm(f - A @ uo) / np.linalg.norm(f)
    print(f"\n{dims}: ||f - A u|| / ||f|| cyclic {res:.2e}, open {reso:.2e}")
    assert res <= 1e-12
    assert reso > 1e-3
    # periodic_axes = 0 gives amg_hip_smooth_line_alt's bits
    assert np.array_equal(uo, amg.smooth_line_alt(*csc(A), np.zeros(f.size), f, dims, omega=1.0, iters=1))


# (dims, levels, masks, periodic): the cycle cases
C2 = ((64, 48), 4, None, 1)
CODD = ((32, 20), 4, (3, 3, 1), 2)      # y periodic: 20 -> 10 -> 5, then left alone (odd) while x goes on
C3 = ((16, 12, 8), 3, None, 5)          # x and z periodic; z is 2 on the last level
CASES = {"64x48": C2, "32x20": CODD, "16x12x8": C3}
_OPS = {}


def problem(name):
    """(A CSR, b, periodic_twin hierarchy) of a cycle case: built once, never modified."""
    if name not in _OPS:
        dims, nl, masks, per = CASES[name]
        A = diffusion(dims, per)
        b = np.random.default_rng(8).standard_normal(A.shape[0])
        for a in (A.data, A.indices, A.indptr, b):
            a.setflags(write=False)
        _OPS[name] = (A, b, PT.PeriodicTwin(A, dims, nl, masks=masks, periodic=per))
    return _OPS[name]


def host_ctor(amg, name, A=None, b=None, **kw):
    dims, nl, masks, per = CASES[name]
    if A is None:
        A, b, _ = problem(name)
    kw = dict(dict(ALT, cyclic_lines=1), **kw)
    per = kw.pop("periodic_axes", per)
    return amg.Multigrid.tensor_periodic(*csc(A), np.array(b), dims, nl, per, axis_masks=masks, **kw)


def dev_ctor(amg, name, **kw):
    dims, nl, masks, per = CASES[name]
    A, b, _ = problem(name)
    kw = dict(dict(ALT, cyclic_lines=1), **kw)
    return amg.Multigrid.tensor_periodic_dev(A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy(),
                                             np.array(b), dims, nl, per, axis_masks=masks, **kw)


@pytest.mark.parametrize("name", list(CASES))
def test_level_op_and_vcycles_equal_twin(amg, name):
    dims, nl, masks, per = CASES[name]
    A, b, pt = problem(name)
    mg = host_ctor(amg, name)
    tw = CT.Twin(pt, OMEGA, 1)
    assert mg.n_levels == tw.nl
    masks_dev = [mg.line_cyclic(l) for l in range(mg.n_levels)]
    assert masks_dev == [tw.mask(l) for l in range(tw.nl)], masks_dev
    assert masks_dev[0] == per
    rng = np.random.default_rng(21)
    print(f"\n{name}: cyclic masks per level {masks_dev}")
    for l in range(mg.n_levels):
        n = mg.get_n_dofs(l)
        assert tuple(mg.level_dims(l)) == tuple(tw.dims[l])
        Al = LT.csr_of(*mg.get_coefficient_matrix(l), n, n)
        u, f = rng.standard_normal(n), rng.standard_normal(n)
        mg.set_vec(l, "u", u)
        mg.set_vec(l, "f", f)
        mg.level_op(l, 0)
        mg.sync()
        got = mg.get_soln(l)
        ref, e64 = CT.sweep_bound(Al, u, f, tw.dims[l], per, OMEGA, 1)
        check(got, ref, e64, np.linalg.norm(got), f"level {l} grid {tw.dims[l]}")
    mg.set_vec(0, "f", b)
    mg.set_vec(0, "u", np.zeros(b.size))
    assert tw.n[-1] <= 256
    u64, uld = np.zeros(b.size), np.zeros(b.size, np.longdouble)
    for _ in range(3):
        u64 = tw.vcycle(u64, b)[0][0]
        uld = tw.vcycle(uld, b, np.longdouble)[0][0]
    e64 = float(np.linalg.norm(u64.astype(np.longdouble) - uld))
    mg.vcycle(3)
    mg.sync()
    got = mg.get_soln(0)
    check(got, uld, e64, np.linalg.norm(got), "level-0 u after 3 V-cycles")
    mg.close()


def state(mg, k=2):
    """the level vectors after k V-cycles; closes the solver"""
    mg.vcycle(k)
    mg.sync()
    st = [(mg.get_soln(l), mg.get_rhs(l)) for l in range(mg.n_levels)]
    mg.close()
    return st


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0].view(np.uint64), y[0].view(np.uint64)) and
                                    np.array_equal(x[1].view(np.uint64), y[1].view(np.uint64)) for x, y in zip(a, b))


def test_no_periodic_axis_changes_no_bit(amg):
    """cyclic_lines = 1 with periodic_axes = 0 is cyclic_lines = 0."""
    dims, nl, masks, _ = C2
    A = diffusion(dims, 0)
    b = np.random.default_rng(8).standard_normal(A.shape[0])
    on = host_ctor(amg, "64x48", A, b, periodic_axes=0, cyclic_lines=1)
    assert [on.line_cyclic(l) for l in range(on.n_levels)] == [0] * nl
    ref = state(host_ctor(amg, "64x48", A, b, periodic_axes=0, cyclic_lines=0))
    assert any(np.any(u != 0) for u, _ in ref)
    assert same(state(on), ref)


@pytest.mark.parametrize("name", ["64x48", "16x12x8"])
def test_paths_constructors_and_layouts_bit_identical(amg, name):
    ref = state(host_ctor(amg, name))
    assert any(np.any(u != 0) for u, _ in ref)
    open_lines = state(host_ctor(amg, name, cyclic_lines=0))
    assert not same(open_lines, ref)
    assert same(state(host_ctor(amg, name, use_graph=False)), ref), "use_graph 0"
    for lay in (amg.LAYOUT_DICT, amg.LAYOUT_SELL, amg.LAYOUT_CSR):
        assert same(state(host_ctor(amg, name, layout=lay)), ref), lay
    off = dev_ctor(amg, name)
    assert off.setup_on_device == 0
    assert same(state(off), ref), "_periodic_dev, device set-up off"
    amg.set_periodic_device_setup(1)
    try:
        on = dev_ctor(amg, name)
        assert on.setup_on_device == 1, "the device path fell back to the host constructor"
        assert [on.line_cyclic(l) for l in range(on.n_levels)][0] == CASES[name][3]
        assert same(state(on), ref), "_periodic_dev, device set-up on"
        assert same(state(dev_ctor(amg, name, use_graph=False)), ref), "_periodic_dev on, use_graph 0"
    finally:
        amg.set_periodic_device_setup(0)


_FRESH = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import amg_ctypes as amg
import test_gpu_line_cyclic as G
if int(sys.argv[3]):
    G.host_ctor(amg, "32x20").vcycle(2)
out = []
for kw in (dict(cyclic_lines=0), dict(cyclic_lines=0, smoother=amg.SM_JACOBI, smoother_iters=2)):
    mg = G.host_ctor(amg, "32x20", **kw)
    mg.vcycle(3); mg.sync()
    out.append(mg.get_soln(0))
np.save(sys.argv[4], np.stack(out))
"""


def test_later_solvers_have_a_fresh_process_bits(amg, tmp_path):
    """An open-line LINE_ALT and a JACOBI solver created after a cyclic one give the bits of a process
    that never made one."""
    outs = []
    for first in (0, 1):
        path = str(tmp_path / f"u{first}.npy")
        p = subprocess.run([sys.executable, "-c", _FRESH, os.path.join(ROOT, "algebraic-multigrid_amd"),
                            os.path.dirname(os.path.abspath(__file__)), str(first), path],
                           capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        outs.append(np.load(path))
    assert np.all(np.isfinite(outs[0])) and np.any(outs[0] != 0)
    assert np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("dims,nl,eps", [((64, 48), 4, (1.0, 1e-2)), ((64, 48), 4, (1.0, 1e-3)),
                                         ((32, 24, 16), 3, (1.0, 1e-2, 1e-2))])
def test_pcg_counts(amg, dims, nl, eps):
    """Strong coupling along the periodic axis x: the device's PCG count to 1e-8 with cyclic lines is the
    twin's +- 1 and strictly below its own count with open lines."""
    A = CT.scaled_diffusion(dims, eps, 1)
    f = np.random.default_rng(0).standard_normal(A.shape[0])
    tw = CT.Twin(PT.PeriodicTwin(A, dims, nl, periodic=1), OMEGA, 1)
    _, kt, relt = tw.pcg(f, 1e-8)
    its = {}
    for cyc in (1, 0):
        mg = amg.Multigrid.tensor_periodic(*csc(A), f, dims, nl, 1, cyclic_lines=cyc, **ALT)
        x, its[cyc], rel = mg.pcg(1e-8, 200)
        true = np.linalg.norm(f - A @ x) / np.linalg.norm(f)
        print(f"\n{dims} eps {eps} cyclic_lines {cyc}: {its[cyc]} iterations, relres {rel:.2e}, true {true:.2e}"
              + (f"; twin {kt} ({relt:.2e})" if cyc else ""))
        assert true <= 1.01e-8
        mg.close()
    assert abs(its[1] - kt) <= 1
    assert its[1] < its[0]


def test_preconditioner_is_symmetric(amg):
    import torch
    dims, nl = (64, 48), 4
    A = CT.scaled_diffusion(dims, (1.0, 1e-2), 1)
    n = A.shape[0]
    mg = amg.Multigrid.tensor_periodic(*csc(A), np.ones(n), dims, nl, 1, cyclic_lines=1, **ALT)
    assert mg.line_cyclic(0) == 1
    rng = np.random.default_rng(3)
    v, w = torch.from_numpy(rng.standard_normal(n)).cuda(), torch.from_numpy(rng.standard_normal(n)).cuda()
    mv, mw = torch.empty_like(v), torch.empty_like(w)
    mg.apply_dev(v.data_ptr(), mv.data_ptr())
    mg.apply_dev(w.data_ptr(), mw.data_ptr())
    mg.sync()
    lhs, rhs = float(mv @ w), float(v @ mw)
    bound = 1e-10 * float(v.norm()) * float(mw.norm())
    print(f"\n<M^-1 v, w> - <v, M^-1 w> = {lhs - rhs:.3e}, bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound
    mg.close()


def test_bytes(amg):
    """16 x 8, 2 levels, x periodic, by hand.  Level 0 (n = 128, 8 lines of 16) is smoothed before and
    after the coarse solve, x cyclic and y open; per sub-sweep the residual (matrix + f, u, r = 24 n) and
    the solve (K-LineX 64 n, K-Line 80 n: 8 positions per chain, no separator); K-LineSeam adds p and r
    in (16 n) and den, gamma, beta in and two entries of r out per line (40 B):
    must move = 2 (2 (mat + 24 n) + 64 n + 80 n + 16 n + 40 * 8).
    amg_hip_cycle_bytes counts the pre-smoother of the coarsest level (8 x 4: n = 32, 4 lines of 8) too:
    against open lines it grows by 2 (16 * 128 + 40 * 8) + (16 * 32 + 40 * 4)."""
    dims = (16, 8)
    A = diffusion(dims, 1)
    b = np.ones(128)
    mk = lambda **kw: amg.Multigrid.tensor_periodic(*csc(A), b, dims, 2, 1, **dict(ALT, **kw))  # noqa: E731
    cyc, opn, bare = mk(cyclic_lines=1), mk(cyclic_lines=0), mk(cyclic_lines=1, smoother_iters=0)
    assert [cyc.line_cyclic(l) for l in range(2)] == [1, 1]
    mat = cyc.level_layout(0)[1]
    seam = 16 * 128 + 40 * 8
    predicted = 2 * (2 * (mat + 24 * 128) + 64 * 128 + 80 * 128 + seam)
    moved = cyc.cycle_must_move() - bare.cycle_must_move()
    print(f"\nmust move: {moved:.0f}, by hand {predicted}; open {opn.cycle_must_move() - bare.cycle_must_move():.0f}")
    assert moved == pytest.approx(predicted, rel=1e-12)
    assert cyc.cycle_must_move() - opn.cycle_must_move() == pytest.approx(2 * seam, rel=1e-12)
    assert cyc.cycle_bytes()[0] - opn.cycle_bytes()[0] == pytest.approx(2 * seam + 16 * 32 + 40 * 4, rel=1e-12)
    for mg in (cyc, opn, bare):
        mg.close()
