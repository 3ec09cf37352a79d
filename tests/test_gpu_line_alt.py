"""Alternating-direction line smoother (AMG_HIP_SM_LINE_ALT) on the device: the stand-alone call and
per-level applications (K-LineX for x, K-Line for y and z) and whole V-cycles against the numpy twin
(tests/line_alt_twin.py), bit-identity across layouts, cycle paths and constructors, convergence on
the split-anisotropy operator against the twin's count and against AMG_HIP_SM_LINE_JACOBI, the
symmetry of the preconditioner, PCG, the byte accounting, and no trace left in later solvers.

The bound of every comparison with the twin comes from the reference side (line_twin.within): with
e64 the 2-norm distance of the twin's float64 result from its longdouble result on the same inputs,
the device must lie within max(8 e64, 1e-14 ||u||) of the longdouble result.  Every test prints the
ratio it found.

K-LineX has three internal periods: the chunk of 64 columns, the 8 runs of one wave, and the
merging of 64 // nx short lines into one run (it changes at nx = 32 | 33, 21 | 22, 16 | 17, ...)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "algebraic-multigrid_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import line_alt_twin as AT  # noqa: E402
import line_twin as T  # noqa: E402

pytestmark = pytest.mark.gpu
SM = 7  # AMG_HIP_SM_LINE_ALT
OMEGA = 0.8


def check(got, ref, e64, scale, what):
    ok, dist, bound, ratio = T.within(got, ref, e64, scale)
    print(f"  {what}: distance {dist:.3e}, e64 {e64:.3e}, ratio {ratio:.2f}, bound {bound:.3e}")
    assert ok, (what, dist, bound, ratio)
    return ratio


def box_stencil(dims, seed):
    """Symmetric, strictly diagonally dominant matrix with random couplings between every pair of
    neighbours in the 3^d box stencil of the grid `dims` (x fastest): on short axes it HAS entries at
    column offsets +-1 across line ends and +-nx across plane ends."""
    rng = np.random.default_rng(seed)
    d3 = tuple(dims) + (1,) * (3 - len(dims))
    nx, ny, nz = d3
    n = nx * ny * nz
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    x, y, z = x.ravel(), y.ravel(), z.ravel()
    rows, cols, vals = [], [], []
    for dz in (0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dz, dy, dx) <= (0, 0, 0):
                    continue
                ok = (x + dx >= 0) & (x + dx < nx) & (y + dy >= 0) & (y + dy < ny) & (z + dz < nz)
                i = np.flatnonzero(ok)
                j = i + dx + nx * dy + nx * ny * dz
                w = -(0.1 + rng.random(i.size)) * (1.0 if (dx != 0) + (dy != 0) + (dz != 0) == 1 else 0.25)
                rows += [i, j]
                cols += [j, i]
                vals += [w, w]
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    A = sp.csc_matrix(A + sp.diags(np.asarray(abs(A).sum(axis=1)).ravel() + 0.05 + 0.1 * rng.random(n)))
    A.sort_indices()
    return A


def standalone(amg, A, dims, what, seed=0, cases=((1, False), (2, False), (1, True), (2, True))):
    rng = np.random.default_rng(seed)
    n = A.shape[0]
    Ar = sp.csr_matrix(A)
    u, f = rng.standard_normal(n), rng.standard_normal(n)
    d3 = tuple(dims) + (1,) * (3 - len(dims))
    worst = 0.0
    for iters, rev in cases:
        got = amg.smooth_line_alt(A.indptr, A.indices, A.data, u, f, dims, omega=OMEGA, iters=iters, reverse=rev)
        ref, e64 = AT.sweep_bound(Ar, u, f, d3, OMEGA, iters, rev)
        worst = max(worst, check(got, ref, e64, np.linalg.norm(got), f"{what} iters {iters} reverse {int(rev)}"))
    return worst


NX = [2, 3, 15, 16, 17, 21, 22, 31, 32, 33, 63, 64, 65, 127, 128, 129]


@pytest.mark.parametrize("nx", NX)
def test_smooth_line_alt_nx(amg, nx):
    """ny = 5: nx below, at and above the chunk of 64 columns and its multiples, and on either side of
    every change of the number of short lines merged into one run."""
    print()
    standalone(amg, box_stencil((nx, 5), nx), (nx, 5), f"{nx} x 5", seed=nx)


@pytest.mark.parametrize("dims", [(7, 1000), (4097, 3), (64, 7), (64, 8), (64, 9), (65, 17), (5, 2, 4), (2, 2, 2),
                                  (9, 1), (1, 9)])
def test_smooth_line_alt_shapes(amg, dims):
    """1000 lines of length 7 (9 to a run, the last run partial, 14 waves); 3 lines of length 4097
    (65 chunks, the last of one column); 7 / 8 / 9 runs of one wave; a 3-D grid with ny = 2, whose
    entries at +-nx across plane ends stay out of T_y; degenerate axes."""
    print()
    standalone(amg, box_stencil(dims, sum(dims)), dims, " x ".join(map(str, dims)), seed=3,
               cases=((1, False), (2, True)))


def test_entries_across_line_ends_stay_out_of_tx(amg):
    """The flat 1-D Laplacian viewed as a 16 x 8 grid HAS entries at +-1 across every line end; with
    them in T_x the x sub-sweep alone would solve the whole system (omega = 1: residual zero)."""
    n = 128
    A = sp.csc_matrix(sp.diags([-np.ones(n - 1), 2.0 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1]))
    A.sort_indices()
    print()
    standalone(amg, A, (16, 8), "flat Laplacian as 16 x 8")
    rng = np.random.default_rng(5)
    f = rng.standard_normal(n)
    u = amg.smooth_line_alt(A.indptr, A.indices, A.data, np.zeros(n), f, (16, 8), omega=1.0, iters=1)
    # lines are decoupled in T: the result differs from the exact solve, and a line's update depends on
    # its own residual only
    assert np.linalg.norm(f - A @ u) > 1e-3 * np.linalg.norm(f)
    f2 = f.copy()
    f2[16:32] += 1.0
    u2 = amg.smooth_line_alt(A.indptr, A.indices, A.data, np.zeros(n), f2, (16, 8), omega=1.0, iters=1)
    # x sub-sweep changes line 1 only; the y sub-sweep (T_y = diagonal here) then spreads through A's +-1
    ref, e64 = AT.sweep_bound(sp.csr_matrix(A), np.zeros(n), f2, (16, 8, 1), 1.0, 1)
    check(u2, ref, e64, np.linalg.norm(u2), "flat Laplacian, shifted line 1")


def diffusion_csr(dims, seed):
    from test_gpu_tensor_dev_setup import diffusion, real_kappa
    return diffusion(dims, real_kappa(seed), 1.0)


def tensor_host(amg, A, b, dims, levels, **kw):
    Ac = sp.csc_matrix(A)
    Ac.sort_indices()
    kw = dict(dict(smoother=SM, smoother_iters=1, omega=OMEGA), **kw)
    return amg.Multigrid.tensor(Ac.indptr.astype(np.int32), Ac.indices.astype(np.int32), Ac.data, b, dims, levels, **kw)


def tensor_dev(amg, A, b, dims, levels, **kw):
    A = sp.csr_matrix(A)
    A.sort_indices()
    kw = dict(dict(smoother=SM, smoother_iters=1, omega=OMEGA), **kw)
    mg = amg.Multigrid.tensor_dev(A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy(), b.copy(),
                                  dims, levels, **kw)
    assert mg.setup_on_device == 1
    return mg


_REF = {}


def problem(name):
    if name not in _REF:
        dims, levels = {"33x20": ((33, 20), 4), "64x64": ((64, 64), 4), "17x12x9": ((17, 12, 9), 3)}[name]
        A = diffusion_csr(dims, 7)
        b = np.random.default_rng(8).standard_normal(A.shape[0])
        _REF[name] = (dims, levels, A, b)
    return _REF[name]


@pytest.mark.parametrize("name", ["33x20", "64x64", "17x12x9"])
@pytest.mark.parametrize("iters", [1, 2])
def test_level_op_equals_twin(amg, name, iters):
    dims, levels, A, b = problem(name)
    mg = tensor_host(amg, A, b, dims, levels, smoother_iters=iters)
    tw = AT.Twin(mg, OMEGA, iters)
    rng = np.random.default_rng(20 + iters)
    print()
    for l in range(mg.n_levels):
        assert mg.line_directions(l) == [s for s, _ in AT.directions(tw.dims[l])]
        n = mg.get_n_dofs(l)
        u, f = rng.standard_normal(n), rng.standard_normal(n)
        mg.set_vec(l, "u", u)
        mg.set_vec(l, "f", f)
        mg.level_op(l, 0)
        mg.sync()
        got = mg.get_soln(l)
        ref, e64 = AT.sweep_bound(tw.A[l], u, f, tw.dims[l], OMEGA, iters)
        check(got, ref, e64, np.linalg.norm(got), f"{name} iters {iters} level {l} grid {tw.dims[l]}")
        assert np.array_equal(mg.get_rhs(l), f)
    mg.close()


@pytest.mark.parametrize("name", ["33x20", "17x12x9"])
def test_vcycles_equal_twin(amg, name):
    dims, levels, A, b = problem(name)
    mg = tensor_host(amg, A, b, dims, levels)
    tw = AT.Twin(mg, OMEGA, 1)
    assert tw.n[-1] <= 256
    u64, uld = np.zeros(b.size), np.zeros(b.size, np.longdouble)
    for _ in range(3):
        u64 = tw.vcycle(u64, b)[0][0]
        uld = tw.vcycle(uld, b, np.longdouble)[0][0]
    e64 = float(np.linalg.norm(u64.astype(np.longdouble) - uld))
    mg.vcycle(3)
    mg.sync()
    got = mg.get_soln(0)
    print()
    check(got, uld, e64, np.linalg.norm(got), f"{name}: level-0 u after 3 V-cycles")
    mg.close()


def _sweep_then_cycles(mg, k=3):
    """one application on every level from seeded vectors, then k V-cycles from u = 0; the states of both"""
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
    st = [(mg.get_soln(l), mg.get_rhs(l)) for l in range(mg.n_levels)]
    mg.close()
    return sweeps, st


def _equal(a, b):
    return (all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and
            all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a[1], b[1])))


@pytest.mark.parametrize("name", ["64x64", "17x12x9"])
def test_layouts_paths_and_constructors_bit_identical(amg, name):
    dims, levels, A, b = problem(name)
    ref = _sweep_then_cycles(tensor_host(amg, A, b, dims, levels))
    assert any(np.any(u != 0) for u in ref[0])
    for lay in (amg.LAYOUT_DICT, amg.LAYOUT_SELL, amg.LAYOUT_CSR):
        assert _equal(_sweep_then_cycles(tensor_host(amg, A, b, dims, levels, layout=lay)), ref), lay
        assert _equal(_sweep_then_cycles(tensor_dev(amg, A, b, dims, levels, layout=lay)), ref), ("dev", lay)
    assert _equal(_sweep_then_cycles(tensor_host(amg, A, b, dims, levels, use_graph=False)), ref)
    assert _equal(_sweep_then_cycles(tensor_dev(amg, A, b, dims, levels, use_graph=False)), ref)
    assert _equal(_sweep_then_cycles(tensor_dev(amg, A, b, dims, levels)), ref)


def test_poisson_tensor_reports_its_path(amg):
    mg = amg.Multigrid.poisson_tensor(64, 4, smoother=SM, omega=OMEGA, smoother_iters=1)
    assert mg.setup_on_device in (0, 1)
    print(f"\npoisson_tensor(64, 4) with AMG_HIP_SM_LINE_ALT: setup_on_device = {mg.setup_on_device}")
    assert mg.line_directions(0) == [1, 64] and mg.line_directions(3) == [1, 8]
    b = mg.get_rhs(0)
    r0 = mg.rss()
    mg.vcycle(3)
    assert mg.rss() < 1e-4 * r0
    assert np.all(np.isfinite(mg.get_soln(0))) and b.size == 4096
    mg.close()


def _device_cycles_to(mg, f, tol=1e-8, max_cycles=60):
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


def test_convergence_split_anisotropy(amg):
    """64 x 48, eps = 1e-3, 4 levels, omega 0.8, through tensor_dev: the device count to 1e-8 equals
    the twin's +- 1 (the twin gave 9); AMG_HIP_SM_LINE_JACOBI omega 0.7 has not reached 1e-8 after 60
    cycles; PCG with the cycle converges in no more iterations than plain cycles."""
    A = AT.split_anisotropy(64, 48, 1e-3)
    f = np.random.default_rng(0).standard_normal(64 * 48)
    mg = tensor_dev(amg, A, f, (64, 48), 4)
    tw = AT.Twin(mg, OMEGA, 1)
    kt, ht = tw.cycles_to(f, 1e-8, 60)
    k, hist = _device_cycles_to(mg, f)
    print(f"\n64 x 48 split anisotropy 1e-3, 4 levels, omega 0.8 to 1e-8: device {k} cycles, twin {kt}; "
          f"history {' '.join(f'{h:.2e}' for h in hist)}")
    assert k is not None and kt is not None and abs(k - kt) <= 1
    mg.set_vec(0, "u", np.zeros(f.size))
    x, it, rel = mg.pcg(1e-8, 100)
    print(f"  PCG to 1e-8: {it} iterations, relres {rel:.2e}")
    assert rel <= 1e-8 and it <= k
    assert np.linalg.norm(f - A @ x) <= 1.01e-8 * np.linalg.norm(f)
    mg.close()
    line = tensor_dev(amg, A, f, (64, 48), 4, smoother=amg.SM_LINE_JACOBI, omega=0.7)
    kl, hl = _device_cycles_to(line, f, 1e-8, 60)
    print(f"  AMG_HIP_SM_LINE_JACOBI omega 0.7: {kl} cycles, ||r|| / ||r0|| after 60: {hl[-1]:.2e}")
    assert kl is None
    line.close()


def test_preconditioner_is_symmetric(amg):
    import torch
    A = AT.split_anisotropy(64, 48, 1e-3)
    n = A.shape[0]
    mg = tensor_dev(amg, A, np.ones(n), (64, 48), 4)
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


def test_must_move_bytes(amg):
    """Per sub-sweep: the residual (matrix + f, u, r = 24 n) and the direction's solve: K-LineX 64 B
    per row (r, dl, ip in, y out; y, cp, u in, u out); K-Line 80 B per interior row and 96 B per
    separator row.  16 x 8, 2 levels, by hand: level 0 has n = 128 and the directions x (stride 1) and
    y (stride 16, 8 positions per chain: no separator), smoothed before and after the coarse solve:
    2 * (2 * (mat + 24 * 128) + 64 * 128 + 80 * 128)."""
    A = diffusion_csr((16, 8), 1)
    b = np.ones(128)
    mg = tensor_host(amg, A, b, (16, 8), 2)
    bare = tensor_host(amg, A, b, (16, 8), 2, smoother_iters=0)
    mat = mg.level_layout(0)[1]
    predicted = 2 * (2 * (mat + 24 * 128) + 64 * 128 + 80 * 128)
    assert mg.cycle_must_move() - bare.cycle_must_move() == pytest.approx(predicted, rel=1e-12)
    with pytest.raises(amg.AmgHipError) as e:
        mg.profile_fine_sweep(3)
    assert e.value.status == amg.EUNSUPPORTED
    mg.close()
    bare.close()


_FRESH = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import amg_ctypes as amg
import test_gpu_line_alt as G
dims, levels, A, b = G.problem("33x20")
for first in (int(sys.argv[3]),):
    if first:
        G.tensor_host(amg, A, b, dims, levels).vcycle(2)
    out = []
    for kw in (dict(smoother=amg.SM_LINE_JACOBI, omega=0.7), dict(smoother=amg.SM_JACOBI, smoother_iters=2, omega=0.8)):
        mg = G.tensor_host(amg, A, b, dims, levels, **kw)
        mg.vcycle(3); mg.sync()
        out.append(mg.get_soln(0))
    np.save(sys.argv[4], np.stack(out))
"""


def test_later_solvers_have_a_fresh_process_bits(amg, tmp_path):
    """A LINE_JACOBI and a JACOBI solver created after a LINE_ALT one give the bits of a process that
    never made one."""
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
