"""Cyclic line solves of the alternating line smoother on periodic axes (opts->cyclic_lines,
amg_hip_line_cyclic, amg_hip_smooth_line_alt_per), the parts that need no GPU: the twin
(tests/line_cyclic_twin.py) against a direct solve with the explicitly assembled cyclic T_a, the
refusals of the option and of the stand-alone call, the getter on host_only hierarchies, and the
iteration counts that motivate the option, recomputed by the twin."""
import os
import sys

import numpy as np
import pytest

sp = pytest.importorskip("scipy.sparse")
spla = pytest.importorskip("scipy.sparse.linalg")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import line_cyclic_twin as CT  # noqa: E402
import periodic_twin as PT  # noqa: E402

SM_ALT, SM_LINE, SM_JACOBI = 7, 6, 3
ALT = dict(smoother=SM_ALT, smoother_iters=1, omega=0.8)


def csc(A):
    Ac = sp.csc_matrix(A)
    Ac.sort_indices()
    return Ac.indptr.astype(np.int32), Ac.indices.astype(np.int32), Ac.data.copy()


def operator(dims, per, nonsym):
    dirichlet = PT.open_sides(len(dims), per)
    A = PT.diffusion(dims, per, dirichlet)
    if nonsym:
        for a in range(len(dims)):
            if (per >> a) & 1:
                A = A + 0.3 * CT.upwind(dims, a, per)
    return sp.csr_matrix(A)


# every length m of the issue on a periodic axis, in 2-D and 3-D
LU_CASES = [((3, 4), 1), ((4, 3), 1), ((7, 5), 1), ((64, 3), 1), ((5, 3), 2), ((5, 4), 2), ((4, 7), 2), ((3, 64), 2),
            ((7, 4), 3), ((3, 4, 7), 1), ((4, 3, 5), 2), ((5, 3, 7), 4), ((4, 7, 3), 7), ((64, 3, 4), 5)]


@pytest.mark.parametrize("nonsym", [False, True])
@pytest.mark.parametrize("dims,per", LU_CASES)
def test_twin_subsweep_is_the_cyclic_solve(dims, per, nonsym):
    """One application of the longdouble twin against the same sub-sweeps with T_a assembled explicitly
    (wrap entries included) and solved by sparse LU: 1e-12 relative."""
    A = operator(dims, per, nonsym)
    assert (abs(A - A.T).nnz > 0) == nonsym
    n = A.shape[0]
    rng = np.random.default_rng(5)
    u0, f = rng.standard_normal(n), rng.standard_normal(n)
    for reverse in (False, True):
        got = CT.apply(A, u0, f, dims, per, 0.8, 1, reverse, np.longdouble)
        dirs = CT.directions(dims, per)
        u = u0.copy()
        for s, m, cyc in (dirs[::-1] if reverse else dirs):
            Ta = CT.cyclic_T(A, s, m) if cyc else None
            if cyc:
                i0, i1, alpha, beta, _ = CT.wrap_entries(A, s, m)
                assert np.all(alpha != 0) and np.all(beta != 0)
                assert np.array_equal(Ta[i0, i1].A1, A[i0, i1].A1) and np.array_equal(Ta[i1, i0].A1, A[i1, i0].A1)
            else:
                dl, dd, du = CT.at.tridiagonal_part(A, s, m)
                Ta = sp.diags([dl[s:], dd, du[:n - s]], [-s, 0, s], format="csr")
            u = u + 0.8 * spla.splu(sp.csc_matrix(Ta)).solve(f - A @ u)
        rel = float(np.linalg.norm(got.astype(np.float64) - u) / np.linalg.norm(u))
        print(f"{dims} per {per} nonsym {nonsym} reverse {reverse}: rel {rel:.2e}")
        assert rel <= 1e-12


def test_twin_with_no_periodic_axis_is_the_open_twin():
    A = operator((7, 5), 0, False)
    rng = np.random.default_rng(1)
    u, f = rng.standard_normal(35), rng.standard_normal(35)
    assert np.array_equal(CT.apply(A, u, f, (7, 5), 0, 0.8, 2), CT.at.apply(A, u, f, (7, 5), 0.8, 2))
    # a periodic axis of 2 points: the wrap edge is the ordinary edge, nothing is cyclic
    assert CT.cyclic_mask((2, 5), 1) == 0 and CT.cyclic_mask((3, 2, 4), 7) == 5


def periodic_host(amg, dims, levels, per, masks=None, **kw):
    A = PT.diffusion(dims, per, PT.open_sides(len(dims), per))
    b = np.ones(A.shape[0])
    return amg.Multigrid.tensor_periodic(*csc(A), b, dims, levels, per, axis_masks=masks, host_only=True, **kw)


def test_symbols_and_header(amg):
    L = amg.lib()
    assert hasattr(L, "amg_hip_line_cyclic") and hasattr(L, "amg_hip_smooth_line_alt_per")
    with open(os.path.join(os.path.dirname(__file__), "..", "include", "amg_hip.h")) as h:
        text = h.read()
    assert "int32_t cyclic_lines;" in text and "NO CYCLIC TRIDIAGONAL SOLVE" not in text
    # the field takes the alignment padding in front of `stream`, in the header and in the binding: no
    # other field moves, the size stays, natural_sides and singular stay the last two fields
    import ctypes as C
    import re
    body = re.sub(r"/\*.*?\*/", "", text[:text.index("} amg_hip_options;")], flags=re.S)
    names = re.findall(r"(\w+);", body[body.rindex("typedef struct"):])
    assert names == [f[0] for f in amg.Options._fields_]
    assert names[names.index("cyclic_lines") - 1:names.index("cyclic_lines") + 2] == ["exact_gs", "cyclic_lines", "stream"]
    O = amg.Options
    assert (O.exact_gs.offset, O.cyclic_lines.offset, O.stream.offset) == (64, 68, 72)
    assert (O.natural_sides.offset, O.singular.offset, C.sizeof(O)) == (104, 108, 112)
    o = O()
    o.cyclic_lines = 1
    amg.lib().amg_hip_default_options(C.byref(o))
    assert o.cyclic_lines == 0


def test_option_errors_arrive_before_the_device(amg):
    """No host_only here: the refusals must not need a device."""
    dims, per = (8, 6), 1
    A = PT.diffusion(dims, per, PT.open_sides(2, per))
    b = np.ones(48)
    for bad in (2, -1):
        with pytest.raises(ValueError, match="cyclic_lines"):
            amg.Multigrid.tensor_periodic(*csc(A), b, dims, 2, per, cyclic_lines=bad, **ALT)
    for sm in (SM_LINE, SM_JACOBI, 0):
        with pytest.raises(ValueError, match="cyclic_lines.*AMG_HIP_SM_LINE_ALT"):
            amg.Multigrid.tensor_periodic(*csc(A), b, dims, 2, per, cyclic_lines=1, smoother=sm, omega=0.8)
    with pytest.raises(ValueError, match="cyclic_lines"):
        amg.Multigrid.tensor_periodic_dev(A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data, b, dims, 2,
                                          per, cyclic_lines=1, smoother=SM_LINE, omega=0.8)
    # the other constructors know no periodic axes
    D = PT.diffusion(dims, 0, PT.open_sides(2, 0))
    with pytest.raises(ValueError, match="cyclic_lines"):
        amg.Multigrid.tensor(*csc(D), b, dims, 2, cyclic_lines=1, **ALT)
    with pytest.raises(ValueError, match="cyclic_lines"):
        amg.Multigrid.tensor_semi(*csc(D), b, dims, 2, axis_masks=[3], cyclic_lines=1, **ALT)
    with pytest.raises(ValueError, match="cyclic_lines"):
        amg.Multigrid.tensor_dev(D.indptr.astype(np.int32), D.indices.astype(np.int32), D.data, b, dims, 2,
                                 cyclic_lines=1, **ALT)


def test_cyclic_lines_with_no_periodic_axis_is_accepted(amg):
    mg = periodic_host(amg, (8, 6), 2, 0, cyclic_lines=1, **ALT)
    assert [mg.line_cyclic(l) for l in range(2)] == [0, 0]
    mg.close()


@pytest.mark.parametrize("dims,levels,per,masks,want", [
    ((8, 6), 3, 1, None, [1, 1, 0]),            # x: 8 -> 4 -> 2: the last level has the wrap edge in T_x already
    ((8, 6), 3, 2, [1, 1], [2, 2, 2]),          # y periodic, never coarsened: 6 on every level
    ((32, 20), 4, 3, [3, 3, 1], [3, 3, 3, 3]),  # y stays 5 (odd) from level 2 on
    ((8, 4, 6), 2, 7, None, [7, 5]),            # y: 4 -> 2
    ((16, 12, 8), 3, 5, None, [5, 5, 1]),       # z: 8 -> 4 -> 2
])
def test_line_cyclic_on_host_only_solvers(amg, dims, levels, per, masks, want):
    mg = periodic_host(amg, dims, levels, per, masks, cyclic_lines=1, **ALT)
    got = [mg.line_cyclic(l) for l in range(mg.n_levels)]
    twin = [CT.cyclic_mask(mg.level_dims(l), per) for l in range(mg.n_levels)]
    assert got == want == twin, (got, twin)
    with pytest.raises(ValueError, match="level out of range"):
        mg.line_cyclic(mg.n_levels)
    mg.close()
    mg = periodic_host(amg, dims, levels, per, masks, cyclic_lines=0, **ALT)
    assert [mg.line_cyclic(l) for l in range(mg.n_levels)] == [0] * len(want)
    mg.close()


def test_line_cyclic_needs_the_smoother(amg):
    mg = periodic_host(amg, (8, 6), 2, 1, smoother=SM_JACOBI, omega=0.8)
    with pytest.raises(ValueError, match="amg_hip_line_cyclic.*AMG_HIP_SM_LINE_ALT"):
        mg.line_cyclic(0)
    mg.close()


def test_host_setup_refuses_a_bad_pivot_and_a_bad_denominator(amg):
    """T' has the pivot 2 d(i0) on the first row of a line: a zero diagonal there is named with level,
    direction and row.  A line operator with zero row sums and nothing off the line is singular; with
    exact arithmetic (powers of two) its denominator is exactly zero and is named too."""
    dims, per = (4, 3), 1
    A = sp.lil_matrix(CT.scaled_diffusion(dims, (1.0, 1.0), per))
    A[4, 4] = 0.0
    b = np.ones(12)
    with pytest.raises(ValueError, match=r"level 0 direction x row 4 .*pivot"):
        amg.Multigrid.tensor_periodic(*csc(sp.csr_matrix(A)), b, dims, 1, per, host_only=True, cyclic_lines=1, **ALT)
    # edges 0-1, 1-2 of weight 0.5 and the wrap edge 2-0 of weight 1 on every x line of a 3 x 4 grid
    M = np.array([[1.5, -0.5, -1.0], [-0.5, 1.0, -0.5], [-1.0, -0.5, 1.5]])
    S = sp.csr_matrix(sp.kron(sp.identity(4), M))
    with pytest.raises(ZeroDivisionError):
        CT.setup(S, 1, 3, np.float64)
    with pytest.raises(ValueError, match=r"level 0 direction x row 0 .*denominator"):
        amg.Multigrid.tensor_periodic(*csc(S), b, (3, 4), 1, per, host_only=True, cyclic_lines=1, **ALT)
    with pytest.raises(ValueError, match=r"direction x row 0 .*denominator"):
        amg.smooth_line_alt(*csc(S), np.zeros(12), b, (3, 4), periodic_axes=1)


def test_stand_alone_argument_errors(amg):
    dims = (6, 5)
    A = PT.diffusion(dims, 1, PT.open_sides(2, 1))
    u, f = np.zeros(30), np.ones(30)
    for bad in (-1, 4, 7):
        with pytest.raises(ValueError, match="amg_hip_smooth_line_alt_per: `periodic_axes`"):
            amg.smooth_line_alt(*csc(A), u, f, dims, periodic_axes=bad)
    with pytest.raises(ValueError, match="amg_hip_smooth_line_alt_per: `n` = 30"):
        amg.smooth_line_alt(*csc(A), u, f, (6, 4), periodic_axes=1)
    with pytest.raises(ValueError, match="omega"):
        amg.smooth_line_alt(*csc(A), u, f, dims, omega=2.0, periodic_axes=1)
    with pytest.raises(ValueError, match="iters"):
        amg.smooth_line_alt(*csc(A), u, f, dims, iters=-1, periodic_axes=1)


def test_counts_of_the_motivating_case():
    """64 x 48, 4 levels, x periodic, eps (1, 1e-2), LINE_ALT omega 0.8 1 + 1, random f, to 1e-8: the
    open lines need about 50 V-cycles / 16 PCG iterations, the cyclic ones about 16 / 9."""
    dims = (64, 48)
    A = CT.scaled_diffusion(dims, (1.0, 1e-2), 1)
    f = np.random.default_rng(0).standard_normal(A.shape[0])
    pt = PT.PeriodicTwin(A, dims, 4, periodic=1)
    counts = {}
    for cyclic in (False, True):
        tw = CT.Twin(pt, 0.8, 1, cyclic)
        cycles, _ = tw.cycles_to(f, 1e-8, 80)
        _, its, rel = tw.pcg(f, 1e-8)
        assert rel <= 1e-8
        counts[cyclic] = (cycles, its)
    print("V-cycles open -> cyclic:", counts[False][0], "->", counts[True][0], " PCG:", counts[False][1], "->",
          counts[True][1])
    assert counts[True][0] is not None and counts[False][0] is not None
    assert counts[True][0] <= counts[False][0] - 4
    assert counts[True][1] <= counts[False][1] - 4
