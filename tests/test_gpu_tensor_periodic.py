"""Periodic axes of the tensor hierarchies on the device (amg_hip_create_tensor_periodic): the
matrix-free transfer kernels with the seam against the CSR SpMV with the R / P of the getter (bitwise),
the cycle across transfer and replay paths (bitwise), one V-cycle and the PCG counts against the scipy
twin (tests/periodic_twin.py), the float, block, Chebyshev, line and multicolour forms on a fully
periodic singular operator, and the _dev constructor against the host constructor (bitwise).

The bound of the comparison with the twin's cycle is tests/test_gpu_tensor.py's: with e64 the distance
of the twin's float64 cycle from its longdouble cycle, the device lies within max(8 e64, 1e-14 ||u||)
of the longdouble cycle (tensor_twin.within).  The PCG counts are held to the twin's, run in the test,
within one iteration.  Every test prints the figures it found."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "algebraic-multigrid_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import natural_twin as N  # noqa: E402
import periodic_twin as PT  # noqa: E402
import semi_twin as S  # noqa: E402
import tensor_twin as T  # noqa: E402

pytestmark = pytest.mark.gpu

JAC = dict(smoother=3, smoother_iters=2, omega=0.8)

# (dims, levels, masks, periodic axes, natural sides): the three cycle cases.  The sides that are neither
# periodic nor natural are Dirichlet.
XY = ((64, 48), 5, None, 3, 0)        # doubly periodic, singular
X_DIR = ((32, 21), 4, None, 1, 0)     # periodic in x, Dirichlet in y; 21 -> 10 -> 5 -> 2 along y
XYZ = ((16, 12, 8), 3, None, 7, 0)    # triply periodic, singular
CYCLE_CASES = (XY, X_DIR, XYZ)
# (32, 20) with 4 levels, fully periodic: y is 5 on level 2 and cannot be coarsened there as a periodic
# axis, so level 2 coarsens x alone (explicit masks)
FORMS = ((32, 20), 4, (3, 3, 1), 3, 0)

_OPS = {}


def op(dims, per, sides=0):
    """(A as CSR, A as CSC, b, singular) of periodic_twin.diffusion / rhs: built once, never modified."""
    key = (tuple(dims), per, sides)
    if key not in _OPS:
        dirichlet = PT.open_sides(len(dims), per) & ~sides
        A = PT.diffusion(dims, per, dirichlet)
        Ac = sp.csc_matrix(A)
        Ac.sort_indices()
        b = PT.rhs(A.shape[0], dirichlet == 0)
        for a in (A.data, A.indices, A.indptr, Ac.data, b):
            a.setflags(write=False)
        _OPS[key] = (A, Ac, b, dirichlet == 0)
    return _OPS[key]


_TWINS = {}


def twin(dims, nl, masks, per, sides):
    key = (tuple(dims), nl, masks, per, sides)
    if key not in _TWINS:
        A, _, _, singular = op(dims, per, sides)
        _TWINS[key] = PT.PeriodicTwin(A, dims, nl, masks=masks, sides=sides, periodic=per, singular=singular)
    return _TWINS[key]


def host_ctor(amg, case, **kw):
    dims, nl, masks, per, sides = case
    _, Ac, b, singular = op(dims, per, sides)
    kw = dict(JAC, **kw)
    return amg.Multigrid.tensor_periodic(Ac.indptr, Ac.indices, Ac.data, b, dims, nl, per, axis_masks=masks,
                                         natural_sides=sides, singular=singular, **kw)


def state(mg):
    mg.sync()
    return [(mg.get_soln(l), mg.get_rhs(l)) for l in range(mg.n_levels)]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0].view(np.uint64), y[0].view(np.uint64)) and
                                    np.array_equal(x[1].view(np.uint64), y[1].view(np.uint64)) for x, y in zip(a, b))


def bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def side_masks(dims, per):
    """Side masks on the axes that are not periodic: every subset on the small 2-D grids, else none,
    all, the low and the high ones."""
    dim = len(dims)
    free = PT.open_sides(dim, per)
    if dim == 2 and max(dims) <= 8:
        return sorted({s & free for s in range(1 << (2 * dim))})
    return sorted({0, free, free & N.low_sides(dim), free & N.high_sides(dim)})


def raw_per(amg, dims, am, sides, per, r=None, uH=None, uh=None):
    """amg_hip_tensor_restrict_per (r given) or amg_hip_tensor_prolong_add_per (uH, uh given) through the
    C interface, whatever the masks: the Python wrappers take these entry points only for a non-zero
    periodic mask.  Returns (status, result)."""
    i64, f64 = C.POINTER(C.c_int64), C.POINTER(C.c_double)
    dim = len(dims)
    d3 = np.array(T.dims3(dims), np.int64)
    n_H = int(np.prod(S.coarse_dims(dims, dim, am)))
    if r is not None:
        src, out = np.ascontiguousarray(r, np.float64), np.empty(n_H)
        st = amg.lib().amg_hip_tensor_restrict_per(dim, d3.ctypes.data_as(i64), am, sides, per,
                                                   src.ctypes.data_as(f64), out.ctypes.data_as(f64))
    else:
        src, out = np.ascontiguousarray(uH, np.float64), np.array(uh, np.float64)
        assert src.size == n_H
        st = amg.lib().amg_hip_tensor_prolong_add_per(dim, d3.ctypes.data_as(i64), am, sides, per,
                                                      src.ctypes.data_as(f64), out.ctypes.data_as(f64))
    return st, out


# ---- 1. transfers -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(4, 4), (6, 4), (8, 6), (5, 4), (33, 20), (32, 20), (64, 48), (4, 4, 4), (6, 4, 3),
                                  (5, 6, 4), (16, 12, 8)])
def test_transfer_kernels_equal_spmv_bitwise(amg, dims):
    """K-TensorRestrict / K-TensorProlong with the seam against amg_hip_spmv with the R and P of
    amg_hip_get_transfer, for every legal (axis mask, periodic mask, side mask).  Legal: a coarsened
    periodic axis is even and has 4 points -- (5, 4) and (33, 20) are periodic in y alone, (6, 4, 3) in
    x and y, (5, 6, 4) in y and z wherever those axes are coarsened.  Lengths 4 and 6 put the seam next
    to the first coarse point; 33 is an odd line, whose fine pairs are not all aligned."""
    dim = len(dims)
    n_h = int(np.prod(dims))
    rng = np.random.default_rng(n_h)
    r, uh = rng.standard_normal(n_h), rng.standard_normal(n_h)
    Ac = sp.identity(n_h, format="csc")  # the transfers do not depend on A
    b = np.ones(n_h)
    axes = [m for m in range(1, 1 << dim) if S.mask_error(dims, dim, m) is None]
    count = seams = zero = 0
    for am, per in itertools.product(axes, range(1 << dim)):
        if PT.level_error(dims, dim, am, per) is not None:
            with pytest.raises(ValueError, match="periodic_axes"):
                amg.tensor_restrict(dims, r, axes=am, periodic_axes=per)
            continue
        for sides in side_masks(dims, per):
            mg = amg.Multigrid.tensor_periodic(Ac.indptr, Ac.indices, Ac.data, b, dims, 2, per, axis_masks=(am,),
                                               natural_sides=sides, host_only=True, **JAC)
            P, R = mg.get_transfer(0, "P"), mg.get_transfer(0, "R")
            n_H = mg.get_n_dofs(1)
            mg.close()
            assert bits(P[2], T.csc_triple(PT.periodic_P(dims, dim, am, sides, per))[2])
            uH = rng.standard_normal(n_H)
            got_r = amg.tensor_restrict(dims, r, axes=am, natural_sides=sides, periodic_axes=per)
            want = amg.spmv(n_H, n_h, *R, r)
            assert bits(got_r, want), (dims, am, per, sides, "restrict")
            got = amg.tensor_prolong_add(dims, uH, uh, axes=am, natural_sides=sides, periodic_axes=per)
            want = uh + amg.spmv(n_h, n_H, *P, uH)
            assert bits(got, want), (dims, am, per, sides, "prolong")
            # the _per entry points themselves, called directly: with mask 0 they are the _bc forms (which
            # is what the wrappers above ran for per == 0), with a mask what the wrappers ran
            st, raw = raw_per(amg, dims, am, sides, per, r=r)
            assert st == 0, (dims, am, per, sides, amg.lib().amg_hip_last_error().decode())
            assert bits(raw, got_r), (dims, am, per, sides, "restrict_per")
            st, raw = raw_per(amg, dims, am, sides, per, uH=uH, uh=uh)
            assert st == 0, (dims, am, per, sides, amg.lib().amg_hip_last_error().decode())
            assert bits(raw, got), (dims, am, per, sides, "prolong_add_per")
            zero += per == 0
            count += 1
            seams += bool(per & am)
    assert seams > 0 and zero > 0
    # every axis periodic where the grid allows it: the prolongation reproduces the constants
    full = S.full_mask(dim)
    per = max(p for p in range(1 << dim) if PT.level_error(dims, dim, full, p) is None)
    if per == PT.all_axes(dim):
        n_H = int(np.prod([d // 2 for d in dims]))
        ones = amg.tensor_prolong_add(dims, np.ones(n_H), np.zeros(n_h), periodic_axes=per)
        assert np.array_equal(ones, np.ones(n_h))
    print(f"\n{dims}: {count} (axis mask, periodic mask, side mask) triples bitwise, {seams} with a seam, "
          f"{zero} with mask 0 through the _per entry points against the _bc forms")


# ---- 2. cycle paths ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CYCLE_CASES, ids=["64x48-xy", "32x21-x", "16x12x8-xyz"])
def test_cycle_paths_agree_bitwise(amg, case):
    """The matrix-free and the CSR transfers, the captured graph and the plain launches, give the same
    level vectors after two V-cycles; amg_hip_level_op dispatches on the same kernels."""
    nl = case[1]
    ref_mg = host_ctor(amg, case)
    assert ref_mg.periodic_axes() == case[3]
    assert [ref_mg.level_transfer_kind(l) for l in range(nl - 1)] == [2] * (nl - 1)
    ref_mg.vcycle(2)
    ref = state(ref_mg)
    ref_mg.close()
    assert all(np.all(np.isfinite(u)) for u, _ in ref) and np.linalg.norm(ref[0][0]) > 0
    for v in (dict(stencil_transfers=False), dict(use_graph=False), dict(stencil_transfers=False, use_graph=False)):
        mg = host_ctor(amg, case, **v)
        if "stencil_transfers" in v:
            assert [mg.level_transfer_kind(l) for l in range(nl - 1)] == [0] * (nl - 1)
        mg.vcycle(2)
        got = state(mg)
        mg.close()
        assert same(got, ref), (case, v)
    out = []
    for st in (True, False):
        mg = host_ctor(amg, case, stencil_transfers=st)
        rng = np.random.default_rng(2)
        mg.set_vec(0, "u", rng.standard_normal(mg.get_n_dofs(0)))
        mg.level_op(0, 1)
        mg.level_op(0, 2)
        mg.set_vec(1, "u", rng.standard_normal(mg.get_n_dofs(1)))
        mg.level_op(0, 3)
        mg.sync()
        out.append((mg.get_rhs(1), mg.get_soln(0)))
        mg.close()
    assert bits(out[0][0], out[1][0]) and bits(out[0][1], out[1][1])


# ---- 3. one cycle against the twin ------------------------------------------------------------------
def check(got, ref, e64, scale, what):
    ok, dist, bound, ratio = T.within(got, ref, e64, scale)
    print(f"  {what}: distance {dist:.3e}, e64 {e64:.3e}, ratio {ratio:.2f}, bound {bound:.3e}")
    assert ok, (what, dist, bound, ratio)


@pytest.mark.parametrize("case", CYCLE_CASES, ids=["64x48-xy", "32x21-x", "16x12x8-xyz"])
def test_one_cycle_equals_twin(amg, case):
    """One V-cycle from zero against the twin's longdouble cycle on every level; on the singular cases
    the pinned last unknown and the last entry of the coarsest right-hand side read exactly +0.0."""
    dims, nl, masks, per, sides = case
    _, _, b, singular = op(dims, per, sides)
    tw = twin(dims, nl, masks, per, sides)
    assert tw.n[-1] <= 257  # the twin's longdouble cycle solves the coarsest level in longdouble
    mg = host_ctor(amg, case)
    u64, f64 = tw.vcycle(np.zeros(b.size), b)
    uld, fld = tw.vcycle(np.zeros(b.size, np.longdouble), b, np.longdouble)
    mg.vcycle(1)
    mg.sync()
    print(f"\n{dims}/{nl} periodic {per}, coarsest solve {mg.coarse_solve_kind()}")
    for l in range(nl):
        got = mg.get_soln(l)
        e64 = float(np.linalg.norm(u64[l].astype(np.longdouble) - uld[l]))
        check(got, uld[l], e64, np.linalg.norm(got), f"level-{l} u")
        if l:
            got = mg.get_rhs(l)
            if singular and l == nl - 1:  # zeroed ahead of the pinned solve
                got, want, w64 = got[:-1], fld[l][:-1], f64[l][:-1]
            else:
                want, w64 = fld[l], f64[l]
            e64 = float(np.linalg.norm(w64.astype(np.longdouble) - want))
            check(got, want, e64, np.linalg.norm(got), f"level-{l} f")
    if singular:
        uc, fc = mg.get_soln(nl - 1), mg.get_rhs(nl - 1)
        assert uc[-1] == 0.0 and not np.signbit(uc[-1])
        assert fc[-1] == 0.0 and not np.signbit(fc[-1])
        assert np.linalg.norm(uc) > 0
    mg.close()


# ---- 4. convergence ---------------------------------------------------------------------------------
def true_relres(A, x, b):
    return float(np.linalg.norm(b - A @ x) / np.linalg.norm(b))


_COUNTS = {}


def twin_counts(dims, nl):
    """(periodic, today's best) PCG counts of the twin on the doubly periodic operator: the periodic
    hierarchy, and natural_sides on every side with `singular`."""
    if dims not in _COUNTS:
        A, _, b, _ = op(dims, 3)
        t_per = twin(dims, nl, None, 3, 0).pcg(b, 1e-8)[1]
        t_nat = N.NaturalTwin(A, dims, nl, sides=15, singular=True).pcg(b, 1e-8)[1]
        _COUNTS[dims] = (t_per, t_nat)
    return _COUNTS[dims]


def test_reference_counts_are_grid_independent():
    """The reference alone: the periodic transfers take the same count at both sizes and at most two
    thirds of today's best at 256 x 256."""
    small, large = twin_counts((64, 48), 5), twin_counts((256, 256), 7)
    print(f"\ntwin PCG counts (periodic, natural all + singular): 64x48/5 {small}, 256x256/7 {large}")
    assert 3 * large[0] <= 2 * large[1], large
    assert small[0] == large[0], (small, large)


@pytest.mark.parametrize("dims,nl", [((64, 48), 5), ((256, 256), 7)])
def test_pcg_counts_equal_twin(amg, dims, nl):
    A, Ac, b, _ = op(dims, 3)
    t_per, t_nat = twin_counts(dims, nl)
    found = []
    for name, want in (("periodic", t_per), ("natural", t_nat)):
        if name == "periodic":
            mg = host_ctor(amg, (dims, nl, None, 3, 0))
        else:
            mg = amg.Multigrid.tensor(Ac.indptr, Ac.indices, Ac.data, b, dims, nl, natural_sides=15, singular=True,
                                      **JAC)
        mg.set_vec(0, "u", np.zeros(b.size))
        x, it, rel = mg.pcg(1e-8, 100)
        mg.close()
        true = true_relres(A, x, b)
        print(f"\n{dims}/{nl} {name}: device PCG {it} iterations (relres {rel:.3e}, true {true:.3e}); twin {want}")
        found.append((name, it, want, true))
    for name, it, want, true in found:
        assert abs(it - want) <= 1, (name, it, want)
        assert true <= 1.01e-8, (name, true)


# ---- 5. other forms ---------------------------------------------------------------------------------
def test_other_forms_on_the_periodic_singular_case(amg):
    torch = pytest.importorskip("torch")
    dims, nl, masks, per, _ = FORMS
    A, _, b, singular = op(dims, per)
    assert singular
    mg = host_ctor(amg, FORMS, layout=amg.LAYOUT_SELL)
    assert [mg.level_dims(l) for l in range(nl)] == [(32, 20, 1), (16, 10, 1), (8, 5, 1), (4, 5, 1)]
    n = b.size
    mg.set_vec(0, "u", np.zeros(n))
    x, it, rel = mg.pcg(1e-8, 100)
    assert rel <= 1e-8 and true_relres(A, x, b) <= 1.01e-8
    mg.set_vec(0, "u", np.zeros(n))
    x32, it32, rel32 = mg.pcg_mixed(1e-8, 100)
    print(f"\n{dims}/{nl} periodic, singular: pcg {it} ({rel:.3e}), pcg_mixed {it32} ({rel32:.3e})")
    assert rel32 <= 1e-8 and it32 <= it + 1, (it, it32)
    assert true_relres(A, x32, b) <= 1.01e-8
    # block PCG: per column the bits of pcg
    rng = np.random.default_rng(11)
    B = rng.standard_normal((n, 3))
    B -= B.mean(axis=0)
    xs, its, rels = [], [], []
    for j in range(3):
        mg.set_vec(0, "f", B[:, j])
        mg.set_vec(0, "u", np.zeros(n))
        xj, itj, relj = mg.pcg(1e-8, 100)
        xs.append(xj), its.append(itj), rels.append(relj)
    X, itb, relb = mg.block_pcg(torch.from_numpy(np.ascontiguousarray(B)).cuda(), rtol=1e-8, max_iters=100)
    torch.cuda.synchronize()
    got = X.cpu().numpy()
    for j in range(3):
        assert bits(got[:, j], xs[j]), j
        assert itb[j] == its[j] and relb[j] == rels[j], j
        assert rels[j] <= 1e-8
    mg.close()
    # Chebyshev and the alternating line smoother (open lines: a wrap entry is a coupling off the line)
    for name, sm in (("line-alt", dict(smoother=amg.SM_LINE_ALT, smoother_iters=1, omega=0.8)),
                     ("chebyshev", dict(smoother=amg.SM_CHEBYSHEV, smoother_iters=1, cheb_degree=2))):
        mg = host_ctor(amg, FORMS, **sm)
        mg.set_vec(0, "u", np.zeros(n))
        x, it, rel = mg.pcg(1e-8, 100)
        mg.close()
        true = true_relres(A, x, b)
        print(f"  {name}: {it} iterations, relres {rel:.3e}, true {true:.3e}")
        assert rel <= 1e-8 and true <= 1.01e-8, (name, it, rel, true)
    # multicolour Gauss-Seidel is not a symmetric preconditioner: plain V-cycles
    mg = host_ctor(amg, FORMS, smoother=amg.SM_MULTICOLOR_GS, smoother_iters=1, omega=1.0)
    mg.set_vec(0, "u", np.zeros(n))
    mg.vcycle(30)
    mg.sync()
    true = true_relres(A, mg.get_soln(0), b)
    mg.close()
    print(f"  multicolour GS: true relative residual {true:.3e} after 30 V-cycles")
    assert true <= 1e-8, true


# ---- 6. the _dev constructor ------------------------------------------------------------------------
@pytest.mark.parametrize("case", [XY, X_DIR, FORMS], ids=["64x48-xy", "32x21-x", "32x20-masks"])
def test_dev_constructor_equals_host_constructor(amg, case):
    dims, nl, masks, per, sides = case
    A, _, b, singular = op(dims, per, sides)
    arrs = (A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy(), np.array(b))
    dev = amg.Multigrid.tensor_periodic_dev(*arrs, dims, nl, per, axis_masks=masks, natural_sides=sides,
                                            singular=singular, **JAC)
    host = host_ctor(amg, case)
    assert dev.setup_on_device == 0 and host.setup_on_device == 0
    assert dev.n_levels == host.n_levels == nl
    assert dev.periodic_axes() == host.periodic_axes() == per
    for l in range(nl):
        assert dev.level_dims(l) == host.level_dims(l), l
        a, c = dev.get_coefficient_matrix(l), host.get_coefficient_matrix(l)
        assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1]) and bits(a[2], c[2]), l
    for l in range(nl - 1):
        assert dev.level_axes(l) == host.level_axes(l) and dev.level_transfer_kind(l) == 2
        for w in "PR":
            a, c = dev.get_transfer(l, w), host.get_transfer(l, w)
            assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1]) and bits(a[2], c[2]), (l, w)
    dev.vcycle(2)
    host.vcycle(2)
    assert same(state(dev), state(host)), case
    dev.close()
    host.close()
    # a malformed CSR array is refused by the check kernel, as by amg_hip_create_tensor_dev
    bad = arrs[1].copy()
    bad[3] = -1
    with pytest.raises(ValueError, match="malformed"):
        amg.Multigrid.tensor_periodic_dev(arrs[0], bad, arrs[2], arrs[3], dims, nl, per, axis_masks=masks,
                                          natural_sides=sides, singular=singular, **JAC)
