"""Semi-coarsening tensor hierarchies (amg_hip_create_tensor_semi), the parts that need no GPU: on
host_only solvers P / R against the Kronecker products of the scipy twin (tests/semi_twin.py) entry
for entry, the level matrices against amg_hip_create_custom on the twin's operators bit for bit, the
level grids and masks, amg_hip_tensor_axis_strength against the numpy rule, the automatic masks on
the anisotropic and the isotropic cases, every argument error -- and, on the twin alone, the
condition that makes the cases worth having: semi-coarsening at most halves the PCG count."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "algebraic-multigrid_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import semi_twin as S  # noqa: E402
import tensor_twin as T  # noqa: E402

JAC = dict(smoother_iters=2, omega=0.8)

# explicit masks: every mask on small odd / even grids, and chains that mix them
EXPLICIT = [((7, 5), (m,)) for m in (1, 2, 3)] + [((8, 6), (1, 2, 3)), ((33, 20), (2, 1, 2, 3)),
                                                   ((2, 3), (1,)), ((2, 3), (2,))]
EXPLICIT += [((7, 5, 3), (m,)) for m in range(1, 8)] + [((8, 6, 4), (4, 1, 2, 7)), ((17, 12, 9), (5, 2, 6, 3)),
                                                         ((2, 3, 2), (5,)), ((2, 3, 2), (2,))]


def csc(A):
    A = sp.csc_matrix(A)
    A.sort_indices()
    return A


def _same_triple(got, want):
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and
            np.array_equal(np.asarray(got[2]).view(np.uint64), np.asarray(want[2]).view(np.uint64)))


def make(amg, A, b, dims, n_levels, masks=None, **kw):
    A = csc(A)
    kw.setdefault("smoother", amg.SM_JACOBI)
    for k, v in JAC.items():
        kw.setdefault(k, v)
    return amg.Multigrid.tensor_semi(A.indptr, A.indices, A.data, b, dims, n_levels, axis_masks=masks,
                                     theta=S.THETA, min_coarse=S.MIN_COARSE, host_only=True, **kw)


def _explicit(dims, masks):
    eps = (1.0, 0.3, 0.05)[:len(dims)]
    A = S.diffusion(dims, eps, seed=7)
    return A, S.rhs(A.shape[0], seed=8), S.SemiTwin(A, dims, masks=masks)


@pytest.mark.parametrize("dims,masks", EXPLICIT)
def test_explicit_masks_against_the_twin(amg, dims, masks):
    """dims, masks, P / R entry for entry, level matrices bit for bit with amg_hip_create_custom."""
    A, b, tw = _explicit(dims, masks)
    nl = len(masks) + 1
    mg = make(amg, A, b, dims, nl, masks)
    assert mg.n_levels == nl
    assert [mg.level_dims(l) for l in range(nl)] == tw.dims
    assert [mg.level_axes(l) for l in range(nl - 1)] == list(masks)
    with pytest.raises(ValueError):
        mg.level_axes(nl - 1)
    assert [mg.level_transfer_kind(l) for l in range(nl - 1)] == [2] * (nl - 1)
    transfers = []
    for l in range(nl - 1):
        P = S.semi_P(tw.dims[l], tw.dim, masks[l])
        assert _same_triple(mg.get_transfer(l, "P"), T.csc_triple(P)), (l, "P")
        assert _same_triple(mg.get_transfer(l, "R"), T.csc_triple(P.T)), (l, "R")
        assert set(np.unique(P.data)) <= {2.0 ** -k for k in range(tw.dim + 1)}
        transfers.append((T.csc_triple(P), T.csc_triple(P.T)))
    A0 = csc(A)
    cu = amg.Multigrid(A0.indptr, A0.indices, A0.data, b, nl, smoother=amg.SM_JACOBI, transfers=transfers,
                       host_only=True, **JAC)
    for l in range(nl):
        assert cu.get_n_dofs(l) == mg.get_n_dofs(l) == tw.n[l], l
        assert _same_triple(mg.get_coefficient_matrix(l), cu.get_coefficient_matrix(l)), l
    cu.close()
    mg.close()
    csr = make(amg, A, b, dims, nl, masks, stencil_transfers=False)
    assert [csr.level_transfer_kind(l) for l in range(nl - 1)] == [0] * (nl - 1)
    assert [csr.level_axes(l) for l in range(nl - 1)] == list(masks)
    csr.close()


@pytest.mark.parametrize("dims,eps", S.ANISO + tuple((d, (1.0,) * len(d)) for d in S.ISO))
def test_axis_strength_equals_the_numpy_rule(amg, dims, eps):
    A, _, tw = S.case(dims, eps)
    M = csc(A)
    w = amg.tensor_axis_strength(M.indptr, M.indices, M.data, dims)
    assert np.array_equal(w.view(np.uint64), S.axis_strength(A, dims).view(np.uint64)), (w, tw.w[0])
    if len(dims) == 2:
        assert w[2] == 0.0
    # a coarse level of the twin (9- / 27-point rows: diagonal neighbours do not count)
    Ac = csc(tw.A[1])
    wc = amg.tensor_axis_strength(Ac.indptr, Ac.indices, Ac.data, tw.dims[1][:len(dims)])
    assert np.array_equal(wc.view(np.uint64), S.axis_strength(tw.A[1], tw.dims[1]).view(np.uint64))


EXPECT = {  # the axes the rule picks per level
    ((33, 20), (1.0, 1e-3)): "x x x x x",
    ((33, 20), (1e-3, 1.0)): "y y y y x",
    ((64, 48), (1.0, 1e-2)): "x x x xy y y",
    ((17, 12, 9), (1.0, 1.0, 1e-3)): "xy xy xy",
    ((17, 12, 9), (1e-3, 1.0, 1e-3)): "y y y xz",
    ((48, 40, 24), (1.0, 1e-2, 1.0)): "xz xz xz xz xy",
}
NAMES = {1: "x", 2: "y", 3: "xy", 4: "z", 5: "xz", 6: "yz", 7: "xyz"}


@pytest.mark.parametrize("dims,eps", S.ANISO)
def test_automatic_masks_on_the_anisotropic_cases(amg, dims, eps):
    A, b, tw = S.case(dims, eps)
    assert " ".join(NAMES[m] for m in tw.masks) == EXPECT[(dims, eps)]
    mg = make(amg, A, b, dims, S.MAX_LEVELS)
    assert mg.n_levels == tw.nl
    assert [mg.level_axes(l) for l in range(tw.nl - 1)] == tw.masks
    assert [mg.level_dims(l) for l in range(tw.nl)] == tw.dims
    assert [mg.get_n_dofs(l) for l in range(tw.nl)] == tw.n
    # the same hierarchy as the explicit constructor on those masks
    ex = make(amg, A, b, dims, tw.nl, tw.masks)
    for l in range(tw.nl):
        assert _same_triple(mg.get_coefficient_matrix(l), ex.get_coefficient_matrix(l)), l
    ex.close()
    # n_levels is a maximum
    cut = make(amg, A, b, dims, 3)
    assert cut.n_levels == 3 and [cut.level_axes(l) for l in range(2)] == tw.masks[:2]
    cut.close()
    mg.close()


@pytest.mark.parametrize("dims", S.ISO)
def test_isotropic_operators_get_full_coarsening(amg, dims):
    dim = len(dims)
    A, b, tw = S.case(dims, (1.0,) * dim)
    assert tw.masks == [S.full_mask(dim)] * (tw.nl - 1)
    mg = make(amg, A, b, dims, S.MAX_LEVELS)
    assert mg.n_levels == tw.nl
    assert [mg.level_axes(l) for l in range(tw.nl - 1)] == tw.masks
    M = csc(A)
    full = amg.Multigrid.tensor(M.indptr, M.indices, M.data, b, dims, tw.nl, smoother=amg.SM_JACOBI,
                                host_only=True, **JAC)
    for l in range(tw.nl):
        assert full.level_dims(l) == mg.level_dims(l)
        assert _same_triple(mg.get_coefficient_matrix(l), full.get_coefficient_matrix(l)), l
    # the full-coarsening constructors report the full mask
    assert [full.level_axes(l) for l in range(tw.nl - 1)] == tw.masks
    with pytest.raises(ValueError):
        full.level_axes(tw.nl - 1)
    full.close()
    mg.close()


def test_the_rule_stops_where_it_says(amg):
    A, b, tw = S.case((33, 20), (1.0, 1e-3))
    # min_coarse: the first level of at most that many rows is the last
    M = csc(A)
    mg = amg.Multigrid.tensor_semi(M.indptr, M.indices, M.data, b, (33, 20), 16, theta=0.5, min_coarse=200,
                                   smoother=amg.SM_JACOBI, host_only=True, **JAC)
    assert [mg.get_n_dofs(l) for l in range(mg.n_levels)] == [660, 320, 160]
    mg.close()
    # no eligible axis: a 1 x 1 grid has one level whatever n_levels says
    one = amg.Multigrid.tensor_semi(np.array([0, 1], np.int32), np.array([0], np.int32), np.array([2.0]),
                                    np.ones(1), (1, 1), 5, theta=0.5, min_coarse=1, smoother=amg.SM_JACOBI,
                                    host_only=True, **JAC)
    assert one.n_levels == 1
    one.close()
    # theta = 1: only the strongest axis
    A2 = S.diffusion((12, 10), (1.0, 0.9), seed=3)
    M2 = csc(A2)
    w = S.axis_strength(A2, (12, 10))
    strict = amg.Multigrid.tensor_semi(M2.indptr, M2.indices, M2.data, np.ones(120), (12, 10), 2, theta=1.0,
                                       min_coarse=1, smoother=amg.SM_JACOBI, host_only=True, **JAC)
    assert strict.level_axes(0) == (1 if w[0] > w[1] else 2)
    strict.close()


def _raw_semi(amg, A, b, dim, dims3, levels, masks, theta=0.5, min_coarse=32, window=0):
    A = csc(A)
    o = amg.Options()
    amg.lib().amg_hip_default_options(C.byref(o))
    o.host_only = 1
    o.window = window
    h = C.c_void_p()
    d = np.array(dims3, np.int64)
    i32, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    cp, ri, v, b = (np.ascontiguousarray(A.indptr, np.int32), np.ascontiguousarray(A.indices, np.int32),
                    np.ascontiguousarray(A.data, np.float64), np.ascontiguousarray(b, np.float64))
    m = None if masks is None else np.ascontiguousarray(masks, np.int32)
    st = amg.lib().amg_hip_create_tensor_semi(A.shape[0], cp.ctypes.data_as(i32), ri.ctypes.data_as(i32),
                                              v.ctypes.data_as(f64), b.ctypes.data_as(f64), dim,
                                              d.ctypes.data_as(C.POINTER(C.c_int64)), levels,
                                              None if m is None else m.ctypes.data_as(i32), theta, min_coarse,
                                              C.byref(o), C.byref(h))
    msg = amg.lib().amg_hip_last_error().decode()
    if st == 0:
        amg.lib().amg_hip_destroy(h)
    return st, msg


def test_argument_errors(amg, oracle):
    A = S.diffusion((12, 10), (1.0, 1e-2))
    b = np.ones(120)
    A3 = S.diffusion((4, 3, 2), (1.0, 1.0, 1.0))
    b3 = np.ones(24)
    ok = _raw_semi(amg, A, b, 2, (12, 10, 1), 3, [1, 3])
    assert ok[0] == 0, ok
    for masks, level, word in (([0, 1], 0, "no axis"), ([1, 0], 1, "no axis"), ([4, 1], 0, "z"),
                               ([1, 5], 1, "z"), ([8, 1], 0, "bits"), ([3, 16], 1, "bits"),
                               ([-1, 1], 0, "bits")):
        st, msg = _raw_semi(amg, A, b, 2, (12, 10, 1), 3, masks)
        assert st == amg.EINVAL and f"level {level}" in msg and word in msg, (masks, msg)
    # a masked axis shorter than 2: y of 10 -> 5 -> 2 -> 1
    st, msg = _raw_semi(amg, A, b, 2, (12, 10, 1), 5, [2, 2, 2, 2])
    assert st == amg.EINVAL and "level 3" in msg and "axis y" in msg, msg
    st, msg = _raw_semi(amg, A3, b3, 3, (4, 3, 2), 3, [4, 4])
    assert st == amg.EINVAL and "level 1" in msg and "axis z" in msg, msg
    assert _raw_semi(amg, A3, b3, 3, (4, 3, 2), 3, [4, 3])[0] == 0
    # the automatic rule's parameters
    for theta in (0.0, -0.5, 1.5, float("nan")):
        st, msg = _raw_semi(amg, A, b, 2, (12, 10, 1), 3, None, theta=theta)
        assert st == amg.EINVAL and "theta" in msg, (theta, msg)
    st, msg = _raw_semi(amg, A, b, 2, (12, 10, 1), 3, None, min_coarse=0)
    assert st == amg.EINVAL and "min_coarse" in msg
    assert _raw_semi(amg, A, b, 2, (12, 10, 1), 3, None, theta=1.0, min_coarse=1)[0] == 0
    # explicit masks ignore theta and min_coarse
    assert _raw_semi(amg, A, b, 2, (12, 10, 1), 3, [1, 3], theta=-1.0, min_coarse=0)[0] == 0
    # the grid
    assert _raw_semi(amg, A, b, 2, (12, 11, 1), 2, [1])[0] == amg.EINVAL
    assert _raw_semi(amg, A, b, 2, (12, 5, 2), 2, [1])[0] == amg.EINVAL
    assert _raw_semi(amg, A, b, 4, (12, 10, 1), 2, [1])[0] == amg.EINVAL
    assert _raw_semi(amg, A, b, 2, (12, 10, 1), 0, None)[0] == amg.EINVAL
    st, msg = _raw_semi(amg, A, b, 2, (12, 10, 1), 2, [1], window=1)
    assert st == amg.EUNSUPPORTED and "amg_hip_create_tensor_semi" in msg
    # every smoother builds, the alternating line smoother included (the level grids are known)
    M = csc(A)
    for sm in (amg.SM_SPGS, amg.SM_REF_JACOBI, amg.SM_SOR, amg.SM_JACOBI, amg.SM_MULTICOLOR_GS,
               amg.SM_CHEBYSHEV, amg.SM_LINE_JACOBI, amg.SM_LINE_ALT):
        mg = amg.Multigrid.tensor_semi(M.indptr, M.indices, M.data, b, (12, 10), 4, axis_masks=(1, 1, 1),
                                       host_only=True, smoother=sm, omega=0.7)
        assert mg.level_dims(3) == (1, 10, 1)
        if sm == amg.SM_LINE_ALT:  # strides of the directions: a level of one x point has its y lines only
            assert mg.line_directions(0) == [1, 12] and mg.line_directions(3) == [1]
        mg.close()
    with pytest.raises(ValueError, match="n_levels - 1"):
        amg.Multigrid.tensor_semi(M.indptr, M.indices, M.data, b, (12, 10), 4, axis_masks=(1, 1), host_only=True)
    # level_axes belongs to tensor solvers
    L, rb = oracle.laplacian(16), oracle.rhs(16)
    flat = amg.Multigrid(L.colptr, L.rowind, L.val, rb, 3, host_only=True)
    with pytest.raises(ValueError):
        flat.level_axes(0)
    flat.close()
    # axis strength: the grid must match
    with pytest.raises(ValueError):
        amg.tensor_axis_strength(M.indptr, M.indices, M.data, (12, 11))
    # the stand-alone transfers check their mask before they look for a device
    for mask in (0, 4, 8, -1):
        with pytest.raises(ValueError):
            amg.tensor_restrict((12, 10), np.ones(120), axes=mask)
    with pytest.raises(ValueError, match="axis x"):
        amg.tensor_prolong_add((1, 10), np.ones(0), np.ones(10), axes=1)


@pytest.mark.parametrize("dims,eps", S.ANISO)
def test_twin_semi_coarsening_halves_the_pcg_count(dims, eps):
    """A condition on the inputs, on the twin alone: on every anisotropic case PCG to 1e-8 with the
    semi-coarsening cycle takes at most half the iterations of the full-coarsening cycle (12 against
    68 down to 9 against 31), and no more than 12."""
    A, b, tw = S.case(dims, eps)
    semi = tw.pcg(b, 1e-8)[1]
    full = S.full_twin(A, dims).pcg(b, 1e-8)[1]
    assert 2 * semi <= full and semi <= 12, (semi, full)


DROPIN_SRC = r"""
#include <cstdlib>
#include <iostream>
#include <amg/grid.hpp>
#include <amg/interpolator.hpp>
#include <amg/multigrid.hpp>
#include <amg/smoother.hpp>

int main(int argc, char** argv) {
  AMG::SemiTensorInterpolator<double> rule(12, 10);
  if (!rule.masks().empty() || rule.theta() != 0.5 || rule.min_coarse() != 32 || rule.dim() != 2) return 2;
  int threw = 0;
  try { rule.make_operators(120, 60, 0); } catch (const std::logic_error&) { ++threw; }
  if (threw != 1) return 3;
  if (argc < 2) { std::cout << "constructed" << std::endl; return 0; }  // CPU: no device
  const int N = std::atoi(argv[1]);
  Eigen::SparseMatrix<double> A = AMG::Grid<double>::laplacian(N);
  Eigen::VectorXd b = AMG::Grid<double>::rhs(N);
  AMG::SemiTensorInterpolator<double> interp(N, N, 1, {1, 2, 3});
  AMG::TrueJacobi<double> jac(0.8, 2);
  AMG::Multigrid<double> mg(&interp, &jac, A, b, 4, 1e-9, 5, 50);
  const int32_t want[3] = {1, 2, 3};
  for (int l = 0; l < 3; ++l) {
    int32_t kind = -1, mask = -1;
    if (amg_hip_level_transfer_kind(mg.native_handle(), l, &kind) != AMG_HIP_OK || kind != 2) return 4;
    if (amg_hip_get_level_axes(mg.native_handle(), l, &mask) != AMG_HIP_OK || mask != want[l]) return 5;
  }
  if (mg.get_n_levels() != 4 || (long)interp.get_P(0).rows() != (long)N * N ||
      (long)interp.get_P(0).cols() != (long)(N / 2) * N || (long)interp.get_P(1).cols() != (long)(N / 2) * (N / 2) ||
      (long)mg.get_n_dofs(3) != (long)(N / 4) * (N / 4))
    return 6;
  bool refused = false;
  try {
    AMG::SemiTensorInterpolator<double> bad(N, N, 1, {1, 2});
    AMG::Multigrid<double> no(&bad, &jac, A, b, 4, 1e-9, 5, 50);
  } catch (const std::invalid_argument&) { refused = true; }
  if (!refused) return 7;
  const double r0 = AMG::rss(A, mg.get_soln(0), b);
  for (int i = 0; i < 6; ++i) mg.vcycle();
  const double r6 = AMG::rss(A, mg.get_soln(0), b);
  std::cout.precision(17);
  std::cout << "drop6 " << r6 / r0 << std::endl;
  return r6 < 1e-4 * r0 ? 0 : 1;
}
"""


def build_dropin(amg, tmp_path):
    src = tmp_path / "semi_dropin.cpp"
    src.write_text(DROPIN_SRC)
    exe = tmp_path / "semi_dropin"
    pkg = os.path.dirname(amg.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe), "-L" + pkg, "-lamg_hip", "-Wl,-rpath," + pkg,
                           "-Wl,-rpath,/opt/rocm/lib"])
    return str(exe)


def test_dropin_semi_interpolator_compiles_and_constructs(amg, tmp_path):
    exe = build_dropin(amg, tmp_path)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "constructed" in p.stdout, p.stdout + p.stderr
