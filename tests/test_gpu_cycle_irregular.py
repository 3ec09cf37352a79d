"""Whole cycles on irregular operators: the strength-based hierarchy (amg_hip_create_rs) of a
k-nearest-neighbour M-matrix (knn(1600, 4, 1): ragged SELL / CSR levels) and of a window-permuted
Laplacian (winperm(40, 8, 2): dictionary levels with thousands of distinct rows), against the oracle
twin on the same hierarchy (oracle.ruge_stueben_hierarchy), in every layout, captured and eager.

  cycles      3 V-cycles, u and f of every level bit for bit: SpGS, true Jacobi 2+2 omega 0.6,
              multicolour GS with the library's colours replayed in the oracle
  level data  level matrices and transfers bit for bit; level_layout(l) is what the host model of the
              layout rule (irregular_mats.plan) gives for the pruned level matrix
  PCG         iteration count of the oracle's PCG, true residual <= 1.01e-10 ||b||
  Chebyshev   bit-identical across layouts and cycle paths; the smoother alone bit for bit against
              tests/cheb_twin.py on every level.  The twin takes the transfers from the solver, but
              its coarsest solve is a scipy LU, not the library's band solve, so whole cycles are
              compared to 1e-10 (the bound of test_gpu_chebyshev.py), not bit for bit
  block       block_vcycles / block_pcg with k = 3 and 8: every column has the bits of the
              single-vector call (Jacobi and Chebyshev: the smoothers the block cycle has)
  float       apply_f32 on the SELL and CSR solvers: finite, non-zero, within 1e-5 of amg_hip_apply
              (the bound of test_gpu_mixed.py for hierarchies without a float twin), same bits
              captured and eager

Largest relative distance of apply_f32 from amg_hip_apply seen on an MI355X: 1.153e-07 (knn, SELL and CSR alike;
winperm 6.855e-08).  Chebyshev: 3 cycles within 9.3e-16 of the twin's."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "algebraic-multigrid_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cheb_twin as CT  # noqa: E402
import irregular_mats as im  # noqa: E402

pytestmark = pytest.mark.gpu

OPS = ["knn", "winperm"]
LAYOUTS = [("csr", im.LAYOUT_CSR), ("sell", im.LAYOUT_SELL), ("dict", im.LAYOUT_DICT), ("auto", im.LAYOUT_AUTO)]
RS = (12, 0.25, 40)                       # max_levels, theta, min_coarse
JAC = dict(smoother=3, smoother_iters=2, omega=0.6)
CHEB = dict(smoother=5, smoother_iters=1, cheb_degree=2)
_SETUP = {}


def setup(oracle, op):
    """(scipy CSR, oracle CSC, right-hand side, the oracle's transfers), made once per operator."""
    if op not in _SETUP:
        M = im.knn(1600, 4, 1) if op == "knn" else im.winperm(40, 8, 2)
        S = M.tocsc()
        S.sort_indices()
        A = oracle.CSC(M.shape[0], M.shape[1], S.indptr, S.indices, S.data)
        b = np.random.default_rng(7).standard_normal(M.shape[0])
        b.setflags(write=False)
        _SETUP[op] = (M, A, b, oracle.ruge_stueben_hierarchy(A, *RS))
    return _SETUP[op]


def solver(amg, oracle, op, **kw):
    M, A, b, Ps = setup(oracle, op)
    mg = amg.Multigrid.ruge_stueben(A.colptr, A.rowind, A.val, b, *RS, exact_coarse_solve=True, exact_gs=True, **kw)
    assert mg.n_levels == len(Ps) + 1
    return mg


def dev(a):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")   # a copy: `a` may be read-only


def state(mg):
    return [(mg.get_soln(l), mg.get_rhs(l)) for l in range(mg.n_levels)]


def same(a, b):
    return all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


@pytest.mark.parametrize("sm", ["spgs", "jacobi", "multicolor"])
@pytest.mark.parametrize("op", OPS)
def test_vcycles_equal_the_oracle_vector_by_vector(amg, oracle, op, sm):
    M, A, b, Ps = setup(oracle, op)
    kw_o = {"spgs": dict(smoother=oracle.SM_SPGS, smoother_iters=1),
            "jacobi": dict(smoother=oracle.SM_TRUE_JACOBI, smoother_iters=2, omega=0.6),
            "multicolor": dict(smoother=oracle.SM_MULTICOLOR, smoother_iters=1)}[sm]
    kw_p = {"spgs": dict(smoother=amg.SM_SPGS, smoother_iters=1), "jacobi": JAC,
            "multicolor": dict(smoother=amg.SM_MULTICOLOR_GS, smoother_iters=1)}[sm]
    for lname, layout in LAYOUTS:
        for graph in (True, False):
            mg = solver(amg, oracle, op, layout=layout, use_graph=graph, **kw_p)
            ref = oracle.Multigrid(A, b, len(Ps) + 1, transfers=Ps, **kw_o)
            L = mg.n_levels
            if sm == "multicolor":
                for l in range(L):
                    col, nc = mg.get_colors(l)
                    ref.set_colors(l, col, nc)
            r0 = ref.rss()
            for c in range(3):
                ref.vcycle()
                mg.vcycle()
                for l in range(L):
                    assert np.array_equal(mg.get_soln(l), ref.get_vec(l, "u")), (op, sm, lname, graph, c, l, "u")
                    assert np.array_equal(mg.get_rhs(l), ref.get_vec(l, "f")), (op, sm, lname, graph, c, l, "f")
                assert abs(mg.rss() - ref.rss()) <= 1e-11 * ref.rss()
            assert ref.rss() < 0.05 * r0                       # the cycle does reduce the residual
            mg.close()


@pytest.mark.parametrize("op", OPS)
def test_level_data_and_layouts(amg, oracle, op):
    M, A, b, Ps = setup(oracle, op)
    ref = oracle.Multigrid(A, b, len(Ps) + 1, transfers=Ps)
    seen = set()
    for lname, layout in LAYOUTS:
        mg = solver(amg, oracle, op, layout=layout, **JAC)
        for l in range(mg.n_levels):
            Al = ref.level_matrix(l)
            for got, want in zip(mg.get_coefficient_matrix(l), (Al.colptr, Al.rowind, Al.val)):
                assert np.array_equal(got, want), (op, lname, l)
            rows = im.pruned(CT.csr_of(Al.colptr, Al.rowind, Al.val, Al.rows, Al.cols))
            want = im.plan(rows, layout)
            assert mg.level_layout(l) == (want.layout, want.stream_bytes), (op, lname, l, mg.level_layout(l), want)
            seen.add((lname, im.LAYOUT_NAME[want.layout], want.typed))
            if l + 1 < mg.n_levels:
                for which in "PR":
                    T = ref.transfer(l, which)
                    for got, want_a in zip(mg.get_transfer(l, which), (T.colptr, T.rowind, T.val)):
                        assert np.array_equal(got, want_a), (op, lname, l, which)
        mg.close()
    # the operator lands where it was meant to
    if op == "knn":
        assert ("auto", "sell", None) in seen and ("dict", "sell", None) in seen
    else:
        assert ("auto", "dict", False) in seen


@pytest.mark.parametrize("op", OPS)
def test_pcg_iterations_and_true_residual(amg, oracle, op):
    M, A, b, Ps = setup(oracle, op)
    ref = oracle.Multigrid(A, b, len(Ps) + 1, transfers=Ps, smoother=oracle.SM_TRUE_JACOBI, smoother_iters=2,
                           omega=0.6)
    ref.set_vec(0, "u", np.zeros(b.size))
    _, it_ref, _ = ref.pcg(1e-10, 100)
    for lname, layout in LAYOUTS:
        mg = solver(amg, oracle, op, layout=layout, **JAC)
        mg.set_vec(0, "u", np.zeros(b.size))
        x, it, rel = mg.pcg(1e-10, 100)
        true = float(np.linalg.norm(b - M @ x) / np.linalg.norm(b))
        print(f"pcg {op} {lname}: {it} iterations (oracle {it_ref}), relres {rel:.3e}, true {true:.3e}")
        assert it == it_ref, (op, lname, it, it_ref)
        assert true <= 1.01e-10, (op, lname, true)
        mg.close()


@pytest.mark.parametrize("op", OPS)
def test_chebyshev_cycles(amg, oracle, op):
    M, A, b, Ps = setup(oracle, op)
    base = None
    rng = np.random.default_rng(5)
    for lname, layout in LAYOUTS:
        for graph in (True, False):
            mg = solver(amg, oracle, op, layout=layout, use_graph=graph, **CHEB)
            if base is None:                                   # the twin, once
                tw = CT.Twin(mg, 2, 0.3, 1.0, 1)
                u = np.zeros(b.size)
                for _ in range(3):
                    u = tw.vcycle(u, b)[0][0]
            if graph:                                          # the smoother alone, bit for bit
                for l in range(mg.n_levels - 1):
                    n = mg.get_n_dofs(l)
                    ul, fl = rng.standard_normal(n), rng.standard_normal(n)
                    mg.set_vec(l, "u", ul)
                    mg.set_vec(l, "f", fl)
                    mg.level_op(l, 0)
                    mg.sync()
                    assert np.array_equal(mg.get_soln(l), tw.smooth(l, ul, fl)), (op, lname, l)
                mg.set_vec(0, "u", np.zeros(b.size))
                mg.set_vec(0, "f", b)
            mg.vcycle(3)
            mg.sync()
            st = state(mg)
            base = base or st
            assert same(st, base), (op, lname, graph)
            d = np.linalg.norm(st[0][0] - u) / np.linalg.norm(u)
            print(f"chebyshev {op} {lname} graph={graph}: distance from the twin's 3 cycles {d:.3e}")
            assert d <= 1e-10
            mg.close()


def single_columns(mg, U0, F0, n):
    out = np.empty_like(U0)
    for j in range(U0.shape[1]):
        mg.set_vec(0, "u", U0[:, j])
        mg.set_vec(0, "f", F0[:, j])
        mg.vcycle(n)
        out[:, j] = mg.get_soln(0)
    return out


@pytest.mark.parametrize("sm", ["jacobi", "chebyshev"])
@pytest.mark.parametrize("op", OPS)
def test_block_cycles_column_by_column(amg, oracle, op, sm):
    M, A, b, Ps = setup(oracle, op)
    kw = JAC if sm == "jacobi" else CHEB
    rng = np.random.default_rng(11)
    n0 = b.size
    U0, F0 = rng.standard_normal((n0, 8)), rng.standard_normal((n0, 8))
    B0 = np.stack([b, 1e-6 * b] + [rng.standard_normal(n0) for _ in range(6)], 1)
    want = want_pcg = None
    for lname, layout in LAYOUTS:
        mg = solver(amg, oracle, op, layout=layout, **kw)
        cols = single_columns(mg, U0, F0, 2)
        want = cols if want is None else want
        assert np.array_equal(cols, want), (op, sm, lname)     # the single-vector cycle across layouts
        for k in (3, 8):                                       # 3 columns run padded to 4
            U = dev(U0[:, :k])
            mg.block_vcycles(U, dev(F0[:, :k]), n=2)
            torch.cuda.synchronize()
            got = U.cpu().numpy()
            for j in range(k):
                assert np.array_equal(got[:, j], want[:, j]), (op, sm, lname, k, j)
        single = []
        for j in range(8):
            mg.set_vec(0, "f", B0[:, j])
            mg.set_vec(0, "u", np.zeros(n0))
            single.append(mg.pcg(1e-9, 60))
        want_pcg = single if want_pcg is None else want_pcg
        for k in (3, 8):
            X, it, rel = mg.block_pcg(dev(B0[:, :k]), rtol=1e-9, max_iters=60)
            torch.cuda.synchronize()
            got = X.cpu().numpy()
            for j in range(k):
                x, it_s, rel_s = want_pcg[j]
                assert (it[j], rel[j]) == (it_s, rel_s), (op, sm, lname, k, j, it[j], it_s)
                assert np.array_equal(got[:, j], x), (op, sm, lname, k, j)
                assert rel_s <= 1e-9
        mg.close()


def _apply(mg, v, f32):
    dv = dev(v)
    dz = torch.empty_like(dv)
    (mg.apply_f32 if f32 else mg.apply_dev)(dv.data_ptr(), dz.data_ptr())
    mg.sync()
    return dz.cpu().numpy()


@pytest.mark.parametrize("lname,layout", [("sell", im.LAYOUT_SELL), ("csr", im.LAYOUT_CSR)])
@pytest.mark.parametrize("op", OPS)
def test_float_cycle(amg, oracle, op, lname, layout):
    M, A, b, Ps = setup(oracle, op)
    out = []
    for graph in (True, False):
        mg = solver(amg, oracle, op, layout=layout, use_graph=graph, **JAC)
        assert mg.level_layout(0)[0] == layout
        z, z64 = _apply(mg, b, True), _apply(mg, b, False)
        assert np.array_equal(z, _apply(mg, b, True))          # the replayed graph
        rel = float(np.linalg.norm(z - z64) / np.linalg.norm(z64))
        print(f"float cycle {op} {lname} graph={graph}: relative distance from amg_hip_apply {rel:.3e}")
        assert np.all(np.isfinite(z)) and np.linalg.norm(z) > 0 and np.linalg.norm(z64) > 0
        assert rel <= 1e-5
        out.append(z)
        mg.close()
    assert np.array_equal(out[0], out[1])
