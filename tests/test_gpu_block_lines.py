"""Block V-cycle, rss and PCG with the line smoothers (amg_hip_set_block_lines) on an MI355X: column j of
every block result must have the bits of the single-vector path on column j, for AMG_HIP_SM_LINE_JACOBI
(K-Line on panels: many-chain and few-chain separator walks, chains without a separator, chains longer
than one LDS chunk), AMG_HIP_SM_LINE_ALT (K-LineX on panels: one chunk, several lines per run, odd nx,
long runs, no x direction, three directions) and cyclic lines (K-LineSeam on panels: every seam width and
strided lines); the solver's own vectors are left alone, the switch off refuses as before, and the dry
run's bytes equal the figure worked by hand.  Every shape is the smallest that still reaches its path."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
sp = pytest.importorskip("scipy.sparse")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import f32_line_twin as LT  # noqa: E402
import line_alt_twin as AT  # noqa: E402
import periodic_twin as PT  # noqa: E402

LINE, ALT = 6, 7  # AMG_HIP_SM_LINE_JACOBI, AMG_HIP_SM_LINE_ALT
K_ALL = (1, 3, 8, 16)


@pytest.fixture
def lines_on(amg):
    amg.set_block_lines(1)
    yield
    amg.set_block_lines(0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def csc(A):
    Ac = sp.csc_matrix(A)
    Ac.sort_indices()
    return Ac.indptr.astype(np.int32), Ac.indices.astype(np.int32), Ac.data.copy()


def nonsym(A):
    """the lower triangle scaled: dl != du in every direction, the rows stay diagonally dominant"""
    return sp.csr_matrix(sp.triu(A) + 0.7 * sp.tril(A, -1))


def long_chains(n, s):
    """tests/test_gpu_line.py's few long chains: a strong coupling at offset s (and a weak one that is no
    multiple of s when s > 1, so that the stride rule picks s)"""
    rng = np.random.default_rng(n)
    offs = [s, 3 * s + 1] if s > 1 else [1]
    bands = [-(0.9 + 0.2 * rng.random(n - offs[0]))] + [-0.05 * rng.random(n - o) for o in offs[1:]]
    A = sp.diags(bands + bands, offs + [-o for o in offs], format="csr")
    return sp.csr_matrix(A + sp.diags(np.asarray(abs(A).sum(axis=1)).ravel() + 0.01 + 0.05 * rng.random(n)))


def alt_operator(dims, eps=1e-2):
    return AT.split_anisotropy(*dims, eps) if len(dims) == 2 else LT.split_anisotropy3(*dims, eps)


def single_columns(mg, U0, F0, n):
    """tests/test_gpu_block.py's scheme: column j = the level-0 solution after set_vec(u, U0[:, j]),
    set_vec(f, F0[:, j]), vcycle(n)"""
    out = np.empty_like(U0)
    for j in range(U0.shape[1]):
        mg.set_vec(0, "u", U0[:, j])
        mg.set_vec(0, "f", F0[:, j])
        mg.vcycle(n)
        out[:, j] = mg.get_soln(0)
    return out


def check_block_equals_single(amg, build, graphs=(True, False), strides=None):
    """2 cycles on random U0, F0 of 16 columns; every k of K_ALL, every graph setting, bit for bit"""
    rng = np.random.default_rng(11)
    ref = build(graphs[0])
    if strides is not None:
        assert [ref.line_stride(l) for l in range(len(strides))] == list(strides)
    n0 = ref.get_n_dofs(0)
    U0 = rng.standard_normal((n0, 16))
    F0 = rng.standard_normal((n0, 16))
    want = single_columns(ref, U0, F0, 2)
    assert np.all(np.isfinite(want)) and not np.array_equal(want, U0)
    solvers = [ref] + [build(g) for g in graphs[1:]]
    for mg in solvers:
        for k in K_ALL:
            U = dev(U0[:, :k])
            mg.block_vcycles(U, dev(F0[:, :k]), n=2)
            torch.cuda.synchronize()
            got = U.cpu().numpy()
            for j in range(k):
                assert np.array_equal(got[:, j], want[:, j]), (k, j, float(np.abs(got[:, j] - want[:, j]).max()))
    for mg in solvers:
        mg.close()


# ---- AMG_HIP_SM_LINE_JACOBI, omega 0.7 ---------------------------------------------------------------
def _jac(iters, g):
    return dict(smoother=LINE, smoother_iters=iters, omega=0.7, use_graph=g)


@pytest.mark.parametrize("iters", [1, 2])
def test_line_jacobi_many_and_few_chains(amg, lines_on, iters):
    """poisson(300, 6): level 0 s = 300 (many chains) with 9 separators per chain, one more than a batch of
    the separator walk; the deeper levels s = 150, 75 (many) and 37, 19 (a workgroup per chain)"""
    check_block_equals_single(amg, lambda g: amg.Multigrid.poisson(300, 6, **_jac(iters, g)),
                              strides=(300, 150, 75, 37, 19))


@pytest.mark.parametrize("iters", [1, 2])
def test_line_jacobi_three_dimensions(amg, lines_on, iters):
    check_block_equals_single(amg, lambda g: amg.Multigrid.poisson(33, 4, dim=3, **_jac(iters, g)))


@pytest.mark.parametrize("n", [31, 32, 33])
@pytest.mark.parametrize("iters", [1, 2])
def test_line_jacobi_chains_around_one_separator(amg, lines_on, n, iters):
    """chains of 31, 32 and 33 rows: no separator, one in the last position, one row after it"""
    check_block_equals_single(amg, lambda g: amg.Multigrid.poisson(n, 2, **_jac(iters, g)), strides=(n,))


@pytest.mark.parametrize("n,s", [(40000, 1), (2 * 40000 + 1, 2)])
@pytest.mark.parametrize("iters", [1, 2])
def test_line_jacobi_long_chains_cross_the_lds_chunks(amg, lines_on, n, s, iters):
    """one and two chains of 1250 separators: more than one chunk of the LDS walk at every pitch (the chunk
    holds 1024 separators up to 4 columns, 512 at 8, 256 at 16), the carries cross the chunk ends"""
    assert (n // s) // 32 == 1250
    A = long_chains(n, s)
    b = np.ones(n)
    check_block_equals_single(amg, lambda g: amg.Multigrid(*csc(A), b, 2, **_jac(iters, g)), graphs=(True,),
                              strides=(s,))


# ---- AMG_HIP_SM_LINE_ALT, omega 0.8, tensor constructors ------------------------------------------------
ALT_CASES = {
    "64x48": ((64, 48), 4),       # nx = 64, 32, 16, 8: one chunk exactly, then 2, 4, 8 lines per run
    "33x20": ((33, 20), 3),       # odd nx
    "130x9": ((130, 9), 2),       # a run of three chunks' length; 9 runs: the last wave partly filled
    "1x40": ((1, 40), 2),         # no x direction; y lines of 40 rows: one separator
    "17x12x9": ((17, 12, 9), 3),  # x, y and z (stride nx ny)
}


@pytest.mark.parametrize("name", list(ALT_CASES))
@pytest.mark.parametrize("sym", ["symmetric", "nonsymmetric"])
@pytest.mark.parametrize("iters", [1, 2])
def test_line_alt(amg, lines_on, name, sym, iters):
    dims, levels = ALT_CASES[name]
    A = alt_operator(dims)
    if sym == "nonsymmetric":
        A = nonsym(A)
    b = np.ones(A.shape[0])
    kw = dict(smoother=ALT, smoother_iters=iters, omega=0.8)
    if dims[0] == 1:  # an axis of one point cannot be coarsened: the semi-coarsening constructor, y alone
        build = lambda g: amg.Multigrid.tensor_semi(*csc(A), b, dims, levels, axis_masks=(2,), use_graph=g, **kw)  # noqa: E731
    else:
        build = lambda g: amg.Multigrid.tensor(*csc(A), b, dims, levels, use_graph=g, **kw)  # noqa: E731
    check_block_equals_single(amg, build)


# ---- cyclic lines ------------------------------------------------------------------------------------
CYCLIC_CASES = {
    # smoothed levels 0 .. 3: x lines of 64, 32, 16, 8 rows (seam widths 64 .. 8); y lines of 48 .. 6, strided
    "64x48": ((64, 48), 5, 3, None),
    "16x12x8": ((16, 12, 8), 2, 4, None),  # z periodic: stride nx ny
    # the coarsest level takes no smoother, so the 4 x 3 grid is reached as a smoothed level here: level 1
    # (x alone is coarsened below it) has x lines of 4 rows (seam width 4) and y lines of 3, the shortest
    "8x6": ((8, 6), 3, 3, (3, 1)),
}


def cyclic_solver(amg, name, g, iters=1, **kw):
    dims, levels, per, masks = CYCLIC_CASES[name]
    A = PT.diffusion(dims, per, PT.open_sides(len(dims), per))
    b = np.ones(A.shape[0])
    return amg.Multigrid.tensor_periodic(*csc(A), b, dims, levels, per, axis_masks=masks, cyclic_lines=1,
                                         use_graph=g, smoother=ALT, smoother_iters=iters, omega=0.8, **kw)


@pytest.mark.parametrize("name", list(CYCLIC_CASES))
@pytest.mark.parametrize("iters", [1, 2])
def test_cyclic_lines(amg, lines_on, name, iters):
    dims, levels, per, _ = CYCLIC_CASES[name]
    probe = cyclic_solver(amg, name, True, iters)
    masks = [probe.line_cyclic(l) for l in range(levels - 1)]
    probe.close()
    assert all(m == per for m in masks), masks   # every smoothed level solves its periodic lines cyclically
    check_block_equals_single(amg, lambda g: cyclic_solver(amg, name, g, iters))


# ---- PCG, rss, state, refusal, bytes -------------------------------------------------------------------
def _alt_6448(amg, levels=4, eps=1e-3, **kw):
    A = alt_operator((64, 48), eps)
    kw = dict(dict(smoother=ALT, smoother_iters=1, omega=0.8), **kw)
    return amg.Multigrid.tensor(*csc(A), np.ones(A.shape[0]), (64, 48), levels, **kw)


def _jac_129(amg, **kw):
    return amg.Multigrid.poisson(129, 5, **dict(dict(smoother=LINE, smoother_iters=1, omega=0.7), **kw))


PCG_SOLVERS = {"line-alt-64x48": _alt_6448, "line-jacobi-129": _jac_129}


@pytest.mark.parametrize("name", list(PCG_SOLVERS))
def test_block_pcg_equals_pcg_per_column(amg, lines_on, name):
    """5 columns that stop at different iterations: a converged start, b, a small multiple of b from a
    random start, and two random right-hand sides"""
    rtol, max_iters = 1e-9, 60
    mg = PCG_SOLVERS[name](amg)
    n0 = mg.get_n_dofs(0)
    rng = np.random.default_rng(9)
    b0 = mg.get_rhs(0)
    mg.set_vec(0, "u", np.zeros(n0))
    xs, _, rel_s = mg.pcg(rtol, max_iters)
    assert rel_s <= rtol
    B0 = np.stack([b0, b0, 1e-6 * b0, rng.standard_normal(n0), rng.standard_normal(n0)], 1)
    X0 = np.zeros_like(B0)
    X0[:, 0] = xs
    X0[:, 2] = rng.standard_normal(n0)
    X = dev(X0)
    X, it, rel = mg.block_pcg(dev(B0), X, rtol=rtol, max_iters=max_iters)
    torch.cuda.synchronize()
    got = X.cpu().numpy()
    assert it[0] == 0
    for j in range(5):
        mg.set_vec(0, "f", B0[:, j])
        mg.set_vec(0, "u", X0[:, j])
        x, it_s, rel_s = mg.pcg(rtol, max_iters)
        print(f"{name} column {j}: {it_s} iterations, relres {rel_s:.3e}")
        assert it[j] == it_s, (j, it[j], it_s)
        assert rel[j] == rel_s, j
        assert rel_s <= rtol, j
        assert np.array_equal(got[:, j], x), j
    assert len(set(it.tolist())) > 1  # the columns really stopped at different times
    mg.close()


@pytest.mark.parametrize("name", list(PCG_SOLVERS))
def test_block_rss_equals_rss_per_column(amg, lines_on, name):
    mg = PCG_SOLVERS[name](amg)
    n0 = mg.get_n_dofs(0)
    rng = np.random.default_rng(4)
    U0, F0 = rng.standard_normal((n0, 5)), rng.standard_normal((n0, 5))
    got = mg.block_rss(dev(U0), dev(F0))
    for j in range(5):
        mg.set_vec(0, "u", U0[:, j])
        mg.set_vec(0, "f", F0[:, j])
        assert got[j] == mg.rss(), (name, j)
    mg.close()


@pytest.mark.parametrize("name", list(PCG_SOLVERS))
def test_block_calls_leave_the_solver_state_alone(amg, lines_on, name):
    mg, twin = PCG_SOLVERS[name](amg), PCG_SOLVERS[name](amg)
    mg.vcycle(2)
    twin.vcycle(2)
    u_before, f_before = mg.get_soln(0), mg.get_rhs(0)
    rng = np.random.default_rng(3)
    n0 = mg.get_n_dofs(0)
    U = dev(rng.standard_normal((n0, 5)))
    mg.block_vcycles(U, dev(rng.standard_normal((n0, 5))), n=2)
    mg.block_pcg(dev(rng.standard_normal((n0, 5))), rtol=1e-8, max_iters=20)
    mg.block_rss(U, dev(rng.standard_normal((n0, 5))))
    mg.block_must_move(5)
    assert np.array_equal(mg.get_soln(0), u_before)
    assert np.array_equal(mg.get_rhs(0), f_before)
    mg.vcycle()
    twin.vcycle()
    assert np.array_equal(mg.get_soln(0), twin.get_soln(0))
    mg.close()
    twin.close()


@pytest.mark.parametrize("name", list(PCG_SOLVERS))
def test_switch_off_a_device_solver_is_refused_and_unchanged(amg, name):
    amg.set_block_lines(0)
    mg = PCG_SOLVERS[name](amg)
    mg.vcycle()
    u, f = mg.get_soln(0), mg.get_rhs(0)
    n0 = mg.get_n_dofs(0)
    U, F = dev(np.ones((n0, 4))), dev(np.ones((n0, 4)))
    for call in (lambda: mg.block_vcycles(U, F), lambda: mg.block_rss(U, F), lambda: mg.block_pcg(F),
                 lambda: mg.block_must_move(4)):
        with pytest.raises(amg.AmgHipError) as e:
            call()
        assert e.value.status == amg.EUNSUPPORTED
        assert "is not supported (true Jacobi and Chebyshev are)" in e.value.message
    torch.cuda.synchronize()
    assert torch.equal(U, dev(np.ones((n0, 4))))
    assert np.array_equal(mg.get_soln(0), u) and np.array_equal(mg.get_rhs(0), f)
    mg.close()


def test_block_must_move_bytes(amg, lines_on):
    """64 x 48, 2 levels, k = 3, by hand.  Level 0: n = 3072 rows, 5 n - 2 (64 + 48) = 15136 entries, so the
    CSR rows are 12 * 15136 + 4 * 3073 B.  Each leg runs two sub-sweeps (x, y), each the residual (matrix;
    u, f, r: 24 n per column) and the line solve with every factor array counted once and every panel once
    per column:
      x, K-LineX: dl, ip, cp = 24 n; r in, y out, y, u in, u out = 40 n per column;
      y, K-Line with s = 64: chains of 48 rows have one separator (position 31), 64 separator rows; dl, ip,
         cp, v, w = 40 n; per column 40 B on the 3008 interior rows (r, y; y, u, u) and 56 B on the separator
         rows (r, both neighbours' y, y out; y, u, u).
    Everything else of the cycle is what a solver with smoother_iters = 0 moves."""
    k = 3
    mg, bare = _alt_6448(amg, levels=2), _alt_6448(amg, levels=2, smoother_iters=0)
    n, nnz, sep = 3072, 15136, 64
    assert mg.get_n_dofs(0) == n and int(amg.lib().amg_hip_get_level_nnz(mg._h, 0)) == nnz
    assert mg.line_directions(0) == [1, 64]
    csr = 12.0 * nnz + 4.0 * (n + 1)
    resid = csr + k * 24.0 * n
    x = 24.0 * n + k * 40.0 * n
    y = 40.0 * n + k * (40.0 * (n - sep) + 56.0 * sep)
    predicted = 2 * ((resid + x) + (resid + y))
    assert mg.block_must_move(k) - bare.block_must_move(k) == pytest.approx(predicted, rel=1e-12)
    mg.close()
    bare.close()
