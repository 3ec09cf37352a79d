"""Single-precision preconditioner on the GPU (amg_hip_apply_f32, amg_hip_pcg_mixed,
amg_hip_f32_must_move; kernels.hip: K-F32).  Smallest shapes that reach every path: panels that do
not fill 64 rows, odd / even axis chains, a non-cubic 3-D box, 16- and 32-bit SELL indices, plain CSR
levels, the three transfer kinds, both smoothers, graph and eager.

Cases (every test runs the ones that apply to it):
  a33 / a64   Multigrid.tensor_dev 33x20 / 3 levels, Multigrid.tensor 64x64 / 5, variable-coefficient
              diffusion, true Jacobi 2+2 omega 0.8, layout SELL
  b           tensor_dev on the 3-D box 17x12x9 / 3 levels
  c33 / c64   a33 / a64 with amg_hip_set_index16(0) (32-bit SELL indices)
  d33 / d64   a33 / a64 with Chebyshev(2) 1+1
  k           d33 with layout CSR (the Chebyshev steps of the plain-CSR kernel)
  m           d33 with amg_hip_set_index16(0) (the Chebyshev steps on 32-bit SELL indices)
  e           amg_hip_create_rs on the 48^2 Laplacian, layout SELL (CSR transfers, kind 0)
  f           amg_hip_create on the 63^2 Laplacian, layout SELL, 3 levels (linear transfers, kind 1)
  g           a33 with layout CSR
  h           a33 with use_graph = 0 (against a33: same bits)
  i           a dictionary-coded solver: refused, the level in the message

Measured on an MI355X (largest ratio of the device's distance from the longdouble cycle to e32, the
float32 twin's distance; for e - g the relative distance from amg_hip_apply): see
profiles/mixed_config_bench.txt."""
import os
import sys

import numpy as np
import pytest

sp = pytest.importorskip("scipy.sparse")
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mixed_twin as MT  # noqa: E402
import tensor_twin as T  # noqa: E402

pytestmark = pytest.mark.gpu

JAC = dict(smoother=3, smoother_iters=2, omega=0.8)
CHEB = dict(smoother=5, smoother_iters=1, cheb_degree=2)
DICT, SELL, CSR = 3, 2, 1
RTOL = 1e-8


def _tensor(amg, grid, dev, **kw):
    dims, levels, A, b, _ = MT.operator(grid)
    if dev:
        return amg.Multigrid.tensor_dev(A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy(),
                                        b.copy(), dims, levels, **kw)
    Ac = A.tocsc()
    Ac.sort_indices()
    return amg.Multigrid.tensor(Ac.indptr.astype(np.int32), Ac.indices.astype(np.int32), Ac.data, b, dims, levels,
                                **kw)


def _laplacian(oracle, n):
    A = oracle.laplacian(n)
    return A, T.csr_of(A.colptr, A.rowind, A.val, n * n, n * n)


_RHS = {}


def _rhs(n):
    """seeded right-hand side, made once per size and never modified"""
    if n not in _RHS:
        _RHS[n] = np.random.default_rng(7).standard_normal(n)
        _RHS[n].setflags(write=False)
    return _RHS[n]


def build(amg, oracle, case):
    """(solver, A as scipy CSR, float64 twin or None, grid name or None).  The solver's right-hand side
    is the seeded vector of its size and its start vector zero."""
    grid = {"33": "33x20", "64": "64x64"}.get(case[1:], None)
    if case[0] in "acdghkm":
        grid = grid or "33x20"
        cheb = case[0] in "dkm"
        kw = dict(CHEB if cheb else JAC, layout=SELL)
        if case[0] in "gk":
            kw["layout"] = CSR
        if case[0] == "h":
            kw["use_graph"] = False
        if case[0] in "cm":
            amg.set_index16(0)
        try:
            mg = _tensor(amg, grid, dev=(grid == "33x20"), **kw)
        finally:
            amg.set_index16(1)  # the library's default; the switch has no getter
        A = MT.operator(grid)[2]
        twin = MT.cheb_twin(grid) if cheb else MT.operator(grid)[4]
    elif case == "b":
        grid = "17x12x9"
        mg = _tensor(amg, grid, dev=True, **dict(JAC, layout=SELL))
        A, twin = MT.operator(grid)[2], MT.operator(grid)[4]
    elif case == "e":
        Ao, A = _laplacian(oracle, 48)
        mg = amg.Multigrid.ruge_stueben(Ao.colptr, Ao.rowind, Ao.val, _rhs(48 * 48), min_coarse=100, layout=SELL,
                                        **JAC)
        twin = None
    elif case == "f":
        Ao, A = _laplacian(oracle, 63)
        mg = amg.Multigrid(Ao.colptr, Ao.rowind, Ao.val, _rhs(63 * 63), 3, layout=SELL, **JAC)
        twin = None
    else:
        raise KeyError(case)
    mg.set_vec(0, "f", _rhs(A.shape[0]))
    return mg, A, twin, grid


TENSOR = ["a33", "a64", "b", "c33", "c64", "d33", "d64", "k", "m"]
OWN = ["e", "f", "g"]


def _apply(mg, v, f32):
    dv = torch.from_numpy(np.array(v)).cuda()
    dz = torch.empty_like(dv)
    (mg.apply_f32 if f32 else mg.apply_dev)(dv.data_ptr(), dz.data_ptr())
    mg.sync()
    return dz.cpu().numpy()


@pytest.mark.parametrize("case", TENSOR)
def test_apply_against_the_twin(amg, oracle, case):
    """device within max(8 e32, 1e-6 ||z||) of the longdouble cycle, e32 = the float32 twin's distance"""
    mg, A, twin, _ = build(amg, oracle, case)
    v = _rhs(A.shape[0])
    z = _apply(mg, v, True)
    zero = np.zeros(v.size)
    ref = twin.vcycle(zero, v, np.longdouble)[0][0]
    z32 = twin.vcycle(zero.astype(np.float32), v.astype(np.float32), np.float32)[0][0]
    e32 = float(np.linalg.norm(np.asarray(z32, np.longdouble) - ref))
    dist = float(np.linalg.norm(np.asarray(z, np.longdouble) - ref))
    bound = max(8.0 * e32, 1e-6 * float(np.linalg.norm(z)))
    print(f"mixed apply {case}: distance {dist:.3e}, e32 {e32:.3e}, ratio {dist / e32:.2f}, bound {bound:.3e}")
    assert np.all(np.isfinite(z)) and np.linalg.norm(z) > 0
    assert dist <= bound
    mg.close()


@pytest.mark.parametrize("case", OWN)
def test_apply_against_the_double_cycle(amg, oracle, case):
    """no twin cycle for these hierarchies: relative 2-norm distance from amg_hip_apply <= 1e-5"""
    mg, A, _, _ = build(amg, oracle, case)
    v = _rhs(A.shape[0])
    z, z64 = _apply(mg, v, True), _apply(mg, v, False)
    rel = float(np.linalg.norm(z - z64) / np.linalg.norm(z64))
    print(f"mixed apply {case}: relative distance from amg_hip_apply {rel:.3e}")
    assert np.linalg.norm(z64) > 0
    assert rel <= 1e-5
    mg.close()


@pytest.mark.parametrize("case", TENSOR + OWN + ["h"])
def test_pcg_mixed_converges_like_pcg(amg, oracle, case):
    mg, A, _, _ = build(amg, oracle, case)
    b = _rhs(A.shape[0])
    bn = np.linalg.norm(b)
    x64, it64, _ = mg.pcg(rtol=RTOL, max_iters=100)
    mg.zero_vec(0, "u")
    x32, it32, rel32 = mg.pcg_mixed(rtol=RTOL, max_iters=100)
    true32 = float(np.linalg.norm(b - A @ x32) / bn)
    true64 = float(np.linalg.norm(b - A @ x64) / bn)
    print(f"mixed pcg {case}: iterations {it64} (double cycle) {it32} (float cycle), true residual "
          f"{true64:.2e} / {true32:.2e}, recurrence {rel32:.2e}")
    assert 0 < it64 < 100
    assert abs(it32 - it64) <= 1
    assert true32 <= 2 * RTOL
    assert np.array_equal(mg.get_rhs(0), b)  # f is b again
    mg.close()


@pytest.mark.parametrize("case", ["a33", "a64"])
def test_pcg_mixed_keeps_double_accuracy(amg, oracle, case):
    """rtol 1e-12: the true float64 residual ends <= 1e-11"""
    mg, A, _, _ = build(amg, oracle, case)
    b = _rhs(A.shape[0])
    x, it, rel = mg.pcg_mixed(rtol=1e-12, max_iters=100)
    true = float(np.linalg.norm(b - A @ x) / np.linalg.norm(b))
    print(f"mixed pcg {case} rtol 1e-12: {it} iterations, true residual {true:.2e}, recurrence {rel:.2e}")
    assert rel <= 1e-12 and true <= 1e-11
    mg.close()


def test_graph_and_eager_give_the_same_bits(amg, oracle):
    out = []
    for case in ("a33", "h"):
        mg, A, _, _ = build(amg, oracle, case)
        v = _rhs(A.shape[0])
        z = _apply(mg, v, True)
        z2 = _apply(mg, v, True)  # the replayed graph
        assert np.array_equal(z, z2)
        out.append((z,) + mg.pcg_mixed(rtol=RTOL, max_iters=100))
        mg.close()
    assert np.array_equal(out[0][0], out[1][0])
    assert np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2] and out[0][3] == out[1][3]


@pytest.mark.parametrize("case", TENSOR + OWN + ["h"])
def test_nothing_else_moves(amg, oracle, case):
    """the solver's own vectors stay, and vcycle() / pcg() afterwards give a fresh solver's bits"""
    fresh, A, _, _ = build(amg, oracle, case)
    fresh.vcycle()
    want_u = fresh.get_soln(0)
    want_pcg = fresh.pcg(rtol=RTOL, max_iters=100)
    fresh.close()
    mg, _, _, _ = build(amg, oracle, case)
    u0, f0 = mg.get_soln(0), mg.get_rhs(0)
    z = _apply(mg, 2.0 * _rhs(A.shape[0]), True)
    assert np.linalg.norm(z) > 0
    assert np.array_equal(mg.get_soln(0), u0) and np.array_equal(mg.get_rhs(0), f0)
    mg.pcg_mixed(rtol=RTOL, max_iters=100)
    mg.set_vec(0, "u", u0)
    mg.vcycle()
    assert np.array_equal(mg.get_soln(0), want_u)
    got = mg.pcg(rtol=RTOL, max_iters=100)
    assert np.array_equal(got[0], want_pcg[0]) and got[1:] == want_pcg[1:]
    mg.close()


@pytest.mark.parametrize("case", TENSOR + OWN)
def test_must_move_is_the_formula(amg, oracle, case):
    """DESIGN.md "Single-precision preconditioner": per launch the matrix (SELL: 4 + w bytes per entry, w
    = 2 or 4, and 8 per panel; CSR: 8 per entry and 4 per row pointer) and 4 bytes per row and vector."""
    mg, A, _, _ = build(amg, oracle, case)
    nl = mg.n_levels
    n = [mg.get_n_dofs(l) for l in range(nl)]
    w = 4 if case[0] in "cm" else 2
    cheb = case[0] in "dkm"

    def mat(l):
        layout, stream = mg.level_layout(l)
        assert layout in (SELL, CSR)
        if layout == SELL:
            panels = (n[l] + 63) // 64
            slots, rest = divmod(stream - 8 * panels, 8 + w)
            assert rest == 0
            return slots * (4 + w) + 8 * panels
        nnz, rest = divmod(stream - 4 * (n[l] + 1), 12)
        assert rest == 0
        return 8 * nnz + 4 * (n[l] + 1)

    def smooth(l):
        if cheb:  # degree 2, one application: the first step writes d, the last reads it
            return 2 * (mat(l) + 12 * n[l]) + 8 * n[l]
        return 2 * (mat(l) + 12 * n[l])  # two sweeps, an even count: no copy home

    total = 4 * n[0] + 24 * n[0]  # the zero guess; v -> float and float -> z
    for l in range(nl - 1):
        total += 2 * smooth(l) + mat(l) + 12 * n[l]  # pre, post, residual
        kind = mg.level_transfer_kind(l)
        if kind == 0:
            nnz_p, nnz_r = mg.get_transfer(l, "P")[1].size, mg.get_transfer(l, "R")[1].size
            total += 8 * nnz_r + 4 * (n[l + 1] + 1) + 4 * n[l] + 8 * n[l + 1]
            total += 8 * nnz_p + 4 * (n[l] + 1) + 4 * n[l + 1] + 8 * n[l]
        else:
            total += 4 * n[l] + 8 * n[l + 1]
            total += 4 * n[l + 1] + 8 * n[l]
    nc = n[-1]
    # f_L widened, the double solve (band of L twice, D, f, u), u_L rounded
    total += 24 * nc + 16 * nc * max(mg.coarse_halfbw(), 1) + 24 * nc
    assert mg.f32_must_move() == float(total)
    mg.close()


def test_a_dictionary_level_is_refused(amg, oracle):
    Ao, _ = _laplacian(oracle, 64)
    mg = amg.Multigrid(Ao.colptr, Ao.rowind, Ao.val, oracle.rhs(64), 3, layout=DICT, **JAC)
    assert mg.level_layout(0)[0] == DICT
    u0 = mg.get_soln(0)
    dv = torch.zeros(64 * 64, dtype=torch.float64, device="cuda")
    for call in (lambda: mg.apply_f32(dv.data_ptr(), dv.data_ptr()), mg.pcg_mixed, mg.f32_must_move):
        with pytest.raises(amg.AmgHipError) as err:
            call()
        assert err.value.status == amg.EUNSUPPORTED
        assert "level 0" in str(err.value) and "AMG_HIP_LAYOUT_SELL" in str(err.value)
    mg.vcycle()  # the solver still works
    assert not np.array_equal(mg.get_soln(0), u0)
    mg.close()
