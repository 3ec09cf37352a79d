"""Single-precision preconditioner on dictionary-coded levels (amg_hip_set_f32_dict; kernels.hip:
K-DictF32), behaviour: the refusal with the switch off and what the switch changes, amg_hip_pcg_mixed
against amg_hip_pcg, amg_hip_apply_f32 against a SELL solver of the same operator bit for bit, graph
against eager, that nothing else moves, amg_hip_f32_must_move against its formula, and the line smoothers
(amg_hip_set_f32_lines) on dictionary levels.  Tolerances are those of tests/test_gpu_mixed.py.
Cases: tests/dict_cases.py."""
import os
import sys

import numpy as np
import pytest

sp = pytest.importorskip("scipy.sparse")
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dict_cases as DC  # noqa: E402

pytestmark = pytest.mark.gpu

DICT, SELL = DC.DICT, DC.SELL
RTOL = 1e-8


@pytest.fixture(autouse=True)
def switches_off_again(amg):
    try:
        yield
    finally:
        amg.set_f32_dict(0)
        amg.set_f32_lines(0)
        amg.set_dict_rows(2)
        amg.set_row_types(1)


def _apply(mg, v, f32):
    dv = torch.from_numpy(np.array(v)).cuda()
    dz = torch.empty_like(dv)
    (mg.apply_f32 if f32 else mg.apply_dev)(dv.data_ptr(), dz.data_ptr())
    mg.sync()
    return dz.cpu().numpy()


def _layouts(mg):
    return [mg.level_layout(l)[0] for l in range(mg.n_levels - 1)]


def _build(amg, oracle, case, **kw):
    """the case's solver on the default layout, its layouts checked; (solver, level-0 matrix as CSR, b)"""
    mg = DC.make(amg, oracle, case, **kw)
    assert _layouts(mg) == DC.CASES[case]["layouts"], case
    A = sp.csr_matrix(DC.level_matrices(mg)[0][0])
    return mg, A, mg.get_rhs(0)


def _float_calls(mg):
    dv = torch.zeros(mg.get_n_dofs(0), dtype=torch.float64, device="cuda")
    return dv, (lambda: mg.apply_f32(dv.data_ptr(), dv.data_ptr()), lambda: mg.pcg_mixed(rtol=RTOL, max_iters=100),
                mg.f32_must_move)


def _refused(amg, mg):
    dv, calls = _float_calls(mg)
    for call in calls:
        with pytest.raises(amg.AmgHipError) as err:
            call()
        assert err.value.status == amg.EUNSUPPORTED
        assert "level 0" in str(err.value) and "AMG_HIP_LAYOUT_SELL" in str(err.value)


def _accepted(mg):
    dv, calls = _float_calls(mg)
    for call in calls:
        call()
    mg.sync()


def test_switch_off_a_dictionary_solver_is_refused(amg, oracle):
    mg, _, _ = _build(amg, oracle, "t33")
    u0 = mg.get_soln(0)
    _refused(amg, mg)
    mg.vcycle()  # the solver still works
    assert not np.array_equal(mg.get_soln(0), u0)
    mg.close()


def test_switch_on_the_same_calls_succeed(amg, oracle):
    mg, A, b = _build(amg, oracle, "t33")
    with amg.f32_dict():
        _accepted(mg)
        assert mg.f32_must_move() > 0
        z = _apply(mg, b, True)
    assert np.all(np.isfinite(z)) and np.linalg.norm(z) > 0
    mg.close()


def test_refused_first_then_accepted(amg, oracle):
    mg, _, _ = _build(amg, oracle, "t33")
    _refused(amg, mg)
    with amg.f32_dict():
        _accepted(mg)
    mg.close()


def test_accepted_first_then_switched_off(amg, oracle):
    mg, _, b = _build(amg, oracle, "t33")
    other, _, _ = _build(amg, oracle, "t33")
    with amg.f32_dict():
        z = _apply(mg, b, True)
    _accepted(mg)  # its float copies exist
    assert np.array_equal(_apply(mg, b, True), z)
    _refused(amg, other)  # a solver without them is refused as before
    mg.close()
    other.close()


@pytest.mark.parametrize("case", ["t33", "box", "per", "cheb2"])
def test_pcg_mixed_converges_like_pcg(amg, oracle, case):
    mg, A, b = _build(amg, oracle, case)
    bn = np.linalg.norm(b)
    x64, it64, _ = mg.pcg(rtol=RTOL, max_iters=100)
    mg.zero_vec(0, "u")
    with amg.f32_dict():
        x32, it32, rel32 = mg.pcg_mixed(rtol=RTOL, max_iters=100)
    true32 = float(np.linalg.norm(b - A @ x32) / bn)
    true64 = float(np.linalg.norm(b - A @ x64) / bn)
    print(f"mixed pcg on dictionary levels {case}: iterations {it64} (double cycle) {it32} (float cycle), true "
          f"residual {true64:.2e} / {true32:.2e}, recurrence {rel32:.2e}")
    assert 0 < it64 < 100
    assert abs(it32 - it64) <= 1
    assert true32 <= 2 * RTOL
    assert np.array_equal(mg.get_rhs(0), b)  # f is b again
    mg.close()


def test_apply_on_the_nonsymmetric_operator(amg, oracle):
    """CG needs symmetry, so nonsym compares one application: relative 2-norm distance from amg_hip_apply
    <= 1e-5 (test_gpu_mixed.py: test_apply_against_the_double_cycle)"""
    mg, A, b = _build(amg, oracle, "nonsym")
    with amg.f32_dict():
        z = _apply(mg, b, True)
    z64 = _apply(mg, b, False)
    rel = float(np.linalg.norm(z - z64) / np.linalg.norm(z64))
    print(f"mixed apply nonsym on dictionary levels: relative distance from amg_hip_apply {rel:.3e}")
    assert np.linalg.norm(z64) > 0
    assert rel <= 1e-5
    mg.close()


@pytest.mark.parametrize("case", ["t33", "box"])
def test_apply_has_the_bits_of_the_sell_solver(amg, oracle, case):
    """the layout does not change the float cycle: both are pinned to the same twin"""
    mg, A, b = _build(amg, oracle, case)
    sell = DC.CASES[case]["make"](amg, oracle, layout=SELL)
    assert _layouts(sell) == [SELL] * (sell.n_levels - 1)
    v = np.random.default_rng(7).standard_normal(b.size)
    with amg.f32_dict():
        z = _apply(mg, v, True)
    zs = _apply(sell, v, True)
    assert np.linalg.norm(z) > 0
    assert np.array_equal(z.view(np.uint64), zs.view(np.uint64))
    mg.close()
    sell.close()


def test_graph_and_eager_give_the_same_bits(amg, oracle):
    out = []
    with amg.f32_dict():
        for graph in (True, False):
            mg, A, b = _build(amg, oracle, "t33", use_graph=graph)
            z = _apply(mg, b, True)
            z2 = _apply(mg, b, True)  # the replayed graph
            assert np.array_equal(z, z2)
            out.append((z,) + mg.pcg_mixed(rtol=RTOL, max_iters=100))
            mg.close()
    assert np.array_equal(out[0][0], out[1][0])
    assert np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2] and out[0][3] == out[1][3]


@pytest.mark.parametrize("case", ["t33", "box", "cheb2"])
def test_nothing_else_moves(amg, oracle, case):
    """the solver's own vectors stay, and vcycle() / pcg() afterwards give a fresh solver's bits"""
    fresh, A, b = _build(amg, oracle, case)
    fresh.vcycle()
    want_u = fresh.get_soln(0)
    want_pcg = fresh.pcg(rtol=RTOL, max_iters=100)
    fresh.close()
    mg, _, _ = _build(amg, oracle, case)
    u0, f0 = mg.get_soln(0), mg.get_rhs(0)
    with amg.f32_dict():
        z = _apply(mg, 2.0 * b, True)
        assert np.linalg.norm(z) > 0
        assert np.array_equal(mg.get_soln(0), u0) and np.array_equal(mg.get_rhs(0), f0)
        mg.pcg_mixed(rtol=RTOL, max_iters=100)
    mg.set_vec(0, "u", u0)
    mg.vcycle()
    assert np.array_equal(mg.get_soln(0), want_u)
    got = mg.pcg(rtol=RTOL, max_iters=100)
    assert np.array_equal(got[0], want_pcg[0]) and got[1:] == want_pcg[1:]
    mg.close()


@pytest.mark.parametrize("case", ["t33", "box", "untyped", "cheb2", "nonsym"])
def test_must_move_is_the_formula(amg, oracle, case):
    """per launch the matrix and 4 bytes per row and vector (test_gpu_mixed.py: test_must_move_is_the_formula).
    A dictionary matrix: the double matrix's stream (amg_hip_level_layout) less 4 bytes per pair of its
    table, ntab recounted from the level matrix; the Jacobi sweep of a level that is not symmetric walks
    the transposed matrix's dictionary (the same row structure here, its own pairs)."""
    mg, _, _ = _build(amg, oracle, case)
    A = DC.level_matrices(mg)[0]
    nl = mg.n_levels
    n = [mg.get_n_dofs(l) for l in range(nl)]
    is_cheb = case == "cheb2"

    def mat(l, transposed=False):
        layout, stream = mg.level_layout(l)
        if layout == DICT:
            ntab = DC.pairs(A[l])
            assert ntab <= 255
            own = stream - 12 * ntab  # row types / code words and the word table
            return own + 8 * (DC.pairs(A[l].T) if transposed else ntab)
        assert layout == SELL
        panels = (n[l] + 63) // 64
        slots, rest = divmod(stream - 8 * panels, 10)
        assert rest == 0
        return slots * 6 + 8 * panels

    def smooth(l):
        if is_cheb:  # degree 2, one application: the first step writes d, the last reads it
            return 2 * (mat(l) + 12 * n[l]) + 8 * n[l]
        return 2 * (mat(l, transposed=(case == "nonsym")) + 12 * n[l])  # two sweeps: no copy home

    total = 4 * n[0] + 24 * n[0]  # the zero guess; v -> float and float -> z
    for l in range(nl - 1):
        total += 2 * smooth(l) + mat(l) + 12 * n[l]  # pre, post, residual
        assert mg.level_transfer_kind(l) == 2
        total += 4 * n[l] + 8 * n[l + 1]
        total += 4 * n[l + 1] + 8 * n[l]
    nc = n[-1]
    total += 24 * nc + 16 * nc * max(mg.coarse_halfbw(), 1) + 24 * nc
    with amg.f32_dict():
        assert mg.f32_must_move() == float(total)
    mg.close()


def _line_solver(amg, oracle, which):
    if which == "alt":
        A, b, dims = DC.operator("33x20")
        mg = amg.Multigrid.tensor_dev(*DC.csr(A), b.copy(), dims, 3, smoother=amg.SM_LINE_ALT, smoother_iters=1,
                                      omega=0.8)
        return mg, A, b
    Ao = oracle.laplacian(64)
    b = np.random.default_rng(7).standard_normal(64 * 64)
    mg = amg.Multigrid(Ao.colptr, Ao.rowind, Ao.val, b, 3, smoother=amg.SM_LINE_JACOBI, omega=0.7)
    return mg, sp.csr_matrix(DC.level_matrices(mg)[0][0]), b


@pytest.mark.parametrize("which", ["alt", "line"])
def test_both_switches_together(amg, oracle, which):
    """the float line smoothers take their residual through the same matrix launch: pcg_mixed within one
    iteration of pcg, one application within 1e-4 relative of amg_hip_apply (the upper end include/amg_hip.h
    documents for the float line cycle)"""
    mg, A, b = _line_solver(amg, oracle, which)
    assert _layouts(mg) == [DICT] * (mg.n_levels - 1)
    bn = np.linalg.norm(b)
    x64, it64, _ = mg.pcg(rtol=RTOL, max_iters=100)
    mg.zero_vec(0, "u")
    with amg.f32_lines():
        _refused(amg, mg)  # the lines alone do not lift the dictionary refusal
        with amg.f32_dict():
            x32, it32, rel32 = mg.pcg_mixed(rtol=RTOL, max_iters=100)
            z = _apply(mg, b, True)
    z64 = _apply(mg, b, False)
    rel = float(np.linalg.norm(z - z64) / np.linalg.norm(z64))
    true32 = float(np.linalg.norm(b - A @ x32) / bn)
    print(f"float lines on dictionary levels ({which}): iterations {it64} / {it32}, true residual {true32:.2e}, one "
          f"application {rel:.2e} from amg_hip_apply")
    assert 0 < it64 < 100 and abs(it32 - it64) <= 1
    assert true32 <= 2 * RTOL
    assert rel <= 1e-4
    mg.close()
