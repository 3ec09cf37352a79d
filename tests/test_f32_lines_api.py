"""Single-precision line smoothers (amg_hip_set_f32_lines), the checks that need no GPU: with the switch
off the float entry points refuse line-smoother solvers exactly as before; with it on the smoother check
lets AMG_HIP_SM_LINE_JACOBI and AMG_HIP_SM_LINE_ALT through to the next checks in the documented order
(window, smoother, one-level, the device); the two new hooks check their arguments first; and the property
the feature rests on, pinned on the numpy twin (tests/f32_line_twin.py): PCG preconditioned with the
float32 alternating-line cycle converges like PCG preconditioned with the float64 one."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sp = pytest.importorskip("scipy.sparse")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import f32_line_twin as LT  # noqa: E402
import line_alt_twin as AT  # noqa: E402
import mixed_twin as MT  # noqa: E402
import tensor_twin as T  # noqa: E402
from test_line_alt import laplacian  # noqa: E402

PTR = 1 << 20  # never dereferenced: every call below is refused before any device work
ALT = dict(smoother=7, smoother_iters=1, omega=0.8, host_only=True)
OLD = "is not supported (true Jacobi and Chebyshev are)"


@pytest.fixture
def lines_on(amg):
    amg.set_f32_lines(1)
    yield
    amg.set_f32_lines(0)


def _alt(amg, levels=2):
    A, b = laplacian((12, 10))
    return amg.Multigrid.tensor(*A, b, (12, 10), levels, **ALT)


def _jacobi(amg, oracle, levels=3):
    A, b = oracle.laplacian(16), oracle.rhs(16)
    return amg.Multigrid(A.colptr, A.rowind, A.val, b, levels, smoother=amg.SM_LINE_JACOBI, omega=0.7, host_only=True)


def _calls(amg, mg):
    L = amg.lib()
    it, rel, by = C.c_int64(0), C.c_double(0), C.c_double(0)
    buf = (C.c_float * 4)()
    return {
        "apply_f32": lambda: L.amg_hip_apply_f32(mg._h, PTR, PTR),
        "pcg_mixed": lambda: L.amg_hip_pcg_mixed(mg._h, 1e-8, 10, C.byref(it), C.byref(rel)),
        "f32_must_move": lambda: L.amg_hip_f32_must_move(mg._h, C.byref(by)),
        "f32_line_subsweep": lambda: L.amg_hip_f32_line_subsweep(mg._h, 0, 0, 0),
        "f32_line_factors": lambda: L.amg_hip_f32_line_factors(mg._h, 0, buf, buf, buf),
    }


def _err(amg):
    return amg.lib().amg_hip_last_error().decode()


def test_symbols_and_helpers(amg):
    L = amg.lib()
    assert L.amg_hip_set_f32_lines.restype is None and L.amg_hip_set_f32_lines.argtypes == [C.c_int32]
    assert L.amg_hip_f32_line_subsweep.argtypes == [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
    assert L.amg_hip_f32_line_factors.argtypes == [C.c_void_p, C.c_int32] + [C.POINTER(C.c_float)] * 3
    with open(os.path.join(os.path.dirname(__file__), "..", "include", "amg_hip.h")) as h:
        assert "void amg_hip_set_f32_lines(int32_t on);" in h.read()
    for name in ("f32_line_subsweep", "f32_line_factors"):
        assert callable(getattr(amg.Multigrid, name))
    mg = _alt(amg)
    try:
        with amg.f32_lines():                  # the context helper turns it on ...
            assert _calls(amg, mg)["apply_f32"]() == amg.EINVAL
        assert _calls(amg, mg)["apply_f32"]() == amg.EUNSUPPORTED   # ... and off again
    finally:
        amg.set_f32_lines(0)
        mg.close()


def test_switch_off_the_refusals_are_todays(amg, oracle):
    for mg, word in ((_alt(amg), "alternating"), (_jacobi(amg, oracle), "line Jacobi")):
        for name, call in _calls(amg, mg).items():
            assert call() == amg.EUNSUPPORTED, name
            assert OLD in _err(amg), (name, _err(amg))
        print(f"switch off, {word}: {_err(amg)}")
        mg.close()


def test_switch_on_host_only_line_solvers_reach_the_device_check(amg, oracle, lines_on):
    for mg in (_alt(amg), _jacobi(amg, oracle)):
        for name, call in _calls(amg, mg).items():
            assert call() == amg.EINVAL, (name, _err(amg))
            assert "host_only" in _err(amg), (name, _err(amg))
        mg.close()


def test_switch_on_the_order_of_the_checks(amg, oracle, lines_on):
    mg = amg.Multigrid.poisson_window(64, 16, 48, 3, smoother=amg.SM_SPGS, smoother_iters=1, omega=1.0,
                                      host_only=True)
    for name, call in _calls(amg, mg).items():  # a window solver first
        assert call() == amg.EUNSUPPORTED, name
        assert "window" in _err(amg), name
    mg.close()
    A, b = oracle.laplacian(16), oracle.rhs(16)   # then the smoother; its message lists the line smoothers
    mg = amg.Multigrid(A.colptr, A.rowind, A.val, b, 1, smoother=amg.SM_SPGS, host_only=True)
    for name, call in _calls(amg, mg).items():
        assert call() == amg.EUNSUPPORTED, name
        msg = _err(amg)
        assert "SparseGaussSeidel" in msg and "AMG_HIP_SM_LINE_JACOBI" in msg and "AMG_HIP_SM_LINE_ALT" in msg, msg
    mg.close()
    for mg in (_alt(amg, levels=1), _jacobi(amg, oracle, levels=1)):   # then one level, before the device
        for name, call in _calls(amg, mg).items():
            assert call() == amg.EUNSUPPORTED, name
            assert "one-level" in _err(amg), (name, _err(amg))
        mg.close()


def test_the_hooks_check_their_arguments_first(amg, lines_on):
    L = amg.lib()
    mg = _alt(amg)
    buf = (C.c_float * 4)()
    assert L.amg_hip_f32_line_subsweep(None, 0, 0, 0) == amg.EINVAL
    assert L.amg_hip_f32_line_factors(None, 0, buf, buf, buf) == amg.EINVAL
    for args in ((None, buf, buf), (buf, None, buf), (buf, buf, None)):
        assert L.amg_hip_f32_line_factors(mg._h, 0, *args) == amg.EINVAL
        assert "null" in _err(amg)
    for d in (-1, 3):
        assert L.amg_hip_f32_line_subsweep(mg._h, 0, d, 0) == amg.EINVAL
        assert "direction" in _err(amg)
    for level in (-1, 2):
        assert L.amg_hip_f32_line_subsweep(mg._h, level, 0, 0) == amg.EINVAL
        assert L.amg_hip_f32_line_factors(mg._h, level, buf, buf, buf) == amg.EINVAL
        assert "level out of range" in _err(amg)
    amg.set_f32_lines(0)                       # bad arguments come before the smoother check as well
    assert L.amg_hip_f32_line_subsweep(mg._h, 0, 3, 0) == amg.EINVAL
    assert L.amg_hip_f32_line_subsweep(mg._h, 0, 0, 0) == amg.EUNSUPPORTED
    mg.close()


def test_the_twins_float32_walk_is_the_plain_loop():
    """f32_line_twin.walk against a scalar np.float32 loop, and the float64 factors against Thomas."""
    rng = np.random.default_rng(1)
    A = AT.split_anisotropy(9, 5, 1e-2)
    D = LT.Direction(A, 1, 9)
    dl64, dd64, du64 = AT.tridiagonal_part(A, 1, 9)
    dl, ip, cp = D.factors32()
    carry = 0.0
    for i in range(45):                        # the flat sequential elimination: dl = 0 restarts every line
        piv = dd64[i] - dl64[i] * carry
        carry = du64[i] * (1.0 / piv)
        assert D.factors[1][i] == 1.0 / piv and D.factors[2][i] == carry
    r = rng.standard_normal(45).astype(np.float32)
    x, y, _ = D.solve32(r)
    F = np.float32
    yy, xx = np.zeros(45, F), np.zeros(45, F)
    prev = F(0)
    for i in range(45):
        prev = F(F(r[i] - F(dl[i] * prev)) * ip[i])
        yy[i] = prev
    nxt = F(0)
    for i in range(44, -1, -1):
        nxt = F(yy[i] - F(cp[i] * nxt))
        xx[i] = nxt
    assert np.array_equal(y.view(np.uint32), yy.view(np.uint32))
    assert np.array_equal(x.view(np.uint32), xx.view(np.uint32))
    exact = D.solve_ld(r.astype(np.longdouble))
    assert np.linalg.norm(x - exact) <= 1e-5 * np.linalg.norm(exact)
    assert (LT.diffusion((9, 5), (np.ones((5, 9)), np.full((5, 9), 0.5))) !=
            AT.diffusion(9, 5, np.ones((5, 9)), np.full((5, 9), 0.5))).nnz == 0


CASES = {"64x48": ((64, 48), 4, 1e-3), "33x20": ((33, 20), 3, 1e-2), "17x12x9": ((17, 12, 9), 3, 1e-2)}


@pytest.mark.parametrize("case", sorted(CASES))
def test_twin_pcg_converges_alike_with_the_float32_line_cycle(case):
    """rtol 1e-8, one alternating line application per leg, omega 0.8, random b of seed 99: iterations
    within +-1 of the float64 cycle's, true float64 residual <= rtol.  Recorded on the twin: 6 / 6
    iterations (float64 / float32 cycle) on all three."""
    rtol = 1e-8
    dims, levels, eps = CASES[case]
    A = AT.split_anisotropy(*dims, eps) if len(dims) == 2 else LT.split_anisotropy3(*dims, eps)
    b = np.random.default_rng(99).standard_normal(A.shape[0])
    cyc = LT.Cycle(T.Twin(A, dims, levels), "alt", 0.8, 1)
    x64, it64, _ = MT.pcg(cyc, b, rtol, np.float64)
    x32, it32, _ = MT.pcg(cyc, b, rtol, np.float32)
    true32 = np.linalg.norm(b - A @ x32) / np.linalg.norm(b)
    true64 = np.linalg.norm(b - A @ x64) / np.linalg.norm(b)
    z64 = np.asarray(cyc.vcycle(np.zeros(b.size), b)[0][0])
    z32 = np.asarray(cyc.vcycle(np.zeros(b.size, np.float32), b.astype(np.float32), np.float32)[0][0], np.float64)
    print(f"twin {case} eps {eps}: iterations float64 {it64} float32 {it32}, true residual {true64:.2e} / "
          f"{true32:.2e}, one cycle float32 against float64 {np.linalg.norm(z32 - z64) / np.linalg.norm(z64):.2e}")
    assert abs(it32 - it64) <= 1
    assert true32 <= rtol
    assert 0 < it64 < 30
