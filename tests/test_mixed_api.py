"""Single-precision preconditioner, the checks that need no GPU: the refusals of amg_hip_apply_f32 /
amg_hip_pcg_mixed / amg_hip_f32_must_move in the documented order on host_only solvers, the ctypes
signatures, and the property the feature rests on, pinned on the numpy twin: PCG preconditioned with
the float32 V-cycle converges like PCG preconditioned with the float64 one."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytest.importorskip("scipy.sparse")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mixed_twin as MT  # noqa: E402

PTR = 1 << 20  # never dereferenced: every call below is refused before any device work
JAC = dict(smoother_iters=2, omega=0.8)


def _host(amg, oracle, smoother, levels=3, **kw):
    A, b = oracle.laplacian(16), oracle.rhs(16)
    return amg.Multigrid(A.colptr, A.rowind, A.val, b, levels, smoother=smoother, host_only=True, **kw)


def _window(amg, smoother):
    return amg.Multigrid.poisson_window(64, 16, 48, 3, smoother=smoother, smoother_iters=1, omega=1.0,
                                        host_only=True)


def _calls(amg, mg):
    L = amg.lib()
    it, rel, by = C.c_int64(0), C.c_double(0), C.c_double(0)
    return {
        "apply_f32": lambda: L.amg_hip_apply_f32(mg._h, PTR, PTR),
        "pcg_mixed": lambda: L.amg_hip_pcg_mixed(mg._h, 1e-8, 10, C.byref(it), C.byref(rel)),
        "f32_must_move": lambda: L.amg_hip_f32_must_move(mg._h, C.byref(by)),
    }


def _err(amg):
    return amg.lib().amg_hip_last_error().decode()


def test_signatures(amg):
    L = amg.lib()
    assert L.amg_hip_apply_f32.restype is C.c_int
    assert L.amg_hip_apply_f32.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p]
    assert L.amg_hip_pcg_mixed.restype is C.c_int
    assert L.amg_hip_pcg_mixed.argtypes == L.amg_hip_pcg.argtypes
    assert L.amg_hip_f32_must_move.restype is C.c_int
    assert L.amg_hip_f32_must_move.argtypes == [C.c_void_p, amg._f64p]
    for name in ("apply_f32", "pcg_mixed", "f32_must_move"):
        assert callable(getattr(amg.Multigrid, name))


def test_null_pointers_and_bad_limits_come_first(amg):
    """EINVAL on a solver that every later check refuses too (window, SparseGaussSeidel)"""
    mg = _window(amg, amg.SM_SPGS)
    L = amg.lib()
    assert L.amg_hip_apply_f32(None, PTR, PTR) == amg.EINVAL
    assert L.amg_hip_apply_f32(mg._h, None, PTR) == amg.EINVAL
    assert L.amg_hip_apply_f32(mg._h, PTR, None) == amg.EINVAL
    assert L.amg_hip_pcg_mixed(None, 1e-8, 10, None, None) == amg.EINVAL
    assert L.amg_hip_f32_must_move(None, C.byref(C.c_double(0))) == amg.EINVAL
    assert L.amg_hip_f32_must_move(mg._h, None) == amg.EINVAL
    for rtol, iters in ((-1.0, 10), (float("nan"), 10), (1e-8, -1)):
        assert L.amg_hip_pcg_mixed(mg._h, rtol, iters, None, None) == amg.EINVAL
        assert "tolerance" in _err(amg)
    # ... and good arguments reach the next check
    assert L.amg_hip_pcg_mixed(mg._h, 1e-8, 10, None, None) == amg.EUNSUPPORTED
    mg.close()


def test_window_then_smoother_then_one_level_then_the_device(amg, oracle):
    mg = _window(amg, amg.SM_SPGS)  # window before the smoother
    for name, call in _calls(amg, mg).items():
        assert call() == amg.EUNSUPPORTED, name
        assert "window" in _err(amg), name
    mg.close()
    for sm, word in ((amg.SM_SPGS, "SparseGaussSeidel"), (amg.SM_SOR, "SOR"), (amg.SM_REF_JACOBI, "AMG::Jacobi"),
                     (amg.SM_MULTICOLOR_GS, "multicolour"), (amg.SM_LINE_JACOBI, "line Jacobi")):
        mg = _host(amg, oracle, sm, levels=1)  # the smoother before the one-level refusal
        for name, call in _calls(amg, mg).items():
            assert call() == amg.EUNSUPPORTED, (name, sm)
            assert word in _err(amg) and "is not supported (true Jacobi and Chebyshev are)" in _err(amg), (name, sm)
        mg.close()
    for sm in (amg.SM_JACOBI, amg.SM_CHEBYSHEV):
        mg = _host(amg, oracle, sm, levels=1, **JAC)  # one level before the device
        for name, call in _calls(amg, mg).items():
            assert call() == amg.EUNSUPPORTED, (name, sm)
            assert "one-level" in _err(amg), (name, sm)
        mg.close()
        mg = _host(amg, oracle, sm, levels=3, **JAC)  # then the device: host_only has none
        for name, call in _calls(amg, mg).items():
            assert call() == amg.EINVAL, (name, sm)
            assert "host_only" in _err(amg), (name, sm)
        mg.close()


@pytest.mark.parametrize("grid", ["33x20", "64x64", "17x12x9"])
def test_twin_pcg_converges_alike_with_the_float32_cycle(grid):
    """rtol 1e-8: iterations within +-1 of the float64 cycle's, true float64 residual <= rtol.
    Recorded on the twin: 33x20 7 / 7, 64x64 8 / 8, 17x12x9 8 / 8 iterations (float64 / float32 cycle),
    equal true residuals to three digits; one float32 cycle differs from the float64 cycle by 7.7e-8 ..
    9.0e-8 relative in the 2-norm."""
    rtol = 1e-8
    dims, levels, A, b, twin = MT.operator(grid)
    x64, it64, _ = MT.pcg(twin, b, rtol, np.float64)
    x32, it32, _ = MT.pcg(twin, b, rtol, np.float32)
    true32 = np.linalg.norm(b - A @ x32) / np.linalg.norm(b)
    true64 = np.linalg.norm(b - A @ x64) / np.linalg.norm(b)
    z64 = np.asarray(twin.vcycle(np.zeros(b.size), b)[0][0])
    z32 = np.asarray(twin.vcycle(np.zeros(b.size, np.float32), b.astype(np.float32), np.float32)[0][0], np.float64)
    print(f"twin {grid}: iterations float64 {it64} float32 {it32}, true residual {true64:.2e} / {true32:.2e}, "
          f"one cycle float32 against float64 {np.linalg.norm(z32 - z64) / np.linalg.norm(z64):.2e}")
    assert abs(it32 - it64) <= 1
    assert true32 <= rtol
    assert 0 < it64 < 30
