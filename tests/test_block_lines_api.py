"""Block cycles with the line smoothers (amg_hip_set_block_lines), the checks that need no GPU: with the
switch off the four block entry points refuse line-smoother solvers exactly as before; with it on the
smoother check lets AMG_HIP_SM_LINE_JACOBI and AMG_HIP_SM_LINE_ALT (cyclic lines included) through to the
device check, and every other check keeps its place in the documented order (null pointers, k, n_cycles,
alignment, rtol / max_iters, window, smoother, the device).  Every solver is host_only and no pointer is
ever dereferenced."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sp = pytest.importorskip("scipy.sparse")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import periodic_twin as PT  # noqa: E402
from test_line_alt import laplacian  # noqa: E402

PTR = 1 << 20  # 16-byte aligned, never dereferenced: every call below is refused before any device work
ALT = dict(smoother=7, smoother_iters=1, omega=0.8, host_only=True)
OLD = "is not supported (true Jacobi and Chebyshev are)"


@pytest.fixture
def lines_on(amg):
    amg.set_block_lines(1)
    yield
    amg.set_block_lines(0)


def _alt(amg, levels=2):
    A, b = laplacian((12, 10))
    return amg.Multigrid.tensor(*A, b, (12, 10), levels, **ALT)


def _jacobi(amg, oracle, levels=3):
    A, b = oracle.laplacian(16), oracle.rhs(16)
    return amg.Multigrid(A.colptr, A.rowind, A.val, b, levels, smoother=amg.SM_LINE_JACOBI, omega=0.7, host_only=True)


def _cyclic(amg):
    dims, per = (12, 10), 1
    A = sp.csc_matrix(PT.diffusion(dims, per, PT.open_sides(2, per)))
    A.sort_indices()
    return amg.Multigrid.tensor_periodic(A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy(),
                                         np.ones(A.shape[0]), dims, 2, per, cyclic_lines=1, **ALT)


def _calls(amg, mg, k=4, F=PTR, U=PTR, rtol=1e-8, n_cycles=1):
    L = amg.lib()
    out = (C.c_double * 16)()
    it = (C.c_int64 * 16)()
    by = C.c_double(0)
    h = mg._h if mg is not None else None
    return {
        "block_vcycles": lambda: L.amg_hip_block_vcycles(h, k, F, U, n_cycles),
        "block_rss": lambda: L.amg_hip_block_rss(h, k, F, U, out),
        "block_pcg": lambda: L.amg_hip_block_pcg(h, k, F, U, rtol, 10, it, out),
        "block_must_move": lambda: L.amg_hip_block_must_move(h, k, C.byref(by)),
    }


def _err(amg):
    return amg.lib().amg_hip_last_error().decode()


def test_symbol_header_and_helper(amg):
    L = amg.lib()
    assert L.amg_hip_set_block_lines.restype is None and L.amg_hip_set_block_lines.argtypes == [C.c_int32]
    with open(os.path.join(os.path.dirname(__file__), "..", "include", "amg_hip.h")) as h:
        assert "void amg_hip_set_block_lines(int32_t on);" in h.read()
    mg = _alt(amg)
    try:
        with amg.block_lines():                # the context helper turns it on ...
            assert _calls(amg, mg)["block_must_move"]() == amg.EINVAL
            assert "host_only" in _err(amg)
        assert _calls(amg, mg)["block_must_move"]() == amg.EUNSUPPORTED   # ... and off again
    finally:
        amg.set_block_lines(0)
        mg.close()


def test_switch_off_the_refusals_are_todays(amg, oracle):
    amg.set_block_lines(0)
    for mg, word in ((_alt(amg), "alternating line Jacobi (AMG_HIP_SM_LINE_ALT)"),
                     (_jacobi(amg, oracle), "line Jacobi (AMG_HIP_SM_LINE_JACOBI)")):
        for name, call in _calls(amg, mg).items():
            assert call() == amg.EUNSUPPORTED, name
            assert _err(amg).endswith("block cycles: the smoother " + word + " " + OLD), (name, _err(amg))
        mg.close()


def test_switch_on_host_only_line_solvers_reach_the_device_check(amg, oracle, lines_on):
    for mg in (_alt(amg), _jacobi(amg, oracle), _cyclic(amg)):
        for name, call in _calls(amg, mg).items():
            assert call() == amg.EINVAL, (name, _err(amg))
            assert "host_only" in _err(amg), (name, _err(amg))
        mg.close()


def test_switch_on_the_argument_checks_still_come_first(amg, oracle, lines_on):
    for mg in (_alt(amg), _jacobi(amg, oracle)):
        for k in (0, 17):                      # bad k
            for name, call in _calls(amg, mg, k=k).items():
                assert call() == amg.EINVAL, name
                assert "k must be in 1 .. 16" in _err(amg), (name, _err(amg))
        for name, call in _calls(amg, mg, F=None).items():   # null pointers
            if name != "block_must_move":
                assert call() == amg.EINVAL, name
                assert "null" in _err(amg), (name, _err(amg))
        for name, call in _calls(amg, None).items():
            assert call() == amg.EINVAL, name
            assert "null" in _err(amg), (name, _err(amg))
        for name, call in _calls(amg, mg, U=PTR + 8).items():  # 8 bytes off a 16-byte boundary
            if name != "block_must_move":
                assert call() == amg.EINVAL, name
                assert "16-byte aligned" in _err(amg), (name, _err(amg))
        assert _calls(amg, mg, n_cycles=-1)["block_vcycles"]() == amg.EINVAL
        assert "n_cycles" in _err(amg)
        assert _calls(amg, mg, rtol=-1.0)["block_pcg"]() == amg.EINVAL
        assert "tolerance" in _err(amg)
        mg.close()


def test_switch_on_window_and_other_smoothers_are_still_refused(amg, oracle, lines_on):
    mg = amg.Multigrid.poisson_window(64, 16, 48, 3, smoother=amg.SM_SPGS, smoother_iters=1, omega=1.0,
                                      host_only=True)
    for name, call in _calls(amg, mg).items():  # a window solver first
        assert call() == amg.EUNSUPPORTED, name
        assert "window" in _err(amg), name
    mg.close()
    A, b = oracle.laplacian(16), oracle.rhs(16)   # then the smoother; its message names the line smoothers
    mg = amg.Multigrid(A.colptr, A.rowind, A.val, b, 2, smoother=amg.SM_SPGS, host_only=True)
    for name, call in _calls(amg, mg).items():
        assert call() == amg.EUNSUPPORTED, name
        msg = _err(amg)
        assert "SparseGaussSeidel" in msg and "AMG_HIP_SM_LINE_JACOBI" in msg and "AMG_HIP_SM_LINE_ALT" in msg, msg
    amg.set_block_lines(0)                        # and with the switch off it is today's text
    for name, call in _calls(amg, mg).items():
        assert call() == amg.EUNSUPPORTED, name
        assert OLD in _err(amg), (name, _err(amg))
    mg.close()
