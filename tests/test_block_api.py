"""Block (multi-right-hand-side) entry points, the checks that need no GPU: argument refusals
in the documented order (EINVAL, then EUNSUPPORTED, then the device), and the torch-facing
wrappers' ValueErrors before any block call reaches C."""
import ctypes as C

import numpy as np
import pytest


def _host_solver(amg, oracle, smoother, **kw):
    A, b = oracle.laplacian(16), oracle.rhs(16)
    return amg.Multigrid(A.colptr, A.rowind, A.val, b, 3, smoother=smoother, host_only=True, **kw)


def _calls(amg, mg, k, p_f, p_u):
    """every block entry point with k columns and the two device pointers (ints or None)"""
    L = amg.lib()
    out = np.zeros(16, np.float64)
    it = np.zeros(16, np.int64)
    b = C.c_double(0)
    return {
        "vcycles": lambda: L.amg_hip_block_vcycles(mg._h, k, p_f, p_u, 1),
        "rss": lambda: L.amg_hip_block_rss(mg._h, k, p_f, p_u, amg._p64(out)),
        "pcg": lambda: L.amg_hip_block_pcg(mg._h, k, p_f, p_u, 1e-8, 10, it.ctypes.data_as(amg._i64p),
                                          amg._p64(out)),
        "must_move": lambda: L.amg_hip_block_must_move(mg._h, k, C.byref(b)),
    }


ALIGNED = 1 << 20  # never dereferenced: every call below is refused before any device work


def test_block_entry_points_refuse_bad_k_and_null_pointers(amg, oracle):
    mg = _host_solver(amg, oracle, amg.SM_JACOBI, smoother_iters=2, omega=0.6)
    for k in (0, 17, -1):
        for name, call in _calls(amg, mg, k, ALIGNED, ALIGNED).items():
            assert call() == amg.EINVAL, (name, k)
            assert "k must be in 1 .. 16" in amg.lib().amg_hip_last_error().decode()
    for name, call in _calls(amg, mg, 4, None, ALIGNED).items():
        if name != "must_move":
            assert call() == amg.EINVAL, name
    for name, call in _calls(amg, mg, 4, ALIGNED, None).items():
        if name != "must_move":
            assert call() == amg.EINVAL, name
    L = amg.lib()
    assert L.amg_hip_block_vcycles(None, 4, ALIGNED, ALIGNED, 1) == amg.EINVAL
    assert L.amg_hip_block_must_move(mg._h, 4, None) == amg.EINVAL
    assert L.amg_hip_block_vcycles(mg._h, 4, ALIGNED, ALIGNED, -1) == amg.EINVAL
    assert L.amg_hip_block_vcycles(mg._h, 4, ALIGNED + 8, ALIGNED, 1) == amg.EINVAL
    assert "aligned" in L.amg_hip_last_error().decode()
    assert L.amg_hip_block_pcg(mg._h, 4, ALIGNED, ALIGNED, -1.0, 10, None, None) == amg.EINVAL
    assert L.amg_hip_block_pcg(mg._h, 4, ALIGNED, ALIGNED, 1e-8, -1, None, None) == amg.EINVAL
    mg.close()


def test_block_entry_points_refuse_lexicographic_smoothers_before_the_device(amg, oracle):
    """EUNSUPPORTED comes before the device check: a host_only SpGS solver says so."""
    for sm, word in ((amg.SM_SPGS, "SparseGaussSeidel"), (amg.SM_SOR, "SOR"),
                     (amg.SM_REF_JACOBI, "AMG::Jacobi")):
        mg = _host_solver(amg, oracle, sm)
        for name, call in _calls(amg, mg, 4, ALIGNED, ALIGNED).items():
            assert call() == amg.EUNSUPPORTED, (name, sm)
            assert word in amg.lib().amg_hip_last_error().decode()
        # EINVAL still comes first
        assert _calls(amg, mg, 17, ALIGNED, ALIGNED)["vcycles"]() == amg.EINVAL
        mg.close()


@pytest.mark.parametrize("smoother", ["jacobi", "chebyshev"])
def test_block_entry_points_fail_on_a_host_only_solver(amg, oracle, smoother):
    sm = amg.SM_JACOBI if smoother == "jacobi" else amg.SM_CHEBYSHEV
    mg = _host_solver(amg, oracle, sm, smoother_iters=2, omega=0.6)
    for name, call in _calls(amg, mg, 3, ALIGNED, ALIGNED).items():
        assert call() == amg.EINVAL, name
        assert "host_only" in amg.lib().amg_hip_last_error().decode(), name
    mg.close()


def test_block_wrappers_check_tensors_in_python(amg, oracle):
    torch = pytest.importorskip("torch")
    mg = _host_solver(amg, oracle, amg.SM_JACOBI, smoother_iters=2, omega=0.6)
    n = mg.get_n_dofs(0)
    good = torch.zeros(n, 4, dtype=torch.float64)
    bad = {
        "shape": torch.zeros(n + 1, 4, dtype=torch.float64),
        "1-d": torch.zeros(n, dtype=torch.float64),
        "k=17": torch.zeros(n, 17, dtype=torch.float64),
        "dtype": torch.zeros(n, 4, dtype=torch.float32),
        "strides": torch.zeros(4, n, dtype=torch.float64).t(),
        "numpy": np.zeros((n, 4)),
    }
    for what, t in bad.items():
        with pytest.raises(ValueError):
            mg.block_vcycles(t, good)
        with pytest.raises(ValueError):
            mg.block_vcycles(good, t)
        with pytest.raises(ValueError):
            mg.block_rss(t, good)
        with pytest.raises(ValueError):
            mg.block_pcg(t)
    with pytest.raises(ValueError, match="shape"):  # F must have U's k
        mg.block_vcycles(good, torch.zeros(n, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="device"):  # a host tensor is not on the solver's device
        mg.block_vcycles(good, good)
    mg.close()
