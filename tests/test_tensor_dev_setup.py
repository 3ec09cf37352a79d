"""amg_hip_create_tensor_dev / Multigrid.tensor_dev, the parts that need no GPU: the exported symbol
and its binding, every argument error (checked before the device is touched: the "device pointers"
here are small integers that must never be dereferenced), the refusal without a device, and the
ValueErrors of the Python wrapper for arrays of the wrong kind."""
import ctypes as C
import subprocess

import numpy as np
import pytest

JAC = dict(smoother=3, smoother_iters=2, omega=0.8)
FAKE = [C.c_void_p(8), C.c_void_p(16), C.c_void_p(24), C.c_void_p(32)]  # rowptr, col, val, b


def raw_create(amg, n, dims, n_levels, dim=None, ptrs=FAKE, **kw):
    """the C entry point itself -> (status, message); `dim` may disagree with len(dims)"""
    d3 = np.array(tuple(dims) + (1,) * (3 - len(dims)), np.int64)
    o = amg.Multigrid._options(kw.pop("smoother", 3), kw.pop("smoother_iters", 2), kw.pop("omega", 0.8), -1, True,
                               kw.pop("stencil_transfers", True), kw.pop("layout", None), False, False, False,
                               False, None, False, False, False, False, False, kw.pop("cheb_degree", 2),
                               kw.pop("cheb_lower", 0.3), kw.pop("cheb_upper", 1.0))
    o.window = int(kw.pop("window", False))
    assert not kw, kw
    h = C.c_void_p()
    st = amg.lib().amg_hip_create_tensor_dev(n, ptrs[0], ptrs[1], ptrs[2], ptrs[3],
                                             len(dims) if dim is None else dim, d3.ctypes.data_as(amg._i64p),
                                             n_levels, C.byref(o), C.byref(h))
    assert st != amg.OK and not h.value
    return st, amg.lib().amg_hip_last_error().decode()


def test_symbol_exported_and_bound(amg):
    out = subprocess.run(["nm", "-D", "--defined-only", amg.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert " T amg_hip_create_tensor_dev\n" in out
    assert "amg_hip_create_tensor_dev" in amg._SIGS
    assert hasattr(amg.Multigrid, "tensor_dev")


def test_argument_errors_come_before_the_device(amg):
    for k in range(4):
        ptrs = list(FAKE)
        ptrs[k] = C.c_void_p(None)
        st, msg = raw_create(amg, 16, (4, 4), 2, ptrs=ptrs)
        assert st == amg.EINVAL and "null" in msg
    for dim in (1, 4, 0, -2):
        st, msg = raw_create(amg, 16, (4, 4), 2, dim=dim)
        assert st == amg.EINVAL and "`dim` must be 2 or 3" in msg
    st, msg = raw_create(amg, 15, (4, 4), 2)
    assert st == amg.EINVAL and "`n` = 15 is not the 4 x 4 x 1 grid of `dims`" in msg
    st, msg = raw_create(amg, 32, (4, 4, 2), 2, dim=2)
    assert st == amg.EINVAL and "`dims[2]` must be 1 when `dim` is 2" in msg
    # 33 x 20 -> 16 x 10 -> 8 x 5 -> 4 x 2 -> 2 x 1: five levels, the sixth would coarsen a 2 x 1 grid
    st, msg = raw_create(amg, 660, (33, 20), 6)
    assert st == amg.EINVAL and "level 5 is not possible: level 4 is a 2 x 1 x 1 grid" in msg
    st, msg = raw_create(amg, 270, (9, 6, 5), 4)
    assert st == amg.EINVAL and "level 3 is not possible: level 2 is a 2 x 1 x 1 grid" in msg
    st, msg = raw_create(amg, 16, (4, 4), 0)
    assert st == amg.EINVAL and "`n_levels`" in msg
    for bad in (dict(cheb_degree=0), dict(cheb_lower=0.0), dict(cheb_lower=1.5, cheb_upper=1.0)):
        st, msg = raw_create(amg, 16, (4, 4), 2, smoother=amg.SM_CHEBYSHEV, **bad)
        assert st == amg.EINVAL and "cheb_" in msg
    for omega in (0.0, 2.0, -1.0):
        st, msg = raw_create(amg, 16, (4, 4), 2, smoother=amg.SM_LINE_JACOBI, omega=omega)
        assert st == amg.EINVAL and "line smoother" in msg
    st, msg = raw_create(amg, 16, (4, 4), 2, smoother=17)
    assert st == amg.EINVAL and "smoother" in msg
    st, msg = raw_create(amg, 16, (4, 4), 2, layout=9)
    assert st == amg.EINVAL and "layout" in msg
    st, msg = raw_create(amg, 16, (4, 4), 2, window=True)
    assert st == amg.EUNSUPPORTED and "window" in msg


def test_level_error_is_worded_as_by_create_tensor(amg):
    cp, ri, v = amg.laplacian(9)
    with pytest.raises(ValueError) as e:
        amg.Multigrid.tensor(cp, ri, v, amg.rhs(9), (9, 9), 5, host_only=True, **JAC)
    st, msg = raw_create(amg, 81, (9, 9), 5)
    assert st == amg.EINVAL and msg == str(e.value) and "level 4 is not possible" in msg


def test_without_a_device_it_fails_with_ehip(amg):
    if amg.device_count() > 0:
        pytest.skip("a HIP device is present: the refusal cannot be seen here")
    for kw in (dict(), dict(smoother=amg.SM_MULTICOLOR_GS, smoother_iters=1)):  # device path and fallback
        st, msg = raw_create(amg, 16, (4, 4), 2, **kw)
        assert st == amg.EHIP, msg
    crow = np.arange(0, 17, dtype=np.int32)
    with pytest.raises(amg.AmgHipError) as e:
        amg.Multigrid.tensor_dev(crow, np.arange(16, dtype=np.int32), np.ones(16), np.ones(16), (4, 4), 2, **JAC)
    assert e.value.status == amg.EHIP


def test_wrapper_refuses_arrays_of_the_wrong_kind(amg):
    torch = pytest.importorskip("torch")
    crow = np.arange(0, 17, dtype=np.int32)
    col = np.arange(16, dtype=np.int32)
    val, b = np.ones(16), np.ones(16)
    make = lambda *a: amg.Multigrid.tensor_dev(*a, (4, 4), 2, **JAC)  # noqa: E731
    with pytest.raises(ValueError, match="crow: expected dtype int32"):
        make(crow.astype(np.int64), col, val, b)
    with pytest.raises(ValueError, match="col: expected dtype int32"):
        make(crow, col.astype(np.int64), val, b)
    with pytest.raises(ValueError, match="val: expected dtype float64"):
        make(crow, col, val.astype(np.float32), b)
    with pytest.raises(ValueError, match="b: expected dtype float64"):
        make(crow, col, val, b.astype(np.float32))
    with pytest.raises(ValueError, match="crow: expected dtype torch.int32"):
        make(torch.from_numpy(crow.astype(np.int64)), col, val, b)
    with pytest.raises(ValueError, match="val: expected dtype torch.float64"):
        make(crow, col, torch.ones(16, dtype=torch.float32), b)
    with pytest.raises(ValueError, match="val: expected a contiguous tensor"):
        make(crow, col, torch.ones(32, dtype=torch.float64)[::2], b)
    with pytest.raises(ValueError, match="col: expected a torch tensor or a numpy array"):
        make(crow, list(col), val, b)
    with pytest.raises(ValueError, match="b: expected a 1-D array"):
        make(crow, col, val, b.reshape(4, 4))
    with pytest.raises(ValueError, match="same number of degrees of freedom, got 16 and 15"):
        make(crow, col, val, b[:15])
    with pytest.raises(ValueError, match="`col` and `val` must have the same length"):
        make(crow, col, val[:15], b)
