"""amg_hip_create_tensor_opdep_dev / Multigrid.tensor_opdep_dev, the parts that need no GPU: the exported
symbol, its declaration and its binding; every argument error, which must arrive before the device is
touched (the "device pointers" are small integers that must never be dereferenced) with the status and
the text of amg_hip_create_tensor_opdep under the new entry point's name; the refusal of null arrays; and
the refusal without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

FAKE = [C.c_void_p(8), C.c_void_p(16), C.c_void_p(24), C.c_void_p(32)]  # rowptr, col, val, b
HOST, DEV = "amg_hip_create_tensor_opdep: ", "amg_hip_create_tensor_opdep_dev: "
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def options(amg, **kw):
    o = amg.Multigrid._options(kw.pop("smoother", 3), 2, 0.8, -1, True, True, None, False, False, False, False, None,
                               False, False, False, False, False, 2, 0.3, 1.0)
    o.window = int(kw.pop("window", False))
    o.natural_sides, o.singular = int(kw.pop("natural_sides", 0)), int(kw.pop("singular", False))
    assert not kw, kw
    return o


def grid_args(amg, dims, dim, masks):
    d3 = None if dims is None else np.array(tuple(dims) + (1,) * (3 - len(dims)), np.int64)
    m = None if masks is None else np.ascontiguousarray(masks, np.int32)
    return (d3, m, len(dims) if dim is None else dim, None if d3 is None else d3.ctypes.data_as(amg._i64p),
            None if m is None else m.ctypes.data_as(amg._i32p))


def raw_dev(amg, n, dims, n_levels, masks, min_coarse=32, dim=None, ptrs=FAKE, **kw):
    """the C entry point itself -> (status, message); `dim` may disagree with len(dims)"""
    keep = grid_args(amg, dims, dim, masks)
    o, h = options(amg, **kw), C.c_void_p()
    st = amg.lib().amg_hip_create_tensor_opdep_dev(n, ptrs[0], ptrs[1], ptrs[2], ptrs[3], keep[2], keep[3], n_levels,
                                                   keep[4], min_coarse, C.byref(o), C.byref(h))
    assert st != amg.OK and not h.value
    return st, amg.lib().amg_hip_last_error().decode()


def raw_host(amg, n, dims, n_levels, masks, min_coarse=32, dim=None, **kw):
    """the host constructor with the same grid arguments (host_only: no device) on arrays it never gets to read"""
    keep = grid_args(amg, dims, dim, masks)
    cp, ri, v = np.arange(n + 2, dtype=np.int32), np.arange(n + 1, dtype=np.int32), np.ones(n + 1)
    b = np.ones(n + 1)
    o, h = options(amg, **kw), C.c_void_p()
    o.host_only = 1
    st = amg.lib().amg_hip_create_tensor_opdep(n, cp.ctypes.data_as(amg._i32p), ri.ctypes.data_as(amg._i32p),
                                               v.ctypes.data_as(amg._f64p), b.ctypes.data_as(amg._f64p), keep[2], keep[3],
                                               n_levels, keep[4], min_coarse, C.byref(o), C.byref(h))
    assert st != amg.OK and not h.value
    return st, amg.lib().amg_hip_last_error().decode()


def test_symbol_exported_declared_and_bound(amg):
    out = subprocess.run(["nm", "-D", "--defined-only", amg.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert " T amg_hip_create_tensor_opdep_dev\n" in out
    with open(os.path.join(ROOT, "include", "amg_hip.h")) as f:
        assert "amg_hip_status amg_hip_create_tensor_opdep_dev(int64_t n, const int32_t* rowptr_dev" in f.read()
    assert "amg_hip_create_tensor_opdep_dev" in amg._SIGS
    assert hasattr(amg.Multigrid, "tensor_opdep_dev")


# (what, status, a piece of the text, arguments)
ALL = 15
CASES = [
    ("dim 1", "EINVAL", "`dim` must be 2 or 3", dict(n=16, dims=(4, 4), n_levels=2, masks=[1], dim=1)),
    ("dim 4", "EINVAL", "`dim` must be 2 or 3", dict(n=16, dims=(4, 4), n_levels=2, masks=[1], dim=4)),
    ("n is not the grid", "EINVAL", "`n` = 15 is not the 4 x 4 x 1 grid", dict(n=15, dims=(4, 4), n_levels=2, masks=[1])),
    ("null dims", "EINVAL", "`dims` is null", dict(n=16, dims=None, n_levels=2, masks=[1], dim=2)),
    ("a mask of two bits", "EINVAL", "names several axes", dict(n=16, dims=(4, 4), n_levels=3, masks=[1, 3])),
    ("a zero mask", "EINVAL", "coarsens no axis", dict(n=16, dims=(4, 4), n_levels=3, masks=[2, 0])),
    ("a masked axis of one point", "EINVAL", "which has 1 point", dict(n=16, dims=(16, 1), n_levels=2, masks=[2])),
    ("min_coarse 0, automatic", "EINVAL", "`min_coarse` must be at least 1",
     dict(n=16, dims=(4, 4), n_levels=4, masks=None, min_coarse=0)),
    ("singular without all sides", "EINVAL", "`singular` = 1 needs every side natural",
     dict(n=16, dims=(4, 4), n_levels=2, masks=[1], singular=True, natural_sides=ALL - 1)),
    ("window", "EUNSUPPORTED", "window", dict(n=16, dims=(4, 4), n_levels=2, masks=[1], window=True)),
]


@pytest.mark.parametrize("what,status,piece,args", CASES, ids=[c[0] for c in CASES])
def test_argument_errors_are_the_host_constructors(amg, what, status, piece, args):
    st, msg = raw_dev(amg, **args)
    st_h, msg_h = raw_host(amg, **args)
    assert st == st_h == getattr(amg, status), (what, st, st_h, msg, msg_h)
    assert piece in msg, msg
    assert msg == msg_h.replace(HOST, DEV), (msg, msg_h)
    assert HOST not in msg


def test_null_arrays_are_refused(amg):
    for k in range(4):
        ptrs = list(FAKE)
        ptrs[k] = C.c_void_p(None)
        st, msg = raw_dev(amg, 16, (4, 4), 2, [1], ptrs=ptrs)
        assert st == amg.EINVAL and "null input array" in msg


def test_without_a_device_it_fails_with_ehip(amg):
    if amg.device_count() > 0:
        pytest.skip("a HIP device is present: the refusal cannot be seen here")
    for kw in (dict(), dict(smoother=amg.SM_MULTICOLOR_GS)):  # device path and fallback
        st, msg = raw_dev(amg, 16, (4, 4), 2, [1], **kw)
        assert st == amg.EHIP, msg
    st, msg = raw_dev(amg, 16, (4, 4), 4, None)  # automatic masks
    assert st == amg.EHIP, msg
    crow = np.arange(0, 17, dtype=np.int32)
    with pytest.raises(amg.AmgHipError) as e:
        amg.Multigrid.tensor_opdep_dev(crow, np.arange(16, dtype=np.int32), np.ones(16), np.ones(16), (4, 4), 2,
                                       axis_masks=[1], smoother=amg.SM_JACOBI, smoother_iters=2, omega=0.8)
    assert e.value.status == amg.EHIP
