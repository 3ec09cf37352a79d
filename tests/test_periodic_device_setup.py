"""amg_hip_set_periodic_device_setup, the parts that need no GPU: the symbol is exported and bound, the
switch leaves the host constructor alone, and the argument refusals of amg_hip_create_tensor_periodic_dev
still come before any device call with the switch on (the _dev form gets fake device pointers)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "algebraic-multigrid_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import periodic_twin as PT  # noqa: E402
import tensor_twin as T  # noqa: E402


@pytest.fixture
def switch_on(amg):
    amg.set_periodic_device_setup(1)
    yield amg
    amg.set_periodic_device_setup(0)


def test_symbol_is_exported_and_bound(amg):
    f = amg.lib().amg_hip_set_periodic_device_setup
    assert f.restype is None and list(f.argtypes) == [C.c_int32]
    assert callable(amg.set_periodic_device_setup)
    with open(os.path.join(ROOT, "include", "amg_hip.h")) as fh:
        assert "void amg_hip_set_periodic_device_setup(int32_t on);" in fh.read()
    for on in (1, 0, 7, 0):  # any non-zero value is "on"; back to the default
        amg.set_periodic_device_setup(on)


def _levels(mg):
    return [(mg.level_dims(l), mg.get_coefficient_matrix(l)) for l in range(mg.n_levels)]


def _same(a, b):
    return len(a) == len(b) and all(
        x[0] == y[0] and np.array_equal(x[1][0], y[1][0]) and np.array_equal(x[1][1], y[1][1]) and
        np.array_equal(x[1][2].view(np.uint64), y[1][2].view(np.uint64)) for x, y in zip(a, b))


@pytest.mark.parametrize("dims,per,masks,nl", [((8, 6), 3, (3, 1), 3), ((6, 4, 3), 7, (3,), 2)])
def test_switch_leaves_the_host_constructor_alone(amg, dims, per, masks, nl):
    A = sp.csc_matrix(PT.diffusion(dims, per))
    A.sort_indices()
    b = PT.rhs(A.shape[0], True)
    out = []
    try:
        for on in (0, 1):
            amg.set_periodic_device_setup(on)
            mg = amg.Multigrid.tensor_periodic(A.indptr, A.indices, A.data, b, dims, nl, per, axis_masks=masks,
                                               singular=True, host_only=True, smoother=amg.SM_JACOBI, smoother_iters=2,
                                               omega=0.8)
            assert mg.setup_on_device == 0 and mg.periodic_axes() == per
            out.append((_levels(mg), [mg.get_transfer(l, "P") for l in range(nl - 1)]))
            mg.close()
    finally:
        amg.set_periodic_device_setup(0)
    assert _same(out[0][0], out[1][0])
    for p, q in zip(out[0][1], out[1][1]):
        assert np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1]) and np.array_equal(p[2], q[2])


def _raw_dev(amg, dims, per, n_levels=2, masks=None, natural_sides=0, singular=0, n=None):
    """status and message of amg_hip_create_tensor_periodic_dev on fake device pointers: an argument
    error returns before anything is dereferenced."""
    i32, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    dim = len(dims)
    nn = int(np.prod(dims)) if n is None else n
    o = amg.Options()
    L = amg.lib()
    L.amg_hip_default_options(C.byref(o))
    o.smoother, o.smoother_iters, o.omega = amg.SM_JACOBI, 2, 0.8
    o.natural_sides, o.singular = natural_sides, singular
    h = C.c_void_p()
    d = np.array(T.dims3(dims), np.int64)
    m = None if masks is None else np.ascontiguousarray(masks, np.int32)
    fake = (C.c_void_p(8),) * 4
    st = L.amg_hip_create_tensor_periodic_dev(nn, *fake, dim, d.ctypes.data_as(i64), per, n_levels,
                                              None if m is None else m.ctypes.data_as(i32), C.byref(o), C.byref(h))
    assert st != 0, "a refusal was expected: nothing may be read through the fake pointers"
    return st, L.amg_hip_last_error().decode()


def test_refusals_still_come_first_with_the_switch_on(switch_on):
    amg = switch_on
    E = amg.EINVAL
    st, msg = _raw_dev(amg, (8, 6), 4)  # periodic_axes itself
    assert st == E and "periodic_axes" in msg, msg
    st, msg = _raw_dev(amg, (8, 6), 2, 3, (3, 2))  # y has 3 points on level 1 and cannot be coarsened
    assert st == E and "periodic_axes" in msg and "level 1" in msg, msg
    st, msg = _raw_dev(amg, (8, 6), 1, natural_sides=1)  # a periodic axis has no sides
    assert st == E and "natural_sides" in msg and "periodic" in msg, msg
    st, msg = _raw_dev(amg, (8, 6), 1, singular=1)  # singular needs the sides of y
    assert st == E and "singular" in msg, msg
    st, msg = _raw_dev(amg, (8, 6), 1, n=47)
    assert st == E and "`n` = 47" in msg, msg
