"""Mean projection (amg_hip_set_mean_projection, amg_hip_get_mean_projection, amg_hip_center_vec), the checks
that need no GPU, on host_only solvers: the symbols are exported and bound, the switch is a flag that works
without a device, the refusals and their messages are those of include/amg_hip.h."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import natural_twin as N  # noqa: E402

JAC = dict(smoother=3, smoother_iters=2, omega=0.8)
NAMES = ("amg_hip_set_mean_projection", "amg_hip_get_mean_projection", "amg_hip_center_vec")


def singular_solver(amg):
    dims = (12, 10)
    A = sp.csc_matrix(N.diffusion(dims, 0))
    A.sort_indices()
    return amg.Multigrid.tensor(A.indptr, A.indices, A.data, N.rhs(A.shape[0], 0), dims, 2, natural_sides=15,
                                singular=True, host_only=True, **JAC)


def regular_solver(amg, oracle):
    A, b = oracle.laplacian(16), oracle.rhs(16)
    return amg.Multigrid(A.colptr, A.rowind, A.val, b, 3, host_only=True, **JAC)


def last_error(amg):
    return amg.lib().amg_hip_last_error().decode()


def test_symbols_exist_and_are_bound(amg):
    L = C.CDLL(amg.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in amg._SIGS, name
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "amg_hip.h")).read()
    assert all(name + "(" in header for name in NAMES)
    for attr in ("set_mean_projection", "mean_projection", "center_vec"):
        assert hasattr(amg.Multigrid, attr), attr


def test_cpp_layer_has_the_setter(tmp_path):
    """AMG::Multigrid<double>::set_mean_projection(bool) compiles against the headers (syntax only: a member of
    a class template is not checked until it is used)"""
    import subprocess
    cxx = "g++"                                             # the compiler of tests/cpp/Makefile
    src = tmp_path / "use.cpp"
    src.write_text("#include <amg/multigrid.hpp>\n"
                   "void use(AMG::Multigrid<double>& m) { m.set_mean_projection(true); m.set_mean_projection(false); }\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", os.path.join(root, "include"), str(src)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr


def test_switch_is_a_flag_on_a_host_only_singular_solver(amg):
    mg = singular_solver(amg)
    try:
        assert mg.mean_projection == 0                      # the default
        mg.set_mean_projection(1)
        assert mg.mean_projection == 1
        mg.set_mean_projection(True)
        assert mg.mean_projection == 1
        mg.set_mean_projection(0)
        assert mg.mean_projection == 0
        L = amg.lib()
        for bad in (2, -1, 17):
            assert L.amg_hip_set_mean_projection(mg._h, bad) == amg.EINVAL
            assert "`on` must be 0 or 1" in last_error(amg) and str(bad) in last_error(amg)
            assert mg.mean_projection == 0
        mg.set_mean_projection(1)
        assert L.amg_hip_set_mean_projection(mg._h, 2) == amg.EINVAL
        assert mg.mean_projection == 1                      # a refused call changes nothing
    finally:
        mg.close()


def test_switch_is_refused_on_a_solver_that_is_not_singular(amg, oracle):
    mg = regular_solver(amg, oracle)
    try:
        L = amg.lib()
        assert mg.mean_projection == 0
        assert L.amg_hip_set_mean_projection(mg._h, 1) == amg.EINVAL
        assert "singular" in last_error(amg)
        assert mg.mean_projection == 0
        with pytest.raises(Exception, match="singular"):
            mg.set_mean_projection(1)
        mg.set_mean_projection(0)                           # off is accepted everywhere
        assert mg.mean_projection == 0
    finally:
        mg.close()


def test_null_arguments(amg):
    L = amg.lib()
    on = C.c_int32(7)
    assert L.amg_hip_set_mean_projection(None, 0) == amg.EINVAL
    assert L.amg_hip_set_mean_projection(None, 1) == amg.EINVAL
    assert L.amg_hip_get_mean_projection(None, C.byref(on)) == amg.EINVAL
    assert L.amg_hip_center_vec(None, 0, 0) == amg.EINVAL
    mg = singular_solver(amg)
    try:
        assert L.amg_hip_get_mean_projection(mg._h, None) == amg.EINVAL
    finally:
        mg.close()


def test_center_vec_refusals(amg):
    mg = singular_solver(amg)
    try:
        L = amg.lib()
        assert mg.n_levels == 2
        for level in (-1, 2, 99):
            assert L.amg_hip_center_vec(mg._h, level, 0) == amg.EINVAL
            assert "level out of range" in last_error(amg)
        for which in (-1, 2, 3):                            # 2 is r for amg_hip_get_vec; not here
            assert L.amg_hip_center_vec(mg._h, 0, which) == amg.EINVAL
            assert "`which` must be 0 (u) or 1 (f)" in last_error(amg)
        for which in (0, 1):                                # a host_only solver has no vectors to centre
            assert L.amg_hip_center_vec(mg._h, 0, which) == amg.EINVAL
            assert "host_only" in last_error(amg)
    finally:
        mg.close()
