"""amg_hip_create_poisson_tensor / amg_hip_setup_on_device, the parts that need no GPU: the exported
symbols, the argument errors (checked before the device is touched), the host_only solver against
Multigrid.tensor on amg.laplacian(n) / amg.rhs(n) (levels, dims, matrices, transfers: bitwise) with
setup_on_device == 0, and the refusal without a device."""
import subprocess

import numpy as np
import pytest

JAC = dict(smoother=3, smoother_iters=2, omega=0.8)


def dev_tensor(amg, n, levels, dim=2, **kw):
    return amg.Multigrid.poisson_tensor(n, levels, dim=dim, device_setup=True, **kw)


def host_tensor(amg, n, levels, dim=2, **kw):
    cp, ri, v = amg.laplacian(n, dim)
    return amg.Multigrid.tensor(cp, ri, v, amg.rhs(n, dim), (n,) * dim, levels, **kw)


def same_hierarchy(got, want):
    """levels, dims, transfer kinds, level matrices and transfers, all bitwise"""
    assert got.n_levels == want.n_levels
    for l in range(want.n_levels):
        assert got.level_dims(l) == want.level_dims(l), l
        assert got.get_n_dofs(l) == want.get_n_dofs(l), l
        for a, b in zip(got.get_coefficient_matrix(l), want.get_coefficient_matrix(l)):
            assert a.dtype == b.dtype and np.array_equal(a, b), l
        if l + 1 < want.n_levels:
            assert got.level_transfer_kind(l) == want.level_transfer_kind(l), l
            for which in ("P", "R"):
                for a, b in zip(got.get_transfer(l, which), want.get_transfer(l, which)):
                    assert a.dtype == b.dtype and np.array_equal(a, b), (l, which)


def test_symbols_exported(amg):
    out = subprocess.run(["nm", "-D", "--defined-only", amg.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for sym in ("amg_hip_create_poisson_tensor", "amg_hip_setup_on_device"):
        assert f" T {sym}\n" in out, sym


@pytest.mark.parametrize("host_only", [False, True])
def test_argument_errors_come_before_the_device(amg, host_only):
    """None of these needs a device, with or without host_only."""
    kw = dict(host_only=host_only, **JAC)
    for dim in (1, 4, 0, -2):
        with pytest.raises(ValueError, match="dim"):
            dev_tensor(amg, 16, 2, dim=dim, **kw)
    for n in (1, 0, -3):
        with pytest.raises(ValueError, match="`n`"):
            dev_tensor(amg, n, 2, **kw)
    # 63 -> 31 -> 15 -> 7 -> 3 -> 1: six levels, the seventh would coarsen the 1 x 1 grid of level 5
    with pytest.raises(ValueError, match="level 6 is not possible: level 5 is a 1 x 1 x 1 grid"):
        dev_tensor(amg, 63, 7, **kw)
    with pytest.raises(ValueError, match="level 3 is not possible: level 2 is a 1 x 1 x 1 grid"):
        dev_tensor(amg, 4, 4, dim=3, **kw)
    with pytest.raises(ValueError, match="level 2 "):
        dev_tensor(amg, 2, 3, **kw)
    for bad in (dict(cheb_degree=0), dict(cheb_lower=0.0), dict(cheb_lower=1.5, cheb_upper=1.0)):
        with pytest.raises(ValueError):
            dev_tensor(amg, 16, 2, smoother=amg.SM_CHEBYSHEV, host_only=host_only, **bad)
    with pytest.raises(amg.AmgHipError) as e:
        dev_tensor(amg, 16, 2, window=True, **kw)
    assert e.value.status == amg.EUNSUPPORTED


def test_level_error_is_worded_as_by_create_tensor(amg):
    msgs = []
    for make in (dev_tensor, host_tensor):
        with pytest.raises(ValueError) as e:
            make(amg, 9, 5, host_only=True, **JAC)
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1] and "level 4 is not possible" in msgs[0]


@pytest.mark.parametrize("n,levels,dim", [(2, 2, 2), (7, 3, 2), (33, 6, 2), (64, 7, 2), (64, 2, 2), (9, 4, 3),
                                          (16, 5, 3), (5, 1, 2)])
@pytest.mark.parametrize("keep", [False, True])
def test_host_only_equals_create_tensor(amg, n, levels, dim, keep):
    kw = dict(host_only=True, keep_structural_zeros=keep, **JAC)
    got, want = dev_tensor(amg, n, levels, dim, **kw), host_tensor(amg, n, levels, dim, **kw)
    assert got.setup_on_device == 0 and want.setup_on_device == 0
    same_hierarchy(got, want)
    got.close()
    want.close()


def test_setup_on_device_is_zero_on_other_host_only_solvers(amg):
    cp, ri, v = amg.laplacian(16)
    mg = amg.Multigrid(cp, ri, v, amg.rhs(16), 3, host_only=True, **JAC)
    assert mg.setup_on_device == 0
    mg.close()
    cheb = dev_tensor(amg, 16, 3, smoother=amg.SM_CHEBYSHEV, host_only=True)
    assert cheb.setup_on_device == 0 and cheb.cheb_bounds(0) == host_tensor(
        amg, 16, 3, smoother=amg.SM_CHEBYSHEV, host_only=True).cheb_bounds(0)
    cheb.close()


def test_without_a_device_it_fails_with_ehip(amg):
    if amg.device_count() > 0:
        pytest.skip("a HIP device is present: the refusal cannot be seen here")
    with pytest.raises(amg.AmgHipError) as e:
        dev_tensor(amg, 16, 3, **JAC)
    assert e.value.status == amg.EHIP
