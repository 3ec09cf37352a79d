"""amg_hip_create_poisson_tensor on the device: the full-coarsening Poisson hierarchy built by the
generator, K-TensorGalerkin and the encoder kernels against the host-built solver
(Multigrid.poisson_tensor without device_setup: host arrays, host Galerkin product) -- level
matrices, dims, transfers and right-hand side with np.array_equal, every level's vectors after every
V-cycle, PCG, one block call, and the options that silently take the host path.  setup_on_device
is asserted everywhere, so no comparison can pass through the fallback."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_tensor_device_setup import same_hierarchy  # noqa: E402

pytestmark = pytest.mark.gpu

JAC = dict(smoother=3, smoother_iters=2, omega=0.8)
CHEB = dict(smoother=5, smoother_iters=1, cheb_degree=2)


def deepest(n):
    """levels of the deepest hierarchy of an n^dim grid: an axis of fewer than 2 points ends it"""
    levels = 1
    while n >= 2:
        n //= 2
        levels += 1
    return levels


def pair(amg, n, levels, dim=2, dev_kw=None, **kw):
    dev = amg.Multigrid.poisson_tensor(n, levels, dim=dim, device_setup=True, **kw, **(dev_kw or {}))
    host = amg.Multigrid.poisson_tensor(n, levels, dim=dim, **kw)
    assert host.setup_on_device == 0
    return dev, host


GRIDS = [(2, 2), (2, 5), (2, 7), (2, 8), (2, 33), (2, 64), (2, 255), (2, 256), (3, 4), (3, 9), (3, 16), (3, 33)]


@pytest.mark.parametrize("dim,n", GRIDS, ids=[f"{n}^{d}" for d, n in GRIDS])
def test_hierarchy_bits(amg, dim, n):
    for levels in sorted({deepest(n), 2}):
        for keep in (False, True):
            dev, host = pair(amg, n, levels, dim, keep_structural_zeros=keep, **JAC)
            assert dev.setup_on_device == 1, (n, dim, levels, keep)
            assert dev.n_levels == levels
            same_hierarchy(dev, host)
            assert [dev.level_transfer_kind(l) for l in range(levels - 1)] == [2] * (levels - 1)
            assert np.array_equal(dev.get_rhs(0), host.get_rhs(0))
            assert np.array_equal(dev.get_rhs(0), amg.rhs(n, dim))
            dev.close()
            host.close()


def _state(mg):
    return [(mg.get_soln(l), mg.get_rhs(l)) for l in range(mg.n_levels)]


CYCLE_CASES = [(2, 255, 6), (2, 256, 6), (3, 33, 4)]


@pytest.mark.parametrize("sm", [JAC, CHEB], ids=["jacobi", "chebyshev"])
@pytest.mark.parametrize("dim,n,levels", CYCLE_CASES, ids=["255^2", "256^2", "33^3"])
def test_vcycles_bitwise(amg, dim, n, levels, sm):
    dev, host = pair(amg, n, levels, dim, **sm)
    assert dev.setup_on_device == 1
    if sm is CHEB:
        assert [dev.cheb_bounds(l) for l in range(levels)] == [host.cheb_bounds(l) for l in range(levels)]
    for cycle in range(3):
        dev.vcycle(1)
        host.vcycle(1)
        dev.sync()
        host.sync()
        for l, (a, b) in enumerate(zip(_state(dev), _state(host))):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (cycle, l)
    assert np.all(np.isfinite(dev.get_soln(0))) and np.linalg.norm(dev.get_soln(0)) > 0
    assert dev.rss() == host.rss()
    dev.close()
    host.close()


def test_pcg_bitwise(amg):
    dev, host = pair(amg, 255, 6, **JAC)
    assert dev.setup_on_device == 1
    x, it, rel = dev.pcg(1e-8, 100)
    xh, ith, relh = host.pcg(1e-8, 100)
    assert rel <= 1e-8 and it == ith and rel == relh and np.array_equal(x, xh)
    dev.close()
    host.close()


def test_block_call_bitwise(amg):
    torch = pytest.importorskip("torch")
    dev, host = pair(amg, 255, 6, **JAC)
    assert dev.setup_on_device == 1
    n0 = dev.get_n_dofs(0)
    rng = np.random.default_rng(11)
    U0, F0 = rng.standard_normal((n0, 3)), rng.standard_normal((n0, 3))
    out = []
    for mg in (dev, host):
        U, F = torch.from_numpy(U0.copy()).cuda(), torch.from_numpy(F0.copy()).cuda()
        mg.block_vcycles(U, F, n=2)
        torch.cuda.synchronize()
        out.append(U.cpu().numpy())
    assert np.array_equal(out[0], out[1]) and not np.array_equal(out[0], U0)
    dev.close()
    host.close()


@pytest.mark.parametrize("name", ["multicolor", "line", "csr_transfers", "host_galerkin"])
def test_fallbacks_take_the_host_path(amg, name):
    kw, dev_kw = dict(JAC), {}
    if name == "multicolor":
        kw = dict(smoother=amg.SM_MULTICOLOR_GS, smoother_iters=1)
    elif name == "line":
        kw = dict(smoother=amg.SM_LINE_JACOBI, smoother_iters=1, omega=0.7)
    elif name == "csr_transfers":
        kw["stencil_transfers"] = False
    else:
        dev_kw = dict(host_galerkin=True)
    for dim, n, levels in ((2, 33, 5), (3, 9, 3)):
        dev, host = pair(amg, n, levels, dim, dev_kw=dev_kw, **kw)
        assert dev.setup_on_device == 0, name
        same_hierarchy(dev, host)
        assert np.array_equal(dev.get_rhs(0), host.get_rhs(0))
        dev.close()
        host.close()


def test_mid_size_1024(amg):
    dev, host = pair(amg, 1024, 8, **JAC)
    assert dev.setup_on_device == 1
    same_hierarchy(dev, host)
    dev.close()
    host.close()
