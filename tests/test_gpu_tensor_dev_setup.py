"""amg_hip_create_tensor_dev: the full-coarsening hierarchy of a caller's device CSR matrix, built on
the device (K-CsrCheck, K-TensorGalerkin, the dictionary encoder, K-SellPack, K-Transpose), against
the host constructor (Multigrid.tensor on the CSC arrays of the same matrix, same options).
Everything is compared with np.array_equal / ==: set-up paths differ in nothing.  Every case first
asserts ON THE HOST SOLVER that its operator exercises what it is meant to (panel layout, a level
that is not bitwise symmetric, the dictionary, 27-entry rows), and setup_on_device is asserted
everywhere, so no comparison can pass through the fallback.

Case (f): at 80 x 70 the AUTO rule picks SELL-64 on every level of the host solver (stencil rows are
too even for 25 % padding), so AUTO is compared but shows one outcome only; the CSR outcome is
covered by the explicit CSR requests of (e) and (f).

Case (d): the 9 x 6 x 5 grid coarsens to 4 x 3 x 2, whose rows cannot hold more than 3 * 3 * 2 = 18
entries: enough for the 32-lane group and too many for the dictionary, but not the 27 of an interior
row.  Case (d27) adds the smallest box beside it that has one, 9 x 6 x 7 -> 4 x 3 x 3, so that the
transpose also sorts its widest column."""
import os
import sys

import numpy as np
import pytest

sp = pytest.importorskip("scipy.sparse")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_tensor_device_setup import same_hierarchy  # noqa: E402

pytestmark = pytest.mark.gpu

JAC = dict(smoother=3, smoother_iters=2, omega=0.8)
CHEB = dict(smoother=5, smoother_iters=1, cheb_degree=2)
LINE = dict(smoother=6, smoother_iters=1, omega=0.7)
DICT, SELL, CSR = 3, 2, 1


def diffusion(dims, kappa, shift):
    """-div(kappa grad u) + shift u on the grid `dims` (x fastest), one coefficient per face between
    two points and kappa's mean on the boundary faces (Dirichlet), as a canonical scipy CSR matrix.
    kappa(axis, count) -> face coefficients; a face coefficient of exactly 0.0 stays in the pattern."""
    dims = tuple(dims)
    n = int(np.prod(dims))
    idx = np.arange(n).reshape(dims[::-1])  # [z][y][x]
    diag = np.full(n, float(shift))
    rows, cols, vals = [], [], []
    for axis in range(len(dims)):
        ax = len(dims) - 1 - axis  # numpy axis of grid axis `axis`
        lo = np.take(idx, np.arange(dims[axis] - 1), axis=ax).ravel()
        hi = np.take(idx, np.arange(1, dims[axis]), axis=ax).ravel()
        k = np.asarray(kappa(axis, lo.size), dtype=np.float64)
        np.add.at(diag, lo, k)
        np.add.at(diag, hi, k)
        edge = float(np.round(k.mean()))
        for side in (0, dims[axis] - 1):
            np.add.at(diag, np.take(idx, [side], axis=ax).ravel(), edge)
        rows += [lo, hi]
        cols += [hi, lo]
        vals += [-k, -k]
    rows.append(np.arange(n))
    cols.append(np.arange(n))
    vals.append(diag)
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    A.sort_indices()
    return A


def integer_kappa(seed, zeros=0):
    rng = np.random.default_rng(seed)

    def kappa(axis, count):
        k = rng.integers(1, 1001, size=count).astype(np.float64)
        if zeros:
            k[rng.choice(count, size=zeros, replace=False)] = 0.0
        return k
    return kappa


def real_kappa(seed):
    rng = np.random.default_rng(seed)
    return lambda axis, count: rng.uniform(1.0, 10.0, size=count)


def anisotropic(axis, count):
    return np.full(count, 1.0 if axis == 0 else 1.0 / 64.0)


_OPS = {}


def operator(name):
    """(dims, levels, CSR matrix, b): built once per name and never modified"""
    if name not in _OPS:
        dims, levels, A = {
            "a": lambda: ((33, 20), 3, diffusion((33, 20), integer_kappa(1), 1.0)),
            "b": lambda: ((33, 20), 3, diffusion((33, 20), real_kappa(2), 1.0)),
            "c": lambda: ((17, 12), 3, diffusion((17, 12), anisotropic, 0.0)),
            "d": lambda: ((9, 6, 5), 2, diffusion((9, 6, 5), real_kappa(4), 1.0)),
            "d27": lambda: ((9, 6, 7), 2, diffusion((9, 6, 7), real_kappa(4), 1.0)),
            "e": lambda: ((33, 20), 3, diffusion((33, 20), integer_kappa(5, zeros=7), 1.0)),
            "f": lambda: ((80, 70), 3, diffusion((80, 70), integer_kappa(1), 1.0)),
        }[name]()
        b = np.random.default_rng(99).standard_normal(A.shape[0])
        for a in (A.indptr, A.indices, A.data, b):
            a.setflags(write=False)
        _OPS[name] = (dims, levels, A, b)
    return _OPS[name]


def host_solver(amg, name, **kw):
    dims, levels, A, b = operator(name)
    kw.pop("host_galerkin", None)  # Multigrid.tensor is the host constructor already
    Ac = A.tocsc()
    Ac.sort_indices()
    mg = amg.Multigrid.tensor(Ac.indptr.astype(np.int32), Ac.indices.astype(np.int32), Ac.data, b, dims, levels,
                              **kw)
    assert mg.setup_on_device == 0
    return mg


def dev_solver(amg, name, as_torch=False, **kw):
    dims, levels, A, b = operator(name)
    arrs = [A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy(), b.copy()]
    if as_torch:
        import torch
        arrs = [torch.from_numpy(a).cuda() for a in arrs]
    return amg.Multigrid.tensor_dev(*arrs, dims, levels, **kw)


def level_symmetry(mg):
    """per level: the matrix equals its transpose bit for bit, structure included"""
    out = []
    for l in range(mg.n_levels):
        cp, ri, v = mg.get_coefficient_matrix(l)
        n = cp.size - 1
        M = sp.csc_matrix((np.arange(1, v.size + 1), ri, cp), shape=(n, n))  # entry numbers keep exact zeros
        T = M.T.tocsc()
        T.sort_indices()
        same = np.array_equal(T.indptr, cp) and np.array_equal(T.indices, ri)
        out.append(bool(same and np.array_equal(v[T.data - 1].view(np.int64), v.view(np.int64))))
    return out


def compare(amg, dev, host, on_device=1, block=True):
    """every observable of the two solvers, bitwise"""
    torch = pytest.importorskip("torch")
    assert dev.setup_on_device == on_device
    L = host.n_levels
    same_hierarchy(dev, host)
    assert [dev.level_transfer_kind(l) for l in range(L - 1)] == [host.level_transfer_kind(l) for l in range(L - 1)]
    assert [dev.level_layout(l) for l in range(L)] == [host.level_layout(l) for l in range(L)]
    assert np.array_equal(dev.get_rhs(0), host.get_rhs(0))
    n0 = host.get_n_dofs(0)
    rng = np.random.default_rng(7)
    u0, f0, v = rng.standard_normal(n0), rng.standard_normal(n0), rng.standard_normal(n0)
    for mg in (dev, host):
        mg.set_vec(0, "u", u0)
        mg.set_vec(0, "f", f0)
    for cycles in (1, 2):  # u after 1 and after 3 V-cycles
        dev.vcycle(cycles)
        host.vcycle(cycles)
        dev.sync()
        host.sync()
        got, want = dev.get_soln(0), host.get_soln(0)
        assert np.array_equal(got, want), cycles
        assert np.all(np.isfinite(got)) and not np.array_equal(got, u0)
    assert dev.rss() == host.rss()
    z = []
    for mg in (dev, host):
        dv = torch.from_numpy(v.copy()).cuda()
        dz = torch.empty_like(dv)
        mg.apply_dev(dv.data_ptr(), dz.data_ptr())
        mg.sync()
        z.append(dz.cpu().numpy())
    assert np.array_equal(z[0], z[1]) and np.linalg.norm(z[0]) > 0
    for mg in (dev, host):
        mg.set_vec(0, "f", f0)
    x, it, rel = dev.pcg(1e-8, 100)
    xh, ith, relh = host.pcg(1e-8, 100)
    assert it == ith and rel == relh and np.array_equal(x, xh) and np.isfinite(rel) and it >= 1
    if not block:
        return
    U0, F0 = rng.standard_normal((n0, 3)), rng.standard_normal((n0, 3))
    out = []
    for mg in (dev, host):
        U, F = torch.from_numpy(U0.copy()).cuda(), torch.from_numpy(F0.copy()).cuda()
        mg.block_vcycles(U, F, n=1)
        torch.cuda.synchronize()
        out.append(U.cpu().numpy())
    assert np.array_equal(out[0], out[1]) and not np.array_equal(out[0], U0)


def run_case(amg, name, expect, as_torch=False, **kw):
    host = host_solver(amg, name, **kw)
    expect(host)
    dev = dev_solver(amg, name, as_torch=as_torch, **kw)
    try:
        compare(amg, dev, host, block=kw.get("smoother") != 6)  # no block cycle with the line smoother
        if kw.get("smoother") == 5:
            assert [dev.cheb_bounds(l) for l in range(host.n_levels)] == \
                   [host.cheb_bounds(l) for l in range(host.n_levels)]
        if kw.get("smoother") == 6:
            assert [dev.line_stride(l) for l in range(host.n_levels)] == \
                   [host.line_stride(l) for l in range(host.n_levels)]
    finally:
        dev.close()
        host.close()


def layouts(mg):
    return [mg.level_layout(l)[0] for l in range(mg.n_levels)]


def expect_a(host):  # K-SellPack alone
    assert [host.level_dims(l) for l in range(3)] == [(33, 20, 1), (16, 10, 1), (8, 5, 1)]
    assert all(level_symmetry(host)) and all(lay in (SELL, CSR) for lay in layouts(host))


def expect_b(host):  # K-Transpose + K-SellPack
    sym = level_symmetry(host)
    assert sym[0] and not all(sym[1:]) and all(lay in (SELL, CSR) for lay in layouts(host))


def expect_c(host):  # the dictionary on a non-cubic box
    assert [host.level_dims(l) for l in range(3)] == [(17, 12, 1), (8, 6, 1), (4, 3, 1)]
    assert all(level_symmetry(host)) and layouts(host) == [DICT] * 3


def expect_d(host):  # 3-D coarse rows beyond the dictionary's 16 entries, not bitwise symmetric
    cp, _, _ = host.get_coefficient_matrix(1)
    assert host.level_dims(1) == (4, 3, 2) and int(np.diff(cp).max()) == 18
    assert not level_symmetry(host)[1] and all(lay in (SELL, CSR) for lay in layouts(host))


def expect_d27(host):  # 27-entry coarse rows: the widest column the transpose sorts
    cp, _, _ = host.get_coefficient_matrix(1)
    assert host.level_dims(1) == (4, 3, 3) and int(np.diff(cp).max()) == 27
    assert not level_symmetry(host)[1] and all(lay in (SELL, CSR) for lay in layouts(host))


@pytest.mark.parametrize("sm", [JAC, CHEB], ids=["jacobi", "chebyshev"])
@pytest.mark.parametrize("name,expect", [("a", expect_a), ("b", expect_b), ("d", expect_d), ("d27", expect_d27)],
                         ids=["a", "b", "d", "d27"])
def test_panel_levels(amg, name, expect, sm):
    run_case(amg, name, expect, as_torch=(name == "b"), **sm)


@pytest.mark.parametrize("sm", [JAC, LINE], ids=["jacobi", "line"])
def test_dictionary_on_a_non_cubic_box(amg, sm):
    run_case(amg, "c", expect_c, **sm)


@pytest.mark.parametrize("layout", [None, CSR], ids=["auto", "csr"])
@pytest.mark.parametrize("keep", [False, True], ids=["pruned", "kept"])
def test_exact_zeros(amg, keep, layout):
    def expect_e(host):
        _, _, v = host.get_coefficient_matrix(0)
        assert np.count_nonzero(v == 0.0) == 2 * 2 * 7  # seven faces per axis, both triangles, stay structural
        assert all(level_symmetry(host))
        assert all(lay == (CSR if layout == CSR else SELL) for lay in layouts(host))
    run_case(amg, "e", expect_e, keep_structural_zeros=keep, layout=layout, **JAC)


@pytest.mark.parametrize("layout", [CSR, SELL, None], ids=["csr", "sell", "auto"])
def test_layout_requests(amg, layout):
    def expect_f(host):
        assert all(level_symmetry(host))
        assert all(lay == (CSR if layout == CSR else SELL) for lay in layouts(host))
    run_case(amg, "f", expect_f, layout=layout, **JAC)


@pytest.mark.parametrize("name", ["multicolor", "csr_transfers", "host_galerkin"])
def test_fallbacks_take_the_host_path(amg, name):
    kw = dict(JAC)
    if name == "multicolor":
        kw = dict(smoother=amg.SM_MULTICOLOR_GS, smoother_iters=1)
    elif name == "csr_transfers":
        kw["stencil_transfers"] = False
    else:
        kw["host_galerkin"] = True
    host = host_solver(amg, "a", **kw)
    dev = dev_solver(amg, "a", **kw)
    try:
        assert dev.setup_on_device == 0, name
        same_hierarchy(dev, host)
        assert [dev.level_layout(l) for l in range(3)] == [host.level_layout(l) for l in range(3)]
        assert np.array_equal(dev.get_rhs(0), host.get_rhs(0))
        dev.vcycle(2)
        host.vcycle(2)
        dev.sync()
        host.sync()
        assert np.array_equal(dev.get_soln(0), host.get_soln(0))
    finally:
        dev.close()
        host.close()


def test_malformed_arrays_are_refused_by_the_check_kernel(amg):
    dims, levels, A, b = operator("c")
    crow, col, val = A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy()
    n = crow.size - 1
    bad = col.copy()
    bad[crow[5] + 1] = n  # one past the last column
    with pytest.raises(ValueError, match="row 5 "):
        amg.Multigrid.tensor_dev(crow, bad, val, b.copy(), dims, levels, **JAC)
    bad = col.copy()
    bad[crow[5] + 1] = -1
    with pytest.raises(ValueError, match="row 5 "):
        amg.Multigrid.tensor_dev(crow, bad, val, b.copy(), dims, levels, **JAC)
    bad = col.copy()
    p = crow[9]
    bad[p], bad[p + 1] = col[p + 1], col[p]  # descending inside row 9
    with pytest.raises(ValueError, match="row 9 "):
        amg.Multigrid.tensor_dev(crow, bad, val, b.copy(), dims, levels, **JAC)
    bad = crow.copy()
    bad[3] = crow[4] + 1  # rowptr decreases after row 3
    with pytest.raises(ValueError, match="row 2 "):
        amg.Multigrid.tensor_dev(bad, col, val, b.copy(), dims, levels, **JAC)
    with pytest.raises(ValueError, match="row 5 "):  # the fallback's options: the check still comes first
        bad = col.copy()
        bad[crow[5] + 1] = n
        amg.Multigrid.tensor_dev(crow, bad, val, b.copy(), dims, levels, smoother=amg.SM_MULTICOLOR_GS)
    mg = dev_solver(amg, "c", **JAC)  # a fresh valid solver afterwards runs
    assert mg.setup_on_device == 1
    mg.vcycle(1)
    mg.sync()
    assert np.all(np.isfinite(mg.get_soln(0))) and np.linalg.norm(mg.get_soln(0)) > 0
    mg.close()
