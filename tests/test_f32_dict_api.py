"""Single-precision cycle on dictionary-coded levels (K-DictF32), the checks that need no GPU: the header's
declaration, the ctypes signature, the context helper, and the property the kernel's Jacobi sum rests
on, pinned on the numpy twin: adding (+0.0f) * x at the diagonal slot of a sum that starts at +0.0f and
runs in ascending-slot order gives the bits of skipping that slot (tests/f32_twin.py: jacobi)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sp = pytest.importorskip("scipy.sparse")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import f32_twin as FT  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_the_header_declares_the_switch():
    with open(os.path.join(ROOT, "include", "amg_hip.h")) as fh:
        text = fh.read()
    assert re.search(r"^void amg_hip_set_f32_dict\(int32_t on\);$", text, re.M)
    assert "unless amg_hip_set_f32_dict(1) is in force" in text


def test_the_binding_has_the_signature(amg):
    fn = amg.lib().amg_hip_set_f32_dict
    assert fn.restype is None
    assert fn.argtypes == [C.c_int32]
    assert amg._SIGS["amg_hip_set_f32_dict"] == (None, [C.c_int32])
    assert callable(amg.set_f32_dict)


def test_the_context_helper_restores_zero(amg, monkeypatch):
    """f32_dict() sets 1 inside and 0 after, also when the block raises; a second entry and exit works"""
    seen = []
    monkeypatch.setattr(amg, "set_f32_dict", lambda on: seen.append(int(on)))
    with amg.f32_dict():
        assert seen == [1]
    assert seen == [1, 0]
    with pytest.raises(KeyError):
        with amg.f32_dict():
            raise KeyError("inside")
    assert seen == [1, 0, 1, 0]
    monkeypatch.undo()
    for _ in range(2):  # the real switch: in and out twice without error
        with amg.f32_dict():
            pass


def _levels(amg, oracle):
    """level matrices of the 16^2 Laplacian hierarchy (host_only: no device)"""
    A, b = oracle.laplacian(16), oracle.rhs(16)
    mg = amg.Multigrid(A.colptr, A.rowind, A.val, b, 3, smoother=amg.SM_JACOBI, smoother_iters=2, omega=0.8,
                       host_only=True)
    out = []
    for l in range(mg.n_levels):
        n = mg.get_n_dofs(l)
        colptr, rowind, val = mg.get_coefficient_matrix(l)
        out.append(sp.csr_matrix(sp.csc_matrix((val, rowind, colptr), shape=(n, n))))
    mg.close()
    return out


def _vectors(rng, n):
    """finite float32 data of both signs with -0.0, +0.0 and denormals mixed in"""
    v = rng.standard_normal(n).astype(F)
    k = rng.integers(0, 6, n)
    v[k == 0] = F(-0.0)
    v[k == 1] = F(0.0)
    tiny = (rng.integers(1, 1 << 22, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31)).view(F)
    v[k == 2] = tiny[k == 2]  # exponent field 0: denormals of both signs
    assert np.all(np.isfinite(v)) and np.any(np.signbit(v) & (v == 0)) and np.any((v != 0) & (np.abs(v) < 1e-38))
    return v


def kernel_jacobi(R, x, f, omega):
    """dict_f32_kernel's CSR_JACOBI on the padded rows: acc from +0.0f over EVERY slot in ascending order,
    the value replaced by +0.0f at the diagonal slot and at empty slots (whose gather is the row's own x),
    the diagonal summed from +0.0f out of the d column, the division run for every row."""
    n = R.shape[0]
    own = np.arange(n)
    on = R.mask & (R.idx == own[:, None])
    acc = np.zeros(n, F)
    diag = np.zeros(n, F)
    with np.errstate(all="ignore"):
        for k in range(R.w):
            a = np.where(R.offd[:, k], R.val[:, k], F(0.0)).astype(F)
            d = np.where(on[:, k], R.val[:, k], F(0.0)).astype(F)
            col = np.where(R.mask[:, k], R.idx[:, k], own)
            acc = np.add(acc, np.multiply(a, x[col]))
            diag = np.add(diag, d)
        nod = diag == 0.0
        q = np.divide(np.subtract(f, acc), np.where(nod, F(1.0), diag))
        out = np.add(x, np.multiply(F(omega), np.subtract(q, x)))
    for a in (acc, diag, q, out):
        assert a.dtype == F
    return np.where(nod, x, out)


def test_the_zero_times_x_term_keeps_the_twins_bits(amg, oracle):
    rng = np.random.default_rng(11)
    for l, M in enumerate(_levels(amg, oracle)):
        for T in (M, sp.csr_matrix(M.T)):
            R = FT.Rows(T)
            assert R.w >= 3 or M.shape[0] < 3
            for _ in range(4):
                x, f = _vectors(rng, M.shape[0]), _vectors(rng, M.shape[0])
                want = FT.jacobi(R, x, f, 0.8)
                got = kernel_jacobi(R, x, f, 0.8)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), l
