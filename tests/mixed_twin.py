"""TEST INFRASTRUCTURE for the single-precision preconditioner (amg_hip_apply_f32 / amg_hip_pcg_mixed):
the operators of its tests and a numpy PCG whose preconditioner is tests/tensor_twin.py's V-cycle in a
chosen precision.  Nothing here reads the library.  Never imported by the product."""
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tensor_twin as T  # noqa: E402

# (dims, levels): the grids the convergence claim was checked on, and the smallest 3-D box with odd
# and even axis chains
GRIDS = {"33x20": ((33, 20), 3), "64x64": ((64, 64), 5), "17x12x9": ((17, 12, 9), 3)}


def diffusion(dims, seed, shift=1.0):
    """-div(kappa grad u) + shift u on the grid `dims` (x fastest): kappa uniform in [1, 10] per face
    between two points, kappa's rounded mean on the boundary faces (Dirichlet); canonical scipy CSR."""
    rng = np.random.default_rng(seed)
    dims = tuple(dims)
    n = int(np.prod(dims))
    idx = np.arange(n).reshape(dims[::-1])  # [z][y][x]
    diag = np.full(n, float(shift))
    rows, cols, vals = [], [], []
    for axis in range(len(dims)):
        ax = len(dims) - 1 - axis
        lo = np.take(idx, np.arange(dims[axis] - 1), axis=ax).ravel()
        hi = np.take(idx, np.arange(1, dims[axis]), axis=ax).ravel()
        k = rng.uniform(1.0, 10.0, size=lo.size)
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


_OPS = {}


def operator(name):
    """(dims, levels, CSR matrix, b, twin): built once per grid and never modified"""
    if name not in _OPS:
        dims, levels = GRIDS[name]
        A = diffusion(dims, seed=2)
        b = np.random.default_rng(99).standard_normal(A.shape[0])
        for a in (A.indptr, A.indices, A.data, b):
            a.setflags(write=False)
        _OPS[name] = (dims, levels, A, b, T.Twin(A, dims, levels, omega=0.8, iters=2))
    return _OPS[name]


def pcg(twin, b, rtol, dtype, max_iters=200):
    """tensor_twin.Twin.pcg with the V-cycle in `dtype` (its input rounded to it, its result widened)
    and everything else in float64; returns (x, iters, relres of the recurrence)."""
    A = twin.A[0]

    def M(r):
        return np.asarray(twin.vcycle(np.zeros(r.size, dtype), r.astype(dtype), dtype)[0][0], np.float64)
    x = np.zeros(twin.n[0])
    r = b - A @ x
    bnorm = np.linalg.norm(b)
    rel = np.linalg.norm(r) / bnorm
    it = 0
    if rel <= rtol:
        return x, it, rel
    z = M(r)
    p = z.copy()
    rz = r @ z
    while it < max_iters:
        q = A @ p
        a = rz / (p @ q)
        x = x + a * p
        r = r - a * q
        it += 1
        rel = np.linalg.norm(r) / bnorm
        if not rel > rtol:
            break
        z = M(r)
        rzn = r @ z
        p = z + (rzn / rz) * p
        rz = rzn
    return x, it, rel


class ChebTwin(T.Twin):
    """tensor_twin.Twin with the Chebyshev smoother (include/amg_hip.h: cheb_lower) in place of true
    Jacobi: `iters` applications of the degree-k polynomial on [lower G, upper G], G = the Gershgorin
    bound of D^-1 A per level; coefficients formed in float64 and rounded to the cycle's dtype."""

    def __init__(self, A, dims, n_levels, degree=2, lower=0.3, upper=1.0, iters=1):
        super().__init__(A, dims, n_levels, iters=iters)
        self.coefs = []
        for M in self.A[:-1]:
            G = float(np.max(np.asarray(abs(M).sum(axis=1)).ravel() / np.abs(M.diagonal())))
            lo, hi = lower * G, upper * G
            theta, delta = (hi + lo) / 2, (hi - lo) / 2
            sigma = theta / delta
            rho = 1.0 / sigma
            alpha, beta = [0.0], [1.0 / theta]
            for _ in range(1, degree):
                rn = 1.0 / (2.0 * sigma - rho)
                alpha.append(rn * rho)
                beta.append(2.0 * rn / delta)
                rho = rn
            self.coefs.append((alpha, beta))

    def _smooth(self, l, off, dg, u, f, dtype):
        alpha, beta = self.coefs[l]
        for _ in range(self.iters):
            d = None
            for a, b in zip(alpha, beta):
                z = (f - off @ u) / dg - u
                d = dtype(b) * z if d is None else dtype(a) * d + dtype(b) * z
                u = u + d
        return u

    def vcycle(self, u0, f0, dtype=np.float64):
        A, P, R = self._mats(dtype)
        u, f = [None] * self.nl, [None] * self.nl
        u[0], f[0] = np.array(u0, dtype), np.array(f0, dtype)
        dg = [M.diagonal() for M in A]
        off = self._off(dtype)
        for l in range(self.nl - 1):
            u[l] = self._smooth(l, off[l], dg[l], u[l], f[l], dtype)
            r = f[l] - A[l] @ u[l]
            u[l + 1] = np.zeros(self.n[l + 1], dtype)
            f[l + 1] = R[l] @ r
        u[-1] = self.coarse_solve(f[-1], dtype)
        for l in range(self.nl - 2, -1, -1):
            u[l] = u[l] + P[l] @ u[l + 1]
            u[l] = self._smooth(l, off[l], dg[l], u[l], f[l], dtype)
        return u, f


_CHEB = {}


def cheb_twin(name):
    if name not in _CHEB:
        dims, levels, A, _, _ = operator(name)
        _CHEB[name] = ChebTwin(A, dims, levels)
    return _CHEB[name]
