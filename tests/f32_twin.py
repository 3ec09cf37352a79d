"""TEST INFRASTRUCTURE: a numpy float32 restatement of the single-precision V-cycle (amg_hip_apply_f32;
kernels.hip: K-F32; solver.cpp: enqueue_f32_vcycle) that is meant to give the device's BITS.

Why that is possible: the library is built without FMA contraction, float division on the device is
the correctly rounded one and float denormals are kept, every row kernel sums a row in ascending column
order from a fixed start, and every transfer weight is a power of two.  So each kernel is a fixed
sequence of IEEE float32 operations per row, and numpy's float32 ufuncs are the same operations.

How it is written: a CSR matrix (sorted columns, values rounded with astype(float32), exact zeros
dropped -- for finite vectors they do not change a bit) is laid out as padded n x w index / value / mask
arrays and walked slot by slot, k = 0 .. w - 1: slot k of every row at once, which is each row's own
ascending-column order.  Every arithmetic step is ONE elementwise ufunc on float32 arrays (no `@`, no
scipy matvec, no sum, no einsum); np.where only selects.  Every array that takes part is float32, and
that is asserted.

Nothing here reads the library and nothing here is imported by the product.  The coarsest solve (the
solver's double solve between two roundings) is a callback: float64 vector -> float64 vector."""
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cheb_twin  # noqa: E402

F = np.float32


def _f(a):
    assert isinstance(a, np.ndarray) and a.dtype == np.float32, getattr(a, "dtype", type(a))
    return a


def rounded(v):
    """float64 (or any) vector -> float32 by IEEE round-to-nearest-even (the device's (float)x)."""
    return np.asarray(v).astype(np.float32)


class Rows:
    """The padded row layout of a matrix: idx, val, mask of shape (n, w), w = the longest row; row i's
    entries in ascending column order in slots 0 .. len_i - 1.  `diag`: the value on the diagonal (0
    where a row has none), `offd`: mask without the diagonal slots.  descending=True reverses each row
    (only to show that the comparison sees an order change)."""

    def __init__(self, M, descending=False):
        M = sp.csr_matrix(M).copy()
        M.sort_indices()
        keep = M.data != 0.0
        cnt_all = np.diff(M.indptr)
        rows = np.repeat(np.arange(M.shape[0]), cnt_all)[keep]
        cols = M.indices[keep].astype(np.int64)
        vals = M.data[keep].astype(np.float32)
        self.shape = M.shape
        n = M.shape[0]
        cnt = np.bincount(rows, minlength=n).astype(np.int64)
        self.cnt = cnt
        w = int(cnt.max()) if n and cnt.size else 0
        self.w = w
        start = np.concatenate([[0], np.cumsum(cnt)[:-1]]) if n else np.zeros(0, np.int64)
        slot = np.arange(rows.size) - start[rows]
        if descending:
            slot = cnt[rows] - 1 - slot
        self.idx = np.zeros((n, w), np.int64)
        self.val = np.zeros((n, w), np.float32)
        self.mask = np.zeros((n, w), bool)
        self.idx[rows, slot] = cols
        self.val[rows, slot] = vals
        self.mask[rows, slot] = True
        on = self.mask & (self.idx == np.arange(n)[:, None])
        self.offd = self.mask & ~on
        self.diag = np.zeros(n, np.float32)
        r_on, k_on = np.nonzero(on)
        self.diag[r_on] = self.val[r_on, k_on]


def _walk(R, x, acc, mask, subtract):
    """acc = acc +- val[:, k] * x[idx[:, k]] for k = 0 .. w - 1 under mask[:, k]"""
    _f(x), _f(acc)
    assert x.shape == (R.shape[1],) and acc.shape == (R.shape[0],)
    with np.errstate(all="ignore"):  # padded slots gather x[0]; np.where drops what they give
        for k in range(R.w):
            p = _f(np.multiply(R.val[:, k], x[R.idx[:, k]]))
            nxt = _f(np.subtract(acc, p) if subtract else np.add(acc, p))
            acc = np.where(mask[:, k], nxt, acc)
    return _f(acc)


def residual(R, x, f):
    """CSR_RESID: acc = f, acc = acc - v x per entry"""
    return _walk(R, x, _f(f).copy(), R.mask, True)


def spmv(R, x):
    """CSR_SPMV: acc = 0, acc = acc + v x per entry"""
    return _walk(R, x, np.zeros(R.shape[0], F), R.mask, False)


def spmv_add(R, x, f):
    """CSR_SPMV_ADD: f + (the SpMV's acc)"""
    return _f(np.add(_f(f), spmv(R, x)))


def _t(R, x, f):
    """(f - sum over the off-diagonal entries) / d, and x where d == 0 (f32_row_epilogue)"""
    acc = _walk(R, x, np.zeros(R.shape[0], F), R.offd, False)
    with np.errstate(all="ignore"):
        q = _f(np.divide(_f(np.subtract(_f(f), acc)), R.diag))
    return q


def jacobi(R, x, f, omega):
    """CSR_JACOBI: x + omega ((f - acc) / d - x), x where d == 0; omega rounded to float32"""
    w = F(omega)
    q = _t(R, x, f)
    with np.errstate(all="ignore"):
        out = _f(np.add(x, _f(np.multiply(w, _f(np.subtract(q, x))))))
    return _f(np.where(R.diag == 0.0, x, out))


def cheb_step(R, x, f, d, alpha, beta, first):
    """One Chebyshev step: t as Jacobi's (x where d == 0), z = t - x, d = beta z on a first step else
    alpha d + beta z, x + d.  Returns (x, d)."""
    a, b = F(alpha), F(beta)
    t = _f(np.where(R.diag == 0.0, x, _t(R, x, f)))
    z = _f(np.subtract(t, x))
    bz = _f(np.multiply(b, z))
    dn = bz if first else _f(np.add(_f(np.multiply(a, _f(d))), bz))
    return _f(np.add(x, dn)), dn


# ---- plain per-row loops in np.float32 scalars: what the padded walk is checked against -------------
def loop(M, mode, x, f=None, omega=None, d=None, alpha=None, beta=None, first=False):
    """The five modes one row at a time, one entry at a time, in np.float32 scalars; mode: "resid",
    "spmv", "spmv_add", "jacobi", "cheb".  Returns out, or (out, d) for "cheb"."""
    M = sp.csr_matrix(M)
    M.sort_indices()
    n = M.shape[0]
    val = M.data.astype(np.float32)
    out = np.zeros(n, F)
    dn = np.zeros(n, F)
    for i in range(n):
        acc = f[i] if mode == "resid" else F(0.0)
        dg = F(0.0)
        for p in range(M.indptr[i], M.indptr[i + 1]):
            c, v = M.indices[p], val[p]
            if mode == "resid":
                acc = F(acc - F(v * x[c]))
            elif mode in ("jacobi", "cheb") and c == i:
                dg = v
            else:
                acc = F(acc + F(v * x[c]))
        if mode in ("resid", "spmv"):
            out[i] = acc
        elif mode == "spmv_add":
            out[i] = F(f[i] + acc)
        elif mode == "jacobi":
            out[i] = x[i] if dg == 0.0 else F(x[i] + F(F(omega) * F(F(F(f[i] - acc) / dg) - x[i])))
        else:
            t = x[i] if dg == 0.0 else F(F(f[i] - acc) / dg)
            z = F(t - x[i])
            dn[i] = F(F(beta) * z) if first else F(F(F(alpha) * d[i]) + F(F(beta) * z))
            out[i] = F(x[i] + dn[i])
    return (out, dn) if mode == "cheb" else out


# ---- the cycle ---------------------------------------------------------------------------------
class Hierarchy:
    """What the float cycle needs of a hierarchy, as Rows:
      rows[l]   CSR(A_l): the residual and the Chebyshev steps
      cols[l]   the arrays of the CSC form of A_l read AS ROWS (A_l transposed): the Jacobi sweep's
                column walk.  On a bitwise symmetric level the same arrays as rows[l].
      R[l], P[l]  the transfers in CSR, walked in row order on every kind of level
    for l < L - 1; n[l] for every level.
    smoother: ("jacobi", omega, iters) or ("cheb", degree, iters, [(lo, hi) per level])
    coarse:   float64 vector -> float64 vector, the double solve on the coarsest level."""

    def __init__(self, A, P, R, smoother, coarse):
        """A: scipy matrices of the levels (the last one is only measured), P / R: scipy matrices"""
        self.nl = len(A)
        assert len(P) == len(R) == self.nl - 1
        self.n = [M.shape[0] for M in A]
        self.rows = [Rows(sp.csr_matrix(M)) for M in A[:-1]]
        self.cols = [Rows(sp.csr_matrix(sp.csc_matrix(M).T)) for M in A[:-1]]
        self.R = [Rows(M) for M in R]
        self.P = [Rows(M) for M in P]
        for l in range(self.nl - 1):
            assert self.R[l].shape == (self.n[l + 1], self.n[l]) and self.P[l].shape == (self.n[l], self.n[l + 1])
        self.smoother, self.coarse = smoother, coarse

    def symmetric(self, l):
        a, b = self.rows[l], self.cols[l]
        return a.w == b.w and np.array_equal(a.idx, b.idx) and np.array_equal(a.mask, b.mask) and \
            np.array_equal(a.val.view(np.uint32), b.val.view(np.uint32))

    def passes(self):
        """kernel launches of one smoothing"""
        return self.smoother[2] * (1 if self.smoother[0] == "jacobi" else self.smoother[1])

    def smooth(self, l, u, f):
        if self.smoother[0] == "jacobi":
            _, omega, iters = self.smoother
            for _ in range(iters):
                u = jacobi(self.cols[l], u, f, omega)
            return u
        _, k, iters, bounds = self.smoother
        alpha, beta = cheb_twin.cheb_coefs(bounds[l][0], bounds[l][1], k)
        for _ in range(iters):
            d = None
            for j in range(k):
                u, d = cheb_step(self.rows[l], u, f, d, alpha[j], beta[j], j == 0)
        return u

    def resid(self, l, u, f):
        return residual(self.rows[l], u, f)

    def restrict(self, l, r):
        return spmv(self.R[l], r)

    def prolong_add(self, l, uH, uh):
        return spmv_add(self.P[l], uH, uh)

    def coarse_solve(self, f):
        x = np.asarray(self.coarse(_f(f).astype(np.float64)))
        assert x.dtype == np.float64
        return x.astype(np.float32)


def cycle(H, v):
    """One float cycle from the zero guess on the right-hand side v (float64, rounded here) in
    enqueue_f32_vcycle's order.  Returns (u, f, r): lists per level of what the cycle leaves there;
    r[L - 1] is None (the coarsest level has no residual vector)."""
    nl = H.nl
    u, f, r = [None] * nl, [None] * nl, [None] * nl
    f[0] = rounded(v)
    u[0] = np.zeros(H.n[0], F)
    for l in range(nl - 1):
        u[l] = H.smooth(l, u[l], f[l])
        r[l] = H.resid(l, u[l], f[l])
        u[l + 1] = np.zeros(H.n[l + 1], F)
        f[l + 1] = H.restrict(l, r[l])
    u[-1] = H.coarse_solve(f[-1])
    for l in range(nl - 2, -1, -1):
        u[l] = H.prolong_add(l, u[l + 1], u[l])
        u[l] = H.smooth(l, u[l], f[l])
    for a in u + f + r[:-1]:
        _f(a)
    return u, f, r


def same_bits(a, b):
    a, b = _f(np.asarray(a)), _f(np.asarray(b))
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
