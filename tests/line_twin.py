"""TEST INFRASTRUCTURE: a numpy / scipy twin of the line smoother (AMG_HIP_SM_LINE_JACOBI) and of the
V-cycle that uses it.  The oracle has no line smoother, so the twin reads the hierarchy the library
built through its getters (get_coefficient_matrix, get_transfer, get_n_dofs) and replays the stride
rule, the sweep and the cycle.  The tridiagonal solves are a plain sequential Thomas walk along every
chain (all chains of a level advance together, one position at a time), in float64 or in
np.longdouble: the longdouble sweep is the reference the device is measured against, and the
distance of the float64 sweep from it is the yardstick of that measurement.  Never imported by the
product."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

assert np.finfo(np.longdouble).eps < 1e-18, "the twin needs an extended-precision long double"


def csr_of(colptr, rowind, val, rows, cols):
    """scipy CSR of a CSC triple (the library's and the oracle's format)."""
    return sp.csc_matrix((np.asarray(val, np.float64), np.asarray(rowind), np.asarray(colptr)),
                         shape=(rows, cols)).tocsr()


def stride_rule(A):
    """The largest distance d = |j - i| >= 1 whose weight w(d) = sum |a_ij| reaches
    (1 - 1e-9) max w; 1 for a matrix without off-diagonal entries."""
    A = sp.coo_matrix(A)
    d = np.abs(A.col.astype(np.int64) - A.row.astype(np.int64))
    off = d >= 1
    if not np.any(off):
        return 1
    w = np.bincount(d[off], weights=np.abs(A.data[off]))
    if w.max() <= 0.0:
        return 1
    return int(np.flatnonzero(w >= (1.0 - 1e-9) * w.max())[-1])


def tridiagonal_part(A, s):
    """(dl, dd, du): the entries of A at column offsets -s, 0, +s of every row (0 where absent)."""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    dd = A.diagonal(0)
    dl, du = np.zeros(n), np.zeros(n)
    if s < n:
        du[:n - s] = A.diagonal(s)
        dl[s:] = A.diagonal(-s)
    return dl, dd, du


def thomas(dl, dd, du, r, s, dtype=np.float64):
    """x with T x = r, T tridiagonal on each chain of rows c, c + s, c + 2s, ...: the sequential
    Thomas walk (no pivoting) along every chain, in `dtype`."""
    n = r.size
    dl, dd, du, r = (np.asarray(a, dtype=dtype) for a in (dl, dd, du, r))
    npos = (n + s - 1) // s
    cp = np.zeros(n, dtype=dtype)
    x = np.zeros(n, dtype=dtype)
    prev = None
    for p in range(npos):
        a, b = p * s, min((p + 1) * s, n)
        k = b - a
        if p == 0:
            den = dd[a:b]
            x[a:b] = r[a:b] / den
        else:
            den = dd[a:b] - dl[a:b] * cp[prev:prev + k]
            x[a:b] = (r[a:b] - dl[a:b] * x[prev:prev + k]) / den
        if np.any(den == 0) or not np.all(np.isfinite(den.astype(np.float64))):
            raise ZeroDivisionError(f"zero or non-finite pivot at position {p}")
        cp[a:b] = du[a:b] / den
        prev = a
    for p in range(npos - 2, -1, -1):
        a = p * s
        nxt = (p + 1) * s
        k = min(nxt + s, n) - nxt          # chains that have a row at position p + 1
        x[a:a + k] = x[a:a + k] - cp[a:a + k] * x[nxt:nxt + k]
    return x


def line_sweep(A, u, f, s, omega, iters=1, dtype=np.float64):
    """`iters` sweeps u <- u + omega T^-1 (f - A u) in `dtype` (the residual included)."""
    A = sp.csr_matrix(A)
    dl, dd, du = tridiagonal_part(A, s)
    Ad = A.astype(dtype)
    u = np.array(u, dtype=dtype, copy=True)
    f = np.asarray(f, dtype=dtype)
    w = dtype(omega)
    for _ in range(iters):
        r = f - Ad @ u
        u = u + w * thomas(dl, dd, du, r, s, dtype)
    return u


def sweep_bound(A, u, f, s, omega, iters):
    """(reference, e64): the longdouble sweep and the 2-norm distance of the float64 sweep from it."""
    ref = line_sweep(A, u, f, s, omega, iters, np.longdouble)
    e64 = float(np.linalg.norm(line_sweep(A, u, f, s, omega, iters, np.float64).astype(np.longdouble) - ref))
    return ref, e64


def within(got, ref, e64, u_scale, factor=8.0):
    """(ok, distance, bound, ratio to e64): the rule of the device tests, distance <= max(factor e64,
    1e-14 ||u||)."""
    dist = float(np.linalg.norm(np.asarray(got, np.longdouble) - ref))
    bound = max(factor * e64, 1e-14 * float(u_scale))
    return dist <= bound, dist, bound, (dist / e64 if e64 > 0 else float("inf") if dist > 0 else 0.0)


def dense_solve(M, b, dtype):
    """Gaussian elimination with partial pivoting in `dtype` (numpy.linalg has no longdouble)."""
    M = np.array(M, dtype=dtype)
    x = np.array(b, dtype=dtype)
    n = x.size
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        if p != k:
            M[[k, p]] = M[[p, k]]
            x[[k, p]] = x[[p, k]]
        m = M[k + 1:, k] / M[k, k]
        M[k + 1:, k:] -= m[:, None] * M[k, k:][None, :]
        x[k + 1:] -= m * x[k]
    for k in range(n - 1, -1, -1):
        x[k] = (x[k] - M[k, k + 1:] @ x[k + 1:]) / M[k, k]
    return x


class Twin:
    """The hierarchy of a Multigrid (its getters) and the V-cycle (multigrid.hpp:263-305) with the
    line smoother on it."""

    def __init__(self, mg, omega=0.7, smoother_iters=1):
        self.nl = mg.n_levels
        self.n = [mg.get_n_dofs(l) for l in range(self.nl)]
        self.A = [csr_of(*mg.get_coefficient_matrix(l), self.n[l], self.n[l]) for l in range(self.nl)]
        self.P = [csr_of(*mg.get_transfer(l, "P"), self.n[l], self.n[l + 1]) for l in range(self.nl - 1)]
        self.R = [csr_of(*mg.get_transfer(l, "R"), self.n[l + 1], self.n[l]) for l in range(self.nl - 1)]
        self.stride = [stride_rule(A) for A in self.A]
        self.omega, self.iters = omega, smoother_iters
        self.coarse = spla.splu(self.A[-1].tocsc())

    def coarse_solve(self, f, dtype):
        """float64: scipy's direct solve; longdouble: dense elimination in longdouble when the coarsest
        level is small enough (<= 256 rows), else the float64 solve."""
        if dtype is np.longdouble and self.n[-1] <= 256:
            return dense_solve(self.A[-1].toarray(), f, dtype)
        return self.coarse.solve(np.asarray(f, np.float64)).astype(dtype)

    def smooth(self, l, u, f, dtype=np.float64):
        return line_sweep(self.A[l], u, f, self.stride[l], self.omega, self.iters, dtype)

    def vcycle(self, u0, f0, dtype=np.float64):
        """One V-cycle from u0 on level 0 with right-hand side f0, in `dtype` (coarse_solve: the coarsest
        level too when it is small); returns (u, f) per level."""
        u, f = [None] * self.nl, [None] * self.nl
        u[0], f[0] = np.array(u0, dtype), np.array(f0, dtype)
        if self.nl == 1:
            u[0] = self.coarse_solve(f[0], dtype)
            return u, f
        for l in range(self.nl - 1):
            u[l] = self.smooth(l, u[l], f[l], dtype)
            r = f[l] - self.A[l].astype(dtype) @ u[l]
            u[l + 1] = np.zeros(self.n[l + 1], dtype)
            f[l + 1] = self.R[l].astype(dtype) @ r
        u[-1] = self.coarse_solve(f[-1], dtype)
        for l in range(self.nl - 2, -1, -1):
            u[l] = u[l] + self.P[l].astype(dtype) @ u[l + 1]
            u[l] = self.smooth(l, u[l], f[l], dtype)
        return u, f

    def cycles_to(self, f0, tol=1e-8, max_cycles=60):
        """(cycles, history): V-cycles from u = 0 until ||r|| / ||r0|| <= tol in the 2-norm (the square
        root of the library's rss ratio); history[k] = ||r|| / ||r0|| after k cycles."""
        A = self.A[0]
        u = np.zeros(self.n[0])
        r0 = float(np.linalg.norm(f0 - A @ u))
        hist = [1.0]
        for k in range(1, max_cycles + 1):
            u = self.vcycle(u, f0)[0][0]
            hist.append(float(np.linalg.norm(f0 - A @ u)) / r0)
            if hist[-1] <= tol:
                return k, hist
        return None, hist
