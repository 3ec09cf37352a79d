"""TEST INFRASTRUCTURE: a numpy / scipy twin of the full-coarsening hierarchies (amg_hip_create_tensor)
and of the true-Jacobi V-cycle on them.  Nothing here reads the library: the coarsening rule
(m -> m // 2 per axis), the 1-D operator P1(m), the Kronecker products P = P1(nz) (x) P1(ny) (x) P1(nx),
R = P^T and the Galerkin chain R (A P) are written down again with scipy, so that the product's
operators can be compared with them entry for entry.  The cycle runs in float64 or np.longdouble: the
longdouble cycle is the reference the device is measured against, and the distance of the float64
cycle from it is the yardstick of that measurement (the rule of tests/line_twin.py).  Never imported
by the product."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

assert np.finfo(np.longdouble).eps < 1e-18, "the twin needs an extended-precision long double"


def csr_of(colptr, rowind, val, rows, cols):
    """scipy CSR of a CSC triple (the library's format)."""
    return sp.csc_matrix((np.asarray(val, np.float64), np.asarray(rowind), np.asarray(colptr)),
                         shape=(rows, cols)).tocsr()


def dims3(dims):
    dims = tuple(int(x) for x in dims)
    return dims + (1,) * (3 - len(dims))


def coarse_dims(dims, dim):
    """Every coarsened axis m -> m // 2; a 2-D grid keeps nz = 1."""
    d = dims3(dims)
    return (d[0] // 2, d[1] // 2, d[2] // 2 if dim == 3 else 1)


def max_levels(dims, dim):
    """Levels possible: one more while every coarsened axis has at least 2 points."""
    d, n = dims3(dims), 1
    while min(d[:dim]) >= 2:
        d, n = coarse_dims(d, dim), n + 1
    return n


def level_dims(dims, dim, n_levels):
    out = [dims3(dims)]
    for _ in range(n_levels - 1):
        out.append(coarse_dims(out[-1], dim))
    return out


def P1(m):
    """m x (m // 2): column j holds 0.5, 1.0, 0.5 on rows 2j, 2j+1, 2j+2, each guarded by < m."""
    rows, cols, vals = [], [], []
    for j in range(m // 2):
        for t, w in enumerate((0.5, 1.0, 0.5)):
            if 2 * j + t < m:
                rows.append(2 * j + t)
                cols.append(j)
                vals.append(w)
    return sp.csc_matrix((vals, (rows, cols)), shape=(m, m // 2))


def tensor_P(dims, dim):
    """P1(nz) (x) P1(ny) (x) P1(nx) as CSC with sorted indices (x fastest: the x factor comes last)."""
    nx, ny, nz = dims3(dims)
    P = sp.kron(P1(ny), P1(nx), format="csc")
    if dim == 3:
        P = sp.kron(P1(nz), P, format="csc")
    P.sort_indices()
    return P


def csc_triple(M):
    M = sp.csc_matrix(M)
    M.sort_indices()
    return M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.astype(np.float64)


def jacobi(off, dg, u, f, omega, iters, dtype):
    """`iters` sweeps u <- u + omega ((f - sum_{j != i} a_ij u_j) / a_ii - u) in `dtype`; `off` = A
    without its diagonal."""
    w = dtype(omega)
    for _ in range(iters):
        u = u + w * ((f - off @ u) / dg - u)
    return u


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
    """Hierarchy of A (scipy, any format) on the grid `dims` with `n_levels` levels, and the V-cycle
    (multigrid.hpp:263-305) with true Jacobi `iters` + `iters` on it."""

    def __init__(self, A, dims, n_levels, omega=0.8, iters=2):
        self.dim = len(tuple(dims))
        assert self.dim in (2, 3)
        assert n_levels <= max_levels(dims, self.dim), "more levels than the grid allows"
        self.nl = n_levels
        self.dims = level_dims(dims, self.dim, n_levels)
        self.n = [d[0] * d[1] * d[2] for d in self.dims]
        self.A = [sp.csr_matrix(A, dtype=np.float64)]
        assert self.A[0].shape == (self.n[0], self.n[0])
        self.P, self.R = [], []
        for l in range(n_levels - 1):
            P = tensor_P(self.dims[l], self.dim)
            self.P.append(P.tocsr())
            self.R.append(P.T.tocsr())
            self.A.append((self.R[l] @ (self.A[l] @ self.P[l])).tocsr())
        self.omega, self.iters = omega, iters
        self.coarse = spla.splu(self.A[-1].tocsc())
        self._ld = {}

    def _mats(self, dtype):
        if dtype is np.float64:
            return self.A, self.P, self.R
        if dtype not in self._ld:
            self._ld[dtype] = ([M.astype(dtype) for M in self.A], [M.astype(dtype) for M in self.P],
                               [M.astype(dtype) for M in self.R])
        return self._ld[dtype]

    def _off(self, dtype):
        key = ("off", dtype)
        if key not in self._ld:
            self._ld[key] = [(M - sp.diags(M.diagonal())).tocsr().astype(dtype) for M in self.A]
        return self._ld[key]

    def complexity(self):
        return sum(M.nnz for M in self.A) / self.A[0].nnz

    def coarse_solve(self, f, dtype):
        """float64: scipy's direct solve; longdouble: dense elimination in longdouble when the coarsest
        level is small enough (<= 256 rows), else the float64 solve."""
        if dtype is np.longdouble and self.n[-1] <= 256:
            return dense_solve(self.A[-1].toarray(), f, dtype)
        return self.coarse.solve(np.asarray(f, np.float64)).astype(dtype)

    def vcycle(self, u0, f0, dtype=np.float64):
        """One V-cycle from u0 with right-hand side f0 in `dtype`; returns (u, f) per level."""
        A, P, R = self._mats(dtype)
        u, f = [None] * self.nl, [None] * self.nl
        u[0], f[0] = np.array(u0, dtype), np.array(f0, dtype)
        if self.nl == 1:
            u[0] = self.coarse_solve(f[0], dtype)
            return u, f
        dg = [M.diagonal() for M in A]
        off = self._off(dtype)
        for l in range(self.nl - 1):
            u[l] = jacobi(off[l], dg[l], u[l], f[l], self.omega, self.iters, dtype)
            r = f[l] - A[l] @ u[l]
            u[l + 1] = np.zeros(self.n[l + 1], dtype)
            f[l + 1] = R[l] @ r
        u[-1] = self.coarse_solve(f[-1], dtype)
        for l in range(self.nl - 2, -1, -1):
            u[l] = u[l] + P[l] @ u[l + 1]
            u[l] = jacobi(off[l], dg[l], u[l], f[l], self.omega, self.iters, dtype)
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

    def pcg(self, b, rtol, max_iters=200):
        """CG on A_0 x = b from x = 0, preconditioned with one V-cycle from zero (amg_hip_pcg's
        algorithm and stopping rule); returns (x, iters, relres)."""
        A = self.A[0]
        x = np.zeros(self.n[0])
        r = b - A @ x
        bnorm = np.linalg.norm(b)
        rel = np.linalg.norm(r) / bnorm
        it = 0
        if rel <= rtol:
            return x, it, rel
        z = self.vcycle(np.zeros_like(r), r)[0][0]
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
            z = self.vcycle(np.zeros_like(r), r)[0][0]
            rzn = r @ z
            p = z + (rzn / rz) * p
            rz = rzn
        return x, it, rel


def within(got, ref, e64, u_scale, factor=8.0):
    """(ok, distance, bound, ratio to e64): distance <= max(factor e64, 1e-14 ||u||)."""
    dist = float(np.linalg.norm(np.asarray(got, np.longdouble) - ref))
    bound = max(factor * e64, 1e-14 * float(u_scale))
    return dist <= bound, dist, bound, (dist / e64 if e64 > 0 else float("inf") if dist > 0 else 0.0)
