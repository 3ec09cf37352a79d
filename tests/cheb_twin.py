"""TEST INFRASTRUCTURE: a numpy / scipy twin of the Chebyshev smoother (AMG_HIP_SM_CHEBYSHEV) and of
the V-cycle that uses it.  The oracle has no Chebyshev smoother, so the twin reads the hierarchy the
library built through its getters (get_coefficient_matrix, get_transfer, get_n_dofs) and replays the
smoother and the cycle with scipy, the coarsest level by a scipy direct solve.  Never imported by
the product."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def csr_of(colptr, rowind, val, rows, cols):
    """scipy CSR of a CSC triple (the library's and the oracle's format)."""
    return sp.csc_matrix((np.asarray(val, np.float64), np.asarray(rowind), np.asarray(colptr)),
                         shape=(rows, cols)).tocsr()


def gershgorin(A):
    """max_i (sum_j |a_ij|) / |a_ii| of a CSR matrix, each row summed in ascending column order
    (one position of every row at a time: the library's order, so the bits agree).  Raises on a
    zero diagonal."""
    A = sp.csr_matrix(A)
    A.sort_indices()
    n = A.shape[0]
    ptr, col, val = A.indptr, A.indices, A.data
    cnt = np.diff(ptr)
    s = np.zeros(n)
    dg = np.zeros(n)
    rows = np.arange(n)
    for j in range(int(cnt.max()) if n else 0):
        live = cnt > j
        at = ptr[:-1][live] + j
        s[live] = s[live] + np.abs(val[at])
        on = col[at] == rows[live]
        dg[rows[live][on]] = val[at][on]
    if np.any(dg == 0.0):
        raise ValueError(f"zero diagonal in row {int(np.flatnonzero(dg == 0.0)[0])}")
    return float(np.max(s / np.abs(dg)))


def cheb_coefs(lo, hi, k):
    """(alpha, beta) of the k steps of one application, in include/amg_hip.h's order."""
    theta, delta = (hi + lo) / 2, (hi - lo) / 2
    sigma = theta / delta
    rho = 1.0 / sigma
    alpha, beta = [0.0], [1.0 / theta]
    for _ in range(1, k):
        rn = 1.0 / (2.0 * sigma - rho)
        alpha.append(rn * rho)
        beta.append(2.0 * rn / delta)
        rho = rn
    return alpha, beta


def cheb_smooth(A, u, f, lo, hi, degree, n_iters):
    """n_iters applications of the degree-k polynomial: per step t = (f - sum_{j!=i} a_ij u_j) / a_ii,
    d = alpha d + beta (t - u) (first step: beta (t - u)), u = u + d."""
    A = sp.csr_matrix(A)
    dg = A.diagonal()
    off = (A - sp.diags(dg)).tocsr()
    alpha, beta = cheb_coefs(lo, hi, degree)
    u = np.array(u, dtype=np.float64, copy=True)
    for _ in range(n_iters):
        d = None
        for j in range(degree):
            t = (f - off @ u) / dg
            z = t - u
            d = beta[j] * z if j == 0 else alpha[j] * d + beta[j] * z
            u = u + d
    return u


def jacobi_smooth(A, u, f, omega, n_iters):
    A = sp.csr_matrix(A)
    dg = A.diagonal()
    off = (A - sp.diags(dg)).tocsr()
    u = np.array(u, dtype=np.float64, copy=True)
    for _ in range(n_iters):
        u = u + omega * ((f - off @ u) / dg - u)
    return u


def residual_polynomial(A, lo, hi, degree):
    """p(D^-1 A) as a dense matrix, p(lam) = T_k((theta - lam) / delta) / T_k(sigma), through the
    eigendecomposition of the symmetric D^-1/2 A D^-1/2 (A SPD)."""
    A = np.asarray(A.todense() if sp.issparse(A) else A, dtype=np.float64)
    dg = np.diag(A)
    s = 1.0 / np.sqrt(dg)
    lam, V = np.linalg.eigh(s[:, None] * A * s[None, :])
    theta, delta = (hi + lo) / 2, (hi - lo) / 2
    T = np.polynomial.chebyshev.Chebyshev.basis(degree)
    p = T((theta - lam) / delta) / T(theta / delta)
    return (s[:, None] * (V * p[None, :]) @ V.T) / s[None, :]


class Twin:
    """The hierarchy of a Multigrid (its getters) and the V-cycle (multigrid.hpp:263-305) with the
    Chebyshev smoother on it."""

    def __init__(self, mg, degree=2, lower=0.3, upper=1.0, smoother_iters=1):
        self.nl = mg.n_levels
        self.n = [mg.get_n_dofs(l) for l in range(self.nl)]
        self.A = [csr_of(*mg.get_coefficient_matrix(l), self.n[l], self.n[l]) for l in range(self.nl)]
        self.P = [csr_of(*mg.get_transfer(l, "P"), self.n[l], self.n[l + 1]) for l in range(self.nl - 1)]
        self.R = [csr_of(*mg.get_transfer(l, "R"), self.n[l + 1], self.n[l]) for l in range(self.nl - 1)]
        self.G = [gershgorin(A) for A in self.A]
        self.bounds = [(lower * G, upper * G) for G in self.G]
        self.degree, self.iters = degree, smoother_iters
        self.coarse = spla.splu(self.A[-1].tocsc())

    def smooth(self, l, u, f):
        lo, hi = self.bounds[l]
        return cheb_smooth(self.A[l], u, f, lo, hi, self.degree, self.iters)

    def vcycle(self, u0, f0):
        """One V-cycle from u0 on level 0 with right-hand side f0; returns (u, f) per level."""
        u, f = [None] * self.nl, [None] * self.nl
        u[0], f[0] = np.array(u0, np.float64), np.array(f0, np.float64)
        for l in range(self.nl - 1):
            u[l] = self.smooth(l, u[l], f[l])
            r = f[l] - self.A[l] @ u[l]
            u[l + 1] = np.zeros(self.n[l + 1])
            f[l + 1] = self.R[l] @ r
        u[-1] = self.coarse.solve(f[-1])
        for l in range(self.nl - 2, -1, -1):
            u[l] = u[l] + self.P[l] @ u[l + 1]
            u[l] = self.smooth(l, u[l], f[l])
        return u, f

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
