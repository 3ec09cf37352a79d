"""TEST INFRASTRUCTURE: a numpy / scipy twin of the alternating-direction line smoother
(AMG_HIP_SM_LINE_ALT) and of the V-cycle that uses it, on top of line_twin: the directions of a
grid, T_a with the entries across line ends zeroed, line_twin's sequential Thomas walk per
direction, in float64 or np.longdouble, and the cycle with the directions ascending on the way
down and descending on the way up.  Never imported by the product."""
import numpy as np
import scipy.sparse as sp

import line_twin as lt


def directions(dims):
    """[(stride, length)] of the axes of length >= 2 of the grid `dims` (x fastest), ascending."""
    out, st = [], 1
    for m in dims:
        if m >= 2:
            out.append((st, int(m)))
        st *= int(m)
    return out


def tridiagonal_part(A, s, m):
    """(dl, dd, du) of T_a: line_twin's part at offsets -s, 0, +s with the entries that join two
    different grid lines (position (i // s) % m at a line end) zeroed."""
    dl, dd, du = lt.tridiagonal_part(A, s)
    q = (np.arange(A.shape[0]) // s) % m
    dl[q == 0] = 0.0
    du[q == m - 1] = 0.0
    return dl, dd, du


def apply(A, u, f, dims, omega, iters=1, reverse=False, dtype=np.float64):
    """`iters` applications: one sub-sweep u <- u + omega T_a^-1 (f - A u) per direction, the residual
    from the current u, in `dtype`.  A grid without a direction does weighted Jacobi."""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    dirs = directions(dims)
    if not dirs:
        parts = [(n, (np.zeros(n), A.diagonal(0), np.zeros(n)))]
    else:
        parts = [(s, tridiagonal_part(A, s, m)) for s, m in dirs]
    if reverse:
        parts = parts[::-1]
    Ad = A.astype(dtype)
    u = np.array(u, dtype=dtype, copy=True)
    f = np.asarray(f, dtype=dtype)
    w = dtype(omega)
    for _ in range(iters):
        for s, (dl, dd, du) in parts:
            r = f - Ad @ u
            u = u + w * lt.thomas(dl, dd, du, r, s, dtype)
    return u


def sweep_bound(A, u, f, dims, omega, iters, reverse=False):
    """(reference, e64): the longdouble application and the distance of the float64 one from it."""
    ref = apply(A, u, f, dims, omega, iters, reverse, np.longdouble)
    e64 = float(np.linalg.norm(apply(A, u, f, dims, omega, iters, reverse, np.float64).astype(np.longdouble) - ref))
    return ref, e64


class Twin(lt.Twin):
    """line_twin's hierarchy reader and V-cycle with the alternating smoother: `dims[l]` the grid of
    level l (mg.level_dims)."""

    def __init__(self, mg, omega=0.8, smoother_iters=1):
        super().__init__(mg, omega, smoother_iters)
        self.dims = [tuple(mg.level_dims(l)) for l in range(self.nl)]
        self._post = False

    def smooth(self, l, u, f, dtype=np.float64):
        return apply(self.A[l], u, f, self.dims[l], self.omega, self.iters, self._post, dtype)

    def vcycle(self, u0, f0, dtype=np.float64):
        """lt.Twin.vcycle with the pre-smoother ascending and the post-smoother descending."""
        u, f = [None] * self.nl, [None] * self.nl
        u[0], f[0] = np.array(u0, dtype), np.array(f0, dtype)
        if self.nl == 1:
            u[0] = self.coarse_solve(f[0], dtype)
            return u, f
        self._post = False
        for l in range(self.nl - 1):
            u[l] = self.smooth(l, u[l], f[l], dtype)
            r = f[l] - self.A[l].astype(dtype) @ u[l]
            u[l + 1] = np.zeros(self.n[l + 1], dtype)
            f[l + 1] = self.R[l].astype(dtype) @ r
        u[-1] = self.coarse_solve(f[-1], dtype)
        self._post = True
        for l in range(self.nl - 2, -1, -1):
            u[l] = u[l] + self.P[l].astype(dtype) @ u[l + 1]
            u[l] = self.smooth(l, u[l], f[l], dtype)
        self._post = False
        return u, f


def diffusion(nx, ny, cx, cy):
    """5-point diffusion on an nx x ny grid (x fastest, Dirichlet) with harmonic-mean edge
    coefficients of the point coefficients cx, cy (arrays of shape (ny, nx)); CSR."""
    def hm(a, b):
        return 2.0 * a * b / (a + b)
    idx = np.arange(nx * ny).reshape(ny, nx)
    ex = hm(cx[:, :-1], cx[:, 1:])          # edge (x, y) - (x + 1, y)
    ey = hm(cy[:-1, :], cy[1:, :])          # edge (x, y) - (x, y + 1)
    diag = np.zeros((ny, nx))
    wl = np.concatenate([cx[:, :1], ex], axis=1)   # west edge of every point (boundary: own coefficient)
    we = np.concatenate([ex, cx[:, -1:]], axis=1)
    ws = np.concatenate([cy[:1, :], ey], axis=0)
    wn = np.concatenate([ey, cy[-1:, :]], axis=0)
    diag = wl + we + ws + wn
    rows = [idx.ravel(), idx[:, :-1].ravel(), idx[:, 1:].ravel(), idx[:-1, :].ravel(), idx[1:, :].ravel()]
    cols = [idx.ravel(), idx[:, 1:].ravel(), idx[:, :-1].ravel(), idx[1:, :].ravel(), idx[:-1, :].ravel()]
    vals = [diag.ravel(), -ex.ravel(), -ex.ravel(), -ey.ravel(), -ey.ravel()]
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))),
                         shape=(nx * ny, nx * ny))


def split_anisotropy(nx, ny, eps):
    """The operator of the smoother's convergence check: x coefficient 1 and y coefficient eps in the
    left half of the domain, the opposite in the right half."""
    left = (np.arange(nx) < nx // 2)[None, :] * np.ones((ny, 1), bool)
    cx = np.where(left, 1.0, eps)
    cy = np.where(left, eps, 1.0)
    return diffusion(nx, ny, cx, cy)
