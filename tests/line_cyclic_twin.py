"""TEST INFRASTRUCTURE: a numpy / scipy twin of the alternating line smoother with CYCLIC lines
(opts->cyclic_lines, amg_hip_smooth_line_alt_per) and of the V-cycle that uses it on
periodic_twin.PeriodicTwin hierarchies.  line_alt_twin.apply with a `periodic` mask: a direction
along a periodic axis of length m >= 3 solves T_a = the open T_a plus the wrap entries alpha = A[i0,
i1], beta = A[i1, i0] of every grid line by the Sherman-Morrison steps of include/amg_hip.h:
T' (the open T_a with the diagonal d(i0) - gamma and d(i1) - alpha beta / gamma, gamma = -A[i0, i0]),
p = T'^-T v, den = 1 + q(i0) + (alpha / gamma) q(i1) with q = T'^-1 u, the corrected residual, and
line_twin.thomas with T', in float64 or np.longdouble (the set-up included).  Never imported by the
product."""
import numpy as np
import scipy.sparse as sp

import line_alt_twin as at
import line_twin as lt
import tensor_twin as T


def cyclic_mask(dims, periodic):
    """The axes of `periodic` that have 3 points or more on the grid `dims`."""
    return sum(1 << a for a, m in enumerate(dims) if (periodic >> a) & 1 and m >= 3)


def directions(dims, periodic=0):
    """[(stride, length, cyclic)] of the axes of length >= 2, ascending."""
    out, st = [], 1
    for a, m in enumerate(dims):
        if m >= 2:
            out.append((st, int(m), bool((periodic >> a) & 1 and m >= 3)))
        st *= int(m)
    return out


def line_rows(n, s, m):
    """(m, n / m) array: column k holds the rows of line k in ascending order; the lines ascend with
    their first row."""
    q = (np.arange(n) // s) % m
    i0 = np.flatnonzero(q == 0)
    return i0[None, :] + s * np.arange(m)[:, None]


def line_thomas(dl, dd, du, r, s, m, dtype):
    """line_twin.thomas on the lines of (s, m): the rows are handed over position by position (every
    line a chain of its own), which is the same arithmetic as the walk along the flat chains, whose
    dl and du are zero at the line ends."""
    rows = line_rows(r.size, s, m)
    flat = rows.ravel()
    x = lt.thomas(np.asarray(dl)[flat], np.asarray(dd)[flat], np.asarray(du)[flat], np.asarray(r)[flat],
                  rows.shape[1], dtype)
    out = np.zeros(r.size, dtype)
    out[flat] = x
    return out


def wrap_entries(A, s, m):
    """(i0, i1, alpha, beta, gamma) per line of (s, m): alpha = A[i0, i1], beta = A[i1, i0] (0 when
    absent), gamma = -A[i0, i0]."""
    A = sp.csr_matrix(A)
    rows = line_rows(A.shape[0], s, m)
    i0, i1 = rows[0], rows[-1]
    alpha = np.asarray(A[i0, i1]).ravel()
    beta = np.asarray(A[i1, i0]).ravel()
    gamma = -A.diagonal()[i0]
    return i0, i1, alpha, beta, gamma


def cyclic_T(A, s, m):
    """The cyclic T_a, explicitly assembled: the open T_a plus the two wrap entries of every line."""
    n = A.shape[0]
    dl, dd, du = at.tridiagonal_part(A, s, m)
    i0, i1, alpha, beta, _ = wrap_entries(A, s, m)
    M = sp.diags([dl[s:], dd, du[:n - s]], [-s, 0, s], format="lil")
    M[i0, i1] = alpha
    M[i1, i0] = beta
    return sp.csr_matrix(M)


def setup(A, s, m, dtype):
    """The kept quantities of a cyclic direction in `dtype`: ((dl, dd', du) of T', p, den, gamma, beta,
    i0, i1, rows)."""
    n = A.shape[0]
    dl, dd, du = (np.asarray(a, dtype) for a in at.tridiagonal_part(A, s, m))
    i0, i1, alpha, beta, gamma = wrap_entries(A, s, m)
    alpha, beta, gamma = (np.asarray(a, dtype) for a in (alpha, beta, gamma))
    dd = dd.copy()
    dd[i0] = dd[i0] - gamma
    dd[i1] = dd[i1] - alpha * beta / gamma
    u, v = np.zeros(n, dtype), np.zeros(n, dtype)
    u[i0], u[i1] = gamma, beta
    v[i0], v[i1] = dtype(1), alpha / gamma
    tl, tu = np.zeros(n, dtype), np.zeros(n, dtype)  # T'^T: the lower entry of row i is the upper of row i - s
    tl[s:] = du[:n - s]
    tu[:n - s] = dl[s:]
    p = line_thomas(tl, dd, tu, v, s, m, dtype)
    q = line_thomas(dl, dd, du, u, s, m, dtype)
    den = (dtype(1) + q[i0]) + (alpha / gamma) * q[i1]
    if np.any(den == 0) or not np.all(np.isfinite(den.astype(np.float64))):
        raise ZeroDivisionError("zero or non-finite Sherman-Morrison denominator")
    return (dl, dd, du), p, den, gamma, beta, i0, i1, line_rows(n, s, m)


def cyclic_solve(parts, r, s, m, dtype):
    """T_a^-1 r by steps 2 and 3 of a sub-sweep; the sum over a line ascends along it."""
    (dl, dd, du), p, den, gamma, beta, i0, i1, rows = parts
    acc = np.zeros(rows.shape[1], dtype)
    for k in range(m):
        acc = acc + p[rows[k]] * r[rows[k]]
    fac = acc / den
    r = r.copy()
    r[i0] = r[i0] - fac * gamma
    r[i1] = r[i1] - fac * beta
    return line_thomas(dl, dd, du, r, s, m, dtype)


def apply(A, u, f, dims, periodic, omega, iters=1, reverse=False, dtype=np.float64, cache=None):
    """line_alt_twin.apply with cyclic lines on the axes of `periodic` of length >= 3.  periodic = 0 is
    line_alt_twin.apply itself.  cache: a dict that keeps the set-up of the directions between calls
    (the open directions then take line_thomas, the same arithmetic in fewer numpy calls)."""
    dirs = directions(dims, periodic)
    if not dirs or (cache is None and not cyclic_mask(dims, periodic)):
        return at.apply(A, u, f, dims, omega, iters, reverse, dtype)
    A = sp.csr_matrix(A)
    cache = {} if cache is None else cache
    for s, m, cyc in dirs:
        if (s, dtype) not in cache:
            cache[(s, dtype)] = setup(A, s, m, dtype) if cyc else at.tridiagonal_part(A, s, m)
    if ("A", dtype) not in cache:
        cache[("A", dtype)] = A.astype(dtype)
    Ad = cache[("A", dtype)]
    u = np.array(u, dtype=dtype, copy=True)
    f = np.asarray(f, dtype=dtype)
    w = dtype(omega)
    for _ in range(iters):
        for s, m, cyc in (dirs[::-1] if reverse else dirs):
            r = f - Ad @ u
            if cyc:
                u = u + w * cyclic_solve(cache[(s, dtype)], r, s, m, dtype)
            else:
                dl, dd, du = cache[(s, dtype)]
                u = u + w * line_thomas(dl, dd, du, r, s, m, dtype)
    return u


def sweep_bound(A, u, f, dims, periodic, omega, iters, reverse=False):
    """(reference, e64): the longdouble application and the distance of the float64 one from it."""
    ref = apply(A, u, f, dims, periodic, omega, iters, reverse, np.longdouble)
    got = apply(A, u, f, dims, periodic, omega, iters, reverse, np.float64)
    return ref, float(np.linalg.norm(got.astype(np.longdouble) - ref))


class Twin(at.Twin):
    """The V-cycle of line_alt_twin.Twin (directions ascending on the way down, descending on the way
    up) on the hierarchy of a periodic_twin.PeriodicTwin `pt`, with cyclic lines along its periodic
    axes (cyclic=False: open lines, opts->cyclic_lines = 0)."""

    def __init__(self, pt, omega=0.8, smoother_iters=1, cyclic=True):
        self.pt = pt
        self.nl, self.n, self.A, self.P, self.R = pt.nl, pt.n, pt.A, pt.P, pt.R
        self.dims = [tuple(d) for d in pt.dims]
        self.omega, self.iters = omega, smoother_iters
        self.periodic = pt.periodic if cyclic else 0
        self._post = False
        self._cache = [dict() for _ in range(self.nl)]

    def mask(self, l):
        """What amg_hip_line_cyclic reports on level l."""
        return cyclic_mask(self.dims[l], self.periodic)

    def coarse_solve(self, f, dtype):
        return self.pt.coarse_solve(f, dtype)

    def smooth(self, l, u, f, dtype=np.float64):
        return apply(self.A[l], u, f, self.dims[l], self.periodic, self.omega, self.iters, self._post, dtype,
                     self._cache[l])

    pcg = T.Twin.pcg


def scaled_diffusion(dims, eps, periodic=0):
    """Constant-coefficient diffusion: eps[a] times the 1-D (-1, 2, -1) operator along axis a, cyclic
    on the axes of `periodic`, Dirichlet on every other side; canonical CSR."""
    A = None
    for a, m in enumerate(dims):
        T1 = sp.lil_matrix(sp.diags([-np.ones(m - 1), 2.0 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1]))
        if (periodic >> a) & 1:
            assert m >= 3
            T1[0, m - 1] = T1[m - 1, 0] = -1.0
        T1 = eps[a] * sp.csr_matrix(T1)
        A = T1 if A is None else sp.kron(sp.identity(m), A) + sp.kron(T1, sp.identity(A.shape[0]))
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    return A


def upwind(dims, axis, periodic):
    """A first-order upwind difference u_i - u_(i-1) along `axis` (cyclic when the axis is periodic):
    what makes an operator nonsymmetric along its lines."""
    D = None
    for a, m in enumerate(dims):
        if a == axis:
            T1 = sp.lil_matrix(sp.diags([-np.ones(m - 1), np.ones(m)], [-1, 0]))
            if (periodic >> a) & 1:
                T1[0, m - 1] = -1.0
            T1 = sp.csr_matrix(T1)
        else:
            T1 = sp.identity(m, format="csr")
        D = T1 if D is None else sp.kron(T1, D)
    D = sp.csr_matrix(D)
    D.sort_indices()
    return D
