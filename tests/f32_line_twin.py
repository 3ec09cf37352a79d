"""TEST INFRASTRUCTURE: the line smoothers of the single-precision cycle (amg_hip_set_f32_lines; kernels.hip:
the K-Line, K-LineX and K-LineSeam solve kernels instantiated on float) restated in numpy float32, on top
of f32_twin (the float residual and transfers), line_twin, line_alt_twin and line_cyclic_twin.

What the device does and the twin repeats:
  factors   no float elimination.  The factors come from the FLOAT64 sequential elimination along every
            line, piv = dd - dl carry, ip = 1 / piv, cp = du ip (the carry is the cp of the row before),
            and are rounded with astype(float32).  A cyclic direction eliminates T' and keeps p, den,
            gamma, beta of line_cyclic_twin.setup, rounded the same way.
  solve     forward y = (r - dl y_) ip, backward x = y - cp x+, then u + omega x with omega rounded to
            float32: one float32 ufunc per operation, no fused multiply-add.
  sub-sweep the float residual of f32_twin, the seam correction where the direction is cyclic, the solve.
  cycle     enqueue_f32_vcycle's order with the directions ascending on the way down and descending on
            the way up; the coarsest solve in double between two roundings.

Everything runs in float32 or in np.longdouble (the reference; its solves are line_twin's and
line_cyclic_twin's own, from the exact entries).  K-LineX walks a line exactly in this order, so with
the device's own float factors the twin's x sub-sweep has the device's bits; K-Line (segments and a
Schur complement on the separators) and the seam's lane sums take another order and are compared by
accuracy: with e32 the distance of the float32 twin from the longdouble one, the device must lie
within max(8 e32, 1e-6 ||u||) of the longdouble result (line_twin.within's factor, its floor scaled
to float epsilon).  Never imported by the product."""
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import f32_twin as FT  # noqa: E402
import line_alt_twin as at  # noqa: E402
import line_cyclic_twin as ct  # noqa: E402
import line_twin as lt  # noqa: E402

F = np.float32
LD = np.longdouble


def _is(a, dtype):
    assert isinstance(a, np.ndarray) and a.dtype == dtype, (getattr(a, "dtype", type(a)), dtype)
    return a


def factors64(dl, dd, du, s):
    """(dl, ip, cp) in float64 of the tridiagonal rows (dl, dd, du) on the flat chains of stride s:
    piv = dd - dl carry, ip = 1 / piv, cp = du ip, position by position."""
    dl, dd, du = (_is(np.asarray(a), np.float64) for a in (dl, dd, du))
    n = dd.size
    ip, cp = np.zeros(n), np.zeros(n)
    prev = 0
    for p in range((n + s - 1) // s):
        a, b = p * s, min((p + 1) * s, n)
        carry = cp[prev:prev + b - a] if p else np.zeros(b - a)
        piv = np.subtract(dd[a:b], np.multiply(dl[a:b], carry))
        if np.any(piv == 0) or not np.all(np.isfinite(piv)):
            raise ZeroDivisionError(f"zero or non-finite pivot at position {p}")
        ip[a:b] = np.divide(1.0, piv)
        cp[a:b] = np.multiply(du[a:b], ip[a:b])
        prev = a
    return dl.copy(), ip, cp


def walk(dl, ip, cp, r, s, dtype):
    """(x, y) on the flat chains of stride s in `dtype`: y = (r - dl y_) ip forwards (y_ = 0 before a
    chain), x = y - cp x+ backwards (x+ = 0 after it).  One ufunc per operation."""
    dl, ip, cp, r = (_is(np.asarray(a), dtype) for a in (dl, ip, cp, r))
    n = r.size
    npos = (n + s - 1) // s
    y = np.zeros(n, dtype)
    prev = 0
    for p in range(npos):
        a, b = p * s, min((p + 1) * s, n)
        ym = y[prev:prev + b - a] if p else np.zeros(b - a, dtype)
        y[a:b] = np.multiply(np.subtract(r[a:b], np.multiply(dl[a:b], ym)), ip[a:b])
        prev = a
    x = np.zeros(n, dtype)
    for p in range(npos - 1, -1, -1):
        a, b = p * s, min((p + 1) * s, n)
        xp = np.zeros(b - a, dtype)
        k = max(0, min(b + s, n) - b)          # chains that have a row at position p + 1
        xp[:k] = x[b:b + k]
        x[a:b] = np.subtract(y[a:b], np.multiply(cp[a:b], xp))
    return _is(x, dtype), _is(y, dtype)


class Direction:
    """One direction of a level: the rows in walking order (`perm`: position by position, `stride`
    chains side by side), its float64 factors, and for a cyclic direction the float64 seam quantities."""

    def __init__(self, A, s, m, cyclic=False, flat=False):
        A = sp.csr_matrix(A)
        n = A.shape[0]
        self.A, self.s, self.m, self.cyclic, self.flat = A, int(s), m, bool(cyclic), flat
        if flat:                               # AMG_HIP_SM_LINE_JACOBI: chains on the flat index, no line ends
            self.perm, self.stride = np.arange(n), min(int(s), n)
            rows = lt.tridiagonal_part(A, s)
        else:
            lines = ct.line_rows(n, s, m)
            self.perm, self.stride = lines.ravel(), lines.shape[1]
            self.lines = lines
            if cyclic:
                rows, p, den, gamma, beta, i0, i1, _ = ct.setup(A, s, m, np.float64)
                self.p, self.den, self.gamma, self.beta, self.i0, self.i1 = p, den, gamma, beta, i0, i1
            else:
                rows = at.tridiagonal_part(A, s, m)
        self.rows64 = tuple(np.asarray(a, np.float64) for a in rows)
        f = factors64(*(a[self.perm] for a in self.rows64), self.stride)
        self.factors = tuple(self._back(a) for a in f)   # (dl, ip, cp), float64, in row order
        self._ld = None

    def _back(self, a):
        out = np.zeros(a.size, a.dtype)
        out[self.perm] = a
        return out

    def factors32(self):
        return tuple(a.astype(F) for a in self.factors)

    def solve32(self, r, factors=None):
        """(x, y, r after the seam) in float32; factors: float32 (dl, ip, cp) in row order (the device's
        own), else the rounded float64 ones."""
        r = _is(r, F)
        if self.cyclic:
            p, den, gamma, beta = (a.astype(F) for a in (self.p, self.den, self.gamma, self.beta))
            acc = np.zeros(self.stride, F)
            for k in range(self.m):            # ascending along every line
                acc = np.add(acc, np.multiply(p[self.lines[k]], r[self.lines[k]]))
            fac = np.divide(acc, den)
            r = r.copy()
            r[self.i0] = np.subtract(r[self.i0], np.multiply(fac, gamma))
            r[self.i1] = np.subtract(r[self.i1], np.multiply(fac, beta))
        dl, ip, cp = self.factors32() if factors is None else (_is(a, F) for a in factors)
        x, y = walk(dl[self.perm], ip[self.perm], cp[self.perm], r[self.perm], self.stride, F)
        return self._back(x), self._back(y), r

    def solve_ld(self, r):
        """T^-1 r in longdouble from the exact entries: line_twin's and line_cyclic_twin's own solves"""
        r = _is(r, LD)
        if self.flat:
            return lt.thomas(*self.rows64, r, self.s, LD)
        if self.cyclic:
            if self._ld is None:
                self._ld = ct.setup(self.A, self.s, self.m, LD)
            return ct.cyclic_solve(self._ld, r, self.s, self.m, LD)
        return ct.line_thomas(*self.rows64, r, self.s, self.m, LD)


class Level:
    """A level matrix with the directions of its smoother.  kind "alt": the axes of length >= 2 of `dims`
    (cyclic where `periodic` says so and the axis has 3 points or more), or weighted Jacobi where there is
    none; kind "jacobi": the one flat direction of line_twin's stride rule."""

    def __init__(self, A, kind, dims=None, periodic=0):
        self.A = sp.csr_matrix(A, dtype=np.float64)
        self.A.sort_indices()
        self.n = self.A.shape[0]
        self.rows = FT.Rows(self.A)
        self.Ald = self.A.astype(LD)
        if kind == "jacobi":
            self.dirs = [Direction(self.A, lt.stride_rule(self.A), None, flat=True)]
        else:
            d = ct.directions(dims, periodic)
            self.dirs = [Direction(self.A, s, m, cyc) for s, m, cyc in d] or \
                [Direction(self.A, self.n, None, flat=True)]   # every row its own chain
        self.x_direction = kind == "alt" and bool(ct.directions(dims, periodic)) and dims[0] >= 2

    def sub32(self, d, u, f, omega, factors=None):
        """(u, r): one float32 sub-sweep of direction d; r is what the device's float r holds after it
        (the forward values where the direction is x, else the residual after the seam)."""
        u, f = _is(u, F), _is(f, F)
        r = FT.residual(self.rows, u, f)
        x, y, r = self.dirs[d].solve32(r, factors)
        u = _is(np.add(u, np.multiply(F(omega), x)), F)
        return u, (y if self.x_direction and d == 0 else r)

    def sub_ld(self, d, u, f, omega):
        u, f = np.asarray(u, LD), np.asarray(f, LD)
        return u + LD(omega) * self.dirs[d].solve_ld(f - self.Ald @ u)

    def order(self, reverse):
        nd = len(self.dirs)
        return range(nd - 1, -1, -1) if reverse else range(nd)

    def smooth(self, u, f, omega, iters, reverse, dtype):
        for _ in range(iters):
            for d in self.order(reverse):
                u = self.sub32(d, u, f, omega)[0] if dtype is F else self.sub_ld(d, u, f, omega)
        return u


def sub_bound(L, d, u, f, omega):
    """(reference, e32) of one sub-sweep from float32 u, f: the longdouble result and the 2-norm distance
    of the float32 twin from it."""
    ref = L.sub_ld(d, u, f, omega)
    e32 = float(np.linalg.norm(L.sub32(d, u, f, omega)[0].astype(LD) - ref))
    return ref, e32


def within(got, ref, e32, u_scale, factor=8.0):
    """(ok, distance, bound, ratio to e32): distance <= max(factor e32, 1e-6 ||u||)"""
    dist = float(np.linalg.norm(np.asarray(got, LD) - ref))
    bound = max(factor * e32, 1e-6 * float(u_scale))
    return dist <= bound, dist, bound, (dist / e32 if e32 > 0 else float("inf") if dist > 0 else 0.0)


class Cycle:
    """The V-cycle with a line smoother on a hierarchy `src` (any of the twins: nl, n, A, P, R,
    coarse_solve(f, dtype); `dims` per level for kind "alt", src.periodic for cyclic lines) in float32,
    float64 or longdouble.  float32: f32_twin's residual and transfers, this file's sub-sweeps, the
    coarsest solve in float64 between two roundings.  The other two: the twins' own arithmetic."""

    def __init__(self, src, kind, omega, iters=1, periodic=0):
        self.src, self.kind, self.omega, self.iters, self.periodic = src, kind, omega, iters, periodic
        self.nl, self.n, self.A = src.nl, list(src.n), src.A
        self.dims = [tuple(d) for d in src.dims] if kind == "alt" else [None] * self.nl
        self.lv = [Level(src.A[l], kind, self.dims[l], periodic) for l in range(self.nl - 1)]
        self.R = [FT.Rows(M) for M in src.R]
        self.P = [FT.Rows(M) for M in src.P]
        self._cache = [dict() for _ in range(self.nl)]

    def _smooth(self, l, u, f, reverse, dtype):
        if dtype is F or dtype is LD:
            return self.lv[l].smooth(u, f, self.omega, self.iters, reverse, dtype)
        if self.kind == "jacobi":
            return lt.line_sweep(self.A[l], u, f, self.lv[l].dirs[0].s, self.omega, self.iters, dtype)
        return ct.apply(self.A[l], u, f, self.dims[l], self.periodic, self.omega, self.iters, reverse, dtype,
                        self._cache[l])

    def vcycle(self, u0, f0, dtype=np.float64):
        """(u, f) per level of one cycle from the zero guess u0 (tensor_twin.Twin.vcycle's signature, so
        that mixed_twin.pcg can drive it)."""
        assert not np.any(u0)
        nl = self.nl
        u, f = [None] * nl, [None] * nl
        if dtype is F:
            f[0] = FT.rounded(f0)
            u[0] = np.zeros(self.n[0], F)
            for l in range(nl - 1):
                u[l] = self._smooth(l, u[l], f[l], False, F)
                r = FT.residual(self.lv[l].rows, u[l], f[l])
                u[l + 1] = np.zeros(self.n[l + 1], F)
                f[l + 1] = FT.spmv(self.R[l], r)
            u[-1] = np.asarray(self.src.coarse_solve(f[-1].astype(np.float64), np.float64), np.float64).astype(F)
            for l in range(nl - 2, -1, -1):
                u[l] = FT.spmv_add(self.P[l], u[l + 1], u[l])
                u[l] = self._smooth(l, u[l], f[l], True, F)
            for a in u + f:
                _is(a, F)
            return u, f
        u[0], f[0] = np.zeros(self.n[0], dtype), np.array(f0, dtype)
        for l in range(nl - 1):
            u[l] = self._smooth(l, u[l], f[l], False, dtype)
            r = f[l] - self.A[l].astype(dtype) @ u[l]
            u[l + 1] = np.zeros(self.n[l + 1], dtype)
            f[l + 1] = self.src.R[l].astype(dtype) @ r
        u[-1] = self.src.coarse_solve(f[-1], dtype)
        for l in range(nl - 2, -1, -1):
            u[l] = u[l] + self.src.P[l].astype(dtype) @ u[l + 1]
            u[l] = self._smooth(l, u[l], f[l], True, dtype)
        return u, f

    def apply_bound(self, v):
        """(reference, e32, float32 result) of one application to the float64 vector v: the longdouble
        cycle on v rounded to float32 (what the device is given), and the float32 twin's distance."""
        v32 = FT.rounded(v)
        ref = self.vcycle(np.zeros(self.n[0], LD), v32.astype(LD), LD)[0][0]
        u32 = self.vcycle(np.zeros(self.n[0], F), v32, F)[0][0]
        return ref, float(np.linalg.norm(u32.astype(LD) - ref)), u32


def diffusion(dims, coef):
    """Diffusion on the grid `dims` (x fastest, 2-D or 3-D, Dirichlet) with the point coefficients coef[a]
    of axis a (arrays of shape dims[::-1]) and harmonic means on the edges; line_alt_twin.diffusion's
    rule in any dimension.  Canonical CSR."""
    dims = tuple(int(m) for m in dims)
    n = int(np.prod(dims))
    idx = np.arange(n).reshape(dims[::-1])
    diag = np.zeros(n)
    rows, cols, vals = [], [], []
    for a, m in enumerate(dims):
        ax = len(dims) - 1 - a
        c = np.asarray(coef[a], np.float64)
        lo, hi = np.take(idx, np.arange(m - 1), axis=ax).ravel(), np.take(idx, np.arange(1, m), axis=ax).ravel()
        cl, ch = np.take(c, np.arange(m - 1), axis=ax).ravel(), np.take(c, np.arange(1, m), axis=ax).ravel()
        e = 2.0 * cl * ch / (cl + ch)
        np.add.at(diag, lo, e)
        np.add.at(diag, hi, e)
        for side in (0, m - 1):                # boundary faces: the point's own coefficient
            np.add.at(diag, np.take(idx, [side], axis=ax).ravel(), np.take(c, [side], axis=ax).ravel())
        rows += [lo, hi]
        cols += [hi, lo]
        vals += [-e, -e]
    rows.append(np.arange(n))
    cols.append(np.arange(n))
    vals.append(diag)
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    A.sort_indices()
    return A


def split_anisotropy3(nx, ny, nz, eps):
    """The 3-D analogue of line_alt_twin.split_anisotropy: x coefficient 1 and y coefficient eps in the
    left half of the box (x < nx // 2), the opposite in the right half, z coefficient eps everywhere: one
    strong direction at every point, as in 2-D."""
    left = np.broadcast_to((np.arange(nx) < nx // 2)[None, None, :], (nz, ny, nx))
    cx = np.where(left, 1.0, eps)
    cy = np.where(left, eps, 1.0)
    return diffusion((nx, ny, nz), (cx, cy, np.full((nz, ny, nx), float(eps))))
