"""TEST INFRASTRUCTURE: a numpy / scipy twin of the tensor hierarchies with NATURAL boundary sides
(amg_hip_options.natural_sides / .singular).  tests/semi_twin.py's SemiTwin with a 6-bit side mask --
bit 2a = the low side of axis a (x = 0, y = 1, z = 2), bit 2a + 1 its high side -- and, for singular
operators, the pinned coarsest solve: the last unknown is 0 and the others solve the leading principal
block.  P1N(m; lo, hi) is tensor_twin.P1(m) whose boundary rows carry the weight 1.0 instead of 0.5 on
the flagged sides: row 0 when `lo`, row m - 1 of an odd m when `hi` (row m - 1 of an even m is a
coarse point).  The operator of the tests is semi_twin.diffusion's construction with shift 0 and
eps 1 whose Dirichlet face term is applied on the sides of a `dirichlet` mask only.  Nothing here
reads the library.  Never imported by the product."""
import os
import sys

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import semi_twin as S  # noqa: E402
import tensor_twin as T  # noqa: E402


def all_sides(dim):
    return (1 << (2 * dim)) - 1


def low_sides(dim):
    return sum(1 << (2 * a) for a in range(dim))


def high_sides(dim):
    return sum(1 << (2 * a + 1) for a in range(dim))


def P1N(m, lo, hi):
    """tensor_twin.P1(m) with entry (0, 0) = 1.0 when `lo` and, for odd m, entry (m - 1, m // 2 - 1)
    = 1.0 when `hi`; the pattern is P1's."""
    P = sp.lil_matrix(T.P1(m))
    if lo:
        assert P[0, 0] == 0.5
        P[0, 0] = 1.0
    if hi and m % 2 == 1:
        assert P[m - 1, m // 2 - 1] == 0.5
        P[m - 1, m // 2 - 1] = 1.0
    return sp.csc_matrix(P)


def natural_P(dims, dim, mask, sides):
    """P_z (x) P_y (x) P_x as CSC with sorted indices: P1N on the axes of `mask` with the side bits of
    the axis, the identity on the others."""
    d = T.dims3(dims)
    f = [P1N(d[a], (sides >> (2 * a)) & 1, (sides >> (2 * a + 1)) & 1) if a < dim and (mask >> a) & 1
         else sp.identity(d[a], format="csc") for a in range(3)]
    P = sp.kron(f[1], f[0], format="csc")
    if dim == 3:
        P = sp.kron(f[2], P, format="csc")
    P = sp.csc_matrix(P)
    P.sort_indices()
    return P


def diffusion(dims, dirichlet=0, seed=2):
    """semi_twin.diffusion(dims, eps = 1, seed, shift = 0) -- the same random stream, the same face
    term -- with the face term added on the sides of the `dirichlet` mask only; canonical scipy CSR.
    dirichlet = 0: every row sums to zero up to rounding and A is singular (constants)."""
    rng = np.random.default_rng(seed)
    dims = tuple(dims)
    n = int(np.prod(dims))
    idx = np.arange(n).reshape(dims[::-1])  # [z][y][x]
    diag = np.zeros(n)
    rows, cols, vals = [], [], []
    for axis in range(len(dims)):
        ax = len(dims) - 1 - axis
        lo = np.take(idx, np.arange(dims[axis] - 1), axis=ax).ravel()
        hi = np.take(idx, np.arange(1, dims[axis]), axis=ax).ravel()
        k = rng.uniform(1.0, 10.0, size=lo.size)
        edge = float(np.round(k.mean()))
        np.add.at(diag, lo, k)
        np.add.at(diag, hi, k)
        for b, side in enumerate((0, dims[axis] - 1)):
            if (dirichlet >> (2 * axis + b)) & 1:
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


def rhs(n, dirichlet=0, seed=99):
    """semi_twin.rhs, minus its mean when no side carries a Dirichlet condition (a consistent system)."""
    b = S.rhs(n, seed)
    return b if dirichlet else b - b.mean()


class NaturalTwin(S.SemiTwin):
    """SemiTwin with the side mask `sides` on every level.  masks: the explicit axis masks, or None
    for full coarsening with `n_levels` levels.  singular: the coarsest solve pins the last unknown."""

    def __init__(self, A, dims, n_levels=None, masks=None, sides=0, singular=False, omega=0.8, iters=2):
        self.dim = len(tuple(dims))
        assert self.dim in (2, 3)
        assert 0 <= sides <= all_sides(self.dim)
        assert not singular or sides == all_sides(self.dim)
        if masks is None:
            masks = [S.full_mask(self.dim)] * (n_levels - 1)
        self.sides, self.singular = int(sides), bool(singular)
        self.dims = [T.dims3(dims)]
        self.A = [sp.csr_matrix(A, dtype=np.float64)]
        self.n = [self.A[0].shape[0]]
        assert self.n[0] == int(np.prod(self.dims[0]))
        self.P, self.R, self.masks, self.w = [], [], [], []
        for l, m in enumerate(int(x) for x in masks):
            assert S.mask_error(self.dims[l], self.dim, m) is None, (l, m, self.dims[l])
            P = natural_P(self.dims[l], self.dim, m, self.sides)
            self.masks.append(m)
            self.P.append(P.tocsr())
            self.R.append(P.T.tocsr())
            self.A.append((self.R[l] @ (self.A[l] @ self.P[l])).tocsr())
            self.dims.append(S.coarse_dims(self.dims[l], self.dim, m))
            self.n.append(self.A[-1].shape[0])
            assert self.n[-1] == int(np.prod(self.dims[-1]))
        self.nl = len(self.A)
        self.omega, self.iters = omega, iters
        nc = self.n[-1]
        self.lead = self.A[-1].tocsc()[:nc - 1, :nc - 1] if self.singular else None
        if self.singular:
            self.coarse = spla.splu(self.lead) if nc > 1 else None
        else:
            self.coarse = spla.splu(self.A[-1].tocsc())
        self._ld = {}

    def coarse_solve(self, f, dtype):
        if not self.singular:
            return super().coarse_solve(f, dtype)
        nc = self.n[-1]
        x = np.zeros(nc, dtype)
        if nc > 1:
            if dtype is np.longdouble and nc <= 257:
                x[:nc - 1] = T.dense_solve(self.lead.toarray(), np.asarray(f)[:nc - 1], dtype)
            else:
                x[:nc - 1] = self.coarse.solve(np.asarray(f[:nc - 1], np.float64)).astype(dtype)
        return x
