"""TEST INFRASTRUCTURE: a numpy / scipy twin of the tensor hierarchies with PERIODIC axes
(amg_hip_create_tensor_periodic).  tests/natural_twin.py's NaturalTwin with a 3-bit periodic mask --
bit a = axis a (x = 0, y = 1, z = 2) -- on top of its side mask: on a coarsened periodic axis of
even length m >= 4 the 1-D factor is P1per(m), m x m/2 with 0.5, 1.0, 0.5 on rows 2j, 2j+1,
(2j+2) mod m of column j, i.e. tensor_twin.P1(m) plus the single entry (0, m/2 - 1) = 0.5; the other
coarsened axes keep P1N with their side bits and an axis outside the level's mask the identity.  The
pinned coarsest solve of singular operators is NaturalTwin's.  The operator of the tests is
natural_twin.diffusion's construction with m wrap-around edges instead of m - 1 edges on the
periodic axes and no face term there.  Nothing here reads the library.  Never imported by the
product."""
import os
import sys

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import natural_twin as N  # noqa: E402
import semi_twin as S  # noqa: E402
import tensor_twin as T  # noqa: E402


def all_axes(dim):
    return (1 << dim) - 1


def open_sides(dim, periodic):
    """Both side bits of every axis that is not periodic: what `singular` needs."""
    return sum(3 << (2 * a) for a in range(dim) if not (periodic >> a) & 1)


def P1per(m):
    """m x m/2 for even m >= 4: column j holds 0.5, 1.0, 0.5 on rows 2j, 2j+1, (2j+2) mod m."""
    assert m >= 4 and m % 2 == 0, m
    rows, cols, vals = [], [], []
    for j in range(m // 2):
        for t, w in enumerate((0.5, 1.0, 0.5)):
            rows.append((2 * j + t) % m)
            cols.append(j)
            vals.append(w)
    P = sp.csc_matrix((vals, (rows, cols)), shape=(m, m // 2))
    Q = sp.lil_matrix(T.P1(m))
    assert Q[0, m // 2 - 1] == 0.0
    Q[0, m // 2 - 1] = 0.5
    assert (sp.csc_matrix(Q) != P).nnz == 0  # P1(m) plus the one wrapped entry
    return P


def level_error(dims, dim, mask, periodic):
    """None, or the periodic axis that `mask` cannot coarsen on the grid `dims`."""
    d = T.dims3(dims)
    for a in range(dim):
        if (mask >> a) & 1 and (periodic >> a) & 1 and (d[a] < 4 or d[a] % 2):
            return "xyz"[a]
    return None


def periodic_P(dims, dim, mask, sides, periodic):
    """P_z (x) P_y (x) P_x as CSC with sorted indices: P1per on the periodic axes of `mask`, P1N with
    the side bits of the axis on its other axes, the identity outside it."""
    d = T.dims3(dims)
    f = []
    for a in range(3):
        if not (a < dim and (mask >> a) & 1):
            f.append(sp.identity(d[a], format="csc"))
        elif (periodic >> a) & 1:
            assert not (sides >> (2 * a)) & 3, "a periodic axis has no sides"
            f.append(P1per(d[a]))
        else:
            f.append(N.P1N(d[a], (sides >> (2 * a)) & 1, (sides >> (2 * a + 1)) & 1))
    P = sp.kron(f[1], f[0], format="csc")
    if dim == 3:
        P = sp.kron(f[2], P, format="csc")
    P = sp.csc_matrix(P)
    P.sort_indices()
    return P


def diffusion(dims, periodic=0, dirichlet=0, seed=2):
    """natural_twin.diffusion -- the same random stream per axis, the same face term on the sides of
    `dirichlet` -- with, on an axis of `periodic`, the m edges (i, (i + 1) mod m) instead of the m - 1
    edges (i, i + 1) and no face term; canonical scipy CSR (duplicate entries, which an axis of 2
    points produces, are summed)."""
    rng = np.random.default_rng(seed)
    dims = tuple(dims)
    n = int(np.prod(dims))
    idx = np.arange(n).reshape(dims[::-1])  # [z][y][x]
    diag = np.zeros(n)
    rows, cols, vals = [], [], []
    for axis in range(len(dims)):
        ax = len(dims) - 1 - axis
        m = dims[axis]
        per = bool((periodic >> axis) & 1)
        assert not (per and (dirichlet >> (2 * axis)) & 3), "a periodic axis has no sides"
        lo = np.take(idx, np.arange(m if per else m - 1), axis=ax).ravel()
        hi = np.take(idx, (np.arange(m) + 1) % m if per else np.arange(1, m), axis=ax).ravel()
        k = rng.uniform(1.0, 10.0, size=lo.size)
        edge = float(np.round(k.mean()))
        np.add.at(diag, lo, k)
        np.add.at(diag, hi, k)
        for b, side in enumerate((0, m - 1)):
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


def rhs(n, singular, seed=99):
    """semi_twin.rhs, minus its mean for a singular operator (a consistent system)."""
    b = S.rhs(n, seed)
    return b - b.mean() if singular else b


class PeriodicTwin(N.NaturalTwin):
    """NaturalTwin with the periodic mask `periodic` on every level.  masks: the explicit axis masks, or
    None for full coarsening with `n_levels` levels.  singular: the coarsest solve pins the last
    unknown (NaturalTwin.coarse_solve); it needs every side of the axes that are not periodic."""

    def __init__(self, A, dims, n_levels=None, masks=None, sides=0, periodic=0, singular=False, omega=0.8,
                 iters=2):
        self.dim = len(tuple(dims))
        assert self.dim in (2, 3)
        assert 0 <= periodic <= all_axes(self.dim)
        assert 0 <= sides <= N.all_sides(self.dim) and not (sides & ~open_sides(self.dim, periodic))
        assert not singular or sides == open_sides(self.dim, periodic)
        if masks is None:
            masks = [S.full_mask(self.dim)] * (n_levels - 1)
        self.sides, self.periodic, self.singular = int(sides), int(periodic), bool(singular)
        self.dims = [T.dims3(dims)]
        self.A = [sp.csr_matrix(A, dtype=np.float64)]
        self.n = [self.A[0].shape[0]]
        assert self.n[0] == int(np.prod(self.dims[0]))
        self.P, self.R, self.masks, self.w = [], [], [], []
        for l, m in enumerate(int(x) for x in masks):
            assert S.mask_error(self.dims[l], self.dim, m) is None, (l, m, self.dims[l])
            assert level_error(self.dims[l], self.dim, m, self.periodic) is None, (l, m, self.dims[l])
            P = periodic_P(self.dims[l], self.dim, m, self.sides, self.periodic)
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
