"""TEST INFRASTRUCTURE: a numpy / scipy twin of the hierarchies with operator-dependent interpolation
(amg_hip_create_tensor_opdep).  tests/semi_twin.py's SemiTwin with ONE coarsened axis per level and
the values of P taken from the rows of the level's matrix, collapsed onto that axis; the pattern is
semi_P's for the same mask.  The weight rule, the automatic rule and the operator of the tests (a
diffusion whose conductivity jumps by powers of ten from block to block) are written down again in
numpy.  Nothing here reads the library.  Never imported by the product."""
import os
import sys

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import semi_twin as S  # noqa: E402
import tensor_twin as T  # noqa: E402

MIN_COARSE, MAX_LEVELS = 32, 24


def axis_of(mask):
    assert mask in (1, 2, 4), mask
    return {1: 0, 2: 1, 4: 2}[mask]


def axis_coord(i, dims, axis):
    d = T.dims3(dims)
    stride = (1, d[0], d[0] * d[1])[axis]
    return (np.asarray(i, np.int64) // stride) % d[axis]


def collapsed_sums(A, dims, axis):
    """(s_m, s_0, s_p) per row: the entries of the row (structural zeros too) whose column has the axis
    coordinate c - 1, c, c + 1, added from +0.0 in ascending column order (np.add.at over the COO entries
    sorted by (row, column) adds in that order)."""
    M = sp.csr_matrix(A, dtype=np.float64)
    M.sort_indices()
    n = M.shape[0]
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(M.indptr))
    col = M.indices.astype(np.int64)
    dc = axis_coord(col, dims, axis) - axis_coord(row, dims, axis)
    out = []
    for want in (-1, 0, 1):
        s = np.zeros(n)
        k = dc == want
        np.add.at(s, row[k], M.data[k])
        out.append(s)
    return out


def opdep_P(A, dims, dim, mask):
    """(P as CSC with sorted indices, W): semi_P's pattern for `mask` (one axis) with the weights of A's
    rows.  Odd axis coordinate c: coarse point (c - 1) / 2, entry 1.0.  Even c: w_lo = (-s_m) / s_0 at
    coarse c / 2 - 1 when c >= 2, w_hi = (-s_p) / s_0 at coarse c / 2 when c + 1 < m, kept even when 0.0.
    W: the compact array, row e = (w_lo, w_hi) of the e-th fine point with even c, 0.0 where the
    neighbour does not exist.  ValueError naming the row for a zero / non-finite s_0 or weight."""
    axis = axis_of(mask)
    d = T.dims3(dims)
    m = d[axis]
    assert axis < dim and m >= 2
    n = d[0] * d[1] * d[2]
    cd = S.coarse_dims(d, dim, mask)
    sm, s0, sp_ = collapsed_sums(A, d, axis)
    i = np.arange(n, dtype=np.int64)
    c = axis_coord(i, d, axis)
    stride = (1, d[0], d[0] * d[1])[axis]
    cstride = (1, cd[0], cd[0] * cd[1])[axis]
    # coarse index of the point with the same other coordinates and axis coordinate 0
    rest = i - c * stride
    if axis == 0:
        cbase = (rest // d[0]) * cd[0]
    elif axis == 1:
        cbase = (rest // (d[0] * d[1])) * (cd[0] * cd[1]) + rest % d[0]
    else:
        cbase = rest
    even = (c % 2) == 0
    ev = i[even]
    with np.errstate(all="ignore"):
        wlo = (-sm[ev]) / s0[ev]
        whi = (-sp_[ev]) / s0[ev]
    has_lo = c[ev] >= 2
    has_hi = c[ev] + 1 < m
    bad = (s0[ev] == 0.0) | ~np.isfinite(s0[ev]) | (has_lo & ~np.isfinite(wlo)) | (has_hi & ~np.isfinite(whi))
    if bad.any():
        raise ValueError(f"row {int(ev[bad][0])}")
    W = np.zeros((ev.size, 2))
    W[has_lo, 0] = wlo[has_lo]
    W[has_hi, 1] = whi[has_hi]
    odd = i[~even]
    rows = np.concatenate([odd, ev[has_lo], ev[has_hi]])
    cols = np.concatenate([cbase[odd] + ((c[odd] - 1) // 2) * cstride,
                           cbase[ev[has_lo]] + (c[ev[has_lo]] // 2 - 1) * cstride,
                           cbase[ev[has_hi]] + (c[ev[has_hi]] // 2) * cstride])
    vals = np.concatenate([np.ones(odd.size), wlo[has_lo], whi[has_hi]])
    nH = cd[0] * cd[1] * cd[2]
    # build the CSC arrays by hand: scipy's constructors may drop or merge explicit zeros
    order = np.lexsort((rows, cols))
    indptr = np.zeros(nH + 1, np.int64)
    np.add.at(indptr, cols + 1, 1)
    P = sp.csc_matrix((vals[order], rows[order].astype(np.int32), np.cumsum(indptr).astype(np.int32)), shape=(n, nH))
    return P, W


def auto_mask(dims, dim, w):
    """The eligible axis (a < dim, at least 2 points) with the largest w[a]; the lowest on a tie; 0: none."""
    d = T.dims3(dims)
    best = -1
    for a in range(dim):
        if d[a] >= 2 and (best < 0 or w[a] > w[best]):
            best = a
    return 0 if best < 0 else 1 << best


def jump(dims, block=8, contrast=4, seed=7, natural=False, shift=0.0):
    """5- / 7-point diffusion whose conductivity is 10^k per block of `block` nodes per axis, k a random
    integer in [0, contrast]; an edge takes the k of the block that holds its lower endpoint; a Dirichlet
    side (natural=False) adds the boundary node's block k to the diagonal; `shift` goes on the diagonal.
    Canonical scipy CSR."""
    rng = np.random.default_rng(seed)
    dims = tuple(int(x) for x in dims)
    n = int(np.prod(dims))
    nb = [(m + block - 1) // block for m in dims]
    kb = 10.0 ** rng.integers(0, contrast + 1, size=nb[::-1]).astype(np.float64)  # [bz][by][bx]
    idx = np.arange(n).reshape(dims[::-1])  # [z][y][x]
    grids = np.meshgrid(*[np.arange(m) // block for m in dims[::-1]], indexing="ij")
    knode = kb[tuple(grids)].ravel()  # the k of every node's block, x fastest
    diag = np.full(n, float(shift))
    rows, cols, vals = [], [], []
    for axis in range(len(dims)):
        ax = len(dims) - 1 - axis
        lo = np.take(idx, np.arange(dims[axis] - 1), axis=ax).ravel()
        hi = np.take(idx, np.arange(1, dims[axis]), axis=ax).ravel()
        k = knode[lo]
        np.add.at(diag, lo, k)
        np.add.at(diag, hi, k)
        if not natural:
            for side in (0, dims[axis] - 1):
                s = np.take(idx, [side], axis=ax).ravel()
                np.add.at(diag, s, knode[s])
        rows += [lo, hi]
        cols += [hi, lo]
        vals += [-k, -k]
    rows.append(np.arange(n))
    cols.append(np.arange(n))
    vals.append(diag)
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    A.sort_indices()
    return A


def nonsymmetric(A, dims, factor=1.3):
    """A with the upper side of every x coupling (column = row + 1 on the same grid line) scaled."""
    nx = T.dims3(dims)[0]
    M = sp.csr_matrix(A, dtype=np.float64, copy=True)
    M.sort_indices()
    row = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    k = (M.indices == row + 1) & (row % nx != nx - 1)
    M.data[k] *= factor
    return M


class OpdepTwin(S.SemiTwin):
    """SemiTwin with one axis per level and opdep_P.  masks: explicit single-axis masks, or None for the
    automatic rule, ending at `max_levels`, at a level of <= `min_coarse` rows or when no axis has 2
    points.  geometric=True keeps the masks and takes semi_P's fixed weights instead (the comparison of
    the tests)."""

    def __init__(self, A, dims, masks=None, min_coarse=MIN_COARSE, max_levels=MAX_LEVELS, omega=0.8, iters=2,
                 geometric=False, pin=False):
        self.dim = len(tuple(dims))
        assert self.dim in (2, 3)
        self.dims = [T.dims3(dims)]
        self.A = [sp.csr_matrix(A, dtype=np.float64)]
        self.n = [self.A[0].shape[0]]
        self.P, self.R, self.masks, self.w, self.W = [], [], [], [], []
        l = 0
        while True:
            if masks is not None:
                if l == len(masks):
                    break
                m = int(masks[l])
            else:
                if l + 1 >= max_levels or self.n[l] <= min_coarse:
                    break
                self.w.append(S.axis_strength(self.A[l], self.dims[l]))
                m = auto_mask(self.dims[l], self.dim, self.w[-1])
                if m == 0:
                    break
            if geometric:
                P, W = S.semi_P(self.dims[l], self.dim, m), None
            else:
                P, W = opdep_P(self.A[l], self.dims[l], self.dim, m)
            self.masks.append(m)
            self.W.append(W)
            self.P.append(P.tocsr())
            self.R.append(P.T.tocsr())
            self.A.append((self.R[l] @ (self.A[l] @ self.P[l])).tocsr())
            self.dims.append(S.coarse_dims(self.dims[l], self.dim, m))
            self.n.append(self.A[-1].shape[0])
            l += 1
        self.nl = len(self.A)
        self.omega, self.iters = omega, iters
        self.pin = pin
        C = self.A[-1].tocsc()
        if pin:  # the singular solve of the library: the last unknown is pinned to 0
            C = C[:-1, :-1]
        self.coarse = spla.splu(C)
        self._ld = {}

    def coarse_solve(self, f, dtype):
        if not self.pin:
            return super().coarse_solve(f, dtype)
        x = np.zeros(self.n[-1], dtype)
        x[:-1] = self.coarse.solve(np.asarray(f[:-1], np.float64))
        return x


_CASES = {}


def case(dims, contrast=4, **kw):
    """(A, b, OpdepTwin with the automatic rule) of the jump operator: built once per case, never modified."""
    key = (tuple(dims), contrast, tuple(sorted(kw.items())))
    if key not in _CASES:
        A = jump(dims, contrast=contrast, **kw)
        b = S.rhs(A.shape[0])
        for a in (A.indptr, A.indices, A.data, b):
            a.setflags(write=False)
        _CASES[key] = (A, b, OpdepTwin(A, dims))
    return _CASES[key]
