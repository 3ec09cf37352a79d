"""TEST INFRASTRUCTURE: a numpy / scipy twin of operator-dependent interpolation on grids with periodic
axes (amg_hip_create_tensor_opdep_periodic).  tests/opdep_twin.py's OpdepTwin with a periodic mask: on
a level that coarsens a periodic axis the rows are collapsed by the axis distance mod m, every even
point has both weights and fine point 0 takes its low one from the last coarse point.  The weight rule,
the eligibility rule and the operator of the tests (opdep_twin.jump with wrap edges) are written down
again in numpy.  Nothing here reads the library.  Never imported by the product."""
import os
import sys

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import opdep_twin as O  # noqa: E402
import semi_twin as S  # noqa: E402
import tensor_twin as T  # noqa: E402

MIN_COARSE, MAX_LEVELS = O.MIN_COARSE, O.MAX_LEVELS


def jump_periodic(dims, periodic, block=8, contrast=4, seed=7, shift=0.0):
    """opdep_twin.jump -- the same block conductivities 10^k from the same random stream -- with, on an
    axis of `periodic` (bit a = axis a), the m edges (i, (i + 1) mod m) instead of the m - 1 edges
    (i, i + 1) and no face term: the wrap edge takes the k of the block of node m - 1, its lower
    endpoint.  The other axes are Dirichlet as in jump.  Canonical scipy CSR."""
    rng = np.random.default_rng(seed)
    dims = tuple(int(x) for x in dims)
    n = int(np.prod(dims))
    nb = [(m + block - 1) // block for m in dims]
    kb = 10.0 ** rng.integers(0, contrast + 1, size=nb[::-1]).astype(np.float64)  # [bz][by][bx]
    idx = np.arange(n).reshape(dims[::-1])  # [z][y][x]
    grids = np.meshgrid(*[np.arange(m) // block for m in dims[::-1]], indexing="ij")
    knode = kb[tuple(grids)].ravel()
    diag = np.full(n, float(shift))
    rows, cols, vals = [], [], []
    for axis in range(len(dims)):
        ax = len(dims) - 1 - axis
        m = dims[axis]
        per = bool((periodic >> axis) & 1)
        assert not per or m >= 3, "a wrap edge on an axis of 2 points doubles the open edge"
        lo = np.take(idx, np.arange(m if per else m - 1), axis=ax).ravel()
        hi = np.take(idx, (np.arange(m) + 1) % m if per else np.arange(1, m), axis=ax).ravel()
        k = knode[lo]
        np.add.at(diag, lo, k)
        np.add.at(diag, hi, k)
        if not per:
            for side in (0, m - 1):
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


def collapsed_sums_per(A, dims, axis):
    """(s_m, s_0, s_p) per row with the axis distance taken mod m: the classes m - 1, 0, 1; the entries
    (structural zeros too) added from +0.0 in ascending column order, as opdep_twin.collapsed_sums."""
    M = sp.csr_matrix(A, dtype=np.float64)
    M.sort_indices()
    n = M.shape[0]
    m = T.dims3(dims)[axis]
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(M.indptr))
    col = M.indices.astype(np.int64)
    dc = (O.axis_coord(col, dims, axis) - O.axis_coord(row, dims, axis)) % m
    out = []
    for want in (m - 1, 0, 1):
        s = np.zeros(n)
        k = dc == want
        np.add.at(s, row[k], M.data[k])
        out.append(s)
    return out


def P_of_weights_per(dims, dim, mask, W):
    """The CSC P (sorted rows in every column, explicit zeros kept) of the compact weights W on a
    PERIODIC axis: fine 2 q takes W[e, 0] from coarse (q - 1) mod (m / 2) and W[e, 1] from coarse q, fine
    2 q + 1 is coarse q with 1.0.  Column m / 2 - 1 of the axis so holds fine 0, m - 2, m - 1 in that order."""
    axis = O.axis_of(mask)
    d = T.dims3(dims)
    m = d[axis]
    assert axis < dim and m >= 4 and m % 2 == 0, (axis, m)
    n = d[0] * d[1] * d[2]
    cd = S.coarse_dims(d, dim, mask)
    mH = m // 2
    i = np.arange(n, dtype=np.int64)
    c = O.axis_coord(i, d, axis)
    stride = (1, d[0], d[0] * d[1])[axis]
    cstride = (1, cd[0], cd[0] * cd[1])[axis]
    rest = i - c * stride
    if axis == 0:
        cbase = (rest // d[0]) * cd[0]
    elif axis == 1:
        cbase = (rest // (d[0] * d[1])) * (cd[0] * cd[1]) + rest % d[0]
    else:
        cbase = rest
    even = (c % 2) == 0
    ev, odd = i[even], i[~even]
    W = np.asarray(W, np.float64).reshape(ev.size, 2)
    q = c[ev] // 2
    rows = np.concatenate([odd, ev, ev])
    cols = np.concatenate([cbase[odd] + ((c[odd] - 1) // 2) * cstride,
                           cbase[ev] + ((q - 1) % mH) * cstride,
                           cbase[ev] + q * cstride])
    vals = np.concatenate([np.ones(odd.size), W[:, 0], W[:, 1]])
    nH = cd[0] * cd[1] * cd[2]
    order = np.lexsort((rows, cols))  # by hand: scipy's constructors may drop or merge explicit zeros
    indptr = np.zeros(nH + 1, np.int64)
    np.add.at(indptr, cols + 1, 1)
    return sp.csc_matrix((vals[order], rows[order].astype(np.int32), np.cumsum(indptr).astype(np.int32)),
                         shape=(n, nH))


def opdep_P_per(A, dims, dim, mask, periodic):
    """(P, W) of the level that coarsens the axis of `mask`: opdep_twin.opdep_P when that axis is not in
    `periodic`; else w_lo = (-s_m) / s_0, w_hi = (-s_p) / s_0 of the sums mod m for EVERY even point, both
    kept whatever they are.  ValueError naming the row for a zero / non-finite s_0 or weight."""
    axis = O.axis_of(mask)
    if not (periodic >> axis) & 1:
        return O.opdep_P(A, dims, dim, mask)
    d = T.dims3(dims)
    sm, s0, sp_ = collapsed_sums_per(A, d, axis)
    i = np.arange(d[0] * d[1] * d[2], dtype=np.int64)
    ev = i[(O.axis_coord(i, d, axis) % 2) == 0]
    with np.errstate(all="ignore"):
        wlo = (-sm[ev]) / s0[ev]
        whi = (-sp_[ev]) / s0[ev]
    bad = (s0[ev] == 0.0) | ~np.isfinite(s0[ev]) | ~np.isfinite(wlo) | ~np.isfinite(whi)
    if bad.any():
        raise ValueError(f"row {int(ev[bad][0])}")
    W = np.stack([wlo, whi], axis=1)
    return P_of_weights_per(d, dim, mask, W), W


def eligible(dims, dim, a, periodic):
    m = T.dims3(dims)[a]
    return (m >= 4 and m % 2 == 0) if (periodic >> a) & 1 else m >= 2


def auto_mask_per(dims, dim, w, periodic):
    """The eligible axis with the largest w[a], the lowest on a tie; 0: none."""
    best = -1
    for a in range(dim):
        if eligible(dims, dim, a, periodic) and (best < 0 or w[a] > w[best]):
            best = a
    return 0 if best < 0 else 1 << best


def cycling_masks(dim, n_levels):
    """x, y, (z,) x, ...: the explicit masks of the measurements."""
    return [1 << (l % dim) for l in range(n_levels - 1)]


class OpdepPeriodicTwin(O.OpdepTwin):
    """OpdepTwin with the periodic mask `periodic`.  seam=False takes opdep_twin.opdep_P on the periodic
    matrix instead -- the wrap entries skipped, what amg_hip_create_tensor_opdep does with such a matrix
    (the comparison of the tests).  pin: the singular coarsest solve (every axis periodic, or the other
    sides natural)."""

    def __init__(self, A, dims, periodic, masks=None, min_coarse=MIN_COARSE, max_levels=MAX_LEVELS, omega=0.8,
                 iters=2, pin=False, seam=True):
        self.dim = len(tuple(dims))
        assert self.dim in (2, 3) and 0 <= periodic < (1 << self.dim)
        self.periodic = int(periodic)
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
                assert eligible(self.dims[l], self.dim, O.axis_of(m), self.periodic), (l, m, self.dims[l])
            else:
                if l + 1 >= max_levels or self.n[l] <= min_coarse:
                    break
                self.w.append(S.axis_strength(self.A[l], self.dims[l]))
                m = auto_mask_per(self.dims[l], self.dim, self.w[-1], self.periodic)
                if m == 0:
                    break
            if seam:
                P, W = opdep_P_per(self.A[l], self.dims[l], self.dim, m, self.periodic)
            else:
                P, W = O.opdep_P(self.A[l], self.dims[l], self.dim, m)
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
        if pin:
            C = C[:-1, :-1]
        self.coarse = spla.splu(C)
        self._ld = {}

    def coarse_solve(self, f, dtype):
        """OpdepTwin's, with the pinned solve in longdouble too when the coarsest level is small (<= 256
        rows): the reference of a V-cycle comparison must not carry the float64 solve's rounding."""
        if self.pin and dtype is np.longdouble and self.n[-1] <= 256:
            x = np.zeros(self.n[-1], dtype)
            x[:-1] = T.dense_solve(self.A[-1].toarray()[:-1, :-1], np.asarray(f[:-1], dtype), dtype)
            return x
        return super().coarse_solve(f, dtype)


_CASES = {}


def case(dims, periodic, n_levels=None, contrast=4):
    """(A, b, twin) of jump_periodic: explicit cycling masks with `n_levels` levels, or (None) the
    automatic rule.  Every axis periodic: the singular case, b with zero mean and the pinned solve.
    Built once per case, never modified."""
    key = (tuple(dims), periodic, n_levels, contrast)
    if key not in _CASES:
        dim = len(dims)
        singular = periodic == (1 << dim) - 1
        A = jump_periodic(dims, periodic, contrast=contrast)
        b = S.rhs(A.shape[0])
        if singular:
            b = b - b.mean()
        for a in (A.indptr, A.indices, A.data, b):
            a.setflags(write=False)
        masks = None if n_levels is None else cycling_masks(dim, n_levels)
        _CASES[key] = (A, b, OpdepPeriodicTwin(A, dims, periodic, masks=masks, pin=singular))
    return _CASES[key]
