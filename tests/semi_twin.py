"""TEST INFRASTRUCTURE: a numpy / scipy twin of the semi-coarsening hierarchies
(amg_hip_create_tensor_semi).  tests/tensor_twin.py's Twin with a per-level axis mask (bit 0 = x,
1 = y, 2 = z): a masked axis of length m goes to m // 2 with P1(m), an unmasked one keeps its length
with the identity, P = P_z (x) P_y (x) P_x.  The automatic rule -- coarsen the axes whose strongest
pure-axis coupling is at least theta times the strongest of all -- is written down again in numpy,
and so is the operator of the tests: tests/mixed_twin.py's diffusion with the conductivities of axis
a scaled by eps[a].  Nothing here reads the library.  Never imported by the product."""
import os
import sys

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tensor_twin as T  # noqa: E402

# (dims, eps per axis): the anisotropic cases, and the isotropic grids on which the rule must give
# full coarsening
ANISO = (((33, 20), (1.0, 1e-3)), ((33, 20), (1e-3, 1.0)), ((64, 48), (1.0, 1e-2)),
         ((17, 12, 9), (1.0, 1.0, 1e-3)), ((17, 12, 9), (1e-3, 1.0, 1e-3)), ((48, 40, 24), (1.0, 1e-2, 1.0)))
ISO = ((33, 20), (17, 12, 9))
THETA, MIN_COARSE, MAX_LEVELS = 0.5, 32, 16


def full_mask(dim):
    return 7 if dim == 3 else 3


def coarse_dims(dims, dim, mask):
    d = T.dims3(dims)
    return tuple(d[a] // 2 if a < dim and (mask >> a) & 1 else d[a] for a in range(3))


def mask_error(dims, dim, mask):
    """None, or why `mask` cannot coarsen the grid `dims`."""
    d = T.dims3(dims)
    if mask == 0:
        return "no axis"
    if mask < 0 or mask > 7:
        return "bits"
    if dim == 2 and mask & 4:
        return "z in 2-D"
    for a in range(3):
        if (mask >> a) & 1 and d[a] < 2:
            return "short axis"
    return None


def semi_P(dims, dim, mask):
    """P_z (x) P_y (x) P_x as CSC with sorted indices: P1(m) on the axes of `mask`, the identity on
    the others."""
    d = T.dims3(dims)
    f = [T.P1(d[a]) if a < dim and (mask >> a) & 1 else sp.identity(d[a], format="csc") for a in range(3)]
    P = sp.kron(f[1], f[0], format="csc")
    if dim == 3:
        P = sp.kron(f[2], P, format="csc")
    P = sp.csc_matrix(P)
    P.sort_indices()
    return P


def axis_strength(A, dims):
    """w[a] = max |a_ij| over the entries whose column differs from the row by +-1 in axis a and by 0
    in the other axes (0.0 when there is none); three float64."""
    nx, ny, _ = T.dims3(dims)
    M = sp.coo_matrix(A)
    r, c = M.row.astype(np.int64), M.col.astype(np.int64)
    d = np.stack([c % nx - r % nx, (c // nx) % ny - (r // nx) % ny, c // (nx * ny) - r // (nx * ny)])
    pure = np.abs(d).sum(axis=0) == 1
    w = np.zeros(3)
    for a in range(3):
        v = np.abs(M.data[pure & (d[a] != 0)])
        if v.size:
            w[a] = v.max()
    return w


def auto_mask(dims, dim, w, theta):
    """Eligible: axes a < dim of length >= 2.  Coarsened: eligible with w[a] >= theta * max eligible w."""
    d = T.dims3(dims)
    ok = [a for a in range(dim) if d[a] >= 2]
    if not ok:
        return 0
    cut = np.float64(theta) * max(w[a] for a in ok)
    return sum(1 << a for a in ok if w[a] >= cut)


def diffusion(dims, eps, seed=2, shift=0.01):
    """tests/mixed_twin.py's diffusion with the face conductivities of axis a (uniform in [1, 10],
    their rounded mean on the Dirichlet faces) scaled by eps[a]; canonical scipy CSR."""
    rng = np.random.default_rng(seed)
    dims = tuple(dims)
    n = int(np.prod(dims))
    idx = np.arange(n).reshape(dims[::-1])  # [z][y][x]
    diag = np.full(n, float(shift))
    rows, cols, vals = [], [], []
    for axis in range(len(dims)):
        ax = len(dims) - 1 - axis
        lo = np.take(idx, np.arange(dims[axis] - 1), axis=ax).ravel()
        hi = np.take(idx, np.arange(1, dims[axis]), axis=ax).ravel()
        k = rng.uniform(1.0, 10.0, size=lo.size)
        edge = float(np.round(k.mean())) * eps[axis]
        k = k * eps[axis]
        np.add.at(diag, lo, k)
        np.add.at(diag, hi, k)
        for side in (0, dims[axis] - 1):
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


def rhs(n, seed=99):
    return np.random.default_rng(seed).standard_normal(n)


class SemiTwin(T.Twin):
    """tensor_twin.Twin on a semi-coarsening hierarchy.  masks: the explicit per-level masks (the
    hierarchy has len(masks) + 1 levels), or None for the automatic rule with `theta`, ending at
    `max_levels`, at a level of <= `min_coarse` rows or when no axis has 2 points."""

    def __init__(self, A, dims, masks=None, theta=THETA, min_coarse=MIN_COARSE, max_levels=MAX_LEVELS,
                 omega=0.8, iters=2):
        self.dim = len(tuple(dims))
        assert self.dim in (2, 3)
        self.dims = [T.dims3(dims)]
        self.A = [sp.csr_matrix(A, dtype=np.float64)]
        self.n = [self.A[0].shape[0]]
        assert self.n[0] == int(np.prod(self.dims[0]))
        self.P, self.R, self.masks, self.w = [], [], [], []
        l = 0
        while True:
            if masks is not None:
                if l == len(masks):
                    break
                m = int(masks[l])
            else:
                if l + 1 >= max_levels or self.n[l] <= min_coarse:
                    break
                self.w.append(axis_strength(self.A[l], self.dims[l]))
                m = auto_mask(self.dims[l], self.dim, self.w[-1], theta)
                if m == 0:
                    break
            assert mask_error(self.dims[l], self.dim, m) is None, (l, m, self.dims[l])
            P = semi_P(self.dims[l], self.dim, m)
            self.masks.append(m)
            self.P.append(P.tocsr())
            self.R.append(P.T.tocsr())
            self.A.append((self.R[l] @ (self.A[l] @ self.P[l])).tocsr())
            self.dims.append(coarse_dims(self.dims[l], self.dim, m))
            self.n.append(self.A[-1].shape[0])
            assert self.n[-1] == int(np.prod(self.dims[-1]))
            l += 1
        self.nl = len(self.A)
        self.omega, self.iters = omega, iters
        self.coarse = spla.splu(self.A[-1].tocsc())
        self._ld = {}


def full_twin(A, dims, min_coarse=MIN_COARSE, max_levels=MAX_LEVELS):
    """tensor_twin.Twin (full coarsening) ending by the same rule: at `max_levels`, at a level of
    <= `min_coarse` rows, or when an axis has fewer than 2 points."""
    dim = len(tuple(dims))
    d, nl = T.dims3(dims), 1
    while nl < max_levels and d[0] * d[1] * d[2] > min_coarse and min(d[:dim]) >= 2:
        d, nl = T.coarse_dims(d, dim), nl + 1
    return T.Twin(A, dims, nl)


_CASES = {}


def case(dims, eps):
    """(A, b, SemiTwin with the automatic rule): built once per case and never modified."""
    key = (tuple(dims), tuple(eps))
    if key not in _CASES:
        A = diffusion(dims, eps)
        b = rhs(A.shape[0])
        for a in (A.indptr, A.indices, A.data, b):
            a.setflags(write=False)
        _CASES[key] = (A, b, SemiTwin(A, dims))
    return _CASES[key]
