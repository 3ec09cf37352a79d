"""TEST INFRASTRUCTURE: the operators, mask chains and the numpy recomputation of the seam that
tests/test_gpu_tensor_opdep_periodic_dev.py (GPU) and tests/test_tensor_opdep_periodic_dev_seam.py (CPU)
share.  Nothing here reads the library.  Never imported by the product."""
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import opdep_periodic_twin as OP  # noqa: E402
import opdep_twin as O  # noqa: E402
import semi_twin as S  # noqa: E402
import tensor_twin as T  # noqa: E402

# (grid, periodic mask) of the set-up comparison: the smallest grids at which the seam can go wrong
GRIDS = [((4, 3), 1), ((6, 5), 3), ((8, 1), 1), ((3, 4), 2), ((5, 8), 2), ((4, 4, 4), 7), ((6, 4, 8), 5),
         ((64, 48), 3), ((16, 16, 16), 7), ((24, 20, 16), 4)]
NONSYM_SEED = 2024  # discriminates on both grids of the seam test (checked there); no other seed was tried


def chain(dims, per):
    """x, y, (z,) x, ... down to the last level the checks allow: a periodic axis is coarsened while its
    length is even and at least 4, another axis while it has 2 points; an axis that cannot is passed over"""
    d, dim, masks, a, idle = list(dims), len(dims), [], 0, 0
    while idle < dim:
        if OP.eligible(d, dim, a, per):
            masks.append(1 << a)
            d[a] //= 2
            idle = 0
        else:
            idle += 1
        a = (a + 1) % dim
    return masks


def all_periodic(dims, per):
    return per == (1 << len(dims)) - 1


def jump(dims, per):
    """(A, b, singular) of opdep_periodic_twin.jump_periodic; every axis periodic: the singular case, b of
    zero mean"""
    A = OP.jump_periodic(dims, per)
    b = S.rhs(A.shape[0])
    singular = all_periodic(dims, per)
    if singular:
        b = b - b.mean()
    return A, b, singular


def nonsymmetric(dims, per, seed=NONSYM_SEED):
    """(A, b, False): the pattern of jump_periodic (wrap entries on the periodic axes) with random
    off-diagonals in [-1.5, -0.5] and a diagonal that dominates its row by a random margin in [0.5, 1.5].
    No entry is a power of two, A is not symmetric, so every product of the Galerkin sums rounds and the
    levels take K-Transpose."""
    rng = np.random.default_rng(seed + 131 * int(np.prod(dims)) + per)
    A = sp.csr_matrix(OP.jump_periodic(dims, per), copy=True)
    A.sort_indices()
    n = A.shape[0]
    row = np.repeat(np.arange(n), np.diff(A.indptr))
    off = A.indices != row
    A.data[off] = rng.uniform(-1.5, -0.5, size=int(off.sum()))
    rowsum = np.zeros(n)
    np.add.at(rowsum, row[off], -A.data[off])
    A.data[~off] = rowsum + rng.uniform(0.5, 1.5, size=n)
    assert (~off).sum() == n
    return A, S.rhs(n), False


def operator(name, dims, per):
    return jump(dims, per) if name == "jump" else nonsymmetric(dims, per)


_CACHE = {}


def case(name, dims, per):
    """operator(...) built once per (name, dims, per) and frozen"""
    key = (name, tuple(dims), per)
    if key not in _CACHE:
        A, b, singular = operator(name, dims, per)
        for a in (A.indptr, A.indices, A.data, b):
            a.setflags(write=False)
        _CACHE[key] = (A, b, singular)
    return _CACHE[key]


def without_wrap(A, dims, axis, store_zero):
    """A with its wrap entries on `axis` (axis distance m - 1) stored as 0.0, or absent from the pattern;
    the diagonal unchanged"""
    M = sp.csr_matrix(A, copy=True)
    M.sort_indices()
    n = M.shape[0]
    m = T.dims3(dims)[axis]
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(M.indptr))
    col = M.indices.astype(np.int64)
    k = np.abs(O.axis_coord(col, dims, axis) - O.axis_coord(row, dims, axis)) == m - 1
    assert k.any()
    if store_zero:
        M.data[k] = 0.0
        return M
    keep = ~k
    ptr = np.zeros(n + 1, np.int64)
    np.add.at(ptr, row[keep] + 1, 1)
    return sp.csr_matrix((M.data[keep], M.indices[keep], np.cumsum(ptr).astype(np.int32)), shape=(n, n))


# ---- the seam, recomputed in numpy in spgemm_rows' order -------------------------------------------------
def galerkin_row(A, P, fine_rows, r_weights):
    """Row I of R (A P) with R's row given as (fine_rows, r_weights) IN THAT ORDER: t = a_ik * P(k, J) over k
    ascending, the first assigned and the rest added; then R(I, i) * (A P)(i, J) over the given i, the first
    assigned and the rest added.  A: CSR; P: CSR.  -> (sorted columns, values)"""
    acc = {}
    for i, r in zip(fine_rows, r_weights):
        ap = {}
        for p in range(A.indptr[i], A.indptr[i + 1]):
            k, a = A.indices[p], A.data[p]
            for q in range(P.indptr[k], P.indptr[k + 1]):
                J, t = P.indices[q], np.float64(a) * np.float64(P.data[q])
                ap[J] = ap[J] + t if J in ap else t
        for J in sorted(ap):
            t = np.float64(r) * ap[J]
            acc[J] = acc[J] + t if J in acc else t
    cols = sorted(acc)
    return np.array(cols, np.int64), np.array([acc[J] for J in cols], np.float64)


def collapse_row(A, dims, axis, i, periodic):
    """(w_lo, w_hi) of fine row i: the entries added in ascending column order from +0.0 by the axis distance
    mod m (periodic) or the plain distance"""
    m = T.dims3(dims)[axis]
    c = int(O.axis_coord(np.array([i]), dims, axis)[0])
    sm = s0 = sp_ = np.float64(0.0)
    for p in range(A.indptr[i], A.indptr[i + 1]):
        dc = int(O.axis_coord(np.array([A.indices[p]]), dims, axis)[0]) - c
        if periodic:
            dc %= m
        v = np.float64(A.data[p])
        if dc == (m - 1 if periodic else -1):
            sm = sm + v
        elif dc == 0:
            s0 = s0 + v
        elif dc == 1:
            sp_ = sp_ + v
    return (-sm) / s0, (-sp_) / s0
