"""Operators for the multicolour-smoother tests (tests/test_multicolor_ops.py,
tests/test_gpu_multicolor_forms.py): boxes with coefficients that vary by column and line parity,
wider stencils that need more colours, 1-D bands with many colours, and a nonsymmetric box.

TEST INFRASTRUCTURE ONLY: numpy / scipy, never imported by the product.  Every generator returns
the CSC triplet (colptr int32, rowind int32, val float64) of a strictly diagonally dominant matrix
with sorted row indices and no duplicate or zero entries."""
import numpy as np
import scipy.sparse as sp


def _csc(n, rows, cols, vals):
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsc()
    A.sum_duplicates()
    A.sort_indices()
    assert A.nnz == np.count_nonzero(A.data)
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)


def _sym(r, off, w):
    """entries w[k] at (r[k], r[k] + off) and mirrored"""
    return [r, r + off], [r + off, r], [w, w]


def _box_parts(nx, ny, stencil):
    n = nx * ny
    r = np.arange(n, dtype=np.int64)
    i, j = r % nx, r // nx
    rows, cols, vals = [], [], []

    def add(mask, off, w):
        w = np.broadcast_to(np.asarray(w, np.float64), r.shape)
        a, b, c = _sym(r[mask], off, w[mask])
        rows.extend(a), cols.extend(b), vals.extend(c)

    # the anisotropic box of tests/test_gpu_patch_xf.py::box2d: the x coupling alternates with the
    # column parity, the y coupling with the line parity, the diagonal is 0.125 larger on odd lines
    add(i < nx - 1, 1, np.where(i % 2 == 0, -1.0, -0.75))
    add(j < ny - 1, nx, np.where(j % 2 == 0, -0.375, -0.5))
    diag = 4.0 + 0.125 * (j % 2)
    if stencil >= 9:
        add((i < nx - 1) & (j < ny - 1), nx + 1, -0.1875)
        add((i >= 1) & (j < ny - 1), nx - 1, -0.09375)
        diag = diag + 1.0
    if stencil >= 13:
        add(i < nx - 2, 2, -0.0625)
        add(j < ny - 2, 2 * nx, -0.0625)
        diag = diag + 0.5
    rows.append(r), cols.append(r), vals.append(diag)
    return n, rows, cols, vals


def box5(nx, ny):
    """5-point box, couplings alternating by column and line parity (off-diagonal row sum <= 2.625,
    diagonal >= 4)"""
    return _csc(*_box_parts(nx, ny, 5))


def box9(nx, ny):
    """box5 plus the diagonal couplings -0.1875 at offset nx + 1 and -0.09375 at offset nx - 1, both
    mirrored; the diagonal raised by 1.0"""
    return _csc(*_box_parts(nx, ny, 9))


def box13(nx, ny):
    """box9 plus -0.0625 at +-2 and +-2 nx; the diagonal raised by another 0.5"""
    return _csc(*_box_parts(nx, ny, 13))


def box5_conv(nx, ny):
    """box5 plus a skew part: +0.0625 / -0.0625 on the upper / lower x coupling and +0.03125 /
    -0.03125 on the y coupling.  Nonsymmetric; the absolute off-diagonal row sum stays <= 2.8125"""
    n, rows, cols, vals = _box_parts(nx, ny, 5)
    r = np.arange(n, dtype=np.int64)
    i, j = r % nx, r // nx
    for mask, off, w in ((i < nx - 1, 1, 0.0625), (j < ny - 1, nx, 0.03125)):
        q = r[mask]
        rows.extend([q, q + off]), cols.extend([q + off, q])
        vals.extend([np.full(q.size, w), np.full(q.size, -w)])
    return _csc(n, rows, cols, vals)


def band(n, offsets, weights, diag):
    """symmetric band: weights[k] at +-offsets[k] on every row where the column is in range, `diag`
    on the diagonal"""
    assert diag > 2.0 * sum(abs(w) for w in weights)
    r = np.arange(n, dtype=np.int64)
    rows, cols, vals = [r], [r], [np.full(n, float(diag))]
    for off, w in zip(offsets, weights):
        a, b, c = _sym(r[: max(n - off, 0)], int(off), np.full(max(n - off, 0), float(w)))
        rows.extend(a), cols.extend(b), vals.extend(c)
    return _csc(n, rows, cols, vals)


def rhs(n):
    return np.sin(0.001 * np.arange(n)) + 1.5


def start(n, seed=11):
    return np.random.default_rng(seed).standard_normal(n)


# name -> (generator call, levels): the operators of the table in tests/test_multicolor_ops.py
BAND1025 = (1025, (1, 3, 7, 12), (-1.0, -0.5, -0.25, -0.125), 4.0)
BAND257 = (257, (1, 3, 7), (-1.0, -0.5, -0.25), 4.0)
