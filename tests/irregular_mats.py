"""TEST INFRASTRUCTURE: seeded generators of irregular sparse matrices (numpy / scipy only) and
`plan`, a host model of the rule by which the library picks a device layout for a matrix
(solver.cpp: upload_mat, layout_of; host_setup.cpp: to_dict, to_sell64).

The suite's other inputs are grid stencils: constant row length, a handful of offsets, a diagonal in
every row, no empty row.  The matrices here have none of these properties, and each generator aims
at one special case of the layout kernels: the pass-length switches and the empty panels of K-SELL
(`staircase`), the +-32767 limit of its 16-bit indices (`far`), the limits of the dictionary encoder
(`dict_limit`), the halo-shifted rectangular blocks of the multi-GPU driver (`halo_block`), exact
zeros that the upload prunes (`with_zeros`).  Every generator returns a scipy CSR matrix with sorted
int32 indices; explicit zeros, where a generator makes them, are kept.  Never imported by the
product."""
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

LAYOUT_AUTO, LAYOUT_CSR, LAYOUT_SELL, LAYOUT_DICT = 0, 1, 2, 3
LAYOUT_NAME = {LAYOUT_AUTO: "auto", LAYOUT_CSR: "csr", LAYOUT_SELL: "sell", LAYOUT_DICT: "dict"}

STAIR_WIDTHS = [1, 3, 4, 5, 6, 7, 8, 9, 10, 15, 16, 17, 24, 25, 0, 2]


def _csr(rows, cols, vals, shape):
    """CSR with sorted int32 indices from triplets without duplicates; explicit zeros stay."""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    vals = np.asarray(vals, np.float64)
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    assert not np.any((np.diff(rows) == 0) & (np.diff(cols) == 0)), "duplicate entry"
    ptr = np.zeros(shape[0] + 1, np.int64)
    np.add.at(ptr, rows + 1, 1)
    M = sp.csr_matrix((vals, cols.astype(np.int32), np.cumsum(ptr).astype(np.int32)), shape=shape)
    M.has_sorted_indices = True
    return M


def _canon(M):
    M = sp.csr_matrix(M)
    M.sort_indices()
    M.indices = M.indices.astype(np.int32)
    M.indptr = M.indptr.astype(np.int32)
    return M


# ---------------------------------------------------------------- generators ----
def knn(n, k, seed, quant=None):
    """Symmetric M-matrix of a symmetrised k-nearest-neighbour graph of n random points in the unit
    square (ordered by x-strip, then y): off-diagonals -(0.1 + U(0, 1)), or minus a draw from `quant`;
    diagonal = sum of the row's weights + 0.05."""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(seed)
    pts = rng.random((n, 2))
    strips = max(1, int(np.sqrt(n) / 2))
    order = np.lexsort((pts[:, 1], np.floor(pts[:, 0] * strips)))
    pts = pts[order]
    kk = min(k, n - 1)
    edges = set()
    if kk > 0:
        _, nb = cKDTree(pts).query(pts, k=kk + 1)
        for i in range(n):
            for j in nb[i, 1:]:
                edges.add((min(i, int(j)), max(i, int(j))))
    edges = np.array(sorted(edges), np.int64).reshape(-1, 2)
    w = 0.1 + rng.random(len(edges)) if quant is None else rng.choice(np.asarray(quant, np.float64), len(edges))
    W = sp.coo_matrix((w, (edges[:, 0], edges[:, 1])), shape=(n, n)).tocsr()
    W = W + W.T
    dg = np.asarray(W.sum(axis=1)).ravel() + 0.05
    return _canon(sp.diags(dg) - W)


def winperm(m, win, seed):
    """The m x m 5-point Laplacian, its dofs permuted randomly inside windows of `win` consecutive
    dofs: few (offset, value) pairs, thousands of distinct rows."""
    rng = np.random.default_rng(seed)
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(m, m))
    L = (sp.kron(sp.identity(m), T) + sp.kron(T, sp.identity(m))).tocsr()
    n = m * m
    new_of_old = np.arange(n)
    for s in range(0, n, win):
        e = min(n, s + win)
        new_of_old[s:e] = s + rng.permutation(e - s)
    C = L.tocoo()
    return _csr(new_of_old[C.row], new_of_old[C.col], C.data, (n, n))


def shapes(n, nsh, K, maxlen, seed, ncols=None, shift=0):
    """Row i takes shape i mod nsh: up to maxlen - 1 distinct off-diagonal offsets in [-K, K] with
    values from {-0.25, -0.5, -1} (entries that would leave the matrix are dropped), diagonal = 1 -
    the sum of the shape's off-diagonal values.  Shape 0 has maxlen - 1 offsets, shape 1 none.
    ncols / shift: row i's diagonal sits in column i + shift of an n x ncols matrix."""
    rng = np.random.default_rng(seed)
    ncols = n if ncols is None else ncols
    cand = np.array([o for o in range(-K, K + 1) if o != 0])
    sh = []
    for s in range(nsh):
        cnt = maxlen - 1 if s == 0 else 0 if s == 1 else int(rng.integers(0, maxlen))
        offs = np.sort(rng.choice(cand, size=cnt, replace=False)) if cnt else np.zeros(0, np.int64)
        vals = rng.choice([-0.25, -0.5, -1.0], size=cnt)
        sh.append((offs, vals, 1.0 - float(np.sum(vals))))
    rows, cols, vals = [], [], []
    for i in range(n):
        offs, v, dg = sh[i % nsh]
        c = i + shift + offs
        ok = (c >= 0) & (c < ncols)
        rows += [i] * (int(ok.sum()) + 1)
        cols += list(c[ok]) + [i + shift]
        vals += list(v[ok]) + [dg]
    return _csr(rows, cols, vals, (n, ncols))


def staircase(widths=STAIR_WIDTHS, n=None, seed=7):
    """One 64-row panel per entry of `widths`: panel p has one row of exactly widths[p] entries, its
    other rows 0 .. widths[p] entries, columns within +-40 of the row; about 3 of 4 non-empty rows
    have a diagonal.  n: number of rows (default 64 len(widths)); rows past n are cut."""
    rng = np.random.default_rng(seed)
    full = 64 * len(widths)
    n = full if n is None else n
    assert full - 63 <= n <= full
    rows, cols, vals = [], [], []
    for p, w in enumerate(widths):
        r0, r1 = 64 * p, min(n, 64 * p + 64)
        longest = r0 + int(rng.integers(0, r1 - r0))
        for i in range(r0, r1):
            cnt = w if i == longest else int(rng.integers(0, w + 1))
            if cnt == 0:
                continue
            lo, hi = max(0, i - 40), min(n - 1, i + 40)
            cand = np.array([c for c in range(lo, hi + 1) if c != i])
            if rng.random() < 0.75 or cand.size < cnt:
                c = np.concatenate([[i], rng.choice(cand, size=cnt - 1, replace=False)])
            else:
                c = rng.choice(cand, size=cnt, replace=False)
            v = np.where(c == i, 4.0 + rng.random(c.size), -(0.25 + rng.random(c.size)))
            rows += [i] * cnt
            cols += list(c)
            vals += list(v)
    return _csr(rows, cols, vals, (n, n))


def far(n, d):
    """Tridiagonal, plus entries at column distance exactly +d (first rows) and -d (last rows)."""
    i = np.arange(n)
    rows = [i, i[1:], i[:-1]]
    cols = [i, i[1:] - 1, i[:-1] + 1]
    vals = [np.full(n, 2.5), np.full(n - 1, -1.0), np.full(n - 1, -1.0)]
    up = np.array([r for r in (0, 1, 100, n - 1 - d) if 0 <= r and r + d < n and d > 1], np.int64)
    dn = np.array([r for r in (d, d + 33, n - 1) if r < n and r - d >= 0 and d > 1], np.int64)
    up, dn = np.unique(up), np.unique(dn)
    rows += [up, dn]
    cols += [up + d, dn - d]
    vals += [np.full(up.size, -0.5), np.full(dn.size, -0.375)]
    return _csr(np.concatenate(rows), np.concatenate(cols), np.concatenate(vals), (n, n))


def dict_limit(kind):
    """Matrices that sit exactly on a limit of the dictionary encoder, and one step past it:
    'pairs255' / 'pairs256' distinct (offset, value) pairs, 'row16' / 'row17' entries in the longest
    row, 'types255' / 'types256' distinct rows, 'row8' / 'row9' entries in the longest row (one code
    word against two)."""
    if kind in ("pairs255", "pairs256"):
        n, k = 300, int(kind[5:]) - 1          # the diagonal pair + k distinct values at offset +1
        i = np.arange(n)
        j = np.arange(k)
        return _csr(np.concatenate([i, j]), np.concatenate([i, j + 1]),
                    np.concatenate([np.full(n, 2.0), -(1.0 + j / 1024.0)]), (n, n))
    if kind in ("row8", "row9", "row16", "row17"):
        n, cnt, r = 200, int(kind[3:]), 100
        i = np.arange(n)
        rows = [i, i[1:], i[:-1]]
        cols = [i, i[1:] - 1, i[:-1] + 1]
        vals = [np.full(n, 2.0), np.full(n - 1, -1.0), np.full(n - 1, -1.0)]
        M = _csr(np.concatenate(rows), np.concatenate(cols), np.concatenate(vals), (n, n)).tolil()
        for c in range(r - cnt // 2, r - cnt // 2 + cnt):
            M[r, c] = 3.0 if c == r else -0.125
        return _canon(M.tocsr())
    if kind in ("types255", "types256"):
        n, T = 600, int(kind[5:]) - 1          # T two-offset rows + the diagonal-only row
        rows, cols, vals = [], [], []
        for i in range(n):
            rows.append(i), cols.append(i), vals.append(2.0)
            if i < n - 32:
                t = i % T
                rows.append(i), cols.append(i + 1 + t % 16), vals.append(-1.0)
                rows.append(i), cols.append(i + 17 + t // 16), vals.append(-0.5)
        return _csr(rows, cols, vals, (n, n))
    raise ValueError(kind)


def halo_block(rows, shift, kind="knn", seed=5):
    """A rows x (rows + 2 shift) block whose row i has its diagonal in column i + shift: the local
    block of a rank of the multi-GPU driver, columns numbered in its halo-extended vector."""
    if kind == "knn":
        return _canon(knn(rows + 2 * shift, 4, seed)[shift:shift + rows, :])
    return shapes(rows, 23, 12, 8, seed, ncols=rows + 2 * shift, shift=shift)


def with_zeros(M, seed=11, tail=70, frac=0.1):
    """A copy of M with some stored values set to +0.0 and -0.0 (about `frac` of them), one row in
    the middle whose entries all become zero, and a tail of `tail` such rows."""
    rng = np.random.default_rng(seed)
    M = _canon(M.copy())
    n = M.shape[0]
    z = np.flatnonzero(rng.random(M.nnz) < frac)
    M.data[z] = np.where(np.arange(z.size) % 2 == 0, 0.0, -0.0)
    for r in [n // 2] + list(range(max(0, n - tail), n)):
        q = np.arange(M.indptr[r], M.indptr[r + 1])
        M.data[q] = np.where(q % 2 == 0, 0.0, -0.0)
    return M


def pruned(M):
    """M without its exact zeros (+0.0 and -0.0): what the pruning uploads keep."""
    M = _canon(M.copy())
    keep = M.data != 0.0
    rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    return _csr(rows[keep], M.indices[keep], M.data[keep], M.shape)


def embed(B, shift=0):
    """The square matrix of max(rows + shift, ncols) rows with row i of the block B in row i + shift:
    the CPU references take square matrices only."""
    size = max(B.shape[0] + shift, B.shape[1])
    rows = np.repeat(np.arange(B.shape[0]), np.diff(B.indptr)) + shift
    return _csr(rows, B.indices, B.data, (size, size))


# ---------------------------------------------------------------- the layout rule ----
Plan = namedtuple("Plan", "layout typed words idx16 stream_bytes pairs row_types slots max_row")


def sell_slots(M):
    """64 x the sum over the 64-row panels of the panel's longest row."""
    cnt = np.diff(M.indptr).astype(np.int64)
    pad = np.concatenate([cnt, np.zeros(-cnt.size % 64, np.int64)])
    return int(64 * pad.reshape(-1, 64).max(axis=1).sum()) if cnt.size else 0


def plan(A, layout, diag_shift=0, index16=True, row_types=True):
    """What upload_mat(A, layout, diag_shift) builds for the CSR matrix A (exact zeros count as
    entries: prune first where the upload prunes) and what layout_of then reports.

    Dictionary iff the longest row has <= 16 entries, there are <= 255 distinct (offset, value
    bits) pairs and nrows + diag_shift <= ncols; typed iff there are <= 255 distinct rows (and the
    row-type switch is on); 1 code word per row iff the longest row has <= 8 entries.  SELL slots =
    64 x sum of the per-panel longest rows; AUTO takes SELL iff slots <= 1.25 nnz + 4096, else CSR;
    16-bit indices iff every col - (row + diag_shift) lies in [-32767, 32767] (and the switch is on).
    stream_bytes: dict typed n + 2048 words + 12 pairs, untyped 8 words n + 12 pairs; SELL 10 or 12
    per slot + 8 per panel; CSR 12 nnz + 4 (n + 1)."""
    A = _canon(A)
    n, nc = A.shape
    cnt = np.diff(A.indptr).astype(np.int64)
    nnz = int(A.nnz)
    max_row = int(cnt.max()) if n else 0
    rows = np.repeat(np.arange(n, dtype=np.int64), cnt)
    off = A.indices.astype(np.int64) - (rows + diag_shift)
    bits = A.data.view(np.int64)
    if nnz:
        uniq, ids = np.unique(np.stack([off, bits], axis=1), axis=0, return_inverse=True)
        pairs, ids = int(uniq.shape[0]), np.asarray(ids).ravel().tolist()
    else:
        pairs, ids = 0, []
    ptr = A.indptr
    distinct_rows = len({tuple(ids[ptr[r]:ptr[r + 1]]) for r in range(n)})
    can_dict = bool(max_row <= 16 and pairs <= 255 and n + diag_shift <= nc and diag_shift >= 0)
    words = 1 if max_row <= 8 else 2
    slots = sell_slots(A)
    fits16 = bool(index16) and bool(nnz == 0 or (off.min() >= -32767 and off.max() <= 32767))
    if layout in (LAYOUT_AUTO, LAYOUT_DICT) and can_dict:
        typed = bool(row_types) and distinct_rows <= 255
        b = (n + 256 * 8 * words if typed else n * 8 * words) + 12 * pairs
        return Plan(LAYOUT_DICT, typed, words, None, b, pairs, distinct_rows, slots, max_row)
    if layout == LAYOUT_AUTO:
        sell = slots <= 1.25 * nnz + 4096.0
    else:
        sell = layout != LAYOUT_CSR
    if sell:
        b = slots * (10 if fits16 else 12) + (n + 63) // 64 * 8
        return Plan(LAYOUT_SELL, None, None, fits16, b, pairs, distinct_rows, slots, max_row)
    return Plan(LAYOUT_CSR, None, None, None, 12 * nnz + 4 * (n + 1), pairs, distinct_rows, slots, max_row)


# ---------------------------------------------------------------- the cases ----
Case = namedtuple("Case", "name A shift")   # A: CSR as handed to the library (explicit zeros kept)


def _cases():
    c = []
    add = lambda name, A, shift=0: c.append(Case(name, A, shift))
    for n in (1, 63, 64, 65, 129, 257, 513):
        add(f"knn-{n}", knn(n, 4, 1))
    add("knn-4097", knn(4097, 4, 1))
    add("knn-quant-513", knn(513, 4, 2, quant=[0.25, 0.5, 1.0]))
    add("winperm-65", winperm(65, 8, 2))
    add("shapes-typed-2w", shapes(5000, 37, 40, 16, 3))
    add("shapes-typed-1w-513", shapes(513, 37, 40, 8, 3))
    add("shapes-untyped-2w", shapes(1537, 300, 20, 16, 3))
    add("shapes-typed-1w-257", shapes(257, 5, 9, 4, 4))
    add("stair", staircase())
    add("stair-trailing-empty", staircase(STAIR_WIDTHS + [0]))
    add("stair-cut", staircase(n=64 * len(STAIR_WIDTHS) - 63))
    add("far-32767", far(33000, 32767))
    add("far-32768", far(33000, 32768))
    for k in ("pairs255", "pairs256", "row16", "row17", "types255", "types256", "row8", "row9"):
        add(f"limit-{k}", dict_limit(k))
    add("halo-knn", halo_block(300, 37, "knn"), 37)
    add("halo-shapes", halo_block(513, 16, "shapes"), 16)
    add("haloT-knn", _canon(halo_block(300, 37, "knn").T))        # rows > ncols: no dictionary
    add("haloT-shapes", _canon(halo_block(513, 16, "shapes").T))
    add("zeros-knn-513", with_zeros(knn(513, 4, 1)))
    add("zeros-shapes-257", with_zeros(shapes(257, 5, 9, 4, 4)))
    add("zeros-stair", with_zeros(staircase()))
    return c


_CASES = None


def cases():
    """The list of cases, built once."""
    global _CASES
    if _CASES is None:
        _CASES = _cases()
    return _CASES


def case(name):
    for c in cases():
        if c.name == name:
            return c
    raise KeyError(name)
