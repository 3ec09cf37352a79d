"""The matrix-layout kernels (K-CSR, K-SELL with 16- and 32-bit indices, K-Dict typed / untyped with
one or two rows per lane) on the irregular matrices of tests/irregular_mats.py: ragged rows, empty
rows, interior and trailing empty panels, rows without a diagonal, the +-32767 index limit, the
limits of the dictionary encoder, halo-shifted rectangular blocks, pruned exact zeros.

Per case and kernel variant: the layout the upload reports is the one `plan` predicts (layout and
stream bytes, so a silent fall-back fails), and residual, SpMV and Jacobi through amg_hip_devmat_*,
amg_hip_smooth (true Jacobi, 2 sweeps), amg_hip_smooth_chebyshev (degree 1, 2, 3) and amg_hip_spmv
equal the CPU oracle / the Chebyshev twin bit for bit, amg_hip_rss_host to 1e-13 (the tree sum).
The oracle itself is checked against a numpy longdouble evaluation on every case.

Which case catches which one-line defect (the first differing rows and panels are in the assertion
message; `stair` panel p has width STAIR_WIDTHS[p]):
  K-SELL  a pass shorter than the panel (`w <= 3` -> `w <= 4`, likewise 5 / 7 / 9)    stair, panels of width 4, 6, 8, 10
          the 8-entry loop without its remainder (`j0 + 8 <= w`)                      stair, widths 10, 15, 17, 25
          `j0 + u <= w` in the accumulate guard (the clamped entry j0 added again)     stair, every panel narrower than its pass
          the 16-bit decode or the diagonal test without `dshift`                      halo-knn (SpMV / Jacobi, sell16)
          16-bit indices taken at distance 32768                                       far-32768 (layout bytes, then values)
          rows of the last panel past n stored, or live rows of it dropped             stair-cut, knn-65 / 129 / 257 / 513
          a pass run on an empty panel                                                 an address error, not a value error: see
                                                                                       DESIGN.md section 3; the cases with such
                                                                                       panels are stair*, zeros-*, haloT-*
  K-CSR   the row walk not clipped to the staged chunk, U longer than the row          knn-4097, stair (rows of 0 .. 25 entries)
  K-Dict  the second code word dropped (entries 9 .. 16)                               limit-row9, limit-row16, shapes-*-2w
          the odd last row of two rows per lane dropped                                every odd n under dict-r2: knn-1,
                                                                                       shapes-typed-1w-513 / -257, halo-shapes
          code 254 (the 255th pair) or type 254 (the 255th row type) read as "none"    limit-pairs255, limit-types255
          row types used where the encoder gave none (256 distinct rows)               limit-types256, winperm-65
          offsets decoded against row instead of row + dshift                          halo-shapes
  upload  -0.0 not pruned, an all-zero row kept                                        zeros-* (stream bytes differ from plan)
Not detectable by value, by construction: a pad slot or a "no entry" code that is gathered and
multiplied (the pad -32768 taken as a column where row >= 32768, the `ok` select of dict_rows dropped)
contributes (+0.0) x, which changes no bit for finite x; `<` for `<=` at a pass-length switch of K-SELL
only lengthens the pass (dead loads).  The suite's vectors are finite.

Left out, with the reason: Jacobi on the transposed halo blocks (rows > ncols: the rows have no
diagonal column), the Chebyshev smoother on cases with a row without diagonal (the library refuses
them: the polynomial is in D^-1 A), the stand-alone square-matrix entry points on the rectangular
cases.

Ratios printed by test_oracle_is_a_reference (distance of the oracle from the longdouble evaluation
over e64, the distance of a plain float64 numpy evaluation from it), largest over all cases:
residual 1.116 (knn-63; the oracle subtracts term by term from f, the numpy evaluation sums first), SpMV
and Jacobi 1.000 on every case (the same operations in the same order); oracle rss within 7.3e-15
relative of the longdouble sum of squares (far-32767, 33000 rows)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "algebraic-multigrid_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cheb_twin as CT  # noqa: E402
import irregular_mats as im  # noqa: E402
import line_twin as LT  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in im.cases()]
OMEGA = 0.7
# name, layout request, index16, dict rows per lane, row types
VARIANTS = [("csr", im.LAYOUT_CSR, 1, 2, 1),
            ("sell16", im.LAYOUT_SELL, 1, 2, 1),
            ("sell32", im.LAYOUT_SELL, 0, 2, 1),
            ("dict-r1", im.LAYOUT_DICT, 1, 1, 1),
            ("dict-r2", im.LAYOUT_DICT, 1, 2, 1),
            ("dict-untyped", im.LAYOUT_DICT, 1, 2, 0),
            ("auto", im.LAYOUT_AUTO, 1, 2, 1)]


@pytest.fixture(scope="module", autouse=True)
def _restore_switches(amg):
    yield
    _defaults(amg)


def _defaults(amg):
    amg.set_default_layout(amg.LAYOUT_AUTO)
    amg.set_index16(True)
    amg.set_dict_rows(2)
    amg.set_row_types(True)


def _switch(amg, variant):
    _, layout, i16, rows, types = variant
    amg.set_default_layout(layout)
    amg.set_index16(i16)
    amg.set_dict_rows(rows)
    amg.set_row_types(types)


def csc_of(M, oracle):
    S = M.tocsc()
    S.sort_indices()
    return oracle.CSC(M.shape[0], M.shape[1], S.indptr, S.indices, S.data)


def csc_of_transpose(M, oracle):
    """The CSR arrays of M are the CSC arrays of M^T."""
    return oracle.CSC(M.shape[1], M.shape[0], M.indptr, M.indices, M.data)


def row_sums(P, x, dtype, shift):
    """Per row, in ascending column order and in `dtype`: the sum of a_ij x_j over all entries, the
    same sum without the diagonal entry (column i + shift), and the diagonal value."""
    n = P.shape[0]
    ptr, col = P.indptr.astype(np.int64), P.indices.astype(np.int64)
    val, xx = P.data.astype(dtype), np.asarray(x).astype(dtype)
    cnt = np.diff(ptr)
    full, off, dg = np.zeros(n, dtype), np.zeros(n, dtype), np.zeros(n, dtype)
    rows = np.arange(n)
    for j in range(int(cnt.max()) if n else 0):
        live = rows[cnt > j]
        at = ptr[live] + j
        t = val[at] * xx[col[at]]
        full[live] = full[live] + t
        on = col[at] == live + shift
        off[live[~on]] = off[live[~on]] + t[~on]
        dg[live[on]] = val[at][on]
    return full, off, dg


def evaluate(P, x, f, shift, dtype, jacobi):
    full, off, dg = row_sums(P, x, dtype, shift)
    fd = np.asarray(f).astype(dtype)
    out = {"residual": fd - full, "spmv": full}
    if jacobi:
        xi = np.asarray(x).astype(dtype)[shift:shift + P.shape[0]]
        safe = np.where(dg == 0, dtype(1), dg)
        out["jacobi"] = np.where(dg == 0, xi, xi + dtype(OMEGA) * ((fd - off) / safe - xi))
    return out


_REF = {}


def reference(name, oracle):
    """Inputs and the oracle's results of one case, computed once and never modified."""
    if name in _REF:
        return _REF[name]
    c = im.case(name)
    P = im.pruned(c.A)
    rows, cols = P.shape
    rng = np.random.default_rng(sum(map(ord, name)))
    x, f = rng.standard_normal(cols), rng.standard_normal(rows)
    jacobi = rows + c.shift <= cols
    E = im.embed(P, c.shift)
    fe = np.zeros(E.shape[0])
    fe[c.shift:c.shift + rows] = f
    xe = np.zeros(E.shape[0])
    xe[:cols] = x
    sl = slice(c.shift, c.shift + rows)
    ref = {"residual": oracle.residual(csc_of(E, oracle), xe, fe)[sl],
           "spmv": oracle.spmv(csc_of(P, oracle), x)}
    if jacobi:
        ref["jacobi"] = oracle.smooth(oracle.SM_TRUE_JACOBI, csc_of_transpose(E, oracle), xe, fe, n_iters=1,
                                      omega=OMEGA)[0][sl]
    square = rows == cols and c.shift == 0
    has_diag = square and bool(np.all(P.diagonal() != 0.0))
    if square:
        ref["jacobi2"] = oracle.smooth(oracle.SM_TRUE_JACOBI, csc_of_transpose(P, oracle), x, f, n_iters=2,
                                       omega=OMEGA)[0]
        ref["rss"] = oracle.rss(csc_of(P, oracle), x, f)
    if has_diag:
        G = CT.gershgorin(P)
        for k in (1, 2, 3):
            ref[f"cheb{k}"] = CT.cheb_smooth(P, x, f, 0.3 * G, 1.0 * G, k, 1)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    x.setflags(write=False)
    f.setflags(write=False)
    _REF[name] = (c, P, x, f, jacobi, square, has_diag, ref)
    return _REF[name]


@pytest.mark.parametrize("name", NAMES)
def test_oracle_is_a_reference(oracle, name):
    """The oracle has not seen rectangular, empty-row or 25-entry-row input before: its results lie
    within max(8 e64, 1e-14 ||.||) of a longdouble evaluation of the same operation, e64 being the
    distance of a plain float64 evaluation from the longdouble one."""
    c, P, x, f, jacobi, square, has_diag, ref = reference(name, oracle)
    ld = evaluate(P, x, f, c.shift, np.longdouble, jacobi)
    f64 = evaluate(P, x, f, c.shift, np.float64, jacobi)
    for op in ld:
        e64 = float(np.linalg.norm(f64[op].astype(np.longdouble) - ld[op]))
        ok, dist, bound, ratio = LT.within(ref[op], ld[op], e64, float(np.linalg.norm(ld[op])))
        print(f"{name} {op}: oracle-longdouble {dist:.3e}, e64 {e64:.3e}, ratio {ratio:.3f}, bound {bound:.3e}")
        assert ok, (name, op, dist, bound)
    if square:
        r = ld["residual"]
        rss_ld = float(np.sum(r * r))
        print(f"{name} rss: oracle / longdouble - 1 = {ref['rss'] / rss_ld - 1:.3e}")
        # a sequential float64 sum of n non-negative squares: relative error below (n + 8) 2^-53
        assert abs(ref["rss"] - rss_ld) <= (P.shape[0] + 8) * 2.0 ** -53 * rss_ld


@pytest.mark.parametrize("name", NAMES)
def test_kernels_equal_the_oracle_in_every_layout(amg, oracle, name):
    c, P, x, f, jacobi, square, has_diag, ref = reference(name, oracle)
    A = c.A                                  # with its explicit zeros: the upload prunes them
    rows, cols = A.shape
    no_diag = np.flatnonzero(row_sums(P, x, np.float64, c.shift)[2] == 0.0)
    PT = csc_of_transpose(P, oracle)         # rows of P as the columns the smoothers walk
    PC = csc_of(P, oracle)
    got = {}
    try:
        for var in VARIANTS:
            vname, layout, i16, _, types = var
            _switch(amg, var)
            want = im.plan(P, layout, c.shift, index16=bool(i16), row_types=bool(types))
            D = amg.DevMat(A.indptr, A.indices, A.data, cols, layout, c.shift)
            try:
                assert D.layout() == (want.layout, want.stream_bytes), (name, vname, D.layout(), want)
                out = {"residual": D.apply(D.RESIDUAL, x, f), "spmv": D.apply(D.SPMV, x)}
                if jacobi:
                    out["jacobi"] = D.apply(D.JACOBI, x, f, omega=OMEGA)
            finally:
                D.close()
            if square:
                out["jacobi2"] = amg.smooth(amg.SM_JACOBI, PT.colptr, PT.rowind, PT.val, x, f, n_iters=2,
                                            omega=OMEGA)[0]
                rss = amg.rss(PC.colptr, PC.rowind, PC.val, x, f)
                assert abs(rss - ref["rss"]) <= 1e-13 * ref["rss"], (name, vname, rss, ref["rss"])
            if has_diag:
                for k in (1, 2, 3):
                    out[f"cheb{k}"] = amg.smooth_chebyshev(PC.colptr, PC.rowind, PC.val, x, f, degree=k)
            for op, v in out.items():
                bad = np.flatnonzero(v != ref[op])
                assert np.array_equal(v, ref[op]), (name, vname, op, "first differing rows", bad[:8],
                                                    "panels", np.unique(bad // 64)[:8])
            if jacobi:
                keep = x[c.shift:c.shift + rows][no_diag]
                assert np.array_equal(out["jacobi"][no_diag], keep), (name, vname)
                if square:
                    assert np.array_equal(out["jacobi2"][no_diag], x[no_diag]), (name, vname)
            got[vname] = out
        first = got[VARIANTS[0][0]]
        for vname, out in got.items():
            for op, v in out.items():
                assert np.array_equal(v, first[op]), (name, vname, op)
    finally:
        _defaults(amg)


def test_the_intended_paths_are_taken(amg):
    """The cases that exist for one code path land on it (DevMat.layout(), not the plan)."""
    def lay(name, layout):
        c = im.case(name)
        D = amg.DevMat(c.A.indptr, c.A.indices, c.A.data, c.A.shape[1], layout, c.shift)
        try:
            return D.layout()
        finally:
            D.close()
    slots = lambda name: im.sell_slots(im.pruned(im.case(name).A))
    panels = lambda name: (im.case(name).A.shape[0] + 63) // 64
    try:
        _defaults(amg)
        assert lay("far-32767", amg.LAYOUT_SELL) == (amg.LAYOUT_SELL, 10 * slots("far-32767") + 8 * panels("far-32767"))
        assert lay("far-32768", amg.LAYOUT_SELL) == (amg.LAYOUT_SELL, 12 * slots("far-32768") + 8 * panels("far-32768"))
        for name in ("limit-pairs256", "limit-row17", "haloT-knn", "haloT-shapes"):
            assert lay(name, amg.LAYOUT_DICT)[0] == amg.LAYOUT_SELL, name
        for name in ("limit-pairs255", "limit-row16", "limit-types255", "limit-types256", "halo-shapes"):
            assert lay(name, amg.LAYOUT_DICT)[0] == amg.LAYOUT_DICT, name
        n = 600                                       # typed: 1 byte per row; untyped: 8
        assert lay("limit-types255", amg.LAYOUT_DICT)[1] == n + 2048 + 12 * 33
        assert lay("limit-types256", amg.LAYOUT_DICT)[1] == 8 * n + 12 * 33
        assert lay("knn-4097", amg.LAYOUT_AUTO)[0] == amg.LAYOUT_CSR
        assert lay("stair-trailing-empty", amg.LAYOUT_AUTO)[0] == amg.LAYOUT_SELL
        assert lay("zeros-stair", amg.LAYOUT_AUTO)[0] == amg.LAYOUT_CSR      # the pruned matrix decides
    finally:
        _defaults(amg)


@pytest.mark.parametrize("name", ["halo-knn", "halo-shapes", "haloT-knn", "haloT-shapes"])
def test_rectangular_spmv(amg, oracle, name):
    """amg_hip_spmv on rows < cols (the dictionary may take it) and rows > cols (it must not)."""
    c, P, x, f, jacobi, square, has_diag, ref = reference(name, oracle)
    M = csc_of(P, oracle)
    try:
        for var in VARIANTS:
            _switch(amg, var)
            got = amg.spmv(P.shape[0], P.shape[1], M.colptr, M.rowind, M.val, x)
            assert np.array_equal(got, ref["spmv"]), (name, var[0])
    finally:
        _defaults(amg)
