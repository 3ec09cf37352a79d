"""TEST INFRASTRUCTURE for the single-precision cycle on dictionary-coded levels (K-DictF32): the
constant-coefficient operators (scipy.sparse.kron of 1-D stencils), the solvers of the named cases on the
DEFAULT layout, the layouts every case must report, and the f32_twin.Hierarchy of a solver from its
getters.  Shared by tests/test_gpu_f32_dict.py and tests/test_gpu_mixed_dict.py; nothing here is imported
by the product.

Cases (true Jacobi 2+2 omega 0.8 unless stated; every level below the coarsest must report the
dictionary layout unless stated):
  lin63, lin64   Multigrid on the 63^2 / 64^2 Laplacian, 3 levels: flat stride-2 transfers, one code word.
                 3969 rows: a partial lane (3969 is odd) and a partial last workgroup
  t33, t33-host  5-point Laplacian on 33x20, 3 levels, tensor_dev / tensor: 9-point Galerkin levels (two
                 code words)
  t35, t34       the same on 35x21 (735 = 3 mod 4) and 34x21 (714 = 2 mod 4): the other tail remainders
  aniso          diag(1, 1e-2) diffusion on 33x20: several off-diagonal values in the pair table
  box            7-point Laplacian on 17x12x9, 3 levels: level 0 dictionary, level 1 (27-entry rows) SELL
  per            5-point operator on (32, 20) periodic in x and y, 4 levels, masks (3, 3, 1): wrap entries
  nat            pure-Neumann 5-point operator on 33x20, singular: boundary row types, the pinned solve
  nonsym         5-point diffusion plus first-order upwind convection, velocity (3, 1.5), on 33x20,
                 Multigrid.tensor: Jacobi walks the transposed matrix's own dictionary
  untyped        t33 built with set_row_types(0): code words streamed per row
  rows1-t33, rows1-lin63   with set_dict_rows(1) while the solver runs: the kernel's other rows-per-lane form
                 (4 rows per lane instead of 2: 3969 = 1 mod 4); rows1-t35, rows1-t34 its other tail
                 remainders, rows1-untyped its code-word loads, rows1-cheb2 its accesses of d
  it1, it3       t33 with smoother_iters 1 and 3
  cheb1 .. cheb3, cheb2-it2   t33 with Chebyshev degree 1, 2, 3; degree 2 with two applications"""
import contextlib

import numpy as np
import scipy.sparse as sp

import f32_twin as FT

DICT, SELL, CSR = 3, 2, 1
JAC = dict(smoother=3, smoother_iters=2, omega=0.8)


def cheb(degree, iters=1):
    return dict(smoother=5, smoother_iters=iters, cheb_degree=degree)


def axis(m, k=1.0, lo=True, hi=True, per=False):
    """k * tridiag(-1, 2, -1) on m points; a side that is not Dirichlet (lo / hi False) has k on its
    diagonal; per: the wrap entries instead of sides"""
    T = sp.diags([np.full(m - 1, -k), np.full(m, 2.0 * k), np.full(m - 1, -k)], [-1, 0, 1]).tolil()
    if per:
        T[0, m - 1] = -k
        T[m - 1, 0] = -k
    else:
        if not lo:
            T[0, 0] = k
        if not hi:
            T[m - 1, m - 1] = k
    return sp.csr_matrix(T)


def grid_op(terms, dims):
    """sum over axes a of I (x) .. (x) terms[a] (x) .. (x) I, x fastest; canonical CSR"""
    A = None
    for a, Ta in enumerate(terms):
        M = None
        for b in range(len(dims)):  # x first: every later axis goes on the left
            F = Ta if b == a else sp.identity(dims[b], format="csr")
            M = F if M is None else sp.kron(F, M, format="csr")
        A = M if A is None else A + M
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    return A


_OPS = {}


def operator(name):
    """(A as CSR, b): built once per name and never modified"""
    if name in _OPS:
        return _OPS[name]
    rng = np.random.default_rng(99)
    if name in ("33x20", "35x21", "34x21"):
        dims = tuple(int(t) for t in name.split("x"))
        A = grid_op([axis(dims[0]), axis(dims[1])], dims)
    elif name == "aniso":
        dims = (33, 20)
        A = grid_op([axis(33, 1.0), axis(20, 1e-2)], dims)
    elif name == "box":
        dims = (17, 12, 9)
        A = grid_op([axis(m) for m in dims], dims)
    elif name == "per":
        dims = (32, 20)
        A = grid_op([axis(32, per=True), axis(20, per=True)], dims)
    elif name == "nat":
        dims = (33, 20)
        A = grid_op([axis(33, lo=False, hi=False), axis(20, lo=False, hi=False)], dims)
    elif name == "nonsym":
        dims = (33, 20)
        up = lambda m, c: sp.csr_matrix(c * (sp.identity(m) - sp.eye(m, k=-1)))  # noqa: E731
        A = grid_op([axis(33) + up(33, 3.0), axis(20) + up(20, 1.5)], dims)
    else:
        raise KeyError(name)
    n = A.shape[0]
    b = rng.standard_normal(n)
    if name in ("per", "nat"):
        b -= b.mean()  # a consistent singular system
    for a in (A.indptr, A.indices, A.data, b):
        a.setflags(write=False)
    _OPS[name] = (A, b, dims)
    return _OPS[name]


def csc(A):
    Ac = sp.csc_matrix(A)
    Ac.sort_indices()
    return Ac.indptr.astype(np.int32), Ac.indices.astype(np.int32), Ac.data.copy()


def csr(A):
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy()


def _tensor(op, levels, dev, **opts):
    def make(amg, oracle, **kw):
        A, b, dims = operator(op)
        o = dict(opts if "smoother" in opts else dict(JAC, **opts), **kw)
        if dev:
            return amg.Multigrid.tensor_dev(*csr(A), b.copy(), dims, levels, **o)
        return amg.Multigrid.tensor(*csc(A), b.copy(), dims, levels, **o)
    return make


def _lin(n):
    def make(amg, oracle, **kw):
        Ao = oracle.laplacian(n)
        b = np.random.default_rng(7).standard_normal(n * n)
        return amg.Multigrid(Ao.colptr, Ao.rowind, Ao.val, b, 3, **dict(JAC, **kw))
    return make


def _per(amg, oracle, **kw):
    A, b, dims = operator("per")
    return amg.Multigrid.tensor_periodic(*csc(A), b.copy(), dims, 4, 3, axis_masks=(3, 3, 1), natural_sides=0,
                                         singular=True, **dict(JAC, **kw))


def _jac(omega, iters):
    return lambda mg: ("jacobi", omega, iters)


def _cheb(degree, iters=1):
    return lambda mg: ("cheb", degree, iters, [mg.cheb_bounds(l) for l in range(mg.n_levels - 1)])


# name -> dict(make, A = the operator's name (None: the solver's own level 0), smoother = what the twin runs,
#              layouts = level_layout of the levels below the coarsest, and the switches of the case)
CASES = {
    "lin63": dict(make=_lin(63), A=None, layouts=[DICT, DICT], kind=1, n0=3969),
    "lin64": dict(make=_lin(64), A=None, layouts=[DICT, DICT], kind=1, n0=4096),
    "t33": dict(make=_tensor("33x20", 3, True), A="33x20", layouts=[DICT, DICT], words=[1, 2]),
    "t33-host": dict(make=_tensor("33x20", 3, False), A="33x20", layouts=[DICT, DICT], words=[1, 2]),
    "t35": dict(make=_tensor("35x21", 3, True), A="35x21", layouts=[DICT, DICT], n0=735),
    "t34": dict(make=_tensor("34x21", 3, True), A="34x21", layouts=[DICT, DICT], n0=714),
    "aniso": dict(make=_tensor("aniso", 3, True), A="aniso", layouts=[DICT, DICT]),
    "box": dict(make=_tensor("box", 3, True), A="box", layouts=[DICT, SELL], width=27),
    "per": dict(make=_per, A="per", layouts=[DICT, DICT, DICT]),
    "nat": dict(make=_tensor("nat", 3, False, natural_sides=15, singular=True), A="nat", layouts=[DICT, DICT]),
    "nonsym": dict(make=_tensor("nonsym", 3, False), A="nonsym", layouts=[DICT, DICT], unsym0=True),
    "untyped": dict(make=_tensor("33x20", 3, True), A="33x20", layouts=[DICT, DICT], untyped=True, words=[1, 2]),
    "rows1-t33": dict(make=_tensor("33x20", 3, True), A="33x20", layouts=[DICT, DICT], rows1=True),
    "rows1-lin63": dict(make=_lin(63), A=None, layouts=[DICT, DICT], kind=1, rows1=True),
    "rows1-t35": dict(make=_tensor("35x21", 3, True), A="35x21", layouts=[DICT, DICT], n0=735, rows1=True),
    "rows1-t34": dict(make=_tensor("34x21", 3, True), A="34x21", layouts=[DICT, DICT], n0=714, rows1=True),
    "rows1-untyped": dict(make=_tensor("33x20", 3, True), A="33x20", layouts=[DICT, DICT], untyped=True,
                          words=[1, 2], rows1=True),
    "rows1-cheb2": dict(make=_tensor("33x20", 3, True, **cheb(2)), A="33x20", layouts=[DICT, DICT],
                        smoother=_cheb(2), passes=2, rows1=True),
    "it1": dict(make=_tensor("33x20", 3, True, smoother_iters=1), A="33x20", layouts=[DICT, DICT],
                smoother=_jac(0.8, 1), passes=1),
    "it3": dict(make=_tensor("33x20", 3, True, smoother_iters=3), A="33x20", layouts=[DICT, DICT],
                smoother=_jac(0.8, 3), passes=3),
    "cheb1": dict(make=_tensor("33x20", 3, True, **cheb(1)), A="33x20", layouts=[DICT, DICT], smoother=_cheb(1),
                  passes=1),
    "cheb2": dict(make=_tensor("33x20", 3, True, **cheb(2)), A="33x20", layouts=[DICT, DICT], smoother=_cheb(2),
                  passes=2),
    "cheb3": dict(make=_tensor("33x20", 3, True, **cheb(3)), A="33x20", layouts=[DICT, DICT], smoother=_cheb(3),
                  passes=3),
    "cheb2-it2": dict(make=_tensor("33x20", 3, True, **cheb(2, 2)), A="33x20", layouts=[DICT, DICT],
                      smoother=_cheb(2, 2), passes=4),
}


def make(amg, oracle, case, **kw):
    """the case's solver; switches that are read when a solver is created are restored here"""
    c = CASES[case]
    if c.get("untyped"):
        amg.set_row_types(0)
    try:
        return c["make"](amg, oracle, **kw)
    finally:
        amg.set_row_types(1)  # the library's default; the switch has no getter


@contextlib.contextmanager
def running(amg, case):
    """the switches of the case that are read at every launch"""
    if CASES[case].get("rows1"):
        amg.set_dict_rows(1)
    try:
        yield
    finally:
        amg.set_dict_rows(2)  # the library's default


def level_matrices(mg):
    """(A, P, R) of the solver as scipy CSC matrices, from its getters"""
    nl = mg.n_levels
    n = [mg.get_n_dofs(l) for l in range(nl)]
    A, P, R = [], [], []
    for l in range(nl):
        colptr, rowind, val = mg.get_coefficient_matrix(l)
        A.append(sp.csc_matrix((val, rowind, colptr), shape=(n[l], n[l])))
    for l in range(nl - 1):
        colptr, rowind, val = mg.get_transfer(l, "P")
        P.append(sp.csc_matrix((val, rowind, colptr), shape=(n[l], n[l + 1])))
        colptr, rowind, val = mg.get_transfer(l, "R")
        R.append(sp.csc_matrix((val, rowind, colptr), shape=(n[l + 1], n[l])))
    return A, P, R


def device_coarse(mg):
    """the solver's own double coarsest solve: float64 -> float64"""
    last = mg.n_levels - 1

    def solve(f64):
        mg.set_vec(last, "f", f64)
        mg.level_op(last, 4)
        return mg.get_soln(last)
    return solve


_HIER = {}


def hierarchy(mg, case):
    """f32_twin.Hierarchy of the solver's level matrices and transfers, made once per case -- every solver
    of a case has the same hierarchy -- with this solver's coarse solve"""
    if case not in _HIER:
        A, P, R = level_matrices(mg)
        sm = CASES[case].get("smoother", _jac(0.8, 2))(mg)
        _HIER[case] = (FT.Hierarchy(A, P, R, sm, None), A)
    H, A = _HIER[case]
    H.coarse = device_coarse(mg)
    return H, A


def pairs(M):
    """number of distinct (column - row, value bits) pairs among the non-zero entries of M: ntab"""
    M = sp.coo_matrix(M)
    keep = M.data != 0.0
    off = (M.col[keep].astype(np.int64) - M.row[keep].astype(np.int64))
    bits = np.ascontiguousarray(M.data[keep]).view(np.uint64)
    return len(set(zip(off.tolist(), bits.tolist())))


def check_path(mg, case, H, A):
    """the path the case is named for was taken, by the getters that exist; a case that silently fell
    back to SELL would test nothing"""
    c = CASES[case]
    nl = mg.n_levels
    assert nl == len(c["layouts"]) + 1
    said = []
    for l in range(nl - 1):
        layout, stream = mg.level_layout(l)
        assert layout == c["layouts"][l], (case, l, layout)
        if layout != DICT:
            continue
        n, nt = A[l].shape[0], pairs(A[l])
        assert nt <= 255
        typed = stream - 12 * nt - n
        untyped = stream - 12 * nt
        if c.get("untyped"):
            assert untyped in (8 * n, 16 * n), (case, l, stream)
            words = untyped // (8 * n)
        else:
            assert typed in (256 * 8, 256 * 16), (case, l, stream, nt)
            words = typed // (256 * 8)
        if "words" in c:
            assert words == c["words"][l], (case, l, words)
        said.append(f"level {l} dictionary, {'code words' if c.get('untyped') else 'row types'}, {words} word(s), "
                    f"{nt} pairs")
    if c["layouts"][0] == DICT and len(set(c["layouts"])) > 1:
        said.append(f"layouts {c['layouts']}")
    assert mg.level_transfer_kind(0) == c.get("kind", 2)
    if "passes" in c:
        assert H.passes() == c["passes"]
    if "width" in c:
        assert max(R.w for R in H.rows) == c["width"]
    if "n0" in c:
        assert mg.get_n_dofs(0) == c["n0"]
    if c.get("unsym0"):
        assert not H.symmetric(0)
        said.append("level 0 not bitwise symmetric")
    if case == "aniso":
        vals = np.unique(sp.csr_matrix(A[0]).data)
        assert vals[vals < 0].size >= 2
    if case == "per":
        assert mg.periodic_axes() == 3
        far = np.abs(sp.coo_matrix(A[0]).col - sp.coo_matrix(A[0]).row).max()
        assert far == 32 * 19  # the y wrap
    if case == "nat":
        assert mg.natural_sides() == 15
    return "; ".join(said)
