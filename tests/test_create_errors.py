"""Every constructor's argument errors, as literals: (entry point, arguments) -> (status, full text of
amg_hip_last_error()).  The set-up code shares its checks between the entry points; this table pins
what each entry point says, and WHICH fault it reports when a call has two, since the host and the
device constructors check in different orders.

No call here reaches a device: the host constructors run with host_only, the `_dev` constructors get
the pointers 8, 16, 24, 32, which must never be dereferenced, and every call fails in its checks.

EXPECTED holds what the library printed before the checks were shared.  Cases that are no fault on an
entry point are not in the table: `window` = 1 and `theta` = 0 are valid for amg_hip_create and
amg_hip_create_rs, and amg_hip_create_poisson_window sets `window` itself."""
import ctypes as C

import numpy as np
import pytest

JACOBI, SOR, CHEB, LINE, ALT = 3, 2, 5, 6, 7
FAKE = (8, 16, 24, 32)  # rowptr, col, val, b of the _dev constructors

HOST = ("create", "create_custom", "create_rs")
TENSOR = ("create_tensor", "create_tensor_semi", "create_tensor_periodic")
DEV = ("create_tensor_dev", "create_tensor_semi_dev", "create_tensor_periodic_dev")
POISSON = ("create_poisson", "create_poisson_tensor", "create_poisson_window")
GRID = TENSOR + DEV
SEMI = ("create_tensor_semi", "create_tensor_semi_dev", "create_tensor_periodic", "create_tensor_periodic_dev")
PERIODIC = ("create_tensor_periodic", "create_tensor_periodic_dev")
WITH_OPTS = HOST + GRID + POISSON
ARRAYS = {e: ("colptr", "rowind", "val", "b") for e in HOST + TENSOR}
ARRAYS.update({e: ("rowptr", "col", "val", "b") for e in DEV})
ARRAYS["create_custom"] += ("P_colptr", "P_rowind", "P_val", "R_colptr", "R_rowind", "R_val")
ARRAYS["tensor_axis_strength"] = ("colptr", "rowind", "val", "w")

_MATS = {}


def grid_matrix(dims):
    """CSC arrays of the 5- / 7-point Laplacian on the grid `dims` (x fastest) and a right-hand side"""
    dims = tuple(dims)
    if dims not in _MATS:
        d = dims + (1,) * (3 - len(dims))
        n = d[0] * d[1] * d[2]
        stride = (1, d[0], d[0] * d[1])
        cp, ri, v = [0], [], []
        for i in range(n):
            at = (i % d[0], i // d[0] % d[1], i // (d[0] * d[1]))
            col = {i: 2.0 * len(dims)}
            for a in range(len(dims)):
                if at[a] > 0:
                    col[i - stride[a]] = -1.0
                if at[a] + 1 < d[a]:
                    col[i + stride[a]] = -1.0
            for r in sorted(col):
                ri.append(r)
                v.append(col[r])
            cp.append(len(ri))
        _MATS[dims] = (np.array(cp, np.int32), np.array(ri, np.int32), np.array(v, np.float64), np.ones(n))
    return _MATS[dims]


def call(amg, entry, dims=(4, 4), dim=None, n=None, n_levels=2, null=(), masks=None, theta=0.5, min_coarse=1,
         periodic=0, pn=4, units=(0, 4), **opts):
    """One call of amg_hip_<entry> -> (status, message).  dims: the grid (of the matrix, too); dim and n
    may disagree with it; null: names of the arguments passed as null pointers; pn, units: the grid
    size and the window of the model-problem constructors; opts: fields of amg_hip_options."""
    lib = amg.lib()
    o = amg.Options()
    lib.amg_hip_default_options(C.byref(o))
    o.smoother, o.smoother_iters, o.omega = JACOBI, 2, 0.8
    o.host_only = 0 if entry in DEV else 1
    for k, val in opts.items():
        assert hasattr(o, k), k
        setattr(o, k, val)
    h = C.c_void_p()
    out = None if "out" in null else C.byref(h)
    d3 = np.array(tuple(dims) + (1,) * (3 - len(dims)), np.int64)
    dimsp = None if "dims" in null else d3.ctypes.data_as(amg._i64p)
    dim = len(dims) if dim is None else dim
    mk = None if masks is None else np.array(masks, np.int32)
    mkp = None if mk is None else amg._p32(mk)
    cp, ri, v, b = (*amg.laplacian(4), amg.rhs(4)) if tuple(dims) == (4, 4) else grid_matrix(dims)
    n = cp.size - 1 if n is None else n
    host = [None if name in null else conv(a)
            for name, conv, a in (("colptr", amg._p32, cp), ("rowind", amg._p32, ri), ("val", amg._p64, v),
                                  ("b", amg._p64, b))]
    dev = [None if name in null else C.c_void_p(p) for name, p in zip(("rowptr", "col", "val", "b"), FAKE)]
    if entry == "create":
        st = lib.amg_hip_create(n, *host, n_levels, C.byref(o), out)
    elif entry == "create_custom":
        # tables of null operators: every call fails before the level loop reads them
        tabs = [None if name in null else (t * 8)()
                for name, t in (("P_colptr", amg._i32p), ("P_rowind", amg._i32p), ("P_val", amg._f64p),
                                ("R_colptr", amg._i32p), ("R_rowind", amg._i32p), ("R_val", amg._f64p))]
        st = lib.amg_hip_create_custom(n, *host, n_levels, *tabs, C.byref(o), out)
    elif entry == "create_rs":
        st = lib.amg_hip_create_rs(n, *host, n_levels, theta, min_coarse, C.byref(o), out)
    elif entry == "create_tensor":
        st = lib.amg_hip_create_tensor(n, *host, dim, dimsp, n_levels, C.byref(o), out)
    elif entry == "create_tensor_semi":
        st = lib.amg_hip_create_tensor_semi(n, *host, dim, dimsp, n_levels, mkp, theta, min_coarse, C.byref(o), out)
    elif entry == "create_tensor_periodic":
        st = lib.amg_hip_create_tensor_periodic(n, *host, dim, dimsp, periodic, n_levels, mkp, C.byref(o), out)
    elif entry == "create_tensor_dev":
        st = lib.amg_hip_create_tensor_dev(n, *dev, dim, dimsp, n_levels, C.byref(o), out)
    elif entry == "create_tensor_semi_dev":
        st = lib.amg_hip_create_tensor_semi_dev(n, *dev, dim, dimsp, n_levels, mkp, theta, min_coarse, C.byref(o),
                                                out)
    elif entry == "create_tensor_periodic_dev":
        st = lib.amg_hip_create_tensor_periodic_dev(n, *dev, dim, dimsp, periodic, n_levels, mkp, C.byref(o), out)
    elif entry == "create_poisson":
        st = lib.amg_hip_create_poisson(dim, pn, n_levels, C.byref(o), out)
    elif entry == "create_poisson_tensor":
        st = lib.amg_hip_create_poisson_tensor(dim, pn, n_levels, C.byref(o), out)
    elif entry == "create_poisson_window":
        st = lib.amg_hip_create_poisson_window(dim, pn, units[0], units[1], n_levels, C.byref(o), out)
    elif entry == "tensor_axis_strength":
        w = np.zeros(3)
        st = lib.amg_hip_tensor_axis_strength(n, *host[:3], dim, dimsp, None if "w" in null else amg._p64(w))
    else:
        raise KeyError(entry)
    if h.value:  # not expected: a case that is no fault
        lib.amg_hip_destroy(h)
    assert st != amg.OK and not h.value, (entry, "the call succeeded")
    return st, lib.amg_hip_last_error().decode()


def _cases():
    """name -> (entry points, arguments of call())"""
    c = {}
    c["null_out"] = (WITH_OPTS, dict(null=("out",)))
    for e, names in ARRAYS.items():
        for a in names:
            c.setdefault("null_" + a, ((), dict(null=(a,))))
            c["null_" + a] = (c["null_" + a][0] + (e,), dict(null=(a,)))
    c["dim_1"] = (GRID + POISSON + ("tensor_axis_strength",), dict(dim=1))
    c["dim_4"] = (GRID + POISSON + ("tensor_axis_strength",), dict(dim=4))
    c["dims_null"] = (GRID + ("tensor_axis_strength",), dict(null=("dims",)))
    c["dims_entry_0"] = (GRID + ("tensor_axis_strength",), dict(dims=(4, 0), n=16))
    c["dims2_is_2_in_2d"] = (GRID + ("tensor_axis_strength",), dict(dims=(4, 4, 2), dim=2, n=32))
    c["n_15"] = (GRID + ("tensor_axis_strength",), dict(n=15))
    c["window"] = (GRID + ("create_poisson_tensor",), dict(window=1))
    c["n_levels_0"] = (WITH_OPTS, dict(n_levels=0))
    full = ("create_tensor", "create_tensor_periodic", "create_tensor_dev", "create_tensor_periodic_dev")
    c["level_9x9_5"] = (full + ("create_poisson_tensor",), dict(dims=(9, 9), n_levels=5, pn=9))
    c["level_9x6x5_4"] = (full, dict(dims=(9, 6, 5), n_levels=4))
    c["mask_0"] = (SEMI, dict(masks=(0,)))
    c["mask_axis_of_one_point"] = (SEMI, dict(dims=(4, 1), masks=(2,)))
    c["mask_bit_3"] = (SEMI, dict(masks=(8,)))
    c["auto_theta_0"] = (("create_tensor_semi", "create_tensor_semi_dev"), dict(theta=0.0))
    c["auto_min_coarse_0"] = (("create_tensor_semi", "create_tensor_semi_dev", "create_rs"), dict(min_coarse=0))
    c["periodic_axes_8"] = (PERIODIC, dict(periodic=8))
    c["periodic_z_in_2d"] = (PERIODIC, dict(periodic=4))
    c["periodic_6_to_3"] = (PERIODIC, dict(dims=(6, 4), n_levels=3, periodic=1))
    c["natural_side_on_periodic_axis"] = (PERIODIC, dict(periodic=1, natural_sides=1))
    c["natural_sides_beyond_2dim"] = (GRID, dict(natural_sides=16))
    c["natural_sides_not_taken"] = (HOST + POISSON, dict(natural_sides=1))
    c["singular_not_taken"] = (HOST + POISSON, dict(singular=1))
    c["singular_one_level"] = (GRID, dict(n_levels=1, singular=1, natural_sides=15))
    c["singular_2"] = (WITH_OPTS, dict(singular=2))
    c["cyclic_lines_2"] = (WITH_OPTS, dict(cyclic_lines=2))
    c["cyclic_lines_not_periodic"] = (tuple(e for e in WITH_OPTS if e not in PERIODIC),
                                      dict(cyclic_lines=1, smoother=ALT))
    c["cyclic_lines_not_line_alt"] = (PERIODIC, dict(cyclic_lines=1, periodic=1))
    c["smoother_17"] = (WITH_OPTS, dict(smoother=17))
    c["smoother_iters_-1"] = (WITH_OPTS, dict(smoother_iters=-1))
    c["cheb_degree_0"] = (WITH_OPTS, dict(smoother=CHEB, cheb_degree=0))
    c["cheb_with_window"] = (WITH_OPTS, dict(smoother=CHEB, window=1))
    c["line_omega_0"] = (WITH_OPTS, dict(smoother=LINE, omega=0.0))
    c["line_omega_2"] = (WITH_OPTS, dict(smoother=LINE, omega=2.0))
    c["line_with_window"] = (WITH_OPTS, dict(smoother=LINE, window=1))
    c["layout_9"] = (WITH_OPTS, dict(layout=9))
    c["sor_omega_3"] = (WITH_OPTS, dict(smoother=SOR, omega=3.0))
    c["line_alt_without_grid"] = (HOST + ("create_poisson", "create_poisson_window"), dict(smoother=ALT))
    c["window_cheb"] = (("create_poisson_window",), dict(smoother=CHEB))
    c["window_line"] = (("create_poisson_window",), dict(smoother=LINE))
    c["window_odd_start"] = (("create_poisson_window",), dict(pn=3, units=(1, 3)))
    c["window_units_out_of_range"] = (("create_poisson_window",), dict(units=(2, 5)))
    c["window_units_empty"] = (("create_poisson_window",), dict(units=(2, 2)))
    # two faults in one call: which one is reported
    c["2_dim_smoother"] = (GRID + POISSON, dict(dim=4, smoother=17))
    c["2_n_window"] = (GRID, dict(n=15, window=1))
    c["2_window_n_levels"] = (GRID + ("create_poisson_tensor",), dict(window=1, n_levels=0))
    c["2_level_smoother"] = (full + ("create_poisson_tensor",), dict(dims=(9, 9), n_levels=5, pn=9, smoother=17))
    c["2_null_dim"] = (GRID + ("tensor_axis_strength",), dict(null=("val",), dim=4))
    c["2_cheb_layout"] = (WITH_OPTS, dict(smoother=CHEB, cheb_degree=0, layout=9))
    c["2_smoother_singular"] = (GRID, dict(smoother=17, n_levels=1, singular=1, natural_sides=15))
    c["2_line_layout"] = (WITH_OPTS, dict(smoother=LINE, omega=0.0, layout=9))
    return c


CASES = _cases()
IDS = sorted(f"{e}/{name}" for name, (entries, _) in CASES.items() for e in entries)

# what the library printed before the checks were shared: "entry/case" -> (status, message)
EXPECTED = {
    'create/2_cheb_layout': (1, '`cheb_degree` must be at least 1, got 0'),
    'create_custom/2_cheb_layout': (1, '`cheb_degree` must be at least 1, got 0'),
    'create_poisson/2_cheb_layout': (1, '`cheb_degree` must be at least 1, got 0'),
    'create_poisson_tensor/2_cheb_layout': (1, '`cheb_degree` must be at least 1, got 0'),
    'create_poisson_window/2_cheb_layout': (
        4,
        'amg_hip_create_poisson_window: the Chebyshev smoother is not sharded'
    ),
    'create_rs/2_cheb_layout': (1, '`cheb_degree` must be at least 1, got 0'),
    'create_tensor/2_cheb_layout': (1, '`cheb_degree` must be at least 1, got 0'),
    'create_tensor_dev/2_cheb_layout': (1, '`cheb_degree` must be at least 1, got 0'),
    'create_tensor_periodic/2_cheb_layout': (1, '`cheb_degree` must be at least 1, got 0'),
    'create_tensor_periodic_dev/2_cheb_layout': (1, '`cheb_degree` must be at least 1, got 0'),
    'create_tensor_semi/2_cheb_layout': (1, '`cheb_degree` must be at least 1, got 0'),
    'create_tensor_semi_dev/2_cheb_layout': (1, '`cheb_degree` must be at least 1, got 0'),
    'create_poisson/2_dim_smoother': (1, 'dim must be 2 or 3 and n >= 1'),
    'create_poisson_tensor/2_dim_smoother': (1, 'amg_hip_create_poisson_tensor: `dim` must be 2 or 3'),
    'create_poisson_window/2_dim_smoother': (1, 'dim must be 2 or 3 and n >= 1'),
    'create_tensor/2_dim_smoother': (1, 'amg_hip_create_tensor: `dim` must be 2 or 3'),
    'create_tensor_dev/2_dim_smoother': (1, 'amg_hip_create_tensor_dev: `dim` must be 2 or 3'),
    'create_tensor_periodic/2_dim_smoother': (1, 'amg_hip_create_tensor_periodic: `dim` must be 2 or 3'),
    'create_tensor_periodic_dev/2_dim_smoother': (1, 'amg_hip_create_tensor_periodic_dev: `dim` must be 2 or 3'),
    'create_tensor_semi/2_dim_smoother': (1, 'amg_hip_create_tensor_semi: `dim` must be 2 or 3'),
    'create_tensor_semi_dev/2_dim_smoother': (1, 'amg_hip_create_tensor_semi_dev: `dim` must be 2 or 3'),
    'create_poisson_tensor/2_level_smoother': (
        1,
        'level 4 is not possible: level 3 is a 1 x 1 x 1 grid and an axis of fewer than 2 points cannot be co'
        'arsened; reduce `n_levels`'
    ),
    'create_tensor/2_level_smoother': (1, 'unknown smoother kind'),
    'create_tensor_dev/2_level_smoother': (
        1,
        'level 4 is not possible: level 3 is a 1 x 1 x 1 grid and an axis of fewer than 2 points cannot be co'
        'arsened; reduce `n_levels`'
    ),
    'create_tensor_periodic/2_level_smoother': (
        1,
        'level 4 is not possible: level 3 is a 1 x 1 x 1 grid and an axis of fewer than 2 points cannot be co'
        'arsened; reduce `n_levels`'
    ),
    'create_tensor_periodic_dev/2_level_smoother': (
        1,
        'level 4 is not possible: level 3 is a 1 x 1 x 1 grid and an axis of fewer than 2 points cannot be co'
        'arsened; reduce `n_levels`'
    ),
    'create/2_line_layout': (1, 'line smoother: `omega` must lie in (0, 2), got 0.000000'),
    'create_custom/2_line_layout': (1, 'line smoother: `omega` must lie in (0, 2), got 0.000000'),
    'create_poisson/2_line_layout': (1, 'line smoother: `omega` must lie in (0, 2), got 0.000000'),
    'create_poisson_tensor/2_line_layout': (1, 'line smoother: `omega` must lie in (0, 2), got 0.000000'),
    'create_poisson_window/2_line_layout': (4, 'amg_hip_create_poisson_window: the line smoother is not sharded'),
    'create_rs/2_line_layout': (1, 'line smoother: `omega` must lie in (0, 2), got 0.000000'),
    'create_tensor/2_line_layout': (1, 'line smoother: `omega` must lie in (0, 2), got 0.000000'),
    'create_tensor_dev/2_line_layout': (1, 'line smoother: `omega` must lie in (0, 2), got 0.000000'),
    'create_tensor_periodic/2_line_layout': (1, 'line smoother: `omega` must lie in (0, 2), got 0.000000'),
    'create_tensor_periodic_dev/2_line_layout': (1, 'line smoother: `omega` must lie in (0, 2), got 0.000000'),
    'create_tensor_semi/2_line_layout': (1, 'line smoother: `omega` must lie in (0, 2), got 0.000000'),
    'create_tensor_semi_dev/2_line_layout': (1, 'line smoother: `omega` must lie in (0, 2), got 0.000000'),
    'create_tensor/2_n_window': (1, 'amg_hip_create_tensor: `n` = 15 is not the 4 x 4 x 1 grid of `dims`'),
    'create_tensor_dev/2_n_window': (1, 'amg_hip_create_tensor_dev: `n` = 15 is not the 4 x 4 x 1 grid of `dims`'),
    'create_tensor_periodic/2_n_window': (
        1,
        'amg_hip_create_tensor_periodic: `n` = 15 is not the 4 x 4 x 1 grid of `dims`'
    ),
    'create_tensor_periodic_dev/2_n_window': (
        1,
        'amg_hip_create_tensor_periodic_dev: `n` = 15 is not the 4 x 4 x 1 grid of `dims`'
    ),
    'create_tensor_semi/2_n_window': (1, 'amg_hip_create_tensor_semi: `n` = 15 is not the 4 x 4 x 1 grid of `dims`'),
    'create_tensor_semi_dev/2_n_window': (
        1,
        'amg_hip_create_tensor_semi_dev: `n` = 15 is not the 4 x 4 x 1 grid of `dims`'
    ),
    'create_tensor/2_null_dim': (1, 'amg_hip_create_tensor: `dim` must be 2 or 3'),
    'create_tensor_dev/2_null_dim': (1, 'null input array'),
    'create_tensor_periodic/2_null_dim': (1, 'amg_hip_create_tensor_periodic: `dim` must be 2 or 3'),
    'create_tensor_periodic_dev/2_null_dim': (1, 'null input array'),
    'create_tensor_semi/2_null_dim': (1, 'amg_hip_create_tensor_semi: `dim` must be 2 or 3'),
    'create_tensor_semi_dev/2_null_dim': (1, 'null input array'),
    'tensor_axis_strength/2_null_dim': (1, 'null argument'),
    'create_tensor/2_smoother_singular': (1, 'unknown smoother kind'),
    'create_tensor_dev/2_smoother_singular': (1, 'unknown smoother kind'),
    'create_tensor_periodic/2_smoother_singular': (1, 'unknown smoother kind'),
    'create_tensor_periodic_dev/2_smoother_singular': (1, 'unknown smoother kind'),
    'create_tensor_semi/2_smoother_singular': (1, 'unknown smoother kind'),
    'create_tensor_semi_dev/2_smoother_singular': (1, 'unknown smoother kind'),
    'create_poisson_tensor/2_window_n_levels': (1, '`n_levels` must be at least 1'),
    'create_tensor/2_window_n_levels': (
        4,
        'amg_hip_create_tensor: window solvers (opt.window) coarsen the flat index; a full-coarsening hierarc'
        'hy is not sharded'
    ),
    'create_tensor_dev/2_window_n_levels': (
        4,
        'amg_hip_create_tensor_dev: window solvers (opt.window) coarsen the flat index; a full-coarsening hie'
        'rarchy is not sharded'
    ),
    'create_tensor_periodic/2_window_n_levels': (
        4,
        'amg_hip_create_tensor_periodic: window solvers (opt.window) coarsen the flat index; a full-coarsenin'
        'g hierarchy is not sharded'
    ),
    'create_tensor_periodic_dev/2_window_n_levels': (
        4,
        'amg_hip_create_tensor_periodic_dev: window solvers (opt.window) coarsen the flat index; a full-coars'
        'ening hierarchy is not sharded'
    ),
    'create_tensor_semi/2_window_n_levels': (
        4,
        'amg_hip_create_tensor_semi: window solvers (opt.window) coarsen the flat index; a semi-coarsening hi'
        'erarchy is not sharded'
    ),
    'create_tensor_semi_dev/2_window_n_levels': (
        4,
        'amg_hip_create_tensor_semi_dev: window solvers (opt.window) coarsen the flat index; a semi-coarsenin'
        'g hierarchy is not sharded'
    ),
    'create_rs/auto_min_coarse_0': (1, '`min_coarse` must be at least 1'),
    'create_tensor_semi/auto_min_coarse_0': (1, 'amg_hip_create_tensor_semi: `min_coarse` must be at least 1'),
    'create_tensor_semi_dev/auto_min_coarse_0': (
        1,
        'amg_hip_create_tensor_semi_dev: `min_coarse` must be at least 1'
    ),
    'create_tensor_semi/auto_theta_0': (1, 'amg_hip_create_tensor_semi: `theta` must be in (0, 1]'),
    'create_tensor_semi_dev/auto_theta_0': (1, 'amg_hip_create_tensor_semi_dev: `theta` must be in (0, 1]'),
    'create/cheb_degree_0': (1, '`cheb_degree` must be at least 1, got 0'),
    'create_custom/cheb_degree_0': (1, '`cheb_degree` must be at least 1, got 0'),
    'create_poisson/cheb_degree_0': (1, '`cheb_degree` must be at least 1, got 0'),
    'create_poisson_tensor/cheb_degree_0': (1, '`cheb_degree` must be at least 1, got 0'),
    'create_poisson_window/cheb_degree_0': (
        4,
        'amg_hip_create_poisson_window: the Chebyshev smoother is not sharded'
    ),
    'create_rs/cheb_degree_0': (1, '`cheb_degree` must be at least 1, got 0'),
    'create_tensor/cheb_degree_0': (1, '`cheb_degree` must be at least 1, got 0'),
    'create_tensor_dev/cheb_degree_0': (1, '`cheb_degree` must be at least 1, got 0'),
    'create_tensor_periodic/cheb_degree_0': (1, '`cheb_degree` must be at least 1, got 0'),
    'create_tensor_periodic_dev/cheb_degree_0': (1, '`cheb_degree` must be at least 1, got 0'),
    'create_tensor_semi/cheb_degree_0': (1, '`cheb_degree` must be at least 1, got 0'),
    'create_tensor_semi_dev/cheb_degree_0': (1, '`cheb_degree` must be at least 1, got 0'),
    'create/cheb_with_window': (4, 'the Chebyshev smoother is not available in a window solver'),
    'create_custom/cheb_with_window': (4, 'the Chebyshev smoother is not available in a window solver'),
    'create_poisson/cheb_with_window': (4, 'the Chebyshev smoother is not available in a window solver'),
    'create_poisson_tensor/cheb_with_window': (
        4,
        'amg_hip_create_poisson_tensor: window solvers (opt.window) coarsen the flat index; a full-coarsening'
        ' hierarchy is not sharded'
    ),
    'create_poisson_window/cheb_with_window': (
        4,
        'amg_hip_create_poisson_window: the Chebyshev smoother is not sharded'
    ),
    'create_rs/cheb_with_window': (4, 'the Chebyshev smoother is not available in a window solver'),
    'create_tensor/cheb_with_window': (
        4,
        'amg_hip_create_tensor: window solvers (opt.window) coarsen the flat index; a full-coarsening hierarc'
        'hy is not sharded'
    ),
    'create_tensor_dev/cheb_with_window': (
        4,
        'amg_hip_create_tensor_dev: window solvers (opt.window) coarsen the flat index; a full-coarsening hie'
        'rarchy is not sharded'
    ),
    'create_tensor_periodic/cheb_with_window': (
        4,
        'amg_hip_create_tensor_periodic: window solvers (opt.window) coarsen the flat index; a full-coarsenin'
        'g hierarchy is not sharded'
    ),
    'create_tensor_periodic_dev/cheb_with_window': (
        4,
        'amg_hip_create_tensor_periodic_dev: window solvers (opt.window) coarsen the flat index; a full-coars'
        'ening hierarchy is not sharded'
    ),
    'create_tensor_semi/cheb_with_window': (
        4,
        'amg_hip_create_tensor_semi: window solvers (opt.window) coarsen the flat index; a semi-coarsening hi'
        'erarchy is not sharded'
    ),
    'create_tensor_semi_dev/cheb_with_window': (
        4,
        'amg_hip_create_tensor_semi_dev: window solvers (opt.window) coarsen the flat index; a semi-coarsenin'
        'g hierarchy is not sharded'
    ),
    'create/cyclic_lines_2': (1, '`cyclic_lines` must be 0 or 1, got 2'),
    'create_custom/cyclic_lines_2': (1, '`cyclic_lines` must be 0 or 1, got 2'),
    'create_poisson/cyclic_lines_2': (1, 'amg_hip_create_poisson: `cyclic_lines` must be 0 or 1, got 2'),
    'create_poisson_tensor/cyclic_lines_2': (
        1,
        'amg_hip_create_poisson_tensor: `cyclic_lines` must be 0 or 1, got 2'
    ),
    'create_poisson_window/cyclic_lines_2': (
        1,
        'amg_hip_create_poisson_window: `cyclic_lines` must be 0 or 1, got 2'
    ),
    'create_rs/cyclic_lines_2': (1, '`cyclic_lines` must be 0 or 1, got 2'),
    'create_tensor/cyclic_lines_2': (1, '`cyclic_lines` must be 0 or 1, got 2'),
    'create_tensor_dev/cyclic_lines_2': (1, '`cyclic_lines` must be 0 or 1, got 2'),
    'create_tensor_periodic/cyclic_lines_2': (1, '`cyclic_lines` must be 0 or 1, got 2'),
    'create_tensor_periodic_dev/cyclic_lines_2': (1, '`cyclic_lines` must be 0 or 1, got 2'),
    'create_tensor_semi/cyclic_lines_2': (1, '`cyclic_lines` must be 0 or 1, got 2'),
    'create_tensor_semi_dev/cyclic_lines_2': (1, '`cyclic_lines` must be 0 or 1, got 2'),
    'create_tensor_periodic/cyclic_lines_not_line_alt': (
        1,
        '`cyclic_lines` = 1 needs the smoother AMG_HIP_SM_LINE_ALT (AMG_HIP_SM_LINE_JACOBI knows no grid line'
        's and keeps open chains)'
    ),
    'create_tensor_periodic_dev/cyclic_lines_not_line_alt': (
        1,
        '`cyclic_lines` = 1 needs the smoother AMG_HIP_SM_LINE_ALT (AMG_HIP_SM_LINE_JACOBI knows no grid line'
        's and keeps open chains)'
    ),
    'create/cyclic_lines_not_periodic': (
        1,
        '`cyclic_lines` = 1: only amg_hip_create_tensor_periodic and amg_hip_create_tensor_periodic_dev know '
        'the periodic axes of a grid; this constructor needs 0'
    ),
    'create_custom/cyclic_lines_not_periodic': (
        1,
        '`cyclic_lines` = 1: only amg_hip_create_tensor_periodic and amg_hip_create_tensor_periodic_dev know '
        'the periodic axes of a grid; this constructor needs 0'
    ),
    'create_poisson/cyclic_lines_not_periodic': (
        1,
        'amg_hip_create_poisson: `cyclic_lines` = 1: only amg_hip_create_tensor_periodic and amg_hip_create_t'
        'ensor_periodic_dev know the periodic axes of a grid; this constructor needs 0'
    ),
    'create_poisson_tensor/cyclic_lines_not_periodic': (
        1,
        'amg_hip_create_poisson_tensor: `cyclic_lines` = 1: only amg_hip_create_tensor_periodic and amg_hip_c'
        'reate_tensor_periodic_dev know the periodic axes of a grid; this constructor needs 0'
    ),
    'create_poisson_window/cyclic_lines_not_periodic': (
        1,
        'unknown smoother kind for this constructor: AMG_HIP_SM_LINE_ALT needs the level grids of amg_hip_cre'
        'ate_tensor'
    ),
    'create_rs/cyclic_lines_not_periodic': (
        1,
        '`cyclic_lines` = 1: only amg_hip_create_tensor_periodic and amg_hip_create_tensor_periodic_dev know '
        'the periodic axes of a grid; this constructor needs 0'
    ),
    'create_tensor/cyclic_lines_not_periodic': (
        1,
        '`cyclic_lines` = 1: only amg_hip_create_tensor_periodic and amg_hip_create_tensor_periodic_dev know '
        'the periodic axes of a grid; this constructor needs 0'
    ),
    'create_tensor_dev/cyclic_lines_not_periodic': (
        1,
        '`cyclic_lines` = 1: only amg_hip_create_tensor_periodic and amg_hip_create_tensor_periodic_dev know '
        'the periodic axes of a grid; this constructor needs 0'
    ),
    'create_tensor_semi/cyclic_lines_not_periodic': (
        1,
        '`cyclic_lines` = 1: only amg_hip_create_tensor_periodic and amg_hip_create_tensor_periodic_dev know '
        'the periodic axes of a grid; this constructor needs 0'
    ),
    'create_tensor_semi_dev/cyclic_lines_not_periodic': (
        1,
        '`cyclic_lines` = 1: only amg_hip_create_tensor_periodic and amg_hip_create_tensor_periodic_dev know '
        'the periodic axes of a grid; this constructor needs 0'
    ),
    'create_poisson/dim_1': (1, 'dim must be 2 or 3 and n >= 1'),
    'create_poisson_tensor/dim_1': (1, 'amg_hip_create_poisson_tensor: `dim` must be 2 or 3'),
    'create_poisson_window/dim_1': (1, 'dim must be 2 or 3 and n >= 1'),
    'create_tensor/dim_1': (1, 'amg_hip_create_tensor: `dim` must be 2 or 3'),
    'create_tensor_dev/dim_1': (1, 'amg_hip_create_tensor_dev: `dim` must be 2 or 3'),
    'create_tensor_periodic/dim_1': (1, 'amg_hip_create_tensor_periodic: `dim` must be 2 or 3'),
    'create_tensor_periodic_dev/dim_1': (1, 'amg_hip_create_tensor_periodic_dev: `dim` must be 2 or 3'),
    'create_tensor_semi/dim_1': (1, 'amg_hip_create_tensor_semi: `dim` must be 2 or 3'),
    'create_tensor_semi_dev/dim_1': (1, 'amg_hip_create_tensor_semi_dev: `dim` must be 2 or 3'),
    'tensor_axis_strength/dim_1': (1, 'amg_hip_tensor_axis_strength: `dim` must be 2 or 3'),
    'create_poisson/dim_4': (1, 'dim must be 2 or 3 and n >= 1'),
    'create_poisson_tensor/dim_4': (1, 'amg_hip_create_poisson_tensor: `dim` must be 2 or 3'),
    'create_poisson_window/dim_4': (1, 'dim must be 2 or 3 and n >= 1'),
    'create_tensor/dim_4': (1, 'amg_hip_create_tensor: `dim` must be 2 or 3'),
    'create_tensor_dev/dim_4': (1, 'amg_hip_create_tensor_dev: `dim` must be 2 or 3'),
    'create_tensor_periodic/dim_4': (1, 'amg_hip_create_tensor_periodic: `dim` must be 2 or 3'),
    'create_tensor_periodic_dev/dim_4': (1, 'amg_hip_create_tensor_periodic_dev: `dim` must be 2 or 3'),
    'create_tensor_semi/dim_4': (1, 'amg_hip_create_tensor_semi: `dim` must be 2 or 3'),
    'create_tensor_semi_dev/dim_4': (1, 'amg_hip_create_tensor_semi_dev: `dim` must be 2 or 3'),
    'tensor_axis_strength/dim_4': (1, 'amg_hip_tensor_axis_strength: `dim` must be 2 or 3'),
    'create_tensor/dims2_is_2_in_2d': (1, 'amg_hip_create_tensor: `dims[2]` must be 1 when `dim` is 2'),
    'create_tensor_dev/dims2_is_2_in_2d': (1, 'amg_hip_create_tensor_dev: `dims[2]` must be 1 when `dim` is 2'),
    'create_tensor_periodic/dims2_is_2_in_2d': (
        1,
        'amg_hip_create_tensor_periodic: `dims[2]` must be 1 when `dim` is 2'
    ),
    'create_tensor_periodic_dev/dims2_is_2_in_2d': (
        1,
        'amg_hip_create_tensor_periodic_dev: `dims[2]` must be 1 when `dim` is 2'
    ),
    'create_tensor_semi/dims2_is_2_in_2d': (1, 'amg_hip_create_tensor_semi: `dims[2]` must be 1 when `dim` is 2'),
    'create_tensor_semi_dev/dims2_is_2_in_2d': (
        1,
        'amg_hip_create_tensor_semi_dev: `dims[2]` must be 1 when `dim` is 2'
    ),
    'tensor_axis_strength/dims2_is_2_in_2d': (1, 'amg_hip_tensor_axis_strength: `dims[2]` must be 1 when `dim` is 2'),
    'create_tensor/dims_entry_0': (1, 'amg_hip_create_tensor: every entry of `dims` must be at least 1'),
    'create_tensor_dev/dims_entry_0': (1, 'amg_hip_create_tensor_dev: every entry of `dims` must be at least 1'),
    'create_tensor_periodic/dims_entry_0': (
        1,
        'amg_hip_create_tensor_periodic: every entry of `dims` must be at least 1'
    ),
    'create_tensor_periodic_dev/dims_entry_0': (
        1,
        'amg_hip_create_tensor_periodic_dev: every entry of `dims` must be at least 1'
    ),
    'create_tensor_semi/dims_entry_0': (1, 'amg_hip_create_tensor_semi: every entry of `dims` must be at least 1'),
    'create_tensor_semi_dev/dims_entry_0': (
        1,
        'amg_hip_create_tensor_semi_dev: every entry of `dims` must be at least 1'
    ),
    'tensor_axis_strength/dims_entry_0': (
        1,
        'amg_hip_tensor_axis_strength: every entry of `dims` must be at least 1'
    ),
    'create_tensor/dims_null': (1, 'amg_hip_create_tensor: `dims` is null'),
    'create_tensor_dev/dims_null': (1, 'amg_hip_create_tensor_dev: `dims` is null'),
    'create_tensor_periodic/dims_null': (1, 'amg_hip_create_tensor_periodic: `dims` is null'),
    'create_tensor_periodic_dev/dims_null': (1, 'amg_hip_create_tensor_periodic_dev: `dims` is null'),
    'create_tensor_semi/dims_null': (1, 'amg_hip_create_tensor_semi: `dims` is null'),
    'create_tensor_semi_dev/dims_null': (1, 'amg_hip_create_tensor_semi_dev: `dims` is null'),
    'tensor_axis_strength/dims_null': (1, 'amg_hip_tensor_axis_strength: `dims` is null'),
    'create/layout_9': (1, 'unknown matrix layout'),
    'create_custom/layout_9': (1, 'unknown matrix layout'),
    'create_poisson/layout_9': (1, 'unknown matrix layout'),
    'create_poisson_tensor/layout_9': (1, 'unknown matrix layout'),
    'create_poisson_window/layout_9': (1, 'unknown matrix layout'),
    'create_rs/layout_9': (1, 'unknown matrix layout'),
    'create_tensor/layout_9': (1, 'unknown matrix layout'),
    'create_tensor_dev/layout_9': (1, 'unknown matrix layout'),
    'create_tensor_periodic/layout_9': (1, 'unknown matrix layout'),
    'create_tensor_periodic_dev/layout_9': (1, 'unknown matrix layout'),
    'create_tensor_semi/layout_9': (1, 'unknown matrix layout'),
    'create_tensor_semi_dev/layout_9': (1, 'unknown matrix layout'),
    'create_tensor/level_9x6x5_4': (
        1,
        'level 3 is not possible: level 2 is a 2 x 1 x 1 grid and an axis of fewer than 2 points cannot be co'
        'arsened; reduce `n_levels`'
    ),
    'create_tensor_dev/level_9x6x5_4': (
        1,
        'level 3 is not possible: level 2 is a 2 x 1 x 1 grid and an axis of fewer than 2 points cannot be co'
        'arsened; reduce `n_levels`'
    ),
    'create_tensor_periodic/level_9x6x5_4': (
        1,
        'level 3 is not possible: level 2 is a 2 x 1 x 1 grid and an axis of fewer than 2 points cannot be co'
        'arsened; reduce `n_levels`'
    ),
    'create_tensor_periodic_dev/level_9x6x5_4': (
        1,
        'level 3 is not possible: level 2 is a 2 x 1 x 1 grid and an axis of fewer than 2 points cannot be co'
        'arsened; reduce `n_levels`'
    ),
    'create_poisson_tensor/level_9x9_5': (
        1,
        'level 4 is not possible: level 3 is a 1 x 1 x 1 grid and an axis of fewer than 2 points cannot be co'
        'arsened; reduce `n_levels`'
    ),
    'create_tensor/level_9x9_5': (
        1,
        'level 4 is not possible: level 3 is a 1 x 1 x 1 grid and an axis of fewer than 2 points cannot be co'
        'arsened; reduce `n_levels`'
    ),
    'create_tensor_dev/level_9x9_5': (
        1,
        'level 4 is not possible: level 3 is a 1 x 1 x 1 grid and an axis of fewer than 2 points cannot be co'
        'arsened; reduce `n_levels`'
    ),
    'create_tensor_periodic/level_9x9_5': (
        1,
        'level 4 is not possible: level 3 is a 1 x 1 x 1 grid and an axis of fewer than 2 points cannot be co'
        'arsened; reduce `n_levels`'
    ),
    'create_tensor_periodic_dev/level_9x9_5': (
        1,
        'level 4 is not possible: level 3 is a 1 x 1 x 1 grid and an axis of fewer than 2 points cannot be co'
        'arsened; reduce `n_levels`'
    ),
    'create/line_alt_without_grid': (
        1,
        'unknown smoother kind for this constructor: AMG_HIP_SM_LINE_ALT needs the level grids of amg_hip_cre'
        'ate_tensor'
    ),
    'create_custom/line_alt_without_grid': (
        1,
        'unknown smoother kind for this constructor: AMG_HIP_SM_LINE_ALT needs the level grids of amg_hip_cre'
        'ate_tensor'
    ),
    'create_poisson/line_alt_without_grid': (
        1,
        'unknown smoother kind for this constructor: AMG_HIP_SM_LINE_ALT needs the level grids of amg_hip_cre'
        'ate_tensor'
    ),
    'create_poisson_window/line_alt_without_grid': (
        1,
        'unknown smoother kind for this constructor: AMG_HIP_SM_LINE_ALT needs the level grids of amg_hip_cre'
        'ate_tensor'
    ),
    'create_rs/line_alt_without_grid': (
        1,
        'unknown smoother kind for this constructor: AMG_HIP_SM_LINE_ALT needs the level grids of amg_hip_cre'
        'ate_tensor'
    ),
    'create/line_omega_0': (1, 'line smoother: `omega` must lie in (0, 2), got 0.000000'),
    'create_custom/line_omega_0': (1, 'line smoother: `omega` must lie in (0, 2), got 0.000000'),
    'create_poisson/line_omega_0': (1, 'line smoother: `omega` must lie in (0, 2), got 0.000000'),
    'create_poisson_tensor/line_omega_0': (1, 'line smoother: `omega` must lie in (0, 2), got 0.000000'),
    'create_poisson_window/line_omega_0': (4, 'amg_hip_create_poisson_window: the line smoother is not sharded'),
    'create_rs/line_omega_0': (1, 'line smoother: `omega` must lie in (0, 2), got 0.000000'),
    'create_tensor/line_omega_0': (1, 'line smoother: `omega` must lie in (0, 2), got 0.000000'),
    'create_tensor_dev/line_omega_0': (1, 'line smoother: `omega` must lie in (0, 2), got 0.000000'),
    'create_tensor_periodic/line_omega_0': (1, 'line smoother: `omega` must lie in (0, 2), got 0.000000'),
    'create_tensor_periodic_dev/line_omega_0': (1, 'line smoother: `omega` must lie in (0, 2), got 0.000000'),
    'create_tensor_semi/line_omega_0': (1, 'line smoother: `omega` must lie in (0, 2), got 0.000000'),
    'create_tensor_semi_dev/line_omega_0': (1, 'line smoother: `omega` must lie in (0, 2), got 0.000000'),
    'create/line_omega_2': (1, 'line smoother: `omega` must lie in (0, 2), got 2.000000'),
    'create_custom/line_omega_2': (1, 'line smoother: `omega` must lie in (0, 2), got 2.000000'),
    'create_poisson/line_omega_2': (1, 'line smoother: `omega` must lie in (0, 2), got 2.000000'),
    'create_poisson_tensor/line_omega_2': (1, 'line smoother: `omega` must lie in (0, 2), got 2.000000'),
    'create_poisson_window/line_omega_2': (4, 'amg_hip_create_poisson_window: the line smoother is not sharded'),
    'create_rs/line_omega_2': (1, 'line smoother: `omega` must lie in (0, 2), got 2.000000'),
    'create_tensor/line_omega_2': (1, 'line smoother: `omega` must lie in (0, 2), got 2.000000'),
    'create_tensor_dev/line_omega_2': (1, 'line smoother: `omega` must lie in (0, 2), got 2.000000'),
    'create_tensor_periodic/line_omega_2': (1, 'line smoother: `omega` must lie in (0, 2), got 2.000000'),
    'create_tensor_periodic_dev/line_omega_2': (1, 'line smoother: `omega` must lie in (0, 2), got 2.000000'),
    'create_tensor_semi/line_omega_2': (1, 'line smoother: `omega` must lie in (0, 2), got 2.000000'),
    'create_tensor_semi_dev/line_omega_2': (1, 'line smoother: `omega` must lie in (0, 2), got 2.000000'),
    'create/line_with_window': (4, 'the line smoother is not available in a window solver'),
    'create_custom/line_with_window': (4, 'the line smoother is not available in a window solver'),
    'create_poisson/line_with_window': (4, 'the line smoother is not available in a window solver'),
    'create_poisson_tensor/line_with_window': (
        4,
        'amg_hip_create_poisson_tensor: window solvers (opt.window) coarsen the flat index; a full-coarsening'
        ' hierarchy is not sharded'
    ),
    'create_poisson_window/line_with_window': (4, 'amg_hip_create_poisson_window: the line smoother is not sharded'),
    'create_rs/line_with_window': (4, 'the line smoother is not available in a window solver'),
    'create_tensor/line_with_window': (
        4,
        'amg_hip_create_tensor: window solvers (opt.window) coarsen the flat index; a full-coarsening hierarc'
        'hy is not sharded'
    ),
    'create_tensor_dev/line_with_window': (
        4,
        'amg_hip_create_tensor_dev: window solvers (opt.window) coarsen the flat index; a full-coarsening hie'
        'rarchy is not sharded'
    ),
    'create_tensor_periodic/line_with_window': (
        4,
        'amg_hip_create_tensor_periodic: window solvers (opt.window) coarsen the flat index; a full-coarsenin'
        'g hierarchy is not sharded'
    ),
    'create_tensor_periodic_dev/line_with_window': (
        4,
        'amg_hip_create_tensor_periodic_dev: window solvers (opt.window) coarsen the flat index; a full-coars'
        'ening hierarchy is not sharded'
    ),
    'create_tensor_semi/line_with_window': (
        4,
        'amg_hip_create_tensor_semi: window solvers (opt.window) coarsen the flat index; a semi-coarsening hi'
        'erarchy is not sharded'
    ),
    'create_tensor_semi_dev/line_with_window': (
        4,
        'amg_hip_create_tensor_semi_dev: window solvers (opt.window) coarsen the flat index; a semi-coarsenin'
        'g hierarchy is not sharded'
    ),
    'create_tensor_periodic/mask_0': (1, 'amg_hip_create_tensor_periodic: level 0: axis mask 0 coarsens no axis'),
    'create_tensor_periodic_dev/mask_0': (
        1,
        'amg_hip_create_tensor_periodic_dev: level 0: axis mask 0 coarsens no axis'
    ),
    'create_tensor_semi/mask_0': (1, 'amg_hip_create_tensor_semi: level 0: axis mask 0 coarsens no axis'),
    'create_tensor_semi_dev/mask_0': (1, 'amg_hip_create_tensor_semi_dev: level 0: axis mask 0 coarsens no axis'),
    'create_tensor_periodic/mask_axis_of_one_point': (
        1,
        'amg_hip_create_tensor_periodic: level 0: axis mask 2 coarsens axis y, which has 1 point on this leve'
        'l (the grid is 4 x 1 x 1)'
    ),
    'create_tensor_periodic_dev/mask_axis_of_one_point': (
        1,
        'amg_hip_create_tensor_periodic_dev: level 0: axis mask 2 coarsens axis y, which has 1 point on this '
        'level (the grid is 4 x 1 x 1)'
    ),
    'create_tensor_semi/mask_axis_of_one_point': (
        1,
        'amg_hip_create_tensor_semi: level 0: axis mask 2 coarsens axis y, which has 1 point on this level (t'
        'he grid is 4 x 1 x 1)'
    ),
    'create_tensor_semi_dev/mask_axis_of_one_point': (
        1,
        'amg_hip_create_tensor_semi_dev: level 0: axis mask 2 coarsens axis y, which has 1 point on this leve'
        'l (the grid is 4 x 1 x 1)'
    ),
    'create_tensor_periodic/mask_bit_3': (
        1,
        'amg_hip_create_tensor_periodic: level 0: axis mask 8 has bits other than 1 (x), 2 (y) and 4 (z)'
    ),
    'create_tensor_periodic_dev/mask_bit_3': (
        1,
        'amg_hip_create_tensor_periodic_dev: level 0: axis mask 8 has bits other than 1 (x), 2 (y) and 4 (z)'
    ),
    'create_tensor_semi/mask_bit_3': (
        1,
        'amg_hip_create_tensor_semi: level 0: axis mask 8 has bits other than 1 (x), 2 (y) and 4 (z)'
    ),
    'create_tensor_semi_dev/mask_bit_3': (
        1,
        'amg_hip_create_tensor_semi_dev: level 0: axis mask 8 has bits other than 1 (x), 2 (y) and 4 (z)'
    ),
    'create_tensor/n_15': (1, 'amg_hip_create_tensor: `n` = 15 is not the 4 x 4 x 1 grid of `dims`'),
    'create_tensor_dev/n_15': (1, 'amg_hip_create_tensor_dev: `n` = 15 is not the 4 x 4 x 1 grid of `dims`'),
    'create_tensor_periodic/n_15': (
        1,
        'amg_hip_create_tensor_periodic: `n` = 15 is not the 4 x 4 x 1 grid of `dims`'
    ),
    'create_tensor_periodic_dev/n_15': (
        1,
        'amg_hip_create_tensor_periodic_dev: `n` = 15 is not the 4 x 4 x 1 grid of `dims`'
    ),
    'create_tensor_semi/n_15': (1, 'amg_hip_create_tensor_semi: `n` = 15 is not the 4 x 4 x 1 grid of `dims`'),
    'create_tensor_semi_dev/n_15': (
        1,
        'amg_hip_create_tensor_semi_dev: `n` = 15 is not the 4 x 4 x 1 grid of `dims`'
    ),
    'tensor_axis_strength/n_15': (1, 'amg_hip_tensor_axis_strength: `n` is not the number of points of `dims`'),
    'create/n_levels_0': (1, '`n_levels` must be at least 1'),
    'create_custom/n_levels_0': (1, '`n_levels` must be at least 1'),
    'create_poisson/n_levels_0': (1, '`n_levels` must be at least 1'),
    'create_poisson_tensor/n_levels_0': (1, '`n_levels` must be at least 1'),
    'create_poisson_window/n_levels_0': (1, 'a window solver needs at least one distributed level (n_levels >= 2)'),
    'create_rs/n_levels_0': (1, '`n_levels` must be at least 1'),
    'create_tensor/n_levels_0': (1, '`n_levels` must be at least 1'),
    'create_tensor_dev/n_levels_0': (1, '`n_levels` must be at least 1'),
    'create_tensor_periodic/n_levels_0': (1, '`n_levels` must be at least 1'),
    'create_tensor_periodic_dev/n_levels_0': (1, '`n_levels` must be at least 1'),
    'create_tensor_semi/n_levels_0': (1, '`n_levels` must be at least 1'),
    'create_tensor_semi_dev/n_levels_0': (1, '`n_levels` must be at least 1'),
    'create_tensor_periodic/natural_side_on_periodic_axis': (
        1,
        '`natural_sides` = 1 names a side of axis x, which `periodic_axes` = 1 makes periodic: a periodic axi'
        's has no sides'
    ),
    'create_tensor_periodic_dev/natural_side_on_periodic_axis': (
        1,
        '`natural_sides` = 1 names a side of axis x, which `periodic_axes` = 1 makes periodic: a periodic axi'
        's has no sides'
    ),
    'create_tensor/natural_sides_beyond_2dim': (
        1,
        '`natural_sides` = 16 has bits other than the 4 sides of a 2-D grid (bit 2a = low side of axis a, bit'
        ' 2a + 1 = high side)'
    ),
    'create_tensor_dev/natural_sides_beyond_2dim': (
        1,
        '`natural_sides` = 16 has bits other than the 4 sides of a 2-D grid (bit 2a = low side of axis a, bit'
        ' 2a + 1 = high side)'
    ),
    'create_tensor_periodic/natural_sides_beyond_2dim': (
        1,
        '`natural_sides` = 16 has bits other than the 4 sides of a 2-D grid (bit 2a = low side of axis a, bit'
        ' 2a + 1 = high side)'
    ),
    'create_tensor_periodic_dev/natural_sides_beyond_2dim': (
        1,
        '`natural_sides` = 16 has bits other than the 4 sides of a 2-D grid (bit 2a = low side of axis a, bit'
        ' 2a + 1 = high side)'
    ),
    'create_tensor_semi/natural_sides_beyond_2dim': (
        1,
        '`natural_sides` = 16 has bits other than the 4 sides of a 2-D grid (bit 2a = low side of axis a, bit'
        ' 2a + 1 = high side)'
    ),
    'create_tensor_semi_dev/natural_sides_beyond_2dim': (
        1,
        '`natural_sides` = 16 has bits other than the 4 sides of a 2-D grid (bit 2a = low side of axis a, bit'
        ' 2a + 1 = high side)'
    ),
    'create/natural_sides_not_taken': (
        1,
        '`natural_sides` = 1: only the tensor constructors (amg_hip_create_tensor, _tensor_semi, _tensor_dev,'
        ' _tensor_semi_dev) know the sides of a grid; this constructor needs 0'
    ),
    'create_custom/natural_sides_not_taken': (
        1,
        '`natural_sides` = 1: only the tensor constructors (amg_hip_create_tensor, _tensor_semi, _tensor_dev,'
        ' _tensor_semi_dev) know the sides of a grid; this constructor needs 0'
    ),
    'create_poisson/natural_sides_not_taken': (
        1,
        'amg_hip_create_poisson: `natural_sides` = 1: only the tensor constructors (amg_hip_create_tensor, _t'
        'ensor_semi, _tensor_dev, _tensor_semi_dev) know the sides of a grid; this constructor needs 0'
    ),
    'create_poisson_tensor/natural_sides_not_taken': (
        1,
        'amg_hip_create_poisson_tensor: `natural_sides` = 1: only the tensor constructors (amg_hip_create_ten'
        'sor, _tensor_semi, _tensor_dev, _tensor_semi_dev) know the sides of a grid; this constructor needs 0'
    ),
    'create_poisson_window/natural_sides_not_taken': (
        1,
        'amg_hip_create_poisson_window: `natural_sides` = 1: only the tensor constructors (amg_hip_create_ten'
        'sor, _tensor_semi, _tensor_dev, _tensor_semi_dev) know the sides of a grid; this constructor needs 0'
    ),
    'create_rs/natural_sides_not_taken': (
        1,
        '`natural_sides` = 1: only the tensor constructors (amg_hip_create_tensor, _tensor_semi, _tensor_dev,'
        ' _tensor_semi_dev) know the sides of a grid; this constructor needs 0'
    ),
    'create_custom/null_P_colptr': (1, 'custom transfer operator arrays are null'),
    'create_custom/null_P_rowind': (1, 'custom transfer operator arrays are null'),
    'create_custom/null_P_val': (1, 'custom transfer operator arrays are null'),
    'create_custom/null_R_colptr': (1, 'custom transfer operator arrays are null'),
    'create_custom/null_R_rowind': (1, 'custom transfer operator arrays are null'),
    'create_custom/null_R_val': (1, 'custom transfer operator arrays are null'),
    'create/null_b': (1, 'null input array'),
    'create_custom/null_b': (1, 'null input array'),
    'create_rs/null_b': (1, 'null input array'),
    'create_tensor/null_b': (1, 'null input array'),
    'create_tensor_dev/null_b': (1, 'null input array'),
    'create_tensor_periodic/null_b': (1, 'null input array'),
    'create_tensor_periodic_dev/null_b': (1, 'null input array'),
    'create_tensor_semi/null_b': (1, 'null input array'),
    'create_tensor_semi_dev/null_b': (1, 'null input array'),
    'create_tensor_dev/null_col': (1, 'null input array'),
    'create_tensor_periodic_dev/null_col': (1, 'null input array'),
    'create_tensor_semi_dev/null_col': (1, 'null input array'),
    'create/null_colptr': (1, 'null input array'),
    'create_custom/null_colptr': (1, 'null input array'),
    'create_rs/null_colptr': (1, 'null input array'),
    'create_tensor/null_colptr': (1, 'null input array'),
    'create_tensor_periodic/null_colptr': (1, 'null input array'),
    'create_tensor_semi/null_colptr': (1, 'null input array'),
    'tensor_axis_strength/null_colptr': (1, 'null argument'),
    'create/null_out': (1, 'out handle pointer is null'),
    'create_custom/null_out': (1, 'out handle pointer is null'),
    'create_poisson/null_out': (1, 'out handle pointer is null'),
    'create_poisson_tensor/null_out': (1, 'out handle pointer is null'),
    'create_poisson_window/null_out': (1, 'out handle pointer is null'),
    'create_rs/null_out': (1, 'out handle pointer is null'),
    'create_tensor/null_out': (1, 'out handle pointer is null'),
    'create_tensor_dev/null_out': (1, 'out handle pointer is null'),
    'create_tensor_periodic/null_out': (1, 'out handle pointer is null'),
    'create_tensor_periodic_dev/null_out': (1, 'out handle pointer is null'),
    'create_tensor_semi/null_out': (1, 'out handle pointer is null'),
    'create_tensor_semi_dev/null_out': (1, 'out handle pointer is null'),
    'create/null_rowind': (1, 'null input array'),
    'create_custom/null_rowind': (1, 'null input array'),
    'create_rs/null_rowind': (1, 'null input array'),
    'create_tensor/null_rowind': (1, 'null input array'),
    'create_tensor_periodic/null_rowind': (1, 'null input array'),
    'create_tensor_semi/null_rowind': (1, 'null input array'),
    'tensor_axis_strength/null_rowind': (1, 'null argument'),
    'create_tensor_dev/null_rowptr': (1, 'null input array'),
    'create_tensor_periodic_dev/null_rowptr': (1, 'null input array'),
    'create_tensor_semi_dev/null_rowptr': (1, 'null input array'),
    'create/null_val': (1, 'null input array'),
    'create_custom/null_val': (1, 'null input array'),
    'create_rs/null_val': (1, 'null input array'),
    'create_tensor/null_val': (1, 'null input array'),
    'create_tensor_dev/null_val': (1, 'null input array'),
    'create_tensor_periodic/null_val': (1, 'null input array'),
    'create_tensor_periodic_dev/null_val': (1, 'null input array'),
    'create_tensor_semi/null_val': (1, 'null input array'),
    'create_tensor_semi_dev/null_val': (1, 'null input array'),
    'tensor_axis_strength/null_val': (1, 'null argument'),
    'tensor_axis_strength/null_w': (1, 'null argument'),
    'create_tensor_periodic/periodic_6_to_3': (
        1,
        'amg_hip_create_tensor_periodic: level 1: `periodic_axes` = 1 makes axis x periodic, and it has 3 poi'
        'nts on this level; a coarsened periodic axis needs an even length of at least 4 (the grid is 3 x 2 x'
        ' 1)'
    ),
    'create_tensor_periodic_dev/periodic_6_to_3': (
        1,
        'amg_hip_create_tensor_periodic_dev: level 1: `periodic_axes` = 1 makes axis x periodic, and it has 3'
        ' points on this level; a coarsened periodic axis needs an even length of at least 4 (the grid is 3 x'
        ' 2 x 1)'
    ),
    'create_tensor_periodic/periodic_axes_8': (
        1,
        'amg_hip_create_tensor_periodic: `periodic_axes` = 8 has bits other than the 2 axes of a 2-D grid (bi'
        't a = axis a: 1 = x, 2 = y, 4 = z)'
    ),
    'create_tensor_periodic_dev/periodic_axes_8': (
        1,
        'amg_hip_create_tensor_periodic_dev: `periodic_axes` = 8 has bits other than the 2 axes of a 2-D grid'
        ' (bit a = axis a: 1 = x, 2 = y, 4 = z)'
    ),
    'create_tensor_periodic/periodic_z_in_2d': (
        1,
        'amg_hip_create_tensor_periodic: `periodic_axes` = 4 has bits other than the 2 axes of a 2-D grid (bi'
        't a = axis a: 1 = x, 2 = y, 4 = z)'
    ),
    'create_tensor_periodic_dev/periodic_z_in_2d': (
        1,
        'amg_hip_create_tensor_periodic_dev: `periodic_axes` = 4 has bits other than the 2 axes of a 2-D grid'
        ' (bit a = axis a: 1 = x, 2 = y, 4 = z)'
    ),
    'create/singular_2': (1, '`singular` must be 0 or 1, got 2'),
    'create_custom/singular_2': (1, '`singular` must be 0 or 1, got 2'),
    'create_poisson/singular_2': (1, 'amg_hip_create_poisson: `singular` must be 0 or 1, got 2'),
    'create_poisson_tensor/singular_2': (1, 'amg_hip_create_poisson_tensor: `singular` must be 0 or 1, got 2'),
    'create_poisson_window/singular_2': (1, 'amg_hip_create_poisson_window: `singular` must be 0 or 1, got 2'),
    'create_rs/singular_2': (1, '`singular` must be 0 or 1, got 2'),
    'create_tensor/singular_2': (1, '`singular` must be 0 or 1, got 2'),
    'create_tensor_dev/singular_2': (1, '`singular` must be 0 or 1, got 2'),
    'create_tensor_periodic/singular_2': (1, '`singular` must be 0 or 1, got 2'),
    'create_tensor_periodic_dev/singular_2': (1, '`singular` must be 0 or 1, got 2'),
    'create_tensor_semi/singular_2': (1, '`singular` must be 0 or 1, got 2'),
    'create_tensor_semi_dev/singular_2': (1, '`singular` must be 0 or 1, got 2'),
    'create/singular_not_taken': (
        1,
        '`singular` = 1 needs every side in `natural_sides`, which only the tensor constructors take'
    ),
    'create_custom/singular_not_taken': (
        1,
        '`singular` = 1 needs every side in `natural_sides`, which only the tensor constructors take'
    ),
    'create_poisson/singular_not_taken': (
        1,
        'amg_hip_create_poisson: `singular` = 1 needs every side in `natural_sides`, which only the tensor co'
        'nstructors take'
    ),
    'create_poisson_tensor/singular_not_taken': (
        1,
        'amg_hip_create_poisson_tensor: `singular` = 1 needs every side in `natural_sides`, which only the te'
        'nsor constructors take'
    ),
    'create_poisson_window/singular_not_taken': (
        1,
        'amg_hip_create_poisson_window: `singular` = 1 needs every side in `natural_sides`, which only the te'
        'nsor constructors take'
    ),
    'create_rs/singular_not_taken': (
        1,
        '`singular` = 1 needs every side in `natural_sides`, which only the tensor constructors take'
    ),
    'create_tensor/singular_one_level': (
        1,
        '`singular` = 1 needs a hierarchy of at least 2 levels: with one level the pinned solve would zero th'
        "e last entry of the caller's own right-hand side"
    ),
    'create_tensor_dev/singular_one_level': (
        1,
        '`singular` = 1 needs a hierarchy of at least 2 levels: with one level the pinned solve would zero th'
        "e last entry of the caller's own right-hand side"
    ),
    'create_tensor_periodic/singular_one_level': (
        1,
        '`singular` = 1 needs a hierarchy of at least 2 levels: with one level the pinned solve would zero th'
        "e last entry of the caller's own right-hand side"
    ),
    'create_tensor_periodic_dev/singular_one_level': (
        1,
        '`singular` = 1 needs a hierarchy of at least 2 levels: with one level the pinned solve would zero th'
        "e last entry of the caller's own right-hand side"
    ),
    'create_tensor_semi/singular_one_level': (
        1,
        '`singular` = 1 needs a hierarchy of at least 2 levels: with one level the pinned solve would zero th'
        "e last entry of the caller's own right-hand side"
    ),
    'create_tensor_semi_dev/singular_one_level': (
        1,
        '`singular` = 1 needs a hierarchy of at least 2 levels: with one level the pinned solve would zero th'
        "e last entry of the caller's own right-hand side"
    ),
    'create/smoother_17': (1, 'unknown smoother kind'),
    'create_custom/smoother_17': (1, 'unknown smoother kind'),
    'create_poisson/smoother_17': (1, 'unknown smoother kind'),
    'create_poisson_tensor/smoother_17': (1, 'unknown smoother kind'),
    'create_poisson_window/smoother_17': (1, 'unknown smoother kind'),
    'create_rs/smoother_17': (1, 'unknown smoother kind'),
    'create_tensor/smoother_17': (1, 'unknown smoother kind'),
    'create_tensor_dev/smoother_17': (1, 'unknown smoother kind'),
    'create_tensor_periodic/smoother_17': (1, 'unknown smoother kind'),
    'create_tensor_periodic_dev/smoother_17': (1, 'unknown smoother kind'),
    'create_tensor_semi/smoother_17': (1, 'unknown smoother kind'),
    'create_tensor_semi_dev/smoother_17': (1, 'unknown smoother kind'),
    'create/smoother_iters_-1': (1, '`smoother_iters` must be >= 0'),
    'create_custom/smoother_iters_-1': (1, '`smoother_iters` must be >= 0'),
    'create_poisson/smoother_iters_-1': (1, '`smoother_iters` must be >= 0'),
    'create_poisson_tensor/smoother_iters_-1': (1, '`smoother_iters` must be >= 0'),
    'create_poisson_window/smoother_iters_-1': (1, '`smoother_iters` must be >= 0'),
    'create_rs/smoother_iters_-1': (1, '`smoother_iters` must be >= 0'),
    'create_tensor/smoother_iters_-1': (1, '`smoother_iters` must be >= 0'),
    'create_tensor_dev/smoother_iters_-1': (1, '`smoother_iters` must be >= 0'),
    'create_tensor_periodic/smoother_iters_-1': (1, '`smoother_iters` must be >= 0'),
    'create_tensor_periodic_dev/smoother_iters_-1': (1, '`smoother_iters` must be >= 0'),
    'create_tensor_semi/smoother_iters_-1': (1, '`smoother_iters` must be >= 0'),
    'create_tensor_semi_dev/smoother_iters_-1': (1, '`smoother_iters` must be >= 0'),
    'create/sor_omega_3': (1, '`omega` must be in [0, 2] but got omega=3.000000\n'),
    'create_custom/sor_omega_3': (1, '`omega` must be in [0, 2] but got omega=3.000000\n'),
    'create_poisson/sor_omega_3': (1, '`omega` must be in [0, 2] but got omega=3.000000\n'),
    'create_poisson_tensor/sor_omega_3': (1, '`omega` must be in [0, 2] but got omega=3.000000\n'),
    'create_poisson_window/sor_omega_3': (1, '`omega` must be in [0, 2] but got omega=3.000000\n'),
    'create_rs/sor_omega_3': (1, '`omega` must be in [0, 2] but got omega=3.000000\n'),
    'create_tensor/sor_omega_3': (1, '`omega` must be in [0, 2] but got omega=3.000000\n'),
    'create_tensor_dev/sor_omega_3': (1, '`omega` must be in [0, 2] but got omega=3.000000\n'),
    'create_tensor_periodic/sor_omega_3': (1, '`omega` must be in [0, 2] but got omega=3.000000\n'),
    'create_tensor_periodic_dev/sor_omega_3': (1, '`omega` must be in [0, 2] but got omega=3.000000\n'),
    'create_tensor_semi/sor_omega_3': (1, '`omega` must be in [0, 2] but got omega=3.000000\n'),
    'create_tensor_semi_dev/sor_omega_3': (1, '`omega` must be in [0, 2] but got omega=3.000000\n'),
    'create_poisson_tensor/window': (
        4,
        'amg_hip_create_poisson_tensor: window solvers (opt.window) coarsen the flat index; a full-coarsening'
        ' hierarchy is not sharded'
    ),
    'create_tensor/window': (
        4,
        'amg_hip_create_tensor: window solvers (opt.window) coarsen the flat index; a full-coarsening hierarc'
        'hy is not sharded'
    ),
    'create_tensor_dev/window': (
        4,
        'amg_hip_create_tensor_dev: window solvers (opt.window) coarsen the flat index; a full-coarsening hie'
        'rarchy is not sharded'
    ),
    'create_tensor_periodic/window': (
        4,
        'amg_hip_create_tensor_periodic: window solvers (opt.window) coarsen the flat index; a full-coarsenin'
        'g hierarchy is not sharded'
    ),
    'create_tensor_periodic_dev/window': (
        4,
        'amg_hip_create_tensor_periodic_dev: window solvers (opt.window) coarsen the flat index; a full-coars'
        'ening hierarchy is not sharded'
    ),
    'create_tensor_semi/window': (
        4,
        'amg_hip_create_tensor_semi: window solvers (opt.window) coarsen the flat index; a semi-coarsening hi'
        'erarchy is not sharded'
    ),
    'create_tensor_semi_dev/window': (
        4,
        'amg_hip_create_tensor_semi_dev: window solvers (opt.window) coarsen the flat index; a semi-coarsenin'
        'g hierarchy is not sharded'
    ),
    'create_poisson_window/window_cheb': (4, 'amg_hip_create_poisson_window: the Chebyshev smoother is not sharded'),
    'create_poisson_window/window_line': (4, 'amg_hip_create_poisson_window: the line smoother is not sharded'),
    'create_poisson_window/window_odd_start': (
        1,
        'a window must begin at an even flat index (coarse dof j <-> fine dof 2j+1, multigrid.hpp:127-130)'
    ),
    'create_poisson_window/window_units_empty': (1, 'window units must satisfy 0 <= unit_begin < unit_end <= n'),
    'create_poisson_window/window_units_out_of_range': (
        1,
        'window units must satisfy 0 <= unit_begin < unit_end <= n'
    ),
}


def test_every_case_has_its_literal():
    assert sorted(EXPECTED) == IDS


@pytest.mark.parametrize("entry", sorted({i.split("/")[0] for i in IDS}))
def test_status_and_message(amg, entry):
    wrong = []
    for name, (entries, kw) in sorted(CASES.items()):
        if entry in entries:
            got = call(amg, entry, **kw)
            if got != EXPECTED[f"{entry}/{name}"]:
                wrong.append((name, got, EXPECTED[f"{entry}/{name}"]))
    assert not wrong, wrong


def test_host_and_dev_twins_say_the_same(amg):
    """the same bad grid, mask or option: the same words after the prefix that names the entry point"""
    shared = ("dim_1", "dim_4", "dims_null", "dims_entry_0", "dims2_is_2_in_2d", "n_15", "window", "level_9x9_5",
              "level_9x6x5_4", "mask_0", "mask_axis_of_one_point", "mask_bit_3", "auto_theta_0", "auto_min_coarse_0",
              "periodic_axes_8", "periodic_z_in_2d", "periodic_6_to_3", "natural_side_on_periodic_axis",
              "natural_sides_beyond_2dim", "singular_one_level", "singular_2", "cyclic_lines_2",
              "cyclic_lines_not_periodic", "cyclic_lines_not_line_alt", "smoother_17", "smoother_iters_-1",
              "cheb_degree_0", "line_omega_0", "line_omega_2", "layout_9", "sor_omega_3")
    seen = 0
    for host, dev in zip(TENSOR, DEV):
        for name in shared:
            entries, kw = CASES[name]
            if host not in entries or dev not in entries:
                continue
            (hs, hm), (ds, dm) = call(amg, host, **kw), call(amg, dev, **kw)
            assert hs == ds, (host, name)
            assert hm.replace(f"amg_hip_{host}: ", "") == dm.replace(f"amg_hip_{dev}: ", ""), (host, name)
            seen += 1
    assert seen >= 70
