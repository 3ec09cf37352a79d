"""Which set-up path built each solver, and what it built.  Every device constructor has a silent
fall-back to the host constructor that gives the same V-cycle bit for bit, so a wrong fall-back (or a
host twin that takes another layout) is invisible to the parity tests.  Here setup_on_device, the
number of levels and, per level, the grid, the layout, the transfer kind, the coarsened axes, the line
directions and the level-0 smoother kernel are literals, recorded from the library before the set-up
code was reorganised; one V-cycle is compared bitwise with the host twin of the constructor:

  poisson            <-> Multigrid (amg_hip_create) on the host arrays
  poisson_tensor     <-> Multigrid.tensor on the host arrays
  tensor_dev         <-> tensor
  tensor_semi_dev    <-> tensor_semi
  tensor_periodic_dev <-> tensor_periodic, with set_periodic_device_setup 0 and 1

65 536 rows (n = 256) is where the host constructor starts to encode on the device; the lexicographic
smoothers take K-GS-scan only above that, so they run at n = 256 and n = 257."""
import os
import sys

import numpy as np
import pytest

sp = pytest.importorskip("scipy.sparse")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import periodic_twin as PT  # noqa: E402
from test_gpu_periodic_device_setup import dev_arrays, frozen  # noqa: E402
from test_gpu_tensor_dev_setup import anisotropic, diffusion, integer_kappa  # noqa: E402

pytestmark = pytest.mark.gpu

SPGS, JACOBI, MC, CHEB, LINE, ALT = 0, 3, 4, 5, 6, 7
SM = {
    "jacobi": dict(smoother=JACOBI, smoother_iters=2, omega=0.8),
    "cheb": dict(smoother=CHEB, smoother_iters=1, cheb_degree=2),
    "line": dict(smoother=LINE, smoother_iters=1, omega=0.7),
    "alt": dict(smoother=ALT, smoother_iters=1, omega=0.8),
    "spgs": dict(smoother=SPGS, smoother_iters=1, keep_residual=True),
    "mc": dict(smoother=MC, smoother_iters=1),
}
_OPS = {}


def operator(name):
    """(A as CSR, A as CSC, b) of a named operator: built once and never modified"""
    if name not in _OPS:
        if name == "box":  # the variable-coefficient operator of tests/test_gpu_tensor_dev_setup.py
            A = diffusion((33, 20, 12), integer_kappa(1), 1.0)
            b = np.random.default_rng(99).standard_normal(A.shape[0])
        elif name == "strip":  # strong along x
            A = diffusion((64, 16), anisotropic, 0.0)
            b = np.random.default_rng(99).standard_normal(A.shape[0])
        else:  # "ring": 32 x 16, periodic in x, natural on the sides of y: singular
            A = PT.diffusion((32, 16), 1, 0)
            b = PT.rhs(A.shape[0], True)
        _OPS[name] = frozen(A, b)
    return _OPS[name]


def poisson(amg, n, levels, dim, sm):
    kw = SM[sm]
    cp, ri, v = amg.laplacian(n, dim)
    return (amg.Multigrid.poisson(n, levels, dim=dim, **kw),
            amg.Multigrid(cp, ri, v, amg.rhs(n, dim), levels, **kw))


def poisson_tensor(amg, n, levels, sm):
    return (amg.Multigrid.poisson_tensor(n, levels, device_setup=True, **SM[sm]),
            amg.Multigrid.poisson_tensor(n, levels, device_setup=False, **SM[sm]))


def tensor_dev(amg, sm, layout):
    A, Ac, b = operator("box")
    kw = dict(SM[sm], layout=layout)
    return (amg.Multigrid.tensor_dev(*dev_arrays(A, b), (33, 20, 12), 3, **kw),
            amg.Multigrid.tensor(Ac.indptr, Ac.indices, Ac.data, b, (33, 20, 12), 3, **kw))


def semi_dev(amg, levels, **rule):
    A, Ac, b = operator("strip")
    return (amg.Multigrid.tensor_semi_dev(*dev_arrays(A, b), (64, 16), levels, **rule, **SM["jacobi"]),
            amg.Multigrid.tensor_semi(Ac.indptr, Ac.indices, Ac.data, b, (64, 16), levels, **rule, **SM["jacobi"]))


def periodic_dev(amg, switch, sm, **kw):
    A, Ac, b = operator("ring")
    kw = dict(SM[sm], natural_sides=12, singular=True, **kw)
    amg.set_periodic_device_setup(switch)
    try:
        return (amg.Multigrid.tensor_periodic_dev(*dev_arrays(A, b), (32, 16), 3, 1, **kw),
                amg.Multigrid.tensor_periodic(Ac.indptr, Ac.indices, Ac.data, b, (32, 16), 3, 1, **kw))
    finally:
        amg.set_periodic_device_setup(0)


AUTO, SELL = 0, 2
CASES = {
    "poisson-2d-256-jacobi": lambda amg: poisson(amg, 256, 6, 2, "jacobi"),
    "poisson-2d-256-cheb": lambda amg: poisson(amg, 256, 6, 2, "cheb"),
    "poisson-2d-256-line": lambda amg: poisson(amg, 256, 6, 2, "line"),
    "poisson-2d-256-spgs": lambda amg: poisson(amg, 256, 6, 2, "spgs"),
    "poisson-2d-257-spgs": lambda amg: poisson(amg, 257, 6, 2, "spgs"),
    "poisson-2d-256-mc": lambda amg: poisson(amg, 256, 6, 2, "mc"),
    "poisson-3d-33-jacobi": lambda amg: poisson(amg, 33, 4, 3, "jacobi"),
    "poisson_tensor-64-jacobi": lambda amg: poisson_tensor(amg, 64, 4, "jacobi"),
    "poisson_tensor-64-alt": lambda amg: poisson_tensor(amg, 64, 4, "alt"),
    "semi_dev-masks": lambda amg: semi_dev(amg, 4, axis_masks=(1, 1, 3)),
    "semi_dev-auto": lambda amg: semi_dev(amg, 6, theta=0.5, min_coarse=32),
    "periodic_dev-off-jacobi": lambda amg: periodic_dev(amg, 0, "jacobi"),
    "periodic_dev-on-jacobi": lambda amg: periodic_dev(amg, 1, "jacobi"),
    "periodic_dev-off-alt-cyclic": lambda amg: periodic_dev(amg, 0, "alt", cyclic_lines=True),
    "periodic_dev-on-alt-cyclic": lambda amg: periodic_dev(amg, 1, "alt", cyclic_lines=True),
}
for _sm in ("jacobi", "cheb", "line", "alt"):
    for _name, _layout in (("auto", AUTO), ("sell", SELL)):
        CASES[f"tensor_dev-{_sm}-{_name}"] = lambda amg, s=_sm, la=_layout: tensor_dev(amg, s, la)


def optional(get, levels):
    out = []
    for l in range(levels):
        try:
            out.append(get(l))
        except ValueError:  # the solver has no such thing (no grid, no line directions)
            out.append(None)
    return out


def describe(amg, mg):
    L = mg.n_levels
    try:
        sweep = mg.fine_sweep_info()[0]
    except (ValueError, amg.AmgHipError):
        sweep = None
    return dict(on_device=mg.setup_on_device, levels=L, dims=optional(mg.level_dims, L),
                layout=[mg.level_layout(l)[0] for l in range(L)],
                transfer=[mg.level_transfer_kind(l) for l in range(L - 1)], axes=optional(mg.level_axes, L - 1),
                dirs=optional(mg.line_directions, L), cyclic=optional(mg.line_cyclic, L), sweep=sweep)


# recorded from the library before its set-up code was reorganised
EXPECTED = {
    'periodic_dev-off-alt-cyclic': dict(
        on_device=0,
        levels=3,
        dims=[(32, 16, 1), (16, 8, 1), (8, 4, 1)],
        layout=[2, 2, 3],
        transfer=[2, 2],
        axes=[3, 3],
        dirs=[[1, 32], [1, 16], [1, 8]],
        cyclic=[1, 1, 1],
        sweep=None,
    ),
    'periodic_dev-off-jacobi': dict(
        on_device=0,
        levels=3,
        dims=[(32, 16, 1), (16, 8, 1), (8, 4, 1)],
        layout=[2, 2, 3],
        transfer=[2, 2],
        axes=[3, 3],
        dirs=[None, None, None],
        cyclic=[None, None, None],
        sweep='sell_kernel<1, true, false>',
    ),
    'periodic_dev-on-alt-cyclic': dict(
        on_device=1,
        levels=3,
        dims=[(32, 16, 1), (16, 8, 1), (8, 4, 1)],
        layout=[2, 2, 3],
        transfer=[2, 2],
        axes=[3, 3],
        dirs=[[1, 32], [1, 16], [1, 8]],
        cyclic=[1, 1, 1],
        sweep=None,
    ),
    'periodic_dev-on-jacobi': dict(
        on_device=1,
        levels=3,
        dims=[(32, 16, 1), (16, 8, 1), (8, 4, 1)],
        layout=[2, 2, 3],
        transfer=[2, 2],
        axes=[3, 3],
        dirs=[None, None, None],
        cyclic=[None, None, None],
        sweep='sell_kernel<1, true, false>',
    ),
    'poisson-2d-256-cheb': dict(
        on_device=1,
        levels=6,
        dims=[None, None, None, None, None, None],
        layout=[3, 3, 3, 3, 3, 3],
        transfer=[1, 1, 1, 1, 1],
        axes=[None, None, None, None, None],
        dirs=[None, None, None, None, None, None],
        cyclic=[None, None, None, None, None, None],
        sweep='dict_kernel<17, 1, 5, false, 2>',
    ),
    'poisson-2d-256-jacobi': dict(
        on_device=1,
        levels=6,
        dims=[None, None, None, None, None, None],
        layout=[3, 3, 3, 3, 3, 3],
        transfer=[1, 1, 1, 1, 1],
        axes=[None, None, None, None, None],
        dirs=[None, None, None, None, None, None],
        cyclic=[None, None, None, None, None, None],
        sweep='dict_kernel<1, 1, 5, false, 2>',
    ),
    'poisson-2d-256-line': dict(
        on_device=1,
        levels=6,
        dims=[None, None, None, None, None, None],
        layout=[3, 3, 3, 3, 3, 3],
        transfer=[1, 1, 1, 1, 1],
        axes=[None, None, None, None, None],
        dirs=[None, None, None, None, None, None],
        cyclic=[None, None, None, None, None, None],
        sweep=None,
    ),
    'poisson-2d-256-mc': dict(
        on_device=0,
        levels=6,
        dims=[None, None, None, None, None, None],
        layout=[3, 3, 3, 3, 3, 3],
        transfer=[1, 1, 1, 1, 1],
        axes=[None, None, None, None, None],
        dirs=[None, None, None, None, None, None],
        cyclic=[None, None, None, None, None, None],
        # level 0 (2 colours, half-bandwidth 256) runs as a K-Strip level; until fine_sweep_info knew that
        # form it named the colour kernel, which this solver never launches on level 0
        sweep='mc_strip_kernel<1, 5, false, true>',
    ),
    'poisson-2d-256-spgs': dict(
        on_device=0,
        levels=6,
        dims=[None, None, None, None, None, None],
        layout=[3, 3, 3, 3, 3, 3],
        transfer=[1, 1, 1, 1, 1],
        axes=[None, None, None, None, None],
        dirs=[None, None, None, None, None, None],
        cyclic=[None, None, None, None, None, None],
        sweep='dict_kernel<1, 1, 5, false, 2>',
    ),
    'poisson-2d-257-spgs': dict(
        on_device=1,
        levels=6,
        dims=[None, None, None, None, None, None],
        layout=[3, 3, 3, 3, 3, 3],
        transfer=[1, 1, 1, 1, 1],
        axes=[None, None, None, None, None],
        dirs=[None, None, None, None, None, None],
        cyclic=[None, None, None, None, None, None],
        sweep='dict_kernel<1, 1, 5, false, 2>',
    ),
    'poisson-3d-33-jacobi': dict(
        on_device=1,
        levels=4,
        dims=[None, None, None, None],
        layout=[3, 3, 3, 3],
        transfer=[1, 1, 1],
        axes=[None, None, None],
        dirs=[None, None, None, None],
        cyclic=[None, None, None, None],
        sweep='dict_kernel<1, 1, 7, false, 2>',
    ),
    'poisson_tensor-64-alt': dict(
        on_device=0,
        levels=4,
        dims=[(64, 64, 1), (32, 32, 1), (16, 16, 1), (8, 8, 1)],
        layout=[3, 3, 3, 3],
        transfer=[2, 2, 2],
        axes=[3, 3, 3],
        dirs=[[1, 64], [1, 32], [1, 16], [1, 8]],
        cyclic=[0, 0, 0, 0],
        sweep=None,
    ),
    'poisson_tensor-64-jacobi': dict(
        on_device=1,
        levels=4,
        dims=[(64, 64, 1), (32, 32, 1), (16, 16, 1), (8, 8, 1)],
        layout=[3, 3, 3, 3],
        transfer=[2, 2, 2],
        axes=[3, 3, 3],
        dirs=[None, None, None, None],
        cyclic=[None, None, None, None],
        sweep='dict_kernel<1, 1, 5, false, 2>',
    ),
    'semi_dev-auto': dict(
        on_device=1,
        levels=5,
        dims=[(64, 16, 1), (32, 16, 1), (16, 16, 1), (8, 16, 1), (4, 8, 1)],
        layout=[3, 3, 3, 3, 3],
        transfer=[2, 2, 2, 2],
        axes=[1, 1, 1, 3],
        dirs=[None, None, None, None, None],
        cyclic=[None, None, None, None, None],
        sweep='dict_kernel<1, 1, 5, false, 1>',
    ),
    'semi_dev-masks': dict(
        on_device=1,
        levels=4,
        dims=[(64, 16, 1), (32, 16, 1), (16, 16, 1), (8, 8, 1)],
        layout=[3, 3, 3, 3],
        transfer=[2, 2, 2],
        axes=[1, 1, 3],
        dirs=[None, None, None, None],
        cyclic=[None, None, None, None],
        sweep='dict_kernel<1, 1, 5, false, 1>',
    ),
    'tensor_dev-alt-auto': dict(
        on_device=1,
        levels=3,
        dims=[(33, 20, 12), (16, 10, 6), (8, 5, 3)],
        layout=[2, 2, 2],
        transfer=[2, 2],
        axes=[7, 7],
        dirs=[[1, 33, 660], [1, 16, 160], [1, 8, 40]],
        cyclic=[0, 0, 0],
        sweep=None,
    ),
    'tensor_dev-alt-sell': dict(
        on_device=1,
        levels=3,
        dims=[(33, 20, 12), (16, 10, 6), (8, 5, 3)],
        layout=[2, 2, 2],
        transfer=[2, 2],
        axes=[7, 7],
        dirs=[[1, 33, 660], [1, 16, 160], [1, 8, 40]],
        cyclic=[0, 0, 0],
        sweep=None,
    ),
    'tensor_dev-cheb-auto': dict(
        on_device=1,
        levels=3,
        dims=[(33, 20, 12), (16, 10, 6), (8, 5, 3)],
        layout=[2, 2, 2],
        transfer=[2, 2],
        axes=[7, 7],
        dirs=[None, None, None],
        cyclic=[None, None, None],
        sweep='sell_kernel<17, true, false>',
    ),
    'tensor_dev-cheb-sell': dict(
        on_device=1,
        levels=3,
        dims=[(33, 20, 12), (16, 10, 6), (8, 5, 3)],
        layout=[2, 2, 2],
        transfer=[2, 2],
        axes=[7, 7],
        dirs=[None, None, None],
        cyclic=[None, None, None],
        sweep='sell_kernel<17, true, false>',
    ),
    'tensor_dev-jacobi-auto': dict(
        on_device=1,
        levels=3,
        dims=[(33, 20, 12), (16, 10, 6), (8, 5, 3)],
        layout=[2, 2, 2],
        transfer=[2, 2],
        axes=[7, 7],
        dirs=[None, None, None],
        cyclic=[None, None, None],
        sweep='sell_kernel<1, true, false>',
    ),
    'tensor_dev-jacobi-sell': dict(
        on_device=1,
        levels=3,
        dims=[(33, 20, 12), (16, 10, 6), (8, 5, 3)],
        layout=[2, 2, 2],
        transfer=[2, 2],
        axes=[7, 7],
        dirs=[None, None, None],
        cyclic=[None, None, None],
        sweep='sell_kernel<1, true, false>',
    ),
    'tensor_dev-line-auto': dict(
        on_device=1,
        levels=3,
        dims=[(33, 20, 12), (16, 10, 6), (8, 5, 3)],
        layout=[2, 2, 2],
        transfer=[2, 2],
        axes=[7, 7],
        dirs=[None, None, None],
        cyclic=[None, None, None],
        sweep=None,
    ),
    'tensor_dev-line-sell': dict(
        on_device=1,
        levels=3,
        dims=[(33, 20, 12), (16, 10, 6), (8, 5, 3)],
        layout=[2, 2, 2],
        transfer=[2, 2],
        axes=[7, 7],
        dirs=[None, None, None],
        cyclic=[None, None, None],
        sweep=None,
    ),
}


def test_every_case_has_its_literal():
    assert sorted(EXPECTED) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_path_and_cycle(amg, name):
    mg, twin = CASES[name](amg)
    try:
        got = describe(amg, mg)
        print(f"\n{name}: {got}")
        assert got == EXPECTED[name]
        assert twin.setup_on_device == 0 and twin.n_levels == mg.n_levels
        mg.vcycle(1)
        twin.vcycle(1)
        mg.sync()
        twin.sync()
        u, ref = mg.get_soln(0), twin.get_soln(0)
        assert np.all(np.isfinite(ref)) and np.linalg.norm(ref) > 0
        assert np.array_equal(u.view(np.uint64), ref.view(np.uint64))
    finally:
        mg.close()
        twin.close()
