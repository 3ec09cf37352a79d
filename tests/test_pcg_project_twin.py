"""tests/pcg_project_twin.py on the CPU, M^-1 = the V-cycle of tests/natural_twin.py's NaturalTwin on pure-Neumann
variable-coefficient diffusion (all sides natural, singular, true Jacobi omega 0.8 2+2), rtol 1e-8, cap 60, from
x = 0, on 64 x 48 / 4 levels, 33 x 20 / 3 and 17 x 12 x 9 / 3:

  project = False   is pcg_twin.pcg, result for result
  projected         b, b + 1e-6 and b + 1e-3 take the iteration count of the unprojected run on the consistent b
                    (taken from that run) and end with relres <= 1e-8; the result has zero mean up to the
                    rounding of the tree sum and the subtract; the caller's b is not written
  unprojected       b + 1e-6 has not converged at the cap and the iterate has run away along the constants:
                    what the switch is for

The bound on the mean: with x the uncentred iterate, S its tree sum and m = fl(S / n), the returned entries are
fl(x_i - m).  Their exact sum is (sum x_i - S) + (S - n m) + the subtracts' roundings: at most
RT.bound(n) sum|x_i| for the tree (reduce_twin.bound), n |m| U <= (1 + U) U sum|x_i| for the divide, and
U sum|x_i - m| <= 2 U (1 + U) sum|x_i| for the subtracts; 4 U covers the last two."""
import math
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import natural_twin as N  # noqa: E402
import pcg_project_twin as PP  # noqa: E402
import pcg_twin as PT  # noqa: E402
import reduce_twin as RT  # noqa: E402

CASES = [((64, 48), 4), ((33, 20), 3), ((17, 12, 9), 3)]
RTOL, CAP = 1e-8, 60

_SETUPS = {}


def setup(oracle, dims, nl):
    """(oracle.CSC of A, b, apply, unprojected run on b): made once per case and never modified"""
    if dims not in _SETUPS:
        A = N.diffusion(dims, 0)
        n = A.shape[0]
        b = N.rhs(n, 0)
        b.setflags(write=False)
        tw = N.NaturalTwin(A, dims, nl, sides=N.all_sides(len(dims)), singular=True, omega=0.8, iters=2)
        Ac = sp.csc_matrix(A)
        Ac.sort_indices()
        Ao = oracle.CSC(n, n, Ac.indptr.astype(np.int32), Ac.indices.astype(np.int32), Ac.data.copy())

        def apply(v):
            return tw.vcycle(np.zeros(n), v)[0][0]

        plain = PT.pcg(Ao, b, np.zeros(n), apply, RTOL, CAP)
        _SETUPS[dims] = (Ao, b, apply, plain)
    return _SETUPS[dims]


def same_run(a, b):
    if not (np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2] and len(a[3]) == len(b[3])):
        return False
    return all(len(s) == len(t) and s[:3] == t[:3] and all(np.array_equal(u, v) for u, v in zip(s[3:], t[3:]))
               for s, t in zip(a[3], b[3]))


@pytest.mark.parametrize("dims,nl", CASES)
def test_without_projection_it_is_pcg_twin(oracle, dims, nl):
    A, b, apply, plain = setup(oracle, dims, nl)
    n = b.size
    assert same_run(PP.pcg(A, b, np.zeros(n), apply, RTOL, CAP, project=False), plain)
    x0 = 1e-3 * np.random.default_rng(4).standard_normal(n)
    for k in (0, 3):
        assert same_run(PP.pcg(A, b, x0, apply, 0.0, k, project=False, keep_iterates=True),
                        PT.pcg(A, b, x0, apply, 0.0, k, keep_iterates=True))


@pytest.mark.parametrize("shift", [0.0, 1e-6, 1e-3])
@pytest.mark.parametrize("dims,nl", CASES)
def test_projected_run_takes_the_consistent_count(oracle, dims, nl, shift):
    A, b, apply, plain = setup(oracle, dims, nl)
    n = b.size
    assert 2 <= plain[1] < CAP and plain[2] <= RTOL
    bs = b + shift
    keep = bs.copy()
    x, it, rel, trace = PP.pcg(A, bs, np.zeros(n), apply, RTOL, CAP, project=True, keep_iterates=True)
    raw = trace[-1][4]
    total, mass = math.fsum(x), math.fsum(np.abs(raw))
    print(f"\n{dims}/{nl} b + {shift:g}: {it} iterations (consistent, unprojected: {plain[1]}), relres {rel:.3e}; "
          f"|sum x| {abs(total):.3e}, bound {(RT.bound(n) + 4 * RT.U) * mass:.3e}, mean of the uncentred x "
          f"{math.fsum(raw) / n:.3e}")
    assert it == plain[1], (it, plain[1])
    assert rel <= RTOL
    assert np.array_equal(x, trace[-1][3]) and np.array_equal(x, PP.centre(raw))
    assert abs(total) <= (RT.bound(n) + 4 * RT.U) * mass
    assert np.array_equal(bs, keep)


@pytest.mark.parametrize("dims,nl", CASES)
def test_unprojected_run_on_an_inconsistent_b_runs_away(oracle, dims, nl):
    A, b, apply, _ = setup(oracle, dims, nl)
    x, it, rel, _ = PT.pcg(A, b + 1e-6, np.zeros(b.size), apply, RTOL, CAP)
    print(f"\n{dims}/{nl} b + 1e-6 unprojected: {it} iterations, relres {rel:.3e}, max|x| {np.abs(x).max():.3e}")
    assert it == CAP and not rel <= RTOL
    assert np.abs(x).max() > 1e6


def test_early_exits_return_the_centred_start(oracle):
    dims, nl = CASES[1]
    A, b, apply, _ = setup(oracle, dims, nl)
    x0 = 1.0 + 1e-3 * np.random.default_rng(4).standard_normal(b.size)
    x, it, rel, trace = PP.pcg(A, b, x0, apply, RTOL, 0, project=True)
    assert it == 0 and trace == [] and np.array_equal(x, PP.centre(x0)) and rel > RTOL
    zero = np.zeros(b.size)
    x, it, rel, _ = PP.pcg(A, zero, zero, apply, RTOL, 50, project=True)
    assert it == 0 and rel == 0.0 and not x.any()
