"""TEST INFRASTRUCTURE: solver.cpp's pcg_run (amg_hip_pcg, amg_hip_pcg_mixed; per column amg_hip_block_pcg)
restated step for step in numpy float64, meant to give the device's BITS.

  the dot products     tests/reduce_twin.py: the device's two-stage tree, not a sequential sum
  r = b - A x, q = A p the oracle's residual and spmv: one row in ascending column order (CSR_RESID starts
                       from b_i and subtracts entry by entry, CSR_SPMV sums from zero)
  the updates          x = x + alpha p, r = r - alpha q, p = z + beta p: one multiply, then one add, per entry
                       (the library is built without FMA contraction)
  alpha, beta          rz / pq and rz_new / rz: IEEE float64 divides (pcg_update_*_kernel forms them on the device)
  the stopping rule    relres = sqrt(r.r) / sqrt(b.b), sqrt(r.r) when b.b is zero; leave before the first
                       iteration when relres <= rtol or max_iters == 0, after one when !(relres > rtol) -- NaN
                       leaves too -- or the count is reached
  z = M^-1 r           the callback `apply`: the oracle's V-cycle from zero, or the float32 twin's cycle

Nothing here reads the library and the product never imports this module."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import reduce_twin as RT  # noqa: E402


def _relres(rr, bnorm):
    with np.errstate(all="ignore"):
        root = float(np.sqrt(np.float64(rr)))       # NaN for a negative or NaN argument, as std::sqrt
    return root / bnorm if bnorm > 0 else root


def first_residual(A, b, x0):
    from oracle import oracle as O
    return O.residual(A, np.ascontiguousarray(x0, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64))


def pcg(A, b, x0, apply, rtol, max_iters, keep_iterates=False):
    """A: oracle.CSC of the level-0 matrix.  Returns (x, iters, relres, trace); trace has one entry per
    iteration: (alpha, beta, relres) -- beta is the one formed after that iteration, None when the loop was
    left before it -- and, with keep_iterates, a fourth member: a copy of x after that iteration."""
    from oracle import oracle as O
    b = np.ascontiguousarray(b, dtype=np.float64)
    x = np.array(x0, dtype=np.float64)
    bnorm = math.sqrt(RT.dot(b, b))
    r = O.residual(A, x, b)
    rel = _relres(RT.dot(r, r), bnorm)
    trace = []
    it = 0
    if rel <= rtol or max_iters == 0:
        return x, it, rel, trace
    z = np.asarray(apply(r), dtype=np.float64)
    p = z.copy()
    rz = np.float64(RT.dot(r, z))
    with np.errstate(all="ignore"):
        while it < max_iters:
            q = O.spmv(A, p)
            pq = np.float64(RT.dot(p, q))
            alpha = np.divide(rz, pq)
            x = np.add(x, np.multiply(alpha, p))
            r = np.subtract(r, np.multiply(alpha, q))
            it += 1
            rel = _relres(RT.dot(r, r), bnorm)
            entry = [float(alpha), None, rel] + ([x.copy()] if keep_iterates else [])
            trace.append(entry)
            if not (rel > rtol) or it >= max_iters:
                break
            z = np.asarray(apply(r), dtype=np.float64)
            rzn = np.float64(RT.dot(r, z))
            beta = np.divide(rzn, rz)
            p = np.add(z, np.multiply(beta, p))
            rz = rzn
            entry[1] = float(beta)
    return x, it, rel, [tuple(e) for e in trace]
