"""TEST INFRASTRUCTURE: tests/pcg_twin.py restated with the mean projection of the PCG drivers
(amg_hip_set_mean_projection; solver.cpp: pcg_run and amg_hip_block_pcg with project_mean, K-Center in
kernels.hip), meant to give the device's BITS.

  centre(v)            v - S / n: S = reduce_twin.sum(v), the device's two-stage tree (launch_sum, square = 0);
                       one IEEE float64 divide of S by float64(n); one subtract per entry
  project = True       1. b~ = centre(b); bnorm = sqrt(b~ . b~); r = b~ - A x0 (the caller's b is left alone)
                       2. after every preconditioner call z = centre(z), then r . z (r is not centred again;
                          the device forms both in one pass, the term being r[i] * (z[i] - m))
                       3. the stopping rule of pcg_twin with that bnorm
                       4. x = centre(x) on every way out, the early ones included
  project = False      pcg_twin.pcg, statement for statement

Everything else -- the dot products, r = b - A x and q = A p through the oracle, the updates, alpha and beta --
is pcg_twin's.  Nothing here reads the library and the product never imports this module."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import reduce_twin as RT  # noqa: E402
from pcg_twin import _relres  # noqa: E402


def centre(v):
    v = np.ascontiguousarray(v, dtype=np.float64)
    return np.subtract(v, np.divide(np.float64(RT.sum(v)), np.float64(v.size)))


def pcg(A, b, x0, apply, rtol, max_iters, project=False, keep_iterates=False):
    """pcg_twin.pcg's arguments and results.  With project and keep_iterates the trace keeps the iterate the
    device would RETURN after that iteration, centre(x), and a fifth member: the uncentred x."""
    from oracle import oracle as O
    b = np.ascontiguousarray(b, dtype=np.float64)
    x = np.array(x0, dtype=np.float64)
    bt = centre(b) if project else b
    bnorm = math.sqrt(RT.dot(bt, bt))
    r = O.residual(A, x, bt)
    rel = _relres(RT.dot(r, r), bnorm)
    trace = []
    it = 0

    def out(v):
        return centre(v) if project else v

    def precond(v):
        z = np.asarray(apply(v), dtype=np.float64)
        return centre(z) if project else z

    if rel <= rtol or max_iters == 0:
        return out(x), it, rel, trace
    z = precond(r)
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
            entry = [float(alpha), None, rel] + ([out(x).copy()] + ([x.copy()] if project else []) if keep_iterates else [])
            trace.append(entry)
            if not (rel > rtol) or it >= max_iters:
                break
            z = precond(r)
            rzn = np.float64(RT.dot(r, z))
            beta = np.divide(rzn, rz)
            p = np.add(z, np.multiply(beta, p))
            rz = rzn
            entry[1] = float(beta)
    return out(x), it, rel, [tuple(e) for e in trace]
