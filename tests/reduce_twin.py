"""TEST INFRASTRUCTURE: the summation ORDER of the device's reductions (kernels.hip: K-SumSq sum_kernel,
K-PCG dot_kernel, block_sum_kernel<KP>; launch_sum / launch_dot / launch_block_sum) restated in numpy
float64, meant to give the device's BITS.

Why that is possible: the library is built without FMA contraction, so a term x[i] * y[i] is one rounded
multiply before any add, and the reduction is a fixed two-stage tree with no atomics:

  grid       g = min(max(ceil(n / 256), 1), 1024) workgroups of 256 threads, G = 256 g threads
  thread     thread t starts from +0.0 and adds term[i] for i = t, t + G, t + 2G, ... in that order
  wave       each 64-lane wave runs v[l] += v[l + off] for off = 32, 16, 8, 4, 2, 1 on ALL 64 lanes at once
             (__shfl_down: a lane whose source lies outside the wave reads itself); lane 0 holds the sum
  workgroup  ((w0 + w1) + w2) + w3 over its four waves: one partial per workgroup
  stage two  the same kernel with ONE workgroup over the g partials (n = g, no squaring)
  block      the same per column of a row-major n x kp panel; the second stage on the g x kp partials

Every arithmetic step below is one elementwise float64 ufunc on whole arrays (no sum, no dot, no `@`).
Nothing here reads the library and the product never imports this module."""
import numpy as np

WG = 256          # threads of a workgroup
WAVE = 64         # lanes of a wave
MAX_GROUPS = 1024  # the cap on the first stage's grid: the scratch holds 1024 partials (x kp)
U = 2.0 ** -53    # unit roundoff of float64


def _f(a):
    assert isinstance(a, np.ndarray) and a.dtype == np.float64, getattr(a, "dtype", type(a))
    return a


def grid(n):
    """(g, G): workgroups and threads of the first stage over n terms"""
    g = min(max(-(-int(n) // WG), 1), MAX_GROUPS)
    return g, WG * g


def depth(n):
    """additions on the longest path of the tree over n terms: the thread's own, six shuffle steps and
    three wave combines, and the same again in the second stage over the g partials"""
    g, G = grid(n)
    return -(-int(n) // G) + 9 + -(-g // WG) + 9


def bound(n):
    """relative distance of the tree's sum of n terms of one sign from math.fsum of the same terms
    (itself correctly rounded: the + 1): the standard bound gamma_{d + 1}"""
    k = depth(n) + 1
    return k * U / (1.0 - k * U)


_LANES = np.arange(WAVE)
_SRC = {off: np.where(_LANES + off < WAVE, _LANES + off, _LANES) for off in (32, 16, 8, 4, 2, 1)}


def _stage(t, g):
    """One launch of g workgroups over the terms t (n, or n x kp): the g (x kp) partials."""
    _f(t)
    n, tail = t.shape[0], t.shape[1:]
    G = WG * g
    acc = np.zeros((G,) + tail, np.float64)
    for s in range(0, n, G):                      # the grid-stride loop, one pass per iteration
        c = t[s:s + G]
        acc[:c.shape[0]] = np.add(acc[:c.shape[0]], c)
    v = acc.reshape((G // WAVE, WAVE) + tail)     # waves x lanes
    for off in (32, 16, 8, 4, 2, 1):              # wave_sum on every lane
        v = np.add(v, v[:, _SRC[off]])
    w = v[:, 0].reshape((g, WG // WAVE) + tail)   # lane 0 of the four waves of each workgroup
    return _f(np.add(np.add(np.add(w[:, 0], w[:, 1]), w[:, 2]), w[:, 3]))


def _reduce(t):
    t = _f(np.ascontiguousarray(t))
    g, _ = grid(t.shape[0])
    return _stage(_stage(t, g), 1)[0]


def _vec(x):
    x = np.asarray(x)
    assert x.dtype == np.float64 and x.ndim == 1, (x.dtype, x.shape)
    return x


def sum(x):  # noqa: A001  (the name the kernel has)
    """launch_sum(square = 0): sum of x[i]"""
    return float(_reduce(_vec(x)))


def sumsq(x):
    """launch_sum(square = 1): sum of x[i] * x[i]"""
    x = _vec(x)
    return float(_reduce(np.multiply(x, x)))


def dot(x, y):
    """launch_dot: sum of x[i] * y[i]"""
    x, y = _vec(x), _vec(y)
    assert x.shape == y.shape
    return float(_reduce(np.multiply(x, y)))


def block(X, Y=None):
    """launch_block_sum on row-major panels: out[j] = sum of X[i, j] (Y None) or of X[i, j] * Y[i, j]"""
    X = np.asarray(X)
    assert X.dtype == np.float64 and X.ndim == 2, (X.dtype, X.shape)
    if Y is None:
        return _reduce(X)
    Y = np.asarray(Y)
    assert Y.dtype == np.float64 and Y.shape == X.shape
    return _reduce(np.multiply(X, Y))


def rss(r):
    """amg_hip_rss's second half: the plain sum over d[i] * d[i], the squares formed by the row kernel
    (CSR_RSSQ) and summed by launch_sum(square = 0).  r: the vector of differences d."""
    r = _vec(r)
    return float(_reduce(np.multiply(r, r)))
