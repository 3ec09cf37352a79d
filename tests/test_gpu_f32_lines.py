"""The line smoothers in the single-precision cycle on the device (amg_hip_set_f32_lines; kernels.hip: the
K-LineX, K-Line and K-LineSeam solve kernels instantiated on float) against tests/f32_line_twin.py.

  1  K-LineX walks a line in the twin's order, so one x sub-sweep (amg_hip_f32_line_subsweep) with the
     device's own float factors (amg_hip_f32_line_factors) has the twin's bits in u and in the float r
     (which holds the forward values afterwards).  The device's factors are the double ones rounded: they
     may differ from float32(the twin's float64 factors) by one float ulp where the two double
     eliminations differ in the last bit.
  2  K-Line (segments and a Schur complement on the separators) takes another order than the sequential
     walk.  With e32 the distance of the float32 twin from the longdouble one, the device must lie within
     max(8 e32, 1e-6 ||u||) of the longdouble result: line_twin.within's factor 8, its floor 1e-14 scaled
     to float epsilon.
  3  amg_hip_apply_f32 within 8 e32 of the longdouble cycle; captured and eager, first and replayed call
     leave the same bits in u, f and r of every level.
  4  cyclic lines (opts->cyclic_lines) on a periodic axis.
  5  amg_hip_pcg_mixed takes the twin's float32 count +- 1 and ends with a true fp64 residual <= rtol.
  6  the double entry points keep their bits, and with the switch off the refusal stays.
  7  amg_hip_f32_must_move is the formula.
The shapes are the smallest that cross each period of the kernels (chunks of 64 columns, 8 runs to a wave,
segments of 32 rows, batches of 8 separators, LDS chunks of 1024 separators).  Every test prints the
figures it found.  The switch is process-wide: the module's fixture turns it off again after every test.

Found on an MI355X: no device factor differs from float32(the twin's float64 factors) on any shape of 1;
largest distance / e32 of a K-Line sub-sweep 1.02 ((7, 1000), (64, 290), (2, 40000)), with cyclic lines
1.31; applications 0.76 .. 1.00 e32 (cyclic lines 1.19); amg_hip_pcg_mixed takes the twin's float32 count
on every case of 5.  The split64 case of 3 is also what showed that a memset node in the captured float
graph can fill with stale bytes on a replay that follows device-to-host copies: the cycle now writes
its zero guess with a kernel."""
import os
import sys

import numpy as np
import pytest

sp = pytest.importorskip("scipy.sparse")
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import f32_line_twin as LT  # noqa: E402
import f32_twin as FT  # noqa: E402
import line_alt_twin as AT  # noqa: E402
import line_cyclic_twin as CT  # noqa: E402
import line_twin as T  # noqa: E402
import mixed_twin as MT  # noqa: E402
import periodic_twin as PT  # noqa: E402

pytestmark = pytest.mark.gpu
SELL = 2
OMEGA = 0.8
ALT = dict(smoother=7, smoother_iters=1, omega=OMEGA, layout=SELL)
F = np.float32
LD = np.longdouble


@pytest.fixture(autouse=True)
def lines_on(amg):
    amg.set_f32_lines(1)
    yield
    amg.set_f32_lines(0)


def _csr(A):
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy()


def _csc(A):
    A = sp.csc_matrix(A)
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy()


def tensor_dev(amg, A, b, dims, levels, **kw):
    mg = amg.Multigrid.tensor_dev(*_csr(A), np.array(b, np.float64), dims, levels, **dict(ALT, **kw))
    assert mg.setup_on_device == 1
    return mg


def dims3(dims):
    return tuple(dims) + (1,) * (3 - len(dims))


def level_matrix(mg, l):
    n = mg.get_n_dofs(l)
    return T.csr_of(*mg.get_coefficient_matrix(l), n, n)


def rnd(rng, n):
    """random float32 without zeros"""
    v = rng.standard_normal(n).astype(F)
    v[v == 0] = F(1)
    return v


def bits_equal(got, want, what):
    assert got.dtype == F and want.dtype == F and np.all(np.isfinite(want)), what
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (f"{what}: {bad.size} of {got.size} entries differ, first at {int(bad[0])}: "
                           f"device {got[bad[0]]!r} twin {want[bad[0]]!r}")


def check(got, ref, e32, scale, what):
    ok, dist, bound, ratio = LT.within(got, ref, e32, scale)
    print(f"  {what}: distance {dist:.3e}, e32 {e32:.3e}, ratio {ratio:.2f}, bound {bound:.3e}")
    assert ok, (what, dist, bound, ratio)
    return ratio


def subsweep(mg, l, d, u, f, reverse=False):
    mg.f32_set_vec(l, "u", u)
    mg.f32_set_vec(l, "f", f)
    mg.f32_line_subsweep(l, d, reverse)
    return mg.f32_get_vec(l, "u")


# ---- 1. K-LineX bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(nx, 9) for nx in (2, 3, 31, 32, 33, 63, 64, 65, 129)] + [(7, 1000), (4097, 3)])
def test_linex_subsweep_has_the_twins_bits(amg, dims):
    """nx below, at and above the merging of short lines into one run and the chunk of 64 columns; nine
    runs (the ninth goes to a second wave); 1000 short lines; 65 chunks with a last one of one column."""
    A = MT.diffusion(dims, seed=2)
    mg = tensor_dev(amg, A, np.ones(A.shape[0]), dims, 2)
    try:
        L = LT.Level(A, "alt", dims3(dims))
        assert L.x_direction and L.dirs[0].s == 1
        dev = mg.f32_line_factors(0)
        want = L.dirs[0].factors32()
        worst, differ = 0, 0
        for g, w, name in zip(dev, want, ("dl", "ip", "cp")):
            ulp = np.abs(g.view(np.int32).astype(np.int64) - w.view(np.int32).astype(np.int64))
            differ += int(np.count_nonzero(ulp))
            worst = max(worst, int(ulp.max()))
            assert np.all(np.signbit(g) == np.signbit(w)), name
        rng = np.random.default_rng(dims[0])
        u, f = rnd(rng, L.n), rnd(rng, L.n)
        got_u = subsweep(mg, 0, 0, u, f)
        got_r = mg.f32_get_vec(0, "r")
        want_u, want_r = L.sub32(0, u, f, OMEGA, factors=dev)
        print(f"\n{dims}: {differ} of {3 * L.n} device factors differ from float32(twin float64 factors), "
              f"at most {worst} ulp")
        assert worst <= 1
        assert not FT.same_bits(want_u, u)
        bits_equal(got_u, want_u, (dims, "u"))
        bits_equal(got_r, want_r, (dims, "r: the forward values"))
        bits_equal(mg.f32_get_vec(0, "f"), f, (dims, "f unchanged"))
    finally:
        mg.close()


# ---- 2. K-Line in float ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(7, 1000), (64, 290), (65, 33), (2, 40000), (5, 2, 4), (17, 12, 9), (2, 2)])
def test_kline_subsweeps_within_the_reference_bound(amg, dims):
    """(7, 1000): few long chains, 31 separators; (64, 290): many chains, past one batch of 8 separators;
    (65, 33): a segment end; (2, 40000): two chains of 1250 separators, the second LDS chunk of
    line_sep_few_kernel; 3-D: y and z; (2, 2): its second level has one row (weighted Jacobi through
    K-Line), which is always the coarsest level.  Every direction of every level, both legs."""
    A = MT.diffusion(dims, seed=2)
    mg = tensor_dev(amg, A, np.ones(A.shape[0]), dims, 2)
    worst = 0.0
    try:
        print()
        for l in range(mg.n_levels):
            d3 = tuple(mg.level_dims(l))
            L = LT.Level(level_matrix(mg, l), "alt", d3)
            assert [D.s for D in L.dirs if not D.flat] == mg.line_directions(l)
            if dims == (2, 2) and l == 1:
                assert L.n == 1 and L.dirs[0].flat
            rng = np.random.default_rng(l + sum(dims))
            u, f = rnd(rng, L.n), rnd(rng, L.n)
            for d in range(len(L.dirs)):
                ref, e32 = LT.sub_bound(L, d, u, f, OMEGA)
                for rev in (False, True):
                    got = subsweep(mg, l, d, u, f, rev)
                    worst = max(worst, check(got, ref, e32, np.linalg.norm(got),
                                             f"{dims} level {l} {d3} direction {d} reverse {int(rev)}"))
        print(f"  {dims}: largest ratio {worst:.2f}")
    finally:
        mg.close()


# ---- 3. whole applications ------------------------------------------------------------------------------
def _mixed33(amg, oracle, **kw):
    dims, levels, A, b, _ = MT.operator("33x20")
    return tensor_dev(amg, A, b, dims, levels, **kw), A, b


def _split64(amg, oracle, **kw):
    A = AT.split_anisotropy(64, 48, 1e-3)
    b = np.random.default_rng(99).standard_normal(A.shape[0])
    return tensor_dev(amg, A, b, (64, 48), 4, **kw), A, b


def _box(iters):
    def make(amg, oracle, **kw):
        dims, levels, A, b, _ = MT.operator("17x12x9")
        return tensor_dev(amg, A, b, dims, levels, smoother_iters=iters, **kw), A, b
    return make


def _lap63(amg, oracle, **kw):
    Ao = oracle.laplacian(63)
    b = np.random.default_rng(99).standard_normal(63 * 63)
    mg = amg.Multigrid(Ao.colptr, Ao.rowind, Ao.val, b, 4, smoother=amg.SM_LINE_JACOBI, smoother_iters=1, omega=0.7,
                       layout=SELL, **kw)
    return mg, T.csr_of(Ao.colptr, Ao.rowind, Ao.val, b.size, b.size), b


CASES = {"mixed33": (_mixed33, "alt", OMEGA, 1), "split64": (_split64, "alt", OMEGA, 1), "box-it1": (_box(1), "alt", OMEGA, 1),
         "box-it2": (_box(2), "alt", OMEGA, 2), "lap63": (_lap63, "jacobi", 0.7, 1)}
_CYC = {}


def cycle_of(mg, case):
    """f32_line_twin.Cycle on the solver's own hierarchy (its getters), once per case"""
    if case not in _CYC:
        _, kind, omega, iters = CASES[case]
        src = AT.Twin(mg, omega, iters) if kind == "alt" else T.Twin(mg, omega, iters)
        _CYC[case] = LT.Cycle(src, kind, omega, iters)
    return _CYC[case]


def _apply(mg, v):
    dv = torch.from_numpy(np.array(v)).cuda()
    dz = torch.empty_like(dv)
    mg.apply_f32(dv.data_ptr(), dz.data_ptr())
    mg.sync()
    return dz.cpu().numpy()


def _state(mg):
    nl = mg.n_levels
    return [mg.f32_get_vec(l, w) for l in range(nl) for w in ("u", "f", "r") if not (w == "r" and l == nl - 1)]


@pytest.mark.parametrize("case", sorted(CASES))
def test_apply_f32_within_the_bound_and_the_same_bits_on_every_path(amg, oracle, case):
    states = []
    print()
    for graph in (True, False):
        mg, A, b = CASES[case][0](amg, oracle, use_graph=graph)
        try:
            cyc = cycle_of(mg, case)
            v = np.random.default_rng(7).standard_normal(cyc.n[0])
            ref, e32, _ = cyc.apply_bound(v)
            for call in ("first", "replayed"):
                z = _apply(mg, v)
                states.append(_state(mg))
                dist = float(np.linalg.norm(z.astype(LD) - ref))
                print(f"  {case} {'graph' if graph else 'eager'} {call}: distance {dist:.3e}, e32 {e32:.3e}, "
                      f"ratio {dist / e32:.2f}; ||z|| {np.linalg.norm(z):.3e}; norms of u f r per level "
                      + " ".join(f"{np.linalg.norm(a.astype(np.float64)):.3e}" for a in states[-1]))
                assert dist <= 8.0 * e32
                assert np.array_equal(z, states[-1][0].astype(np.float64))
        finally:
            mg.close()
    for st in states[1:]:
        assert len(st) == len(states[0])
        for a, b0 in zip(st, states[0]):
            bits_equal(a, b0, (case, "graph / eager, first / replayed"))


# ---- 4. cyclic lines ------------------------------------------------------------------------------------
def test_cyclic_lines(amg):
    """64 x 48, x periodic and 100 times stronger, 4 levels, cyclic_lines = 1"""
    dims, nl = (64, 48), 4
    A = CT.scaled_diffusion(dims, (1.0, 1e-2), 1)
    b = np.random.default_rng(99).standard_normal(A.shape[0])
    mg = amg.Multigrid.tensor_periodic(*_csc(A), b, dims, nl, 1, cyclic_lines=1, **ALT)
    try:
        pt = PT.PeriodicTwin(A, dims, nl, periodic=1)
        cyc = LT.Cycle(pt, "alt", OMEGA, 1, periodic=1)
        print()
        for l in range(nl - 1):
            assert mg.line_cyclic(l) == 1 and cyc.lv[l].dirs[0].cyclic and not cyc.lv[l].dirs[1].cyclic
            rng = np.random.default_rng(40 + l)
            u, f = rnd(rng, cyc.n[l]), rnd(rng, cyc.n[l])
            for d in (0, 1):
                ref, e32 = LT.sub_bound(cyc.lv[l], d, u, f, OMEGA)
                got = subsweep(mg, l, d, u, f)
                check(got, ref, e32, np.linalg.norm(got), f"cyclic level {l} {cyc.dims[l]} direction {d}")
        v = np.random.default_rng(7).standard_normal(cyc.n[0])
        ref, e32, _ = cyc.apply_bound(v)
        z = _apply(mg, v)
        dist = float(np.linalg.norm(z.astype(LD) - ref))
        print(f"  application: distance {dist:.3e}, e32 {e32:.3e}, ratio {dist / e32:.2f}")
        assert dist <= 8.0 * e32
        zero = np.zeros(b.size)
        mg.set_vec(0, "u", zero)
        x, it, rel = mg.pcg(1e-8, 100)
        mg.set_vec(0, "u", zero)
        xm, itm, relm = mg.pcg_mixed(1e-8, 100)
        true = np.linalg.norm(b - A @ xm) / np.linalg.norm(b)
        print(f"  PCG to 1e-8: double cycle {it} iterations, float cycle {itm}, true residual {true:.2e}")
        assert abs(it - itm) <= 1 and rel <= 1e-8 and relm <= 1e-8
        assert true <= 1e-8
    finally:
        mg.close()


# ---- 5. PCG ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
def test_pcg_mixed_takes_the_twins_count(amg, oracle, case):
    mg, A, b = CASES[case][0](amg, oracle)
    try:
        cyc = cycle_of(mg, case)
        _, it_twin, _ = MT.pcg(cyc, b, 1e-8, np.float32)
        zero = np.zeros(b.size)
        said = []
        for rtol in (1e-8, 1e-12):
            mg.set_vec(0, "u", zero)
            x, it, rel = mg.pcg_mixed(rtol, 200)
            true = np.linalg.norm(b - A @ x) / np.linalg.norm(b)
            said.append(f"rtol {rtol:g}: {it} iterations, relres {rel:.2e}, true residual {true:.2e}")
            assert np.array_equal(x, mg.get_soln(0))
            assert rel <= rtol and it < 200
            if rtol == 1e-8:
                assert abs(it - it_twin) <= 1, (it, it_twin)
                assert true <= rtol
        print(f"\n{case}: twin float32 count {it_twin}; " + "; ".join(said))
    finally:
        mg.close()


# ---- 6. nothing else moves ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["split64", "lap63"])
def test_the_double_entry_points_keep_their_bits(amg, oracle, case):
    mg, A, b = CASES[case][0](amg, oracle)
    try:
        zero = np.zeros(b.size)

        def double_results():
            mg.set_vec(0, "u", zero)
            mg.vcycle(2)
            mg.sync()
            u = mg.get_soln(0)
            mg.set_vec(0, "u", zero)
            return u, mg.pcg(1e-8, 100)
        u0, p0 = double_results()
        z = _apply(mg, b)                      # makes the float copies
        assert np.linalg.norm(z) > 0
        mg.set_vec(0, "u", zero)
        mg.pcg_mixed(1e-8, 100)
        u1, p1 = double_results()
        assert np.array_equal(u0, u1) and np.array_equal(p0[0], p1[0]) and p0[1:] == p1[1:]
        assert np.array_equal(mg.get_rhs(0), b)
        amg.set_f32_lines(0)                   # off: today's refusal, also once the copies exist
        dv = torch.zeros(b.size, dtype=torch.float64, device="cuda")
        for call in (lambda: mg.apply_f32(dv.data_ptr(), dv.data_ptr()), lambda: mg.pcg_mixed(1e-8, 5), mg.f32_must_move,
                     lambda: mg.f32_line_subsweep(0, 0), lambda: mg.f32_get_vec(0, "u")):
            with pytest.raises(amg.AmgHipError) as err:
                call()
            assert err.value.status == amg.EUNSUPPORTED
            assert "is not supported (true Jacobi and Chebyshev are)" in str(err.value)
    finally:
        mg.close()


# ---- 7. must-move bytes -----------------------------------------------------------------------------------
def _separators(n, s):
    """rows on a separator position (p % 32 == 31 on their chain) of the chains of stride s"""
    return sum(min(s, n - p * s) for p in range(31, (n + s - 1) // s, 32))


def _must_move_by_hand(mg, solve):
    """enqueue_f32_vcycle's launches; solve(l) = the bytes of the line solves of one smoothing of level l"""
    nl = mg.n_levels
    n = [mg.get_n_dofs(l) for l in range(nl)]

    def mat(l):
        layout, stream = mg.level_layout(l)
        assert layout == SELL
        panels = (n[l] + 63) // 64
        slots, rest = divmod(stream - 8 * panels, 10)      # 8 + 2 bytes per slot in double
        assert rest == 0
        return 6 * slots + 8 * panels
    total = 4 * n[0] + 24 * n[0]               # the zero guess; v -> float and float -> z
    for l in range(nl - 1):
        subsweeps, bytes_ = solve(l)
        total += 2 * (subsweeps * (mat(l) + 12 * n[l]) + bytes_)   # pre and post: residual + solve per sub-sweep
        total += mat(l) + 12 * n[l]                               # the cycle's residual
        assert mg.level_transfer_kind(l) in (1, 2)
        total += 4 * n[l] + 8 * n[l + 1] + 4 * n[l + 1] + 8 * n[l]
    nc = n[-1]
    total += 24 * nc + 16 * nc * max(mg.coarse_halfbw(), 1) + 24 * nc
    return float(total)


def test_must_move_is_the_formula(amg, oracle):
    """Per sub-sweep the float matrix pass + 12 n, then K-LineX 32 n, K-Line 40 (n - n_sep) + 48 n_sep.
    16 x 8 / 2 levels, LINE_ALT: level 0 has 128 rows, x (K-LineX) and y (stride 16, 8 positions: no
    separator): 32 * 128 + 40 * 128 per smoothing.  64^2 / 4 levels, LINE_JACOBI: every level one K-Line
    direction of the level's stride."""
    A = MT.diffusion((16, 8), seed=2)
    mg = tensor_dev(amg, A, np.ones(128), (16, 8), 2)
    try:
        assert mg.line_directions(0) == [1, 16] and _separators(128, 16) == 0
        want = _must_move_by_hand(mg, lambda l: (2, 32 * 128 + 40 * 128))
        got = mg.f32_must_move()
        print(f"\n16 x 8 / 2 LINE_ALT: {got:.0f} bytes, by hand {want:.0f}")
        assert got == want
    finally:
        mg.close()
    Ao = oracle.laplacian(64)
    mg = amg.Multigrid(Ao.colptr, Ao.rowind, Ao.val, oracle.rhs(64), 4, smoother=amg.SM_LINE_JACOBI, omega=0.7,
                       layout=SELL)
    try:
        def solve(l):
            n, s = mg.get_n_dofs(l), mg.line_stride(l)
            sep = _separators(n, s)
            return 1, 40 * (n - sep) + 48 * sep
        seps = [_separators(mg.get_n_dofs(l), mg.line_stride(l)) for l in range(3)]
        assert any(seps)
        want = _must_move_by_hand(mg, solve)
        got = mg.f32_must_move()
        print(f"64^2 / 4 LINE_JACOBI: strides {[mg.line_stride(l) for l in range(3)]}, separator rows {seps}: "
              f"{got:.0f} bytes, by hand {want:.0f}")
        assert got == want
    finally:
        mg.close()
