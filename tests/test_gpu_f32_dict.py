"""The single-precision V-cycle on dictionary-coded levels (amg_hip_set_f32_dict; kernels.hip: K-DictF32)
bit for bit against its float32 restatement tests/f32_twin.py, as tests/test_gpu_f32_bitwise.py does for
the SELL / CSR levels: step by step on random data through amg_hip_f32_set_vec / amg_hip_f32_level_op /
amg_hip_f32_get_vec, and as a whole cycle (every level's u, f and r, captured and eager, first and
replayed call).  Equality is on view(np.uint32) everywhere.  The level matrices and transfers come from
the solver's getters; the coarsest solve is the solver's own double one.

Every case first asserts the layouts it is named for (dict_cases.check_path): a solver that fell back to
SELL would test nothing.  Without the feature every case is refused with AMG_HIP_EUNSUPPORTED.
Cases: tests/dict_cases.py."""
import os
import sys

import numpy as np
import pytest

sp = pytest.importorskip("scipy.sparse")
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dict_cases as DC  # noqa: E402
import f32_twin as FT  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def switch(amg):
    amg.set_f32_dict(1)
    try:
        yield
    finally:
        amg.set_f32_dict(0)
        amg.set_dict_rows(2)
        amg.set_row_types(1)


def rnd(rng, n):
    return rng.standard_normal(n).astype(np.float32)


def bits_equal(got, want, what):
    assert got.dtype == np.float32 and want.dtype == np.float32, what
    assert np.all(np.isfinite(want)), what
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (f"{what}: {bad.size} of {got.size} entries differ, first at {int(bad[0])}: "
                           f"device {got[bad[0]]!r} twin {want[bad[0]]!r}")


# ---- a. single steps on random data -----------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(DC.CASES))
def test_single_steps_have_the_twins_bits(amg, oracle, case):
    mg = DC.make(amg, oracle, case)
    try:
        with DC.running(amg, case):
            H, A = DC.hierarchy(mg, case)
            path = DC.check_path(mg, case, H, A)
            nl = mg.n_levels
            rng = np.random.default_rng(nl * 1000 + H.n[0])
            done = []
            for l in range(nl - 1):
                u, f = rnd(rng, H.n[l]), rnd(rng, H.n[l])
                mg.f32_set_vec(l, "u", u)
                mg.f32_set_vec(l, "f", f)
                bits_equal(mg.f32_get_vec(l, "u"), u, (case, l, "set / get"))
                mg.f32_level_op(l, 0)
                u1 = H.smooth(l, u, f)
                bits_equal(mg.f32_get_vec(l, "u"), u1, (case, l, "op 0: u after the smoother"))
                bits_equal(mg.f32_get_vec(l, "f"), f, (case, l, "op 0: f unchanged"))
                assert not FT.same_bits(u1, u)
                mg.f32_level_op(l, 1)
                r = H.resid(l, u1, f)
                bits_equal(mg.f32_get_vec(l, "r"), r, (case, l, "op 1: r"))
                bits_equal(mg.f32_get_vec(l, "u"), u1, (case, l, "op 1: u unchanged"))
                mg.f32_set_vec(l + 1, "u", rnd(rng, H.n[l + 1]))  # op 2 has to zero it
                mg.f32_level_op(l, 2)
                bits_equal(mg.f32_get_vec(l + 1, "f"), H.restrict(l, r), (case, l, "op 2: f of the coarser level"))
                assert not np.any(mg.f32_get_vec(l + 1, "u").view(np.uint32)), (case, l, "op 2: u_H is +0.0")
                uH = rnd(rng, H.n[l + 1])
                mg.f32_set_vec(l + 1, "u", uH)
                mg.f32_level_op(l, 3)
                bits_equal(mg.f32_get_vec(l, "u"), H.prolong_add(l, uH, u1), (case, l, "op 3: u"))
                done.append(l)
            fL = rnd(rng, H.n[-1])
            mg.f32_set_vec(nl - 1, "f", fL)
            mg.f32_level_op(nl - 1, 4)
            bits_equal(mg.f32_get_vec(nl - 1, "u"), H.coarse_solve(fL), (case, nl - 1, "op 4: u"))
            print(f"\n{case}: {path}; n = {H.n}; ops 0 1 2 3 bit for bit on levels {done}, op 4 on level {nl - 1}")
    finally:
        mg.close()


# ---- b. the whole cycle -----------------------------------------------------------------------------
def _apply(mg, v):
    dv = torch.from_numpy(np.array(v)).cuda()
    dz = torch.empty_like(dv)
    mg.apply_f32(dv.data_ptr(), dz.data_ptr())
    mg.sync()
    return dz.cpu().numpy()


@pytest.mark.parametrize("case", sorted(DC.CASES))
def test_the_cycle_leaves_the_twins_bits_on_every_level(amg, oracle, case):
    said = []
    for graph in (True, False):
        mg = DC.make(amg, oracle, case, use_graph=graph)
        try:
            with DC.running(amg, case):
                H, A = DC.hierarchy(mg, case)
                DC.check_path(mg, case, H, A)
                nl = mg.n_levels
                v = np.random.default_rng(7).standard_normal(H.n[0])
                if DC.CASES[case]["A"] in ("per", "nat"):
                    v -= v.mean()
                u, f, r = FT.cycle(H, v)
                assert np.linalg.norm(u[0]) > 0
                for call in ("first", "second"):
                    z = _apply(mg, v)
                    where = (case, "graph" if graph else "eager", call)
                    for l in range(nl):
                        bits_equal(mg.f32_get_vec(l, "u"), u[l], where + (l, "u"))
                        bits_equal(mg.f32_get_vec(l, "f"), f[l], where + (l, "f"))
                        if l < nl - 1:
                            bits_equal(mg.f32_get_vec(l, "r"), r[l], where + (l, "r"))
                    assert z.dtype == np.float64
                    assert np.array_equal(z.view(np.uint64), u[0].astype(np.float64).view(np.uint64))
                said.append(f"{'graph' if graph else 'eager'}: u f r of levels 0 .. {nl - 2}, u f of level {nl - 1}, "
                            "z = widen(u_0), first and replayed call")
        finally:
            mg.close()
    print(f"\n{case}: " + "; ".join(said))


@pytest.mark.parametrize("case", ["t33", "nonsym", "box"])
def test_the_comparison_sees_a_reversed_row_order(amg, oracle, case):
    """control: the device's residual and Jacobi sweep on level 0 have the ascending sums' bits and NOT the
    descending ones', so the comparisons above would catch a kernel that walked a row the other way round"""
    mg = DC.make(amg, oracle, case)
    try:
        H, A = DC.hierarchy(mg, case)
        DC.check_path(mg, case, H, A)
        rng = np.random.default_rng(5)
        u, f = rnd(rng, H.n[0]), rnd(rng, H.n[0])
        mg.f32_set_vec(0, "u", u)
        mg.f32_set_vec(0, "f", f)
        mg.f32_level_op(0, 1)
        got = mg.f32_get_vec(0, "r")
        bits_equal(got, H.resid(0, u, f), "ascending residual")
        down = FT.residual(FT.Rows(sp.csr_matrix(A[0]), descending=True), u, f)
        differ_r = int(np.count_nonzero(got.view(np.uint32) != down.view(np.uint32)))
        mg.f32_level_op(0, 0)
        got = mg.f32_get_vec(0, "u")
        bits_equal(got, H.smooth(0, u, f), "ascending sweeps")
        Rd = FT.Rows(sp.csr_matrix(sp.csc_matrix(A[0]).T), descending=True)
        down = FT.jacobi(Rd, FT.jacobi(Rd, u, f, 0.8), f, 0.8)
        differ_j = int(np.count_nonzero(got.view(np.uint32) != down.view(np.uint32)))
        print(f"\n{case} level 0: the descending sums differ from the device in {differ_r} (residual) and "
              f"{differ_j} (two Jacobi sweeps) of {got.size} entries")
        assert differ_r >= 1 and differ_j >= 1
    finally:
        mg.close()
