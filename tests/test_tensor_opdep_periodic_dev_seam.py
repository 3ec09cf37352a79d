"""The fixtures of tests/test_gpu_tensor_opdep_periodic_dev.py can tell a wrong seam from a right one (no GPU).

That test compares the device-built hierarchy of amg_hip_create_tensor_opdep_periodic_dev with the host
constructor's bit for bit; it proves the seam only if a seam done the open way would CHANGE those bits.  On the
nonsymmetric operator of tests/opdep_periodic_dev_cases.py, for (6, 5) per 3 and (4, 4, 4) per 7, the last
coarse row of the axis of R (A P) is recomputed in numpy in spgemm_rows' order, once with the fine rows in the
order 0, m - 2, m - 1 and once in the open order m - 2, m - 1, 0: the first equals the host_only solver's level-1
row bit for bit, the second differs from it in at least one word.  Likewise the weights: fine row 0 collapsed by
the distance mod m gives the solver's w_lo(0), by the plain distance another value.

Seed: opdep_periodic_dev_cases.NONSYM_SEED = 2024 discriminates on both grids; it is the first one tried.

Then the wording of include/amg_hip.h and of the Python layer for the changed entry point and the switch."""
import os
import sys

import numpy as np
import pytest

sp = pytest.importorskip("scipy.sparse")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import opdep_periodic_dev_cases as K  # noqa: E402
import opdep_periodic_twin as OP  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = (((6, 5), 3), ((4, 4, 4), 7))


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def csr_of_csc(triple, rows, cols):
    """CSR of a CSC triple by hand, stored zeros kept"""
    cp, ri, v = (np.asarray(a) for a in triple)
    col = np.repeat(np.arange(cols, dtype=np.int64), np.diff(cp))
    order = np.lexsort((col, ri))
    ptr = np.zeros(rows + 1, np.int64)
    np.add.at(ptr, ri.astype(np.int64) + 1, 1)
    return sp.csr_matrix((np.asarray(v, np.float64)[order], col[order].astype(np.int32), np.cumsum(ptr).astype(np.int32)),
                         shape=(rows, cols))


def host_only(amg, A, b, dims, per, masks):
    Ac = sp.csc_matrix(A)
    Ac.sort_indices()
    return amg.Multigrid.tensor_opdep_periodic(Ac.indptr, Ac.indices, Ac.data, b, dims, len(masks) + 1, per,
                                               axis_masks=masks, smoother=amg.SM_JACOBI, smoother_iters=2, omega=0.8,
                                               host_only=True)


@pytest.mark.parametrize("dims,per", CASES)
def test_the_order_of_the_seam_rows_changes_the_bits(amg, dims, per):
    A, b, _ = K.case("nonsymmetric", dims, per)
    assert abs(A - A.T).max() > 0.1
    masks = K.chain(dims, per)
    assert masks[0] == 1  # level 0 coarsens x, which is periodic
    mg = host_only(amg, A, b, dims, per, masks)
    try:
        n0, n1 = mg.get_n_dofs(0), mg.get_n_dofs(1)
        m, mH = dims[0], dims[0] // 2
        assert n1 == n0 // 2 and mg.level_axes(0) == 1
        Pc = mg.get_transfer(0, "P")  # CSC: column I holds R's row I
        P = csr_of_csc(Pc, n0, n1)
        A0 = csr_of_csc(mg.get_coefficient_matrix(0), n0, n0)
        assert np.array_equal(bits(A0.data), bits(A.data)) and np.array_equal(A0.indices, A.indices)
        A1 = csr_of_csc(mg.get_coefficient_matrix(1), n1, n1)
        differing = 0
        seam_rows = [I for I in range(n1) if I % mH == mH - 1]
        assert len(seam_rows) == n1 // mH
        for I in seam_rows:
            lo, hi = Pc[0][I], Pc[0][I + 1]
            fine, w = [int(i) for i in Pc[1][lo:hi]], [float(x) for x in Pc[2][lo:hi]]
            line = (I // mH) * m
            assert fine == [line, line + m - 2, line + m - 1] and w[2] == 1.0, (I, fine)
            want = (A1.indices[A1.indptr[I]:A1.indptr[I + 1]], A1.data[A1.indptr[I]:A1.indptr[I + 1]])
            cols, vals = K.galerkin_row(A, P, fine, w)  # 0, m - 2, m - 1
            assert np.array_equal(cols, want[0]) and np.array_equal(bits(vals), bits(want[1])), (I, "the seam order")
            cols, vals = K.galerkin_row(A, P, fine[1:] + fine[:1], w[1:] + w[:1])  # m - 2, m - 1, 0: the open order
            assert np.array_equal(cols, want[0])  # the pattern does not depend on the order
            differing += int((bits(vals) != bits(want[1])).sum())
        print(f"\n{dims} per {per}: {differing} words of {len(seam_rows)} seam rows differ in the open order")
        assert differing >= 1, "this seed does not discriminate: choose another"
    finally:
        mg.close()


@pytest.mark.parametrize("dims,per", CASES)
def test_the_distance_mod_m_changes_the_weight_of_fine_row_0(amg, dims, per):
    A, b, _ = K.case("nonsymmetric", dims, per)
    masks = K.chain(dims, per)
    mg = host_only(amg, A, b, dims, per, masks)
    try:
        W = mg.axis_weights(0)
    finally:
        mg.close()
    wlo_per, whi_per = K.collapse_row(A, dims, 0, 0, True)
    wlo_open, whi_open = K.collapse_row(A, dims, 0, 0, False)
    assert bits(W[0, 0]) == bits(wlo_per) and bits(W[0, 1]) == bits(whi_per)
    assert bits(wlo_open) != bits(wlo_per) and wlo_per != 0.0
    assert bits(whi_open) == bits(whi_per)  # the high neighbour of fine 0 is the same either way
    # and the twin's rule is the same one
    Wt = OP.opdep_P_per(A, dims, len(dims), 1, per)[1]
    assert np.array_equal(bits(Wt), bits(W))


def test_header_and_python_layer_say_what_the_switch_governs(amg):
    with open(os.path.join(ROOT, "include", "amg_hip.h")) as f:
        h = " ".join(f.read().replace(" * ", " ").split())
    decl = h.index("amg_hip_status amg_hip_create_tensor_opdep_periodic_dev(int64_t n, const int32_t* rowptr_dev")
    comment = h[h.rindex("/*", 0, decl):decl]
    assert "With amg_hip_set_periodic_device_setup(1)" in comment
    assert "K-AxisWeights with the seam" in comment and "K-AxisGalerkin with the seam" in comment
    assert "amg_hip_setup_on_device reports 1 unless it fell back" in comment
    assert "With the switch off (the default)" in comment and "amg_hip_setup_on_device reports 0" in comment
    assert "not written yet" not in h
    sw = h.index("void amg_hip_set_periodic_device_setup(int32_t on);")
    comment = h[h.rindex("/*", 0, sw):sw]
    assert "amg_hip_create_tensor_periodic_dev" in comment and "amg_hip_create_tensor_opdep_periodic_dev" in comment
    assert "default 0" in comment
    on = h.index("amg_hip_status amg_hip_setup_on_device(")
    assert "amg_hip_create_tensor_opdep_periodic_dev under amg_hip_set_periodic_device_setup(1)" in h[h.rindex("/*", 0, on):on]
    assert "set_periodic_device_setup(1)" in amg.Multigrid.tensor_opdep_periodic_dev.__doc__
    assert "tensor_opdep_periodic_dev" in amg.set_periodic_device_setup.__doc__
