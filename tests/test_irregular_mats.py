"""The irregular test matrices (tests/irregular_mats.py) are what the GPU tests take them for, and
`plan`, the host model of the layout rule, agrees with the library's own dictionary encoder
(amg_hip_dict_probe needs no device) on every one of them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import irregular_mats as im  # noqa: E402

NAMES = [c.name for c in im.cases()]

# what each case is there to hit: layout under AUTO / under a DICT request, dict typed?, code words
INTENT = {
    "knn-1": ("dict", "dict", True, 1),
    "knn-63": ("sell", "sell", None, None),
    "knn-64": ("sell", "sell", None, None),
    "knn-65": ("sell", "sell", None, None),
    "knn-129": ("sell", "sell", None, None),
    "knn-257": ("sell", "sell", None, None),
    "knn-513": ("sell", "sell", None, None),
    "knn-4097": ("csr", "sell", None, None),             # padding: 35520 slots > 1.25 nnz + 4096
    "knn-quant-513": ("dict", "dict", False, 2),
    "winperm-65": ("dict", "dict", False, 1),
    "shapes-typed-2w": ("dict", "dict", True, 2),
    "shapes-typed-1w-513": ("dict", "dict", True, 1),
    "shapes-untyped-2w": ("dict", "dict", False, 2),
    "shapes-typed-1w-257": ("dict", "dict", True, 1),
    "stair": ("sell", "sell", None, None),
    "stair-trailing-empty": ("sell", "sell", None, None),
    "stair-cut": ("sell", "sell", None, None),
    "far-32767": ("dict", "dict", True, 1),
    "far-32768": ("dict", "dict", True, 1),
    "limit-pairs255": ("dict", "dict", True, 1),
    "limit-pairs256": ("sell", "sell", None, None),
    "limit-row16": ("dict", "dict", True, 2),
    "limit-row17": ("sell", "sell", None, None),
    "limit-types255": ("dict", "dict", True, 1),
    "limit-types256": ("dict", "dict", False, 1),
    "limit-row8": ("dict", "dict", True, 1),
    "limit-row9": ("dict", "dict", True, 2),
    "halo-knn": ("sell", "sell", None, None),
    "halo-shapes": ("dict", "dict", True, 1),
    "haloT-knn": ("sell", "sell", None, None),
    "haloT-shapes": ("sell", "sell", None, None),
    "zeros-knn-513": ("sell", "sell", None, None),
    "zeros-shapes-257": ("dict", "dict", True, 1),
    "zeros-stair": ("csr", "sell", None, None),
}


def test_every_case_has_a_stated_intent():
    assert sorted(INTENT) == sorted(NAMES)
    sizes = {c.A.shape[0] for c in im.cases()}
    assert {1, 63, 64, 65, 129, 257, 513, 4097} <= sizes
    assert max(sizes) == 33000


@pytest.mark.parametrize("name", NAMES)
def test_plan_agrees_with_the_dictionary_encoder(amg, name):
    c = im.case(name)
    A = c.A
    assert A.indices.dtype == np.int32 and A.indptr.dtype == np.int32
    for r in range(A.shape[0]):
        assert np.all(np.diff(A.indices[A.indptr[r]:A.indptr[r + 1]]) > 0), r   # sorted, no duplicates
    P = im.pruned(A)
    assert np.all(P.data != 0.0)
    auto, want_dict = im.plan(P, im.LAYOUT_AUTO, c.shift), im.plan(P, im.LAYOUT_DICT, c.shift)
    got = amg.dict_probe(P.indptr, P.indices, P.data, P.shape[1], c.shift)
    if want_dict.layout == im.LAYOUT_DICT:
        assert got == (want_dict.pairs, want_dict.row_types if want_dict.typed else 0, want_dict.words)
    else:
        assert got is None
    i_auto, i_dict, typed, words = INTENT[name]
    assert im.LAYOUT_NAME[auto.layout] == i_auto and im.LAYOUT_NAME[want_dict.layout] == i_dict
    assert (want_dict.typed, want_dict.words) == (typed, words)
    # explicit requests hold; the byte formulas tell the variants apart
    assert im.plan(P, im.LAYOUT_CSR, c.shift).stream_bytes == 12 * P.nnz + 4 * (P.shape[0] + 1)
    s16, s32 = im.plan(P, im.LAYOUT_SELL, c.shift), im.plan(P, im.LAYOUT_SELL, c.shift, index16=False)
    assert s16.layout == s32.layout == im.LAYOUT_SELL and not s32.idx16
    assert s32.stream_bytes == 12 * s32.slots + 8 * ((P.shape[0] + 63) // 64)
    if s16.idx16:
        assert s32.stream_bytes - s16.stream_bytes == 2 * s16.slots
    if want_dict.layout == im.LAYOUT_DICT and want_dict.typed:
        untyped = im.plan(P, im.LAYOUT_DICT, c.shift, row_types=False)
        assert not untyped.typed and untyped.stream_bytes == 8 * words * P.shape[0] + 12 * untyped.pairs


def test_the_limit_cases_sit_on_their_limits():
    p = lambda k: im.plan(im.dict_limit(k), im.LAYOUT_DICT)
    assert (p("pairs255").pairs, p("pairs256").pairs) == (255, 256)
    assert (p("row16").max_row, p("row17").max_row) == (16, 17)
    assert (p("types255").row_types, p("types256").row_types) == (255, 256)
    assert (p("row8").max_row, p("row9").max_row) == (8, 9)
    assert p("pairs256").layout == p("row17").layout == im.LAYOUT_SELL
    assert p("types255").typed and not p("types256").typed


@pytest.mark.parametrize("d,fits", [(32767, True), (32768, False)])
def test_far_reaches_the_16_bit_limit(d, fits):
    A = im.far(33000, d)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    off = A.indices.astype(np.int64) - rows
    assert off.max() == d and off.min() == -d
    assert np.count_nonzero(np.abs(off) == d) >= 6
    assert im.plan(A, im.LAYOUT_SELL).idx16 is fits


def test_staircase_panels():
    W = im.STAIR_WIDTHS
    for widths, n in ((W, None), (W + [0], None), (W, 64 * len(W) - 63)):
        A = im.staircase(widths, n=n)
        cnt = np.diff(A.indptr)
        pad = np.concatenate([cnt, np.zeros(-cnt.size % 64, cnt.dtype)]).reshape(-1, 64)
        assert list(pad.max(axis=1)) == list(widths)               # one row of exactly the width
        assert pad.min(axis=1).max() <= 3 and np.count_nonzero(cnt == 0) >= 64   # ragged, empty rows
        dg = A.diagonal() != 0
        assert 0.6 < dg[cnt > 0].mean() < 0.9                      # some rows have no diagonal
    assert im.staircase(W + [0]).shape[0] == 64 * 17
    assert im.staircase(W, n=961).shape[0] == 961 and np.diff(im.staircase(W, n=961).indptr)[-1] == 2


def test_pruning_cases_have_signed_zeros_an_empty_row_and_an_empty_tail():
    for name in ("zeros-knn-513", "zeros-shapes-257", "zeros-stair"):
        A = im.case(name).A
        z = A.data[A.data == 0.0]
        assert np.any(np.signbit(z)) and np.any(~np.signbit(z))
        cnt = np.diff(im.pruned(A).indptr)
        n = cnt.size
        assert cnt[n // 2] == 0 and np.all(cnt[n - 70:] == 0) and np.diff(A.indptr)[n - 70:].sum() > 0
        assert cnt.reshape(-1)[(n - 1) // 64 * 64:].max() == 0    # the last panel is empty


def test_halo_blocks_keep_their_diagonal_at_the_shift():
    for name in ("halo-knn", "halo-shapes"):
        c = im.case(name)
        rows, cols = c.A.shape
        assert cols == rows + 2 * c.shift
        E = im.embed(c.A, c.shift)
        T = im.case(name.replace("halo", "haloT")).A
        assert T.shape == (cols, rows) and im.plan(T, im.LAYOUT_DICT).layout == im.LAYOUT_SELL
        assert E.shape == (cols, cols) and np.all(E.diagonal()[c.shift:c.shift + rows] != 0.0)
        lo = c.A.indices.min(), c.A.indices.max()
        assert lo[0] < c.shift and lo[1] >= rows + c.shift        # both halos are referenced
