"""k_seq_sums / k_seq_sums_many (onepiece_amd/csrc/seq_sums.hip) themselves, through op_debug_seq_sums and op_debug_seq_sums_many: every sum and
the count bit-equal to the plain in-order float32 definition (tests/seq_sums_common.py reference(), which tests/test_seq_sums_cpu.py holds to the
library's host loop), NaNs compared as NaNs.  No tolerance anywhere.

Sizes come from the kernel's tile (op_debug_seq_tile_rows): with P items per tile, the counts sit on the pipeline's regime changes -- nothing, the
prologue's two tiles, a tile +- 1, exactly 2 / 3 / 4 tiles, and 20 tiles for the steady state -- on data whose sums depend on their order (asserted
before the device is touched: summed in float64, or last to first, at least half of the accumulators differ).  Every buffer is longer than the
problem and its tail is NaN, inside the allocation: a word from behind item n that reaches a sum makes it NaN.  Special values cross a tile boundary
(n = P + 5): products that underflow, sums that overflow and meet the other infinity, signed zeros, cancellation, a NaN column.  The many-problem
launch runs 1, 2, 9 and 32 workgroups with an empty problem, a null-pointer problem and the longest one among them, and equals the stand-alone
launch problem by problem."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from onepiece_amd import _lib as L
import seq_sums_common as S

LAYOUTS = [0, 1, 2]
SIZE_NAMES = ["0", "1", "2", "P-1", "P", "P+1", "2P-1", "2P", "2P+1", "3P", "3P+1", "4P", "4P+1", "5P+7", "20P+5"]


def _P(layout):
    p = L.load().op_debug_seq_tile_rows() // S.ROWS_PER_ITEM[layout]
    assert p > 0
    return p


def _size(layout, name):
    P = _P(layout)
    sizes = dict(zip(SIZE_NAMES, S.sweep_sizes(P)))
    assert len(sizes) == len(S.sweep_sizes(P))
    return P, sizes[name]


def _sums(layout, uploaded, n_items):
    """the device's sums of the first n_items items of `uploaded` (all of it goes to the device)"""
    out = np.full(S.NACC[layout] + 1, 123.0, np.float32)
    if uploaded is None:
        L.check(L.load().op_debug_seq_sums(layout, None, 0, n_items, out.ctypes.data))
        return out
    uploaded = np.ascontiguousarray(uploaded, np.float32).reshape(-1, S.ITEM_FLOATS[layout])
    L.check(L.load().op_debug_seq_sums(layout, uploaded.ctypes.data, len(uploaded), n_items, out.ctypes.data))
    return out


def _poisoned(layout, rows, P):
    """the rows with 2P + 3 items of NaN behind them"""
    rows = S.items(layout, rows)
    return np.concatenate([rows, np.full((2 * P + 3, S.ITEM_FLOATS[layout]), np.nan, np.float32)])


def _sums_many(layout, problems):
    """problems: [n, ITEM_FLOATS] arrays, or None for a null pointer with no items"""
    k = len(problems)
    keep = [None if p is None else np.ascontiguousarray(p, np.float32) for p in problems]
    ptrs = (C.c_void_p * max(k, 1))(*[None if p is None else p.ctypes.data for p in keep])
    counts = np.array([0 if p is None else len(p) for p in keep] or [0], np.uint32)
    out = np.full((max(k, 1), S.NACC.get(layout, 42) + 1), 123.0, np.float32)
    rc = L.load().op_debug_seq_sums_many(layout, C.cast(ptrs, C.c_void_p), counts.ctypes.data, k, out.ctypes.data)
    return rc, out


def _differing(got, want):
    return np.nonzero(S.canonical_bits(got) != S.canonical_bits(want))[0].tolist()


@pytest.mark.parametrize("name", SIZE_NAMES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_size_sweep_over_the_pipelines_regime_changes(layout, name):
    P, n = _size(layout, name)
    rows = S.sweep_rows(layout, P)[:n]
    want = S.sweep_reference(layout, P, n)
    if n >= P:   # the comparison below can only notice a re-associated sum if the sum depends on its order
        d64, drev, need = S.order_sensitivity(layout, rows)
        assert d64 >= need and drev >= need, (d64, drev, need)
    got = _sums(layout, _poisoned(layout, rows, P), n)
    assert got[-1:].view(np.uint32)[0] == n
    assert S.same_bits(got, want), "accumulators %s differ" % _differing(got, want)
    if n == 0:
        assert not got.view(np.uint32).any(), "nothing to sum: +0 everywhere, count 0"
        empty = _sums(layout, None, 0)
        assert not empty.view(np.uint32).any(), "rows = NULL, nothing uploaded"


def _special(layout, kind, P):
    n, nf = P + 5, S.ITEM_FLOATS[layout]
    if kind == "negative_zeros":
        return S.negative_zeros(n, nf)
    if kind == "nan_column":
        return S.nan_column(n, nf, 15, P + 2, 2 if layout < 2 else 1)
    return getattr(S, kind)(n, nf, 10 + len(kind))


@pytest.mark.parametrize("kind", ["wide", "denormal_products", "overflowing", "signed_zeros", "negative_zeros", "cancelling", "nan_column"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_special_values_across_a_tile_boundary(layout, kind):
    P = _P(layout)
    rows = _special(layout, kind, P)
    want = S.reference(layout, rows)
    sums = want[:-1]
    tiny = np.float32(np.finfo(np.float32).tiny)
    # the input does what its name says, by the reference
    if kind == "denormal_products":
        own = sums[:36] if layout < 2 else sums
        assert ((np.abs(own) < tiny) & (own != 0)).sum() >= (6 if layout < 2 else 2), "denormal sums to keep (off the diagonal, where the signs are mixed)"
        assert layout == 2 or (np.abs(sums[36:]) >= tiny).all()
    elif kind == "overflowing":
        assert np.isnan(sums).any() and np.isinf(sums).any(), "inf meets -inf in some sums, others stay infinite"
    elif kind in ("signed_zeros", "negative_zeros"):
        assert np.signbit(rows).any() and not sums.view(np.uint32).any(), "+0 everywhere"
    elif kind == "nan_column":
        hit = np.zeros(S.NACC[layout], bool)
        if layout < 2:
            for a in range(6):
                hit[a * 6 + 2] = hit[2 * 6 + a] = True
            hit[36 + 2] = True
        else:
            hit[1] = True
        assert np.array_equal(np.isnan(sums), hit), "exactly the accumulators that involve the column"
    got = _sums(layout, _poisoned(layout, rows, P), len(rows))
    assert got[-1:].view(np.uint32)[0] == len(rows)
    assert S.same_bits(got, want), "accumulators %s differ" % _differing(got, want)
    if kind == "nan_column":
        assert np.array_equal(np.isnan(got[:-1]), np.isnan(sums))


def _launches(layout, k, P):
    """what each launch of k workgroups sums: item counts from the sweep's list, None = a null pointer with no items.  An empty problem, a
    null-pointer one (k >= 2) and the longest are always among them, shuffled; where k has no room for all three, in several launches"""
    sizes = S.sweep_sizes(P)
    big = sizes[-1]
    if k == 1:
        return [[big], [0], [None]]
    if k == 2:
        return [[None, big], [big, 0]]
    rng = np.random.default_rng(100 * layout + k)
    picks = [0, None, big] + [int(n) for n in rng.choice(sizes[:-1], k - 3)]
    return [[picks[i] for i in rng.permutation(k)]]


@pytest.mark.parametrize("k", [1, 2, 9, 32])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_many_problems_in_one_launch_equal_the_reference_and_the_single_launch(layout, k):
    P = _P(layout)
    launches = _launches(layout, k, P)
    seen = [n for picks in launches for n in picks]
    assert 0 in seen and S.sweep_sizes(P)[-1] in seen and (None in seen or k < 2) and all(len(picks) == k for picks in launches)
    alone = {}
    for picks in launches:
        problems = [None if n is None else S.sweep_rows(layout, P)[:n] for n in picks]
        rc, out = _sums_many(layout, problems)
        L.check(rc)
        for i, pick in enumerate(picks):
            n = pick or 0
            want = S.sweep_reference(layout, P, n)
            assert out[i, -1:].view(np.uint32)[0] == n
            assert S.same_bits(out[i], want), "problem %d (%d items): accumulators %s differ" % (i, n, _differing(out[i], want))
            if pick not in alone:   # "results do not depend on who sums with whom" (seq_sums.hpp)
                alone[pick] = _sums(layout, problems[i], n)
            assert np.array_equal(out[i].view(np.uint32), alone[pick].view(np.uint32)), "problem %d (%d items) alone" % (i, n)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_many_refuses_no_problems_and_more_than_a_batch(layout):
    one = S.sweep_rows(layout, _P(layout))[:3]
    assert _sums_many(layout, [])[0] == L.OP_ERR_INVALID
    assert _sums_many(layout, [one] * 33)[0] == L.OP_ERR_INVALID
    assert _sums_many(layout, [one] * 32)[0] == 0
    assert _sums_many(3, [one])[0] == L.OP_ERR_INVALID


def test_argument_errors_of_the_single_entry():
    lib = L.load()
    rows = S.wide(5, 7, 1)
    out = np.zeros(43, np.float32)
    assert lib.op_debug_seq_sums(3, rows.ctypes.data, 5, 5, out.ctypes.data) == L.OP_ERR_INVALID
    assert lib.op_debug_seq_sums(-1, rows.ctypes.data, 5, 5, out.ctypes.data) == L.OP_ERR_INVALID
    assert lib.op_debug_seq_sums(0, None, 5, 5, out.ctypes.data) == L.OP_ERR_INVALID
    assert lib.op_debug_seq_sums(0, None, 5, 0, out.ctypes.data) == L.OP_ERR_INVALID
    assert lib.op_debug_seq_sums(0, rows.ctypes.data, 5, 6, out.ctypes.data) == L.OP_ERR_INVALID
    assert lib.op_debug_seq_sums(0, rows.ctypes.data, 5, 5, None) == L.OP_ERR_INVALID
    assert not out.any()
    assert lib.op_debug_seq_sums(0, rows.ctypes.data, 5, 5, out.ctypes.data) == 0 and S.same_bits(out, S.reference(0, rows))
