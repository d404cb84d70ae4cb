"""The numpy reference of the sequential-sum tests (tests/seq_sums_common.py reference()) IS the library's host loop: a stand-alone host program
(tests/cpp/seq_sums_host_check.cpp, compiled with -ffp-contract=off against host_math.hpp) runs op_host::track_sums_reference_order -- the
library's restatement of the reference's accumulation -- with one and with two rows per pixel on rows and an acceptance mask read from a file,
and every sum and the count are bit-equal to reference() over the accepted rows (NaNs compared as NaNs): for order-sensitive data and for the
special values tests/test_seq_sums_gpu.py feeds the kernel -- products that underflow, sums that overflow and meet the other infinity,
signed zeros, cancellation, a NaN column.  The size sweep's inputs are also held here to the condition that makes a bit comparison with
reference() meaningful: summed in float64, or last to first, at least half of the accumulators (both of layout 2's) come out different."""
import os
import subprocess

import numpy as np
import pytest

import seq_sums_common as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PIX = 1000


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("seq_sums") / "seq_sums_host_check"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I", os.path.join(ROOT, "onepiece_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "seq_sums_host_check.cpp"), "-o", str(exe)])
    return str(exe)


def _host_loop(program, tmp_path, rows, mask):
    rows = np.ascontiguousarray(rows, np.float32).reshape(-1, 14)
    mask = np.ascontiguousarray(mask, np.int32)
    assert len(rows) == len(mask)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([len(rows)], np.int32).tobytes() + rows.tobytes() + mask.tobytes())
    subprocess.run([program, str(src), str(dst)], check=True, timeout=60)
    out = np.fromfile(dst, np.float32)
    assert out.shape == (86,)
    return out[:43], out[43:]


def _mask(n, seed, rejected):
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 1 << 20, n).astype(np.int32)   # pair_t: the target pixel's index, 0 included
    m[0] = 0
    if rejected:
        m[rng.uniform(size=n) < 0.3] = -1
        m[n // 2] = -1
    return m


INPUTS = {
    "wide": lambda: S.wide(N_PIX, 14, 7),
    "denormal_products": lambda: S.denormal_products(N_PIX, 14, 11),
    "overflowing": lambda: S.overflowing(N_PIX, 14, 12),
    "signed_zeros": lambda: S.signed_zeros(N_PIX, 14, 13),
    "cancelling": lambda: S.cancelling(N_PIX, 14, 14),
    "nan_column": lambda: S.nan_column(N_PIX, 14, 15, N_PIX // 2, 2),
}


@pytest.mark.parametrize("rejected", [False, True], ids=["all_accepted", "some_rejected"])
@pytest.mark.parametrize("name", sorted(INPUTS))
def test_the_numpy_reference_is_the_librarys_host_loop(program, tmp_path, name, rejected):
    rows, mask = INPUTS[name](), _mask(N_PIX, 3, rejected)
    kept = rows[mask >= 0]
    assert rejected == (len(kept) < N_PIX) and len(kept) > N_PIX // 2
    one, two = _host_loop(program, tmp_path, rows, mask)
    want_one, want_two = S.reference(0, kept[:, :7]), S.reference(1, kept)
    assert one[42:].view(np.uint32)[0] == len(kept) == two[42:].view(np.uint32)[0]
    assert S.same_bits(one, want_one), np.nonzero(S.canonical_bits(one) != S.canonical_bits(want_one))[0]
    assert S.same_bits(two, want_two), np.nonzero(S.canonical_bits(two) != S.canonical_bits(want_two))[0]


def test_the_special_inputs_hold_the_values_they_are_named_after():
    tiny = np.float32(np.finfo(np.float32).tiny)
    p = S.products(0, S.denormal_products(N_PIX, 7, 11))
    assert (np.abs(p[:, :36]) < tiny).all() and (p[:, :36] != 0).any() and (p[:, :36] == 0).any() and (np.abs(p[:, 36:]) >= tiny).all()
    ref = S.reference(0, S.denormal_products(N_PIX, 7, 11))[:36]
    assert ((np.abs(ref) < tiny) & (ref != 0)).sum() >= 6, "sums that are denormal themselves (off the diagonal, where the signs are mixed)"
    assert (np.abs(S.reference(2, S.denormal_products(N_PIX, 2, 11))[:2]) < tiny).all()
    for layout in (0, 1, 2):
        ref = S.reference(layout, S.overflowing(N_PIX, S.ITEM_FLOATS[layout], 12))[:-1]
        assert np.isnan(ref).any() and np.isinf(ref).any(), "inf meets -inf in some sums, others stay infinite"
        ref = S.reference(layout, S.signed_zeros(N_PIX, S.ITEM_FLOATS[layout], 13))
        assert not ref[:-1].view(np.uint32).any(), "+0 everywhere"
    assert not S.reference(2, S.negative_zeros(N_PIX, 2))[:2].view(np.uint32).any()
    assert np.signbit(S.signed_zeros(N_PIX, 7, 13)).any() and not np.signbit(S.signed_zeros(N_PIX, 7, 13)).all()


def test_the_vectorised_products_equal_the_scalar_definition():
    """products() forms all products of a row at once; the definition is acc[a*6+b] += J[a]*J[b], acc[36+a] += J[a]*r, one at a time"""
    rows = S.wide(50, 7, 5)
    acc = np.zeros(42, np.float32)
    for row in rows:
        J, r = row[:6], row[6]
        for a in range(6):
            for b in range(6):
                acc[a * 6 + b] = np.float32(acc[a * 6 + b] + np.float32(J[a] * J[b]))
            acc[36 + a] = np.float32(acc[36 + a] + np.float32(J[a] * r))
    assert S.same_bits(acc, S.reference(0, rows)[:42])
    two = S.wide(25, 14, 5)
    assert S.same_bits(S.reference(1, two)[:42], S.reference(0, two.reshape(50, 7))[:42]), "a layout-1 item is two consecutive rows"
    assert S.reference(1, two)[42:].view(np.uint32)[0] == 25


@pytest.mark.parametrize("layout", [0, 1, 2])
def test_the_sweeps_inputs_are_order_sensitive(hip, layout):
    """the condition of the size sweep (tests/test_seq_sums_gpu.py), on the reference alone"""
    P = hip.load().op_debug_seq_tile_rows() // S.ROWS_PER_ITEM[layout]
    assert P > 0
    for n in S.sweep_sizes(P):
        if n >= P:
            d64, drev, need = S.order_sensitivity(layout, S.sweep_rows(layout, P)[:n])
            print("layout %d n %d: %d (float64) and %d (last to first) of %d accumulators differ" % (layout, n, d64, drev, S.NACC[layout]))
            assert d64 >= need and drev >= need, (layout, n, d64, drev, need)
