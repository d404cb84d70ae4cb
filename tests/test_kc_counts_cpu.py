"""k_integrate's lean instantiations read voxels_updated, voxels_written and the store mask off the weights (csrc/integrate.hip, kWCount): a lean
update is wv = w, w' = RN(w + 1.0f) on an integer weight, so the weight after a batch's frames minus the weight as loaded is the number of the
voxel's hits, and the voxel has to be stored exactly when the two differ.

The weight chain of voxel_update<true, true> in numpy.float32 (the only operations that touch w: wsum = w + 1.0f, w = wsum; the guard's division
path leaves it alone), next to the same chain in Python integers, for hit patterns over 1 .. 64 frames from the start weights 0 (the default voxel),
1 and 2^19 - 64 (the last batch the host launches lean: lean_frames <= 2^19, the running batch included): none, one (first / last / a middle frame),
all, alternating, and random ones of every density."""
import numpy as np

STARTS = (0, 1, (1 << 19) - 64)


def _patterns(n, rng):
    yield np.zeros(n, bool)
    yield np.ones(n, bool)
    for k in {0, n // 2, n - 1}:
        p = np.zeros(n, bool); p[k] = True
        yield p
    yield np.arange(n) % 2 == 0
    yield np.arange(n) % 2 == 1
    for density in (0.05, 0.3, 0.5, 0.8, 0.97):
        for _ in range(4):
            yield rng.random(n) < density


def _chain(w0, hits):
    """The device's float chain and the exact integer chain."""
    w, wi = np.float32(w0), int(w0)
    for h in hits:
        if h:
            wsum = np.float32(w + np.float32(1.0))   # wv = w (lean: no validity select), wsum = wv + 1.0f
            w = wsum                                 # w = wsum; the `slow` lanes redo the quotients, not this
            wi += 1
    return w, wi


def test_weight_difference_is_the_hit_count_and_differs_exactly_when_there_is_a_hit():
    rng = np.random.default_rng(20260)
    cases = 0
    for n in range(1, 65):
        for w0 in STARTS:
            for hits in _patterns(n, rng):
                w, wi = _chain(w0, hits)
                k = int(hits.sum())
                before = np.float32(w0)
                assert float(before) == w0 and float(w) == wi == w0 + k          # integers, exactly representable all the way
                diff = np.float32(w - before)                                    # the device's v_sub_f32 ...
                assert float(diff) == k and int(np.uint32(diff)) == k            # ... and v_cvt_u32_f32: the voxel's share of voxels_updated
                assert bool(w != before) == (k > 0)                              # the store mask / voxels_written
                cases += 1
    assert cases == 3 * (25 + 26 + 62 * 27)                                      # ({0, n // 2, n - 1} has one member for n = 1, two for n = 2)


def test_the_last_lean_weight_is_far_below_the_first_float_that_absorbs_a_one():
    w = np.float32((1 << 19) + 64)                                               # more than any lean launch can reach, the 64-frame build included
    assert np.float32(w + np.float32(1.0)) - w == 1 and w < np.float32(1 << 24)
    big = np.float32(1 << 24)
    assert np.float32(big + np.float32(1.0)) == big                              # where the argument would end
