"""The image preparation of op_tracker_dense_tracking (odometry_prep.hip and the preparation part of odometry.hip): grey and depth
conversion, 3x3 Gaussian, NormalizeIntensity in all three sums modes, pyrDown and Sobel -- image for image and bit for bit against
the CPU oracle, at the smallest and most awkward shapes the entry accepts, on inputs that cover the conversions' edges (helpers.prep_*),
plus one check of the definitions that does not use the oracle's filters at all (float64, scipy), and a tracker that is replayed and
reused against fresh ones.

Every level gets ONE iteration: the preparation is complete before the loop starts, and nothing here asserts a pose the loop computed
(at these sizes the loop is in the regime TRACK_CASES of test_odometry_gpu.py documents).  Everything is bit equality except the two
derived bounds of part 4."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from onepiece_amd import odometry as O, integration as I
from helpers import prep_pair

# (w, h, levels) against the 32x8 blur tile, the 256-thread pyrDown / Sobel groups and the entry's limits
SHAPES = [(4, 4, 1),        # the minimum
          (7, 13, 2),       # level 1 is 3x6, both sizes odd
          (31, 7, 1),       # one partial tile
          (32, 8, 1),       # exactly one tile
          (33, 9, 2),       # one pixel into the next tile on both axes
          (64, 16, 3),      # whole tiles, multiples of 256 at levels 0 and 1
          (100, 52, 4),     # the deepest pyramid that stays >= 3 pixels: 12x6 at the top
          (161, 121, 3)]    # the odd case of test_dense_tracking_odd_image_size, for colour this time
U16_SHAPES = [(33, 9, 2), (64, 16, 3), (100, 52, 4)]
FP64_SHAPES = [(33, 9, 2), (100, 52, 4), (161, 121, 3)]
KINDS = ("color", "depth", "color_dx", "color_dy", "depth_dx", "depth_dy")


def _intrinsics(w, h):
    return float(max(w, h)), float(max(w, h)), (w - 1) / 2.0, (h - 1) / 2.0


def _camera(w, h, depth_scale=1000.0):
    cam = I.PinholeCamera("OPEN3D_DATASET")
    cam.fx, cam.fy, cam.cx, cam.cy = _intrinsics(w, h)
    cam.width, cam.height, cam.depth_scale = w, h, depth_scale
    return cam


def _tracker(sums):
    odo = O.Odometry(I.PinholeCamera("OPEN3D_DATASET"))
    odo.SetSums(sums)
    return odo


def _images(odo, levels):
    return {(fname, KINDS[kind], l): odo.ReadPyramid(f, kind, l)
            for l in range(levels) for f, fname in enumerate(("source", "target")) for kind in range(6) if f == 1 or kind < 2}


def _to_device(a):
    import torch
    if a.dtype == np.uint16:
        a = a.view(np.int16)        # same bits; the entry takes either 16-bit type
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _track(odo, w, h, levels, frames, depth_scale=1000.0, init_T=None, device=False, points=True, keep=None):
    """One DenseTracking call with one iteration per level -> (result, every prepared image).  keep: a list that takes the device copies
    of the frames, so that the next call's copies cannot land on the same addresses."""
    odo.SetCamera(_camera(w, h, depth_scale))
    odo.SetMultiScale(levels)
    odo.iter_count_per_level = [1] * levels
    if device:
        frames = [_to_device(a) for a in frames]
        if keep is not None:
            keep.extend(frames)
    res = odo.DenseTracking(frames[0], frames[1], frames[2], frames[3], init_T, 0, want_points=points)
    return res, _images(odo, levels)


_REF = {}


def _case(oracle, w, h, levels, u16_scale=None, seed=None):
    """Frames and the oracle's run of them, computed once per case and read-only afterwards."""
    key = (w, h, levels, u16_scale, seed)
    if key not in _REF:
        frames = prep_pair(w, h, 1000 * w + h if seed is None else seed, u16_scale)
        ocam = oracle.make_camera(*_intrinsics(w, h), w, h, 1000.0 if u16_scale is None else float(u16_scale))
        ref = oracle.dense_tracking(ocam, *frames, iters=(1,) * levels, term=0, want_pyramids=True)
        for a in list(frames) + list(ref["pyramids"].values()):
            a.setflags(write=False)
        _REF[key] = (frames, ref)
    return _REF[key]


def _same_bits(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float32, what
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), "%s: NaN at %d pixels, reference at %d" % (what, gn.sum(), rn.sum())
    bad = (got.view(np.uint32) != ref.view(np.uint32)) & ~rn
    assert not bad.any(), "%s: %d of %d pixels differ, first at %s: %r != %r" % (
        what, bad.sum(), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], ref[bad][0])


def _all_same_bits(got, ref, what, only=None):
    for key in sorted(got):
        if only is None or key[1] in only:
            _same_bits(got[key], ref[key], "%s %s" % (what, key))


def _has_pairs(ref):
    """The condition of every case but the 'no pairs' one: the oracle found identity-pose pairs, so its normalisation is finite."""
    P = ref["pyramids"]
    return bool(np.isfinite(P[("source", "color", 0)]).all() and np.isfinite(P[("target", "color", 0)]).all())


# ---- 1. reference-order modes: every prepared image equals the oracle bit for bit ----------------------------------------------
REF_ORDER_CASES = [(w, h, lv, None) for (w, h, lv) in SHAPES] + [(w, h, lv, s) for (w, h, lv) in U16_SHAPES for s in (1000, 5000)]


@pytest.mark.parametrize("w,h,levels,u16_scale", REF_ORDER_CASES)
def test_reference_order_images_equal_the_oracle_bit_for_bit(oracle, w, h, levels, u16_scale):
    """reference_f32, the mode a new tracker starts in: NormalizeIntensity sums the same floats in the same order as
    orc_normalize_intensity (k_rows_count, k_emit_scan, k_norm_pairs_compact, k_seq_sums<kSeqTwoValues>, host division), so colour, depth
    and all four gradient images are the oracle's at every level -- identical NaN placement, identical bits elsewhere."""
    frames, ref = _case(oracle, w, h, levels, u16_scale)
    assert _has_pairs(ref)
    got, imgs = _track(_tracker("reference_f32"), w, h, levels, frames, 1000.0 if u16_scale is None else float(u16_scale))
    _all_same_bits(imgs, ref["pyramids"], "%dx%d" % (w, h))
    assert got.iterations == ref["iterations"]


def test_host_order_images_equal_the_oracle_bit_for_bit(oracle):
    """reference_f32_host: the two means come from the host loop in odometry.hip instead of k_seq_sums."""
    w, h, levels = 33, 9, 2
    frames, ref = _case(oracle, w, h, levels)
    assert _has_pairs(ref)
    got, imgs = _track(_tracker("reference_f32_host"), w, h, levels, frames)
    _all_same_bits(imgs, ref["pyramids"], "%dx%d host" % (w, h))
    assert got.iterations == ref["iterations"]


# ---- 2. fp64 mode: colour pinned to one rounding of the scale -------------------------------------------------------------------
def _blurred(oracle, frames, depth_scale):
    """Un-normalised blurred intensity and blurred NaN depth of both frames (oracle building blocks)."""
    cs, ct, ds, dt = frames
    grey = [oracle.prep_blur3(oracle.prep_intensity(c)) for c in (cs, ct)]
    depth = [oracle.prep_blur3(oracle.prep_depth_nan(d, depth_scale)) for d in (ds, dt)]
    return grey, depth


def _identity_pairs(oracle, w, h, depth):
    z = np.zeros((h, w), np.float32)
    lv = dict(zip(("fx", "fy", "cx", "cy"), _intrinsics(w, h)), width=w, height=h)
    for k in O.TRACK_IMAGES:
        lv[k] = z
    lv["source_depth"], lv["target_depth"] = depth
    return oracle.pixel_correspondences(lv, np.eye(4, dtype=np.float32))


def _scale_candidates(values):
    """k_norm_scales' f32(0.5 / f64(f32(sum) / f32(n))) for the exactly rounded sum and its two float32 neighbours: the device's double
    partial sums may round the other way when the sum sits on a float32 boundary, and that is the only freedom."""
    s = np.float32(math.fsum(values.astype(np.float64).tolist()))
    n = np.float32(len(values))
    with np.errstate(invalid="ignore", divide="ignore"):
        return [np.float32(0.5 / np.float64(np.float32(S) / n)) for S in (s, np.nextafter(s, np.float32(-np.inf)), np.nextafter(s, np.float32(np.inf)))]


def _fit_scale(dev, blurred, cands, what):
    """The candidate for which blurred * s + 0.0f IS the device image; no ratio is fitted."""
    for s in cands:
        exp = blurred * s + np.float32(0.0)
        if np.array_equal(exp.view(np.uint32), dev.view(np.uint32)):
            return s
    worst = [float(np.abs(blurred * s + np.float32(0.0) - dev).max()) for s in cands]
    pytest.fail("%s: no candidate scale %r reproduces the device image (max abs difference per candidate %r)" % (what, cands, worst))


def _fp64_scales(oracle, w, h, frames, imgs, depth_scale=1000.0):
    grey, depth = _blurred(oracle, frames, depth_scale)
    pairs = _identity_pairs(oracle, w, h, depth)
    assert len(pairs) > 0
    s_s = _fit_scale(imgs[("source", "color", 0)], grey[0], _scale_candidates(grey[0][pairs[:, 0], pairs[:, 1]]), "source colour")
    s_t = _fit_scale(imgs[("target", "color", 0)], grey[1], _scale_candidates(grey[1][pairs[:, 2], pairs[:, 3]]), "target colour")
    return s_s, s_t


@pytest.mark.parametrize("w,h,levels", FP64_SHAPES)
def test_fp64_colour_is_one_rounding_of_the_scale(oracle, w, h, levels):
    """fp64 mode (k_norm_scales): depth and depth gradients are the oracle's bits.  Level-0 colour is blurred * s + 0.0f bit for bit, with
    s formed as k_norm_scales does from the float64 sums (math.fsum) of the source intensities at the source pixels and the target
    intensities at the PAIRED target pixels of the identity-pose pairs.  Once the scale is fixed nothing else may differ: the higher
    colour levels and the colour gradients are the oracle's pyrDown / Sobel of the DEVICE's level-0 colour, bit for bit."""
    frames, ref = _case(oracle, w, h, levels)
    assert _has_pairs(ref)
    got, imgs = _track(_tracker("fp64"), w, h, levels, frames)
    _all_same_bits(imgs, ref["pyramids"], "%dx%d" % (w, h), only=("depth", "depth_dx", "depth_dy"))
    assert got.iterations == ref["iterations"]
    _fp64_scales(oracle, w, h, frames, imgs)
    for f in ("source", "target"):
        for l in range(1, levels):
            _same_bits(imgs[(f, "color", l)], oracle.prep_pyrdown(imgs[(f, "color", l - 1)]), "%s colour level %d" % (f, l))
    for l in range(levels):
        for axis, name in enumerate(("color_dx", "color_dy")):
            _same_bits(imgs[("target", name, l)], oracle.prep_sobel(imgs[("target", "color", l)], axis), "%s level %d" % (name, l))


# ---- 3. no correspondences --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sums", ["reference_f32", "fp64"])
def test_no_correspondences_then_a_normal_pair(oracle, sums):
    """Blank depth in both frames, then in the target alone: no identity-pose pair, both means 0/0.  Colour and colour gradients are NaN
    exactly where the oracle's are, depth is the oracle's, tracking fails, the pose stays the initial one.  A normal pair on the SAME
    tracker afterwards gives the bits of a fresh tracker: no NaN scale and no stale count survives."""
    w, h, levels = 16, 8, 1
    frames, normal = _case(oracle, w, h, levels)
    assert _has_pairs(normal)
    cs, ct, ds, dt = frames
    blank = np.zeros((h, w), np.float32)
    init = oracle.se3_exp(np.array([0.01, -0.006, 0.008, 0.004, -0.003, 0.005], np.float32))
    ocam = oracle.make_camera(*_intrinsics(w, h), w, h, 1000.0)
    odo = _tracker(sums)
    for what, sd in (("both blank", blank), ("target blank", ds)):
        ref = oracle.dense_tracking(ocam, cs, ct, sd, blank, iters=(1,), term=0, init_T=init, want_pyramids=True)
        assert np.isnan(ref["pyramids"][("source", "color", 0)]).all() and np.isnan(ref["pyramids"][("target", "color", 0)]).all()
        got, imgs = _track(odo, w, h, levels, (cs, ct, sd, blank), init_T=init)
        _all_same_bits(imgs, ref["pyramids"], what)
        assert not got.tracking_success and not ref["tracking_success"]
        assert np.array_equal(got.T.view(np.uint32), init.view(np.uint32)) and np.array_equal(ref["T"].view(np.uint32), init.view(np.uint32))
        assert got.iterations == ref["iterations"]
    got, imgs = _track(odo, w, h, levels, frames)
    fresh, fresh_imgs = _track(_tracker(sums), w, h, levels, frames)
    _all_same_bits(imgs, fresh_imgs, "after the blank pairs")
    assert np.array_equal(got.T.view(np.uint32), fresh.T.view(np.uint32)) and got.iterations == fresh.iterations
    assert np.array_equal(got.pixel_correspondence_set, fresh.pixel_correspondence_set)
    if sums == "reference_f32":
        _all_same_bits(imgs, normal["pyramids"], "after the blank pairs, against the oracle")


# ---- 4. independent float64 check of the definitions ----------------------------------------------------------------------------
BLUR = np.array([0.25, 0.5, 0.25])
PYR = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
SOBEL_D, SOBEL_S = np.array([-1.0, 0.0, 1.0]), np.array([1.0, 2.0, 1.0])


def _check_filter(ndi, dev, inp, kx, ky, what, half=False):
    """dev against the separable filter (kx along rows, then ky along columns, reflect-101 = scipy's `mirror`) of inp in float64.
    NaN exactly where any tap of the window is NaN (zero-weight taps included); elsewhere within the bound of the module's part 4."""
    nan = np.isnan(inp)
    x = np.where(nan, 0.0, inp.astype(np.float64))
    ref = ndi.correlate1d(ndi.correlate1d(x, kx, axis=1, mode="mirror"), ky, axis=0, mode="mirror")
    ref_nan = ndi.maximum_filter(nan.astype(np.uint8), size=(len(ky), len(kx)), mode="mirror").astype(bool)
    if half:
        h, w = inp.shape
        ref, ref_nan = ref[0:2 * (h // 2):2, 0:2 * (w // 2):2], ref_nan[0:2 * (h // 2):2, 0:2 * (w // 2):2]
    assert dev.shape == ref.shape, what
    assert np.array_equal(np.isnan(dev), ref_nan), "%s: NaN placement" % what
    top = float(np.abs(x).max())
    bound = (len(kx) + len(ky)) * 2.0 ** -23 * np.abs(kx).sum() * np.abs(ky).sum() * top
    err = np.abs(dev.astype(np.float64) - ref)[~ref_nan]
    print("%s: max error %.3g, bound %.3g" % (what, err.max(initial=0.0), bound))
    assert err.max(initial=0.0) <= bound, "%s: error %g exceeds %g" % (what, err.max(), bound)


@pytest.mark.parametrize("w,h,levels,u16_scale", [(33, 9, 2, None), (100, 52, 4, None), (64, 16, 3, 5000)])
def test_definitions_against_float64_filters(oracle, w, h, levels, u16_scale):
    """Oracle and kernels were written from one reading of reflect-101, the taps and the grey weights; this check shares none of it.  The
    raw frames are converted in numpy and filtered with scipy.ndimage.correlate1d(mode="mirror") in float64, rows then columns; every
    stage takes the DEVICE's image of the stage before as its exact input, so each comparison sees one filter's rounding only.

    Grey.  The candidate preimage Y / 255 (Y from the oracle's fixed-point formula, accepted only if float32(Y) / 255.0f reproduces it) must
    satisfy |Y - (0.299 R + 0.587 G + 0.114 B)| <= 0.5 + e, e = 255 * sum |c_i - C_i / 2^14| over the three 14-bit coefficients: 0.5 for
    the rounding to an integer, e for the most the coefficients' own error can move the sum over the byte range.  Evaluated in integers.

    Filters.  A pass with n taps forms n products and n - 1 sums, each rounded once to float32 (relative error <= 2^-24) and each bounded
    by S |k| * max |x|: the pass is off by at most (2n - 1) * 2^-24 * S |k| * max |x|.  The second pass multiplies the first's error by
    S |ky| and adds its own on values bounded by S |kx| * max |x|, hence
        |err| <= (nx + ny) * 2^-23 * S |kx| * S |ky| * max |finite input|
    with 2 * 2^-24 * S |kx| S |ky| max |x| to spare, which covers the second-order terms, the float64 reference's own rounding, and the one
    extra float32 rounding of the stages that convert as well (u16 / depth_scale; intensity * scale).  Fused multiply-adds only remove
    roundings.  A wrong tap or border index is off by a fraction of max |x|: four orders of magnitude more."""
    ndi = pytest.importorskip("scipy.ndimage")
    depth_scale = 1000.0 if u16_scale is None else float(u16_scale)
    frames, ref = _case(oracle, w, h, levels, u16_scale)
    assert _has_pairs(ref)
    got, imgs = _track(_tracker("fp64"), w, h, levels, frames, depth_scale)
    # grey
    coeff, fixed = np.array([0.299, 0.587, 0.114]), np.array([4899, 9617, 1868])
    e = 255.0 * np.abs(coeff - fixed / 16384.0).sum()
    assert e <= 0.02
    grey = []
    for c in frames[:2]:
        cand = oracle.prep_intensity(c)
        G = np.rint(cand.astype(np.float64) * 255.0)
        assert np.array_equal((G.astype(np.float32) / np.float32(255.0)).view(np.uint32), cand.view(np.uint32))
        exact1000 = c.astype(np.int64) @ np.array([299, 587, 114])                      # 1000 * (0.299 R + 0.587 G + 0.114 B), exact
        worst = np.abs(1000 * G.astype(np.int64) - exact1000).max() / 1000.0
        print("grey: max |G - exact| = %.4f, bound %.4f" % (worst, 0.5 + e))
        assert worst <= 0.5 + e
        grey.append(cand)
    # depth validity in float64
    raw = []
    for d in frames[2:]:
        d64 = d.astype(np.float64)
        if u16_scale is None:
            valid = (d64 > 0.5) & (d64 < 4.0)
            raw.append(np.where(valid, d64, np.nan))
        else:
            valid = (d64 > 0.5 * depth_scale) & (d64 < 4.0 * depth_scale)
            raw.append(np.where(valid, d64 / depth_scale, np.nan))
    s = _fp64_scales(oracle, w, h, frames, imgs, depth_scale)
    for k, f in enumerate(("source", "target")):
        _check_filter(ndi, imgs[(f, "depth", 0)], raw[k], BLUR, BLUR, "%s depth blur" % f)
        unscaled = imgs[(f, "color", 0)].astype(np.float64) / np.float64(s[k])      # the scale of part 2 divided out
        _check_filter(ndi, unscaled, grey[k], BLUR, BLUR, "%s colour blur" % f)
        for l in range(1, levels):
            for kind in ("depth", "color"):
                _check_filter(ndi, imgs[(f, kind, l)], imgs[(f, kind, l - 1)], PYR, PYR, "%s %s pyrDown to level %d" % (f, kind, l), half=True)
    for l in range(levels):
        for kind in ("depth", "color"):
            _check_filter(ndi, imgs[("target", kind + "_dx", l)], imgs[("target", kind, l)], SOBEL_D, SOBEL_S, "%s d/dx level %d" % (kind, l))
            _check_filter(ndi, imgs[("target", kind + "_dy", l)], imgs[("target", kind, l)], SOBEL_S, SOBEL_D, "%s d/dy level %d" % (kind, l))


# ---- 5. replay and reuse against a fresh tracker ------------------------------------------------------------------------------------
def _reuse_calls(names):
    p1, p2 = prep_pair(64, 48, 501), prep_pair(64, 48, 502)
    p2_u16 = p2[:2] + prep_pair(64, 48, 502, 1000)[2:]
    calls = {"P1": (64, 48, 3, p1), "P2 (replay: new pointers and contents)": (64, 48, 3, p2),
             "96x64 (new key, larger buffers)": (96, 64, 3, prep_pair(96, 64, 503)),
             "P1 again (captured anew into the larger buffers)": (64, 48, 3, p1),
             "P2 as u16": (64, 48, 3, p2_u16), "P2 with two levels": (64, 48, 2, p2)}
    return [(n, calls[n]) for n in calls if names is None or n in names]


@pytest.mark.parametrize("sums,steps", [("fp64", None), ("reference_f32", ("P1", "P2 (replay: new pointers and contents)",
                                                                           "P1 again (captured anew into the larger buffers)"))])
def test_replayed_and_reused_tracker_equals_a_fresh_one(sums, steps):
    """One tracker fed device-resident frames (no xyz pairs asked for: in fp64 mode the launches are captured into a graph on the first
    call and replayed while the key holds; frame pointers travel through prep_dev) through a change of contents, of shape, back, of depth
    format and of level count.  After every call all prepared images, T, iterations and the pixel pairs are the bits of a FRESH tracker
    given the same call with host frames, so the comparison also crosses the upload path.  reference_f32: the same on the path that is
    never captured."""
    a = _tracker(sums)
    held = []       # every call's device frames stay alive: a replay that read the previous call's pointers would read the previous frames
    for name, (w, h, levels, frames) in _reuse_calls(steps):
        got, imgs = _track(a, w, h, levels, frames, device=True, points=False, keep=held)
        b = _tracker(sums)
        ref, ref_imgs = _track(b, w, h, levels, frames, points=False)
        del b
        assert sorted(imgs) == sorted(ref_imgs)
        _all_same_bits(imgs, ref_imgs, name)
        assert np.array_equal(got.T.view(np.uint32), ref.T.view(np.uint32)), name
        assert got.iterations == ref.iterations, name
        assert got.tracking_success == ref.tracking_success, name
        assert len(ref.pixel_correspondence_set) > 0 and np.array_equal(got.pixel_correspondence_set, ref.pixel_correspondence_set), name
