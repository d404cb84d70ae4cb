"""Parity of the HIP dense RGB-D tracker (csrc/odometry.hip, through the C-ABI) against the CPU oracle
(oracle/onepiece_oracle.c, restating Odometry/DenseOdometryFunction.cpp + Odometry.cpp:621-687).

Bar: the projective association incl. the reference's source-indexed z-buffer is integer work ->
bit-exact pairs; poses within 1e-4 relative (north_star's ICP/tracking tolerance).  The reference
sums the normal equations sequentially in float; the HIP path sums the same float products in
double, so it is additionally compared (much tighter) with the oracle's double-accumulating
diagnostic mode, which isolates the reference's own rounding noise from real differences.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from onepiece_amd import odometry as O, integration as I
from helpers import track_levels, rel_err

POSE_TOL = 1e-4


@pytest.fixture(scope="module")
def odo():
    """A tracker in the fp64-reduction mode (what the tolerances of this module's step-by-step tests were set for; since round 6 a new tracker starts in the
    reference-order mode, OP_RUNTIME_OPT_TRACKER_DEFAULT_SUMS -- the tests of THAT mode create their own trackers or switch explicitly)."""
    t = O.Odometry(I.PinholeCamera("OPEN3D_DATASET"))
    t.SetSums("fp64")
    return t


def _perturb(T, k):
    from onepiece_amd import registration as R
    x = np.array([0.01, -0.006, 0.008, 0.004, -0.003, 0.005], np.float32) * k
    return (R.Se3ToSE3(x) @ T).astype(np.float32)


@pytest.mark.parametrize("scale,level", [(4, 0), (1, 0), (1, 2)])
def test_pixel_correspondences_bit_exact(oracle, odo, scale, level):
    levels, T_true = track_levels(100, 103, holes=True, scale=scale)
    lv = levels[level]
    for T in (np.eye(4, dtype=np.float32), T_true, _perturb(T_true, 1.0), _perturb(T_true, -4.0)):
        ref = oracle.pixel_correspondences(lv, T)
        got = odo.ComputeCorrespondencePixelWise(lv, T)
        assert len(ref) > 0.2 * lv["width"] * lv["height"]
        assert np.array_equal(got, ref)


def test_zbuffer_quirk_strip(oracle, odo):
    """The hand-checked 1x4 strip of tests/test_oracle_golden.py, on the GPU."""
    nan = np.float32(np.nan)
    lv = {"width": 4, "height": 1, "fx": 1.0, "fy": 1.0, "cx": 0.0, "cy": 0.0}
    z = np.zeros((1, 4), np.float32)
    for k in O.TRACK_IMAGES:
        lv[k] = z
    lv["source_depth"] = np.array([[1.0, 0.99, 1.01, nan]], np.float32)
    lv["target_depth"] = np.full((1, 4), 1.0, np.float32)
    T = np.eye(4, dtype=np.float32); T[0, 3] = -1.0
    assert odo.ComputeCorrespondencePixelWise(lv, T).tolist() == [[0, 0, 0, 0], [0, 1, 0, 0]]
    assert odo.ComputeCorrespondencePixelWise(lv, np.eye(4)).tolist() == oracle.pixel_correspondences(lv, np.eye(4)).tolist()


def test_long_dependency_chain(oracle, odo):
    """A fronto-parallel plane under a one-pixel sideways shift: every pixel's acceptance depends on its
    left neighbour's (equal depths -> 'existing > new' is false), i.e. a chain as long as the row."""
    W, H = 640, 8
    lv = {"width": W, "height": H, "fx": 500.0, "fy": 500.0, "cx": 320.0, "cy": 4.0}
    z = np.zeros((H, W), np.float32)
    for k in O.TRACK_IMAGES:
        lv[k] = z
    lv["source_depth"] = np.full((H, W), 2.0, np.float32)
    lv["target_depth"] = np.full((H, W), 2.0, np.float32)
    T = np.eye(4, dtype=np.float32); T[0, 3] = -2.0 / 500.0   # exactly one pixel to the left at z = 2
    ref = oracle.pixel_correspondences(lv, T)
    got = odo.ComputeCorrespondencePixelWise(lv, T)
    assert np.array_equal(got, ref)
    assert 0.4 * W * H < len(ref) < 0.6 * W * H              # alternating accept / reject along each row


@pytest.mark.parametrize("term", [0, 1, 2])
def test_single_iteration(oracle, odo, term):
    """One Gauss-Newton step at full resolution: identical pairs, xyz, and the updated pose."""
    levels, T_true = track_levels(100, 102, holes=True, scale=1)
    init = _perturb(T_true, 0.5)
    odo.SetMultiScale(1); odo.iter_count_per_level = [1]
    got = odo.MultiScaleComputing(levels[:1], init, term, want_log=True)
    ref = oracle.dense_track(levels[:1], (1,), term=term, init_T=init)
    assert got.iterations == 1 and got.per_iter_count[0] == ref["per_iter_count"][0]
    assert np.array_equal(got.pixel_correspondence_set, ref["pixel_correspondences"])
    assert rel_err(got.T, ref["T"]) <= POSE_TOL
    oracle.lib().orc_set_accumulate_double(1)
    try:
        ref_d = oracle.dense_track(levels[:1], (1,), term=term, init_T=init)
    finally:
        oracle.lib().orc_set_accumulate_double(0)
    assert rel_err(got.T, ref_d["T"]) <= 2e-6          # same float products, double sums on both sides
    assert abs(got.rmse - ref["rmse"]) <= 1e-4 * ref["rmse"]
    assert got.tracking_success == ref["tracking_success"]
    # correspondence_set: level-0 xyz of source AND target at the SOURCE pixel (Odometry.cpp:676-683)
    c = got.pixel_correspondence_set
    lv = levels[0]
    u, v = c[:, 1].astype(np.float32), c[:, 0].astype(np.float32)
    for k, img in ((0, lv["source_depth"]), (1, lv["target_depth"])):
        zz = img[c[:, 0], c[:, 1]]
        exp = np.stack([(u - np.float32(lv["cx"])) * zz / np.float32(lv["fx"]),
                        (v - np.float32(lv["cy"])) * zz / np.float32(lv["fy"]), zz], 1).astype(np.float32)
        exp[~(zz > 0)] = -1.0
        assert np.array_equal(got.correspondence_set[:, k].view(np.uint32), exp.view(np.uint32))


# (source, target, scale, term, strict): `strict` cases are well conditioned -> the plain 1e-4 bar.
# The others sit where the reference's own float accumulation noise is amplified by its association
# step (acceptance patterns flip with 1e-7 pose changes); there the bar is "no farther from the
# reference than the reference is from itself when it sums in double" (oracle diagnostic mode).
TRACK_CASES = [(300, 301, 1, 0, True), (500, 503, 1, 0, True), (100, 102, 4, 0, True), (300, 302, 2, 2, True),
               (300, 301, 1, 2, True), (300, 302, 2, 1, False), (100, 102, 2, 1, False), (100, 102, 2, 2, False),
               (100, 102, 1, 0, False)]


@pytest.mark.parametrize("i,j,scale,term,strict", TRACK_CASES)
def test_multi_scale_tracking(oracle, odo, i, j, scale, term, strict):
    levels, T_true = track_levels(i, j, holes=True, scale=scale)
    odo.SetMultiScale(3); odo.iter_count_per_level = [4, 8, 16]
    cam = I.PinholeCamera("OPEN3D_DATASET")
    cam.width, cam.height = levels[0]["width"], levels[0]["height"]
    odo.SetCamera(cam)
    got = odo.MultiScaleComputing(levels, None, term, want_log=True)
    ref = oracle.dense_track(levels, (4, 8, 16), term=term)
    oracle.lib().orc_set_accumulate_double(1)
    try:
        ref_d = oracle.dense_track(levels, (4, 8, 16), term=term)
    finally:
        oracle.lib().orc_set_accumulate_double(0)
    noise = rel_err(ref["T"], ref_d["T"])                  # the reference's own rounding noise
    bar = POSE_TOL if strict else max(POSE_TOL, 3.0 * noise)
    assert rel_err(got.T, ref["T"]) <= bar
    assert rel_err(got.T, ref_d["T"]) <= bar
    assert got.iterations == ref["iterations"]
    assert got.per_iter_count[0] == ref["per_iter_count"][0] == ref_d["per_iter_count"][0]
    n_pix = np.array([levels[2]["width"] * levels[2]["height"]] * 16 + [levels[1]["width"] * levels[1]["height"]] * 8 +
                     [levels[0]["width"] * levels[0]["height"]] * 4)[:got.iterations]
    dcount = np.abs(got.per_iter_count.astype(np.int64) - ref["per_iter_count"])
    assert np.all(dcount <= (1e-3 if strict else 3e-2) * n_pix + 2)
    assert got.tracking_success == ref["tracking_success"]
    assert abs(got.rmse - ref["rmse"]) <= (1e-3 if strict else 5e-2) * ref["rmse"]
    assert got.n_correspondences == got.per_iter_count[-1] == len(got.pixel_correspondence_set)
    # the tracker does recover the motion (sanity, loose: the reference's association is crude)
    assert np.abs(got.T - T_true).max() < 5e-3
    odo.SetCamera(I.PinholeCamera("OPEN3D_DATASET"))


@pytest.mark.parametrize("i,j,scale,term", [(100, 102, 1, 0), (300, 302, 2, 1), (500, 503, 2, 2)])
def test_teacher_forced_steps(oracle, odo, i, j, scale, term):
    """Every step of a whole coarse-to-fine run, without letting rounding noise accumulate: restart the
    GPU from the oracle's pose before iteration k (oracle in double-sum mode) and require the SAME
    correspondence count and the same updated pose after one step."""
    levels, _ = track_levels(i, j, holes=True, scale=scale)
    cam = I.PinholeCamera("OPEN3D_DATASET")
    cam.width, cam.height = levels[0]["width"], levels[0]["height"]
    odo.SetCamera(cam)
    oracle.lib().orc_set_accumulate_double(1)
    try:
        ref = oracle.dense_track(levels, (4, 8, 16), term=term)
    finally:
        oracle.lib().orc_set_accumulate_double(0)
    level_of = [2] * 16 + [1] * 8 + [0] * 4
    odo.SetMultiScale(1); odo.iter_count_per_level = [1]
    prev = np.eye(4, dtype=np.float32)
    worst = 0.0
    for k in range(ref["iterations"]):
        got = odo.MultiScaleComputing([levels[level_of[k]]], prev, term, want_correspondences=False, want_log=True)
        assert got.per_iter_count[0] == ref["per_iter_count"][k], k
        worst = max(worst, rel_err(got.T, ref["per_iter_T"][k]))
        prev = ref["per_iter_T"][k]
    assert worst <= 5e-6
    odo.SetCamera(I.PinholeCamera("OPEN3D_DATASET"))


def test_early_out_and_success_flags(oracle, odo):
    """Identity motion: ratio > 0.9 at level 0 stops after ONE iteration there (Odometry.cpp:669-670);
    ratios always divide by the full-resolution pixel count."""
    levels, _ = track_levels(100, 100, holes=False, scale=2)
    cam = I.PinholeCamera("OPEN3D_DATASET"); cam.width, cam.height = levels[0]["width"], levels[0]["height"]
    odo.SetCamera(cam); odo.SetMultiScale(3); odo.iter_count_per_level = [4, 8, 16]
    got = odo.MultiScaleComputing(levels, None, 0, want_log=True)
    ref = oracle.dense_track(levels, (4, 8, 16), term=0)
    assert ref["iterations"] == 16 + 8 + 1 and got.iterations == ref["iterations"]
    assert np.array_equal(got.per_iter_count, ref["per_iter_count"])
    assert got.tracking_success and ref["tracking_success"]
    # a camera twice as large as the images: ratio < 0.3 -> failure, no early-out
    cam.width, cam.height = 2 * levels[0]["width"], 2 * levels[0]["height"]
    odo.SetCamera(cam)
    got = odo.MultiScaleComputing(levels, None, 0)
    ref = oracle.dense_track(levels, (4, 8, 16), full_w=cam.width, full_h=cam.height, term=0)
    assert got.iterations == 28 == ref["iterations"] and not got.tracking_success and not ref["tracking_success"]
    odo.SetCamera(I.PinholeCamera("OPEN3D_DATASET"))


def test_device_resident_pyramids(odo):
    import torch
    levels, T_true = track_levels(100, 101, holes=True, scale=2)
    cam = I.PinholeCamera("OPEN3D_DATASET"); cam.width, cam.height = levels[0]["width"], levels[0]["height"]
    odo.SetCamera(cam); odo.SetMultiScale(3); odo.iter_count_per_level = [4, 8, 16]
    host = odo.MultiScaleComputing(levels, None, 0)
    dev_levels = []
    for lv in levels:
        d = dict(lv)
        for k in O.TRACK_IMAGES:
            d[k] = torch.from_numpy(np.ascontiguousarray(lv[k])).cuda()
        dev_levels.append(d)
    dev = odo.MultiScaleComputing(dev_levels, None, 0)
    assert np.array_equal(host.T, dev.T) and np.array_equal(host.pixel_correspondence_set, dev.pixel_correspondence_set)
    assert host.rmse == dev.rmse
    odo.SetCamera(I.PinholeCamera("OPEN3D_DATASET"))


def _room_pair(i, j, u16=False, holes=True):
    from onepiece_amd import synthetic as S
    out = []
    for k in (i, j):
        d, c, p = S.room_frame(k)
        d = d.copy()
        if holes:
            d[100:140, 200:300] = 0.0
            d[300:340, 80:140] = 7.5
            d[::37, ::29] = 0.2
        if u16:
            d = np.round(d * 1000.0).astype(np.uint16)
        out.append((d, c, p))
    return out


@pytest.mark.parametrize("u16", [False, True])
def test_dense_tracking_image_preparation(oracle, odo, u16):
    """op_tracker_dense_tracking's image preparation (conversion, 3x3 Gaussian, NormalizeIntensity,
    pyrDown, Sobel) against the oracle's restatement of the same definitions (NOT against OpenCV, which
    the reference does not vendor): depth pyramids bit-exact incl. NaN placement, colour within the
    float-vs-double summation difference of the NormalizeIntensity means."""
    (d1, c1, _), (d0, c0, _) = _room_pair(301, 300, u16=u16)
    odo.SetCamera(I.PinholeCamera("OPEN3D_DATASET")); odo.SetMultiScale(3); odo.iter_count_per_level = [4, 8, 16]
    got = odo.DenseTracking(c1, c0, d1, d0, None, 0)
    ref = oracle.dense_tracking(oracle.make_camera(), c1, c0, d1, d0, (4, 8, 16), 0, want_pyramids=True)
    P = ref["pyramids"]
    for level in range(3):
        for f, fname in ((0, "source"), (1, "target")):
            g = odo.ReadPyramid(f, 1, level)
            r = P[(fname, "depth", level)]
            assert np.array_equal(np.isnan(g), np.isnan(r))
            assert np.array_equal(g.view(np.uint32)[~np.isnan(r)], r.view(np.uint32)[~np.isnan(r)])
            # colour: identical up to ONE global factor per frame -- the NormalizeIntensity mean, which the
            # reference accumulates sequentially in float over ~3e5 pixels (off by ~6e-5 from the exact mean)
            gc, rc = odo.ReadPyramid(f, 0, level), P[(fname, "color", level)]
            ratio = np.median(gc / np.maximum(rc, 1e-6))
            assert abs(ratio - 1.0) <= 2e-4
            assert np.abs(gc - ratio * rc).max() <= 2e-6
        for kind, kname in ((4, "depth_dx"), (5, "depth_dy")):
            g, r = odo.ReadPyramid(1, kind, level), P[("target", kname, level)]
            assert np.array_equal(np.isnan(g), np.isnan(r))
            assert np.array_equal(g.view(np.uint32)[~np.isnan(r)], r.view(np.uint32)[~np.isnan(r)])
        for kind, kname in ((2, "color_dx"), (3, "color_dy")):
            g, r = odo.ReadPyramid(1, kind, level), P[("target", kname, level)]
            assert np.abs(g - r).max() <= 2e-4 * max(np.abs(r).max(), 1e-3) + 1e-6
    # and the tracking result itself
    assert got.iterations == ref["iterations"] and got.tracking_success == ref["tracking_success"]
    assert rel_err(got.T, ref["T"]) <= POSE_TOL


def test_dense_tracking_end_to_end(oracle, odo):
    """DenseTracking from raw colour/depth entirely on the GPU recovers the motion; device-resident raw
    frames give the same answer as host frames."""
    import torch
    (d1, c1, p1), (d0, c0, p0) = _room_pair(301, 300, holes=False)
    odo.SetCamera(I.PinholeCamera("OPEN3D_DATASET")); odo.SetMultiScale(3); odo.iter_count_per_level = [4, 8, 16]
    res = odo.DenseTracking(c1, c0, d1, d0, None, 0)
    T_true = np.linalg.inv(p0.astype(np.float64)) @ p1.astype(np.float64)
    assert res.tracking_success and np.abs(res.T - T_true).max() < 5e-3
    assert len(res.pixel_correspondence_set) == res.n_correspondences > 0.3 * 640 * 480
    tc = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dev = odo.DenseTracking(tc(c1), tc(c0), tc(d1), tc(d0), None, 0)
    assert np.array_equal(dev.T, res.T) and np.array_equal(dev.pixel_correspondence_set, res.pixel_correspondence_set)
    # feeding the pyramids the GPU just built back through the "pyramids given" entry point reproduces
    # the result exactly (same kernels, same inputs)
    again = odo.MultiScaleComputing(odo.PreparedLevels(), None, 0)
    assert np.array_equal(again.T, res.T) and np.array_equal(again.pixel_correspondence_set, res.pixel_correspondence_set)


def test_argument_errors(odo):
    from onepiece_amd import _lib as L
    levels, _ = track_levels(100, 101, holes=False, scale=4)
    odo.SetMultiScale(3); odo.iter_count_per_level = [4, 8, 16]
    with pytest.raises(L.OnePieceHipError):
        odo.MultiScaleComputing(levels, None, 7)
    odo.iter_count_per_level = [200, 100, 16]
    with pytest.raises(L.OnePieceHipError):
        odo.MultiScaleComputing(levels, None, 0)
    odo.iter_count_per_level = [4, 8, 16]


def test_dense_slam_pose_chain(oracle):
    """DenseSlam::UpdateFrame's tracking + pose chaining (DenseSlam.cpp:8-36) over a short synthetic
    sequence: the chained poses follow the oracle's chain (same per-pair DenseTracking, same
    global = global_last * T^-1) and stay near the ground-truth trajectory."""
    from onepiece_amd import dense_slam as DS, synthetic as S
    n = 8
    frames = [S.room_frame(600 + i) for i in range(n)]
    slam = DS.DenseSlam(I.PinholeCamera("OPEN3D_DATASET"))
    ref_poses = [np.eye(4, dtype=np.float32)]
    for i, (d, c, _p) in enumerate(frames):
        assert slam.UpdateFrame(c, d)
        if i:
            r = oracle.dense_tracking(oracle.make_camera(), frames[i - 1][1], c, frames[i - 1][0], d, (4, 8, 16), 0)
            assert r["tracking_success"]
            ref_poses.append(DS._mat4_mul_f32(ref_poses[-1], oracle.mat4_inverse(r["T"])))
    g0 = np.linalg.inv(frames[0][2].astype(np.float64))
    for i in range(n):
        assert rel_err(slam.global_poses[i], ref_poses[i]) <= 1e-3      # per-pair agreement is 1e-4..1e-3 (see TRACK_CASES)
        assert np.abs(np.asarray(slam.global_poses[i], np.float64) - g0 @ frames[i][2].astype(np.float64))[:3, 3].max() < 0.05  # odometry drift of the reference algorithm itself
    assert slam.last_tracking_frame_id == n - 1 and all(slam.tracking_success)


def test_degenerate_inputs(oracle, odo):
    """Edge cases the reference's loop meets: no valid depth at all (zero pairs -> singular normal
    equations -> pose untouched, rmse = 0/0 = NaN, failure), a single valid pixel, and zero iterations."""
    W, H = 64, 48
    lv = {"width": W, "height": H, "fx": 60.0, "fy": 60.0, "cx": 31.5, "cy": 23.5}
    z = np.zeros((H, W), np.float32)
    for k in O.TRACK_IMAGES:
        lv[k] = z
    lv["source_depth"] = np.full((H, W), np.nan, np.float32)
    lv["target_depth"] = np.full((H, W), 1.5, np.float32)
    cam = I.PinholeCamera("OPEN3D_DATASET"); cam.width, cam.height = W, H
    odo.SetCamera(cam); odo.SetMultiScale(1); odo.iter_count_per_level = [3]
    init = _perturb(np.eye(4, dtype=np.float32), 1.0)
    got = odo.MultiScaleComputing([lv], init, 0, want_log=True)
    ref = oracle.dense_track([lv], (3,), term=0, init_T=init)
    assert got.n_correspondences == 0 == len(ref["pixel_correspondences"]) and got.iterations == ref["iterations"] == 3
    assert np.array_equal(got.T, init) and np.array_equal(ref["T"], init)
    assert np.isnan(got.rmse) and np.isnan(ref["rmse"]) and not got.tracking_success and not ref["tracking_success"]
    # exactly one valid source pixel
    sd = lv["source_depth"].copy(); sd[20, 30] = 1.5
    lv["source_depth"] = sd
    got = odo.MultiScaleComputing([lv], None, 2)
    ref = oracle.dense_track([lv], (3,), term=2)
    assert got.pixel_correspondence_set.tolist() == ref["pixel_correspondences"].tolist() == [[20, 30, 20, 30]]
    assert rel_err(got.T, ref["T"]) <= POSE_TOL
    # zero iterations everywhere: nothing executed, empty result, pose = init
    odo.iter_count_per_level = [0]
    got = odo.MultiScaleComputing([lv], init, 0)
    ref = oracle.dense_track([lv], (0,), term=0, init_T=init)
    assert got.iterations == 0 == ref["iterations"] and got.n_correspondences == 0 and np.array_equal(got.T, init)
    assert not got.tracking_success and not ref["tracking_success"]
    odo.SetCamera(I.PinholeCamera("OPEN3D_DATASET"))


def test_pipelined_dense_slam_equals_sequential():
    """DenseSlam(pipeline=4): several frame pairs in flight on separate trackers/streams, resolved in order.
    Poses, flags and the order of the on_tracked callbacks are identical to the sequential loop -- also when a
    frame fails to track (a blank depth image), which invalidates the pairs speculatively enqueued after it."""
    import torch
    from onepiece_amd import dense_slam as DS, synthetic as S
    n = 14
    dev = torch.device("cuda", 0)
    depth, rgb, _poses = S.room_sequence_torch(200, n, dev)
    depth = depth.clone()
    depth[6] = 0.0                                     # frame 6 cannot be tracked; 7 must be tracked against 5
    cam = I.PinholeCamera("OPEN3D_DATASET")
    seen = {1: [], 4: []}
    runs = {}
    for p in (1, 4):
        slam = DS.DenseSlam(cam, pipeline=p, on_tracked=lambda fid, c, d, T, p=p: seen[p].append((fid, T.copy())))
        for i in range(n):
            slam.UpdateFrame(rgb[i], depth[i])
        slam.Finish()
        runs[p] = slam
    a, b = runs[1], runs[4]
    assert a.tracking_success == b.tracking_success and a.tracking_success[6] is False and all(a.tracking_success[:6]) and all(a.tracking_success[7:])
    assert a.last_tracking_frame_id == b.last_tracking_frame_id == n - 1
    for i in range(n):
        assert np.array_equal(a.global_poses[i], b.global_poses[i]), i
    assert [f for f, _ in seen[1]] == [f for f, _ in seen[4]] == [i for i in range(n) if i != 6]
    assert all(np.array_equal(x[1], y[1]) for x, y in zip(seen[1], seen[4]))


def test_pipelined_dense_slam_with_the_trackers_summing_together_equals_sequential():
    """test_pipelined_dense_slam_equals_sequential with OP_RUNTIME_OPT_TRACKER_BATCH_SUMS = 1 and twelve pairs in flight in the reference-order mode (the
    default): from twelve trackers running at the same time on, their per-iteration sequential sums are taken in one launch (seq_sums.hpp).  Poses, flags and
    callbacks equal the sequential chain's.  The option is silent: that twelve trackers DID meet in a given round depends on their threads' timing and is not
    observable from here -- what this pins is that results do not depend on whether they do."""
    import torch
    from onepiece_amd import dense_slam as DS, synthetic as S, _lib as L
    lib = L.load()
    n = 30
    dev = torch.device("cuda", 0)
    depth, rgb, _poses = S.room_sequence_torch(200, n, dev)
    depth = depth.clone()
    depth[6] = 0.0                                     # frame 6 cannot be tracked; 7 must be tracked against 5
    cam = I.PinholeCamera("OPEN3D_DATASET")
    seen = {1: [], 12: []}
    runs = {}
    for p in (1, 12):
        L.check(lib.op_runtime_set_option(L.OP_RUNTIME_OPT_TRACKER_BATCH_SUMS, 1 if p > 1 else 0))
        try:
            slam = DS.DenseSlam(cam, pipeline=p, on_tracked=lambda fid, c, d, T, p=p: seen[p].append((fid, T.copy())))
            slam.SetSums("reference_f32")
            for i in range(n):
                slam.UpdateFrame(rgb[i], depth[i])
            slam.Finish()
        finally:
            L.check(lib.op_runtime_set_option(L.OP_RUNTIME_OPT_TRACKER_BATCH_SUMS, 0))
        runs[p] = slam
    a, b = runs[1], runs[12]
    assert a.tracking_success == b.tracking_success and a.tracking_success[6] is False and all(a.tracking_success[:6]) and all(a.tracking_success[7:])
    assert a.last_tracking_frame_id == b.last_tracking_frame_id == n - 1
    for i in range(n):
        assert np.array_equal(a.global_poses[i], b.global_poses[i]), i
    assert [f for f, _ in seen[1]] == [f for f, _ in seen[12]] == [i for i in range(n) if i != 6]
    assert all(np.array_equal(x[1], y[1]) for x, y in zip(seen[1], seen[12]))


def test_dense_tracking_odd_image_size(oracle, odo):
    """Odd width/height: pyrDown targets (cols/2, rows/2), so 161x121 -> 80x60 -> 40x30; preparation and tracking
    agree with the oracle there too."""
    from onepiece_amd import synthetic as S
    w, h = 161, 121
    fx, fy, cx, cy = S.FX / 4, S.FY / 4, S.CX / 4, S.CY / 4
    frames = []
    for k in (300, 301):
        d, c = S.room_render(S.room_pose(k), width=w, height=h, fx=fx, fy=fy, cx=cx, cy=cy)
        d = d.copy(); d[30:45, 50:90] = 0.0
        frames.append((d, c))
    cam = I.PinholeCamera("OPEN3D_DATASET")
    cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height = fx, fy, cx, cy, w, h
    odo.SetCamera(cam); odo.SetMultiScale(3); odo.iter_count_per_level = [4, 8, 16]
    got = odo.DenseTracking(frames[1][1], frames[0][1], frames[1][0], frames[0][0], None, 0)
    ocam = oracle.make_camera(fx, fy, cx, cy, w, h)
    ref = oracle.dense_tracking(ocam, frames[1][1], frames[0][1], frames[1][0], frames[0][0], (4, 8, 16), 0, want_pyramids=True)
    for level, (lw, lh) in enumerate(((161, 121), (80, 60), (40, 30))):
        g, r = odo.ReadPyramid(1, 1, level), ref["pyramids"][("target", "depth", level)]
        assert g.shape == r.shape == (lh, lw)
        assert np.array_equal(np.isnan(g), np.isnan(r)) and np.array_equal(g.view(np.uint32)[~np.isnan(r)], r.view(np.uint32)[~np.isnan(r)])
        g, r = odo.ReadPyramid(1, 5, level), ref["pyramids"][("target", "depth_dy", level)]
        assert np.array_equal(np.isnan(g), np.isnan(r)) and np.array_equal(g.view(np.uint32)[~np.isnan(r)], r.view(np.uint32)[~np.isnan(r)])
    # the loop itself is covered elsewhere; at 40x30 pixels on the coarsest level a free run is in the regime where the
    # reference does not reproduce itself (see TRACK_CASES) -- here only that both land on the same motion
    assert got.iterations == ref["iterations"] and rel_err(got.T, ref["T"]) <= 1e-2
    odo.SetCamera(I.PinholeCamera("OPEN3D_DATASET"))


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_pixel_correspondences_fuzz(oracle, odo, seed):
    """Unstructured depth (noise, NaN speckle, steps) and random small motions: the acceptance chains become
    irregular (they jump between rows and stop at NaNs) -- pairs stay bit-identical to the oracle's raster-order loop."""
    rng = np.random.default_rng(seed)
    W, H = 213, 97
    lv = {"width": W, "height": H, "fx": 180.0 + seed, "fy": 175.0, "cx": 105.3, "cy": 47.9}
    z = np.zeros((H, W), np.float32)
    for k in O.TRACK_IMAGES:
        lv[k] = z
    base = (1.2 + 0.8 * rng.random((H, W))).astype(np.float32)
    base[:, W // 2:] += 0.5                                       # a depth step
    src = base + rng.normal(scale=0.01, size=(H, W)).astype(np.float32)
    tgt = base + rng.normal(scale=0.01, size=(H, W)).astype(np.float32)
    src[rng.random((H, W)) < 0.05] = np.nan
    tgt[rng.random((H, W)) < 0.05] = np.nan
    lv["source_depth"], lv["target_depth"] = src, tgt
    for trial in range(4):
        x = np.concatenate([rng.uniform(-0.03, 0.03, 3), rng.uniform(-0.02, 0.02, 3)]).astype(np.float32)
        T = oracle.se3_exp(x)
        ref = oracle.pixel_correspondences(lv, T)
        got = odo.ComputeCorrespondencePixelWise(lv, T)
        assert np.array_equal(got, ref) and len(ref) > 100


def test_chains_longer_than_the_lds_window(oracle, odo):
    """A fronto-parallel plane shifted by exactly one pixel UP at 640x480: every acceptance chain runs along its column
    (one link per row, up to 479 links), far beyond the rows a workgroup stages in LDS -- the global fallback of the walk."""
    W, H = 640, 480
    lv = {"width": W, "height": H, "fx": 500.0, "fy": 500.0, "cx": 320.0, "cy": 240.0}
    z = np.zeros((H, W), np.float32)
    for k in O.TRACK_IMAGES:
        lv[k] = z
    lv["source_depth"] = np.full((H, W), 2.0, np.float32)
    lv["target_depth"] = np.full((H, W), 2.0, np.float32)
    T = np.eye(4, dtype=np.float32); T[1, 3] = -2.0 / 500.0
    ref = oracle.pixel_correspondences(lv, T)
    got = odo.ComputeCorrespondencePixelWise(lv, T)
    assert np.array_equal(got, ref)
    assert 0.4 * W * H < len(ref) < 0.6 * W * H      # alternating accept / reject down every column
    # and a link that does not fit the 16-bit code: 110 rows up in one step (depth step makes the gate pass)
    T2 = np.eye(4, dtype=np.float32); T2[1, 3] = -110 * 2.0 / 500.0
    ref = oracle.pixel_correspondences(lv, T2)
    got = odo.ComputeCorrespondencePixelWise(lv, T2)
    assert np.array_equal(got, ref) and len(ref) > 0


@pytest.mark.parametrize("i,j,scale,term,strict", TRACK_CASES)
def test_multi_scale_tracking_with_reference_order_sums(oracle, i, j, scale, term, strict):
    """The validation mode OP_TRACK_SUMS_REFERENCE_F32 on ALL of TRACK_CASES, the ill-conditioned ones included: when every
    iteration's Jacobian rows (computed by the kernels) are summed sequentially in float32 like the reference's loop
    (DenseOdometryFunction.cpp:297-381), the whole free-running coarse-to-fine loop follows the CPU path step for step --
    identical correspondence counts at EVERY iteration, identical final pairs, poses to float rounding.  What the default
    (fp64) mode differs by on the relaxed cases is therefore the summation order alone."""
    levels, _ = track_levels(i, j, holes=True, scale=scale)
    odo = O.Odometry(I.PinholeCamera("OPEN3D_DATASET"))
    odo.SetSums("reference_f32")
    odo.SetMultiScale(3); odo.iter_count_per_level = [4, 8, 16]
    cam = I.PinholeCamera("OPEN3D_DATASET")
    cam.width, cam.height = levels[0]["width"], levels[0]["height"]
    odo.SetCamera(cam)
    got = odo.MultiScaleComputing(levels, None, term, want_log=True)
    ref = oracle.dense_track(levels, (4, 8, 16), term=term)
    assert got.iterations == ref["iterations"]
    assert np.array_equal(got.per_iter_count, ref["per_iter_count"])
    assert np.array_equal(got.pixel_correspondence_set, ref["pixel_correspondences"])
    assert rel_err(got.T, ref["T"]) <= 1e-6
    assert np.abs(got.per_iter_T - ref["per_iter_T"]).max() <= 1e-6
    assert got.tracking_success == ref["tracking_success"] and abs(got.rmse - ref["rmse"]) <= 1e-6 * max(ref["rmse"], 1e-9)


def test_dense_slam_pose_chain_with_reference_order_sums(oracle):
    """example/DenseFusion's tracking half over 12 frames with the validation mode: the chained poses equal the oracle's
    chain to 1e-5 (the image preparation and NormalizeIntensity run on the device in both modes; only the loop's sums differ)."""
    from onepiece_amd import dense_slam as DS, synthetic as S
    n = 12
    frames = [S.room_frame(600 + i) for i in range(n)]
    slam = DS.DenseSlam(I.PinholeCamera("OPEN3D_DATASET"))
    slam.rgbd_odometry.SetSums("reference_f32")
    ref_poses = [np.eye(4, dtype=np.float32)]
    for k, (d, c, _p) in enumerate(frames):
        assert slam.UpdateFrame(c, d)
        if k:
            r = oracle.dense_tracking(oracle.make_camera(), frames[k - 1][1], c, frames[k - 1][0], d, (4, 8, 16), 0)
            ref_poses.append(DS._mat4_mul_f32(ref_poses[-1], oracle.mat4_inverse(r["T"])))
    err = max(rel_err(slam.global_poses[k], ref_poses[k]) for k in range(n))
    assert err <= 1e-5, err


def test_device_sequential_sums_equal_the_host_loop_bit_for_bit():
    """OP_TRACK_SUMS_REFERENCE_F32 sums on the device (k_seq_sums: one wave owns the 36 + 6 float32 accumulators and walks the compacted rows in
    raster order); OP_TRACK_SUMS_REFERENCE_F32_HOST brings all rows to the host and runs the reference's loop there.  Same operands in the same
    order: every per-iteration pose is bit-identical, for the hybrid, photometric and geometric terms (2 / 1 / 1 rows per pixel), on levels whose
    row counts are not multiples of the tile size, and end to end from raw frames (NormalizeIntensity's two sequential means included)."""
    from onepiece_amd import synthetic as S
    for (i, j, scale, term) in ((100, 102, 1, 0), (300, 301, 2, 1), (640, 643, 2, 2), (10, 11, 4, 0)):
        levels, _ = track_levels(i, j, holes=True, scale=scale)
        out = {}
        for sums in ("reference_f32", "reference_f32_host"):
            odo = O.Odometry(I.PinholeCamera("OPEN3D_DATASET"))
            odo.SetSums(sums)
            odo.SetMultiScale(3); odo.iter_count_per_level = [4, 8, 16]
            cam = I.PinholeCamera("OPEN3D_DATASET")
            cam.width, cam.height = levels[0]["width"], levels[0]["height"]
            odo.SetCamera(cam)
            out[sums] = odo.MultiScaleComputing(levels, None, term, want_log=True)
        a, b = out["reference_f32"], out["reference_f32_host"]
        assert a.iterations == b.iterations and np.array_equal(a.per_iter_count, b.per_iter_count), (i, j, term)
        assert np.array_equal(np.asarray(a.per_iter_T).view(np.uint32), np.asarray(b.per_iter_T).view(np.uint32)), (i, j, term)
        assert np.array_equal(np.asarray(a.T).view(np.uint32), np.asarray(b.T).view(np.uint32))
    d0, c0, _ = S.room_frame(600); d1, c1, _ = S.room_frame(601)
    res = {}
    for sums in ("reference_f32", "reference_f32_host"):
        odo = O.Odometry(I.PinholeCamera("OPEN3D_DATASET"))
        odo.SetSums(sums)
        res[sums] = odo.DenseTracking(c1, c0, d1, d0, None, 0)
    assert np.array_equal(np.asarray(res["reference_f32"].T).view(np.uint32), np.asarray(res["reference_f32_host"].T).view(np.uint32))
    assert res["reference_f32"].iterations == res["reference_f32_host"].iterations
