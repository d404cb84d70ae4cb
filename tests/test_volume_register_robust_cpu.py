"""The linearisations and Huber weights of op_volume_register_robust_* without a device: the numpy restatement of the definition
(tests/volume_register_robust_common.py) on hand-made fields where rows and sums have a closed form, the restated Gauss-Newton loop against the
TRUTH on the clouds where the NORMAL linearisation zig-zags, and what of the entries needs no device -- the refusals, the bindings, the struct
sizes, the class surface.

The model of the convergence cases: the room through D.frames(D.CAM_64, 40, stride=5) into 2 cm voxels, truncation 0.1, fused by the oracle.  A
cloud is one frame's hit points in world coordinates (3072 points); the true transformation is the identity; the start is D.perturbed(identity, 1),
41.8 mm / 0.97 degrees off; min_step 1e-5, max_distance 0.1.  The measured figures are in the docstrings of the tests."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import volume_register_color_common as K
import volume_register_common as R
import volume_register_robust_common as B
import volume_sample_common as S

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "host", "one_piece")
NAMES = ("op_volume_register_robust_default_options", "op_volume_register_robust_system", "op_volume_register_robust_points",
         "op_volume_register_robust_frame")
EYE = np.eye(4, dtype=F32)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def test_slope_one_field_all_modes_give_the_existing_closed_form():
    """s = z - Z0: |grad s| = 1, so the three linearisations are the same system, R.rows_of's"""
    grid = S.Grid(R.HAND_KEYS, R.hand_blocks(), R.HAND_RES)
    pts = R.hand_cloud()
    rows8, reason8 = R.rows_of(grid, pts, EYE, 0.1)
    gsums, _m, gcounts = R.fold(rows8, reason8)
    assert all(gcounts[k] > 0 for k in R.COUNT_NAMES)
    for mode in (B.NORMAL, B.GRADIENT, B.METRIC):
        w = B.rows_of(grid, pts, None, EYE, 0.1, mode=mode)
        assert np.array_equal(w["reason"], reason8)
        assert np.array_equal(_bits(w["rows"][:, :8]), _bits(rows8)) and not w["rows"][:, 8:].any(), mode
        sums, _b, counts = B.fold(w)
        assert np.array_equal(sums[:28], gsums) and sums[28] == 0 and sums[29] == gsums[27] == sums[30], mode
        assert counts == dict(gcounts, colored=0, downweighted=0, color_downweighted=0), mode
    used = reason8 == 0
    p = pts[used]
    z = np.zeros(len(p), F32)
    assert np.array_equal(rows8[used], np.stack([z, z, z + 1, p[:, 1], -p[:, 0], z, p[:, 2] - F32(R.HAND_Z0), z + 1], axis=1))


def _steep(color=False):
    return S.Grid(R.HAND_KEYS, B.steep_blocks(color), R.HAND_RES)


def test_slope_two_field_closed_form_per_mode():
    """s = 2 (z - Z0) on the same blocks: d = (0, 0, 2 res), n = (0, 0, 1), |grad s| = 2, everything dyadic.  max_distance 0.1 gates the stored
    sdf: R.HAND_POINTS keep their reasons (|s| = 1/32 and 3/32 are used, 3/8 is too far)."""
    grid = _steep()
    pts = R.hand_cloud()
    want = None
    for mode in (B.NORMAL, B.GRADIENT, B.METRIC):
        w = B.rows_of(grid, pts, None, EYE, 0.1, mode=mode)
        for i, (what, _p, reason) in enumerate(R.HAND_POINTS):
            assert w["reason"][i] == reason, (what, int(w["reason"][i]))
        used = w["reason"] == 0
        p = pts[used]
        z = np.zeros(len(p), F32)
        dz = p[:, 2] - F32(R.HAND_Z0)
        unit = np.stack([z, z, z + 1, p[:, 1], -p[:, 0], z], axis=1)
        row, r = {B.NORMAL: (unit, 2 * dz), B.GRADIENT: (2 * unit, 2 * dz), B.METRIC: (unit, dz)}[mode]
        assert np.array_equal(w["rows"][used, :6], row) and np.array_equal(w["rows"][used, 6], r) and (w["rows"][used, 7] == 1).all(), mode
        assert not w["rows"][~used].any() and not w["rows"][:, 8:].any()
        assert np.array_equal(w["s"][used], 2 * dz) and np.array_equal(w["r"][used], r)
        sums, _b, counts = B.fold(w)
        d = lambda v: v.astype(np.float64)
        closed = [np.sum(d(row[:, a]) * d(row[:, b])) for a, b in R.PAIRS] + [np.sum(d(r) * d(row[:, a])) for a in range(6)]
        closed += [np.sum(d(r) ** 2), 0.0, np.sum(d(2 * dz) ** 2), np.sum(d(r) ** 2)]
        assert np.array_equal(sums, np.array(closed)), mode                # dyadic terms of a few bits: every sum is exact
        assert all(counts[k] > 0 for k in R.COUNT_NAMES) and counts["downweighted"] == 0
        want = want or counts
        assert counts == want, mode                                        # the USED set does not depend on the linearisation


HUBER = 1 / 64


def _huber_points():
    """x = y = -1/8 (deep inside the blocks below the origin), r = z - Z0 = k / 128 for k in KS: below the threshold 1/64, at it, above, at 4 x"""
    ks = np.array([1, -1, 2, -2, 3, -3, 8, -8, 0], np.float64)
    return ks, np.stack([np.full(len(ks), -0.125), np.full(len(ks), -0.125), R.HAND_Z0 + ks / 128.0], axis=1).astype(F32)


def test_huber_closed_form():
    """METRIC on the slope-two field, huber = 1/64: |r| = 1/128 and 1/64 keep w = 1, 3/128 gets w = 2/3, 1/16 gets exactly w = 1/4, q = 1/2"""
    grid = _steep()
    ks, pts = _huber_points()
    plain = B.rows_of(grid, pts, None, EYE, 0.2, mode=B.METRIC)
    assert (plain["reason"] == 0).all() and np.array_equal(plain["r"], (ks / 128.0).astype(F32))
    w = B.rows_of(grid, pts, None, EYE, 0.2, mode=B.METRIC, huber=HUBER)
    assert w["down"].tolist() == [False, False, False, False, True, True, True, True, False]
    _s, _b, counts = B.fold(w)
    assert counts["downweighted"] == 4 and counts["used"] == len(ks)
    keep = ~w["down"]
    assert np.array_equal(_bits(w["rows"][keep]), _bits(plain["rows"][keep]))
    four = np.abs(ks) == 8
    assert np.array_equal(w["rows"][four, :7], F32(0.5) * plain["rows"][four, :7])      # q = 1/2 exactly
    assert np.array_equal(w["rows"][four, 6], np.array([1 / 32, -1 / 32], F32))
    three = np.abs(ks) == 3
    q = np.sqrt(F32(HUBER) / F32(3 / 128))
    assert np.array_equal(w["rows"][three, :7], q * plain["rows"][three, :7]) and q.dtype == F32
    assert np.array_equal(w["r"], plain["r"]) and np.array_equal(w["s"], plain["s"])   # sums[29] and sums[30] stay unweighted
    a, b = B.fold(w)[0], B.fold(plain)[0]
    assert a[29] == b[29] and a[30] == b[30] and a[27] < b[27]
    # the threshold applies to r: under NORMAL r = s = 2 (z - Z0), so 1/64 is already above it
    n = B.rows_of(grid, pts, None, EYE, 0.2, mode=B.NORMAL, huber=HUBER)
    assert n["down"].tolist() == [False, False, True, True, True, True, True, True, False]
    # huber = 0 is no weights, bit for bit, in every mode; so is a threshold above every residual
    cloud = R.hand_cloud()
    for mode in (B.NORMAL, B.GRADIENT, B.METRIC):
        a = B.rows_of(grid, cloud, None, EYE, 0.1, mode=mode)
        for h in (0.0, 1.0):
            b = B.rows_of(grid, cloud, None, EYE, 0.1, mode=mode, huber=h)
            assert np.array_equal(_bits(a["rows"]), _bits(b["rows"])) and not b["down"].any(), (mode, h)
            assert np.array_equal(B.fold(a)[0], B.fold(b)[0])


def test_huber_color_closed_form():
    """the 0.5 + x colour planes: y = m - delta with delta = 1/128, 1/64, 3/128, 1/16 (exact: a multiple of m's ulp below m), so rc = delta;
    huber_color = 1/64 leaves the first two, gives 1/16 exactly wc = 1/4, qc = 1/2.  max_distance 0.5 keeps most of the cloud."""
    grid = _steep(color=True)
    cloud = R.hand_cloud()
    used0 = R.rows_of(grid, cloud, EYE, 0.5)[1] == 0
    with np.errstate(all="ignore"):
        m, _g = K.model_intensity(grid, cloud)
    deltas = np.array([0, 1 / 128, 1 / 64, 3 / 128, 1 / 16], F32)[np.arange(len(cloud)) % 5]
    with np.errstate(all="ignore"):
        y = (m - deltas).astype(F32)
    y[~np.isfinite(y)] = 0.5
    cs = 0.75
    for mode in (B.NORMAL, B.METRIC):
        plain = B.rows_of(grid, cloud, y, EYE, 0.5, cs, mode=mode)
        assert np.array_equal(plain["colored"], used0) and np.array_equal(plain["rc"][used0], deltas[used0])
        w = B.rows_of(grid, cloud, y, EYE, 0.5, cs, mode=mode, huber_color=HUBER)
        assert np.array_equal(w["cdown"], used0 & (deltas > HUBER)) and w["cdown"].sum() > 20 and not w["down"].any()
        assert np.array_equal(_bits(w["rows"][:, :8]), _bits(plain["rows"][:, :8]))                    # the geometric half is untouched
        keep = ~w["cdown"]
        assert np.array_equal(_bits(w["rows"][keep]), _bits(plain["rows"][keep]))
        four = used0 & (deltas == F32(1 / 16))
        assert four.sum() > 10 and np.array_equal(w["rows"][four, 8:15], F32(0.5) * plain["rows"][four, 8:15])
        assert np.array_equal(w["rows"][four, 14], np.full(four.sum(), F32(0.5) * (F32(cs) * F32(1 / 16)), F32))
        a, _b, ca = B.fold(w)
        b, _b, cb = B.fold(plain)
        assert ca["color_downweighted"] == int(w["cdown"].sum()) and cb["color_downweighted"] == 0 and ca["colored"] == cb["colored"]
        assert a[28] == b[28] and a[29] == b[29] and a[30] == b[30] and a[27] < b[27]
        z = B.rows_of(grid, cloud, y, EYE, 0.5, cs, mode=mode, huber_color=0.0)
        assert np.array_equal(_bits(z["rows"]), _bits(plain["rows"]))
        both = B.rows_of(grid, cloud, y, EYE, 0.5, cs, mode=mode, huber=HUBER, huber_color=HUBER)
        assert both["down"].any() and np.array_equal(both["cdown"], w["cdown"]) and np.array_equal(_bits(both["rows"][:, 8:]), _bits(w["rows"][:, 8:]))
    # NORMAL without thresholds is the colour entry's restatement
    rows, reason, colored, rc = K.rows_of(grid, cloud, y, EYE, 0.5, cs)
    w = B.rows_of(grid, cloud, y, EYE, 0.5, cs)
    assert np.array_equal(_bits(w["rows"]), _bits(rows)) and np.array_equal(w["rc"], rc)
    assert np.array_equal(B.fold(w)[0][:30], K.fold(rows, reason, colored, rc)[0])
    # color_scale 0: huber_color is not looked at
    w = B.rows_of(grid, cloud, None, EYE, 0.5, 0.0, huber_color=HUBER)
    assert not w["cdown"].any() and not w["rows"][:, 8:].any()


def _case(oracle, hip, what, mode, **kw):
    return B.case(oracle, hip.load(), what, mode, **kw)


@pytest.mark.parametrize("what", [12, 20, 30, "scene"])
def test_metric_converges_within_ten_iterations(oracle, hip, what):
    """Measured with the library's own solve (iterations until |x| < 1e-5 / final error): frame 12: 5 / 1.507 mm / 0.020 degrees (error per
    iteration 41.8 36.8 5.2 1.4 1.5); frame 20: 5 / 0.659 mm / 0.034 degrees; frame 30: 6 / 3.626 mm / 0.052 degrees; the eight-frame scene: 5 /
    0.666 mm.  Bounds: twice the float64 prototype's counts (5, 5, 6, 5), a quarter voxel, 0.1 degrees."""
    res, t, r = _case(oracle, hip, what, B.METRIC)
    assert res["status"] == R.CONVERGED and res["iterations"] <= 10
    assert t < 0.005 and r < 0.1


@pytest.mark.parametrize("what", [12, 20, "scene"])
def test_normal_does_not_converge_within_ten_iterations(oracle, hip, what):
    """The zig-zag of the inconsistent pair (n, s).  Measured: the 10th step is 2.9e-4 on frame 12 (error per iteration 41.8 10.1
    4.5 1.5 2.2 0.8 1.7 1.0 1.4 1.2 mm), 1.4e-4 on frame 20, 1.4e-4 on the scene (the float64 prototype needs 23, 18 and more than 15
    iterations)."""
    res, _t, _r = _case(oracle, hip, what, B.NORMAL)
    assert res["status"] == R.MAX_ITERATIONS and res["iterations"] == 10


def test_frame_zero_slides_but_metric_does_not_swing(oracle, hip):
    """Frame 0 is rank deficient (it slides in every mode: the pose is not asserted); NORMAL keeps swinging between two poses, METRIC creeps.
    Measured last_step after 20 iterations: NORMAL 0.0789 (the error swings 49 <-> 110 mm), METRIC 2.51e-4 (73.8 mm)."""
    normal, _t, _r = _case(oracle, hip, 0, B.NORMAL, max_iterations=20)
    metric, _t, _r = _case(oracle, hip, 0, B.METRIC, max_iterations=20)
    assert normal["iterations"] == 20 and normal["last_step"] > 0.05
    assert metric["last_step"] < 1e-3


@pytest.mark.parametrize("what", [12, 20, 30])
def test_huber_weights_hold_against_outliers(oracle, hip, what):
    """20 % of the cloud pushed 3 - 8 cm off (B.with_outliers, default_rng(7)), METRIC, 30 iterations at the most: the final error with
    huber = 0.01 is below the error without.  Measured, mm without / with (points down-weighted at the returned pose): frame 12: 1.350 / 1.191 (493); frame 20:
    2.721 / 0.797 (496); frame 30: 3.201 / 1.674 (508)."""
    plain, t0, _r = _case(oracle, hip, what, B.METRIC, max_iterations=30, outliers=True)
    robust, t1, _r = _case(oracle, hip, what, B.METRIC, max_iterations=30, huber=0.01, outliers=True)
    assert plain["downweighted"] == 0 and robust["downweighted"] > 0 and robust["first_downweighted"] > 0
    assert t1 < t0


def test_abi_refusals_bindings_and_struct_sizes(hip, tmp_path):
    lib = hip.load()
    text = open(os.path.join(ROOT, "include", "onepiece_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in hip.SIGNATURES and hasattr(lib, name), name
    assert lib.op_abi_version() == 1
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "onepiece_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d %d\\n", '
                   "sizeof(op_volume_register_options), sizeof(op_volume_register_robust_result), offsetof(op_volume_register_options, huber), "
                   "offsetof(op_volume_register_options, huber_color), offsetof(op_volume_register_robust_result, downweighted), "
                   "offsetof(op_volume_register_robust_result, first_downweighted), offsetof(op_volume_register_robust_result, rmse_residual), "
                   "offsetof(op_volume_register_robust_result, first_rmse_residual), OP_REGISTER_LIN_NORMAL, OP_REGISTER_LIN_GRADIENT, OP_REGISTER_LIN_METRIC); "
                   "return 0; }\n")
    exe = tmp_path / "sizes.bin"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    O, Rs = hip.RegisterOptions, hip.RegisterRobustResult
    assert sizes[:8] == [C.sizeof(O), C.sizeof(Rs), O.huber.offset, O.huber_color.offset, Rs.downweighted.offset, Rs.first_downweighted.offset, Rs.rmse_residual.offset,
                         Rs.first_rmse_residual.offset] == [12, 208, 4, 8, 168, 184, 192, 200]
    assert sizes[8:] == [hip.OP_REGISTER_LIN_NORMAL, hip.OP_REGISTER_LIN_GRADIENT, hip.OP_REGISTER_LIN_METRIC] == [0, 1, 2]

    # refusals: decided before any device use
    pts, y = np.zeros((4, 3), F32), np.zeros(4, F32)
    T = np.eye(4, dtype=F32).reshape(16)
    depth, rgb = np.ones((4, 4), F32), np.zeros((4, 4, 3), np.uint8)
    sums, counts, rows = np.full(31, 7.0), np.full(7, 7, np.uint64), np.full((4, 16), 7.0, F32)
    res = hip.RegisterRobustResult()
    res.color.base.iterations = 77
    par = lambda it=5, cs=1.0: hip.RegisterColorParams(hip.RegisterParams(it, 0.1, 0.0, 6), cs, 0.0)
    opt = lambda lin=2, h=0.0, hc=0.0: hip.RegisterOptions(lin, h, hc)
    p = lambda a: C.c_void_p(a.ctypes.data)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    dp, up = sums.ctypes.data_as(C.POINTER(C.c_double)), counts.ctypes.data_as(C.POINTER(C.c_uint64))
    fake = C.c_void_p(0x1000)                                          # a non-NULL volume that must never be looked at
    H, cam, F = hip.OP_MEM_HOST, hip.Camera(50, 50, 2, 2, 4, 4, 1000), hip.OP_DEPTH_F32
    sysc = lambda v=fake, x=p(pts), yy=p(y), mem=H, cs=1.0, s=dp, o=None: lib.op_volume_register_robust_system(v, x, yy, 4, mem, fp(T), 0.1, cs, 0.0, C.byref(o or opt()), s, up,
                                                                                                               p(rows))
    ptsc = lambda v=fake, x=p(pts), yy=p(y), mem=H, pr=None, r=C.byref(res), o=None: lib.op_volume_register_robust_points(v, x, yy, 4, mem, fp(T), C.byref(pr or par()),
                                                                                                                           C.byref(o or opt()), r)
    frame = lambda v=fake, d=p(depth), c=p(rgb), mem=H, stride=1, pr=None, r=C.byref(res), o=None: lib.op_volume_register_robust_frame(
        v, C.byref(cam), d, F, c, mem, stride, fp(T), C.byref(pr or par()), C.byref(o or opt()), r)
    nan, inf = float("nan"), float("inf")
    cases = {
        "default_options: null volume": lambda: lib.op_volume_register_robust_default_options(None, C.byref(opt())),
        "default_options: null options": lambda: lib.op_volume_register_robust_default_options(fake, None),
        "system: null volume": lambda: sysc(v=None),
        "system: null sums": lambda: sysc(s=None),
        "system: null xyz": lambda: sysc(x=None),
        "system: null intensity": lambda: sysc(yy=None),
        "system: bad mem": lambda: sysc(mem=2),
        "system: color_scale < 0": lambda: sysc(cs=-1.0),
        "system: color_scale NaN": lambda: sysc(cs=nan),
        "system: linearization 3": lambda: sysc(o=opt(lin=3)),
        "system: linearization -1": lambda: sysc(o=opt(lin=-1)),
        "system: huber < 0": lambda: sysc(o=opt(h=-0.01)),
        "system: huber NaN": lambda: sysc(o=opt(h=nan)),
        "system: huber inf": lambda: sysc(o=opt(h=inf)),
        "system: huber_color < 0": lambda: sysc(o=opt(hc=-0.01)),
        "system: huber_color NaN": lambda: sysc(o=opt(hc=nan)),
        "system: huber_color inf, color_scale 0": lambda: sysc(cs=0.0, o=opt(hc=inf)),
        "points: null volume": lambda: ptsc(v=None),
        "points: null result": lambda: ptsc(r=None),
        "points: null xyz": lambda: ptsc(x=None),
        "points: null intensity": lambda: ptsc(yy=None),
        "points: null intensity, default params": lambda: lib.op_volume_register_robust_points(fake, p(pts), None, 4, H, fp(T), None, None, C.byref(res)),
        "points: bad mem": lambda: ptsc(mem=-1),
        "points: max_iterations < 0": lambda: ptsc(pr=par(it=-1)),
        "points: color_scale < 0": lambda: ptsc(pr=par(cs=-0.5)),
        "points: linearization 7": lambda: ptsc(o=opt(lin=7)),
        "points: huber < 0": lambda: ptsc(o=opt(h=-1.0)),
        "points: huber_color NaN": lambda: ptsc(o=opt(hc=nan)),
        "frame: null volume": lambda: frame(v=None),
        "frame: null result": lambda: frame(r=None),
        "frame: null depth": lambda: frame(d=None),
        "frame: bad mem": lambda: frame(mem=3),
        "frame: pixel_stride 0": lambda: frame(stride=0),
        "frame: max_iterations < 0": lambda: frame(pr=par(it=-1)),
        "frame: color_scale inf": lambda: frame(pr=par(cs=inf)),
        "frame: linearization 3, no rgb": lambda: frame(c=None, o=opt(lin=3)),
        "frame: huber inf": lambda: frame(o=opt(h=inf)),
        "frame: huber_color < 0": lambda: frame(o=opt(hc=-2.0)),
    }
    for what, call in cases.items():
        assert call() == hip.OP_ERR_INVALID, what
        assert lib.op_last_error().startswith(b"op_volume_register_robust_%s:" % what.split(":")[0].encode()), (what, lib.op_last_error())   # the entry's own name
    assert (sums == 7.0).all() and (counts == 7).all() and (rows == 7.0).all() and res.color.base.iterations == 77      # nothing was written
    from onepiece_amd import integration as I
    for name in ("RegisterPointsRobust", "RegisterFrameRobust", "RobustRegistrationSystem"):
        assert callable(getattr(I.CubeHandler, name)), name
    assert I.CubeHandler.LINEARIZATIONS == B.MODES and I.CubeHandler.ROBUST_COUNT_NAMES == B.COUNT_NAMES


def test_class_surface_compiles(hip, tmp_path):
    """tests/cpp/register_robust_surface_check.cpp against host/one_piece as C++11, warnings as errors"""
    subprocess.check_call(["make", "-s"], cwd=HOST)
    lib = os.path.join(ROOT, "onepiece_amd")
    src = os.path.join(ROOT, "tests", "cpp", "register_robust_surface_check.cpp")
    exe = tmp_path / "register_robust_surface_check"
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I", HOST, "-I", os.path.join(ROOT, "include"), src, "-L", HOST, "-lone_piece_hip_host",
                           "-L", lib, "-lonepiece_hip", "-Wl,-rpath," + HOST, "-Wl,-rpath," + lib, "-o", str(exe)])
    assert subprocess.run([str(exe)], capture_output=True).returncode == 2          # it starts and links: the usage exit, no device touched
    ch = " ".join(open(os.path.join(HOST, "Integration", "CubeHandler.h")).read().split())
    for sig in ("std::shared_ptr<registration::RegistrationResult> RegisterPointCloudRobust(const geometry::PointCloud& pcd,",
                "std::shared_ptr<registration::RegistrationResult> RegisterRGBDRobust(const cv::Mat& depth, const cv::Mat& rgb, const geometry::TransformationMatrix& init_pose,",
                "bool RobustRegistrationSystem(const geometry::Point3List& points, const std::vector<float>& intensity, const geometry::TransformationMatrix& T,"):
        assert sig in ch, sig
