"""The colour term of op_volume_register_color_* without a device: the numpy restatement of its definition (tests/volume_register_color_common.py)
on a hand-made field where rows and sums have a closed form, the restated Gauss-Newton loop against the TRUTH on the scene the geometric
registration cannot hold, and what of the entries needs no device -- the refusals, the binding, the struct sizes, the class surface.

The sliding scene: the room through D.frames(D.CAM_64, 8, stride=5) into 2 cm voxels, truncation 0.1, fused by the oracle (one corner of the room:
tests/test_volume_register_cpu.py calls it "NOT usable").  The cloud is every third of the eight frames' hit points in world coordinates (8192
points) with the intensity of their pixels; the true transformation is the identity; the start is D.perturbed(identity, 1), 41.8 mm / 0.97 degrees
off; 15 iterations, max_distance 0.1.  The measured figures are in the docstrings of the two tests."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import volume_register_color_common as K
import volume_register_common as R
import volume_sample_common as S

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "host", "one_piece")
EIGEN = "/root/reference/3rdparty/Eigen"
NAMES = ("op_volume_register_color_default_params", "op_volume_register_color_system", "op_volume_register_color_points", "op_volume_register_rgbd")


def _hand_intensities(pts):
    """observed intensities for K's hand-made field: the model's exact intensity plus 1/16 -- every third point -- so that rc = -1/16 or 0"""
    c = F32(0.5) + pts[:, 0]
    y = K.intensity(np.stack([c, c, c], axis=1))
    y[::3] = y[::3] + F32(0.0625)
    return y


def test_hand_made_field_gives_the_closed_form():
    vox = K.hand_blocks()
    grid = S.Grid(R.HAND_KEYS, vox, R.HAND_RES)
    pts = R.hand_cloud()
    T = np.eye(4, dtype=F32)
    with np.errstate(all="ignore"):
        y = _hand_intensities(pts)
    cs = 0.75
    rows, reason, colored, rc = K.rows_of(grid, pts, y, T, 0.1, cs)
    rows8, reason8 = R.rows_of(grid, pts, T, 0.1)
    assert np.array_equal(reason, reason8) and np.array_equal(rows[:, :8].view(np.uint32), rows8.view(np.uint32))   # the geometry is untouched
    for i, (what, _p, want) in enumerate(R.HAND_POINTS):
        assert reason[i] == want, (what, int(reason[i]))
    used = reason == 0
    assert np.array_equal(colored, used) and used.sum() > 50               # every used point has a finite intensity here: all are coloured
    # the closed form: the colour of every sample is exactly 0.5 + x at its point, so m and g are the intensity formula on exact inputs
    p = pts[used]
    h, res = F32(0.5) * F32(R.HAND_RES), F32(R.HAND_RES)
    tri = lambda c: K.intensity(np.stack([c, c, c], axis=1))
    m = tri(F32(0.5) + p[:, 0])
    g0 = (tri(F32(0.5) + (p[:, 0] + h)) - tri(F32(0.5) + (p[:, 0] - h))) / res
    assert (np.abs(g0.astype(np.float64) - float(K.ISUM)) < 1e-4).all()    # I' = I(1, 1, 1) to the rounding of the difference quotient
    z = np.zeros(len(p), F32)
    c = F32(cs)
    want_jc = np.stack([c * g0, z, z, z, c * (p[:, 2] * g0), c * (-(p[:, 1] * g0))], axis=1)
    want_r = m - y[used]
    assert np.array_equal(rows[used, 8:14], want_jc)                       # jc = cs I' (1, 0, 0, 0, p2, -p1)
    assert np.array_equal(rows[used, 14], c * want_r) and (rows[used, 15] == 1).all() and np.array_equal(rc[used], want_r)
    assert set(np.unique(want_r).tolist()) == {-0.0625, 0.0}
    assert not rows[~used].any()
    # the 30 sums against the closed form's terms: the same terms, so the two fsums are within the rounding of their additions (here: equal)
    sums, bound, counts = K.fold(rows, reason, colored, rc)
    d = lambda v: v.astype(np.float64)
    j, s = d(rows8[used, :6]), d(rows8[used, 6])
    closed = [np.sum(j[:, a] * j[:, b] + d(want_jc[:, a] * want_jc[:, b])) for a, b in R.PAIRS]
    closed += [np.sum(s * j[:, a] + d((c * want_r) * want_jc[:, a])) for a in range(6)]
    closed += [np.sum(s * s + d(c * want_r) ** 2), np.sum(d(want_r) ** 2), np.sum(s * s)]
    err = np.abs(sums - np.array(closed))
    assert (err <= bound + 2.0 ** -53 * np.abs(sums)).all(), (err, bound)
    gsums, _m, gcounts = R.fold(rows8, reason8)
    assert sums[29] == gsums[27] and {k: counts[k] for k in R.COUNT_NAMES} == gcounts and counts["colored"] == counts["used"]
    assert sums[28] == (used[::3].sum()) * 0.0625 ** 2

    # a NaN and an infinite intensity: used, not coloured, the geometric half stays
    first = int(np.flatnonzero(used)[0])
    for bad in (np.nan, np.inf, -np.inf):
        y2 = y.copy()
        y2[first] = bad
        rows2, reason2, colored2, rc2 = K.rows_of(grid, pts, y2, T, 0.1, cs)
        assert reason2[first] == 0 and not colored2[first] and rc2[first] == 0 and not rows2[first, 8:].any()
        assert np.array_equal(rows2[first, :8], rows[first, :8]) and colored2.sum() == colored.sum() - 1
    # a residual just above and just below max_color_residual: |rc| = 1/16 at every third point
    third = np.flatnonzero(used & (np.arange(len(pts)) % 3 == 0))
    assert len(third) > 10 and (np.abs(rc[third]) == 0.0625).all()
    at, above, below = 0.0625, float(np.nextafter(F32(0.0625), F32(0))), float(np.nextafter(F32(0.0625), F32(1)))
    for limit, kept in ((at, True), (above, False), (below, True)):        # the limit just below |rc| gates it, the limit at or above keeps it
        _r, _re, col3, _rc = K.rows_of(grid, pts, y, T, 0.1, cs, max_color_residual=limit)
        assert bool(col3[third].all()) == kept and bool(col3[third].any()) == kept, limit
        assert col3[used & (np.arange(len(pts)) % 3 != 0)].all()           # rc = 0 passes any positive limit
    # color_scale = 0: the geometric system, nothing coloured
    s0, c0 = K.system(grid, pts, None, T, 0.1, 0.0)
    assert np.array_equal(s0[:28], gsums) and s0[28] == 0 and s0[29] == gsums[27] and c0["colored"] == 0


def _run_loop(lib, grid, cloud, y, init, color_scale):
    trace = []
    evaluate = lambda T: K.system(grid, cloud, y, T, K.TRUNC, color_scale)
    res = K.loop(lib, evaluate, init, 15, min_step=0.0, trace=trace)
    for k, (T, counts, rmse, rmse_c, step) in enumerate(trace):
        t, r = R.pose_error(T)
        print("  iteration %2d: used %d, coloured %d, rmse %.5f, colour rmse %.5f, pose error %.3f mm / %.5f deg, step %.2e" % (
            k, counts["used"], counts["colored"], rmse, rmse_c, t * 1e3, r, step))
    t, r = R.pose_error(res["T"])
    print("  final: used %d, coloured %d, rmse %.5f (first %.5f), colour rmse %.5f (first %.5f), pose error %.3f mm / %.5f deg" % (
        res["used"], res["colored"], res["rmse"], res["first_rmse"], res["rmse_color"], res["first_rmse_color"], t * 1e3, r))
    return res, t, r


def test_the_restated_loop_holds_the_sliding_scene(oracle, hip):
    """The eight-frame cloud (8192 points).  Bounds, as the feature was specified: without the colour term the loop ends more than 30 mm off
    (the scene slides); with color_scale 1 translation < 2 mm (a tenth of a voxel), rotation < 0.05 degrees, the smallest eigenvalue of JtJ at the
    truth > 100, final colour rmse < first / 5.
    Measured with the library's own op_ldlt_solve6 / op_se3_exp (the figures of a float64 numpy solve, to the digits shown): 8066 points used and
    coloured at the truth, sdf rmse 0.00076, colour rmse 0.00166; eigenvalues of JtJ at the truth 4.3, 66.3, 311.7, 2831.6, 4803.8, 8251.1 without
    and 260.6, 436.5, 1139.5, 7050.0, 10549.1, 15011.5 with the term.  color_scale 0: 92 mm off after one step, 66.6 mm / 2.80 degrees after 15, the
    step still 3.2e-4 (the rmse falls to 0.00087 all the while).  color_scale 1: 11.8 mm, 2.4 mm, 0.34 mm after the first three steps, 0.503 mm /
    below 1e-4 degrees from the 6th on, the step 3.6e-8 at the 8th and around 1e-8 after; 8062 points used and coloured, sdf rmse 0.02558 ->
    0.00075, colour rmse 0.02223 -> 0.00166 (a factor 13)."""
    lib = hip.load()
    sc = K.color_scene(oracle)
    assert len(sc["cloud"]) == 8192 == len(sc["y"])
    t0, r0 = R.pose_error(sc["init"])
    assert 0.041 < t0 < 0.043 and 0.96 < r0 < 0.98
    eye = np.eye(4, dtype=F32)
    s_geo, c_geo = K.system(sc["grid"], sc["cloud"], sc["y"], eye, K.TRUNC, 0.0)
    s_col, c_col = K.system(sc["grid"], sc["cloud"], sc["y"], eye, K.TRUNC, 1.0)
    e_geo, e_col = K.jtj_eigenvalues(s_geo), K.jtj_eigenvalues(s_col)
    print("at the truth: used %d, coloured %d, rmse %.5f, colour rmse %.5f" % (c_col["used"], c_col["colored"], K.rmse_geometric(s_col, c_col["used"]),
                                                                                 K.rmse_color(s_col, c_col["colored"])))
    print("eigenvalues of JtJ at the truth: geometric %s; with colour %s" % (np.round(e_geo, 1).tolist(), np.round(e_col, 1).tolist()))
    assert c_geo["used"] == c_col["used"] == c_col["colored"] > 7500 and s_col[29] == s_geo[27]
    print("color_scale 0:")
    geo, tg, _rg = _run_loop(lib, sc["grid"], sc["cloud"], sc["y"], sc["init"], 0.0)
    print("color_scale 1:")
    col, t, r = _run_loop(lib, sc["grid"], sc["cloud"], sc["y"], sc["init"], 1.0)
    assert geo["iterations"] == col["iterations"] == 15
    assert tg > 0.030                                                      # the scene does slide without the term
    assert t < 0.002
    assert r < 0.05
    assert e_col[0] > 100
    assert col["rmse_color"] < col["first_rmse_color"] / 5


def test_the_restated_loop_holds_a_single_frame(oracle, hip):
    """Frame 3 alone, every pixel with depth (3072 points): translation < 2 mm, rotation < 0.05 degrees with color_scale 1.
    Measured with the library's solve: 11.4 mm, 1.75 mm, 0.16 mm after the first three steps, 0.352 mm / below 1e-4 degrees from the 8th on, the
    step around 1e-7; 3038 points used and coloured, sdf rmse 0.02582 -> 0.00063, colour rmse 0.02211 -> 0.00135."""
    lib = hip.load()
    sc = K.color_scene(oracle)
    assert len(sc["frame3"]) == 3072 == len(sc["y3"])
    print("color_scale 1, frame 3:")
    _col, t, r = _run_loop(lib, sc["grid"], sc["frame3"], sc["y3"], sc["init"], 1.0)
    assert t < 0.002
    assert r < 0.05


def test_abi_refusals_binding_and_struct_sizes(hip, tmp_path):
    lib = hip.load()
    text = open(os.path.join(ROOT, "include", "onepiece_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in hip.SIGNATURES and hasattr(lib, name), name
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "onepiece_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
                   "sizeof(op_volume_register_color_params), sizeof(op_volume_register_color_result), offsetof(op_volume_register_color_params, color_scale), "
                   "offsetof(op_volume_register_color_result, colored), offsetof(op_volume_register_color_result, rmse_color), "
                   "offsetof(op_volume_register_color_result, first_rmse_color)); return 0; }\n")
    exe = tmp_path / "sizes.bin"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P, Rs = hip.RegisterColorParams, hip.RegisterColorResult
    assert sizes == [C.sizeof(P), C.sizeof(Rs), P.color_scale.offset, Rs.colored.offset, Rs.rmse_color.offset, Rs.first_rmse_color.offset] == [24, 168, 16, 136, 152, 160]

    # refusals: decided before any device use
    pts, y = np.zeros((4, 3), F32), np.zeros(4, F32)
    T = np.eye(4, dtype=F32).reshape(16)
    depth, rgb = np.ones((4, 4), F32), np.zeros((4, 4, 3), np.uint8)
    sums, counts, rows = np.full(30, 7.0), np.full(5, 7, np.uint64), np.full((4, 16), 7.0, F32)
    res = hip.RegisterColorResult()
    res.base.iterations = 77
    par = lambda it=5, cs=1.0: hip.RegisterColorParams(hip.RegisterParams(it, 0.1, 0.0, 6), cs, 0.0)
    p = lambda a: C.c_void_p(a.ctypes.data)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    dp, up = sums.ctypes.data_as(C.POINTER(C.c_double)), counts.ctypes.data_as(C.POINTER(C.c_uint64))
    fake = C.c_void_p(0x1000)                                          # a non-NULL volume that must never be looked at
    H, cam, F = hip.OP_MEM_HOST, hip.Camera(50, 50, 2, 2, 4, 4, 1000), hip.OP_DEPTH_F32
    sysc = lambda v=fake, x=p(pts), yy=p(y), mem=H, cs=1.0, s=dp: lib.op_volume_register_color_system(v, x, yy, 4, mem, fp(T), 0.1, cs, 0.0, s, up, p(rows))
    ptsc = lambda v=fake, x=p(pts), yy=p(y), mem=H, pr=None, r=C.byref(res): lib.op_volume_register_color_points(v, x, yy, 4, mem, fp(T), C.byref(pr or par()), r)
    rgbd = lambda v=fake, d=p(depth), c=p(rgb), mem=H, stride=1, pr=None, r=C.byref(res): lib.op_volume_register_rgbd(
        v, C.byref(cam), d, F, c, mem, stride, fp(T), C.byref(pr or par()), r)
    cases = {
        "default_params: null volume": lambda: lib.op_volume_register_color_default_params(None, C.byref(par())),
        "default_params: null params": lambda: lib.op_volume_register_color_default_params(fake, None),
        "system: null volume": lambda: sysc(v=None),
        "system: null sums": lambda: sysc(s=None),
        "system: null xyz": lambda: sysc(x=None),
        "system: null intensity": lambda: sysc(yy=None),
        "system: bad mem": lambda: sysc(mem=2),
        "system: color_scale < 0": lambda: sysc(cs=-1.0),
        "system: color_scale NaN": lambda: sysc(cs=float("nan")),
        "system: color_scale inf": lambda: sysc(cs=float("inf")),
        "points: null volume": lambda: ptsc(v=None),
        "points: null result": lambda: ptsc(r=None),
        "points: null xyz": lambda: ptsc(x=None),
        "points: null intensity": lambda: ptsc(yy=None),
        "points: null intensity, default params": lambda: lib.op_volume_register_color_points(fake, p(pts), None, 4, H, fp(T), None, C.byref(res)),
        "points: bad mem": lambda: ptsc(mem=-1),
        "points: max_iterations < 0": lambda: ptsc(pr=par(it=-1)),
        "points: color_scale < 0": lambda: ptsc(pr=par(cs=-0.5)),
        "points: color_scale NaN": lambda: ptsc(pr=par(cs=float("nan"))),
        "rgbd: null volume": lambda: rgbd(v=None),
        "rgbd: null result": lambda: rgbd(r=None),
        "rgbd: null depth": lambda: rgbd(d=None),
        "rgbd: null rgb": lambda: rgbd(c=None),
        "rgbd: bad mem": lambda: rgbd(mem=3),
        "rgbd: pixel_stride 0": lambda: rgbd(stride=0),
        "rgbd: max_iterations < 0": lambda: rgbd(pr=par(it=-1)),
        "rgbd: color_scale inf": lambda: rgbd(pr=par(cs=float("inf"))),
    }
    for what, call in cases.items():
        assert call() == hip.OP_ERR_INVALID, what
        entry = what.split(":")[0]
        name = b"op_volume_register_rgbd:" if entry == "rgbd" else b"op_volume_register_color_%s:" % entry.encode()
        assert lib.op_last_error().startswith(name), (what, lib.op_last_error())                               # the entry's own name
    assert (sums == 7.0).all() and (counts == 7).all() and (rows == 7.0).all() and res.base.iterations == 77      # nothing was written
    from onepiece_amd import integration as I
    for name in ("RegisterColoredPoints", "RegisterRGBD", "ColorRegistrationSystem", "Intensity"):
        assert callable(getattr(I.CubeHandler, name)), name
    c = np.array([[0.25, 0.5, 1.0], [1.0, 1.0, 1.0]], F32)
    assert np.array_equal(I.CubeHandler.Intensity(c), K.intensity(c)) and I.CubeHandler.Intensity(c)[1] == K.ISUM


def test_class_surface_compiles(hip, tmp_path):
    """tests/cpp/register_color_surface_check.cpp against host/one_piece as C++11, and against the real Eigen where the reference's vendored copy exists"""
    subprocess.check_call(["make", "-s"], cwd=HOST)
    lib = os.path.join(ROOT, "onepiece_amd")
    src = os.path.join(ROOT, "tests", "cpp", "register_color_surface_check.cpp")
    exe = tmp_path / "register_color_surface_check"
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I", HOST, "-I", os.path.join(ROOT, "include"), src, "-L", HOST, "-lone_piece_hip_host",
                           "-L", lib, "-lonepiece_hip", "-Wl,-rpath," + HOST, "-Wl,-rpath," + lib, "-o", str(exe)])
    assert subprocess.run([str(exe)], capture_output=True).returncode == 2          # it starts and links: the usage exit, no device touched
    ch = " ".join(open(os.path.join(HOST, "Integration", "CubeHandler.h")).read().split())
    for sig in ("std::shared_ptr<registration::RegistrationResult> RegisterColoredPointCloud(const geometry::PointCloud& pcd,",
                "std::shared_ptr<registration::RegistrationResult> RegisterRGBD(const cv::Mat& depth, const cv::Mat& rgb, const geometry::TransformationMatrix& init_pose,",
                "bool ColorRegistrationSystem(const geometry::Point3List& points, const std::vector<float>& intensity, const geometry::TransformationMatrix& T,"):
        assert sig in ch, sig
    if os.path.isdir(EIGEN):
        subprocess.check_call(["g++", "-std=c++11", "-O1", "-w", "-msse4.2", "-DONEPIECE_HAVE_EIGEN", "-I", EIGEN, "-I", HOST, "-I", os.path.join(ROOT, "include"),
                               "-fsyntax-only", src, os.path.join(HOST, "src", "CubeHandler.cpp")])
