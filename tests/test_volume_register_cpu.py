"""op_volume_register_* without a device: the numpy restatement of its definition (tests/volume_register_common.py) on a hand-made field where the
system has a closed form, the restated Gauss-Newton loop against the TRUTH on the room, and what of the entries needs no device -- the refusals,
the binding, the struct sizes, the class surface.

Convergence scene: the room through D.frames(D.CAM_64, 8, stride=25) into 2 cm voxels, truncation 0.1, fused by the oracle; the cloud is every third
of the eight frames' hit points in world coordinates (8192 points), so the true transformation is the identity; the start is
D.perturbed(identity, 1), 4.2 cm and 0.97 degrees off.  Measured with a float64 solve when the feature was specified: 8033 points used at the
truth, eigenvalues of JtJ from 256 to 11 852, translation error 1.1 mm after 3 iterations and between 0.40 and 0.75 mm from the 5th on (the
iterates oscillate with the flipping of a few `used` flags), rotation error below 1e-4 degrees, rmse 0.034 -> 0.0030.  Bounds: translation < 2 mm
(a tenth of a voxel, about 3x the largest value seen after the 5th iteration), rotation < 0.05 degrees, final rmse < first_rmse / 5.
(The frames 5 room frames apart are NOT usable for this: the eigenvalues of JtJ run from 4.3 to 8251 there and the cloud slides along the walls --
the scene's rank deficiency)"""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np

import volume_register_common as R
import volume_sample_common as S

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "host", "one_piece")
EIGEN = "/root/reference/3rdparty/Eigen"
NAMES = ("op_volume_register_default_params", "op_volume_register_system", "op_volume_register_points", "op_volume_register_depth")


def test_hand_made_field_gives_the_closed_form():
    vox = R.hand_blocks()
    grid = S.Grid(R.HAND_KEYS, vox, R.HAND_RES)
    pts = R.hand_cloud()
    rows, reason = R.rows_of(grid, pts, np.eye(4, dtype=F32), 0.1)
    for i, (what, _p, want) in enumerate(R.HAND_POINTS):
        assert reason[i] == want, (what, int(reason[i]))
    sums, _mags, counts = R.fold(rows, reason)
    print(counts)
    assert counts["used"] > 50 and counts["invalid"] > 50 and counts["no_gradient"] > 10 and counts["too_far"] > 20 and sum(counts.values()) == len(pts)
    used = reason == 0
    p = pts[used].astype(np.float64)
    z = np.zeros(len(p))
    want_rows = np.stack([z, z, z + 1, p[:, 1], -p[:, 0], z, p[:, 2] - R.HAND_Z0, z + 1], axis=1)
    assert np.array_equal(rows[used].astype(np.float64), want_rows)    # every used row is (0, 0, 1, p1, -p0, 0) and s the exact distance
    assert not rows[~used].any()
    assert (np.abs(p[:, 2] - R.HAND_Z0) <= 0.1).all() and (np.abs(pts[reason == 3, 2].astype(np.float64) - R.HAND_Z0) > 0.1).all()
    # the closed form: few-bit dyadic values, so every product and every partial sum is exact in double
    j, s = want_rows[:, :6], want_rows[:, 6]
    closed = [np.sum(j[:, a] * j[:, b]) for a, b in R.PAIRS] + [np.sum(s * j[:, a]) for a in range(6)] + [np.sum(s * s)]
    assert np.array_equal(sums, np.array(closed))
    assert sums[R.PAIRS.index((2, 2))] == counts["used"]
    # without the gate the far points are used
    _s, c0 = R.system(grid, pts, np.eye(4, dtype=F32), 0.0)
    assert c0["too_far"] == 0 and c0["used"] == counts["used"] + counts["too_far"] and c0["no_gradient"] == counts["no_gradient"]


def test_the_restated_loop_finds_the_truth(oracle, hip):
    lib = hip.load()
    sc = R.reg_scene(oracle)
    assert len(sc["cloud"]) == 8192
    t0, r0 = R.pose_error(sc["init"])
    assert 0.041 < t0 < 0.043 and 0.96 < r0 < 0.98
    _sums, at_truth = R.system(sc["grid"], sc["cloud"], np.eye(4, dtype=F32), R.TRUNC)
    trace = []
    res = R.loop(lib, lambda T: R.system(sc["grid"], sc["cloud"], T, R.TRUNC), sc["init"], 15, min_step=0.0, trace=trace)
    for k, (T, counts, rmse, step) in enumerate(trace):
        print("iteration %2d: used %d, rmse %.5f, pose error %.3f mm / %.5f deg, step %.2e" % ((k, counts["used"], rmse) + tuple(
            v * s for v, s in zip(R.pose_error(T), (1e3, 1.0))) + (step,)))
    t, r = R.pose_error(res["T"])
    print("used at the truth %d; final: used %d, rmse %.5f (first %.5f), pose error %.3f mm / %.5f deg" % (at_truth["used"], res["used"], res["rmse"], res["first_rmse"], t * 1e3, r))
    assert at_truth["used"] > 7500
    assert res["status"] == R.MAX_ITERATIONS and res["iterations"] == 15
    assert t < 0.002
    assert r < 0.05
    assert res["rmse"] < res["first_rmse"] / 5


def _header():
    return open(os.path.join(ROOT, "include", "onepiece_hip.h")).read()


def test_abi_refusals_binding_and_struct_sizes(hip, tmp_path):
    lib = hip.load()
    text = _header()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in hip.SIGNATURES and hasattr(lib, name), name
    for k, name in enumerate(("OP_REGISTER_CONVERGED", "OP_REGISTER_MAX_ITERATIONS", "OP_REGISTER_TOO_FEW_POINTS", "OP_REGISTER_SINGULAR")):
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, text)
        assert m and int(m.group(1)) == k == getattr(hip, name), name
    # sizeof as a C compiler sees the header
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "onepiece_hip.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", '
                   "sizeof(op_volume_register_params), sizeof(op_volume_register_result), offsetof(op_volume_register_result, used), "
                   "offsetof(op_volume_register_result, rmse)); return 0; }\n")
    exe = tmp_path / "sizes.bin"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [C.sizeof(hip.RegisterParams), C.sizeof(hip.RegisterResult), hip.RegisterResult.used.offset, hip.RegisterResult.rmse.offset] == [16, 136, 72, 112]

    # refusals: decided before any device use
    pts = np.zeros((4, 3), F32)
    T = np.eye(4, dtype=F32).reshape(16)
    depth = np.ones((4, 4), F32)
    sums, counts, rows = np.full(28, 7.0), np.full(4, 7, np.uint64), np.full((4, 8), 7.0, F32)
    res, par = hip.RegisterResult(), hip.RegisterParams(5, 0.1, 0.0, 6)
    res.iterations = 77
    bad_par = hip.RegisterParams(-1, 0.1, 0.0, 6)
    p = lambda a: C.c_void_p(a.ctypes.data)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    dp, up = sums.ctypes.data_as(C.POINTER(C.c_double)), counts.ctypes.data_as(C.POINTER(C.c_uint64))
    fake = C.c_void_p(0x1000)                                          # a non-NULL volume that must never be looked at
    H, cam = hip.OP_MEM_HOST, hip.Camera(50, 50, 2, 2, 4, 4, 1000)
    cases = {
        "default_params: null volume": lambda: lib.op_volume_register_default_params(None, C.byref(par)),
        "system: null volume": lambda: lib.op_volume_register_system(None, p(pts), 4, H, fp(T), 0.1, dp, up, p(rows)),
        "system: null sums": lambda: lib.op_volume_register_system(fake, p(pts), 4, H, fp(T), 0.1, None, up, None),
        "system: null xyz": lambda: lib.op_volume_register_system(fake, None, 4, H, fp(T), 0.1, dp, up, None),
        "system: bad mem": lambda: lib.op_volume_register_system(fake, p(pts), 4, 2, fp(T), 0.1, dp, up, None),
        "points: null volume": lambda: lib.op_volume_register_points(None, p(pts), 4, H, fp(T), C.byref(par), C.byref(res)),
        "points: null result": lambda: lib.op_volume_register_points(fake, p(pts), 4, H, fp(T), C.byref(par), None),
        "points: null xyz": lambda: lib.op_volume_register_points(fake, None, 4, H, fp(T), C.byref(par), C.byref(res)),
        "points: bad mem": lambda: lib.op_volume_register_points(fake, p(pts), 4, -1, fp(T), C.byref(par), C.byref(res)),
        "points: max_iterations < 0": lambda: lib.op_volume_register_points(fake, p(pts), 4, H, fp(T), C.byref(bad_par), C.byref(res)),
        "depth: null volume": lambda: lib.op_volume_register_depth(None, C.byref(cam), p(depth), hip.OP_DEPTH_F32, H, 1, fp(T), C.byref(par), C.byref(res)),
        "depth: null result": lambda: lib.op_volume_register_depth(fake, C.byref(cam), p(depth), hip.OP_DEPTH_F32, H, 1, fp(T), C.byref(par), None),
        "depth: bad mem": lambda: lib.op_volume_register_depth(fake, C.byref(cam), p(depth), hip.OP_DEPTH_F32, 3, 1, fp(T), C.byref(par), C.byref(res)),
        "depth: pixel_stride 0": lambda: lib.op_volume_register_depth(fake, C.byref(cam), p(depth), hip.OP_DEPTH_F32, H, 0, fp(T), C.byref(par), C.byref(res)),
        "depth: max_iterations < 0": lambda: lib.op_volume_register_depth(fake, C.byref(cam), p(depth), hip.OP_DEPTH_F32, H, 1, fp(T), C.byref(bad_par), C.byref(res)),
    }
    for what, call in cases.items():
        assert call() == hip.OP_ERR_INVALID, what
        assert lib.op_last_error().startswith(b"op_volume_register_%s:" % what.split(":")[0].encode()), (what, lib.op_last_error())   # the entry's own name
    assert (sums == 7.0).all() and (counts == 7).all() and (rows == 7.0).all() and res.iterations == 77      # nothing was written
    from onepiece_amd import integration as I
    for name in ("RegisterPoints", "RegisterDepth", "RegistrationSystem"):
        assert callable(getattr(I.CubeHandler, name)), name


def test_class_surface_compiles(hip, tmp_path):
    """tests/cpp/register_surface_check.cpp against host/one_piece as C++11, and against the real Eigen where the reference's vendored copy exists"""
    subprocess.check_call(["make", "-s"], cwd=HOST)
    lib = os.path.join(ROOT, "onepiece_amd")
    src = os.path.join(ROOT, "tests", "cpp", "register_surface_check.cpp")
    exe = tmp_path / "register_surface_check"
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I", HOST, "-I", os.path.join(ROOT, "include"), src, "-L", HOST, "-lone_piece_hip_host",
                           "-L", lib, "-lonepiece_hip", "-Wl,-rpath," + HOST, "-Wl,-rpath," + lib, "-o", str(exe)])
    assert subprocess.run([str(exe)], capture_output=True).returncode == 2          # it starts and links: the usage exit, no device touched
    ch = " ".join(open(os.path.join(HOST, "Integration", "CubeHandler.h")).read().split())
    for sig in ("std::shared_ptr<registration::RegistrationResult> RegisterPointCloud(const geometry::PointCloud& pcd,",
                "std::shared_ptr<registration::RegistrationResult> RegisterDepth(const cv::Mat& depth, const geometry::TransformationMatrix& init_pose,",
                "bool RegistrationSystem(const geometry::Point3List& points, const geometry::TransformationMatrix& T, float max_distance,"):
        assert sig in ch, sig
    if os.path.isdir(EIGEN):
        subprocess.check_call(["g++", "-std=c++11", "-O1", "-w", "-msse4.2", "-DONEPIECE_HAVE_EIGEN", "-I", EIGEN, "-I", HOST, "-I", os.path.join(ROOT, "include"),
                               "-fsyntax-only", src, os.path.join(HOST, "src", "CubeHandler.cpp")])
