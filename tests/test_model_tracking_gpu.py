"""Frame-to-model tracking on the device: op_volume_render_frame against the packing rule applied to op_volume_raycast's outputs (bit for bit),
op_tracker_track_model against the composition render -> download -> op_tracker_dense_tracking (bit for bit), the reconstruction loop, and
the LiveFusion driver."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from onepiece_amd import _lib as L, integration as I, odometry as OD, synthetic as S
from model_tracking_common import LOOP_ITERS, LOOP_RES, compose, pack_rgb, room_frame, run_loops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_FRAMES = (0, 5, 10)
VIEW = 10   # the room frame whose pose the model is rendered at


def _camera(width=S.W, height=S.H, sx=1.0, sy=1.0):
    cam = I.PinholeCamera()
    cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height, cam.depth_scale = S.FX * sx, S.FY * sy, S.CX * sx, S.CY * sy, width, height, 1000.0
    return cam


def _new_volume():
    hv = I.CubeHandler(_camera(), max_blocks=1 << 16)
    hv.SetVoxelResolution(LOOP_RES)
    return hv


@pytest.fixture(scope="module")
def frames():
    """room frames by index, rendered once"""
    return {i: room_frame(i) for i in sorted(set(MODEL_FRAMES) | {15})}


@pytest.fixture(scope="module")
def model(frames):
    """three room frames at 10 mm; read-only for the tests that share it"""
    hv = _new_volume()
    for i in MODEL_FRAMES:
        pose, d, c = frames[i]
        hv.IntegrateImage(d, c, pose)
    hv.Synchronize()
    return hv


def _render(hv, pose, cam, mem="host", misalign=False):
    """op_volume_render_frame through the C-ABI -> (rgb [h,w,3] uint8, depth [h,w] float32, n_valid)"""
    lib = L.load()
    pose = np.ascontiguousarray(pose, np.float32).reshape(16)
    n = C.c_uint64(12345)
    h, w = cam.height, cam.width
    if mem == "host":
        rgb = np.full((h, w, 3), 77, np.uint8)
        d = np.full((h, w), -1.0, np.float32)
        L.check(lib.op_volume_render_frame(hv._h, C.byref(cam), pose.ctypes.data_as(L._fp), C.c_void_p(rgb.ctypes.data), d.ctypes.data_as(L._fp),
                                           L.OP_MEM_HOST, C.byref(n)))
        return rgb, d, int(n.value)
    import torch
    off = 1 if misalign else 0   # rgb one byte, depth one float off their allocations: no dword stores, no 16-byte loads
    t_rgb = torch.full((h * w * 3 + 4,), 77, dtype=torch.uint8, device="cuda")
    t_d = torch.full((h * w + 4,), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    L.check(lib.op_volume_render_frame(hv._h, C.byref(cam), pose.ctypes.data_as(L._fp), C.c_void_p(t_rgb.data_ptr() + off),
                                       C.cast(C.c_void_p(t_d.data_ptr() + 4 * off), L._fp), L.OP_MEM_DEVICE, C.byref(n)))
    rgb_all, d_all = t_rgb.cpu().numpy(), t_d.cpu().numpy()
    # nothing outside the frame was written
    assert (rgb_all[:off] == 77).all() and (rgb_all[off + h * w * 3:] == 77).all() and (d_all[:off] == -1).all() and (d_all[off + h * w:] == -1).all()
    return rgb_all[off:off + h * w * 3].reshape(h, w, 3).copy(), d_all[off:off + h * w].reshape(h, w).copy(), int(n.value)


def _check_packing(hv, pose, cam, mem, misalign=False, expect_hits=True):
    d, _n, col = hv.Raycast(pose, cam)
    rgb, depth, n = _render(hv, pose, cam, mem, misalign)
    assert np.array_equal(depth.view(np.uint32), d.view(np.uint32)), "depth differs from op_volume_raycast's"
    assert rgb.tobytes() == pack_rgb(col).tobytes(), "bytes differ from the packing rule on op_volume_raycast's colours"
    assert n == int((d > 0).sum())
    if expect_hits:
        assert n > 0 and rgb.any()
    else:
        assert n == 0 and not rgb.any() and not depth.any()
    return n


# ---- 1. packing -----------------------------------------------------------------------------------------------------------------------------------
CAMERAS = {"640x480": lambda: _camera(),
           "37x29": lambda: _camera(37, 29, 37.0 / S.W, 29.0 / S.H),            # 1073 pixels: odd, no multiple of 4 or 64
           "64x1": lambda: _camera(64, 1, 64.0 / S.W, 1.0 / S.H)}


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("camera", sorted(CAMERAS))
def test_render_frame_is_the_packing_rule_on_the_raycast(model, camera, mem):
    n = _check_packing(model, S.room_pose(VIEW), CAMERAS[camera](), mem)
    print("%s %s: %d valid pixels" % (camera, mem, n))


@pytest.mark.parametrize("camera", ["640x480", "37x29"])
def test_render_frame_into_misaligned_device_buffers(model, camera):
    """the scalar-access form of the packing kernel (an rgb pointer that admits no dword stores, a depth pointer that admits no 16-byte loads)"""
    _check_packing(model, S.room_pose(VIEW), CAMERAS[camera](), "device", misalign=True)


@pytest.mark.parametrize("mem", ["host", "device"])
def test_render_frame_of_nothing_is_an_all_zero_frame(model, mem):
    away = S.room_pose(VIEW).astype(np.float32) @ np.diag([-1.0, 1.0, -1.0, 1.0]).astype(np.float32)   # half a turn about the camera's y axis
    _check_packing(model, away, _camera(), mem, expect_hits=False)
    _check_packing(_new_volume(), S.room_pose(VIEW), _camera(), mem, expect_hits=False)                 # a freshly created volume
    _check_packing(_new_volume(), S.room_pose(VIEW), CAMERAS["37x29"](), mem, expect_hits=False)


# ---- 2. queue visibility ----------------------------------------------------------------------------------------------------------------------------
def test_render_frame_sees_the_frames_queued_before_it(frames):
    cam = _camera()
    out = []
    for sync in (False, True):
        hv = _new_volume()
        for i in MODEL_FRAMES[:2]:
            pose, d, c = frames[i]
            hv.IntegrateImage(d, c, pose)
        if sync:
            hv.Synchronize()
        out.append(_render(hv, frames[MODEL_FRAMES[1]][0], cam))
    (rgb_a, d_a, n_a), (rgb_b, d_b, n_b) = out
    assert n_a == n_b > 0 and rgb_a.tobytes() == rgb_b.tobytes() and d_a.tobytes() == d_b.tobytes()


# ---- 3. tracking is the composition -----------------------------------------------------------------------------------------------------------------
def _tracker(sums):
    odo = OD.Odometry(_camera())
    odo.SetSums(sums)
    return odo


def _same_result(a, b):
    assert np.array_equal(a.T.view(np.uint32), b.T.view(np.uint32)) or np.array_equal(a.T, b.T, equal_nan=True), (a.T, b.T)
    assert (a.rmse == b.rmse or (np.isnan(a.rmse) and np.isnan(b.rmse))), (a.rmse, b.rmse)
    assert (a.n_correspondences, a.iterations, a.tracking_success) == (b.n_correspondences, b.iterations, b.tracking_success)


INIT_T = {"identity": np.eye(4, dtype=np.float32),
          "offset": np.array([[0.9998, -0.0175, 0.0, 0.01], [0.0175, 0.9998, 0.0, -0.008], [0.0, 0.0, 1.0, 0.005], [0.0, 0.0, 0.0, 1.0]], np.float32)}


def _to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _composition(odo, src_rgb, src_d, tgt_rgb, tgt_d, init_T, device):
    if device:
        return odo.DenseTracking(_to_device(src_rgb), _to_device(tgt_rgb), _to_device(src_d), _to_device(tgt_d), init_T, 0, want_correspondences=False)
    return odo.DenseTracking(src_rgb, tgt_rgb, src_d, tgt_d, init_T, 0, want_correspondences=False)


def _check_pose(res, model_pose):
    """pose = model_pose @ inv(T): four float32 products of magnitude <= 4 per entry plus the float32 inverse -> 1e-5 absolute"""
    if res.tracking_success:
        assert np.abs(res.pose.astype(np.float64) - compose(model_pose, res.T)).max() <= 1e-5
    else:
        assert np.array_equal(res.pose, np.asarray(model_pose, np.float32))


@pytest.mark.parametrize("init", sorted(INIT_T))
@pytest.mark.parametrize("where", ["host", "device"])
def test_track_model_is_render_then_dense_tracking(model, frames, where, init):
    """reference-order sums (the default mode)"""
    model_pose = S.room_pose(VIEW).astype(np.float32)
    src_rgb, src_d, n_valid = _render(model, model_pose, _camera())
    _pose, tgt_d, tgt_rgb = frames[15]
    want = _composition(_tracker("reference_f32"), src_rgb, src_d, tgt_rgb, tgt_d, INIT_T[init], where == "device")
    tgt = (_to_device(tgt_rgb), _to_device(tgt_d)) if where == "device" else (tgt_rgb, tgt_d)
    got = _tracker("reference_f32").DenseTrackingToModel(model, model_pose, tgt[0], tgt[1], INIT_T[init], 0)
    print("T\n%s\nrmse %.6g, %d pairs, %d iterations, success %s, model pixels %d" % (got.T, got.rmse, got.n_correspondences, got.iterations, got.tracking_success, got.model_pixels))
    _same_result(got, want)
    assert got.tracking_success and got.model_pixels == n_valid
    _check_pose(got, model_pose)


@pytest.mark.parametrize("where", ["host", "device"])
def test_track_model_in_the_fp64_mode(model, frames, where):
    """The fp64 sums are per-workgroup partials added in a fixed order; whether the existing path repeats itself bit for bit is checked first
    (two runs of op_tracker_dense_tracking on one pair), and only then is the new entry held to equality with it."""
    model_pose = S.room_pose(VIEW).astype(np.float32)
    src_rgb, src_d, n_valid = _render(model, model_pose, _camera())
    _pose, tgt_d, tgt_rgb = frames[15]
    dev = where == "device"
    runs = [_composition(_tracker("fp64"), src_rgb, src_d, tgt_rgb, tgt_d, None, dev) for _ in range(2)]
    deterministic = runs[0].T.tobytes() == runs[1].T.tobytes() and runs[0].rmse == runs[1].rmse
    print("existing fp64 path run-to-run deterministic (%s frames): %s" % (where, deterministic))
    tgt = (_to_device(tgt_rgb), _to_device(tgt_d)) if dev else (tgt_rgb, tgt_d)
    got = _tracker("fp64").DenseTrackingToModel(model, model_pose, tgt[0], tgt[1], None, 0)
    assert got.tracking_success and got.model_pixels == n_valid
    if deterministic:
        _same_result(got, runs[0])
    else:
        assert (got.n_correspondences, got.iterations) == (runs[0].n_correspondences, runs[0].iterations)
        assert np.abs(got.T - runs[0].T).max() <= 1e-5
    _check_pose(got, model_pose)


def test_track_model_with_a_16_bit_target(model, frames):
    """The model view's depth is float whatever the target's format.  Raw depth d / 1000 and the float32 image holding those quotients pass the
    same validity test (thresholds 0.5 and 4 against 500 and 4000 raw: the quotient is monotone in d), so the two calls must agree bit for bit."""
    model_pose = S.room_pose(VIEW).astype(np.float32)
    _pose, tgt_d, tgt_rgb = frames[15]
    raw = np.round(tgt_d * 1000.0).astype(np.uint16)
    as_float = raw.astype(np.float32) / np.float32(1000.0)
    a = _tracker("reference_f32").DenseTrackingToModel(model, model_pose, tgt_rgb, raw, None, 0)
    b = _tracker("reference_f32").DenseTrackingToModel(model, model_pose, tgt_rgb, as_float, None, 0)
    _same_result(a, b)
    assert a.tracking_success


# ---- 4. empty model -----------------------------------------------------------------------------------------------------------------------------
def test_track_model_on_an_empty_volume(frames):
    model_pose = S.room_pose(VIEW).astype(np.float32)
    _pose, tgt_d, tgt_rgb = frames[15]
    zero_rgb, zero_d = np.zeros_like(tgt_rgb), np.zeros_like(tgt_d)
    want = _composition(_tracker("reference_f32"), zero_rgb, zero_d, tgt_rgb, tgt_d, None, False)
    got = _tracker("reference_f32").DenseTrackingToModel(_new_volume(), model_pose, tgt_rgb, tgt_d, None, 0)
    print("empty model: success %s, %d pairs, %d iterations" % (got.tracking_success, got.n_correspondences, got.iterations))
    assert got.model_pixels == 0
    _same_result(got, want)
    _check_pose(got, model_pose)


# ---- 5. the loop ------------------------------------------------------------------------------------------------------------------------------------
def test_frame_to_model_loop_drifts_less_than_frame_to_frame():
    cam = _camera()
    hv = _new_volume()
    odo_m, odo_f = OD.Odometry(cam), OD.Odometry(cam)
    odo_m.iter_count_per_level = list(LOOP_ITERS); odo_f.iter_count_per_level = list(LOOP_ITERS)

    def track_model(model_pose, rgb, depth):
        r = odo_m.DenseTrackingToModel(hv, model_pose, rgb, depth, None, 0)
        return r.T, r.tracking_success, r.model_pixels

    def track_pair(sc, tc, sd, td):
        r = odo_f.DenseTracking(sc, tc, sd, td, None, 0, want_correspondences=False)
        return r.T, r.tracking_success

    out = run_loops(range(0, 41, 5), hv.IntegrateImage, track_model, track_pair)
    for i, em, ef, npx in zip(out["frames"][1:], out["model_err"], out["frame_err"], out["model_pixels"]):
        print("frame %2d: frame-to-frame %.4f m / %.2f deg, frame-to-model %.4f m / %.2f deg, model view %.3f of the image"
              % (i, ef[0], ef[1], em[0], em[1], npx / float(cam.width * cam.height)))
    assert all(out["model_ok"])
    assert min(out["model_pixels"]) >= 0.9 * cam.width * cam.height
    assert out["model_err"][-1][0] < out["frame_err"][-1][0]


# ---- 6. the driver ----------------------------------------------------------------------------------------------------------------------------------
def _live_fusion(tmp, track):
    exe = os.path.join(ROOT, "examples", "cpp", "LiveFusion.bin")
    assert os.path.exists(exe), "examples/cpp/LiveFusion.bin is not built"
    out = os.path.join(str(tmp), track)
    os.makedirs(out)
    p = subprocess.run([exe, "--synthetic", "9", "5", "1", "--res", "0.01", "--track", track], cwd=out, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True, timeout=120)   # (writes trajectory.txt and pose_error.txt into its working directory)
    print(p.stdout)
    assert p.returncode == 0
    poses = np.loadtxt(os.path.join(out, "trajectory.txt")).reshape(-1, 4, 4)
    errors = np.loadtxt(os.path.join(out, "pose_error.txt")).reshape(-1, 3)
    return poses, errors


def test_live_fusion_driver(tmp_path):
    poses, err_model = _live_fusion(tmp_path, "model")
    assert poses.shape == (9, 4, 4) and np.isfinite(poses).all()
    for P in poses:   # rigid: orthonormal rotation of determinant 1, last row 0 0 0 1
        assert np.abs(P[:3, :3] @ P[:3, :3].T - np.eye(3)).max() < 1e-4 and abs(np.linalg.det(P[:3, :3]) - 1.0) < 1e-4
        assert np.array_equal(P[3], [0.0, 0.0, 0.0, 1.0])
    _poses_f, err_frame = _live_fusion(tmp_path, "frame")
    assert len(err_model) == len(err_frame) == 9
    assert err_model[-1, 1] < err_frame[-1, 1]   # columns: frame, translation error (m), rotation error (deg)
