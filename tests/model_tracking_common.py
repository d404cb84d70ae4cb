"""What the frame-to-model tests share (inputs and the packing rule's numpy statement; no product code)."""
import numpy as np

from onepiece_amd import synthetic as S

LOOP_RES = 0.01
LOOP_ITERS = (4, 8, 16)


def pack_rgb(colors):
    """The packing rule of op_volume_render_frame, stated in numpy: (uint8)min(max(c * 255.0f + 0.5f, 0.0f), 255.0f), the product and
    the sum each rounded to float32."""
    c = np.asarray(colors, np.float32)
    s = (c * np.float32(255.0)).astype(np.float32) + np.float32(0.5)
    return np.minimum(np.maximum(s, np.float32(0.0)), np.float32(255.0)).astype(np.uint8)


def room_frame(i):
    """(pose, depth, rgb) of synthetic room frame i with the default camera."""
    pose = S.room_pose(i)
    d, c = S.room_render(pose)
    return pose, d, c


def pose_error(est, truth):
    """(translation error in metres, rotation error in degrees) of an estimated camera pose."""
    est, truth = np.asarray(est, np.float64), np.asarray(truth, np.float64)
    dt = float(np.linalg.norm(est[:3, 3] - truth[:3, 3]))
    R = est[:3, :3].T @ truth[:3, :3]
    return dt, float(np.degrees(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0))))


def compose(model_pose, T):
    """Camera pose of the tracked frame: model_pose @ inv(T), in float64."""
    return np.asarray(model_pose, np.float64) @ np.linalg.inv(np.asarray(T, np.float64))


def run_loops(frames, integrate, track_model, track_pair):
    """The two reconstruction loops over `frames` (indices into the room sequence), sharing nothing but the first pose.
      integrate(depth, rgb, pose)                       fuses a frame into the model;
      track_model(model_pose, rgb, depth) -> (T, ok, model_pixels)   tracks a frame against the model rendered at model_pose;
      track_pair(src_rgb, tgt_rgb, src_depth, tgt_depth) -> (T, ok) tracks two frames.
    Frame-to-model: every frame is tracked against the model rendered at the last good pose and fused at its estimated pose (a failed
    track is not fused).  Frame-to-frame: poses chained as DenseSlam does.  Returns a dict of per-frame lists."""
    out = {"frames": list(frames), "model_err": [], "frame_err": [], "model_ok": [], "frame_ok": [], "model_pixels": []}
    pose0, d0, c0 = room_frame(frames[0])
    integrate(d0, c0, pose0)
    model_pose = pose0.astype(np.float32)
    chain_pose = pose0.astype(np.float64)
    prev = (c0, d0)
    for i in frames[1:]:
        truth, d, c = room_frame(i)
        T, ok, npx = track_model(model_pose, c, d)
        if ok:
            model_pose = compose(model_pose, T).astype(np.float32)
            integrate(d, c, model_pose)
        out["model_ok"].append(bool(ok)); out["model_pixels"].append(int(npx)); out["model_err"].append(pose_error(model_pose, truth))
        T, ok = track_pair(prev[0], c, prev[1], d)
        if ok:
            chain_pose = compose(chain_pose, T)
        out["frame_ok"].append(bool(ok)); out["frame_err"].append(pose_error(chain_pose, truth))
        prev = (c, d)
    return out
