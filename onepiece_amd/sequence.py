"""The reference's on-disk RGB-D sequence format ("TUM-format" in BASELINE.json):

    <dir>/associate.txt    one line per frame:  t_rgb  rgb_path  t_depth  depth_path
    <dir>/trajectory.txt   one line per frame:  16 floats = row-major 4x4 camera-to-world pose

read by tool::ReadImageSequence / ReadImageSequenceWithPose (/root/reference/src/Tool/IO.cpp:59-108).
Depth images are 16-bit PNGs in 1/depth_scale metres, colour images 8-bit PNGs; the examples load
them with cv::imread (colour arrives as B,G,R) and convert depth with tool::ConvertDepthTo32F
(Tool/ImageProcessing.cpp:68-91).  This module is harness code (file IO + one elementwise
conversion), not part of the measured path; PNG coding is PIL's.
"""
import os

import numpy as np


def WriteImageSequence(path, depths_m, rgbs_bgr, poses, depth_scale=1000.0):
    """Writes the sequence; depth in metres is quantised to uint16 = round(d * depth_scale)."""
    from PIL import Image
    os.makedirs(os.path.join(path, "rgb"), exist_ok=True)
    os.makedirs(os.path.join(path, "depth"), exist_ok=True)
    with open(os.path.join(path, "associate.txt"), "w") as fa, open(os.path.join(path, "trajectory.txt"), "w") as ft:
        for i, (d, c, p) in enumerate(zip(depths_m, rgbs_bgr, poses)):
            t = "%.6f" % (i / 30.0)
            rgb_name, depth_name = "rgb/%06d.png" % i, "depth/%06d.png" % i
            d16 = np.clip(np.round(np.asarray(d, np.float64) * depth_scale), 0, 65535).astype(np.uint16)
            Image.fromarray(d16).save(os.path.join(path, depth_name))                         # 16-bit greyscale PNG
            Image.fromarray(np.ascontiguousarray(np.asarray(c, np.uint8)[:, :, ::-1])).save(os.path.join(path, rgb_name))  # stored as RGB
            fa.write("%s %s %s %s\n" % (t, rgb_name, t, depth_name))
            ft.write(" ".join("%.9g" % float(x) for x in np.asarray(p, np.float32).reshape(16)) + "\n")


def ReadImageSequence(path):
    """tool::ReadImageSequence (IO.cpp:59-80) -> (rgb_files, depth_files)."""
    rgb_files, depth_files = [], []
    with open(os.path.join(path, "associate.txt")) as f:
        for line in f:
            tok = line.split()
            if len(tok) < 4:
                continue
            rgb_files.append(os.path.join(path, tok[1]))
            depth_files.append(os.path.join(path, tok[3]))
    return rgb_files, depth_files


def ReadImageSequenceWithPose(path):
    """tool::ReadImageSequenceWithPose (IO.cpp:81-108) -> (rgb_files, depth_files, poses[n,4,4] f32)."""
    traj = os.path.join(path, "trajectory.txt")
    if not os.path.exists(traj):
        print("[ReadImageSequenceWithPose]::[ERROR]::No file named trajectory.txt.")
        return [], [], np.zeros((0, 4, 4), np.float32)
    rgb_files, depth_files = ReadImageSequence(path)
    poses = []
    with open(traj) as f:
        for line in f:
            tok = line.split()
            if len(tok) >= 16:
                poses.append(np.array([np.float32(t) for t in tok[:16]], np.float32).reshape(4, 4))
    if len(poses) != len(rgb_files):
        print("[ReadImageSequenceWithPose]::[WARNING]:: The number of images and poses do not match.")
    return rgb_files, depth_files, np.stack(poses) if poses else np.zeros((0, 4, 4), np.float32)


# ---- the ScanNet layout (tool::ReadImageSequenceFromScannet[WithPose], IO.cpp:109-197; example/GenerateModelFromScannet.cpp) -----------------
#   <dir>/_info.txt                 "key = value" lines: sizes, m_depthShift (the depth scale), the two 4x4 intrinsic matrices, m_frames.size
#   <dir>/frame-%06d.color.jpg      colour image of the colour camera (this repository writes and reads .color.png: no JPEG coder on the path)
#   <dir>/frame-%06d.depth.png      16-bit depth of the depth camera
#   <dir>/frame-%06d.pose.txt       4 x 4 camera-to-world pose
_SCANNET_SKIPPED = ("m_versionNumber", "m_sensorName", "m_calibrationColorExtrinsic", "m_calibrationDepthExtrinsic")


def WriteScannetSequence(path, depths_m, colors_bgr, poses, depth_cam, color_cam, depth_scale=1000, color_ext="png", extra_info_lines=()):
    """Writes a ScanNet-layout directory.  depth_cam / color_cam: (fx, fy, cx, cy, width, height); depth in metres is quantised to
    uint16 = round(d * depth_scale).  extra_info_lines are appended to _info.txt as they are (tests plant an unknown key with them)."""
    from PIL import Image
    os.makedirs(path, exist_ok=True)

    def k4(c):
        return "%.9g 0 %.9g 0 0 %.9g %.9g 0 0 0 1 0 0 0 0 1" % (c[0], c[2], c[1], c[3])

    eye = "1 0 0 0 0 1 0 0 0 0 1 0 0 0 0 1"
    n = len(depths_m)
    with open(os.path.join(path, "_info.txt"), "w") as f:
        f.write("m_versionNumber = 4\nm_sensorName = synthetic\n")
        f.write("m_colorWidth = %d\nm_colorHeight = %d\nm_depthWidth = %d\nm_depthHeight = %d\n" % (color_cam[4], color_cam[5], depth_cam[4], depth_cam[5]))
        f.write("m_depthShift = %d\n" % int(depth_scale))
        f.write("m_calibrationColorIntrinsic = %s\nm_calibrationColorExtrinsic = %s\n" % (k4(color_cam), eye))
        f.write("m_calibrationDepthIntrinsic = %s\nm_calibrationDepthExtrinsic = %s\n" % (k4(depth_cam), eye))
        f.write("m_frames.size = %d\n" % n)
        for line in extra_info_lines:
            f.write(line + "\n")
    for i, (d, c, p) in enumerate(zip(depths_m, colors_bgr, poses)):
        stem = os.path.join(path, "frame-%06d" % i)
        d16 = np.clip(np.round(np.asarray(d, np.float64) * depth_scale), 0, 65535).astype(np.uint16)
        Image.fromarray(d16).save(stem + ".depth.png")
        Image.fromarray(np.ascontiguousarray(np.asarray(c, np.uint8)[:, :, ::-1])).save(stem + ".color." + color_ext)   # stored as RGB
        with open(stem + ".pose.txt", "w") as f:
            for row in np.asarray(p, np.float32).reshape(4, 4):
                f.write(" ".join("%.9g" % float(x) for x in row) + "\n")


def ReadImageSequenceFromScannet(path):
    """tool::ReadImageSequenceFromScannet (IO.cpp:109-175) -> (rgb_files, depth_files, rgb_camera, depth_camera), cameras as
    (fx, fy, cx, cy, width, height, depth_scale) with the colour camera's depth_scale left at the class default 1000.  Like the reference: lines are
    split at " = "; a line that does not split in two, or an unknown key, prints the warning and ENDS the parse (what was read so far is kept);
    the colour names end in .color.jpg whatever is on disk."""
    val = dict(cw=-1, ch=-1, dw=-1, dh=-1, shift=-1, n=0)
    kc, kd = [0.0] * 4, [0.0] * 4
    with open(os.path.join(path, "_info.txt")) as f:
        for line in f:
            parts = [t for t in line.rstrip("\n").split(" = ") if t]
            if len(parts) != 2:
                print("[Warning]::[ReadImageSequenceFromScannet]::Wrong format of _info.txt")
                break
            key, value = parts
            ints = {"m_colorWidth": "cw", "m_colorHeight": "ch", "m_depthWidth": "dw", "m_depthHeight": "dh", "m_depthShift": "shift", "m_frames.size": "n"}
            if key in _SCANNET_SKIPPED:
                continue
            if key in ints:
                val[ints[key]] = int(value.split()[0])
            elif key in ("m_calibrationColorIntrinsic", "m_calibrationDepthIntrinsic"):
                t = [float(np.float32(x)) for x in value.split()]
                (kc if key == "m_calibrationColorIntrinsic" else kd)[:] = [t[0], t[5], t[2], t[6]]   # fx, fy, cx, cy
            else:
                print("[Warning]::[ReadImageSequenceFromScannet]::Wrong format of _info.txt")
                break
    rgb_camera = (kc[0], kc[1], kc[2], kc[3], val["cw"], val["ch"], 1000.0)
    depth_camera = (kd[0], kd[1], kd[2], kd[3], val["dw"], val["dh"], float(val["shift"]))
    rgb_files = [os.path.join(path, "frame-%06d.color.jpg" % i) for i in range(val["n"])]
    depth_files = [os.path.join(path, "frame-%06d.depth.png" % i) for i in range(val["n"])]
    return rgb_files, depth_files, rgb_camera, depth_camera


def ReadImageSequenceFromScannetWithPose(path):
    """tool::ReadImageSequenceFromScannetWithPose (IO.cpp:177-197) -> (rgb_files, depth_files, poses [n, 4, 4] f32, rgb_camera, depth_camera)."""
    rgb_files, depth_files, rgb_camera, depth_camera = ReadImageSequenceFromScannet(path)
    poses = np.zeros((len(rgb_files), 4, 4), np.float32)
    for i in range(len(rgb_files)):
        with open(os.path.join(path, "frame-%06d.pose.txt" % i)) as f:
            poses[i] = np.array([np.float32(t) for t in f.read().split()[:16]], np.float32).reshape(4, 4)
    return rgb_files, depth_files, poses, rgb_camera, depth_camera


def imread(path, unchanged=False):
    """What cv::imread hands the examples: colour as uint8 B,G,R; with unchanged (-1) the stored
    16-bit depth as uint16."""
    from PIL import Image
    img = Image.open(path)
    a = np.array(img)
    if unchanged:
        return a.astype(np.uint16) if a.dtype != np.uint16 else a
    if a.ndim == 2:
        a = np.stack([a, a, a], axis=-1)
    return np.ascontiguousarray(a[:, :, 2::-1].astype(np.uint8))


def ConvertDepthTo32F(depth, depth_scale):
    """tool::ConvertDepthTo32F (ImageProcessing.cpp:68-91): uint16 / depth_scale in float32, negatives -> 0."""
    d = np.asarray(depth)
    if d.dtype == np.float32:
        return d.copy()
    if d.dtype != np.uint16:
        raise SystemExit("[ImageProcessing]::[ERROR]::Unknown depth image type: %s" % d.dtype)
    out = d.astype(np.float32) / np.float32(depth_scale)
    out[out < 0] = 0
    return out


class FramePrefetcher:
    """Decodes the PNG pairs of a sequence ahead of the consumer on a pool of host threads (PIL releases
    the GIL while inflating), so that file IO does not cap the fusion rate (1000 frames/s
    x 2.1 MB = 2.1 GB/s of decoded pixels).  Iterating yields (index, rgb_bgr_u8, depth_u16) in order.

        for i, rgb, depth in FramePrefetcher(rgb_files, depth_files, indices=range(0, n, 10)):
            ...
    """

    def __init__(self, rgb_files, depth_files, indices=None, workers=16, ahead=64):
        from concurrent.futures import ThreadPoolExecutor
        self.rgb_files, self.depth_files = rgb_files, depth_files
        self.indices = list(range(len(rgb_files)) if indices is None else indices)
        self.ahead = max(1, int(ahead))
        self._pool = ThreadPoolExecutor(max_workers=max(1, int(workers)))

    def _load(self, i):
        return i, imread(self.rgb_files[i]), imread(self.depth_files[i], unchanged=True)

    def __iter__(self):
        from collections import deque
        pending = deque()
        it = iter(self.indices)
        try:
            for i in it:
                pending.append(self._pool.submit(self._load, i))
                if len(pending) >= self.ahead:
                    yield pending.popleft().result()
            while pending:
                yield pending.popleft().result()
        finally:
            for f in pending:
                f.cancel()

    def close(self):
        self._pool.shutdown(wait=False)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
