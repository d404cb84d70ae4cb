"""tool::AlignColorToDepth (reference Tool/IO.cpp:9-58) restated in numpy, the discriminating inputs of the tests, and the naive variants the
inputs have to tell apart.  DESIGN.md section 0 has the definition in words; this file is the one the CPU and GPU tests compare with.

Every float32 product, quotient and sum below is rounded on its own (numpy float32 arithmetic does not contract), in the reference's order."""
import json
import os
import subprocess

import numpy as np

F = np.float32
IDENTITY = np.eye(4, dtype=np.float32)


def camera(fx, fy, cx, cy, width, height, depth_scale=1000.0):
    return (float(F(fx)), float(F(fy)), float(F(cx)), float(F(cy)), int(width), int(height), float(F(depth_scale)))


def depth_metres(depth, depth_cam):
    d = np.asarray(depth)
    if d.dtype == np.uint16:
        return d.astype(np.float32) / F(depth_cam[6])       # ConvertDepthTo32F: (float)d / depth_scale
    return d.astype(np.float32, copy=False)


def project(depth, color_cam, depth_cam, color_to_depth=None, divide_w=True):
    """(valid, uf, vf, p2): valid = z > 0; uf, vf float32 as IO.cpp:49 leaves them (garbage where not valid)."""
    z = depth_metres(depth, depth_cam)
    h, w = z.shape
    M = IDENTITY if color_to_depth is None else np.asarray(color_to_depth, np.float32).reshape(4, 4)
    fx_d, fy_d, cx_d, cy_d = (F(t) for t in depth_cam[:4])
    fx_c, fy_c, cx_c, cy_c = (F(t) for t in color_cam[:4])
    with np.errstate(all="ignore"):
        valid = z > 0                                         # NaN and negatives fail
        zz = np.where(valid, z, F(1))
        u = np.arange(w, dtype=np.float32)[None, :]
        v = np.arange(h, dtype=np.float32)[:, None]
        x = (u - cx_d) * zz / fx_d                            # Geometry.cpp:94-96
        y = (v - cy_d) * zz / fy_d
        one = F(1)
        q = [((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * zz) + M[r, 3] * one for r in range(4)]   # Geometry.cpp:31-32
        if divide_w:
            p0, p1, p2 = q[0] / q[3], q[1] / q[3], q[2] / q[3]   # :33
        else:
            p0, p1, p2 = q[0], q[1], q[2]
        a, b, c = p0 / p2, p1 / p2, p2 / p2                   # IO.cpp:49
        uf = fx_c * a + cx_c * c
        vf = fy_c * b + cy_c * c
    assert uf.dtype == np.float32 and vf.dtype == np.float32
    return valid, uf, vf, p2


def _to_int(t, nearest=False):
    """(int)((double)t + 0.5): truncation toward zero; (ok, value) with ok False for NaN and for values whose truncation is no int."""
    with np.errstate(all="ignore"):
        d = np.rint(t.astype(np.float64)) if nearest else t.astype(np.float64) + 0.5
    ok = (d > -2147483649.0) & (d < 2147483648.0)             # NaN fails both
    val = np.trunc(np.where(ok, d, 0.0)).astype(np.int64)
    return ok, val


def align(color, depth, color_cam, depth_cam, color_to_depth=None, variant=None):
    """The definition.  variant: None, or one of the naive readings the tests must be able to tell from it:
    'nearest' (round to nearest instead of + 0.5 and truncate), 'color_height' (the colour camera's height as the vertical bound),
    'front_only' (additionally p2 > 0), 'no_w' (no division by q.w)."""
    color = np.ascontiguousarray(color, np.uint8)
    hc, wc = color.shape[:2]
    z = depth_metres(depth, depth_cam)
    assert z.shape == (depth_cam[5], depth_cam[4]), "the depth image has the depth camera's size"
    valid, uf, vf, p2 = project(depth, color_cam, depth_cam, color_to_depth, divide_w=variant != "no_w")
    oku, cu = _to_int(uf, variant == "nearest")
    okv, cv = _to_int(vf, variant == "nearest")
    v_bound = color_cam[5] if variant == "color_height" else depth_cam[5]     # IO.cpp:33: the DEPTH camera's height
    acc = valid & oku & okv & (cu >= 0) & (cu < color_cam[4]) & (cv >= 0) & (cv < v_bound)
    acc &= (cu < wc) & (cv < hc)                               # the one deviation: never read outside the image that was passed
    if variant == "front_only":
        with np.errstate(all="ignore"):
            acc &= p2 > 0
    out = np.zeros(z.shape + (3,), np.uint8)
    out[acc] = color[cv[acc], cu[acc]]
    return out


VARIANTS = ("nearest", "color_height", "front_only", "no_w")


def _color(rng, h, w):
    # every pixel distinct from its neighbours and never (0, 0, 0): a wrong or a missing sample shows
    return rng.integers(1, 256, size=(h, w, 3), dtype=np.uint8)


def _rigid(rx, ry, rz, t):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    R = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = t
    return M.astype(np.float32)


def _next(x, n):
    x = F(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, F(np.inf) if n > 0 else F(-np.inf))
    return x


def cases():
    """name -> dict(color, depth, color_cam, depth_cam, color_to_depth).  All tiny."""
    rng = np.random.default_rng(20240917)
    out = {}

    def add(name, color, depth, ccam, dcam, M=None):
        out[name] = dict(color=np.ascontiguousarray(color), depth=np.ascontiguousarray(depth), color_cam=ccam, depth_cam=dcam,
                         color_to_depth=None if M is None else np.ascontiguousarray(M, np.float32))

    # odd sizes: 3-byte stores and rows that start at any byte offset
    d = rng.uniform(0.5, 3.0, (5, 7)).astype(np.float32)
    add("odd_7x5_13x9", _color(rng, 9, 13), d, camera(11.0, 10.5, 6.2, 4.4, 13, 9), camera(6.1, 5.9, 3.3, 2.4, 7, 5), _rigid(0.01, -0.02, 0.015, (0.02, -0.01, 0.005)))
    # one pixel past a 64 x 16 tile both ways
    d = rng.uniform(0.4, 4.0, (17, 65)).astype(np.float32)
    add("tile_65x17", _color(rng, 40, 90), d, camera(70.0, 69.0, 44.5, 19.5, 90, 40), camera(52.0, 51.0, 32.0, 8.2, 65, 17), _rigid(0.0, 0.03, 0.0, (0.05, 0.0, 0.0)))
    # uint16 depth, depth_scale 1000, zeros included
    d16 = rng.integers(0, 4000, (12, 20)).astype(np.uint16)
    d16[::3, ::4] = 0
    add("u16_scale1000", _color(rng, 24, 30), d16, camera(25.0, 25.0, 14.7, 11.9, 30, 24), camera(17.0, 17.0, 9.6, 5.8, 20, 12, 1000.0), _rigid(0.02, 0.0, -0.01, (-0.03, 0.02, 0.0)))
    # zeros, negatives, NaN, inf
    d = rng.uniform(0.5, 2.0, (9, 11)).astype(np.float32)
    d[0, :] = 0.0; d[1, ::2] = -1.5; d[2, 1::2] = np.nan; d[3, 3] = np.inf; d[4, 4] = -0.0
    add("bad_depth", _color(rng, 9, 11), d, camera(9.0, 9.0, 5.0, 4.0, 11, 9), camera(9.0, 9.0, 5.0, 4.0, 11, 9))
    # rotation + translation
    d = rng.uniform(0.8, 2.5, (14, 18)).astype(np.float32)
    add("rigid", _color(rng, 30, 36), d, camera(30.0, 29.0, 18.2, 14.6, 36, 30), camera(15.0, 15.0, 9.1, 7.2, 18, 14), _rigid(0.05, -0.04, 0.1, (0.1, -0.05, 0.02)))
    # projective last row: w != 1, and != a constant
    M = _rigid(0.0, 0.02, 0.0, (0.01, 0.0, 0.0))
    M[3] = (0.02, -0.01, 0.1, 0.9)
    add("projective_w", _color(rng, 30, 36), d, camera(30.0, 29.0, 18.2, 14.6, 36, 30), camera(15.0, 15.0, 9.1, 7.2, 18, 14), M)
    # planted uf: identity transform, fx = fy = 1, z = 1, colour cx = 0, so that uf of depth column 1 is x = 1 - cx_d; cx_d = 1 - t plants the
    # target t (both subtractions are exact for these values: test_planted_targets_land_where_intended).  One 3 x 2 depth image per target.
    wc = 8
    targets = [F(-1.25), F(-0.75), F(-0.5), F(0.25), F(0.5), _next(wc - 0.5, -1), F(wc - 0.5), _next(wc - 0.5, 1), F(3.0e9), F(-3.0e9), F(2147483520.0), F(1.5)]
    for i, t in enumerate(targets):
        dcam = camera(1.0, 1.0, float(F(1.0) - t), 0.0, 3, 2)
        dd = np.ones((2, 3), np.float32)
        add("planted_uf_%02d" % i, _color(rng, 4, wc), dd, camera(1.0, 1.0, 0.0, 0.0, wc, 4), dcam)
    # w == 0 on one row (z == 1): p is NaN there and the pixel is rejected; without the division it would be sampled
    M = np.eye(4, dtype=np.float32)
    M[3] = (0.0, 0.0, 1.0, -1.0)
    d = rng.uniform(1.5, 2.5, (6, 8)).astype(np.float32)
    d[3, :] = 1.0
    add("projective_w_zero", _color(rng, 6, 8), d, camera(6.0, 6.0, 4.0, 3.0, 8, 6), camera(6.0, 6.0, 4.0, 3.0, 8, 6), M)
    # p2 < 0 (behind the colour camera, still sampled) and p2 == 0
    M = np.eye(4, dtype=np.float32)
    M[2, 2] = -1.0                                            # p2 = -z
    add("behind_color_camera", _color(rng, 10, 12), rng.uniform(0.5, 2.0, (10, 12)).astype(np.float32), camera(8.0, 8.0, 6.0, 5.0, 12, 10), camera(8.0, 8.0, 6.0, 5.0, 12, 10), M)
    M = np.eye(4, dtype=np.float32)
    M[2, 3] = -1.0                                            # p2 = z - 1: exactly 0 where z == 1, negative below
    d = rng.uniform(0.5, 2.0, (6, 8)).astype(np.float32)
    d[2, :] = 1.0
    add("p2_zero", _color(rng, 6, 8), d, camera(6.0, 6.0, 4.0, 3.0, 8, 6), camera(6.0, 6.0, 4.0, 3.0, 8, 6), M)
    # depth_cam.height < colour rows: colour rows at and below that height are never sampled (the colour camera sees more, vertically)
    d = rng.uniform(0.8, 2.0, (8, 16)).astype(np.float32)
    add("depth_height_below_color_rows", _color(rng, 24, 16), d, camera(12.0, 36.0, 8.0, 12.0, 16, 24), camera(12.0, 12.0, 8.0, 4.0, 16, 8))
    # depth_cam.height > colour rows: rows the reference would read past its image are rejected
    d = rng.uniform(0.8, 2.0, (20, 10)).astype(np.float32)
    add("depth_height_above_color_rows", _color(rng, 6, 10), d, camera(8.0, 8.0, 5.0, 10.0, 10, 6), camera(8.0, 8.0, 5.0, 10.0, 10, 20))
    # equal cameras + identity: the colour image itself wherever z > 0 (integer cx, cy and powers of two keep uf == u exactly)
    d = rng.uniform(0.5, 3.0, (16, 24)).astype(np.float32)
    d[5, 5] = 0.0
    add("equal_cameras_identity", _color(rng, 16, 24), d, camera(16.0, 16.0, 12.0, 8.0, 24, 16), camera(16.0, 16.0, 12.0, 8.0, 24, 16))
    return out


def two_camera_frames(n, width=64, height=48, cwidth=100, cheight=80, first=100, step=1):
    """n synthetic two-camera frames of the analytic room (onepiece_amd.synthetic): (depth_cam, color_cam, color_to_depth, depths, colors, poses)."""
    from onepiece_amd import synthetic as S
    depths, colors, poses = [], [], []
    dcam = ccam = M = None
    for i in range(n):
        pose = S.room_pose(first + i * step)
        d, c, dcam, ccam, M = S.room_render_two_cameras(pose, width=width, height=height, color_width=cwidth, color_height=cheight, tint=i)
        depths.append(d); colors.append(c); poses.append(pose.astype(np.float32))
    return dcam, ccam, M, np.stack(depths), np.stack(colors), np.stack(poses)


# ---- the class surface through examples/cpp/ScannetIntegration.bin ----------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "examples", "cpp", "ScannetIntegration.bin")


def write_case(tmp, case, depth_image_shape=None):
    """params.txt, color.u8 and depth.f32 | depth.u16 as ScannetIntegration --align (and tests/cpp/align_eigen_check.cpp) read them."""
    tmp = str(tmp)
    color, depth = case["color"], case["depth"]
    M = IDENTITY if case["color_to_depth"] is None else case["color_to_depth"]
    u16 = depth.dtype == np.uint16
    nums = list(case["color_cam"][:6]) + list(case["depth_cam"][:7]) + [color.shape[0], color.shape[1], int(u16)] + [float(t) for t in np.asarray(M, np.float32).reshape(16)]
    if depth_image_shape is not None:
        nums += list(depth_image_shape)
    with open(os.path.join(tmp, "params.txt"), "w") as f:
        f.write(" ".join(repr(float(t)) if isinstance(t, float) else str(int(t)) for t in nums) + "\n")
    color.tofile(os.path.join(tmp, "color.u8"))
    depth.tofile(os.path.join(tmp, "depth.u16" if u16 else "depth.f32"))


def run_driver(args, timeout=300, with_output=False):
    r = subprocess.run([DRIVER] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, "ScannetIntegration.bin %s failed (%d):\n%s\n%s" % (" ".join(map(str, args)), r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    js = json.loads(r.stdout.strip().splitlines()[-1])
    return (js, r.stdout) if with_output else js


def align_through_driver(tmp, case, path, depth_image_shape=None):
    """tool::AlignColorToDepth of the class surface on one case -> (result json with the driver's whole output under "stdout", aligned image)."""
    write_case(tmp, case, depth_image_shape)
    js, text = run_driver(["--align", str(tmp), "--path", path], with_output=True)
    js["stdout"] = text
    out = np.fromfile(os.path.join(str(tmp), "aligned.u8"), np.uint8)
    return js, out.reshape(case["depth_cam"][5], case["depth_cam"][4], 3)


def read_volume_dump(d):
    keys = np.fromfile(os.path.join(str(d), "volume_keys.i32"), np.int32).reshape(-1, 3)
    vox = np.fromfile(os.path.join(str(d), "volume_voxels.f32"), np.float32).reshape(len(keys), 512, 5)
    return keys, vox
