"""What tests/test_downsample_cpu.py and tests/test_downsample_gpu.py share: the numpy float32 restatement of geometry::PointCloud::DownSample
(host/one_piece/src/PointCloud.cpp:88-115) and of geometry::TransformPoint (Geometry.cpp:19-23), the clouds both files plant, and the driver."""
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "examples", "cpp", "SubmapModel.bin")
f32 = np.float32


def cells_of(points, grid_len):
    """(int)floorf(p / grid_len) per axis: an IEEE float32 division, then floor."""
    return np.floor(np.asarray(points, f32) / f32(grid_len)).astype(np.int64)


def downsample_ref(points, grid_len, colors=None, normals=None):
    """The host loop, restated: points in input order, a float32 accumulator row per cell in order of first appearance, one division by
    float32(count) at the end.  -> (points, colors or None, normals or None)."""
    arrays = [np.ascontiguousarray(a, f32).reshape(-1, 3) for a in (points, colors, normals) if a is not None]
    cells = cells_of(arrays[0], grid_len)
    slot_of, counts = {}, []
    sums = [np.zeros_like(a) for a in arrays]
    for i, cell in enumerate(map(tuple, cells.tolist())):
        j = slot_of.get(cell)
        if j is None:
            slot_of[cell] = len(counts)
            for s, a in zip(sums, arrays):
                s[len(counts)] = a[i]
            counts.append(1)
        else:
            for s, a in zip(sums, arrays):
                s[j] += a[i]  # float32 row += float32 row: three separate adds
            counts[j] += 1
    m = len(counts)
    div = np.asarray(counts, f32).reshape(-1, 1)
    out = [s[:m] / div for s in sums]
    assert all(o.dtype == f32 for o in out)
    it = iter(out)
    return tuple(next(it) if a is not None else None for a in (points, colors, normals))


def transform_ref(T, points):
    """TransformPoint: ((T(r,0) x + T(r,1) y) + T(r,2) z) + T(r,3) * 1.0f per row, the first three divided by the fourth."""
    T = np.asarray(T, f32).reshape(4, 4)
    p = np.asarray(points, f32).reshape(-1, 3)
    q = [((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] * f32(1.0) for r in range(4)]
    out = np.stack([q[0] / q[3], q[1] / q[3], q[2] / q[3]], axis=1)
    assert out.dtype == f32
    return out


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(got, want):
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


def random_cloud(n, seed, attributes=2):
    """n points in a 2 m cube around the origin, with colours in [0, 1] and unit normals."""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-1.0, 1.0, size=(n, 3)).astype(f32)
    col = rng.uniform(0.0, 1.0, size=(n, 3)).astype(f32)
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-9)).astype(f32)
    return pts, (col if attributes >= 1 else None), (nrm if attributes >= 2 else None)


def too_wide_cloud(grid_len=0.05, seed=3):
    """A cloud 3 * 10^6 cells wide on x: more than the packed key of the device entry holds, nothing the host loop minds."""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-1.0, 1.0, size=(500, 3)).astype(f32)
    pts[::7, 0] += f32(3.0e6 * grid_len)
    col = rng.uniform(0.0, 1.0, size=(500, 3)).astype(f32)
    return pts, col


def run_driver(args, timeout=300):
    r = subprocess.run([DRIVER] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, "SubmapModel.bin %s failed (%d):\n%s\n%s" % (" ".join(map(str, args)), r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def read_cloud(directory, tag):
    """-> (points, colors) of a dump; a missing or empty colour file gives None."""
    pts = np.fromfile(os.path.join(directory, tag + "_points.f32"), f32).reshape(-1, 3)
    cfile = os.path.join(directory, tag + "_colors.f32")
    col = np.fromfile(cfile, f32).reshape(-1, 3) if os.path.exists(cfile) and os.path.getsize(cfile) else None
    return pts, col


def downsample_through_driver(tmp, path, points, colors, grid_len):
    """One cloud through geometry::PointCloud::DownSample of the class surface (SubmapModel.bin --cloud) -> (result.json, points, colors)."""
    tmp = str(tmp)
    np.ascontiguousarray(points, f32).tofile(os.path.join(tmp, "in_points.f32"))
    args = ["--cloud", os.path.join(tmp, "in_points.f32"), "--grid", repr(float(grid_len)), "--path", path, "--dump", tmp]
    if colors is not None:
        np.ascontiguousarray(colors, f32).tofile(os.path.join(tmp, "in_colors.f32"))
        args += ["--colors", os.path.join(tmp, "in_colors.f32")]
    js = run_driver(args)
    return (js,) + read_cloud(tmp, "cloud")
