"""Voxel-grid down-sampling on the device (op_point_cloud_downsample, op_points_from_rgbd_downsampled, the opt-in class surface) against the
numpy float32 restatement of the host loop (downsample_common.downsample_ref; tests/test_downsample_cpu.py pins that one to the host loop itself).
Every comparison is bitwise, on points, colours, normals and the count: there are no tolerances.  The shapes are the smallest at which each
kernel can go wrong: around the wave and the workgroup, more than one sort tile, more than 65 536 cells, one cell that holds everything."""
import ctypes as C
import os

import numpy as np
import pytest

import downsample_common as D

pytestmark = pytest.mark.gpu
f32 = np.float32
GRID = 0.05

_reference = {}


def reference(key, make):
    """key -> (inputs, restated outputs), computed once and shared; nobody writes to either."""
    if key not in _reference:
        ins = make()
        _reference[key] = (ins, D.downsample_ref(ins[0], ins[3], ins[1], ins[2]))
        for a in _reference[key][0][:3] + _reference[key][1]:
            if a is not None:
                a.setflags(write=False)
    return _reference[key]


def device_downsample(R, pts, col, nrm, g):
    pcd, c = R.PointCloud(pts, nrm).DownSample(g, col)
    return pcd.points, c, pcd.normals


def check(got, want):
    for name, a, b in zip(("points", "colors", "normals"), got, want):
        if b is None or (a is None and len(b) == 0):  # (an empty cloud has no normals to carry)
            assert a is None, name
        else:
            assert a is not None and a.shape == b.shape, "%s: %s cells, expected %s" % (name, None if a is None else a.shape, b.shape)
            assert np.array_equal(D.bits(a), D.bits(b)), "%s differ in %d of %d words" % (name, int((D.bits(a) != D.bits(b)).sum()), b.size)


# ---- 1. sizes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attributes", [0, 1, 2], ids=["bare", "colors", "colors+normals"])
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 257, 4097, 70001])
def test_sizes(hip, n, attributes):
    from onepiece_amd import registration as R
    (pts, col, nrm, g), want = reference(("sizes", n), lambda: D.random_cloud(n, 100 + n) + (GRID,))
    use = (pts, col if attributes >= 1 else None, nrm if attributes >= 2 else None)
    check(device_downsample(R, *use, g), (want[0], want[1] if attributes >= 1 else None, want[2] if attributes >= 2 else None))


# ---- 2. one cell holds everything ----------------------------------------------------------------------------------------------------------
def _one_cell(n):
    rng = np.random.default_rng(7000 + n)
    spread = lambda: (rng.uniform(1.0, 2.0, size=(n, 3)) * 2.0 ** rng.integers(2, 10, size=(n, 3))).astype(f32)  # [4, 1024): eight binades
    return spread(), spread() / f32(1024), None, 1024.0


def _pairwise(a):
    a = a.copy()
    while len(a) > 1:
        if len(a) & 1:
            a = np.concatenate([a, np.zeros((1, a.shape[1]), f32)])
        a = a[0::2] + a[1::2]
    return a[0]


@pytest.mark.parametrize("n", [3000, 70001])
def test_one_cell_holds_everything(hip, n):
    from onepiece_amd import registration as R
    (pts, col, _, g), want = reference(("one_cell", n), lambda: _one_cell(n))
    assert len(want[0]) == 1
    in_order = np.cumsum(pts, axis=0, dtype=f32)[-1]          # the CPU's in-order float32 sum ...
    assert np.array_equal(D.bits(in_order / f32(n)), D.bits(want[0][0]))
    backwards = np.cumsum(pts[::-1], axis=0, dtype=f32)[-1]  # ... differs in bits from the reversed and from the pairwise sum, on every axis:
    assert (D.bits(in_order) != D.bits(backwards)).all() and (D.bits(in_order) != D.bits(_pairwise(pts))).all()  # an atomic or a tree sum cannot pass
    check(device_downsample(R, pts, col, None, g), want)


# ---- 3. every point its own cell -----------------------------------------------------------------------------------------------------------
def _own_cells(n=70001, side=48):
    rng = np.random.default_rng(31)
    ids = rng.permutation(side ** 3)[:n]  # distinct cells, in shuffled order
    cell = np.stack([ids // (side * side), (ids // side) % side, ids % side], axis=1) - side // 2
    pts = ((cell + 0.5) * GRID).astype(f32)
    return pts, rng.uniform(0, 1, size=(n, 3)).astype(f32), None, GRID


def test_every_point_its_own_cell(hip):
    from onepiece_amd import registration as R
    (pts, col, _, g), want = reference("own_cells", _own_cells)
    assert len(want[0]) == len(pts) > 65536
    got = device_downsample(R, pts, col, None, g)
    check(got, want)
    assert D.same_bits(got[0], pts) and D.same_bits(got[1], col)  # first appearance = input order; x / 1.0f = x


# ---- 4. interleaved members ----------------------------------------------------------------------------------------------------------------
def _interleaved(n=60000, n_cells=300):
    rng = np.random.default_rng(41)
    origin = rng.permutation(40 ** 3)[:n_cells]
    origin = np.stack([origin // 1600, (origin // 40) % 40, origin % 40], axis=1) - 20
    member = np.arange(n) % n_cells  # round-robin: a cell's members span the whole input
    pts = ((origin[member] + rng.uniform(0.05, 0.95, size=(n, 3))) * GRID).astype(f32)
    return pts, rng.uniform(0, 1, size=(n, 3)).astype(f32), None, GRID, member


def test_interleaved_members_and_the_same_cloud_sorted_by_cell(hip):
    from onepiece_amd import registration as R
    pts, col, _, g, member = _interleaved()
    (_, _, _, _), want = reference("interleaved", lambda: (pts, col, None, g))
    assert len(want[0]) == 300
    check(device_downsample(R, pts, col, None, g), want)
    order = np.argsort(member, kind="stable")
    (spts, scol, _, _), swant = reference("interleaved_sorted", lambda: (pts[order].copy(), col[order].copy(), None, g))
    check(device_downsample(R, spts, scol, None, g), swant)
    assert D.same_bits(swant[0], want[0])  # the restatement says: same members in the same order, same first appearances -> the same cloud


# ---- 5. cell boundaries --------------------------------------------------------------------------------------------------------------------
def _reciprocal_mismatches(g, want=100):
    """float32 values p with floorf(p / g) != floorf(p * (1.0f / g)): multiples of g and the floats around them."""
    g = f32(g)
    k = np.arange(-60000, 60000, dtype=f32)
    base = k * g
    cand = [base]
    for _ in range(2):
        cand += [np.nextafter(cand[-1], f32(np.inf))]
    cand += [np.nextafter(base, f32(-np.inf))]
    p = np.unique(np.concatenate(cand))
    bad = p[np.floor(p / g) != np.floor(p * (f32(1.0) / g))]
    assert len(bad) >= want, "only %d values found for grid_len %g" % (len(bad), g)
    return bad[:: max(1, len(bad) // (3 * want))][: 3 * want]


def _boundaries(g):
    rng = np.random.default_rng(51)
    planted = _reciprocal_mismatches(g)
    x = np.concatenate([planted, np.nextafter(planted, f32(-np.inf)), np.nextafter(planted, f32(np.inf))])  # neighbours on either side
    k = np.arange(-50, 50, dtype=f32) * f32(g)  # exactly on k * grid_len, negative ones included, and one float below
    x = np.concatenate([x, k, np.nextafter(k, f32(-np.inf))]).astype(f32)
    x = np.concatenate([x, x])  # every value twice, so every cell has members to sum
    y = lambda: rng.uniform(-0.12, -0.105, len(x)).astype(f32)  # one (negative) cell of every grid_len used here
    const = np.full(len(x), 0.012, f32)
    pts = np.concatenate([np.stack([x, y(), const], axis=1), np.stack([const, y(), x], axis=1)])  # the planted values decide x cells, then z cells
    pts = np.ascontiguousarray(pts[rng.permutation(len(pts))])
    return pts, rng.uniform(0, 1, size=pts.shape).astype(f32), None, g


@pytest.mark.parametrize("g", [0.025, 0.05, 0.1])
def test_cell_boundaries(hip, g):
    from onepiece_amd import registration as R
    (pts, col, _, _), want = reference(("boundaries", g), lambda: _boundaries(g))
    assert (pts < 0).any() and (D.cells_of(pts, g) != np.trunc(pts / f32(g))).any()  # floor is not trunc here
    check(device_downsample(R, pts, col, None, g), want)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["nan", "inf", "beyond_int", "too_wide", "grid_len_0"])
def test_refusals_return_their_code_and_leave_the_device_usable(hip, what):
    from onepiece_amd import registration as R
    (pts, col, nrm, g), want = reference(("sizes", 4097), lambda: D.random_cloud(4097, 100 + 4097) + (GRID,))
    bad, code = pts.copy(), hip.OP_ERR_INVALID
    if what == "nan":
        bad[1234, 1] = np.nan
    elif what == "inf":
        bad[4096, 2] = -np.inf
    elif what == "beyond_int":
        bad[77, 0] = 1.0e9  # / 0.05 = 2e10
    elif what == "too_wide":
        bad, _ = D.too_wide_cloud(g)
        code = hip.OP_ERR_CAPACITY
    with pytest.raises(hip.OnePieceHipError) as e:
        R.PointCloud(bad).DownSample(0.0 if what == "grid_len_0" else g)
    assert e.value.code == code
    if what == "too_wide":
        assert "3000" in str(e.value)  # the message names the extent (3 000 0xx cells)
    check(device_downsample(R, pts, col, nrm, g), want)


# ---- 7. device memory ----------------------------------------------------------------------------------------------------------------------
def test_device_memory_gives_the_same_bits(hip):
    import torch
    from onepiece_amd import registration as R
    (pts, col, nrm, g), want = reference(("sizes", 4097), lambda: D.random_cloud(4097, 100 + 4097) + (GRID,))
    dev = [torch.from_numpy(a.copy()).cuda() for a in (pts, col, nrm)]
    got = R.DownSampleArrays(dev[0], dev[1], dev[2], g)
    assert all(t.is_cuda for t in got)
    check([t.cpu().numpy() for t in got], want)
    assert D.same_bits(dev[0].cpu().numpy(), pts)  # inputs are read, never written


# ---- 8. fused entry ------------------------------------------------------------------------------------------------------------------------
def _frame(w, h, fmt):
    from onepiece_amd import integration as I
    rng = np.random.default_rng(w * 1000 + h)
    cam = I.PinholeCamera()
    cam.width, cam.height = w, h
    cam.fx = cam.fy = 0.8 * w
    cam.cx, cam.cy = w / 2 - 0.5, h / 2 - 0.25
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    z = 1.5 + 0.4 * np.sin(u / 9.0) + 0.3 * np.cos(v / 7.0)  # a smooth surface 0.8 .. 2.2 m away: neighbouring pixels share 5 cm cells
    invalid = rng.uniform(size=(h, w)) < 0.15
    invalid[1, 2] = True
    if fmt == "u16":
        cam.depth_scale = 1000.0
        depth = np.round(z * 1000.0).astype(np.uint16)
        depth[invalid] = 0
    else:
        cam.depth_scale = 1.0
        depth = z.astype(f32)
        depth[invalid] = 0.0
        depth[0, 0], depth[h - 1, w - 1] = np.nan, -1.0
    rgb = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    return cam, depth, rgb


def _pose():
    a, b = 0.3, -0.2
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rz @ Rx, (0.31, -1.27, 0.08)
    return T.astype(f32)


@pytest.mark.parametrize("fmt", ["u16", "f32"])
@pytest.mark.parametrize("shape", [(4, 4), (33, 17), (161, 121)], ids=lambda s: "%dx%d" % s)
def test_fused_entry(hip, shape, fmt):
    from onepiece_amd import registration as R
    cam, depth, rgb = _frame(shape[0], shape[1], fmt)
    loaded, colors = R.LoadFromRGBD(rgb, depth, cam)
    assert 0 < len(loaded.points) < shape[0] * shape[1]  # invalid pixels were planted and dropped
    T = _pose()
    want = D.downsample_ref(D.transform_ref(T, loaded.points), GRID, colors)
    got, got_c = R.LoadFromRGBDDownSampled(rgb, depth, cam, T, GRID)
    check((got.points, got_c, None), want)
    if shape != (4, 4):
        assert len(want[0]) < len(loaded.points)  # cells with several members
    plain, plain_c = R.LoadFromRGBDDownSampled(rgb, depth, cam, None, GRID)  # T = NULL: LoadFromRGBD + DownSample
    two_steps = device_downsample(R, loaded.points, colors, None, GRID)
    check((plain.points, plain_c, None), two_steps)
    check(two_steps, D.downsample_ref(loaded.points, GRID, colors))


# ---- 9. class surface ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def submap_dumps(tmp_path_factory):
    assert os.path.exists(D.DRIVER), "examples/cpp/SubmapModel.bin is not built (make -C examples/cpp)"
    out = {}
    for path in ("host", "device", "fused"):
        d = str(tmp_path_factory.mktemp("submap_" + path))
        out[path] = (d, D.run_driver(["--frames", 3, "--warmup", 0, "--path", path, "--dump", d]))
    return out


def test_submap_model_is_the_same_cloud_on_all_three_paths(hip, submap_dumps):
    host_dir, host_js = submap_dumps["host"]
    assert 1000 <= host_js["final_points"] <= 20000
    assert len(host_js["frame_points"]) == 3 and host_js["merged_points"] == sum(host_js["frame_points"])
    for path in ("device", "fused"):
        d, js = submap_dumps[path]
        assert js["path"] == path
        assert (js["frame_points"], js["merged_points"], js["final_points"]) == (host_js["frame_points"], host_js["merged_points"], host_js["final_points"])
        for tag in ["frame_%02d" % i for i in range(3)] + ["merged", "final"]:
            (hp, hc), (p, c) = D.read_cloud(host_dir, tag), D.read_cloud(d, tag)
            assert len(hp) > 0 and hc is not None and c is not None
            assert D.same_bits(p, hp) and D.same_bits(c, hc), "%s: %s differs from the host path" % (path, tag)


def test_class_surface_falls_back_for_a_cloud_the_device_refuses(hip, tmp_path):
    pts, col = D.too_wide_cloud(GRID)
    (tmp_path / "host").mkdir()
    (tmp_path / "device").mkdir()
    _, host_p, host_c = D.downsample_through_driver(tmp_path / "host", "host", pts, col, GRID)
    _, dev_p, dev_c = D.downsample_through_driver(tmp_path / "device", "device", pts, col, GRID)
    want = D.downsample_ref(pts, GRID, col)
    check((host_p, host_c, None), want)
    check((dev_p, dev_c, None), want)
    ok_p, ok_c, _ = D.random_cloud(4097, 100 + 4097)  # and a cloud the device takes goes through it with the same bits
    (tmp_path / "ok").mkdir()
    _, p, c = D.downsample_through_driver(tmp_path / "ok", "device", ok_p, ok_c, GRID)
    check((p, c, None), D.downsample_ref(ok_p, GRID, ok_c))
