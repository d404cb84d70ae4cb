"""tool::AlignColorToDepth on the device (csrc/align_color.hip) and as the front of the fusion path: byte for byte the numpy restatement of
tests/align_color_common.py (which tests/test_align_color_cpu.py ties to the host loop and to Eigen), and voxel for voxel the volume that fusing the
restatement's aligned images gives."""
import os

import numpy as np
import pytest

import align_color_common as A

pytestmark = pytest.mark.gpu
CASES = A.cases()


def _cam(hip, t):
    c = hip.Camera()
    c.fx, c.fy, c.cx, c.cy, c.width, c.height = t[:6]
    c.depth_scale = t[6] if len(t) > 6 else 1000.0
    return c


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_alignment_is_the_restatement(name, hip):
    import torch
    from onepiece_amd import tool as T
    case = CASES[name]
    want = A.align(**case)
    cc, dc = _cam(hip, case["color_cam"]), _cam(hip, case["depth_cam"])
    got = T.AlignColorToDepth(case["color"], case["depth"], cc, dc, case["color_to_depth"])
    assert np.array_equal(got, want), "host buffers"
    depth = case["depth"]
    d_depth = torch.from_numpy(depth.view(np.int16) if depth.dtype == np.uint16 else depth).cuda()
    d_color = torch.from_numpy(case["color"]).cuda()
    torch.cuda.synchronize()
    d_out = T.AlignColorToDepth(d_color, d_depth, cc, dc, case["color_to_depth"])
    assert np.array_equal(d_out.cpu().numpy(), want), "device buffers"


def test_refusals(hip):
    import ctypes as C
    case = CASES["odd_7x5_13x9"]
    cc, dc = _cam(hip, case["color_cam"]), _cam(hip, case["depth_cam"])
    out = np.zeros((5, 7, 3), np.uint8)
    lib = hip.load()
    vp = lambda a: C.c_void_p(a.ctypes.data)
    call = lambda color, depth, rows, cols: lib.op_align_color_to_depth(C.byref(cc), C.byref(dc), color, rows, cols, depth, hip.OP_DEPTH_F32, None, hip.OP_MEM_HOST, 0, vp(out))
    assert call(None, vp(case["depth"]), 9, 13) == hip.OP_ERR_INVALID
    assert call(vp(case["color"]), None, 9, 13) == hip.OP_ERR_INVALID
    assert call(vp(case["color"]), vp(case["depth"]), 0, 13) == hip.OP_ERR_INVALID
    assert call(vp(case["color"]), vp(case["depth"]), 9, -1) == hip.OP_ERR_INVALID
    from onepiece_amd import tool as T
    with pytest.raises(ValueError):
        T.AlignColorToDepth(case["color"], case["depth"][:4], cc, dc)     # a depth image that is not the depth camera's size


def _sorted_map(handler):
    keys, vox = handler.GetCubeMap()
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    return keys[order], vox[order].view(np.uint32)


@pytest.fixture(scope="module")
def frames35(hip):
    """35 two-camera frames (depth 64 x 48, colour 100 x 80, every frame its own tint) and the volume of the restatement's aligned images."""
    dcam, ccam, M, depths, colors, poses = A.two_camera_frames(35, step=7)
    cd, cc = A.camera(*dcam), A.camera(*ccam)
    aligned = np.stack([A.align(colors[i], depths[i], cc, cd, M) for i in range(35)])
    assert all(aligned[i].any() for i in range(35)) and len({aligned[i].tobytes() for i in range(35)}) == 35
    return dict(dcam=_cam(hip, cd), ccam=_cam(hip, cc), M=M, depths=depths, colors=colors, poses=poses, aligned=aligned)


def _volume(hip, F):
    from onepiece_amd import integration as I
    v = I.CubeHandler(F["dcam"], device=0, max_blocks=1 << 15)
    v.SetVoxelResolution(0.02)
    return v


def _reference_map(hip, F, n):
    b = _volume(hip, F)
    for i in range(n):
        b.IntegrateImage(F["depths"][i], F["aligned"][i], F["poses"][i])
    return _sorted_map(b)


def test_fused_entry_bit_for_bit(hip, frames35):
    F = frames35
    a = _volume(hip, F)
    for i in range(3):
        a.IntegrateImageUnaligned(F["depths"][i], F["colors"][i], F["poses"][i], F["ccam"], F["M"])
    ka, xa = _sorted_map(a)
    kb, xb = _reference_map(hip, F, 3)
    assert len(ka) > 50 and np.array_equal(ka, kb) and np.array_equal(xa, xb)


def test_ring_turnover(hip, frames35):
    """35 frames: a 32-frame batch is launched while later aligned images are being produced, and the ring's slots are told apart by the tints."""
    import torch
    F = frames35
    kb, xb = _reference_map(hip, F, 35)
    d_depth, d_color = torch.from_numpy(F["depths"]).cuda(), torch.from_numpy(F["colors"]).cuda()
    torch.cuda.synchronize()
    seq = _volume(hip, F)
    seq.IntegrateSequenceUnaligned(d_depth, d_color, F["poses"], F["ccam"], F["M"])
    ks, xs = _sorted_map(seq)
    one = _volume(hip, F)
    for i in range(35):
        one.IntegrateImageUnaligned(d_depth[i], d_color[i], F["poses"][i], F["ccam"], F["M"])
    ko, xo = _sorted_map(one)
    host = _volume(hip, F)
    for i in range(35):
        host.IntegrateImageUnaligned(F["depths"][i], F["colors"][i], F["poses"][i], F["ccam"], F["M"])
    kh, xh = _sorted_map(host)
    assert np.array_equal(ks, ko) and np.array_equal(xs, xo), "the sequence form against 35 single calls"
    assert np.array_equal(ks, kb) and np.array_equal(xs, xb), "against the volume of the restatement's images"
    assert np.array_equal(kh, kb) and np.array_equal(xh, xb), "host images through the same ring"
    # twice round the ring (2 x 32 slots) on one volume: 70 more frames, slots reused after their batches retired
    again = _volume(hip, F)
    for rep in range(3):
        again.IntegrateSequenceUnaligned(d_depth, d_color, F["poses"], F["ccam"], F["M"])
    b3 = _volume(hip, F)
    for rep in range(3):
        for i in range(35):
            b3.IntegrateImage(F["depths"][i], F["aligned"][i], F["poses"][i])
    k3, x3 = _sorted_map(again)
    kr, xr = _sorted_map(b3)
    assert np.array_equal(k3, kr) and np.array_equal(x3, xr), "105 frames: every ring slot reused"


@pytest.mark.parametrize("name", ["odd_7x5_13x9", "tile_65x17", "u16_scale1000", "projective_w_zero"])
def test_class_surface_option_off_and_on(name, tmp_path, hip):
    case = CASES[name]
    (tmp_path / "h").mkdir(); (tmp_path / "d").mkdir()
    jh, host = A.align_through_driver(tmp_path / "h", case, "host")
    jd, dev = A.align_through_driver(tmp_path / "d", case, "device")
    assert jh["option_default"] == 0 and jd["option_default"] == 0
    assert np.array_equal(host, A.align(**case)) and np.array_equal(dev, host)


def test_class_surface_falls_back_for_a_depth_image_the_device_entry_is_not_told_of(tmp_path, hip):
    """A depth image smaller than the depth camera: the reference walks the image and writes into a camera-sized output; the device entry knows
    one size only, so the class surface takes the host loop -- without an error, with the same bytes."""
    case = dict(CASES["tile_65x17"])
    case["depth"] = np.ascontiguousarray(case["depth"][:11, :40])
    (tmp_path / "h").mkdir(); (tmp_path / "d").mkdir()
    jh, host = A.align_through_driver(tmp_path / "h", case, "host", depth_image_shape=(11, 40))
    jd, dev = A.align_through_driver(tmp_path / "d", case, "device", depth_image_shape=(11, 40))
    assert host.any() and not host[11:].any() and not host[:, 40:].any()
    assert np.array_equal(dev, host)
    full = A.align(**CASES["tile_65x17"])
    assert np.array_equal(host[:11, :40], full[:11, :40])


def test_class_surface_falls_back_when_the_device_entry_refuses(tmp_path, hip):
    """A colour camera of height 0: the definition never reads that field, so the host loop gives the ordinary image; op_align_color_to_depth
    refuses a non-positive size with OP_ERR_INVALID.  With option 15 on the class surface must take the host loop then, silently."""
    import ctypes as C
    case = dict(CASES["rigid"])
    cc = list(case["color_cam"]); cc[5] = 0
    case["color_cam"] = tuple(cc)
    want = A.align(**CASES["rigid"])
    assert want.any() and np.array_equal(A.align(**case), want)
    out = np.zeros_like(want)
    rc = hip.load().op_align_color_to_depth(C.byref(_cam(hip, case["color_cam"])), C.byref(_cam(hip, case["depth_cam"])), C.c_void_p(case["color"].ctypes.data),
                                            case["color"].shape[0], case["color"].shape[1], C.c_void_p(case["depth"].ctypes.data), hip.OP_DEPTH_F32,
                                            case["color_to_depth"].ctypes.data_as(C.POINTER(C.c_float)), hip.OP_MEM_HOST, 0, C.c_void_p(out.ctypes.data))
    assert rc == hip.OP_ERR_INVALID, "the entry itself refuses this input"
    (tmp_path / "h").mkdir(); (tmp_path / "d").mkdir()
    jh, host = A.align_through_driver(tmp_path / "h", case, "host")
    jd, dev = A.align_through_driver(tmp_path / "d", case, "device")
    assert np.array_equal(host, want) and np.array_equal(dev, want)
    assert "ERROR" not in jd["stdout"]


def test_python_mirrors_check_the_depth_size(hip, frames35):
    import torch
    F = frames35
    v = _volume(hip, F)
    with pytest.raises(ValueError):
        v.IntegrateImageUnaligned(F["depths"][0][:40], F["colors"][0], F["poses"][0], F["ccam"], F["M"])
    d_depth, d_color = torch.from_numpy(F["depths"][:2, :40]).contiguous().cuda(), torch.from_numpy(F["colors"][:2]).cuda()
    with pytest.raises(ValueError):
        v.IntegrateSequenceUnaligned(d_depth, d_color, F["poses"][:2], F["ccam"], F["M"])


def test_driver_three_paths(tmp_path, hip):
    from onepiece_amd import sequence as Q
    dcam, ccam, M, depths, colors, poses = A.two_camera_frames(30, step=3)
    d = str(tmp_path / "scene0000_00")
    # the driver aligns with the identity, as the reference's driver does: the two sensors' offset is simply not modelled there
    Q.WriteScannetSequence(d, depths, colors, poses, dcam, ccam, depth_scale=1000)
    dumps = {}
    for path in ("host", "device", "fused"):
        out = tmp_path / path
        out.mkdir()
        js = A.run_driver([d, "--voxel", 0.02, "--path", path, "--color-ext", "png", "--dump", str(out)])
        assert js["frames"] == 3 and js["of"] == 30 and js["blocks"] > 50
        dumps[path] = A.read_volume_dump(out)
    kh, xh = dumps["host"]
    assert (xh[..., 2:][xh[..., 1] > 0] >= 0).all()
    for path in ("device", "fused"):
        k, x = dumps[path]
        assert np.array_equal(k, kh) and np.array_equal(x.view(np.uint32), xh.view(np.uint32)), path
