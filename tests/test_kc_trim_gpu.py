"""k_integrate's trimmed frame loop (csrc/integrate.hip: the folded pixel certificate of project_pixel<true>, voxel_update<true, true> without
the weight half of its guard, the wave-uniform `changed` masks and the scalar count of written voxels, the weight sum formed in place) against
the CPU oracle: block keys, every voxel bit for bit, voxels_updated and voxels_written equal to the oracle's counts.

The set-up of tests/test_kc_lean_gpu.py: a 33-frame sequence = one full 32-frame launch (the stealing draw) + a 1-frame launch (the chunk draw),
at 160 x 120 and at 150 x 101 (sides that are no multiples of the 64 x 16 pixel tiles of the frame preparation), into 4 cm voxels.  Truncation
0.1 takes the lean update (only the numerator half of the guard is compiled), 1.5 the one with the select (both halves).  voxels_written counts,
per launch, the voxels the launch stored: for the oracle, the voxels whose weight differs before and after the launch's frames."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from onepiece_amd import integration as I, synthetic as S

RES = 0.04
N = 33
CAMS = {
    "160x120": (S.FX / 4, S.FY / 4, S.CX / 4, S.CY / 4, 160, 120, 1000.0),
    "150x101": (S.FX / 4, S.FY / 4, 74.5, 50.0, 150, 101, 1000.0),
}
SNAPS = (1, 10, 32)   # frames after which the oracle's volume is kept: the launch boundaries the tests below use
_cache = {}


def _frames(shape):
    """(depth [N,h,w], rgb [N,h,w,3], poses [N,4,4]) on the host, rendered once per shape; frames 6 apart so that the views overlap."""
    key = ("frames", shape)
    if key not in _cache:
        cam = CAMS[shape]
        poses = np.stack([S.room_pose(300 + 6 * k) for k in range(N)]).astype(np.float32)
        fr = [S.room_render(p, width=cam[4], height=cam[5], fx=cam[0], fy=cam[1], cx=cam[2], cy=cam[3]) for p in poses]
        _cache[key] = (np.stack([f[0] for f in fr]), np.stack([f[1] for f in fr]), poses)
    return _cache[key]


def _device(shape):
    import torch
    key = ("device", shape)
    if key not in _cache:
        d, c, _p = _frames(shape)
        dev = torch.device("cuda:0")
        _cache[key] = (torch.from_numpy(d).to(dev).contiguous(), torch.from_numpy(c).to(dev).contiguous())
        torch.cuda.synchronize()
    return _cache[key]


def _oracle_run(oracle, shape, trunc):
    """The oracle's volume after the N frames, frame by frame, computed once and read-only: keys, voxels, blocks selected and voxels updated
    per frame, and {n: (keys, voxels)} after the first n frames for n in SNAPS."""
    key = ("oracle", shape, trunc)
    if key not in _cache:
        d, c, poses = _frames(shape)
        ov = oracle.Volume(oracle.make_camera(*CAMS[shape]), voxel_res=RES, trunc=trunc)
        sel, upd, snaps = [], [], {}
        for k in range(N):
            n, _vis, nu = ov.integrate(d[k], c[k], poses[k])
            sel.append(n); upd.append(nu)
            if k + 1 in SNAPS:
                snaps[k + 1] = ov.export()
        ok, ox = ov.export()
        ox.setflags(write=False)
        _cache[key] = (ok, ox, sel, upd, snaps)
    return _cache[key]


def _written(before, after):
    """Voxels a launch that took the volume from `before` to `after` (each (keys, voxels), or None for the empty volume) has stored: those
    whose bits differ.  (An update always changes the weight at truncations < 1; from 1 on it can replace a voxel of weight 1 by another.)"""
    ka, xa = after
    xa = xa.view(np.uint32)
    if before is None:
        return int((xa[..., 1] != np.float32(0).view(np.uint32)).sum())
    kb, xb = before
    row = {tuple(k): i for i, k in enumerate(kb)}
    default = np.array([999, 0, -1, -1, -1], np.float32).view(np.uint32)
    n = 0
    for i, k in enumerate(ka):
        j = row.get(tuple(k))
        n += int((xa[i] != (xb[j].view(np.uint32) if j is not None else default)).any(axis=-1).sum())
    return n


def _handler(shape, trunc):
    cam = CAMS[shape]
    hcam = I.PinholeCamera()
    hcam.fx, hcam.fy, hcam.cx, hcam.cy, hcam.width, hcam.height, hcam.depth_scale = cam
    hv = I.CubeHandler(hcam, device=0, max_blocks=1 << 14)
    hv.SetVoxelResolution(RES)
    hv.SetTruncation(trunc)
    return hv


def _equal(hv, ok, ox):
    hk, hx = hv.GetCubeMap()
    assert hk.shape == ok.shape and np.array_equal(hk, ok), "block keys differ"
    assert np.array_equal(hx.view(np.uint32), ox.view(np.uint32)), "voxels differ"


@pytest.mark.parametrize("trunc", [0.1, 1.5])
@pytest.mark.parametrize("shape", list(CAMS))
def test_sequence_and_both_counters_equal_the_oracle(oracle, shape, trunc):
    ok, ox, sel, upd, snaps = _oracle_run(oracle, shape, trunc)
    assert 100 < len(ok) < 4000 and sum(upd) > 100000
    if trunc >= 1:
        assert (ox[..., 0][ox[..., 1] > 0] >= 1).any()     # stored observations that IsValid rejects exist: the select is live here
    written = _written(None, snaps[32]) + upd[32]           # the 32-frame launch stores every voxel it changed once; the 1-frame launch its updates
    depth, rgb = _device(shape)
    hv = _handler(shape, trunc)
    hv.IntegrateSequence(depth, rgb, _frames(shape)[2])
    st = hv.Stats()                                         # (flushes the 33rd frame)
    print("%s trunc %.9g: %d blocks, updated %d (oracle %d), written %d (oracle %d), launches %d" % (shape, trunc, len(ok), st["voxels_updated"], sum(upd), st["voxels_written"], written, st["launches"]))
    assert st["frames"] == N and st["launches"] == 2
    assert st["blocks_selected"] == sum(sel)
    assert st["voxels_updated"] == sum(upd)
    assert st["voxels_written"] == written
    _equal(hv, ok, ox)


def test_a_volume_that_is_not_plain(oracle):
    """Download, upload (the volume is no longer the kernel's own: its blocks take the general update, blocks allocated later the one with the
    select), fuse the rest in one 23-frame launch."""
    shape, trunc = "160x120", 0.1
    ok, ox, _sel, upd, snaps = _oracle_run(oracle, shape, trunc)
    depth, rgb = _device(shape)
    poses = _frames(shape)[2]
    hv = _handler(shape, trunc)
    hv.IntegrateSequence(depth[:10], rgb[:10], poses[:10])
    k, v = hv.GetCubeMap()
    assert np.array_equal(k, snaps[10][0]) and np.array_equal(v.view(np.uint32), snaps[10][1].view(np.uint32))
    hv.SetCubeMap(k, v)
    n_before = hv.BlockCount()
    hv.IntegrateSequence(depth[10:], rgb[10:], poses[10:])
    assert hv.BlockCount() > n_before                      # both kinds of block in the second part
    _equal(hv, ok, ox)
    st = hv.Stats()                                        # (SetCubeMap replaces the map and starts the statistics again)
    assert st["frames"] == N - 10 and st["launches"] == 1
    assert st["voxels_updated"] == sum(upd[10:])
    assert st["voxels_written"] == _written(snaps[10], (ok, ox))


def test_with_the_raycasters_summaries_present(oracle):
    """One view before fusing: k_integrate then restates the summaries of the blocks it changes from the voxels it holds."""
    shape, trunc = "160x120", 0.1
    ok, ox, _sel, upd, snaps = _oracle_run(oracle, shape, trunc)
    depth, rgb = _device(shape)
    poses = _frames(shape)[2]
    view = S.room_pose(330)
    hv = _handler(shape, trunc)
    hv.IntegrateSequence(depth[:1], rgb[:1], poses[:1])
    hv.Raycast(view)
    hv.IntegrateSequence(depth[1:], rgb[1:], poses[1:])    # 32 frames: one full launch
    _equal(hv, ok, ox)
    st = hv.Stats()
    assert st["launches"] == 2 and st["voxels_updated"] == sum(upd)
    assert st["voxels_written"] == upd[0] + _written(snaps[1], (ok, ox))
    with_sum = hv.Raycast(view)
    hv.SetRaycastPrune(False)
    without = hv.Raycast(view)
    assert with_sum[0].any() and with_sum[0].tobytes() == without[0].tobytes()
    ov = oracle.Volume(oracle.make_camera(*CAMS[shape]), voxel_res=RES, trunc=trunc)
    ov.load(ok, ox)
    assert np.array_equal(with_sum[0].view(np.uint32), ov.raycast(view)[0].view(np.uint32))

