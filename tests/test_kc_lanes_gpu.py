"""k_integrate with the lane map of onepiece_amd/csrc/kc_lanes.hpp (the lanes of a wave cover a sub-box of the block, a thread's two voxels lie
one sub-box apart in z; tests/test_kc_lanes_cpu.py holds the map itself): every instantiation still fuses what the CPU oracle fuses.

A wrong map moves observations to other voxels of the same block, so the comparison is the whole volume: block keys, every voxel bit for bit,
voxels_updated and voxels_written equal to the oracle's counts.  Shapes: 33 frames (a full 32-frame launch + a 1-frame launch) and 70 frames
(32 + 32 + 6) of the room at 37 x 29 and 64 x 48 into 4 cm voxels, truncation 0.1 (the lean instantiation) and 0.6 (plain); a volume that is not
plain (general update, scratch-using instantiation); the sum form against the oracle by its own bar (same blocks, counts and integer weights,
sdf and colour within 1e-4); a signed launch (integrations and de-integrations in one batch) with its three outcome counters; a caller's cube
list with blocks no frame hits; and the raycaster's summaries restated by the kernel, against summaries rebuilt from scratch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import deintegrate_common as D
from onepiece_amd import integration as I, synthetic as S

RES = 0.04
N = 70
CAMS = {
    "37x29": (30.0, 30.0, 18.25, 14.25, 37, 29, 1000.0),
    "64x48": (52.0, 52.0, 31.75, 23.25, 64, 48, 1000.0),
}
CUTS = (1, 10, 32, 33, 42, 64, 65, 70)                  # every launch boundary the tests below use
DEFAULT = np.array([999, 0, -1, -1, -1], np.float32).view(np.uint32)
_cache = {}


def _frames(shape):
    """(depth [N,h,w], rgb [N,h,w,3], poses [N,4,4]) on the host, rendered once per shape; frames 3 apart so that the views overlap."""
    key = ("frames", shape)
    if key not in _cache:
        cam = CAMS[shape]
        poses = np.stack([S.room_pose(300 + 3 * k) for k in range(N)]).astype(np.float32)
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
    """The oracle's volume over the N frames, once per (shape, truncation), read-only: blocks selected and voxels updated per frame, and the
    exported state after each frame count of CUTS."""
    key = ("oracle", shape, trunc)
    if key not in _cache:
        d, c, poses = _frames(shape)
        ov = oracle.Volume(oracle.make_camera(*CAMS[shape]), voxel_res=RES, trunc=trunc)
        sel, upd, snaps = [], [], {}
        for k in range(N):
            n, _vis, nu = ov.integrate(d[k], c[k], poses[k])
            sel.append(n); upd.append(nu)
            if k + 1 in CUTS:
                snaps[k + 1] = ov.export()
        for s in snaps.values():
            s[1].setflags(write=False)
        _cache[key] = (sel, upd, snaps)
    return _cache[key]


def _changed(before, after):
    """Voxels whose bits differ between two states of the volume (None: the empty volume) = what a launch between them stores."""
    ka, xa = after
    xa = xa.view(np.uint32)
    row = {} if before is None else {tuple(k): i for i, k in enumerate(before[0])}
    n = 0
    for i, k in enumerate(ka):
        j = row.get(tuple(k))
        n += int((xa[i] != (before[1][j].view(np.uint32) if j is not None else DEFAULT)).any(axis=-1).sum())
    return n


def _written(snaps, cuts, start=None):
    total, prev = 0, start
    for n in cuts:
        total += _changed(prev, snaps[n])
        prev = snaps[n]
    return total


def _handler(shape, trunc, max_blocks=1 << 14):
    hcam = I.PinholeCamera()
    hcam.fx, hcam.fy, hcam.cx, hcam.cy, hcam.width, hcam.height, hcam.depth_scale = CAMS[shape]
    hv = I.CubeHandler(hcam, device=0, max_blocks=max_blocks)
    hv.SetVoxelResolution(RES)
    hv.SetTruncation(trunc)
    return hv


def _equal(hv, ok, ox):
    hk, hx = hv.GetCubeMap()
    assert hk.shape == ok.shape and np.array_equal(hk, ok), "block keys differ"
    diff = (hx.view(np.uint32) != ox.view(np.uint32)).any(axis=-1)
    assert not diff.any(), "%d voxels differ, the first at (block, in-plane index) %s" % (int(diff.sum()), np.argwhere(diff)[0])


@pytest.mark.parametrize("trunc", [0.1, 0.6])
@pytest.mark.parametrize("n", [33, 70])
@pytest.mark.parametrize("shape", list(CAMS))
def test_sequence_and_both_counters_equal_the_oracle(oracle, shape, n, trunc):
    cuts = tuple(range(32, n, 32)) + (n,)                   # 33: launches of 32 + 1 frames; 70: 32 + 32 + 6
    sel, upd, snaps = _oracle_run(oracle, shape, trunc)
    ok, ox = snaps[n]
    assert 100 < len(ok) < 4000 and sum(upd[:n]) > 50000
    depth, rgb = _device(shape)
    hv = _handler(shape, trunc)
    hv.IntegrateSequence(depth[:n], rgb[:n], _frames(shape)[2][:n])
    st = hv.Stats()
    written = _written(snaps, cuts)
    print("%s, %d frames, trunc %.9g: %d blocks, updated %d (oracle %d), written %d (oracle %d)"
          % (shape, n, trunc, len(ok), st["voxels_updated"], sum(upd[:n]), st["voxels_written"], written))
    assert st["frames"] == n and st["launches"] == len(cuts) and st["blocks_selected"] == sum(sel[:n])
    assert st["voxels_updated"] == sum(upd[:n])
    assert st["voxels_written"] == written
    _equal(hv, ok, ox)


def test_a_volume_that_is_not_plain(oracle):
    """Download and upload after 10 frames: the uploaded blocks take the general update (two branches, four divisions), blocks allocated later
    the plain one; the rest is fused in launches of 32 + 28 frames."""
    shape, trunc = "64x48", 0.1
    _sel, upd, snaps = _oracle_run(oracle, shape, trunc)
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
    _equal(hv, *snaps[70])
    st = hv.Stats()
    assert st["frames"] == N - 10 and st["launches"] == 2
    assert st["voxels_updated"] == sum(upd[10:])
    assert st["voxels_written"] == _written(snaps, (42, 70), start=snaps[10])


@pytest.mark.parametrize("shape", list(CAMS))
def test_sum_form_sees_the_same_observations(oracle, shape):
    """OP_VOLUME_UPDATE_SUM_FORM: the same blocks, the same count of observations and the same (integer) weights as the oracle, voxel by voxel;
    sdf within 1e-4 of the truncation and colour within 1e-4 of the running mean (the sum form's own bar, tests/test_integration_gpu.py:
    one rounding per batch instead of one per frame); unobserved voxels untouched."""
    trunc = 0.1
    sel, upd, snaps = _oracle_run(oracle, shape, trunc)
    ok, ox = snaps[70]
    depth, rgb = _device(shape)
    hv = _handler(shape, trunc)
    hv.SetUpdateMode("sum_form")
    hv.IntegrateSequence(depth, rgb, _frames(shape)[2])
    st = hv.Stats()
    assert st["frames"] == N and st["blocks_selected"] == sum(sel) and st["voxels_updated"] == sum(upd)
    hk, hx = hv.GetCubeMap()
    assert np.array_equal(hk, ok)
    assert np.array_equal(hx[..., 1], ox[..., 1])
    seen = ox[..., 1] > 0
    e_sdf = np.abs(hx[..., 0].astype(np.float64) - ox[..., 0])[seen].max() / trunc
    e_col = np.abs(hx[..., 2:].astype(np.float64) - ox[..., 2:])[seen].max()
    print("%s sum form: sdf off by %.3g of the truncation, colour by %.3g" % (shape, e_sdf, e_col))
    assert e_sdf <= 1e-4 and e_col <= 1e-4
    assert np.array_equal(hx[~seen].view(np.uint32), ox[~seen].view(np.uint32))


@pytest.mark.parametrize("trunc", [0.1, 0.6])
def test_a_signed_launch_and_its_three_outcome_counters(oracle, trunc):
    """33 frames fused, frames 10 .. 20 de-integrated: the 33rd frame and the eleven de-integrations share ONE signed launch.  Expected volume and
    counters: tests/deintegrate_common.py (the oracle for fused frames, the definition's four steps in numpy for de-integrated ones)."""
    shape = "37x29"
    d, c, poses = _frames(shape)
    fr = [(np.ascontiguousarray(d[k], np.float32), np.ascontiguousarray(c[k], np.uint8), poses[k]) for k in range(33)]
    m = D.Model(oracle, CAMS[shape], trunc, res=RES)
    for f in fr:
        m.integrate(f)
    for f in fr[10:21]:
        m.deintegrate(f)
    assert m.counts["reverted"] > 10000 and m.counts["reset"] > 100
    depth, rgb = _device(shape)
    hv = _handler(shape, trunc)
    hv.IntegrateSequence(depth[:33], rgb[:33], poses[:33])
    hv.DeintegrateSequence(depth[10:21], rgb[10:21], poses[10:21])
    _equal(hv, *m.export())
    got = hv.DeintegrateStats()
    print("trunc %g: de-integration counters %s (restatement %s)" % (trunc, got, m.counts))
    assert got == m.counts
    st = hv.Stats()
    assert st["launches"] == 2
    assert (st["frames"], st["blocks_selected"], st["voxels_updated"]) == (m.entries, m.selected, m.updated)


@pytest.mark.parametrize("shape", list(CAMS))
def test_a_callers_cube_list_with_blocks_no_frame_hits(oracle, shape):
    """op_volume_integrate_cubes: the frame's own selection between two listed blocks that nothing projects into.  Those are allocated, loaded by
    every lane of the map, find no observation, store nothing and count nothing."""
    _sel, upd, snaps = _oracle_run(oracle, shape, 0.1)
    d, c, poses = _frames(shape)
    hv = _handler(shape, 0.1)
    ids = hv.PrepareCubes(d[0], poses[0])                  # allocates the selection, fuses nothing
    far = np.array([[900, 900, 900], [-900, 5, 7]], np.int32)
    hv.IntegrateCubes(d[0], c[0], poses[0], np.concatenate([far[:1], ids, far[1:]]))
    st = hv.Stats()
    assert st["launches"] == 1 and st["voxels_updated"] == upd[0] and st["voxels_written"] == upd[0] == _changed(None, snaps[1])
    hk, hx = hv.GetCubeMap()
    mine = ~((hk[:, None, :] == far[None]).all(-1).any(1))
    assert (~mine).sum() == 2 and np.array_equal(hx[~mine].view(np.uint32), np.broadcast_to(DEFAULT, (2, 512, 5)))
    assert np.array_equal(hk[mine], snaps[1][0]) and np.array_equal(hx[mine].view(np.uint32), snaps[1][1].view(np.uint32))


def test_summaries_restated_by_the_kernel_equal_summaries_rebuilt_from_scratch(oracle):
    """One view before fusing, so that the summary array exists: every wave of k_integrate then states the signs of its own voxels and the workgroup
    restates the block's summary.  The raycast that uses them must equal, byte for byte, the raycast of a second volume that received the same
    voxels by upload and so builds its summaries from nothing -- and the oracle's raycast of these voxels."""
    shape, trunc = "64x48", 0.1
    _sel, upd, snaps = _oracle_run(oracle, shape, trunc)
    ok, ox = snaps[70]
    depth, rgb = _device(shape)
    poses = _frames(shape)[2]
    view = S.room_pose(400)
    hv = _handler(shape, trunc)
    hv.IntegrateSequence(depth[:1], rgb[:1], poses[:1])
    hv.Raycast(view)
    hv.IntegrateSequence(depth[1:], rgb[1:], poses[1:])    # 32 + 32 + 5 frames
    _equal(hv, ok, ox)
    st = hv.Stats()
    assert st["launches"] == 4 and st["voxels_updated"] == sum(upd)
    assert st["voxels_written"] == _written(snaps, (1, 33, 65, 70))
    kept = hv.Raycast(view)
    fresh = _handler(shape, trunc)
    fresh.SetCubeMap(ok, ox)
    rebuilt = fresh.Raycast(view)
    assert kept[0].any() and kept[0].tobytes() == rebuilt[0].tobytes()
    hv.SetRaycastPrune(False)
    assert kept[0].tobytes() == hv.Raycast(view)[0].tobytes()
    ov = oracle.Volume(oracle.make_camera(*CAMS[shape]), voxel_res=RES, trunc=trunc)
    ov.load(ok, ox)
    assert np.array_equal(kept[0].view(np.uint32), ov.raycast(view)[0].view(np.uint32))
