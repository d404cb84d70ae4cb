"""k_prepare_frames with per-frame in-frustum certificates (onepiece_amd/csrc/ka_cert.hpp, select.hip k_prepare_frames<true>) against the oracle, bit for bit.

Images of 37 x 29, 64 x 16, 68 x 17 (a width that is no multiple of 4: the narrow load path) and 2047 x 2 pixels; a centred principal point, one on
integers (column 0 and row 0 on the frustum's planes) and an off-centre one; a rigid pose, one with a projective bottom row (no certificate) and a
rigid one 100 m away.  The frames hold, spread over the image, depths at the near and far distances and one ulp either side, at the certificate's
z_lo and z_hi and their neighbours, 0, -1, NaN, +inf and 1e38; the 16-bit frames 0, 1 and 65535.  Per frame: ComputeBounding's box and inside
count, PrepareCubes' list (it reads the packed records through the tile ranges) and the fused volume equal the oracle's.  A 33-frame sequence
crosses a batch boundary and mixes certified and refused frames in one launch: keys, voxels and both counters equal the oracle's.  The
-DKA_TRACE build of the library (make -C onepiece_amd/csrc katrace: select.hip recompiled, never the library the package loads), loaded by a
fresh process of its own, counts the wave passes that hold an uncertified lane (they run the full sequence for those lanes): none for interior
pixels at mid-range depth, all for a refused pose, some for the integer principal point."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from onepiece_amd import _lib as L, integration as I, synthetic as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((37, 29), (64, 16), (68, 17), (2047, 2))
NEAR, FAR = 0.5, 5.0


def _cams(w, h):
    f = 0.8 * w
    return {"centred": (f, f, (w - 1) / 2.0, (h - 1) / 2.0, w, h, 1000.0), "integer": (f, f, float(w // 2), float(h // 2), w, h, 1000.0),
            "off_centre": (f, 0.9 * f, w / 4.0, (h - 1) / 2.0, w, h, 1000.0)}


def _poses():
    rigid = S.room_pose(12).astype(np.float32)
    proj = rigid.copy(); proj[3] = (1e-3, -2e-3, 5e-4, 1.0)
    far = rigid.copy(); far[:3, 3] += np.float32([100.0, -60.0, 80.0])
    return {"rigid": rigid, "projective": proj, "rigid_100m": far}


def _hcam(cam):
    c = I.PinholeCamera()
    c.fx, c.fy, c.cx, c.cy, c.width, c.height, c.depth_scale = cam
    return c


def _certificate(cam, pose, near=NEAR, far=FAR):
    rect, z, quot = np.zeros(4, np.int32), np.zeros(2, np.float32), np.zeros(3, np.int32)
    pose = np.ascontiguousarray(pose, np.float32).reshape(16)
    L.check(L.load().op_debug_ka_certificate(C.byref(_hcam(cam)), pose.ctypes.data_as(C.POINTER(C.c_float)), far, near, rect.ctypes.data, z.ctypes.data_as(C.POINTER(C.c_float)),
                                            quot.ctypes.data))
    return rect, z, quot


def _frame(w, h, z_lo, z_hi, seed):
    """A slanted surface at mid-range depth with the issue's special depths planted every 53rd pixel, each special at several columns and rows."""
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    d = (1.2 + 1.5 * u / w + 0.3 * v / h + rng.uniform(0, 0.01, (h, w))).astype(np.float32)
    up = lambda x: np.nextafter(np.float32(x), np.float32(np.inf))
    dn = lambda x: np.nextafter(np.float32(x), np.float32(0))
    special = [NEAR, up(NEAR), dn(NEAR), FAR, up(FAR), dn(FAR), 0.0, -1.0, np.nan, np.inf, 1e38]
    if z_lo <= z_hi:
        special += [z_lo, up(z_lo), dn(z_lo), z_hi, up(z_hi), dn(z_hi)]
    flat = d.reshape(-1)
    for k, s in enumerate(special):
        flat[3 * k + 1::53] = np.float32(s)
    c = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return d, c


def _volumes(oracle, cam, res=0.04):
    ov = oracle.Volume(oracle.make_camera(*cam), voxel_res=res)
    hv = I.CubeHandler(_hcam(cam))
    hv.SetVoxelResolution(res)
    return ov, hv


def _same_volume(ov, hv):
    ok, ovx = ov.export()
    hk, hvx = hv.GetCubeMap()
    assert hk.shape == ok.shape and np.array_equal(hk, ok), "block keys differ"
    assert np.array_equal(hvx.view(np.uint32), ovx.view(np.uint32)), "voxels differ"
    return len(ok)


def _check_frame(oracle, cam, d, c, pose, what):
    ov, hv = _volumes(oracle, cam)
    omx, omn, oin = oracle.compute_bounding(ov.cam, d, pose)
    hmx, hmn, hin = hv.ComputeBounding(d, pose)
    assert oin == hin, "%s: inside count %d, oracle %d" % (what, hin, oin)
    assert np.array_equal(omx.view(np.uint32), hmx.view(np.uint32)) and np.array_equal(omn.view(np.uint32), hmn.view(np.uint32)), what + ": bounding box"
    oids, ocand = ov.prepare_cubes(d, pose)
    hids, hcand = hv.PrepareCubes(d, pose, return_candidates=True)
    assert ocand == hcand and np.array_equal(oids, hids), what + ": cube list"
    n, _nvis, nupd = ov.integrate(d, c, pose)
    hv.IntegrateImage(d, c, pose)
    st = hv.Stats()
    assert st["blocks_selected"] == n and st["voxels_updated"] == nupd, what + ": counters"
    _same_volume(ov, hv)
    return oin


@pytest.mark.parametrize("w,h", SHAPES)
def test_frames_against_the_oracle(oracle, w, h):
    certified = inside = 0
    for cname, cam in _cams(w, h).items():
        for pname, pose in _poses().items():
            rect, z, quot = _certificate(cam, pose)
            assert quot[0] == 1 and quot[1] == 1, "the cameras of this test take the short quotients"
            has = rect[0] <= rect[1]
            assert has == (pname != "projective"), (cname, pname, rect, z)
            certified += int(has)
            d, c = _frame(w, h, z[0], z[1], seed=w + len(cname) + len(pname))
            inside += _check_frame(oracle, cam, d, c, pose, "%dx%d %s %s" % (w, h, cname, pname))
    assert certified == 6 and inside > 0


@pytest.mark.parametrize("w,h", SHAPES)
def test_16_bit_depth_against_the_oracle(oracle, w, h):
    cam = _cams(w, h)["centred"]
    for scale in (1000.0, 5000.0):
        cam = cam[:6] + (scale,)
        pose = _poses()["rigid"]
        assert _certificate(cam, pose)[2][2] == 1, "depth_scale %g takes the short quotient" % scale
        d, c = _frame(w, h, 1.0, 0.0, seed=h)
        d16 = np.round(np.nan_to_num(np.clip(d, 0, 60.0), nan=0.0, posinf=0.0) * scale).clip(0, 65535).astype(np.uint16)
        flat = d16.reshape(-1)
        flat[2::41] = 0; flat[5::41] = 1; flat[7::41] = 65535
        assert _check_frame(oracle, cam, d16, c, pose, "%dx%d uint16 / %g" % (w, h, scale)) > 0


def test_a_sequence_that_mixes_certified_and_refused_frames_in_one_batch(oracle):
    import torch
    dev = torch.device("cuda:0")
    s = 8
    cam = (S.FX / s, S.FY / s, S.CX / s, S.CY / s, S.W // s, S.H // s, 1000.0)
    n = 33
    ds, cs, poses, has = [], [], [], []
    for i in range(n):
        pose = S.room_pose(40 + 3 * i).astype(np.float32)
        if i % 5 == 2:
            pose[3] = (0.0, 0.0, 2e-3, 1.0)        # projective: no certificate, the whole frame takes the full sequence
        elif i % 7 == 3:
            pose[0, 0] += np.float32(1e-3)         # no rotation any more: refused as well
        rect, _z, _q = _certificate(cam, pose)
        has.append(bool(rect[0] <= rect[1]))
        d, c = S.room_render(S.room_pose(40 + 3 * i), width=cam[4], height=cam[5], fx=cam[0], fy=cam[1], cx=cam[2], cy=cam[3])
        ds.append(d); cs.append(c); poses.append(pose)
    assert 8 <= sum(has) < n and not all(has[:16]) and any(has[:16]) and not all(has[16:32]) and any(has[16:32])
    ov, hv = _volumes(oracle, cam, res=0.02)
    sel = upd = 0
    for d, c, p in zip(ds, cs, poses):
        k, _nvis, nupd = ov.integrate(d, c, p)
        sel += k; upd += nupd
    depth = torch.from_numpy(np.stack(ds)).to(dev)
    rgb = torch.from_numpy(np.stack(cs)).to(dev)
    torch.cuda.synchronize()
    hv.IntegrateSequence(depth, rgb, np.stack(poses))
    st = hv.Stats()
    assert st["frames"] == n and st["launches"] == 2, st
    assert st["blocks_selected"] == sel and st["voxels_updated"] == upd, (st, sel, upd)
    assert _same_volume(ov, hv) > 100


def test_fallback_wave_counter_of_the_trace_build():
    """A fresh process loads the trace build alone (tests/tools/ka_trace_check.py: plain ctypes, the C-ABI), as the 64-frame build is tested."""
    path = os.path.join(ROOT, "onepiece_amd", "libonepiece_hip_katrace.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "onepiece_amd", "csrc"), "katrace"])
    assert not hasattr(L.load(), "op_debug_ka_trace"), "the counter stays out of the default build"
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "ka_trace_check.py"), path], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    got = json.loads(run.stdout.strip().splitlines()[-1])
    w, h = 64, 16
    waves = (w // 64) * (h // 4) * 4                     # wave passes: 64 x 4 pixels per wave, four pixel slots per thread
    assert got["centred"] == [waves, 0, w * h]           # interior pixels at mid-range depth: no wave has an uncertified lane
    assert got["projective"][:2] == [waves, waves]       # a refused pose: every wave pass takes the full sequence
    total, fallback, inside = got["integer"]
    assert total == waves and 0 < fallback < waves and 0 < inside < w * h
