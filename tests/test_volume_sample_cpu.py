"""The numpy restatement of op_volume_sample (tests/volume_sample_common.py) pinned to the committed oracle, and what of the entry can be checked
without a device: the constants, the binding, the refusals.

The two definitions the entry exposes are restated by the oracle already: the raycaster's sample, normal and colour in orc_volume_raycast, and
ReadVoxelInterpolate in orc_volume_transform.  So the restatement's TRILINEAR mode must reproduce the oracle's colours and normals at the oracle's
own hit points, and its REFERENCE mode every voxel of the oracle's transformed volume, bit for bit.

Volumes: the room at 37 x 29 into 4 cm voxels (6 frames) and at 64 x 48 into 2 cm voxels (8 frames), truncation 0.1."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import deintegrate_common as D
import volume_sample_common as S

F32 = np.float32
VOLUMES = {"cam37": (D.CAM_37, 6, 0.04), "cam64": (D.CAM_64, 8, 0.02)}
TRUNC = 0.1
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _volume(oracle, name):
    if name not in _cache:
        camt, n, res = VOLUMES[name]
        fr = D.frames(camt, n)
        vol = oracle.Volume(oracle.make_camera(*camt), voxel_res=res, trunc=TRUNC)
        for f in fr:
            vol.integrate(*f)
        keys, vox = vol.export()
        _cache[name] = (vol, fr, keys, vox, S.Grid(keys, vox, res))
    return _cache[name]


@pytest.mark.parametrize("name", list(VOLUMES))
def test_trilinear_mode_is_the_oracles_raycast_sample(oracle, name):
    camt, n, res = VOLUMES[name]
    vol, fr, keys, vox, grid = _volume(oracle, name)
    for which in (0, n // 2):
        pose = fr[which][2]
        depth, normals, colors = vol.raycast(pose)
        hit, pts = S.hit_points(pose, camt, depth)
        got = S.sample(keys, vox, res, pts, mode=S.TRILINEAR, gradients=True, grid=grid)
        valid = (got["status"] & S.INVALID) == 0
        col = np.where(valid[:, None], got["voxels"][:, 2:], F32(0.0))
        has_grad = (got["status"] & S.NO_GRADIENT) == 0
        nrm = S.normalised(got["gradients"], has_grad)
        print("%s pose %d: %d hit pixels, %d valid samples, %d valid gradients" % (name, which, int(hit.sum()), int(valid.sum()), int(has_grad.sum())))
        assert hit.sum() > 1000
        bad_c = (_bits(col) != _bits(colors[hit])).any(axis=1)
        bad_n = (_bits(nrm) != _bits(normals[hit])).any(axis=1)
        assert not bad_c.any(), "%d colours differ from the oracle's" % int(bad_c.sum())
        assert not bad_n.any(), "%d normals differ from the oracle's" % int(bad_n.sum())
        assert has_grad.sum() > 0.9 * hit.sum() and (nrm[has_grad] != 0).any(axis=1).all()


@pytest.mark.parametrize("name", list(VOLUMES))
def test_reference_mode_is_the_oracles_transform(oracle, name):
    camt, n, res = VOLUMES[name]
    vol, fr, keys, vox, grid = _volume(oracle, name)
    a = 0.3
    T = np.eye(4, dtype=F32)
    T[:3, :3] = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]).astype(F32)
    T[:3, 3] = [0.013, -0.027, 0.031]
    tk, tv = vol.transform(T).export()
    centres = S.block_voxel_centres(tk, res).reshape(-1, 3)
    got = S.sample(keys, vox, res, centres, T=oracle.mat4_inverse(T), mode=S.REFERENCE, grid=grid)
    bad = (_bits(got["voxels"]) != _bits(tv.reshape(-1, 5))).any(axis=1)
    print("%s: %d voxels of the transformed volume, %d observed" % (name, len(centres), int((tv[..., 1] != 0).sum())))
    assert len(centres) > 100000 and (tv[..., 1] != 0).sum() > 1000
    assert not bad.any(), "%d voxels differ from the oracle's transform" % int(bad.sum())
    assert np.array_equal((got["status"] & S.INVALID) != 0, tv.reshape(-1, 5)[:, 1] == 0)


@pytest.mark.parametrize("name", list(VOLUMES))
def test_query_mix_holds_every_class(oracle, name):
    camt, n, res = VOLUMES[name]
    _vol, _fr, keys, vox, grid = _volume(oracle, name)
    q = S.query_mix(keys, res)
    got = S.sample(keys, vox, res, q, gradients=True, grid=grid)
    st = got["stats"]
    print("%s: %s" % (name, st))
    assert len(q) == 4097 and st["queries"] == 4097 and st["out_of_range"] == 0
    least = 0.05 * len(q)
    assert st["valid"] >= least and len(q) - st["valid"] >= least and st["gradients"] >= least
    ref = S.sample(keys, vox, res, q, mode=S.REFERENCE, grid=grid)["stats"]
    assert ref["valid"] >= least and len(q) - ref["valid"] >= least
    assert st["max_abs_sdf"] <= TRUNC * 1.0001 and st["sum_sq_sdf"] > 0


def test_constants_and_binding_match_the_header(hip):
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "onepiece_hip.h")).read()
    for name, want in (("OP_SAMPLE_TRILINEAR", S.TRILINEAR), ("OP_SAMPLE_REFERENCE", S.REFERENCE), ("OP_SAMPLE_INVALID", S.INVALID),
                       ("OP_SAMPLE_NO_GRADIENT", S.NO_GRADIENT), ("OP_SAMPLE_OUT_OF_RANGE", S.OUT_OF_RANGE)):
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, text)
        assert m and int(m.group(1)) == want == getattr(hip, name), name
    m = re.search(r"typedef struct \{([^}]*)\} op_volume_sample_stats;", text)
    fields = [f.strip() for part in m.group(1).split(";") if part.strip() for f in part.split(None, 1)[1].split(",")]
    assert fields == [k for k, _t in hip.SampleStats._fields_] == list(S.STAT_NAMES)
    assert C.sizeof(hip.SampleStats) == 56
    from onepiece_amd import integration as I
    assert callable(I.CubeHandler.Sample) and callable(I.CubeHandler.SampleDevice)


def test_refusals_need_no_device(hip):
    lib = hip.load()
    pts = np.zeros((4, 3), F32)
    vox, grad, status = np.zeros((4, 5), F32), np.zeros((4, 3), F32), np.zeros(4, np.uint8)
    st = hip.SampleStats()
    p = lambda a: C.c_void_p(a.ctypes.data)
    cases = {
        "null volume": (None, p(pts), 4, hip.OP_MEM_HOST, None, hip.OP_SAMPLE_TRILINEAR, p(vox), p(grad), p(status), C.byref(st)),
        "null xyz": (None, None, 4, hip.OP_MEM_HOST, None, hip.OP_SAMPLE_TRILINEAR, p(vox), None, p(status), None),
        "no output": (None, p(pts), 4, hip.OP_MEM_HOST, None, hip.OP_SAMPLE_TRILINEAR, None, None, None, None),
        "bad mem": (None, p(pts), 4, 2, None, hip.OP_SAMPLE_TRILINEAR, p(vox), None, None, None),
        "bad mode": (None, p(pts), 4, hip.OP_MEM_HOST, None, 2, p(vox), None, None, None),
        "gradients in the reference mode": (None, p(pts), 4, hip.OP_MEM_HOST, None, hip.OP_SAMPLE_REFERENCE, p(vox), p(grad), None, None),
    }
    for what, args in cases.items():
        assert lib.op_volume_sample(*args) == hip.OP_ERR_INVALID, what
        assert b"op_volume_sample" in lib.op_last_error() or what == "null volume", what
    assert not vox.any() and not grad.any() and not status.any()       # nothing was written
