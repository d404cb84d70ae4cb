"""op_volume_sample on the device (csrc/volume_sample.hip) against the numpy restatement of its definition (tests/volume_sample_common.py, which
tests/test_volume_sample_cpu.py pins to the oracle) over volumes that come from the oracle or from hand-made blocks -- never from the code under
test: every voxel, gradient and status bit, the counts and the maximum of the statistics exactly, its two sums to the rounding of their additions.

Shapes: the room at 37 x 29 into 4 cm voxels (6 frames) and at 64 x 48 into 2 cm voxels (8 frames); batches of 4097 queries (17 workgroups, the
last one a single lane) and of 1, 63, 64 and 65 (around one wave); 70 hand-made blocks of 1/32 m voxels, where voxel centres and block faces are
exact in float32."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import deintegrate_common as D
import volume_sample_common as S
from onepiece_amd import _lib as L
from onepiece_amd import integration as I

pytestmark = pytest.mark.gpu

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOLUMES = {"cam37": (D.CAM_37, 6, 0.04), "cam64": (D.CAM_64, 8, 0.02)}
TRUNC = 0.1
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _handler(camt, res, trunc=TRUNC, max_blocks=1 << 13):
    hcam = I.PinholeCamera()
    hcam.fx, hcam.fy, hcam.cx, hcam.cy, hcam.width, hcam.height, hcam.depth_scale = camt
    hv = I.CubeHandler(hcam, device=0, max_blocks=max_blocks)
    hv.SetVoxelResolution(res)
    hv.SetTruncation(trunc)
    return hv


def _scene(oracle, name):
    """the oracle's volume of `name`, its frames, its export, the restatement's grid over it and the 4097 queries"""
    if name not in _cache:
        camt, n, res = VOLUMES[name]
        fr = D.frames(camt, n)
        vol = oracle.Volume(oracle.make_camera(*camt), voxel_res=res, trunc=TRUNC)
        for f in fr:
            vol.integrate(*f)
        keys, vox = vol.export()
        _cache[name] = {"vol": vol, "frames": fr, "keys": keys, "vox": vox, "grid": S.Grid(keys, vox, res), "q": S.query_mix(keys, res), "want": {}}
    return _cache[name]


def _want(sc, res, mode, gradients):
    key = (mode, gradients)
    if key not in sc["want"]:
        sc["want"][key] = S.sample(sc["keys"], sc["vox"], res, sc["q"], mode=mode, gradients=gradients, grid=sc["grid"])
    return sc["want"][key]


def _fused(sc, camt, res, **kw):
    hv = _handler(camt, res, **kw)
    for f in sc["frames"]:
        hv.IntegrateImage(*f)
    return hv                                                         # (no accessor called: the last frames are still queued)


def _check_stats(got, want, what):
    print("%s: device %s, restatement %s" % (what, got, want))
    for k in ("queries", "valid", "gradients", "out_of_range"):
        assert got[k] == want[k], (what, k)
    assert F32(got["max_abs_sdf"]) == F32(want["max_abs_sdf"]), what
    n = max(want["valid"], 2)
    for k in ("sum_abs_sdf", "sum_sq_sdf"):                           # every term is exact in double: only the order of the additions differs
        assert abs(got[k] - want[k]) <= (n - 1) * 2.0 ** -53 * abs(want[k]), (what, k, got[k], want[k])


def _check(got, want, what, nan_ok=False):
    """got: Sample's tuple (voxels, status[, gradients][, stats]); want: the restatement's dict"""
    vox, status = got[0], got[1]
    assert np.array_equal(status, want["status"]), "%s: %d status bytes differ" % (what, int((status != want["status"]).sum()))
    bad = _bits(vox) != _bits(want["voxels"])
    if nan_ok:                                                        # the payload of a NaN is not part of the definition
        bad &= ~(np.isnan(vox) & np.isnan(want["voxels"]))
    assert not bad.any(), "%s: %d voxels differ" % (what, int(bad.any(axis=1).sum()))
    k = 2
    if want["gradients"] is not None:
        badg = (_bits(got[k]) != _bits(want["gradients"])).any(axis=1)
        assert not badg.any(), "%s: %d gradients differ" % (what, int(badg.sum()))
        k += 1
    if len(got) > k:
        _check_stats(got[k], want["stats"], what)


MODES = [("trilinear", S.TRILINEAR, False), ("trilinear", S.TRILINEAR, True), ("reference", S.REFERENCE, False)]


@pytest.mark.parametrize("source", ["fused", "uploaded"])
@pytest.mark.parametrize("name", list(VOLUMES))
def test_01_batch_against_the_restatement(oracle, name, source):
    camt, _n, res = VOLUMES[name]
    sc = _scene(oracle, name)
    if source == "fused":
        hv = _fused(sc, camt, res)
    else:
        hv = _handler(camt, res)
        hv.SetCubeMap(sc["keys"], sc["vox"])
    for mode, m, grads in MODES:
        got = hv.Sample(sc["q"], mode=mode, gradients=grads, stats=True)
        _check(got, _want(sc, res, m, grads), "%s %s %s gradients=%s" % (name, source, mode, grads))
    k, v = hv.GetCubeMap()
    assert np.array_equal(k, sc["keys"]) and np.array_equal(_bits(v), _bits(sc["vox"]))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_02_device_buffers_and_small_batches(oracle, n):
    """host and device buffers; the device buffers start 4 bytes (the status bytes 1 byte) into their allocation and are fenced by sentinels"""
    import torch
    name = "cam37"
    camt, _n, res = VOLUMES[name]
    sc = _scene(oracle, name)
    hv = _cache.get("hv37")
    if hv is None:
        hv = _cache["hv37"] = _fused(sc, camt, res)
    q = sc["q"][-n:]                                                  # (the tail of the batch: other queries than test_01's first lanes)
    dev = torch.device("cuda:0")
    for mode, m, grads in MODES:
        want = S.sample(sc["keys"], sc["vox"], res, q, mode=m, gradients=grads, grid=sc["grid"])
        _check(hv.Sample(q, mode=mode, gradients=grads, stats=True), want, "host n=%d %s" % (n, mode))
        pts = torch.full((3 * n + 2,), 7.0, dtype=torch.float32, device=dev)
        pts[1:1 + 3 * n] = torch.from_numpy(q.reshape(-1)).to(dev)
        vox = torch.full((5 * n + 2,), 12345.0, dtype=torch.float32, device=dev)
        grad = torch.full((3 * n + 2,), 12345.0, dtype=torch.float32, device=dev)
        stat = torch.full((n + 2,), 99, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        st = hv.SampleDevice(pts[1:].data_ptr(), n, vox[1:].data_ptr(), stat[1:].data_ptr(), grad[1:].data_ptr() if grads else 0, mode=mode, stats=True)
        assert pts[1:].data_ptr() % 16 == 4 and stat[1:].data_ptr() % 16 == 1
        hvox, hgrad, hstat = vox.cpu().numpy(), grad.cpu().numpy(), stat.cpu().numpy()
        for a, fence in ((hvox, 12345.0), (hgrad, 12345.0), (hstat, 99)):
            assert a[0] == fence and a[-1] == fence, "a write outside the n entries"
        got = (hvox[1:-1].reshape(n, 5), hstat[1:-1]) + ((hgrad[1:-1].reshape(n, 3),) if grads else ()) + (st,)
        if not grads:
            assert (hgrad == 12345.0).all()
        _check(got, want, "device n=%d %s" % (n, mode))
    # outputs one at a time (the other pointers NULL)
    want = S.sample(sc["keys"], sc["vox"], res, q, gradients=True, grid=sc["grid"])
    lib = L.load()
    stat_only, grad_only = np.full(n, 99, np.uint8), np.zeros((n, 3), F32)
    st = L.SampleStats()
    qq = np.ascontiguousarray(q)
    L.check(lib.op_volume_sample(hv._h, C.c_void_p(qq.ctypes.data), n, L.OP_MEM_HOST, None, L.OP_SAMPLE_TRILINEAR, None, None, C.c_void_p(stat_only.ctypes.data), None))
    assert np.array_equal(stat_only, want["status"] & ~np.uint8(S.NO_GRADIENT))   # no gradient asked for: the bit is never set
    L.check(lib.op_volume_sample(hv._h, C.c_void_p(qq.ctypes.data), n, L.OP_MEM_HOST, None, L.OP_SAMPLE_TRILINEAR, None, C.c_void_p(grad_only.ctypes.data), None, None))
    assert np.array_equal(_bits(grad_only), _bits(want["gradients"]))
    L.check(lib.op_volume_sample(hv._h, C.c_void_p(qq.ctypes.data), n, L.OP_MEM_HOST, None, L.OP_SAMPLE_TRILINEAR, None, None, None, C.byref(st)))
    _check_stats(I.CubeHandler._sample_stats(st), dict(want["stats"], gradients=0), "stats only, n=%d" % n)


@pytest.mark.parametrize("name", list(VOLUMES))
def test_03_raycast_tie(oracle, name):
    """at the hit points of the device's own Raycast views the sampled colours are its colours and the normalised gradients its normals"""
    camt, n, res = VOLUMES[name]
    sc = _scene(oracle, name)
    hv = _fused(sc, camt, res)
    for which in (0, n // 2):
        pose = sc["frames"][which][2]
        depth, normals, colors = hv.Raycast(pose)
        hit, pts = S.hit_points(pose, camt, depth)
        vox, status, grad = hv.Sample(pts, gradients=True)
        valid, has_grad = (status & S.INVALID) == 0, (status & S.NO_GRADIENT) == 0
        col = np.where(valid[:, None], vox[:, 2:], F32(0.0))
        nrm = S.normalised(grad, has_grad)
        print("%s pose %d: %d hit pixels, %d valid samples, %d gradients" % (name, which, int(hit.sum()), int(valid.sum()), int(has_grad.sum())))
        assert hit.sum() > 1000 and has_grad.sum() > 0.9 * hit.sum()
        assert np.array_equal(_bits(col), _bits(colors[hit])) and np.array_equal(_bits(nrm), _bits(normals[hit]))


def test_04_transform_tie(oracle):
    """the REFERENCE sample at the mapped-back centres of op_volume_transform's result is that result, voxel for voxel (the 4 cm volume)"""
    camt, _n, res = VOLUMES["cam37"]
    sc = _scene(oracle, "cam37")
    hv = _fused(sc, camt, res)
    a = 0.3
    T = np.eye(4, dtype=F32)
    T[:3, :3] = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]).astype(F32)
    T[:3, 3] = [0.013, -0.027, 0.031]
    tk, tv = hv.Transform(T).GetCubeMap(sort=False)
    centres = S.block_voxel_centres(tk, res).reshape(-1, 3)
    vox, status = hv.Sample(centres, T=I.mat4_inverse(T), mode="reference")
    assert len(centres) > 100000 and (tv[..., 1] != 0).sum() > 1000
    bad = (_bits(vox) != _bits(tv.reshape(-1, 5))).any(axis=1)
    assert not bad.any(), "%d of %d voxels differ from the transformed volume" % (int(bad.sum()), len(bad))
    assert np.array_equal((status & S.INVALID) != 0, tv.reshape(-1, 5)[:, 1] == 0)


# ---- hand-made blocks ----------------------------------------------------------------------------------------------------------------
EDGE_RES = 0.03125                                                    # 1/32: voxel centres, faces and the range bound are exact in float32
HOLES = {(-2, -1, -2), (0, 1, 1), (2, 2, 1), (2, 2, -2), (-2, 2, 1), (2, -1, 1), (1, 2, -1), (-2, 2, -1), (2, 0, -2), (-1, 2, 0)}
EDGE_KEYS = np.array([k for k in ((x, y, z) for z in range(-2, 2) for y in range(-1, 3) for x in range(-2, 3)) if k not in HOLES], np.int32)


def _edge_blocks():
    """70 blocks of a 5 x 4 x 4 arrangement with 10 holes; every voxel observed (integer weights 1..5) except the few planted below"""
    assert len(EDGE_KEYS) == 70
    rng = np.random.default_rng(11)
    vox = np.empty((70, 512, 5), F32)
    vox[..., 0] = rng.uniform(-0.1, 0.1, (70, 512)).astype(F32)
    vox[..., 1] = rng.integers(1, 6, (70, 512)).astype(F32)
    vox[..., 2:] = rng.random((70, 512, 3)).astype(F32)
    row = {tuple(k): i for i, k in enumerate(EDGE_KEYS.tolist())}

    def plant(voxel, weight):
        b = tuple(np.asarray(voxel) >> 3)
        l = np.asarray(voxel) & 7
        vox[row[b], l[0] + 8 * l[1] + 64 * l[2], 1] = weight
    plant((2, 2, 2), 0.0)
    plant((4, 4, 4), np.nan)
    plant((6, 2, 2), -2.0)
    plant((2, 2, 11), 0.0)                                            # the +h sample on z of the gradient query below, and of nothing else of it
    return vox


def _p(g):
    """the point whose g = p * 32 - 0.5 is exactly `g` (dyadic g of few bits)"""
    return ((np.asarray(g, np.float64) + 0.5) / 32.0).astype(F32)


EDGE_QUERIES = [
    # (what, g, expected TRILINEAR status with gradients asked for; None = whatever the restatement says)
    ("a voxel centre", (1, 5, 3), None), ("the first voxel of a block", (0, 0, 0), None), ("the last voxel of a block", (7, 7, -1), None),
    ("a centre at negative coordinates", (-1, -8, -9), None), ("a block face", (7.5, 3.25, 2.5), 0), ("a block edge", (7.5, 7.5, 3.5), 0),
    ("a block corner", (7.5, 7.5, -0.5), 0), ("negative, floor not truncation", (-0.5, -2.25, -10.75), 0), ("negative fractions", (-3.75, -0.25, -14.875), 0),
    ("2 blocks, one absent", (3.5, 7.5, 10.5), S.INVALID | S.NO_GRADIENT), ("4 blocks, one absent", (3.5, 7.5, 7.5), S.INVALID | S.NO_GRADIENT),
    ("8 blocks, one absent", (-8.5, -0.5, -8.5), S.INVALID | S.NO_GRADIENT),
    ("a tap of weight 0", (1.5, 1.5, 1.5), S.INVALID | S.NO_GRADIENT), ("a tap of weight NaN", (3.25, 3.5, 3.75), S.INVALID | S.NO_GRADIENT),
    ("a tap of weight -2", (5.5, 1.5, 1.5), S.INVALID | S.NO_GRADIENT),
    ("only the +h sample on z is bad", (2.25, 2.25, 9.75), S.NO_GRADIENT),
    ("just inside the bound", (8388599.5, 0, 0), S.INVALID | S.NO_GRADIENT), ("just inside the bound, negative", (0, -8388599.5, 0), S.INVALID | S.NO_GRADIENT),
    ("on the bound", (8388600.0, 0, 0), S.INVALID | S.NO_GRADIENT | S.OUT_OF_RANGE), ("on the bound, negative", (0, 0, -8388600.0), S.INVALID | S.NO_GRADIENT | S.OUT_OF_RANGE),
]
EDGE_RAW = [("NaN", (np.nan, 0.1, 0.1)), ("+Inf", (0.1, np.inf, 0.1)), ("-Inf", (0.1, 0.1, -np.inf)), ("1e30", (1e30, 0.1, 0.1)), ("-1e30", (0.1, -1e30, 0.1))]


def test_05_edges():
    vox = _edge_blocks()
    hv = _handler(D.CAM_37, EDGE_RES)
    hv.AddCubes(EDGE_KEYS, vox)
    pts = np.concatenate([np.stack([_p(g) for _w, g, _s in EDGE_QUERIES]), np.array([p for _w, p in EDGE_RAW], F32)])
    grid = S.Grid(EDGE_KEYS, vox, EDGE_RES)
    g = pts[:len(EDGE_QUERIES)] * F32(32.0) - F32(0.5)
    assert np.array_equal(g, np.array([q[1] for q in EDGE_QUERIES], F32))          # the queries are where they are meant to be
    want = S.sample(EDGE_KEYS, vox, EDGE_RES, pts, gradients=True, grid=grid)
    for i, (what, gq, status) in enumerate(EDGE_QUERIES):
        if status is not None:
            assert want["status"][i] == status, (what, want["status"][i])
    for i, (what, gq, _s) in enumerate(EDGE_QUERIES[:4]):                           # f = 0: the stored voxel itself
        held, t = grid.fetch(np.array([gq], np.int64))
        assert held[0] and np.array_equal(_bits(want["voxels"][i]), _bits(t[0])), what
    assert (want["status"][len(EDGE_QUERIES):] == (S.INVALID | S.NO_GRADIENT | S.OUT_OF_RANGE)).all()
    i = [q[0] for q in EDGE_QUERIES].index("only the +h sample on z is bad")
    h = F32(0.5) * F32(EDGE_RES)
    six = [S.trilinear(grid, pts[i:i + 1] + np.array(e, F32) * h)[0][0] for e in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    assert six == [True, True, True, True, False, True]
    _check(hv.Sample(pts, gradients=True, stats=True), want, "edges, trilinear with gradients")
    _check(hv.Sample(pts, stats=True), S.sample(EDGE_KEYS, vox, EDGE_RES, pts, grid=grid), "edges, trilinear")
    wref = S.sample(EDGE_KEYS, vox, EDGE_RES, pts, mode=S.REFERENCE, grid=grid)
    assert (wref["status"][len(EDGE_QUERIES):] == (S.INVALID | S.OUT_OF_RANGE)).all() and (wref["status"][-len(EDGE_RAW) - 2:-len(EDGE_RAW)] & S.OUT_OF_RANGE).all()
    got = hv.Sample(pts, mode="reference")
    _check(got, wref, "edges, reference", nan_ok=True)
    k, v = hv.GetCubeMap()
    order = np.lexsort((EDGE_KEYS[:, 2], EDGE_KEYS[:, 1], EDGE_KEYS[:, 0]))
    assert np.array_equal(k, EDGE_KEYS[order]) and np.array_equal(_bits(v), _bits(vox[order]))


def test_06_transform_argument(oracle):
    """T given = the points transformed in numpy in the stated order, sampled without T; also a projective T (w != 1) and one that sends points to infinity"""
    camt, n, res = VOLUMES["cam37"]
    sc = _scene(oracle, "cam37")
    hv = _fused(sc, camt, res)
    pose = sc["frames"][2][2]
    depth = sc["frames"][2][0]
    z = depth.reshape(-1)
    u, v = np.meshgrid(np.arange(camt[4], dtype=F32), np.arange(camt[5], dtype=F32))
    cam_pts = np.stack([(u.reshape(-1) - F32(camt[2])) * z / F32(camt[0]), (v.reshape(-1) - F32(camt[3])) * z / F32(camt[1]), z], axis=1).astype(F32)[z > 0]
    proj = (pose * F32(1.3)).astype(F32)                              # the same map with q.w = 1.3: the division is not a no-op
    proj[3, :3] = [1e-4, -2e-4, 5e-5]
    degenerate = pose.copy()
    degenerate[3] = [0, 0, 0, 0]                                      # q.w = 0: every point goes to +-Inf or NaN
    for what, T in (("a pose", pose), ("a projective matrix", proj), ("w = 0", degenerate)):
        pre = S.transform_points(T, cam_pts)
        for mode, m, grads in MODES:
            got = hv.Sample(cam_pts, T=T, mode=mode, gradients=grads, stats=True)
            same = hv.Sample(pre, mode=mode, gradients=grads, stats=True)
            want = S.sample(sc["keys"], sc["vox"], res, cam_pts, T=T, mode=m, gradients=grads, grid=sc["grid"])
            _check(got, want, "%s, %s" % (what, mode))
            _check(same, want, "%s pre-transformed, %s" % (what, mode))
        if what != "w = 0":
            assert want["stats"]["valid"] > 0.5 * len(cam_pts)        # the frame's own points lie on the model's surface
        if what == "w = 0":
            assert want["stats"]["out_of_range"] == len(cam_pts)


def test_07_no_explicit_sync_growth_and_collection(oracle):
    camt, n, res = VOLUMES["cam37"]
    sc = _scene(oracle, "cam37")
    want = [_want(sc, res, m, g) for _mode, m, g in MODES]
    # a frame integrated just before the query is part of the answer (the queue is flushed first)
    hv = _handler(camt, res)
    for f in sc["frames"][:-1]:
        hv.IntegrateImage(*f)
    before = hv.Sample(sc["q"])
    hv.IntegrateImage(*sc["frames"][-1])
    for (mode, m, grads), w in zip(MODES, want):
        _check(hv.Sample(sc["q"], mode=mode, gradients=grads, stats=True), w, "right after IntegrateImage, %s" % mode)
    assert not np.array_equal(_bits(before[0]), _bits(want[0]["voxels"]))           # (the last frame matters)
    # after the pool has grown
    small = _fused(sc, camt, res, max_blocks=64)
    for (mode, m, grads), w in zip(MODES, want):
        _check(small.Sample(sc["q"], mode=mode, gradients=grads, stats=True), w, "after a pool growth, %s" % mode)
    assert small.GrowthStats()["grows"] > 0
    # after CollectGarbage has moved blocks: nine empty blocks far away take the first pool slots, the room is fused behind them, the collection
    # drops the nine and moves nine blocks of the room into their slots (a block without an observed voxel and an absent one sample alike)
    moved = _handler(camt, res)
    for i in range(9):
        moved.AddCube((100 + i, 100, 100))
    for f in sc["frames"]:
        moved.IntegrateImage(*f)
    for (mode, m, grads), w in zip(MODES, want):
        _check(moved.Sample(sc["q"], mode=mode, gradients=grads, stats=True), w, "with empty blocks in the pool, %s" % mode)
    st = moved.CollectGarbage()
    print(st)
    assert st["blocks_moved"] >= 9 and st["removed_unobserved"] >= 9
    for (mode, m, grads), w in zip(MODES, want):
        _check(moved.Sample(sc["q"], mode=mode, gradients=grads, stats=True), w, "after CollectGarbage, %s" % mode)


@pytest.mark.parametrize("source", ["fused", "uploaded"])
def test_08_sampling_leaves_the_volume_alone(oracle, source):
    """GetCubeMap before and after is bit-equal, and fusing on afterwards gives the oracle's volume: on a volume that only fusion wrote (the
    plain, lean update) and on an uploaded one (the general update)"""
    camt, n, res = VOLUMES["cam37"]
    sc = _scene(oracle, "cam37")
    half = n // 2
    ov = oracle.Volume(oracle.make_camera(*camt), voxel_res=res, trunc=TRUNC)
    for f in sc["frames"][:half]:
        ov.integrate(*f)
    hk, hx = ov.export()
    hv = _handler(camt, res)
    if source == "fused":
        for f in sc["frames"][:half]:
            hv.IntegrateImage(*f)
    else:
        hv.SetCubeMap(hk, hx)
    k0, v0 = hv.GetCubeMap(sort=False)
    for mode, _m, grads in MODES:
        hv.Sample(sc["q"], mode=mode, gradients=grads, stats=True)
    hv.Sample(sc["q"], T=sc["frames"][0][2])
    k1, v1 = hv.GetCubeMap(sort=False)
    assert np.array_equal(k0, k1) and np.array_equal(_bits(v0), _bits(v1))
    for f in sc["frames"][half:]:
        hv.IntegrateImage(*f)
    hv.Sample(sc["q"][:100])
    k2, v2 = hv.GetCubeMap()
    assert np.array_equal(k2, sc["keys"]) and np.array_equal(_bits(v2), _bits(sc["vox"]))


def test_09_empty_volume_and_refusals(oracle):
    camt, _n, res = VOLUMES["cam37"]
    sc = _scene(oracle, "cam37")
    hv = _handler(camt, res)
    q = sc["q"][:300]
    vox, status, grad, st = hv.Sample(q, gradients=True, stats=True)
    assert (status == (S.INVALID | S.NO_GRADIENT)).all() and not grad.any() and np.array_equal(_bits(vox), _bits(np.broadcast_to(S.DEFAULT_VOXEL, (300, 5))))
    assert st == {"queries": 300, "valid": 0, "gradients": 0, "out_of_range": 0, "sum_abs_sdf": 0.0, "sum_sq_sdf": 0.0, "max_abs_sdf": 0.0}
    vox, status = hv.Sample(q, mode="reference")
    assert (status == S.INVALID).all() and np.array_equal(_bits(vox), _bits(np.broadcast_to(S.DEFAULT_VOXEL, (300, 5))))
    assert hv.BlockCount() == 0
    # n = 0: OP_OK and zero stats
    vox, status, st = hv.Sample(np.zeros((0, 3), F32), stats=True)
    assert len(vox) == 0 and len(status) == 0 and st["queries"] == 0 and st["valid"] == 0
    # refusals, with a live volume
    lib = L.load()
    p = lambda a: C.c_void_p(a.ctypes.data)
    pts, o5, o3, o1 = np.zeros((4, 3), F32), np.zeros((4, 5), F32), np.zeros((4, 3), F32), np.zeros(4, np.uint8)
    assert lib.op_volume_sample(hv._h, None, 4, L.OP_MEM_HOST, None, L.OP_SAMPLE_TRILINEAR, p(o5), None, None, None) == L.OP_ERR_INVALID
    assert lib.op_volume_sample(hv._h, p(pts), 4, L.OP_MEM_HOST, None, L.OP_SAMPLE_TRILINEAR, None, None, None, None) == L.OP_ERR_INVALID
    assert lib.op_volume_sample(hv._h, p(pts), 4, 7, None, L.OP_SAMPLE_TRILINEAR, p(o5), None, None, None) == L.OP_ERR_INVALID
    assert lib.op_volume_sample(hv._h, p(pts), 4, L.OP_MEM_HOST, None, -1, p(o5), None, None, None) == L.OP_ERR_INVALID
    assert lib.op_volume_sample(hv._h, p(pts), 4, L.OP_MEM_HOST, None, L.OP_SAMPLE_REFERENCE, p(o5), p(o3), p(o1), None) == L.OP_ERR_INVALID
    assert lib.op_volume_sample(None, p(pts), 4, L.OP_MEM_HOST, None, L.OP_SAMPLE_TRILINEAR, p(o5), None, None, None) == L.OP_ERR_INVALID
    assert not o5.any() and not o3.any() and not o1.any()
    assert lib.op_volume_sample(hv._h, None, 0, L.OP_MEM_HOST, None, L.OP_SAMPLE_TRILINEAR, p(o5), None, None, None) == L.OP_OK


def _run(cmd, timeout=120):
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    assert run.returncode == 0, "%s\n%s\n%s" % (" ".join(map(str, cmd)), run.stdout[-2000:], run.stderr[-2000:])
    return run.stdout


@pytest.mark.parametrize("mode", ["trilinear", "reference"])
def test_10_driver_paths_write_the_same_bytes(mode, tmp_path):
    """examples/cpp/ModelQuery: the device path and the path there was before (GetCubeMap + a host loop of the same definition) dump identical
    bytes, with gradients in the trilinear mode, for the model's own mesh vertices and for a frame's points with its pose as T"""
    import json
    exe = os.path.join(ROOT, "examples", "cpp", "ModelQuery.bin")
    assert os.path.exists(exe), "examples/cpp/ModelQuery.bin is not built (__graft_entry__.build())"
    for queries in ("mesh", "frame"):
        out = {}
        for path in ("host", "device"):
            d = tmp_path / ("%s_%s" % (queries, path))
            d.mkdir()
            cmd = [exe, "--synthetic", "6", "5", "1", "--res", "0.04", "--queries", queries, "--mode", mode, "--path", path, "--dump", str(d)]
            if mode == "trilinear":
                cmd.append("--gradients")
            res = json.loads(_run(cmd).strip().splitlines()[-1])
            files = ["voxels.bin", "status.bin"] + (["gradients.bin"] if mode == "trilinear" else [])
            out[path] = (res, {f: open(d / f, "rb").read() for f in files})
        (rh, fh), (rd, fd) = out["host"], out["device"]
        n = rh["n"]
        print(queries, mode, rd["stats"], rd["ms"])
        assert n == rd["n"] > 1000 and len(fh["voxels.bin"]) == 20 * n and len(fh["status.bin"]) == n
        for f in fh:
            assert fh[f] == fd[f], "%s differs between the host and the device path (%s, %s)" % (f, queries, mode)
        for k in ("queries", "valid", "gradients", "out_of_range"):
            assert rh["stats"][k] == rd["stats"][k]
        assert rd["stats"]["valid"] > 0.5 * n and (mode == "reference" or rd["stats"]["gradients"] > 0.5 * n)


def test_11_class_surface(oracle, tmp_path):
    """CubeHandler::SampleVoxels / SampleGradients / DistanceToModel (host/one_piece) return what the C-ABI returns for the same volume and points"""
    camt, _n, res = VOLUMES["cam37"]
    sc = _scene(oracle, "cam37")
    exe = tmp_path / "sample_surface_check"
    host, lib = os.path.join(ROOT, "host", "one_piece"), os.path.join(ROOT, "onepiece_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-I", host, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "sample_surface_check.cpp"),
                           "-L", host, "-lone_piece_hip_host", "-L", lib, "-lonepiece_hip", "-Wl,-rpath," + host, "-Wl,-rpath," + lib, "-o", str(exe)])
    hv = _handler(camt, res)
    hv.SetCubeMap(sc["keys"], sc["vox"])
    hv.WriteToFile(tmp_path / "room.map")
    back = _handler(camt, res)
    back.ReadFromFile(tmp_path / "room.map")
    q = sc["q"][:1500]
    q.tofile(tmp_path / "points.bin")
    text = _run([str(exe), str(tmp_path / "room.map"), repr(res), str(tmp_path / "points.bin"), str(tmp_path / "out")])
    T = np.eye(4, dtype=F32)
    T[:3, 3] = [0.01, -0.02, 0.005]
    rd = lambda name, dt, cols: np.fromfile(tmp_path / ("out" + name), dt).reshape((-1, cols) if cols else -1)
    for name, kw in (("_tri", {}), ("_ref", {"mode": "reference"}), ("_tri_T", {"T": T})):
        vox, status = back.Sample(q, **kw)
        assert np.array_equal(_bits(rd(name + "_voxels.bin", F32, 5)), _bits(vox)) and np.array_equal(rd(name + "_status.bin", np.uint8, 0), status), name
    vox, status, grad, st = back.Sample(q, gradients=True, stats=True)
    assert np.array_equal(_bits(rd("_gradients.bin", F32, 3)), _bits(grad)) and np.array_equal(rd("_gradient_status.bin", np.uint8, 0), status)
    _v, _s, st_T = back.Sample(q, T=T, stats=True)
    rows = [line.split() for line in text.strip().splitlines()[-2:]]
    for row, want in zip(rows, (st, st_T)):
        assert int(row[0]) == want["queries"] == 1500 and int(row[1]) == want["valid"] > 100
        assert float(row[2]) == want["sum_abs_sdf"] and float(row[3]) == want["sum_sq_sdf"] and F32(row[4]) == F32(want["max_abs_sdf"])
