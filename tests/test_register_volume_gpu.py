"""op_volume_band_voxels, op_volume_register_offset_* and op_volume_register_volume on the device (csrc/volume_band.hip, the OFFSET instantiations of
k_volume_register in csrc/volume_register.hip) against the numpy restatement of their definitions (tests/volume_register_volume_common.py) over
volumes that come from the oracle or from hand-made blocks through SetCubeMap / AddCubes -- never from the code under test: the list bit for bit
and in order; every row of sixteen bit for bit, the seven counts exactly, the 31 sums to the rounding of their additions; offset == NULL against
the robust entries bit for bit; the volume entry against the offset entry on the list, against the loop made by hand, and against the restated
loop of tests/test_register_volume_cpu.py's convergence case.

Volumes: hand-made sources of 1, 2 and 9 blocks whose weights select 0 .. 4097 voxels (the wave, workgroup and block edges), the scenes of
tests/test_volume_register_robust_gpu.py, the seven hand-made blocks of 1/32 m voxels, and the two overlapping submaps of the convergence case."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import deintegrate_common as D
import test_volume_register_robust_gpu as G
import volume_register_color_common as K
import volume_register_common as R
import volume_register_robust_common as B
import volume_register_volume_common as V
import volume_sample_common as S
from onepiece_amd import _lib as L
from onepiece_amd import integration as I

pytestmark = pytest.mark.gpu

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 63, 64, 65, 255, 256, 257, 4097)
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 4097)
_cache = {}
_bits, _same64, _handler = G._bits, G._same64, G._handler


# ---- the list ----------------------------------------------------------------------------------------------------------------------------------
def _counted_source(count, seed=0):
    """ceil(count / 512) blocks (one at least, two for 513, nine for 4097), every sdf inside the default band, colours random, weight 2 on the first
    `count` voxels in (block, voxel) order and 0 elsewhere"""
    m = max(1, -(-count // 512))
    rng = np.random.default_rng(seed + count)
    keys = np.array([(k - 3, 2 - k % 3, k // 2) for k in range(m)], np.int32)
    vox = np.empty((m, 512, 5), F32)
    vox[..., 0] = rng.uniform(-0.03, 0.03, (m, 512)).astype(F32)
    vox[..., 1] = 0.0
    vox[..., 2:] = rng.random((m, 512, 3), dtype=F32)
    vox.reshape(-1, 5)[:count, 1] = 2.0
    return keys, vox


def _band_on_device(hv, sel, cap, want_intensity=True):
    """op_volume_band_voxels with every buffer on the device, 4 bytes into its allocation and fenced by sentinels -> (rc, n, xyz, sdf, intensity)"""
    import torch
    dev = torch.device("cuda:0")
    bufs = [torch.full((k * cap + 2,), 12345.0, dtype=torch.float32, device=dev) for k in (3, 1, 1)]
    torch.cuda.synchronize()
    n = C.c_size_t(0)
    rc = L.load().op_volume_band_voxels(hv._h, C.byref(sel), C.c_void_p(bufs[0][1:].data_ptr()), C.c_void_p(bufs[1][1:].data_ptr()),
                                        C.c_void_p(bufs[2][1:].data_ptr()) if want_intensity else None, L.OP_MEM_DEVICE, cap, C.byref(n))
    host = [b.cpu().numpy() for b in bufs]
    for h in host:
        assert h[0] == 12345.0 and h[-1] == 12345.0, "a write outside the buffer"
    return rc, n.value, host[0][1:-1].reshape(cap, 3), host[1][1:-1], host[2][1:-1]


@pytest.mark.parametrize("count", COUNTS)
def test_01_band_voxels_against_the_restatement(count):
    res, trunc = 0.02, 0.1
    keys, vox = _counted_source(count)
    hv = _handler(D.CAM_37, res, trunc)
    hv.SetCubeMap(keys, vox)
    k, v = hv.GetCubeMap(sort=False)                                  # the pool order is the list's block order
    assert len(k) == len(keys) == {0: 1, 513: 2, 4097: 9}.get(count, 1)
    for stride in (1, 2, 8):
        xyz, sdf, y, index = V.select(k, v, res, trunc, min_weight=1.0, stride=stride)
        if stride == 1:
            assert len(xyz) == count
        got = hv.BandVoxels(voxel_stride=stride)
        tag = "count %d stride %d: %d selected" % (count, stride, len(xyz))
        assert len(got[0]) == len(xyz), tag
        assert np.array_equal(_bits(got[0]), _bits(xyz)) and np.array_equal(_bits(got[1]), _bits(sdf)) and np.array_equal(_bits(got[2]), _bits(y)), tag
        assert hv.BandVoxels(voxel_stride=stride, intensity=False)[2] is None
        sel = hv._band_params(None, None, stride)
        n = len(xyz)
        # device buffers, exactly as large as the list
        rc, got_n, dx, ds, dy = _band_on_device(hv, sel, max(n, 1))
        assert rc == L.OP_OK and got_n == n, tag
        assert np.array_equal(_bits(dx[:n]), _bits(xyz)) and np.array_equal(_bits(ds[:n]), _bits(sdf)) and np.array_equal(_bits(dy[:n]), _bits(y)), tag
        rc, got_n, dx, ds, dy = _band_on_device(hv, sel, max(n, 1), want_intensity=False)
        assert rc == L.OP_OK and np.array_equal(_bits(ds[:n]), _bits(sdf)) and (dy == 12345.0).all(), tag
        # the count query, and a capacity one short: the count comes back, nothing is written
        q = C.c_size_t(77)
        L.check(L.load().op_volume_band_voxels(hv._h, C.byref(sel), None, None, None, L.OP_MEM_HOST, 0, C.byref(q)))
        assert q.value == n, tag
        if n > 1:
            rc, got_n, dx, ds, dy = _band_on_device(hv, sel, n - 1)
            assert rc == L.OP_ERR_CAPACITY and got_n == n and (dx == 12345.0).all() and (ds == 12345.0).all() and (dy == 12345.0).all(), tag
    k2, v2 = hv.GetCubeMap(sort=False)
    assert np.array_equal(k, k2) and np.array_equal(_bits(v), _bits(v2))


def test_02_band_parameters(oracle):
    """the defaults, band <= 0 = the truncation, min_weight and the band on a fused volume; a volume of another resolution; the empty volume"""
    sm = V.submaps(oracle)
    hv = _handler(B.MODEL_CAM, B.MODEL_RES)
    hv.SetCubeMap(sm["B"]["keys"], sm["B"]["vox"])
    k, v = hv.GetCubeMap(sort=False)
    p = L.BandParams(7.0, 7.0, 7)
    L.check(L.load().op_volume_band_default_params(hv._h, C.byref(p)))
    assert (p.band, p.min_weight, p.voxel_stride) == (F32(2.0) * F32(B.MODEL_RES), 1.0, 1)
    for kw in (dict(), dict(band=0.0), dict(band=-1.0), dict(band=0.04, voxel_stride=2), dict(band=0.1, min_weight=3.0, voxel_stride=4), dict(band=0.02, min_weight=0.0)):
        xyz, sdf, y, _i = V.select(k, v, B.MODEL_RES, B.TRUNC, band=kw.get("band"), min_weight=kw.get("min_weight", 1.0), stride=kw.get("voxel_stride", 1))
        got = hv.BandVoxels(**kw)
        print(kw, len(xyz))
        assert len(xyz) > 1000 and len(got[0]) == len(xyz), kw
        assert np.array_equal(_bits(got[0]), _bits(xyz)) and np.array_equal(_bits(got[1]), _bits(sdf)) and np.array_equal(_bits(got[2]), _bits(y)), kw
    assert len(hv.BandVoxels(band=0.04, voxel_stride=2)[0]) == 14845
    keys, vox = _counted_source(513)
    wide = _handler(D.CAM_37, 0.04, 0.2)
    wide.SetCubeMap(keys, vox)
    k, v = wide.GetCubeMap(sort=False)
    xyz, sdf, y, _i = V.select(k, v, 0.04, 0.2)
    got = wide.BandVoxels()
    assert len(xyz) == 513 and np.array_equal(_bits(got[0]), _bits(xyz)) and np.array_equal(_bits(got[1]), _bits(sdf))
    empty = _handler(D.CAM_37, 0.04, 0.2)
    assert [len(a) for a in empty.BandVoxels()] == [0, 0, 0]


# ---- the offset system -------------------------------------------------------------------------------------------------------------------------
def _offsets(n):
    """target values: 0, dyadic values, NaN and both infinities"""
    idx = np.arange(n)
    o = ((idx % 7) - 3).astype(F32) / F32(256.0)
    o[idx % 8 == 0] = 0.0
    o[idx % 16 == 5] = np.nan
    o[idx % 32 == 9] = np.inf
    o[idx % 32 == 25] = -np.inf
    return o


def _device_offset_system(hv, q, o, y, T, tail, opt, rows):
    """op_volume_register_offset_system with every buffer on the device, 4 bytes into its allocation and fenced by sentinels"""
    import torch
    n = len(q)
    dev = torch.device("cuda:0")

    def fenced(a):
        t = torch.full((a.size + 2,), 7.0, dtype=torch.float32, device=dev)
        t[1:1 + a.size] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(dev)
        return t
    pts, oo, yy = fenced(q), fenced(o), fenced(y)
    out = torch.full((16 * n + 2,), 12345.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    sums, counts = np.zeros(31), np.zeros(7, np.uint64)
    Tm = np.ascontiguousarray(T, F32).reshape(16)
    ro = L.RegisterOptions(opt["linearization"], opt["huber"], opt["huber_color"])
    L.check(L.load().op_volume_register_offset_system(hv._h, C.c_void_p(pts[1:].data_ptr()), C.c_void_p(oo[1:].data_ptr()), C.c_void_p(yy[1:].data_ptr()), n, L.OP_MEM_DEVICE,
                                                      Tm.ctypes.data_as(L._fp), float(tail[0]), float(tail[1]), float(tail[2]), C.byref(ro),
                                                      sums.ctypes.data_as(C.POINTER(C.c_double)), counts.ctypes.data_as(L._u64p), C.c_void_p(out[1:].data_ptr()) if rows else None))
    host = out.cpu().numpy()
    assert host[0] == 12345.0 and host[-1] == 12345.0, "a write outside the n rows"
    if not rows:
        assert (host == 12345.0).all()
    return sums, dict(zip(B.COUNT_NAMES, (int(c) for c in counts))), host[1:-1].reshape(n, 16)


@pytest.mark.parametrize("mode", [B.NORMAL, B.GRADIENT, B.METRIC])
@pytest.mark.parametrize("name", ["slide", "hand"])
def test_03_offset_system_against_the_restatement(oracle, name, mode):
    sc = G._scene(oracle, name)
    hv = G._volume(sc, "uploaded")
    T = sc["T"]
    o = _offsets(len(sc["q"]))
    for cs, weights in G.CONFIGS:
        tail, opt = G._args(sc, mode, cs, weights)
        whole = V.rows_of(sc["grid"], sc["q"], o, sc["y"], T, *tail, mode=mode, huber=opt["huber"], huber_color=opt["huber_color"])
        plain = G._want(sc, mode, cs, weights)
        lost = (plain["reason"] == 0) & (whole["reason"] == 1)
        assert lost.sum() > 50 and (whole["reason"] == 0).sum() > 500      # used points that a non-finite target value makes invalid, and used ones
        moved = (whole["reason"] == 0) & (whole["rows"][:, 6] != plain["rows"][:, 6])
        assert moved.sum() > 300, "the target values change residuals"
        for n in SIZES:
            tag = "%s mode %d color_scale %g weights %d n=%d" % (name, mode, cs, weights, n)
            w = G._head(whole, n)
            q, y = sc["q"][:n], sc["y"][:n]
            sums, counts, got = hv.OffsetRegistrationSystem(q, o[:n], y, T, *tail, rows=True, **opt)
            bad = (_bits(got) != _bits(w["rows"])).any(axis=1)
            assert not bad.any(), "%s: %d rows differ, first %d" % (tag, int(bad.sum()), int(np.argmax(bad)))
            G._check_system(sums, counts, w, tag)
            again, c2 = hv.OffsetRegistrationSystem(q, o[:n], y, T, *tail, **opt)                # rows = NULL, a second call: the same bits
            assert _same64(again, sums) and c2 == counts, tag
            # offset == NULL IS the robust entry: sums, counts and rows bit for bit
            rs, rc, rrows = hv.RobustRegistrationSystem(q, y, T, *tail, rows=True, **opt)
            ns, nc, nrows = hv.OffsetRegistrationSystem(q, None, y, T, *tail, rows=True, **opt)
            assert _same64(ns, rs) and nc == rc and np.array_equal(_bits(nrows), _bits(rrows)), tag
            if n in (65, 4097):
                dsums, dcounts, drows = _device_offset_system(hv, q, o[:n], y, T, tail, opt, rows=True)
                assert np.array_equal(_bits(drows), _bits(got)) and dcounts == counts and _same64(dsums, sums), tag
                dsums, dcounts, _r = _device_offset_system(hv, q, o[:n], y, T, tail, opt, rows=False)
                assert dcounts == counts and _same64(dsums, sums), tag
    # all-zero options with target values: NORMAL without weights through the OFFSET kernel; without them: the existing entries
    tail = (sc["gate"], G.SCALE, G.LIMIT)
    w = V.rows_of(sc["grid"], sc["q"], o, sc["y"], T, *tail)
    sums, counts, got = hv.OffsetRegistrationSystem(sc["q"], o, sc["y"], T, *tail, rows=True, **G.ZERO)
    assert np.array_equal(_bits(got), _bits(w["rows"]))
    G._check_system(sums, counts, w, "zero options")
    zs, zc, zrows = hv.OffsetRegistrationSystem(sc["q"], None, sc["y"], T, *tail, rows=True, **G.ZERO)
    cs_, cc, crows = hv.ColorRegistrationSystem(sc["q"], sc["y"], T, *tail, rows=True)
    assert _same64(zs[:30], cs_) and np.array_equal(_bits(zrows), _bits(crows)) and zc == dict(cc, downweighted=0, color_downweighted=0)


def test_04_offset_points_is_the_loop(oracle):
    """the loop made by hand from the one-pass entry equals the library's loop bit for bit; offset == NULL is op_volume_register_robust_points"""
    sc = K.color_scene(oracle)
    hv = _handler(K.COL_CAM, K.COL_RES)
    hv.SetCubeMap(sc["keys"], sc["vox"])
    q, y, init = sc["cloud"], sc["y"], sc["init"]
    rng = np.random.default_rng(3)
    o = (rng.integers(-4, 5, len(q)) / 1024.0).astype(F32)
    o[::97] = np.nan
    for mode, cs in (("gradient", 1.0), ("metric", 0.0), ("normal", 0.4)):
        opt = dict(linearization=mode, huber=0.01, huber_color=0.01)
        yy = y if cs > 0 else None
        want = V.loop(L.load(), lambda T: hv.OffsetRegistrationSystem(q, o, yy, T, B.TRUNC, cs, 0.0, **opt), init, 5)
        got = hv.RegisterPointsOffset(q, o, yy, init, max_iterations=5, min_step=0.0, color_scale=cs, **opt)
        assert want["iterations"] == 5 and got["invalid"] >= len(q[::97])
        G._same_result(got, want, "five iterations, %s" % mode)
        G._same_result(hv.RegisterPointsOffset(q, None, yy, init, max_iterations=4, min_step=0.0, color_scale=cs, **opt),
                       hv.RegisterPointsRobust(q, yy, init, max_iterations=4, min_step=0.0, color_scale=cs, **opt), "offset NULL, %s" % mode)
    G._same_result(hv.RegisterPointsOffset(q, None, y, init, max_iterations=4, min_step=0.0, color_scale=1.0, **G.ZERO),
                   hv.RegisterColoredPoints(q, y, init, max_iterations=4, min_step=0.0), "offset NULL, zero options", robust=False)
    got = hv.RegisterPointsOffset(np.zeros((0, 3), F32), np.zeros(0, F32), None, init)
    assert got["status"] == R.TOO_FEW_POINTS and got["iterations"] == 0 and np.array_equal(_bits(got["T"]), _bits(init))


# ---- volume against volume ---------------------------------------------------------------------------------------------------------------------
def _submap_volumes(oracle):
    if "A" not in _cache:
        sm = V.submaps(oracle)
        for name in ("A", "B"):
            hv = _handler(B.MODEL_CAM, B.MODEL_RES)
            hv.SetCubeMap(sm[name]["keys"], sm[name]["vox"])
            _cache[name] = hv
    return _cache["A"], _cache["B"]


def _same_volume_result(got, want, what, selected):
    G._same_result(got, want, what)
    assert got["selected"] == selected, (what, got["selected"], selected)


@pytest.mark.parametrize("mode,cs", [("gradient", 0.0), ("gradient", 1.0), ("metric", 0.5), ("normal", 0.0)])
def test_05_volume_entry_is_the_offset_entry_on_the_list(oracle, mode, cs):
    A, Bv = _submap_volumes(oracle)
    init = V.submaps(oracle)["init"]
    sel = dict(band=0.04, voxel_stride=2)
    xyz, sdf, y = Bv.BandVoxels(**sel)
    kw = dict(max_iterations=4, min_step=0.0, color_scale=cs, linearization=mode, huber=0.01, huber_color=0.02)
    got = A.RegisterVolume(Bv, init, **sel, **kw)
    want = A.RegisterPointsOffset(xyz, sdf, y if cs > 0 else None, init, **kw)
    print(mode, cs, {k: v for k, v in got.items() if k != "T"}, R.pose_error(got["T"]))
    assert got["iterations"] == 4 and got["used"] > len(xyz) / 4 and (got["colored"] > 0) == (cs > 0)
    _same_volume_result(got, want, "%s color_scale %g" % (mode, cs), len(xyz))
    if cs == 0.0 and mode == "gradient":
        # against the loop made by hand from the one-pass entry
        opt = dict(linearization=mode, huber=0.01, huber_color=0.02)
        hand = V.loop(L.load(), lambda T: A.OffsetRegistrationSystem(xyz, sdf, None, T, B.TRUNC, 0.0, 0.0, **opt), init, 4)
        G._same_result(got, hand, "the loop by hand")
        # NULL options: GRADIENT without weights; NULL selection and parameters: the defaults
        r = L.RegisterVolumeResult()
        T0 = np.ascontiguousarray(init, F32).reshape(16)
        L.check(L.load().op_volume_register_volume(A._h, Bv._h, T0.ctypes.data_as(L._fp), None, None, None, C.byref(r)))
        dx, ds, dy = Bv.BandVoxels()
        want = A.RegisterPointsOffset(dx, ds, dy, init, color_scale=1.0, linearization="gradient", huber=0.0, huber_color=0.0)
        got = dict(A._register_robust_result(r.robust), selected=int(r.selected))
        _same_volume_result(got, want, "NULL selection, parameters and options", len(dx))
        assert got["colored"] > 0 and got["status"] in (R.CONVERGED, R.MAX_ITERATIONS)


def test_06_hand_blocks_register_onto_themselves():
    vox = B.steep_blocks(color=True)
    hv = _handler(D.CAM_37, R.HAND_RES, trunc=0.25)
    hv.AddCubes(R.HAND_KEYS, vox)
    for mode in ("normal", "gradient", "metric"):
        for cs in (0.0, 1.0):
            got = hv.RegisterVolume(hv, None, color_scale=cs, linearization=mode, max_iterations=5)
            assert got["status"] == R.CONVERGED and got["iterations"] == 1 and got["last_step"] == 0.0, (mode, cs, got)
            assert np.array_equal(_bits(got["T"]), _bits(np.eye(4, dtype=F32))) and got["selected"] == 512 and 100 < got["used"] < 512
            assert got["rmse_residual"] == 0.0 and got["first_rmse_residual"] == 0.0 and got["rmse_color"] == 0.0 and got["rmse"] == 1 / 32
            assert got["colored"] == (got["used"] if cs > 0 else 0)
    xyz, sdf, y = hv.BandVoxels()
    sums, counts = hv.OffsetRegistrationSystem(xyz, sdf, y, np.eye(4), 0.25, 1.0, 0.0, linearization="gradient")
    assert not sums[21:29].any() and sums[30] == 0.0 and sums[29] == counts["used"] / 1024 and counts["used"] == got["used"]
    # a source of twice the target's resolution holding the same field at its own voxel centres: the centres use the source's resolution,
    # the samples the target's -- the residual is zero again wherever the target has a complete sample
    keys = np.array([(-1, -1, -1), (0, -1, -1), (-1, 0, -1), (0, 0, -1)], np.int32)
    centres = S.block_voxel_centres(keys, 2 * R.HAND_RES)
    coarse = np.empty((4, 512, 5), F32)
    coarse[..., 0] = F32(2.0) * (centres[..., 2] - F32(R.HAND_Z0))
    coarse[..., 1] = 1.0
    coarse[..., 2:] = (F32(0.5) + centres[..., 0])[..., None]
    src = _handler(D.CAM_37, 2 * R.HAND_RES, trunc=0.25)
    src.AddCubes(keys, coarse)
    got = hv.RegisterVolume(src, None, band=0.125, color_scale=1.0, max_iterations=5)
    k, v = src.GetCubeMap(sort=False)
    xyz, sdf, y, _i = V.select(k, v, 2 * R.HAND_RES, 0.25, band=0.125)
    w = V.rows_of(S.Grid(R.HAND_KEYS, vox, R.HAND_RES), xyz, sdf, y, np.eye(4, dtype=F32), 0.25, color_scale=1.0, mode=B.GRADIENT)
    assert got["selected"] == len(xyz) and got["used"] == (w["reason"] == 0).sum() > 20 and got["invalid"] == (w["reason"] == 1).sum() > 0
    assert got["status"] == R.CONVERGED and got["iterations"] == 1 and got["rmse_residual"] == 0.0 and np.array_equal(_bits(got["T"]), _bits(np.eye(4, dtype=F32)))


def test_07_convergence_case_on_the_device(oracle):
    """tests/test_register_volume_cpu.py's case through the library: T is the restated loop's bit for bit (the device's sums differ from math.fsum's
    by at most (used - 1) 2^-53 relative, far below what moves a float32 component of the step), and so are the iteration count, the status and
    the counts; the three conditions of the CPU test hold for the device's own result."""
    ref, _t, _r, selected = V.case(oracle, L.load(), offsets=True)
    _zero, t0, _r0, _n = V.case(oracle, L.load(), offsets=False)
    A, Bv = _submap_volumes(oracle)
    # (the restated list is in the oracle's sorted block order, the device's in its pool order: math.fsum's sums do not depend on the order)
    got = A.RegisterVolume(Bv, V.submaps(oracle)["init"], band=V.CASE_BAND, min_weight=V.CASE_MIN_WEIGHT, voxel_stride=V.CASE_STRIDE, max_iterations=V.CASE_ITERATIONS,
                           min_step=V.CASE_MIN_STEP, max_distance=B.TRUNC, color_scale=0.0, linearization="gradient")
    t, r = R.pose_error(got["T"])
    print("device: %d selected, %d iterations, %s, last step %.2e, %.3f mm / %.5f deg, used %d" % (
        got["selected"], got["iterations"], got["status_name"], got["last_step"], t * 1e3, r, got["used"]))
    assert got["selected"] == selected == 14845
    assert np.array_equal(_bits(got["T"]), _bits(ref["T"]))
    for key in ("iterations", "status", "used", "invalid", "no_gradient", "too_far", "first_used", "downweighted", "first_downweighted"):
        assert got[key] == ref[key], (key, got[key], ref[key])
    assert t < 0.006 and t < t0 and got["used"] >= got["selected"] / 2 and got["status"] == R.CONVERGED


def test_08_queued_frames_are_seen_and_the_volumes_only_read(oracle):
    sm = V.submaps(oracle)
    fr = B.model(oracle)["frames"]
    A, Bv = _submap_volumes(oracle)
    init = sm["init"]
    kw = dict(band=0.04, voxel_stride=2, max_iterations=3, min_step=0.0, color_scale=1.0)
    want = A.RegisterVolume(Bv, init, **kw)
    # the target's frames still queued (no accessor called first): the samples do not depend on the pool order, so the result is the same bits
    queued = _handler(B.MODEL_CAM, B.MODEL_RES)
    for f in fr[V.SUB_A]:
        queued.IntegrateImage(*f)
    got = queued.RegisterVolume(Bv, init, **kw)
    _same_volume_result(got, want, "the target's frames were queued", want["selected"])
    # the source's frames still queued: its pool order is the fusion's, so the list is a permutation -- the counts are the same, the sums differ
    # in the rounding of their additions
    source = _handler(B.MODEL_CAM, B.MODEL_RES)
    for f in fr[V.SUB_B]:
        source.IntegrateImage(*f)
    got = A.RegisterVolume(source, init, **kw)
    for key in ("selected", "iterations", "status", "used", "invalid", "no_gradient", "too_far", "first_used", "colored", "first_colored"):
        assert got[key] == want[key], (key, got[key], want[key])
    assert np.allclose(got["T"], want["T"], rtol=0, atol=1e-5)
    for hv, name in ((queued, "A"), (source, "B"), (A, "A"), (Bv, "B")):
        k, v = hv.GetCubeMap()
        assert np.array_equal(k, sm[name]["keys"]) and np.array_equal(_bits(v), _bits(sm[name]["vox"])), name
    # an empty selection: zero sums, TOO_FEW_POINTS, T = init_T
    got = A.RegisterVolume(Bv, init, min_weight=1000.0)
    assert got["selected"] == 0 and got["status"] == R.TOO_FEW_POINTS and got["iterations"] == 0 and got["used"] == 0 and np.array_equal(_bits(got["T"]), _bits(init))
    assert got["rmse"] == 0.0 and got["rmse_residual"] == 0.0
    empty = _handler(B.MODEL_CAM, B.MODEL_RES)
    got = A.RegisterVolume(empty, init)
    assert got["selected"] == 0 and got["status"] == R.TOO_FEW_POINTS and np.array_equal(_bits(got["T"]), _bits(init))
    got = empty.RegisterVolume(Bv, init, band=0.04, voxel_stride=2)
    assert got["selected"] == 14845 and got["used"] == 0 and got["invalid"] == 14845 and got["status"] == R.TOO_FEW_POINTS


def test_09_refusals(oracle):
    lib = L.load()
    A, Bv = _submap_volumes(oracle)
    T = np.eye(4, dtype=F32).reshape(16)
    fp = T.ctypes.data_as(L._fp)
    r = L.RegisterVolumeResult()
    for args in ((None, Bv._h, fp, None, None, None, C.byref(r)), (A._h, None, fp, None, None, None, C.byref(r)), (A._h, Bv._h, None, None, None, None, C.byref(r)),
                 (A._h, Bv._h, fp, None, None, None, None)):
        assert lib.op_volume_register_volume(*args) == L.OP_ERR_INVALID
    n = C.c_size_t(0)
    for bad in (L.BandParams(0.04, 1.0, 0), L.BandParams(0.04, 1.0, 3), L.BandParams(0.04, 1.0, 16), L.BandParams(0.04, 1.0, -2), L.BandParams(0.04, -1.0, 1),
                L.BandParams(0.04, float("nan"), 1), L.BandParams(0.04, float("inf"), 1), L.BandParams(float("nan"), 1.0, 1)):
        assert lib.op_volume_register_volume(A._h, Bv._h, fp, C.byref(bad), None, None, C.byref(r)) == L.OP_ERR_INVALID
        assert lib.op_volume_band_voxels(Bv._h, C.byref(bad), None, None, None, L.OP_MEM_HOST, 0, C.byref(n)) == L.OP_ERR_INVALID
    assert lib.op_volume_band_voxels(Bv._h, None, None, None, None, 5, 0, C.byref(n)) == L.OP_ERR_INVALID
    assert lib.op_volume_band_voxels(Bv._h, None, None, None, None, L.OP_MEM_HOST, 0, None) == L.OP_ERR_INVALID
    o = L.RegisterOptions(3, 0.0, 0.0)
    assert lib.op_volume_register_volume(A._h, Bv._h, fp, None, None, C.byref(o), C.byref(r)) == L.OP_ERR_INVALID
    p = A._register_color_params(-1, None, None, None, None, None)
    assert lib.op_volume_register_volume(A._h, Bv._h, fp, None, C.byref(p), None, C.byref(r)) == L.OP_ERR_INVALID
    q = np.zeros((4, 3), F32)
    sums = np.zeros(31)
    assert lib.op_volume_register_offset_system(A._h, None, None, None, 4, L.OP_MEM_HOST, fp, 0.1, 0.0, 0.0, None, sums.ctypes.data_as(C.POINTER(C.c_double)), None,
                                                None) == L.OP_ERR_INVALID
    assert lib.op_volume_register_offset_points(A._h, C.c_void_p(q.ctypes.data), None, None, 4, L.OP_MEM_HOST, None, None, None, C.byref(L.RegisterRobustResult())) == L.OP_ERR_INVALID


def test_10_volumes_on_different_devices_are_refused():
    count = C.c_int(0)
    L.check(L.load().op_device_count(C.byref(count)))
    if count.value < 2:
        pytest.skip("one device")
    a, b = _handler(D.CAM_37, 0.04), None
    hcam = I.PinholeCamera()
    hcam.fx, hcam.fy, hcam.cx, hcam.cy, hcam.width, hcam.height, hcam.depth_scale = D.CAM_37
    b = I.CubeHandler(hcam, device=1, max_blocks=1 << 10)
    T = np.eye(4, dtype=F32).reshape(16)
    assert L.load().op_volume_register_volume(a._h, b._h, T.ctypes.data_as(L._fp), None, None, None, C.byref(L.RegisterVolumeResult())) == L.OP_ERR_INVALID


# ---- the driver and the class surface ----------------------------------------------------------------------------------------------------------
DRIVER = ["--synthetic", "6", "5", "1", "--res", "0.04", "--submaps", "2"]


def _driver_volumes(d):
    """the two volumes examples/cpp/SubmapAlignment wrote with --out: the model submap 1 was registered against, and submap 1 (the driver's camera,
    voxel size and truncation)"""
    out = []
    for name in ("model_1.map", "submap_1.map"):
        hv = I.CubeHandler(I.PinholeCamera(), device=0, max_blocks=1 << 13)
        hv.SetVoxelResolution(0.04)
        hv.ReadFromFile(d / name)
        out.append(hv)
    return out


def _close(got, want, what):
    """two runs over the same source volume uploaded twice: the list is the same up to the order of its blocks, so everything that is counted at the
    start pose is equal and the rest equal up to the rounding of the sums' additions"""
    for k in ("selected", "first_used", "first_colored", "iterations", "status"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert abs(got["used"] - want["used"]) <= 2 + want["used"] // 1000, (what, got["used"], want["used"])
    assert np.allclose(got["T"], want["T"], rtol=0, atol=1e-5), (what, got["T"], want["T"])
    for k in ("first_rmse", "first_rmse_color", "first_rmse_residual"):
        assert abs(got[k] - want[k]) <= 1e-12 + 1e-9 * abs(want[k]), (what, k, got[k], want[k])


def test_11_driver_and_class_surface(tmp_path):
    """examples/cpp/SubmapAlignment completes on every path at the smallest synthetic setting; what its volume path found is what the Python entry
    finds for the volumes it dumped; CubeHandler::RegisterVolume / GetBandVoxels compile under g++ -std=c++11 and agree with the C-ABI"""
    exe = os.path.join(ROOT, "examples", "cpp", "SubmapAlignment.bin")
    assert os.path.exists(exe), "examples/cpp/SubmapAlignment.bin is not built (__graft_entry__.build())"
    out = {}
    for path, extra in (("volume", ["--out", str(tmp_path)]), ("cloud", []), ("mesh", []), ("volume-geometric", ["--color", "off", "--voxel-stride", "2", "--band", "-1"])):
        run = subprocess.run([exe] + DRIVER + ["--path", path.split("-")[0]] + extra, capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
        lines = run.stdout.strip().splitlines()
        print(path, lines)
        out[path] = json.loads(lines[-1])
        reg = out[path]["registered"]
        assert len(reg) == 1 and len([l for l in lines if l.startswith("submap 1 ")]) == 1 and reg[0]["points"] > 1000
        assert reg[0]["used"] > 0 or not path.startswith("volume")          # (the cloud route may lose every point: the whole band with target value 0 diverges)
        assert out[path]["doubled_surface"]["valid"] > 1000 and out[path]["doubled_surface"]["rmse_mm"] > 0
        assert 40 < reg[0]["error_before"]["mm"] < 50
    assert out["volume"]["color"] == "on" and out["cloud"]["color"] == "off" and out["volume-geometric"]["registered"][0]["colored"] == 0
    assert out["volume-geometric"]["voxel_stride"] == 2 and out["volume-geometric"]["band"] == 0 and F32(out["volume"]["band"]) == F32(2.0) * F32(0.04)
    bad = subprocess.run([exe] + DRIVER + ["--path", "surface"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "usage" in bad.stdout
    bad = subprocess.run([exe] + DRIVER + ["--voxel-stride", "3"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "usage" in bad.stdout
    # the volume path's dumps through the Python entry
    model, sub = _driver_volumes(tmp_path)
    reg = out["volume"]["registered"][0]
    start = np.array(reg["start"], F32).reshape(4, 4)
    got = model.RegisterVolume(sub, start, max_iterations=30, color_scale=1.0, linearization="gradient")
    want = dict(selected=reg["points"], first_used=reg["first_used"], first_colored=got["first_colored"], iterations=reg["iterations"], status=reg["status"], used=reg["used"],
                T=np.array(reg["T"], F32).reshape(4, 4), first_rmse=got["first_rmse"], first_rmse_color=got["first_rmse_color"], first_rmse_residual=got["first_rmse_residual"])
    _close(got, want, "the driver's volume path")
    assert abs(got["rmse"] - reg["rmse"]) < 1e-6 and abs(got["rmse_residual"] - reg["rmse_residual"]) < 1e-6
    # the class surface
    check = tmp_path / "register_volume_surface_check"
    host, lib = os.path.join(ROOT, "host", "one_piece"), os.path.join(ROOT, "onepiece_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I", host, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "register_volume_surface_check.cpp"),
                           "-L", host, "-lone_piece_hip_host", "-L", lib, "-lonepiece_hip", "-Wl,-rpath," + host, "-Wl,-rpath," + lib, "-o", str(check)])
    (tmp_path / "start.txt").write_text(" ".join("%.9g" % v for v in start.reshape(-1)))
    run = subprocess.run([str(check), str(tmp_path / "model_1.map"), str(tmp_path / "submap_1.map"), "0.04", str(tmp_path / "start.txt")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:] + run.stderr[-2000:])   # (7: RegisterVolume is not the offset entry on GetBandVoxels' list)
    rows = {l.split()[0]: l.split()[1:] for l in run.stdout.strip().splitlines() if l.split() and l.split()[0] in ("given", "defaults")}

    def parsed(row):
        names = ("selected", "iterations", "status", "used", "invalid", "no_gradient", "too_far", "first_used", "colored", "first_colored")
        d = {k: int(v) for k, v in zip(names, row[:10])}
        d.update({k: float(v) for k, v in zip(("rmse", "first_rmse", "first_rmse_color", "first_rmse_residual"), row[10:14])})
        assert float(row[14]) == d["rmse"]
        d["T"] = np.array([F32(v) for v in row[15:]], F32).reshape(4, 4)
        return d
    want = parsed(rows["given"])
    got = model.RegisterVolume(sub, start, band=0.0, min_weight=2.0, voxel_stride=2, max_iterations=5, max_distance=0.1, min_step=0.0, min_points=6, color_scale=0.5,
                               max_color_residual=0.25, linearization="metric", huber=0.01, huber_color=0.02)
    assert want["selected"] > 200 and want["used"] > 100 and want["colored"] > 0
    _close(got, want, "RegisterVolume with everything given")
    _close(model.RegisterVolume(sub, start), parsed(rows["defaults"]), "RegisterVolume with the defaults")
