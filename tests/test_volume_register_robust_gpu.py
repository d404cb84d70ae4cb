"""op_volume_register_robust_* on the device (csrc/volume_register.hip, the ROBUST instantiations of k_volume_register) against the numpy restatement
of its definition (tests/volume_register_robust_common.py) over volumes that come from the oracle or from hand-made blocks -- never from the code
under test: per linearisation, with and without Huber weights, geometric and coloured, every row of sixteen bit for bit, the seven counts exactly,
the 31 sums to the rounding of their additions; all-zero options against the colour and the geometric entries bit for bit; the loop against the
same loop made by hand from the one-pass entry; the frame entry against the points entry; the convergence cases of
tests/test_volume_register_robust_cpu.py against the restated loop.

Volumes: the sliding scene of the colour tests (eight 64 x 48 frames, 2 cm voxels), seven hand-made blocks of 1/32 m voxels holding s = 2 (z - Z0)
and colour 0.5 + x, the forty-frame model and the eight-frame scene of the convergence cases.  Batches of 1, 63, 64, 65, 255, 256, 257 and 4097
points (the wave and workgroup edges)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import deintegrate_common as D
import volume_register_color_common as K
import volume_register_common as R
import volume_register_robust_common as B
import volume_sample_common as S
from onepiece_amd import _lib as L
from onepiece_amd import integration as I

pytestmark = pytest.mark.gpu

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 63, 64, 65, 255, 256, 257, 4097)
SCALE, LIMIT = 0.6, 0.05                                              # color_scale, max_color_residual of the coloured configurations
# (color_scale, with both Huber thresholds or without) per configuration; the thresholds are the scene's (_scene)
CONFIGS = [(0.0, False), (0.0, True), (SCALE, False), (SCALE, True)]
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same64(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def _handler(camt, res, trunc=B.TRUNC, max_blocks=1 << 13):
    hcam = I.PinholeCamera()
    hcam.fx, hcam.fy, hcam.cx, hcam.cy, hcam.width, hcam.height, hcam.depth_scale = camt
    hv = I.CubeHandler(hcam, device=0, max_blocks=max_blocks)
    hv.SetVoxelResolution(res)
    hv.SetTruncation(trunc)
    return hv


def _scene(oracle, name):
    """-> dict(camt, res, frames, keys, vox, grid, q [4097,3], y [4097], T, gate, huber, huber_color)"""
    if name in _cache:
        return _cache[name]
    if name == "slide":
        sc = K.color_scene(oracle)
        T = D.perturbed(np.eye(4, dtype=F32), 1)
        out = dict(camt=K.COL_CAM, res=K.COL_RES, frames=sc["frames"], keys=sc["keys"], vox=sc["vox"], grid=sc["grid"], gate=0.05, T=T, huber=0.01, huber_color=0.01)
        out["q"], out["y"] = K.mixed_cloud(sc["grid"], sc["keys"], K.COL_RES, sc["cloud"], sc["y"], T, 0.05)
    else:
        vox = B.steep_blocks(color=True)
        out = dict(camt=D.CAM_37, res=R.HAND_RES, frames=None, keys=R.HAND_KEYS, vox=vox, grid=S.Grid(R.HAND_KEYS, vox, R.HAND_RES), gate=0.25, T=np.eye(4, dtype=F32),
                   huber=1 / 64, huber_color=1 / 64)
        q = R.hand_cloud(n=4097 - len(R.HAND_POINTS))
        with np.errstate(all="ignore"):
            c = F32(0.5) + q[:, 0]
            y = K.intensity(np.stack([c, c, c], axis=1))
        idx = np.arange(len(q))
        y[idx % 2 == 0] += F32(0.03125)                               # coloured and down-weighted
        y[idx % 5 == 0] += F32(0.0625)                                # gated by LIMIT
        y[idx % 16 == 1] = np.nan
        y[idx % 32 == 7] = -np.inf
        out["q"], out["y"] = q, np.ascontiguousarray(y)
    out["want"] = {}
    _cache[name] = out
    return out


def _args(sc, mode, cs, weights):
    """the positional tail (max_distance, color_scale, max_color_residual) and the options of a configuration"""
    return (sc["gate"], cs, LIMIT), dict(linearization=mode, huber=sc["huber"] if weights else 0.0, huber_color=sc["huber_color"] if weights else 0.0)


def _want(sc, mode, cs, weights):
    """the restatement of all 4097 points under a configuration (computed once)"""
    key = (mode, cs, weights)
    if key not in sc["want"]:
        tail, o = _args(sc, mode, cs, weights)
        sc["want"][key] = B.rows_of(sc["grid"], sc["q"], sc["y"], sc["T"], *tail, mode=mode, huber=o["huber"], huber_color=o["huber_color"])
    return sc["want"][key]


def _head(w, n):
    return {k: v[:n] for k, v in w.items()}


def _volume(sc, source):
    hv = _handler(sc["camt"], sc["res"])
    if source == "fused" and sc["frames"] is not None:
        for f in sc["frames"]:
            hv.IntegrateImage(*f)                                     # (no accessor called: the last frames are still queued)
    elif sc["frames"] is not None:
        hv.SetCubeMap(sc["keys"], sc["vox"])
    else:
        hv.AddCubes(sc["keys"], sc["vox"])
    return hv


def _check_system(got_sums, got_counts, w, what):
    """the counts exactly; each of the 31 sums within (k - 1) 2^-53 sum |term| of math.fsum, k the number of terms the slot received"""
    sums, bound, counts = B.fold(w)
    assert got_counts == counts, (what, got_counts, counts)
    if counts["used"] == 0:
        assert not np.asarray(got_sums).any(), what
        return
    err = np.abs(np.asarray(got_sums) - sums)
    assert (err <= bound).all(), (what, int(np.argmax(err - bound)), err, bound)


def _device_system(hv, q, y, T, tail, o, rows):
    """op_volume_register_robust_system with every buffer on the device, 4 bytes into its allocation and fenced by sentinels"""
    import torch
    n = len(q)
    dev = torch.device("cuda:0")
    pts = torch.full((3 * n + 2,), 7.0, dtype=torch.float32, device=dev)
    pts[1:1 + 3 * n] = torch.from_numpy(np.ascontiguousarray(q).reshape(-1)).to(dev)
    yy = torch.full((n + 2,), 7.0, dtype=torch.float32, device=dev)
    yy[1:1 + n] = torch.from_numpy(np.ascontiguousarray(y)).to(dev)
    out = torch.full((16 * n + 2,), 12345.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    sums, counts = np.zeros(31), np.zeros(7, np.uint64)
    Tm = np.ascontiguousarray(T, F32).reshape(16)
    opt = L.RegisterOptions(o["linearization"], o["huber"], o["huber_color"])
    L.check(L.load().op_volume_register_robust_system(hv._h, C.c_void_p(pts[1:].data_ptr()), C.c_void_p(yy[1:].data_ptr()), n, L.OP_MEM_DEVICE, Tm.ctypes.data_as(L._fp),
                                                      float(tail[0]), float(tail[1]), float(tail[2]), C.byref(opt), sums.ctypes.data_as(C.POINTER(C.c_double)),
                                                      counts.ctypes.data_as(L._u64p), C.c_void_p(out[1:].data_ptr()) if rows else None))
    host = out.cpu().numpy()
    assert host[0] == 12345.0 and host[-1] == 12345.0, "a write outside the n rows"
    if not rows:
        assert (host == 12345.0).all()
    return sums, dict(zip(B.COUNT_NAMES, (int(c) for c in counts))), host[1:-1].reshape(n, 16)


@pytest.mark.parametrize("mode", [B.NORMAL, B.GRADIENT, B.METRIC])
@pytest.mark.parametrize("name,source", [("slide", "fused"), ("slide", "uploaded"), ("hand", "uploaded")])
def test_01_system_against_the_restatement(oracle, name, source, mode):
    sc = _scene(oracle, name)
    hv = _volume(sc, source)
    T = sc["T"]
    for cs, weights in CONFIGS:
        tail, o = _args(sc, mode, cs, weights)
        whole = _want(sc, mode, cs, weights)
        for n in SIZES:
            tag = "%s %s mode %d color_scale %g weights %d n=%d" % (name, source, mode, cs, weights, n)
            w = _head(whole, n)
            seen = {k: int((w["reason"] == k).sum()) for k in range(4)}
            bare = (w["reason"] == 0) & ~w["colored"]
            nonfinite = int((bare & ~np.isfinite(sc["y"][:n])).sum())
            if n in (63, 4097):
                print(tag, seen, "coloured", int(w["colored"].sum()), "down-weighted", int(w["down"].sum()), int(w["cdown"].sum()), "used with a non-finite intensity", nonfinite)
            if n >= 63:
                assert min(seen.values()) > 0, (tag, "the batch holds every reject reason")
                if weights:
                    assert 0 < w["down"].sum() < seen[0], (tag, "down-weighted and fully weighted points")
                if cs > 0:
                    assert w["colored"].any() and nonfinite > 0, tag
                    if weights and n >= 255:                          # (the hand-made cloud's first 63 points hold seven coloured ones)
                        assert 0 < w["cdown"].sum() < w["colored"].sum(), tag
            sums, counts, got = hv.RobustRegistrationSystem(sc["q"][:n], sc["y"][:n], T, *tail, rows=True, **o)
            bad = (_bits(got) != _bits(w["rows"])).any(axis=1)
            assert not bad.any(), "%s: %d rows differ, first %d" % (tag, int(bad.sum()), int(np.argmax(bad)))
            _check_system(sums, counts, w, tag)
            plain, c2 = hv.RobustRegistrationSystem(sc["q"][:n], sc["y"][:n], T, *tail, **o)      # rows = NULL: the same bits
            assert _same64(plain, sums) and c2 == counts, tag
            if n in (65, 4097):
                dsums, dcounts, drows = _device_system(hv, sc["q"][:n], sc["y"][:n], T, tail, o, rows=True)
                assert np.array_equal(_bits(drows), _bits(got)) and dcounts == counts and _same64(dsums, sums), tag
                dsums, dcounts, _r = _device_system(hv, sc["q"][:n], sc["y"][:n], T, tail, o, rows=False)
                assert dcounts == counts and _same64(dsums, sums), tag
    if sc["frames"] is not None:
        k, v = hv.GetCubeMap()
        assert np.array_equal(k, sc["keys"]) and np.array_equal(_bits(v), _bits(sc["vox"]))


ROBUST_KEYS = ("downweighted", "color_downweighted", "first_downweighted")


def _same_result(got, want, what, robust=True):
    assert np.array_equal(_bits(got["T"]), _bits(want["T"])), what
    for k in ("iterations", "status", "used", "invalid", "no_gradient", "too_far", "first_used", "colored", "first_colored") + (ROBUST_KEYS if robust else ()):
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("rmse", "first_rmse", "last_step", "rmse_color", "first_rmse_color") + (("rmse_residual", "first_rmse_residual") if robust else ()):
        assert np.float64(got[k]).view(np.uint64) == np.float64(want[k]).view(np.uint64), (what, k, got[k], want[k])


ZERO = dict(linearization="normal", huber=0.0, huber_color=0.0)


def test_02_zero_options_are_the_existing_entries(oracle):
    sc = _scene(oracle, "slide")
    hv = _volume(sc, "uploaded")
    T, gate = sc["T"], sc["gate"]
    lib = L.load()
    for n in SIZES:
        q, y = sc["q"][:n], sc["y"][:n]
        for cs in (SCALE, 0.0):
            want_sums, want_counts, want_rows = hv.ColorRegistrationSystem(q, y, T, gate, cs, LIMIT, rows=True)
            sums, counts, rows = hv.RobustRegistrationSystem(q, y, T, gate, cs, LIMIT, rows=True, **ZERO)
            assert _same64(sums[:30], want_sums) and _same64(sums[30], sums[29]) and np.array_equal(_bits(rows), _bits(want_rows)), (n, cs)
            assert counts == dict(want_counts, downweighted=0, color_downweighted=0), (n, cs)
            plain, c2 = hv.RobustRegistrationSystem(q, y, T, gate, cs, LIMIT, **ZERO)
            assert _same64(plain, sums) and c2 == counts, (n, cs)
        # options = NULL through the C-ABI, and color_scale 0 against the geometric entry (the intensities are not read: NULL is accepted)
        gs, gc, grows = hv.RegistrationSystem(q, T, gate, rows=True)
        sums, counts, rows = np.zeros(31), np.zeros(7, np.uint64), np.empty((n, 16), F32)
        Tm = np.ascontiguousarray(T, F32).reshape(16)
        L.check(lib.op_volume_register_robust_system(hv._h, C.c_void_p(q.ctypes.data), None, n, L.OP_MEM_HOST, Tm.ctypes.data_as(L._fp), gate, 0.0, LIMIT, None,
                                                     sums.ctypes.data_as(C.POINTER(C.c_double)), counts.ctypes.data_as(L._u64p), C.c_void_p(rows.ctypes.data)))
        assert _same64(sums[:28], gs) and sums[28] == 0.0 and _same64(sums[29:], [gs[27], gs[27]]) and [int(c) for c in counts] == [gc[k] for k in R.COUNT_NAMES] + [0, 0, 0]
        assert np.array_equal(_bits(rows[:, :8]), _bits(grows)) and not rows[:, 8:].any()
    # huber_color alone with color_scale 0 is still the geometric system
    a, ca = hv.RobustRegistrationSystem(sc["q"], None, T, gate, 0.0, 0.0, linearization="normal", huber=0.0, huber_color=0.01)
    assert _same64(a[:28], hv.RegistrationSystem(sc["q"], T, gate)[0]) and ca["color_downweighted"] == 0
    dsums, dcounts, drows = _device_system(hv, sc["q"][:257], sc["y"][:257], T, (gate, SCALE, LIMIT), dict(linearization=0, huber=0.0, huber_color=0.0), rows=True)
    want_sums, _c, want_rows = hv.ColorRegistrationSystem(sc["q"][:257], sc["y"][:257], T, gate, SCALE, LIMIT, rows=True)
    assert _same64(dsums[:30], want_sums) and np.array_equal(_bits(drows), _bits(want_rows))
    # the loops
    cs = K.color_scene(oracle)
    kw = dict(max_iterations=5, min_step=0.0)
    want = hv.RegisterColoredPoints(cs["cloud"], cs["y"], cs["init"], **kw)
    got = hv.RegisterPointsRobust(cs["cloud"], cs["y"], cs["init"], color_scale=1.0, **kw, **ZERO)
    _same_result(got, want, "zero options, coloured points", robust=False)
    assert got["downweighted"] == got["color_downweighted"] == got["first_downweighted"] == 0 and got["rmse_residual"] == got["rmse"] and got["first_rmse_residual"] == got["first_rmse"]
    want = hv.RegisterPoints(cs["cloud"], cs["init"], **kw)
    got = hv.RegisterPointsRobust(cs["cloud"], None, cs["init"], **kw, **ZERO)
    _same_result(got, dict(want, colored=0, first_colored=0, rmse_color=0.0, first_rmse_color=0.0), "zero options, points", robust=False)
    depth, rgb, pose = cs["frames"][3]
    init = D.perturbed(pose, 1)
    for stride in (1, 3):
        kw = dict(pixel_stride=stride, max_iterations=4, min_step=0.0)
        _same_result(hv.RegisterFrameRobust(depth, rgb, init, **kw, **ZERO), hv.RegisterRGBD(depth, rgb, init, **kw), "zero options, rgbd, stride %d" % stride, robust=False)
        want = hv.RegisterDepth(depth, init, **kw)
        _same_result(hv.RegisterFrameRobust(depth, None, init, **kw, **ZERO), dict(want, colored=0, first_colored=0, rmse_color=0.0, first_rmse_color=0.0),
                     "zero options, depth, stride %d" % stride, robust=False)
    o = L.RegisterOptions(7, 7.0, 7.0)
    L.check(lib.op_volume_register_robust_default_options(hv._h, C.byref(o)))
    assert (o.linearization, o.huber, o.huber_color) == (L.OP_REGISTER_LIN_METRIC, 0.0, 0.0)


def test_03_the_sums_are_repeatable(oracle):
    sc = _scene(oracle, "slide")
    hv = _volume(sc, "uploaded")
    T = sc["T"]
    big_q, big_y = np.ascontiguousarray(np.tile(sc["q"], (80, 1))), np.ascontiguousarray(np.tile(sc["y"], 80))   # 327 760 points: two trips for some lanes
    for mode, cs in ((B.METRIC, SCALE), (B.GRADIENT, 0.0)):
        tail, o = _args(sc, mode, cs, True)
        for q, y in ((sc["q"], sc["y"]), (big_q, big_y)):
            a, ca = hv.RobustRegistrationSystem(q, y, T, *tail, **o)
            b, cb = hv.RobustRegistrationSystem(q, y, T, *tail, **o)
            assert ca == cb and ca["downweighted"] > 0.1 * len(q) and _same64(a, b)
            if len(q) == len(sc["q"]):
                c, cc, r1 = hv.RobustRegistrationSystem(q, y, T, *tail, rows=True, **o)
                d, cd, r2 = hv.RobustRegistrationSystem(q, y, T, *tail, rows=True, **o)
                assert cc == cd == ca and _same64(c, a) and _same64(d, a) and np.array_equal(_bits(r1), _bits(r2))
        # the long batch is 80 times the short one: the counts exactly, the sums to the rounding of the additions
        w = _want(sc, mode, cs, True)
        _check_system(a, ca, {k: np.tile(v, (80, 1) if v.ndim == 2 else 80) for k, v in w.items()}, "80 x 4097 points, mode %d" % mode)


def _by_hand(hv, q, y, init, max_iterations, color_scale, o, limit=0.0, min_step=0.0, min_points=6, max_distance=B.TRUNC, trace=None):
    return B.loop(L.load(), lambda T: hv.RobustRegistrationSystem(q, y, T, max_distance, color_scale, limit, **o), init, max_iterations, min_step=min_step,
                  min_points=min_points, trace=trace)


@pytest.mark.parametrize("mode", ["normal", "gradient", "metric"])
def test_04_the_loop_is_the_loop(oracle, mode):
    """six rounds made by hand from the one-pass entry equal the library's loop bit for bit: coloured and geometric, with both thresholds"""
    sc = K.color_scene(oracle)
    hv = _cache.get("hv_slide")
    if hv is None:
        hv = _cache["hv_slide"] = _handler(K.COL_CAM, K.COL_RES)
        hv.SetCubeMap(sc["keys"], sc["vox"])
    q, y, init = sc["cloud"], sc["y"], sc["init"]
    o = dict(linearization=mode, huber=0.01, huber_color=0.01)
    trace = []
    want = _by_hand(hv, q, y, init, 6, 1.0, o, trace=trace)
    got = hv.RegisterPointsRobust(q, y, init, max_iterations=6, min_step=0.0, color_scale=1.0, **o)
    print(mode, {k: v for k, v in got.items() if k != "T"})
    assert want["iterations"] == 6 and want["status"] == R.MAX_ITERATIONS and want["colored"] > 7500 and want["first_downweighted"] > 1000
    _same_result(got, want, "six iterations, coloured")
    _same_result(hv.RegisterPointsRobust(q, None, init, max_iterations=6, min_step=0.0, **o), _by_hand(hv, q, None, init, 6, 0.0, o), "six iterations, geometric")
    _same_result(hv.RegisterPointsRobust(q, y, init, max_iterations=6, min_step=0.0, color_scale=0.3, max_color_residual=0.02, linearization=mode, huber=0.0, huber_color=0.005),
                 _by_hand(hv, q, y, init, 6, 0.3, dict(linearization=mode, huber=0.0, huber_color=0.005), limit=0.02), "color_scale 0.3, gated, huber_color alone")
    # the stop rule: a min_step the second step undercuts and the first does not
    steps = [t[4] for t in trace]
    assert steps[1] < steps[0]
    min_step = float(F32(np.sqrt(steps[0] * steps[1])))
    want = _by_hand(hv, q, y, init, 6, 1.0, o, min_step=min_step)
    assert want["iterations"] == 2 and want["status"] == R.CONVERGED
    _same_result(hv.RegisterPointsRobust(q, y, init, max_iterations=6, min_step=min_step, color_scale=1.0, **o), want, "converged at the second step")
    # max_iterations = 0, n = 0 and the empty volume
    got = hv.RegisterPointsRobust(q, y, init, max_iterations=0, color_scale=1.0, **o)
    assert got["status"] == R.MAX_ITERATIONS and got["iterations"] == 0 and got["downweighted"] == got["first_downweighted"] == trace[0][1]["downweighted"]
    assert got["rmse_residual"] == got["first_rmse_residual"] > 0
    empty = _handler(K.COL_CAM, K.COL_RES)
    for what, h, qq, yy in (("the empty volume", empty, q[:300], y[:300]), ("n = 0", hv, np.zeros((0, 3), F32), np.zeros(0, F32))):
        sums, counts, rows = h.RobustRegistrationSystem(qq, yy, init, B.TRUNC, 1.0, 0.0, rows=True, **o)
        assert not sums.any() and counts == dict({k: 0 for k in B.COUNT_NAMES}, invalid=len(qq)) and not rows.any(), what
        got = h.RegisterPointsRobust(qq, yy, init, color_scale=1.0, **o)
        assert got["status"] == R.TOO_FEW_POINTS and got["iterations"] == 0 and np.array_equal(_bits(got["T"]), _bits(init)) and got["downweighted"] == 0, what


@pytest.mark.parametrize("stride", [1, 3])
def test_05_frame_entry_is_the_points_entry(oracle, stride):
    sc = K.color_scene(oracle)
    hv = _cache.get("hv_slide")
    if hv is None:
        hv = _cache["hv_slide"] = _handler(K.COL_CAM, K.COL_RES)
        hv.SetCubeMap(sc["keys"], sc["vox"])
    depth, rgb, pose = sc["frames"][4]
    depth = depth.copy()
    depth[5, 7] = 0.0                                                 # pixels without depth are skipped, on and off the stride's lattice
    depth[6, 9] = 0.0
    depth[9, 12] = 0.0
    init = D.perturbed(pose, 1)
    lib = L.load()
    w, h = K.COL_CAM[4], K.COL_CAM[5]
    pts, n = np.zeros((w * h, 3), F32), C.c_size_t(0)
    mask = depth > 0
    index = np.cumsum(mask.reshape(-1)) - 1                           # pixel -> row of the compacted cloud
    keep = np.zeros((h, w), bool)
    keep[::stride, ::stride] = True
    sel = (keep & mask).reshape(-1)
    y = K.intensity_of_bytes(rgb).reshape(-1)[sel]                    # the restated intensity of the kept pixels, row-major
    o = dict(linearization="metric", huber=0.01, huber_color=0.01)
    kw = dict(max_iterations=5, min_step=0.0)
    wants = {}
    for fmt in ("f32", "u16"):
        raw = depth if fmt == "f32" else np.round(depth * 1000.0).astype(np.uint16)
        L.check(lib.op_points_from_depth(C.byref(hv.camera), C.c_void_p(raw.ctypes.data), L.OP_DEPTH_F32 if fmt == "f32" else L.OP_DEPTH_U16, L.OP_MEM_HOST, 0,
                                         C.c_void_p(pts.ctypes.data), C.byref(n)))
        assert n.value == mask.sum() == w * h - 3
        sub = pts[index[sel]]
        want = hv.RegisterPointsRobust(sub, y, init, color_scale=1.0, **kw, **o)
        got = hv.RegisterFrameRobust(raw, rgb, init, pixel_stride=stride, **kw, **o)
        print(stride, fmt, len(sub), {k: v for k, v in got.items() if k != "T"}, R.pose_error(got["T"], pose))
        assert got["colored"] == got["used"] > 0.8 * len(sub) and got["first_downweighted"] > 0
        _same_result(got, want, "stride %d %s" % (stride, fmt))
        _same_result(hv.RegisterFrameRobust(raw, None, init, pixel_stride=stride, linearization="gradient", huber=0.01, **kw),
                     hv.RegisterPointsRobust(sub, None, init, linearization="gradient", huber=0.01, **kw), "geometric, stride %d %s" % (stride, fmt))
        wants[fmt] = want
    if stride == 1:
        import torch
        dd, cc = torch.from_numpy(depth).to("cuda:0"), torch.from_numpy(np.ascontiguousarray(rgb)).to("cuda:0")
        _same_result(hv.RegisterFrameRobust(dd, cc, init, pixel_stride=1, **kw, **o), wants["f32"], "device images")
        got = hv.RegisterFrameRobust(np.zeros((h, w), F32), rgb, init, **o)                   # a frame without a valid pixel
        assert got["status"] == R.TOO_FEW_POINTS and got["used"] == 0 and got["downweighted"] == 0 and np.array_equal(_bits(got["T"]), _bits(init))


def _case_volume(oracle, what):
    key = "hv_scene" if what == "scene" else "hv_model"
    if key not in _cache:
        if what == "scene":
            sc = R.reg_scene(oracle)
            hv = _handler(R.REG_CAM, R.REG_RES)
        else:
            sc = B.model(oracle)
            hv = _handler(B.MODEL_CAM, B.MODEL_RES)
        hv.SetCubeMap(sc["keys"], sc["vox"])
        _cache[key] = hv
    return _cache[key]


@pytest.mark.parametrize("what,mode,iters,huber,outliers", [
    (12, B.METRIC, 10, 0.0, False), (20, B.METRIC, 10, 0.0, False), (30, B.METRIC, 10, 0.0, False), ("scene", B.METRIC, 10, 0.0, False),
    (12, B.NORMAL, 10, 0.0, False), (20, B.NORMAL, 10, 0.0, False), ("scene", B.NORMAL, 10, 0.0, False),
    (0, B.NORMAL, 20, 0.0, False), (0, B.METRIC, 20, 0.0, False),
    (20, B.METRIC, 30, 0.0, True), (20, B.METRIC, 30, 0.01, True)])
def test_06_convergence_cases_on_the_device(oracle, what, mode, iters, huber, outliers):
    """The cases of tests/test_volume_register_robust_cpu.py through the library: T is the restated loop's bit for bit (the device's sums differ
    from math.fsum's by at most (used - 1) 2^-53 relative, far below what moves a float32 component of the step), and so are the iteration count,
    the status and the counts; the bounds of the CPU tests hold for the device's own result."""
    ref, _t, _r = B.case(oracle, L.load(), what, mode, max_iterations=iters, huber=huber, outliers=outliers)
    _grid, cloud = B.case_inputs(oracle, what, outliers)
    hv = _case_volume(oracle, what)
    got = hv.RegisterPointsRobust(cloud, None, B.model_init(), max_iterations=iters, min_step=1e-5, max_distance=B.TRUNC, linearization=mode, huber=huber)
    t, r = R.pose_error(got["T"])
    print("device: %s mode %d: %d iterations, %s, last step %.2e, %.3f mm / %.5f deg, used %d, downweighted %d" % (
        what, mode, got["iterations"], got["status_name"], got["last_step"], t * 1e3, r, got["used"], got["downweighted"]))
    assert np.array_equal(_bits(got["T"]), _bits(ref["T"]))
    for k in ("iterations", "status", "used", "invalid", "no_gradient", "too_far", "first_used", "downweighted", "first_downweighted"):
        assert got[k] == ref[k], (k, got[k], ref[k])
    if what == 0:
        assert got["last_step"] > 0.05 if mode == B.NORMAL else got["last_step"] < 1e-3
    elif outliers:
        assert (got["downweighted"] > 0) == (huber > 0)
    elif mode == B.METRIC:
        assert got["status"] == R.CONVERGED and got["iterations"] <= 10 and t < 0.005 and r < 0.1
    else:
        assert got["status"] == R.MAX_ITERATIONS and got["iterations"] == 10


def test_07_the_volume_is_only_read(oracle):
    """GetCubeMap before and after is bit-equal; frames fused without an accessor in between are seen"""
    sc = K.color_scene(oracle)
    hv = _handler(K.COL_CAM, K.COL_RES)
    for f in sc["frames"]:
        hv.IntegrateImage(*f)
    q, y, init = sc["cloud"][:3000], sc["y"][:3000], sc["init"]
    o = dict(linearization="metric", huber=0.01, huber_color=0.01)
    got = hv.RegisterPointsRobust(q, y, init, max_iterations=4, min_step=0.0, color_scale=1.0, **o)   # (the frames are still queued when the call arrives)
    ref = _handler(K.COL_CAM, K.COL_RES)
    ref.SetCubeMap(sc["keys"], sc["vox"])
    _same_result(got, ref.RegisterPointsRobust(q, y, init, max_iterations=4, min_step=0.0, color_scale=1.0, **o), "queued frames are seen")
    k0, v0 = hv.GetCubeMap(sort=False)
    hv.RegisterPointsRobust(q, y, init, max_iterations=3, color_scale=1.0, **o)
    hv.RegisterPointsRobust(q, None, init, max_iterations=3, linearization="gradient")
    hv.RobustRegistrationSystem(q, y, init, B.TRUNC, 1.0, 0.0, rows=True, **o)
    fr = sc["frames"]
    hv.RegisterFrameRobust(fr[1][0], fr[1][1], D.perturbed(fr[1][2], 1), pixel_stride=2, max_iterations=3, **o)
    hv.RegisterFrameRobust(fr[1][0], None, D.perturbed(fr[1][2], 1), pixel_stride=2, max_iterations=3, **o)
    k1, v1 = hv.GetCubeMap(sort=False)
    assert np.array_equal(k0, k1) and np.array_equal(_bits(v0), _bits(v1))
    k2, v2 = hv.GetCubeMap()
    assert np.array_equal(k2, sc["keys"]) and np.array_equal(_bits(v2), _bits(sc["vox"]))


def test_08_class_surface(oracle, tmp_path):
    """CubeHandler::RobustRegistrationSystem / RegisterPointCloudRobust / RegisterRGBDRobust (host/one_piece) return what the C-ABI returns for the
    same volume and inputs"""
    sc = K.color_scene(oracle)
    exe = tmp_path / "register_robust_surface_check"
    host, lib = os.path.join(ROOT, "host", "one_piece"), os.path.join(ROOT, "onepiece_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-I", host, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "register_robust_surface_check.cpp"),
                           "-L", host, "-lone_piece_hip_host", "-L", lib, "-lonepiece_hip", "-Wl,-rpath," + host, "-Wl,-rpath," + lib, "-o", str(exe)])
    hv = _handler(K.COL_CAM, K.COL_RES)
    hv.SetCubeMap(sc["keys"], sc["vox"])
    hv.WriteToFile(tmp_path / "room.map")
    back = _handler(K.COL_CAM, K.COL_RES)
    back.ReadFromFile(tmp_path / "room.map")
    depth, rgb, pose = sc["frames"][4]
    hit, pts = S.hit_points(pose, K.COL_CAM, depth)
    q = np.ascontiguousarray(pts[:3000], F32)
    colors = np.ascontiguousarray((rgb.astype(F32) / F32(255.0))[hit][:3000])          # what LoadFromRGBD leaves in pcd.colors: stored channel order, byte / 255
    y = K.intensity(colors)
    start = D.perturbed(pose, 1)
    q.tofile(tmp_path / "points.bin")
    colors.tofile(tmp_path / "colors.bin")
    depth.tofile(tmp_path / "depth.bin")
    np.ascontiguousarray(rgb).tofile(tmp_path / "rgb.bin")
    (tmp_path / "pose.txt").write_text(" ".join("%.9g" % v for v in start.reshape(-1)))
    camt = K.COL_CAM
    run = subprocess.run([str(exe)] + [str(tmp_path / f) for f in ("room.map",)] + [repr(K.COL_RES)] + [str(tmp_path / f) for f in ("points.bin", "colors.bin", "depth.bin", "rgb.bin")] +
                         [repr(float(v)) for v in camt[:4]] + [str(camt[4]), str(camt[5]), str(tmp_path / "pose.txt")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = {l.split()[0]: l.split()[1:] for l in run.stdout.strip().splitlines() if l.split() and l.split()[0] in ("system", "points", "defaults", "bare", "rgbd", "depth")}
    init = np.eye(4, dtype=F32)
    init[:3, 3] = [0.01, -0.02, 0.005]
    h, hc = float(F32(0.005)), float(F32(0.01))
    sums, counts = back.RobustRegistrationSystem(q, y, init, 0.1, 0.5, 0.25, linearization="gradient", huber=h, huber_color=hc)
    row = lines["system"]
    assert [int(v) for v in row[:7]] == [counts[k] for k in B.COUNT_NAMES] and counts["colored"] > 1000 and counts["downweighted"] > 0
    assert _same64(np.array([float(v) for v in row[7:]]), sums)

    def same(row, want):
        assert [int(v) for v in row[:12]] == [want[k] for k in ("iterations", "status", "used", "invalid", "no_gradient", "too_far", "first_used", "colored", "first_colored") + ROBUST_KEYS]
        assert [float(v) for v in row[12:18]] == [want[k] for k in ("rmse", "first_rmse", "rmse_color", "first_rmse_color", "rmse_residual", "first_rmse_residual")]
        assert float(row[18]) == want["rmse"]
        assert np.array_equal(_bits(np.array([F32(v) for v in row[19:]], F32)), _bits(want["T"].reshape(-1)))
    kw = dict(max_iterations=4, max_distance=0.1, min_step=0.0, min_points=6, color_scale=0.5, max_color_residual=0.25, linearization="metric", huber=h, huber_color=hc)
    same(lines["points"], back.RegisterPointsRobust(q, y, init, **kw))
    same(lines["defaults"], back.RegisterPointsRobust(q, y, color_scale=1.0))
    same(lines["bare"], back.RegisterPointsRobust(q, None, init, **dict(kw, color_scale=0.0)))
    same(lines["rgbd"], back.RegisterFrameRobust(depth, rgb, start, pixel_stride=2, **kw))
    same(lines["depth"], back.RegisterFrameRobust(depth, None, start, pixel_stride=2, **kw))


DRIVER = ["--synthetic", "6", "5", "1", "--res", "0.04", "--perturb", "3", "--iters", "6"]


def test_09_driver_linearizations():
    """examples/cpp/ModelRegistration --linearization / --huber / --huber-color: without the flags the driver prints what it printed before they
    existed; with them one line per registered frame with its iteration count, status and last step, and the JSON line names the options."""
    exe = os.path.join(ROOT, "examples", "cpp", "ModelRegistration.bin")
    assert os.path.exists(exe), "examples/cpp/ModelRegistration.bin is not built (__graft_entry__.build())"
    out, text = {}, {}
    for what, extra in (("none", []), ("normal", ["--linearization", "normal"]), ("metric", ["--linearization", "metric"]), ("gradient", ["--linearization", "gradient", "--huber", "0.01"]),
                        ("color", ["--color", "on", "--linearization", "metric", "--huber", "0.01", "--huber-color", "0.02"])):
        run = subprocess.run([exe] + DRIVER + extra, capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
        text[what] = run.stdout.strip().splitlines()
        out[what] = json.loads(text[what][-1])
        print(what, text[what])
    old_keys = ["frames", "stride", "first", "res", "path", "registered", "iters", "iterations", "points", "used_last", "error_before", "error_after", "rmse", "ms"]
    assert not [l for l in text["none"] if l.startswith("frame ")] and list(out["none"].keys()) == old_keys
    strip = lambda d, drop=(): {k: v for k, v in d.items() if k != "ms" and k not in drop}
    new = ("linearization", "huber", "huber_color", "downweighted_last", "rmse_residual", "rmse_color", "colored_last", "color_scale")
    # NORMAL without thresholds through the robust entry is the registration the driver ran before
    assert strip(out["normal"], new) == strip(out["none"]) and out["normal"]["linearization"] == "normal"
    for what in ("normal", "metric", "gradient", "color"):
        frames = [l for l in text[what][:-1] if l.startswith("frame ")]
        assert len(frames) == out[what]["registered"] == 2 and all("iterations" in l and "status" in l and "last step" in l for l in frames), what
    assert out["metric"]["linearization"] == "metric" and out["metric"]["huber"] == 0 and out["metric"]["downweighted_last"] == 0
    assert out["gradient"]["huber"] == 0.01 and out["color"]["huber_color"] == 0.02 and out["color"]["colored_last"] > 0
    assert out["metric"]["error_before"] == out["none"]["error_before"]
    bad = subprocess.run([exe] + DRIVER + ["--linearization", "cubic"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "usage" in bad.stdout
    bad = subprocess.run([exe] + DRIVER + ["--path", "sample", "--linearization", "metric"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "usage" in bad.stdout
