"""op_volume_register_batch_* on the device (csrc/volume_register.hip, k_volume_register_batch) against the SINGLE entries of the same library, which
tests/test_volume_register_robust_gpu.py and its neighbours pin to the numpy restatement: every cloud's sums as 64-bit patterns and counts exactly,
every field of every frame's result bit for bit, whatever else the batch holds and in whatever order; the stats against the restated scheduler
(tests/volume_register_batch_common.py) fed with the evaluations the restated loop's trace gives.

Volumes come from the oracle or from hand-made blocks, never from the code under test: the sliding scene of the colour tests (eight 64 x 48 frames,
2 cm voxels) and the seven hand-made blocks of 1/32 m voxels holding s = 2 (z - Z0) and colour 0.5 + x."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import deintegrate_common as D
import volume_register_batch_common as BT
import volume_register_color_common as K
import volume_register_common as R
import volume_register_robust_common as B
from onepiece_amd import _lib as L
from onepiece_amd import integration as I

pytestmark = pytest.mark.gpu

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the wave and workgroup edges, a cloud with no workgroup, and one cloud past the 1024-row cap: a second trip for 257 lanes, ragged at its end
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 4097, 262144 + 257)
SCALE, LIMIT, GATE, HUBER = 0.6, 0.05, 0.25, 1 / 64
CONFIGS = [(0.0, False), (0.0, True), (SCALE, False), (SCALE, True)]   # (color_scale, with both Huber thresholds or without), as the robust tests
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


RESULT_INTS = ("iterations", "status", "used", "invalid", "no_gradient", "too_far", "first_used", "colored", "first_colored", "downweighted", "color_downweighted",
               "first_downweighted")
RESULT_DOUBLES = ("rmse", "first_rmse", "last_step", "rmse_color", "first_rmse_color", "rmse_residual", "first_rmse_residual")


def _same_result(got, want, what):
    """every field of op_volume_register_robust_result"""
    assert set(got) == set(want) == set(RESULT_INTS) | set(RESULT_DOUBLES) | {"T", "status_name"}, what
    assert np.array_equal(_bits(got["T"]), _bits(want["T"])), what
    for k in RESULT_INTS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in RESULT_DOUBLES:
        assert np.float64(got[k]).view(np.uint64) == np.float64(want[k]).view(np.uint64), (what, k, got[k], want[k])


# ---- one evaluation -----------------------------------------------------------------------------------------------------------------------------
def _hand():
    """-> dict(hv, q, y, off, starts, T): the hand-made blocks and ten clouds of SIZES points cut from one hand cloud, each with a pose of its own"""
    if "hand" not in _cache:
        hv = _handler(D.CAM_37, R.HAND_RES)
        hv.AddCubes(R.HAND_KEYS, B.steep_blocks(color=True))
        total = sum(SIZES)
        q = R.hand_cloud(n=total - len(R.HAND_POINTS))
        idx = np.arange(total)
        with np.errstate(all="ignore"):
            c = F32(0.5) + q[:, 0]
            y = K.intensity(np.stack([c, c, c], axis=1))
        y[idx % 2 == 0] += F32(0.03125)                               # coloured and down-weighted
        y[idx % 5 == 0] += F32(0.0625)                                # gated by LIMIT
        y[idx % 16 == 1] = np.nan
        y[idx % 32 == 7] = -np.inf
        off = ((idx % 5) - 2).astype(F32) / F32(64.0)
        off[3::11] = np.nan
        off[5::13] = np.inf
        off[6::17] = -np.inf
        starts = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.uint64)
        T = np.tile(np.eye(4, dtype=F32), (len(SIZES), 1, 1))
        for c in range(len(SIZES)):
            T[c, :3, 3] = [(c % 3) / 128, 0.0, -(c % 4) / 128]
        _cache["hand"] = dict(hv=hv, q=q, y=np.ascontiguousarray(y), off=off, starts=starts, T=T)
    return _cache["hand"]


@pytest.mark.parametrize("mode", [B.NORMAL, B.GRADIENT, B.METRIC])
def test_01_one_evaluation_is_the_single_system(mode):
    """ten clouds in one launch, each at its own T: sums as 64-bit patterns and counts exactly against op_volume_register_offset_system on each cloud
    alone; geometric and coloured, with and without Huber weights (all-zero options under NORMAL: the rows of 32 and 35), and with target values
    that hold NaN and +-inf"""
    h = _hand()
    hv, q, y, starts, T = h["hv"], h["q"], h["y"], h["starts"], h["T"]
    for cs, weights, off in [c + (None,) for c in CONFIGS] + [(0.0, False, h["off"]), (SCALE, True, h["off"])]:
        o = dict(linearization=mode, huber=HUBER if weights else 0.0, huber_color=HUBER if weights else 0.0)
        sums, counts = hv.BatchRegistrationSystem(q, starts, off, y, T, GATE, cs, LIMIT, **o)
        assert sums.shape == (len(SIZES), 31) and len(counts) == len(SIZES)
        for c, n in enumerate(SIZES):
            a, b = int(starts[c]), int(starts[c + 1])
            tag = "mode %d color_scale %g weights %d offsets %d cloud %d n=%d" % (mode, cs, weights, off is not None, c, n)
            want, wc = hv.OffsetRegistrationSystem(q[a:b], None if off is None else off[a:b], y[a:b], T[c], GATE, cs, LIMIT, **o)
            assert counts[c] == wc, (tag, counts[c], wc)
            assert _same64(sums[c], want), (tag, sums[c], want)
            assert sum(wc[k] for k in R.COUNT_NAMES) == n, tag
            if n >= 4097:                                             # the comparison is not between zeros
                assert min(wc[k] for k in R.COUNT_NAMES) > 0 and want[27] > 0 and want[11] > 0, tag
                assert (wc["colored"] > 0) == (cs > 0) and (wc["downweighted"] > 0) == weights, tag
        again, c2 = hv.BatchRegistrationSystem(q, starts, off, y, T, GATE, cs, LIMIT, **o)
        assert _same64(again, sums) and c2 == counts
    # a batch that does not begin at point 0, with an empty cloud in the middle: cloud c is whatever [starts[c], starts[c + 1]) says
    st = np.array([5, 5 + 257, 5 + 257, 5 + 257 + 64], np.uint64)
    o = dict(linearization=mode, huber=HUBER, huber_color=HUBER)
    sums, counts = hv.BatchRegistrationSystem(q[:400], st, None, y[:400], T[:3], GATE, SCALE, LIMIT, **o)
    for c in range(3):
        a, b = int(st[c]), int(st[c + 1])
        want, wc = hv.OffsetRegistrationSystem(q[a:b], None, y[a:b], T[c], GATE, SCALE, LIMIT, **o)
        assert _same64(sums[c], want) and counts[c] == wc, c


# ---- the loops ----------------------------------------------------------------------------------------------------------------------------------
O = dict(linearization="metric", huber=0.01, huber_color=0.01)
KW = dict(max_iterations=3, min_step=1e-3)                            # three iterations: the frames that start centimetres off end on MAX_ITERATIONS


def _slide(oracle):
    """-> dict(hv, depths [10,h,w], rgbs [10,h,w,3], inits [10,4,4], poses): the eight frames of the sliding scene with planted starts, so that the
    frames stop in different rounds, and two frames without a usable point"""
    if "slide" not in _cache:
        sc = K.color_scene(oracle)
        hv = _handler(K.COL_CAM, K.COL_RES)
        hv.SetCubeMap(sc["keys"], sc["vox"])
        fr = sc["frames"]
        shift = lambda pose, d: (np.asarray(pose, np.float64) @ np.array([[1, 0, 0, d], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])).astype(F32)
        away = np.diag([-1.0, 1.0, -1.0, 1.0])                        # half a turn about y and fifty metres aside: the camera looks away from the model
        away[0, 3] = 50.0
        depths = [f[0] for f in fr] + [np.zeros_like(fr[0][0]), fr[5][0]]
        rgbs = [f[1] for f in fr] + [fr[0][1], fr[5][1]]
        inits = [np.asarray(fr[0][2], F32), shift(fr[1][2], 0.01), shift(fr[2][2], 0.02), shift(fr[3][2], 0.04)] + [D.perturbed(fr[k][2], k) for k in (4, 5, 6, 7)] + \
                [np.asarray(fr[0][2], F32), (np.asarray(fr[5][2], np.float64) @ away).astype(F32)]
        _cache["slide"] = dict(hv=hv, depths=np.ascontiguousarray(np.stack(depths), F32), rgbs=np.ascontiguousarray(np.stack(rgbs), np.uint8),
                               inits=np.ascontiguousarray(np.stack(inits), F32), poses=[f[2] for f in fr])
    return _cache["slide"]


def _raw(depths, fmt):
    return depths if fmt == "f32" else np.round(depths * 1000.0).astype(np.uint16)


def _kept(raw, stride):
    return [int((d[::stride, ::stride] > 0).sum()) for d in raw]


def _singles(s, raw, color, stride, frames=None):
    key = ("singles", raw.dtype.str, color, stride)
    if key not in _cache:
        _cache[key] = [s["hv"].RegisterFrameRobust(raw[f], s["rgbs"][f] if color else None, s["inits"][f], pixel_stride=stride, **KW, **O) for f in range(len(raw))]
    return _cache[key] if frames is None else [_cache[key][f] for f in frames]


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("fmt", ["f32", "u16"])
@pytest.mark.parametrize("color", [True, False])
def test_02_every_frame_follows_its_own_loop(oracle, stride, fmt, color):
    s = _slide(oracle)
    hv, raw = s["hv"], _raw(s["depths"], fmt)
    want = _singles(s, raw, color, stride)
    got, stats = hv.RegisterFramesRobust(raw, s["rgbs"] if color else None, s["inits"], pixel_stride=stride, **KW, **O)
    evaluations = [w["iterations"] + 1 for w in want]
    print(stride, fmt, color, [(w["status_name"], w["iterations"], w["used"]) for w in want], stats)
    for f, (g, w) in enumerate(zip(got, want)):
        _same_result(g, w, "frame %d stride %d %s colour %d" % (f, stride, fmt, color))
    # the planted cases: the two frames without a usable point stop on their first evaluation, the others iterate, and not all equally long
    assert [want[f]["status"] for f in (8, 9)] == [R.TOO_FEW_POINTS] * 2 and want[8]["invalid"] == 0 and want[9]["invalid"] == _kept(raw, stride)[9] > 0
    assert all(np.array_equal(_bits(got[f]["T"]), _bits(s["inits"][f])) for f in (8, 9))
    assert all(w["used"] > 50 and w["iterations"] >= 1 for w in want[:8]) and any(w["status"] == R.MAX_ITERATIONS for w in want[:8])
    assert len(set(evaluations)) >= 2
    assert stats == BT.stats_of(evaluations, _kept(raw, stride)), (stats, evaluations)
    assert stats["evaluations"] < stats["rounds"] * len(want)         # a stopped frame costs nothing more


def _back_projected(s, stride):
    """the kept pixels of every frame as the depth entries form them (op_points_from_depth on the whole image, then the stride's lattice), with the
    restated intensities -> (points [n,3], y [n], starts)"""
    key = ("points", stride)
    if key not in _cache:
        lib, hv = L.load(), s["hv"]
        w, h = K.COL_CAM[4], K.COL_CAM[5]
        pts, ys, starts = [], [], [0]
        for depth, rgb in zip(s["depths"], s["rgbs"]):
            buf, n = np.zeros((w * h, 3), F32), C.c_size_t(0)
            L.check(lib.op_points_from_depth(C.byref(hv.camera), C.c_void_p(depth.ctypes.data), L.OP_DEPTH_F32, L.OP_MEM_HOST, 0, C.c_void_p(buf.ctypes.data), C.byref(n)))
            mask = depth > 0
            index = np.cumsum(mask.reshape(-1)) - 1
            keep = np.zeros((h, w), bool)
            keep[::stride, ::stride] = True
            sel = (keep & mask).reshape(-1)
            pts.append(buf[index[sel]])
            ys.append(K.intensity_of_bytes(rgb).reshape(-1)[sel])
            starts.append(starts[-1] + int(sel.sum()))
        _cache[key] = (np.ascontiguousarray(np.concatenate(pts), F32), np.ascontiguousarray(np.concatenate(ys), F32), np.array(starts, np.uint64))
    return _cache[key]


def test_03_stats_against_the_restated_loop(oracle):
    """the evaluations per frame from the restated loop's trace (len(trace) + 1: tests/volume_register_batch_common.py) around the single one-pass
    entry, on the frames' back-projected points; the restated scheduler turns them into the stats the batch must report"""
    s = _slide(oracle)
    hv, stride = s["hv"], 3
    q, y, starts = _back_projected(s, stride)
    evaluations = []
    for f in range(len(s["depths"])):
        a, b = int(starts[f]), int(starts[f + 1])
        trace = []
        res = B.loop(L.load(), lambda T: hv.RobustRegistrationSystem(q[a:b], y[a:b], T, B.TRUNC, 1.0, 0.0, **O), s["inits"][f], KW["max_iterations"], min_step=KW["min_step"],
                     trace=trace)
        evaluations.append(len(trace) + 1)
        assert res["iterations"] == len(trace)
    got, stats = hv.RegisterFramesRobust(s["depths"], s["rgbs"], s["inits"], pixel_stride=stride, **KW, **O)
    print(evaluations, stats)
    assert stats == BT.stats_of(evaluations, np.diff(starts.astype(np.int64)).tolist())
    assert [g["iterations"] + 1 for g in got] == evaluations
    assert BT.rounds_of(evaluations)[0] == list(range(len(evaluations))) and len(BT.rounds_of(evaluations)[-1]) < len(evaluations)
    # max_iterations 0: one evaluation each, at the start
    got, stats = hv.RegisterFramesRobust(s["depths"], s["rgbs"], s["inits"], pixel_stride=stride, max_iterations=0, **O)
    assert stats["rounds"] == 1 and stats["evaluations"] == len(got) and stats["launches"] == 2
    for f, g in enumerate(got):
        _same_result(g, hv.RegisterFrameRobust(s["depths"][f], s["rgbs"][f], s["inits"][f], pixel_stride=stride, max_iterations=0, **O), "max_iterations 0, frame %d" % f)


def test_04_order_and_company_do_not_matter(oracle):
    s = _slide(oracle)
    hv, stride = s["hv"], 3
    want = _singles(s, s["depths"], True, stride)
    n = len(want)
    for what, frames in (("reversed", list(range(n))[::-1]), ("without frame 2", [f for f in range(n) if f != 2]), ("frame 6 alone", [6]), ("frame 8 alone: no point", [8])):
        got, stats = hv.RegisterFramesRobust(s["depths"][frames], s["rgbs"][frames], s["inits"][frames], pixel_stride=stride, **KW, **O)
        for g, f in zip(got, frames):
            _same_result(g, want[f], "%s, frame %d" % (what, f))
        assert stats == BT.stats_of([want[f]["iterations"] + 1 for f in frames], [_kept(s["depths"], stride)[f] for f in frames]), what
    assert stats["launches"] == 0 and stats["points"] == 0            # (the last batch: nothing to launch)
    # an empty volume: every frame ends on its first evaluation, T = init
    empty = _handler(K.COL_CAM, K.COL_RES)
    got, stats = empty.RegisterFramesRobust(s["depths"], s["rgbs"], s["inits"], pixel_stride=stride, **KW, **O)
    assert all(g["status"] == R.TOO_FEW_POINTS and g["used"] == 0 and np.array_equal(_bits(g["T"]), _bits(s["inits"][f])) for f, g in enumerate(got))
    assert stats["rounds"] == 1 and stats["evaluations"] == n


@pytest.mark.parametrize("stride", [1, 3])
def test_05_frames_entry_is_the_points_entry(oracle, stride):
    """the frames entry against the points entry on the back-projected points; the points entry against the single points entry, with offsets too"""
    s = _slide(oracle)
    hv = s["hv"]
    q, y, starts = _back_projected(s, stride)
    frames = _singles(s, s["depths"], True, stride)
    got, stats = hv.RegisterPointsBatch(q, starts, None, y, s["inits"], color_scale=1.0, **KW, **O)
    for f, (g, w) in enumerate(zip(got, frames)):
        _same_result(g, w, "points batch against the frame entry, stride %d frame %d" % (stride, f))
    assert stats == BT.stats_of([w["iterations"] + 1 for w in frames], np.diff(starts.astype(np.int64)).tolist())
    geo, _st = hv.RegisterPointsBatch(q, starts, None, None, s["inits"], linearization="gradient", huber=0.01, **KW)
    fgeo, _st = hv.RegisterFramesRobust(s["depths"], None, s["inits"], pixel_stride=stride, linearization="gradient", huber=0.01, **KW)
    for f, (g, w) in enumerate(zip(geo, fgeo)):
        _same_result(g, w, "geometric, stride %d frame %d" % (stride, f))
    if stride == 3:                                                   # target values, and all-zero options (the colour entry's rows of 35)
        off = ((np.arange(len(q)) % 7) - 3).astype(F32) / F32(2000.0)
        off[4::19] = np.nan
        for o, oo in ((O, off), (dict(linearization="normal", huber=0.0, huber_color=0.0), None)):
            got, _st = hv.RegisterPointsBatch(q, starts, oo, y, s["inits"], color_scale=0.5, max_color_residual=0.1, **KW, **o)
            for f in range(len(got)):
                a, b = int(starts[f]), int(starts[f + 1])
                _same_result(got[f], hv.RegisterPointsOffset(q[a:b], None if oo is None else oo[a:b], y[a:b], s["inits"][f], color_scale=0.5, max_color_residual=0.1, **KW, **o),
                             "offsets %d, frame %d" % (oo is not None, f))


def test_06_device_memory_and_repeats_give_the_same_bits(oracle):
    import torch
    s = _slide(oracle)
    hv, stride = s["hv"], 3
    want = _singles(s, s["depths"], True, stride)
    dd, cc = torch.from_numpy(s["depths"]).to("cuda:0"), torch.from_numpy(s["rgbs"]).to("cuda:0")
    for turn in range(2):
        got, stats = hv.RegisterFramesRobust(dd, cc, s["inits"], pixel_stride=stride, **KW, **O)
        for f, (g, w) in enumerate(zip(got, want)):
            _same_result(g, w, "device images, call %d, frame %d" % (turn, f))
    raw = torch.from_numpy(_raw(s["depths"], "u16").view(np.int16)).to("cuda:0")
    got, _st = hv.RegisterFramesRobust(raw, None, s["inits"], pixel_stride=1, **KW, **O)
    for f, (g, w) in enumerate(zip(got, _singles(s, _raw(s["depths"], "u16"), False, 1))):
        _same_result(g, w, "device u16 images, frame %d" % f)
    # the points entry with every buffer on the device, 4 bytes into its allocation
    q, y, starts = _back_projected(s, stride)
    n, nf = len(q), len(want)
    pts = torch.full((3 * n + 2,), 7.0, dtype=torch.float32, device="cuda:0")
    pts[1:1 + 3 * n] = torch.from_numpy(q.reshape(-1)).to("cuda:0")
    yy = torch.full((n + 2,), 7.0, dtype=torch.float32, device="cuda:0")
    yy[1:1 + n] = torch.from_numpy(y).to("cuda:0")
    torch.cuda.synchronize()
    p = hv._register_color_params(KW["max_iterations"], None, KW["min_step"], None, 1.0, None)
    opt, res, st = hv._register_options(**O), (L.RegisterRobustResult * nf)(), L.RegisterBatchStats()
    T0 = np.ascontiguousarray(s["inits"], F32).reshape(nf, 16)
    L.check(L.load().op_volume_register_batch_points(hv._h, C.c_void_p(pts[1:].data_ptr()), None, C.c_void_p(yy[1:].data_ptr()), starts.ctypes.data_as(L._u64p), nf, L.OP_MEM_DEVICE,
                                                     T0.ctypes.data_as(L._fp), C.byref(p), C.byref(opt), res, C.byref(st)))
    for f in range(nf):
        _same_result(hv._register_robust_result(res[f]), want[f], "device points, frame %d" % f)
    assert float(pts[0]) == 7.0 and float(pts[-1]) == 7.0 and float(yy[0]) == 7.0 and float(yy[-1]) == 7.0
    # the volume is only read
    k0, v0 = hv.GetCubeMap(sort=False)
    hv.RegisterFramesRobust(s["depths"], s["rgbs"], s["inits"], pixel_stride=2, **KW, **O)
    k1, v1 = hv.GetCubeMap(sort=False)
    assert np.array_equal(k0, k1) and np.array_equal(_bits(v0), _bits(v1))


def test_07_class_surface(oracle, tmp_path):
    """CubeHandler::RegisterFramesRobust / RegisterPointCloudsRobust (host/one_piece): the check compares every element with the single calls of the
    class byte for byte itself; its printed poses are the C-ABI's"""
    s = _slide(oracle)
    hv = s["hv"]
    exe = tmp_path / "register_batch_surface_check"
    host, lib = os.path.join(ROOT, "host", "one_piece"), os.path.join(ROOT, "onepiece_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-I", host, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "register_batch_surface_check.cpp"),
                           "-L", host, "-lone_piece_hip_host", "-L", lib, "-lonepiece_hip", "-Wl,-rpath," + host, "-Wl,-rpath," + lib, "-o", str(exe)])
    hv.WriteToFile(tmp_path / "room.map")
    n = len(s["depths"])
    s["depths"].tofile(tmp_path / "depths.bin")
    s["rgbs"].tofile(tmp_path / "rgbs.bin")
    (tmp_path / "poses.txt").write_text("\n".join(" ".join("%.9g" % v for v in T.reshape(-1)) for T in s["inits"]))
    camt = K.COL_CAM
    run = subprocess.run([str(exe), str(tmp_path / "room.map"), repr(K.COL_RES), str(tmp_path / "depths.bin"), str(tmp_path / "rgbs.bin")] + [repr(float(v)) for v in camt[:4]] +
                         [str(camt[4]), str(camt[5]), str(tmp_path / "poses.txt"), str(n)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    rows = [l.split() for l in run.stdout.strip().splitlines()]
    kw = dict(max_iterations=3, max_distance=0.1, min_step=float(F32(1e-3)), min_points=6, color_scale=0.5, max_color_residual=0.25, linearization="metric", huber=float(F32(0.01)),
              huber_color=float(F32(0.01)))
    for what, rgbs in (("rgbd", s["rgbs"]), ("depth", None)):
        want, stats = hv.RegisterFramesRobust(s["depths"], rgbs, s["inits"], pixel_stride=2, **kw)
        got = [r for r in rows if r[0] == what]
        assert len(got) == n
        for f, (r, w) in enumerate(zip(got, want)):
            assert [int(v) for v in r[1:6]] == [f, w["iterations"], w["status"], w["used"], w["downweighted"]], (what, f)
            assert [float(v) for v in r[6:9]] == [w["rmse"], w["rmse_residual"], w["rmse"]], (what, f)
            assert np.array_equal(_bits(np.array([F32(v) for v in r[9:]], F32)), _bits(w["T"].reshape(-1))), (what, f)
        line = [r for r in rows if r[0] == "stats" and int(r[1]) == (rgbs is not None)][0]
        assert [int(v) for v in line[2:]] == [stats[k] for k in ("rounds", "launches", "evaluations", "points")]
    assert len([r for r in rows if r[0] == "cloud"]) == n


REFINE = ["--synthetic", "6", "5", "1", "--res", "0.04", "--perturb", "3", "--path", "refine", "--stride", "8", "--iters", "6"]


def test_08_pose_correction_refines_on_the_device(oracle, tmp_path):
    """examples/cpp/PoseCorrection --path refine: the single and the batch mode write byte-identical pose files; the frames whose refined pose is nearer
    the truth than its start are exactly those for which the numpy restatement of the same flow says so (the room of onepiece_amd.synthetic fused
    by the oracle at the drifted poses, the restated METRIC loop on every eighth pixel); no threshold is written down"""
    from onepiece_amd import synthetic as SY
    import volume_sample_common as S
    exe = os.path.join(ROOT, "examples", "cpp", "PoseCorrection.bin")
    assert os.path.exists(exe), "examples/cpp/PoseCorrection.bin is not built (__graft_entry__.build())"
    out = {}
    for mode in ("single", "batch"):
        run = subprocess.run([exe] + REFINE + ["--refine", mode, "--dump", str(tmp_path / (mode + ".txt"))], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
        out[mode] = json.loads(run.stdout.strip().splitlines()[-1])
        print(mode, out[mode]["refine"], out[mode]["weight_mismatches"], out[mode]["max_abs_sdf_diff"])
    assert (tmp_path / "single.txt").read_bytes() == (tmp_path / "batch.txt").read_bytes()
    a, b = out["single"]["refine"], out["batch"]["refine"]
    assert a["error_after_mm_deg"] == b["error_after_mm_deg"] and a["error_before_mm_deg"] == b["error_before_mm_deg"]
    assert b["rounds"] >= 1 and b["evaluations"] <= 3 * b["rounds"] and b["launches"] == 2 * b["rounds"] and a["rounds"] == 0
    # the same flow restated on the CPU
    n, stride, k_moved, px = 6, 5, 3, 8
    camt = (SY.FX, SY.FY, SY.CX, SY.CY, SY.W, SY.H, 1000.0)
    moved = [(2 * k + 1) * n // (2 * k_moved) for k in range(k_moved)]
    vol = oracle.Volume(oracle.make_camera(*camt), voxel_res=0.04)
    frames = []
    for k in range(n):
        pose = SY.room_pose(k * stride)                              # SEED 1: the orbit starts at step 0
        depth, rgb = SY.room_render(pose)
        at = D.perturbed(pose, k) if k in moved else pose
        vol.integrate(depth, rgb, at)
        frames.append((depth, pose, at))
    keys, vox = vol.export()
    grid = S.Grid(keys, vox, 0.04)
    poses = {int(l.split()[0]): np.array([F32(v) for v in l.split()[1:]], F32).reshape(4, 4) for l in (tmp_path / "batch.txt").read_text().strip().splitlines()}
    assert sorted(poses) == moved
    nearer_device, nearer_restated = [], []
    for k in moved:
        depth, pose, at = frames[k]
        v, u = np.meshgrid(np.arange(0, SY.H, px), np.arange(0, SY.W, px), indexing="ij")
        z = depth[v, u].astype(F32)
        pts = np.stack([(u.astype(F32) - F32(SY.CX)) * z / F32(SY.FX), (v.astype(F32) - F32(SY.CY)) * z / F32(SY.FY), z], axis=-1).reshape(-1, 3)[z.reshape(-1) > 0]
        res = B.loop(L.load(), lambda T: B.system(grid, pts, None, T, 0.1, mode=B.METRIC), at, 6, min_step=1e-5)
        before = R.pose_error(at, pose)[0]
        print(k, "start %.2f mm, restated %.2f mm, device %.2f mm" % (before * 1e3, R.pose_error(res["T"], pose)[0] * 1e3, R.pose_error(poses[k], pose)[0] * 1e3))
        if R.pose_error(res["T"], pose)[0] < before:
            nearer_restated.append(k)
        if R.pose_error(poses[k], pose)[0] < before:
            nearer_device.append(k)
    assert nearer_device == nearer_restated
