"""op_volume_register_* on the device (csrc/volume_register.hip) against the numpy restatement of its definition (tests/volume_register_common.py,
built from tests/volume_sample_common.py, which tests/test_volume_sample_cpu.py pins to the oracle) over volumes that come from the oracle or from
hand-made blocks -- never from the code under test: every row bit for bit, the counts exactly, the 28 sums to the rounding of their additions; the
loop against the same loop made by hand from the one-pass entry; the pose against the truth.

Volumes: the convergence scene (the room through eight 64 x 48 frames 25 room frames apart, 2 cm voxels), the room at 37 x 29 into 4 cm voxels
(6 frames), seven hand-made blocks of 1/32 m voxels.  Batches of 1, 63, 64, 65, 255, 256, 257 and 4097 points (the wave and workgroup edges; 4097
is 17 workgroups, the last one a single lane)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import deintegrate_common as D
import volume_register_common as R
import volume_sample_common as S
from onepiece_amd import _lib as L
from onepiece_amd import integration as I

pytestmark = pytest.mark.gpu

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 63, 64, 65, 255, 256, 257, 4097)
MARGIN = 1e-3                                                         # test_04's relative margin on the rmse (its docstring says where it comes from)
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _handler(camt, res, trunc=R.TRUNC, max_blocks=1 << 13):
    hcam = I.PinholeCamera()
    hcam.fx, hcam.fy, hcam.cx, hcam.cy, hcam.width, hcam.height, hcam.depth_scale = camt
    hv = I.CubeHandler(hcam, device=0, max_blocks=max_blocks)
    hv.SetVoxelResolution(res)
    hv.SetTruncation(trunc)
    return hv


def _far(T):
    out = np.array(T, F32).reshape(4, 4).copy()
    out[0, 3] += F32(100.0)                                           # every point 100 m away: no block there
    return out


def _with_specials(pts, keys, res, n=4097, seed=9):
    """n points: `pts` cycled, with NaN, +-1e9 and points of unobserved space (a jittered voxel centre next to the held blocks) planted among them"""
    rng = np.random.default_rng(seed)
    q = np.ascontiguousarray(pts[rng.permutation(len(pts))[np.arange(n) % len(pts)]], F32).copy()
    mix = S.query_mix(keys, res, n=n, seed=seed)                      # +-1.5 voxels around held voxels: valid, unobserved and edge cases
    q[5::7] = mix[5::7]
    for k in range(1, n, 61):
        q[k] = [(np.nan, 0.1, 0.1), (1e9, 0.1, 0.1), (0.1, -1e9, 0.1), (0.1, 0.1, 1e9)][(k // 61) % 4]
    return q


def _scene(oracle, name):
    """-> dict(camt, res, frames, keys, vox, grid, q [4097,3], poses {what: T})"""
    if name in _cache:
        return _cache[name]
    if name == "reg64":
        sc = R.reg_scene(oracle)
        out = dict(camt=R.REG_CAM, res=R.REG_RES, frames=sc["frames"], keys=sc["keys"], vox=sc["vox"], grid=sc["grid"])
        out["q"] = _with_specials(sc["cloud"], sc["keys"], R.REG_RES)
        truth = np.eye(4, dtype=F32)
    elif name == "cam37":
        camt, res = D.CAM_37, 0.04
        fr = D.frames(camt, 6)
        vol = oracle.Volume(oracle.make_camera(*camt), voxel_res=res, trunc=R.TRUNC)
        for f in fr:
            vol.integrate(*f)
        keys, vox = vol.export()
        cloud = np.concatenate([S.hit_points(f[2], camt, f[0])[1] for f in fr])
        out = dict(camt=camt, res=res, frames=fr, keys=keys, vox=vox, grid=S.Grid(keys, vox, res), q=_with_specials(cloud, keys, res))
        truth = np.eye(4, dtype=F32)
    else:
        vox = R.hand_blocks()
        out = dict(camt=D.CAM_37, res=R.HAND_RES, frames=None, keys=R.HAND_KEYS, vox=vox, grid=S.Grid(R.HAND_KEYS, vox, R.HAND_RES))
        out["q"] = R.hand_cloud(n=4097 - len(R.HAND_POINTS))
        truth = np.eye(4, dtype=F32)
    out["poses"] = {"truth": truth, "perturbed": D.perturbed(truth, 1), "far": _far(truth)}
    out["want"] = {}
    out["gate"] = 0.1 if name == "hand" else 0.05                    # (below the truncation on the fused volumes: they store no |sdf| beyond it)
    _cache[name] = out
    return out


def _want(sc, what):
    """the restatement's rows and reasons of all 4097 points at pose `what` (computed once)"""
    if what not in sc["want"]:
        sc["want"][what] = R.rows_of(sc["grid"], sc["q"], sc["poses"][what], sc["gate"])
    return sc["want"][what]


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


def _check_system(got_sums, got_counts, rows, reason, what):
    sums, mags, counts = R.fold(rows, reason)
    assert got_counts == counts, (what, got_counts, counts)
    used = counts["used"]
    if used == 0:
        assert not np.asarray(got_sums).any(), what                   # exactly zero
        return
    bound = max(used - 1, 1) * 2.0 ** -53 * mags                      # every term is exact in double: only the order of the additions differs
    err = np.abs(np.asarray(got_sums) - sums)
    assert (err <= bound).all(), (what, int(np.argmax(err - bound)), err.max())


def _device_system(hv, q, T, max_distance, rows):
    """op_volume_register_system with every buffer on the device, 4 bytes into its allocation and fenced by sentinels"""
    import torch
    n = len(q)
    dev = torch.device("cuda:0")
    pts = torch.full((3 * n + 2,), 7.0, dtype=torch.float32, device=dev)
    pts[1:1 + 3 * n] = torch.from_numpy(np.ascontiguousarray(q).reshape(-1)).to(dev)
    out = torch.full((8 * n + 2,), 12345.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    sums, counts = np.zeros(28), np.zeros(4, np.uint64)
    Tm = np.ascontiguousarray(T, F32).reshape(16)
    L.check(L.load().op_volume_register_system(hv._h, C.c_void_p(pts[1:].data_ptr()), n, L.OP_MEM_DEVICE, Tm.ctypes.data_as(L._fp), float(max_distance),
                                               sums.ctypes.data_as(C.POINTER(C.c_double)), counts.ctypes.data_as(L._u64p),
                                               C.c_void_p(out[1:].data_ptr()) if rows else None))
    host = out.cpu().numpy()
    assert host[0] == 12345.0 and host[-1] == 12345.0, "a write outside the n rows"
    if not rows:
        assert (host == 12345.0).all()
    return sums, dict(zip(R.COUNT_NAMES, (int(c) for c in counts))), host[1:-1].reshape(n, 8)


@pytest.mark.parametrize("source", ["fused", "uploaded"])
@pytest.mark.parametrize("name", ["reg64", "cam37", "hand"])
def test_01_system_against_the_restatement(oracle, name, source):
    sc = _scene(oracle, name)
    hv = _volume(sc, source)
    for what, T in sc["poses"].items():
        rows, reason = _want(sc, what)
        seen = {k: int((reason == k).sum()) for k in range(4)}
        print(name, source, what, seen)
        if what == "far":
            assert seen[1] == 4097
        elif name != "hand" or what == "truth":
            assert min(seen.values()) > 0, "the batch holds every class"
        for n in SIZES:
            tag = "%s %s %s n=%d" % (name, source, what, n)
            sums, counts, got = hv.RegistrationSystem(sc["q"][:n], T, sc["gate"], rows=True)
            bad = (_bits(got) != _bits(rows[:n])).any(axis=1)
            assert not bad.any(), "%s: %d rows differ" % (tag, int(bad.sum()))
            _check_system(sums, counts, rows[:n], reason[:n], tag)
            plain, c2 = hv.RegistrationSystem(sc["q"][:n], T, sc["gate"])          # rows = NULL: the same bits
            assert np.array_equal(plain.view(np.uint64), sums.view(np.uint64)) and c2 == counts, tag
            if n in (65, 4097):
                dsums, dcounts, drows = _device_system(hv, sc["q"][:n], T, sc["gate"], rows=True)
                assert np.array_equal(_bits(drows), _bits(got)) and dcounts == counts and np.array_equal(dsums.view(np.uint64), sums.view(np.uint64)), tag
                dsums, dcounts, _r = _device_system(hv, sc["q"][:n], T, sc["gate"], rows=False)
                assert dcounts == counts and np.array_equal(dsums.view(np.uint64), sums.view(np.uint64)), tag
    # without the gate
    rows, reason = R.rows_of(sc["grid"], sc["q"][:257], sc["poses"]["perturbed"], 0.0)
    sums, counts, got = hv.RegistrationSystem(sc["q"][:257], sc["poses"]["perturbed"], 0.0, rows=True)
    assert np.array_equal(_bits(got), _bits(rows)) and counts["too_far"] == 0
    _check_system(sums, counts, rows, reason, "%s %s no gate" % (name, source))
    if sc["frames"] is not None:
        k, v = hv.GetCubeMap()
        assert np.array_equal(k, sc["keys"]) and np.array_equal(_bits(v), _bits(sc["vox"]))


def test_02_the_sums_are_repeatable(oracle):
    sc = _scene(oracle, "reg64")
    hv = _volume(sc, "uploaded")
    big = np.ascontiguousarray(np.tile(sc["q"], (80, 1)))             # 327 760 points: more than 1024 workgroups, two trips for some lanes
    for q in (sc["q"], big):
        a, ca = hv.RegistrationSystem(q, sc["poses"]["perturbed"], sc["gate"])
        b, cb = hv.RegistrationSystem(q, sc["poses"]["perturbed"], sc["gate"])
        assert ca == cb and ca["used"] > 0.4 * len(q) and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    # the long batch is 80 times the short one: the counts exactly, the sums to the rounding of the additions
    rows, reason = _want(sc, "perturbed")
    _check_system(a, ca, np.tile(rows, (80, 1)), np.tile(reason, 80), "80 x 4097 points")


def _by_hand(hv, q, init, max_iterations, min_step=0.0, min_points=6, max_distance=R.TRUNC, trace=None):
    return R.loop(L.load(), lambda T: hv.RegistrationSystem(q, T, max_distance), init, max_iterations, min_step=min_step, min_points=min_points, trace=trace)


def _same_result(got, want, what):
    assert np.array_equal(_bits(got["T"]), _bits(want["T"])), what
    for k in ("iterations", "status", "used", "invalid", "no_gradient", "too_far", "first_used"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("rmse", "first_rmse", "last_step"):
        assert np.float64(got[k]).view(np.uint64) == np.float64(want[k]).view(np.uint64), (what, k, got[k], want[k])


def test_03_the_loop_is_the_loop(oracle):
    sc = R.reg_scene(oracle)
    hv = _handler(R.REG_CAM, R.REG_RES)
    hv.SetCubeMap(sc["keys"], sc["vox"])
    q, init = sc["cloud"], sc["init"]
    trace = []
    want = _by_hand(hv, q, init, 6, trace=trace)
    got = hv.RegisterPoints(q, init, max_iterations=6, min_step=0.0)
    print({k: v for k, v in got.items() if k != "T"})
    assert want["iterations"] == 6 and want["status"] == R.MAX_ITERATIONS
    _same_result(got, want, "six iterations")
    # the stop rule: a min_step the second step undercuts and the first does not
    steps = [t[3] for t in trace]
    assert steps[1] < steps[0]
    min_step = float(F32(math.sqrt(steps[0] * steps[1])))
    want = _by_hand(hv, q, init, 6, min_step=min_step)
    got = hv.RegisterPoints(q, init, max_iterations=6, min_step=min_step)
    assert want["iterations"] == 2 and want["status"] == R.CONVERGED
    _same_result(got, want, "converged at the second step")
    # min_points above used: nothing moves
    too_many = trace[0][1]["used"] + 1
    got = hv.RegisterPoints(q, init, max_iterations=6, min_step=0.0, min_points=too_many)
    _same_result(got, _by_hand(hv, q, init, 6, min_points=too_many), "too few points")
    assert got["status"] == R.TOO_FEW_POINTS and got["iterations"] == 0 and np.array_equal(_bits(got["T"]), _bits(init)) and got["used"] == got["first_used"] == too_many - 1
    # max_iterations = 0: one evaluation at init_T; the defaults (params = NULL) are default_params'
    got = hv.RegisterPoints(q, init, max_iterations=0)
    assert got["status"] == R.MAX_ITERATIONS and got["iterations"] == 0 and got["rmse"] == got["first_rmse"] == trace[0][2]
    p = L.RegisterParams()
    L.check(L.load().op_volume_register_default_params(hv._h, C.byref(p)))
    assert (p.max_iterations, p.max_distance, p.min_step, p.min_points) == (30, F32(R.TRUNC), F32(1e-5), 6)
    r = L.RegisterResult()
    qq, t0 = np.ascontiguousarray(q), np.ascontiguousarray(init, F32).reshape(16)
    L.check(L.load().op_volume_register_points(hv._h, C.c_void_p(qq.ctypes.data), len(qq), L.OP_MEM_HOST, t0.ctypes.data_as(L._fp), None, C.byref(r)))
    _same_result(I.CubeHandler._register_result(r), hv.RegisterPoints(q, init), "params = NULL")


def test_04_pose_recovery(oracle):
    """Same scene and bounds as tests/test_volume_register_cpu.py::test_the_restated_loop_finds_the_truth: translation < 2 mm, rotation < 0.05 degrees,
    final rmse < first_rmse / 5 after 15 iterations from 4.2 cm / 0.97 degrees.
    The independent judge: the restatement's rmse at the device's final T must not exceed the restated loop's final rmse by more than MARGIN.
    Measured on the MI355X: the device's final T is the restated loop's bit for bit (pose error 0.498 mm / below 1e-4 degrees, 8034 points used,
    rmse 0.002975277 both ways), a relative excess of 0.  The device's sums differ from math.fsum's by at most (used - 1) * 2^-53 relative, far
    below what moves a float32 component of the step, and the cost is flat to second order at its minimum; what could move the rmse is a point
    whose `used` flag flips, and between the loop's own late iterations those flips move it by 0.3 % (0.00297 <-> 0.00298).  MARGIN is a third of
    that, 0.1 %; the cap was 1 %."""
    sc = R.reg_scene(oracle)
    hv = _handler(R.REG_CAM, R.REG_RES)
    for f in sc["frames"]:
        hv.IntegrateImage(*f)
    got = hv.RegisterPoints(sc["cloud"], sc["init"], max_iterations=15, min_step=0.0)
    t, r = R.pose_error(got["T"])
    print("device: used %d, rmse %.6f (first %.6f), pose error %.3f mm / %.5f deg" % (got["used"], got["rmse"], got["first_rmse"], t * 1e3, r))
    assert got["status"] == R.MAX_ITERATIONS and got["iterations"] == 15
    assert t < 0.002
    assert r < 0.05
    assert got["rmse"] < got["first_rmse"] / 5
    evaluate = lambda T: R.system(sc["grid"], sc["cloud"], T, R.TRUNC)
    ref = R.loop(L.load(), evaluate, sc["init"], 15, min_step=0.0)
    sums, counts = evaluate(got["T"])
    judged = R.rmse_of(sums, counts["used"])
    excess = judged / ref["rmse"] - 1.0
    print("restated loop: rmse %.9f; the restatement at the device's T: rmse %.9f, used %d; relative excess %.3e" % (ref["rmse"], judged, counts["used"], excess))
    assert counts["used"] == got["used"] and abs(judged - got["rmse"]) <= 1e-12
    assert excess <= MARGIN


@pytest.mark.parametrize("stride", [1, 3])
def test_05_depth_entry_is_the_points_entry(oracle, stride):
    sc = R.reg_scene(oracle)
    hv = _cache.get("hv_reg")
    if hv is None:
        hv = _cache["hv_reg"] = _handler(R.REG_CAM, R.REG_RES)
        hv.SetCubeMap(sc["keys"], sc["vox"])
    depth, _rgb, pose = sc["frames"][4]
    depth = depth.copy()
    depth[5, 7] = 0.0                                                 # pixels without depth are skipped, on and off the stride's lattice
    depth[6, 9] = 0.0
    depth[9, 12] = 0.0
    init = D.perturbed(pose, 1)
    lib = L.load()
    w, h = R.REG_CAM[4], R.REG_CAM[5]
    pts, n = np.zeros((w * h, 3), F32), C.c_size_t(0)
    L.check(lib.op_points_from_depth(C.byref(hv.camera), C.c_void_p(depth.ctypes.data), L.OP_DEPTH_F32, L.OP_MEM_HOST, 0, C.c_void_p(pts.ctypes.data), C.byref(n)))
    mask = depth > 0
    assert n.value == mask.sum() == w * h - 3
    index = np.cumsum(mask.reshape(-1)) - 1                           # pixel -> row of the compacted cloud
    keep = np.zeros((h, w), bool)
    keep[::stride, ::stride] = True
    sub = pts[index[(keep & mask).reshape(-1)]]
    wants = {}
    for fmt in ("f32", "u16"):
        if fmt == "u16":
            raw = np.round(depth * 1000.0).astype(np.uint16)
            L.check(lib.op_points_from_depth(C.byref(hv.camera), C.c_void_p(raw.ctypes.data), L.OP_DEPTH_U16, L.OP_MEM_HOST, 0, C.c_void_p(pts.ctypes.data), C.byref(n)))
            sub = pts[index[(keep & mask).reshape(-1)]]
        else:
            raw = depth
        want = hv.RegisterPoints(sub, init, max_iterations=5, min_step=0.0)
        got = hv.RegisterDepth(raw, init, pixel_stride=stride, max_iterations=5, min_step=0.0)
        print(stride, fmt, len(sub), {k: v for k, v in got.items() if k != "T"}, R.pose_error(got["T"], pose))
        assert got["used"] > 0.8 * len(sub) and got["used"] + got["invalid"] + got["no_gradient"] + got["too_far"] == len(sub)
        _same_result(got, want, "stride %d %s" % (stride, fmt))
        wants[fmt] = want
    if stride == 1:
        import torch
        dev = torch.from_numpy(depth).to("cuda:0")
        _same_result(hv.RegisterDepth(dev, init, pixel_stride=1, max_iterations=5, min_step=0.0), wants["f32"], "a device image")


@pytest.mark.parametrize("source", ["fused", "uploaded"])
def test_06_the_volume_is_only_read(oracle, source):
    """GetCubeMap before and after is bit-equal; frames fused without an accessor in between are seen; fusing on afterwards gives the oracle's volume"""
    sc = R.reg_scene(oracle)
    fr = sc["frames"]
    half = len(fr) // 2
    ov = oracle.Volume(oracle.make_camera(*R.REG_CAM), voxel_res=R.REG_RES, trunc=R.TRUNC)
    for f in fr[:half]:
        ov.integrate(*f)
    hk, hx = ov.export()
    ref = _handler(R.REG_CAM, R.REG_RES)                              # the oracle's half volume, uploaded
    ref.SetCubeMap(hk, hx)
    hv = _handler(R.REG_CAM, R.REG_RES)
    if source == "fused":
        for f in fr[:half]:
            hv.IntegrateImage(*f)
    else:
        hv.SetCubeMap(hk, hx)
    q, init = sc["cloud"][:3000], sc["init"]
    got = hv.RegisterPoints(q, init, max_iterations=4, min_step=0.0)  # (fused: the frames are still queued when the call arrives)
    _same_result(got, ref.RegisterPoints(q, init, max_iterations=4, min_step=0.0), "queued frames are seen")
    assert got["used"] > 500
    k0, v0 = hv.GetCubeMap(sort=False)
    hv.RegisterPoints(q, init, max_iterations=3)
    hv.RegistrationSystem(q, init, R.TRUNC, rows=True)
    hv.RegisterDepth(fr[1][0], D.perturbed(fr[1][2], 1), pixel_stride=2, max_iterations=3)
    k1, v1 = hv.GetCubeMap(sort=False)
    assert np.array_equal(k0, k1) and np.array_equal(_bits(v0), _bits(v1))
    for f in fr[half:]:
        hv.IntegrateImage(*f)
    full = hv.RegisterPoints(q, init, max_iterations=2, min_step=0.0)
    whole = _handler(R.REG_CAM, R.REG_RES)
    whole.SetCubeMap(sc["keys"], sc["vox"])
    _same_result(full, whole.RegisterPoints(q, init, max_iterations=2, min_step=0.0), "right after IntegrateImage")
    k2, v2 = hv.GetCubeMap()
    assert np.array_equal(k2, sc["keys"]) and np.array_equal(_bits(v2), _bits(sc["vox"]))


def test_07_edges(oracle):
    sc = R.reg_scene(oracle)
    init = sc["init"]
    empty = _handler(R.REG_CAM, R.REG_RES)
    held = _handler(R.REG_CAM, R.REG_RES)
    held.SetCubeMap(sc["keys"], sc["vox"])
    for what, hv, q in (("the empty volume", empty, sc["cloud"][:300]), ("n = 0", held, np.zeros((0, 3), F32)), ("n = 0 on the empty volume", empty, np.zeros((0, 3), F32))):
        sums, counts, rows = hv.RegistrationSystem(q, init, R.TRUNC, rows=True)
        assert not sums.any() and counts == {"used": 0, "invalid": len(q), "no_gradient": 0, "too_far": 0} and not rows.any(), what
        got = hv.RegisterPoints(q, init)
        assert got["status"] == R.TOO_FEW_POINTS and got["iterations"] == 0 and np.array_equal(_bits(got["T"]), _bits(init)), what
        assert got["used"] == got["first_used"] == 0 and got["rmse"] == got["first_rmse"] == 0.0 and got["invalid"] == len(q), what
    assert empty.BlockCount() == 0
    lib = L.load()
    sums, r = np.zeros(28), L.RegisterResult()
    t0 = np.ascontiguousarray(init, F32).reshape(16)
    assert lib.op_volume_register_system(held._h, None, 0, L.OP_MEM_HOST, t0.ctypes.data_as(L._fp), 0.1, sums.ctypes.data_as(C.POINTER(C.c_double)), None, None) == L.OP_OK
    assert lib.op_volume_register_points(held._h, None, 0, L.OP_MEM_DEVICE, t0.ctypes.data_as(L._fp), None, C.byref(r)) == L.OP_OK and r.status == R.TOO_FEW_POINTS
    # a depth image without a valid pixel
    got = held.RegisterDepth(np.zeros((R.REG_CAM[5], R.REG_CAM[4]), F32), init)
    assert got["status"] == R.TOO_FEW_POINTS and got["used"] == 0 and got["invalid"] == 0 and np.array_equal(_bits(got["T"]), _bits(init))
    # refusals with a live volume
    pts = np.zeros((4, 3), F32)
    assert lib.op_volume_register_points(held._h, C.c_void_p(pts.ctypes.data), 4, L.OP_MEM_HOST, t0.ctypes.data_as(L._fp), None, None) == L.OP_ERR_INVALID
    assert lib.op_volume_register_points(held._h, None, 4, L.OP_MEM_HOST, t0.ctypes.data_as(L._fp), None, C.byref(r)) == L.OP_ERR_INVALID
    assert lib.op_volume_register_system(held._h, C.c_void_p(pts.ctypes.data), 4, L.OP_MEM_HOST, t0.ctypes.data_as(L._fp), 0.1, None, None, None) == L.OP_ERR_INVALID


def test_09_driver_paths_agree():
    """examples/cpp/ModelRegistration: the fused path and the path there was before (op_volume_sample per iteration + a host loop over the rows) take the
    same iterations over the same points and end at the same place -- their sums differ in the order of the additions only, and the driver prints
    six digits"""
    import json
    exe = os.path.join(ROOT, "examples", "cpp", "ModelRegistration.bin")
    assert os.path.exists(exe), "examples/cpp/ModelRegistration.bin is not built (__graft_entry__.build())"
    out = {}
    for path in ("sample", "fused"):
        run = subprocess.run([exe, "--synthetic", "6", "5", "1", "--res", "0.04", "--perturb", "3", "--iters", "3", "--path", path], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
        out[path] = json.loads(run.stdout.strip().splitlines()[-1])
        print(path, out[path])
    a, b = out["sample"], out["fused"]
    assert a["registered"] == b["registered"] == 2 and a["iterations"] == b["iterations"] == 6 and a["points"] == b["points"] == 640 * 480
    assert a["used_last"] == b["used_last"] > 0.5 * a["points"]
    assert a["error_before"] == b["error_before"] and 30 < a["error_before"]["mm"] < 50
    for k in ("mm", "deg", "max_mm", "max_deg"):
        assert abs(a["error_after"][k] - b["error_after"][k]) <= 1e-3 * max(a["error_after"][k], 1e-3), k
    for k in ("first", "final"):
        assert abs(a["rmse"][k] - b["rmse"][k]) <= 1e-5 * a["rmse"][k], k
    assert b["rmse"]["final"] < b["rmse"]["first"]


def test_08_class_surface(oracle, tmp_path):
    """CubeHandler::RegistrationSystem / RegisterPointCloud / RegisterDepth (host/one_piece) return what the C-ABI returns for the same volume and inputs"""
    sc = R.reg_scene(oracle)
    exe = tmp_path / "register_surface_check"
    host, lib = os.path.join(ROOT, "host", "one_piece"), os.path.join(ROOT, "onepiece_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-I", host, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "register_surface_check.cpp"),
                           "-L", host, "-lone_piece_hip_host", "-L", lib, "-lonepiece_hip", "-Wl,-rpath," + host, "-Wl,-rpath," + lib, "-o", str(exe)])
    hv = _handler(R.REG_CAM, R.REG_RES)
    hv.SetCubeMap(sc["keys"], sc["vox"])
    hv.WriteToFile(tmp_path / "room.map")
    back = _handler(R.REG_CAM, R.REG_RES)
    back.ReadFromFile(tmp_path / "room.map")
    q = sc["cloud"][:3000]
    q.tofile(tmp_path / "points.bin")
    depth, _rgb, pose = sc["frames"][4]
    start = D.perturbed(pose, 1)
    depth.tofile(tmp_path / "depth.bin")
    (tmp_path / "pose.txt").write_text(" ".join("%.9g" % v for v in start.reshape(-1)))
    camt = R.REG_CAM
    run = subprocess.run([str(exe), str(tmp_path / "room.map"), repr(R.REG_RES), str(tmp_path / "points.bin"), str(tmp_path / "depth.bin")] +
                         [repr(float(v)) for v in camt[:4]] + [str(camt[4]), str(camt[5]), str(tmp_path / "pose.txt")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = {l.split()[0]: l.split()[1:] for l in run.stdout.strip().splitlines() if l.split() and l.split()[0] in ("system", "points", "defaults", "depth")}
    init = np.eye(4, dtype=F32)
    init[:3, 3] = [0.01, -0.02, 0.005]
    sums, counts = back.RegistrationSystem(q, init, 0.1)
    row = lines["system"]
    assert [int(v) for v in row[:4]] == [counts[k] for k in R.COUNT_NAMES] and counts["used"] > 1000
    assert np.array_equal(np.array([float(v) for v in row[4:]]).view(np.uint64), sums.view(np.uint64))

    def same(row, want, details=True):
        if details:
            assert [int(v) for v in row[:7]] == [want[k] for k in ("iterations", "status", "used", "invalid", "no_gradient", "too_far", "first_used")]
            assert float(row[7]) == want["rmse"] and float(row[8]) == want["first_rmse"]
        assert float(row[9]) == want["rmse"]
        assert np.array_equal(_bits(np.array([F32(v) for v in row[10:]], F32)), _bits(want["T"].reshape(-1)))
    same(lines["points"], back.RegisterPoints(q, init, max_iterations=4, max_distance=0.1, min_step=0.0, min_points=6))
    same(lines["defaults"], back.RegisterPoints(q), details=False)
    same(lines["depth"], back.RegisterDepth(depth, start, pixel_stride=2, max_iterations=4, max_distance=0.1, min_step=0.0, min_points=6))
