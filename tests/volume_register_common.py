"""op_volume_register_* restated in numpy float32 (test infrastructure shared by tests/test_volume_register_cpu.py and
tests/test_volume_register_gpu.py), built from the pieces of tests/volume_sample_common.py -- which tests/test_volume_sample_cpu.py pins to the
committed oracle.

The definition is the header's (include/onepiece_hip.h, op_volume_register_system / _points): the transformed point, the trilinear sdf, its
central difference and the raycaster's normalisation come from S; the cross products are separate float32 operations; the 28 terms are widened to
float64 and summed by math.fsum.  The loop solves and exponentiates with the library's own host exports (op_ldlt_solve6, op_se3_exp: no device
needed) and restates the 4x4 product in float32."""
import ctypes as C
import math

import numpy as np

import deintegrate_common as D
import volume_sample_common as S

F32 = np.float32
CONVERGED, MAX_ITERATIONS, TOO_FEW_POINTS, SINGULAR = 0, 1, 2, 3
COUNT_NAMES = ("used", "invalid", "no_gradient", "too_far")
PAIRS = [(a, b) for a in range(6) for b in range(a, 6)]              # sums[0..20]: the upper triangle row by row

# the convergence scene: the room through eight 64 x 48 frames 25 room frames apart, 2 cm voxels, truncation 0.1
REG_CAM, REG_FRAMES, REG_STRIDE, REG_RES, TRUNC = D.CAM_64, 8, 25, 0.02, 0.1


def rows_of(grid, points, T, max_distance):
    """-> (rows [n,8] float32: j[6], s, used as 1.0 / 0.0, eight zeros for an unused point; reason [n]: 0 used, 1 invalid, 2 no gradient, 3 too far)"""
    p = S.transform_points(T, points)
    valid, _oor, acc = S.trilinear(grid, p)
    s = acc[:, 0].astype(F32)
    d, ok = S.gradient(grid, p)
    with np.errstate(all="ignore"):
        l2 = d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        has_normal = ok & (l2 > 0)
        near = np.abs(s) <= F32(max_distance) if max_distance > 0 else np.ones(len(p), bool)     # False for NaN
        nrm = S.normalised(d, ok)
        reason = np.where(~valid, 1, np.where(~has_normal, 2, np.where(~near, 3, 0)))
        used = reason == 0
        j = np.stack([nrm[:, 0], nrm[:, 1], nrm[:, 2],
                      p[:, 1] * nrm[:, 2] - p[:, 2] * nrm[:, 1],
                      p[:, 2] * nrm[:, 0] - p[:, 0] * nrm[:, 2],
                      p[:, 0] * nrm[:, 1] - p[:, 1] * nrm[:, 0]], axis=1).astype(F32)
    rows = np.zeros((len(p), 8), F32)
    rows[used, :6] = j[used]
    rows[used, 6] = s[used]
    rows[used, 7] = 1.0
    return rows, reason


def terms_of(rows):
    """the 28 terms of every used row, float64 [k,28]: (double)(j_a j_b), (double)(s j_a), (double)s (double)s"""
    r = rows[rows[:, 7] != 0]
    j, s = r[:, :6], r[:, 6]
    t = [(j[:, a] * j[:, b]).astype(np.float64) for a, b in PAIRS]
    t += [(s * j[:, a]).astype(np.float64) for a in range(6)]
    t.append(s.astype(np.float64) * s.astype(np.float64))
    return np.stack(t, axis=1) if len(r) else np.zeros((0, 28))


def fold(rows, reason):
    """-> (sums [28] by math.fsum, sum of |term| [28], counts dict)"""
    t = terms_of(rows)
    sums = np.array([math.fsum(t[:, k]) for k in range(28)])
    mags = np.array([math.fsum(np.abs(t[:, k])) for k in range(28)])
    return sums, mags, {name: int((reason == k).sum()) for k, name in enumerate(COUNT_NAMES)}


def system(grid, points, T, max_distance):
    rows, reason = rows_of(grid, points, T, max_distance)
    sums, _m, counts = fold(rows, reason)
    return sums, counts


def mul4(a, b):
    """the float32 4x4 product, each element ((a0 b0 + a1 b1) + a2 b2) + a3 b3"""
    a, b = np.asarray(a, F32).reshape(4, 4), np.asarray(b, F32).reshape(4, 4)
    c = np.empty((4, 4), F32)
    for r in range(4):
        for k in range(4):
            c[r, k] = ((a[r, 0] * b[0, k] + a[r, 1] * b[1, k]) + a[r, 2] * b[2, k]) + a[r, 3] * b[3, k]
    return c


def solve_step(lib, sums):
    """x = op_ldlt_solve6(JTJ, JTr) and op_se3_exp(x), through the library's host exports"""
    JTJ = np.zeros((6, 6))
    for k, (a, b) in enumerate(PAIRS):
        JTJ[a, b] = JTJ[b, a] = sums[k]
    JTr = np.ascontiguousarray(sums[21:27], np.float64)
    x, E = np.zeros(6, F32), np.zeros(16, F32)
    dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
    fp = lambda v: v.ctypes.data_as(C.POINTER(C.c_float))
    JTJ = np.ascontiguousarray(JTJ.reshape(36))
    assert lib.op_ldlt_solve6(dp(JTJ), dp(JTr), fp(x)) == 0
    assert lib.op_se3_exp(fp(x), fp(E)) == 0
    return x, E.reshape(4, 4)


def rmse_of(sums, used):
    return math.sqrt(sums[27] / used) if used else 0.0


def loop(lib, evaluate, init_T, max_iterations, min_step=0.0, min_points=6, trace=None):
    """The host loop of op_volume_register_points around evaluate(T) -> (sums [28], counts dict) -> dict of the result's fields.
    trace: a list that receives (T, counts, rmse, |x|) per iteration."""
    T = np.asarray(init_T, F32).reshape(4, 4).copy()
    res = {"iterations": 0, "status": MAX_ITERATIONS, "last_step": 0.0}
    first, current = None, None
    for _it in range(max_iterations):
        current = evaluate(T)
        sums, counts = current
        first = first or current
        if counts["used"] < max(min_points, 0):
            res["status"] = TOO_FEW_POINTS
            break
        x, E = solve_step(lib, sums)
        if not np.isfinite(x).all():
            res["status"] = SINGULAR
            break
        ss = sum(float(v) * float(v) for v in x)                      # in x's order, in double
        if trace is not None:
            trace.append((T.copy(), dict(counts), rmse_of(sums, counts["used"]), math.sqrt(ss)))
        T = mul4(E, T)
        current = None
        res["iterations"] += 1
        res["last_step"] = math.sqrt(ss)
        if ss < float(F32(min_step)) * float(F32(min_step)):
            res["status"] = CONVERGED
            break
    if current is None:
        current = evaluate(T)
    if first is None:
        first = current
        if current[1]["used"] < max(min_points, 0):
            res["status"] = TOO_FEW_POINTS
    sums, counts = current
    res.update(counts)
    res.update(T=T, rmse=rmse_of(sums, counts["used"]), first_used=first[1]["used"], first_rmse=rmse_of(first[0], first[1]["used"]))
    return res


def pose_error(T, truth=None):
    """-> (translation error in metres, rotation error in degrees) of T against `truth` (identity by default)"""
    T = np.asarray(T, np.float64).reshape(4, 4)
    E = T if truth is None else T @ np.linalg.inv(np.asarray(truth, np.float64).reshape(4, 4))
    c = min(1.0, max(-1.0, (np.trace(E[:3, :3]) - 1.0) / 2.0))
    return float(np.linalg.norm(E[:3, 3])), math.degrees(math.acos(c))


_scene = {}


def reg_scene(oracle):
    """the convergence scene, fused by the oracle -> dict(frames, keys, vox, grid, cloud: every third of the eight frames' hit points, world)"""
    if not _scene:
        fr = D.frames(REG_CAM, REG_FRAMES, stride=REG_STRIDE)
        vol = oracle.Volume(oracle.make_camera(*REG_CAM), voxel_res=REG_RES, trunc=TRUNC)
        for f in fr:
            vol.integrate(*f)
        keys, vox = vol.export()
        cloud = np.concatenate([S.hit_points(f[2], REG_CAM, f[0])[1] for f in fr])[::3]
        _scene.update(frames=fr, keys=keys, vox=vox, grid=S.Grid(keys, vox, REG_RES), cloud=np.ascontiguousarray(cloud, F32),
                      init=D.perturbed(np.eye(4), 1))
    return _scene


# ---- the hand-made field: seven blocks of 1/32 m voxels around the origin holding s = z - Z0 at every voxel centre, block (0, 0, 0) absent -------
HAND_RES = 0.03125
HAND_Z0 = -0.0625
HAND_KEYS = np.array([k for k in ((x, y, z) for z in (-1, 0) for y in (-1, 0) for x in (-1, 0)) if k != (0, 0, 0)], np.int32)


def hand_blocks():
    centres = S.block_voxel_centres(HAND_KEYS, HAND_RES)              # exact: multiples of 1/64
    vox = np.empty((len(HAND_KEYS), 512, 5), F32)
    vox[..., 0] = centres[..., 2] - F32(HAND_Z0)
    vox[..., 1] = 1.0
    vox[..., 2:] = 0.5
    return vox


# (what, point, reason) -- every coordinate a multiple of 1/128: g = 32 p - 0.5 has quarter fractions, every weight, product and sum is exact
HAND_POINTS = [
    ("on the surface side, deep inside", (-0.125, -0.125, -0.0625 + 1 / 128), 0),
    ("a block face", (-0.125, 0.0, -0.125 + 1 / 64), 0),
    ("farther than max_distance", (-0.125, -0.125, 0.125), 3),
    ("in the absent block", (0.125, 0.125, 0.125), 1),
    ("only the +h sample on x reaches the absent block", (-3 / 128, 11 / 128, 3 / 128), 2),
    ("NaN", (np.nan, 0.0, 0.0), 1), ("1e9", (1e9, 0.0, 0.0), 1), ("-1e9", (0.0, -1e9, 0.0), 1),
]


def hand_cloud(n=400, seed=5):
    rng = np.random.default_rng(seed)
    rnd = rng.integers(-38, 39, (n, 3)).astype(np.float64) / 128.0
    return np.concatenate([np.array([p for _w, p, _r in HAND_POINTS], np.float64), rnd]).astype(F32)
