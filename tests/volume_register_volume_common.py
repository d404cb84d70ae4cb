"""op_volume_band_voxels, op_volume_register_offset_* and op_volume_register_volume restated in numpy float32 (test infrastructure shared by
tests/test_register_volume_cpu.py and tests/test_register_volume_gpu.py), built on tests/volume_register_robust_common.py (B: the linearisations,
the Huber weights, the fold and the loop), tests/volume_sample_common.py (S: the samples, the voxel centres) and tests/deintegrate_common.py (D:
the frames and the start).  This is the feature's reference.

The definitions are the header's (include/onepiece_hip.h).  The selection: a voxel is selected iff w > 0, w >= min_weight, |sdf| <= band and its
local coordinates are multiples of the stride; blocks in the order given, voxels x + 8y + 64z ascending.  The offset system: B.rows_of with ONE
change -- the residual the linearisation starts from is s - o, one float32 subtraction; the USED rule, max_distance and the stored-sdf sum keep
s; a non-finite o makes the point invalid."""
import numpy as np

import deintegrate_common as D
import volume_register_color_common as K
import volume_register_robust_common as B
import volume_sample_common as S

F32 = np.float32

# the submaps of the convergence case: the forty frames of B's model, A = the first 25, B = the last 25 (ten frames shared), both at their true poses
SUB_A, SUB_B = slice(0, 25), slice(15, 40)
CASE_BAND, CASE_STRIDE, CASE_MIN_WEIGHT, CASE_ITERATIONS, CASE_MIN_STEP = 0.04, 2, 1.0, 15, 1e-5


def default_band(res):
    """2.0f * res"""
    return float(F32(2.0) * F32(res))


def select(keys, vox, res, trunc, band=None, min_weight=1.0, stride=1, intensity=True):
    """the band voxels of (keys [m,3], vox [m,512,5]) in the given block order -> (xyz [n,3], sdf [n], intensity [n] or None, (block, voxel) [n,2]);
    band None: 2 res; band <= 0: trunc"""
    keys = np.asarray(keys, np.int32).reshape(-1, 3)
    vox = np.asarray(vox, F32).reshape(-1, 512, 5)
    band = F32(default_band(res) if band is None else band)
    if not band > 0:
        band = F32(trunc)
    vid = np.arange(512)
    on_lattice = ((vid & 7) | ((vid >> 3) & 7) | (vid >> 6)) & (stride - 1) == 0
    s, w = vox[..., 0], vox[..., 1]
    with np.errstate(all="ignore"):
        ok = (w > 0) & (w >= F32(min_weight)) & (np.abs(s) <= band) & on_lattice[None, :]      # (False for NaN)
    index = np.argwhere(ok)                                           # row-major: block ascending, voxel ascending
    b, v = index[:, 0], index[:, 1]
    centres = S.block_voxel_centres(keys, res)
    y = K.intensity(vox[b, v, 2:5]) if intensity else None
    return np.ascontiguousarray(centres[b, v], F32), np.ascontiguousarray(s[b, v], F32), y, index


def rows_of(grid, points, offset, y, T, max_distance, color_scale=0.0, max_color_residual=0.0, mode=B.NORMAL, huber=0.0, huber_color=0.0):
    """B.rows_of with a target value per point (offset None IS B.rows_of) -> the same dict"""
    if offset is None:
        return B.rows_of(grid, points, y, T, max_distance, color_scale, max_color_residual, mode, huber, huber_color)
    with K._samples_taken_once():
        rows, reason, colored, rc = K._rows_of(grid, points, y, T, max_distance, color_scale, max_color_residual)
        p = S.transform_points(T, points)
        d, _ok = S.gradient(grid, p)
    o = np.asarray(offset, F32).reshape(-1)
    n = len(rows)
    assert len(o) == n
    finite = np.isfinite(o)
    reason = np.where(finite, reason, 1)                              # a non-finite target value: invalid
    colored = colored & finite
    rc = np.where(colored, rc, F32(0.0)).astype(F32)
    used = reason == 0
    res = F32(grid.res)
    s = rows[:, 6].copy()
    with np.errstate(all="ignore"):
        e = (s - o).astype(F32)                                       # the one change
        a, r = rows[:, :3].copy(), e.copy()
        if mode == B.GRADIENT:
            a = (d / res).astype(F32)
        elif mode == B.METRIC:
            l2 = d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
            r = (e / (np.sqrt(l2) / res)).astype(F32)
        else:
            assert mode == B.NORMAL, mode
        j = np.stack([a[:, 0], a[:, 1], a[:, 2],
                      p[:, 1] * a[:, 2] - p[:, 2] * a[:, 1],
                      p[:, 2] * a[:, 0] - p[:, 0] * a[:, 2],
                      p[:, 0] * a[:, 1] - p[:, 1] * a[:, 0]], axis=1).astype(F32)
        r = np.where(used, r, F32(0.0)).astype(F32)
        q, down = B.huber_scale(r, huber)
        qc, cdown = B.huber_scale(rc, huber_color if color_scale > 0 else 0.0)
        out = np.zeros((n, 16), F32)
        if huber > 0:
            j, rw = (q[:, None] * j).astype(F32), (q * r).astype(F32)
        else:
            rw = r
        out[used, :6] = j[used]
        out[used, 6] = rw[used]
        out[used, 7] = 1.0
        if color_scale > 0 and huber_color > 0:
            out[:, 8:14] = qc[:, None] * rows[:, 8:14]
            out[:, 14] = qc * rows[:, 14]
        else:
            out[:, 8:15] = rows[:, 8:15]
        out[:, 15] = rows[:, 15]
        out[~colored, 8:] = 0
    return dict(rows=out, reason=reason, colored=colored, rc=rc, s=np.where(used, s, F32(0.0)).astype(F32), r=r, down=down & used, cdown=cdown & colored)


fold = B.fold                                                         # the 31 sums, their bounds, the seven counts
loop = B.loop                                                         # the one loop


def system(grid, points, offset, y, T, max_distance, color_scale=0.0, max_color_residual=0.0, mode=B.NORMAL, huber=0.0, huber_color=0.0):
    sums, _b, counts = fold(rows_of(grid, points, offset, y, T, max_distance, color_scale, max_color_residual, mode, huber, huber_color))
    return sums, counts


_submaps = {}


def submaps(oracle):
    """the two overlapping submaps, fused by the oracle at their true poses (the truth is the identity) -> dict(A / B: dict(keys, vox, grid), init)"""
    if not _submaps:
        fr = B.model(oracle)["frames"]
        for name, part in (("A", SUB_A), ("B", SUB_B)):
            vol = oracle.Volume(oracle.make_camera(*B.MODEL_CAM), voxel_res=B.MODEL_RES, trunc=B.TRUNC)
            for f in fr[part]:
                vol.integrate(*f)
            keys, vox = vol.export()
            _submaps[name] = dict(keys=keys, vox=vox, grid=S.Grid(keys, vox, B.MODEL_RES))
        _submaps["init"] = B.model_init()
    return _submaps


_case = {}


def case(oracle, lib, offsets=True):
    """the restated loop of the convergence case (computed once per session): B's band voxels (band 0.04, stride 2, min_weight 1) against A, GRADIENT,
    15 iterations, min_step 1e-5, max_distance the truncation, geometric; offsets False: the same points with target value 0 (the route a user had
    before) -> (result dict, translation error in metres, rotation error in degrees, selected); prints the error per iteration"""
    if offsets not in _case:
        sm = submaps(oracle)
        xyz, sdf, _y, _i = select(sm["B"]["keys"], sm["B"]["vox"], B.MODEL_RES, B.TRUNC, band=CASE_BAND, min_weight=CASE_MIN_WEIGHT, stride=CASE_STRIDE, intensity=False)
        o = sdf if offsets else np.zeros_like(sdf)
        trace = []
        res = loop(lib, lambda T: system(sm["A"]["grid"], xyz, o, None, T, B.TRUNC, mode=B.GRADIENT), sm["init"], CASE_ITERATIONS, min_step=CASE_MIN_STEP, trace=trace)
        t, r = B.R.pose_error(res["T"])
        print("submap B against A, %s: %d selected; error mm per iteration %s; %d iterations, status %d, last step %.2e, final %.3f mm / %.5f deg, used %d" % (
            "own sdf as target value" if offsets else "target value 0", len(xyz), " ".join("%.1f" % (B.R.pose_error(tr[0])[0] * 1e3) for tr in trace),
            res["iterations"], res["status"], res["last_step"], t * 1e3, r, res["used"]))
        _case[offsets] = (res, t, r, len(xyz))
    return _case[offsets]
