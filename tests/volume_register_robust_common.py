"""The linearisations and Huber weights of op_volume_register_robust_* restated in numpy float32 (test infrastructure shared by
tests/test_volume_register_robust_cpu.py and tests/test_volume_register_robust_gpu.py), built on tests/volume_register_common.py (p, s, the USED rule,
n, the four counts) and tests/volume_register_color_common.py (rc, the COLOURED rule, jc, rcs).  This is the feature's reference.

The definition is the header's (include/onepiece_hip.h, op_volume_register_robust_system): the linearisation picks the row vector a and the
residual r -- NORMAL (n, s), GRADIENT (d / res, s), METRIC (n, s / (sqrt(l2) / res)) --, the row is (a ; p x a) with the cross products of the
geometric entry, the Huber weight w = min(1, huber / |r|) scales row and residual by sqrt(w), one float32 product each, and the colour term
likewise by its own.  Every operation is ONE float32 operation of numpy.  The 31 terms are widened to float64 and summed by math.fsum."""
import math

import numpy as np

import deintegrate_common as D
import volume_register_color_common as K
import volume_register_common as R
import volume_sample_common as S

F32 = np.float32
NORMAL, GRADIENT, METRIC = 0, 1, 2
MODES = {"normal": NORMAL, "gradient": GRADIENT, "metric": METRIC}
COUNT_NAMES = K.COUNT_NAMES + ("downweighted", "color_downweighted")
PAIRS = R.PAIRS

# the model of the convergence cases: the room through forty 64 x 48 frames 5 room frames apart, 2 cm voxels, truncation 0.1
MODEL_CAM, MODEL_FRAMES, MODEL_STRIDE, MODEL_RES, TRUNC = D.CAM_64, 40, 5, 0.02, 0.1


def huber_scale(r, huber):
    """-> (q = sqrtf(w), down = w < 1) of residuals r: w = 1 when |r| <= huber, else huber / |r|; huber <= 0: no weights"""
    r = np.asarray(r, F32)
    if not huber > 0:
        return np.ones(len(r), F32), np.zeros(len(r), bool)
    with np.errstate(all="ignore"):
        a = np.abs(r)
        w = np.where(a <= F32(huber), F32(1.0), F32(huber) / a).astype(F32)
        return np.sqrt(w).astype(F32), w < 1


def rows_of(grid, points, y, T, max_distance, color_scale=0.0, max_color_residual=0.0, mode=NORMAL, huber=0.0, huber_color=0.0):
    """-> dict(rows [n,16] float32: j[6], r, used, jc[6], rcs, colored -- what enters the sums; reason [n] as R.rows_of; colored [n] bool;
    rc [n]: the unscaled, unweighted colour residual, zero unless coloured; s [n]: the stored sdf, zero unless used; r [n]: the unweighted
    residual, zero unless used; down, cdown [n] bool)"""
    with K._samples_taken_once():
        rows, reason, colored, rc = K._rows_of(grid, points, y, T, max_distance, color_scale, max_color_residual)
        p = S.transform_points(T, points)
        d, ok = S.gradient(grid, p)
    n = len(rows)
    used = reason == 0
    res = F32(grid.res)
    s = rows[:, 6].copy()
    with np.errstate(all="ignore"):
        a, r = rows[:, :3].copy(), s.copy()
        if mode == GRADIENT:
            a = (d / res).astype(F32)
        elif mode == METRIC:
            l2 = d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
            r = (s / (np.sqrt(l2) / res)).astype(F32)
        else:
            assert mode == NORMAL, mode
        j = np.stack([a[:, 0], a[:, 1], a[:, 2],
                      p[:, 1] * a[:, 2] - p[:, 2] * a[:, 1],
                      p[:, 2] * a[:, 0] - p[:, 0] * a[:, 2],
                      p[:, 0] * a[:, 1] - p[:, 1] * a[:, 0]], axis=1).astype(F32)
        r = np.where(used, r, F32(0.0)).astype(F32)
        q, down = huber_scale(r, huber)
        qc, cdown = huber_scale(rc, huber_color if color_scale > 0 else 0.0)
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


def terms_of(w):
    """the 31 terms of every used row, float64 [k,31]: K.terms_of's 28 system terms from the scaled rows, rc rc, s s (stored sdf), r r (unweighted)"""
    u = w["reason"] == 0
    if not u.any():
        return np.zeros((0, 31))
    t, _col = K.terms_of(w["rows"], w["rc"])
    d = lambda v: v[u].astype(np.float64)
    return np.concatenate([t[:, :29], (d(w["s"]) * d(w["s"]))[:, None], (d(w["r"]) * d(w["r"]))[:, None]], axis=1)


def fold(w):
    """-> (sums [31] by math.fsum, the bound of each slot [31]: (k - 1) 2^-53 sum |term| with k the number of terms the slot receives, counts dict)"""
    t = terms_of(w)
    sums = np.array([math.fsum(t[:, k]) for k in range(31)])
    mags = np.array([math.fsum(np.abs(t[:, k])) for k in range(31)])
    n_terms = np.array([len(t)] * 28 + [int(w["colored"].sum()) if len(t) else 0, len(t), len(t)])
    bound = np.maximum(n_terms - 1, 0) * 2.0 ** -53 * mags
    counts = {name: int((w["reason"] == k).sum()) for k, name in enumerate(R.COUNT_NAMES)}
    counts.update(colored=int(w["colored"].sum()), downweighted=int(w["down"].sum()), color_downweighted=int(w["cdown"].sum()))
    return sums, bound, counts


def system(grid, points, y, T, max_distance, color_scale=0.0, max_color_residual=0.0, mode=NORMAL, huber=0.0, huber_color=0.0):
    sums, _b, counts = fold(rows_of(grid, points, y, T, max_distance, color_scale, max_color_residual, mode, huber, huber_color))
    return sums, counts


def rmse_residual(sums, used):
    return math.sqrt(sums[30] / used) if used else 0.0


def loop(lib, evaluate, init_T, max_iterations, min_step=0.0, min_points=6, trace=None):
    """op_volume_register_robust_points' host loop: K.loop (the one loop) around evaluate(T) -> (sums [31], counts dict of COUNT_NAMES), and the
    fields the robust result adds, from the first and the last evaluation."""
    seen = []

    def ev(T):
        out = evaluate(T)
        if not seen:
            seen.append(out)
        seen[1:] = [out]
        return out
    res = K.loop(lib, ev, init_T, max_iterations, min_step=min_step, min_points=min_points, trace=trace)
    first, last = seen[0], seen[-1]
    res.update(first_downweighted=first[1]["downweighted"], rmse_residual=rmse_residual(last[0], last[1]["used"]),
               first_rmse_residual=rmse_residual(first[0], first[1]["used"]))
    return res


def model_init():
    """the start of every convergence case: 41.8 mm / 0.97 degrees off the identity"""
    return D.perturbed(np.eye(4), 1)


_model = {}


def model(oracle):
    """the forty-frame model, fused by the oracle -> dict(frames, keys, vox, grid, init; cloud(i): frame i's hit points in world coordinates)"""
    if not _model:
        fr = D.frames(MODEL_CAM, MODEL_FRAMES, stride=MODEL_STRIDE)
        vol = oracle.Volume(oracle.make_camera(*MODEL_CAM), voxel_res=MODEL_RES, trunc=TRUNC)
        for f in fr:
            vol.integrate(*f)
        keys, vox = vol.export()
        clouds = {}

        def cloud(i):
            if i not in clouds:
                clouds[i] = np.ascontiguousarray(S.hit_points(fr[i][2], MODEL_CAM, fr[i][0])[1], F32)
            return clouds[i]
        _model.update(frames=fr, keys=keys, vox=vox, grid=S.Grid(keys, vox, MODEL_RES), init=D.perturbed(np.eye(4), 1), cloud=cloud)
    return _model


def with_outliers(cloud, seed=7, share=0.2, lo=0.03, hi=0.08):
    """`share` of the points pushed lo..hi metres off in random directions (np.random.default_rng(seed))"""
    rng = np.random.default_rng(seed)
    out = np.asarray(cloud, np.float64).copy()
    pick = rng.permutation(len(out))[:int(round(share * len(out)))]
    v = rng.normal(size=(len(pick), 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    out[pick] += v * rng.uniform(lo, hi, len(pick))[:, None]
    return np.ascontiguousarray(out, F32)


_runs = {}


def case(oracle, lib, what, mode, max_iterations=10, huber=0.0, outliers=False):
    """the restated loop of a convergence case (computed once per session): `what` a frame of the model or "scene" (R.reg_scene), geometric,
    min_step 1e-5, max_distance TRUNC -> (result dict, translation error in metres, rotation error in degrees); prints the error per iteration"""
    key = (what, mode, max_iterations, huber, outliers)
    if key not in _runs:
        grid, cloud = case_inputs(oracle, what, outliers)
        trace = []
        res = loop(lib, lambda T: system(grid, cloud, None, T, TRUNC, mode=mode, huber=huber), model_init(), max_iterations, min_step=1e-5, trace=trace)
        t, r = R.pose_error(res["T"])
        print("%s mode %d huber %g%s: error mm per iteration %s; %d iterations, status %d, last step %.2e, final %.3f mm / %.5f deg, used %d, downweighted %d, "
              "residual rmse %.5f" % (what, mode, huber, " outliers" if outliers else "", " ".join("%.1f" % (R.pose_error(tr[0])[0] * 1e3) for tr in trace),
                                      res["iterations"], res["status"], res["last_step"], t * 1e3, r, res["used"], res["downweighted"], res["rmse_residual"]))
        _runs[key] = (res, t, r)
    return _runs[key]


def case_inputs(oracle, what, outliers=False):
    """-> (grid, cloud) of a convergence case"""
    if what == "scene":
        sc = R.reg_scene(oracle)
        grid, cloud = sc["grid"], sc["cloud"]
    else:
        md = model(oracle)
        grid, cloud = md["grid"], md["cloud"](what)
    return grid, with_outliers(cloud) if outliers else cloud


# ---- the hand-made field of volume_register_common with slope 2: s = 2 (z - Z0) at every voxel centre (dyadic: rows and sums are exact) --------
def steep_blocks(color=False):
    vox = K.hand_blocks() if color else R.hand_blocks()
    vox[..., 0] = F32(2.0) * vox[..., 0]
    return vox
