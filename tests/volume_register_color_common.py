"""The colour term of op_volume_register_color_* restated in numpy float32 (test infrastructure shared by tests/test_volume_register_color_cpu.py
and tests/test_volume_register_color_gpu.py), built from tests/volume_register_common.py (the geometric part, unchanged) and
tests/volume_sample_common.py (the trilinear colour sums).

The definition is the header's (include/onepiece_hip.h, op_volume_register_color_system): p, s, the USED rule, the row j and the four counts are
R.rows_of's; the model intensity is I(c) = (0.114 c0 + 0.587 c1) + 0.299 c2 of the colour sums of the same sample, its gradient the central
difference of I over the six shifted samples divided by res; every product, sum and quotient is ONE float32 operation of numpy.  The terms are
widened to float64 -- geometric + colour in one double -- and summed by math.fsum."""
import contextlib
import math

import numpy as np

import deintegrate_common as D
import volume_register_common as R
import volume_sample_common as S

F32 = np.float32
COUNT_NAMES = R.COUNT_NAMES + ("colored",)
PAIRS = R.PAIRS

# the scene the geometric registration cannot hold: eight 64 x 48 frames 5 room frames apart (one corner of the room), 2 cm voxels, truncation 0.1
COL_CAM, COL_FRAMES, COL_STRIDE, COL_RES, TRUNC = D.CAM_64, 8, 5, 0.02, 0.1


def intensity(c):
    """I(c) of colour triples [n,3] float32 in stored channel order"""
    c = np.asarray(c, F32)
    with np.errstate(all="ignore"):
        return ((F32(0.114) * c[..., 0] + F32(0.587) * c[..., 1]) + F32(0.299) * c[..., 2]).astype(F32)


def intensity_of_bytes(rgb):
    """y of pixels' three bytes: I(b0 / 255.0f, b1 / 255.0f, b2 / 255.0f)"""
    return intensity(np.asarray(rgb, np.uint8).astype(F32) / F32(255.0))


def model_intensity(grid, p):
    """-> (m [n]: I of the colour sums at p, g [n,3]: (I(p + h e_a) - I(p - h e_a)) / res); meaningful where the point is used"""
    p = np.asarray(p, F32).reshape(-1, 3)
    h = F32(0.5) * grid.res
    with np.errstate(all="ignore"):
        m = intensity(S.trilinear(grid, p)[2][:, 2:5])
        g = np.zeros((len(p), 3), F32)
        for a in range(3):
            pp, pm = p.copy(), p.copy()
            pp[:, a] = p[:, a] + h
            pm[:, a] = p[:, a] - h
            ip, im = intensity(S.trilinear(grid, pp)[2][:, 2:5]), intensity(S.trilinear(grid, pm)[2][:, 2:5])
            g[:, a] = (ip - im) / grid.res
    return m, g


@contextlib.contextmanager
def _samples_taken_once():
    """R.rows_of and model_intensity take the same seven samples (S.trilinear returns all five planes): within the block a repeated S.trilinear call
    on the same grid and points returns the first call's result"""
    plain, seen = S.trilinear, {}

    def once(grid, p):
        key = (id(grid), np.asarray(p, F32).tobytes())
        if key not in seen:
            seen[key] = plain(grid, p)
        return seen[key]
    S.trilinear = once
    try:
        yield
    finally:
        S.trilinear = plain


def rows_of(grid, points, y, T, max_distance, color_scale, max_color_residual=0.0):
    """-> (rows [n,16] float32: j[6], s, used, jc[6], rcs, colored; reason [n] as R.rows_of; colored [n] bool; rc [n] float32, zero unless coloured)"""
    with _samples_taken_once():
        return _rows_of(grid, points, y, T, max_distance, color_scale, max_color_residual)


def _rows_of(grid, points, y, T, max_distance, color_scale, max_color_residual):
    rows8, reason = R.rows_of(grid, points, T, max_distance)
    n = len(rows8)
    rows = np.zeros((n, 16), F32)
    rows[:, :8] = rows8
    colored, rc = np.zeros(n, bool), np.zeros(n, F32)
    if color_scale > 0:
        p = S.transform_points(T, points)
        y = np.asarray(y, F32).reshape(-1)
        cs = F32(color_scale)
        m, g = model_intensity(grid, p)
        with np.errstate(all="ignore"):
            r = m - y
            gate = np.abs(r) <= F32(max_color_residual) if max_color_residual > 0 else np.ones(n, bool)
            colored = (reason == 0) & np.isfinite(y) & gate
            jc = np.stack([cs * g[:, 0], cs * g[:, 1], cs * g[:, 2],
                           cs * (p[:, 1] * g[:, 2] - p[:, 2] * g[:, 1]),
                           cs * (p[:, 2] * g[:, 0] - p[:, 0] * g[:, 2]),
                           cs * (p[:, 0] * g[:, 1] - p[:, 1] * g[:, 0])], axis=1).astype(F32)
            rcs = cs * r
        rows[colored, 8:14] = jc[colored]
        rows[colored, 14] = rcs[colored]
        rows[colored, 15] = 1.0
        rc[colored] = r[colored]
    return rows, reason, colored, rc


def terms_of(rows, rc):
    """the 30 terms of every used row, float64 [k,30], and how many non-zero terms each slot holds per row [k,30]"""
    u = rows[:, 7] != 0
    r, rc = rows[u], np.asarray(rc, F32)[u]
    if not len(r):
        return np.zeros((0, 30)), np.zeros((0, 30), int)
    j, s, jc, rcs, col = r[:, :6], r[:, 6], r[:, 8:14], r[:, 14], r[:, 15] != 0
    d = lambda v: v.astype(np.float64)
    z = lambda v: np.where(col, d(v), 0.0)
    t = [d(j[:, a] * j[:, b]) + z(jc[:, a] * jc[:, b]) for a, b in PAIRS]
    t += [d(s * j[:, a]) + z(rcs * jc[:, a]) for a in range(6)]
    t.append(d(s) * d(s) + np.where(col, d(rcs) * d(rcs), 0.0))
    t.append(np.where(col, d(rc) * d(rc), 0.0))
    t.append(d(s) * d(s))
    return np.stack(t, axis=1), col


def fold(rows, reason, colored, rc):
    """-> (sums [30] by math.fsum, the rounding bound of each slot [30], counts dict).
    The bound: slot k is a sum of k_n doubles, each the rounded sum of a geometric and a colour term; an addition order of k_n terms is within
    (k_n - 1) 2^-53 sum |term| of the exact sum of the terms (first order), and the terms themselves are rounded once where a colour term was added
    (2^-53 |term|)."""
    t, col = terms_of(rows, rc)
    sums = np.array([math.fsum(t[:, k]) for k in range(30)])
    mags = np.array([math.fsum(np.abs(t[:, k])) for k in range(30)])
    n_terms = np.array([len(t)] * 28 + [int(col.sum()) if len(t) else 0, len(t)])
    bound = np.maximum(n_terms - 1, 0) * 2.0 ** -53 * mags
    counts = {name: int((reason == k).sum()) for k, name in enumerate(R.COUNT_NAMES)}
    counts["colored"] = int(np.asarray(colored).sum())
    return sums, bound, counts


def system(grid, points, y, T, max_distance, color_scale, max_color_residual=0.0):
    rows, reason, colored, rc = rows_of(grid, points, y, T, max_distance, color_scale, max_color_residual)
    sums, _b, counts = fold(rows, reason, colored, rc)
    return sums, counts


def rmse_color(sums, colored):
    return math.sqrt(sums[28] / colored) if colored else 0.0


def rmse_geometric(sums, used):
    return math.sqrt(sums[29] / used) if used else 0.0


def loop(lib, evaluate, init_T, max_iterations, min_step=0.0, min_points=6, trace=None):
    """op_volume_register_color_points' host loop: R.loop's (the same solve, exponential, product, stop rules and statuses) around
    evaluate(T) -> (sums [30], counts dict with `colored`) -> dict of the result's fields, base fields by their own names.
    trace: a list that receives (T, counts, sdf rmse, colour rmse, |x|) per iteration."""
    T = np.asarray(init_T, F32).reshape(4, 4).copy()
    res = {"iterations": 0, "status": R.MAX_ITERATIONS, "last_step": 0.0}
    first, current = None, None
    for _it in range(max_iterations):
        current = evaluate(T)
        sums, counts = current
        first = first or current
        if counts["used"] < max(min_points, 0):
            res["status"] = R.TOO_FEW_POINTS
            break
        x, E = R.solve_step(lib, sums)
        if not np.isfinite(x).all():
            res["status"] = R.SINGULAR
            break
        ss = sum(float(v) * float(v) for v in x)
        if trace is not None:
            trace.append((T.copy(), dict(counts), rmse_geometric(sums, counts["used"]), rmse_color(sums, counts["colored"]), math.sqrt(ss)))
        T = R.mul4(E, T)
        current = None
        res["iterations"] += 1
        res["last_step"] = math.sqrt(ss)
        if ss < float(F32(min_step)) * float(F32(min_step)):
            res["status"] = R.CONVERGED
            break
    if current is None:
        current = evaluate(T)
    if first is None:
        first = current
        if current[1]["used"] < max(min_points, 0):
            res["status"] = R.TOO_FEW_POINTS
    sums, counts = current
    res.update(counts)
    res.update(T=T, rmse=rmse_geometric(sums, counts["used"]), first_used=first[1]["used"], first_rmse=rmse_geometric(first[0], first[1]["used"]),
               first_colored=first[1]["colored"], rmse_color=rmse_color(sums, counts["colored"]),
               first_rmse_color=rmse_color(first[0], first[1]["colored"]))
    return res


def jtj_eigenvalues(sums):
    JTJ = np.zeros((6, 6))
    for k, (a, b) in enumerate(PAIRS):
        JTJ[a, b] = JTJ[b, a] = sums[k]
    return np.linalg.eigvalsh(JTJ)


_scene = {}


def color_scene(oracle):
    """the sliding scene, fused by the oracle -> dict(frames, keys, vox, grid, cloud / y: every third of the eight frames' hit points in world
    coordinates with the intensity of their pixels, frame3 / y3: every hit point of frame 3, init)"""
    if not _scene:
        fr = D.frames(COL_CAM, COL_FRAMES, stride=COL_STRIDE)
        vol = oracle.Volume(oracle.make_camera(*COL_CAM), voxel_res=COL_RES, trunc=TRUNC)
        for f in fr:
            vol.integrate(*f)
        keys, vox = vol.export()
        pts, ys = [], []
        for depth, rgb, pose in fr:
            hit, p = S.hit_points(pose, COL_CAM, depth)
            pts.append(p)
            ys.append(intensity_of_bytes(rgb)[hit])
        _scene.update(frames=fr, keys=keys, vox=vox, grid=S.Grid(keys, vox, COL_RES),
                      cloud=np.ascontiguousarray(np.concatenate(pts)[::3], F32), y=np.ascontiguousarray(np.concatenate(ys)[::3], F32),
                      frame3=np.ascontiguousarray(pts[3], F32), y3=np.ascontiguousarray(ys[3], F32), init=D.perturbed(np.eye(4), 1))
    return _scene


# ---- the hand-made field of volume_register_common with all three colour planes 0.5 + x at the voxel centres ---------------------------------
ISUM = (F32(0.114) * F32(1.0) + F32(0.587) * F32(1.0)) + F32(0.299) * F32(1.0)      # I(1, 1, 1) as the formula rounds it


def hand_blocks():
    vox = R.hand_blocks()
    centres = S.block_voxel_centres(R.HAND_KEYS, R.HAND_RES)
    vox[..., 2:] = (F32(0.5) + centres[..., 0])[..., None]
    return vox


MIX_PATTERN = (0, 0, 1, 0, 2, 0, 3, 0)                                # the reason wanted at index i % 8


def mixed_cloud(grid, keys, res, cloud, y, T, max_distance, n=4097, seed=9):
    """n points with intensities in which, at pose T, every class occurs within every 32 consecutive indices: a pool -- `cloud` with its
    intensities `y`, S.query_mix's jittered voxel centres with the model's own intensity, NaN, +-1e9 -- is classified by the RESTATEMENT's reason
    and dealt out by MIX_PATTERN; of the used points' intensities index 1 mod 16 is NaN, 7 mod 32 infinite (used, not coloured) and 3 mod 16 half
    a unit off (gated by any max_color_residual below 0.4)."""
    rng = np.random.default_rng(seed)
    mix = S.query_mix(keys, res, n=3 * n, seed=seed)
    special = np.array([(np.nan, 0.1, 0.1), (1e9, 0.1, 0.1), (0.1, -1e9, 0.1), (0.1, 0.1, 1e9)], F32)
    order = rng.permutation(len(cloud))[:2 * n]
    pool = np.concatenate([np.asarray(cloud, F32)[order], mix, np.tile(special, (8, 1))]).astype(F32)
    _rows, reason = R.rows_of(grid, pool, T, max_distance)
    by_reason = [np.flatnonzero(reason == k) for k in range(4)]
    assert all(len(b) > 0 for b in by_reason), [len(b) for b in by_reason]
    taken = [0, 0, 0, 0]
    pick = np.empty(n, np.int64)
    for i in range(n):
        k = MIX_PATTERN[i % 8]
        pick[i] = by_reason[k][taken[k] % len(by_reason[k])]
        taken[k] += 1
    pts = np.ascontiguousarray(pool[pick])
    with np.errstate(all="ignore"):
        m, _g = model_intensity(grid, S.transform_points(T, pts))
    yy = np.where(np.isfinite(m), m, F32(0.5)).astype(F32)
    from_cloud = pick < len(order)                                   # those keep the frame's own intensity
    yy[from_cloud] = np.asarray(y, F32)[order[pick[from_cloud]]]
    idx = np.arange(n)
    yy[idx % 16 == 1] = np.nan
    yy[idx % 16 == 3] += F32(0.5)
    yy[idx % 32 == 7] = np.inf
    return pts, np.ascontiguousarray(yy)
