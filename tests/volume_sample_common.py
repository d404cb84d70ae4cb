"""op_volume_sample restated in numpy float32 (test infrastructure shared by tests/test_volume_sample_cpu.py and tests/test_volume_sample_gpu.py).

The definition is the header's (include/onepiece_hip.h, op_volume_sample): both modes, the gradient, the status bits and the statistics, over an
export (keys [m,3] int32, voxels [m,512,5] float32).  Every product, sum and quotient is ONE float32 operation of numpy, in the definition's
order; nothing is contracted.  tests/test_volume_sample_cpu.py pins this file to the committed oracle's raycast and transform.
"""
import math

import numpy as np

F32 = np.float32
DEFAULT_VOXEL = np.array([999.0, 0.0, -1.0, -1.0, -1.0], F32)
TRILINEAR, REFERENCE = 0, 1
INVALID, NO_GRADIENT, OUT_OF_RANGE = 1, 2, 4
LIMIT = F32(8388600.0)
STAT_NAMES = ("queries", "valid", "gradients", "out_of_range", "sum_abs_sdf", "sum_sq_sdf", "max_abs_sdf")


class Grid:
    """block id -> row of the export, as a dense table over the bounding box of the keys"""

    def __init__(self, keys, vox, res):
        self.keys = np.asarray(keys, np.int64).reshape(-1, 3)
        self.vox = np.ascontiguousarray(vox, F32).reshape(-1, 512, 5)
        self.res = F32(res)
        if len(self.keys):
            self.lo = self.keys.min(axis=0)
            self.ext = self.keys.max(axis=0) - self.lo + 1
        else:
            self.lo, self.ext = np.zeros(3, np.int64), np.ones(3, np.int64)
        self.table = np.full(tuple(self.ext), -1, np.int64)
        if len(self.keys):
            k = self.keys - self.lo
            self.table[k[:, 0], k[:, 1], k[:, 2]] = np.arange(len(self.keys))

    def fetch(self, p):
        """voxels at the integer voxel coordinates p [n,3] -> (held [n] bool, voxels [n,5]; the default voxel where the block is not held)"""
        p = np.asarray(p, np.int64)
        b = (p >> 3) - self.lo                                        # floor division by 8
        inside = ((b >= 0) & (b < self.ext)).all(axis=1)
        bc = np.where(inside[:, None], b, 0)
        row = np.where(inside, self.table[bc[:, 0], bc[:, 1], bc[:, 2]], -1)
        held = row >= 0
        vid = (p[:, 0] & 7) + (p[:, 1] & 7) * 8 + (p[:, 2] & 7) * 64
        out = np.broadcast_to(DEFAULT_VOXEL, (len(p), 5)).copy()
        if len(self.vox):
            out[held] = self.vox[row[held], vid[held]]
        return held, out


def transform_points(T, pts):
    """q = ((m0 x + m1 y) + m2 z) + m3 * 1 per row, p = q.xyz / q.w (TransformPoints' order)"""
    M = np.asarray(T, F32).reshape(4, 4)
    p = np.asarray(pts, F32).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        q = [((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] * F32(1.0) for r in range(4)]
        return np.stack([q[0] / q[3], q[1] / q[3], q[2] / q[3]], axis=1).astype(F32)


def _in_range(g):
    with np.errstate(all="ignore"):
        return (np.abs(g) < LIMIT).all(axis=1)                        # False for NaN


def trilinear(grid, p):
    """-> (valid [n], out_of_range [n], sums [n,5]: the five planes accumulated in tap order; meaningful where valid)"""
    p = np.asarray(p, F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        inv = F32(1.0) / grid.res
        g = p * inv - F32(0.5)
        ok = _in_range(g)
        g = np.where(ok[:, None], g, F32(0.0))
        b = np.floor(g)
        i = b.astype(np.int64)
        f = g - b
        valid = ok.copy()
        acc = np.zeros((len(p), 5), F32)
        for k in range(8):
            bit = np.array([k & 1, (k >> 1) & 1, (k >> 2) & 1])
            held, t = grid.fetch(i + bit)
            valid &= held & (t[:, 1] > 0)                             # NaN and negative weights are unobserved
            w3 = [f[:, a] if bit[a] else F32(1.0) - f[:, a] for a in range(3)]
            w = (w3[0] * w3[1]) * w3[2]
            acc = acc + w[:, None] * t
    return valid, ~ok, acc


def gradient(grid, p):
    """d_a = s(p + h e_a) - s(p - h e_a), h = 0.5 res -> (d [n,3], zero unless all six samples are valid; ok [n])"""
    p = np.asarray(p, F32).reshape(-1, 3)
    h = F32(0.5) * grid.res
    d = np.zeros((len(p), 3), F32)
    ok = np.ones(len(p), bool)
    with np.errstate(all="ignore"):
        for a in range(3):
            pp, pm = p.copy(), p.copy()
            pp[:, a] = p[:, a] + h
            pm[:, a] = p[:, a] - h
            vp, _o, sp = trilinear(grid, pp)
            vm, _o, sm = trilinear(grid, pm)
            ok &= vp & vm
            d[:, a] = sp[:, 0] - sm[:, 0]
    d[~ok] = 0
    return d, ok


def normalised(d, ok):
    """the raycaster's normal from the difference: d / sqrt(d0 d0 + (d1 d1 + d2 d2)), zero unless ok and the length is positive"""
    with np.errstate(all="ignore"):
        l2 = d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        good = ok & (l2 > 0)
        n = d / np.sqrt(l2)[:, None]
    return np.where(good[:, None], n, F32(0.0)).astype(F32)


def _scale(a, wgt):                                                   # TSDFVoxel::operator*(float)
    dflt = (wgt == 0) | (a[:, 1] == 0)
    return np.where(dflt[:, None], DEFAULT_VOXEL, a * wgt[:, None]).astype(F32)


def _add(a, b):                                                       # TSDFVoxel::add
    r = a + b
    r = np.where((b[:, 1] == 0)[:, None], a, r)
    return np.where((a[:, 1] == 0)[:, None], b, r).astype(F32)


def _stage(a, b, t):                                                  # one lerp stage of ReadVoxelInterpolate
    empty = ~((a[:, 1] != 0) | (b[:, 1] != 0))
    s = _add(_scale(a, F32(1.0) - t), _scale(b, t))
    d = (F32(1.0) - t) * (a[:, 1] != 0).astype(F32) + t * (b[:, 1] != 0).astype(F32)
    r = _scale(s, F32(1.0) / d)
    return np.where(empty[:, None], DEFAULT_VOXEL, r).astype(F32)


def reference(grid, p):
    """ReadVoxelInterpolate as k_transform_fill evaluates it -> (out_of_range [n], voxel [n,5])"""
    p = np.asarray(p, F32).reshape(-1, 3)
    res = grid.res
    with np.errstate(all="ignore"):
        half = res / F32(2.0)
        n = p - half
        e = n / res
        ok = _in_range(e)
        p0 = np.floor(np.where(ok[:, None], e, F32(0.0))).astype(np.int64)
        w = (n - p0.astype(F32) * res) / res
        v = [grid.fetch(p0 + np.array([k & 1, (k >> 1) & 1, (k >> 2) & 1]))[1] for k in range(8)]
        xw, yw, zw = w[:, 0], w[:, 1], w[:, 2]
        z1 = _stage(_stage(v[0], v[1], xw), _stage(v[2], v[3], xw), yw)
        z2 = _stage(_stage(v[4], v[5], xw), _stage(v[6], v[7], xw), yw)
        r = _stage(z1, z2, zw)
    r[~ok] = DEFAULT_VOXEL
    return ~ok, r


def sample(keys, vox, res, points, T=None, mode=TRILINEAR, gradients=False, grid=None):
    """op_volume_sample -> {"voxels" [n,5], "status" [n] uint8, "gradients" [n,3] or None, "stats" dict}"""
    grid = grid if grid is not None else Grid(keys, vox, res)
    p = np.asarray(points, F32).reshape(-1, 3)
    if T is not None:
        p = transform_points(T, p)
    status = np.zeros(len(p), np.uint8)
    grad = None
    if mode == TRILINEAR:
        valid, oor, acc = trilinear(grid, p)
        out = np.where(valid[:, None], acc, DEFAULT_VOXEL).astype(F32)
        status[~valid] |= INVALID
        status[oor] |= OUT_OF_RANGE
        if gradients:
            grad, ok = gradient(grid, p)
            ok &= ~oor
            grad[~ok] = 0
            status[~ok] |= NO_GRADIENT
    else:
        assert not gradients
        oor, out = reference(grid, p)
        status[(out[:, 1] == 0) | oor] |= INVALID
        status[oor] |= OUT_OF_RANGE
    good = (status & INVALID) == 0
    s = out[good, 0].astype(np.float64)
    stats = {"queries": len(p), "valid": int(good.sum()), "gradients": int(((status & NO_GRADIENT) == 0).sum()) if gradients else 0,
             "out_of_range": int(oor.sum()), "sum_abs_sdf": math.fsum(np.abs(s)), "sum_sq_sdf": math.fsum(s * s),
             "max_abs_sdf": float(np.abs(out[good, 0]).max()) if good.any() else 0.0}
    return {"voxels": out, "status": status, "gradients": grad, "stats": stats}


def hit_points(pose, camt, depth):
    """the raycaster's hit points: dcx = (u - cx) / fx, d_r = (P_r0 dcx + P_r1 dcy) + P_r2, p_r = P_r3 + depth d_r -> (pixel mask [h,w], points [k,3])"""
    P = np.asarray(pose, F32).reshape(4, 4)
    fx, fy, cx, cy, w, h = F32(camt[0]), F32(camt[1]), F32(camt[2]), F32(camt[3]), camt[4], camt[5]
    depth = np.asarray(depth, F32).reshape(h, w)
    u, v = np.meshgrid(np.arange(w, dtype=F32), np.arange(h, dtype=F32))
    dcx, dcy = (u - cx) / fx, (v - cy) / fy
    hit = depth > 0
    pts = np.stack([P[r, 3] + depth * ((P[r, 0] * dcx + P[r, 1] * dcy) + P[r, 2]) for r in range(3)], axis=-1).astype(F32)
    return hit, pts[hit]


def block_voxel_centres(keys, res):
    """centre of voxel i of block k, as Transform forms it: ((float)k * 8) * res + ((float)i * res + res / 2) -> [m,512,3], voxel index x + 8y + 64z"""
    res = F32(res)
    keys = np.asarray(keys, np.int32).reshape(-1, 3)
    vid = np.arange(512)
    loc = np.stack([vid & 7, (vid >> 3) & 7, vid >> 6], axis=1).astype(F32)
    start = (keys.astype(F32) * F32(8.0)) * res
    return (start[:, None, :] + (loc[None, :, :] * res + res / F32(2.0))).astype(F32)


def query_mix(keys, res, n=4097, seed=3):
    """n queries: voxel centres of held blocks plus uniform jitter of +-1.5 voxels"""
    rng = np.random.default_rng(seed)
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    b = keys[rng.integers(0, len(keys), n)]
    vox = rng.integers(0, 8, (n, 3))
    jit = rng.uniform(-1.5, 1.5, (n, 3))
    return (((b * 8 + vox) + 0.5 + jit) * float(res)).astype(F32)
