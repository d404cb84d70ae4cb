"""op_volume_coarsen restated in numpy float32 (test infrastructure shared by tests/test_volume_coarsen_cpu.py and tests/test_volume_coarsen_gpu.py).

The definition is the header's (include/onepiece_hip.h, op_volume_coarsen): result block B = source blocks 2B + {0,1}^3, coarse voxel g = the fine
voxels 2g + (i, j, k) visited in the order c = i + 2j + 4k; a child contributes iff w > 0 && w >= min_weight; W, S and C_m are accumulated from
0.0f over the contributing children in that order, every product and every sum ONE float32 operation of numpy (a Python loop over c: no np.sum
over the child axis); sdf = S / W, colour = C / W, weight = W * 0.125f; the default voxel where nothing contributes.

Also the crafted volume both test files use (crafted()): 17 blocks of 3 cm voxels that hold every case the definition names."""
import numpy as np

import volume_sample_common as S

F32 = np.float32
STAT_NAMES = ("src_blocks", "dst_blocks", "voxels_full", "voxels_partial", "voxels_empty", "dropped_min_weight")


def sort_blocks(keys, vox):
    """blocks in (x, y, z) order of their ids, as CubeHandler.GetCubeMap returns them"""
    keys = np.asarray(keys, np.int32).reshape(-1, 3)
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    return keys[order], np.ascontiguousarray(vox, F32).reshape(-1, 512, 5)[order]


def _coarsen(keys, vox, min_weight):
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    vox = np.ascontiguousarray(vox, F32).reshape(-1, 512, 5)
    mw = F32(min_weight)
    keys2 = np.unique(keys >> 1, axis=0) if len(keys) else np.zeros((0, 3), np.int64)      # arithmetic shift; rows sorted (x, y, z)
    nd = len(keys2)
    row = {tuple(k): r for r, k in enumerate(keys.tolist())}
    # the 16^3 fine voxels under every result block, [block, z, y, x, 5]; the default voxel where the source block is missing
    fine = np.broadcast_to(S.DEFAULT_VOXEL, (nd, 16, 16, 16, 5)).copy()
    for d, (bx, by, bz) in enumerate(keys2.tolist()):
        for cz in (0, 1):
            for cy in (0, 1):
                for cx in (0, 1):
                    r = row.get((2 * bx + cx, 2 * by + cy, 2 * bz + cz))
                    if r is not None:
                        fine[d, 8 * cz:8 * cz + 8, 8 * cy:8 * cy + 8, 8 * cx:8 * cx + 8] = vox[r].reshape(8, 8, 8, 5)
    shape = (nd, 8, 8, 8)
    W, Sd = np.zeros(shape, F32), np.zeros(shape, F32)
    Cm = [np.zeros(shape, F32) for _ in range(3)]
    n, dropped = np.zeros(shape, np.int64), 0
    with np.errstate(all="ignore"):
        for c in range(8):                                            # c = i + 2j + 4k ascending
            i, j, k = c & 1, (c >> 1) & 1, c >> 2
            ch = fine[:, k::2, j::2, i::2]
            w, s = ch[..., 1], ch[..., 0]
            use = (w > 0) & (w >= mw)                                 # False for NaN
            W = np.where(use, W + w, W).astype(F32)
            Sd = np.where(use, Sd + w * s, Sd).astype(F32)
            for m in range(3):
                Cm[m] = np.where(use, Cm[m] + w * ch[..., 2 + m], Cm[m]).astype(F32)
            n += use
            dropped += int(((w > 0) & ~use).sum())
        some = n > 0
        out = np.broadcast_to(S.DEFAULT_VOXEL, shape + (5,)).copy()
        out[..., 0] = np.where(some, Sd / W, F32(999.0))
        out[..., 1] = np.where(some, W * F32(0.125), F32(0.0))
        for m in range(3):
            out[..., 2 + m] = np.where(some, Cm[m] / W, F32(-1.0))
    stats = {"src_blocks": len(keys), "dst_blocks": nd, "voxels_full": int((n == 8).sum()), "voxels_partial": int(((n > 0) & (n < 8)).sum()),
             "voxels_empty": int((n == 0).sum()), "dropped_min_weight": dropped}
    return keys2.astype(np.int32), out.reshape(nd, 512, 5).astype(F32), stats, n.reshape(nd, 512)


def coarsen(keys, vox, res, min_weight=0.0):
    """one level -> (keys2 [m,3] int32 sorted (x, y, z), vox2 [m,512,5] float32, stats dict); the result's voxel size is float32(2) * res"""
    keys2, vox2, stats, _n = _coarsen(keys, vox, min_weight)
    return keys2, vox2, stats


def coarsen_levels(keys, vox, res, levels, min_weight=0.0):
    """`levels` applications, one after the other -> (keys, vox, res, the last level's stats)"""
    stats = None
    for _l in range(levels):
        keys, vox, stats = coarsen(keys, vox, res, min_weight)
        res = F32(2.0) * F32(res)
    return keys, vox, res, stats


def child_counts(keys, vox, min_weight=0.0):
    """-> {coarse global voxel (x, y, z): contributing children} for every voxel of every result block"""
    keys2, _v, _s, n = _coarsen(keys, vox, min_weight)
    vid = np.arange(512)
    loc = np.stack([vid & 7, (vid >> 3) & 7, vid >> 6], axis=1)
    return {tuple((8 * k + l).tolist()): int(c) for k, row in zip(keys2.astype(np.int64), n) for l, c in zip(loc, row)}


# ---- the crafted volume ------------------------------------------------------------------------------------------------------------------
CRAFT_RES = 0.03
CRAFT_WEIGHTS = np.array([0, 0.125, 0.5, 1, 3, 1000], F32)
OCTET = [(x, y, z) for z in (0, 1) for y in (0, 1) for x in (0, 1)]                       # all eight children of result block (0, 0, 0)
LONE = (4, 4, 4)                                                                          # result block (2, 2, 2): its seven siblings are missing
SIGNED = [(-3, -3, -3), (-2, -2, -2), (-1, -1, -1), (-3, 0, 1), (1, -2, -1), (0, 1, -3), (-1, -3, 0), (-2, -1, 1)]   # with the octet: -3..1 on every axis
CRAFT_KEYS = np.array(OCTET + [LONE] + SIGNED, np.int32)
# coarse global voxels of result block (0, 0, 0) with planted children: (voxel, eight weights in the order c, children at min_weight 0, at 1)
PLANTED = [
    ((1, 1, 1), (0, 0, 0, 0, 0, 0, 0, 0), 0, 0),
    ((2, 1, 1), (0, 0, 0, 1, 0, 0, 0, 0), 1, 1),
    ((3, 1, 1), (3, 1, 0.5, 0, 1000, 0.125, 1, 3), 7, 5),            # min_weight 1 removes some of its children ...
    ((5, 5, 5), (3, 3, 3, 3, 3, 3, 3, 3), 8, 8),
    ((1, 2, 3), (0.5, 0.125, 0.5, 0.5, 0.125, 0.125, 0.5, 0.5), 8, 0),  # ... and all of this one's
    ((6, 2, 5), (1000, 0.125, 1, 1, 1, 1, 1, 1), 8, 7),              # a weight that swallows a small one
]


def _set_children(keys, vox, g, weights, rng):
    row = {tuple(k): r for r, k in enumerate(keys.tolist())}
    for c, w in enumerate(weights):
        f = (2 * g[0] + (c & 1), 2 * g[1] + ((c >> 1) & 1), 2 * g[2] + (c >> 2))
        r = row[(f[0] >> 3, f[1] >> 3, f[2] >> 3)]
        v = (f[0] & 7) + 8 * (f[1] & 7) + 64 * (f[2] & 7)
        vox[r, v, 1] = w
        if w == 0:
            vox[r, v, 0] = (np.nan, np.inf, 999.0)[c % 3]
            vox[r, v, 2:] = -1.0
        else:
            vox[r, v, 0] = F32(rng.uniform(-0.09, 0.09))
            vox[r, v, 2:] = rng.uniform(0, 1, 3).astype(F32)


_crafted = {}


def crafted(seed=11):
    """-> (keys [17,3] int32, vox [17,512,5] float32): weights from CRAFT_WEIGHTS; a weight-0 voxel holds NaN, +inf or 999 as sdf and -1 as colours;
    the PLANTED voxels hold exactly the child counts listed (checked here, through the restatement's own predicate)"""
    if seed not in _crafted:
        rng = np.random.default_rng(seed)
        keys = CRAFT_KEYS.copy()
        m = len(keys)
        assert m <= 27 and len({tuple(k) for k in keys.tolist()}) == m
        for a in range(3):
            assert set(keys[:, a].tolist()) >= {-3, -2, -1, 0, 1}
        assert not any(tuple(k) in {tuple(q) for q in keys.tolist()} for k in
                       [(LONE[0] + x, LONE[1] + y, LONE[2] + z) for z in (0, 1) for y in (0, 1) for x in (0, 1) if (x, y, z) != (0, 0, 0)])
        vox = np.empty((m, 512, 5), F32)
        vox[..., 0] = rng.uniform(-0.09, 0.09, (m, 512)).astype(F32)
        vox[..., 1] = CRAFT_WEIGHTS[rng.integers(0, len(CRAFT_WEIGHTS), (m, 512))]
        vox[..., 2:] = rng.uniform(0, 1, (m, 512, 3)).astype(F32)
        zero = vox[..., 1] == 0
        vox[..., 0][zero] = np.array([np.nan, np.inf, 999.0], F32)[rng.integers(0, 3, int(zero.sum()))]
        vox[..., 2:][zero] = -1.0
        for g, weights, _n0, _n1 in PLANTED:
            _set_children(keys, vox, g, weights, rng)
        for mw, col in ((0.0, 2), (1.0, 3)):
            counts = child_counts(keys, vox, mw)
            for p in PLANTED:
                assert counts[p[0]] == p[col], (p, mw, counts[p[0]])
        assert set(np.unique(vox[..., 1]).tolist()) == set(CRAFT_WEIGHTS.tolist())
        assert np.isnan(vox[..., 0]).any() and np.isinf(vox[..., 0]).any() and (vox[..., 0] == 999).any()
        _crafted[seed] = (keys, vox)
    k, v = _crafted[seed]
    return k.copy(), v.copy()


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same_blocks(got_keys, got_vox, want_keys, want_vox):
    """blocks matched by key (pool order is not part of the contract); every voxel bit for bit -> number of differing voxels"""
    gk, gv = sort_blocks(got_keys, got_vox)
    wk, wv = sort_blocks(want_keys, want_vox)
    assert np.array_equal(gk, wk), "block ids differ: %d against %d blocks" % (len(gk), len(wk))
    return int((bits(gv) != bits(wv)).any(axis=-1).sum())
