"""Inputs and float32 restatements shared by test_global_registration_cpu.py and test_global_registration_gpu.py.

Inputs are built deterministically from onepiece_amd.synthetic (nothing is read from disk):
  room_clouds()        two views of the synthetic room, each in its own camera frame, voxel-grid down-sampled at 0.05 m
  adversarial_cloud()  a lattice (exact distance ties), exact duplicates (dist == 0), one isolated point (m - 1 == 0) and a clump of more than
                       1000 points inside one 27-cell neighbourhood (the top-knn selection has to cut)
The restatements follow host/one_piece/src/GlobalRegistration.cpp and RansacRigid.cpp in numpy float32, elementwise (one rounding per
operation, no fused multiply-add), in the operand order written there.
"""
import json
import os
import subprocess

import numpy as np

from helpers import room_cloud
from onepiece_amd import synthetic as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(ROOT, "examples", "cpp", "GlobalRegistration.bin")
KNN, RADIUS, VOXEL = 100, 0.25, 0.05     # DenseSlam.h:49-68 (the radius is compared with squared distances)
ROOM_FRAMES = (100, 130)                 # source, target: 10.8 degrees of the orbit apart
F = np.float32


def downsample(points, normals, voxel=VOXEL):
    """One point per occupied cell of edge `voxel`: the mean of its points and the normalised mean of its normals, cells in order of first
    appearance (a test INPUT: what matters is that it is deterministic and a few thousand points)."""
    keep = np.isfinite(points).all(1) & (points[:, 2] > 0)
    points, normals = points[keep].astype(np.float64), normals[keep].astype(np.float64)
    cells = np.floor(points / voxel).astype(np.int64)
    _, first, inverse = np.unique(cells, axis=0, return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    order = np.argsort(np.argsort(first))          # rank of every unique cell by first appearance
    slot = order[inverse]
    count = np.bincount(slot).astype(np.float64)
    p = np.stack([np.bincount(slot, points[:, k]) / count for k in range(3)], axis=1)
    nrm = np.stack([np.bincount(slot, normals[:, k]) for k in range(3)], axis=1)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-12)
    return p.astype(F), nrm.astype(F)


def room_clouds():
    out = []
    for i in ROOM_FRAMES:
        _depth, p, n = room_cloud(i, scale=2)
        out.append(downsample(p, n))
    return out


def room_motion():
    """source camera -> target camera"""
    return np.linalg.inv(S.room_pose(ROOM_FRAMES[1]).astype(np.float64)) @ S.room_pose(ROOM_FRAMES[0]).astype(np.float64)


def adversarial_cloud():
    rng = np.random.default_rng(20240607)
    g = np.arange(14, dtype=F) * F(0.125)                                          # 14^3 lattice, spacing 1/8: exact ties in every direction
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    clump = (F(3.0) + rng.random((1200, 3)).astype(F) * F(0.3)).astype(F)          # 1200 points in a 0.3 m cube: all within one neighbourhood
    dup = np.concatenate([lattice[100:140], clump[:40]])                           # exact duplicates of points that come earlier
    lone = np.array([[40.0, -30.0, 25.0]], F)                                      # no neighbour within the radius
    pts = np.concatenate([lattice, clump, dup, lone]).astype(F)
    nrm = rng.normal(size=pts.shape)
    nrm[0:len(lattice):3] = [0.0, 0.0, 1.0]                                        # opposed axis-aligned normals on a lattice: theta = +-pi exactly,
    nrm[1:len(lattice):3] = [0.0, 0.0, -1.0]                                       # pairs ON the wrap between bins 10 and 0
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return pts, nrm.astype(F)


def write_ply(path, points, normals):
    rec = np.concatenate([points, normals], axis=1).astype("<f4")
    with open(path, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                 "property float nx\nproperty float ny\nproperty float nz\nend_header\n" % len(rec)).encode())
        f.write(rec.tobytes())


def run_example(args, dump, timeout=600):
    os.makedirs(dump, exist_ok=True)
    run = subprocess.run([EXAMPLE] + list(args) + ["--dump", dump], capture_output=True, text=True, timeout=timeout)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "[ERROR]" not in run.stdout, run.stdout[-3000:]
    return load_dump(dump)


def load_dump(dump):
    d = {"json": json.load(open(os.path.join(dump, "result.json")))}
    for name in os.listdir(dump):
        stem, ext = os.path.splitext(name)
        if ext == ".f32":
            d[stem] = np.fromfile(os.path.join(dump, name), "<f4")
        elif ext == ".i32":
            d[stem] = np.fromfile(os.path.join(dump, name), "<i4")
    for tag in ("source", "target"):
        n = len(d[tag + "_points"]) // 3
        for k in ("points", "normals"):
            d[tag + "_" + k] = d[tag + "_" + k].reshape(n, 3)
        for k in ("spfh", "fpfh"):
            d[tag + "_" + k] = d[tag + "_" + k].reshape(n, 33)
        d[tag + "_neighbours"] = d[tag + "_neighbours"].reshape(n, -1)
    return d


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def pair_analysis(points, normals, neighbours, tol=1e-6):
    """For every (point, neighbour-list slot >= 1): is the pair FLAGGED -- does the first angle sit within `tol` bins of a bin boundary?
    The operands of the atan2 are formed in float32 exactly as ComputePairDescriptor forms them (the host's atan2f and a correctly rounded
    atan2 see the same two floats and differ by at most one ulp of the angle); from those, x = 11 (theta + pi) / (2 pi) in float64.
    -> (flagged [n,knn] bool, m [n] list lengths, each [n] the integer increment 100 // (m - 1), w [n,knn] float32 1/dist of the second pass)"""
    n, knn = neighbours.shape
    valid = neighbours >= 0
    valid[:, 0] = False
    q = np.where(neighbours >= 0, neighbours, 0)
    with np.errstate(all="ignore"):
        ps, u = points[:, None, :], np.broadcast_to(normals[:, None, :], (n, knn, 3))
        pt, nt = points[q], normals[q]
        delta = pt - ps
        distance = np.sqrt(_dot(delta, delta))
        direction = delta / distance[..., None]
        v = _cross(u, direction)
        degenerate = np.sqrt(_dot(v, v)) == 0
        w = _cross(u, v)
        theta = np.arctan2(_dot(w, nt).astype(np.float64), _dot(u, nt).astype(np.float64))
        x = 11.0 * (theta + np.pi) / (2.0 * np.pi)
        near = np.abs(x - np.round(x)) < tol          # the integers 0 and 11 are the +-pi wrap
        back = ps - pt
        dist2 = np.sqrt(_dot(back, back))
        weight = np.where(dist2 > 0, F(1) / dist2, F(0)).astype(F)
    flagged = valid & near & ~degenerate & np.isfinite(x)
    m = (neighbours >= 0).sum(1)
    each = np.where(m > 1, 100 // np.maximum(m - 1, 1), 0)
    return flagged, m, each, np.where(valid, weight, F(0))


def cyclic_moves(delta):
    """The fewest moves of one unit between ADJACENT bins (0 and 10 adjacent) that produce the integer difference `delta` [11]; None if the
    units do not balance."""
    if delta.sum() != 0:
        return None
    c = np.cumsum(delta)
    return int(np.abs(c - int(np.median(c))).sum())


def check_features(host, dev, tag, enforce_shares):
    """Rules 1-3 of the feature stage for one cloud of two dumps.  -> dict of the measured shares"""
    P, N = host[tag + "_points"], host[tag + "_normals"]
    assert np.array_equal(P.view(np.uint32), dev[tag + "_points"].view(np.uint32)) and np.array_equal(N.view(np.uint32), dev[tag + "_normals"].view(np.uint32))
    nb_h, nb_d = host[tag + "_neighbours"], dev[tag + "_neighbours"]
    assert nb_h.shape == nb_d.shape
    bad = np.nonzero((nb_h != nb_d).any(1))[0]
    assert len(bad) == 0, "neighbour lists differ on %d points, first %d: host %s device %s" % (len(bad), bad[0], nb_h[bad[0]], nb_d[bad[0]])
    flagged, m, each, w = pair_analysis(P, N, nb_h)
    k = flagged.sum(1)
    sh, sd = host[tag + "_spfh"], dev[tag + "_spfh"]
    # thirds 2 and 3: bit-identical everywhere
    assert np.array_equal(sh[:, 11:].view(np.uint32), sd[:, 11:].view(np.uint32)), "SPFH thirds 2/3 differ"
    differs = (sh[:, :11].view(np.uint32) != sd[:, :11].view(np.uint32)).any(1)
    assert not (differs & (k == 0)).any(), "SPFH third 1 differs on %d points without a flagged pair" % (differs & (k == 0)).sum()
    moved = np.zeros(len(P), np.int64)
    for i in np.nonzero(differs)[0]:
        diff = sd[i, :11].astype(np.float64) - sh[i, :11].astype(np.float64)
        assert each[i] > 0 and np.all(diff % each[i] == 0), (i, diff, each[i])
        moves = cyclic_moves((diff / each[i]).astype(np.int64))
        assert moves is not None and moves <= k[i], "point %d: %s needs %s moves of %d, %d flagged pairs" % (i, diff, moves, each[i], k[i])
        moved[i] = moves
    # FPFH: untainted points bit-identical; tainted ones within what their flagged pairs can move
    q = np.where(nb_h >= 0, nb_h, 0)
    neighbour_flagged = ((k[q] > 0) & (nb_h >= 0))
    neighbour_flagged[:, 0] = False
    tainted = (k > 0) | neighbour_flagged.any(1)
    fh, fd = host[tag + "_fpfh"], dev[tag + "_fpfh"]
    same = (fh.view(np.uint32) == fd.view(np.uint32))
    assert same[~tainted].all(), "FPFH differs on %d untainted points" % (~same[~tainted].all(1)).sum()
    assert same[:, 11:].all(), "FPFH thirds 2/3 differ"
    # third 1 of a tainted point: acc[b] changes by at most sum_q w_q each_q k_q, times the third's scale 100 / sum (unchanged: a move keeps
    # a histogram's total), plus the point's own moved increments; float32 accumulation of <= m non-negative terms adds (m + 2) ulps of the value
    third_sum = np.where(w > 0, sh[:, :11].astype(np.float64).sum(1)[q], 0.0).sum(1)
    scale = np.where(third_sum != 0, 100.0 / np.where(third_sum != 0, third_sum, 1.0), 0.0)
    swing = (w.astype(np.float64) * (each[q] * k[q])).sum(1) * scale + each * k
    slack = 2.0 * (m + 2) * 2.0 ** -24 * (np.abs(fh[:, :11]).max(1) + swing)
    err = np.abs(fd[:, :11].astype(np.float64) - fh[:, :11].astype(np.float64)).max(1)
    worst = np.argmax(err - (swing + slack))
    assert np.all(err <= swing + slack), "FPFH of point %d off by %g, bound %g" % (worst, err[worst], (swing + slack)[worst])
    shares = {"points": int(len(P)), "flagged_points": int((k > 0).sum()), "flagged_share": float((k > 0).mean()), "tainted_share": float(tainted.mean()),
              "spfh_points_that_differ": int(differs.sum()), "fpfh_points_that_differ": int((~same.all(1)).sum())}
    print(tag, shares)
    if enforce_shares:
        assert shares["flagged_share"] <= 0.01, shares
        assert shares["tainted_share"] <= 0.05, shares
    return shares


def feature_match_reference(src, tgt):
    """FeatureMatching3D's scan: d2 summed over the 33 bins in order in float32, the first minimum."""
    if len(tgt) == 0:
        return np.full(len(src), -1, np.int32)
    out = np.empty(len(src), np.int32)
    for lo in range(0, len(src), 512):
        s = src[lo:lo + 512]
        d2 = np.zeros((len(s), len(tgt)), F)
        for b in range(33):
            e = s[:, b, None] - tgt[None, :, b]
            d2 += e * e
        out[lo:lo + 512] = np.argmin(d2, axis=1)
    return out


def inlier_reference(src, tgt, Ts, threshold):
    """RansacRigid.cpp::Inlier for every (hypothesis, pair) in float32 -> bool [H, n]"""
    T = np.asarray(Ts, F).reshape(-1, 12)
    sx, sy, sz = (src[None, :, k] for k in range(3))
    d = []
    for r in range(3):
        a, b, c, t = (T[:, 4 * r + k, None] for k in range(4))
        d.append(((a * sx + b * sy) + c * sz) + t - tgt[None, :, r])
    return np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) < F(threshold)
