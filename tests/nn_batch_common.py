"""Shared by tests/test_nn_batch_cpu.py and tests/test_nn_batch_gpu.py: the planted clouds, the numpy restatement of the distance and of the
example's label loop, and the calls into examples/cpp/LabelTransfer.bin (the class surface: --path host is the loop of KnnSearch(q, ..., 1)
over a finished op_host::NanoTree and touches no device, --path device forwards to the index).

The distance is nanoflann's L2_Simple_Adaptor in float32: d = 0; d += dx*dx; d += dy*dy; d += dz*dz (0 + x is x, so ((dx*dx + dy*dy) + dz*dz))."""
import json
import os
import subprocess

import numpy as np

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "examples", "cpp", "LabelTransfer.bin")
INF = float("inf")
DOUBT_REL = f32(2.0 ** -15)   # kDoubtRel of onepiece_amd/csrc/nn_batch.hip


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint16)


def dist2(targets, queries):
    """[n, m] float32 squared distances, every product and sum rounded on its own"""
    d = queries[:, None, :].astype(f32) - targets[None, :, :].astype(f32)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def dist2_of(targets, queries, idx):
    """the distance of every query to the target it was given (+inf where idx is -1)"""
    out = np.full(len(queries), np.inf, f32)
    ok = idx >= 0
    d = queries[ok].astype(f32) - targets[idx[ok]].astype(f32)
    out[ok] = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return out


def brute_force(targets, queries, max_sq_dist=INF):
    """-> (idx, d2, runner_up): the minimum over (distance, index), -1 / inf at or beyond the cutoff, and the second smallest distance"""
    n = len(queries)
    if len(targets) == 0:
        return np.full(n, -1, np.int32), np.full(n, np.inf, f32), np.full(n, np.inf, f32)
    idx, best, second = np.empty(n, np.int32), np.empty(n, f32), np.full(n, np.inf, f32)
    for s in range(0, n, 512):
        d = dist2(targets, queries[s:s + 512])
        idx[s:s + 512] = d.argmin(axis=1)
        if d.shape[1] > 1:
            part = np.partition(d, 1, axis=1)
            best[s:s + 512], second[s:s + 512] = part[:, 0], part[:, 1]
        else:
            best[s:s + 512] = d[:, 0]
    miss = ~(best < f32(max_sq_dist))
    runner = second.copy()
    idx[miss], best[miss] = -1, np.inf
    return idx, best, runner


def reported(best, runner_up):
    """what k_nn_query hands to the host: runner-up equal to the best (tied), or within DOUBT_REL of it (doubtful)"""
    found = np.isfinite(best)
    tied = found & (runner_up == best)
    doubtful = found & ~tied & (runner_up <= best + best * DOUBT_REL)
    return tied, doubtful


def transfer_ref(targets, labels, queries, max_sq_dist, default_label):
    """example/GetLabelUsingKDTree.cpp:49-60 with the nearest neighbour by brute force; the planted clouds of its users have no ties"""
    idx, best, runner = brute_force(targets, queries, max_sq_dist)
    assert not (np.isfinite(runner) & (runner == best) & (idx >= 0)).any(), "the cloud has ties: brute force does not say what the tree picks"
    out = np.full(len(queries), default_label, np.asarray(labels).dtype)
    out[idx >= 0] = np.asarray(labels)[idx[idx >= 0]]
    return out, idx


# ---- planted clouds ------------------------------------------------------------------------------------------------------------------------
def uniform_cloud():
    rng = np.random.default_rng(20261)
    return rng.uniform(0, 1, (2000, 3)).astype(f32), rng.uniform(0, 1, (4097, 3)).astype(f32)


def outside_queries():
    rng = np.random.default_rng(20262)
    q = rng.uniform(0, 1, (257, 3)).astype(f32)
    side = rng.integers(0, 3, 257)
    q[np.arange(257), side] += rng.choice([-60.0, 45.0], 257).astype(f32)  # far beyond the unit cube along one axis
    q[::5] += f32(30)                                                        # and along all three
    return q


def one_cell_cloud():
    rng = np.random.default_rng(20263)  # a small cluster far from the origin: the cell cannot be finer than 2^-12 of 1000
    t = (1000 + rng.uniform(0, 0.01, (300, 3))).astype(f32)
    q = (1000 + rng.uniform(-0.02, 0.03, (200, 3))).astype(f32)
    return t, q


def two_clusters():
    rng = np.random.default_rng(20264)
    t = rng.uniform(0, 1, (600, 3)).astype(f32)
    t[300:, 0] += f32(1000)
    q = rng.uniform(0, 1, (500, 3)).astype(f32)
    q[:, 0] = rng.uniform(-100, 1100, 500).astype(f32)  # along the empty stretch between the clusters, and beyond both
    return t, q


def lattice():
    """integer lattice 8 x 8 x 8, every target twice; queries with one, two or three half-integer coordinates: 2 x 2-, 4- and 8-way ties"""
    rng = np.random.default_rng(20265)
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 3).astype(f32)
    t = np.concatenate([g, g])[rng.permutation(1024)]
    base = rng.integers(0, 7, (300, 3)).astype(f32)
    halves = np.zeros((300, 3), f32)
    for i in range(300):
        halves[i, rng.permutation(3)[:1 + i % 3]] = 0.5
    return np.ascontiguousarray(t), base + halves


def quantised():
    rng = np.random.default_rng(20266)
    return (rng.integers(0, 65, (2000, 3)) / 64.0).astype(f32), (rng.integers(0, 65, (4096, 3)) / 64.0).astype(f32)


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------
def run_driver(args, timeout=120):
    assert os.path.exists(DRIVER), "examples/cpp/LabelTransfer.bin is not built (make -C examples/cpp)"
    r = subprocess.run([DRIVER] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, "LabelTransfer %s: exit %d\n%s\n%s" % (" ".join(map(str, args)), r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def raw_run(tmp, path, steps, max_sq_dist=INF, labels=None, labels16=None, default_label=0):
    """steps: [("cloud", array) | ("batch", array), ...] in order -> (per batch (idx, dist, labels or None, labels16 or None), result.json)"""
    tmp = str(tmp)
    os.makedirs(tmp, exist_ok=True)
    args = ["--path", path, "--dump", tmp, "--max-dist", "inf" if max_sq_dist == INF else repr(float(max_sq_dist)), "--default", default_label]
    for k, (kind, a) in enumerate(steps):
        f = os.path.join(tmp, "in_%d.f32" % k)
        np.ascontiguousarray(a, f32).tofile(f)
        args += ["--" + kind, f]
    if labels is not None:
        np.ascontiguousarray(labels, np.int32).tofile(os.path.join(tmp, "labels.i32"))
        args += ["--labels", os.path.join(tmp, "labels.i32")]
    if labels16 is not None:
        np.ascontiguousarray(labels16, np.uint16).tofile(os.path.join(tmp, "labels.u16"))
        args += ["--labels16", os.path.join(tmp, "labels.u16")]
    js = run_driver(args)
    out = []
    for b in range(sum(1 for kind, _ in steps if kind == "batch")):
        tag = os.path.join(tmp, "batch_%d" % b)
        out.append((np.fromfile(tag + "_idx.i32", np.int32), np.fromfile(tag + "_dist.f32", f32),
                    np.fromfile(tag + "_labels.i32", np.int32) if labels is not None else None,
                    np.fromfile(tag + "_labels.u16", np.uint16) if labels16 is not None else None))
    return out, js
