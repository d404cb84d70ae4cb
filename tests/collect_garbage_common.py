"""Garbage collection of a volume restated on the CPU (test infrastructure shared by tests/test_collect_garbage_cpu.py and
tests/test_collect_garbage_gpu.py).

The definition (include/onepiece_hip.h, op_volume_collect_garbage): a block is kept iff it is inside the box of block ids (inclusive; no box =
everything is inside) and observed (some voxel has w > 0 and w >= min_weight, float32 compares; NaN and negative weights fail).  With n blocks
before and m kept, a kept block in a slot < m stays; the dropped slots below m, ascending, receive the kept blocks at or above m, ascending.
`keep_flags` is the predicate on an export, `pool_order` the order rule on a flag vector, `collect` both on a volume given in POOL order.
The expected volume itself is always deintegrate_common.Model's export (sorted by key) or a hand-made list of blocks, never the code under test.
"""
import os
import subprocess

import numpy as np

import deintegrate_common as D

F32 = np.float32
KEPT, OUTSIDE, UNOBSERVED = 0, 1, 2
STAT_NAMES = ("blocks_before", "blocks_kept", "removed_outside", "removed_unobserved", "blocks_moved")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def keep_flags(keys, vox, min_weight=0.0, box=None):
    """-> uint8 [n]: KEPT, OUTSIDE or UNOBSERVED per block of (keys [n,3] int32, vox [n,512,5] float32)."""
    keys = np.asarray(keys, np.int32).reshape(-1, 3)
    w = np.asarray(vox, F32).reshape(len(keys), 512, 5)[..., 1]
    with np.errstate(invalid="ignore"):
        observed = ((w > F32(0.0)) & (w >= F32(min_weight))).any(axis=1)
    inside = np.ones(len(keys), bool)
    if box is not None:
        lo, hi = (np.asarray(b, np.int64).reshape(3) for b in box)
        inside = ((keys >= lo) & (keys <= hi)).all(axis=1)
    return np.where(~inside, OUTSIDE, np.where(observed, KEPT, UNOBSERVED)).astype(np.uint8)


def pool_order(flags):
    """The pool-order rule -> (src [m]: the pre-collection slot of the block that ends in slot i, moved)."""
    keep = np.asarray(flags) == KEPT
    n, m = len(keep), int(keep.sum())
    src = np.arange(m, dtype=np.int64)
    holes = np.flatnonzero(~keep[:m])
    tails = m + np.flatnonzero(keep[m:])
    assert len(holes) == len(tails) and m <= n
    src[holes] = tails
    return src, len(holes)


def stats_of(flags):
    flags = np.asarray(flags)
    return dict(zip(STAT_NAMES, (len(flags), int((flags == KEPT).sum()), int((flags == OUTSIDE).sum()), int((flags == UNOBSERVED).sum()), pool_order(flags)[1])))


def collect(keys, vox, min_weight=0.0, box=None):
    """(keys, vox) in POOL order -> (keys', vox', stats) in the pool order the definition prescribes."""
    keys, vox = np.asarray(keys, np.int32).reshape(-1, 3), np.asarray(vox, F32).reshape(-1, 512, 5)
    flags = keep_flags(keys, vox, min_weight, box)
    src, _moved = pool_order(flags)
    return np.ascontiguousarray(keys[src]), np.ascontiguousarray(vox[src]), stats_of(flags)


def filtered(keys, vox, min_weight=0.0, box=None):
    """a key-sorted export with the dropped blocks taken out (still sorted) -> (keys', vox', flags)"""
    flags = keep_flags(keys, vox, min_weight, box)
    return np.ascontiguousarray(np.asarray(keys)[flags == KEPT]), np.ascontiguousarray(np.asarray(vox)[flags == KEPT]), flags


# ---- the pose-correction scenario the issue measured: 20 frames of the room at CAM_64 into 2 cm voxels, truncation 0.1; every 4th frame is
# re-integrated at perturbed(pose, i) and then back at its true pose
SCENARIO_CAM, SCENARIO_RES, SCENARIO_TRUNC, SCENARIO_FRAMES, SCENARIO_MOVED = D.CAM_64, 0.02, 0.1, 20, (0, 4, 8, 12, 16)
_scenario = {}


def scenario_frames():
    if "frames" not in _scenario:
        _scenario["frames"] = D.frames(SCENARIO_CAM, SCENARIO_FRAMES)
    return _scenario["frames"]


def scenario_model(O):
    """-> (blocks after the 20 frames, keys, vox, model) of the repaired volume, computed once (read-only)"""
    if "model" not in _scenario:
        fr = scenario_frames()
        m = D.Model(O, SCENARIO_CAM, SCENARIO_TRUNC, res=SCENARIO_RES)
        for f in fr:
            m.integrate(f)
        before = len(m.export()[0])
        for i in SCENARIO_MOVED:
            away = D.perturbed(fr[i][2], i)
            m.reintegrate(fr[i], away)
            m.reintegrate((fr[i][0], fr[i][1], away), fr[i][2])
        k, v = m.export()
        v.setflags(write=False)
        _scenario["model"] = (before, k, v, m)
    return _scenario["model"]


def build_check(out_dir):
    """compiles tests/cpp/collect_garbage_check.cpp (C++11) against the class surface -> the executable's path"""
    host, lib = os.path.join(ROOT, "host", "one_piece"), os.path.join(ROOT, "onepiece_amd")
    if not os.path.exists(os.path.join(host, "libone_piece_hip_host.so")):
        subprocess.check_call(["make", "-s"], cwd=host)
    exe = os.path.join(str(out_dir), "collect_garbage_check.bin")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I", host, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "collect_garbage_check.cpp"),
                           "-L", host, "-lone_piece_hip_host", "-L", lib, "-lonepiece_hip", "-Wl,-rpath," + host, "-Wl,-rpath," + lib, "-o", exe])
    return exe
