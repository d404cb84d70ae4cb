"""Garbage collection without a GPU: the restatement's pool-order rule (tests/collect_garbage_common.py) against a brute-force version that
moves one block at a time, the share of empty blocks the pose-correction scenario leaves behind (the oracle plus deintegrate_common), and the new
entry's surface (OP_ERR_NO_DEVICE without a device; a C++ translation unit that calls the new CubeHandler members compiles and links)."""
import ctypes as C
import os
import subprocess

import numpy as np

import collect_garbage_common as G
import deintegrate_common as D


def brute_force_order(flags):
    """One block at a time: while a dropped slot lies below the number of kept blocks, the lowest such slot takes the block of the lowest kept slot
    at or above that number which has not moved yet.  -> (src per final slot, moves)"""
    keep = [f == G.KEPT for f in flags]
    m = sum(keep)
    slots = list(range(len(keep)))                                    # slots[i] = the original slot of the block now in slot i (None: freed)
    live = list(keep)
    moves = 0
    while True:
        hole = next((i for i in range(m) if not live[i]), None)
        if hole is None:
            break
        tail = next(i for i in range(m, len(keep)) if live[i])
        slots[hole], live[hole], live[tail], slots[tail] = slots[tail], True, False, None
        moves += 1
    assert all(live[:m]) and not any(live[m:])
    return slots[:m], moves


def _check_order(flags):
    flags = np.asarray(flags, np.uint8)
    src, moved = G.pool_order(flags)
    want, moves = brute_force_order(flags.tolist())
    assert src.tolist() == want and moved == moves, flags.tolist()
    st = G.stats_of(flags)
    assert st["blocks_before"] == len(flags) and st["blocks_kept"] == len(src) and st["blocks_moved"] == moved
    assert st["blocks_kept"] + st["removed_outside"] + st["removed_unobserved"] == len(flags)
    kept = np.flatnonzero(flags == G.KEPT)
    assert sorted(src.tolist()) == kept.tolist()                      # a permutation of the kept blocks
    stay = kept[kept < len(src)]
    assert np.array_equal(src[stay], stay)                            # kept blocks below m stay where they are
    return moved


def test_pool_order_rule_against_one_block_at_a_time():
    K, U, O = G.KEPT, G.UNOBSERVED, G.OUTSIDE
    assert _check_order([]) == 0                                      # n = 0
    assert _check_order([K] * 9) == 0                                 # all kept
    assert _check_order([U] * 5 + [O] * 4) == 0                       # none kept
    assert _check_order([U] * 69 + [K]) == 1                          # one kept, in the last slot
    assert _check_order([U, O, U] + [K] * 7) == 3                     # all holes in the head
    assert _check_order([K] * 7 + [U, O, U]) == 0                     # all holes in the tail
    assert _check_order([U, K] * 35) == 18                            # alternating, 70 slots: m = 35, holes 0, 2, .., 34, tails 35, 37, .., 69
    rng = np.random.default_rng(20261019)
    moved = 0
    for n in list(range(1, 40)) + [70, 127, 128, 129, 1023, 1024, 1025, 2500]:
        for p in (0.1, 0.5, 0.9):
            flags = np.where(rng.random(n) < p, G.KEPT, rng.integers(1, 3, n)).astype(np.uint8)
            moved += _check_order(flags)
    assert moved > 500


def test_alternating_count():
    # [U, K] * 35: kept slots are the odd ones, m = 35; dropped slots below 35 are 0, 2, .., 34 = 18; kept at or above 35 are 35, 37, .., 69 = 18
    src, moved = G.pool_order(np.array([G.UNOBSERVED, G.KEPT] * 35, np.uint8))
    assert moved == 18 and src[0] == 35 and src[34] == 69 and src[1] == 1


def test_keep_flags_predicate_and_box():
    vox = np.broadcast_to(D.DEFAULT_VOXEL, (8, 512, 5)).copy()
    keys = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [4, 0, 0], [5, 0, 0], [-1, 2, 7], [1, 1, 1]], np.int32)
    vox[1, 3, 1] = 1.0
    vox[2, 511, 1] = 3.0
    vox[3, 0, 1] = np.nan
    vox[4, 100, 1] = -2.0
    vox[5, 7, 1] = 0.5
    vox[6, 9, 1] = np.inf
    vox[7, 64, 1] = 2.0
    K, U, O = G.KEPT, G.UNOBSERVED, G.OUTSIDE
    assert G.keep_flags(keys, vox).tolist() == [U, K, K, U, U, K, K, K]
    assert G.keep_flags(keys, vox, 1.0).tolist() == [U, K, K, U, U, U, K, K]
    assert G.keep_flags(keys, vox, 2.0).tolist() == [U, U, K, U, U, U, K, K]
    assert G.keep_flags(keys, vox, 3.5).tolist() == [U, U, U, U, U, U, K, U]
    assert G.keep_flags(keys, vox, 0.0, ([1, 0, 0], [3, 1, 1])).tolist() == [O, K, K, U, O, O, O, K]   # inclusive on both ends
    assert G.keep_flags(keys, vox, 0.0, ([2, 0, 0], [1, 0, 0])).tolist() == [O] * 8                    # lo > hi: nothing is inside
    k2, v2, st = G.collect(keys, vox, 2.0)
    assert k2.tolist() == [[-1, 2, 7], [1, 1, 1], [2, 0, 0]] and st == dict(zip(G.STAT_NAMES, (8, 3, 0, 5, 2)))
    assert np.array_equal(v2[0].view(np.uint32), vox[6].view(np.uint32)) and np.array_equal(v2[2].view(np.uint32), vox[2].view(np.uint32))


def test_the_pose_correction_scenario_leaves_a_tenth_of_its_blocks_empty(oracle):
    """20 frames at CAM_64 into 2 cm voxels, every 4th moved to a perturbed pose and back: the oracle plus the de-integration restatement."""
    before, keys, vox, _m = G.scenario_model(oracle)
    flags = G.keep_flags(keys, vox)
    empty = int((flags == G.UNOBSERVED).sum())
    whole = int(D.is_default(vox).all(axis=1).sum())
    print("pose-correction scenario: %d blocks after fusion, %d after the repair, %d with no voxel of weight > 0 (%.1f %%), %d of them all-default"
          % (before, len(keys), empty, 100.0 * empty / len(keys), whole))
    assert len(keys) > before
    assert empty >= 0.10 * len(keys)
    assert (flags == G.OUTSIDE).sum() == 0
    fk, fv, _ = G.filtered(keys, vox)
    assert len(fk) == len(keys) - empty and (fv[..., 1] > 0).any(axis=1).all()


def test_new_entry_fails_loudly_without_a_device(hip):
    import torch
    lib = hip.load()
    st = hip.CollectStats()
    lo = (C.c_int32 * 3)(0, 0, 0)
    if torch.cuda.is_available():                                     # with a device the same call gets as far as its null volume
        assert lib.op_volume_collect_garbage(None, 0.0, None, None, C.byref(st)) == hip.OP_ERR_INVALID
        return
    for rc in (lib.op_volume_collect_garbage(None, 0.0, None, None, C.byref(st)), lib.op_volume_collect_garbage(None, -1.0, lo, None, None),
               lib.op_volume_collect_last_stats(None, C.byref(st))):
        assert rc == hip.OP_ERR_NO_DEVICE and b"no CPU fallback" in lib.op_last_error()
    from onepiece_amd import integration as I
    assert callable(I.CubeHandler.CollectGarbage)


def test_a_translation_unit_that_calls_the_new_members_compiles_and_links(hip, tmp_path):
    src = open(os.path.join(G.ROOT, "tests", "cpp", "collect_garbage_check.cpp")).read()
    for call in ("CollectGarbage()", "CollectGarbage(2.f)", "CropToCubes(", "CollectStats()"):
        assert call in src
    exe = G.build_check(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True)      # the usage line: the binary starts (no GPU needed)
    assert out.returncode == 0 and "usage" in out.stdout
