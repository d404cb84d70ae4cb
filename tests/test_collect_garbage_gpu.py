"""CubeHandler::CollectGarbage on the device (csrc/volume_gc.hip; op_volume_collect_garbage) against the numpy restatement of its definition
(tests/collect_garbage_common.py) over volumes that come from the oracle plus the de-integration restatement (deintegrate_common.Model) or from
hand-made blocks -- never from the code under test: which blocks go, the pool order afterwards slot by slot, every voxel bit, the statistics,
and what fusion, growth and the volume's consumers make of the collected volume.

Shapes: 70 hand-made blocks (one upload call each, so pool slot = call order); the room at 37 x 29 into 4 cm voxels and at 64 x 48 into 2 cm
voxels (the pose-correction scenario: 20 frames, 5 of them moved to a perturbed pose and back; 1275 blocks, 212 of them empty)."""
import struct
import subprocess

import numpy as np
import pytest

import collect_garbage_common as G
import deintegrate_common as D
from onepiece_amd import integration as I

pytestmark = pytest.mark.gpu

F32 = np.float32
_cache = {}


def _handler(camt, trunc=0.1, res=D.RES, max_blocks=1 << 13):
    hcam = I.PinholeCamera()
    hcam.fx, hcam.fy, hcam.cx, hcam.cy, hcam.width, hcam.height, hcam.depth_scale = camt
    hv = I.CubeHandler(hcam, device=0, max_blocks=max_blocks)
    hv.SetVoxelResolution(res)
    hv.SetTruncation(trunc)
    return hv


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same(got, want, what, ordered=True):
    """keys and every voxel bit; ordered: slot by slot (both in pool order), otherwise both sorted by key"""
    (gk, gv), (wk, wv) = got, want
    assert gk.shape == np.asarray(wk).shape and np.array_equal(gk, wk), "block keys differ %s" % what
    diff = (_bits(gv) != _bits(wv)).any(axis=-1)
    assert not diff.any(), "%d voxels differ %s" % (int(diff.sum()), what)


# ---- hand-made blocks ----------------------------------------------------------------------------------------------------------------
N_PLANTED = 70
PLANTED_KEYS = np.array([[i % 5 - 2, (i // 5) % 4 - 1, i // 20 - 2] for i in range(N_PLANTED)], np.int32)


def _planted(holes):
    """70 blocks; slot i is a hole (all-default; the first hole holds only a NaN weight, the second only a weight of -2) iff holes[i], otherwise
    it holds ~40 observed voxels with integer weights up to 1 (even live blocks) or 3 (odd ones)"""
    rng = np.random.default_rng(7)
    vox = np.broadcast_to(D.DEFAULT_VOXEL, (N_PLANTED, 512, 5)).copy()
    n_hole = n_live = 0
    for i in range(N_PLANTED):
        if holes[i]:
            if n_hole == 0:
                vox[i, 300, 1] = np.nan
            elif n_hole == 1:
                vox[i, 511, 1] = -2.0
            n_hole += 1
            continue
        top = 1.0 if n_live % 2 == 0 else 3.0
        at = rng.choice(512, 40, replace=False)
        vox[i, at, 0] = rng.uniform(-0.1, 0.1, 40).astype(F32)
        vox[i, at, 1] = rng.integers(1, int(top) + 1, 40).astype(F32)
        vox[i, at[0], 1] = top                                        # the block's largest weight, at a random voxel (any lane of the wave)
        vox[i, at, 2:] = rng.random((40, 3)).astype(F32)
        n_live += 1
    return vox


PATTERNS = {
    "holes in the head": [i < 20 for i in range(N_PLANTED)],
    "holes in the tail": [i >= 50 for i in range(N_PLANTED)],
    "alternating": [i % 2 == 0 for i in range(N_PLANTED)],
    "none": [False] * N_PLANTED,
    "all": [True] * N_PLANTED,
    "one live block in the last slot": [i != N_PLANTED - 1 for i in range(N_PLANTED)],
    "mixed": [(i * 7) % 10 < 4 for i in range(N_PLANTED)],
}


def _upload_in_slot_order(vox, keys=PLANTED_KEYS):
    hv = _handler(D.CAM_37)
    for i in range(len(keys)):
        hv.AddCubes(keys[i:i + 1], vox[i:i + 1])                      # one block per call: pool slot = call order
    _same(hv.GetCubeMap(sort=False), (keys, vox), "after the uploads (pool slot = call order)")
    return hv


def _upload_at_once(vox, keys=PLANTED_KEYS):
    """one upload call for all blocks (quick); the pool order is then whatever the insert made of it, so it is read back: the blocks must be the
    planted ones, and the expected collection starts from that order -> (handler, keys in pool order, the planted voxels in pool order)"""
    hv = _handler(D.CAM_37)
    hv.AddCubes(keys, vox)
    pk, pv = hv.GetCubeMap(sort=False)
    row = {tuple(k): i for i, k in enumerate(keys.tolist())}
    assert len(pk) == len(keys) and sorted(map(tuple, pk.tolist())) == sorted(row)
    order = np.array([row[tuple(k)] for k in pk.tolist()])
    _same((pk, pv), (keys[order], vox[order]), "after the upload")
    return hv, keys[order], vox[order]


def _check_collected(hv, keys, vox, min_weight, box, what):
    want_k, want_v, want_st = G.collect(keys, vox, min_weight, box)
    st = hv.CollectGarbage(min_weight, box)
    print("%s: %s (restatement %s)" % (what, st, want_st))
    _same(hv.GetCubeMap(sort=False), (want_k, want_v), what)
    assert hv.BlockCount() == want_st["blocks_kept"] == len(want_k)
    assert st == want_st
    import ctypes as C
    from onepiece_amd import _lib as L
    last = L.CollectStats()
    L.check(L.load().op_volume_collect_last_stats(hv._h, C.byref(last)))
    assert {k: int(getattr(last, k)) for k in G.STAT_NAMES} == want_st  # the volume remembers what its last collection did
    kept = {tuple(k) for k in want_k.tolist()}
    for k in keys.tolist():
        assert hv.HasCube(k) == (tuple(k) in kept), (what, k)
    return st


@pytest.mark.parametrize("pattern", [p for p in PATTERNS if p != "mixed"])
def test_01_planted_holes_by_position(pattern):
    vox = _planted(PATTERNS[pattern])
    hv = _upload_in_slot_order(vox)
    st = _check_collected(hv, PLANTED_KEYS, vox, 0.0, None, pattern)
    n_holes = sum(PATTERNS[pattern])
    assert st["removed_unobserved"] == n_holes and st["removed_outside"] == 0
    assert st["blocks_moved"] == {"holes in the head": 20, "holes in the tail": 0, "alternating": 18, "none": 0, "all": 0, "one live block in the last slot": 1}[pattern]


@pytest.mark.parametrize("min_weight", [0.0, 1.0, 2.0, 3.5])
def test_02_min_weight(min_weight):
    holes = PATTERNS["mixed"]
    vox = _planted(holes)
    hv = _upload_in_slot_order(vox)
    st = _check_collected(hv, PLANTED_KEYS, vox, min_weight, None, "min_weight %g" % min_weight)
    odd_live = sum(1 for i, k in enumerate(np.flatnonzero(~np.array(holes))) if i % 2 == 1)
    live = N_PLANTED - sum(holes)
    assert st["blocks_kept"] == {0.0: live, 1.0: live, 2.0: odd_live, 3.5: 0}[min_weight]
    nan_block, neg_block = np.flatnonzero(holes)[:2]
    assert np.isnan(vox[nan_block, :, 1]).any() and (vox[neg_block, :, 1] == -2).any()
    assert not hv.HasCube(PLANTED_KEYS[nan_block]) and not hv.HasCube(PLANTED_KEYS[neg_block])


def test_03_crop():
    import ctypes as C
    from onepiece_amd import _lib as L
    vox = _planted(PATTERNS["mixed"])
    boxes = {"inclusive bounds": ([0, -1, -2], [1, 2, 0]), "a single block id": ([1, 2, 0], [1, 2, 0]), "holds nothing": ([50, 50, 50], [60, 60, 60]),
             "lo > hi on one axis": ([-2, 1, -2], [2, -1, 1]), "everything": ([-2, -1, -2], [2, 2, 1])}
    for what, box in boxes.items():
        if what == "inclusive bounds":
            hv, pk, pv = _upload_in_slot_order(vox), PLANTED_KEYS, vox
        else:
            hv, pk, pv = _upload_at_once(vox)
        st = _check_collected(hv, pk, pv, 0.0, box, "crop, " + what)
        lo, hi = np.array(box[0]), np.array(box[1])
        inside = ((PLANTED_KEYS >= lo) & (PLANTED_KEYS <= hi)).all(axis=1)
        assert st["removed_outside"] == int((~inside).sum())          # an unobserved block outside the box counts as outside
        assert st["removed_unobserved"] == int((inside & np.array(PATTERNS["mixed"])).sum())
        if what in ("holds nothing", "lo > hi on one axis"):
            assert st["blocks_kept"] == 0 and st["removed_outside"] == N_PLANTED
        if what == "inclusive bounds":
            got = hv.GetCubeMap()[0]
            assert 0 < st["blocks_kept"] < inside.sum() and (got == lo).all(axis=1).any() and (got == hi).all(axis=1).any()   # both corners are live blocks
        if what == "everything":
            assert st["removed_outside"] == 0
    # refusals: the volume is untouched
    hv, pk, pv = _upload_at_once(vox)
    lib, lo = L.load(), (C.c_int32 * 3)(-2, -1, -2)
    st = L.CollectStats()
    assert lib.op_volume_collect_garbage(hv._h, 0.0, lo, None, C.byref(st)) == L.OP_ERR_INVALID
    assert lib.op_volume_collect_garbage(hv._h, 0.0, None, lo, C.byref(st)) == L.OP_ERR_INVALID
    for bad in (-1.0, float("nan"), float("inf")):
        assert lib.op_volume_collect_garbage(hv._h, bad, None, None, None) == L.OP_ERR_INVALID
        with pytest.raises(L.OnePieceHipError):
            hv.CollectGarbage(bad)
    _same(hv.GetCubeMap(sort=False), (pk, pv), "after the refused calls")
    assert lib.op_volume_collect_garbage(hv._h, 0.0, None, None, None) == L.OP_OK      # stats may be NULL
    assert hv.BlockCount() == N_PLANTED - sum(PATTERNS["mixed"])


# ---- the pose-correction scenario ----------------------------------------------------------------------------------------------------
def _repaired_volume():
    """the scenario on the device, nothing collected yet; no accessor is called: the last frames are still queued"""
    fr = G.scenario_frames()
    hv = _handler(G.SCENARIO_CAM, G.SCENARIO_TRUNC, G.SCENARIO_RES)
    for f in fr:
        hv.IntegrateImage(*f)
    for i in G.SCENARIO_MOVED:
        away = D.perturbed(fr[i][2], i)
        hv.ReintegrateImage(fr[i][0], fr[i][1], fr[i][2], away)
        hv.ReintegrateImage(fr[i][0], fr[i][1], away, fr[i][2])
    return hv


def _scenario_expected(oracle):
    _before, keys, vox, m = G.scenario_model(oracle)
    fk, fv, flags = G.filtered(keys, vox)
    return keys, vox, fk, fv, int((flags == G.UNOBSERVED).sum()), m


def test_04_pose_correction_scenario(oracle):
    keys, vox, fk, fv, empties, _m = _scenario_expected(oracle)
    assert empties >= 0.10 * len(keys)
    hv = _repaired_volume()
    st = hv.CollectGarbage()
    print("scenario: %s" % st)
    assert st["blocks_before"] == len(keys) and st["removed_unobserved"] == empties and st["removed_outside"] == 0 and st["blocks_kept"] == len(fk)
    _same(hv.GetCubeMap(), (fk, fv), "after CollectGarbage()")


def test_10_idempotence(oracle):
    keys, vox, fk, fv, empties, _m = _scenario_expected(oracle)
    hv = _repaired_volume()
    first = hv.CollectGarbage()
    assert first["removed_unobserved"] == empties and first["blocks_moved"] > 0
    k1, v1 = hv.GetCubeMap(sort=False)
    second = hv.CollectGarbage()
    assert second == dict(zip(G.STAT_NAMES, (len(fk), len(fk), 0, 0, 0)))
    k2, v2 = hv.GetCubeMap(sort=False)
    assert k1.tobytes() == k2.tobytes() and v1.tobytes() == v2.tobytes()


def _tri_set(pts, col):
    from volume_golden_common import sorted_bits
    return sorted_bits(np.concatenate([pts.reshape(-1, 9), col.reshape(-1, 9)], axis=1)) if len(pts) else np.zeros((0, 18), np.uint32)


def test_07_consumers_do_not_notice_pure_collection(oracle, tmp_path):
    from helpers import procedural_mc_table, MC_EDGE_PAIRS
    from volume_golden_common import map_blocks, sorted_bits
    keys, _vox, fk, _fv, empties, _m = _scenario_expected(oracle)
    fr = G.scenario_frames()
    views = [fr[3][2], fr[14][2]]
    hv = _repaired_volume()
    tab = procedural_mc_table()

    def look(name):
        out = {}
        out["mesh"] = _tri_set(*hv.ExtractTriangleMesh(tab, MC_EDGE_PAIRS))
        p, c = hv.GetPointCloud()
        out["cloud"] = sorted_bits(np.concatenate([p, c], axis=1))
        path = tmp_path / (name + ".map")
        hv.WriteToFile(path)
        out["file"] = map_blocks(path.read_bytes())
        out["views"] = [[_bits(a).copy() for a in hv.Raycast(p_)] for p_ in views]     # (the raycaster's block summaries exist from here on)
        out["frames"] = [hv.RenderFrame(p_) for p_ in views]
        return out
    before = look("before")
    assert len(before["mesh"]) > 1000 and len(before["cloud"]) > 1000 and all((v[0] != 0).sum() > 500 for v in before["views"])
    st = hv.CollectGarbage()
    assert st["removed_unobserved"] == empties and st["blocks_moved"] > 0
    after = look("after")
    assert np.array_equal(before["mesh"], after["mesh"]), "the mesh soup as a set of triangles"
    assert np.array_equal(before["cloud"], after["cloud"]), "the point cloud as a set"
    assert len(before["file"]) == len(keys) and len(after["file"]) == len(fk)
    assert after["file"] == [b for b in before["file"] if len(b) > 16], "the file's blocks: the same set without the blocks that list no voxel"
    for b, a in zip(before["views"], after["views"]):
        for x, y in zip(b, a):
            assert np.array_equal(x, y), "raycast depth / normal / colour bits"
    for b, a in zip(before["frames"], after["frames"]):
        assert np.array_equal(b[0], a[0]) and np.array_equal(_bits(b[1]), _bits(a[1])) and b[2] == a[2]


def test_11_class_surface(oracle, tmp_path):
    _keys, _vox, fk, fv, empties, _m = _scenario_expected(oracle)
    fr = G.scenario_frames()
    camt = G.SCENARIO_CAM
    exe = G.build_check(tmp_path)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<4i7f", len(fr), camt[4], camt[5], 2 * len(G.SCENARIO_MOVED), camt[0], camt[1], camt[2], camt[3], camt[6], G.SCENARIO_RES, G.SCENARIO_TRUNC))
        for d, c, p in fr:
            f.write(np.ascontiguousarray(d, F32).tobytes() + np.ascontiguousarray(c, np.uint8).tobytes() + np.ascontiguousarray(p, F32).tobytes())
        for i in G.SCENARIO_MOVED:
            away = D.perturbed(fr[i][2], i)
            for a, b in ((fr[i][2], away), (away, fr[i][2])):
                f.write(struct.pack("<i", i) + np.ascontiguousarray(a, F32).tobytes() + np.ascontiguousarray(b, F32).tobytes())
    out = subprocess.run([exe, "gc", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = (tmp_path / "out.bin").read_bytes()
    top = np.frombuffer(raw[:48], np.uint64)
    n = int(top[0])
    gk = np.frombuffer(raw[48:48 + 12 * n], np.int32).reshape(n, 3)
    gv = np.frombuffer(raw[48 + 12 * n:], F32).reshape(n, 512, 5)
    order = np.lexsort((gk[:, 2], gk[:, 1], gk[:, 0]))
    assert top[1:5].tolist() == [len(_keys), len(fk), 0, empties]
    _same((gk[order], gv[order]), (fk, fv), "CubeHandler::CollectGarbage() + GetCubeMap()")


# ---- fusion after a collection -------------------------------------------------------------------------------------------------------
def _frames37(stride=5):
    if ("f37", stride) not in _cache:
        _cache[("f37", stride)] = D.frames(D.CAM_37, 33, stride)
    return _cache[("f37", stride)]


def _collected_then_fused(oracle, trunc, n_first, min_weight, key, stride=5, prepare=None, later=None):
    """the model: (PrepareCubes of frame `prepare`, which allocates its selection and updates nothing, then) n_first frames, the filter, the remaining
    frames of the 33 (or the frames `later`) -> (keys before the filter, flags, final keys, final voxels, model)"""
    if key not in _cache:
        fr = _frames37(stride)
        m = D.Model(oracle, D.CAM_37, trunc)
        if prepare is not None:
            m.vol.prepare_cubes(fr[prepare][0], fr[prepare][2])
        for f in fr[:n_first]:
            m.integrate(f)
        k0, v0 = m.export()
        fk, fv, flags = G.filtered(k0, v0, min_weight)
        m.vol.clear()                                                 # (load assigns blocks, it drops none)
        m.vol.load(fk, fv)
        for f in (fr[n_first:] if later is None else [fr[i] for i in later]):
            m.integrate(f)
        k1, v1 = m.export()
        v1.setflags(write=False)
        _cache[key] = (k0, flags, k1, v1, m)
    return _cache[key]


def _check_fused(hv, exp, what):
    _k0, _flags, k1, v1, m = exp
    _same(hv.GetCubeMap(), (k1, v1), what)
    st = hv.Stats()
    assert (st["frames"], st["blocks_selected"], st["voxels_visited"], st["voxels_updated"]) == (m.entries, m.selected, 512 * m.selected, m.updated)


def test_05_freed_slots_are_fresh(oracle):
    """25 frames, 15 orbit steps apart (at the other tests' 5 only 16 blocks have a largest weight of 1); the blocks only one frame saw lie at the two
    ends of the sweep, so the 8 frames fused after the collection are the first and the last four again"""
    stride, later = 15, [0, 1, 2, 3, 21, 22, 23, 24]
    exp = _collected_then_fused(oracle, 0.1, 25, 2.0, "fresh", stride, later=later)
    k0, flags, k1, _v1, _m = exp
    dropped = {tuple(k) for k in k0[flags != G.KEPT].tolist()}
    recreated = len(dropped & {tuple(k) for k in k1.tolist()})
    print("min_weight 2 drops %d of %d blocks; the 8 later frames re-create %d of them" % (len(dropped), len(k0), recreated))
    assert recreated >= 20
    fr = _frames37(stride)
    hv = _handler(D.CAM_37, 0.1)
    for f in fr[:25]:
        hv.IntegrateImage(*f)
    st = hv.CollectGarbage(min_weight=2.0)
    want = G.stats_of(flags)                                          # (blocks_moved depends on the pool order, which the sorted export does not have)
    assert all(st[k] == want[k] for k in G.STAT_NAMES[:4]) and st["removed_unobserved"] == len(dropped)
    for i in later:
        hv.IntegrateImage(*fr[i])
    _check_fused(hv, exp, "8 frames after collect_garbage(min_weight = 2)")


@pytest.mark.parametrize("trunc", [0.1, 0.6])
def test_06_plain_volume(oracle, trunc):
    """never de-integrated: plain, and lean at truncation 0.1; the collection drops what PrepareCubes selected and nothing updated"""
    exp = _collected_then_fused(oracle, trunc, 20, 0.0, ("plain", trunc))
    k0, flags, _k1, _v1, _m = exp
    fr = _frames37()
    hv = _handler(D.CAM_37, trunc)
    for f in fr[:20]:
        hv.IntegrateImage(*f)
    st = hv.CollectGarbage()
    print("plain volume, truncation %g: %s" % (trunc, st))
    assert (st["blocks_before"], st["blocks_kept"], st["removed_unobserved"]) == (len(k0), int((flags == G.KEPT).sum()), int((flags == G.UNOBSERVED).sum()))
    for f in fr[20:]:
        hv.IntegrateImage(*f)
    _check_fused(hv, exp, "13 frames after CollectGarbage() on a plain volume, truncation %g" % trunc)


def test_06_plain_volume_with_blocks_that_were_selected_and_never_updated(oracle):
    """PrepareCubes of a frame further along the orbit allocates its selection -- the first slots of the pool -- on a volume that stays plain and lean:
    the blocks the 20 frames do not reach go, fused blocks move into their slots, the freed slots are handed out again, and the exact forms of the
    update still give the oracle's bits"""
    exp = _collected_then_fused(oracle, 0.1, 20, 0.0, "prepared", prepare=32)
    k0, flags, k1, v1, m = exp
    empties = int((flags == G.UNOBSERVED).sum())
    assert empties >= 20
    fr = _frames37()
    hv = _handler(D.CAM_37, 0.1)
    hv.PrepareCubes(fr[32][0], fr[32][2])
    for f in fr[:20]:
        hv.IntegrateImage(*f)
    st = hv.CollectGarbage()
    print("plain volume with prepared blocks: %s" % st)
    assert (st["blocks_before"], st["blocks_kept"], st["removed_unobserved"]) == (len(k0), len(k0) - empties, empties)
    assert st["blocks_moved"] >= 20                                   # the empty blocks lie in the head of the pool
    for f in fr[20:]:
        hv.IntegrateImage(*f)
    _same(hv.GetCubeMap(), (k1, v1), "13 frames after CollectGarbage() on a plain volume with prepared blocks")
    assert hv.Stats()["voxels_updated"] == m.updated


def test_06_volume_that_is_no_longer_plain(oracle):
    """after a de-integration the blocks that existed then take the general update (pool slots below plain_from): the collection moves some of them
    to lower slots and frees slots above them, and the frames fused afterwards still give the oracle's bits"""
    fr = _frames37(15)
    moved = (4, 8)
    if "not plain" not in _cache:
        m = D.Model(oracle, D.CAM_37, 0.1)
        for f in fr[:20]:
            m.integrate(f)
        for i in moved:
            away = D.perturbed(fr[i][2], i)
            m.reintegrate(fr[i], away)
            m.reintegrate((fr[i][0], fr[i][1], away), fr[i][2])
        k0, v0 = m.export()
        fk, fv, flags = G.filtered(k0, v0, 2.0)
        m.vol.clear()
        m.vol.load(fk, fv)
        for f in fr[20:]:
            m.integrate(f)
        k1, v1 = m.export()
        v1.setflags(write=False)
        _cache["not plain"] = (k0, flags, k1, v1, m)
    exp = _cache["not plain"]
    k0, flags, _k1, _v1, _m = exp
    assert 20 <= (flags != G.KEPT).sum() < len(k0)
    hv = _handler(D.CAM_37, 0.1)
    for f in fr[:20]:
        hv.IntegrateImage(*f)
    for i in moved:
        away = D.perturbed(fr[i][2], i)
        hv.ReintegrateImage(fr[i][0], fr[i][1], fr[i][2], away)
        hv.ReintegrateImage(fr[i][0], fr[i][1], away, fr[i][2])
    st = hv.CollectGarbage(2.0)
    print("volume that is no longer plain: %s" % st)
    assert (st["blocks_before"], st["blocks_kept"]) == (len(k0), int((flags == G.KEPT).sum()))
    for f in fr[20:]:
        hv.IntegrateImage(*f)
    _check_fused(hv, exp, "13 frames after collect_garbage(2) on a de-integrated volume")


def test_08_queued_frames_are_in_the_result(oracle):
    fr = _frames37()
    m = D.Model(oracle, D.CAM_37, 0.1)
    for f in fr[:5]:
        m.integrate(f)
    k0, v0 = m.export()
    fk, fv, flags = G.filtered(k0, v0, 2.0)
    assert 0 < len(fk) < len(k0)
    hv = _handler(D.CAM_37, 0.1)
    for f in fr[:5]:
        hv.IntegrateImage(*f)                                         # fewer than a batch: nothing is launched before the call
    st = hv.CollectGarbage(2.0)
    assert st["blocks_before"] == len(k0) and st["blocks_kept"] == len(fk)
    _same(hv.GetCubeMap(), (fk, fv), "five queued frames, then collect_garbage(2)")


def test_09_growth_afterwards(oracle):
    exp = _collected_then_fused(oracle, 0.1, 3, 2.0, "growth")
    k0, flags, k1, _v1, _m = exp
    fr = _frames37()
    hv = _handler(D.CAM_37, 0.1, max_blocks=64)
    for f in fr[:3]:
        hv.IntegrateImage(*f)
    st = hv.CollectGarbage(2.0)
    assert st["blocks_kept"] == int((flags == G.KEPT).sum()) and st["blocks_before"] == len(k0)
    g0 = hv.GrowthStats()
    assert len(k1) > g0["max_blocks"], "the remaining frames need more blocks than the pool holds"
    for f in fr[3:]:
        hv.IntegrateImage(*f)
    _check_fused(hv, exp, "fusion that outgrows the pool after a collection")
    g1 = hv.GrowthStats()
    assert g1["grows"] > g0["grows"] and g1["max_blocks"] > g0["max_blocks"]
