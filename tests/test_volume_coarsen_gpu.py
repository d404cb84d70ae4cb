"""op_volume_coarsen on the device (csrc/volume_coarsen.hip) against the numpy restatement of its definition (tests/volume_coarsen_common.py) over
volumes that are uploaded from hand-made blocks, the crafted blocks and the oracle's fusion -- never from the code under test.  Every comparison
is bit for bit, blocks matched by key: pool order is the allocation pass's and is not part of the contract.

Shapes: 7 hand-made blocks, the 17 crafted blocks (a full octet, a lone block, ids -3..1 on every axis: one to eight claimants per result block, one
and several workgroups), the convergence scene at 2 cm (a few thousand blocks: many waves of claims on one table), a pool of ONE block that has to grow, and 3300 scattered blocks that outgrow the automatic size."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import deintegrate_common as D
import volume_coarsen_common as K
import volume_register_common as R
import volume_sample_common as S
from onepiece_amd import _lib as L
from onepiece_amd import integration as I

pytestmark = pytest.mark.gpu

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_want = {}


def _handler(res, camt=R.REG_CAM, max_blocks=1 << 13):
    hcam = I.PinholeCamera()
    hcam.fx, hcam.fy, hcam.cx, hcam.cy, hcam.width, hcam.height, hcam.depth_scale = camt
    hv = I.CubeHandler(hcam, device=0, max_blocks=max_blocks)
    hv.SetVoxelResolution(res)
    hv.SetTruncation(R.TRUNC)
    return hv


def _source(oracle, name):
    """-> (keys, vox, res) of the named source volume"""
    if name == "hand":
        return R.HAND_KEYS, R.hand_blocks(), R.HAND_RES
    if name == "crafted":
        return K.crafted() + (K.CRAFT_RES,)
    sc = R.reg_scene(oracle)
    return sc["keys"], sc["vox"], R.REG_RES


def _restated(oracle, name, min_weight):
    """the restatement's one level of the named source, computed once"""
    if (name, min_weight) not in _want:
        keys, vox, res = _source(oracle, name)
        _want[(name, min_weight)] = K.coarsen(keys, vox, res, min_weight)
    return _want[(name, min_weight)]


def _uploaded(oracle, name):
    keys, vox, res = _source(oracle, name)
    hv = _handler(res)
    hv.SetCubeMap(keys, vox)
    return hv


def _coarsen(hv, levels=1, min_weight=0.0, max_blocks=0):
    """the C entry itself -> (a CubeHandler around the new volume, its stats as a dict)"""
    lib = L.load()
    h, st = C.c_void_p(), L.CoarsenStats()
    rc = lib.op_volume_coarsen(hv._h, levels, min_weight, max_blocks, C.byref(h), C.byref(st))
    assert rc == L.OP_OK, lib.op_last_error()
    out = I.CubeHandler._wrap(h, hv.camera, hv.device)
    return out, {k: int(getattr(st, k)) for k in K.STAT_NAMES}


def _same(got, want_keys, want_vox, what):
    gk, gv = got.GetCubeMap(sort=False)
    bad = K.same_blocks(gk, gv, want_keys, want_vox)
    assert bad == 0, "%s: %d voxels differ" % (what, bad)


@pytest.mark.parametrize("name,min_weight", [("hand", 0.0), ("crafted", 0.0), ("crafted", 1.0), ("scene", 0.0), ("scene", 2.0)])
def test_01_one_level_against_the_restatement(oracle, name, min_weight):
    keys, vox, res = _source(oracle, name)
    hv = _uploaded(oracle, name)
    before = hv.GetCubeMap()
    out, st = _coarsen(hv, 1, min_weight)
    k2, v2, want = _restated(oracle, name, min_weight)
    print(name, min_weight, st)
    assert st == want
    _same(out, k2, v2, "%s min_weight %g" % (name, min_weight))
    assert F32(out.GetVoxelResolution()) == F32(2.0) * F32(res)
    after = hv.GetCubeMap()
    assert np.array_equal(before[0], after[0]) and np.array_equal(K.bits(before[1]), K.bits(after[1]))   # the source is not changed
    assert np.array_equal(K.bits(after[1]), K.bits(K.sort_blocks(keys, vox)[1]))
    assert F32(hv.GetVoxelResolution()) == F32(res)


@pytest.mark.parametrize("name", ["crafted", "scene"])
def test_02_two_levels(oracle, name):
    keys, vox, res = _source(oracle, name)
    hv = _uploaded(oracle, name)
    both, st_both = _coarsen(hv, 2, 0.125)
    one, _st = _coarsen(hv, 1, 0.125)
    two, st_two = _coarsen(one, 1, 0.125)
    kk, vv, rr, want = K.coarsen_levels(keys, vox, res, 2, 0.125)
    assert st_both == st_two == want
    _same(both, kk, vv, "levels = 2")
    _same(two, kk, vv, "two calls of levels = 1")
    assert F32(both.GetVoxelResolution()) == F32(two.GetVoxelResolution()) == rr == F32(4.0) * F32(res)


def test_03_a_pool_that_is_too_small_grows(oracle):
    hv = _uploaded(oracle, "crafted")
    out, st = _coarsen(hv, 1, 0.0, max_blocks=1)
    k2, v2, want = _restated(oracle, "crafted", 0.0)
    assert st == want
    _same(out, k2, v2, "max_blocks = 1")
    g = out.GrowthStats()
    print(g)
    assert g["grows"] >= 1 and g["max_blocks"] >= len(k2)


def test_03b_the_automatic_size_grows_for_a_sparse_source():
    """3300 blocks of which no two share a result block: more than the third of the source's count the automatic size starts with"""
    rng = np.random.default_rng(5)
    keys = np.array([(2 * x, 2 * y, 2 * z - 15) for x in range(15) for y in range(15) for z in range(15)], np.int32)[:3300]
    vox = np.empty((len(keys), 512, 5), F32)
    vox[..., 0] = rng.uniform(-0.05, 0.05, vox.shape[:2])
    vox[..., 1] = rng.integers(0, 4, vox.shape[:2])
    vox[..., 2:] = rng.uniform(0, 1, vox.shape[:2] + (3,))
    hv = _handler(0.03)
    hv.SetCubeMap(keys, vox)
    auto, st = _coarsen(hv)
    sized, st_sized = _coarsen(hv, max_blocks=4096)
    assert st == st_sized and st["dst_blocks"] == st["src_blocks"] == 3300 and st["voxels_full"] > 0 and st["voxels_partial"] > 0
    assert auto.GrowthStats()["grows"] >= 1 and sized.GrowthStats() == {"max_blocks": 4096, "grows": 0, "replayed_batches": 0}
    ak, av = auto.GetCubeMap()
    sk, sv = sized.GetCubeMap()
    assert np.array_equal(ak, K.sort_blocks(keys >> 1, vox)[0]) and np.array_equal(ak, sk) and np.array_equal(K.bits(av), K.bits(sv))
    # one block against the restatement
    k1, v1, _s = K.coarsen(keys[1234:1235], vox[1234:1235], 0.03)
    row = [tuple(k) for k in ak.tolist()].index(tuple(k1[0].tolist()))
    assert np.array_equal(K.bits(av[row]), K.bits(v1[0]))


def test_04_an_empty_source():
    hv = _handler(0.03)
    out, st = _coarsen(hv, 3, 0.0)
    assert out.BlockCount() == 0 and st == dict.fromkeys(K.STAT_NAMES, 0)
    assert F32(out.GetVoxelResolution()) == F32(8.0) * F32(0.03)


def test_05_the_result_is_an_ordinary_volume(oracle):
    sc = R.reg_scene(oracle)
    hv = _uploaded(oracle, "scene")
    k2, v2, _st = _restated(oracle, "scene", 0.0)
    res2 = F32(2.0) * F32(R.REG_RES)
    out, _s = _coarsen(hv)
    # sampled like any volume: the trilinear rule with gradients, against the restatement of op_volume_sample over the restated coarse grid
    q = S.query_mix(k2, res2)
    want = S.sample(k2, v2, res2, q, gradients=True)
    vox, status, grad = out.Sample(q, mode="trilinear", gradients=True)
    assert np.array_equal(status, want["status"])
    assert np.array_equal(K.bits(vox), K.bits(want["voxels"])) and np.array_equal(K.bits(grad), K.bits(want["gradients"]))
    assert int(((status & S.INVALID) == 0).sum()) > 500
    # collected and merged like any volume
    other, _s = _coarsen(hv)
    gc = out.CollectGarbage()
    seen = (v2[..., 1] > 0).any(axis=1)
    assert gc["blocks_before"] == len(k2) and gc["blocks_kept"] == int(seen.sum())
    out.Merge(other)
    assert out.BlockCount() == len(k2)
    mk, mv = out.GetCubeMap()
    was = seen
    assert np.array_equal(mk, k2)                                     # (the restatement's ids are sorted as GetCubeMap sorts them)
    assert np.array_equal(K.bits(mv[~was]), K.bits(v2[~was]))         # a block the collection dropped comes back as the copy's
    both = (v2[..., 1] > 0) & was[:, None]
    assert np.array_equal(mv[..., 1][both], (v2[..., 1] + v2[..., 1])[both])   # TSDFVoxel::operator+ of two equal copies: the weights add
    # fused into like any volume: the general update, since the volume is foreign
    fresh, _s = _coarsen(hv)
    fresh._trunc = R.TRUNC
    k0, v0 = fresh.GetCubeMap()
    depth, rgb, pose = sc["frames"][0]
    fresh.IntegrateImage(depth, rgb, pose)
    k1, v1 = fresh.GetCubeMap()
    rows = {tuple(k): r for r, k in enumerate(k1.tolist())}
    kept = np.array([rows[tuple(k)] for k in k0.tolist()])
    changed = (K.bits(v1[kept]) != K.bits(v0)).any(axis=-1)
    print("one frame into the coarse copy: %d of %d voxels changed, %d blocks -> %d" % (int(changed.sum()), changed.size, len(k0), len(k1)))
    assert changed.sum() > 1000
    w0, w1 = v0[..., 1][changed], v1[kept][..., 1][changed]
    assert (w1 == w0 + 1).all()                                       # the running mean took the fractional weight as it is


def test_06_python_and_cpp_surfaces_equal_the_c_entry(oracle, tmp_path):
    hv = _uploaded(oracle, "crafted")
    out, st = _coarsen(hv, 2, 1.0)
    py = hv.Coarsen(2, 1.0)
    assert py.coarsen_stats == st and py.GetVoxelResolution() == out.GetVoxelResolution()
    ck, cv = out.GetCubeMap()
    pk, pv = py.GetCubeMap()
    assert np.array_equal(ck, pk) and np.array_equal(K.bits(cv), K.bits(pv))
    once = hv.Coarsen()
    k2, v2, _want1 = _restated(oracle, "crafted", 0.0)
    _same(once, k2, v2, "Coarsen()")
    # the C++ class over the same blocks, read from a .map file (which keeps |sdf| < 1 and weight != 0: the counts of blocks are what is compared)
    host = os.path.join(ROOT, "host", "one_piece")
    lib = os.path.join(ROOT, "onepiece_amd")
    subprocess.check_call(["make", "-s"], cwd=host)
    exe = tmp_path / "coarsen_surface_check"
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-I", host, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "coarsen_surface_check.cpp"),
                           "-L", host, "-lone_piece_hip_host", "-L", lib, "-lonepiece_hip", "-Wl,-rpath," + host, "-Wl,-rpath," + lib, "-o", str(exe)])
    path = str(tmp_path / "crafted.map")
    hv.WriteToFile(path)
    back = _handler(K.CRAFT_RES)
    back.ReadFromFile(path)
    want2, st2 = _coarsen(back, 2, 1.0)
    run = subprocess.run([str(exe), path, repr(K.CRAFT_RES), "2", "1"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = {l.split()[0]: l.split()[1:] for l in run.stdout.splitlines() if l.startswith(("coarse ", "once "))}
    print(run.stdout)
    c = lines["coarse"]
    assert F32(float(c[0])) == F32(4.0) * F32(K.CRAFT_RES)
    assert int(c[1]) == int(np.floor(np.floor(F32(1.0) / (F32(4.0) * F32(K.CRAFT_RES))) / 8))   # the handler's own c_para took the new voxel size
    assert int(c[2]) == want2.BlockCount() and [int(v) for v in c[3:9]] == [st2[k] for k in K.STAT_NAMES]
    o = lines["once"]
    assert F32(float(o[0])) == F32(2.0) * F32(K.CRAFT_RES) and F32(float(o[4])) == F32(K.CRAFT_RES) and int(o[6]) == back.BlockCount()


def test_07_driver_device_and_host_paths_write_the_same_bytes(tmp_path):
    exe = os.path.join(ROOT, "examples", "cpp", "ModelLod.bin")
    assert os.path.exists(exe), "examples/cpp/ModelLod.bin is not built (__graft_entry__.build())"
    dumps, levels = {}, {}
    for path in ("device", "host"):
        run = subprocess.run([exe, "--synthetic", "8", "25", "1", "--res", "0.02", "--levels", "2", "--path", path, "--out", str(tmp_path)], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stdout + run.stderr
        levels[path] = [json.loads(l) for l in run.stdout.splitlines() if l.startswith("{")]
        dumps[path] = open(str(tmp_path / ("lod_%s.blocks" % path)), "rb").read()
        print(path, levels[path])
    assert len(dumps["device"]) > 0 and len(dumps["device"]) % (12 + 512 * 20) == 0
    assert dumps["device"] == dumps["host"]
    for dev, host in zip(levels["device"], levels["host"]):
        assert [dev[k] for k in ("level", "blocks", "stats", "triangles")] == [host[k] for k in ("level", "blocks", "stats", "triangles")]
    assert [l["level"] for l in levels["device"]] == [0, 1, 2]
    l0, l1, l2 = levels["device"]
    assert len(dumps["device"]) == l2["blocks"] * (12 + 512 * 20)
    assert l2["blocks"] < l1["blocks"] < l0["blocks"] and l1["stats"]["src_blocks"] == l0["blocks"] and l2["stats"]["src_blocks"] == l1["blocks"]
    assert abs(l1["res"] - 0.04) < 1e-6 and abs(l2["res"] - 0.08) < 1e-6
    for l in levels["device"]:                                        # the fidelity line is present
        assert l["fidelity_vertices"] == 3 * l0["triangles"] and l["fidelity_rmse"] >= 0 and 0 <= l["fidelity_invalid"] < 1 and l["fidelity_p95"] >= 0
        assert l["triangles"] > 0 and l["pixels_seen"] > 0


def test_08_driver_registers_against_the_coarse_model():
    exe = os.path.join(ROOT, "examples", "cpp", "ModelRegistration.bin")
    assert os.path.exists(exe), "examples/cpp/ModelRegistration.bin is not built (__graft_entry__.build())"
    args = [exe, "--synthetic", "6", "5", "1", "--res", "0.04", "--perturb", "3", "--iters", "3", "--path", "fused"]
    run = subprocess.run(args + ["--coarse", "1"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    print(run.stdout)
    rows = [l for l in run.stdout.splitlines() if l.startswith("coarse ")]
    assert len(rows) == 2 and rows[0].startswith("coarse 0: per iteration") and rows[1].startswith("coarse 1: per iteration")
    got = json.loads([l for l in run.stdout.splitlines() if l.startswith("{")][-1])
    assert got["coarse"]["levels"] == 1 and got["coarse"]["blocks"] > 0 and got["coarse"]["per_iteration_median"] > 0
    plain = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and not [l for l in plain.stdout.splitlines() if l.startswith("coarse ")]
    base = json.loads([l for l in plain.stdout.splitlines() if l.startswith("{")][-1])
    assert "coarse" not in base
    for k in ("registered", "iterations", "points", "used_last", "error_before", "error_after", "rmse"):   # nothing else changes
        assert base[k] == got[k], k
