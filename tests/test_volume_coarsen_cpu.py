"""op_volume_coarsen without a device: the numpy restatement of its definition (tests/volume_coarsen_common.py) over the hand-made field, the crafted
volume and the oracle's fusion of the convergence scene; what a coarse level costs in fidelity and what the restated registration loop makes of
it; the C-ABI's declaration, binding and refusals; the C++ class surface."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np

import volume_coarsen_common as K
import volume_register_common as R
import volume_sample_common as S

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "host", "one_piece")
EIGEN = "/root/reference/3rdparty/Eigen"


def test_hand_made_field_is_exact():
    """s = z - Z0 at 1/32 m, weights 1, colours 0.5: every coarse sdf is the coarse centre's z - Z0 (dyadic values, equal weights: every partial
    sum is exact), weights and colours come back unchanged, and the absent block (0, 0, 0) stays absent"""
    keys2, vox2, stats = K.coarsen(R.HAND_KEYS, R.hand_blocks(), R.HAND_RES)
    want_keys = sorted(k for k in ((x, y, z) for x in (-1, 0) for y in (-1, 0) for z in (-1, 0)) if k != (0, 0, 0))
    assert [tuple(k) for k in keys2.tolist()] == want_keys
    centres = S.block_voxel_centres(keys2, 2 * R.HAND_RES)
    seen = vox2[..., 1] > 0
    assert np.array_equal(vox2[..., 0][seen], (centres[..., 2] - F32(R.HAND_Z0))[seen])
    assert (vox2[..., 1][seen] == 1.0).all() and (vox2[..., 2:][seen] == 0.5).all()
    assert (vox2[~seen] == S.DEFAULT_VOXEL).all()
    # a result block holds the one source block of its octet that exists: an eighth of its voxels
    assert seen.sum(axis=1).tolist() == [64] * 7
    assert stats == {"src_blocks": 7, "dst_blocks": 7, "voxels_full": 7 * 64, "voxels_partial": 0, "voxels_empty": 7 * 448, "dropped_min_weight": 0}


def test_crafted_volume():
    keys, vox = K.crafted()
    for mw in (0.0, 1.0):
        keys2, vox2, stats, n = K._coarsen(keys, vox, mw)
        print("min_weight %g: %s" % (mw, stats))
        assert stats["src_blocks"] == 17 and stats["dst_blocks"] == len(keys2) == len({tuple(k) for k in (keys >> 1).tolist()})
        assert tuple(keys2.min(axis=0)) == (-2, -2, -2) and (-1, -1, -1) in {tuple(k) for k in keys2.tolist()}   # -3 -> -2, -2 and -1 -> -1
        seen = n > 0
        assert np.isfinite(vox2[seen]).all()                          # no NaN or inf from under a weight of 0
        assert (vox2[~seen] == S.DEFAULT_VOXEL).all()
        assert (vox2[..., 1][seen] > 0).all()
        assert stats["voxels_full"] + stats["voxels_partial"] + stats["voxels_empty"] == 512 * len(keys2)
        assert stats["voxels_full"] > 0 and stats["voxels_partial"] > 0 and stats["voxels_empty"] > 0
        w = vox[..., 1]
        assert stats["dropped_min_weight"] == int(((w > 0) & (w < mw)).sum())
        assert (stats["dropped_min_weight"] > 0) == (mw > 0)
        # weight == W / 8 bitwise: W summed here once more, child by child in the order c, in float32
        row = {tuple(k): r for r, k in enumerate(keys2.tolist())}
        for g, weights, n0, n1 in K.PLANTED:
            r, v = row[tuple(c >> 3 for c in g)], (g[0] & 7) + 8 * (g[1] & 7) + 64 * (g[2] & 7)
            assert n[r, v] == (n0 if mw == 0 else n1)
            W = F32(0.0)
            for wc in weights:
                if wc > 0 and wc >= mw:
                    W = F32(W + F32(wc))
            want = F32(W / F32(8.0)) if n[r, v] else F32(0.0)
            assert K.bits(vox2[r, v, 1]) == K.bits(want), (g, mw)
            if not n[r, v]:
                assert (vox2[r, v] == S.DEFAULT_VOXEL).all()
    # the lone block: one source block of eight -> an eighth of the result block can be observed
    keys2, vox2, _s = K.coarsen(keys, vox, K.CRAFT_RES)
    lone = vox2[[tuple(k) for k in keys2.tolist()].index((2, 2, 2))].reshape(8, 8, 8, 5)
    assert (lone[4:] == S.DEFAULT_VOXEL).all() and (lone[:, 4:] == S.DEFAULT_VOXEL).all() and (lone[:, :, 4:] == S.DEFAULT_VOXEL).all()
    assert (lone[:4, :4, :4, 1] > 0).any()


def test_two_levels_are_one_level_twice():
    keys, vox = K.crafted()
    k1, v1, _s1 = K.coarsen(keys, vox, K.CRAFT_RES, 0.125)
    k2, v2, s2 = K.coarsen(k1, v1, 2 * K.CRAFT_RES, 0.125)
    kk, vv, res, ss = K.coarsen_levels(keys, vox, K.CRAFT_RES, 2, 0.125)
    assert np.array_equal(kk, k2) and np.array_equal(K.bits(vv), K.bits(v2)) and ss == s2
    assert res == F32(4) * F32(K.CRAFT_RES) and ss["src_blocks"] == len(k1)
    assert len(k2) < len(k1) < len(keys)


def _surface_fit(grid, cloud):
    out = S.sample(None, None, None, cloud, gradients=True, grid=grid)
    good = (out["status"] & S.INVALID) == 0
    s = out["voxels"][good, 0].astype(np.float64)
    return math.sqrt(float(np.mean(s * s))) if good.any() else float("nan"), float(good.mean())


def test_fidelity_of_the_coarse_grid(oracle):
    """The convergence scene (2 cm voxels, the oracle's fusion) sampled at the frames' own hit points, which lie on the surface: rmse of the
    trilinear sdf and the share of valid samples, on the fine grid and on the restated coarse grids.  Measured when this test was written:
        fine    (2 cm): rmse 0.00311 m, valid 0.9939
        level 1 (4 cm): rmse 0.00298 m, valid 0.9888   (the mean over eight voxels also averages the fusion's noise: the rmse does not grow)
        level 2 (8 cm): rmse 0.00349 m, valid 0.9861
    The bounds are about twice the gap seen: the valid share may fall by 0.010 (seen 0.0051) and 0.016 (seen 0.0078); the rmse may be 1.08 times
    the fine one at level 1 (seen 0.96: a gap of 4 % the other way) and 1.25 times at level 2 (seen 1.12)."""
    sc = R.reg_scene(oracle)
    fine_rmse, fine_valid = _surface_fit(sc["grid"], sc["cloud"])
    k1, v1, _s = K.coarsen(sc["keys"], sc["vox"], R.REG_RES)
    l1_rmse, l1_valid = _surface_fit(S.Grid(k1, v1, 2 * R.REG_RES), sc["cloud"])
    k2, v2, _s = K.coarsen(k1, v1, 2 * R.REG_RES)
    l2_rmse, l2_valid = _surface_fit(S.Grid(k2, v2, 4 * R.REG_RES), sc["cloud"])
    print("fine: rmse %.5f valid %.4f; level 1: rmse %.5f valid %.4f; level 2: rmse %.5f valid %.4f" % (fine_rmse, fine_valid, l1_rmse, l1_valid, l2_rmse, l2_valid))
    assert l1_valid >= fine_valid - 0.010 and l2_valid >= fine_valid - 0.016
    assert l1_rmse <= 1.08 * fine_rmse and l2_rmse <= 1.25 * fine_rmse


def test_the_restated_loop_on_the_coarse_grid(oracle, hip):
    """op_volume_register_points' loop, restated, from the scene's perturbed start against the coarse grid, next to the fine grid's trace: asserted
    only that it ends closer to the truth than it started (the figures are DESIGN.md's)"""
    lib = hip.load()
    sc = R.reg_scene(oracle)
    k1, v1, _s = K.coarsen(sc["keys"], sc["vox"], R.REG_RES)
    grids = {"fine": sc["grid"], "coarse": S.Grid(k1, v1, 2 * R.REG_RES)}
    t0, r0 = R.pose_error(sc["init"])
    end = {}
    for name, grid in grids.items():
        trace = []
        res = R.loop(lib, lambda T: R.system(grid, sc["cloud"], T, R.TRUNC), sc["init"], 8, min_step=0.0, trace=trace)
        for k, (T, counts, rmse, step) in enumerate(trace):
            print("%s iteration %d: used %d, rmse %.5f, pose error %.3f mm / %.5f deg, step %.2e" % ((name, k, counts["used"], rmse) + tuple(
                v * s for v, s in zip(R.pose_error(T), (1e3, 1.0))) + (step,)))
        end[name] = R.pose_error(res["T"])
        print("%s: start %.3f mm / %.5f deg, end %.3f mm / %.5f deg, used %d, rmse %.5f" % (name, t0 * 1e3, r0, end[name][0] * 1e3, end[name][1], res["used"], res["rmse"]))
    assert end["coarse"][0] < t0 and end["coarse"][1] < r0


def test_abi_declaration_binding_and_refusals(hip, tmp_path):
    lib = hip.load()
    text = open(os.path.join(ROOT, "include", "onepiece_hip.h")).read()
    assert re.search(r"\bint op_volume_coarsen\(op_volume \*src, int levels, float min_weight,\s*uint64_t max_blocks, op_volume \*\*out,", text)
    assert re.search(r"\}\s*op_volume_coarsen_stats;", text)
    assert "op_volume_coarsen" in hip.SIGNATURES and hasattr(lib, "op_volume_coarsen")
    assert re.search(r"#define OP_ABI_VERSION 1\b", text) and lib.op_abi_version() == 1
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "onepiece_hip.h"\nint main(void) { printf("%zu %zu\\n", '
                   "sizeof(op_volume_coarsen_stats), offsetof(op_volume_coarsen_stats, dropped_min_weight)); return 0; }\n")
    exe = tmp_path / "sizes.bin"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [C.sizeof(hip.CoarsenStats), hip.CoarsenStats.dropped_min_weight.offset] == [48, 40]
    assert [k for k, _t in hip.CoarsenStats._fields_] == list(K.STAT_NAMES)

    # the refusals: decided before any device work, and before the volume is looked at
    fake = C.c_void_p(0x1000)
    out, st = C.c_void_p(0x77), hip.CoarsenStats()
    st.src_blocks = 77
    cases = {
        "null src": lambda: lib.op_volume_coarsen(None, 1, 0.0, 0, C.byref(out), C.byref(st)),
        "null out": lambda: lib.op_volume_coarsen(fake, 1, 0.0, 0, None, C.byref(st)),
        "levels 0": lambda: lib.op_volume_coarsen(fake, 0, 0.0, 0, C.byref(out), C.byref(st)),
        "levels -1": lambda: lib.op_volume_coarsen(fake, -1, 0.0, 0, C.byref(out), C.byref(st)),
        "levels 5": lambda: lib.op_volume_coarsen(fake, 5, 0.0, 0, C.byref(out), C.byref(st)),
        "min_weight < 0": lambda: lib.op_volume_coarsen(fake, 1, -0.5, 0, C.byref(out), C.byref(st)),
        "min_weight NaN": lambda: lib.op_volume_coarsen(fake, 1, float("nan"), 0, C.byref(out), C.byref(st)),
    }
    for what, call in cases.items():
        assert call() == hip.OP_ERR_INVALID, what
        assert lib.op_last_error().startswith(b"op_volume_coarsen:"), (what, lib.op_last_error())
        assert not out.value or what == "null out", what              # a refused call hands no volume out
    assert st.src_blocks == 77
    from onepiece_amd import integration as I
    assert callable(I.CubeHandler.Coarsen)


def test_class_surface_compiles(hip, tmp_path):
    """tests/cpp/coarsen_surface_check.cpp against host/one_piece as C++11, and against the real Eigen where the reference's vendored copy exists"""
    subprocess.check_call(["make", "-s"], cwd=HOST)
    lib = os.path.join(ROOT, "onepiece_amd")
    src = os.path.join(ROOT, "tests", "cpp", "coarsen_surface_check.cpp")
    exe = tmp_path / "coarsen_surface_check"
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I", HOST, "-I", os.path.join(ROOT, "include"), src, "-L", HOST, "-lone_piece_hip_host",
                           "-L", lib, "-lonepiece_hip", "-Wl,-rpath," + HOST, "-Wl,-rpath," + lib, "-o", str(exe)])
    assert subprocess.run([str(exe)], capture_output=True).returncode == 2          # it starts and links: the usage exit, no device touched
    ch = " ".join(open(os.path.join(HOST, "Integration", "CubeHandler.h")).read().split())
    assert "std::shared_ptr<CubeHandler> Coarsen(int levels = 1, float min_weight = 0" in ch
    if os.path.isdir(EIGEN):
        subprocess.check_call(["g++", "-std=c++11", "-O1", "-w", "-msse4.2", "-DONEPIECE_HAVE_EIGEN", "-I", EIGEN, "-I", HOST, "-I", os.path.join(ROOT, "include"),
                               "-fsyntax-only", src, os.path.join(HOST, "src", "CubeHandler.cpp")])
