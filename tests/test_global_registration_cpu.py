"""Global registration, the part that needs no GPU: the C-ABI surface of the new entries, the option constant, the example driver on the host
path (features only: RANSAC's 8-point fits go through the library and need a device), the input-only shares that the GPU tests rely on,
and the compiled kernels' register budget."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import global_registration_common as G

ROOT = G.ROOT


def _gpu_present():
    import torch
    return torch.cuda.is_available()


def test_entries_refuse_without_a_gpu(hip):
    """No GPU: OP_ERR_NO_DEVICE from every new entry, never a host fallback (with a GPU the same calls succeed)."""
    lib = hip.load()
    rng = np.random.default_rng(1)
    p = rng.random((20, 3)).astype(np.float32)
    f = rng.random((20, 33)).astype(np.float32)
    T = np.tile(np.eye(4, dtype=np.float32)[:3].reshape(1, 12), (2, 1))
    out_f, out_i, out_u, n = np.zeros((20, 33), np.float32), np.zeros(20, np.int32), np.zeros(2, np.uint32), C.c_size_t(0)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    calls = [lambda: lib.op_fpfh_compute(vp(p), vp(p), 20, 10, 0.25, hip.OP_MEM_HOST, 0, vp(out_f), None, None),
             lambda: lib.op_feature_match(vp(f), 20, vp(f), 20, hip.OP_MEM_HOST, 0, vp(out_i)),
             lambda: lib.op_ransac_count_inliers(vp(p), vp(p), 20, vp(T), 2, 0.1, hip.OP_MEM_HOST, 0, vp(out_u)),
             lambda: lib.op_ransac_inlier_ids(vp(p), vp(p), 20, vp(T), 0.1, hip.OP_MEM_HOST, 0, vp(out_i), C.byref(n))]
    for call in calls:
        rc = call()
        if _gpu_present():
            assert rc == 0, lib.op_last_error()
        else:
            assert rc == hip.OP_ERR_NO_DEVICE and b"no CPU fallback" in lib.op_last_error()


def test_argument_checks(hip):
    lib = hip.load()
    p = np.zeros((4, 3), np.float32)
    out = np.zeros((4, 33), np.float32)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    assert lib.op_fpfh_compute(None, vp(p), 4, 10, 0.25, hip.OP_MEM_HOST, 0, vp(out), None, None) == hip.OP_ERR_INVALID
    assert lib.op_fpfh_compute(vp(p), vp(p), 4, 0, 0.25, hip.OP_MEM_HOST, 0, vp(out), None, None) == hip.OP_ERR_INVALID
    assert lib.op_fpfh_compute(vp(p), vp(p), 4, 257, 0.25, hip.OP_MEM_HOST, 0, vp(out), None, None) == hip.OP_ERR_INVALID
    assert lib.op_fpfh_compute(vp(p), vp(p), 4, 10, 0.0, hip.OP_MEM_HOST, 0, vp(out), None, None) == hip.OP_ERR_INVALID
    assert lib.op_fpfh_compute(vp(p), vp(p), 4, 10, 0.25, 7, 0, vp(out), None, None) == hip.OP_ERR_INVALID
    assert lib.op_feature_match(None, 4, vp(out), 4, hip.OP_MEM_HOST, 0, vp(out)) == hip.OP_ERR_INVALID
    assert lib.op_ransac_count_inliers(vp(p), vp(p), 4, None, 1, 0.1, hip.OP_MEM_HOST, 0, vp(out)) == hip.OP_ERR_INVALID
    assert lib.op_ransac_inlier_ids(vp(p), vp(p), 4, vp(out), 0.1, hip.OP_MEM_HOST, 0, vp(out), None) == hip.OP_ERR_INVALID


def test_option_constant_matches_the_header_and_round_trips(hip):
    text = open(os.path.join(ROOT, "include", "onepiece_hip.h")).read()
    assert int(re.search(r"#define OP_RUNTIME_OPT_GLOBAL_REGISTRATION (\d+)", text).group(1)) == hip.OP_RUNTIME_OPT_GLOBAL_REGISTRATION
    lib, v = hip.load(), C.c_longlong(-1)
    assert lib.op_runtime_get_option(hip.OP_RUNTIME_OPT_GLOBAL_REGISTRATION, C.byref(v)) == 0 and v.value == 0   # host path unless asked
    assert lib.op_runtime_set_option(hip.OP_RUNTIME_OPT_GLOBAL_REGISTRATION, 2) == hip.OP_ERR_INVALID
    assert lib.op_runtime_set_option(hip.OP_RUNTIME_OPT_GLOBAL_REGISTRATION, 1) == 0
    assert lib.op_runtime_get_option(hip.OP_RUNTIME_OPT_GLOBAL_REGISTRATION, C.byref(v)) == 0 and v.value == 1
    assert lib.op_runtime_set_option(hip.OP_RUNTIME_OPT_GLOBAL_REGISTRATION, 0) == 0
    assert lib.op_abi_version() == 1


def test_example_is_built_and_documents_itself():
    assert os.path.exists(G.EXAMPLE), "examples/cpp/GlobalRegistration.bin is not built (make -C examples/cpp)"
    run = subprocess.run([G.EXAMPLE], capture_output=True, text=True, timeout=60)
    assert run.returncode == 2 and "--path host|device" in run.stdout


def test_input_shares_on_the_host_path(tmp_path):
    """Flagged (a pair within 1e-6 bins of a boundary of the first angle) and tainted (flagged, or a neighbour is) points depend on the input
    alone.  The host path against itself checks the rule's bookkeeping; the shares of the room clouds must stay under 1 % and 5 %."""
    (ps, ns), (pt, nt) = G.room_clouds()
    assert 2000 <= len(ps) <= 9000 and 2000 <= len(pt) <= 9000, (len(ps), len(pt))
    G.write_ply(str(tmp_path / "s.ply"), ps, ns)
    G.write_ply(str(tmp_path / "t.ply"), pt, nt)
    d = G.run_example([str(tmp_path / "s.ply"), str(tmp_path / "t.ply"), "--as-given", "--features-only", "--path", "host"], str(tmp_path / "host"))
    assert np.array_equal(d["source_points"], ps) and np.array_equal(d["target_normals"], nt)       # the PLY round trip keeps every bit
    for tag in ("source", "target"):
        G.check_features(d, d, tag, enforce_shares=True)
        assert np.isfinite(d[tag + "_fpfh"]).all() and (d[tag + "_neighbours"][:, 0] == np.arange(len(d[tag + "_points"]))).all()
    pa, na = G.adversarial_cloud()
    assert 3500 <= len(pa) <= 4500
    G.write_ply(str(tmp_path / "a.ply"), pa, na)
    d = G.run_example([str(tmp_path / "a.ply"), str(tmp_path / "s.ply"), "--as-given", "--features-only", "--path", "host"], str(tmp_path / "adv"))
    shares = G.check_features(d, d, "source", enforce_shares=False)
    nb = d["source_neighbours"]
    m = (nb >= 0).sum(1)
    assert m.max() == G.KNN and m.min() == 1 and shares["flagged_points"] > 0          # the cut, the isolated point and boundary pairs are all there


def test_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """hipcc --offload-arch=gfx950 --save-temps: no VGPR spills and no scratch in k_feature_match and k_ransac_count (nor in the others);
    the figures are recorded in profiles/global_reg_kernel_resources.txt."""
    src = os.path.join(ROOT, "onepiece_amd", "csrc", "global_reg.hip")
    flags = "--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-slp-vectorize".split()
    subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["--save-temps", "-c", src, "-o", "global_reg.o"], cwd=str(tmp_path), check=True, capture_output=True, timeout=600)
    asm = open(str(tmp_path / "global_reg-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    seen = {}
    for block in asm.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        seen[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, block).group(1)) for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    for kernel in ("k_fpfh_neighbours", "k_spfh", "k_fpfh", "k_feature_match", "k_ransac_count", "k_ransac_inlier_ids"):
        hit = [v for k, v in seen.items() if re.search(r"\d%sE" % kernel, k)]
        assert len(hit) == 1, (kernel, sorted(seen))
        print(kernel, hit[0])
        assert hit[0]["vgpr_spill_count"] == 0 and hit[0]["sgpr_spill_count"] == 0 and hit[0]["private_segment_fixed_size"] == 0, (kernel, hit[0])
        assert hit[0]["group_segment_fixed_size"] <= 64 * 1024
    recorded = open(os.path.join(ROOT, "profiles", "global_reg_kernel_resources.txt")).read()
    for kernel in ("k_feature_match", "k_ransac_count"):
        assert kernel in recorded
    # device writes are vector stores and HIP atomics only: no scalar-unit instruction of the compiled code writes memory or touches the data cache
    scalar_writes = sorted(set(re.findall(r"^\s+(s_\w*(?:store|atomic|dcache)\w*)", asm, flags=re.M)))
    assert not scalar_writes, scalar_writes


# ---- the host path against the independent statement of FPFH (exact radius neighbours + the arithmetic of 3DFeature.cpp) ------------------

def _is_random(name):
    return not (name.startswith("degenerate") or name == "adversarial")


@pytest.mark.parametrize("name", G.CASE_NAMES)
def test_host_path_against_the_reference(name, tmp_path):
    """Neighbour lists equal to the brute-force search in order and count; SPFH / FPFH thirds 2 and 3 bit-identical to the float32 restatement;
    third 1 by the one-bin rule.  The clumps run at every knn of CPU_CLUMP_KNN, everything else at DenseSlam's 100."""
    p, n, knn, radius = G.case(name)
    for k in (G.CPU_CLUMP_KNN if name.startswith("clump") else (knn,)):
        got = G.path_features(str(tmp_path / ("knn%d" % k)), p, n, k, radius)
        assert got["json"]["knn"] == k and np.array_equal(got["source_points"], p)
        G.check_against_reference(G.case_reference(name, k), got, enforce_shares=name.startswith("room"))
        G.check_list_properties(name, k, got)


def test_the_reference_alone_stays_inside_the_caps():
    """flagged <= 1 % and tainted <= 5 % of the room clouds' points depend on the input and the reference alone"""
    for name in ("room source", "room target"):
        ref = G.case_reference(name)
        G.check_features(ref, ref, "source", enforce_shares=True)


@pytest.mark.parametrize("name", G.CASE_NAMES)
def test_float64_cross_check_of_the_restatement(name):
    """spfh_reference's float32 bins against float64 bins wherever float64 is not within DELTA of a boundary.  Random inputs: at most 1 % of
    the pairs are excluded.  Degenerate sets: exactly the constructed pairs are.  The adversarial cloud: every constructed pair is (duplicates
    and the opposed normals on its lattice); its normals elsewhere are random, and what else is excluded stays under 1 % of the pairs."""
    p, n, _knn, _radius = G.case(name)
    nb = G.case_reference(name)["source_neighbours"]
    excluded, share = G.float64_cross_check(p, n, nb, name)
    pairs = max(int((nb[:, 1:] >= 0).sum()), 1)
    if _is_random(name):
        assert share <= 0.01, share
    elif name == "adversarial":
        constructed = G.adversarial_constructed(p, n, nb)
        assert constructed.sum() > 1000 and not (constructed & ~excluded).any()
        assert (excluded & ~constructed).sum() <= 0.01 * pairs, (excluded & ~constructed).sum()
    else:
        constructed = G.constructed_pairs(G.degenerate_sets()[name[len("degenerate: "):]][4], nb)
        assert np.array_equal(excluded, constructed), (excluded.sum(), constructed.sum())


def test_inputs_reach_what_they_are_built_for():
    """the cell-edge clouds hold pairs on both sides of the radius; the far cloud's lists are neither empty nor cut; a clump's are cut; a
    lower-indexed duplicate takes slot 0; d2 == radius is not a neighbour"""
    for radius in G.CELL_EDGE_RADII:
        p, _n, _knn, _r = G.case("cell edge %g" % radius)
        a, b = p[0::9].astype(np.float32), p[1::9].astype(np.float32)      # the straddling pair of every group
        d = b - a
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        assert (d2 < np.float32(radius)).any() and not (d2 < np.float32(radius)).all(), radius
    m = (G.case_reference("far")["source_neighbours"] >= 0).sum(1)
    print("far cloud: mean list length", m.mean())
    assert 5 <= m.mean() <= 50
    assert ((G.case_reference("clump 1025")["source_neighbours"] >= 0).sum(1) == 256).sum() >= 1025
    nb = G.case_reference("degenerate: duplicates of earlier points")["source_neighbours"]
    assert (nb[60:, 0] < 60).all() and (nb[:60, 0] == np.arange(60)).all()
    nb = G.case_reference("degenerate: lattice with d2 == radius")["source_neighbours"]
    assert (nb >= 0).sum(1).max() == 27 and (nb >= 0).sum(1).min() == 8                                     # 3^3 around an inner point, 2^3 at a corner
    nb, p = G.case_reference("clump lattice")["source_neighbours"], G.case("clump lattice")[0]
    rows = np.nonzero(nb[:, 100] >= 0)[0]
    d, e = p[nb[rows, 99]] - p[rows], p[nb[rows, 100]] - p[rows]
    assert len(rows) >= 513 and ((d * d).sum(1) == (e * e).sum(1)).any()                                                     # the cut at 100 falls inside a shell of tied d2
