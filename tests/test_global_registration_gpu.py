"""Global registration on the device against the host path (OP_RUNTIME_OPT_GLOBAL_REGISTRATION 0, run through examples/cpp/GlobalRegistration.bin)
and, for the direct C-ABI entries, against the float32 numpy restatements of global_registration_common.py; FPFH also against that module's
independent statement (exact radius neighbours by brute force, then the arithmetic of the reference's 3DFeature.cpp).

The one permitted difference is the first Darboux angle's bin for pairs that sit on a bin boundary (the host's atan2f is its libm's, the device
rounds a double atan2 once): global_registration_common.check_features states the rule."""
import numpy as np
import pytest

import global_registration_common as G
from onepiece_amd import registration as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def plys(tmp_path_factory):
    d = tmp_path_factory.mktemp("gr_inputs")
    (ps, ns), (pt, nt) = G.room_clouds()
    pa, na = G.adversarial_cloud()
    out = {}
    for name, (p, n) in (("source", (ps, ns)), ("target", (pt, nt)), ("adversarial", (pa, na))):
        out[name] = str(d / (name + ".ply"))
        G.write_ply(out[name], p, n)
        out[name + "_arrays"] = (p, n)
    return out


@pytest.fixture(scope="module")
def room_runs(plys, tmp_path_factory):
    """the two room clouds through the whole flow, DenseSlam's parameters (40 000 iterations), host and device"""
    d = tmp_path_factory.mktemp("gr_room")
    args = [plys["source"], plys["target"], "--as-given"]
    host = G.run_example(args + ["--path", "host"], str(d / "host"))
    dev = G.run_example(args + ["--path", "device"], str(d / "device"))
    return host, dev, args, d


@pytest.fixture(scope="module")
def adversarial_runs(plys, tmp_path_factory):
    d = tmp_path_factory.mktemp("gr_adv")
    args = [plys["adversarial"], plys["source"], "--as-given", "--features-only"]
    return G.run_example(args + ["--path", "host"], str(d / "host")), G.run_example(args + ["--path", "device"], str(d / "device"))


def test_features_of_the_room_clouds(room_runs):
    """rules 1-3: neighbour lists identical; SPFH / FPFH bit-identical except where flagged pairs allow a moved increment; shares under the caps"""
    host, dev = room_runs[0], room_runs[1]
    for tag in ("source", "target"):
        G.check_features(host, dev, tag, enforce_shares=True)


def test_features_of_the_adversarial_cloud(adversarial_runs):
    """ties, duplicates, an isolated point and a clump that forces the top-knn cut: lists identical in order and count, the same per-point rule"""
    host, dev = adversarial_runs
    shares = G.check_features(host, dev, "source", enforce_shares=False)
    m = (dev["source_neighbours"] >= 0).sum(1)
    assert m.max() == G.KNN and m.min() == 1 and shares["flagged_points"] > 0


def test_python_mirror_matches_the_class_surface(plys, room_runs, adversarial_runs):
    for name, dump, tag in (("source", room_runs[1], "source"), ("adversarial", adversarial_runs[1], "source")):
        p, n = plys[name + "_arrays"]
        fpfh, nb, spfh = R.ComputeFPFHFeature(R.PointCloud(p, n), knn=G.KNN, radius=G.RADIUS, return_debug=True)
        assert np.array_equal(nb, dump[tag + "_neighbours"])
        assert np.array_equal(spfh.view(np.uint32), dump[tag + "_spfh"].view(np.uint32)) and np.array_equal(fpfh.view(np.uint32), dump[tag + "_fpfh"].view(np.uint32))
        assert np.array_equal(R.ComputeFPFHFeature(R.PointCloud(p, n), knn=G.KNN, radius=G.RADIUS).view(np.uint32), fpfh.view(np.uint32))
    p, n = plys["source_arrays"]   # a small knn and another radius: padded lists, the prefix property of the (d2, index) order
    _f, nb7, _s = R.ComputeFPFHFeature(R.PointCloud(p, n), knn=7, radius=G.RADIUS, return_debug=True)
    assert np.array_equal(nb7, room_runs[1]["source_neighbours"][:, :7])


def test_feature_match_is_the_host_scan(room_runs, adversarial_runs):
    rng = np.random.default_rng(5)
    cases = []
    a, b = (rng.random((700, 33)) * 100).astype(np.float32), (rng.random((1111, 33)) * 100).astype(np.float32)      # neither a multiple of a tile
    cases.append(("random", a, b))
    cases.append(("room fpfh", room_runs[0]["source_fpfh"], room_runs[0]["target_fpfh"]))
    cases.append(("adversarial fpfh", adversarial_runs[0]["source_fpfh"], adversarial_runs[0]["target_fpfh"]))
    dup = np.concatenate([b[:300], b[:300], b[100:400], b[:77]])                                                        # exact duplicate rows: the lowest index wins
    cases.append(("duplicates", np.concatenate([b[:350], a[:33]]), dup))
    cases.append(("integer features, many exact ties", rng.integers(0, 3, (513, 33)).astype(np.float32), rng.integers(0, 3, (3000, 33)).astype(np.float32)))
    cases.append(("one target", a[:65], b[:1]))
    cases.append(("no target", a[:10], b[:0]))
    for name, s, t in cases:
        want = G.feature_match_reference(s, t)
        got = R.FeatureMatching3D(s, t)
        if len(t) == 0:
            assert got.shape == (0, 2), name
            continue
        assert np.array_equal(got[:, 0], np.arange(len(s))) and np.array_equal(got[:, 1], want), "%s: %d of %d differ" % (name, (got[:, 1] != want).sum(), len(s))
    got = R.FeatureMatching3D(dup[:350], dup)
    assert np.array_equal(got[:, 1], np.arange(350) % 300)


def test_ransac_counts_and_inlier_ids_are_exact():
    rng = np.random.default_rng(11)

    def transforms(H):
        T = np.zeros((H, 3, 4), np.float32)
        for h in range(H):
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            T[h, :, :3] = q
            T[h, :, 3] = rng.normal(size=3) * 0.2
        T[::7] = np.eye(4, dtype=np.float32)[:3]     # the identity: residuals below are exact
        return T

    for H, n in ((1, 8), (3, 9), (257, 300), (1000, 2049), (40000, 3000)):
        src = np.round(rng.normal(size=(n, 3)) * 8).astype(np.float32) / np.float32(8)          # multiples of 1/8
        tgt = src.copy()
        tgt[::3, 0] += np.float32(0.5)        # under the identity: residual EXACTLY 0.5 == threshold -> not an inlier (strictly below)
        tgt[1::3, 1] -= np.float32(0.375)     # 0.375 < 0.5 -> inlier
        tgt[2::3] += (rng.normal(size=tgt[2::3].shape) * 0.4).astype(np.float32)
        Ts = transforms(H)
        threshold = 0.5
        counts = R.CountInliersRANSAC(src, tgt, Ts, threshold)
        want = np.concatenate([G.inlier_reference(src, tgt, Ts[h:h + 1000], threshold).sum(1) for h in range(0, H, 1000)]).astype(np.uint32)
        assert np.array_equal(counts, want), (H, n, np.nonzero(counts != want)[0][:5])
        assert counts[0] == want[0] == len(tgt[1::3]) + (G.inlier_reference(src, tgt, Ts[:1], threshold)[0][2::3]).sum()
        assert want[0] < n - len(tgt[::3]) + 1                                                   # none of the residuals that EQUAL the threshold counted
        for h in sorted({0, H // 2, H - 1, int(np.argmax(want))}):
            ids = R.InlierIdsRANSAC(src, tgt, Ts[h], threshold)
            assert np.array_equal(ids, np.nonzero(G.inlier_reference(src, tgt, Ts[h:h + 1], threshold)[0])[0]), (H, n, h)
    assert np.array_equal(R.CountInliersRANSAC(src[:0], tgt[:0], Ts[:5], 0.5), np.zeros(5, np.uint32))
    full = np.concatenate([Ts[:2], np.tile(np.float32([0, 0, 0, 1]), (2, 1, 1))], axis=1)        # [H,4,4] input: the last row is ignored
    assert np.array_equal(R.CountInliersRANSAC(src, tgt, full, 0.5), counts[:2])


def _compare_tail(host, dev):
    for key in ("matches", "matches_kept", "inlier_ids", "correspondence_set_index"):
        assert np.array_equal(host[key], dev[key]), "%s differ (%d vs %d entries)" % (key, len(host[key]), len(dev[key]))
    assert np.array_equal(host["T"].view(np.uint32), dev["T"].view(np.uint32)), (host["T"], dev["T"])
    assert np.array_equal(host["rmse"].view(np.uint32), dev["rmse"].view(np.uint32))


def test_class_surface_end_to_end(room_runs, tmp_path):
    """matching, the three rejections, RANSAC's winner, T (bitwise), inlier ids, rmse and correspondence_set_index: identical on both paths;
    T is the scene's motion within the margin tests/test_reference_examples.py uses for DenseFusion's poses (0.25)."""
    host, dev, args, _d = room_runs
    same_features = all(np.array_equal(host[t + "_fpfh"].view(np.uint32), dev[t + "_fpfh"].view(np.uint32)) for t in ("source", "target"))
    if not same_features and not np.array_equal(host["matches"], dev["matches"]):
        # a flagged pair moved a feature enough to change a match: matching is exact GIVEN features, so this stage gets the HOST features on both paths
        print("features differ on flagged points: the device path is re-run on the host path's features")
        dev = G.run_example(args + ["--path", "device", "--load-features", str(_d / "host")], str(tmp_path / "device_on_host_features"))
    assert len(host["matches"]) == 2 * len(host["source_points"]) and 16 <= len(host["matches_kept"]) <= len(host["matches"])
    _compare_tail(host, dev)
    assert host["json"]["max_iteration"] == 40000 and len(host["inlier_ids"]) >= 8
    T, want = dev["T"].reshape(4, 4).astype(np.float64), G.room_motion()
    print("T", T, "motion", want, "inliers", len(dev["inlier_ids"]), "rmse", dev["rmse"], "ms host", host["json"]["ms"], "ms device", dev["json"]["ms"])
    assert np.abs(T[:3, 3] - want[:3, 3]).max() < 0.25 and np.abs(T[:3, :3] - want[:3, :3]).max() < 0.25


def test_class_surface_synthetic_views(tmp_path):
    """--synthetic: LoadFromDepth, DownSample, EstimateNormals, then the same flow; few iterations (the full count runs above)"""
    args = ["--synthetic", "--max-iteration", "4000"]
    host = G.run_example(args + ["--path", "host"], str(tmp_path / "host"))
    dev = G.run_example(args + ["--path", "device"], str(tmp_path / "device"))
    for tag in ("source", "target"):
        assert 2000 <= len(host[tag + "_points"]) <= 9000
        G.check_features(host, dev, tag, enforce_shares=True)
    if not np.array_equal(host["matches"], dev["matches"]):
        print("features differ on flagged points: the device path is re-run on the host path's features")
        dev = G.run_example(args + ["--path", "device", "--load-features", str(tmp_path / "host")], str(tmp_path / "device_on_host_features"))
    _compare_tail(host, dev)
    T, want = np.array(dev["json"]["T"]).reshape(4, 4), np.array(dev["json"]["expected_T"]).reshape(4, 4)
    print("T", T, "expected", want)
    assert np.abs(T[:3, 3] - want[:3, 3]).max() < 0.25 and np.abs(T[:3, :3] - want[:3, :3]).max() < 0.25


def test_small_and_degenerate_sets_through_the_class_surface(plys, tmp_path):
    """fewer than / exactly 8 kept matches and tiny clouds take the same early exits on both paths"""
    p, n = plys["source_arrays"]
    G.write_ply(str(tmp_path / "a.ply"), p[:9], n[:9])
    G.write_ply(str(tmp_path / "b.ply"), p[:40], n[:40])
    for pair in ((str(tmp_path / "a.ply"), str(tmp_path / "b.ply")), (str(tmp_path / "b.ply"), str(tmp_path / "b.ply"))):
        args = list(pair) + ["--as-given", "--max-iteration", "500"]
        host = G.run_example(args + ["--path", "host"], str(tmp_path / "host"))
        dev = G.run_example(args + ["--path", "device"], str(tmp_path / "device"))
        G.check_features(host, dev, "source", enforce_shares=False)
        if np.array_equal(host["source_fpfh"].view(np.uint32), dev["source_fpfh"].view(np.uint32)) and np.array_equal(host["target_fpfh"].view(np.uint32), dev["target_fpfh"].view(np.uint32)):
            _compare_tail(host, dev)


# ---- the device path against the independent statement of FPFH ----------------------------------------------------------------------------

def _device_dump(p, n, knn, radius):
    fpfh, nb, spfh = R.ComputeFPFHFeature(R.PointCloud(p, n), knn=knn, radius=radius, return_debug=True)
    return {"source_points": p, "source_normals": n, "source_neighbours": nb, "source_spfh": spfh, "source_fpfh": fpfh}


@pytest.mark.parametrize("name", G.CASE_NAMES)
def test_device_path_against_the_reference(name):
    """The same clouds and the same assertions as the host path's test in test_global_registration_cpu.py: lists equal to the brute-force
    search in order and count, thirds 2 and 3 bit-identical, third 1 by the one-bin rule.  The clumps at every knn of GPU_CLUMP_KNN."""
    p, n, knn, radius = G.case(name)
    for k in (G.GPU_CLUMP_KNN if name.startswith("clump") else (knn,)):
        got = _device_dump(p, n, k, radius)
        G.check_against_reference(G.case_reference(name, k), got, enforce_shares=name.startswith("room"))
        G.check_list_properties(name, k, got)


def test_device_memory_through_the_c_abi_equals_host_memory():
    """op_fpfh_compute with OP_MEM_DEVICE inputs and outputs (torch tensors' data_ptr) against the OP_MEM_HOST call: bit for bit"""
    import ctypes as C
    import torch
    from onepiece_amd import _lib as L
    p, n, _knn, radius = G.case("cell edge 0.05")
    knn = 65
    want = _device_dump(p, n, knn, radius)
    dp, dn = torch.from_numpy(p).cuda(), torch.from_numpy(n).cuda()
    f = torch.full((len(p), 33), -7.0, dtype=torch.float32, device="cuda")
    s = torch.full((len(p), 33), -7.0, dtype=torch.float32, device="cuda")
    nb = torch.full((len(p), knn), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    vp = lambda t: C.c_void_p(t.data_ptr())
    L.check(L.load().op_fpfh_compute(vp(dp), vp(dn), len(p), knn, float(radius), L.OP_MEM_DEVICE, 0, vp(f), vp(nb), vp(s)))
    torch.cuda.synchronize()
    assert np.array_equal(nb.cpu().numpy(), want["source_neighbours"])
    assert np.array_equal(s.cpu().numpy().view(np.uint32), want["source_spfh"].view(np.uint32))
    assert np.array_equal(f.cpu().numpy().view(np.uint32), want["source_fpfh"].view(np.uint32))
    G.check_against_reference(G.with_knn(G.case_reference("cell edge 0.05"), knn), want)
