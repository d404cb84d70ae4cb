"""tool::AlignColorToDepth without a GPU: the numpy restatement the GPU tests compare with IS the class surface's host loop (through
examples/cpp/ScannetIntegration.bin --align, which touches no device on the host path) and IS what Eigen computes for the two expressions it restates;
and reproduces the images the reference's own compiled function gives (tests/golden/align_color_reference.npz); the discriminating inputs are shown
to discriminate; the ScanNet readers, C++ and Python, are checked on directories written here."""
import os
import subprocess

import numpy as np
import pytest

import align_color_common as A

CASES = A.cases()
EIGEN = "/root/reference/3rdparty/Eigen"


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_is_the_host_loop(name, tmp_path, hip):
    case = CASES[name]
    js, got = A.align_through_driver(tmp_path, case, "host")
    assert js["option_default"] == 0, "OP_RUNTIME_OPT_COLOR_ALIGNMENT must default to 0"
    assert np.array_equal(got, A.align(**case))


def test_restatement_is_what_eigen_computes(tmp_path):
    """TransformPoint and color_K * (p / p[2]) evaluated by Eigen itself, bit for bit: pins the order of the sums and the six divisions."""
    if not os.path.isdir(EIGEN):
        pytest.skip("the reference's Eigen headers are not on this machine")
    exe = str(tmp_path / "align_eigen_check.bin")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-msse4.2", "-w", "-I", EIGEN, os.path.join(A.ROOT, "tests", "cpp", "align_eigen_check.cpp"), "-o", exe])
    checked = 0
    for name in sorted(CASES):
        case = CASES[name]
        d = tmp_path / name
        d.mkdir()
        A.write_case(d, case)
        subprocess.check_call([exe, str(d)], timeout=60)
        h, w = case["depth_cam"][5], case["depth_cam"][4]
        uv = np.fromfile(str(d / "eigen_uv.f32"), np.float32).reshape(h, w, 2)
        valid, uf, vf, _ = A.project(case["depth"], case["color_cam"], case["depth_cam"], case["color_to_depth"])
        for mine, eig in ((uf, uv[..., 0]), (vf, uv[..., 1])):
            m, e = mine[valid], eig[valid]
            assert np.array_equal(np.isnan(m), np.isnan(e)), name
            ok = ~np.isnan(m)
            assert np.array_equal(m[ok].view(np.uint32), e[ok].view(np.uint32)), name   # bits: the sign of a zero included
            checked += int(ok.sum())
    assert checked > 2000


GOLDEN = os.path.join(A.ROOT, "tests", "golden", "align_color_reference.npz")
GOLDEN_LEFT_OUT = {"depth_height_above_color_rows"}   # the reference reads past its colour image there: undefined, and the definition's one deviation


def test_restatement_reproduces_the_reference(tmp_path):
    """tests/golden/align_color_reference.npz holds the images the reference's own compiled tool::AlignColorToDepth gives for the inputs of this
    suite (tests/tools/gen_align_color_golden.py).  This is what pins the rules Eigen does not: truncating rounding, the depth camera's height as
    the bound, no p2 test, the zero fill, the byte order of the copy."""
    g = np.load(GOLDEN)
    names = {k.split("/")[0] for k in g.files}
    assert names == set(CASES) - GOLDEN_LEFT_OUT
    for name in sorted(names):
        case = CASES[name]
        # the fixture's inputs are this suite's inputs, bit for bit
        assert g[name + "/color"].tobytes() == case["color"].tobytes() and g[name + "/depth"].dtype == case["depth"].dtype
        assert g[name + "/depth"].tobytes() == case["depth"].tobytes()
        assert tuple(g[name + "/color_cam"]) == tuple(case["color_cam"]) and tuple(g[name + "/depth_cam"]) == tuple(case["depth_cam"])
        M = A.IDENTITY if case["color_to_depth"] is None else case["color_to_depth"]
        assert g[name + "/color_to_depth"].tobytes() == np.ascontiguousarray(M, np.float32).tobytes()
        assert np.array_equal(A.align(**case), g[name + "/aligned"]), name
    # and the fixture itself tells the naive readings apart
    for variant in A.VARIANTS:
        assert any(not np.array_equal(A.align(variant=variant, **CASES[n]), g[n + "/aligned"]) for n in names), variant


def _write_info(d, lines):
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "_info.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


INFO = ["m_versionNumber = 4", "m_sensorName = StructureSensor", "m_colorWidth = 1296", "m_colorHeight = 968", "m_depthWidth = 640", "m_depthHeight = 480",
        "m_depthShift = 1000", "m_calibrationColorIntrinsic = 1170.1875 0 647.75 0 0 1171.5 483.75 0 0 0 1 0 0 0 0 1",
        "m_calibrationColorExtrinsic = 1 0 0 0 0 1 0 0 0 0 1 0 0 0 0 1", "m_calibrationDepthIntrinsic = 571.625 0 319.5 0 0 572.25 239.5 0 0 0 1 0 0 0 0 1",
        "m_calibrationDepthExtrinsic = 1 0 0 0 0 1 0 0 0 0 1 0 0 0 0 1", "m_frames.size = 12"]


def test_cpp_scannet_reader(tmp_path, hip):
    """tool::ReadImageSequenceFromScannetWithPose of the class surface, through ScannetIntegration.bin --list (no device)."""
    d = str(tmp_path / "scene0000_00")
    _write_info(d, INFO)
    pose = np.arange(16, dtype=np.float32).reshape(4, 4) * np.float32(0.25) - np.float32(1.5)
    for i in range(12):
        with open(os.path.join(d, "frame-%06d.pose.txt" % i), "w") as f:
            f.write("\n".join(" ".join("%.9g" % x for x in row) for row in (pose + i)) + "\n")
    js = A.run_driver(["--list", d])
    assert js["rgb_files"] == [d + "/frame-%06d.color.jpg" % i for i in range(12)]
    assert js["depth_files"] == [d + "/frame-%06d.depth.png" % i for i in range(12)]
    assert js["rgb_camera"] == [1170.1875, 1171.5, 647.75, 483.75, 1296, 968, -1]      # SetPara's default depth scale
    assert js["depth_camera"] == [571.625, 572.25, 319.5, 239.5, 640, 480, 1000]
    poses = np.array(js["poses"], np.float32).reshape(12, 4, 4)
    assert np.array_equal(poses[0], pose) and np.array_equal(poses[11], pose + 11)
    # an unknown key: the warning, and the parse ends there -- the sizes before it are kept, m_depthShift and everything after it are not read
    d2 = str(tmp_path / "scene0000_01")
    _write_info(d2, INFO[:6] + ["m_unknownKey = 1"] + INFO[6:])
    js, text = A.run_driver(["--list", d2], with_output=True)
    assert "Wrong format of _info.txt" in text
    assert js["rgb_files"] == [] and js["depth_files"] == [] and js["poses"] == []
    assert js["rgb_camera"] == [0, 0, 0, 0, 1296, 968, -1] and js["depth_camera"] == [0, 0, 0, 0, 640, 480, -1]
    # a line that does not split in two at " = " ends the parse the same way
    d3 = str(tmp_path / "scene0000_02")
    _write_info(d3, INFO[:7] + ["m_colorWidth=7"] + INFO[7:])
    js, text = A.run_driver(["--list", d3], with_output=True)
    assert "Wrong format of _info.txt" in text
    assert js["rgb_files"] == [] and js["depth_camera"] == [0, 0, 0, 0, 640, 480, 1000] and js["rgb_camera"][4] == 1296


@pytest.mark.parametrize("variant", A.VARIANTS)
def test_inputs_discriminate(variant):
    """Each naive reading of the definition gives a different image on at least one input."""
    differs = [n for n in sorted(CASES) if not np.array_equal(A.align(variant=variant, **CASES[n]), A.align(**CASES[n]))]
    assert differs, variant


def test_planted_targets_land_where_intended():
    want = {0: (-1.5, -0.5), 1: (-1.5, -0.5), 2: (-0.5, 0.5), 3: (-0.5, 0.5)}
    hit = {}
    for i in range(12):
        c = CASES["planted_uf_%02d" % i]
        valid, uf, vf, _ = A.project(c["depth"], c["color_cam"], c["depth_cam"], c["color_to_depth"])
        hit[i] = float(uf[0, 1])
        assert valid.all()
    for i, (lo, hi) in want.items():
        assert lo <= hit[i] <= hi and hit[i] not in (-1.5,), (i, hit[i])
    wc = 8
    assert np.float32(hit[5]) == np.nextafter(np.float32(wc - 0.5), np.float32(0)) and hit[6] == wc - 0.5 and np.float32(hit[7]) == np.nextafter(np.float32(wc - 0.5), np.float32(99))
    assert hit[8] > 2.0 ** 31 and hit[9] < -2.0 ** 31
    # (-1.5, 0.5) truncates to column 0; W - 0.5 and above leave the image; values beyond int are rejected, not wrapped
    outs = [A.align(**CASES["planted_uf_%02d" % i])[0, 1] for i in range(12)]
    cols = [CASES["planted_uf_%02d" % i]["color"] for i in range(12)]
    for i in (0, 1, 2, 3):
        assert np.array_equal(outs[i], cols[i][0, 0])
    assert np.array_equal(outs[4], cols[4][0, 1])             # 0.5 + 0.5 = 1
    assert np.array_equal(outs[5], cols[5][0, wc - 1])
    for i in (6, 7, 8, 9, 10):
        assert not outs[i].any()


def test_quirks_kept():
    c = CASES["behind_color_camera"]
    assert A.align(**c).any(), "a point behind the colour camera is still sampled"
    c = CASES["depth_height_below_color_rows"]
    valid, uf, vf, _ = A.project(c["depth"], c["color_cam"], c["depth_cam"], c["color_to_depth"])
    lands_below = valid & (vf + np.float32(0.5) >= c["depth_cam"][5]) & (vf < c["color"].shape[0] - 1)
    assert lands_below.any() and not A.align(**c)[lands_below].any(), "colour rows at and below the depth camera's height are never sampled"
    c = CASES["depth_height_above_color_rows"]
    valid, uf, vf, _ = A.project(c["depth"], c["color_cam"], c["depth_cam"], c["color_to_depth"])
    past = valid & (vf + np.float32(0.5) >= c["color"].shape[0]) & (vf + np.float32(0.5) < c["depth_cam"][5])
    assert past.any() and not A.align(**c)[past].any(), "rows past the colour image are rejected, not read"
    c = CASES["equal_cameras_identity"]
    z = c["depth"] > 0
    out = A.align(**c)
    assert np.array_equal(out[z], c["color"][z]) and not out[~z].any()


def test_scannet_directory_round_trip(tmp_path):
    from onepiece_amd import sequence as Q, synthetic as S
    dcam, ccam, M, depths, colors, poses = A.two_camera_frames(3, width=32, height=24, cwidth=50, cheight=40)
    d = str(tmp_path / "scene0000_00")
    Q.WriteScannetSequence(d, depths, colors, poses, dcam, ccam, depth_scale=1000)
    assert sorted(os.listdir(d))[:4] == ["_info.txt", "frame-000000.color.png", "frame-000000.depth.png", "frame-000000.pose.txt"]
    rgb_files, depth_files, rposes, rc, dc = Q.ReadImageSequenceFromScannetWithPose(d)
    assert [os.path.basename(f) for f in rgb_files] == ["frame-%06d.color.jpg" % i for i in range(3)]      # the reference's names, whatever is on disk
    assert [os.path.basename(f) for f in depth_files] == ["frame-%06d.depth.png" % i for i in range(3)]
    assert rc[4:6] == (50, 40) and dc[4:7] == (32, 24, 1000.0)
    assert np.allclose(rc[:4], ccam[:4], rtol=1e-6) and np.allclose(dc[:4], dcam[:4], rtol=1e-6)
    assert np.array_equal(rposes, poses)
    for i in range(3):
        assert np.array_equal(Q.imread(rgb_files[i][:-3] + "png"), colors[i])
        d16 = Q.imread(depth_files[i], unchanged=True)
        assert d16.dtype == np.uint16 and np.array_equal(d16, np.clip(np.round(depths[i].astype(np.float64) * 1000), 0, 65535).astype(np.uint16))
    # an unknown key ends the parse: what follows it is not read (m_frames.size comes last, so no frames are listed)
    d2 = str(tmp_path / "scene0000_01")
    Q.WriteScannetSequence(d2, depths, colors, poses, dcam, ccam)
    lines = open(os.path.join(d2, "_info.txt")).read().splitlines()
    at = [i for i, l in enumerate(lines) if l.startswith("m_depthShift")][0]
    open(os.path.join(d2, "_info.txt"), "w").write("\n".join(lines[:at] + ["m_unknownKey = 1"] + lines[at:]) + "\n")
    rgb_files, depth_files, rc, dc = Q.ReadImageSequenceFromScannet(d2)
    assert rgb_files == [] and rc[4:6] == (50, 40) and dc[4:6] == (32, 24) and dc[6] == -1.0 and dc[0] == 0.0
