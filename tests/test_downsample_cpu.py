"""Voxel-grid down-sampling without a GPU: the device entries refuse loudly, the option constant matches the header, and the numpy
restatement the GPU tests compare against is the class surface's host loop, bit for bit (through examples/cpp/SubmapModel.bin --cloud,
which touches no device on the host path)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import downsample_common as D

ROOT = D.ROOT


def test_entries_fail_loudly_without_a_gpu(hip):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from onepiece_amd import integration as I, registration as R
    pts, col, nrm = D.random_cloud(100, 1)
    with pytest.raises(hip.OnePieceHipError) as e:
        R.PointCloud(pts, nrm).DownSample(0.05, col)
    assert e.value.code == hip.OP_ERR_NO_DEVICE
    cam = I.PinholeCamera()
    cam.width, cam.height = 8, 6
    with pytest.raises(hip.OnePieceHipError) as e:
        R.LoadFromRGBDDownSampled(np.zeros((6, 8, 3), np.uint8), np.ones((6, 8), np.float32), cam, np.eye(4, dtype=np.float32))
    assert e.value.code == hip.OP_ERR_NO_DEVICE
    n = C.c_size_t(7)  # an empty cloud is no excuse either: as everywhere else, the device comes first
    assert hip.load().op_point_cloud_downsample(None, None, None, 0, 0.05, hip.OP_MEM_HOST, 0, None, None, None, C.byref(n)) == hip.OP_ERR_NO_DEVICE


def test_option_constant_matches_the_header_and_round_trips(hip):
    text = open(os.path.join(ROOT, "include", "onepiece_hip.h")).read()
    m = re.search(r"#define\s+OP_RUNTIME_OPT_POINT_CLOUD_DOWNSAMPLE\s+(\d+)", text)
    assert m and int(m.group(1)) == hip.OP_RUNTIME_OPT_POINT_CLOUD_DOWNSAMPLE == 12
    lib, v = hip.load(), C.c_longlong(-1)
    assert lib.op_runtime_get_option(hip.OP_RUNTIME_OPT_POINT_CLOUD_DOWNSAMPLE, C.byref(v)) == 0 and v.value == 0   # host loop unless asked
    assert lib.op_runtime_set_option(hip.OP_RUNTIME_OPT_POINT_CLOUD_DOWNSAMPLE, 2) == hip.OP_ERR_INVALID
    try:
        assert lib.op_runtime_set_option(hip.OP_RUNTIME_OPT_POINT_CLOUD_DOWNSAMPLE, 1) == 0
        assert lib.op_runtime_get_option(hip.OP_RUNTIME_OPT_POINT_CLOUD_DOWNSAMPLE, C.byref(v)) == 0 and v.value == 1
        g = C.c_longlong(-1)  # the neighbouring option is untouched
        assert lib.op_runtime_get_option(hip.OP_RUNTIME_OPT_GLOBAL_REGISTRATION, C.byref(g)) == 0 and g.value == 0
    finally:
        lib.op_runtime_set_option(hip.OP_RUNTIME_OPT_POINT_CLOUD_DOWNSAMPLE, 0)


def test_bad_arguments_are_refused_before_any_device_is_looked_for(hip):
    pts, _, _ = D.random_cloud(10, 2)
    out, n = np.empty_like(pts), C.c_size_t(0)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    for g in (0.0, -0.05, float("nan"), float("inf")):
        assert hip.load().op_point_cloud_downsample(vp(pts), None, None, len(pts), g, hip.OP_MEM_HOST, 0, vp(out), None, None, C.byref(n)) == hip.OP_ERR_INVALID
    assert hip.load().op_point_cloud_downsample(vp(pts), None, None, len(pts), 0.05, 7, 0, vp(out), None, None, C.byref(n)) == hip.OP_ERR_INVALID
    assert hip.load().op_point_cloud_downsample(vp(pts), vp(pts), None, len(pts), 0.05, hip.OP_MEM_HOST, 0, vp(out), None, None, C.byref(n)) == hip.OP_ERR_INVALID  # colours in, no room out


@pytest.mark.parametrize("case", ["random", "boundaries", "too_wide", "one_cell"])
def test_restatement_is_the_host_loop(case, tmp_path):
    assert os.path.exists(D.DRIVER), "examples/cpp/SubmapModel.bin is not built (make -C examples/cpp)"
    g = 0.05
    if case == "random":
        pts, col, _ = D.random_cloud(5000, 11)
    elif case == "boundaries":  # negative coordinates, points on k * grid_len and a float either side
        k = np.arange(-40, 40, dtype=np.float32) * np.float32(g)
        x = np.concatenate([k, np.nextafter(k, np.float32(-np.inf)), np.nextafter(k, np.float32(np.inf))])
        rng = np.random.default_rng(5)
        pts = np.stack([x, rng.uniform(-0.2, 0.2, len(x)).astype(np.float32), rng.permutation(x)], axis=1)
        col = rng.uniform(0, 1, size=pts.shape).astype(np.float32)
    elif case == "too_wide":
        pts, col = D.too_wide_cloud(g)
    else:  # one cell, eight binades: the order of the adds shows in the bits
        rng = np.random.default_rng(9)
        pts = (rng.uniform(1.0, 2.0, size=(3000, 3)) * 2.0 ** rng.integers(2, 10, size=(3000, 3))).astype(np.float32)
        col, g = None, 1024.0
    js, got_p, got_c = D.downsample_through_driver(tmp_path, "host", pts, col, g)
    want_p, want_c, _ = D.downsample_ref(pts, g, col)
    assert js["points"] == len(pts) and js["cells"] == len(want_p)
    assert D.same_bits(got_p, want_p)
    assert (col is None and got_c is None) or D.same_bits(got_c, want_c)
