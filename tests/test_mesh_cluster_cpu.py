"""Clustering mesh simplification without a GPU: the device entries refuse loudly, the option constant matches the header, and the numpy
restatement the GPU tests compare against is the class surface's host loop, bit for bit (through examples/cpp/MeshSimplify.bin --mesh, which
touches no device on the host path)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mesh_cluster_common as M

vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)


def _call(hip, pts, tri, g, mem=None, nv=None, outs=None):
    out_p, out_t = outs if outs is not None else (np.empty_like(pts), np.empty_like(tri))
    nv_out, nt_out = C.c_size_t(7), C.c_size_t(7)
    rc = hip.load().op_mesh_cluster_simplify(vp(pts), None, None, len(pts) if nv is None else nv, vp(tri), len(tri), g, hip.OP_MEM_HOST if mem is None else mem, 0,
                                             vp(out_p), None, None, vp(out_t), C.byref(nv_out), C.byref(nt_out))
    return rc, nv_out.value, nt_out.value


def test_entries_fail_loudly_without_a_gpu(hip):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from onepiece_amd import integration as I, registration as R
    from helpers import procedural_mc_table, MC_EDGE_PAIRS
    pts, col, nrm, tri = M.random_soup(21, 1)
    with pytest.raises(hip.OnePieceHipError) as e:
        R.cluster_simplify(pts, col, nrm, tri, 0.05)
    assert e.value.code == hip.OP_ERR_NO_DEVICE
    assert _call(hip, pts, tri[:0], 0.05)[0] == hip.OP_ERR_NO_DEVICE  # an empty mesh is no excuse either: as everywhere else, the device comes first
    with pytest.raises(hip.OnePieceHipError):  # (a volume cannot even be created)
        I.CubeHandler().ExtractSimplifiedTriangleMesh(procedural_mc_table(), MC_EDGE_PAIRS, 0.02)
    nv, nt = C.c_size_t(0), C.c_size_t(0)
    assert hip.load().op_volume_extract_mesh_clustered(None, None, None, None, 0.02, None, None, 0, None, 0, C.byref(nv), C.byref(nt)) == hip.OP_ERR_INVALID


def test_option_constant_matches_the_header_and_round_trips(hip):
    text = open(os.path.join(M.ROOT, "include", "onepiece_hip.h")).read()
    m = re.search(r"#define\s+OP_RUNTIME_OPT_MESH_CLUSTERING\s+(\d+)", text)
    assert m and int(m.group(1)) == hip.OP_RUNTIME_OPT_MESH_CLUSTERING == 13
    lib, v = hip.load(), C.c_longlong(-1)
    assert lib.op_runtime_get_option(hip.OP_RUNTIME_OPT_MESH_CLUSTERING, C.byref(v)) == 0 and v.value == 0   # host loop unless asked
    assert lib.op_runtime_set_option(hip.OP_RUNTIME_OPT_MESH_CLUSTERING, 2) == hip.OP_ERR_INVALID
    try:
        assert lib.op_runtime_set_option(hip.OP_RUNTIME_OPT_MESH_CLUSTERING, 1) == 0
        assert lib.op_runtime_get_option(hip.OP_RUNTIME_OPT_MESH_CLUSTERING, C.byref(v)) == 0 and v.value == 1
        for other in (hip.OP_RUNTIME_OPT_GLOBAL_REGISTRATION, hip.OP_RUNTIME_OPT_POINT_CLOUD_DOWNSAMPLE):  # the neighbouring options are untouched
            g = C.c_longlong(-1)
            assert lib.op_runtime_get_option(other, C.byref(g)) == 0 and g.value == 0
    finally:
        lib.op_runtime_set_option(hip.OP_RUNTIME_OPT_MESH_CLUSTERING, 0)


def test_bad_arguments_are_refused_before_any_device_is_looked_for(hip):
    pts, col, _, tri = M.random_soup(10, 2)
    for g in (0.0, -0.05, float("nan"), float("inf")):
        assert _call(hip, pts, tri, g) == (hip.OP_ERR_INVALID, 7, 7)
    assert _call(hip, pts, tri, 0.05, mem=7)[0] == hip.OP_ERR_INVALID
    assert _call(hip, pts, tri, 0.05, nv=0)[0] == hip.OP_ERR_INVALID        # triangles over no vertices
    out_p, out_t, n = np.empty_like(pts), np.empty_like(tri), C.c_size_t(0)
    lib = hip.load()
    assert lib.op_mesh_cluster_simplify(vp(pts), vp(col), None, len(pts), vp(tri), len(tri), 0.05, hip.OP_MEM_HOST, 0, vp(out_p), None, None, vp(out_t), C.byref(n),
                                        C.byref(n)) == hip.OP_ERR_INVALID   # colours in, no room out
    assert lib.op_mesh_cluster_simplify(vp(pts), None, None, len(pts), vp(tri), len(tri), 0.05, hip.OP_MEM_HOST, 0, vp(out_p), None, None, None, C.byref(n),
                                        C.byref(n)) == hip.OP_ERR_INVALID   # no room for the triangles
    assert lib.op_mesh_cluster_simplify(vp(pts), None, None, len(pts), vp(tri), len(tri), 0.05, hip.OP_MEM_HOST, 0, vp(out_p), None, None, vp(out_t), None,
                                        C.byref(n)) == hip.OP_ERR_INVALID
    huge = (0xffffffff // 3) + 1  # corners beyond 32-bit indices: refused by the count alone, nothing is read
    assert lib.op_mesh_cluster_simplify(vp(pts), None, None, len(pts), vp(tri), huge, 0.05, hip.OP_MEM_HOST, 0, vp(out_p), None, None, vp(out_t), C.byref(n),
                                        C.byref(n)) == hip.OP_ERR_CAPACITY


@pytest.mark.parametrize("case", sorted(M.PLANTED))
def test_restatement_is_the_host_loop(case, tmp_path):
    assert os.path.exists(M.DRIVER), "examples/cpp/MeshSimplify.bin is not built (make -C examples/cpp)"
    pts, col, nrm, tri, g = M.PLANTED[case]()
    js, got = M.simplify_through_driver(tmp_path, "host", pts, col, nrm, tri, g)
    want = M.cluster_ref(pts, col, nrm, tri, g)
    assert js["points"] == len(pts) and js["triangles"] == len(tri)
    assert js["points_out"] == len(want[0]) and js["triangles_out"] == len(want[3])
    M.check(got, want)
    if case == "one_cell":
        assert len(want[0]) == 0 and len(want[3]) == 0
    elif case == "dropped_representative":
        # P is represented by vertex 0 (colour, normal) though its triangle collapsed; its position is the mean over all FOUR corners that fell into P
        # (vertex 1 counted twice: it is shared by triangles 0 and 3); its number, 1, comes from the surviving triangle [4, 3, 5]; Q and vertex 6 are gone
        assert np.array_equal(want[3], np.array([[0, 1, 2], [3, 4, 5], [2, 0, 1]], np.uint32))
        assert M.same_bits(want[1][1], col[0]) and M.same_bits(want[2][1], nrm[0])
        p64 = pts.astype(np.float64)
        assert M.same_bits(want[0][1], ((((0.0 + p64[0]) + p64[1]) + p64[3]) + p64[1]) / np.float64(4))
        assert len(want[0]) == 6
    elif case == "indexed":
        assert 0 < len(want[3]) < len(tri) and len(want[0]) < len(pts) - 100
