"""Mesh normals and pruning without a GPU: the device entries refuse loudly, the option constant matches the header, and the numpy restatements the
GPU tests compare against are the class surface's host loops, bit for bit (through examples/cpp/MeshPostprocess.bin --mesh, which touches no device on
the host path).  The planted discriminators are shown to discriminate here, so that the GPU tests cannot pass with the wrong order or sign."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mesh_post_common as P

f32, u32 = np.float32, np.uint32
vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)


def _normals(hip, pts, tri, nv=None, nt=None, mem=None, out="own"):
    o = np.empty_like(pts) if isinstance(out, str) else out
    return hip.load().op_mesh_compute_normals(vp(pts), len(pts) if nv is None else nv, vp(tri), len(tri) if nt is None else nt, hip.OP_MEM_HOST if mem is None else mem, 0, vp(o))


def _prune(hip, pts, tri, nt=None, nv=None, mem=None, col=None, outs=None, counts=3):
    out_p, out_c, out_t = outs if outs is not None else (np.empty_like(pts), None if col is None else np.empty_like(pts), np.empty_like(tri))
    n = [C.c_size_t(7) for _ in range(3)]
    ref = [C.byref(x) if i < counts else None for i, x in enumerate(n)]
    rc = hip.load().op_mesh_prune(vp(pts), vp(col), None, len(pts) if nv is None else nv, vp(tri), len(tri) if nt is None else nt, 2, hip.OP_MEM_HOST if mem is None else mem, 0,
                                  vp(out_p), vp(out_c), None, vp(out_t), ref[0], ref[1], ref[2])
    return rc, tuple(x.value for x in n)


def test_entries_fail_loudly_without_a_gpu(hip):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from onepiece_amd import integration as I, registration as R
    from helpers import procedural_mc_table, MC_EDGE_PAIRS
    pts, col, nrm, tri = P.random_soup(21, 1)
    for call in (lambda: R.compute_mesh_normals(pts, tri), lambda: R.prune_mesh(pts, col, nrm, tri, 2)):
        with pytest.raises(hip.OnePieceHipError) as e:
            call()
        assert e.value.code == hip.OP_ERR_NO_DEVICE
    assert _normals(hip, pts, tri[:0]) == hip.OP_ERR_NO_DEVICE  # an empty mesh is no excuse either: as everywhere else, the device comes first
    assert _prune(hip, pts, tri[:0])[0] == hip.OP_ERR_NO_DEVICE
    with pytest.raises(hip.OnePieceHipError):  # (a volume cannot even be created)
        I.CubeHandler().ExtractProcessedTriangleMesh(procedural_mc_table(), MC_EDGE_PAIRS, 0.02, 10, True)
    nv, nt = C.c_size_t(0), C.c_size_t(0)
    assert hip.load().op_volume_extract_mesh_processed(None, None, None, None, 0.02, 0, None, None, None, 0, None, 0, C.byref(nv), C.byref(nt)) == hip.OP_ERR_INVALID


def test_option_constant_matches_the_header_and_round_trips(hip):
    text = open(os.path.join(P.ROOT, "include", "onepiece_hip.h")).read()
    m = re.search(r"#define\s+OP_RUNTIME_OPT_MESH_POSTPROCESS\s+(\d+)", text)
    assert m and int(m.group(1)) == hip.OP_RUNTIME_OPT_MESH_POSTPROCESS == 14
    lib, v = hip.load(), C.c_longlong(-1)
    assert lib.op_abi_version() == 1
    assert lib.op_runtime_get_option(hip.OP_RUNTIME_OPT_MESH_POSTPROCESS, C.byref(v)) == 0 and v.value == 0   # host loops unless asked
    assert lib.op_runtime_set_option(hip.OP_RUNTIME_OPT_MESH_POSTPROCESS, 2) == hip.OP_ERR_INVALID
    assert lib.op_runtime_set_option(hip.OP_RUNTIME_OPT_MESH_POSTPROCESS, -1) == hip.OP_ERR_INVALID
    try:
        assert lib.op_runtime_set_option(hip.OP_RUNTIME_OPT_MESH_POSTPROCESS, 1) == 0
        assert lib.op_runtime_get_option(hip.OP_RUNTIME_OPT_MESH_POSTPROCESS, C.byref(v)) == 0 and v.value == 1
        for other in (hip.OP_RUNTIME_OPT_GLOBAL_REGISTRATION, hip.OP_RUNTIME_OPT_POINT_CLOUD_DOWNSAMPLE, hip.OP_RUNTIME_OPT_MESH_CLUSTERING):  # the neighbours are untouched
            g = C.c_longlong(-1)
            assert lib.op_runtime_get_option(other, C.byref(g)) == 0 and g.value == 0
    finally:
        lib.op_runtime_set_option(hip.OP_RUNTIME_OPT_MESH_POSTPROCESS, 0)


def test_bad_arguments_are_refused_before_any_device_is_looked_for(hip):
    pts, col, _, tri = P.random_soup(10, 2)
    huge = (0xffffffff // 3) + 1  # corners beyond 32-bit indices: refused by the count alone, nothing is read
    assert _normals(hip, pts, tri, mem=7) == hip.OP_ERR_INVALID
    assert _normals(hip, pts, tri, out=None) == hip.OP_ERR_INVALID          # no room for the normals
    assert _normals(hip, None, tri, nv=len(pts)) == hip.OP_ERR_INVALID
    assert _normals(hip, pts, None, nt=len(tri)) == hip.OP_ERR_INVALID
    assert _normals(hip, pts, tri, nv=0, out=None) == hip.OP_ERR_INVALID    # triangles over no vertices
    assert _normals(hip, pts, tri, nt=huge) == hip.OP_ERR_CAPACITY
    assert _prune(hip, pts, tri, mem=7) == (hip.OP_ERR_INVALID, (7, 7, 7))
    assert _prune(hip, pts, tri, nv=0)[0] == hip.OP_ERR_INVALID
    assert _prune(hip, pts, tri, nt=huge) == (hip.OP_ERR_CAPACITY, (7, 7, 7))
    assert _prune(hip, pts, tri, col=col, outs=(np.empty_like(pts), None, np.empty_like(tri)))[0] == hip.OP_ERR_INVALID   # colours in, no room out
    assert _prune(hip, pts, tri, outs=(np.empty_like(pts), None, None))[0] == hip.OP_ERR_INVALID                           # no room for the triangles
    for counts in (0, 1, 2):
        assert _prune(hip, pts, tri, counts=counts)[0] == hip.OP_ERR_INVALID
    nv, nt = C.c_size_t(7), C.c_size_t(7)
    lib = hip.load()
    for g in (-0.05, float("nan"), float("inf")):  # (no volume either: the grid length is looked at first)
        assert lib.op_volume_extract_mesh_processed(None, None, None, None, g, 0, None, None, None, 0, None, 0, C.byref(nv), C.byref(nt)) == hip.OP_ERR_INVALID
        assert "grid_len" in lib.op_last_error().decode()
    assert lib.op_volume_extract_mesh_processed(None, None, None, None, 0.0, 0, None, None, None, 0, None, 0, None, C.byref(nt)) == hip.OP_ERR_INVALID
    assert (nv.value, nt.value) == (7, 7)


@pytest.mark.parametrize("case", sorted(P.PLANTED))
def test_restatements_are_the_host_loops(case, tmp_path):
    assert os.path.exists(P.DRIVER), "examples/cpp/MeshPostprocess.bin is not built (make -C examples/cpp)"
    (pts, col, nrm, tri), min_points = P.PLANTED[case]()
    for op in ("normals", "prune", "both"):
        (tmp_path / op).mkdir()
        js, got = P.post_through_driver(tmp_path / op, "host", op, pts, col, nrm, tri, min_points)
        assert js["points"] == len(pts) and js["triangles"] == len(tri) and js["path"] == "host"
        if op == "normals":
            want = (pts, col, P.normals_ref(pts, tri), tri.astype(u32))
            assert js["pruned"] is None
        else:
            want = (P.prune_ref if op == "prune" else P.both_ref)(pts, col, nrm, tri, min_points)
            assert js["pruned"] == want[4]
        assert js["points_out"] == len(want[0]) and js["triangles_out"] == len(want[3])
        P.check(got, want[:4])
    pruned = P.prune_ref(pts, col, nrm, tri, min_points)
    if case in ("indexed_1366", "islands", "degenerate"):
        assert 0 < len(pruned[3]) < len(tri) and pruned[4] > 0  # some components kept, some dropped
    elif case in ("fan", "strip_decreasing", "grid"):
        assert len(pruned[3]) == len(tri)
    elif case == "strip_shuffled":
        assert len(pruned[3]) == 0 and pruned[4] == 502  # min_points is the component's size: <=


def test_normals_then_prune_is_prune_then_normals():
    for case in ("indexed_1366", "grid", "islands", "degenerate", "fan"):
        (pts, col, _, tri), min_points = P.PLANTED[case]()
        first = P.prune_ref(pts, col, P.normals_ref(pts, tri), tri, min_points)
        second = P.both_ref(pts, col, None, tri, min_points)
        P.check(first[:4], second[:4])
        assert first[4] == second[4]


def _pairwise(a):
    a = a.copy()
    while len(a) > 1:
        if len(a) & 1:
            a = np.concatenate([a, np.zeros(1, a.dtype)])
        a = a[0::2] + a[1::2]
    return a[0]


def test_the_fan_tells_the_in_order_chain_from_a_reversed_one_and_from_a_tree():
    pts, _, _, tri = P.fan()
    centre = P.fan_centre(tri)
    face = P.face_normals(pts, tri)
    corners = np.flatnonzero(tri.reshape(-1) == centre)
    assert len(corners) == 2000
    in_order = P.vertex_sums(face, tri, len(pts))[centre]
    reverse = P.vertex_sums(face, tri, len(pts), order=list(range(3 * len(tri)))[::-1])[centre]
    tree = np.array([_pairwise(face[corners // 3, k]) for k in range(3)], f32)
    assert (P.bits(in_order) != P.bits(reverse)).any() and (P.bits(in_order) != P.bits(tree)).any(), (in_order, reverse, tree)
    assert P.same_bits(P.normals_ref(pts, tri)[centre], P._normalize(in_order.reshape(1, 3))[0])


def test_the_negative_zero_mesh_carries_the_sign_in_the_face_and_loses_it_in_the_vertex():
    for indexed in (False, True):
        pts, _, _, tri = P.negative_zero_mesh(indexed)
        face = P.face_normals(pts, tri)
        signed = (P.bits(face) == 0x80000000)
        assert signed.any(axis=1).all() and signed[:, 0].any() and signed[:, 1].any()  # every face normal has a -0 component, on x or on y
        nrm = P.normals_ref(pts, tri)
        assert not (P.bits(nrm) == 0x80000000).any() and (P.bits(nrm) == 0).any(axis=1).all()  # 0 + (-0) = +0
        # the shortcut that writes the face normal straight into an unshared vertex would differ from the definition
        if not indexed:
            assert (P.bits(np.repeat(face, 3, axis=0)) != P.bits(nrm)).any()


def test_tiny_and_huge_edges_reach_the_ranges_they_are_planted_for():
    tiny = P.scaled_soup(200, -23, -19, 61)
    with np.errstate(under="ignore"):
        a, b = tiny[0][1::3] - tiny[0][0::3], tiny[0][2::3] - tiny[0][0::3]
        prod = np.abs(a[:, 1] * b[:, 2])
    assert ((prod > 0) & (prod < np.finfo(f32).tiny)).any() and (prod == 0).any()      # sub-normal products, and products that vanish
    assert (np.abs(P.normals_ref(tiny[0], tiny[3])) > 0).any()
    large = P.scaled_soup(200, 9, 9, 63)
    n = P.normals_ref(large[0], large[3])
    assert np.isfinite(n).all() and (np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1) < 1e-6).all()  # squares near 1e36: finite
    assert np.isfinite(P.normals_ref(*[P.scaled_soup(200, 18, 18, 62)[i] for i in (0, 3)])).all()           # 1e18: the squared length overflows, no NaN


def test_the_island_boundary_is_less_or_equal():
    mesh, sizes = P.islands()
    pts, col, nrm, tri = mesh
    at = P.prune_ref(pts, col, nrm, tri, sizes[149])        # an island's exact vertex count: that island goes
    below = P.prune_ref(pts, col, nrm, tri, sizes[149] - 1)  # one below: it stays
    assert len(below[3]) - len(at[3]) == 150 and below[4] + sizes[149] == at[4]
    assert at[4] == sum(s for s in sizes if s <= sizes[149])
