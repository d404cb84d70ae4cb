"""Clustering mesh simplification on the device (op_mesh_cluster_simplify, op_volume_extract_mesh_clustered, the opt-in class surface) against the
numpy restatement of the host loop (mesh_cluster_common.cluster_ref; tests/test_mesh_cluster_cpu.py pins that one to the host loop itself).
Every comparison is bitwise on points, colours and normals and exact on the triangles: there are no tolerances.  The shapes are the smallest at
which each kernel can go wrong: corner counts around the wave, the workgroup, a sort tile and 65 536, one cell that holds everything."""
import ctypes as C
import os

import numpy as np
import pytest

import mesh_cluster_common as M

pytestmark = pytest.mark.gpu
bits = M.bits
f32, f64, u32 = np.float32, np.float64, np.uint32
GRID = 0.05

_reference = {}


def reference(key, make):
    """key -> (inputs, restated outputs), computed once and shared; nobody writes to either."""
    if key not in _reference:
        ins = make()
        _reference[key] = (ins, M.cluster_ref(*ins[:5]))
        for a in _reference[key][0][:4] + _reference[key][1]:
            if a is not None:
                a.setflags(write=False)
    return _reference[key]


def _soup(nt):
    pts, col, nrm, tri = M.random_soup(nt, 100 + nt, GRID)
    return pts, col, nrm, tri, GRID


# ---- 1. sizes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attributes", [0, 1, 2], ids=["bare", "colors", "colors+normals"])
@pytest.mark.parametrize("nt", [0, 1, 2, 21, 22, 85, 86, 1366, 23334])
def test_sizes(hip, nt, attributes):
    from onepiece_amd import registration as R
    (pts, col, nrm, tri, g), want = reference(("sizes", nt), lambda: _soup(nt))
    got = R.cluster_simplify(pts, col if attributes >= 1 else None, nrm if attributes >= 2 else None, tri, g)
    M.check(got, (want[0], want[1] if attributes >= 1 else None, want[2] if attributes >= 2 else None, want[3]))
    if nt >= 85:
        assert 0 < len(want[3]) < nt  # some triangles kept, some dropped


# ---- 2. an indexed mesh --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [0.001, 0.03], ids=["merges_nothing", "three_edges"])
def test_indexed_mesh(hip, g):
    from onepiece_amd import registration as R
    (pts, col, nrm, tri, _), want = reference(("indexed", g), lambda: M.grid_mesh() + (g,))
    M.check(R.cluster_simplify(pts, col, nrm, tri, g), want)
    if g == 0.001:  # every vertex its own cell: nothing is dropped, the output is the referenced vertices in order of first appearance
        first = tri.reshape(-1)[np.sort(np.unique(tri.reshape(-1), return_index=True)[1])]
        assert len(want[3]) == len(tri) and len(want[0]) == len(pts) - 100
        assert M.same_bits(want[0], pts[first]) and M.same_bits(want[1], col[first]) and M.same_bits(want[2], nrm[first])
    else:
        assert 0 < len(want[3]) < len(tri)


# ---- 3. / 4. the representative sits in a dropped triangle; a cell only dropped triangles see ------------------------------------------------
def test_representative_in_a_dropped_triangle_and_a_cell_that_vanishes(hip):
    from onepiece_amd import registration as R
    (pts, col, nrm, tri, g), want = reference("dropped", lambda: M.representative_in_a_dropped_triangle() + (1.0,))
    got = R.cluster_simplify(pts, col, nrm, tri, g)
    M.check(got, want)
    assert np.array_equal(got[3], np.array([[0, 1, 2], [3, 4, 5], [2, 0, 1]], u32))  # P's number comes from the surviving triangle; Q left no gap
    assert M.same_bits(got[1][1], col[0]) and M.same_bits(got[2][1], nrm[0])           # the FIRST corner's colour and normal
    p64 = pts.astype(f64)
    assert M.same_bits(got[0][1], ((((0.0 + p64[0]) + p64[1]) + p64[3]) + p64[1]) / f64(4))  # the mean over all corners, the dropped triangle's included
    assert len(got[0]) == 6


# ---- 5. everything in one cell; three interleaved chains ------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [1000, 23334])
def test_everything_in_one_cell(hip, nt):
    from onepiece_amd import registration as R
    pts, col, _, tri = M.one_cell_soup(nt)
    assert len(np.unique(M.cells_of(pts, 1024.0), axis=0)) == 1
    got = R.cluster_simplify(pts, col, None, tri, 1024.0)
    assert got[0].shape == (0, 3) and got[1].shape == (0, 3) and got[2] is None and got[3].shape == (0, 3)


def _pairwise(a):
    a = a.copy()
    while len(a) > 1:
        if len(a) & 1:
            a = np.concatenate([a, np.zeros(1, a.dtype)])
        a = a[0::2] + a[1::2]
    return a[0]


@pytest.mark.parametrize("nt", [128, 23334])
def test_three_interleaved_chains(hip, nt):
    """Each cell is one chain of nt corners whose mean is planted on a float32 rounding tie (mesh_cluster_common.tie_chain): the in-order double
    sum (the definition), a pairwise double sum and a float32 sum give three different float32 means, asserted here on the x axis of cell A.  A
    sum kernel that adds in double by a tree or by atomics in another order, or in float32, cannot produce the restatement's bits."""
    from onepiece_amd import registration as R
    (pts, col, _, tri, g), want = reference(("chains", nt), lambda: M.three_chain_mesh(nt)[:4] + (1e18,))
    assert len(want[0]) == 3 and len(want[3]) == nt
    x = pts[0::3, 0]  # cell A's members, in corner order
    in_order, pairwise, single = np.cumsum(x.astype(f64))[-1], _pairwise(x.astype(f64)), np.cumsum(x, dtype=f32)[-1]
    word = lambda v: int(np.asarray(v, f32).view(u32))
    means = [word(f32(in_order / f64(nt))), word(f32(pairwise / f64(nt))), word(single / f32(nt))]
    assert len(set(means)) == 3 and word(f32(f64(single) / f64(nt))) not in means[:2], [hex(v) for v in means]
    assert means[1] == means[0] + 1  # the tie: one float32 apart
    assert word(want[0][0, 0]) == means[0] and word(want[0][1, 0]) == means[0] and word(-want[0][2, 0]) == means[0]
    M.check(R.cluster_simplify(pts, col, None, tri, g), want)


# ---- 6. cell boundaries --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [0.00625, 0.01, 0.05])
def test_cell_boundaries(hip, g):
    from onepiece_amd import registration as R
    bad = M.reciprocal_mismatches(g)
    assert len(bad) >= 100, "only %d values with floorf(p / g) != floorf(p * (1 / g)) for grid_len %g" % (len(bad), g)
    planted = bad[:: max(1, len(bad) // 300)][:300]
    (pts, col, _, tri, _), want = reference(("boundaries", g), lambda: M.boundary_soup(g, planted) + (g,))
    assert (pts < 0).any() and (M.cells_of(pts, g) != np.trunc(pts / f32(g))).any()  # floor is not trunc here
    assert len(want[3]) == len(tri)
    M.check(R.cluster_simplify(pts, col, None, tri, g), want)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["nan", "inf", "beyond_int", "too_wide", "grid_len_0", "index"])
def test_refusals_return_their_code_and_leave_the_device_usable(hip, what):
    from onepiece_amd import registration as R
    (pts, col, nrm, tri, g), want = reference(("sizes", 1366), lambda: _soup(1366))
    bad, bad_tri, code = pts.copy(), tri.copy(), hip.OP_ERR_INVALID
    if what == "nan":
        bad[1234, 1] = np.nan
    elif what == "inf":
        bad[4097, 2] = -np.inf
    elif what == "beyond_int":
        bad[77, 0] = 1.0e9  # / 0.05 = 2e10
    elif what == "too_wide":
        bad, _, _, bad_tri = M.too_wide_mesh(g)
        code = hip.OP_ERR_CAPACITY
    elif what == "index":
        bad_tri[700, 1] = len(pts)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    out_p, out_c, out_t = np.full_like(bad, 7.5), np.full_like(bad, 7.5), np.full_like(bad_tri, 77)
    nv, nt = C.c_size_t(9), C.c_size_t(9)
    rc = hip.load().op_mesh_cluster_simplify(vp(bad), vp(bad), None, len(bad), vp(bad_tri), len(bad_tri), 0.0 if what == "grid_len_0" else g, hip.OP_MEM_HOST, 0,
                                             vp(out_p), vp(out_c), None, vp(out_t), C.byref(nv), C.byref(nt))
    assert rc == code
    assert (out_p == 7.5).all() and (out_c == 7.5).all() and (out_t == 77).all()  # nothing written
    if what == "too_wide":
        assert "3000" in hip.load().op_last_error().decode()  # the message names the extent (3 000 0xx cells)
    M.check(R.cluster_simplify(pts, col, nrm, tri, g), want)


# ---- 8. device memory ----------------------------------------------------------------------------------------------------------------------
def test_device_memory_gives_the_same_bits(hip):
    from onepiece_amd import registration as R
    (pts, col, nrm, tri, g), want = reference(("sizes", 1366), lambda: _soup(1366))
    M.check(R.cluster_simplify(pts, col, nrm, tri, g, device_memory=True), want)
    (ipts, icol, inrm, itri, ig), iwant = reference(("indexed", 0.03), lambda: M.grid_mesh() + (0.03,))
    M.check(R.cluster_simplify(ipts, icol, inrm, itri, ig, device_memory=True), iwant)


# ---- 9. fused entry ------------------------------------------------------------------------------------------------------------------------
RES = 0.02


@pytest.fixture(scope="module")
def volumes():
    from onepiece_amd import integration as I, synthetic as S
    from helpers import small_camera
    cam = small_camera(4)
    out = {}
    for frames in ((0,), (0, 10, 20)):
        hcam = I.PinholeCamera()
        hcam.fx, hcam.fy, hcam.cx, hcam.cy, hcam.width, hcam.height, hcam.depth_scale = cam
        hv = I.CubeHandler(hcam, max_blocks=1 << 16)
        hv.SetVoxelResolution(RES)
        for i in frames:
            pose = S.room_pose(i)
            d, c = S.room_render(pose, width=cam[4], height=cam[5], fx=cam[0], fy=cam[1], cx=cam[2], cy=cam[3])
            hv.IntegrateImage(d, c, pose)
        out[frames] = hv
    return out


@pytest.mark.parametrize("g", [RES, 2 * RES], ids=["res", "2res"])
@pytest.mark.parametrize("frames", [(0,), (0, 10, 20)], ids=["1frame", "3frames"])
def test_fused_entry(hip, volumes, frames, g):
    from onepiece_amd import registration as R
    from helpers import procedural_mc_table, MC_EDGE_PAIRS
    hv, tab = volumes[frames], procedural_mc_table()
    pts, col = hv.ExtractTriangleMesh(tab, MC_EDGE_PAIRS)
    assert len(pts) > 3000 and len(pts) % 3 == 0
    tri = M.soup_triangles(len(pts) // 3)
    want = M.cluster_ref(pts, col, None, tri, g)
    assert 0 < len(want[3]) < len(tri)
    two_steps = R.cluster_simplify(pts, col, None, tri, g)
    M.check(two_steps, want)
    fp, fc, ft = hv.ExtractSimplifiedTriangleMesh(tab, MC_EDGE_PAIRS, g)
    M.check((fp, fc, None, ft), two_steps)


def test_fused_entry_one_block_empty_volume_full_collapse_and_small_buffers(hip, volumes):
    from onepiece_amd import integration as I, registration as R
    from helpers import procedural_mc_table, MC_EDGE_PAIRS
    hv, tab = volumes[(0, 10, 20)], procedural_mc_table()
    keys, _ = hv.GetCubeMap()
    checked = 0
    for k in keys[:: max(1, len(keys) // 12)]:  # only_block
        pts, col = hv.GenerateMeshByCube(k, tab, MC_EDGE_PAIRS)
        got = hv.ExtractSimplifiedTriangleMesh(tab, MC_EDGE_PAIRS, RES, only_block=k)
        want = M.cluster_ref(pts, col, None, M.soup_triangles(len(pts) // 3), RES) if len(pts) else (np.zeros((0, 3), f32), None, None, np.zeros((0, 3), u32))
        M.check((got[0], got[1], None, got[2]), want)
        checked += len(want[3])
    assert checked > 0
    assert all(len(a) == 0 for a in hv.ExtractSimplifiedTriangleMesh(tab, MC_EDGE_PAIRS, RES, only_block=(9999, 9999, 9999)))
    empty = I.CubeHandler()
    empty.SetVoxelResolution(RES)
    assert all(len(a) == 0 for a in empty.ExtractSimplifiedTriangleMesh(tab, MC_EDGE_PAIRS, RES))
    one = volumes[(0,)]
    k1, _ = one.GetCubeMap()
    meshed = ((k, one.GenerateMeshByCube(k, tab, MC_EDGE_PAIRS)[0]) for k in k1)
    keys0 = [next(k for k, p in meshed if len(p) and len(np.unique(M.cells_of(p, 100 * RES), axis=0)) == 1)]  # a block with a mesh, inside one 2 m cell
    collapsed = one.ExtractSimplifiedTriangleMesh(tab, MC_EDGE_PAIRS, 100 * RES)
    soup_p, soup_c = one.ExtractTriangleMesh(tab, MC_EDGE_PAIRS)
    few = M.cluster_ref(soup_p, soup_c, None, M.soup_triangles(len(soup_p) // 3), 100 * RES)  # 2 m cells: all but the triangles across a cell wall collapse
    assert len(few[3]) * 20 < len(soup_p) // 3
    M.check((collapsed[0], collapsed[1], None, collapsed[2]), few)
    gone = one.ExtractSimplifiedTriangleMesh(tab, MC_EDGE_PAIRS, 100 * RES, only_block=keys0[0])  # one 16 cm block inside one 2 m cell: nothing is left
    assert len(one.GenerateMeshByCube(keys0[0], tab, MC_EDGE_PAIRS)[0]) > 0 and all(len(a) == 0 for a in gone)
    # refusals of the fused entry: grid_len 0, buffers one row short -- the code, nothing written, the true sizes reported, and the volume still answers
    lib, L = hip.load(), hip
    tt, ep = np.ascontiguousarray(tab, np.int32).reshape(-1), np.ascontiguousarray(MC_EDGE_PAIRS, np.int32).reshape(-1)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    vp = lambda a: C.c_void_p(a.ctypes.data)
    want = hv.ExtractSimplifiedTriangleMesh(tab, MC_EDGE_PAIRS, RES)
    nv, nt = C.c_size_t(0), C.c_size_t(0)
    assert lib.op_volume_extract_mesh_clustered(hv._h, ip(tt), ip(ep), None, 0.0, None, None, 0, None, 0, C.byref(nv), C.byref(nt)) == L.OP_ERR_INVALID
    assert lib.op_volume_extract_mesh_clustered(hv._h, ip(tt), ip(ep), None, RES, None, None, 0, None, 0, C.byref(nv), C.byref(nt)) == 0
    assert nv.value >= len(want[0]) and nt.value >= len(want[2]) and nv.value == 3 * nt.value  # upper bounds: the soup's sizes
    for short_v, short_t in ((1, 0), (0, 1)):
        p, c, t = np.full((len(want[0]), 3), 7.5, f32), np.full((len(want[0]), 3), 7.5, f32), np.full((len(want[2]), 3), 77, u32)
        rc = lib.op_volume_extract_mesh_clustered(hv._h, ip(tt), ip(ep), None, RES, vp(p), vp(c), len(p) - short_v, vp(t), len(t) - short_t, C.byref(nv), C.byref(nt))
        assert rc == L.OP_ERR_CAPACITY and (nv.value, nt.value) == (len(want[0]), len(want[2]))
        assert (p == 7.5).all() and (c == 7.5).all() and (t == 77).all()
    p, c, t = np.empty((len(want[0]), 3), f32), np.empty((len(want[0]), 3), f32), np.empty((len(want[2]), 3), u32)
    assert lib.op_volume_extract_mesh_clustered(hv._h, ip(tt), ip(ep), None, RES, vp(p), vp(c), len(p), vp(t), len(t), C.byref(nv), C.byref(nt)) == 0  # exactly enough
    M.check((p, c, None, t), (want[0], want[1], None, want[2]))


# ---- 10. class surface ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def room_dumps(tmp_path_factory):
    assert os.path.exists(M.DRIVER), "examples/cpp/MeshSimplify.bin is not built (make -C examples/cpp)"
    out = {}
    for path in ("host", "device", "fused"):
        d = str(tmp_path_factory.mktemp("mesh_" + path))
        out[path] = (d, M.run_driver(["--frames", 3, "--res", RES, "--warmup", 0, "--path", path, "--dump", d]))
    return out


def _soup_of(directory):
    return tuple(np.fromfile(os.path.join(directory, "soup_%s.f32" % name), f32).reshape(-1, 3) for name in ("points", "colors"))


def test_extract_and_simplify_is_the_same_mesh_on_all_three_paths(hip, room_dumps):
    """Every path dumps the bits of the host loop.  The loop's result follows the ORDER of the soup (cells and vertices by first appearance, sums in
    corner order), the soup follows the pool order of the blocks, and the order in which a frame's blocks enter the pool (an atomic counter) differs
    from one process to the next -- on the host path too.  So each process also dumps the soup of its own volume: the three soups are the same
    triangles, and each path's files are, bit for bit, the restatement of the host loop on that process's own soup (files of two processes are
    identical exactly when their pool orders are)."""
    from helpers import triangle_soup
    host_dir, host_js = room_dumps["host"]
    host_soup = _soup_of(host_dir)
    assert host_js["soup_triangles"] == len(host_soup[0]) // 3 > host_js["triangles_out"] > 1000
    for path in ("host", "device", "fused"):
        d, js = room_dumps[path]
        pts, col = _soup_of(d)
        got = M.read_mesh(d)
        assert js["path"] == path and got[1] is not None and got[2] is None
        assert (js["soup_triangles"], js["points_out"], js["triangles_out"]) == (host_js["soup_triangles"], host_js["points_out"], host_js["triangles_out"])
        assert (len(got[0]), len(got[3])) == (js["points_out"], js["triangles_out"])
        assert np.array_equal(bits(triangle_soup(pts, col)), bits(triangle_soup(*host_soup))), "%s: not the host path's triangles" % path
        M.check(got, M.cluster_ref(pts, col, None, M.soup_triangles(len(pts) // 3), RES))
        if np.array_equal(bits(pts), bits(host_soup[0])):  # the same pool order: then the same files
            M.check(got, M.read_mesh(host_dir))


def test_class_surface_falls_back_for_a_mesh_the_device_refuses(hip, tmp_path):
    pts, col, nrm, tri = M.too_wide_mesh(GRID)
    want = M.cluster_ref(pts, col, nrm, tri, GRID)
    for path in ("host", "device"):
        (tmp_path / path).mkdir()
        _, got = M.simplify_through_driver(tmp_path / path, path, pts, col, nrm, tri, GRID)
        M.check(got, want)
    (ipts, icol, inrm, itri, ig), iwant = reference(("indexed", 0.03), lambda: M.grid_mesh() + (0.03,))  # and a mesh the device takes goes through it with the same bits
    (tmp_path / "ok").mkdir()
    _, got = M.simplify_through_driver(tmp_path / "ok", "device", ipts, icol, inrm, itri, ig)
    M.check(got, iwant)
