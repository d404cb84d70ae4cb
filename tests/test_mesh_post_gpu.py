"""Mesh normals and small-component pruning on the device (op_mesh_compute_normals, op_mesh_prune, op_volume_extract_mesh_processed, the opt-in class
surface) against the numpy restatements of the host loops (mesh_post_common.normals_ref / prune_ref; tests/test_mesh_post_cpu.py pins those to the host
loops themselves and shows that the planted discriminators discriminate).  Every comparison is bitwise on points, colours and normals and exact on the
triangles and counts: there are no tolerances.  The shapes are the smallest at which each kernel can go wrong: corner counts around the wave and the
workgroup, a long chain, one contended root, hooks that always re-root."""
import ctypes as C
import os

import numpy as np
import pytest

import mesh_cluster_common as M
import mesh_post_common as P
from test_mesh_cluster_gpu import RES, volumes  # noqa: F401  (the small 1- and 3-frame volumes, a module-scoped fixture)

pytestmark = pytest.mark.gpu
bits = P.bits
f32, u32 = np.float32, np.uint32
SIZES = [0, 1, 2, 21, 22, 85, 86, 1366, 23334]

_cache = {}


def cached(key, make):
    """key -> value, computed once and shared; nobody writes to it."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _mesh(kind, nt):
    return cached((kind, nt), lambda: P.random_soup(nt, 100 + nt) if kind == "soup" else P.indexed_mesh(nt, 200 + nt))


def _normals_want(key, mesh):
    return cached(("normals",) + key, lambda: P.normals_ref(mesh[0], mesh[3]))


def _prune_want(key, mesh, min_points):
    return cached(("prune", min_points) + key, lambda: P.prune_ref(*mesh, min_points))


def same(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype
    assert np.array_equal(bits(a), bits(b)), "%d of %d words differ" % (int((bits(a) != bits(b)).sum()), b.size)


def check_prune(got, want):
    P.check(got[:4], want[:4])
    assert got[4] == want[4], "pruned %d, expected %d" % (got[4], want[4])


# ---- 1. sizes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["soup", "indexed"])
@pytest.mark.parametrize("nt", SIZES)
def test_normals_sizes(hip, nt, kind):
    from onepiece_amd import registration as R
    mesh = _mesh(kind, nt)
    same(R.compute_mesh_normals(mesh[0], mesh[3]), _normals_want((kind, nt), mesh))


@pytest.mark.parametrize("attributes", [0, 1, 2], ids=["bare", "colors", "colors+normals"])
@pytest.mark.parametrize("kind", ["soup", "indexed"])
@pytest.mark.parametrize("nt", SIZES)
def test_prune_sizes(hip, nt, kind, attributes):
    from onepiece_amd import registration as R
    pts, col, nrm, tri = _mesh(kind, nt)
    min_points = 4 if kind == "indexed" else 2  # indexed: single triangles and pairs go, the large component stays; a soup (3 vertices each) stays whole
    want = _prune_want((kind, nt), (pts, col, nrm, tri), min_points)
    got = R.prune_mesh(pts, col if attributes >= 1 else None, nrm if attributes >= 2 else None, tri, min_points)
    check_prune(got, (want[0], want[1] if attributes >= 1 else None, want[2] if attributes >= 2 else None, want[3], want[4]))
    if kind == "indexed" and nt >= 1366:
        assert 0 < len(want[3]) < nt and want[4] > 0


# ---- 2. normals: the planted meshes --------------------------------------------------------------------------------------------------------
NORMALS_CASES = {
    "grid": lambda: P.grid_mesh(),
    "fan": lambda: P.fan(),
    "degenerate": lambda: P.repeated_and_degenerate(),
    "negative_zero_indexed": lambda: P.negative_zero_mesh(True),
    "negative_zero_soup": lambda: P.negative_zero_mesh(False),
    "tiny_edges": lambda: P.scaled_soup(200, -23, -19, 61),
    "huge_edges": lambda: P.scaled_soup(200, 18, 18, 62),
    "large_edges": lambda: P.scaled_soup(200, 9, 9, 63),
}


@pytest.mark.parametrize("case", sorted(NORMALS_CASES))
def test_normals_planted(hip, case):
    """The fan is the order discriminator and the negative-zero meshes the sign discriminator (asserted without a GPU in test_mesh_post_cpu.py): a
    vertex sum by a tree or by float atomics, or a face normal written straight into an unshared vertex, cannot give these bits."""
    from onepiece_amd import registration as R
    mesh = cached(("planted", case), NORMALS_CASES[case])
    want = _normals_want(("planted", case), mesh)
    got = R.compute_mesh_normals(mesh[0], mesh[3])
    same(got, want)
    if case == "grid":
        used = np.zeros(len(mesh[0]), bool)
        used[mesh[3].reshape(-1)] = True
        assert (~used).sum() == 100 and (bits(got[~used]) == 0).all()  # a vertex nothing refers to keeps (+0, +0, +0)
    elif case == "degenerate":
        assert (bits(got[6]) == 0).all() and (bits(got[7]) == 0).all()  # a point three times contributes zeros
    elif case.startswith("negative_zero"):
        assert not (bits(got) == 0x80000000).any()


def test_normals_overwrite_and_an_empty_mesh_gives_zeros(hip):
    pts, _, _, tri = _mesh("indexed", 86)
    out = np.full_like(pts, 7.5)
    assert hip.load().op_mesh_compute_normals(C.c_void_p(pts.ctypes.data), len(pts), None, 0, hip.OP_MEM_HOST, 0, C.c_void_p(out.ctypes.data)) == 0
    assert (bits(out) == 0).all()  # nt == 0: nv rows of zeros


# ---- 3. prune: the planted meshes ----------------------------------------------------------------------------------------------------------
def _prune_cases():
    cases = {"strip_decreasing": (P.strip(5000), [100, 5001, 5002]), "strip_shuffled": (P.strip(5000, True), [100, 5001, 5002]), "fan": (P.fan(), [0, 2001, 2002]),
             "grid": (P.grid_mesh(), [0, 10, 1 << 40])}
    for name, mesh in P.small_cases().items():
        cases[name] = (mesh, [0, 1, 2, 3, 4, 5, 6])
    return cases


PRUNE_NAMES = ["strip_decreasing", "strip_shuffled", "fan", "grid", "one", "share_vertex", "share_edge", "disjoint", "vvw"]


@pytest.mark.parametrize("case", PRUNE_NAMES)
def test_prune_planted(hip, case):
    """decreasing ids: in triangle order every hook re-roots the component; the fan: every union meets at one root; min_points 0 keeps everything
    referenced, a min_points above everything leaves an empty mesh without attributes"""
    from onepiece_amd import registration as R
    mesh, thresholds = cached("prune_cases", _prune_cases)[case]
    for min_points in thresholds:
        want = _prune_want(("planted", case), mesh, min_points)
        check_prune(R.prune_mesh(*mesh, min_points), want)
    sizes = [len(_prune_want(("planted", case), mesh, m)[3]) for m in thresholds]
    assert sizes[0] == len(mesh[3]) and sizes[-1] == 0  # the first keeps every triangle, the last none
    empty = R.prune_mesh(*mesh, thresholds[-1])
    assert all(len(a) == 0 for a in empty[:4]) and empty[4] == len(np.unique(mesh[3]))


def test_prune_islands_at_and_below_an_exact_size(hip):
    """300 islands of 1 .. 300 triangles (3 .. 302 vertices): min_points at an island's exact vertex count drops it (<=), one below keeps it"""
    from onepiece_amd import registration as R
    mesh, sizes = cached("islands", P.islands)
    for island in (1, 150, 300):
        at, below = sizes[island - 1], sizes[island - 1] - 1
        got_at, got_below = R.prune_mesh(*mesh, at), R.prune_mesh(*mesh, below)
        check_prune(got_at, _prune_want(("islands",), mesh, at))
        check_prune(got_below, _prune_want(("islands",), mesh, below))
        assert len(got_below[3]) - len(got_at[3]) == island and got_at[4] - got_below[4] == at


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["nan", "inf", "index"])
def test_refusals_return_their_code_write_nothing_and_leave_the_device_usable(hip, what):
    from onepiece_amd import registration as R
    mesh = _mesh("indexed", 1366)
    pts, col, nrm, tri = mesh
    bad, bad_tri = pts.copy(), tri.copy()
    if what == "index":
        bad_tri[700, 1] = len(pts)
    else:
        bad[int(tri[333, 2]), 1] = np.nan if what == "nan" else -np.inf
    vp = lambda a: C.c_void_p(a.ctypes.data)
    lib = hip.load()
    out = np.full_like(bad, 7.5)
    assert lib.op_mesh_compute_normals(vp(bad), len(bad), vp(bad_tri), len(bad_tri), hip.OP_MEM_HOST, 0, vp(out)) == hip.OP_ERR_INVALID
    assert (out == 7.5).all()
    if what == "index":
        out_p, out_c, out_t = np.full_like(bad, 7.5), np.full_like(bad, 7.5), np.full_like(bad_tri, 77)
        n = [C.c_size_t(9) for _ in range(3)]
        rc = lib.op_mesh_prune(vp(bad), vp(col), None, len(bad), vp(bad_tri), len(bad_tri), 4, hip.OP_MEM_HOST, 0, vp(out_p), vp(out_c), None, vp(out_t), C.byref(n[0]), C.byref(n[1]),
                               C.byref(n[2]))
        assert rc == hip.OP_ERR_INVALID and (out_p == 7.5).all() and (out_c == 7.5).all() and (out_t == 77).all() and [x.value for x in n] == [0, 0, 0]
    else:  # pruning reads no coordinate: the same mesh prunes
        got = R.prune_mesh(bad, col, None, tri, 4)
        want = _prune_want(("indexed", 1366), mesh, 4)
        assert np.array_equal(got[3], want[3]) and got[4] == want[4]
    same(R.compute_mesh_normals(pts, tri), _normals_want(("indexed", 1366), mesh))  # the next good call
    check_prune(R.prune_mesh(pts, col, nrm, tri, 4), _prune_want(("indexed", 1366), mesh, 4))


def test_nan_at_an_unreferenced_vertex_is_accepted(hip):
    from onepiece_amd import registration as R
    mesh = cached(("planted", "grid"), NORMALS_CASES["grid"])
    bad = P.with_nan(mesh, referenced=False)
    got = R.compute_mesh_normals(bad[0], bad[3])
    same(got, _normals_want(("planted", "grid"), mesh))  # (the vertex is never read: its normal is zero like every unreferenced one's)


# ---- 5. device memory ----------------------------------------------------------------------------------------------------------------------
def test_device_memory_gives_the_same_bits(hip):
    from onepiece_amd import registration as R
    for key in (("soup", 1366), ("indexed", 1366)):
        mesh = _mesh(*key)
        same(R.compute_mesh_normals(mesh[0], mesh[3], device_memory=True), _normals_want(key, mesh))
        m = 4 if key[0] == "indexed" else 2
        check_prune(R.prune_mesh(*mesh, m, device_memory=True), _prune_want(key, mesh, m))
    fan = cached(("planted", "fan"), NORMALS_CASES["fan"])
    same(R.compute_mesh_normals(fan[0], fan[3], device_memory=True), _normals_want(("planted", "fan"), fan))


# ---- 6. fused entry ------------------------------------------------------------------------------------------------------------------------
def _tail_ref(pts, col, g, min_points, normals):
    """ExtractTriangleMesh's soup through the restatements -> (points, colors, normals or None, triangles)"""
    m = (pts, col, None, M.soup_triangles(len(pts) // 3))
    if g > 0 and len(pts):
        m = M.cluster_ref(pts, col, None, m[3], g)
    if min_points > 0 and len(m[3]):
        m = P.prune_ref(m[0], m[1], None, m[3], min_points)[:4]
    nrm = P.normals_ref(m[0], m[3]) if normals and len(m[3]) else None
    return m[0], m[1], nrm, m[3]


def _soup(volumes, frames):  # noqa: F811
    from helpers import procedural_mc_table, MC_EDGE_PAIRS
    return cached(("soup", frames), lambda: volumes[frames].ExtractTriangleMesh(procedural_mc_table(), MC_EDGE_PAIRS))


@pytest.mark.parametrize("normals", [False, True], ids=["plain", "normals"])
@pytest.mark.parametrize("min_points", [0, 50])
@pytest.mark.parametrize("g", [0.0, RES, 2 * RES], ids=["soup", "res", "2res"])
@pytest.mark.parametrize("frames", [(0,), (0, 10, 20)], ids=["1frame", "3frames"])
def test_fused_entry(hip, volumes, frames, g, min_points, normals):  # noqa: F811
    from helpers import procedural_mc_table, MC_EDGE_PAIRS
    pts, col = _soup(volumes, frames)
    assert len(pts) > 3000 and len(pts) % 3 == 0
    base = cached(("tail", frames, g, min_points), lambda: _tail_ref(pts, col, g, min_points, False))
    want = (base[0], base[1], cached(("tail_normals", frames, g, min_points), lambda: P.normals_ref(base[0], base[3])) if normals and len(base[3]) else None, base[3])
    got = volumes[frames].ExtractProcessedTriangleMesh(procedural_mc_table(), MC_EDGE_PAIRS, g, min_points, normals)
    if not len(want[3]):
        assert all(a is None or len(a) == 0 for a in got)
        assert min_points == 50  # everything pruned (at g == 0 always: an unshared triangle is a component of three vertices)
        return
    P.check(got, want)
    if g == 0.0:
        assert np.array_equal(got[3].reshape(-1), np.arange(len(pts), dtype=u32))  # the soup, triangles[c] = c
    if g == 0.0:
        assert min_points == 0


def test_fused_entry_one_block_empty_volume_and_small_buffers(hip, volumes):  # noqa: F811
    from onepiece_amd import integration as I
    from helpers import procedural_mc_table, MC_EDGE_PAIRS
    hv, tab = volumes[(0, 10, 20)], procedural_mc_table()
    keys, _ = hv.GetCubeMap()
    checked = 0
    for k in keys[:: max(1, len(keys) // 8)]:  # only_block
        pts, col = hv.GenerateMeshByCube(k, tab, MC_EDGE_PAIRS)
        got = hv.ExtractProcessedTriangleMesh(tab, MC_EDGE_PAIRS, RES, 3, True, only_block=k)
        want = _tail_ref(pts, col, RES, 3, True)
        if len(want[3]):
            P.check(got, want)
        else:
            assert all(a is None or len(a) == 0 for a in got)
        checked += len(want[3])
    assert checked > 0
    assert all(a is None or len(a) == 0 for a in hv.ExtractProcessedTriangleMesh(tab, MC_EDGE_PAIRS, RES, 3, True, only_block=(9999, 9999, 9999)))
    empty = I.CubeHandler()
    empty.SetVoxelResolution(RES)
    assert all(a is None or len(a) == 0 for a in empty.ExtractProcessedTriangleMesh(tab, MC_EDGE_PAIRS, RES, 50, True))
    # the sizing call's bounds, buffers one row short -- the code, nothing written, the true sizes reported -- and exactly enough
    lib, L = hip.load(), hip
    tt, ep = np.ascontiguousarray(tab, np.int32).reshape(-1), np.ascontiguousarray(MC_EDGE_PAIRS, np.int32).reshape(-1)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    vp = lambda a: C.c_void_p(a.ctypes.data)
    want = hv.ExtractProcessedTriangleMesh(tab, MC_EDGE_PAIRS, RES, 50, True)
    soup = _soup(volumes, (0, 10, 20))[0]
    nv, nt = C.c_size_t(0), C.c_size_t(0)
    assert lib.op_volume_extract_mesh_processed(hv._h, ip(tt), ip(ep), None, -1.0, 50, None, None, None, 0, None, 0, C.byref(nv), C.byref(nt)) == L.OP_ERR_INVALID
    assert lib.op_volume_extract_mesh_processed(hv._h, ip(tt), ip(ep), None, RES, 50, None, None, None, 0, None, 0, C.byref(nv), C.byref(nt)) == 0
    assert (nv.value, nt.value) == (len(soup), len(soup) // 3) and nv.value >= len(want[0]) and nt.value >= len(want[3])  # upper bounds: the soup's sizes
    for short_v, short_t in ((1, 0), (0, 1)):
        p, c, n = (np.full((len(want[0]), 3), 7.5, f32) for _ in range(3))
        t = np.full((len(want[3]), 3), 77, u32)
        rc = lib.op_volume_extract_mesh_processed(hv._h, ip(tt), ip(ep), None, RES, 50, vp(p), vp(c), vp(n), len(p) - short_v, vp(t), len(t) - short_t, C.byref(nv), C.byref(nt))
        assert rc == L.OP_ERR_CAPACITY and (nv.value, nt.value) == (len(want[0]), len(want[3]))
        assert (p == 7.5).all() and (c == 7.5).all() and (n == 7.5).all() and (t == 77).all()
    p, c, n, t = np.empty((len(want[0]), 3), f32), np.empty((len(want[0]), 3), f32), np.empty((len(want[0]), 3), f32), np.empty((len(want[3]), 3), u32)
    assert lib.op_volume_extract_mesh_processed(hv._h, ip(tt), ip(ep), None, RES, 50, vp(p), vp(c), vp(n), len(p), vp(t), len(t), C.byref(nv), C.byref(nt)) == 0
    P.check((p, c, n, t), want)


# ---- 7. class surface ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["indexed_1366", "fan", "degenerate", "negative_zero_soup", "islands"])
def test_class_surface_device_path_equals_the_host_path(hip, case, tmp_path):
    assert os.path.exists(P.DRIVER), "examples/cpp/MeshPostprocess.bin is not built (make -C examples/cpp)"
    (pts, col, nrm, tri), min_points = P.PLANTED[case]()
    want = P.both_ref(pts, col, nrm, tri, min_points)
    out = {}
    for path in ("host", "device"):
        (tmp_path / path).mkdir()
        js, out[path] = P.post_through_driver(tmp_path / path, path, "both", pts, col, nrm, tri, min_points)
        assert js["path"] == path and js["pruned"] == want[4]
        P.check(out[path], want[:4])
    P.check(out["device"], out["host"])


def test_class_surface_falls_back_for_a_mesh_the_device_refuses(hip, tmp_path):
    (mesh, min_points) = P.PLANTED["grid"]()
    pts, col, nrm, tri = P.with_nan(mesh, referenced=True)
    out = {}
    for path in ("host", "device"):
        (tmp_path / path).mkdir()
        _, out[path] = P.post_through_driver(tmp_path / path, path, "normals", pts, col, nrm, tri, min_points)
    assert np.isnan(out["host"][2]).any()
    P.check(out["device"], out["host"])  # NaN rows included: the host loop ran on both paths


@pytest.fixture(scope="module")
def room_dumps(tmp_path_factory):
    assert os.path.exists(P.DRIVER), "examples/cpp/MeshPostprocess.bin is not built (make -C examples/cpp)"
    out = {}
    for path in ("host", "device", "fused"):
        d = str(tmp_path_factory.mktemp("post_" + path))
        out[path] = (d, P.run_driver(["--frames", 3, "--res", RES, "--grid", RES, "--min-points", 50, "--normals", "--warmup", 0, "--path", path, "--dump", d]))
    return out


def test_the_whole_tail_is_the_same_mesh_on_all_three_paths(hip, room_dumps):
    """Pool order, hence soup order, differs between processes: each path is compared with the restatements applied to the soup
    that its own process dumped; the sizes, which do not depend on the order, agree across the paths."""
    host_js = room_dumps["host"][1]
    for path in ("host", "device", "fused"):
        d, js = room_dumps[path]
        pts, col = (np.fromfile(os.path.join(d, "soup_%s.f32" % name), f32).reshape(-1, 3) for name in ("points", "colors"))
        got = P.read_mesh(d)
        want = _tail_ref(pts, col, RES, 50, True)
        assert js["path"] == path and js["soup_triangles"] == len(pts) // 3 == host_js["soup_triangles"]
        assert (js["points_out"], js["triangles_out"]) == (len(want[0]), len(want[3])) == (host_js["points_out"], host_js["triangles_out"])
        assert 1000 < len(want[3])
        if path != "fused":
            clustered = M.cluster_ref(pts, col, None, M.soup_triangles(len(pts) // 3), RES)
            assert js["pruned"] == P.prune_ref(clustered[0], clustered[1], None, clustered[3], 50)[4]
        P.check(got, want)
