"""Per-call device temporaries live in an op::Scope bound to the stream that uses them (csrc/common.hpp): whatever way an entry point leaves -- done,
refused, or because an allocation failed half way -- every buffer it took from the buffer cache is back there.

The buffer cache keeps what it has handed out in a live set; op_debug_cache_live counts it.  Every case reads the count before it creates its
objects and again after it has destroyed them.  The allocation failures are injected: OP_RUNTIME_OPT_ALLOC_FAULT = k makes the k-th request to
the cache from now return hipErrorOutOfMemory on the host, before HIP or the cache is touched (no GPU fault is involved), and is 0 again once it
has fired.  Sweeping k = 1, 2, ... fails every allocation of an entry in turn; the first k at which the call succeeds is the number of requests
the entry makes plus one, and that number is asserted from a reading of the code (the `allocs` of every entry below).

Before these entries moved onto op::Scope the sweep failed for op_volume_upload alone (three buffers left in the live set: a row of OP_HIP
allocations lost the earlier ones when a later one failed); the temporaries op_icp_create lost were lost on failing copies and synchronisations,
which this hook does not inject.

Inputs are the smallest that reach every allocation: volumes of 3 hand-made blocks entered through op_volume_upload, a 16 x 12 camera, clouds of
200 points, the procedural marching-cubes table of tests/helpers.py."""
import ctypes as C
import gc

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

W_, H_, NPX = 16, 12, 16 * 12
NPTS = 200
SWEEP_CAP = 64


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _blocks(keys, seed):
    """3 blocks whose sdf crosses zero on a diagonal plane of each block (whatever the order of the 512 voxels in it), all observed."""
    idx = np.arange(512)
    a, b, c = idx % 8, (idx // 8) % 8, idx // 64
    vox = np.empty((len(keys), 512, 5), np.float32)
    for i in range(len(keys)):
        vox[i, :, 0] = ((a + b + c) - 10.3 - 0.5 * i - 0.25 * seed) * 0.004
        vox[i, :, 1] = 1 + (idx + i + seed) % 3
        vox[i, :, 2], vox[i, :, 3], vox[i, :, 4] = 0.25 + a / 16.0, 0.25 + b / 16.0, 0.25 + c / 16.0
    return np.asarray(keys, np.int32), vox


class World:
    """Host data shared by every case; never written after it is made."""

    def __init__(self, L):
        rng = np.random.default_rng(7)
        self.cam = L.Camera(20.0, 20.0, 8.0, 6.0, W_, H_, 1000.0)
        self.pose = np.eye(4, dtype=np.float32).reshape(-1)
        self.A = _blocks([[0, 0, 8], [1, 0, 8], [0, 1, 8]], 0)   # 0.64 .. 0.72 m in front of the identity pose (near plane 0.5)
        self.B = _blocks([[0, 0, 8], [1, 1, 8], [2, 0, 8]], 1)
        self.tri = np.ascontiguousarray(helpers.procedural_mc_table(), np.int32)
        self.edges = np.ascontiguousarray(helpers.MC_EDGE_PAIRS, np.int32)
        self.queries = (rng.random((NPTS, 3)) * [0.16, 0.16, 0.08] + [0.0, 0.0, 0.64]).astype(np.float32)
        depth = rng.integers(500, 1500, (H_, W_)).astype(np.uint16)
        depth[rng.random((H_, W_)) < 0.2] = 0
        self.depth = depth
        self.rgb = rng.integers(0, 256, (H_, W_, 3)).astype(np.uint8)
        xy = rng.random((NPTS, 2)).astype(np.float32)
        self.cloud = np.concatenate([xy, 0.1 * np.sin(4 * xy[:, :1]) * np.cos(3 * xy[:, 1:])], 1).astype(np.float32)
        n = rng.normal(size=(NPTS, 3))
        self.normals = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
        self.moved = (self.cloud + rng.normal(scale=0.003, size=(NPTS, 3))).astype(np.float32)
        self.inliers = np.stack([np.arange(NPTS), rng.permutation(NPTS)], 1).astype(np.int32)
        self.pairs = np.concatenate([self.cloud, self.moved], 1).astype(np.float32)
        self.rows = rng.normal(size=(50, 7)).astype(np.float32)
        self.X, self.Y = (rng.random(NPTS) - 0.5).astype(np.float32), (rng.random(NPTS) - 0.5).astype(np.float32)
        self.Z = (0.5 + rng.random(NPTS)).astype(np.float32)


@pytest.fixture(scope="module")
def world(hip):
    return World(hip)


class Case:
    """The device objects of one case and the entry under test.  call() makes the entry's call and returns its code; what the call produced is
    result() (read with the hook off); invalid() is a call the entry refuses with OP_ERR_INVALID; allocs is the number of requests to the buffer
    cache one call() makes once the objects exist and the call has been made before (read off the code)."""

    def __init__(self, L, W):
        self.L, self.lib, self.W = L, L.load(), W
        self.volumes = []
        self.prepare = lambda: None
        self.result = lambda: b""

    def volume(self, blocks=None):
        v = C.c_void_p()
        self.L.check(self.lib.op_volume_create(C.byref(self.W.cam), 0.01, 0.1, 5.0, 0.5, 0, 64, C.byref(v)))
        self.volumes.append(v)
        if blocks is not None:
            self.L.check(self.lib.op_volume_upload(v, _ip(blocks[0]), _fp(blocks[1]), len(blocks[0])))
        return v

    def download(self, v):
        keys, vox, n = np.zeros((8, 3), np.int32), np.zeros((8, 512, 5), np.float32), C.c_size_t(0)
        self.L.check(self.lib.op_volume_download(v, _ip(keys), _fp(vox), 8, C.byref(n)))
        order = np.lexsort(keys[:n.value].T[::-1])
        return keys[:n.value][order].tobytes() + vox[:n.value][order].tobytes()

    def close(self):
        for v in self.volumes:
            self.L.check(self.lib.op_volume_destroy(v))
        self.volumes = []


def e_download(c):
    v = c.volume(c.W.A)
    keys, vox, n = np.zeros((3, 3), np.int32), np.zeros((3, 512, 5), np.float32), C.c_size_t(0)
    c.call = lambda: c.lib.op_volume_download(v, _ip(keys), _fp(vox), 3, C.byref(n))
    c.result = lambda: keys.tobytes() + vox.tobytes() + bytes(n)
    c.invalid = lambda: c.lib.op_volume_download(None, _ip(keys), _fp(vox), 3, C.byref(n))
    c.allocs = 1            # the staging buffer


def e_upload(c):
    v = c.volume(c.W.A)
    keys, vox = c.W.A
    c.call = lambda: c.lib.op_volume_upload(v, _ip(keys), _fp(vox), 3)
    c.result = lambda: c.download(v)
    c.invalid = lambda: c.lib.op_volume_upload(v, None, _fp(vox), 3)
    c.allocs = 3            # keys, slots, voxels of a chunk


def e_merge(c):
    dst, src = c.volume(), c.volume(c.W.B)

    def prepare():          # the same destination every time
        c.L.check(c.lib.op_volume_clear(dst))
        c.L.check(c.lib.op_volume_upload(dst, _ip(c.W.A[0]), _fp(c.W.A[1]), 3))
    c.prepare = prepare
    c.call = lambda: c.lib.op_volume_merge(dst, src)
    c.result = lambda: c.download(dst)
    c.invalid = lambda: c.lib.op_volume_merge(dst, None)
    c.allocs = 1            # the slots of the source's blocks


def e_point_cloud(c, short=0):
    v = c.volume(c.W.A)
    n = C.c_size_t(0)
    c.L.check(c.lib.op_volume_point_cloud(v, None, None, 0, C.byref(n)))
    c.total = n.value
    assert c.total > 0
    xyz, col = np.zeros((c.total, 3), np.float32), np.zeros((c.total, 3), np.float32)
    c.call = lambda: c.lib.op_volume_point_cloud(v, _fp(xyz), _fp(col), c.total - short, C.byref(n))
    c.result = lambda: xyz.tobytes() + col.tobytes() + bytes(n)
    c.invalid = lambda: c.lib.op_volume_point_cloud(v, _fp(xyz), _fp(col), c.total, None)
    c.count = n
    c.allocs = 4            # counts, offsets; points, colours


def e_extract_mesh(c, short=0):
    v = c.volume(c.W.A)
    n = C.c_size_t(0)
    c.L.check(c.lib.op_volume_extract_mesh(v, _ip(c.W.tri), _ip(c.W.edges), None, None, None, 0, C.byref(n)))
    c.total = n.value
    assert c.total > 0
    pts, col = np.zeros((c.total, 3), np.float32), np.zeros((c.total, 3), np.float32)
    c.call = lambda: c.lib.op_volume_extract_mesh(v, _ip(c.W.tri), _ip(c.W.edges), None, _fp(pts), _fp(col), c.total - short, C.byref(n))
    c.result = lambda: pts.tobytes() + col.tobytes() + bytes(n)
    c.invalid = lambda: c.lib.op_volume_extract_mesh(v, None, _ip(c.W.edges), None, _fp(pts), _fp(col), c.total, C.byref(n))
    c.count = n
    c.allocs = 8            # list, counts, offsets, table, edges, neighbours; points, colours


def e_extract_mesh_clustered(c):
    v = c.volume(c.W.A)
    nv, nt = C.c_size_t(0), C.c_size_t(0)
    c.L.check(c.lib.op_volume_extract_mesh_clustered(v, _ip(c.W.tri), _ip(c.W.edges), None, 0.02, None, None, 0, None, 0, C.byref(nv), C.byref(nt)))
    cap_v, cap_t = nv.value, nt.value
    assert cap_t > 0
    pts, col, tri = np.zeros((cap_v, 3), np.float32), np.zeros((cap_v, 3), np.float32), np.zeros((cap_t, 3), np.uint32)
    c.call = lambda: c.lib.op_volume_extract_mesh_clustered(v, _ip(c.W.tri), _ip(c.W.edges), None, 0.02, _vp(pts), _vp(col), cap_v, _vp(tri), cap_t,
                                                             C.byref(nv), C.byref(nt))
    c.result = lambda: pts.tobytes() + col.tobytes() + tri.tobytes() + bytes(nv) + bytes(nt)
    c.invalid = lambda: c.lib.op_volume_extract_mesh_clustered(v, _ip(c.W.tri), _ip(c.W.edges), None, 0.0, _vp(pts), _vp(col), cap_v, _vp(tri), cap_t,
                                                                C.byref(nv), C.byref(nt))
    # the soup's 8; the clustering: bounds, 9 per-corner and per-triangle arrays, the sort's scratch, 5 per-cell arrays, and for host output
    # the vertices, the triangles and the colours
    c.allocs = 8 + 1 + 9 + 1 + 5 + 3


def e_raycast(c):
    v = c.volume(c.W.A)
    depth, nrm, col = np.zeros(NPX, np.float32), np.zeros((NPX, 3), np.float32), np.zeros((NPX, 3), np.float32)
    c.call = lambda: c.lib.op_volume_raycast(v, C.byref(c.W.cam), _fp(c.W.pose), _fp(depth), _fp(nrm), _fp(col), c.L.OP_MEM_HOST)
    c.result = lambda: depth.tobytes() + nrm.tobytes() + col.tobytes()
    c.invalid = lambda: c.lib.op_volume_raycast(v, C.byref(c.W.cam), None, _fp(depth), _fp(nrm), _fp(col), c.L.OP_MEM_HOST)
    c.allocs = 3            # the three device images (the view's block list and counters are the volume's)


def e_render_frame(c):
    v = c.volume(c.W.A)
    rgb, depth, n = np.zeros((NPX, 3), np.uint8), np.zeros(NPX, np.float32), C.c_uint64(0)
    c.call = lambda: c.lib.op_volume_render_frame(v, C.byref(c.W.cam), _fp(c.W.pose), _vp(rgb), _fp(depth), c.L.OP_MEM_HOST, C.byref(n))
    c.result = lambda: rgb.tobytes() + depth.tobytes() + bytes(n)
    c.invalid = lambda: c.lib.op_volume_render_frame(v, C.byref(c.W.cam), None, _vp(rgb), _fp(depth), c.L.OP_MEM_HOST, C.byref(n))
    c.allocs = 2            # the two device images


def e_sample(c):
    v = c.volume(c.W.A)
    L = c.L
    vox, grad, status, stats = np.zeros((NPTS, 5), np.float32), np.zeros((NPTS, 3), np.float32), np.zeros(NPTS, np.uint8), L.SampleStats()
    c.call = lambda: c.lib.op_volume_sample(v, _vp(c.W.queries), NPTS, L.OP_MEM_HOST, None, L.OP_SAMPLE_TRILINEAR, _vp(vox), _vp(grad), _vp(status), C.byref(stats))
    c.result = lambda: vox.tobytes() + grad.tobytes() + status.tobytes() + repr([getattr(stats, f) for f, _ in stats._fields_]).encode()
    c.invalid = lambda: c.lib.op_volume_sample(v, _vp(c.W.queries), NPTS, L.OP_MEM_HOST, None, 7, _vp(vox), _vp(grad), _vp(status), C.byref(stats))
    c.allocs = 6            # queries; voxels, gradients, status; the partial rows and their pinned copy


def e_has_cube(c):
    v = c.volume(c.W.A)
    present = C.c_int(-1)
    c.call = lambda: c.lib.op_volume_has_cube(v, 1, 0, 8, C.byref(present))
    c.result = lambda: bytes(present)
    c.invalid = lambda: c.lib.op_volume_has_cube(v, 1, 0, 8, None)
    c.allocs = 1


def e_points_from_depth(c):
    L = c.L
    xyz, n = np.zeros((NPX, 3), np.float32), C.c_size_t(0)
    c.call = lambda: c.lib.op_points_from_depth(C.byref(c.W.cam), _vp(c.W.depth), L.OP_DEPTH_U16, L.OP_MEM_HOST, 0, _vp(xyz), C.byref(n))
    c.result = lambda: xyz.tobytes() + bytes(n)
    c.invalid = lambda: c.lib.op_points_from_depth(None, _vp(c.W.depth), L.OP_DEPTH_U16, L.OP_MEM_HOST, 0, _vp(xyz), C.byref(n))
    c.allocs = 5            # depth, counts, starts, points; the scan's block totals


def e_points_from_rgbd(c):
    L = c.L
    xyz, col, n = np.zeros((NPX, 3), np.float32), np.zeros((NPX, 3), np.float32), C.c_size_t(0)
    c.call = lambda: c.lib.op_points_from_rgbd(C.byref(c.W.cam), _vp(c.W.depth), L.OP_DEPTH_U16, _vp(c.W.rgb), L.OP_MEM_HOST, 0, _vp(xyz), _vp(col), C.byref(n))
    c.result = lambda: xyz.tobytes() + col.tobytes() + bytes(n)
    c.invalid = lambda: c.lib.op_points_from_rgbd(C.byref(c.W.cam), _vp(c.W.depth), L.OP_DEPTH_U16, None, L.OP_MEM_HOST, 0, _vp(xyz), _vp(col), C.byref(n))
    c.allocs = 7            # as from depth alone, and the colours and the colour image


# what op_icp_create takes for a target without normals: the points twice (as given, sorted into cells), the bounding box (per call), the cell
# table, the per-cell counts (per call) and the scan's block totals (per call), the grid barrier, the result, the pose, the stage and its pinned copy
ICP_CREATE_ALLOCS = 11


def e_estimate_normals(c):
    out = np.zeros((NPTS, 3), np.float32)
    c.call = lambda: c.lib.op_estimate_normals(_vp(c.W.cloud), NPTS, 0.1, 10, c.L.OP_MEM_HOST, 0, _vp(out))
    c.result = lambda: out.tobytes()
    c.invalid = lambda: c.lib.op_estimate_normals(_vp(c.W.cloud), NPTS, 0.1, 0, c.L.OP_MEM_HOST, 0, _vp(out))
    c.allocs = ICP_CREATE_ALLOCS + 1   # a search grid over the cloud, and the normals


def e_icp_create(c):
    def call():
        h = C.c_void_p()
        rc = c.lib.op_icp_create(_vp(c.W.cloud), _vp(c.W.normals), NPTS, 0.05, c.L.OP_MEM_HOST, 0, C.byref(h))
        assert (rc == 0) == bool(h.value)
        if h.value:
            c.L.check(c.lib.op_icp_destroy(h))
        return rc
    c.call = call
    c.invalid = lambda: c.lib.op_icp_create(_vp(c.W.cloud), _vp(c.W.normals), NPTS, 0.0, c.L.OP_MEM_HOST, 0, C.byref(C.c_void_p()))
    c.allocs = ICP_CREATE_ALLOCS + 1   # and the target's normals


def e_rigid_point_to_plane(c):
    W, T = c.W, np.zeros(16, np.float32)
    c.call = lambda: c.lib.op_estimate_rigid_point_to_plane(_vp(W.moved), NPTS, _vp(W.cloud), _vp(W.normals), NPTS, _vp(W.inliers), NPTS, c.L.OP_MEM_HOST, 0, _fp(T))
    c.result = lambda: T.tobytes()
    c.invalid = lambda: c.lib.op_estimate_rigid_point_to_plane(_vp(W.moved), NPTS, _vp(W.cloud), _vp(W.normals), NPTS, _vp(W.inliers), NPTS, c.L.OP_MEM_HOST, 0, None)
    c.allocs = 6            # source, target, normals, pairs; partial sums, sums


def e_rigid_transformation(c):
    W, T = c.W, np.zeros(16, np.float32)
    c.call = lambda: c.lib.op_estimate_rigid_transformation_ex(_vp(W.pairs), NPTS, c.L.OP_MEM_HOST, 0, c.L.OP_ICP_FINISH_FP64, _fp(T))
    c.result = lambda: T.tobytes()
    c.invalid = lambda: c.lib.op_estimate_rigid_transformation_ex(_vp(W.pairs), NPTS, c.L.OP_MEM_HOST, 0, c.L.OP_ICP_FINISH_FP64, None)
    c.allocs = 3            # pairs; partial sums, sums


def e_bilateral_filter(c):
    L, out = c.L, np.zeros(NPX, np.float32)
    c.call = lambda: c.lib.op_bilateral_filter_depth(_vp(c.W.depth), L.OP_DEPTH_U16, 1000.0, W_, H_, 1, 5, 0.05, 2.0, L.OP_MEM_HOST, 0, None, _fp(out))
    c.result = lambda: out.tobytes()
    c.invalid = lambda: c.lib.op_bilateral_filter_depth(_vp(c.W.depth), 9, 1000.0, W_, H_, 1, 5, 0.05, 2.0, L.OP_MEM_HOST, 0, None, _fp(out))
    c.allocs = 2            # the image and the filtered image


def e_debug_seq_sums(c):
    out = np.zeros(64, np.float32)
    c.call = lambda: c.lib.op_debug_seq_sums(0, _vp(c.W.rows), 50, 50, _vp(out))
    c.result = lambda: out.tobytes()
    c.invalid = lambda: c.lib.op_debug_seq_sums(9, _vp(c.W.rows), 50, 50, _vp(out))
    c.allocs = 1            # the rows (the sums' own buffers do not come from the cache here)


def e_debug_project_uv(c):
    W, out = c.W, np.zeros((NPTS, 4), np.int32)
    c.call = lambda: c.lib.op_debug_project_uv(517.3, 516.5, 318.6, 255.3, _vp(W.X), _vp(W.Y), _vp(W.Z), NPTS, 0, _vp(out))
    c.result = lambda: out.tobytes()
    c.invalid = lambda: c.lib.op_debug_project_uv(517.3, 516.5, 318.6, 255.3, None, _vp(W.Y), _vp(W.Z), NPTS, 0, _vp(out))
    c.allocs = 2            # the coordinates, the pixels


ENTRIES = {f.__name__[2:]: f for f in (
    e_download, e_upload, e_merge, e_point_cloud, e_extract_mesh, e_extract_mesh_clustered, e_raycast, e_render_frame, e_sample, e_has_cube,
    e_points_from_depth, e_points_from_rgbd, e_estimate_normals, e_icp_create, e_rigid_point_to_plane, e_rigid_transformation, e_bilateral_filter,
    e_debug_seq_sums, e_debug_project_uv)}


def _live(lib):
    dev, pinned = C.c_uint64(0), C.c_uint64(0)
    assert lib.op_debug_cache_live(0, C.byref(dev), C.byref(pinned)) == 0
    return dev.value, pinned.value


class _Checked:
    """with _Checked(hip, world, make) as c: the case's objects exist inside; afterwards they are destroyed and the live set is what it was."""

    def __init__(self, L, W, make, **kw):
        self.L, self.W, self.make, self.kw = L, W, make, kw

    def __enter__(self):
        gc.collect()        # objects other tests left to the collector are destroyed now, not half way through the case
        self.base = _live(self.L.load())
        self.case = Case(self.L, self.W)
        try:
            self.make(self.case, **self.kw)
        except BaseException:
            self.case.close()
            raise
        return self.case

    def __exit__(self, exc_type, exc, tb):
        lib = self.L.load()
        lib.op_runtime_set_option(self.L.OP_RUNTIME_OPT_ALLOC_FAULT, 0)
        self.case.close()
        if exc_type is None:
            after = _live(lib)
            print("live buffers (device, pinned): before %s, after %s" % (self.base, after))
            assert after == self.base
        return False


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_clean_exit_returns_every_buffer(hip, world, name):
    with _Checked(hip, world, ENTRIES[name]) as c:
        c.prepare()
        assert c.call() == hip.OP_OK, hip.load().op_last_error()
        c.result()


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_refused_call_returns_every_buffer(hip, world, name):
    with _Checked(hip, world, ENTRIES[name]) as c:
        c.prepare()
        assert c.invalid() == hip.OP_ERR_INVALID


@pytest.mark.parametrize("make", [e_point_cloud, e_extract_mesh], ids=["point_cloud", "extract_mesh"])
def test_capacity_refusal_returns_every_buffer(hip, world, make):
    with _Checked(hip, world, make, short=1) as c:
        c.count.value = 0
        assert c.call() == hip.OP_ERR_CAPACITY
        assert c.count.value == c.total          # the count says what is needed


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_injected_allocation_failure_returns_every_buffer(hip, world, name):
    lib = hip.load()
    fault = C.c_longlong(-1)
    with _Checked(hip, world, ENTRIES[name]) as c:
        c.prepare()
        assert c.call() == hip.OP_OK, lib.op_last_error()
        before = c.result()
        first_ok = None
        for k in range(1, SWEEP_CAP + 1):
            c.prepare()
            assert lib.op_runtime_set_option(hip.OP_RUNTIME_OPT_ALLOC_FAULT, k) == 0
            rc = c.call()
            assert lib.op_runtime_get_option(hip.OP_RUNTIME_OPT_ALLOC_FAULT, C.byref(fault)) == 0
            assert lib.op_runtime_set_option(hip.OP_RUNTIME_OPT_ALLOC_FAULT, 0) == 0
            if rc == hip.OP_OK:
                first_ok = k
                break
            assert rc == hip.OP_ERR_HIP, (k, rc, lib.op_last_error())
            assert fault.value == 0, (k, fault.value)   # it fired inside the call
        print("%s: the call succeeds from k = %s on; %d allocations read off the code" % (name, first_ok, c.allocs))
        assert first_ok is not None, "still failing at k = %d" % SWEEP_CAP
        assert first_ok >= 2, "k = 1 did not fail: the call allocated nothing"
        assert first_ok == c.allocs + 1
        c.prepare()
        assert c.call() == hip.OP_OK, lib.op_last_error()
        assert c.result() == before
