"""What tests/test_mesh_post_cpu.py and tests/test_mesh_post_gpu.py share: the numpy restatements of geometry::TriangleMesh::ComputeNormals and
Prune (host/one_piece/src/TriangleMesh.cpp: the loops + Compact), the meshes both files plant, and the driver."""
import json
import os
import subprocess

import numpy as np

from mesh_cluster_common import ROOT, bits, check, grid_mesh, random_soup, read_mesh, same_bits, soup_triangles  # noqa: F401  (re-exported)

DRIVER = os.path.join(ROOT, "examples", "cpp", "MeshPostprocess.bin")
f32, u32 = np.float32, np.uint32


def _normalize(v):
    """TriangleMesh.cpp Normalize on rows: n = sqrt((v0 v0 + v1 v1) + v2 v2) in float32; rows with n > 0 are divided by it."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        n = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        assert n.dtype == f32
        out = v.copy()
        pos = n > 0
        out[pos] = v[pos] / n[pos, None]
    return out


def face_normals(points, triangles):
    """Per triangle, float32: (p1 - p0) x (p2 - p0) with every product rounded before the subtraction (numpy evaluates one ufunc at a time: no FMA),
    then Normalize."""
    pts = np.ascontiguousarray(points, f32).reshape(-1, 3)
    tri = np.ascontiguousarray(triangles).reshape(-1, 3).astype(np.int64)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        a, b = pts[tri[:, 1]] - pts[tri[:, 0]], pts[tri[:, 2]] - pts[tri[:, 0]]
        n = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)
    assert n.dtype == f32
    return _normalize(n.reshape(-1, 3))


def vertex_sums(face, triangles, nv, order=None):
    """normals[v] = +0, then += the face normal once per corner that refers to v, in corner order (or in `order`, a permutation of the corners):
    float32 numpy scalars, a Python loop over the corners."""
    corners = np.ascontiguousarray(triangles).reshape(-1).astype(np.int64).tolist()
    rows = [[f32(0), f32(0), f32(0)] for _ in range(nv)]
    comp = [[f32(x) for x in r] for r in face.tolist()]
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for c in (range(len(corners)) if order is None else order):
            acc, n = rows[corners[c]], comp[c // 3]
            acc[0] = acc[0] + n[0]; acc[1] = acc[1] + n[1]; acc[2] = acc[2] + n[2]
    return np.asarray(rows, f32).reshape(-1, 3)


def normals_ref(points, triangles):
    """TriangleMesh::ComputeNormals -> normals [nv,3] float32"""
    nv = len(np.asarray(points).reshape(-1, 3))
    return _normalize(vertex_sums(face_normals(points, triangles), triangles, nv))


def prune_ref(points, colors, normals, triangles, min_points):
    """TriangleMesh::Prune: a plain union-find over the vertices, component size = referenced vertices, a triangle is kept when its component's size is
    > min_points; Compact numbers the vertices by first appearance among the kept corners -> (points, colors or None, normals or None, triangles, pruned)."""
    pts = np.ascontiguousarray(points, f32).reshape(-1, 3)
    tri = np.ascontiguousarray(triangles).reshape(-1, 3).astype(np.int64)
    parent = list(range(len(pts)))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    rows = tri.tolist()
    for r in rows:
        a = find(r[0])
        for k in (1, 2):
            b = find(r[k])
            if a != b:
                parent[b] = a
    referenced = np.zeros(len(pts), bool)
    referenced[tri.reshape(-1)] = True
    root = np.asarray([find(v) for v in range(len(pts))], np.int64)
    size = np.bincount(root[referenced], minlength=len(pts)) if len(pts) else np.zeros(0, np.int64)
    keep = size[root[tri[:, 0]]] > min_points if len(tri) else np.zeros(0, bool)
    pruned = int((referenced & (size[root] <= min_points)).sum()) if len(pts) else 0
    new_of, order, out_tri = {}, [], []
    for r in tri[keep].tolist():
        out = []
        for v in r:
            o = new_of.get(v)
            if o is None:
                o = new_of[v] = len(order)
                order.append(v)
            out.append(o)
        out_tri.append(out)
    order = np.asarray(order, np.int64)
    carry = lambda a: None if a is None else np.ascontiguousarray(a, f32).reshape(-1, 3)[order].reshape(-1, 3)
    return pts[order].reshape(-1, 3), carry(colors), carry(normals), np.asarray(out_tri, u32).reshape(-1, 3), pruned


# ---- planted meshes: each -> (points, colors, normals, triangles) ------------------------------------------------------------------------------

def _attributes(pts, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 1, size=pts.shape).astype(f32), rng.normal(size=pts.shape).astype(f32)


def indexed_mesh(nt, seed):
    """nt triangles with random corners among 3 nt + 5 vertices: one large component, many small ones, vertices nothing refers to, now and then a
    triangle that uses a vertex twice"""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-1, 1, size=(3 * nt + 5, 3)).astype(f32)
    tri = rng.integers(0, 3 * nt + 5, size=(nt, 3)).astype(u32)
    return (pts,) + _attributes(pts, seed + 1) + (tri,)


def fan(n=2000, seed=23):
    """n triangles around vertex `centre`, rim heights random so that every face normal tilts another way, triangle order shuffled: the centre's normal
    is a chain of n float32 adds whose result depends on the order"""
    rng = np.random.default_rng(seed)
    th = np.linspace(0, 2 * np.pi, n + 1)
    rim = np.stack([np.cos(th), np.sin(th), rng.uniform(-0.4, 0.4, n + 1)], axis=1)
    pts = np.concatenate([[[0.013, -0.007, 0.31]], rim])
    place = rng.permutation(len(pts))
    shuffled = np.empty_like(pts)
    shuffled[place] = pts
    tri = np.stack([np.full(n, place[0]), place[1:n + 1], place[2:n + 2]], axis=1)[rng.permutation(n)]
    shuffled = shuffled.astype(f32)
    return (shuffled,) + _attributes(shuffled, seed) + (tri.astype(u32),)


def fan_centre(tri):
    return int(np.bincount(tri.reshape(-1)).argmax())


def repeated_and_degenerate():
    """triangle 0 uses vertex 1 twice (zero area as well), triangle 1 has three collinear vertices, triangle 2 is a point three times, 3 and 4 are honest
    and share vertices with the others; vertex 6 is a component of its own, vertex 7 is unreferenced"""
    pts = np.array([[0, 0, 0], [1, 0.5, 0.25], [2, 1, 0.5], [0, 1, 0], [1, 1, 1], [0.5, 0.25, 2], [3, 3, 3], [9, 9, 9]], f32)
    tri = np.array([[0, 1, 1], [0, 1, 2], [6, 6, 6], [0, 3, 4], [1, 4, 5], [5, 5, 4]], u32)
    return (pts,) + _attributes(pts, 4) + (tri,)


def negative_zero_mesh(indexed, n=40, seed=31):
    """Triangles p0, p0 + (s, 0, 0), p0 + (0, s, -s): a = (s, 0, 0), b = (0, s, -s) gives n0 = 0 * -s - 0 * s = (-0) - (+0) = -0, so every face normal is
    (-0, 1, 1) / sqrt 2; others mirrored for a -0 on y.  Indexed: every triangle occurs twice."""
    rng = np.random.default_rng(seed)
    pts, tri = [], []
    for i in range(n):
        p0, s = rng.uniform(-1, 1, 3).astype(f32), f32(2.0 ** rng.integers(-3, 3))
        e1, e2 = (f32([s, 0, 0]), f32([0, s, -s])) if i % 2 == 0 else (f32([0, s, 0]), f32([-s, 0, s]))
        base = len(pts)
        pts += [p0, p0 + e1, p0 + e2]
        tri.append([base, base + 1, base + 2])
    pts, tri = np.asarray(pts, f32), np.asarray(tri, u32)
    if indexed:  # every triangle twice: shared vertices, chains of two, the same signs
        tri = np.concatenate([tri, tri])[rng.permutation(2 * n)]
    return (pts,) + _attributes(pts, seed) + (tri,)


def scaled_soup(nt, lo, hi, seed):
    """a random soup whose edges run from 10^lo to 10^hi"""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(lo, hi, size=(nt, 1, 1))
    pts = (rng.uniform(-1, 1, size=(nt, 3, 3)) * scale).reshape(-1, 3).astype(f32)
    return (pts,) + _attributes(pts, seed) + (soup_triangles(nt),)


def strip(n=5000, shuffled=False, seed=41):
    """n triangles (i, i + 1, i + 2) with the ids DEcreasing along the strip, so that in triangle order every union hooks the old root under a new,
    smaller one; shuffled: the ids permuted"""
    rng = np.random.default_rng(seed)
    nv = n + 2
    ids = np.arange(nv)[::-1].copy()
    if shuffled:
        ids = rng.permutation(nv)
    pts = rng.uniform(-1, 1, size=(nv, 3)).astype(f32)
    tri = np.stack([ids[:-2], ids[1:-1], ids[2:]], axis=1).astype(u32)
    return (pts,) + _attributes(pts, seed) + (tri,)


def islands(count=300, extra=50, seed=47):
    """island i = 1 .. count is a strip of i triangles over i + 2 vertices of its own; ids and triangle order shuffled, `extra` unreferenced vertices.
    -> (mesh, vertex count of every island)"""
    rng = np.random.default_rng(seed)
    tri, base = [], 0
    for i in range(1, count + 1):
        tri += [[base + j, base + j + 1, base + j + 2] for j in range(i)]
        base += i + 2
    nv = base + extra
    ids = rng.permutation(nv)
    tri = ids[np.asarray(tri)][rng.permutation(len(tri))].astype(u32)
    pts = rng.uniform(-1, 1, size=(nv, 3)).astype(f32)
    return (pts,) + _attributes(pts, seed) + (tri,), [i + 2 for i in range(1, count + 1)]


def small_cases():
    """the smallest meshes of the prune list -> {name: mesh}"""
    pts = np.random.default_rng(3).uniform(-1, 1, size=(8, 3)).astype(f32)
    at = _attributes(pts, 3)
    mk = lambda rows: (pts,) + at + (np.asarray(rows, u32).reshape(-1, 3),)
    return {"one": mk([[4, 2, 6]]), "share_vertex": mk([[0, 1, 2], [2, 3, 4]]), "share_edge": mk([[5, 1, 2], [2, 1, 7]]), "disjoint": mk([[7, 6, 5], [0, 1, 2]]),
            "vvw": mk([[3, 3, 5], [0, 1, 2]])}


def with_nan(mesh, referenced=True):
    """a copy of the mesh with a NaN planted at a referenced (or an unreferenced) vertex"""
    pts, col, nrm, tri = mesh
    used = np.zeros(len(pts), bool)
    used[tri.reshape(-1)] = True
    v = int(np.flatnonzero(used if referenced else ~used)[len(pts) // 7 % max(1, int((used if referenced else ~used).sum()))])
    bad = pts.copy()
    bad[v, 1] = np.nan
    return bad, col, nrm, tri


# what the CPU file pins to the host loop and the GPU file runs through the class surface: name -> (mesh, min_points)
PLANTED = {
    "soup_86": lambda: (random_soup(86, 86), 0),
    "indexed_1366": lambda: (indexed_mesh(1366, 1366), 4),
    "grid": lambda: (grid_mesh(), 10),
    "fan": lambda: (fan(), 100),
    "degenerate": lambda: (repeated_and_degenerate(), 2),
    "negative_zero_indexed": lambda: (negative_zero_mesh(True), 0),
    "negative_zero_soup": lambda: (negative_zero_mesh(False), 0),
    "tiny_edges": lambda: (scaled_soup(200, -23, -19, 61), 0),
    "huge_edges": lambda: (scaled_soup(200, 18, 18, 62), 0),
    "large_edges": lambda: (scaled_soup(200, 9, 9, 63), 0),
    "strip_decreasing": lambda: (strip(500), 100),
    "strip_shuffled": lambda: (strip(500, True), 502),
    "islands": lambda: (islands(60)[0], 32),
}


def run_driver(args, timeout=600):
    r = subprocess.run([DRIVER] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, "MeshPostprocess.bin %s failed (%d):\n%s\n%s" % (" ".join(map(str, args)), r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def post_through_driver(tmp, path, op, points, colors, normals, triangles, min_points):
    """One mesh through geometry::TriangleMesh::Prune and / or ComputeNormals of the class surface (MeshPostprocess.bin --mesh) -> (result.json, mesh)."""
    tmp = str(tmp)
    np.ascontiguousarray(points, f32).tofile(os.path.join(tmp, "in_points.f32"))
    np.ascontiguousarray(triangles, u32).tofile(os.path.join(tmp, "in_triangles.u32"))
    args = ["--mesh", os.path.join(tmp, "in_points.f32"), "--triangles", os.path.join(tmp, "in_triangles.u32"), "--op", op, "--min-points", int(min_points), "--path", path,
            "--dump", tmp]
    for name, a in (("colors", colors), ("normals", normals)):
        if a is not None:
            np.ascontiguousarray(a, f32).tofile(os.path.join(tmp, "in_%s.f32" % name))
            args += ["--" + name, os.path.join(tmp, "in_%s.f32" % name)]
    return run_driver(args), read_mesh(tmp)


def both_ref(points, colors, normals, triangles, min_points):
    """Prune, then ComputeNormals: what --op both runs -> (points, colors, normals, triangles, pruned)"""
    p, c, _, t, pruned = prune_ref(points, colors, normals, triangles, min_points)
    return p, c, normals_ref(p, t), t, pruned
