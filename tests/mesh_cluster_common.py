"""What tests/test_mesh_cluster_cpu.py and tests/test_mesh_cluster_gpu.py share: the numpy restatement of geometry::TriangleMesh::ClusteringSimplify
(host/one_piece/src/TriangleMesh.cpp: the loop + Compact) in plain Python over the corners, the meshes both files plant, and the driver."""
import json
import os
import subprocess

import numpy as np

from downsample_common import ROOT, bits, cells_of, same_bits  # noqa: F401  (re-exported)

DRIVER = os.path.join(ROOT, "examples", "cpp", "MeshSimplify.bin")
f32, f64, u32 = np.float32, np.float64, np.uint32


def cluster_ref(points, colors, normals, triangles, grid_len):
    """Corner c = 3 t + k is vertex v = triangles[t, k].  Cells in order of first appearance over the corners; a cell's representative is the vertex
    of its first corner; its position np.float32(sum / np.float64(count)) with a float64 accumulator per cell and axis, added to in corner order;
    a triangle whose three cells are not distinct is dropped; new indices by first appearance among the kept corners; colours and normals are the
    representative's.  -> (points, colors or None, normals or None, triangles uint32 [k,3])."""
    pts = np.ascontiguousarray(points, f32).reshape(-1, 3)
    tri = np.ascontiguousarray(triangles).reshape(-1, 3).astype(np.int64)
    cell_rows = [tuple(r) for r in cells_of(pts, grid_len).tolist()]
    as_double = pts.astype(f64).tolist()  # (python floats are IEEE doubles: += below is one double add)
    slot_of, rep, count, sx, sy, sz = {}, [], [], [], [], []
    corner_cell = []
    for v in tri.reshape(-1).tolist():
        j = slot_of.get(cell_rows[v])
        if j is None:
            j = slot_of[cell_rows[v]] = len(rep)
            rep.append(v); count.append(0); sx.append(0.0); sy.append(0.0); sz.append(0.0)
        p = as_double[v]
        sx[j] += p[0]; sy[j] += p[1]; sz[j] += p[2]
        count[j] += 1
        corner_cell.append(j)
    with np.errstate(over="ignore"):
        mean = (np.stack([np.asarray(a, f64) for a in (sx, sy, sz)], axis=1).reshape(-1, 3) / np.asarray(count, f64).reshape(-1, 1)).astype(f32)
    corner_cell = np.asarray(corner_cell, np.int64).reshape(-1, 3)
    a, b, c = corner_cell[:, 0], corner_cell[:, 1], corner_cell[:, 2]
    keep = (a != b) & (a != c) & (b != c)
    new_of, order, out_tri = {}, [], []
    for row in corner_cell[keep].tolist():
        out = []
        for j in row:
            o = new_of.get(j)
            if o is None:
                o = new_of[j] = len(order)
                order.append(j)
            out.append(o)
        out_tri.append(out)
    order = np.asarray(order, np.int64)
    reps = np.asarray(rep, np.int64)[order] if len(order) else np.zeros(0, np.int64)
    carry = lambda a: None if a is None else np.ascontiguousarray(a, f32).reshape(-1, 3)[reps].reshape(-1, 3)
    return mean[order].reshape(-1, 3), carry(colors), carry(normals), np.asarray(out_tri, u32).reshape(-1, 3)


def check(got, want):
    """bitwise on points, colours and normals, exact on the triangles; no tolerance"""
    for name, a, b in zip(("points", "colors", "normals"), got[:3], want[:3]):
        if b is None or len(b) == 0:  # (an empty mesh has no attributes to carry)
            assert a is None or len(a) == 0, name
        else:
            assert a is not None and a.shape == b.shape, "%s: %s rows, expected %s" % (name, None if a is None else a.shape, b.shape)
            assert np.array_equal(bits(a), bits(b)), "%s differ in %d of %d words" % (name, int((bits(a) != bits(b)).sum()), b.size)
    assert got[3].dtype == u32 and got[3].shape == want[3].shape, "triangles: %s, expected %s" % (got[3].shape, want[3].shape)
    assert np.array_equal(got[3], want[3]), "triangles differ in %d of %d rows" % (int((got[3] != want[3]).any(axis=1).sum()), len(want[3]))


def soup_triangles(nt):
    return np.arange(3 * nt, dtype=u32).reshape(-1, 3)


def random_soup(nt, seed, grid_len=0.05):
    """nt unshared triangles with edges of about one cell in a box of about nt cells: some collapse, some survive, cells are shared between triangles.
    -> (points, colors, normals, triangles)"""
    rng = np.random.default_rng(seed)
    side = grid_len * max(2.0, round(nt ** (1.0 / 3.0)))
    centre = rng.uniform(-side / 2, side / 2, size=(nt, 1, 3))
    pts = (centre + rng.uniform(-0.7 * grid_len, 0.7 * grid_len, size=(nt, 3, 3))).reshape(-1, 3).astype(f32)
    col = rng.uniform(0.0, 1.0, size=pts.shape).astype(f32)
    nrm = rng.normal(size=pts.shape)
    nrm = (nrm / np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-9)).astype(f32)
    return pts, col, nrm, soup_triangles(nt)


def grid_mesh(side=40, edge=0.01, extra=100, seed=17):
    """side x side quads of a wavy sheet, two triangles each, vertices shared, triangle order shuffled; `extra` vertices nothing refers to are mixed in."""
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(side + 1), np.arange(side + 1), indexing="ij")
    sheet = np.stack([u * edge + 0.003, v * edge + 0.002, 0.03 * np.sin(u / 5.0) + 0.02 * np.cos(v / 4.0) + 0.004], axis=-1).reshape(-1, 3)
    pts = np.concatenate([sheet, rng.uniform(-1, 1, size=(extra, 3))])
    place = rng.permutation(len(pts))  # vertex i of the sheet sits in row place[i]
    shuffled = np.empty_like(pts)
    shuffled[place] = pts
    idx = lambda i, j: place[i * (side + 1) + j]
    tri = []
    for i in range(side):
        for j in range(side):
            tri += [[idx(i, j), idx(i + 1, j), idx(i, j + 1)], [idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)]]
    tri = np.asarray(tri, u32)[rng.permutation(2 * side * side)]
    col = rng.uniform(0, 1, size=shuffled.shape).astype(f32)
    nrm = rng.normal(size=shuffled.shape).astype(f32)
    return shuffled.astype(f32), col, nrm, tri


def too_wide_mesh(grid_len=0.05, seed=3):
    """A soup 3 * 10^6 cells wide on x: more than the packed key of the device entry holds, nothing the host loop minds."""
    pts, col, nrm, tri = random_soup(160, seed, grid_len)
    pts = pts.copy()
    pts[::21, 0] += f32(3.0e6 * grid_len)
    return pts, col, nrm, tri


def one_cell_soup(nt, seed=9):
    """every corner in the cell [1024, 2048)^3 of grid_len 1024, spread over a binade"""
    rng = np.random.default_rng(seed + nt)
    pts = rng.uniform(1024.0, 2047.0, size=(3 * nt, 3)).astype(f32)
    return pts, rng.uniform(0, 1, size=pts.shape).astype(f32), None, soup_triangles(nt)


def tie_chain(n, m=0x9A3C70, lead=64):
    """n positive float32 values whose exact mean, summed as the definition sums them, is the midpoint T = (m + 1/2) * 2^10 of two neighbouring
    float32 (m even: the tie rounds DOWN to m * 2^10).  x[0] = a; x[1 .. lead] = b, each below half a float32 ulp of a, with a + lead * b = T * n
    exactly; the rest is a quarter of a double ulp of that sum.  In double the in-order chain keeps every b and loses every small member: its mean
    is T, float32 m * 2^10.  Any sum that lets the small members meet first (pairwise, a tree, atomics in another order) keeps some of them: its
    mean is above T, float32 (m + 1) * 2^10.  A float32 chain loses the b as well and lands ulps away."""
    assert m % 2 == 0 and n % 2 == 0 and n > lead + 1
    total = (2 * m + 1) * (n // 2) * 2 ** 10          # T * n, an integer
    A = (total >> 24) - 3
    rest = total - (A << 24)
    assert rest % lead == 0
    a, b = f32(A * 2.0 ** 24), f32(rest // lead)
    assert int(a) == A << 24 and int(b) * lead == rest
    x = np.full(n, f32(np.spacing(f64(total)) / 4), f32)
    x[0] = a
    x[1:1 + lead] = b
    return x


def three_chain_mesh(nt=23334):
    """Three cells of grid_len 1e18, every triangle one corner in each (all kept), so each cell is a chain of nt corners interleaved with the others.
    On x every chain is tie_chain(nt) (cells A and B; cell C holds the negatives: a negative coordinate cannot share a cell with a positive one),
    so the float32 mean of a cell tells the in-order double chain from every other way of summing."""
    g = f32(1e18)
    x = tie_chain(nt)
    y = lambda cell: np.full(nt, (cell + 0.5) * 1e18, f32)
    z = np.full(nt, 0.25e18, f32)
    A = np.stack([x, y(0), z], axis=1)
    B = np.stack([x, y(1), z], axis=1)
    C = np.stack([-x, y(0), z], axis=1)
    pts = np.stack([A, B, C], axis=1).reshape(-1, 3).astype(f32)
    col = np.random.default_rng(5).uniform(0, 1, size=pts.shape).astype(f32)
    return pts, col, None, soup_triangles(nt), g


def reciprocal_mismatches(g, want=100):
    """float32 values p with floorf(p / g) != floorf(p * (1.0f / g)): multiples of g and the floats around them"""
    g = f32(g)
    base = np.arange(-60000, 60000, dtype=f32) * g
    cand = [base]
    for _ in range(2):
        cand += [np.nextafter(cand[-1], f32(np.inf))]
    cand += [np.nextafter(base, f32(-np.inf))]
    p = np.unique(np.concatenate(cand))
    bad = p[np.floor(p / g) != np.floor(p * (f32(1.0) / g))]
    return bad


def boundary_soup(g, planted):
    """Per planted value p (and its float neighbours, and k * g with one float below): a triangle (p, y, z), (p + 3 g, y, z), (p, y + 3 g, z) and
    the same with x and z exchanged -- three distinct cells, so every triangle is kept and every planted value decides a cell; each twice."""
    rng = np.random.default_rng(51)
    g = f32(g)
    x = np.concatenate([planted, np.nextafter(planted, f32(-np.inf)), np.nextafter(planted, f32(np.inf))])
    k = np.arange(-50, 50, dtype=f32) * g
    x = np.concatenate([x, k, np.nextafter(k, f32(-np.inf)), np.nextafter(k, f32(np.inf))]).astype(f32)
    x = np.concatenate([x, x])
    x = x[rng.permutation(len(x))]
    y0 = rng.uniform(-2.4, -2.1, len(x)).astype(f32) * g   # one negative cell
    z0 = np.full(len(x), 0.3, f32) * g
    step = f32(3.0) * g
    first = np.stack([np.stack([x, y0, z0], 1), np.stack([x + step, y0, z0], 1), np.stack([x, y0 + step, z0], 1)], axis=1)
    second = first[:, :, ::-1]
    pts = np.ascontiguousarray(np.concatenate([first, second]).reshape(-1, 3), f32)
    col = rng.uniform(0, 1, size=pts.shape).astype(f32)
    return pts, col, None, soup_triangles(len(pts) // 3)


def representative_in_a_dropped_triangle(g=1.0):
    """Cell P = (0,0,0) is first entered by triangle 0, which collapses (two corners in P); triangle 1 passes through P and survives.  Cell Q = (5,0,0)
    is seen only by triangle 0 and vanishes; triangle 2 lies elsewhere and keeps its numbering.  Indexed, with a shared vertex."""
    pts = np.array([[0.10, 0.20, 0.30],   # 0  P  first corner of all: P's representative, in the dropped triangle
                    [0.70, 0.60, 0.50],   # 1  P
                    [5.50, 0.50, 0.50],   # 2  Q  only in the dropped triangle
                    [0.40, 0.90, 0.80],   # 3  P  the surviving triangle's corner in P
                    [1.50, 0.50, 0.50],   # 4  cell (1,0,0)
                    [0.50, 1.50, 0.50],   # 5  cell (0,1,0)
                    [9.25, 9.50, 9.75],   # 6  a vertex nothing refers to
                    [3.50, 3.50, 0.50],   # 7
                    [4.50, 3.50, 0.50],   # 8
                    [3.50, 4.50, 0.50]],  # 9
                   f32) * f32(g)
    tri = np.array([[0, 1, 2], [4, 3, 5], [7, 8, 9], [5, 4, 1]], u32)
    col = (np.arange(30, dtype=f32).reshape(10, 3) + f32(0.5)) / f32(32)
    nrm = -col
    return pts, col, nrm, tri


PLANTED = {
    "random": lambda: random_soup(1366, 1366) + (0.05,),
    "indexed": lambda: grid_mesh() + (0.03,),
    "dropped_representative": lambda: representative_in_a_dropped_triangle() + (1.0,),
    "one_cell": lambda: one_cell_soup(1000) + (1024.0,),
    "three_chains": lambda: three_chain_mesh(2000)[:4] + (1e18,),
    "boundaries": lambda: boundary_soup(0.05, reciprocal_mismatches(0.05)[:100]) + (0.05,),
    "too_wide": lambda: too_wide_mesh() + (0.05,),
}


def run_driver(args, timeout=600):
    r = subprocess.run([DRIVER] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, "MeshSimplify.bin %s failed (%d):\n%s\n%s" % (" ".join(map(str, args)), r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def read_mesh(directory):
    """-> (points, colors or None, normals or None, triangles) of a dump; an empty attribute file gives None"""
    def rows(name, dtype):
        f = os.path.join(directory, name)
        return np.fromfile(f, dtype).reshape(-1, 3) if os.path.exists(f) and os.path.getsize(f) else None
    pts, tri = rows("mesh_points.f32", f32), rows("mesh_triangles.u32", u32)
    return (np.zeros((0, 3), f32) if pts is None else pts, rows("mesh_colors.f32", f32), rows("mesh_normals.f32", f32), np.zeros((0, 3), u32) if tri is None else tri)


def simplify_through_driver(tmp, path, points, colors, normals, triangles, grid_len):
    """One mesh through geometry::TriangleMesh::ClusteringSimplify of the class surface (MeshSimplify.bin --mesh) -> (result.json, mesh)."""
    tmp = str(tmp)
    np.ascontiguousarray(points, f32).tofile(os.path.join(tmp, "in_points.f32"))
    np.ascontiguousarray(triangles, u32).tofile(os.path.join(tmp, "in_triangles.u32"))
    args = ["--mesh", os.path.join(tmp, "in_points.f32"), "--triangles", os.path.join(tmp, "in_triangles.u32"), "--grid", repr(float(grid_len)), "--path", path, "--dump", tmp]
    for name, a in (("colors", colors), ("normals", normals)):
        if a is not None:
            np.ascontiguousarray(a, f32).tofile(os.path.join(tmp, "in_%s.f32" % name))
            args += ["--" + name, os.path.join(tmp, "in_%s.f32" % name)]
    return run_driver(args), read_mesh(tmp)
