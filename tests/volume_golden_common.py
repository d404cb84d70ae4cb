"""Cases of tests/golden/volume_ops_reference.npz (numpy only): what oracle/tools/gen_volume_golden.py feeds to the REFERENCE's own
CubeHandler, and what the tests need to read the fixture -- its layout, the NaN rule and the block hash.  The generator stores every input
beside the reference's output; the tests read both from the fixture and never call the input builders below.

Fixture keys: "<case>/in/<array>" and "<case>/out/<array>".  A block set is keys [n,3] in sorted (x, y, z) order with voxels [n,512,5]
{sdf, weight, r, g, b} when n <= FULL_BLOCKS, else one 64-bit FNV-1a hash per block over its 512 x 5 float32 bit patterns in voxel-id order,
every NaN first replaced by 0x7fc00000 (x86 and GPU NaN sign / payload need not agree and nothing in the reference reads them).

LEFT_OUT names the cases that are not in the fixture, each with its reason."""
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "volume_ops_reference.npz")
FULL_BLOCKS = 8
NAN_BITS = np.uint32(0x7FC00000)

LEFT_OUT = {
    "fusion/frame_without_a_point_in_the_frustum":
        "ComputeBounding leaves max_pos / min_pos at -FLT_MAX / FLT_MAX and PrepareCubes converts floor(FLT_MAX / resolution) to int "
        "(CubeHandler.cpp:129-155, VoxelCube.h:68-74): undefined in the reference",
}


# ---- reading the fixture -------------------------------------------------------------------------------------------------------
def canonical_bits(vox):
    """float32 array -> its uint32 bit patterns with every NaN replaced by 0x7fc00000"""
    vox = np.ascontiguousarray(vox, np.float32)
    bits = vox.view(np.uint32).copy()
    bits[np.isnan(vox)] = NAN_BITS
    return bits


def block_hashes(vox):
    """[n,512,5] float32 -> [n] uint64: FNV-1a over each block's canonical bit patterns, little-endian bytes, voxel-id order"""
    data = canonical_bits(vox).reshape(len(vox), 512 * 5).view(np.uint8).astype(np.uint64)
    h = np.full(len(vox), 0xCBF29CE484222325, np.uint64)
    prime = np.uint64(0x100000001B3)
    with np.errstate(over="ignore"):
        for k in range(data.shape[1]):
            h ^= data[:, k]
            h *= prime
    return h


_fixture = None


def load():
    global _fixture
    if _fixture is None:
        with np.load(FIXTURE) as z:
            _fixture = {k: z[k] for k in z.files}
    return _fixture


def case_names(prefix):
    """the cases "<prefix>/<name>" of the fixture, sorted"""
    return sorted({k.split("/in/")[0] for k in load() if k.startswith(prefix + "/") and "/in/" in k})


def inputs(case):
    p = case + "/in/"
    return {k[len(p):]: v for k, v in load().items() if k.startswith(p)}


def outputs(case):
    p = case + "/out/"
    return {k[len(p):]: v for k, v in load().items() if k.startswith(p)}


def assert_block_set(out, name, keys, vox):
    """(keys, vox) sorted by key == the reference's block set `name` of `out`, bit for bit after the NaN rule"""
    want = out[name + "/keys"]
    assert keys.shape == want.shape and np.array_equal(keys, want), "%s: block ids differ (%d against %d)" % (name, len(keys), len(want))
    if name + "/voxels" in out:
        a, b = canonical_bits(vox), canonical_bits(out[name + "/voxels"])
        bad = np.argwhere(a != b)
        assert not len(bad), "%s: %d values differ, first at block %s voxel %d plane %d: %r against %r" % (
            name, len(bad), keys[bad[0][0]].tolist(), bad[0][1], bad[0][2], vox[tuple(bad[0])], out[name + "/voxels"][tuple(bad[0])])
    else:
        got = block_hashes(vox)
        bad = np.flatnonzero(got != out[name + "/hash"])
        assert not len(bad), "%s: %d of %d blocks differ, first %s" % (name, len(bad), len(keys), keys[bad[0]].tolist())


def sorted_rows(*cols):
    """rows of the concatenated columns, sorted lexicographically by their canonical bit patterns' float values"""
    a = np.concatenate([np.asarray(c, np.float32).reshape(len(cols[0]), -1) for c in cols], axis=1)
    return a[np.lexsort(a.T[::-1])]


def params(fx, fy, cx, cy, w, h, depth_scale, res, trunc, far, near):
    return np.array([fx, fy, cx, cy, w, h, depth_scale, res, trunc, far, near], np.float32)


# ---- input builders (generator only) ------------------------------------------------------------------------------------------
def _rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _pose(axis, angle, t, bottom=(0, 0, 0, 1)):
    T = np.eye(4)
    T[:3, :3] = _rot(axis, angle)
    T[:3, 3] = t
    T[3] = bottom
    return T.astype(np.float32)


def _camera(w, h):
    s = 640 // w
    return 514.817 / s, 515.375 / s, 318.771 / s, 238.447 / s, w, h, 1000.0


def _depth(w, h, seed, base, tilt=0.0):
    """metres: a tilted wall with a depth step of 0.3 m, 3 mm of per-pixel noise, a hole (0), a patch beyond the far plane (7 m) and one
    inside the near plane (0.2 m), single-pixel holes"""
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    d = base + tilt * (u / w - 0.5) + 0.1 * (v / h - 0.5) + 0.003 * rng.standard_normal((h, w))
    d[:, (5 * w) // 8:] += 0.3
    d[h // 6:h // 6 + h // 8, w // 5:w // 5 + w // 6] = 0.0
    d[(2 * h) // 3:(2 * h) // 3 + h // 8, w // 10:w // 10 + w // 8] = 7.0
    d[h // 2:h // 2 + h // 10, (3 * w) // 4:(3 * w) // 4 + w // 10] = 0.2
    d[::7, ::11] = 0.0
    return d


def _rgb(w, h, seed):
    """every pixel differs from its neighbours, every channel from the others (and the image still compresses)"""
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    blocks = np.random.default_rng(seed).integers(0, 256, (h // 10 + 1, w // 10 + 1, 3))
    return ((16 * (u % 8) + 29 * (v % 8))[..., None] + np.array([0, 85, 170]) + blocks[v // 10, u // 10]).astype(np.uint8)


def fusion_cases():
    """name -> {params, depth [n,h,w] u16 | f32, rgb [n,h,w,3] u8, poses [n,16]}"""
    def case(w, h, u16, res, frames, trunc=0.1, far=5.0, near=0.5, seed=0):
        depth = np.stack([_depth(w, h, seed + 10 * k, f[0], f[1]) for k, f in enumerate(frames)])
        depth = np.round(depth * 1000).astype(np.uint16) if u16 else (np.round(depth * 4096) / 4096).astype(np.float32)
        return {"params": params(*_camera(w, h), res, trunc, far, near), "depth": depth,
                "rgb": np.stack([_rgb(w, h, seed + 10 * k + 1) for k in range(len(frames))]),
                "poses": np.stack([f[2] for f in frames]).reshape(len(frames), 16)}

    out = {}
    out["u16_80x60_res002_rotating"] = case(80, 60, True, 0.02, [
        (1.5, 0.2, _pose((0, 1, 0), 0.00, (0.3, 0.2, 0.1))), (1.5, 0.2, _pose((0, 1, 0), 0.12, (0.35, 0.2, 0.1))),
        (1.45, 0.1, _pose((0.2, 1, 0.1), 0.25, (0.4, 0.25, 0.12)))], seed=100)
    out["f32_40x30_res001_negative_ids"] = case(40, 30, False, 0.01, [
        (0.7, 0.1, _pose((1, 0, 0), 0.05, (-0.9, -0.6, -1.3))), (0.72, 0.05, _pose((1, 0.3, 0), 0.10, (-0.92, -0.6, -1.3)))], seed=200)
    out["u16_40x30_res004_trunc_near_far"] = case(40, 30, True, 0.04, [
        (1.2, 0.3, _pose((0, 0, 1), 0.3 * k, (0.05 * k, -0.1, -0.4))) for k in range(4)], trunc=0.17, far=1.4, near=0.9, seed=300)
    out["f32_80x60_res004_step_noise"] = case(80, 60, False, 0.04, [
        (2.0, 0.6, _pose((0, 1, 0), -0.2, (-1.0, 0.0, 0.3))), (2.1, 0.5, _pose((0.1, 1, 0.1), -0.1, (-0.95, 0.05, 0.35)))], seed=400)
    out["u16_40x30_res004_two_frames"] = case(40, 30, True, 0.04, [
        (0.8, 0.1, _pose((0, 1, 0), 0.1, (0.1, -0.2, 0.05))), (0.82, 0.1, _pose((0.1, 1, 0), 0.2, (0.15, -0.2, 0.05)))], seed=600)
    # bottom row 0 0 0 2: ComputeBounding halves the cloud (TransformPoints divides by w), the update does not (head<3>() of pose_inv * p)
    out["u16_80x60_res002_bottom_row_2"] = case(80, 60, True, 0.02, [
        (1.5, 1.6, _pose((0, 1, 0), 0.05, (0.0, 0.0, 0.0), bottom=(0, 0, 0, 2))), (1.5, 1.6, _pose((0, 1, 0), 0.08, (0.02, 0.0, 0.0), bottom=(0, 0, 0, 2)))],
        seed=500)
    return out


HAND_RES = np.float32(0.02)
HAND_TRUNC = np.float32(0.1)
HAND_KEYS = np.array([[x, y, z] for x in (-1, 0) for y in (-1, 0) for z in (-1, 0)] + [[1, -1, 0], [2, 2, 2], [37, -41, 5]], np.int32)
ALL_DEFAULT_BLOCK = (1, -1, 0)          # present but never observed: the +x neighbour of (0, -1, 0)
LONE_BLOCKS = ((2, 2, 2), (37, -41, 5))  # no +x / +y / +z neighbour
# planted values: (block, voxel id, sdf, weight, colour or None = keep) -- layer 7 and interior voxels, so that mesh cells meet them
_t = HAND_TRUNC
PLANTED = [
    ((0, 0, 0), 0 + 8 * 0 + 64 * 0, 0.25, 0.0, None),              # weight 0 with |sdf| < 1
    ((0, 0, 0), 1 + 8 * 1 + 64 * 1, 0.0, 2.0, None),               # sdf 0.0
    ((0, 0, 0), 2 + 8 * 1 + 64 * 1, -0.0, 2.0, None),              # sdf -0.0
    ((0, 0, 0), 3 + 8 * 2 + 64 * 1, 1.0, 1.0, None),               # IsValid at sdf == 1
    ((0, 0, 0), 4 + 8 * 2 + 64 * 1, 0.99999994, 1.0, None),        # ... and one ulp below
    ((-1, 0, 0), 7 + 8 * 3 + 64 * 2, float(_t), 1.0, None),         # |sdf| == truncation exactly
    ((-1, 0, 0), 7 + 8 * 4 + 64 * 2, -float(_t), 1.0, None),
    ((-1, 0, 0), 6 + 8 * 3 + 64 * 2, float(np.nextafter(_t, np.float32(1))), 1.0, None),
    ((-1, 0, 0), 6 + 8 * 4 + 64 * 2, float(np.nextafter(_t, np.float32(0))), 1.0, None),
    ((0, -1, 0), 2 + 8 * 7 + 64 * 3, 0.3, -2.0, None),             # negative weight
    ((0, -1, -1), 3 + 8 * 3 + 64 * 7, float("nan"), 1.0, None),    # NaN sdf
    ((0, -1, -1), 5 + 8 * 3 + 64 * 7, float("inf"), 1.0, None),    # +inf sdf
    ((-1, -1, 0), 4 + 8 * 4 + 64 * 4, 0.2, float("nan"), None),    # NaN weight
    ((-1, -1, -1), 5 + 8 * 5 + 64 * 5, 0.15, 1.0, (-1.0, -1.0, -1.0)),  # default colour beside observed voxels
    ((2, 2, 2), 7 + 8 * 7 + 64 * 7, -0.05, 3.0, None),
]


def hand_volume():
    """(params, keys, voxels): a 2x2x2 cluster around the origin holding a sphere (radius 0.11 m: its zero set crosses the block borders at the
    blocks' last voxel layers), two lone blocks holding a tilted plane through their centres, one all-default block; sdf = distance / truncation
    where that is inside (-1, 1), default (999, 0, -1) elsewhere; then PLANTED."""
    keys = HAND_KEYS
    vox = np.empty((len(keys), 512, 5), np.float32)
    vox[..., 0], vox[..., 1], vox[..., 2:] = 999.0, 0.0, -1.0
    i = np.arange(512)
    off = np.stack([i & 7, (i >> 3) & 7, i >> 6], 1)
    normal = np.array([0.3, 0.2, 1.0]) / np.linalg.norm([0.3, 0.2, 1.0])
    for b, k in enumerate(keys):
        if tuple(k) == ALL_DEFAULT_BLOCK:
            continue
        p = (k[None, :] * 8 + off + 0.5) * float(HAND_RES)
        if tuple(k) in LONE_BLOCKS:
            d = (p - (k + 0.5) * 8 * float(HAND_RES)) @ normal
        else:
            d = np.linalg.norm(p - np.array([0.005, -0.003, 0.002]), axis=1) - 0.11
        s = (d / float(HAND_TRUNC)).astype(np.float32)
        obs = np.abs(s) < 1
        vox[b, obs, 0] = s[obs]
        vox[b, obs, 1] = (1 + (i % 4))[obs]
        vox[b, obs, 2:] = (0.5 + 0.5 * np.sin(p * np.array([9.0, 13.0, 17.0]) + b)).astype(np.float32)[obs]
    for blk, vid, sdf, w, col in PLANTED:
        b = int(np.flatnonzero((keys == blk).all(1))[0])
        vox[b, vid, 0], vox[b, vid, 1] = sdf, w
        if col is not None:
            vox[b, vid, 2:] = col
        elif vox[b, vid, 2] == -1:
            vox[b, vid, 2:] = (0.25, 0.5, 0.75)
    return params(*_camera(80, 60), HAND_RES, HAND_TRUNC, 5.0, 0.5), keys, vox


TRANSFORM_NAMES = ("identity", "shift_one_voxel", "shift_one_block", "shift_half_voxel", "small_rigid", "quarter_turn", "large_rotation",
                   "mirror", "scale_6", "scale_sixth", "bottom_row_2")


def transforms(res):
    """[11,16] float32 in the order of TRANSFORM_NAMES, for a volume of voxel size `res`"""
    res = np.float32(res)
    def shift(t):
        T = np.eye(4, dtype=np.float32); T[:3, 3] = t; return T
    def scale(s):
        T = np.eye(4, dtype=np.float32); T[0, 0] = T[1, 1] = T[2, 2] = s; return T
    quarter = np.array([[0, -1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)
    mirror = np.diag([-1, 1, 1, 1]).astype(np.float32)
    bottom = _pose((0, 0, 1), 0.1, (0.02, -0.01, 0.03), bottom=(0, 0, 0, 2))
    mats = [np.eye(4, dtype=np.float32), shift((res, 0, 0)), shift((0, -8 * res, 8 * res)), shift((res / 2, res / 2, -res / 2)),
            _pose((0.3, 1, 0.2), 0.07, (0.03, -0.02, 0.05)), quarter, _pose((1, 2, 3), 2.4, (0.1, 0.2, -0.3)), mirror,
            scale(np.float32(6)), scale(np.float32(1) / np.float32(6)), bottom]
    return np.stack(mats).reshape(len(mats), 16)


def merge_other(keys, vox):
    """the volume merged INTO the hand-built one: two of its blocks with other values -- weight zero on every third voxel, the opposite of the
    planted negative weight where that sits, one zero-weight voxel facing each kind of voxel -- and two blocks it does not have"""
    okeys = np.array([[0, -1, 0], [-1, 0, 0], [1, 0, 0], [-5, 3, 2]], np.int32)
    ovox = np.empty((4, 512, 5), np.float32)
    i = np.arange(512)
    for b in range(4):
        ovox[b, :, 0] = (0.9 * np.cos(0.37 * i + b)).astype(np.float32)
        ovox[b, :, 1] = np.where(i % 3 == 0, 0.0, 1.0 + (i % 5))
        ovox[b, :, 2:] = np.stack([(i % 7) / 7.0, (i % 11) / 11.0, (i % 13) / 13.0], 1)
    ovox[0, 2 + 8 * 7 + 64 * 3, 1] = 2.0      # meets the planted weight -2: the sum is 0
    return okeys, ovox


# ---- the checks, shared by the CPU oracle's and the HIP path's tests -------------------------------------------------------------
# `make(params)` gives an empty volume of either side behind one small interface (the adapters live in the test files):
#   prepare(depth, pose) -> ids [n,3]; integrate(depth, rgb, pose); integrate_cubes(depth, rgb, pose, ids) or None when the side has none;
#   export() -> (keys, vox) sorted; load(keys, vox); transform(T, nearest) -> volume; resolution(); merge(other, T=None) -> refused?;
#   point_cloud() -> (points, colors); mesh(tri_table, edge_pairs, only_block=None) -> (points, colors); add_cube(id); count();
#   write(path); read(path, legacy=False)
def sorted_bits(rows):
    """rows of a float32 matrix as canonical bit patterns, sorted lexicographically (so that -0.0 / 0.0 and NaN rows have one place)"""
    bits = canonical_bits(rows).reshape(len(rows), -1)
    return bits[np.lexsort(bits.T[::-1])]


def tables():
    out = outputs("tables")
    return out["tables/tri_table"], out["tables/edge_pairs"]


def check_fusion(make, case):
    cin, out = inputs(case), outputs(case)
    vol = make(cin["params"])
    listed = make(cin["params"])
    n = len(cin["poses"])
    for f in range(n):
        pose = cin["poses"][f].reshape(4, 4)
        ids = vol.prepare(cin["depth"][f], pose)
        want = out["frame%d/cube_id_list" % f]
        assert ids.shape == want.shape and np.array_equal(ids, want), "%s frame %d: cube_id_list differs (%d against %d)" % (case, f, len(ids), len(want))
        vol.integrate(cin["depth"][f], cin["rgb"][f], pose)
        assert_block_set(out, "frame%d" % f, *vol.export())
        if listed is not None and listed.integrate_cubes(cin["depth"][f], cin["rgb"][f], pose, want) is None:
            listed = None
    if listed is not None:  # Integrator::IntegrateImage over the reference's own candidate list
        assert_block_set(out, "frame%d" % (n - 1), *listed.export())


def loaded(make, case):
    cin = inputs(case)
    vol = make(cin["params"])
    vol.load(cin["keys"], cin["voxels"])
    return vol, cin, outputs(case)


def check_transform(make, case, k, nearest):
    vol, cin, out = loaded(make, case)
    res = vol.transform(cin["transforms"][k].reshape(4, 4), nearest)
    # TransformNearest never copies c_para into its result (CubeHandler.h:301-305): the default resolution
    assert np.float32(res.resolution()) == (np.float32(0.01) if nearest else cin["params"][7])
    assert_block_set(out, ("nearest%d" if nearest else "transform%d") % k, *res.export())


def check_point_cloud(make, case):
    vol, cin, out = loaded(make, case)
    p, c = vol.point_cloud()
    want = np.concatenate([out["point_cloud/points"], out["point_cloud/colors"]], 1)
    assert len(p) == len(want) > 0
    assert np.array_equal(sorted_bits(np.concatenate([p, c], 1)), sorted_bits(want))


def check_mesh(make, case):
    from helpers import triangle_soup
    vol, cin, out = loaded(make, case)
    tri, pairs = tables()
    total = 0
    for k, key in enumerate(cin["keys"]):  # GenerateMeshByCube: the streams in order
        p, c = vol.mesh(tri, pairs, only_block=key)
        wp, wc = out["block_mesh%d/points" % k], out["block_mesh%d/colors" % k]
        assert p.shape == wp.shape, "block %s: %d vertices against %d" % (key.tolist(), len(p), len(wp))
        assert np.array_equal(canonical_bits(p), canonical_bits(wp)) and np.array_equal(canonical_bits(c), canonical_bits(wc)), key.tolist()
        total += len(p)
    p, c = vol.mesh(tri, pairs)
    assert len(p) == len(out["mesh/points"]) == total > 0
    assert np.array_equal(sorted_bits(triangle_soup(p, c)), sorted_bits(triangle_soup(out["mesh/points"], out["mesh/colors"])))


def check_add_cube(make, case):
    vol, cin, out = loaded(make, case)
    counts = []
    for key in cin["add_cubes"]:
        vol.add_cube(key)
        counts.append(vol.count())
    assert counts == out["add_cubes/counts"].tolist()
    assert_block_set(out, "add_cubes", *vol.export())


def map_blocks(data):
    """the per-block byte strings of a .map stream, sorted (the reference writes its blocks in hash-map order)"""
    f = np.frombuffer(data, np.float32)
    n = int(np.frombuffer(data[:4], np.uint32)[0])
    ptr, blocks = 1, []
    for _ in range(n):
        start = ptr
        ptr += 3
        while f[ptr] != -2.0:
            ptr += 6
        ptr += 1
        blocks.append(f[start:ptr].tobytes())
    assert ptr == len(f)
    return sorted(blocks)


def check_map_file(make, case, tmp_path):
    vol, cin, out = loaded(make, case)
    ref_bytes = out["map_file/bytes"].tobytes()
    (tmp_path / "reference.map").write_bytes(ref_bytes)
    back = make(cin["params"])
    back.read(tmp_path / "reference.map")
    assert_block_set(out, "map_file", *back.export())
    vol.write(tmp_path / "own.map")
    own = (tmp_path / "own.map").read_bytes()
    assert len(own) == len(ref_bytes)
    a, b = map_blocks(own), map_blocks(ref_bytes)
    assert [canonical_bits(np.frombuffer(x, np.float32)).tobytes() for x in a] == [canonical_bits(np.frombuffer(x, np.float32)).tobytes() for x in b]
    again = make(cin["params"])
    again.read(tmp_path / "own.map")
    assert_block_set(out, "map_file", *again.export())


def check_legacy(make, tmp_path):
    cin, out = inputs("legacy"), outputs("legacy")
    (tmp_path / "legacy.map").write_bytes(cin["legacy_stream"].tobytes())
    vol = make(cin["params"])
    vol.read(tmp_path / "legacy.map", legacy=True)
    assert_block_set(out, "legacy", *vol.export())


def check_merge(make, case):
    hand, first = inputs("volume/hand"), inputs("merge/overlapping_and_disjoint")
    cin, out = inputs(case), outputs(case)
    dst = make(cin["params"])
    dst.load(hand["keys"], hand["voxels"])
    other = make(cin["other_params"])
    other.load(first["other_keys"], first["other_voxels"])
    T = cin["merge_transform"].reshape(4, 4) if "merge_transform" in cin else None
    refused = dst.merge(other, T)
    assert bool(refused) == (cin["other_params"][7] != cin["params"][7])
    assert_block_set(out, "merged", *dst.export())
