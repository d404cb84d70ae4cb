"""The CPU oracle against the REFERENCE's own CubeHandler (tests/golden/volume_ops_reference.npz, written by oracle/tools/gen_volume_golden.py
from a run of the reference's Integration/*.cpp): fusion, Transform / TransformNearest, Merge, GetPointCloud, the two mesh calls, AddCube and the
.map formats, case by case and bit for bit after the NaN rule of tests/volume_golden_common.py.  The HIP path meets the same fixture in
tests/test_volume_golden_gpu.py.  The self-checks at the end compute from the stored inputs that every edge the cases were built for occurs."""
import os

import numpy as np
import pytest

import volume_golden_common as V


class OracleVolume:
    def __init__(self, oracle, params, handle=None):
        self.o, self.params = oracle, params
        self.cam = oracle.make_camera(*[float(x) for x in params[:4]], int(params[4]), int(params[5]), float(params[6]))
        self.v = handle if handle is not None else oracle.Volume(self.cam, voxel_res=float(params[7]), trunc=float(params[8]), far=float(params[9]),
                                                                 near=float(params[10]))

    def prepare(self, depth, pose):
        return self.v.prepare_cubes(depth, pose)[0]

    def integrate(self, depth, rgb, pose):
        self.v.integrate(depth, rgb, pose)

    def integrate_cubes(self, depth, rgb, pose, ids):
        return None  # the oracle fuses through its own selection only

    def export(self):
        return self.v.export()

    def load(self, keys, vox):
        self.v.load(keys, vox)

    def transform(self, T, nearest):
        return OracleVolume(self.o, self.params, self.v.transform(T, nearest=nearest))

    def resolution(self):
        return self.v.resolution()

    def merge(self, other, T=None):
        if T is not None:
            if other.resolution() != self.resolution():  # CubeHandler.h:170-174
                return True
            other = other.transform(T, False)
        return self.v.merge(other.v) != 0

    def point_cloud(self):
        return self.v.point_cloud()

    def mesh(self, tri, pairs, only_block=None):
        return self.v.extract_mesh(tri, pairs, only_block=only_block)

    def count(self):
        return self.v.block_count()

    def add_cube(self, key):  # CubeHandler::AddCube (CubeHandler.h:192-198): a default block unless present
        keys, _ = self.v.export()
        if not (keys == np.asarray(key)).all(1).any():
            vox = np.empty((1, 512, 5), np.float32)
            vox[..., 0], vox[..., 1], vox[..., 2:] = 999.0, 0.0, -1.0
            self.v.load(np.asarray(key, np.int32).reshape(1, 3), vox)

    def write(self, path):
        assert self.v.write_file(path) == 0

    def read(self, path, legacy=False):
        assert self.v.read_file(path, legacy_float=legacy) == 0


@pytest.fixture
def make(oracle):
    return lambda params: OracleVolume(oracle, params)


FUSION = V.case_names("fusion")
VOLUMES = ("volume/hand", "volume/fused")
MERGES = V.case_names("merge")


def test_the_fixture_holds_the_cases_and_keeps_its_size():
    assert len(FUSION) == 6 and sorted(VOLUMES) == V.case_names("volume") and len(MERGES) == 3
    assert len(V.LEFT_OUT) <= 3 and all(len(reason) > 20 for reason in V.LEFT_OUT.values())
    golden = os.path.dirname(V.FIXTURE)
    assert os.path.getsize(V.FIXTURE) < os.path.getsize(os.path.join(golden, "nanoflann_golden.json"))
    for name in FUSION:  # 2-4 frames, both depth types, the three resolutions
        assert 2 <= len(V.inputs(name)["poses"]) <= 4
    assert {V.inputs(n)["depth"].dtype for n in FUSION} == {np.dtype(np.uint16), np.dtype(np.float32)}
    assert {float(V.inputs(n)["params"][7]) for n in FUSION} == {float(np.float32(r)) for r in (0.01, 0.02, 0.04)}
    assert any((V.outputs(n)["frame0/keys"] < 0).all(1).any() for n in FUSION)
    assert any(V.inputs(n)["poses"][0][15] != 1 for n in FUSION)
    assert len(V.inputs("volume/hand")["transforms"]) == len(V.TRANSFORM_NAMES) == 11


def test_block_hash_known_answers():
    """FNV-1a 64 as published: offset basis for no data is not reachable here, so one block of zeros and the NaN rule."""
    z = np.zeros((1, 512, 5), np.float32)
    h = 0xCBF29CE484222325
    for _ in range(512 * 5 * 4):
        h = (h * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    assert int(V.block_hashes(z)[0]) == h
    a, b = z.copy(), z.copy()
    a[0, 3, 1] = np.float32(np.nan)
    b.view(np.uint32)[0, 3, 1] = 0xFFC00123  # another NaN
    assert V.block_hashes(a)[0] == V.block_hashes(b)[0] != V.block_hashes(z)[0]


@pytest.mark.parametrize("case", FUSION)
def test_fusion(make, case):
    V.check_fusion(make, case)


@pytest.mark.parametrize("nearest", [False, True], ids=["trilinear", "nearest"])
@pytest.mark.parametrize("k", range(11), ids=V.TRANSFORM_NAMES)
@pytest.mark.parametrize("case", VOLUMES)
def test_transform(make, case, k, nearest):
    V.check_transform(make, case, k, nearest)


@pytest.mark.parametrize("case", MERGES)
def test_merge(make, case):
    V.check_merge(make, case)


@pytest.mark.parametrize("case", VOLUMES)
def test_point_cloud(make, case):
    V.check_point_cloud(make, case)


@pytest.mark.parametrize("case", VOLUMES)
def test_mesh(make, case):
    V.check_mesh(make, case)


@pytest.mark.parametrize("case", VOLUMES)
def test_add_cube(make, case):
    V.check_add_cube(make, case)


@pytest.mark.parametrize("case", VOLUMES)
def test_map_file(make, case, tmp_path):
    V.check_map_file(make, case, tmp_path)


def test_legacy_float_map(make, tmp_path):
    V.check_legacy(make, tmp_path)


# ---- the fixture exercises what it was built for (plain numpy over the stored inputs) -------------------------------------------
def _centres(keys, res):
    """voxel centres as GetGlobalPoint forms them (VoxelCube.h:75-80), float32: [n,512,3]"""
    i = np.arange(512)
    off = np.stack([i & 7, (i >> 3) & 7, i >> 6], 1).astype(np.float32)
    return (keys[:, None, :].astype(np.float32) * np.float32(8)) * res + (off[None] * res + res / np.float32(2))


def _hand():
    cin = V.inputs("volume/hand")
    return cin, cin["keys"], cin["voxels"], cin["params"][7], dict(zip(V.TRANSFORM_NAMES, cin["transforms"].reshape(-1, 4, 4)))


def test_selfcheck_planted_voxel_values():
    cin, keys, vox, res, T = _hand()
    sdf, w = vox[..., 0], vox[..., 1]
    trunc = cin["params"][8]
    assert ((w == 0) & (np.abs(sdf) < 1)).sum() >= 1
    assert ((sdf == 0) & ~np.signbit(sdf) & (w != 0)).sum() >= 1 and ((sdf == 0) & np.signbit(sdf) & (w != 0)).sum() >= 1
    assert (sdf == 1).sum() >= 1 and (sdf == np.float32(0.99999994)).sum() >= 1
    assert ((np.abs(sdf) == trunc) & (w != 0)).sum() == 2 and (sdf == trunc).sum() == 1 and (sdf == -trunc).sum() == 1
    assert (sdf == np.nextafter(trunc, np.float32(1))).sum() == 1 and (sdf == np.nextafter(trunc, np.float32(0))).sum() == 1
    assert (w < 0).sum() >= 1 and np.isnan(sdf).sum() >= 1 and np.isposinf(sdf).sum() >= 1 and np.isnan(w).sum() >= 1
    assert ((w > 0) & (vox[..., 2] == -1)).sum() >= 1
    assert any((w[b] == 0).all() and (sdf[b] == 999).all() for b in range(len(keys)))
    cluster = {(x, y, z) for x in (-1, 0) for y in (-1, 0) for z in (-1, 0)}
    assert cluster <= {tuple(k) for k in keys.tolist()} and (37, -41, 5) in {tuple(k) for k in keys.tolist()}
    # the zero set crosses block borders at a block's last voxel layer: a sign change between layer 7 and the neighbour's layer 0
    b0, b1 = [int(np.flatnonzero((keys == k).all(1))[0]) for k in ((-1, 0, 0), (0, 0, 0))]
    last, first = vox[b0].reshape(8, 8, 8, 5)[:, :, 7], vox[b1].reshape(8, 8, 8, 5)[:, :, 0]
    both = (last[..., 1] > 0) & (first[..., 1] > 0)
    assert (both & ((last[..., 0] > 0) != (first[..., 0] > 0))).sum() >= 1


def _tap_weights(keys, res, shift):
    """x / y / z weights of ReadVoxelInterpolate (VoxelCube.cpp:11-13) at the voxels of blocks `keys` under a pure shift (whose inverse is exact)"""
    pos = (_centres(keys, res) - shift[None, None, :]) - res / np.float32(2)
    n0 = np.floor(pos / res)
    return (pos - n0 * res) / res


def test_selfcheck_taps_on_voxel_centres_have_weights_of_exactly_zero():
    """Transform already takes half a voxel off the position (CubeHandler.h:263-264), so it is the identity and the shifts by whole voxels that put
    every tap on a voxel centre -- interpolation weights of exactly 0, the `_weight == 0` branch of TSDFVoxel::operator* (TSDFVoxel.h:61) -- while the
    shift by half a voxel blends equally (weights 0.5)."""
    cin, keys, vox, res, T = _hand()
    observed = vox[..., 1] != 0
    for name in ("identity", "shift_one_voxel", "shift_one_block"):
        assert np.array_equal(T[name][:3, :3], np.eye(3)) and T[name][3].tolist() == [0, 0, 0, 1]
        wgt = _tap_weights(keys, res, T[name][:3, 3])
        assert ((wgt == 0).all(axis=2) & observed).sum() > 1000, name
    half = _tap_weights(keys, res, T["shift_half_voxel"][:3, 3])
    assert np.abs(half - 0.5).max() < 1e-3
    # a weight of exactly 0 meets the voxels whose product with 0 is not 0: the NaN weight, the NaN and the infinite sdf
    assert np.isnan(vox[..., 1]).any() and np.isnan(vox[..., 0]).any() and np.isinf(vox[..., 0]).any()


def test_selfcheck_scale_6_overflows_the_claim_set():
    """one source block's voxels reach more than 128 distinct result blocks (kClaimSet of k_transform_alloc)"""
    cin, keys, vox, res, T = _hand()
    pos = _centres(keys, res) * np.float32(6) - res / np.float32(2)
    p0 = np.floor(pos / res).astype(np.int64)
    most = 0
    for b in range(len(keys)):
        ids = {tuple(r) for k in range(8) for r in ((p0[b] + [(k & 1), (k >> 1) & 1, (k >> 2) & 1]) >> 3).tolist()}
        most = max(most, len(ids))
    assert most > 128
    assert T["scale_6"][0, 0] == 6 and T["scale_6"][3, 3] == 1


def test_selfcheck_scale_sixth_leaves_the_tap_box():
    """one result block's taps span more than 64 source blocks (kSrcBox of k_transform_fill_wave): the fill falls back to a probe per tap"""
    out = V.outputs("volume/hand")
    cin, keys, vox, res, T = _hand()
    rkeys = out["transform9/keys"]
    pos = _centres(rkeys, res) * np.float32(6) - res / np.float32(2)        # trans^-1 = scale by 6
    p0 = np.floor(pos / res).astype(np.int64)
    lo, hi = p0.min(1) >> 3, (p0.max(1) + 1) >> 3
    boxes = np.prod(hi - lo + 1, axis=1)
    assert boxes.max() > 64
    # ... and the box of such a block holds source blocks that exist
    have = {tuple(k) for k in keys.tolist()}
    b = int(np.argmax(boxes))
    inside = [k for k in have if all(lo[b][a] <= k[a] <= hi[b][a] for a in range(3))]
    assert len(inside) >= 1


def test_selfcheck_mesh_cells_meet_absent_neighbours():
    """per direction, a cell on the last layer whose own-block corners are all valid while the neighbour block is absent (CubeHandler.cpp:93-97)"""
    cin, keys, vox, res, T = _hand()
    have = {tuple(k) for k in keys.tolist()}
    valid = ~((vox[..., 0] >= 1) | (vox[..., 1] <= 0))        # TSDFVoxel::IsValid
    for axis in range(3):
        cells = 0
        for b, k in enumerate(keys.tolist()):
            nb = list(k); nb[axis] += 1
            if tuple(nb) in have:
                continue
            g = valid[b].reshape(8, 8, 8)                       # [z, y, x]
            layer = np.take(g, 7, axis=2 - axis)                # the last layer along `axis`
            cells += int((layer[:-1, :-1] & layer[1:, :-1] & layer[:-1, 1:] & layer[1:, 1:]).sum())
        assert cells >= 1, axis
    # and a neighbour that is present but holds nothing valid
    assert tuple(V.ALL_DEFAULT_BLOCK) in have


def test_selfcheck_merge_meets_every_weight_combination():
    hand, first = V.inputs("volume/hand"), V.inputs("merge/overlapping_and_disjoint")
    have = {tuple(k): b for b, k in enumerate(hand["keys"].tolist())}
    seen = set()
    disjoint = overlapping = 0
    for b, k in enumerate(first["other_keys"].tolist()):
        if tuple(k) not in have:
            disjoint += 1
            continue
        overlapping += 1
        wa, wb = hand["voxels"][have[tuple(k)], :, 1], first["other_voxels"][b, :, 1]
        seen |= set(zip((wa != 0).tolist(), (wb != 0).tolist()))
        assert ((wa + wb == 0) & (wa != 0)).sum() >= 1 or tuple(k) != (0, -1, 0)   # weights -2 and 2: the sum is 0
    assert disjoint >= 1 and overlapping >= 1 and seen == {(False, False), (False, True), (True, False), (True, True)}
