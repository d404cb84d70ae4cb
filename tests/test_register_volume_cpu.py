"""Volume against volume without a device: the numpy restatement (tests/volume_register_volume_common.py) of op_volume_band_voxels' selection and
of the offset system on hand-made blocks where everything has a closed form, the selection's edges, and the restated Gauss-Newton loop on two
overlapping submaps against the TRUTH.

The convergence case: the forty 64 x 48 frames of the robust tests' model (2 cm voxels, truncation 0.1); submap A is frames [:25], submap B frames
[15:], both fused by the oracle at their true poses, so the true transformation is the identity; the start is D.perturbed(identity, 1), 41.8 mm /
0.97 degrees off.  B's band voxels (band 0.04, stride 2, min_weight 1: 14 845 points) are registered against A under GRADIENT, 15 iterations,
min_step 1e-5.  Measured with this restatement (float32 rows, the library's float32 solve): 3.112 mm / 0.074 degrees after 6 iterations,
CONVERGED, 10 684 of 14 845 used; the same points with target value 0: 14.349 mm / 0.102 degrees after 5 iterations."""
import ctypes as C
import os

import numpy as np
import pytest

import volume_register_color_common as K
import volume_register_common as R
import volume_register_robust_common as B
import volume_register_volume_common as V
import volume_sample_common as S

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(4, dtype=F32)
NAMES = ("op_volume_band_default_params", "op_volume_band_voxels", "op_volume_register_offset_system", "op_volume_register_offset_points",
         "op_volume_register_volume")


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _hand():
    vox = B.steep_blocks(color=True)
    return vox, S.Grid(R.HAND_KEYS, vox, R.HAND_RES)


@pytest.mark.parametrize("mode", [B.NORMAL, B.GRADIENT, B.METRIC])
@pytest.mark.parametrize("color_scale", [0.0, 1.0])
def test_hand_blocks_register_onto_themselves(hip, mode, color_scale):
    """The source is the target and T = I: at a voxel centre g is an integer, the sample is the stored value exactly, so every used residual --
    s - o and m - y -- is exactly 0, sums[21..27] are 0, and one loop step leaves T the identity with CONVERGED."""
    vox, grid = _hand()
    xyz, sdf, y, index = V.select(R.HAND_KEYS, vox, R.HAND_RES, 0.25)
    assert len(xyz) == 4 * 64 * 2 and np.array_equal(np.abs(sdf), np.full(len(sdf), 1 / 32, F32))   # |2 (z - Z0)| <= 1/16: the two layers next to Z0, in the four lower blocks
    w = V.rows_of(grid, xyz, sdf, y, EYE, 0.25, color_scale=color_scale, mode=mode)
    used = w["reason"] == 0
    assert 100 < used.sum() < len(xyz) and (w["reason"] != 3).all()   # the voxels on the outer faces have no complete sample
    assert not w["rows"][:, 6].any() and not w["r"].any() and not w["rows"][:, 14].any()
    assert np.array_equal(w["s"][used], sdf[used])                    # the stored sdf itself, where the residual is zero
    assert w["colored"].sum() == (used.sum() if color_scale > 0 else 0)
    sums, _b, counts = V.fold(w)
    assert not sums[21:29].any() and sums[30] == 0 and sums[29] == used.sum() / 1024 and sums[0:21].any()
    res = V.loop(hip.load(), lambda T: V.system(grid, xyz, sdf, y, T, 0.25, color_scale=color_scale, mode=mode), EYE, 5, min_step=1e-5)
    assert res["status"] == R.CONVERGED and res["iterations"] == 1 and res["last_step"] == 0.0
    assert np.array_equal(_bits(res["T"]), _bits(EYE)) and res["rmse_residual"] == 0.0 and res["rmse"] == 1 / 32
    # target value 0 on the same points is the system a user had before: its residual is the stored sdf
    z = V.rows_of(grid, xyz, np.zeros_like(sdf), y, EYE, 0.25, color_scale=color_scale, mode=mode)
    assert np.array_equal(z["reason"], w["reason"]) and z["rows"][used, 6].all()


def test_zero_offsets_are_the_robust_rows():
    vox, grid = _hand()
    q = R.hand_cloud()
    with np.errstate(all="ignore"):
        c = F32(0.5) + q[:, 0]
        y = K.intensity(np.stack([c, c, c], axis=1))
    y[::7] += F32(0.03125)
    T = EYE.copy()
    T[:3, 3] = [1 / 128, 0, -1 / 128]
    for mode in (B.NORMAL, B.GRADIENT, B.METRIC):
        for cs, huber, huber_color in ((0.0, 0.0, 0.0), (0.0, 1 / 64, 0.0), (0.6, 0.0, 0.0), (0.6, 1 / 64, 1 / 64)):
            want = B.rows_of(grid, q, y, T, 0.25, cs, 0.05, mode, huber, huber_color)
            got = V.rows_of(grid, q, np.zeros(len(q), F32), y, T, 0.25, cs, 0.05, mode, huber, huber_color)
            assert (want["reason"] == 0).sum() > 50
            for k in want:
                a, b = want[k], got[k]
                assert np.array_equal(_bits(a), _bits(b)) if a.dtype == F32 else np.array_equal(a, b), (mode, cs, huber, k)
            none = V.rows_of(grid, q, None, y, T, 0.25, cs, 0.05, mode, huber, huber_color)
            assert all(np.array_equal(want[k], none[k], equal_nan=True) for k in want)


def test_offsets_move_the_residual_and_nothing_else():
    """dyadic target values on the slope-two field: r = (s - o) per mode, the gate and sums[29] on s; NaN and inf are invalid"""
    _vox, grid = _hand()
    q = R.hand_cloud()
    o = (np.arange(len(q)) % 5 - 2).astype(F32) / F32(64.0)
    o[3::11] = np.nan
    o[5::13] = np.inf
    o[6::17] = -np.inf
    plain = B.rows_of(grid, q, None, EYE, 0.1)
    assert all((plain["reason"] == k).any() for k in range(4))
    for mode, div in ((B.NORMAL, 1), (B.GRADIENT, 1), (B.METRIC, 2)):
        base = B.rows_of(grid, q, None, EYE, 0.1, mode=mode)
        w = V.rows_of(grid, q, o, None, EYE, 0.1, mode=mode)
        fin = np.isfinite(o)
        assert np.array_equal(w["reason"], np.where(fin, plain["reason"], 1)) and (~fin & (plain["reason"] == 0)).any()
        used = w["reason"] == 0
        assert np.array_equal(w["rows"][used, :6], base["rows"][used, :6])          # the row does not see the target value
        assert np.array_equal(w["r"][used], (base["s"][used] - o[used]) / F32(div)) and np.array_equal(w["rows"][used, 6], w["r"][used])
        assert np.array_equal(w["s"][used], base["s"][used]) and not w["rows"][~used].any()
        sums, _b, counts = V.fold(w)
        assert counts["used"] == used.sum() and counts["invalid"] == (plain["reason"] == 1).sum() + (~fin & (plain["reason"] != 1)).sum()
        assert sums[29] == np.sum(base["s"][used].astype(np.float64) ** 2) and sums[30] == np.sum(w["r"][used].astype(np.float64) ** 2)
        # the gate is on the stored sdf: a point 3/8 away stays too far whatever its target value says
        far = plain["reason"] == 3
        assert far.any() and (w["reason"][far & fin] == 3).all()
    h = V.rows_of(grid, q, o, None, EYE, 0.1, mode=B.NORMAL, huber=1 / 64)
    n = V.rows_of(grid, q, o, None, EYE, 0.1, mode=B.NORMAL)
    assert np.array_equal(h["down"], np.abs(n["r"]) > F32(1 / 64)) and h["down"].any() and not h["down"].all()


def _one_block(weight, sdf):
    vox = np.empty((1, 512, 5), F32)
    vox[..., 0], vox[..., 1], vox[..., 2:] = sdf, weight, 0.25
    return np.zeros((1, 3), np.int32), vox


def test_selection_edges():
    res, trunc = 0.02, 0.1
    keys, vox = _one_block(1.0, 0.01)
    below = np.nextafter(F32(3.0), F32(0.0))
    vox[0, 0, 1], vox[0, 1, 1], vox[0, 2, 1], vox[0, 3, 1] = below, 3.0, 0.0, -1.0
    assert V.select(keys, vox, res, trunc, min_weight=3.0)[3][:, 1].tolist() == [1]      # just below min_weight is out, exactly at it is in
    assert len(V.select(keys, vox, res, trunc, min_weight=0.0)[0]) == 510               # min_weight 0 still wants w > 0
    band = F32(0.04)
    keys, vox = _one_block(1.0, 1.0)
    vox[0, :6, 0] = [band, -band, np.nextafter(band, F32(1.0)), np.nan, 0.0, -0.0]
    assert V.select(keys, vox, res, trunc, band=0.04)[3][:, 1].tolist() == [0, 1, 4, 5]   # |sdf| exactly at the band is in, NaN is out
    vox[0, 6, 0], vox[0, 7, 0] = F32(trunc), np.nextafter(F32(trunc), F32(1.0))
    assert V.select(keys, vox, res, trunc, band=0.0)[3][:, 1].tolist() == [0, 1, 2, 4, 5, 6]   # band <= 0: the truncation
    assert V.select(keys, vox, res, trunc, band=-1.0)[3][:, 1].tolist() == [0, 1, 2, 4, 5, 6]
    assert V.default_band(res) == float(F32(2.0) * F32(res))
    vox[0, 8, 0] = F32(V.default_band(res))
    assert V.select(keys, vox, res, trunc)[3][:, 1].tolist() == [0, 1, 4, 5, 8]           # the default: 2 res, weight 1, stride 1
    # default voxels (sdf 999, weight 0, colour -1) are never selected
    dk, dv = _one_block(0.0, 999.0)
    assert len(V.select(dk, dv, res, trunc, band=1e9, min_weight=0.0)[0]) == 0
    # the lattice of a stride: 512, 64, 8, 1 candidates per block, in voxel order, at the centres S.block_voxel_centres gives
    keys = np.array([[1, -2, 3], [0, 0, 0]], np.int32)
    vox = np.concatenate([_one_block(2.0, 0.01)[1], _one_block(2.0, -0.01)[1]])
    vox[..., 2:] = np.random.default_rng(1).random((2, 512, 3), dtype=F32)
    centres = S.block_voxel_centres(keys, res)
    for stride, per_block in ((1, 512), (2, 64), (4, 8), (8, 1)):
        xyz, sdf, y, index = V.select(keys, vox, res, trunc, stride=stride)
        assert len(xyz) == 2 * per_block and np.array_equal(index[:, 0], np.repeat([0, 1], per_block))
        v = index[:per_block, 1]
        assert (np.diff(v) > 0).all() and ((v & 7) % stride == 0).all() and (((v >> 3) & 7) % stride == 0).all() and ((v >> 6) % stride == 0).all()
        assert np.array_equal(_bits(xyz), _bits(centres[index[:, 0], index[:, 1]])) and np.array_equal(sdf, np.repeat([0.01, -0.01], per_block).astype(F32))
        assert np.array_equal(_bits(y), _bits(K.intensity(vox[index[:, 0], index[:, 1], 2:])))


def test_submap_converges_on_its_neighbour(oracle, hip):
    """B's band voxels against A (the module docstring's case).  The float64 experiment of the design note ended at 3.1 mm; 6 mm leaves room for the
    float32 solve.  Measured: 3.112 mm, 0.074 degrees, 6 iterations, 10 684 of 14 845 used; with target value 0: 14.349 mm."""
    res, t, r, selected = V.case(oracle, hip.load(), offsets=True)
    zero, t0, _r0, _n = V.case(oracle, hip.load(), offsets=False)
    assert selected == 14845
    assert t < 0.006, t
    assert t < t0, (t, t0)                                            # nearer than the same points with target value 0
    assert res["used"] >= selected / 2, (res["used"], selected)       # a condition: the case cannot pass by shedding points
    assert res["status"] == R.CONVERGED and res["iterations"] <= V.CASE_ITERATIONS and r < 0.2


def test_bindings_and_refusals_without_a_device(hip):
    """the header, the bindings and the class surface name the entries; the NULL refusals are decided before any device use"""
    header = open(os.path.join(ROOT, "include", "onepiece_hip.h")).read()
    lib = hip.load()
    for name in NAMES:
        assert name + "(" in header and hasattr(lib, name), name
    assert C.sizeof(hip.BandParams) == 12 and C.sizeof(hip.RegisterVolumeResult) == C.sizeof(hip.RegisterRobustResult) + 8
    T = EYE.reshape(16).copy()
    fp = T.ctypes.data_as(hip._fp)
    r, n = hip.RegisterVolumeResult(), C.c_size_t(0)
    assert lib.op_volume_register_volume(None, None, fp, None, None, None, C.byref(r)) == hip.OP_ERR_INVALID
    assert lib.op_last_error().startswith(b"op_volume_register_volume:"), lib.op_last_error()             # the entry's own name
    assert lib.op_volume_band_voxels(None, None, None, None, None, hip.OP_MEM_HOST, 0, C.byref(n)) == hip.OP_ERR_INVALID
    assert lib.op_volume_band_default_params(None, C.byref(hip.BandParams())) == hip.OP_ERR_INVALID
    sums = np.zeros(31)
    assert lib.op_volume_register_offset_system(None, None, None, None, 0, hip.OP_MEM_HOST, fp, 0.1, 0.0, 0.0, None, sums.ctypes.data_as(C.POINTER(C.c_double)), None,
                                                None) == hip.OP_ERR_INVALID
    assert lib.op_last_error().startswith(b"op_volume_register_offset_system:"), lib.op_last_error()
    assert lib.op_volume_register_offset_points(None, None, None, None, 0, hip.OP_MEM_HOST, fp, None, None, C.byref(hip.RegisterRobustResult())) == hip.OP_ERR_INVALID
    assert lib.op_last_error().startswith(b"op_volume_register_offset_points:"), lib.op_last_error()
    from onepiece_amd import integration as I
    for name in ("BandVoxels", "RegisterPointsOffset", "OffsetRegistrationSystem", "RegisterVolume"):
        assert callable(getattr(I.CubeHandler, name)), name
