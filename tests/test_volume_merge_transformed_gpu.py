"""op_volume_merge_transformed / _many on the device (include/onepiece_hip.h states the definition: the sequence Transform + Merge per source, in
order, without the intermediate volume).  G1 / G2 compare with the reference's own run (tests/golden/volume_ops_reference.npz), G3-G6 with the
two-step device route -- which tests/test_volume_golden_gpu.py pins to the same fixture and tests/test_volume_merge_transformed_cpu.py C1 shows to
be the reference's -- in the same order; bit for bit after the NaN rule, as block maps sorted by key.  G4 covers membership only while C3 of the
CPU file passes.  G7 the counts, G8 the destination's bookkeeping, G9 the driver."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import volume_golden_common as V
import volume_merge_transformed_common as M
from onepiece_amd import _lib as L
from onepiece_amd import integration as I
from test_volume_golden_gpu import HipVolume, make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _stats(st):
    return {k: int(getattr(st, k)) for k, _t in L.MergeTransformedStats._fields_}


def merge_single(dst, src, T):
    """the single C entry -> (return code, stats)"""
    T = np.ascontiguousarray(T, F32).reshape(16)
    st = L.MergeTransformedStats()
    rc = L.load().op_volume_merge_transformed(dst.v._h, src.v._h, _fp(T), None, C.byref(st))
    return rc, _stats(st)


def merge_many(dst, srcs, Ts):
    """the many C entry -> (return code, stats)"""
    Ts = np.ascontiguousarray(np.stack([np.asarray(T, F32).reshape(16) for T in Ts]) if len(srcs) else np.zeros((0, 16), F32))
    handles = (C.c_void_p * max(len(srcs), 1))(*[s.v._h for s in srcs])
    st = L.MergeTransformedStats()
    rc = L.load().op_volume_merge_transformed_many(dst.v._h, handles, _fp(Ts), None, len(srcs), C.byref(st))
    return rc, _stats(st)


def fused(case, params=None, dst_pool=None):
    """the case through ONE op_volume_merge_transformed_many call -> (dst (keys, vox), stats, dst volume)"""
    dst, vols, order = M.build(make, case, params)
    if dst_pool is not None:  # the same content in a volume created with a pool of `dst_pool` blocks
        small = HipVolume(dst.params, I.CubeHandler(dst.v.camera, max_blocks=dst_pool))
        small.v.SetVoxelResolution(float(dst.params[7]))
        small.v.SetTruncation(float(dst.params[8]))
        keys, vox = dst.export()
        if len(keys):
            small.load(keys, vox)
        dst = small
    dst.grows_before = dst.v.GrowthStats()["grows"]
    rc, st = merge_many(dst, [vols[s] for s, _T in order], [T for _s, T in order])
    assert rc == L.OP_OK, L.load().op_last_error()
    return dst.export(), st, dst


# ---- G1 -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["single", "many"])
@pytest.mark.parametrize("k", range(11), ids=V.TRANSFORM_NAMES)
@pytest.mark.parametrize("case", ("volume/hand", "volume/fused"))
def test_g1_into_an_empty_volume_it_is_the_references_transform(case, k, entry):
    params = V.inputs(case)["params"]
    dst, vols, order = M.build(make, M.case_golden_transform(case, k), params)
    rc, st = merge_single(dst, vols[0], order[0][1]) if entry == "single" else merge_many(dst, vols, [order[0][1]])
    assert rc == L.OP_OK, L.load().op_last_error()
    keys, vox = dst.export()
    V.assert_block_set(V.outputs(case), "transform%d" % k, keys, vox)
    assert st["sources"] == 1 and st["src_blocks"] == len(V.inputs(case)["keys"]) and st["touched_blocks"] == st["created_blocks"] == st["pairs"] == len(keys)
    assert st["voxels_copied"] == 512 * len(keys) and st["voxels_kept"] == st["voxels_blended"] == st["voxels_reset"] == 0


# ---- G2 -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["single", "many"])
def test_g2_merge_with_transform_is_the_references(entry):
    dst, vols, order = M.build(make, M.case_golden_merge())
    rc, _st = merge_single(dst, vols[0], order[0][1]) if entry == "single" else merge_many(dst, vols, [order[0][1]])
    assert rc == L.OP_OK, L.load().op_last_error()
    V.assert_block_set(V.outputs("merge/with_transform"), "merged", *dst.export())


def test_g2_a_resolution_mismatch_is_refused_and_changes_nothing(capsys):
    hand, first, cin = V.inputs("volume/hand"), V.inputs("merge/overlapping_and_disjoint"), V.inputs("merge/refused_resolution_mismatch")
    assert cin["other_params"][7] != cin["params"][7]
    dst, other, same = make(cin["params"]), make(cin["other_params"]), make(cin["params"])
    dst.load(hand["keys"], hand["voxels"])
    other.load(first["other_keys"], first["other_voxels"])
    same.load(first["other_keys"], first["other_voxels"])
    before = dst.export()
    T = np.eye(4, dtype=F32)
    for rc, st in (merge_single(dst, other, T), merge_many(dst, [other], [T]), merge_many(dst, [same, other], [T, T])):
        assert rc == L.OP_ERR_MISMATCH and L.load().op_last_error().decode() == "[Warning]::[MergeVoxelHash]::Voxel resolution is not identical."
        assert st["touched_blocks"] == 0
        M.assert_same_blocks(dst.export(), before, "after a refused call")
    V.assert_block_set(V.outputs("merge/refused_resolution_mismatch"), "merged", *dst.export())
    assert dst.v.MergeTransformed(other.v, T) is None and "Voxel resolution is not identical" in capsys.readouterr().out   # the Python surface: the warning line, no change
    M.assert_same_blocks(dst.export(), before, "after the refused MergeTransformed")


def test_g2_the_other_refusals_change_nothing():
    dst, vols, order = M.build(make, M.case_g3())
    before = dst.export()
    T = np.eye(4, dtype=F32).reshape(16)
    lib = L.load()
    handles = (C.c_void_p * 2)(vols[0].v._h, None)
    assert lib.op_volume_merge_transformed_many(dst.v._h, handles, _fp(np.tile(T, 2)), None, 2, None) == L.OP_ERR_INVALID      # a NULL source
    handles = (C.c_void_p * 2)(vols[0].v._h, dst.v._h)
    assert lib.op_volume_merge_transformed_many(dst.v._h, handles, _fp(np.tile(T, 2)), None, 2, None) == L.OP_ERR_INVALID      # the destination among the sources
    assert lib.op_volume_merge_transformed_many(dst.v._h, None, _fp(T), None, 1, None) == L.OP_ERR_INVALID
    assert lib.op_volume_merge_transformed_many(dst.v._h, handles, None, None, 1, None) == L.OP_ERR_INVALID
    assert lib.op_volume_merge_transformed(dst.v._h, None, _fp(T), None, None) == L.OP_ERR_INVALID
    assert lib.op_volume_merge_transformed(dst.v._h, dst.v._h, _fp(T), None, None) == L.OP_ERR_INVALID
    M.assert_same_blocks(dst.export(), before, "after the refused calls")


# ---- G3 - G6: against the two-step route -------------------------------------------------------------------------------------------------------------
CASES = {
    "g3_three_poses": lambda: M.case_g3(),
    "g3_three_poses_reversed": lambda: M.case_g3(reverse=True),
    "g3_one_source_twice": M.case_g3_twice,
    "g3_identity_weight_sum_zero": M.case_identity_reset,
    "g4_membership": lambda: M.case_g4(),
    "g4_membership_reversed": lambda: M.case_g4(reverse=True),
    "g5_group_edge_65_sources": M.case_g5_group_edge,
    "g5_empty_source_in_the_middle": M.case_g5_empty_source,
    "g5_empty_destination": M.case_g5_empty_dst,
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_g3_to_g5_one_call_equals_the_two_step_route(name):
    case = CASES[name]()
    trace = []
    want = M.two_step(make, case, trace)
    got, st, _dst = fused(case)
    M.assert_same_blocks(got, want, name)
    exp = M.expected_stats(trace, len(case[1]), sum(len(case[2][s][0]) for s, _T in case[1]))
    print(name, st)
    assert st == exp, (name, st, exp)                                                       # G7: the counts
    assert st["voxels_copied"] + st["voxels_kept"] + st["voxels_blended"] + st["voxels_reset"] == 512 * st["pairs"]
    if name == "g5_group_edge_65_sources":   # some destination blocks receive sources of both groups
        assert st["sources"] == 65 and st["pairs"] > st["touched_blocks"] > 65
    if name == "g3_identity_weight_sum_zero":
        assert st["voxels_reset"] >= 1
    if name.startswith("g3_three"):
        assert st["voxels_blended"] > 0 and st["voxels_kept"] > 0 and 0 < st["created_blocks"] < st["touched_blocks"]


def test_g5_no_sources_and_sources_without_blocks_change_nothing():
    dst, vols, _order = M.build(make, M.case_g3())
    before = dst.export()
    rc, st = merge_many(dst, [], [])
    assert rc == L.OP_OK and st == dict(sources=0, src_blocks=0, touched_blocks=0, created_blocks=0, pairs=0, voxels_copied=0, voxels_kept=0, voxels_blended=0,
                                        voxels_reset=0)
    empty = make(M.hand_params())
    rc, st = merge_many(dst, [empty, empty], [np.eye(4, dtype=F32)] * 2)
    assert rc == L.OP_OK and st["sources"] == 2 and st["pairs"] == 0
    M.assert_same_blocks(dst.export(), before, "after the empty calls")
    assert dst.v.MergeTransformed([], []) == dict(st, sources=0)


def test_g6_the_claim_pass_outgrows_the_pool_and_runs_again():
    case = M.case_g6()
    want = M.two_step(make, case)
    got, st, dst = fused(case, dst_pool=1)   # the smallest pool the constructor accepts
    M.assert_same_blocks(got, want, "g6")
    growth = dst.v.GrowthStats()
    print("g6:", st, growth)
    assert growth["grows"] > dst.grows_before and st["touched_blocks"] > 128 and st["created_blocks"] == len(want[0]) - len(case[0][0])


# ---- G8 -------------------------------------------------------------------------------------------------------------------------------------------
def test_g8_the_destination_is_kept_as_merge_keeps_it():
    """after G3, on the fused and on the two-step destination: RenderFrame from one pose gives byte-equal frames, one further IntegrateImage into each
    leaves equal maps, CollectGarbage reports equal counts"""
    case = M.case_g3()
    _got, _st, a = fused(case)
    b, vols, order = M.build(make, case)
    for s, T in order:
        assert not b.merge(vols[s], np.asarray(T, F32).reshape(4, 4))
    pose = np.eye(4, dtype=F32)
    pose[2, 3] = -0.8
    ra, rb = a.v.RenderFrame(pose), b.v.RenderFrame(pose)
    assert ra[2] == rb[2] > 0 and np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1].view(np.uint32), rb[1].view(np.uint32))
    w, h = int(a.params[4]), int(a.params[5])
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    depth = (0.75 + 0.002 * (u % 5)).astype(F32)
    rgb = np.stack([(3 * u + v) % 256, (u + 5 * v) % 256, (7 * u) % 256], 2).astype(np.uint8)
    for side in (a, b):
        side.integrate(depth, rgb, pose)
    M.assert_same_blocks(a.export(), b.export(), "after one more frame")
    ca, cb = a.v.CollectGarbage(), b.v.CollectGarbage()
    assert ca == cb and ca["blocks_kept"] > 0
    M.assert_same_blocks(a.export(), b.export(), "after CollectGarbage")


# ---- G9 -------------------------------------------------------------------------------------------------------------------------------------------
def test_g9_the_driver_places_and_recomposes_the_same_model_either_way(tmp_path):
    exe = os.path.join(ROOT, "examples", "cpp", "SubmapAlignment.bin")
    assert os.path.exists(exe), "examples/cpp/SubmapAlignment.bin is not built (__graft_entry__.build())"
    out = {}
    for merge, recompose in (("two-step", "single"), ("fused", "batch")):
        d = tmp_path / merge
        d.mkdir()
        run = subprocess.run([exe, "--synthetic", "24", "5", "1", "--submaps", "3", "--res", "0.02", "--iters", "3", "--merge", merge, "--recompose", recompose,
                              "--out", str(d)], capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
        out[merge] = json.loads(run.stdout.strip().splitlines()[-1])
        assert out[merge]["merge"] == merge and out[merge]["recompose"] == recompose and out[merge]["recompose_ms"] > 0
        assert out[merge]["recompose_stats"]["sources"] == 3 and out[merge]["recompose_stats"]["touched_blocks"] > 100
    assert out["fused"]["merge_stats"]["sources"] == 2 and out["two-step"]["merge_stats"]["sources"] == 0
    assert [r["T"] for r in out["fused"]["registered"]] == [r["T"] for r in out["two-step"]["registered"]]
    for name in ("model.map", "recomposed.map"):
        a, b = (V.map_blocks((tmp_path / m / name).read_bytes()) for m in ("two-step", "fused"))
        assert len(a) == len(b) > 100, (name, len(a), len(b))
        assert [V.canonical_bits(np.frombuffer(x, F32)).tobytes() for x in a] == [V.canonical_bits(np.frombuffer(x, F32)).tobytes() for x in b], name
    # a union counted once by the batch call, once per call by the single ones
    assert out["fused"]["recompose_stats"]["pairs"] == out["two-step"]["recompose_stats"]["pairs"]
    assert out["fused"]["recompose_stats"]["touched_blocks"] <= out["two-step"]["recompose_stats"]["touched_blocks"]
    bad = subprocess.run([exe, "--synthetic", "24", "5", "1", "--merge", "both"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "usage" in bad.stdout
