"""op_volume_merge_transformed / _many without a GPU: the sequence that DEFINES the entry (Transform + Merge per source, in order), run on the CPU
oracle, reproduces the reference's own run (C1), so what tests/test_volume_merge_transformed_gpu.py expects is the reference's; the cases bite (C2:
order matters, C3: the membership case is real); the header and the binding declare the entries (C4) and they refuse a NULL volume (C5)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import volume_golden_common as V
import volume_merge_transformed_common as M
from test_volume_golden_cpu import OracleVolume

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS_FIELDS = ["sources", "src_blocks", "touched_blocks", "created_blocks", "pairs", "voxels_copied", "voxels_kept", "voxels_blended", "voxels_reset"]


@pytest.fixture
def make(oracle):
    return lambda params: OracleVolume(oracle, params)


# ---- C1 -------------------------------------------------------------------------------------------------------------------------------------------
def test_c1_the_sequence_reproduces_the_references_merge_with_transform(make):
    V.assert_block_set(V.outputs("merge/with_transform"), "merged", *M.two_step(make, M.case_golden_merge()))


@pytest.mark.parametrize("k", range(11), ids=V.TRANSFORM_NAMES)
@pytest.mark.parametrize("case", ("volume/hand", "volume/fused"))
def test_c1_into_an_empty_destination_the_sequence_is_the_references_transform(make, case, k):
    V.assert_block_set(V.outputs(case), "transform%d" % k, *M.two_step(make, M.case_golden_transform(case, k), params=V.inputs(case)["params"]))


# ---- C2 -------------------------------------------------------------------------------------------------------------------------------------------
def test_c2_order_matters_in_the_three_source_case(make):
    given, reverse = M.two_step(make, M.case_g3()), M.two_step(make, M.case_g3(reverse=True))
    n = M.differing_voxels(given, reverse)
    print("voxels that differ between the two orders:", n)
    assert n >= 1


# ---- C3 -------------------------------------------------------------------------------------------------------------------------------------------
def _resampled_outside_the_claim_set(make, keys, vox, T, block):
    """ReadVoxelInterpolate of the source (keys, vox) at the voxels of `block`, which is NOT in the source's claim set under T: the source is given
    one more, never observed block (default voxels: what an absent block reads as, so no value anywhere changes) whose own claim set holds `block`,
    and Transform of that is read at `block`.  None when no such helper block is found."""
    res = float(M.RES)
    centre = (np.asarray(block, np.float64) * 8 + 4) * res
    back = np.linalg.inv(T.astype(np.float64)) @ np.append(centre, 1.0)
    home = np.floor(back[:3] / back[3] / res / 8).astype(np.int64)
    have = {tuple(k) for k in keys.tolist()}
    default = np.empty((1, 512, 5), np.float32)
    default[..., 0], default[..., 1], default[..., 2:] = 999.0, 0.0, -1.0
    for d in sorted(np.ndindex(3, 3, 3), key=lambda d: sum(abs(c - 1) for c in d)):
        helper = tuple(int(h + c - 1) for h, c in zip(home, d))
        if helper in have:
            continue
        v = make(M.hand_params())
        v.load(np.concatenate([keys, np.asarray(helper, np.int32).reshape(1, 3)]), np.concatenate([vox, default]))
        rk, rv = v.transform(T, False).export()
        at = np.flatnonzero((rk == np.asarray(block)).all(1))
        if len(at):
            return rv[int(at[0])]
    return None


def test_c3_the_membership_case_is_real(make):
    """at least one (block, source) pair: the block is in the union of the claim sets, not in C_k, and source k resampled there has observed voxels"""
    _dst, order, sources = M.case_g4()
    claims = []
    for s, T in order:
        v = make(M.hand_params())
        v.load(*sources[s])
        claims.append({tuple(k) for k in v.transform(T, False).export()[0].tolist()})
    union = set().union(*claims)
    print("claim set sizes:", [len(c) for c in claims], "union:", len(union))
    assert M.MEMBERSHIP_BLOCK in union and M.MEMBERSHIP_BLOCK not in claims[0] and M.MEMBERSHIP_BLOCK in claims[1]
    found = []
    for k, (s, T) in enumerate(order):
        for block in sorted(union - claims[k]):
            r = _resampled_outside_the_claim_set(make, sources[s][0], sources[s][1], T, block)
            if r is not None and (r[:, 1] != 0).any():
                found.append((block, k, int((r[:, 1] != 0).sum())))
    print("(block, source, voxels of weight != 0 the source would give there):", found)
    assert any(block == M.MEMBERSHIP_BLOCK and k == 0 for block, k, _n in found)


# ---- C4 -------------------------------------------------------------------------------------------------------------------------------------------
def test_c4_the_header_and_the_binding_declare_the_entries(hip):
    text = open(os.path.join(ROOT, "include", "onepiece_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*op_volume_merge_transformed_stats\s*;", code)
    assert m, "op_volume_merge_transformed_stats is not declared"
    assert re.fullmatch(r"\s*uint64_t\s+(.*?);\s*", m.group(1), flags=re.S), m.group(1)
    assert [f.strip() for f in re.fullmatch(r"\s*uint64_t\s+(.*?);\s*", m.group(1), flags=re.S).group(1).split(",")] == STATS_FIELDS
    assert re.search(r"int\s+op_volume_merge_transformed\s*\(\s*op_volume\s*\*\s*dst\s*,\s*op_volume\s*\*\s*src\s*,\s*const\s+float\s+T\[16\]\s*,\s*const\s+float\s*\*\s*T_inv\s*,"
                     r"\s*op_volume_merge_transformed_stats\s*\*\s*stats\s*\)\s*;", code)
    assert re.search(r"int\s+op_volume_merge_transformed_many\s*\(\s*op_volume\s*\*\s*dst\s*,\s*op_volume\s*\*\s*const\s*\*\s*srcs\s*,\s*const\s+float\s*\*\s*Ts\s*,"
                     r"\s*const\s+float\s*\*\s*T_invs\s*,\s*size_t\s+n\s*,\s*op_volume_merge_transformed_stats\s*\*\s*stats\s*\)\s*;", code)
    assert [(k, t) for k, t in hip.MergeTransformedStats._fields_] == [(k, C.c_uint64) for k in STATS_FIELDS]
    assert C.sizeof(hip.MergeTransformedStats) == 72
    assert len(hip.SIGNATURES["op_volume_merge_transformed"][1]) == 5 and len(hip.SIGNATURES["op_volume_merge_transformed_many"][1]) == 6
    lib = hip.load()
    assert hasattr(lib, "op_volume_merge_transformed") and hasattr(lib, "op_volume_merge_transformed_many")


# ---- C5 -------------------------------------------------------------------------------------------------------------------------------------------
def test_c5_both_entries_refuse_a_null_destination_without_a_device(hip):
    lib = hip.load()
    T = np.eye(4, dtype=np.float32).reshape(16)
    fp = T.ctypes.data_as(C.POINTER(C.c_float))
    st = hip.MergeTransformedStats()
    assert lib.op_volume_merge_transformed(None, None, fp, None, C.byref(st)) == hip.OP_ERR_INVALID
    assert lib.op_volume_merge_transformed_many(None, None, fp, None, 0, C.byref(st)) == hip.OP_ERR_INVALID
    assert lib.op_volume_merge_transformed_many(None, None, None, None, 3, None) == hip.OP_ERR_INVALID
    assert st.sources == 0 and lib.op_last_error()
