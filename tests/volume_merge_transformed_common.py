"""Cases and checks of op_volume_merge_transformed / _many (numpy only; the CPU oracle's and the HIP path's tests share them).

The entry is DEFINED as the sequence Transform(T_k) + Merge over the sources in order (include/onepiece_hip.h), so every expectation here is that
sequence: run on the CPU oracle it reproduces the reference's own run of tests/golden/volume_ops_reference.npz (test_volume_merge_transformed_cpu.py
C1), run on the device through the existing two entries -- which tests/test_volume_golden_gpu.py pins to the same fixture -- it is what the new
entry is compared with, bit for bit after the NaN rule, as block maps sorted by key.

A `make(params)` gives an empty volume of either side (the adapters of tests/test_volume_golden_cpu.py / _gpu.py): load, export, transform, merge."""
import numpy as np

import volume_golden_common as V

RES = V.HAND_RES  # 0.02: every case here uses the hand-built volume's parameters


def hand_params():
    return V.inputs("volume/hand")["params"]


def observed_block(key, seed):
    """one block, all 512 voxels observed: sdf in (-1, 1), weights 1..4, colours in (0, 1)"""
    i = np.arange(512)
    vox = np.empty((1, 512, 5), np.float32)
    vox[0, :, 0] = (0.8 * np.sin(0.21 * i + seed)).astype(np.float32)
    vox[0, :, 1] = 1 + ((i + seed) % 4)
    vox[0, :, 2:] = np.stack([((i + seed) % 7) / 7.0 + 0.05, (i % 11) / 11.0 + 0.03, (i % 13) / 13.0 + 0.02], 1)
    return np.asarray(key, np.int32).reshape(1, 3), vox


def rot_z(degrees, t):
    """rotation about z by Rodrigues' formula in double, cast to float32, with translation t"""
    a = np.deg2rad(float(degrees))
    K = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    T[:3, 3] = t
    return T.astype(np.float32)


def shift(t):
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = t
    return T


# ---- the cases: (dst (keys, vox) or None = empty, [(source index, T)], [source (keys, vox)]) ---------------------------------------------------
def case_g3(reverse=False):
    """dst = the hand volume; merge_other at the golden transforms 4 (small_rigid), 3 (shift_half_voxel), 5 (quarter_turn)"""
    hand, first = V.inputs("volume/hand"), V.inputs("merge/overlapping_and_disjoint")
    T = hand["transforms"].reshape(-1, 4, 4)
    order = [(0, T[4]), (0, T[3]), (0, T[5])]
    return (hand["keys"], hand["voxels"]), order[::-1] if reverse else order, [(first["other_keys"], first["other_voxels"])]


def case_g3_twice():
    """one source twice, at two poses"""
    dst, order, sources = case_g3()
    return dst, [order[0], order[2]], sources


def case_identity_reset():
    """one block of weight 2 everywhere, at the identity, into the same block of weight -2 everywhere: wherever the taps sit exactly on voxel
    centres the weight arrives unchanged and the sum is 0 -- the `reset` branch of the update"""
    (keys, vox), (_k, src) = observed_block((0, 0, 0), 3), observed_block((0, 0, 0), 4)
    vox[..., 1], src[..., 1] = -2.0, 2.0
    return (keys, vox), [(0, np.eye(4, dtype=np.float32))], [(keys, src)]


MEMBERSHIP_T_A = (45.0, (0.04, 0.14, 0.003))
MEMBERSHIP_BLOCK = (-1, 2, 0)


def case_g4(reverse=False):
    """The membership case.  Source A: block (0, 0, 0), every voxel observed, turned by 45 degrees about z and moved by (0.04, 0.14, 0.003): its claim
    set C_A has 8 blocks, and block (-1, 2, 0) is not one of them although A's backward taps reach observed voxels from there.  Source B: one observed
    block (-1, 2, 0) under shift_half_voxel, whose claim set holds (-1, 2, 0): the block is in the union, and must receive nothing from A."""
    A, B = observed_block((0, 0, 0), 1), observed_block(MEMBERSHIP_BLOCK, 2)
    TB = V.inputs("volume/hand")["transforms"].reshape(-1, 4, 4)[3]
    order = [(0, rot_z(*MEMBERSHIP_T_A)), (1, TB)]
    return None, order[::-1] if reverse else order, [A, B]


def case_g5_group_edge():
    """65 single-block sources, each half a block further along x than the last: destination blocks around x = 32 receive sources on both sides of
    the edge between the first group of 64 and the second"""
    sources = [observed_block((0, 0, 0), s) for s in range(65)]
    return None, [(s, shift((np.float32(4 * s) * RES, 0, 0))) for s in range(65)], sources


def case_g5_empty_source():
    """a source without blocks in the middle of the list"""
    dst, order, sources = case_g3()
    empty = (np.zeros((0, 3), np.int32), np.zeros((0, 512, 5), np.float32))
    return dst, [order[0], (1, order[1][1]), order[2]], sources + [empty]


def case_g5_empty_dst():
    dst, order, sources = case_g3()
    return None, order, sources


def case_g6():
    """the hand volume under scale_6 (far more blocks than the destination's pool holds)"""
    hand = V.inputs("volume/hand")
    return (hand["keys"], hand["voxels"]), [(0, hand["transforms"].reshape(-1, 4, 4)[8])], [(hand["keys"], hand["voxels"])]


def case_golden_transform(case, k):
    """volume `case` of the fixture under its transform k, into an empty destination: the reference's own transform<k> is the expectation"""
    cin = V.inputs(case)
    return None, [(0, cin["transforms"][k].reshape(4, 4))], [(cin["keys"], cin["voxels"])]


def case_golden_merge():
    """merge/with_transform of the fixture: the reference's own `merged` is the expectation"""
    hand, first, cin = V.inputs("volume/hand"), V.inputs("merge/overlapping_and_disjoint"), V.inputs("merge/with_transform")
    return (hand["keys"], hand["voxels"]), [(0, cin["merge_transform"].reshape(4, 4))], [(first["other_keys"], first["other_voxels"])]


# ---- both sides --------------------------------------------------------------------------------------------------------------------------------
def build(make, case, params=None):
    """-> (dst volume, [source volumes], [(source index, T)]) of one side"""
    params = hand_params() if params is None else params
    dst_blocks, order, sources = case
    dst = make(params)
    if dst_blocks is not None:
        dst.load(*dst_blocks)
    vols = []
    for keys, vox in sources:
        v = make(params)
        if len(keys):
            v.load(keys, vox)
        vols.append(v)
    return dst, vols, order


def two_step(make, case, trace=None, params=None):
    """the defining sequence on one side: dst.merge(source.transform(T)) in order -> the final (keys, vox); trace (a list) receives, per source,
    (the Transform result's (keys, vox), dst's (keys, vox) BEFORE that Merge)"""
    dst, vols, order = build(make, case, params)
    for s, T in order:
        tmp = vols[s].transform(np.asarray(T, np.float32).reshape(4, 4), False)
        if trace is not None:
            trace.append((tmp.export(), dst.export()))
        assert not dst.merge(tmp)
    return dst.export()


def assert_same_blocks(got, want, what):
    """two (keys, vox) sorted by key: equal bit for bit after the NaN rule"""
    gk, gv = got
    wk, wv = want
    assert gk.shape == wk.shape and np.array_equal(gk, wk), "%s: block ids differ (%d against %d)" % (what, len(gk), len(wk))
    a, b = V.canonical_bits(gv), V.canonical_bits(wv)
    bad = np.argwhere(a != b)
    assert not len(bad), "%s: %d values differ, first at block %s voxel %d plane %d: %r against %r" % (
        what, len(bad), gk[bad[0][0]].tolist(), bad[0][1], bad[0][2], gv[tuple(bad[0])], wv[tuple(bad[0])])


def differing_voxels(a, b):
    """how many voxels of two (keys, vox) differ (a block only one of them has counts with all its voxels)"""
    da = {tuple(k): V.canonical_bits(v) for k, v in zip(a[0].tolist(), a[1])}
    db = {tuple(k): V.canonical_bits(v) for k, v in zip(b[0].tolist(), b[1])}
    n = 512 * len(set(da) ^ set(db))
    for k in set(da) & set(db):
        n += int((da[k] != db[k]).any(axis=1).sum())
    return n


def expected_stats(trace, n_sources, src_blocks):
    """the counts of the definition from the two-step route's intermediates: the claim sets are the Transform results' block sets, and every
    (block of C_k, voxel) visit is classified by the comparisons of TSDFVoxel::operator+= in their order"""
    st = dict(sources=n_sources, src_blocks=src_blocks, touched_blocks=0, created_blocks=0, pairs=0, voxels_copied=0, voxels_kept=0, voxels_blended=0,
              voxels_reset=0)
    union, at_start = set(), None
    for (tk, tv), (dk, dv) in trace:
        have = {tuple(k): b for b, k in enumerate(dk.tolist())}
        if at_start is None:
            at_start = set(have)
        st["pairs"] += len(tk)
        union |= {tuple(k) for k in tk.tolist()}
        for b, k in enumerate(tk.tolist()):
            tw = dv[have[tuple(k)], :, 1] if tuple(k) in have else np.zeros(512, np.float32)   # AddCube: default voxels
            rw = tv[b, :, 1]
            with np.errstate(invalid="ignore"):
                copied = tw == 0
                kept = ~copied & (rw == 0)
                blended = ~copied & ~kept & ((tw + rw) != 0)      # (NaN != 0: a NaN weight lands here)
            st["voxels_copied"] += int(copied.sum())
            st["voxels_kept"] += int(kept.sum())
            st["voxels_blended"] += int(blended.sum())
            st["voxels_reset"] += int((~copied & ~kept & ~blended).sum())
    st["touched_blocks"] = len(union)
    st["created_blocks"] = len(union - (at_start or set()))
    return st
