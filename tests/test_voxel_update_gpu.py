"""voxel_update<true> (csrc/integrate.hip) -- the update of a volume only the fusion kernel has written, with one unrefined
hardware reciprocal of the integer weight sum and three operations per quotient (csrc/volume_core.hpp div_int_rcp) -- on
the device, against the two-branch form with four IEEE divisions (op_debug_voxel_update), bit for bit.

The operands are what such a volume can hold (integer weights, colours that are means of byte / 255, stored defaults) and
what the guard has to catch: weight sums around and far beyond 2^19, sdf numerators that cancel to nothing, to just below
and to just above 2^-60 -- each alone, and all of them mixed lane by lane so that one wave takes both paths at once.
tests/test_voxel_quotient_cpu.py is the same statement in exact arithmetic for ANY reciprocal within 2^-23 / b of 1 / b;
test_hardware_reciprocal_is_within_the_proofs_hypothesis checks that v_rcp_f32 is such a reciprocal."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 1 << 20
B_MAX = 1 << 19     # voxel_update<true>: a weight sum above it takes the plain division
GUARD = 2.0 ** -60  # ... and so does an sdf numerator below it


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _update(s, w, c, new_sdf, rgba):
    """-> (out_fast, out_ref) as uint32 [n, 5]"""
    from onepiece_amd import _lib as L
    lib = L.load()
    n = len(s)
    s, w, new_sdf = (np.ascontiguousarray(a, np.float32) for a in (s, w, new_sdf))
    c = [np.ascontiguousarray(c[:, k], np.float32) for k in range(3)]
    rgba = np.ascontiguousarray(rgba, np.uint32)
    assert all(len(a) == n for a in (w, new_sdf, rgba, c[0]))
    fast, ref = np.empty((n, 5), np.float32), np.empty((n, 5), np.float32)
    L.check(lib.op_debug_voxel_update(_vp(s), _vp(w), _vp(c[0]), _vp(c[1]), _vp(c[2]), _vp(new_sdf), _vp(rgba), n, _vp(fast), _vp(ref)))
    return fast.view(np.uint32), ref.view(np.uint32)


def _byte_means(rng, w):
    """Colours a fused voxel can hold after w observations: the float32 nearest to (a sum of w bytes) / 255 / w; w <= 0: the default -1."""
    wi = np.maximum(w.astype(np.int64), 1)[:, None]
    total = rng.integers(0, 255 * wi + 1, (len(w), 3))
    return np.where((w <= 0)[:, None], np.float32(-1.0), (total / (255.0 * wi)).astype(np.float32))


def _rgba(rng, n):
    return rng.integers(0, 1 << 24, n).astype(np.uint32) | np.uint32(1 << 24)   # byte 3 of a packed pixel is 1


def _sdf(rng, n, trunc=0.04):
    return rng.uniform(-trunc, trunc, n).astype(np.float32)


def _weights_group(rng, w):
    w = w.astype(np.float32)
    return _sdf(rng, len(w)), w, _byte_means(rng, w), _sdf(rng, len(w)), _rgba(rng, len(w))


def _invalid_group(rng, n):
    """stored voxels TSDFVoxel::IsValid refuses: the default {999, 0, -1}, an sdf >= 1 under a positive weight, a weight <= 0"""
    kind = rng.integers(0, 4, n)
    s = np.choose(kind, [np.float32(999.0), rng.uniform(1.0, 3.0, n).astype(np.float32), _sdf(rng, n), np.float32(1.0)]).astype(np.float32)
    w = np.choose(kind, [np.float32(0.0), rng.integers(1, 2000, n).astype(np.float32), -rng.integers(0, 3, n).astype(np.float32), np.float32(7.0)]).astype(np.float32)
    c = np.where((kind == 0)[:, None], np.float32(-1.0), rng.uniform(0, 1, (n, 3)).astype(np.float32))
    return s, w, c, _sdf(rng, n), _rgba(rng, n)


def _colour_group(rng, n):
    """every byte value in every channel, against means of bytes of every small weight"""
    w = rng.integers(1, 300, n).astype(np.float32)
    b = np.arange(n, dtype=np.uint32) & 0xff
    rgba = b | (((b * 7 + 3) & 0xff) << 8) | (((255 - b) & 0xff) << 16) | np.uint32(1 << 24)
    assert len(np.unique(rgba & 0xff)) == 256 and len(np.unique((rgba >> 8) & 0xff)) == 256 and len(np.unique((rgba >> 16) & 0xff)) == 256
    return _sdf(rng, n), w, _byte_means(rng, w), _sdf(rng, n), rgba


def _cancel_group(rng, n, mode):
    """w * s + new_sdf = ns exactly, with ns = 0 (mode 0), just above the guard threshold (1: 2^-60 .. 2^-60 + 8 * 2^-80 and a few
    binades up) or just below it (2: down to 2^-80); either sign.  The stored sdf is tiny so that the sum's last place is 2^-80."""
    w = rng.integers(1, 2000, n).astype(np.float32)
    s = (rng.integers(1 << 20, 1 << 21, n) * 2.0 ** -80 / w.astype(np.float64)).astype(np.float32) * rng.choice(np.float32([-1, 1]), n)
    p = (w * s).astype(np.float32).astype(np.float64)            # the product as the kernel rounds it
    unit = 2.0 ** -80
    if mode == 0:
        j = np.zeros(n)
    elif mode == 1:
        j = 2.0 ** 20 + rng.integers(0, 9, n) * np.where(rng.random(n) < 0.5, 1.0, 2.0 ** rng.integers(0, 12, n))
    else:
        j = np.where(rng.random(n) < 0.5, 2.0 ** 20 - rng.integers(1, 9, n), rng.integers(1, 1 << 20, n)).astype(np.float64)
    ns = j * unit * rng.choice([-1.0, 1.0], n)
    new = (ns - p).astype(np.float32)
    ok = (new.astype(np.float64) == ns - p) & (new != 0)         # keep the cases where the observation is a float (nearly all); no -0
    assert ok.mean() > 0.9
    s, w, new = s[ok], w[ok], new[ok]
    got = (w * s + new).astype(np.float32)
    assert np.array_equal(got.astype(np.float64), ns[ok])
    below = (np.abs(got) < np.float32(GUARD)) & (got != 0)
    assert (mode == 0 and not got.any()) or (mode == 1 and not below.any() and (np.abs(got) == np.float32(GUARD)).any()) or (mode == 2 and below.all())
    k = len(s)
    return s, w, _byte_means(rng, w), new, _rgba(rng, k)


def _groups(rng, n):
    yield "w in {0,1,2,3,31,1999}", _weights_group(rng, rng.choice([0, 1, 2, 3, 31, 1999], n))
    yield "w random below 2^19", _weights_group(rng, rng.integers(1, B_MAX, n))
    yield "w in 2^19-2 .. 2^19+2", _weights_group(rng, B_MAX + rng.integers(-2, 3, n))
    yield "w = 2^24", _weights_group(rng, np.full(n, 1 << 24))
    yield "w = 2^25 - 1", _weights_group(rng, np.full(n, (1 << 25) - 1))
    yield "stored invalid voxels", _invalid_group(rng, n)
    yield "byte colours", _colour_group(rng, n)
    yield "sdf numerator cancels to 0", _cancel_group(rng, n, 0)
    yield "sdf numerator just above 2^-60", _cancel_group(rng, n, 1)
    yield "sdf numerator just below 2^-60", _cancel_group(rng, n, 2)


def _agree(name, ops):
    fast, ref = _update(*ops)
    bad = np.flatnonzero((fast != ref).any(axis=1))
    assert len(bad) == 0, "%s: %d of %d differ; first: s w c new rgba = %r -> fast %r ref %r" % (
        name, len(bad), len(fast), [np.asarray(a)[bad[0]].tolist() for a in ops], fast[bad[0]].view(np.float32).tolist(), ref[bad[0]].view(np.float32).tolist())
    return ref.view(np.float32)


def test_hardware_reciprocal_is_within_the_proofs_hypothesis():
    """div_int_rcp's hypothesis: y = v_rcp_f32(b) has |y - 1/b| <= 2^-23 / b for every integer b in [1, 2^19] -- |y b - 1| <= 2^-23,
    which float64 evaluates without rounding (24 + 20 bits) -- and v_rcp_f32(1) = 1."""
    from onepiece_amd import _lib as L
    lib = L.load()
    b = np.arange(1, B_MAX + 1, dtype=np.float32)
    y = np.empty_like(b)
    L.check(lib.op_debug_rcp(_vp(b), len(b), _vp(y)))
    err = np.abs(y.astype(np.float64) * b.astype(np.float64) - 1.0)
    worst = int(np.argmax(err))
    print("v_rcp_f32 over [1, 2^19]: max |y b - 1| = 2^%.3f at b = %d" % (np.log2(err[worst]), worst + 1))
    assert err[worst] <= 2.0 ** -23, (worst + 1, float(y[worst]), err[worst])
    assert y[0] == 1.0
    pow2 = b[np.log2(b) % 1 == 0]
    assert np.array_equal(y[pow2.astype(np.int64) - 1], (1.0 / pow2).astype(np.float32))


def test_fast_update_equals_the_divisions_group_by_group():
    rng = np.random.default_rng(2019)
    for name, ops in _groups(rng, N):
        ref = _agree(name, ops)
        if name == "w random below 2^19":   # the hook's reference IS the reference's formula: numpy's float32 arithmetic is IEEE too
            s, w, c, new, rgba = ops
            assert np.array_equal(ref[:, 0], (w * s + new) / (w + np.float32(1))) and np.array_equal(ref[:, 1], w + np.float32(1))
            n0 = (rgba & 0xff).astype(np.float32) / np.float32(255.0)
            assert np.array_equal(ref[:, 2], (w * c[:, 0] + n0) / (w + np.float32(1)))
        if name == "stored invalid voxels":  # replaced by the observation
            assert np.array_equal(ref[:, 0], ops[3]) and np.all(ref[:, 1] == 1.0)


def test_fast_update_with_every_group_in_every_wave():
    """The groups dealt lane by lane: every wave of 64 holds weights on both sides of 2^19, cancelled and ordinary numerators, invalid
    voxels -- guarded and unguarded lanes side by side under one ballot."""
    rng = np.random.default_rng(64)
    parts = [ops for _name, ops in _groups(rng, N // 8)]
    k = min(len(p[0]) for p in parts)
    cols = []
    for j in range(5):
        a = np.stack([np.asarray(p[j])[:k] for p in parts], axis=1)      # [k, groups(, 3)]: consecutive lanes come from different groups
        cols.append(a.reshape((-1,) + a.shape[2:]))
    assert len(cols[0]) >= N
    _agree("mixed", tuple(c[:N] for c in cols))


def test_one_batch_fused_twice_gives_identical_bytes():
    """32 frames of 64 x 48 pixels, one k_integrate launch, into two fresh volumes: the guard's ballot (like everything else in the
    kernel) leaves no dependence on which lanes share a wave or on the order workgroups draw blocks."""
    import torch
    from onepiece_amd import integration as I, synthetic as S
    s = 10
    cam = I.PinholeCamera()
    cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height = S.FX / s, S.FY / s, S.CX / s, S.CY / s, S.W // s, S.H // s
    assert (cam.width, cam.height) == (64, 48)
    dev = torch.device("cuda:0")
    poses = np.stack([S.room_pose(200 + i) for i in range(32)])
    frames = [S.room_render(p, xp=torch, device=dev, width=cam.width, height=cam.height, fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy) for p in poses]
    depth, rgb = torch.stack([f[0] for f in frames]).contiguous(), torch.stack([f[1] for f in frames]).contiguous()
    torch.cuda.synchronize()
    maps = []
    for _ in range(2):
        hv = I.CubeHandler(cam, device=0, max_blocks=1 << 16)
        hv.SetVoxelResolution(0.02)
        hv.IntegrateSequence(depth, rgb, poses)
        hv.Synchronize()
        assert hv.Stats()["launches"] == 1 and hv.Stats()["voxels_updated"] > 100000
        maps.append(hv.GetCubeMap())
    (ka, va), (kb, vb) = maps
    assert len(ka) > 100 and np.array_equal(ka, kb) and va.tobytes() == vb.tobytes()
