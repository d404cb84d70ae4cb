"""k_integrate's frame loop after two removals (csrc/integrate.hip, volume_core.hpp, px_round.hpp):
  * the certified pixel projection multiplies by v_rcp_f32(Z) as the hardware delivers it; its error bound rests on |1 - Z y| <= d_rcp
    (px_round.hpp kPxRcpErr, read through op_debug_px_rcp_err), which the first test holds the device to over every significand;
  * the lean instantiations read voxels_updated, voxels_written and the store mask off the weights after the frames (kWCount) instead of
    counting ballots per update; every other instantiation keeps the counters it had.
The projection is compared with the host's double formula (Integrator.cpp:20-21: the float quotient (f X) / Z, then + 0.5 + c in double,
truncated toward zero) around every pixel boundary of a 640 x 480 and a 37 x 29 camera; fusion with the CPU oracle: block keys, every voxel bit
for bit, both counters equal to the oracle's counts.

Fusion shapes: 33 frames (a full 32-frame launch + a 1-frame launch) and 70 frames (32 + 32 + 6: weights carried across batches) of the room at
37 x 29 and 64 x 48 into 4 cm voxels; truncation 0.1 (lean) and 0.6 (plain, not lean: the ballot counters); a sequence whose truncation goes
0.1 -> 0.6 -> 0.1 between batches (lean, plain, plain: the counts continue across instantiations); a volume that is not plain; the raycaster's
summaries present; a pool of 64 blocks that has to grow (the poisoned batch is replayed); Clear() and the same again.  voxels_written counts,
per launch, the voxels the launch stored: for the oracle, the voxels whose bits differ before and after the launch's frames.

(A pair form of the certificate -- one decision for a thread's two voxels -- was measured and not kept: there is one projection per lane in
op_debug_project_uv_image as in the kernel, and the waves below mix certified and uncertified lanes in their first half, their second half,
both and neither.)"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from onepiece_amd import integration as I, synthetic as S

INT_MIN = np.iinfo(np.int32).min


# ---- the reciprocal ------------------------------------------------------------------------------------------------------------------
def _rcp(lib, L, x):
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    L.check(lib.op_debug_rcp(C.c_void_p(x.ctypes.data), len(x), C.c_void_p(out.ctypes.data)))
    return out


def test_unrefined_reciprocal_is_within_d_rcp_for_every_significand():
    from onepiece_amd import _lib as L
    lib = L.load()
    d_rcp = lib.op_debug_px_rcp_err()
    assert 2.0 ** -24 <= d_rcp <= 2.0 ** -22
    rng = np.random.default_rng(7)
    sig = np.arange(1 << 23, dtype=np.uint32)
    sets = [("[1, 2)", (sig | np.uint32(0x3f800000)).view(np.float32)), ("[-2, -1)", (sig | np.uint32(0xbf800000)).view(np.float32))]
    for e in (-60, -1, 59):
        s = rng.integers(0, 1 << 23, 1 << 16).astype(np.uint32)
        sets.append(("binade 2^%d" % e, ((np.uint32(127 + e) << np.uint32(23)) | s).view(np.float32)))
    worst = 0.0
    for name, z in sets:
        y = _rcp(lib, L, z)
        err = np.abs(1.0 - z.astype(np.float64) * y.astype(np.float64))   # exact: a 24 x 24 bit product and a difference near 0
        i = int(np.argmax(err))
        print("%s: max |1 - Z y| = %.9g = %.5f * 2^-23 at Z = %r" % (name, err[i], err[i] / 2.0 ** -23, float(z[i])))
        worst = max(worst, float(err[i]))
        assert err[i] <= d_rcp, (name, float(z[i]), float(y[i]))
    assert worst > 2.0 ** -25                                            # (the sweep saw a reciprocal that is not correctly rounded: it measures something)


# ---- the projection ------------------------------------------------------------------------------------------------------------------
PCAMS = {
    "640x480": (514.817, 515.375, 318.771, 238.447, 640, 480),
    "37x29": (30.0, 30.0, 18.25, 14.25, 37, 29),
}


def _project(lib, L, cam, X, Y, Z):
    fx, fy, cx, cy, w, h = cam
    X, Y, Z = (np.ascontiguousarray(a, np.float32) for a in (X, Y, Z))
    out = np.empty((len(X), 4), np.int32)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    L.check(lib.op_debug_project_uv_image(float(fx), float(fy), float(cx), float(cy), int(w), int(h), vp(X), vp(Y), vp(Z), len(X), 0, vp(out)))
    return out


def _host_pixel(f, c, P, Z):
    """Integrator.cpp:20-21 on the host: a = (f * P) / Z in float, t = (double)a + 0.5 + (double)c, truncated toward zero; INT_MIN where no int holds it."""
    with np.errstate(all="ignore"):
        a = (np.float32(f) * P.astype(np.float32)) / Z.astype(np.float32)
        t = a.astype(np.float64) + 0.5 + np.float64(np.float32(c))
        ok = (t > -2147483649.0) & (t < 2147483648.0)
        return np.where(ok, np.trunc(np.where(ok, t, 0.0)), INT_MIN).astype(np.int64)


def _agree(cam, out, X, Y, Z):
    fx, fy, cx, cy, w, h = cam
    ru, rv = _host_pixel(fx, cx, X, Z), _host_pixel(fy, cy, Y, Z)
    r_in = (ru >= 0) & (ru < w) & (rv >= 0) & (rv < h)
    f_in = out[:, 0] != INT_MIN
    bad = (r_in != f_in) | (r_in & ((out[:, 0] != ru) | (out[:, 1] != rv)))
    assert not bad.any(), (np.flatnonzero(bad)[:5], out[bad][:5], ru[bad][:5], rv[bad][:5])
    return float(r_in.mean())


def _band_operands(rng, n, f, c, extent, width, risky):
    """P and Z with (f * P) / Z + c + 0.5 within +-width of an integer in [-3, extent + 3] on the lanes `risky`, anywhere in the image on the others."""
    k = rng.integers(-3, extent + 4, n).astype(np.float64)
    t = np.where(risky, k + rng.uniform(-width, width, n), rng.uniform(0.0, extent, n))
    Z = rng.uniform(0.2, 8.0, n) * np.where(rng.random(n) < 0.05, -1.0, 1.0)
    a = t - (np.float64(np.float32(c)) + 0.5)
    P = (a * Z / np.float64(np.float32(f))).astype(np.float32)
    return P, Z.astype(np.float32)


@pytest.mark.parametrize("name", list(PCAMS))
def test_projection_equals_the_double_formula_around_every_pixel_boundary(name):
    from onepiece_amd import _lib as L
    lib = L.load()
    cam = PCAMS[name]
    fx, fy, cx, cy, w, h = cam
    rng = np.random.default_rng(13)
    n = 1 << 19
    lane, wave = np.arange(n) & 63, (np.arange(n) >> 6) & 3
    # waves by turns: all lanes near a boundary, the first half only, the second half only, a random eighth
    risky = (wave == 0) | ((wave == 1) & (lane < 32)) | ((wave == 2) & (lane >= 32)) | ((wave == 3) & (rng.random(n) < 0.125))
    other = lambda m, e: rng.uniform(0.05, 0.95, m) * e
    # 2e-5 lies inside the band the certificate refuses at 640 pixels (h2 = 1.8e-4 of a unit interval), 2e-4 straddles it, 5e-3 is mostly outside it
    for width in (2e-5, 2e-4, 5e-3):
        X, Z = _band_operands(rng, n, fx, cx, w, width, risky)
        Y = ((other(n, h) - (cy + 0.5)) * Z / fy).astype(np.float32)
        _agree(cam, _project(lib, L, cam, X, Y, Z), X, Y, Z)
        Y, Z = _band_operands(rng, n, fy, cy, h, width, risky)
        X = ((other(n, w) - (cx + 0.5)) * Z / fx).astype(np.float32)
        _agree(cam, _project(lib, L, cam, X, Y, Z), X, Y, Z)
    # both axes at once: x within the band, y a few ulp around exact boundary quotients
    X, Z = _band_operands(rng, n, fx, cx, w, 2e-4, risky)
    Y = ((rng.integers(-2, h + 3, n) - (np.float64(np.float32(cy)) + 0.5)) * Z.astype(np.float64) / np.float64(np.float32(fy))).astype(np.float32)
    Y = (Y.view(np.int32) + rng.integers(-8, 9, n).astype(np.int32)).view(np.float32)
    _agree(cam, _project(lib, L, cam, X, Y, Z), X, Y, Z)
    # camera-like operands: mostly the fast path, a good share inside the image
    Z = rng.uniform(0.05, 20.0, n).astype(np.float32)
    X, Y = (rng.uniform(-1, 1, n) * Z * (0.7 * w / fx)).astype(np.float32), (rng.uniform(-1, 1, n) * Z * (0.7 * h / fy)).astype(np.float32)
    assert _agree(cam, _project(lib, L, cam, X, Y, Z), X, Y, Z) > 0.3
    # the specials of tests/test_px_certified_gpu.py mixed into waves of ordinary lanes
    sp = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38, 0.0, -0.0, 1e-45, 2.0 ** -61, 2.0 ** 61, 1e7, -1e7], np.float32)
    m = 1 << 16
    X, Y, Z = (rng.uniform(lo, hi, m).astype(np.float32) for lo, hi in ((-1, 1), (-1, 1), (0.5, 4)))
    for arr in (X, Y, Z):
        idx = rng.integers(0, m, m // 64)
        arr[idx] = rng.choice(sp, len(idx))
    out = _project(lib, L, cam, X, Y, Z)
    fin = ~np.isinf(Z)   # Z = +-inf: the plain quotient is 0, the shared reciprocal NaN (no pixel) -- as in tests/test_px_certified_gpu.py
    _agree(cam, out[fin], X[fin], Y[fin], Z[fin])
    assert np.all(out[~fin][:, :2] == INT_MIN)


# ---- fusion --------------------------------------------------------------------------------------------------------------------------
RES = 0.04
N = 70
# (fx, fy, cx, cy, width, height, depth_scale): principal points with short fractions, so that both axes take the certified projection
CAMS = {
    "37x29": (30.0, 30.0, 18.25, 14.25, 37, 29, 1000.0),
    "64x48": (52.0, 52.0, 31.75, 23.25, 64, 48, 1000.0),
}
DEFAULT = np.array([999, 0, -1, -1, -1], np.float32).view(np.uint32)
_cache = {}


def _frames(shape):
    """(depth [N,h,w], rgb [N,h,w,3], poses [N,4,4]) on the host, rendered once per shape; frames 3 apart so that the views overlap."""
    key = ("frames", shape)
    if key not in _cache:
        cam = CAMS[shape]
        poses = np.stack([S.room_pose(300 + 3 * k) for k in range(N)]).astype(np.float32)
        fr = [S.room_render(p, width=cam[4], height=cam[5], fx=cam[0], fy=cam[1], cx=cam[2], cy=cam[3]) for p in poses]
        _cache[key] = (np.stack([f[0] for f in fr]), np.stack([f[1] for f in fr]), poses)
    return _cache[key]


def _device(shape):
    import torch
    key = ("device", shape)
    if key not in _cache:
        d, c, _p = _frames(shape)
        dev = torch.device("cuda:0")
        _cache[key] = (torch.from_numpy(d).to(dev).contiguous(), torch.from_numpy(c).to(dev).contiguous())
        torch.cuda.synchronize()
    return _cache[key]


def _changed(before, after):
    """Voxels whose bits differ between two states (keys, voxels) of the volume (None: the empty volume) = what a launch between them stores."""
    ka, xa = after
    xa = xa.view(np.uint32)
    row = {} if before is None else {tuple(k): i for i, k in enumerate(before[0])}
    n = 0
    for i, k in enumerate(ka):
        j = row.get(tuple(k))
        n += int((xa[i] != (before[1][j].view(np.uint32) if j is not None else DEFAULT)).any(axis=-1).sum())
    return n


def _oracle_run(oracle, shape, truncs, cuts):
    """The oracle's volume over the N frames, computed once and read-only.  truncs: the truncation of each frame (a change of truncation moves the
    voxels into a volume created with the new one -- the oracle has no setter); cuts: the frame counts after which the state is kept (the launch
    boundaries of the tests).  Returns keys, voxels, blocks selected and voxels updated per frame, {n: (keys, voxels)}."""
    key = ("oracle", shape, tuple(truncs), tuple(cuts))
    if key not in _cache:
        d, c, poses = _frames(shape)
        cam = oracle.make_camera(*CAMS[shape])
        ov = oracle.Volume(cam, voxel_res=RES, trunc=truncs[0])
        sel, upd, snaps = [], [], {}
        for k in range(N):
            if k and truncs[k] != truncs[k - 1]:
                state = ov.export(sort=False)
                ov = oracle.Volume(cam, voxel_res=RES, trunc=truncs[k])
                ov.load(*state)
            n, _vis, nu = ov.integrate(d[k], c[k], poses[k])
            sel.append(n); upd.append(nu)
            if k + 1 in cuts:
                snaps[k + 1] = ov.export()
        for s in snaps.values():
            s[1].setflags(write=False)
        _cache[key] = (snaps[N][0], snaps[N][1], sel, upd, snaps)
    return _cache[key]


def _written(snaps, cuts):
    """voxels_written of launches that end after cuts[0] < cuts[1] < ... frames, from the empty volume."""
    total, prev = 0, None
    for n in cuts:
        total += _changed(prev, snaps[n])
        prev = snaps[n]
    return total


def _handler(shape, trunc, max_blocks=1 << 14):
    hcam = I.PinholeCamera()
    hcam.fx, hcam.fy, hcam.cx, hcam.cy, hcam.width, hcam.height, hcam.depth_scale = CAMS[shape]
    hv = I.CubeHandler(hcam, device=0, max_blocks=max_blocks)
    hv.SetVoxelResolution(RES)
    hv.SetTruncation(trunc)
    return hv


def _equal(hv, ok, ox):
    hk, hx = hv.GetCubeMap()
    assert hk.shape == ok.shape and np.array_equal(hk, ok), "block keys differ"
    assert np.array_equal(hx.view(np.uint32), ox.view(np.uint32)), "voxels differ"


def _cuts(n):
    return tuple(range(32, n, 32)) + (n,)


@pytest.mark.parametrize("trunc", [0.1, 0.6])
@pytest.mark.parametrize("n", [33, 70])
@pytest.mark.parametrize("shape", list(CAMS))
def test_sequence_and_both_counters_equal_the_oracle(oracle, shape, n, trunc):
    cuts = _cuts(n)                                         # 33: launches of 32 + 1 frames; 70: 32 + 32 + 6
    _k, _x, sel, upd, snaps = _oracle_run(oracle, shape, (trunc,) * N, (32, 33, 64, 70))
    ok, ox = snaps[n]
    assert 100 < len(ok) < 4000 and sum(upd[:n]) > 50000
    depth, rgb = _device(shape)
    hv = _handler(shape, trunc)
    hv.IntegrateSequence(depth[:n], rgb[:n], _frames(shape)[2][:n])
    st = hv.Stats()                                         # (flushes the last, short batch)
    written = _written(snaps, cuts)
    print("%s, %d frames, trunc %.9g: %d blocks, updated %d (oracle %d), written %d (oracle %d), launches %d"
          % (shape, n, trunc, len(ok), st["voxels_updated"], sum(upd[:n]), st["voxels_written"], written, st["launches"]))
    assert st["frames"] == n and st["launches"] == len(cuts)
    assert st["blocks_selected"] == sum(sel[:n])
    assert st["voxels_updated"] == sum(upd[:n])
    assert st["voxels_written"] == written
    _equal(hv, ok, ox)


@pytest.mark.parametrize("shape", list(CAMS))
def test_truncation_switched_between_batches(oracle, shape):
    """0.1 for 32 frames (lean), 0.6 for 32 (plain: the first truncation above 0.5 ends the lean form for good), 0.1 for 6 (plain): three launches,
    three instantiations' worth of counters in one pair of totals."""
    truncs = (0.1,) * 32 + (0.6,) * 32 + (0.1,) * 6
    ok, ox, sel, upd, snaps = _oracle_run(oracle, shape, truncs, (32, 64, 70))
    depth, rgb = _device(shape)
    poses = _frames(shape)[2]
    hv = _handler(shape, 0.1)
    hv.IntegrateSequence(depth[:32], rgb[:32], poses[:32])
    hv.Flush()
    hv.SetTruncation(0.6)
    hv.IntegrateSequence(depth[32:64], rgb[32:64], poses[32:64])
    hv.Flush()
    hv.SetTruncation(0.1)
    hv.IntegrateSequence(depth[64:], rgb[64:], poses[64:])
    st = hv.Stats()
    assert st["frames"] == N and st["launches"] == 3
    assert st["voxels_updated"] == sum(upd)
    assert st["voxels_written"] == _written(snaps, (32, 64, 70))
    _equal(hv, ok, ox)


def test_a_volume_that_is_not_plain(oracle):
    """Download, upload (the volume is no longer the kernel's own: its blocks take the general update, blocks allocated later the one with the
    select), fuse the rest in launches of 32 + 28 frames."""
    shape, trunc = "64x48", 0.1
    ok, ox, _sel, upd, snaps = _oracle_run(oracle, shape, (trunc,) * N, (10, 42, 70))
    depth, rgb = _device(shape)
    poses = _frames(shape)[2]
    hv = _handler(shape, trunc)
    hv.IntegrateSequence(depth[:10], rgb[:10], poses[:10])
    k, v = hv.GetCubeMap()
    assert np.array_equal(k, snaps[10][0]) and np.array_equal(v.view(np.uint32), snaps[10][1].view(np.uint32))
    hv.SetCubeMap(k, v)
    n_before = hv.BlockCount()
    hv.IntegrateSequence(depth[10:], rgb[10:], poses[10:])
    assert hv.BlockCount() > n_before                      # both kinds of block in the second part
    _equal(hv, ok, ox)
    st = hv.Stats()                                        # (SetCubeMap replaces the map and starts the statistics again)
    assert st["frames"] == N - 10 and st["launches"] == 2
    assert st["voxels_updated"] == sum(upd[10:])
    assert st["voxels_written"] == _changed(snaps[10], snaps[42]) + _changed(snaps[42], snaps[70])


def test_with_the_raycasters_summaries_present(oracle):
    """One view before fusing: k_integrate then restates the summaries of the blocks it changes from the voxels it holds."""
    shape, trunc = "64x48", 0.1
    ok, ox, _sel, upd, snaps = _oracle_run(oracle, shape, (trunc,) * N, (1, 33, 65, 70))
    depth, rgb = _device(shape)
    poses = _frames(shape)[2]
    view = S.room_pose(400)
    hv = _handler(shape, trunc)
    hv.IntegrateSequence(depth[:1], rgb[:1], poses[:1])
    hv.Raycast(view)
    hv.IntegrateSequence(depth[1:], rgb[1:], poses[1:])    # 32 + 32 + 5 frames
    _equal(hv, ok, ox)
    st = hv.Stats()
    assert st["launches"] == 4 and st["voxels_updated"] == sum(upd)
    assert st["voxels_written"] == _written(snaps, (1, 33, 65, 70))
    with_sum = hv.Raycast(view)
    hv.SetRaycastPrune(False)
    without = hv.Raycast(view)
    assert with_sum[0].any() and with_sum[0].tobytes() == without[0].tobytes()
    ov = oracle.Volume(oracle.make_camera(*CAMS[shape]), voxel_res=RES, trunc=trunc)
    ov.load(ok, ox)
    assert np.array_equal(with_sum[0].view(np.uint32), ov.raycast(view)[0].view(np.uint32))


def test_a_small_pool_grows_and_clear_starts_again(oracle):
    """A pool of 64 blocks: the batch that exhausts it is poisoned on the device (nothing fused, nothing counted), the host grows the pool and
    replays it.  Then Clear() and the same sequence again: the volume and the statistics start from nothing, the lean form with them."""
    shape, trunc = "64x48", 0.1
    ok, ox, sel, upd, snaps = _oracle_run(oracle, shape, (trunc,) * N, (32, 33, 64, 70))
    assert len(ok) > 4 * 64
    depth, rgb = _device(shape)
    poses = _frames(shape)[2]
    hv = _handler(shape, trunc, max_blocks=64)
    for rnd in range(2):
        hv.IntegrateSequence(depth, rgb, poses)
        st = hv.Stats()
        print("round %d: %s, growth %s" % (rnd, st, hv.GrowthStats()))
        _equal(hv, ok, ox)
        assert st["frames"] == N and st["blocks_selected"] == sum(sel)
        assert st["voxels_updated"] == sum(upd)
        assert st["voxels_written"] == _written(snaps, (32, 64, 70))
        hv.Clear()
        assert hv.BlockCount() == 0


def _coverage(oracle, shape):
    """Per launch of the 33- and 70-frame sequences, counted on the host from the oracle frame by frame: blocks the launch selected, those of them
    none of whose voxels any of its frames updated, and (full launches) blocks that all 32 frames updated."""
    key = ("coverage", shape)
    if key not in _cache:
        d, c, poses = _frames(shape)
        ov = oracle.Volume(oracle.make_camera(*CAMS[shape]), voxel_res=RES, trunc=0.1)
        selected, hit, before = [], [], {}
        for k in range(N):
            ids, _nc = ov.prepare_cubes(d[k], poses[k])
            selected.append(set(map(tuple, ids)))
            ov.integrate(d[k], c[k], poses[k])
            keys, vox = ov.export(sort=False)
            wsum = vox[..., 1].astype(np.float64).sum(axis=1)      # (truncation 0.1: every update adds 1 to a weight)
            now = dict(zip(map(tuple, keys), wsum))
            hit.append({key for key, w in now.items() if w != before.get(key, 0.0)})
            before = now
        out = []
        for lo, hi in ((0, 32), (32, 33), (32, 64), (64, 70)):
            sel = set().union(*selected[lo:hi])
            out.append((len(sel), len(sel - set().union(*hit[lo:hi])), len(set.intersection(*hit[lo:hi])) if hi - lo == 32 else 0))
        _cache[key] = out
    return _cache[key]


@pytest.mark.parametrize("shape", list(CAMS))
def test_blocks_hit_by_no_frame_and_by_every_frame_of_a_batch(oracle, shape):
    """Both ends of what the weight difference has to count.  A block that all 32 frames of a launch select and update is in the sequences above.
    A block that a launch selects and none of whose voxels any of its frames updates is not, and cannot be: PrepareCubes (CubeHandler.cpp:171-181)
    selects a block exactly when one of its eight corner voxels passes the band test of IntegrateImage, so the frame that selects a block hits it.
    A caller's cube list (IntegrateCubes) has no such tie: a listed block that nothing projects into is allocated, loaded, finds every difference
    0, stores nothing and counts nothing."""
    cov = _coverage(oracle, shape)
    print(shape, "per launch (selected, never hit, hit by all 32):", cov)
    assert all(never == 0 for _sel, never, _all in cov)
    assert cov[0][2] > 0 and cov[2][2] > 0
    _k, _x, sel, upd, snaps = _oracle_run(oracle, shape, (0.1,) * N, (1, 33, 65, 70))
    d, c, poses = _frames(shape)
    hv = _handler(shape, 0.1)
    ids = hv.PrepareCubes(d[0], poses[0])                  # allocates the selection, fuses nothing
    far = np.array([[900, 900, 900], [-900, 5, 7]], np.int32)
    hv.IntegrateCubes(d[0], c[0], poses[0], np.concatenate([far[:1], ids, far[1:]]))
    st = hv.Stats()
    assert st["launches"] == 1 and st["voxels_updated"] == upd[0] and st["voxels_written"] == upd[0] == _changed(None, snaps[1])
    hk, hx = hv.GetCubeMap()
    mine = ~((hk[:, None, :] == far[None]).all(-1).any(1))
    assert (~mine).sum() == 2 and np.array_equal(hx[~mine].view(np.uint32), np.broadcast_to(DEFAULT, (2, 512, 5)))
    assert np.array_equal(hk[mine], snaps[1][0]) and np.array_equal(hx[mine].view(np.uint32), snaps[1][1].view(np.uint32))
