"""k_integrate's certified projection without the window test on Z (csrc/integrate.hip, volume_core.hpp project_pixel_uv<true, false>,
zwin_cert.hpp), on the device.

The certified kinds of k_integrate no longer test 2^-60 <= |Z| < 2^60 per lane: the host proves |Z| < 2^59 for every frame of a launch
(zwin_certified_batch in launch_integrate; a batch it refuses takes the exact projection), and a small, zero or denormal Z is either inside the
certificate's hypotheses or refused by the certificate itself because v_rcp_f32 returns +-inf for it -- the last test measures that.

37 x 29 pixels, 8 cm voxels, 33 frames per case (a launch of 32 and a launch of one), truncations 0.1 and 0.6.  Every case compares block keys, every
voxel bit for bit, voxels_updated and voxels_written with the expected volume, requires voxels_updated > 0 of the expected volume itself, and reads
which form the launches took from op_debug_volume_gather_kinds:
  (a) room poses: certified;
  (b) pure translations whose camera plane passes exactly through a plane of voxel centres (M[11] = minus a voxel centre's z, so Z == 0 there; the
      images hold depths below the truncation, so that the planes next to it are hit): certified;
  (c) inverse poses scaled by 2^-70 .. 2^-77 (row 2 = (2^-70, 0, 0, 0) and the like; rows 0 and 1 scaled with it, so that the quotients are those of
      an ordinary camera): every Z lies in about [2^-82, 2^-69], far below the former window: certified;
  (d) the same scaled by a further 2^-60: every Z is denormal or zero: certified (the host's bound has no lower side), every lane refused on the
      device by the reciprocal;
  (e) one frame of the full launch has an inverse pose with row 2 = 2^70 (1, 1, 1, 1): the host refuses the certificate and the launch takes the
      exact projection; the launch of one ordinary frame stays certified;
  (f) a volume that is not plain, the sum form by its own bar (weights equal, sdf within 1e-4 of the truncation, colour within 1e-4) and a signed
      launch (frames 10 .. 20 de-integrated in one launch with the 33rd frame), each with the poses of (a) and of (c).

Expected volumes.  (a), (b): the oracle's Volume.integrate.  The oracle derives the inverse from the pose, and no float32 pose has an inverse like
(c)'s, (d)'s or (e)'s (its determinant is 2^210 and beyond), so those frames are given to the device with an explicit pose_inv, and their expected
volume is put together from the oracle's own functions -- orc_compute_bounding and orc_cube_id for the candidates, orc_get_sdf (the oracle's
projection, pixel rounding and depth lookup for a SUPPLIED inverse) for the corner test and for every voxel -- with TSDFVoxel::operator+ in numpy
float32 (`Restated`).  The first test holds Restated to Volume.integrate on all 33 room frames: counts frame by frame, three snapshots bit for bit."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import deintegrate_common as D
from onepiece_amd import integration as I, synthetic as S

F32 = np.float32
CAM = (30.0, 30.0, 18.25, 14.25, 37, 29, 1000.0)
W, H = CAM[4], CAM[5]
RES = 0.08
N = 33
CUTS = (32, 33)
NEAR, FAR = 0.5, 5.0
DEFAULT = np.array([999, 0, -1, -1, -1], F32).view(np.uint32)
EXACT, FAST_RAW, FAST_2D = 0, 1, 2
_cache = {}


# ---- the expected volume for frames with a supplied inverse pose ---------------------------------------------------------------------------
class Restated:
    """CubeHandler::IntegrateImage (CubeHandler.cpp:147-210, Integrator.cpp:36-94) with the inverse pose SUPPLIED: the oracle's functions for
    everything that touches the pose, the image and the rounding; the candidate loop and TSDFVoxel::operator+ (TSDFVoxel.h:24-39) in float32."""
    IDX = 2.0 ** 28      # the index image holds (pixel + 1) * 2^28: fl(that - Z) is the value itself for |Z| < 16, so the pixel comes back exactly

    def __init__(self, O, trunc, near=NEAR, far=FAR):
        self.O, self.L, self.trunc, self.near, self.far = O, O.lib(), F32(trunc), near, far
        self.cam = O.make_camera(*CAM)
        self.blocks = {}                                      # key -> [512, 5] float32
        res, half = F32(RES), F32(RES) / F32(2)
        x = np.arange(8, dtype=F32) * res + half              # VoxelCentroidOffSet (VoxelCube.h:48-61)
        v = np.arange(512)
        self.off = np.stack([x[v & 7], x[(v >> 3) & 7], x[v >> 6]], axis=1).astype(F32)
        self.corners = (0, 7, 56, 63, 448, 455, 504, 511)      # CubeHandler.cpp:158-162
        self.cube_res = res * F32(8)
        self.idx_img = ((np.arange(W * H) + 1) * self.IDX).astype(F32)
        self.fp = C.POINTER(C.c_float)
        self.p, self.cam_ref = (C.c_float * 3)(), C.byref(self.cam)

    def _sdf(self, x, y, z, inv, img):
        """orc_get_sdf at the point (x, y, z) (Python floats holding float32 values); inv and img are prepared pointers"""
        self.p[0], self.p[1], self.p[2] = x, y, z
        return self.L.orc_get_sdf(self.cam_ref, self.p, inv, img, 0)

    def select(self, depth, pose, inv):
        mx, mn, inside = self.O.compute_bounding(self.cam, depth, pose, self.far, self.near)
        if inside == 0:
            return []
        lo, hi = (C.c_int * 3)(), (C.c_int * 3)()
        self.L.orc_cube_id(F32(RES), mx.ctypes.data_as(self.fp), hi)
        self.L.orc_cube_id(F32(RES), mn.ctypes.data_as(self.fp), lo)
        inv_p, img_p, trunc = inv.ctypes.data_as(self.fp), depth.ctypes.data, float(self.trunc)
        corner = self.off[list(self.corners)]
        out = []
        for i in range(lo[0] - 1, hi[0] + 2):
            for j in range(lo[1] - 1, hi[1] + 2):
                for k in range(lo[2] - 1, hi[2] + 2):
                    pts = (np.array([i, j, k], F32) * self.cube_res + corner).astype(F32).tolist()   # CubeHandler.cpp:166-170
                    if min(abs(self._sdf(x, y, z, inv_p, img_p)) for x, y, z in pts) < trunc:
                        out.append((i, j, k))
        return out

    def integrate(self, depth, rgb, pose, pose_inv):
        """-> (blocks selected, voxels updated)"""
        depth = np.ascontiguousarray(depth, F32)
        pose = np.ascontiguousarray(pose, F32).reshape(16)
        inv = np.ascontiguousarray(pose_inv, F32).reshape(16)
        col = (np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3).astype(F32) / F32(255.0)).astype(F32)
        sel = self.select(depth, pose, inv)
        inv_p, img_p, idx_p, trunc = inv.ctypes.data_as(self.fp), depth.ctypes.data, self.idx_img.ctypes.data, float(self.trunc)
        updated = 0
        for key in sel:
            vox = self.blocks.setdefault(key, np.tile(np.array([999, 0, -1, -1, -1], F32), (512, 1)))
            start = (np.array(key, F32) * F32(8.0)) * F32(RES)   # VoxelCube.h:75-80
            pts = (start + self.off).astype(F32).tolist()
            vids, news, pix = [], [], []
            for vid, (x, y, z) in enumerate(pts):
                new = self._sdf(x, y, z, inv_p, img_p)            # (a C float: the comparison in double is the float comparison)
                if abs(new) < trunc:                              # (999: off the image or no depth)
                    vids.append(vid); news.append(new); pix.append(self._sdf(x, y, z, inv_p, idx_p) / self.IDX)
            if not vids:
                continue
            vids, new, pix = np.array(vids), np.array(news, F32), np.array(pix)
            assert np.all(pix == np.floor(pix)) and pix.min() >= 1 and pix.max() <= W * H
            c = col[pix.astype(np.int64) - 1]
            # TSDFVoxel::operator+ with other = (new, 1, c) (TSDFVoxel.h:24-39): every product, sum and quotient one float32 operation
            s, w, cc = vox[vids, 0], vox[vids, 1], vox[vids, 2:]
            valid = ~((s >= 1) | (w <= 0))                        # TSDFVoxel::IsValid (TSDFVoxel.h:75-78)
            wsum = np.where(valid, w + F32(1.0), F32(1.0)).astype(F32)
            s2 = ((w * s).astype(F32) + (F32(1.0) * new).astype(F32)).astype(F32) / wsum
            c2 = ((w[:, None] * cc).astype(F32) + (F32(1.0) * c).astype(F32)).astype(F32) / wsum[:, None]
            vox[vids, 0] = np.where(valid, s2, new)
            vox[vids, 1] = wsum
            vox[vids, 2:] = np.where(valid[:, None], c2, c)
            updated += len(vids)
        return len(sel), updated

    def export(self):
        keys = np.array(sorted(self.blocks), np.int32).reshape(-1, 3)
        vox = np.stack([self.blocks[tuple(k)] for k in keys.tolist()]) if len(keys) else np.zeros((0, 512, 5), F32)
        return keys, vox.astype(F32)

    def load(self, keys, vox):
        self.blocks = {tuple(k): np.array(v, F32) for k, v in zip(np.asarray(keys).tolist(), vox)}


def _inv4(m12):
    return np.concatenate([np.asarray(m12, F32).reshape(12), np.array([0, 0, 0, 1], F32)])


# ---- frames --------------------------------------------------------------------------------------------------------------------------------
def _room():
    if "room" not in _cache:
        poses = np.stack([S.room_pose(300 + 3 * k) for k in range(N)]).astype(F32)
        fr = [S.room_render(p, width=W, height=H, fx=CAM[0], fy=CAM[1], cx=CAM[2], cy=CAM[3]) for p in poses]
        _cache["room"] = [(np.ascontiguousarray(d, F32), np.ascontiguousarray(c, np.uint8), p) for (d, c), p in zip(fr, poses)]
    return _cache["room"]


def _patchwork(k, values):
    """An image of 3 x 3 pixel patches holding `values` by turns, shifted from frame to frame; colours from the position."""
    i, j = np.mgrid[0:H, 0:W]
    d = np.asarray(values, F32)[(i // 3 + 2 * (j // 3) + k) % len(values)]
    rgb = np.stack([(7 * i + k) % 256, (11 * j + 3 * k) % 256, (5 * (i + j)) % 256], axis=-1).astype(np.uint8)
    return np.ascontiguousarray(d, F32), np.ascontiguousarray(rgb)


def _centre(block, voxel):
    """The float32 coordinate of a voxel centre as the kernel and the reference form it."""
    return (F32(block) * F32(8.0)) * F32(RES) + (F32(voxel) * F32(RES) + F32(RES) / F32(2))


def _plane_frames():
    """(b): the camera looks along +z from a voxel centre: X == Y == Z == 0 for that voxel, Z == 0 for its whole plane of centres.  Depths of 5, 12,
    21 and 33 cm reach the next planes (8, 16, 24 ... cm) within either truncation; 1.2 and 2 m lie inside the frustum and give the bounding box."""
    out = []
    for k in range(N):
        t = np.array([_centre(k % 3 - 1, (2 * k) % 8), _centre(k % 2, (3 * k) % 8), _centre(-(k % 4), (5 * k) % 8)], F32)
        pose = np.eye(4, dtype=F32)
        pose[:3, 3] = t
        d, c = _patchwork(k, (0.05, 1.2, 0.12, 2.0, 0.21, 0.33))
        out.append((d, c, pose))
    return out


def _scaled_frames(extra):
    """(c), (d): a camera at (tx, ty) looking along +x, its inverse pose scaled by e = 2^-(70 + k % 8 + extra): Z = e * px.  The forward pose (bounding
    box and frustum only) is the same camera unscaled.  Depths below the truncations hit whatever projects onto them (sdf = d - Z = d to the last bit);
    0.7 m lies inside the frustum and gives the bounding box."""
    out = []
    for k in range(N):
        ty, tz = F32(0.1 + 0.02 * (k % 5)), F32(-0.07 + 0.03 * (k % 3))
        fwd = np.array([[0, 0, 1, 0], [1, 0, 0, ty], [0, 1, 0, tz], [0, 0, 0, 1]], F32)
        e = F32(2.0 ** -(70 + k % 8 + extra))
        inv = np.array([[0, e, 0, -ty * e], [0, 0, e, -tz * e], [e, 0, 0, 0]], F32)
        d, c = _patchwork(k, (0.03, 0.7, 0.08, 0.3, 0.0))
        out.append((d, c, fwd, _inv4(inv)))
    return out


def _with_inverse(O, frames):
    return [(d, c, p, O.mat4_inverse(p).astype(F32).reshape(16)) for d, c, p in frames]


# ---- expected volumes (computed once, read-only) -------------------------------------------------------------------------------------------
def _changed(before, after):
    ka, xa = after
    xa = xa.view(np.uint32)
    row = {} if before is None else {tuple(k): i for i, k in enumerate(before[0].tolist())}
    n = 0
    for i, k in enumerate(ka.tolist()):
        j = row.get(tuple(k))
        n += int((xa[i] != (before[1][j].view(np.uint32) if j is not None else DEFAULT)).any(axis=-1).sum())
    return n


def _expectation(snaps, sel, upd):
    """snaps: the volume after 10, 32 and 33 frames; sel, upd: blocks selected and voxels updated per frame.  voxels_written counts, per launch, the
    voxels the launch stored: the voxels whose bits differ before and after the launch's frames (an update always changes the weight)."""
    for s in snaps.values():
        s[1].setflags(write=False)
    return {"snaps": snaps, "selected": sum(sel), "updated": sum(upd), "sel": tuple(sel), "upd": tuple(upd),
            "written": _changed(None, snaps[32]) + _changed(snaps[32], snaps[33])}


def _expect_oracle(O, name, frames, trunc, near=NEAR):
    key = ("oracle", name, trunc)
    if key not in _cache:
        ov = O.Volume(O.make_camera(*CAM), voxel_res=RES, trunc=trunc, far=FAR, near=near)
        sel, upd, snaps = [], [], {}
        for k, (d, c, p) in enumerate(frames):
            n, _v, nu = ov.integrate(d, c, p)
            sel.append(n); upd.append(nu)
            if k + 1 in (10,) + CUTS:
                snaps[k + 1] = ov.export()
        _cache[key] = _expectation(snaps, sel, upd)
    return _cache[key]


def _expect_restated(O, name, frames, trunc):
    key = ("restated", name, trunc)
    if key not in _cache:
        m = Restated(O, trunc)
        sel, upd, snaps = [], [], {}
        for k, (d, c, p, inv) in enumerate(frames):
            n, nu = m.integrate(d, c, p, inv)
            sel.append(n); upd.append(nu)
            if k + 1 in (10,) + CUTS:
                snaps[k + 1] = m.export()
        _cache[key] = _expectation(snaps, sel, upd)
    return _cache[key]


# ---- the device ----------------------------------------------------------------------------------------------------------------------------
def _handler(trunc, near=NEAR):
    hcam = I.PinholeCamera()
    hcam.fx, hcam.fy, hcam.cx, hcam.cy, hcam.width, hcam.height, hcam.depth_scale = CAM
    hv = I.CubeHandler(hcam, device=0, max_blocks=1 << 13)
    hv.SetVoxelResolution(RES)
    hv.SetTruncation(trunc)
    if near != NEAR:
        hv.SetNearPlane(near)
    return hv


def _fuse(hv, frames):
    for f in frames:
        hv.IntegrateImage(f[0], f[1], f[2], f[3] if len(f) > 3 else None)


def _kinds(hv):
    out = (C.c_ulonglong * 3)()
    from onepiece_amd import _lib as L
    L.check(hv._lib.op_debug_volume_gather_kinds(hv._h, out))
    return list(out)


def _equal(hv, ok, ox):
    hk, hx = hv.GetCubeMap()
    assert hk.shape == ok.shape and np.array_equal(hk, ok), "block keys differ"
    diff = (hx.view(np.uint32) != ox.view(np.uint32)).any(axis=-1)
    assert not diff.any(), "%d voxels differ, the first at (block, in-plane index) %s" % (int(diff.sum()), np.argwhere(diff)[0])


def _check_case(name, hv, frames, exp, kinds):
    ok, ox = exp["snaps"][N]
    assert exp["updated"] > 0 and len(ok) >= 10               # the expected volume itself: something was fused, into tens of blocks
    _fuse(hv, frames)
    st = hv.Stats()
    print("%s: %d blocks, selected %d, updated %d (expected %d), written %d (expected %d), launches by kind %s"
          % (name, len(ok), st["blocks_selected"], st["voxels_updated"], exp["updated"], st["voxels_written"], exp["written"], _kinds(hv)))
    assert st["frames"] == N and st["launches"] == 2 and st["blocks_selected"] == exp["selected"]
    assert st["voxels_updated"] == exp["updated"]
    assert st["voxels_written"] == exp["written"]
    _equal(hv, ok, ox)
    assert _kinds(hv) == kinds


@pytest.mark.parametrize("trunc", [0.1, 0.6])
def test_restated_integration_equals_the_oracles_on_room_frames(oracle, trunc):
    """What (c), (d) and (e) are compared with, held to Volume.integrate where both exist: all 33 room frames -- blocks selected and voxels updated
    frame by frame, keys and every voxel bit for bit after 10, 32 and 33 frames, voxels_written of the two launches."""
    room = _room()
    a = _expect_oracle(oracle, "room", room, trunc)
    b = _expect_restated(oracle, "room", _with_inverse(oracle, room), trunc)
    assert a["sel"] == b["sel"] and a["upd"] == b["upd"] and min(a["upd"]) > 0
    for n in (10,) + CUTS:
        (ok, ox), (mk, mx) = a["snaps"][n], b["snaps"][n]
        assert np.array_equal(ok, mk) and np.array_equal(ox.view(np.uint32), mx.view(np.uint32)), n
    assert a["written"] == b["written"]


@pytest.mark.parametrize("trunc", [0.1, 0.6])
def test_a_room_poses_are_certified(oracle, trunc):
    _check_case("(a) trunc %g" % trunc, _handler(trunc), _room(), _expect_oracle(oracle, "room", _room(), trunc), [0, 0, 2])


@pytest.mark.parametrize("trunc", [0.1, 0.6])
def test_b_camera_plane_through_a_plane_of_voxel_centres(oracle, trunc):
    frames = _plane_frames()
    for d, c, p in frames:                                    # the inverse is the exact one, and Z vanishes on the camera's own plane of centres
        inv = oracle.mat4_inverse(p).astype(F32)
        assert np.array_equal(inv[:3, :3], np.eye(3, dtype=F32)) and np.array_equal(inv[:3, 3], -p[:3, 3])
        assert F32(p[2, 3]) + inv[2, 3] * F32(1.0) == 0
    exp = _expect_oracle(oracle, "plane", frames, trunc, near=0.01)
    keys = exp["snaps"][N][0]
    for k in (0, 1, 5, 32):                                   # the block that holds the camera's voxel is among the fused ones: lanes with Z == 0 ran
        blk = [-1 + k % 3, k % 2, -(k % 4)]
        assert (keys == np.array(blk, np.int32)).all(axis=1).any(), (k, blk)
    _check_case("(b) trunc %g" % trunc, _handler(trunc, near=0.01), frames, exp, [0, 0, 2])


@pytest.mark.parametrize("trunc", [0.1, 0.6])
def test_c_depths_far_below_the_former_window(oracle, trunc):
    frames = _scaled_frames(0)
    assert max(abs(f[3][8]) for f in frames) == 2.0 ** -70 and all(f[3][9] == f[3][10] == f[3][11] == 0 for f in frames)
    _check_case("(c) trunc %g" % trunc, _handler(trunc), frames, _expect_restated(oracle, "scaled0", frames, trunc), [0, 0, 2])


@pytest.mark.parametrize("trunc", [0.1, 0.6])
def test_d_denormal_and_zero_depths(oracle, trunc):
    frames = _scaled_frames(60)
    assert max(abs(f[3][8]) for f in frames) == 2.0 ** -130    # times a coordinate of at most a few metres: below 2^-126
    _check_case("(d) trunc %g" % trunc, _handler(trunc), frames, _expect_restated(oracle, "scaled60", frames, trunc), [0, 0, 2])


@pytest.mark.parametrize("trunc", [0.1, 0.6])
def test_e_a_frame_the_host_refuses_sends_its_launch_to_the_exact_projection(oracle, trunc):
    """Frame 5 keeps its pose for the bounding box but gets an inverse whose row 2 is 2^70 (1, 1, 1, 1): finite, |Z| up to 2^72.  Nothing of that
    frame can be in band (the restated selection is empty), so the expected volume is the oracle's over the other 32 frames."""
    room = _room()
    bad = 5
    absurd = oracle.mat4_inverse(room[bad][2]).astype(F32).reshape(16)
    absurd[8:12] = 2.0 ** 70
    assert Restated(oracle, trunc).select(room[bad][0], np.ascontiguousarray(room[bad][2], F32).reshape(16), absurd) == []
    rest = room[:bad] + room[bad + 1:]
    key = ("oracle-e", trunc)
    if key not in _cache:
        ov = oracle.Volume(oracle.make_camera(*CAM), voxel_res=RES, trunc=trunc, far=FAR, near=NEAR)
        sel = upd = 0
        for k, (d, c, p) in enumerate(rest):
            n, _v, nu = ov.integrate(d, c, p)
            sel += n; upd += nu
            if k == 30:
                s32 = ov.export()                              # after the device's first launch: 31 ordinary frames and the absurd one
        s33 = ov.export()
        _cache[key] = {"snaps": {N: s33}, "selected": sel, "updated": upd, "written": _changed(None, s32) + _changed(s32, s33)}
    frames = [f if k != bad else (f[0], f[1], f[2], absurd) for k, f in enumerate(room)]
    _check_case("(e) trunc %g" % trunc, _handler(trunc), frames, _cache[key], [1, 0, 1])


# ---- (f): the other update forms -----------------------------------------------------------------------------------------------------------
def _family(oracle, which, trunc):
    if which == "room":
        return _room(), _expect_oracle(oracle, "room", _room(), trunc)
    frames = _scaled_frames(0)
    return frames, _expect_restated(oracle, "scaled0", frames, trunc)


@pytest.mark.parametrize("trunc", [0.1, 0.6])
@pytest.mark.parametrize("which", ["room", "scaled"])
def test_f_a_volume_that_is_not_plain(oracle, which, trunc):
    frames, exp = _family(oracle, which, trunc)
    assert exp["updated"] > 0
    hv = _handler(trunc)
    _fuse(hv, frames[:10])
    k, v = hv.GetCubeMap()
    assert np.array_equal(k, exp["snaps"][10][0]) and np.array_equal(v.view(np.uint32), exp["snaps"][10][1].view(np.uint32))
    hv.SetCubeMap(k, v)
    _fuse(hv, frames[10:])
    st = hv.Stats()                                            # (SetCubeMap starts the statistics again)
    assert st["frames"] == N - 10 and st["launches"] == 1 and st["blocks_selected"] == sum(exp["sel"][10:])
    assert st["voxels_updated"] == sum(exp["upd"][10:]) > 0
    assert st["voxels_written"] == _changed(exp["snaps"][10], exp["snaps"][N])
    _equal(hv, *exp["snaps"][N])
    assert _kinds(hv) == [0, 0, 2]


@pytest.mark.parametrize("trunc", [0.1, 0.6])
@pytest.mark.parametrize("which", ["room", "scaled"])
def test_f_sum_form_by_its_own_bar(oracle, which, trunc):
    """OP_VOLUME_UPDATE_SUM_FORM: the same blocks, counts and (integer) weights, voxel by voxel; sdf within 1e-4 of the truncation and colour within
    1e-4 of the running mean (the sum form's own bar, tests/test_kc_lanes_gpu.py); unobserved voxels untouched."""
    frames, exp = _family(oracle, which, trunc)
    ok, ox = exp["snaps"][N]
    assert exp["updated"] > 0
    hv = _handler(trunc)
    hv.SetUpdateMode("sum_form")
    _fuse(hv, frames)
    st = hv.Stats()
    assert st["frames"] == N and st["launches"] == 2 and st["blocks_selected"] == exp["selected"] and st["voxels_updated"] == exp["updated"]
    assert st["voxels_written"] == exp["written"]             # a voxel is stored when the launch observed it at least once: its weight changes in the exact form too
    hk, hx = hv.GetCubeMap()
    assert np.array_equal(hk, ok) and np.array_equal(hx[..., 1], ox[..., 1])
    seen = ox[..., 1] > 0
    e_sdf = np.abs(hx[..., 0].astype(np.float64) - ox[..., 0])[seen].max() / trunc
    e_col = np.abs(hx[..., 2:].astype(np.float64) - ox[..., 2:])[seen].max()
    print("%s sum form, trunc %g: sdf off by %.3g of the truncation, colour by %.3g" % (which, trunc, e_sdf, e_col))
    assert e_sdf <= 1e-4 and e_col <= 1e-4
    assert np.array_equal(hx[~seen].view(np.uint32), ox[~seen].view(np.uint32))
    assert _kinds(hv) == [0, 0, 2]


class _RestatedModel(D.Model):
    """tests/deintegrate_common.py's model with Restated in the oracle volume's place (frames carry their inverse pose)."""

    def __init__(self, O, trunc):
        self.O, self.trunc = O, trunc
        self.vol = Restated(O, trunc)
        self.counts = {"frames": 0, "reverted": 0, "reset": 0, "skipped": 0}
        self.updated = self.entries = self.selected = 0
        self.last = None

    def observation(self, frame):
        alone = Restated(self.O, self.trunc)
        alone.integrate(*frame)
        return alone.export()

    def integrate(self, frame):
        n, nu = self.vol.integrate(*frame)
        self.updated += nu; self.entries += 1; self.selected += n
        return self


@pytest.mark.parametrize("trunc", [0.1, 0.6])
@pytest.mark.parametrize("which", ["room", "scaled"])
def test_f_a_signed_launch(oracle, which, trunc):
    """33 frames fused, frames 10 .. 20 de-integrated: the 33rd frame and the eleven de-integrations share one signed launch.  Expected volume and
    counters as in tests/test_kc_lanes_gpu.py (tests/deintegrate_common.py: the definition's four steps in numpy on the frame fused alone)."""
    key = ("signed", which, trunc)
    frames = _room() if which == "room" else _scaled_frames(0)
    if key not in _cache:
        m = D.Model(oracle, CAM, trunc, res=RES) if which == "room" else _RestatedModel(oracle, trunc)
        for f in frames[:32]:
            m.integrate(f)
        written = _changed(None, m.export())                  # the launch of 32 fused frames
        # The signed launch stores every voxel that its fused entry hits or that a de-integration is applied to (step 1 of the definition), once:
        # the union over its twelve entries, whether or not the bits end up different.
        touched = set()
        bk, bv = m.observation(frames[32])
        touched.update((tuple(k), int(v)) for k, blk in zip(bk.tolist(), bv) for v in np.flatnonzero(blk[:, 1] == 1))
        m.integrate(frames[32])
        for f in frames[10:21]:
            bk, bv = m.observation(f)
            k, v = m.export()
            row = {tuple(q): i for i, q in enumerate(k.tolist())}
            for q, blk in zip(bk.tolist(), bv):
                if tuple(q) in row:                           # (a block the volume does not hold yet is allocated with default voxels: nothing to revert)
                    cur = v[row[tuple(q)]]
                    can = (blk[:, 1] == 1) & ~((cur[:, 0] >= 1) | (cur[:, 1] <= 0)) & (cur[:, 1] >= 1)
                    touched.update((tuple(q), int(i)) for i in np.flatnonzero(can))
            m.deintegrate(f)
        _cache[key] = (m.export(), dict(m.counts), (m.entries, m.selected, m.updated), written + len(touched))
    (ok, ox), counts, totals, written = _cache[key]
    assert totals[2] > 0 and counts["reverted"] + counts["reset"] > 0
    hv = _handler(trunc)
    _fuse(hv, frames)
    for f in frames[10:21]:
        hv.DeintegrateImage(f[0], f[1], f[2], f[3] if len(f) > 3 else None)
    _equal(hv, ok, ox)
    got = hv.DeintegrateStats()
    print("%s signed, trunc %g: %s (restatement %s)" % (which, trunc, got, counts))
    assert got == counts
    st = hv.Stats()
    assert st["launches"] == 2 and (st["frames"], st["blocks_selected"], st["voxels_updated"]) == totals
    assert st["voxels_written"] == written
    assert _kinds(hv) == [0, 0, 2]


# ---- (g): the hypothesis about the reciprocal ----------------------------------------------------------------------------------------------
def test_g_reciprocal_of_zero_and_of_denormals_is_infinite_and_low_binades_are_within_d_rcp():
    """What px_round.hpp's argument needs of v_rcp_f32 once the window test is gone: +-inf for +-0 and for every denormal (then t'' = fma(nx, y, kb) is
    +-inf or NaN and the certificate refuses the lane), and |1 - Z y| <= d_rcp with a normal y in the binades 2^-126 .. 2^-61 the window test used to
    keep out (tests/test_kc_diet_gpu.py sweeps every significand of [1, 2))."""
    from onepiece_amd import _lib as L
    lib = L.load()

    def rcp(x):
        x = np.ascontiguousarray(x, F32)
        out = np.empty_like(x)
        L.check(lib.op_debug_rcp(C.c_void_p(x.ctypes.data), len(x), C.c_void_p(out.ctypes.data)))
        return out

    y = rcp(np.array([0.0, -0.0], F32))
    assert np.isposinf(y[0]) and np.isneginf(y[1])
    rng = np.random.default_rng(11)
    den = np.concatenate([np.array([1, 2, 3, 1 << 22, (1 << 23) - 2, (1 << 23) - 1], np.uint32), 1 << np.arange(23, dtype=np.uint32),
                          rng.integers(1, 1 << 23, 1 << 16).astype(np.uint32)])
    for sign in (0, 0x80000000):
        x = (den | np.uint32(sign)).view(F32)
        assert np.all(x != 0) and np.all(np.abs(x) < F32(2.0 ** -126))
        y = rcp(x)
        assert np.all(np.isinf(y)) and np.array_equal(np.signbit(y), np.signbit(x)), (x[~np.isinf(y)][:4], y[~np.isinf(y)][:4])
    d_rcp = lib.op_debug_px_rcp_err()
    worst = 0.0
    for e in range(-126, -60):
        s = rng.integers(0, 1 << 23, 1 << 12).astype(np.uint32)
        s[:2] = (0, (1 << 23) - 1)
        for sign in (0, 0x80000000):
            z = ((np.uint32(127 + e) << np.uint32(23)) | s | np.uint32(sign)).view(F32)
            y = rcp(z)
            assert np.all(np.isfinite(y)) and np.all(np.abs(y) >= F32(2.0 ** -126))
            err = np.abs(1.0 - z.astype(np.float64) * y.astype(np.float64))   # exact: a 24 x 24 bit product and a difference near 0
            assert err.max() <= d_rcp, (e, float(z[np.argmax(err)]))
            worst = max(worst, float(err.max()))
    print("binades 2^-126 .. 2^-61: max |1 - Z y| = %.5f * 2^-23" % (worst / 2.0 ** -23))
    assert worst > 2.0 ** -25
