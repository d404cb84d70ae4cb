"""De-integration restated on the CPU (test infrastructure shared by tests/test_deintegrate_cpu.py and tests/test_deintegrate_gpu.py).

The definition (include/onepiece_hip.h, op_volume_deintegrate): D(depth, rgb, pose) takes the steps of IntegrateImage -- same prepared frame, same
selected (and allocated) blocks, same pixel, same predicate -- and a voxel that passes receives TSDFVoxel::operator+ (TSDFVoxel.h:24-39) with an
observation of weight -1.  Neither the selection nor the predicate depends on what the volume stores, so the oracle gives the exact observation set
of a frame B without any change: fuse B ALONE into a fresh oracle volume with the same settings.  Its keys are B's selection; a voxel there has weight
1 iff B hits it and then holds exactly (o, 1, oc).  `apply_deintegrate` is steps 1-4 of the definition in numpy float32 on two exports; a continued
run is `oracle.Volume.load(expected)` followed by `integrate`.
"""
import numpy as np

from onepiece_amd import synthetic as S

F32 = np.float32
DEFAULT_VOXEL = np.array([999.0, 0.0, -1.0, -1.0, -1.0], F32)

# the issue's two cameras: (fx, fy, cx, cy, width, height, depth_scale)
CAM_37 = (30.0, 30.0, 18.25, 14.25, 37, 29, 1000.0)
CAM_64 = (52.0, 52.0, 31.75, 23.75, 64, 48, 1000.0)
RES = 0.04


def frames(camt, n, stride=5):
    """n frames of the analytic room, frame k = room frame k * stride: (depth [h,w] f32, rgb [h,w,3] u8, pose [4,4] f32) each."""
    out = []
    for k in range(n):
        pose = S.room_pose(k * stride)
        d, c = S.room_render(pose, width=camt[4], height=camt[5], fx=camt[0], fy=camt[1], cx=camt[2], cy=camt[3])
        out.append((np.ascontiguousarray(d, F32), np.ascontiguousarray(c, np.uint8), pose))
    return out


def deintegrate_voxels(s, w, c, o, oc):
    """Steps 1-4 for arrays of hit voxels: stored (s, w, c [n,3]), observation (o, oc [n,3]); every product, sum and quotient is one float32
    operation of numpy (no contraction).  -> (s', w', c', applied, reset)."""
    s, w, c, o, oc = (np.asarray(a, F32) for a in (s, w, c, o, oc))
    with np.errstate(all="ignore"):
        applied = ~((s >= 1) | (w <= 0)) & (w >= 1)                  # 1.
        rw = (w + F32(-1.0)).astype(F32)                              # 2.
        reset = applied & (rw == 0)                                   # 3.
        rev = applied & ~reset                                        # 4.
        den = np.where(rev, rw, F32(1.0)).astype(F32)
        s4 = ((w * s).astype(F32) + (F32(-1.0) * o).astype(F32)).astype(F32) / den
        c4 = ((w[:, None] * c).astype(F32) + (F32(-1.0) * oc).astype(F32)).astype(F32) / den[:, None]
    s2 = np.where(rev, s4.astype(F32), np.where(reset, F32(999.0), s)).astype(F32)
    w2 = np.where(rev, rw, np.where(reset, F32(0.0), w)).astype(F32)
    c2 = np.where(rev[:, None], c4.astype(F32), np.where(reset[:, None], F32(-1.0), c)).astype(F32)
    return s2, w2, c2, applied, reset


def _key_index(keys):
    return {tuple(k): i for i, k in enumerate(np.asarray(keys).tolist())}


def apply_deintegrate(keys, vox, bkeys, bvox):
    """The state (keys [n,3], vox [n,512,5]) after D(B), where (bkeys, bvox) is the export of B fused alone.
    -> (keys', vox', counts): keys' = keys + B's selection (sorted), counts = {"hits", "reverted", "reset", "skipped"}."""
    have = _key_index(keys)
    extra = [k for k in np.asarray(bkeys).tolist() if tuple(k) not in have]
    if extra:
        keys = np.concatenate([np.asarray(keys, np.int32).reshape(-1, 3), np.asarray(extra, np.int32)])
        fresh = np.broadcast_to(DEFAULT_VOXEL, (len(extra), 512, 5))
        vox = np.concatenate([np.asarray(vox, F32).reshape(-1, 512, 5), fresh])
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0])) if len(keys) else np.zeros(0, np.int64)
    keys, vox = np.ascontiguousarray(keys[order]), np.array(vox[order], F32)
    at = _key_index(keys)
    rows = np.array([at[tuple(k)] for k in np.asarray(bkeys).tolist()], np.int64)
    cur = vox[rows]                                                   # [m,512,5] copies
    hit = bvox[..., 1] == 1                                           # B alone: weight 1 iff B hits the voxel
    s2, w2, c2, applied, reset = deintegrate_voxels(cur[hit][:, 0], cur[hit][:, 1], cur[hit][:, 2:], bvox[hit][:, 0], bvox[hit][:, 2:])
    new = cur[hit]
    new[:, 0], new[:, 1], new[:, 2:] = s2, w2, c2
    cur[hit] = new
    vox[rows] = cur
    n_hit, n_app, n_rst = int(hit.sum()), int(applied.sum()), int(reset.sum())
    return keys, vox, {"hits": n_hit, "reverted": n_app - n_rst, "reset": n_rst, "skipped": n_hit - n_app}


class Model:
    """The expected volume: the oracle for integrations, apply_deintegrate for de-integrations, in call order."""

    def __init__(self, O, camt, trunc, res=RES):
        self.O, self.camt, self.trunc, self.res = O, camt, trunc, res
        self.vol = O.Volume(O.make_camera(*camt), voxel_res=res, trunc=trunc)
        self.counts = {"frames": 0, "reverted": 0, "reset": 0, "skipped": 0}
        self.updated = 0                                              # integration updates (op_volume_stats' voxels_updated)
        self.entries = 0                                              # every queue entry (op_volume_stats' frames)
        self.selected = 0                                             # sum of selection lengths over the entries
        self.last = None                                              # counts of the last de-integration

    def observation(self, frame):
        alone = self.O.Volume(self.O.make_camera(*self.camt), voxel_res=self.res, trunc=self.trunc)
        alone.integrate(*frame)
        return alone.export()

    def integrate(self, frame):
        n, _nv, nu = self.vol.integrate(*frame)
        self.updated += nu
        self.entries += 1
        self.selected += n
        return self

    def deintegrate(self, frame):
        bk, bv = self.observation(frame)
        k, v = self.vol.export()
        k2, v2, cnt = apply_deintegrate(k, v, bk, bv)
        self.vol.load(k2, v2)
        self.counts["frames"] += 1
        for name in ("reverted", "reset", "skipped"):
            self.counts[name] += cnt[name]
        self.entries += 1
        self.selected += len(bk)
        self.last = cnt
        return self

    def reintegrate(self, frame, new_pose):
        return self.deintegrate(frame).integrate((frame[0], frame[1], new_pose))

    def export(self):
        return self.vol.export()


def is_default(vox):
    """bit for bit the default voxel, for every voxel of `vox` [..., 5]"""
    return np.all(np.asarray(vox, F32).view(np.uint32) == DEFAULT_VOXEL.view(np.uint32), axis=-1)


def perturbed(pose, k):
    """`pose` moved by a few centimetres and about a degree (a drifted estimate of frame k); deterministic."""
    a = 0.015 + 0.002 * (k % 3)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = [0.03, -0.02 + 0.005 * (k % 2), 0.025]
    return (np.asarray(pose, np.float64) @ T).astype(F32)
