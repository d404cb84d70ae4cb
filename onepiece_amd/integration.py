"""Host-side mirror of one_piece::integration::CubeHandler over the C-ABI (include/onepiece_hip.h).

Same method names, argument meaning and error behaviour as the reference class
(/root/reference/src/Integration/CubeHandler.h:24-366) for the hot path, so the parity tests read
like the reference's own usage (example/ImageSequenceIntegration.cpp:27-42).  This module contains
no arithmetic of its own: every method forwards to libonepiece_hip.so, which fails loudly when no
GPU / no built library is present.

Images are numpy arrays (host, copied by the call) or torch CUDA tensors (used in place).  Poses
are 4x4 camera-to-world matrices (row-major numpy, i.e. `pose[r, c]` == Eigen `pose(r, c)`).
"""
import ctypes as C

import numpy as np

from . import _lib as L
from ._lib import Camera


def PinholeCamera(camera_type="OPEN3D_DATASET"):
    """camera::PinholeCamera presets (Camera/Camera.h:76-104); default ctor = OPEN3D_DATASET."""
    cam = Camera()
    L.check(L.load().op_camera_preset({"TUM_DATASET": 0, "OPEN3D_DATASET": 1}[camera_type], C.byref(cam)))
    return cam


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _image_arg(img, kind):
    """-> (pointer, fmt, mem, keepalive).  kind: 'depth' | 'rgb'.

    CUDA torch tensors are used in place by kernels on the LIBRARY's streams (each volume / tracker / ICP object
    owns one), not on torch's: the tensor's contents must be final when the kernels run, so torch's current stream is
    drained first if it still has work queued (L.torch_ready; nothing when it is idle).  A tensor produced on ANOTHER
    torch stream is the caller's to synchronise."""
    if hasattr(img, "data_ptr"):  # torch tensor
        if not img.is_cuda or not img.is_contiguous():
            raise ValueError("torch images must be contiguous CUDA tensors")
        import torch
        if kind == "depth":
            if img.dtype == torch.float32:
                fmt = L.OP_DEPTH_F32
            elif img.dtype in (torch.uint16, torch.int16):
                fmt = L.OP_DEPTH_U16
            else:
                raise ValueError("depth must be float32 (CV_32FC1) or uint16 (CV_16UC1)")
        else:
            if img.dtype != torch.uint8:
                raise ValueError("rgb must be uint8 (CV_8UC3)")
            fmt = 0
        L.torch_ready(img)
        return C.c_void_p(img.data_ptr()), fmt, L.OP_MEM_DEVICE, img
    a = np.ascontiguousarray(img)
    if kind == "depth":
        if a.dtype == np.uint16:
            fmt = L.OP_DEPTH_U16
        else:
            a = _f32(a)
            fmt = L.OP_DEPTH_F32
    else:
        a = np.ascontiguousarray(a, dtype=np.uint8)
        fmt = 0
    return C.c_void_p(a.ctypes.data), fmt, L.OP_MEM_HOST, a


class CubeHandler:
    """integration::CubeHandler: the voxel-block-hashed TSDF volume, resident on one MI355X."""

    def __init__(self, camera=None, device=0, max_blocks=0):
        self._lib = L.load()
        self.camera = camera if camera is not None else PinholeCamera()
        self.device = device
        self._h = C.c_void_p()
        # defaults: VoxelResolution 0.01 (VoxelCube.h:27), truncation 0.1 (Integrator.h:23),
        # far 5.0 / near 0.5 (CubeHandler.h:363-364)
        self._res, self._trunc, self._far, self._near = 0.01, 0.1, 5.0, 0.5
        self._alive = []
        L.check(self._lib.op_volume_create(C.byref(self.camera), self._res, self._trunc, self._far,
                                           self._near, device, max_blocks, C.byref(self._h)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._lib.op_volume_destroy(h)
            self._h = None

    # -- configuration (CubeHandler.h:36-39,137-144,339-346)
    def SetVoxelResolution(self, resolution):
        self._res = float(resolution)
        L.check(self._lib.op_volume_set_resolution(self._h, self._res))

    def SetTruncation(self, trunc):
        self._trunc = float(trunc)
        L.check(self._lib.op_volume_set_truncation(self._h, self._trunc))

    def SetCamera(self, camera):
        self.camera = camera
        L.check(self._lib.op_volume_set_camera(self._h, C.byref(camera)))

    def SetFarPlane(self, far):
        self._far = float(far)
        L.check(self._lib.op_volume_set_near_far(self._h, self._near, self._far))

    def SetNearPlane(self, near):
        self._near = float(near)
        L.check(self._lib.op_volume_set_near_far(self._h, self._near, self._far))

    def Clear(self):
        L.check(self._lib.op_volume_clear(self._h))

    def SetUpdateMode(self, mode):
        """Extension (op_volume_set_option / OP_VOLUME_OPT_UPDATE): "exact" (default; the reference's frame-by-frame running mean, voxels
        bit-identical to the CPU path) or "sum_form" (one weighted mean per batch of frames: same blocks and weights, sdf / colour to
        float rounding; a faster integrate kernel)."""
        value = {"exact": L.OP_VOLUME_UPDATE_EXACT, "sum_form": L.OP_VOLUME_UPDATE_SUM_FORM}[mode]
        L.check(self._lib.op_volume_set_option(self._h, L.OP_VOLUME_OPT_UPDATE, value))

    def SetSelectMode(self, mode):
        """Extension (op_volume_set_option / OP_VOLUME_OPT_SELECT): which form of the selection step batches take -- "auto" (default: in batches of
        >= 20 frames the frames record their selections and one pass claims every block once), "direct" (every frame claims its blocks itself) or an
        int n >= 1 (every batch of >= 2 frames records, except frames whose range has more than n super-blocks).  The selected set is the same in every mode."""
        value = {"auto": L.OP_VOLUME_SELECT_AUTO, "direct": L.OP_VOLUME_SELECT_DIRECT}.get(mode, mode)
        L.check(self._lib.op_volume_set_option(self._h, L.OP_VOLUME_OPT_SELECT, int(value)))

    # -- the hot path
    def ComputeBounding(self, depth, pose):
        """CubeHandler.cpp:116-145 -> (max_pos, min_pos, n_points_inside_frustum)."""
        p, fmt, mem, _keep = _image_arg(depth, "depth")
        pose = _f32(pose).reshape(16)
        mx, mn, n = np.empty(3, np.float32), np.empty(3, np.float32), C.c_size_t(0)
        L.check(self._lib.op_volume_compute_bounding(self._h, p, fmt, mem, _fp(pose), _fp(mx), _fp(mn), C.byref(n)))
        return mx, mn, int(n.value)

    def PrepareCubes(self, depth, pose, pose_inv=None, return_candidates=False):
        """CubeHandler.cpp:147-196 -> cube_id_list (n x 3 int32, reference loop order)."""
        p, fmt, mem, _keep = _image_arg(depth, "depth")
        pose = _f32(pose).reshape(16)
        pinv = _f32(pose_inv).reshape(16) if pose_inv is not None else None
        cap = 1 << 16
        while True:
            ids = np.empty((cap, 3), np.int32)
            n, nc = C.c_size_t(0), C.c_size_t(0)
            L.check(self._lib.op_volume_prepare_cubes(self._h, p, fmt, mem, _fp(pose), _fp(pinv) if pinv is not None else None,
                                                      _ip(ids), cap, C.byref(n), C.byref(nc)))
            if n.value <= cap:
                out = ids[:n.value].copy()
                return (out, int(nc.value)) if return_candidates else out
            cap = int(n.value)

    def IntegrateImage(self, depth, rgb, pose, pose_inv=None):
        """CubeHandler.cpp:197-210.  Asynchronous; any accessor below synchronises."""
        pd, fmt, mem, _k1 = _image_arg(depth, "depth")
        pr, _f, mem2, _k2 = _image_arg(rgb, "rgb")
        if mem != mem2:
            raise ValueError("depth and rgb must both be host arrays or both be device tensors")
        pose = _f32(pose).reshape(16)
        pinv = _f32(pose_inv).reshape(16) if pose_inv is not None else None
        # host buffers are borrowed for the call only (the library stages them before returning); device
        # tensors must stay alive until the next synchronising call -- keep a reference until then
        L.check(self._lib.op_volume_integrate(self._h, pd, fmt, pr, mem, _fp(pose), _fp(pinv) if pinv is not None else None))
        if mem == L.OP_MEM_DEVICE:
            self._alive.append((_k1, _k2))
            if len(self._alive) > 4096:
                self.Synchronize()

    def IntegrateCubes(self, depth, rgb, pose, cube_ids, pose_inv=None):
        """Integrator::IntegrateImage (Integrator.cpp:36-94) for a caller-chosen cube list (n x 3 int32): the frame is fused
        into exactly those cubes, allocated when absent, without PrepareCubes' selection.  Synchronous."""
        pd, fmt, mem, _k1 = _image_arg(depth, "depth")
        pr, _f, mem2, _k2 = _image_arg(rgb, "rgb")
        if mem != mem2:
            raise ValueError("depth and rgb must both be host arrays or both be device tensors")
        pose = _f32(pose).reshape(16)
        pinv = _f32(pose_inv).reshape(16) if pose_inv is not None else None
        ids = np.ascontiguousarray(cube_ids, np.int32).reshape(-1, 3)
        L.check(self._lib.op_volume_integrate_cubes(self._h, pd, fmt, pr, mem, _fp(pose), _fp(pinv) if pinv is not None else None, _ip(ids), len(ids)))

    def IntegrateFrame(self, rgbd, pose, pose_inv=None):
        """CubeHandler::IntegrateImage(const geometry::RGBDFrame&, pose) (CubeHandler.cpp:211-214)."""
        return self.IntegrateImage(rgbd.depth, rgbd.rgb, pose, pose_inv)

    def IntegrateSequence(self, depth, rgb, poses):
        """n frames resident on the device (torch tensors [n,h,w] / [n,h,w,3]); identical to n
        IntegrateImage calls in order (example/ImageSequenceIntegration.cpp:27-42)."""
        n = depth.shape[0]
        pd, fmt, mem, _k1 = _image_arg(depth, "depth")
        pr, _f, mem2, _k2 = _image_arg(rgb, "rgb")
        if mem != L.OP_MEM_DEVICE or mem2 != L.OP_MEM_DEVICE:
            raise ValueError("IntegrateSequence needs device-resident frames")
        poses = _f32(poses).reshape(n, 16)
        npx = self.camera.width * self.camera.height
        dstride = npx * (2 if fmt == L.OP_DEPTH_U16 else 4)
        L.check(self._lib.op_volume_integrate_sequence(self._h, pd, dstride, fmt, pr, npx * 3, _fp(poses), n))
        # a remainder of the call waits in the library's queue for the next frames: the tensors stay referenced until the next Synchronize
        self._alive.append((_k1, _k2))
        if len(self._alive) > 4096:
            self.Synchronize()

    # -- de-integration (extension; op_volume_deintegrate* / op_volume_reintegrate*: TSDFVoxel::operator+ with weight -1 under IntegrateImage's predicate)
    def _image_pair(self, depth, rgb):
        pd, fmt, mem, k1 = _image_arg(depth, "depth")
        pr, _f, mem2, k2 = _image_arg(rgb, "rgb")
        if mem != mem2:
            raise ValueError("depth and rgb must both be host arrays or both be device tensors")
        return pd, fmt, pr, mem, (k1, k2)

    def _keep(self, mem, keep):
        if mem == L.OP_MEM_DEVICE:
            self._alive.append(keep)
            if len(self._alive) > 4096:
                self.Synchronize()

    def DeintegrateImage(self, depth, rgb, pose, pose_inv=None):
        """Takes a frame that was fused at `pose` out again (the steps of IntegrateImage with an observation of weight -1; a voxel whose
        weight returns to 0 is the default voxel again).  Asynchronous, in call order with the integrations around it."""
        pd, fmt, pr, mem, keep = self._image_pair(depth, rgb)
        pose = _f32(pose).reshape(16)
        pinv = _f32(pose_inv).reshape(16) if pose_inv is not None else None
        L.check(self._lib.op_volume_deintegrate(self._h, pd, fmt, pr, mem, _fp(pose), _fp(pinv) if pinv is not None else None))
        self._keep(mem, keep)

    def ReintegrateImage(self, depth, rgb, old_pose, new_pose):
        """DeintegrateImage(depth, rgb, old_pose) then IntegrateImage(depth, rgb, new_pose) on one uploaded copy of the images, in one launch."""
        pd, fmt, pr, mem, keep = self._image_pair(depth, rgb)
        old, new = _f32(old_pose).reshape(16), _f32(new_pose).reshape(16)
        L.check(self._lib.op_volume_reintegrate(self._h, pd, fmt, pr, mem, _fp(old), _fp(new)))
        self._keep(mem, keep)

    def _sequence_args(self, depth, rgb):
        pd, fmt, pr, mem, keep = self._image_pair(depth, rgb)
        if mem != L.OP_MEM_DEVICE:
            raise ValueError("the sequence forms need device-resident frames")
        npx = self.camera.width * self.camera.height
        return pd, npx * (2 if fmt == L.OP_DEPTH_U16 else 4), fmt, pr, npx * 3, keep

    def DeintegrateSequence(self, depth, rgb, poses):
        """n device-resident frames (torch tensors [n,h,w] / [n,h,w,3]); identical to n DeintegrateImage calls in order."""
        n = depth.shape[0]
        pd, ds, fmt, pr, rs, keep = self._sequence_args(depth, rgb)
        poses = _f32(poses).reshape(n, 16)
        L.check(self._lib.op_volume_deintegrate_sequence(self._h, pd, ds, fmt, pr, rs, _fp(poses), n))
        self._keep(L.OP_MEM_DEVICE, keep)

    def ReintegrateSequence(self, depth, rgb, old_poses, new_poses):
        """n device-resident frames moved from old_poses[f] to new_poses[f]; identical to n ReintegrateImage calls in order (16 frames per launch)."""
        n = depth.shape[0]
        pd, ds, fmt, pr, rs, keep = self._sequence_args(depth, rgb)
        old, new = _f32(old_poses).reshape(n, 16), _f32(new_poses).reshape(n, 16)
        L.check(self._lib.op_volume_reintegrate_sequence(self._h, pd, ds, fmt, pr, rs, _fp(old), _fp(new), n))
        self._keep(L.OP_MEM_DEVICE, keep)

    def DeintegrateStats(self):
        """De-integrations since create / Clear (synchronises): frames, and of their voxels that passed the update predicate those reverted,
        reset to the default voxel and skipped (op_volume_deintegrate_stats)."""
        v = [C.c_uint64(0) for _ in range(4)]
        L.check(self._lib.op_volume_deintegrate_stats(self._h, *[C.byref(x) for x in v]))
        return {"frames": v[0].value, "reverted": v[1].value, "reset": v[2].value, "skipped": v[3].value}

    def CollectGarbage(self, min_weight=0.0, box=None):
        """CubeHandler::CollectGarbage (declared at CubeHandler.h:357, defined nowhere in the reference; op_volume_collect_garbage): drops every
        block without a voxel of weight > 0 and >= min_weight and, with box = (lo, hi) in block ids (inclusive), every block outside it; the pool
        is compacted in place on the device.  Synchronises.  -> {"blocks_before", "blocks_kept", "removed_outside", "removed_unobserved",
        "blocks_moved"}."""
        st = L.CollectStats()
        lo = hi = None
        if box is not None:
            lo, hi = (np.ascontiguousarray(b, np.int32).reshape(3) for b in box)
        L.check(self._lib.op_volume_collect_garbage(self._h, float(min_weight), None if lo is None else _ip(lo), None if hi is None else _ip(hi), C.byref(st)))
        self._alive = []
        return {k: int(getattr(st, k)) for k, _t in L.CollectStats._fields_}

    def IntegrateImageUnaligned(self, depth, rgb, pose, rgb_camera, color_to_depth=None, pose_inv=None):
        """Extension: IntegrateImage(depth, tool::AlignColorToDepth(rgb, depth, rgb_camera, this camera, color_to_depth), pose) for a colour image
        from a second camera ([hc, wc, 3], any size) -- the ScanNet flow (example/GenerateModelFromScannet.cpp, Tool/IO.cpp:9-58).  The alignment
        runs on the volume's stream into a ring the volume owns (op_volume_integrate_unaligned); asynchronous like IntegrateImage."""
        pd, fmt, mem, _k1 = _image_arg(depth, "depth")
        pr, _f, mem2, _k2 = _image_arg(rgb, "rgb")
        if mem != mem2:
            raise ValueError("depth and rgb must both be host arrays or both be device tensors")
        if len(_k2.shape) != 3 or _k2.shape[2] != 3:
            raise ValueError("rgb must be [rows, cols, 3]")
        if tuple(_k1.shape) != (self.camera.height, self.camera.width):
            raise ValueError("the depth image must have the volume camera's size")
        pose = _f32(pose).reshape(16)
        pinv = _f32(pose_inv).reshape(16) if pose_inv is not None else None
        m = _f32(color_to_depth).reshape(16) if color_to_depth is not None else None
        L.check(self._lib.op_volume_integrate_unaligned(self._h, pd, fmt, pr, int(_k2.shape[0]), int(_k2.shape[1]), C.byref(rgb_camera),
                                                        _fp(m) if m is not None else None, mem, _fp(pose), _fp(pinv) if pinv is not None else None))
        if mem == L.OP_MEM_DEVICE:
            self._alive.append((_k1, _k2))
            if len(self._alive) > 4096:
                self.Synchronize()

    def IntegrateSequenceUnaligned(self, depth, rgb, poses, rgb_camera, color_to_depth=None):
        """n device-resident frames (torch tensors [n, h, w] / [n, hc, wc, 3]) with one colour camera and one color_to_depth; identical to n
        IntegrateImageUnaligned calls in order (op_volume_integrate_unaligned_sequence)."""
        n = depth.shape[0]
        pd, fmt, mem, _k1 = _image_arg(depth, "depth")
        pr, _f, mem2, _k2 = _image_arg(rgb, "rgb")
        if mem != L.OP_MEM_DEVICE or mem2 != L.OP_MEM_DEVICE:
            raise ValueError("IntegrateSequenceUnaligned needs device-resident frames")
        if len(rgb.shape) != 4 or rgb.shape[0] != n or rgb.shape[3] != 3:
            raise ValueError("rgb must be [n, rows, cols, 3]")
        if tuple(depth.shape) != (n, self.camera.height, self.camera.width):
            raise ValueError("depth must be [n, h, w] of the volume camera's size")
        poses = _f32(poses).reshape(n, 16)
        m = _f32(color_to_depth).reshape(16) if color_to_depth is not None else None
        npx = self.camera.width * self.camera.height
        rows, cols = int(rgb.shape[1]), int(rgb.shape[2])
        L.check(self._lib.op_volume_integrate_unaligned_sequence(self._h, pd, npx * (2 if fmt == L.OP_DEPTH_U16 else 4), fmt, pr, rows * cols * 3, rows, cols,
                                                                 C.byref(rgb_camera), _fp(m) if m is not None else None, _fp(poses), n))
        self._alive.append((_k1, _k2))
        if len(self._alive) > 4096:
            self.Synchronize()

    def Flush(self):
        """launch the queued frames now (a batch smaller than 32) without waiting for them"""
        L.check(self._lib.op_volume_flush(self._h))

    def Synchronize(self):
        L.check(self._lib.op_volume_sync(self._h))
        self._alive = []

    def Stream(self):
        s = C.c_void_p()
        L.check(self._lib.op_volume_stream(self._h, C.byref(s)))
        return s.value

    def Stats(self):
        f, b, vis, upd = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        L.check(self._lib.op_volume_stats(self._h, C.byref(f), C.byref(b), C.byref(vis), C.byref(upd)))
        ln, br, vw, sc = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        L.check(self._lib.op_volume_stats_launches(self._h, C.byref(ln), C.byref(br), C.byref(vw), C.byref(sc)))
        return {"frames": f.value, "blocks_selected": b.value, "voxels_visited": vis.value, "voxels_updated": upd.value,
                "launches": ln.value, "blocks_read": br.value, "voxels_written": vw.value, "integrate_shader_cycles": sc.value}

    def GrowthStats(self):
        """capacity in blocks, pool growths, batches launched again after a growth (no synchronisation)"""
        m, g, r = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        L.check(self._lib.op_volume_growth_stats(self._h, C.byref(m), C.byref(g), C.byref(r)))
        return {"max_blocks": m.value, "grows": g.value, "replayed_batches": r.value}

    def ProfileEnable(self, sample_every=1):
        """HIP-event timing of K1/K2/K3 on the volume's own stream (measurement hook)."""
        L.check(self._lib.op_volume_profile_enable(self._h, int(sample_every)))

    def ProfileRead(self):
        """-> per-LAUNCH average ms of the three kernels + launches/frames covered by the samples."""
        ms = (C.c_double * 3)()
        n, nf = C.c_uint64(0), C.c_uint64(0)
        L.check(self._lib.op_volume_profile_read(self._h, ms, C.byref(n), C.byref(nf)))
        n, nf = int(n.value), int(nf.value)
        names = ("prepare_ms", "select_ms", "integrate_ms")
        return {"launches": n, "frames": nf, **{k: (ms[i] / n if n else float("nan")) for i, k in enumerate(names)}}

    # -- accessors (all synchronise)
    def BlockCount(self):
        n = C.c_size_t(0)
        L.check(self._lib.op_volume_block_count(self._h, C.byref(n)))
        return int(n.value)

    def HasCube(self, cube_id):
        r = C.c_int(0)
        L.check(self._lib.op_volume_has_cube(self._h, int(cube_id[0]), int(cube_id[1]), int(cube_id[2]), C.byref(r)))
        return bool(r.value)

    def GetCubeMap(self, sort=True):
        """CubeHandler.h:347-350 -> (keys n x 3 int32, voxels n x 512 x 5 float32 {sdf,w,c0,c1,c2}).
        The reference map's iteration order is unspecified; keys come back sorted (x, y, z)."""
        n = self.BlockCount()
        keys = np.empty((n, 3), np.int32)
        vox = np.empty((n, 512, 5), np.float32)
        got = C.c_size_t(0)
        L.check(self._lib.op_volume_download(self._h, _ip(keys), _fp(vox), n, C.byref(got)))
        if sort and n:
            order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
            keys, vox = keys[order], vox[order]
        return keys, vox

    def SetCubeMap(self, keys, voxels):
        """CubeHandler.h:351-356."""
        self.Clear()
        self.AddCubes(keys, voxels)

    def AddCubes(self, keys, voxels):
        keys = np.ascontiguousarray(keys, np.int32).reshape(-1, 3)
        voxels = _f32(voxels).reshape(-1, 512, 5)
        L.check(self._lib.op_volume_upload(self._h, _ip(keys), _fp(voxels), keys.shape[0]))

    def AddCube(self, cube_id):
        """CubeHandler::AddCube (CubeHandler.h:191-197): a default block (sdf 999, weight 0, colour -1) unless present."""
        if self.HasCube(cube_id):
            return
        vox = np.empty((1, 512, 5), np.float32)
        vox[..., 0], vox[..., 1], vox[..., 2:] = 999.0, 0.0, -1.0
        self.AddCubes(np.asarray(cube_id, np.int32).reshape(1, 3), vox)

    def Merge(self, another, trans=None):
        """CubeHandler::Merge (CubeHandler.h:145-177): mismatching resolution -> warning line, no change.
        With `trans`: Merge(*another.Transform(trans)) (:168-177)."""
        if trans is not None:
            if another.GetVoxelResolution() != self.GetVoxelResolution():
                print("[Warning]::[MergeVoxelHash]::Voxel resolution is not identical.")
                return
            another = another.Transform(trans)
        rc = self._lib.op_volume_merge(self._h, another._h)
        if rc == L.OP_ERR_MISMATCH:
            print(self._lib.op_last_error().decode())
            return
        L.check(rc)

    def MergeTransformed(self, others, transforms):
        """Extension (op_volume_merge_transformed_many states the definition): what `for o, T in zip(others, transforms): self.Merge(o, T)`
        leaves in this volume, bit for bit, in one device call and without the intermediate volumes -- every source is resampled straight into
        this volume's blocks.  `others`: one CubeHandler or a list; `transforms`: one 4 x 4 matrix or as many as there are sources.  A source of
        another resolution -> the reference's warning line, no change, None.  Returns the call's counts: {"sources", "src_blocks",
        "touched_blocks", "created_blocks", "pairs", "voxels_copied", "voxels_kept", "voxels_blended", "voxels_reset"}."""
        if isinstance(others, CubeHandler):
            others, transforms = [others], [transforms]
        others = list(others)
        Ts = np.ascontiguousarray(np.stack([_f32(T).reshape(16) for T in transforms]) if len(others) else np.zeros((0, 16), np.float32))
        if Ts.shape[0] != len(others):
            raise ValueError("MergeTransformed: %d sources, %d transforms" % (len(others), Ts.shape[0]))
        handles = (C.c_void_p * max(len(others), 1))(*[o._h for o in others])
        st = L.MergeTransformedStats()
        rc = self._lib.op_volume_merge_transformed_many(self._h, handles, _fp(Ts), None, len(others), C.byref(st))
        if rc == L.OP_ERR_MISMATCH:
            print(self._lib.op_last_error().decode())
            return None
        L.check(rc)
        return {k: int(getattr(st, k)) for k, _t in L.MergeTransformedStats._fields_}

    # -- resampling, point cloud, .map files (CubeHandler.h:40-128,242-338; CubeHandler.cpp:45-69)
    @classmethod
    def _wrap(cls, handle, camera, device):
        out = cls.__new__(cls)
        out._lib = L.load()
        out.camera, out.device, out._h = camera, device, handle
        out._alive = []
        res = C.c_float(0)
        L.check(out._lib.op_volume_resolution(handle, C.byref(res)))
        out._res, out._trunc, out._far, out._near = float(res.value), None, None, None
        return out

    def _transform(self, trans, nearest, max_blocks):
        T = _f32(trans).reshape(16)
        h = C.c_void_p()
        L.check(self._lib.op_volume_transform(self._h, _fp(T), None, 1 if nearest else 0, max_blocks, C.byref(h)))
        out = CubeHandler._wrap(h, self.camera, self.device)
        out._trunc, out._far, out._near = self._trunc, self._far, self._near
        return out

    def Transform(self, trans, max_blocks=0):
        """CubeHandler::Transform (CubeHandler.h:242-298): trilinear resampling -> new CubeHandler."""
        return self._transform(trans, False, max_blocks)

    def TransformNearest(self, trans, max_blocks=0):
        """CubeHandler::TransformNearest (CubeHandler.h:299-338).  Like the reference, the result keeps
        the DEFAULT voxel resolution 0.01 (c_para is not copied there)."""
        return self._transform(trans, True, max_blocks)

    def Coarsen(self, levels=1, min_weight=0.0, max_blocks=0):
        """Extension (op_volume_coarsen states the definition; not in the reference): a NEW CubeHandler of 2^levels times the voxel size, each
        level's voxel the weighted mean of its 2 x 2 x 2 fine voxels of weight > 0 and >= min_weight, its weight their sum / 8.  This volume is
        not changed.  The last level's counts are the result's `coarsen_stats`: {"src_blocks", "dst_blocks", "voxels_full", "voxels_partial",
        "voxels_empty", "dropped_min_weight"}."""
        h, st = C.c_void_p(), L.CoarsenStats()
        L.check(self._lib.op_volume_coarsen(self._h, int(levels), float(min_weight), int(max_blocks), C.byref(h), C.byref(st)))
        out = CubeHandler._wrap(h, self.camera, self.device)
        out._trunc, out._far, out._near = self._trunc, self._far, self._near
        out.coarsen_stats = {k: int(getattr(st, k)) for k, _t in L.CoarsenStats._fields_}
        return out

    def GetVoxelResolution(self):
        return self._res

    def GetPointCloud(self):
        """CubeHandler::GetPointCloud (CubeHandler.cpp:45-69) -> (points [n,3], colors [n,3])."""
        n = C.c_size_t(0)
        L.check(self._lib.op_volume_point_cloud(self._h, None, None, 0, C.byref(n)))
        xyz = np.empty((max(n.value, 1), 3), np.float32)
        col = np.empty((max(n.value, 1), 3), np.float32)
        L.check(self._lib.op_volume_point_cloud(self._h, _fp(xyz), _fp(col), n.value, C.byref(n)))
        return xyz[:n.value], col[:n.value]

    def ExtractTriangleMesh(self, tri_table, edge_pairs, only_block=None):
        """CubeHandler::ExtractTriangleMesh (CubeHandler.cpp:9-44) on the GPU -> (points [n,3], colors [n,3]); triangle k
        is vertices 3k..3k+2 (MarchingCube() pushes unshared vertices).  tri_table (256 x 16) / edge_pairs (12 x 2) are
        the caller's marching-cubes tables (the reference's MCLookTable / EdgeIndexPairs)."""
        tt = np.ascontiguousarray(tri_table, np.int32).reshape(256 * 16)
        ep = np.ascontiguousarray(edge_pairs, np.int32).reshape(24)
        ob = None if only_block is None else np.ascontiguousarray(only_block, np.int32).reshape(3)
        obp = None if ob is None else _ip(ob)
        n = C.c_size_t(0)
        L.check(self._lib.op_volume_extract_mesh(self._h, _ip(tt), _ip(ep), obp, None, None, 0, C.byref(n)))
        pts, col = np.empty((max(n.value, 1), 3), np.float32), np.empty((max(n.value, 1), 3), np.float32)
        if n.value:
            L.check(self._lib.op_volume_extract_mesh(self._h, _ip(tt), _ip(ep), obp, _fp(pts), _fp(col), n.value, C.byref(n)))
        return pts[:n.value].copy(), col[:n.value].copy()

    def ExtractSimplifiedTriangleMesh(self, tri_table, edge_pairs, grid_len, only_block=None):
        """ExtractTriangleMesh followed by TriangleMesh::ClusteringSimplify(grid_len) (MeshSimplification.cpp:579-657) in one device call
        (op_volume_extract_mesh_clustered): the triangle soup never leaves the device -> (points [m,3], colors [m,3], triangles [k,3] uint32),
        the bits of registration.cluster_simplify over ExtractTriangleMesh's soup."""
        tt = np.ascontiguousarray(tri_table, np.int32).reshape(256 * 16)
        ep = np.ascontiguousarray(edge_pairs, np.int32).reshape(24)
        ob = None if only_block is None else np.ascontiguousarray(only_block, np.int32).reshape(3)
        obp = None if ob is None else _ip(ob)
        nv, nt = C.c_size_t(0), C.c_size_t(0)  # upper bounds from the sizing call, the true sizes from the filling one
        L.check(self._lib.op_volume_extract_mesh_clustered(self._h, _ip(tt), _ip(ep), obp, float(grid_len), None, None, 0, None, 0, C.byref(nv), C.byref(nt)))
        pts, col = np.empty((max(nv.value, 1), 3), np.float32), np.empty((max(nv.value, 1), 3), np.float32)
        tri = np.empty((max(nt.value, 1), 3), np.uint32)
        if nt.value:
            L.check(self._lib.op_volume_extract_mesh_clustered(self._h, _ip(tt), _ip(ep), obp, float(grid_len), C.c_void_p(pts.ctypes.data), C.c_void_p(col.ctypes.data),
                                                               nv.value, C.c_void_p(tri.ctypes.data), nt.value, C.byref(nv), C.byref(nt)))
        return pts[:nv.value].copy(), col[:nv.value].copy(), tri[:nt.value].copy()

    def ExtractProcessedTriangleMesh(self, tri_table, edge_pairs, grid_len=0.0, min_points=0, compute_normals=False, only_block=None):
        """ExtractTriangleMesh, then ClusteringSimplify(grid_len) if grid_len > 0, then Prune(min_points) if min_points > 0, then ComputeNormals if asked,
        in one device call (op_volume_extract_mesh_processed): only the finished mesh leaves the device ->
        (points [m,3], colors [m,3], normals [m,3] or None, triangles [k,3] uint32)."""
        tt = np.ascontiguousarray(tri_table, np.int32).reshape(256 * 16)
        ep = np.ascontiguousarray(edge_pairs, np.int32).reshape(24)
        ob = None if only_block is None else np.ascontiguousarray(only_block, np.int32).reshape(3)
        obp = None if ob is None else _ip(ob)
        nv, nt = C.c_size_t(0), C.c_size_t(0)  # upper bounds from the sizing call, the true sizes from the filling one
        L.check(self._lib.op_volume_extract_mesh_processed(self._h, _ip(tt), _ip(ep), obp, float(grid_len), int(min_points), None, None, None, 0, None, 0, C.byref(nv), C.byref(nt)))
        pts, col = np.empty((max(nv.value, 1), 3), np.float32), np.empty((max(nv.value, 1), 3), np.float32)
        nrm = np.empty((max(nv.value, 1), 3), np.float32) if compute_normals else None
        tri = np.empty((max(nt.value, 1), 3), np.uint32)
        if nt.value:
            L.check(self._lib.op_volume_extract_mesh_processed(self._h, _ip(tt), _ip(ep), obp, float(grid_len), int(min_points), C.c_void_p(pts.ctypes.data),
                                                               C.c_void_p(col.ctypes.data), None if nrm is None else C.c_void_p(nrm.ctypes.data), nv.value,
                                                               C.c_void_p(tri.ctypes.data), nt.value, C.byref(nv), C.byref(nt)))
        return pts[:nv.value].copy(), col[:nv.value].copy(), None if nrm is None else nrm[:nv.value].copy(), tri[:nt.value].copy()

    def GenerateMeshByCube(self, cube_id, tri_table, edge_pairs):
        """CubeHandler::GenerateMeshByCube (CubeHandler.cpp:70-114) for one block."""
        return self.ExtractTriangleMesh(tri_table, edge_pairs, only_block=cube_id)

    def Raycast(self, pose, camera=None):
        """Ray casting (north_star; no reference counterpart) -> (depth [h,w], normals [h,w,3],
        colors [h,w,3]); depth 0 = no hit."""
        cam = camera if camera is not None else self.camera
        pose = _f32(pose).reshape(16)
        d = np.zeros((cam.height, cam.width), np.float32)
        n = np.zeros((cam.height, cam.width, 3), np.float32)
        c = np.zeros((cam.height, cam.width, 3), np.float32)
        L.check(self._lib.op_volume_raycast(self._h, C.byref(cam), _fp(pose), _fp(d), _fp(n), _fp(c), L.OP_MEM_HOST))
        return d, n, c

    def RaycastDevice(self, pose, depth_ptr, normals_ptr=0, colors_ptr=0, camera=None):
        """The same with outputs that stay in HBM: device addresses (e.g. torch tensor.data_ptr()) of W*H / W*H*3 float32 buffers on the
        volume's device; 0 = not wanted.  Returns when the images are complete."""
        cam = camera if camera is not None else self.camera
        pose = _f32(pose).reshape(16)
        as_fp = lambda a: C.cast(C.c_void_p(int(a)), L._fp) if a else None
        L.check(self._lib.op_volume_raycast(self._h, C.byref(cam), _fp(pose), as_fp(depth_ptr), as_fp(normals_ptr), as_fp(colors_ptr), L.OP_MEM_DEVICE))

    def RenderFrame(self, pose, camera=None):
        """The model seen from `pose` as an RGB-D frame (op_volume_render_frame; no reference counterpart) -> (rgb [h,w,3] uint8,
        depth [h,w] float32 metres, 0 = no hit, n_valid): the format IntegrateImage and Odometry.DenseTracking take."""
        cam = camera if camera is not None else self.camera
        pose = _f32(pose).reshape(16)
        rgb = np.zeros((cam.height, cam.width, 3), np.uint8)
        d = np.zeros((cam.height, cam.width), np.float32)
        n = C.c_uint64(0)
        L.check(self._lib.op_volume_render_frame(self._h, C.byref(cam), _fp(pose), C.c_void_p(rgb.ctypes.data), _fp(d), L.OP_MEM_HOST, C.byref(n)))
        return rgb, d, int(n.value)

    def RenderFrameDevice(self, pose, rgb_ptr, depth_ptr, camera=None):
        """The same into buffers that stay in HBM: device addresses (e.g. torch tensor.data_ptr()) of a W*H*3 uint8 and a W*H float32 buffer on
        the volume's device.  Returns the number of valid pixels, when the frame is complete."""
        cam = camera if camera is not None else self.camera
        pose = _f32(pose).reshape(16)
        n = C.c_uint64(0)
        L.check(self._lib.op_volume_render_frame(self._h, C.byref(cam), _fp(pose), C.c_void_p(int(rgb_ptr)), C.cast(C.c_void_p(int(depth_ptr)), L._fp),
                                                 L.OP_MEM_DEVICE, C.byref(n)))
        return int(n.value)

    # -- point queries (extension; op_volume_sample: the raycaster's trilinear rule or ReadVoxelInterpolate at the caller's points)
    _SAMPLE_MODES = {"trilinear": L.OP_SAMPLE_TRILINEAR, "reference": L.OP_SAMPLE_REFERENCE}

    @staticmethod
    def _sample_stats(st):
        return {k: (int if t is C.c_uint64 else float)(getattr(st, k)) for k, t in L.SampleStats._fields_}

    def Sample(self, points, T=None, mode="trilinear", gradients=False, stats=False):
        """What the model holds at `points` ([n,3] float32, host): mode "trilinear" is the raycaster's strict trilinear sample (valid iff all
        eight taps are observed), "reference" is VoxelCube::ReadVoxelInterpolate as Transform evaluates it.  T: a 4x4 applied to the points first.
        -> (voxels [n,5] {sdf, weight, c0, c1, c2}, status [n] uint8 of OP_SAMPLE_* bits[, gradients [n,3]: the unnormalised central difference
        of the trilinear sdf at +-res/2][, stats dict]).  Synchronises; the volume is only read."""
        pts = np.ascontiguousarray(_f32(points).reshape(-1, 3))
        n = len(pts)
        vox, status = np.empty((n, 5), np.float32), np.empty(n, np.uint8)
        grad = np.empty((n, 3), np.float32) if gradients else None
        st = L.SampleStats() if stats else None
        Tm = _f32(T).reshape(16) if T is not None else None
        L.check(self._lib.op_volume_sample(self._h, C.c_void_p(pts.ctypes.data), n, L.OP_MEM_HOST, _fp(Tm) if Tm is not None else None,
                                           self._SAMPLE_MODES[mode], C.c_void_p(vox.ctypes.data), C.c_void_p(grad.ctypes.data) if gradients else None,
                                           C.c_void_p(status.ctypes.data), C.byref(st) if stats else None))
        self._alive = []
        out = (vox, status)
        if gradients:
            out += (grad,)
        if stats:
            out += (self._sample_stats(st),)
        return out

    def SampleDevice(self, points_ptr, n, voxels_ptr=0, status_ptr=0, gradients_ptr=0, T=None, mode="trilinear", stats=False):
        """The same with buffers that stay in HBM: device addresses (e.g. torch tensor.data_ptr()) of n x 3 float32 points and of the n x 5 float32,
        n uint8 and n x 3 float32 outputs on the volume's device; 0 = not wanted.  Returns the stats dict (or None) when the outputs are complete."""
        st = L.SampleStats() if stats else None
        Tm = _f32(T).reshape(16) if T is not None else None
        ptr = lambda a: C.c_void_p(int(a)) if a else None
        L.check(self._lib.op_volume_sample(self._h, ptr(points_ptr), int(n), L.OP_MEM_DEVICE, _fp(Tm) if Tm is not None else None, self._SAMPLE_MODES[mode],
                                           ptr(voxels_ptr), ptr(gradients_ptr), ptr(status_ptr), C.byref(st) if stats else None))
        self._alive = []
        return self._sample_stats(st) if stats else None

    # -- registration against the field (extension; op_volume_register_*: the trilinear sdf is the residual, its normalised gradient the normal)
    REGISTER_STATUS = ("converged", "max_iterations", "too_few_points", "singular")

    def _register_params(self, max_iterations, max_distance, min_step, min_points):
        p = L.RegisterParams()
        L.check(self._lib.op_volume_register_default_params(self._h, C.byref(p)))
        for k, val in (("max_iterations", max_iterations), ("max_distance", max_distance), ("min_step", min_step), ("min_points", min_points)):
            if val is not None:
                setattr(p, k, val)
        return p

    @staticmethod
    def _register_result(r):
        out = {k: getattr(r, k) for k, _t in L.RegisterResult._fields_ if k != "T"}
        out["T"] = np.array(r.T, np.float32).reshape(4, 4)
        out["status_name"] = CubeHandler.REGISTER_STATUS[r.status]
        return out

    # what every cloud-taking method makes of its arrays, every system method of its outputs and every frame method of its images
    @staticmethod
    def _offset_inputs(points, offset, intensity):
        pts = np.ascontiguousarray(_f32(points).reshape(-1, 3))
        o = np.ascontiguousarray(_f32(offset).reshape(-1)) if offset is not None else None
        y = np.ascontiguousarray(_f32(intensity).reshape(-1)) if intensity is not None else None
        if o is not None and len(o) != len(pts):
            raise ValueError("one target value per point")
        if y is not None and len(y) != len(pts):
            raise ValueError("one intensity per point")
        ptr = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
        return pts, o, y, ptr

    def _registration_system(self, n, n_sums, n_counts, row_width, rows, call):
        """call(sums, counts, rows or None) is the C entry on buffers of the extent it writes -> (sums, counts dict[, rows])"""
        sums, counts = np.zeros(n_sums, np.float64), np.zeros(n_counts, np.uint64)
        out = np.empty((n, row_width), np.float32) if rows else None
        L.check(call(sums.ctypes.data_as(C.POINTER(C.c_double)), counts.ctypes.data_as(L._u64p), C.c_void_p(out.ctypes.data) if rows else None))
        self._alive = []
        cd = dict(zip(self.ROBUST_COUNT_NAMES, (int(c) for c in counts)))
        return (sums, cd, out) if rows else (sums, cd)

    @staticmethod
    def _frame_images(depth, rgb, names="depth and rgb"):
        """-> (depth pointer, depth format, rgb pointer, mem, what keeps them alive); rgb None: no colour image, a NULL pointer"""
        pd, fmt, mem, k1 = _image_arg(depth, "depth")
        pr, k2 = None, None
        if rgb is not None:
            pr, _f, mem2, k2 = _image_arg(rgb, "rgb")
            if mem != mem2:
                raise ValueError("%s must both be host arrays or both be device tensors" % names)
        return pd, fmt, pr, mem, (k1, k2)

    def RegistrationSystem(self, points, T, max_distance, rows=False):
        """The point-to-plane system of `points` ([n,3] float32, host) at the 4x4 `T` against the model (op_volume_register_system)
        -> (sums [28] float64: the upper triangle of JtJ row by row, Jtr, sum of s^2; counts dict[, rows [n,8]: j[6], s, used])."""
        pts, _o, _y, ptr = self._offset_inputs(points, None, None)
        Tm = _f32(T).reshape(16)
        return self._registration_system(len(pts), 28, 4, 8, rows, lambda sums, counts, out: self._lib.op_volume_register_system(
            self._h, ptr(pts), len(pts), L.OP_MEM_HOST, _fp(Tm), float(max_distance), sums, counts, out))

    def RegisterPoints(self, points, init_T=None, max_iterations=None, max_distance=None, min_step=None, min_points=None):
        """Gauss-Newton registration of `points` ([n,3] float32, host) against the model from `init_T` (default identity) -> dict of
        op_volume_register_result's fields (T [4,4]: points to model).  None = the default (30 iterations, the truncation, 1e-5, 6)."""
        pts, _o, _y, ptr = self._offset_inputs(points, None, None)
        T0 = _f32(np.eye(4) if init_T is None else init_T).reshape(16)
        p, r = self._register_params(max_iterations, max_distance, min_step, min_points), L.RegisterResult()
        L.check(self._lib.op_volume_register_points(self._h, ptr(pts), len(pts), L.OP_MEM_HOST, _fp(T0), C.byref(p), C.byref(r)))
        self._alive = []
        return self._register_result(r)

    def RegisterDepth(self, depth, init_pose, pixel_stride=1, camera=None, max_iterations=None, max_distance=None, min_step=None, min_points=None):
        """The same for a depth image (numpy or CUDA torch tensor) back-projected on the device (every pixel_stride-th pixel in both directions)
        from `init_pose` (camera to world) -> the result dict, T the refined pose."""
        pd, fmt, _pr, mem, keep = self._frame_images(depth, None)
        pose = _f32(init_pose).reshape(16)
        p, r = self._register_params(max_iterations, max_distance, min_step, min_points), L.RegisterResult()
        L.check(self._lib.op_volume_register_depth(self._h, C.byref(camera) if camera is not None else None, pd, fmt, mem, int(pixel_stride), _fp(pose),
                                                   C.byref(p), C.byref(r)))
        del keep
        self._alive = []
        return self._register_result(r)

    # -- the colour term (op_volume_register_color_* / _rgbd: the model's intensity at the point against the observed one, a second residual)
    def _register_color_params(self, max_iterations, max_distance, min_step, min_points, color_scale, max_color_residual):
        p = L.RegisterColorParams()
        L.check(self._lib.op_volume_register_color_default_params(self._h, C.byref(p)))
        for k, val in (("max_iterations", max_iterations), ("max_distance", max_distance), ("min_step", min_step), ("min_points", min_points)):
            if val is not None:
                setattr(p.base, k, val)
        for k, val in (("color_scale", color_scale), ("max_color_residual", max_color_residual)):
            if val is not None:
                setattr(p, k, val)
        return p

    @staticmethod
    def _register_color_result(r):
        out = CubeHandler._register_result(r.base)
        out.update({k: getattr(r, k) for k in ("colored", "first_colored", "rmse_color", "first_rmse_color")})
        return out

    @staticmethod
    def Intensity(colors):
        """I(c) = (0.114 c0 + 0.587 c1) + 0.299 c2 in float32 of colour triples in stored channel order ([n,3] float32, byte / 255)."""
        c = _f32(colors).reshape(-1, 3)
        return (np.float32(0.114) * c[:, 0] + np.float32(0.587) * c[:, 1]) + np.float32(0.299) * c[:, 2]

    def ColorRegistrationSystem(self, points, intensity, T, max_distance, color_scale=1.0, max_color_residual=0.0, rows=False):
        """The point-to-plane system with the colour term (op_volume_register_color_system) of `points` ([n,3] float32) with observed
        intensities `intensity` ([n] float32; may be None with color_scale 0) -> (sums [30] float64: 0..27 as RegistrationSystem with the
        colour terms added, [28] the sum of rc^2, [29] the geometric sum of s^2; counts dict with `colored`[, rows [n,16]: j[6], s, used, jc[6],
        rcs, colored])."""
        pts, _o, y, ptr = self._offset_inputs(points, None, intensity)
        Tm = _f32(T).reshape(16)
        return self._registration_system(len(pts), 30, 5, 16, rows, lambda sums, counts, out: self._lib.op_volume_register_color_system(
            self._h, ptr(pts), ptr(y), len(pts), L.OP_MEM_HOST, _fp(Tm), float(max_distance), float(color_scale), float(max_color_residual), sums, counts, out))

    def RegisterColoredPoints(self, points, intensity, init_T=None, max_iterations=None, max_distance=None, min_step=None, min_points=None,
                              color_scale=None, max_color_residual=None):
        """RegisterPoints with the colour term: `intensity` [n] float32 in the volume's colour units (Intensity(colors) of a cloud's colours)
        -> the result dict with colored, first_colored, rmse_color, first_rmse_color.  color_scale None = 1, 0 = RegisterPoints."""
        pts, _o, y, ptr = self._offset_inputs(points, None, intensity)
        T0 = _f32(np.eye(4) if init_T is None else init_T).reshape(16)
        p = self._register_color_params(max_iterations, max_distance, min_step, min_points, color_scale, max_color_residual)
        r = L.RegisterColorResult()
        L.check(self._lib.op_volume_register_color_points(self._h, ptr(pts), ptr(y), len(pts), L.OP_MEM_HOST, _fp(T0), C.byref(p), C.byref(r)))
        self._alive = []
        return self._register_color_result(r)

    def RegisterRGBD(self, depth, rgb, init_pose, pixel_stride=1, camera=None, max_iterations=None, max_distance=None, min_step=None, min_points=None,
                     color_scale=None, max_color_residual=None):
        """RegisterDepth with the colour term: every kept pixel's intensity comes from its three bytes of `rgb` (uint8 [H,W,3], stored channel
        order; numpy or CUDA torch tensor like `depth`) -> the result dict, T the refined pose."""
        pd, fmt, pr, mem, keep = self._image_pair(depth, rgb)
        pose = _f32(init_pose).reshape(16)
        p = self._register_color_params(max_iterations, max_distance, min_step, min_points, color_scale, max_color_residual)
        r = L.RegisterColorResult()
        L.check(self._lib.op_volume_register_rgbd(self._h, C.byref(camera) if camera is not None else None, pd, fmt, pr, mem, int(pixel_stride), _fp(pose),
                                                  C.byref(p), C.byref(r)))
        del keep
        self._alive = []
        return self._register_color_result(r)

    # -- consistent linearisations and Huber weights (op_volume_register_robust_*: row and residual agree; the sdf is projective, |grad s| is not 1)
    LINEARIZATIONS = {"normal": L.OP_REGISTER_LIN_NORMAL, "gradient": L.OP_REGISTER_LIN_GRADIENT, "metric": L.OP_REGISTER_LIN_METRIC}
    ROBUST_COUNT_NAMES = ("used", "invalid", "no_gradient", "too_far", "colored", "downweighted", "color_downweighted")

    def _register_options(self, linearization, huber, huber_color):
        o = L.RegisterOptions()
        L.check(self._lib.op_volume_register_robust_default_options(self._h, C.byref(o)))
        if linearization is not None:
            o.linearization = self.LINEARIZATIONS[linearization] if isinstance(linearization, str) else int(linearization)
        for k, val in (("huber", huber), ("huber_color", huber_color)):
            if val is not None:
                setattr(o, k, val)
        return o

    @staticmethod
    def _register_robust_result(r):
        out = CubeHandler._register_color_result(r.color)
        out.update({k: getattr(r, k) for k in ("downweighted", "color_downweighted", "first_downweighted", "rmse_residual", "first_rmse_residual")})
        return out

    def RobustRegistrationSystem(self, points, intensity, T, max_distance, color_scale=0.0, max_color_residual=0.0, linearization=None, huber=None,
                                 huber_color=None, rows=False):
        """ColorRegistrationSystem under a linearisation ("normal" | "gradient" | "metric" or its number; None = metric) and Huber thresholds
        (None = 0 = no weights) (op_volume_register_robust_system) -> (sums [31] float64: 0..29 as ColorRegistrationSystem from the scaled rows,
        [30] the sum of the unweighted r^2; counts dict with `downweighted` and `color_downweighted`[, rows [n,16]: what enters the sums])."""
        pts, _o, y, ptr = self._offset_inputs(points, None, intensity)
        Tm = _f32(T).reshape(16)
        opt = self._register_options(linearization, huber, huber_color)
        return self._registration_system(len(pts), 31, 7, 16, rows, lambda sums, counts, out: self._lib.op_volume_register_robust_system(
            self._h, ptr(pts), ptr(y), len(pts), L.OP_MEM_HOST, _fp(Tm), float(max_distance), float(color_scale), float(max_color_residual), C.byref(opt),
            sums, counts, out))

    def RegisterPointsRobust(self, points, intensity=None, init_T=None, max_iterations=None, max_distance=None, min_step=None, min_points=None,
                             color_scale=None, max_color_residual=None, linearization=None, huber=None, huber_color=None):
        """RegisterColoredPoints under a linearisation and Huber thresholds (op_volume_register_robust_points).  intensity None: the geometric
        registration (color_scale 0) -> the result dict with downweighted, color_downweighted, first_downweighted, rmse_residual,
        first_rmse_residual.  linearization None = metric; "normal" with no threshold is RegisterColoredPoints bit for bit."""
        pts, _o, y, ptr = self._offset_inputs(points, None, intensity)
        if y is None and color_scale is None:
            color_scale = 0.0
        T0 = _f32(np.eye(4) if init_T is None else init_T).reshape(16)
        p = self._register_color_params(max_iterations, max_distance, min_step, min_points, color_scale, max_color_residual)
        o, r = self._register_options(linearization, huber, huber_color), L.RegisterRobustResult()
        L.check(self._lib.op_volume_register_robust_points(self._h, ptr(pts), ptr(y), len(pts), L.OP_MEM_HOST, _fp(T0), C.byref(p), C.byref(o), C.byref(r)))
        self._alive = []
        return self._register_robust_result(r)

    def RegisterFrameRobust(self, depth, rgb, init_pose, pixel_stride=1, camera=None, max_iterations=None, max_distance=None, min_step=None, min_points=None,
                            color_scale=None, max_color_residual=None, linearization=None, huber=None, huber_color=None):
        """RegisterRGBD (rgb None: RegisterDepth) under a linearisation and Huber thresholds (op_volume_register_robust_frame) -> the result dict,
        T the refined pose."""
        pd, fmt, pr, mem, keep = self._frame_images(depth, rgb)
        pose = _f32(init_pose).reshape(16)
        p = self._register_color_params(max_iterations, max_distance, min_step, min_points, color_scale, max_color_residual)
        o, r = self._register_options(linearization, huber, huber_color), L.RegisterRobustResult()
        L.check(self._lib.op_volume_register_robust_frame(self._h, C.byref(camera) if camera is not None else None, pd, fmt, pr, mem, int(pixel_stride), _fp(pose),
                                                          C.byref(p), C.byref(o), C.byref(r)))
        del keep
        self._alive = []
        return self._register_robust_result(r)

    # -- a target value per point, and one fused volume against another (op_volume_band_voxels, op_volume_register_offset_*, op_volume_register_volume)
    def _band_params(self, band, min_weight, voxel_stride):
        p = L.BandParams()
        L.check(self._lib.op_volume_band_default_params(self._h, C.byref(p)))
        for k, val in (("band", band), ("min_weight", min_weight), ("voxel_stride", voxel_stride)):
            if val is not None:
                setattr(p, k, val)
        return p

    def BandVoxels(self, band=None, min_weight=None, voxel_stride=None, intensity=True):
        """The band voxels of this volume (op_volume_band_voxels): weight > 0 and >= min_weight, |sdf| <= band (0: the truncation), every
        voxel_stride-th voxel per axis (1, 2, 4, 8) -> (centres [n,3], sdf [n], intensity [n] or None) float32, blocks in pool order
        (GetCubeMap(sort=False)'s), voxels x + 8y + 64z ascending.  None = the default (2 voxels, 1, 1)."""
        p = self._band_params(band, min_weight, voxel_stride)
        n = C.c_size_t(0)
        L.check(self._lib.op_volume_band_voxels(self._h, C.byref(p), None, None, None, L.OP_MEM_HOST, 0, C.byref(n)))
        cap = n.value
        xyz, sdf = np.empty((cap, 3), np.float32), np.empty(cap, np.float32)
        y = np.empty(cap, np.float32) if intensity else None
        if cap:
            L.check(self._lib.op_volume_band_voxels(self._h, C.byref(p), C.c_void_p(xyz.ctypes.data), C.c_void_p(sdf.ctypes.data),
                                                    C.c_void_p(y.ctypes.data) if intensity else None, L.OP_MEM_HOST, cap, C.byref(n)))
        return xyz, sdf, y

    def OffsetRegistrationSystem(self, points, offset, intensity, T, max_distance, color_scale=0.0, max_color_residual=0.0, linearization=None, huber=None,
                                 huber_color=None, rows=False):
        """RobustRegistrationSystem with a target value per point (op_volume_register_offset_system): the residual starts from s - offset[i];
        the max_distance gate and sums[29] keep the stored sdf.  offset None IS RobustRegistrationSystem."""
        pts, o, y, ptr = self._offset_inputs(points, offset, intensity)
        Tm = _f32(T).reshape(16)
        opt = self._register_options(linearization, huber, huber_color)
        return self._registration_system(len(pts), 31, 7, 16, rows, lambda sums, counts, out: self._lib.op_volume_register_offset_system(
            self._h, ptr(pts), ptr(o), ptr(y), len(pts), L.OP_MEM_HOST, _fp(Tm), float(max_distance), float(color_scale), float(max_color_residual), C.byref(opt),
            sums, counts, out))

    def RegisterPointsOffset(self, points, offset, intensity=None, init_T=None, max_iterations=None, max_distance=None, min_step=None, min_points=None,
                             color_scale=None, max_color_residual=None, linearization=None, huber=None, huber_color=None):
        """RegisterPointsRobust with a target value per point (op_volume_register_offset_points) -> the same result dict.  offset None IS
        RegisterPointsRobust."""
        pts, o, y, ptr = self._offset_inputs(points, offset, intensity)
        if y is None and color_scale is None:
            color_scale = 0.0
        T0 = _f32(np.eye(4) if init_T is None else init_T).reshape(16)
        p = self._register_color_params(max_iterations, max_distance, min_step, min_points, color_scale, max_color_residual)
        opt, r = self._register_options(linearization, huber, huber_color), L.RegisterRobustResult()
        L.check(self._lib.op_volume_register_offset_points(self._h, ptr(pts), ptr(o), ptr(y), len(pts), L.OP_MEM_HOST, _fp(T0), C.byref(p), C.byref(opt), C.byref(r)))
        self._alive = []
        return self._register_robust_result(r)

    def RegisterVolume(self, source, init_T=None, band=None, min_weight=None, voxel_stride=None, max_iterations=None, max_distance=None, min_step=None,
                       min_points=None, color_scale=None, max_color_residual=None, linearization="gradient", huber=None, huber_color=None):
        """Registers the band voxels of the CubeHandler `source` against this volume from `init_T` (source to this; default identity)
        (op_volume_register_volume): each source voxel's own sdf is the value this volume's field should have at its centre -> the robust
        result dict with `selected`, T the refined source-to-target transform.  Selection None = the source's defaults (2 voxels, weight 1,
        stride 1); the linearisation defaults to "gradient" here; color_scale None = 1 (a source voxel carries its colour), 0 = geometric."""
        T0 = _f32(np.eye(4) if init_T is None else init_T).reshape(16)
        sel = source._band_params(band, min_weight, voxel_stride)
        p = self._register_color_params(max_iterations, max_distance, min_step, min_points, color_scale, max_color_residual)
        opt, r = self._register_options(linearization, huber, huber_color), L.RegisterVolumeResult()
        L.check(self._lib.op_volume_register_volume(self._h, source._h, _fp(T0), C.byref(sel), C.byref(p), C.byref(opt), C.byref(r)))
        self._alive = []
        out = self._register_robust_result(r.robust)
        out["selected"] = int(r.selected)
        return out

    # -- many clouds or frames in one call (op_volume_register_batch_*: every cloud follows the single entries' loop, the clouds of a round share a launch)
    @staticmethod
    def _batch_stats(st):
        return {k: int(getattr(st, k)) for k, _t in L.RegisterBatchStats._fields_}

    @staticmethod
    def _batch_inputs(points, starts, offset, intensity):
        pts, o, y, ptr = CubeHandler._offset_inputs(points, offset, intensity)
        st = np.ascontiguousarray(starts, dtype=np.uint64).reshape(-1)
        if len(st) < 1 or int(st[-1]) > len(pts):
            raise ValueError("starts holds n_clouds + 1 offsets into the points")
        return pts, o, y, ptr, st, len(st) - 1

    def BatchRegistrationSystem(self, points, starts, offset, intensity, T, max_distance, color_scale=0.0, max_color_residual=0.0, linearization=None,
                                huber=None, huber_color=None):
        """OffsetRegistrationSystem of many clouds in one launch (op_volume_register_batch_system): cloud c is points[starts[c]:starts[c + 1]]
        at its own T[c] -> (sums [n_clouds,31] float64, list of counts dicts), each bit for bit the single call's."""
        pts, o, y, ptr, st, n = self._batch_inputs(points, starts, offset, intensity)
        Tm = _f32(T).reshape(n, 16) if n else np.zeros((0, 16), np.float32)
        opt = self._register_options(linearization, huber, huber_color)
        sums, counts = np.zeros((n, 31), np.float64), np.zeros((n, 7), np.uint64)
        L.check(self._lib.op_volume_register_batch_system(self._h, ptr(pts), ptr(o), ptr(y), st.ctypes.data_as(L._u64p), n, L.OP_MEM_HOST, _fp(Tm), float(max_distance),
                                                          float(color_scale), float(max_color_residual), C.byref(opt),
                                                          sums.ctypes.data_as(C.POINTER(C.c_double)), counts.ctypes.data_as(L._u64p)))
        self._alive = []
        return sums, [dict(zip(self.ROBUST_COUNT_NAMES, (int(c) for c in row))) for row in counts]

    def RegisterPointsBatch(self, points, starts, offset=None, intensity=None, init_T=None, max_iterations=None, max_distance=None, min_step=None, min_points=None,
                            color_scale=None, max_color_residual=None, linearization=None, huber=None, huber_color=None):
        """RegisterPointsOffset of many clouds in one call (op_volume_register_batch_points): cloud c is points[starts[c]:starts[c + 1]], from
        init_T[c] ([n_clouds,4,4]; None: identities) -> (list of the result dicts RegisterPointsOffset returns, each bit for bit the single call's;
        stats dict: rounds, launches, evaluations, points)."""
        pts, o, y, ptr, st, n = self._batch_inputs(points, starts, offset, intensity)
        if y is None and color_scale is None:
            color_scale = 0.0
        T0 = _f32(np.tile(np.eye(4), (n, 1, 1)) if init_T is None else init_T).reshape(n, 16) if n else np.zeros((0, 16), np.float32)
        p = self._register_color_params(max_iterations, max_distance, min_step, min_points, color_scale, max_color_residual)
        opt, res, stats = self._register_options(linearization, huber, huber_color), (L.RegisterRobustResult * max(n, 1))(), L.RegisterBatchStats()
        L.check(self._lib.op_volume_register_batch_points(self._h, ptr(pts), ptr(o), ptr(y), st.ctypes.data_as(L._u64p), n, L.OP_MEM_HOST, _fp(T0), C.byref(p),
                                                          C.byref(opt), res, C.byref(stats)))
        self._alive = []
        return [self._register_robust_result(res[c]) for c in range(n)], self._batch_stats(stats)

    def RegisterFramesRobust(self, depths, rgbs, init_poses, pixel_stride=1, camera=None, max_iterations=None, max_distance=None, min_step=None, min_points=None,
                             color_scale=None, max_color_residual=None, linearization=None, huber=None, huber_color=None):
        """RegisterFrameRobust of many frames in one call (op_volume_register_batch_frames).  depths: [n,h,w] float32 or uint16, rgbs: [n,h,w,3]
        uint8 or None (geometric), both numpy arrays (or lists of images) or both contiguous CUDA torch tensors; init_poses [n,4,4]
        -> (list of the result dicts RegisterFrameRobust returns, each bit for bit the single call's; stats dict)."""
        if isinstance(depths, (list, tuple)):
            depths = np.stack([np.asarray(d) for d in depths]) if len(depths) else np.zeros((0, 1, 1), np.float32)
        if isinstance(rgbs, (list, tuple)):
            rgbs = np.stack([np.asarray(c) for c in rgbs]) if len(rgbs) else None
        n = int(depths.shape[0])
        if rgbs is not None and int(rgbs.shape[0]) != n:
            raise ValueError("one colour image per depth image")
        pd, fmt, pr, mem, keep = self._frame_images(depths, rgbs, "depths and rgbs")
        cam = camera if camera is not None else self.camera
        npx = cam.width * cam.height
        if n and (int(np.prod(depths.shape[1:])) != npx or (rgbs is not None and int(np.prod(rgbs.shape[1:])) != 3 * npx)):
            raise ValueError("the images do not have the camera's size")
        poses = _f32(init_poses).reshape(n, 16) if n else np.zeros((0, 16), np.float32)
        p = self._register_color_params(max_iterations, max_distance, min_step, min_points, color_scale, max_color_residual)
        opt, res, stats = self._register_options(linearization, huber, huber_color), (L.RegisterRobustResult * max(n, 1))(), L.RegisterBatchStats()
        L.check(self._lib.op_volume_register_batch_frames(self._h, C.byref(camera) if camera is not None else None, pd, npx * (2 if fmt == L.OP_DEPTH_U16 else 4), fmt,
                                                          pr, npx * 3, mem, int(pixel_stride), _fp(poses), n, C.byref(p), C.byref(opt), res, C.byref(stats)))
        del keep
        self._alive = []
        return [self._register_robust_result(res[f]) for f in range(n)], self._batch_stats(stats)

    def RaycastStats(self):
        """Measurement hook: what the last Raycast call did (op_volume_raycast_stats)."""
        v = [C.c_uint64(0) for _ in range(4)]
        L.check(self._lib.op_volume_raycast_stats(self._h, *[C.byref(x) for x in v]))
        return {"visible_blocks": v[0].value, "dropped_unloaded": v[1].value, "loaded_blocks": v[2].value, "marched_blocks": v[3].value}

    def SetRaycastPrune(self, on):
        """Extension (OP_VOLUME_OPT_RAYCAST_PRUNE): whether later views of the unchanged volume may drop blocks by what earlier views learnt
        about them (default on; the images are identical either way)."""
        L.check(self._lib.op_volume_set_option(self._h, L.OP_VOLUME_OPT_RAYCAST_PRUNE, 1 if on else 0))

    def WriteToFile(self, filename):
        L.check(self._lib.op_volume_write_file(self._h, str(filename).encode()))
        return True

    def ReadFromFile(self, filename):
        L.check(self._lib.op_volume_read_file(self._h, str(filename).encode(), 0))
        return True

    def ReadFromFileFloat(self, filename):
        L.check(self._lib.op_volume_read_file(self._h, str(filename).encode(), 1))
        return True

    def GetCubeID(self, point):
        """CubeHandler.h:185-189 / VoxelCube.h:63-74 (float floor, then floor-div by 8)."""
        p = _f32(point)
        pb = np.floor(p / np.float32(self._res)).astype(np.int64)
        return (pb >> 3).astype(np.int32)


def hash_key(x, y, z):
    """geometry::VoxelGridHasher (Geometry/Geometry.h:101-112)."""
    return int(L.load().op_hash_key(int(x), int(y), int(z)))


def mat4_inverse(m):
    m = _f32(m).reshape(16)
    out = np.empty(16, np.float32)
    L.check(L.load().op_mat4_inverse(_fp(m), _fp(out)))
    return out.reshape(4, 4)


def frustum_planes(camera, pose, far=5.0, near=0.5):
    pose = _f32(pose).reshape(16)
    out = np.empty(24, np.float32)
    L.check(L.load().op_frustum_planes(C.byref(camera), _fp(pose), far, near, _fp(out)))
    return out.reshape(6, 4)
