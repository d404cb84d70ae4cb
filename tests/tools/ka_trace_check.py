"""Run by tests/test_ka_cert_gpu.py in a fresh process: loads the -DKA_TRACE build of the library (argv[1]) through its C-ABI alone and prints, as one
JSON line, k_prepare_frames<true>'s two counters (wave passes over a pixel slot with a valid lane, those of them with an uncertified lane) and the
inside count of ComputeBounding for three 64 x 16 frames at depth 1.5 m: a centred camera with a rigid pose, the same with a projective bottom row
(no certificate), and a camera whose principal point lies on integers (column 0 and row 0 on the frustum's planes)."""
import ctypes as C
import json
import math
import sys

import numpy as np


class Camera(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("width", C.c_int32), ("height", C.c_int32), ("depth_scale", C.c_float)]


def main():
    lib = C.CDLL(sys.argv[1])
    fp = C.POINTER(C.c_float)
    lib.op_volume_create.argtypes = [C.POINTER(Camera), C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_uint64, C.POINTER(C.c_void_p)]
    lib.op_volume_compute_bounding.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, fp, fp, fp, C.POINTER(C.c_size_t)]
    lib.op_volume_destroy.argtypes = [C.c_void_p]
    lib.op_debug_ka_trace.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    w, h, f = 64, 16, 51.2
    a = 0.4
    rigid = np.array([[math.cos(a), 0, math.sin(a), 0.3], [0, 1, 0, -0.1], [-math.sin(a), 0, math.cos(a), 0.7], [0, 0, 0, 1]], np.float32)
    proj = rigid.copy(); proj[3] = (1e-3, -2e-3, 5e-4, 1.0)
    d = np.full((h, w), 1.5, np.float32)
    out = {}
    for name, cx, cy, pose in (("centred", (w - 1) / 2.0, (h - 1) / 2.0, rigid), ("projective", (w - 1) / 2.0, (h - 1) / 2.0, proj), ("integer", w / 2.0, h / 2.0, rigid)):
        cam, vol = Camera(f, f, cx, cy, w, h, 1000.0), C.c_void_p()
        assert lib.op_volume_create(C.byref(cam), 0.04, 0.1, 5.0, 0.5, 0, 0, C.byref(vol)) == 0
        cnt = (C.c_ulonglong * 2)()
        assert lib.op_debug_ka_trace(cnt, 1) == 0
        mx, mn, n = np.empty(3, np.float32), np.empty(3, np.float32), C.c_size_t(0)
        p = np.ascontiguousarray(pose.reshape(16))
        assert lib.op_volume_compute_bounding(vol, d.ctypes.data, 0, 0, p.ctypes.data_as(fp), mx.ctypes.data_as(fp), mn.ctypes.data_as(fp), C.byref(n)) == 0   # OP_DEPTH_F32, OP_MEM_HOST
        assert lib.op_debug_ka_trace(cnt, 1) == 0
        assert lib.op_volume_destroy(vol) == 0
        out[name] = [int(cnt[0]), int(cnt[1]), int(n.value)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
