"""op_volume_register_batch_* without a device: the header, the bindings and their signatures, the struct's layout, every refusal (decided before
any device use: the volume handed in is a pointer that must never be looked at), n_clouds == 0, and the restated round scheduler
(tests/volume_register_batch_common.py) pinned on a hand case."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import volume_register_batch_common as BT

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("op_volume_register_batch_system", "op_volume_register_batch_points", "op_volume_register_batch_frames")


def test_bindings_signatures_and_struct_layout(hip, tmp_path):
    """(fails on a library without the batch entries)"""
    lib = hip.load()
    text = open(os.path.join(ROOT, "include", "onepiece_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in hip.SIGNATURES and hasattr(lib, name), name
    assert lib.op_abi_version() == 1
    vp, fp, u64p, dp = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    par, opt, res, st = (C.POINTER(t) for t in (hip.RegisterColorParams, hip.RegisterOptions, hip.RegisterRobustResult, hip.RegisterBatchStats))
    assert hip.SIGNATURES["op_volume_register_batch_system"] == (C.c_int, [vp, vp, vp, vp, u64p, C.c_size_t, C.c_int, fp, C.c_float, C.c_float, C.c_float, opt, dp, u64p])
    assert hip.SIGNATURES["op_volume_register_batch_points"] == (C.c_int, [vp, vp, vp, vp, u64p, C.c_size_t, C.c_int, fp, par, opt, res, st])
    assert hip.SIGNATURES["op_volume_register_batch_frames"] == (C.c_int, [vp, C.POINTER(hip.Camera), vp, C.c_size_t, C.c_int, vp, C.c_size_t, C.c_int, C.c_int, fp, C.c_size_t,
                                                                           par, opt, res, st])
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "onepiece_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", '
                   "sizeof(op_volume_register_batch_stats), offsetof(op_volume_register_batch_stats, rounds), offsetof(op_volume_register_batch_stats, launches), "
                   "offsetof(op_volume_register_batch_stats, evaluations), offsetof(op_volume_register_batch_stats, points)); return 0; }\n")
    exe = tmp_path / "sizes.bin"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = hip.RegisterBatchStats
    assert sizes == [C.sizeof(S), S.rounds.offset, S.launches.offset, S.evaluations.offset, S.points.offset] == [24, 0, 4, 8, 16]
    from onepiece_amd import integration as I
    for name in ("RegisterFramesRobust", "RegisterPointsBatch", "BatchRegistrationSystem"):
        assert callable(getattr(I.CubeHandler, name)), name


def test_refusals_and_the_empty_batch_without_a_device(hip):
    lib = hip.load()
    n = 3
    pts, y, off = np.zeros((12, 3), F32), np.zeros(12, F32), np.zeros(12, F32)
    starts = np.array([0, 4, 4, 12], np.uint64)
    down = np.array([0, 8, 4, 12], np.uint64)
    T = np.tile(np.eye(4, dtype=F32).reshape(16), (n, 1))
    depth, rgb = np.ones((n, 4, 4), F32), np.zeros((n, 4, 4, 3), np.uint8)
    sums, counts = np.full((n, 31), 7.0), np.full((n, 7), 7, np.uint64)
    res = (hip.RegisterRobustResult * n)()
    for r in res:
        r.color.base.iterations = 77
    stats = hip.RegisterBatchStats(7, 7, 7, 7)
    par = lambda it=5, cs=1.0: hip.RegisterColorParams(hip.RegisterParams(it, 0.1, 0.0, 6), cs, 0.0)
    opt = lambda lin=2, h=0.0, hc=0.0: hip.RegisterOptions(lin, h, hc)
    p = lambda a: C.c_void_p(a.ctypes.data)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    dp = sums.ctypes.data_as(C.POINTER(C.c_double))
    fake = C.c_void_p(0x1000)                                          # a non-NULL volume that must never be looked at
    H, cam, F, U = hip.OP_MEM_HOST, hip.Camera(50, 50, 2, 2, 4, 4, 1000), hip.OP_DEPTH_F32, hip.OP_DEPTH_U16
    sysc = lambda v=fake, x=p(pts), o=p(off), yy=p(y), st=u64(starts), nc=n, mem=H, t=fp(T), cs=1.0, s=dp, op=None: lib.op_volume_register_batch_system(
        v, x, o, yy, st, nc, mem, t, 0.1, cs, 0.0, C.byref(op or opt()), s, u64(counts))
    ptsc = lambda v=fake, x=p(pts), o=p(off), yy=p(y), st=u64(starts), nc=n, mem=H, t=fp(T), pr=None, r=res, op=None: lib.op_volume_register_batch_points(
        v, x, o, yy, st, nc, mem, t, C.byref(pr or par()), C.byref(op or opt()), r, C.byref(stats))
    frames = lambda v=fake, d=p(depth), ds=64, fmt=F, c=p(rgb), cs=48, mem=H, stride=1, t=fp(T), nf=n, pr=None, r=res, op=None: lib.op_volume_register_batch_frames(
        v, C.byref(cam), d, ds, fmt, c, cs, mem, stride, t, nf, C.byref(pr or par()), C.byref(op or opt()), r, C.byref(stats))
    nan, inf = float("nan"), float("inf")
    cases = {
        "system: null volume": lambda: sysc(v=None),
        "system: null starts": lambda: sysc(st=None),
        "system: decreasing starts": lambda: sysc(st=u64(down)),
        "system: null T": lambda: sysc(t=None),
        "system: null sums": lambda: sysc(s=None),
        "system: null xyz": lambda: sysc(x=None),
        "system: null intensity": lambda: sysc(yy=None),
        "system: bad mem": lambda: sysc(mem=2),
        "system: color_scale < 0": lambda: sysc(cs=-1.0),
        "system: color_scale NaN": lambda: sysc(cs=nan),
        "system: linearization 3": lambda: sysc(op=opt(lin=3)),
        "system: huber < 0": lambda: sysc(op=opt(h=-0.01)),
        "system: huber_color inf, color_scale 0": lambda: sysc(cs=0.0, op=opt(hc=inf)),
        "points: null volume": lambda: ptsc(v=None),
        "points: null starts": lambda: ptsc(st=None),
        "points: decreasing starts": lambda: ptsc(st=u64(down)),
        "points: null init_T": lambda: ptsc(t=None),
        "points: null results": lambda: ptsc(r=None),
        "points: null xyz": lambda: ptsc(x=None),
        "points: null intensity": lambda: ptsc(yy=None),
        "points: null intensity, default params": lambda: lib.op_volume_register_batch_points(fake, p(pts), None, None, u64(starts), n, H, fp(T), None, None, res, None),
        "points: bad mem": lambda: ptsc(mem=-1),
        "points: max_iterations < 0": lambda: ptsc(pr=par(it=-1)),
        "points: color_scale < 0": lambda: ptsc(pr=par(cs=-0.5)),
        "points: linearization 7": lambda: ptsc(op=opt(lin=7)),
        "points: huber_color NaN": lambda: ptsc(op=opt(hc=nan)),
        "frames: null volume": lambda: frames(v=None),
        "frames: null results": lambda: frames(r=None),
        "frames: null depth": lambda: frames(d=None),
        "frames: null init_poses": lambda: frames(t=None),
        "frames: bad mem": lambda: frames(mem=3),
        "frames: bad depth format": lambda: frames(fmt=9),
        "frames: pixel_stride 0": lambda: frames(stride=0),
        "frames: depth stride smaller than an image": lambda: frames(ds=60),
        "frames: u16 depth stride smaller than an image": lambda: frames(fmt=U, ds=30),
        "frames: depth stride no multiple of four bytes": lambda: frames(ds=66),
        "frames: rgb stride smaller than an image": lambda: frames(cs=47),
        "frames: max_iterations < 0": lambda: frames(pr=par(it=-1)),
        "frames: color_scale inf": lambda: frames(pr=par(cs=inf)),
        "frames: linearization 3, no rgb": lambda: frames(c=None, op=opt(lin=3)),
        "frames: huber inf": lambda: frames(op=opt(h=inf)),
    }
    for what, call in cases.items():
        assert call() == hip.OP_ERR_INVALID, what
        assert lib.op_last_error().startswith(b"op_volume_register_batch_%s:" % what.split(":")[0].encode()), (what, lib.op_last_error())   # the entry's own name
    # the empty batch: OP_OK, nothing written, the volume not looked at
    assert sysc(nc=0) == hip.OP_OK and ptsc(nc=0) == hip.OP_OK and frames(nf=0) == hip.OP_OK
    assert (sums == 7.0).all() and (counts == 7).all() and all(r.color.base.iterations == 77 for r in res)
    assert (stats.rounds, stats.launches, stats.evaluations, stats.points) == (7, 7, 7, 7)


def test_the_scheduler_on_a_hand_case():
    """five clouds whose own loops make 4, 1, 2, 4 and 1 evaluations (1: TOO_FEW_POINTS on the first, or max_iterations 0); cloud 4 has no point"""
    evaluations, points = [4, 1, 2, 4, 1], [300, 10, 70000, 1, 0]
    assert BT.rounds_of(evaluations) == [[0, 1, 2, 3, 4], [0, 2, 3], [0, 3], [0, 3]]
    assert BT.stats_of(evaluations, points) == dict(rounds=4, launches=8, evaluations=12, points=70311)
    # a stopped cloud costs nothing more: the evaluations of a round are the clouds still in it
    assert [len(r) for r in BT.rounds_of(evaluations)] == [5, 3, 2, 2] and sum(len(r) for r in BT.rounds_of(evaluations)) == sum(evaluations)
    # rounds in which only pointless clouds are left launch nothing
    assert BT.stats_of([1, 3], [50, 0]) == dict(rounds=3, launches=2, evaluations=4, points=50)
    assert BT.stats_of([], []) == dict(rounds=0, launches=0, evaluations=0, points=0)
    assert BT.rounds_of([0, 0]) == []
    # the workgroups of a cloud: RegRun::open's formula
    assert [BT.workgroups(n) for n in (0, 1, 256, 257, 262144, 262145, 10 ** 7)] == [0, 1, 1, 2, 1024, 1024, 1024]
