"""Regenerates tests/golden/volume_ops_reference.npz: the inputs of tests/volume_golden_common.py and what the REFERENCE's own
integration::CubeHandler makes of them -- IntegrateImage / PrepareCubes, SetCubeMap, Transform, TransformNearest, Merge, GetPointCloud,
GenerateMeshByCube, ExtractTriangleMesh, AddCube, WriteToFile / ReadFromFile / ReadFromFileFloat, and its marching-cubes tables.  Build
container only: the reference's Integration/*.cpp and Geometry/{TriangleMesh,Geometry,PointCloud}.cpp are compiled where they lie, with
oracle/tools/volume_golden/main.cpp, against the cv::Mat stand-in of tests/tools/align_color_golden/opencv2 and the vendored Eigen / Sophus /
tinyply / nanoflann, with the reference's -std=c++11 -O3 -msse4.2, into oracle/_ref/volume_golden/.  Only data is written to the repository.
Not called from build(); the tests read the fixture only.

    python oracle/tools/gen_volume_golden.py"""
import glob
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import volume_golden_common as V  # noqa: E402

REF = "/root/reference"
_TYPES = [np.dtype(np.float32), np.dtype(np.int32), np.dtype(np.uint8), np.dtype(np.uint16), np.dtype(np.uint64)]
# the hand-built stream of tests/test_volume_ops_gpu.py::test_legacy_float_map_format
LEGACY_STREAM = np.array([123.0, 2.0, 1.0, -2.0, 3.0, 0.0, 5.0, 0.25, 3.0, 77.0, -0.5, 1.0, -2.0, 2.0, 5.0, 510.0, 255.0, 127.5, 2.0, 77.0, 30.0,
                          60.0, 90.0, 3.0, -4.0, 0.0, 9.0, 0.0, 0.0, 0.125, 1.0, -2.0, 0.0], np.float32)


def build():
    out = os.path.join(ROOT, "oracle", "_ref", "volume_golden")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "volume_golden")
    src = sorted(glob.glob(os.path.join(REF, "src", "Integration", "*.cpp")))
    src += [os.path.join(REF, "src", "Geometry", f) for f in ("TriangleMesh.cpp", "Geometry.cpp", "PointCloud.cpp")]
    inc = [os.path.join(ROOT, "tests", "tools", "align_color_golden"), os.path.join(REF, "src")]
    inc += [os.path.join(REF, "3rdparty", d) for d in ("Eigen", "Sophus", "tinyply/source", "nanoflann/include")]
    main = os.path.join(ROOT, "oracle", "tools", "volume_golden", "main.cpp")
    newest = max(os.path.getmtime(f) for f in [main] + glob.glob(os.path.join(inc[0], "opencv2", "**", "*.hpp"), recursive=True))
    if not os.path.exists(exe) or os.path.getmtime(exe) < newest:
        # -include set: MeshSimplification.h uses std::set without its header
        subprocess.check_call(["g++", "-std=c++11", "-O3", "-msse4.2", "-w", "-include", "set", "-ffunction-sections", "-fdata-sections"]
                              + ["-I" + i for i in inc] + [main] + src + ["-Wl,--gc-sections", "-pthread", "-o", exe])
    return exe


def write_bag(path, arrays):
    with open(path, "wb") as f:
        for name, a in arrays.items():
            a = np.ascontiguousarray(a)
            f.write(struct.pack("<I", len(name)) + name.encode() + struct.pack("<II", _TYPES.index(a.dtype), a.ndim))
            f.write(struct.pack("<%dQ" % a.ndim, *a.shape))
            f.write(a.tobytes())


def read_bag(path):
    out = {}
    with open(path, "rb") as f:
        while True:
            head = f.read(4)
            if not head:
                return out
            name = f.read(struct.unpack("<I", head)[0]).decode()
            t, rank = struct.unpack("<II", f.read(8))
            dims = struct.unpack("<%dQ" % rank, f.read(8 * rank))
            n = int(np.prod(dims, dtype=np.int64)) if rank else 1
            out[name] = np.frombuffer(f.read(n * _TYPES[t].itemsize), _TYPES[t]).reshape(dims).copy()


def run(exe, arrays):
    with tempfile.TemporaryDirectory() as tmp:
        write_bag(os.path.join(tmp, "in"), arrays)
        subprocess.check_call([exe, os.path.join(tmp, "in"), os.path.join(tmp, "out"), tmp])
        return read_bag(os.path.join(tmp, "out"))


def store(fixture, case, arrays_in, arrays_out, skip_in=()):
    """inputs as they are; of every block set the keys, and the voxels (at most FULL_BLOCKS blocks) or one hash per block"""
    for k, a in arrays_in.items():
        if k not in skip_in:
            fixture[case + "/in/" + k] = a
    for k, a in arrays_out.items():
        if k.endswith("/voxels") and len(a) > V.FULL_BLOCKS:
            fixture[case + "/out/" + k[:-len("voxels")] + "hash"] = V.block_hashes(a)
        else:
            fixture[case + "/out/" + k] = a


def generate(exe):
    fx = {}
    store(fx, "tables", {"tables": np.zeros(1, np.int32)}, run(exe, {"tables": np.zeros(1, np.int32)}))
    fused = None
    for name, case in V.fusion_cases().items():
        out = run(exe, case)
        assert all(len(out["frame%d/cube_id_list" % k]) for k in range(len(case["poses"]))), name  # (an empty frame is LEFT_OUT: undefined)
        store(fx, "fusion/" + name, case, out)
        if name == "u16_40x30_res004_two_frames":
            last = len(case["poses"]) - 1
            fused = (case["params"], out["frame%d/keys" % last], out["frame%d/voxels" % last])
    flag = np.zeros(1, np.int32)
    hp, hk, hv = V.hand_volume()
    for name, (p, k, v) in (("hand", (hp, hk, hv)), ("fused", fused)):
        ask = {"params": p, "keys": k, "voxels": v, "transforms": V.transforms(p[7]), "point_cloud": flag, "mesh": flag, "map_file": flag,
               "add_cubes": np.array([[100, -100, 7], k[0], [100, -100, 7], [-3, 0, 0]], np.int32)}
        store(fx, "volume/" + name, ask, run(exe, ask))
    ok, ov = V.merge_other(hk, hv)
    other = {"params": hp, "keys": hk, "voxels": hv, "other_params": hp, "other_keys": ok, "other_voxels": ov}
    hand_in = ("keys", "voxels")  # stored once, under volume/hand
    store(fx, "merge/overlapping_and_disjoint", other, run(exe, other), skip_in=hand_in)
    refused = dict(other, other_params=np.concatenate([hp[:7], [np.float32(0.04)], hp[8:]]).astype(np.float32))
    store(fx, "merge/refused_resolution_mismatch", refused, run(exe, refused), skip_in=hand_in + ("other_keys", "other_voxels"))
    moved = dict(other, merge_transform=V.transforms(hp[7])[4])
    store(fx, "merge/with_transform", moved, run(exe, moved), skip_in=hand_in + ("other_keys", "other_voxels"))
    legacy = {"params": hp, "keys": hk[:0], "voxels": hv[:0], "legacy_stream": LEGACY_STREAM}
    store(fx, "legacy", legacy, run(exe, legacy))
    return fx


def main():
    exe = build()
    a, b = generate(exe), generate(exe)
    assert a.keys() == b.keys() and all(np.array_equal(V.canonical_bits(a[k]) if a[k].dtype == np.float32 else a[k],
                                                       V.canonical_bits(b[k]) if b[k].dtype == np.float32 else b[k]) for k in a), "two runs differ"
    np.savez_compressed(V.FIXTURE, **a)
    print("wrote %s (%d arrays, %d bytes)" % (V.FIXTURE, len(a), os.path.getsize(V.FIXTURE)))


if __name__ == "__main__":
    main()
