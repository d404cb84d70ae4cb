"""k_integrate's lane map (onepiece_amd/csrc/kc_lanes.hpp): which lane of which wave of a workgroup owns which voxel of the 8 x 8 x 8 block.

A tiny host program is compiled against the header and prints the map for ZT = 2 (four waves, two slots per thread); the properties the kernel
relies on are checked on that table:
  * (wave, slot, lane) -> in-plane offset is a bijection onto 0 .. 511 and equals x + 8 y + 64 z with coordinates in 0 .. 7;
  * a thread's two slots share (x, y) and lie kSlotStride words apart (the kernel addresses slot 1 by that constant);
  * the lanes of a wave cover one kBX x kBY x kBZ sub-box per slot;
  * a wave's plane access is made of whole aligned runs of kRun consecutive words, read by consecutive lanes in ascending order
    (so two swapped lanes fail here even though they keep the bijection).
The kept map is pinned by EXPECT: changing the header without a measurement behind it fails the first test."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZT, WAVES = 2, 4
EXPECT = {"kBX": 8, "kBY": 4, "kBZ": 2, "kSlotStride": 128, "kRun": 32}

PROGRAM = r"""
#include <cstdio>
#include "kc_lanes.hpp"
int main() {
    using namespace kc_lanes;
    std::printf("%d %d %d %d %d\n", kBX, kBY, kBZ, kSlotStride, kRun);
    for (int w = 0; w < 4; ++w)
        for (int s = 0; s < 2; ++s)
            for (int l = 0; l < 64; ++l) std::printf("%d %d %d %d\n", vx<2>(w, s, l), vy<2>(w, s, l), vz<2>(w, s, l), offset<2>(w, s, l));
    static_assert(offset<2>(0, 0, 0) == 0 && vz<2>(0, 1, 0) == kBZ, "usable in constant expressions");
    return 0;
}
"""


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    d = tmp_path_factory.mktemp("kc_lanes")
    src, exe = d / "lanes.cpp", d / "lanes"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "onepiece_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split("\n")
    consts = dict(zip(("kBX", "kBY", "kBZ", "kSlotStride", "kRun"), map(int, out[0].split())))
    t = np.array([[int(v) for v in line.split()] for line in out[1:] if line], dtype=np.int64).reshape(WAVES, ZT, 64, 4)
    return consts, t


def check_map(consts, t):
    """Every property of the docstring; raises AssertionError."""
    bx, by, bz, stride, run = (consts[k] for k in ("kBX", "kBY", "kBZ", "kSlotStride", "kRun"))
    x, y, z, off = t[..., 0], t[..., 1], t[..., 2], t[..., 3]
    assert bx * by * bz == 64 and stride == 64 * bz
    for c in (x, y, z):
        assert c.min() == 0 and c.max() == 7
    assert np.array_equal(off, x + 8 * y + 64 * z)
    assert np.array_equal(np.sort(off.ravel()), np.arange(512))
    assert np.array_equal(x[:, 0], x[:, 1]) and np.array_equal(y[:, 0], y[:, 1])
    assert np.array_equal(off[:, 1], off[:, 0] + stride) and np.array_equal(z[:, 1], z[:, 0] + bz)
    for w in range(WAVES):
        for s in range(ZT):
            ext = [np.unique(c[w, s]) for c in (x, y, z)]
            assert [len(e) for e in ext] == [bx, by, bz]                         # a full sub-box ...
            assert all(e[0] % len(e) == 0 and e[-1] - e[0] == len(e) - 1 for e in ext)   # ... aligned to its own size
            o = off[w, s].reshape(64 // run, run)                                # consecutive lanes, run by run
            assert np.all(o[:, 0] % run == 0)                                    # aligned (run words = 4 run bytes)
            assert np.array_equal(o, o[:, :1] + np.arange(run))                  # whole, ascending with the lane


def test_the_kept_map_has_the_properties_the_kernel_relies_on(table):
    consts, t = table
    assert consts == EXPECT
    check_map(consts, t)


def test_the_voxel_of_every_lane_is_the_one_the_design_states(table):
    consts, t = table
    bx, by, bz = consts["kBX"], consts["kBY"], consts["kBZ"]
    ny, nz = 8 // by, 8 // bz
    for w in range(WAVES):
        for s in range(ZT):
            box = w * ZT + s                                                     # z-box fastest, then y-box, then x-box
            for l in range(64):
                want = (box // (nz * ny) * bx + l % bx, box // nz % ny * by + l // bx % by, box % nz * bz + l // (bx * by))
                assert tuple(t[w, s, l, :3]) == want


def test_swapped_lanes_and_a_shifted_slot_are_caught(table):
    consts, t = table
    bad = t.copy()
    bad[1, 0, [5, 6]] = bad[1, 0, [6, 5]]                                        # still a bijection
    with pytest.raises(AssertionError):
        check_map(consts, bad)
    bad = t.copy()
    bad[2, 1, :, 0] = (bad[2, 1, :, 0] + 1) % 8                                  # slot 1 of a wave in other columns than slot 0
    bad[2, 1, :, 3] = bad[2, 1, :, 0] + 8 * bad[2, 1, :, 1] + 64 * bad[2, 1, :, 2]
    with pytest.raises(AssertionError):
        check_map(consts, bad)
