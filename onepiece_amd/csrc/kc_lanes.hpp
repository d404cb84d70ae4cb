// kc_lanes.hpp -- which lane of which wave of a k_integrate workgroup owns which voxel of the 8 x 8 x 8 block (integrate.hip).  Plain C++14: host code
// (tests/test_kc_lanes_cpu.py) includes it as it stands.
// The 64 lanes of a wave cover a sub-box of kBX x kBY x kBZ voxels, so that one gather instruction projects to a compact patch of the image whatever
// the view direction, and voxels behind one another share pixels (tools/kc_lane_footprint.py: distinct 128-byte lines per gather instruction).
// A thread's ZT voxels (its slots) keep (x, y) and lie kBZ apart in z: the partial sums of the pose rows over x and y stay shared.
// The storage layout is untouched: five planes per block, in-plane index x + 8 y + 64 z.
#pragma once

namespace kc_lanes {

constexpr int kBX = 8, kBY = 4, kBZ = 2;                                    // the sub-box of a wave's lanes: x fastest, then y, then z (profiles/kc_lanes_ab.txt)
constexpr int kNY = 8 / kBY, kNZ = 8 / kBZ;                                 // sub-boxes of the block along y and z
static_assert(kBX * kBY * kBZ == 64 && 8 % kBX == 0 && 8 % kBY == 0 && 8 % kBZ == 0, "a wave's lanes fill one sub-box of the block");
constexpr int kSlotStride = 64 * kBZ;                                       // in-plane distance of a thread's consecutive slots (floats)
constexpr int kRun = kBX == 8 ? 8 * kBY : kBX;                              // voxels of one contiguous run of a wave's plane access (4-byte words)

// sub-box number wave * ZT + slot -> z-box fastest, then y-box, then x-box: with ZT dividing kNZ a thread's slots differ in the z-box only
template <int ZT> constexpr int box(int wave, int slot) { static_assert(kNZ % ZT == 0, "a thread's slots are sub-boxes behind one another"); return wave * ZT + slot; }
template <int ZT> constexpr int vx(int wave, int slot, int lane) { return box<ZT>(wave, slot) / (kNZ * kNY) * kBX + lane % kBX; }
template <int ZT> constexpr int vy(int wave, int slot, int lane) { return box<ZT>(wave, slot) / kNZ % kNY * kBY + lane / kBX % kBY; }
template <int ZT> constexpr int vz(int wave, int slot, int lane) { return box<ZT>(wave, slot) % kNZ * kBZ + lane / (kBX * kBY); }
// in-plane offset of the voxel: offset(wave, slot, lane) = offset(wave, 0, lane) + slot * kSlotStride
template <int ZT> constexpr int offset(int wave, int slot, int lane) { return vx<ZT>(wave, slot, lane) + 8 * vy<ZT>(wave, slot, lane) + 64 * vz<ZT>(wave, slot, lane); }

} // namespace kc_lanes
