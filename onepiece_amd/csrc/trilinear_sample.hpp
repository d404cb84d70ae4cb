// trilinear_sample.hpp -- the raycaster's strict trilinear sample (include/onepiece_hip.h, op_volume_raycast: "sample"), shared by the raycaster
// (raycast.hip: the LDS march, its rare previous-sample lookups, the shading pass), the point queries (volume_sample.hip: OP_SAMPLE_TRILINEAR
// and its gradient) and the registration against the field (volume_register.hip: residual and normal).  One copy of the arithmetic: same
// operations, same order, every product and sum rounded separately.
// `View` is whatever carries inv_res = 1.0f / res (the raycaster's RcView, the point queries' SampleView, the registration's RegView).
#pragma once
#include "volume_core.hpp"

namespace opv {

// base voxel i = floor(g), fraction f = g - floor(g) of g = p * (1 / res) - 0.5
struct RcCell { int i0, i1, i2; float f0, f1, f2; };
template <class View>
__device__ __forceinline__ RcCell rc_cell(const View& W, float x, float y, float z) {
    const float g0 = x * W.inv_res - 0.5f, g1 = y * W.inv_res - 0.5f, g2 = z * W.inv_res - 0.5f;
    const float b0 = floorf(g0), b1 = floorf(g1), b2 = floorf(g2);
    return RcCell{(int)b0, (int)b1, (int)b2, g0 - b0, g1 - b1, g2 - b2};
}
// weight of tap k = i + (k & 1, (k >> 1) & 1, (k >> 2) & 1)
__device__ __forceinline__ float rc_weight(const RcCell& c, int k) {
    const float wx = (k & 1) ? c.f0 : 1.0f - c.f0, wy = (k & 2) ? c.f1 : 1.0f - c.f1, wz = (k & 4) ? c.f2 : 1.0f - c.f2;
    return (wx * wy) * wz;
}

struct BlockCache { int cx, cy, cz, idx; }; // a lane's last block: id -> pool slot (< 0: absent)

// the point queries' range rule (volume_sample.hip, volume_register.hip): decided before any conversion to int
constexpr float kSampleLimit = 8388600.0f; // |g| below this: floor(g) and floor(g) + 1 convert exactly and their block ids lie inside kCoordLimit
static_assert((8388600 + 1) / 8 < kCoordLimit, "taps -8388600 .. 8388601: every block id of an in-range sample is a legal one");
__device__ __forceinline__ bool sample_in_range(float g0, float g1, float g2) { // false for NaN
    return fabsf(g0) < kSampleLimit && fabsf(g1) < kSampleLimit && fabsf(g2) < kSampleLimit;
}

// trilinear sample through the hash (the march's rare previous-sample lookups, k_rc_finish, the point queries): false = not all 8 voxels observed
// (a tap in no held block, or of weight <= 0 or NaN)
template <bool COL, class View>
__device__ bool rc_sample_global(const VolView& V, const View& W, BlockCache& bc, float x, float y, float z, float* sdf, float* col) {
    const RcCell c = rc_cell(W, x, y, z);
    float acc = 0, a0 = 0, a1 = 0, a2 = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int px = c.i0 + (k & 1), py = c.i1 + ((k >> 1) & 1), pz = c.i2 + ((k >> 2) & 1);
        const int bx = px >> 3, by = py >> 3, bz = pz >> 3;
        if (!(bx == bc.cx && by == bc.cy && bz == bc.cz)) { bc.cx = bx; bc.cy = by; bc.cz = bz; bc.idx = table_find(V, bx, by, bz); }
        if (bc.idx < 0) return false;
        const float* t = V.pool + (size_t)bc.idx * kBlockFloats + ((px - bx * 8) + (py - by * 8) * 8 + (pz - bz * 8) * 64);
        if (!(t[kVox] > 0)) return false;
        const float w = rc_weight(c, k);
        acc += w * t[0];
        if (COL) { a0 += w * t[2 * kVox]; a1 += w * t[3 * kVox]; a2 += w * t[4 * kVox]; } // colour planes only at the hit / where voxels are asked for
    }
    *sdf = acc;
    if (COL) { col[0] = a0; col[1] = a1; col[2] = a2; }
    return true;
}

} // namespace opv
