// voxel_interp.hpp -- VoxelCube::ReadVoxelInterpolate (Integration/VoxelCube.cpp:6-50) in pieces: the voxel fetch and the TSDFVoxel operators
// one lerp stage is made of.  Shared by CubeHandler::Transform (volume_ops.hip: k_transform_fill*) and the point queries (volume_sample.hip:
// OP_SAMPLE_REFERENCE).  One copy of the arithmetic.
#pragma once
#include "volume_core.hpp"

namespace opv {

__device__ __forceinline__ Vox5 default_voxel() { return Vox5{999.0f, 0.0f, -1.0f, -1.0f, -1.0f}; }

// cube_map.find(GetCubeID(p)) + GetVoxel(GetVoxelID(p)) (VoxelCube.h:63-67,81-86); default voxel if absent
static __device__ Vox5 fetch_voxel(const VolView& S, int px, int py, int pz) {
    const int cx = px >> 3, cy = py >> 3, cz = pz >> 3; // floor((p + 0.0) / 8)
    const int idx = table_find(S, cx, cy, cz);
    if (idx < 0) return default_voxel();
    const int vid = (px - cx * 8) + (py - cy * 8) * 8 + (pz - cz * 8) * 64;
    const float* t = S.pool + (size_t)idx * kBlockFloats + vid;
    return Vox5{t[0], t[kVox], t[2 * kVox], t[3 * kVox], t[4 * kVox]};
}
// TSDFVoxel::operator*(float) (TSDFVoxel.h:56-67)
__device__ __forceinline__ Vox5 vox_scale(const Vox5& a, float wgt) {
    if (wgt == 0 || a.w == 0) return default_voxel();
    return Vox5{a.s * wgt, a.w * wgt, a.c0 * wgt, a.c1 * wgt, a.c2 * wgt};
}
// TSDFVoxel::add (TSDFVoxel.h:40-51)
__device__ __forceinline__ Vox5 vox_add_direct(const Vox5& a, const Vox5& b) {
    if (a.w == 0) return b;
    if (b.w == 0) return a;
    return Vox5{a.s + b.s, a.w + b.w, a.c0 + b.c0, a.c1 + b.c1, a.c2 + b.c2};
}
// one stage of ReadVoxelInterpolate (VoxelCube.cpp:17-20):
// ((a * (1 - t)).add(b * t)) / ((1 - t) * (a.weight != 0) + t * (b.weight != 0))
__device__ __forceinline__ Vox5 interp_stage(const Vox5& a, const Vox5& b, float t) {
    if (!(a.w != 0 || b.w != 0)) return default_voxel();
    const Vox5 sum = vox_add_direct(vox_scale(a, 1 - t), vox_scale(b, t));
    const float d = (1 - t) * (float)(a.w != 0) + t * (float)(b.w != 0);
    return vox_scale(sum, 1 / d); // operator/(w) = operator*(1 / w) (TSDFVoxel.h:68-71)
}
// the seven stages over the taps v[k] = voxel at p0 + (k & 1, (k >> 1) & 1, (k >> 2) & 1), in ReadVoxelInterpolate's order
__device__ __forceinline__ Vox5 interp_taps(const Vox5 (&v)[8], float xw, float yw, float zw) {
    const Vox5 z1v = interp_stage(interp_stage(v[0], v[1], xw), interp_stage(v[2], v[3], xw), yw);
    const Vox5 z2v = interp_stage(interp_stage(v[4], v[5], xw), interp_stage(v[6], v[7], xw), yw);
    return interp_stage(z1v, z2v, zw);
}

} // namespace opv
