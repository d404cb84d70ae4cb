// voxel_interp.hpp -- the reference's arithmetic on TSDFVoxels, once: the plane access of a voxel in the pool, TSDFVoxel::operator+ with general
// weights (voxel_merge), and VoxelCube::ReadVoxelInterpolate (Integration/VoxelCube.cpp:6-50) in pieces -- the voxel fetch and the TSDFVoxel
// operators one lerp stage is made of.  Users: CubeHandler::Merge (volume_ops.hip: k_merge_blocks; volume_merge_transformed.hip: k_merge_fill),
// CubeHandler::Transform (transform_body.hpp, the body of k_transform_fill_wave and k_merge_fill; volume_ops.hip: k_transform_fill, the nearest
// form) and the point queries (volume_sample.hip: OP_SAMPLE_REFERENCE).  Also here, because the same kernels share it: the decode of
// k_insert_keys' coded slot.
#pragma once
#include "volume_core.hpp"

namespace opv {

__device__ __forceinline__ Vox5 default_voxel() { return Vox5{999.0f, 0.0f, -1.0f, -1.0f, -1.0f}; }

// the five planes of one voxel of a block (pool or LDS copy): t points at its sdf, plane p is t[p * kVox]
__device__ __forceinline__ Vox5 load_planes(const float* t) { return Vox5{t[0], t[kVox], t[2 * kVox], t[3 * kVox], t[4 * kVox]}; }
__device__ __forceinline__ void store_planes(float* t, const Vox5& v) {
    t[0] = v.s; t[kVox] = v.w; t[2 * kVox] = v.c0; t[3 * kVox] = v.c1; t[4 * kVox] = v.c2;
}

// voxels[id] += b on the planes at t: TSDFVoxel::operator+ with general weights (TSDFVoxel.h:24-39), or a plain copy when the block was just
// created (`fresh`: CubeHandler::Merge assigns the whole cube, CubeHandler.h:160-163).  note(kind) is called inside the branch taken.
enum { kMergeCopied = 0, kMergeKept = 1, kMergeBlended = 2, kMergeReset = 3 };
template <class Note>
__device__ __forceinline__ void voxel_merge(float* t, const Vox5& b, bool fresh, Note note) {
    const float tw = t[kVox];
    if (fresh || tw == 0) { store_planes(t, b); note(kMergeCopied); return; } // copy / "weight == 0 -> return other"
    if (b.w == 0) { note(kMergeKept); return; }
    const float w = tw + b.w;
    if (w != 0) {
        const Vox5 a = load_planes(t);
        t[0] = (tw * a.s + b.w * b.s) / w;
        t[2 * kVox] = (tw * a.c0 + b.w * b.c0) / w;
        t[3 * kVox] = (tw * a.c1 + b.w * b.c1) / w;
        t[4 * kVox] = (tw * a.c2 + b.w * b.c2) / w;
        note(kMergeBlended);
    } else { // the default voxel but for its weight, which is w (= 0) below
        const Vox5 d = default_voxel();
        t[0] = d.s; t[2 * kVox] = t[3 * kVox] = t[4 * kVox] = d.c2;
        note(kMergeReset);
    }
    t[kVox] = w;
}

// The slot k_insert_keys left for a key that has one (the kernels leave on -1, "none", before they come here): the table slot, or
// -(slot + 2) when that insert created it (*fresh, where asked for).  Returns the pool slot (through tvals; < 0: none).
__device__ __forceinline__ int slot_to_pool(int idx, const int* __restrict__ tvals, bool* fresh = nullptr) {
    const bool created = idx <= -2;
    if (created) idx = -(idx + 2);
    if (fresh) *fresh = created;
    return tvals[idx];
}

// cube_map.find(GetCubeID(p)) + GetVoxel(GetVoxelID(p)) (VoxelCube.h:63-67,81-86); default voxel if absent
static __device__ Vox5 fetch_voxel(const VolView& S, int px, int py, int pz) {
    const int cx = px >> 3, cy = py >> 3, cz = pz >> 3; // floor((p + 0.0) / 8)
    const int idx = table_find(S, cx, cy, cz);
    if (idx < 0) return default_voxel();
    const int vid = (px - cx * 8) + (py - cy * 8) * 8 + (pz - cz * 8) * 64;
    return load_planes(S.pool + (size_t)idx * kBlockFloats + vid);
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
