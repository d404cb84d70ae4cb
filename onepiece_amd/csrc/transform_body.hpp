// transform_body.hpp -- the two passes of CubeHandler::Transform (Integration/CubeHandler.h:199-298) as device bodies, shared by the kernels that
// resample into a NEW volume (volume_ops.hip: k_transform_alloc, k_transform_fill_wave) and by the ones that resample straight into an existing
// one (volume_merge_transformed.hip: k_merge_claim, k_merge_fill).  One copy of the positions, the claim set and the taps.
#pragma once
#include "volume_core.hpp"
#include "voxel_interp.hpp"

namespace opv {

// pass 1: AddTransformedCube / AddTransformedCubeNearest (CubeHandler.h:199-241), executed with the RESULT's CubePara (alloc_res), for the source
// block with id (kx, ky, kz), by a workgroup of 512 threads (one per voxel).  A block's 512 voxels land in a handful of result blocks: the
// workgroup gathers the distinct ids in a small LDS set and claims each ONCE (a voxel-by-voxel claim was ~2 000 hash probes per source block,
// most of them for ids another voxel had just entered).  claim(cx, cy, cz) is what AddCube means to the caller; s_set is the caller's LDS.
constexpr int kClaimSet = 128; // slots of the set (a power of two); a workgroup whose voxels reach more distinct blocks claims the overflow directly
template <bool NEAREST, class Claim>
__device__ __forceinline__ void transform_claim_body(unsigned long long* s_set, int kx, int ky, int kz, State* dst_state, const float* M, float alloc_res, Claim claim) {
    const int vid = threadIdx.x;
    if (vid < kClaimSet) s_set[vid] = kEmptyKey;
    __syncthreads();
    const float half = alloc_res / 2;
    const float px = ((float)kx * 8.0f) * alloc_res + ((float)(vid & 7) * alloc_res + half);
    const float py = ((float)ky * 8.0f) * alloc_res + ((float)((vid >> 3) & 7) * alloc_res + half);
    const float pz = ((float)kz * 8.0f) * alloc_res + ((float)(vid >> 6) * alloc_res + half);
    const float q0 = ((M[0] * px + M[1] * py) + M[2] * pz) + M[3] * 1.0f;
    const float q1 = ((M[4] * px + M[5] * py) + M[6] * pz) + M[7] * 1.0f;
    const float q2 = ((M[8] * px + M[9] * py) + M[10] * pz) + M[11] * 1.0f;
    const float q3 = ((M[12] * px + M[13] * py) + M[14] * pz) + M[15] * 1.0f;
    const float n0 = NEAREST ? q0 / q3 : q0 / q3 - half, n1 = NEAREST ? q1 / q3 : q1 / q3 - half,
                n2 = NEAREST ? q2 / q3 : q2 / q3 - half;
    const int p0 = (int)floorf(n0 / alloc_res), p1 = (int)floorf(n1 / alloc_res), p2 = (int)floorf(n2 / alloc_res);
    int lx = INT_MIN, ly = INT_MIN, lz = INT_MIN;
#pragma unroll
    for (int k = 0; k < (NEAREST ? 1 : 8); ++k) {
        const int cx = (p0 + (k & 1)) >> 3, cy = (p1 + ((k >> 1) & 1)) >> 3, cz = (p2 + ((k >> 2) & 1)) >> 3;
        if (cx == lx && cy == ly && cz == lz) continue;
        lx = cx; ly = cy; lz = cz;
        if (!key_in_range(cx, cy, cz)) { atomicOr(&dst_state->overflow, 8u); continue; }
        // enter the id into the workgroup's set; a full set (never, for a rigid motion) falls back to the direct claim
        const unsigned long long key = pack_key(cx, cy, cz);
        unsigned sl = (unsigned)(hash_key_dev(cx, cy, cz) * 0x9E3779B97F4A7C15ULL >> 57) & (kClaimSet - 1);
        bool placed = false;
        for (int probe = 0; probe < kClaimSet; ++probe, sl = (sl + 1) & (kClaimSet - 1)) {
            const unsigned long long cur = s_set[sl];
            if (cur == key) { placed = true; break; }
            if (cur == kEmptyKey) {
                const unsigned long long old = atomicCAS(&s_set[sl], kEmptyKey, key);
                if (old == kEmptyKey || old == key) { placed = true; break; }
            }
        }
        if (!placed) claim(cx, cy, cz);
    }
    __syncthreads();
    if (vid < kClaimSet && s_set[vid] != kEmptyKey) {
        const unsigned long long key = s_set[vid];
        claim((int)(key >> 42) - kCoordLimit, (int)((key >> 21) & 0x1FFFFFull) - kCoordLimit, (int)(key & 0x1FFFFFull) - kCoordLimit); // AddCube
    }
}

// pass 2, trilinear, for ONE WAVE and the result block with id (kx, ky, kz) (eight z-slices of 64 voxels in turn): every voxel of the block reads
// the source through trans^-1 (CubeHandler.h:257-294) with the SOURCE's CubePara (src_res).  The taps of a block's 512 voxels fall into a few
// source blocks (a rotated 8^3 cube spans at most three per axis): the wave takes the bounding box of its taps in block coordinates by a shuffle
// reduction, looks every block of the box up ONCE (up to kSrcBox of them) into its own LDS words s_slot, and the taps index that table -- eight
// hash probes per voxel become none.  A box beyond kSrcBox blocks (a projective `trans`, NaN) probes per tap.  An int overflow of p + 1 only
// ever widens the box: fallback.  put(zs, r) receives ReadVoxelInterpolate's result for voxel lane + 64 zs, zs = 0..7 in order.
// UNROLL: how many slices the tap loop holds at once (2 for a body whose put only stores; 8 where put indexes registers by zs).
constexpr int kSrcBox = 64;
__device__ __forceinline__ Vox5 load_voxel(const VolView& S, int idx, int px, int py, int pz) {
    if (idx < 0) return default_voxel();
    return load_planes(S.pool + (size_t)idx * kBlockFloats + ((px & 7) + (py & 7) * 8 + (pz & 7) * 64));
}
template <int UNROLL, class Put>
__device__ __forceinline__ void transform_fill_wave_body(const VolView& S, int* s_slot, int kx, int ky, int kz, const float* M, float src_res, Put put) {
    const int lane = threadIdx.x;
    const float half = src_res / 2;
    float n0[8], n1[8], n2[8];
    int p0[8], p1[8], p2[8];
    int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
#pragma unroll
    for (int zs = 0; zs < 8; ++zs) {
        const int vid = lane + 64 * zs;
        const float px = ((float)kx * 8.0f) * src_res + ((float)(vid & 7) * src_res + half);
        const float py = ((float)ky * 8.0f) * src_res + ((float)((vid >> 3) & 7) * src_res + half);
        const float pz = ((float)kz * 8.0f) * src_res + ((float)(vid >> 6) * src_res + half);
        const float q0 = ((M[0] * px + M[1] * py) + M[2] * pz) + M[3] * 1.0f;
        const float q1 = ((M[4] * px + M[5] * py) + M[6] * pz) + M[7] * 1.0f;
        const float q2 = ((M[8] * px + M[9] * py) + M[10] * pz) + M[11] * 1.0f;
        const float q3 = ((M[12] * px + M[13] * py) + M[14] * pz) + M[15] * 1.0f;
        n0[zs] = q0 / q3 - half; n1[zs] = q1 / q3 - half; n2[zs] = q2 / q3 - half;
        p0[zs] = (int)floorf(n0[zs] / src_res); p1[zs] = (int)floorf(n1[zs] / src_res); p2[zs] = (int)floorf(n2[zs] / src_res);
        lo[0] = min(lo[0], p0[zs] >> 3); hi[0] = max(hi[0], (int)(((long long)p0[zs] + 1) >> 3));
        lo[1] = min(lo[1], p1[zs] >> 3); hi[1] = max(hi[1], (int)(((long long)p1[zs] + 1) >> 3));
        lo[2] = min(lo[2], p2[zs] >> 3); hi[2] = max(hi[2], (int)(((long long)p2[zs] + 1) >> 3));
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
        for (int o = 32; o > 0; o >>= 1) { lo[a] = min(lo[a], __shfl_xor(lo[a], o, 64)); hi[a] = max(hi[a], __shfl_xor(hi[a], o, 64)); }
    const int x0 = lo[0], y0 = lo[1], z0 = lo[2];
    const long long ex = (long long)hi[0] - x0 + 1, ey = (long long)hi[1] - y0 + 1, ez = (long long)hi[2] - z0 + 1;
    const bool boxed = ex * ey <= kSrcBox && ex * ey * ez <= kSrcBox; // (uniform)
    if (boxed) {
        if (lane < (int)(ex * ey * ez)) s_slot[lane] = table_find(S, x0 + lane % (int)ex, y0 + (lane / (int)ex) % (int)ey, z0 + lane / (int)(ex * ey));
        __syncthreads(); // (one wave: orders the LDS writes before the reads below)
    }
    auto fetch = [&](int tx, int ty, int tz) -> Vox5 {
        if (!boxed) return fetch_voxel(S, tx, ty, tz);
        return load_voxel(S, s_slot[((tx >> 3) - x0) + (int)ex * (((ty >> 3) - y0) + (int)ey * ((tz >> 3) - z0))], tx, ty, tz);
    };
#pragma unroll UNROLL
    for (int zs = 0; zs < 8; ++zs) {
        Vox5 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = fetch(p0[zs] + (k & 1), p1[zs] + ((k >> 1) & 1), p2[zs] + ((k >> 2) & 1));
        // ReadVoxelInterpolate (VoxelCube.cpp:6-50)
        const float xw = (n0[zs] - (float)p0[zs] * src_res) / src_res, yw = (n1[zs] - (float)p1[zs] * src_res) / src_res,
                    zw = (n2[zs] - (float)p2[zs] * src_res) / src_res;
        put(zs, interp_taps(v, xw, yw, zw));
    }
}

} // namespace opv
