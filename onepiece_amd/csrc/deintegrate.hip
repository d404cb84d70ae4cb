// deintegrate.hip -- k_update_signed: the fusion kernel of a batch that holds at least one DE-INTEGRATION (op_volume_deintegrate* /
// op_volume_reintegrate*, include/onepiece_hip.h; volume_core.hpp lists the translation units).  file:line citations are relative to the
// reference's src directory.
//
// A de-integrated frame takes the steps of Integrator::IntegrateImage (Integration/Integrator.cpp:52-92) -- k_prepare_frames and k_select* have
// packed it and selected (and allocated) its blocks exactly as for a fused frame, because neither depends on what the volume stores -- and
// every voxel that passes the update predicate (pixel inside, d > 0, |new_sdf| < truncation) receives TSDFVoxel::operator+
// (Integration/TSDFVoxel.h:24-39) with an observation of weight -1: the inverse of the running mean.  For the stored voxel (s, w, c), the
// observation o = new_sdf and oc = byte / 255 per channel:
//   1. applied iff TSDFVoxel::IsValid (!(s >= 1 || w <= 0), TSDFVoxel.h:75-78) and w >= 1; otherwise the voxel stays as it is (`skipped`):
//      an unobserved or invalid voxel, a fractional weight below 1 from an upload or a merge.  (The reference's `weight == 0 -> return other`
//      would store a weight of -1; that is not reproduced.)
//   2. rw = w + (-1);
//   3. rw == 0: the voxel becomes the default voxel {999, 0, -1, -1, -1} -- the reference's default-constructed `result` (`reset`);
//   4. otherwise s' = (w * s + (-1) * o) / rw, the same per colour channel, w' = rw (`reverted`): every product, sum and quotient rounded to
//      float32, plain IEEE divisions (weights need not be integers here), no contraction (-ffp-contract=off).
// A fused (positive) frame of such a batch takes the reference's literal two-branch update, what k_integrate's general form computes.
//
// The kernel is k_integrate's skeleton without its specialisations: one workgroup per block of the batch list (blist / bmask, drawn from the
// per-XCD counters in chunks), a thread owns kZT voxels of one (x, y) column, a wave loads one z-slice of 256 contiguous bytes per plane, every
// selected entry of the batch is applied in call order in registers, and a voxel that changed is stored once.  The sign of an entry is a bit
// of the batch's sign mask: wave-uniform.  The pixel is project_pixel / project_pixel_uv and the packed frame of volume_core.hpp, the
// gathers are k_integrate's two forms: by construction the pixel integration used.
#include "volume_core.hpp"

namespace {

constexpr int kZT = 2;                       // voxels of a column per thread
constexpr int kWavesWg = 8 / kZT;            // waves per workgroup = z-groups per block
constexpr int kSignedMinWaves = 4;           // waves per SIMD it is compiled for: the four true divisions of an update need registers
constexpr int kSignedGrid = 256 * kSignedMinWaves * 4 / kWavesWg; // resident workgroups (they draw blocks; a multiple of the 8 XCDs)
static_assert(kSignedGrid % kKcShares == 0, "one drawing workgroup per share at least");

typedef unsigned int us_v2u __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned wave_uniform(unsigned x) { return (unsigned)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ unsigned long long wave_uniform(unsigned long long x) {
    return ((unsigned long long)wave_uniform((unsigned)(x >> 32)) << 32) | wave_uniform((unsigned)x);
}

// the slots of op_volume::dei_partial
constexpr int kDeiReverted = 0, kDeiReset = kPartialGrid, kDeiSkipped = 2 * kPartialGrid, kDeiFrames = 3 * kPartialGrid;

template <bool FAST, bool G2D>
__global__ __launch_bounds__(64 * kWavesWg, kSignedMinWaves) void k_update_signed(BatchInv B, CamParams C, VolView V, const uint2* __restrict__ pimg, State* st, int n_frames,
                                                                                  bmask_t sign, unsigned long long* __restrict__ upd_partial,
                                                                                  unsigned long long* __restrict__ sel_partial, unsigned long long* __restrict__ chg_partial,
                                                                                  unsigned long long* __restrict__ dei_partial) {
    __shared__ unsigned s_cnt[kWavesWg][5];
    __shared__ float s_c255[256];             // (float)b / 255.0f for every byte (Integrator.cpp:78), as k_integrate rounds it
    __shared__ unsigned s_next;
    const unsigned long long t_in = __builtin_amdgcn_s_memtime();
    // the selection has consumed the frames' bounding accumulators: back to the identity for the next batch (also when poisoned), as k_integrate does
    for (unsigned k = blockIdx.x * blockDim.x + threadIdx.x; k < (unsigned)(kMaxBatch * kAccSlots * 8); k += gridDim.x * blockDim.x) (&st->acc[0][0][0])[k] = 0u;
    if (st->overflow & 3u) return; // pool / table exhausted in this or an earlier batch: nothing is applied, the host grows the volume and replays
    const int tid = threadIdx.x, lane = tid & 63, zg = tid >> 6;
    for (int k = tid; k < 256; k += blockDim.x) s_c255[k] = (float)k / 255.0f;
    const unsigned npix = (unsigned)(C.width * C.height);
    const float half = C.res / 2;
    // VoxelCentroidOffSet (VoxelCube.h:48-61): x*res + half with x = lane & 7, y = lane >> 3
    const float ox = (float)(lane & 7) * C.res + half;
    const float oy = (float)(lane >> 3) * C.res + half;
    const float __attribute__((address_space(4)))* kargs =
        (const float __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr(); // BatchInv B = offset 0 of the kernarg segment
    (void)B;
    unsigned upd = 0, rev = 0, rst = 0, skp = 0, chg = 0, sel = 0, nblk = 0; // per lane; sel and nblk: thread 0's
    // the batch list in chunks of 32 blocks, chunk c to share c % 8 (k_integrate's dealing for short batches): the workgroups of share x draw positions
    const unsigned n0 = st->n_blist < V.max_blocks ? st->n_blist : V.max_blocks;
    const unsigned n_chunks = (n0 + 31u) >> 5;
    const unsigned per0 = ((n_chunks + (unsigned)kKcShares - 1u) / (unsigned)kKcShares) << 5;
    const unsigned xcd = blockIdx.x % (unsigned)kKcShares;
    unsigned* ctr = &st->kc_next[xcd * 16u];
    for (;;) {
        if (tid == 0) s_next = atomicAdd(ctr, 1u);
        __syncthreads();
        const unsigned j = s_next;
        if (j >= per0) break;
        const unsigned b = (((j >> 5) * (unsigned)kKcShares + xcd) << 5) + (j & 31u);
        const int tslot = b < n0 ? V.blist[b] : -1;
        const int idx = tslot >= 0 ? V.tvals[tslot] : -1; // idx < 0: pool overflow (reported through st->overflow)
        if (idx >= 0) {
            const bmask_t mask = wave_uniform(V.bmask[tslot]);
            if (tid == 0) { sel += mask_popc(mask); ++nblk; }
            const int kx = V.keys[3 * idx], ky = V.keys[3 * idx + 1], kz = V.keys[3 * idx + 2];
            float* vox = V.pool + (size_t)idx * kBlockFloats + (zg * kZT) * 64 + lane;
            float s[kZT], w[kZT], c0[kZT], c1[kZT], c2[kZT], pz[kZT];
#pragma unroll
            for (int z = 0; z < kZT; ++z) {
                const float* p = vox + z * 64;
                s[z] = p[0]; w[z] = p[kVox]; c0[z] = p[2 * kVox]; c1[z] = p[3 * kVox]; c2[z] = p[4 * kVox];
                // GetGlobalPoint (VoxelCube.h:75-80): Point3(id) * CUBE_SIZE * VoxelResolution + offset
                pz[z] = ((float)kz * 8.0f) * C.res + ((float)(zg * kZT + z) * C.res + half);
            }
            const float px = ((float)kx * 8.0f) * C.res + ox;
            const float py = ((float)ky * 8.0f) * C.res + oy;
            unsigned changed = 0u;
            // one selected entry: projections of the thread's kZT voxels and their {depth, rgba} gathers
            auto project = [&](int f, us_v2u (&rec)[kZT], float (&zc)[kZT]) {
                const float __attribute__((address_space(4)))* M = kargs + f * 12;
                // (frame base in 32 bits: check_cam keeps kMaxBatch x npix x 8 below 2^32)
                const char* fbase = (const char*)pimg + (unsigned)f * (npix * 8u);
                const __amdgpu_buffer_rsrc_t frame = __builtin_amdgcn_make_buffer_rsrc((void*)fbase, 0, (int)(npix * 8u), 0x00020000);
                const px_v4i frame2d = gather2d_rsrc(fbase, C.width, C.height);
                const float a0 = M[0] * px + M[1] * py, a1 = M[4] * px + M[5] * py, a2 = M[8] * px + M[9] * py;
#pragma unroll
                for (int z = 0; z < kZT; ++z) {
                    const float q0 = (a0 + M[2] * pz[z]) + M[3] * 1.0f;
                    const float q1 = (a1 + M[6] * pz[z]) + M[7] * 1.0f;
                    const float q2 = (a2 + M[10] * pz[z]) + M[11] * 1.0f;
                    zc[z] = q2;
                    if (G2D) { // off-image: a row the descriptor answers with zeros
                        int u, v;
                        project_pixel_uv<FAST>(C, q0, q1, q2, u, v);
                        rec[z] = gather2d(frame2d, u, v, C.width);
                    } else {
                        const int pix = project_pixel<FAST>(C, q0, q1, q2); // off-image: pixel -1 = an offset the buffer answers with zeros
                        rec[z] = __builtin_amdgcn_raw_buffer_load_b64(frame, pix * 8, 0, 0);
                    }
                }
            };
            // ... and its update of the voxels in registers, with the entry's sign (wave-uniform)
            auto apply = [&](int f, const us_v2u (&rec)[kZT], const float (&zc)[kZT]) {
                const bool negative = ((sign >> f) & 1u) != 0u;
#pragma unroll
                for (int z = 0; z < kZT; ++z) {
                    const float d = __uint_as_float(rec[z].x);      // off-image pixels carry d == 0
                    const float o = d - zc[z];
                    const bool seen = d > 0, near = fabsf(o) < C.trunc; // Integrator.cpp:70,74
                    if (!(seen & near)) continue;
                    const unsigned rgba = rec[z].y;
                    const float n0c = s_c255[rgba & 0xffu], n1c = s_c255[(rgba >> 8) & 0xffu], n2c = s_c255[(rgba >> 16) & 0xffu];
                    const bool valid = !(s[z] >= 1 || w[z] <= 0);   // TSDFVoxel::IsValid (TSDFVoxel.h:75-78)
                    if (negative) {
                        const bool can = valid && w[z] >= 1;
                        const float rw = w[z] + (-1.0f);            // TSDFVoxel::operator+ with other = (o, -1, oc) (TSDFVoxel.h:24-39)
                        const bool zero = rw == 0;
                        // (the three counters as plain sums of 0 / 1: incremented in three branches they end up as one indexed array in scratch)
                        skp += can ? 0u : 1u; rst += (can & zero) ? 1u : 0u; rev += (can & !zero) ? 1u : 0u;
                        if (can) {
                            if (zero) {
                                s[z] = 999.0f; w[z] = 0.0f; c0[z] = -1.0f; c1[z] = -1.0f; c2[z] = -1.0f;
                            } else {
                                s[z] = (w[z] * s[z] + (-1.0f) * o) / rw;
                                c0[z] = (w[z] * c0[z] + (-1.0f) * n0c) / rw;
                                c1[z] = (w[z] * c1[z] + (-1.0f) * n1c) / rw;
                                c2[z] = (w[z] * c2[z] + (-1.0f) * n2c) / rw;
                                w[z] = rw;
                            }
                            changed |= 1u << z;
                        }
                    } else {
                        if (valid) {
                            const float wsum = w[z] + 1.0f;         // other = (o, 1, oc)
                            s[z] = (w[z] * s[z] + 1.0f * o) / wsum;
                            c0[z] = (w[z] * c0[z] + 1.0f * n0c) / wsum;
                            c1[z] = (w[z] * c1[z] + 1.0f * n1c) / wsum;
                            c2[z] = (w[z] * c2[z] + 1.0f * n2c) / wsum;
                            w[z] = wsum;
                        } else {
                            s[z] = o; w[z] = 1.0f; c0[z] = n0c; c1[z] = n1c; c2[z] = n2c;
                        }
                        ++upd;
                        changed |= 1u << z;
                    }
                }
            };
            // the entries that selected the block, in call order; the gathers of the NEXT entry are issued before the current entry's updates
            // (two record sets, the loop unrolled by two, as in k_integrate)
            us_v2u recA[kZT], recB[kZT];
            float zcA[kZT], zcB[kZT];
            bmask_t m = mask;
            if (m != 0u) {
                int fA = mask_ctz(m), fB = 0;
                m &= m - 1u;
                project(fA, recA, zcA);
                for (;;) {
                    const bool more1 = m != 0u;
                    if (more1) { fB = mask_ctz(m); m &= m - 1u; project(fB, recB, zcB); }
                    apply(fA, recA, zcA);
                    if (!more1) break;
                    const bool more2 = m != 0u;
                    if (more2) { fA = mask_ctz(m); m &= m - 1u; project(fA, recA, zcA); }
                    apply(fB, recB, zcB);
                    if (!more2) break;
                }
            }
#pragma unroll
            for (int z = 0; z < kZT; ++z)
                if ((changed >> z) & 1u) {
                    float* p = vox + z * 64;
                    p[0] = s[z]; p[kVox] = w[z]; p[2 * kVox] = c0[z]; p[3 * kVox] = c1[z]; p[4 * kVox] = c2[z];
                }
            chg += (unsigned)__popc(changed);
        }
        __syncthreads();                                   // every wave has read the mask and the draw
        if (tslot >= 0 && tid == 0) V.bmask[tslot] = (bmask_t)0; // the owner clears it for the next batch
    }
    // per-workgroup counters into kPartialGrid slots
    upd = wave_sum(upd); rev = wave_sum(rev); rst = wave_sum(rst); skp = wave_sum(skp); chg = wave_sum(chg);
    if (lane == 0) { s_cnt[zg][0] = upd; s_cnt[zg][1] = rev; s_cnt[zg][2] = rst; s_cnt[zg][3] = skp; s_cnt[zg][4] = chg; }
    __syncthreads();
    if (tid == 0) {
        unsigned t[5] = {0, 0, 0, 0, 0};
        for (int k = 0; k < kWavesWg; ++k)
            for (int q = 0; q < 5; ++q) t[q] += s_cnt[k][q];
        const unsigned slot_c = blockIdx.x % (unsigned)kPartialGrid;
        atomicAdd(&upd_partial[slot_c], (unsigned long long)t[0]);
        atomicAdd(&sel_partial[slot_c], (unsigned long long)sel);
        atomicAdd(&chg_partial[slot_c], (unsigned long long)t[4]);
        atomicAdd(&chg_partial[kPartialGrid + slot_c], (unsigned long long)nblk);
        atomicAdd(&dei_partial[kDeiReverted + slot_c], (unsigned long long)t[1]);
        atomicAdd(&dei_partial[kDeiReset + slot_c], (unsigned long long)t[2]);
        atomicAdd(&dei_partial[kDeiSkipped + slot_c], (unsigned long long)t[3]);
        if (blockIdx.x == 0) {
            st->stat_frames += (unsigned long long)n_frames;
            st->stat_launches += 1ull;
            dei_partial[kDeiFrames] += (unsigned long long)mask_popc(sign);
        }
        atomicMax(&st->kc_t[blockIdx.x % (unsigned)kKcTSlots], (unsigned long long)__builtin_amdgcn_s_memtime() - t_in);
    }
}

} // namespace

namespace opv {

void launch_update_signed(op_volume* v, const BatchInv& I, const CamParams& C, int nf, bmask_t sign) {
    const VolView V = v->view();
#define OP_KS(FASTPX, G2DV) hipLaunchKernelGGL((k_update_signed<FASTPX, G2DV>), dim3(kSignedGrid), dim3(64 * kWavesWg), 0, v->stream, I, C, V, (const uint2*)v->pimg, \
                                               v->state, nf, sign, v->upd_partial, v->sel_partial, v->chg_partial, v->dei_partial)
    // the gather forms are k_integrate's (launch_integrate): the structured one for certified cameras whose rows fit the descriptor's stride field
    if (C.fast_px && gather2d_fits(C.width)) OP_KS(true, true);
    else if (C.fast_px) OP_KS(true, false);
    else OP_KS(false, false);
#undef OP_KS
}

int vol_deintegrate_counts(op_volume* v, unsigned long long out[4]) {
    std::vector<unsigned long long> part((size_t)kDeiFrames + 1);
    OP_HIP(hipMemcpy(part.data(), v->dei_partial, part.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    out[0] = part[kDeiFrames]; out[1] = out[2] = out[3] = 0;
    for (int i = 0; i < kPartialGrid; ++i) { out[1] += part[kDeiReverted + i]; out[2] += part[kDeiReset + i]; out[3] += part[kDeiSkipped + i]; }
    return OP_OK;
}

} // namespace opv
