// integrate.hip -- KC k_integrate: Integrator::IntegrateImage (Integration/Integrator.cpp:36-94) + TSDFVoxel::operator+ (TSDFVoxel.h:24-39) for all frames
// of a batch (volume_core.hpp lists the translation units).  file:line citations are relative to /root/reference/src.
#include "volume_core.hpp"
#include "kc_lanes.hpp"

namespace {

// ---------------------------------------------------------------------------------------------
// KC: Integrator::IntegrateImage (Integrator.cpp:36-94) for all frames of the batch (k_integrate below).
// ---------------------------------------------------------------------------------------------
typedef unsigned int kc_v2u __attribute__((ext_vector_type(2)));

// PLAIN: the volume's content has only ever been written by this kernel since it was created / cleared (no upload, merge,
// resampling or file in between; the host tracks it).  Then every stored voxel is either the default or a running mean
// of finite in-band observations: weights are integers >= 1, colours are means of byte/255 values (non-negative, so their
// numerators w*c + n never cancel), and the update can be evaluated
//   * branch-free: an invalid voxel (TSDFVoxel::IsValid false) is the valid formula with weight 0 --
//     (0*s + new)/(0 + 1) = new exactly for finite s -- instead of a second code path with five selects;
//   * with ONE unrefined reciprocal y = v_rcp_f32(wsum) shared by the four quotients, each of them one multiply and one
//     residual/correction pair (div_int_rcp, volume_core.hpp: its comment carries the proof): bit-identical to the IEEE
//     division because the divisor is an integer.  The proof needs wsum <= 2^19 and quotient, residual and correction
//     that are 0 or normal floats.  For a numerator n with |n| >= 2^-60 and wsum <= 2^19: |q0| >= 2^-60 * 2^-19 * (1 - 2^-23)
//     > 2^-80, so ulp(q0) >= 2^-103; a non-zero residual is a multiple of ulp(q0)/2, >= 2^-104; its correction r*y is
//     >= 2^-104 * 2^-19 * (1 - 2^-23) > 2^-124: all above 2^-126, whatever the denormal mode.  (2^-100, the bound of the
//     five-operation form this replaces, would leave r as small as 2^-144.)  Colour numerators are 0 or >= 2^-32 (no
//     cancellation: at least one byte/255 term, or all zero); the sdf numerator CAN cancel to something tiny.  So ONE guard,
//     one ballot: a lane with wsum > 2^19 (a voxel seen in more than half a million frames), or whose |w*s + new| is below
//     2^-60, takes the plain division for all four of its quotients, out of line (never, in practice).
//     wsum = 1 (a first observation or an invalid voxel): y = 1, q0 = n, r = 0 -- the numerator exactly.
// LEAN (PLAIN, and besides: every frame the volume has fused since it was created / cleared was fused by the exact update with a
// truncation T <= 0.5, and there were at most 2^19 of them; the host tracks it, launch_integrate): the validity select of the first item
// goes too, wv = w.  It is dead code under these hypotheses, because no stored voxel can be invalid with a weight other than 0:
//   hypotheses: a stored voxel is the default {999, 0, -1, -1, -1} (TSDFVoxel.h:79-81; k_fill_pool) or the result of k >= 1 updates with
//     observations |o| < T (the band test), each update s' = RN(RN(RN(w*s) + o) / (w + 1)) with the integer weight w = k - 1 <= 2^19 - 1
//     (at most one update per fused frame).  The short quotient is that division bit for bit (div_int_rcp), the guard's division is it.
//   the default voxel needs no test: its weight is exactly 0, so wv = w = 0 is what the select would have chosen; 0 * 999 = 0 and
//     0 * -1 = -0 are exact, the numerators are the observation and the new colour, the divisor is 1.  It is the only voxel with w <= 0.
//   the fixed-point step: each of the three roundings multiplies the magnitude by at most 1 + 2^-24 (a denormal product w*s is off by
//     at most 2^-150 instead, below everything here), so with g = (1 + 2^-24)^3 = 1 + d, d < 3.0000004 * 2^-24:
//       |s'| <= (w |s| + T) g / (w + 1).
//     For a bound B this maps |s| <= B to |s'| <= B as soon as (w B + T) g <= (w + 1) B, i.e. T g <= B (1 - w d).  B_W = T g / (1 - W d)
//     satisfies that for every w <= W at once (1 - w d >= 1 - W d), and the first update (w = 0) gives |s'| = |o| < T <= B_W: by induction
//     every voxel with weight <= W + 1 has |s| <= B_W.
//   where 2^19 enters: W = 2^19 gives W d < 0.09376, B_W < 1.1035 T, and T <= 0.5 gives |s| < 0.552 < 1: TSDFVoxel::IsValid holds for every
//     voxel of weight >= 1, the select would have passed w through.  Past 2^19 frames the bound keeps growing (it is void at w = 1 / d,
//     5.6 million) and from w = 2^24 on, where w + 1 = w, the update is no mean at all: the host then goes back to the form with the
//     select (as it does for T > 0.5, where one observation can itself be invalid from T >= 1 on, and after a sum-form batch, whose
//     roundings this argument does not cover).  tests/test_kc_lean_cpu.py runs the operation sequence to weight 2^19 on adversarial
//     streams (the worst |s| / T it finds is 1 - 2^-24: the mean does not leave the observations' range there) and checks that the colour means, convex combinations of values in [0, 1] under the
//     same three monotone roundings, stay in [0, 1].
//   the counters come from the weights (kWCount in k_integrate): under these hypotheses every update is wv = w, w' = RN(w + 1) with an integer
//     w <= 2^19 + kMaxBatch - 1 < 2^24, so w' = w + 1 exactly, and the guard's division path (the `slow` lanes) replaces the four quotients only, never
//     w.  A voxel's weight after the batch's frames minus its weight as loaded is therefore, exactly in float, the number of its updates in the
//     batch: the sum of these differences over a block's voxels is the block's share of voxels_updated (kept per lane as an integer, folded with
//     wave_sum at the kernel's end, as the sum form folds chg), a voxel was updated -- and has to be stored -- exactly when the two weights differ, and
//     the population count of that compare is the wave's share of voxels_written.  So the lean frame loop carries no ballot of the hits, no
//     s_bcnt1 / s_add for upd and no s_or for the store mask (2 + 2 + 2 scalar instructions per frame half).  Every other instantiation keeps them:
//     there an invalid voxel restarts at weight 1 (wv = 0), and from T >= 1 on an update can leave the weight at 1, so the difference is not the count.
//     tests/test_kc_counts_cpu.py runs the weight chain; tests/test_kc_diet_gpu.py holds both counters to the oracle's.
// Without PLAIN (arbitrary uploaded data: NaN, infinities, denormals, fractional weights) the update is the reference's
// two-branch form with four true divisions.
// ---------------------------------------------------------------------------------------------
// KC.  One workgroup per block of the batch list; the resident workgroups draw blocks from per-XCD counters.  Every voxel is
// read ONCE, every frame that selected the block is applied to it in frame order in registers (bit-identical to the
// reference's frame-by-frame running mean) and it is written once -- HBM traffic per voxel drops from 40 B per frame to
// 40 B per batch; block ownership is exclusive, so the read-modify-write needs no atomics.  A thread owns ZT voxels
// of one (x, y) column of the block (z = zg*ZT .. zg*ZT + ZT-1), a wave owns ZT z-slices, a workgroup of 8/ZT waves owns
// the block.  What that buys, per voxel and frame:
//   * everything that is uniform over the wave -- the frame's bit test, the three s_load_dwordx4 of its pose rows, the buffer
//     resource of its packed image, the loop control -- is paid once per ZT voxels instead of once per voxel (a third of the
//     issue slots of a one-voxel-per-thread kernel go to scalar and branch instructions, profiles/r03_issue_costs.json);
//   * the partial sums M[r][0]*px + M[r][1]*py of the three pose rows depend on x and y only and are shared by the ZT voxels
//     (the same two rounded products and one rounded sum the reference forms for each of them: bit-identical);
//   * ZT independent dependency chains per thread hide the VALU and gather latencies that eight waves per SIMD hid before,
//     so the kernel runs at a lower occupancy with a larger register budget.
// A plane row of a z-slice is still one 256-byte wave access.  Frames are applied in ascending order; the gathers of the
// NEXT selected frame are issued before the current frame's updates (two record sets, the frame loop unrolled by two).
// ---------------------------------------------------------------------------------------------
// one voxel's five planes {sdf, weight, colour} of its block in the pool (kVox floats apart)
__device__ __forceinline__ void voxel_load(const float* p, float& s, float& w, float& c0, float& c1, float& c2) {
    s = p[0]; w = p[kVox]; c0 = p[2 * kVox]; c1 = p[3 * kVox]; c2 = p[4 * kVox];
}
__device__ __forceinline__ void voxel_store(float* p, float s, float w, float c0, float c1, float c2) {
    p[0] = s; p[kVox] = w; p[2 * kVox] = c0; p[3 * kVox] = c1; p[4 * kVox] = c2;
}
template <bool PLAIN, bool LEAN = false>
__device__ __forceinline__ void voxel_update(float& s, float& w, float& c0, float& c1, float& c2, float new_sdf, unsigned rgba, const float* s_c255) {
    const float n0 = s_c255[rgba & 0xffu], n1 = s_c255[(rgba >> 8) & 0xffu], n2 = s_c255[(rgba >> 16) & 0xffu];
    if (PLAIN) {
        // TSDFVoxel::IsValid (TSDFVoxel.h:75-78) false -> weight 0 in the same formula (see the PLAIN comment above); LEAN: only w == 0 is invalid
        const float wv = LEAN ? w : ((s >= 1 || w <= 0) ? 0.0f : w);
        // the four products first, the weight sum after them: it can then be formed in the weight's own register (no copy of the weight is kept alive)
        const float ps = wv * s, p0 = wv * c0, p1 = wv * c1, p2 = wv * c2;
        const float wsum = wv + 1.0f;
        const float y = __builtin_amdgcn_rcpf(wsum);            // unrefined: div_int_rcp needs 1 ulp only
        const float ns = ps + 1.0f * new_sdf;
        const float m0 = p0 + 1.0f * n0, m1 = p1 + 1.0f * n1, m2 = p2 + 1.0f * n2;
        float qs = div_int_rcp(ns, wsum, y), q0 = div_int_rcp(m0, wsum, y), q1 = div_int_rcp(m1, wsum, y), q2 = div_int_rcp(m2, wsum, y);
        // outside div_int_rcp's hypotheses (see the PLAIN comment above).  | and not ||: two compares whose masks meet in scalar registers,
        // no divergent region for the right-hand side.  A numerator of exactly 0 would pass through div_int_rcp unharmed (q0 = r = 0), but
        // telling it from a tiny one costs a third compare per update; it is as rare as a tiny one and the division gives the same 0.
        // LEAN: the weight half cannot fire.  The host launches this form only while lean_frames <= 2^19, counted with the running batch included
        // (launch_integrate), a voxel gains at most one per fused frame, so no weight sum formed here exceeds 2^19: only the numerator is tested.
        const bool slow = LEAN ? !(fabsf(ns) >= 0x1p-60f) : ((wsum > 0x1p19f) | !(fabsf(ns) >= 0x1p-60f));
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(slow) != 0ull, 0)) {
            if (slow) { qs = ns / wsum; q0 = m0 / wsum; q1 = m1 / wsum; q2 = m2 / wsum; }
        }
        s = qs; c0 = q0; c1 = q1; c2 = q2;
        w = wsum;
    } else if (!(s >= 1 || w <= 0)) { // TSDFVoxel::IsValid (TSDFVoxel.h:75-78)
        const float wsum = w + 1.0f;  // TSDFVoxel::operator+ with other = (new_sdf, 1.0, c) (TSDFVoxel.h:24-39)
        s = (w * s + 1.0f * new_sdf) / wsum;
        c0 = (w * c0 + 1.0f * n0) / wsum;
        c1 = (w * c1 + 1.0f * n1) / wsum;
        c2 = (w * c2 + 1.0f * n2) / wsum;
        w = wsum;
    } else {
        s = new_sdf; w = 1.0f; c0 = n0; c1 = n1; c2 = n2;
    }
}

// De-integration (op_volume_deintegrate* / op_volume_reintegrate*, include/onepiece_hip.h).  A de-integrated frame takes the steps of
// Integrator::IntegrateImage (Integration/Integrator.cpp:52-92) -- k_prepare_frames and k_select* have packed it and selected (and allocated) its
// blocks exactly as for a fused frame, because neither depends on what the volume stores -- and every voxel that passes the update predicate
// (pixel inside, d > 0, |new_sdf| < truncation) receives TSDFVoxel::operator+ (TSDFVoxel.h:24-39) with an observation of weight -1: the inverse of
// the running mean.  For the stored voxel (s, w, c), the observation o = new_sdf and oc = byte / 255 per channel:
//   1. applied iff TSDFVoxel::IsValid (!(s >= 1 || w <= 0), TSDFVoxel.h:75-78) and w >= 1; otherwise the voxel stays as it is (`skipped`):
//      an unobserved or invalid voxel, a fractional weight below 1 from an upload or a merge.  (The reference's `weight == 0 -> return other`
//      would store a weight of -1; that is not reproduced.)
//   2. rw = w + (-1);
//   3. rw == 0: the voxel becomes the default voxel {999, 0, -1, -1, -1} -- the reference's default-constructed `result` (`reset`);
//   4. otherwise s' = (w * s + (-1) * o) / rw, the same per colour channel, w' = rw (`reverted`): every product, sum and quotient rounded to
//      float32, plain IEEE divisions (weights need not be integers here), no contraction (-ffp-contract=off).
// A fused (positive) entry of a batch that holds a de-integration takes voxel_update<false>: the PLAIN and LEAN hypotheses do not survive a weight of -1.
// voxel_revert is steps 1-4.  Every lane of the wave calls it, `hit` = its voxel passes the update predicate, and gets back step 1's verdict (`can`)
// and step 3's (`zero`): the kernel counts the three outcomes from the scalar masks of these compares, as it counts the hits of a fused frame.
__device__ __forceinline__ void voxel_revert(bool hit, float& s, float& w, float& c0, float& c1, float& c2, float new_sdf, unsigned rgba, const float* s_c255, bool& can,
                                             bool& zero) {
    can = hit & !(s >= 1 || w <= 0) & (w >= 1);
    const float rw = w + (-1.0f);
    zero = rw == 0;
    if (!can) return;
    const float n0 = s_c255[rgba & 0xffu], n1 = s_c255[(rgba >> 8) & 0xffu], n2 = s_c255[(rgba >> 16) & 0xffu];
    if (zero) {
        s = 999.0f; w = 0.0f; c0 = -1.0f; c1 = -1.0f; c2 = -1.0f;
    } else {
        s = (w * s + (-1.0f) * new_sdf) / rw;
        c0 = (w * c0 + (-1.0f) * n0) / rw;
        c1 = (w * c1 + (-1.0f) * n1) / rw;
        c2 = (w * c2 + (-1.0f) * n2) / rw;
        w = rw;
    }
}

// SUMF (opt-in, OP_VOLUME_UPDATE_SUM_FORM): the frames of the batch are not applied one by one.  Per voxel the kernel keeps the NUMBER of in-band
// observations of the batch, the sum of their sdf values and the sums of their colour bytes (exact integers), and forms the weighted mean with the
// stored voxel ONCE per batch: s' = (w s + sum sdf) / (w + n), c' = (w c + sum bytes / 255) / (w + n), w' = w + n -- TSDFVoxel::operator+
// (TSDFVoxel.h:24-39) applied n times in exact arithmetic.  Same blocks, same pixels, same weights (integers); sdf and colour differ from the
// frame-by-frame running mean by float rounding only (a few 1e-7 relative; north_star's bar is 1e-4).  Per voxel and frame the ~35 instructions
// of the exactly rounded update shrink to 7 (two selects, one float add, two byte-pair adds with their masks).
#ifdef KC_TRACE // development aid (make EXTRA=-DKC_TRACE): where a workgroup of the last k_integrate launch spent its time, per wave; dumped by op_volume_destroy
__device__ unsigned long long g_kc_trace[4096 * 4 * 8];
#define KC_T(K) do { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); kt_[K] += now_ - kt_last_; kt_last_ = now_; } while (0)
#define KC_N(K, V) do { kt_[K] += (V); } while (0)
#else
#define KC_T(K) do { } while (0)
#define KC_N(K, V) do { } while (0)
#endif
// G2D: the frame's records are gathered through a structured descriptor (gather2d, volume_core.hpp) that does the row test and the address
// arithmetic; the host launches it for certified cameras whose rows fit the stride field (launch_integrate), every other launch keeps the raw form.
template <bool FAST, bool PLAIN, int ZT, bool SUMF = false, bool LEAN = false, bool G2D = false, bool SIGNED = false>
__global__ __launch_bounds__(512 / ZT, (SUMF ? KC_SUM_MIN_WAVES : SIGNED ? KC_SIGNED_MIN_WAVES : KC_COL_MIN_WAVES)) void k_integrate(BatchInv B, CamParams C, VolView V, const uint2* __restrict__ pimg, State* st,
                                                                            int n_frames, unsigned long long* __restrict__ upd_partial,
                                                                            unsigned long long* __restrict__ sel_partial, unsigned long long* __restrict__ chg_partial,
                                                                            unsigned plain_from, unsigned* __restrict__ rc_sum, unsigned rc_stamp, bmask_t sign,
                                                                            unsigned long long* __restrict__ dei_partial) {
    static_assert(!SIGNED || !(PLAIN || SUMF || LEAN), "the PLAIN and LEAN hypotheses do not survive a weight of -1");
    constexpr int kWaves = 8 / ZT;            // waves per workgroup = z-groups per block
    constexpr bool kSummaries = !SUMF && !SIGNED; // the raycaster's block summaries are restated by the exact update of fused frames only (the host invalidates them otherwise)
    constexpr bool kWCount = LEAN && !SUMF;   // voxels_updated, voxels_written and the store mask are read off the weights after the frames (LEAN paragraph above)
    __shared__ unsigned s_cnt[kWaves][SIGNED ? 5 : 2];
    __shared__ unsigned s_sign[2][kWaves];    // rc_sum: per wave, does its part of the block hold an observed sdf <= 0 (bit 0) / > 0 (bit 1) after the batch
    __shared__ float s_c255[256];             // (float)b / 255.0f for every byte (Integrator.cpp:78), correctly rounded once
    __shared__ unsigned s_next[2];
    const unsigned long long t_in = __builtin_amdgcn_s_memtime();
#ifdef KC_TRACE
    unsigned long long kt_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, kt_last_ = t_in;
#endif
    // KB has consumed the frames' bounding accumulators: back to the identity for the next batch (also when poisoned)
    for (unsigned k = blockIdx.x * blockDim.x + threadIdx.x; k < (unsigned)(kMaxBatch * kAccSlots * 8); k += gridDim.x * blockDim.x) (&st->acc[0][0][0])[k] = 0u;
    if (st->overflow & 3u) return; // pool / table exhausted in this or an earlier batch: nothing is fused, the host replays
    const int tid = threadIdx.x, lane = tid & 63, zg = tid >> 6;
    if (!SUMF) for (int k = tid; k < 256; k += blockDim.x) s_c255[k] = (float)k / 255.0f;
    const unsigned npix = (unsigned)(C.width * C.height);
    const float half = C.res / 2;
    // VoxelCentroidOffSet (VoxelCube.h:48-61): x*res + half, with the voxel (x, y, z) of this lane's slot 0 from the lane map (kc_lanes.hpp)
    const int lx = kc_lanes::vx<ZT>(zg, 0, lane), ly = kc_lanes::vy<ZT>(zg, 0, lane), lz = kc_lanes::vz<ZT>(zg, 0, lane);
    const float ox = (float)lx * C.res + half;
    const float oy = (float)ly * C.res + half;
    const float __attribute__((address_space(4)))* kargs =
        (const float __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr(); // BatchInv B = offset 0 of the kernarg segment
    (void)B;
    unsigned upd = 0, sel = 0, chg = 0, nblk = 0;   // upd and (exact update) chg: per WAVE (scalar counts of hit ballots), the others per lane; kWCount: upd per lane
    unsigned neg_hit = 0, neg_can = 0, rst = 0;     // SIGNED, per wave: the voxels de-integrated entries hit, those voxel_revert was applied to, those it reset
    // XCD-aware order (workgroup b runs on XCD b % 8, each XCD has its own 4 MiB L2; blocks that gather the same pixels should meet in one L2)
    // and dynamic scheduling (blocks differ in work: 1..32 frames touch them; the workgroups of an XCD DRAW list positions from one counter,
    // the next one before the current block is processed so that the atomic's round trip is hidden).  Two ways of dealing the batch list to
    // the eight draw counters:
    //  * eighths + stealing, for full batches (>= KC_STEAL_MIN_FRAMES frames): share x is the x-th contiguous eighth of the list and XCD x
    //    starts on it; the eighths hold the same number of blocks but not the same work, so a workgroup whose share is exhausted reads all
    //    eight counters (one round trip) and goes on with the share that has the most left.
    //    Per 32-frame launch: eighths alone 689 us, with stealing 627-631 us;
    //  * chunks, for short batches: share x is every eighth chunk of kChunk blocks (every XCD a sample of the whole list), no stealing: for
    //    ONE frame per launch, where the kernel is HBM-bound and the work per block uniform, 79 us against 95 us with stealing (its last look
    //    costs a short launch more than it can win).  Measured crossover (tools/prof_driver.bin batch=N under the tracer, stealing vs chunks):
    //    8 frames 207 vs 194 us, 16: 360 vs 356, 24: 524 vs 527, 32: 677 vs 687.
    // Either way a share is per0 list positions, position j of share x is list entry b below, and entries past the list's end are skipped.
    const bool eighths = n_frames >= KC_STEAL_MIN_FRAMES;
    constexpr unsigned kChunkLog2 = 5u, kChunk = 1u << kChunkLog2;
    const unsigned n0 = st->n_blist < V.max_blocks ? st->n_blist : V.max_blocks;
    const unsigned n_chunks = (n0 + kChunk - 1u) >> kChunkLog2;
    const unsigned per0 = eighths ? (n0 + (unsigned)kKcShares - 1u) / (unsigned)kKcShares : ((n_chunks + (unsigned)kKcShares - 1u) / (unsigned)kKcShares) << kChunkLog2;
    unsigned xcd = blockIdx.x % (unsigned)kKcShares;          // the share this workgroup draws from: its own first
    for (;;) {
    unsigned* ctr = &st->kc_next[xcd * 16u];
    if (tid == 0) s_next[0] = atomicAdd(ctr, 1u);
    __syncthreads();
    unsigned slot = 0u;
    for (unsigned j = s_next[0]; j < per0;) {
        if (tid == 0) s_next[slot ^ 1u] = atomicAdd(ctr, 1u);
        const unsigned b = eighths ? xcd * per0 + j : (((j >> kChunkLog2) * (unsigned)kKcShares + xcd) << kChunkLog2) + (j & (kChunk - 1u));
        KC_T(0);
        const int tslot = b < n0 ? V.blist[b] : -1;
        const int idx = tslot >= 0 ? V.tvals[tslot] : -1; // idx < 0: pool overflow (reported through st->overflow)
        KC_N(6, 1);
        if (idx >= 0) {
            const bmask_t mask = V.bmask[tslot];
            if (zg == 0) { sel += mask_popc(mask); ++nblk; }
            const int kx = V.keys[3 * idx], ky = V.keys[3 * idx + 1], kz = V.keys[3 * idx + 2];
            float* vox = V.pool + (size_t)idx * kBlockFloats + (lx + 8 * ly + 64 * lz);
            float s[ZT], w[ZT], c0[ZT], c1[ZT], c2[ZT], pz[ZT];
#pragma unroll
            for (int z = 0; z < ZT; ++z) {
                // (the sum form needs the stored voxel only after the frames: it is loaded there, and the registers are free until then)
                if (!SUMF) voxel_load(vox + z * kc_lanes::kSlotStride, s[z], w[z], c0[z], c1[z], c2[z]);
                // GetGlobalPoint (VoxelCube.h:75-80): Point3(id) * CUBE_SIZE * VoxelResolution + offset
                pz[z] = ((float)kz * 8.0f) * C.res + ((float)(lz + z * kc_lanes::kBZ) * C.res + half);
            }
            const float px = ((float)kx * 8.0f) * C.res + ox;
            const float py = ((float)ky * 8.0f) * C.res + oy;
            float w0[ZT];                                  // kWCount: the weights as loaded (two registers; the flagship instantiation has them to spare)
#pragma unroll
            for (int z = 0; z < ZT; ++z) w0[z] = kWCount ? w[z] : 0.0f;
            // voxels to write back.  Exact update: the hit masks are already in scalar registers, so one wave-uniform 64-bit mask per z collects
            // them (no per-lane v_or per update); the stores run under it and its population count is the wave's share of voxels_written.
            // Sum form: per lane, known only after the frames.
            unsigned changed = 0u;
            unsigned long long changed_m[ZT];
#pragma unroll
            for (int z = 0; z < ZT; ++z) changed_m[z] = 0ull;
            // sum form: sdf sum, byte sums of colour channels 0 and 2 in the two halves of one word, of channel 1 in the low half of another whose
            // high half counts the observations (<= 64 frames x 255 < 2^16)
            float ssum[ZT];
            unsigned acc02[ZT], acc1n[ZT];
#pragma unroll
            for (int z = 0; z < ZT; ++z) { ssum[z] = 0.0f; acc02[z] = 0u; acc1n[z] = 0u; }
            // one selected frame: projections of the thread's ZT voxels and their {depth, rgba} gathers
            auto project = [&](int f, kc_v2u (&rec)[ZT], float (&zc)[ZT]) {
                int fo = f;
                asm volatile("" : "+s"(fo));
                const float __attribute__((address_space(4)))* M = kargs + fo * 12;
                // (frame base in 32 bits: check_cam keeps kMaxBatch x npix x 8 below 2^32)
                const char* fbase = (const char*)pimg + (unsigned)fo * (npix * 8u);
                const __amdgpu_buffer_rsrc_t frame = __builtin_amdgcn_make_buffer_rsrc((void*)fbase, 0, (int)(npix * 8u), 0x00020000);
                const px_v4i frame2d = gather2d_rsrc(fbase, C.width, C.height);
                const float a0 = M[0] * px + M[1] * py, a1 = M[4] * px + M[5] * py, a2 = M[8] * px + M[9] * py;
#pragma unroll
                for (int z = 0; z < ZT; ++z) {
                    const float q0 = (a0 + M[2] * pz[z]) + M[3] * 1.0f;
                    const float q1 = (a1 + M[6] * pz[z]) + M[7] * 1.0f;
                    const float q2 = (a2 + M[10] * pz[z]) + M[11] * 1.0f;
                    zc[z] = q2;
                    if (G2D) { // off-image: a row the descriptor answers with zeros
                        int u, v;
                        project_pixel_uv<FAST, false>(C, q0, q1, q2, u, v); // (no window test on q2: launch_integrate has the host's bound on it)
                        rec[z] = gather2d(frame2d, u, v, C.width);
                    } else {
                        const int pix = project_pixel<FAST, false>(C, q0, q1, q2); // off-image: pixel -1 = an offset the buffer answers with zeros
                        rec[z] = __builtin_amdgcn_raw_buffer_load_b64(frame, pix * 8, 0, 0);
                    }
                }
            };
            // PLAIN: every block of the volume was written by this kernel only.  Otherwise (the volume has seen an upload, a merge, a
            // sum-form unpack or a file): the blocks that existed then (pool slots below plain_from) hold arbitrary data and take the
            // general update; blocks allocated since are this kernel's own and keep the fast one.  Uniform per block.
            const bool plain_block = PLAIN || (unsigned)idx >= plain_from;
            // SIGNED: `negative` is the entry's bit of the batch's sign mask (wave-uniform) -- a de-integration
            auto apply = [&](const kc_v2u (&rec)[ZT], const float (&zc)[ZT], auto plain_c, bool negative) {
                constexpr bool kPlain = decltype(plain_c)::value;
#pragma unroll
                for (int z = 0; z < ZT; ++z) {
                    const float d = __uint_as_float(rec[z].x); // off-image pixels carry d == 0 -> skipped like `continue`
                    const float new_sdf = d - zc[z];
                    // Integrator.cpp:70,74 (d > 0 and |sdf| < truncation): two compares whose masks meet in scalar registers (& and not &&, as in
                    // project_pixel) and one divergent region.  NaN and infinities fail the second compare, d <= 0 and -0 the first.
                    const bool seen = d > 0, near = fabsf(new_sdf) < C.trunc, hit = seen & near;
                    if constexpr (SIGNED) {
                        if (negative) { // the same predicate, the inverse update; its outcomes counted where the masks are, like the hits below
                            bool can, zero;
                            voxel_revert(hit, s[z], w[z], c0[z], c1[z], c2[z], new_sdf, rec[z].y, s_c255, can, zero);
                            const unsigned long long m_can = __builtin_amdgcn_ballot_w64(can);
                            neg_hit += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(seen) & __builtin_amdgcn_ballot_w64(near));
                            neg_can += (unsigned)__builtin_popcountll(m_can);
                            rst += (unsigned)__builtin_popcountll(m_can & __builtin_amdgcn_ballot_w64(zero));
                            changed_m[z] |= m_can;
                            continue;
                        }
                    }
                    if (kWCount) { // lean: no ballot, no count, no mask per update -- the weights carry all three (LEAN paragraph above)
                        if (hit) voxel_update<true, true>(s[z], w[z], c0[z], c1[z], c2[z], new_sdf, rec[z].y, s_c255);
                        continue;
                    }
                    // the wave's hits, counted where the masks already are: control flow is wave-uniform here and every lane of the wave is live.
                    // (The ballot of each compare IS its scalar mask; the ballot of their conjunction would be rebuilt from a per-lane 0 / 1.)
                    const unsigned long long hits = __builtin_amdgcn_ballot_w64(seen) & __builtin_amdgcn_ballot_w64(near);
                    upd += (unsigned)__builtin_popcountll(hits);
                    if (SUMF) { // branch-free: an observation that misses adds zeros
                        ssum[z] += hit ? new_sdf : 0.0f;
                        const unsigned t = hit ? rec[z].y : 0u;           // byte 3 of a packed pixel is 1 (k_prepare_frames): the count
                        acc02[z] += t & 0x00ff00ffu;
                        acc1n[z] += (t >> 8) & 0x00ff00ffu;
                    } else {
                        changed_m[z] |= hits;
                        if (hit) voxel_update<kPlain, kPlain && LEAN>(s[z], w[z], c0[z], c1[z], c2[z], new_sdf, rec[z].y, s_c255);
                    }
                }
            };
            kc_v2u recA[ZT], recB[ZT];
            float zcA[ZT], zcB[ZT];
            bool negA = false, negB = false;               // SIGNED: each record set's own sign, read where its entry is projected
#ifdef KC_TRACE
            { float keep_ = px + py + pz[0]; if (!SUMF) keep_ += s[0]; asm volatile("" :: "v"(keep_)); KC_T(1); } // (the block's metadata and voxels have arrived)
#endif
            auto frames = [&](auto plain_c) {
                bmask_t m = mask;                                 // wave-uniform
                if (!m) return;
                int f = mask_ctz(m); m &= m - 1u;
                project(f, recA, zcA);
                if constexpr (SIGNED) negA = ((sign >> f) & 1u) != 0u;
                for (;;) {
                    const bool more1 = m != 0u;
                    if (more1) {
                        f = mask_ctz(m); m &= m - 1u; project(f, recB, zcB);
                        if constexpr (SIGNED) negB = ((sign >> f) & 1u) != 0u;
                    }
                    apply(recA, zcA, plain_c, negA);
                    if (!more1) break;
                    const bool more2 = m != 0u;
                    if (more2) {
                        f = mask_ctz(m); m &= m - 1u; project(f, recA, zcA);
                        if constexpr (SIGNED) negA = ((sign >> f) & 1u) != 0u;
                    }
                    apply(recB, zcB, plain_c, negB);
                    if (!more2) break;
                }
            };
            // SIGNED: the general update for every block, whatever plain_from says
            if constexpr (SIGNED) frames(std::false_type{});
            else if (SUMF || PLAIN || plain_block) frames(std::true_type{}); else frames(std::false_type{});
            KC_T(2); KC_N(7, mask_popc(mask));
            if (SUMF) {
#pragma unroll
                for (int z = 0; z < ZT; ++z)
                    if (acc1n[z] >> 16) voxel_load(vox + z * kc_lanes::kSlotStride, s[z], w[z], c0[z], c1[z], c2[z]);
#pragma unroll
                for (int z = 0; z < ZT; ++z) {
                    const unsigned cnt = acc1n[z] >> 16;
                    if (cnt) {
                        changed |= 1u << z;
                        // TSDFVoxel::operator+ (TSDFVoxel.h:24-39) for the batch's observations at once; an invalid voxel (IsValid false,
                        // :75-78) is replaced by their mean, as the first observation would have replaced it
                        const bool valid = !(s[z] >= 1 || w[z] <= 0);
                        const float wv = valid ? w[z] : 0.0f, nf = (float)cnt, wsum = wv + nf;
                        const float b0 = (float)(acc02[z] & 0xffffu) / 255.0f, b1 = (float)(acc1n[z] & 0xffffu) / 255.0f, b2 = (float)(acc02[z] >> 16) / 255.0f;
                        s[z] = ((valid ? wv * s[z] : 0.0f) + ssum[z]) / wsum;
                        c0[z] = ((valid ? wv * c0[z] : 0.0f) + b0) / wsum;
                        c1[z] = ((valid ? wv * c1[z] : 0.0f) + b1) / wsum;
                        c2[z] = ((valid ? wv * c2[z] : 0.0f) + b2) / wsum;
                        w[z] = wsum;
                    }
                }
            }
            if (kWCount) { // the weights' differences are the voxel's hits of the batch (exact: integers <= 2^19 + kMaxBatch), a changed weight is a voxel to store
#pragma unroll
                for (int z = 0; z < ZT; ++z) {
                    const bool wrote = w[z] != w0[z];
                    upd += (unsigned)(w[z] - w0[z]);       // (per lane)
                    chg += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(wrote));
                    if (wrote) voxel_store(vox + z * kc_lanes::kSlotStride, s[z], w[z], c0[z], c1[z], c2[z]);
                }
            } else {
#pragma unroll
                for (int z = 0; z < ZT; ++z)
                    if (SUMF ? ((changed >> z) & 1u) != 0u : ((changed_m[z] >> lane) & 1ull) != 0ull) voxel_store(vox + z * kc_lanes::kSlotStride, s[z], w[z], c0[z], c1[z], c2[z]);
                if (SUMF) chg += (unsigned)__popc(changed);
                else {
#pragma unroll
                    for (int z = 0; z < ZT; ++z) chg += (unsigned)__builtin_popcountll(changed_m[z]);
                }
            }
            // The raycaster's block summaries (raycast.hip: k_rc_neighbours drops blocks by them before loading a voxel) describe exactly what is in
            // registers here -- the block's 512 voxels after the batch: the kernel that changes a block restates its summary, so views between fusions
            // find every block they meet described instead of starting from nothing (the host does not invalidate the summaries for such a batch).
            if (kSummaries && rc_sum) {                    // (uniform)
                bool neg = false, pos = false;
#pragma unroll
                for (int z = 0; z < ZT; ++z) { const bool obs = w[z] > 0; neg |= obs && s[z] <= 0; pos |= obs && s[z] > 0; }
                const unsigned f = (__builtin_amdgcn_ballot_w64(neg) ? 1u : 0u) | (__builtin_amdgcn_ballot_w64(pos) ? 2u : 0u);
                if (lane == 0) s_sign[slot][zg] = f;
            }
        }
        KC_T(3);
        __syncthreads();                                   // every wave has read the mask; s_next[slot ^ 1] is visible
        KC_T(4);
        if (tslot >= 0 && tid == 0) V.bmask[tslot] = (bmask_t)0; // the owner clears it for the next batch
        if (kSummaries && rc_sum && idx >= 0 && tid == 0) {     // (s_sign[slot] is written again two blocks on, behind the next barrier)
            unsigned f = 0u;
#pragma unroll
            for (int k = 0; k < kWaves; ++k) f |= s_sign[slot][k];
            rc_sum[idx] = (rc_stamp << 2) | f;
        }
        slot ^= 1u;
        j = s_next[slot];
    }
    if (!eighths) break;
    // the share is exhausted: look at all the draw counters at once (one round trip) and go on with the share that has the most left
    __syncthreads();                                          // everybody has read the last draw
    if (tid < 64) {
        unsigned left = 0u;
        if (tid < kKcShares) {
            const unsigned c = __hip_atomic_load(&st->kc_next[(unsigned)tid * 16u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            left = c < per0 ? per0 - c : 0u;
        }
        unsigned key = ((left < 0x7fffffu ? left : 0x7fffffu) << 8) | (unsigned)tid; // most left, ties to the higher share index (any fixed rule)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const unsigned x = __shfl_xor(key, o, 64); key = x > key ? x : key; }
        if (tid == 0) s_next[0] = key;
    }
    __syncthreads();
    const unsigned key = s_next[0];
    if ((key >> 8) == 0u) break;                              // nothing left anywhere
    xcd = key & 0xffu;
    __syncthreads();                                          // s_next[0] is written again at the top
    }
#ifdef KC_TRACE
    KC_T(5);
    if (lane == 0 && blockIdx.x < 4096) for (int k = 0; k < 8; ++k) g_kc_trace[((size_t)blockIdx.x * 4 + zg) * 8 + k] = kt_[k];
#endif
    // per-workgroup counters into kPartialGrid slots
    if (SUMF) chg = wave_sum(chg);                            // (upd is the wave's total already, and so is the exact update's chg)
    if (kWCount) upd = wave_sum(upd);                         // (... except where it was kept per lane)
    if (lane == 0) { s_cnt[zg][0] = upd; s_cnt[zg][1] = chg; }
    if constexpr (SIGNED) if (lane == 0) { s_cnt[zg][2] = neg_can - rst; s_cnt[zg][3] = rst; s_cnt[zg][4] = neg_hit - neg_can; } // reverted, reset, skipped
    __syncthreads();
    if (tid == 0) {
        unsigned t = 0, c = 0;
        for (int k = 0; k < kWaves; ++k) { t += s_cnt[k][0]; c += s_cnt[k][1]; }
        const unsigned slot_c = blockIdx.x % (unsigned)kPartialGrid;
        if constexpr (SIGNED) {
            unsigned d[3] = {0, 0, 0};
            for (int k = 0; k < kWaves; ++k)
                for (int q = 0; q < 3; ++q) d[q] += s_cnt[k][2 + q];
            atomicAdd(&dei_partial[kDeiReverted + slot_c], (unsigned long long)d[0]);
            atomicAdd(&dei_partial[kDeiReset + slot_c], (unsigned long long)d[1]);
            atomicAdd(&dei_partial[kDeiSkipped + slot_c], (unsigned long long)d[2]);
            if (blockIdx.x == 0) dei_partial[kDeiFrames] += (unsigned long long)mask_popc(sign);
        }
        atomicAdd(&upd_partial[slot_c], (unsigned long long)t);
        atomicAdd(&sel_partial[slot_c], (unsigned long long)sel);
        atomicAdd(&chg_partial[slot_c], (unsigned long long)c);
        atomicAdd(&chg_partial[kPartialGrid + slot_c], (unsigned long long)nblk);
        if (blockIdx.x == 0) { st->stat_frames += (unsigned long long)n_frames; st->stat_launches += 1ull; }
        atomicMax(&st->kc_t[blockIdx.x % (unsigned)kKcTSlots], (unsigned long long)__builtin_amdgcn_s_memtime() - t_in);
    }
}

// test hooks: both forms of the voxel update for n operand sets, lanes packed 64 to a wave in input order (see op_debug_voxel_update),
// and the hardware reciprocal div_int_rcp's proof starts from (op_debug_rcp)
__global__ __launch_bounds__(256) void k_debug_voxel_update(const float* __restrict__ s, const float* __restrict__ w, const float* __restrict__ c0, const float* __restrict__ c1,
                                                            const float* __restrict__ c2, const float* __restrict__ new_sdf, const unsigned* __restrict__ rgba, long long n,
                                                            float* __restrict__ out_fast, float* __restrict__ out_ref) {
    __shared__ float s_c255[256];
    s_c255[threadIdx.x] = (float)threadIdx.x / 255.0f;
    __syncthreads();
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    if (i >= n) return;
    float a[5] = {s[i], w[i], c0[i], c1[i], c2[i]}, b[5] = {a[0], a[1], a[2], a[3], a[4]};
    voxel_update<true>(a[0], a[1], a[2], a[3], a[4], new_sdf[i], rgba[i], s_c255);
    voxel_update<false>(b[0], b[1], b[2], b[3], b[4], new_sdf[i], rgba[i], s_c255);
    for (int k = 0; k < 5; ++k) { out_fast[5 * i + k] = a[k]; out_ref[5 * i + k] = b[k]; }
}
__global__ void k_debug_rcp(const float* __restrict__ x, long long n, float* __restrict__ out) {
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    if (i < n) out[i] = __builtin_amdgcn_rcpf(x[i]);
}
// k_integrate's structured gather (volume_core.hpp gather2d) of n pixels (u, v) of one frame of a stack of packed images; column_test == 0: the
// descriptor alone (vindex = v, voffset = u * 8), what the hardware's own range check makes of them
__global__ void k_debug_gather2d(const uint2* __restrict__ img, int width, int height, int frame, int column_test, const int* __restrict__ uv, long long n,
                                 uint2* __restrict__ out) {
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    if (i >= n) return;
    int fo = frame;
    asm volatile("" : "+s"(fo));
    const px_v4i rsrc = gather2d_rsrc(img + (size_t)fo * ((size_t)width * height), width, height);
    const px_v2u r = column_test ? gather2d(rsrc, uv[2 * i], uv[2 * i + 1], width) : op_struct_buffer_load_b64(rsrc, uv[2 * i + 1], uv[2 * i] << 3, 0, 0);
    out[i] = make_uint2(r.x, r.y);
}

// ---------------------------------------------------------------------------------------------
// export / import / merge kernels
// ---------------------------------------------------------------------------------------------
// SoA pool -> AoS {sdf,w,c0,c1,c2} x 512 for blocks [first, first+count)
} // namespace

namespace opv {

// A batch of the exact update leaves the summaries of the blocks it touches exact (k_integrate restates them) and touches nothing else: views of the
// volume after it may go on using what is known.  Needs the summary array (a raycast has run on this volume) in the pool's current size and epoch.
bool vol_fusion_keeps_summaries(const op_volume* v) {
    const bool sum_form = v->update_mode == OP_VOLUME_UPDATE_SUM_FORM && v->trunc < 1.0f;
    return !sum_form && v->rc_sum != nullptr && v->rc_cap >= v->max_blocks && (v->content_gen >> 30) == v->rc_sum_epoch;
}

// k_integrate's instantiations: every update form with every gather form, and no other
enum { kUpdSum, kUpdLean, kUpdPlain, kUpdGeneral, kUpdSigned };  // SUMF / PLAIN + LEAN / PLAIN / neither / SIGNED
enum { kGatExact, kGatFastRaw, kGatFast2d };                     // the exact projection with the raw gather; the certified one with the raw and with the structured gather
template <int UPD, int GAT>
void launch_kc(op_volume* v, const BatchInv& I, const CamParams& C, int nf, bmask_t sign, unsigned* rc_sum) {
    constexpr bool kSum = UPD == kUpdSum, kSigned = UPD == kUpdSigned;
    constexpr int kZt = kSum ? KC_ZT_SUM : KC_ZT;
    hipLaunchKernelGGL((k_integrate<GAT != kGatExact, (UPD <= kUpdPlain), kZt, kSum, UPD == kUpdLean, GAT == kGatFast2d, kSigned>),
                       dim3(kSum ? kColGridSum : kSigned ? kSignedGrid : kColGrid), dim3(512 / kZt), 0, v->stream, I, C, v->view(), (const uint2*)v->pimg, v->state, nf,
                       v->upd_partial, v->sel_partial, v->chg_partial, v->plain_from, rc_sum, (unsigned)(v->content_gen & 0x3fffffffull), sign, v->dei_partial);
}

void launch_integrate(op_volume* v, const BatchInv& I, const CamParams& C, int nf, bmask_t sign) {
    // The sum form tests TSDFVoxel::IsValid on the STORED voxel once per batch where the reference re-tests it before every frame (Integrator.cpp:74-87,
    // TSDFVoxel.h:75-78): the two agree to rounding only while no OBSERVATION can itself be invalid, i.e. truncation < 1 (an observed sdf is < truncation;
    // a stored voxel of any origin gets the test).  With truncation >= 1 the exact update runs, whatever the option says.
    // A batch that holds a de-integration (sign != 0) is exact whatever the option says, and the host has invalidated the summaries (vol_enqueue_batch).
    const bool sum_form = !sign && v->update_mode == OP_VOLUME_UPDATE_SUM_FORM && v->trunc < 1.0f;
    // the raycaster's summaries are kept current by this launch (vol_fusion_keeps_summaries: the host has then NOT advanced the content generation)
    unsigned* rc_sum = !sign && vol_fusion_keeps_summaries(v) ? v->rc_sum : nullptr;
    // LEAN (see voxel_update): what the volume holds was fused by the exact update with truncations <= 0.5 only, in at most 2^19 frames, this batch
    // included (a replayed batch counts again: the bound is a sufficient one).  !(<=) so that a NaN truncation counts as too large.
    // (A signed launch: vol_enqueue_batch has ended plain and lean_ok until the volume is cleared.)
    if (sum_form || !(v->trunc <= 0.5f)) v->lean_ok = false;
    v->lean_frames += (uint64_t)nf;
    const bool lean = v->plain && v->lean_ok && v->lean_frames <= (1ull << 19);
    const int upd = sign ? kUpdSigned : sum_form ? kUpdSum : lean ? kUpdLean : v->plain ? kUpdPlain : kUpdGeneral;
    // the structured gather: certified projection and rows that fit the descriptor's stride field (2047 pixels), else the raw form.
    // The certified kinds project without the window test on Z: they need the host's bound on |Z| for every frame of THIS launch (zwin_cert.hpp;
    // a replayed batch comes here again with its logged BatchInv).  A batch with a frame it refuses -- an absurd pose or resolution --
    // takes the exact projection, which needs nothing.
    const bool zwin = C.fast_px && zwin_certified_batch(&I.f[0].m[0], nf, C.res);
    const int gat = !zwin ? kGatExact : gather2d_fits(C.width) ? kGatFast2d : kGatFastRaw;
    typedef void (*launch_fn)(op_volume*, const BatchInv&, const CamParams&, int, bmask_t, unsigned*);
    static const launch_fn table[5][3] = {
        {launch_kc<kUpdSum, kGatExact>, launch_kc<kUpdSum, kGatFastRaw>, launch_kc<kUpdSum, kGatFast2d>},
        {launch_kc<kUpdLean, kGatExact>, launch_kc<kUpdLean, kGatFastRaw>, launch_kc<kUpdLean, kGatFast2d>},
        {launch_kc<kUpdPlain, kGatExact>, launch_kc<kUpdPlain, kGatFastRaw>, launch_kc<kUpdPlain, kGatFast2d>},
        {launch_kc<kUpdGeneral, kGatExact>, launch_kc<kUpdGeneral, kGatFastRaw>, launch_kc<kUpdGeneral, kGatFast2d>},
        {launch_kc<kUpdSigned, kGatExact>, launch_kc<kUpdSigned, kGatFastRaw>, launch_kc<kUpdSigned, kGatFast2d>}};
    ++v->kc_gather_launches[gat];
    table[upd][gat](v, I, C, nf, sign, rc_sum);
}

void kc_trace_dump(op_volume* v) {
#ifdef KC_TRACE
    if (hipSetDevice(v->device) == hipSuccess && hipDeviceSynchronize() == hipSuccess) {
        const int nw = kColGrid * (8 / KC_ZT);
        std::vector<unsigned long long> t((size_t)4096 * 4 * 8);
        if (hipMemcpyFromSymbol(t.data(), HIP_SYMBOL(g_kc_trace), t.size() * 8) == hipSuccess) {
            double sum[8] = {0}, mx[8] = {0};
            for (int w = 0; w < nw; ++w)
                for (int k = 0; k < 8; ++k) { const double d = (double)t[(size_t)w * 8 + k]; sum[k] += d; mx[k] = std::max(mx[k], d); }
            const double n = nw;
            fprintf(stderr, "kc trace (shader cycles per wave of the last launch, %d waves; mean/max): draw+list %.0f/%.0f metadata+voxels %.0f/%.0f frames %.0f/%.0f stores %.0f/%.0f barrier %.0f/%.0f tail %.0f/%.0f | blocks %.1f/%.0f frames applied %.0f/%.0f\n",
                    nw, sum[0] / n, mx[0], sum[1] / n, mx[1], sum[2] / n, mx[2], sum[3] / n, mx[3], sum[4] / n, mx[4], sum[5] / n, mx[5], sum[6] / n, mx[6], sum[7] / n, mx[7]);
        }
    }
#else
    (void)v;
#endif
#ifdef OP_PX_TRACE
    unsigned long long pw[2] = {0, 0};
    if (hipSetDevice(v->device) == hipSuccess && hipDeviceSynchronize() == hipSuccess && hipMemcpyFromSymbol(pw, HIP_SYMBOL(g_px_waves), sizeof(pw)) == hipSuccess)
        fprintf(stderr, "px trace (k_integrate, since load): %llu wave-projections, %llu took the exact fallback (%.3f %%)\n", pw[0], pw[1],
                pw[0] ? 100.0 * (double)pw[1] / (double)pw[0] : 0.0);
#endif
}

} // namespace opv

extern "C" {

int op_debug_voxel_update(const float* s, const float* w, const float* c0, const float* c1, const float* c2, const float* new_sdf, const unsigned* rgba, long long n,
                          float* out_fast, float* out_ref) {
    if (!s || !w || !c0 || !c1 || !c2 || !new_sdf || !rgba || !out_fast || !out_ref) return fail(OP_ERR_INVALID, "null argument");
    if (n < 0 || n > (1ll << 28)) return fail(OP_ERR_INVALID, "n out of range [0, 2^28]");
    OP_TRY(op::use_device(0));
    if (n == 0) return OP_OK;
    const size_t N = (size_t)n;
    op::Scope tmp; // (the hooks here run on the null stream)
    tmp.bind(nullptr);
    float* d_in = nullptr;   // 7 operand planes of n words
    float* d_out = nullptr;  // out_fast, out_ref: n x 5 each
    OP_TRY(tmp.alloc(&d_in, 7 * N));
    OP_TRY(tmp.alloc(&d_out, 10 * N));
    const void* src[7] = {s, w, c0, c1, c2, new_sdf, rgba};
    for (int k = 0; k < 7; ++k) OP_HIP(hipMemcpy(d_in + k * N, src[k], N * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_debug_voxel_update, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, 0, (const float*)d_in, (const float*)(d_in + N), (const float*)(d_in + 2 * N),
                       (const float*)(d_in + 3 * N), (const float*)(d_in + 4 * N), (const float*)(d_in + 5 * N), (const unsigned*)(d_in + 6 * N), n, d_out, d_out + 5 * N);
    OP_HIP(hipMemcpy(out_fast, d_out, 5 * N * 4, hipMemcpyDeviceToHost));
    OP_HIP(hipMemcpy(out_ref, d_out + 5 * N, 5 * N * 4, hipMemcpyDeviceToHost));
    return OP_OK;
}

int op_debug_rcp(const float* x, long long n, float* out) {
    if (!x || !out) return fail(OP_ERR_INVALID, "null argument");
    if (n < 0 || n > (1ll << 28)) return fail(OP_ERR_INVALID, "n out of range [0, 2^28]");
    OP_TRY(op::use_device(0));
    if (n == 0) return OP_OK;
    const size_t N = (size_t)n;
    op::Scope tmp;
    tmp.bind(nullptr);
    float* d = nullptr;      // x, then out
    OP_TRY(tmp.alloc(&d, 2 * N));
    OP_HIP(hipMemcpy(d, x, N * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_debug_rcp, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, 0, (const float*)d, n, d + N);
    OP_HIP(hipMemcpy(out, d + N, N * 4, hipMemcpyDeviceToHost));
    return OP_OK;
}

double op_debug_px_rcp_err(void) { return kPxRcpErr; }

int op_debug_volume_gather_kinds(op_volume* v, unsigned long long* out) {
    if (!v || !out) return fail(OP_ERR_INVALID, "null argument");
    for (int k = 0; k < 3; ++k) out[k] = (unsigned long long)v->kc_gather_launches[k];
    return OP_OK;
}

int op_debug_gather2d(const unsigned* images, int width, int height, int n_frames, int frame, int column_test, const int* uv, long long n, unsigned* out) {
    if (!images || !uv || !out) return fail(OP_ERR_INVALID, "null argument");
    if (width <= 0 || !gather2d_fits(width) || height <= 0 || n_frames <= 0 || frame < 0 || frame >= n_frames || (long long)width * height * n_frames > (1ll << 24))
        return fail(OP_ERR_INVALID, "op_debug_gather2d: rows of 1 .. %d pixels, a frame of the stack, at most 2^24 pixels in all", kGather2dMaxWidth);
    if (n < 0 || n > (1ll << 24)) return fail(OP_ERR_INVALID, "n out of range [0, 2^24]");
    for (long long i = 0; i < 2 * n; ++i) // what project_pixel_uv can return: a certified |t''| is below 2^23
        if (uv[i] < -(1 << 23) || uv[i] >= (1 << 23)) return fail(OP_ERR_INVALID, "op_debug_gather2d: coordinates in [-2^23, 2^23)");
    if (!column_test) // the descriptor alone: whatever the hardware checks, base + v * stride + u * 8 has to stay inside the stack
        for (long long i = 0; i < n; ++i) {
            const long long rec = ((long long)frame * height + uv[2 * i + 1]) * width + uv[2 * i];
            if (rec < 0 || rec >= (long long)width * height * n_frames) return fail(OP_ERR_INVALID, "op_debug_gather2d: without the column test every address must lie in the stack");
        }
    OP_TRY(op::use_device(0));
    if (n == 0) return OP_OK;
    const size_t N = (size_t)n, img_bytes = (size_t)width * height * n_frames * 8;
    op::Scope tmp;
    tmp.bind(nullptr);
    char* d = nullptr;       // the images, then uv, then out
    OP_TRY(tmp.alloc(&d, img_bytes + 16 * N));
    OP_HIP(hipMemcpy(d, images, img_bytes, hipMemcpyHostToDevice));
    OP_HIP(hipMemcpy(d + img_bytes, uv, 8 * N, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_debug_gather2d, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, 0, (const uint2*)d, width, height, frame, column_test, (const int*)(d + img_bytes), n,
                       (uint2*)(d + img_bytes + 8 * N));
    OP_HIP(hipMemcpy(out, d + img_bytes + 8 * N, 8 * N, hipMemcpyDeviceToHost));
    return OP_OK;
}

} // extern "C"
