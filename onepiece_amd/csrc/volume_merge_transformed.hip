// volume_merge_transformed.hip -- op_volume_merge_transformed / _many (include/onepiece_hip.h states the definition): CubeHandler::Merge with a
// pose (the reference's Integration/CubeHandler.h:168-177, as its example/MergeMultipleSubmaps.cpp:34-42 uses it) for one or many sources,
// WITHOUT the intermediate volume of op_volume_transform + op_volume_merge: the sources are resampled straight into the destination's blocks.
//
// Per group of at most kGroup = 64 consecutive sources, on the destination's stream (the sources are idle: vol_block_count has synchronised them):
//   k_merge_claim   one workgroup per source block over all sources of the group; it finds its source in the group's table by a wave-uniform
//                   binary search (scalar loads) and runs pass 1 of Transform (transform_body.hpp, the body of k_transform_alloc<false>) with that
//                   source's T, claiming into the DESTINATION's table.  Every claimed block gets bit k of a 64-bit mask (per-call scratch, one word
//                   per table slot -- not the volume's bmask, which belongs to fusion batches) by atomicOr; the lane that sees the word go from 0
//                   appends the table slot to the touched list.  Idempotent but for mask and list: if the claims outgrow the pool, vol_block_count
//                   grows it (which re-hashes) and the pass runs again on a zeroed mask and list.  That is sound because a newly claimed pool slot
//                   holds default voxels (k_fill_pool: at creation, after a clear, over the new part of a grown pool, over what CollectGarbage
//                   frees), so `t.w == 0 -> copy` needs no "fresh" flag.
//   k_merge_fill    one wave per touched block, eight z-slices of 64 voxels (the form of k_transform_fill_wave).  The block's 512 voxels are
//                   loaded ONCE into 10 KB of the wave's LDS (in registers -- 8 slices x 5 values, every slice index a constant, so the tap loop fully
//                   unrolled -- the compiler reports 244 VGPRs and 2 waves per SIMD; in LDS 142 and 3, with the LDS itself admitting 15 waves per
//                   CU: DESIGN.md section 3.11), then for each set bit k of its mask, ascending, pass 2 of
//                   Transform (transform_body.hpp, the body of k_transform_fill_wave) with source k's T^-1 yields r for every voxel and
//                   TSDFVoxel::operator+= (voxel_merge, voxel_interp.hpp: what k_merge_blocks calls) folds it in; the block is stored ONCE.  A destination block is owned
//                   by exactly one wave; blocks outside the union are neither read nor written.  No floating-point atomics anywhere; the counts
//                   go through integer atomics on kParts rows of words (a wave adds to row blockIdx % kParts), which the host adds up.
// Per-call device scratch (op::Scope): the mask (8 B per table slot), the list (4 B per pool slot), the group's source table, the counters -- no
// voxel pool.
#include "volume_core.hpp"
#include "voxel_interp.hpp"
#include "transform_body.hpp"

namespace {

constexpr int kGroup = 64;   // sources per launch pair: one bit of the mask each
constexpr int kParts = 256;  // rows of the counters (7 words each: 14 KB for the host to read, below the size at which a pageable copy is staged)
constexpr int kCnt = 7;      // copied, kept, blended, reset, pairs, touched, created
struct MtSource {
    VolView S;
    Mat4 T, Ti;
    unsigned first; // the source's workgroups are [first, first of the next entry) of k_merge_claim's grid
};

__global__ __launch_bounds__(512) void k_merge_claim(const MtSource* __restrict__ tab, int n_src, VolView D, State* dst_state, float res,
                                                     unsigned long long* __restrict__ mask, int* __restrict__ list, unsigned list_cap, unsigned* __restrict__ n_touched) {
    __shared__ unsigned long long s_set[kClaimSet];
    const unsigned b = blockIdx.x;
    int lo = 0, hi = n_src - 1; // the last entry whose first <= b (entries without blocks share their successor's first and are passed over)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].first <= b) lo = mid; else hi = mid - 1;
    }
    const int k = lo;
    const int* keys = tab[k].S.keys + 3 * (size_t)(b - tab[k].first);
    const Mat4 T = tab[k].T;
    transform_claim_body<false>(s_set, keys[0], keys[1], keys[2], dst_state, T.m, res, [&](int cx, int cy, int cz) {
        bool created;
        const int slot = table_claim(D, dst_state, cx, cy, cz, &created); // AddCube into the destination
        if (slot < 0) return;
        if (atomicOr(&mask[slot], 1ull << k) == 0ull) {
            const unsigned i = atomicAdd(n_touched, 1u);
            if (i < list_cap) list[i] = slot; // (more than the pool holds: the pass runs again after the growth)
        }
    });
}

__global__ __launch_bounds__(64) void k_merge_fill(const MtSource* __restrict__ tab, VolView D, float res, const unsigned long long* __restrict__ mask,
                                                   const int* __restrict__ list, unsigned first_new, unsigned char* __restrict__ seen,
                                                   unsigned long long* __restrict__ parts) {
    __shared__ int s_slot[kSrcBox];
    __shared__ float s_t[kBlockFloats]; // the destination block while the sources are folded into it
    const int lane = threadIdx.x;
    const int slot = list[blockIdx.x];
    const int idx = D.tvals[slot]; // table slot -> pool slot (claimed by the previous kernel)
    if (idx < 0) return;
    const unsigned long long m0 = mask[slot];
    unsigned long long m = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(m0 >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)m0);
    const int kx = D.keys[3 * (size_t)idx], ky = D.keys[3 * (size_t)idx + 1], kz = D.keys[3 * (size_t)idx + 2];
    float* pool = D.pool + (size_t)idx * kBlockFloats + lane;
    float* t = s_t + lane; // voxel lane + 64 zs of plane p: t[p * kVox + 64 * zs] (consecutive lanes, consecutive words: no bank conflicts)
#pragma unroll 8
    for (int i = 0; i < 5 * 8; ++i) t[64 * i] = pool[64 * i];
    const unsigned pairs = (unsigned)__popcll(m);
    unsigned ck = 0, br = 0; // this lane's visits: copied | kept << 16, blended | reset << 16 (at most 8 x 64 of a kind)
    while (m) {
        const int k = __builtin_ctzll(m);
        m &= m - 1;
        const VolView S = tab[k].S;
        const Mat4 Ti = tab[k].Ti;
        transform_fill_wave_body<2>(S, s_slot, kx, ky, kz, Ti.m, res, [&](int zs, const Vox5& r) {
            // voxels[voxel_id] += r (never a fresh block: a newly claimed one holds default voxels, whose weight of 0 means "copy")
            voxel_merge(t + 64 * zs, r, false, [&](int kind) {
                if (kind == kMergeCopied) ck += 1u;
                else if (kind == kMergeKept) ck += 1u << 16;
                else if (kind == kMergeBlended) br += 1u;
                else br += 1u << 16;
            });
        });
        __syncthreads(); // (one wave: the taps of this source have read s_slot before the next source's look-ups overwrite it)
    }
#pragma unroll 8
    for (int i = 0; i < 5 * 8; ++i) pool[64 * i] = t[64 * i];
    ck = wave_sum(ck); br = wave_sum(br); // at most 64 lanes x 512 visits of a kind: 2^15, inside a half word
    if (lane == 0) {
        bool first = true; // the first group of this call that touches the block counts it (a call of one group keeps no `seen` bytes)
        if (seen) { first = seen[idx] == 0; seen[idx] = 1; }
        unsigned long long* row = parts + (size_t)(blockIdx.x % kParts) * kCnt;
        if (ck & 0xffffu) atomicAdd(&row[0], (unsigned long long)(ck & 0xffffu));
        if (ck >> 16) atomicAdd(&row[1], (unsigned long long)(ck >> 16));
        if (br & 0xffffu) atomicAdd(&row[2], (unsigned long long)(br & 0xffffu));
        if (br >> 16) atomicAdd(&row[3], (unsigned long long)(br >> 16));
        atomicAdd(&row[4], (unsigned long long)pairs);
        if (first) atomicAdd(&row[5], 1ull);
        if (first && (unsigned)idx >= first_new) atomicAdd(&row[6], 1ull);
    }
}

// the refusals, before any device use
int merge_transformed_check(const char* who, op_volume* dst, op_volume* const* srcs, const float* Ts, size_t n) {
    if (!dst) return fail(OP_ERR_INVALID, "%s: null volume", who);
    if (n && (!srcs || !Ts)) return fail(OP_ERR_INVALID, "%s: null argument", who);
    for (size_t k = 0; k < n; ++k) {
        if (!srcs[k]) return fail(OP_ERR_INVALID, "%s: source %zu is null", who, k);
        if (srcs[k] == dst) return fail(OP_ERR_INVALID, "%s: cannot merge a volume into itself (source %zu)", who, k);
        if (srcs[k]->device != dst->device) return fail(OP_ERR_INVALID, "%s: source %zu is on another device", who, k);
    }
    for (size_t k = 0; k < n; ++k)
        if (srcs[k]->res != dst->res) // CubeHandler.h:147-151: warn and leave dst untouched
            return fail(OP_ERR_MISMATCH, "[Warning]::[MergeVoxelHash]::Voxel resolution is not identical.");
    return OP_OK;
}

int merge_transformed(const char* who, op_volume* dst, op_volume* const* srcs, const float* Ts, const float* T_invs, size_t n, op_volume_merge_transformed_stats* stats) {
    OP_TRY(merge_transformed_check(who, dst, srcs, Ts, n));
    OP_HIP(hipSetDevice(dst->device));
    op_volume_merge_transformed_stats st{};
    st.sources = n;
    if (stats) *stats = st;
    // like every accessor: what is queued on the destination and on every source is flushed and complete before the kernels below read it
    unsigned nd0 = 0;
    OP_TRY(vol_block_count(dst, &nd0));
    std::vector<unsigned> ns(n, 0u);
    for (size_t k = 0; k < n; ++k) { OP_TRY(vol_block_count(srcs[k], &ns[k])); st.src_blocks += ns[k]; }
    op::Scope call; // what outlives a group: the bytes that keep `touched_blocks` a union across groups
    call.bind(dst->stream);
    unsigned char* seen = nullptr;
    size_t seen_cap = 0;
    std::vector<MtSource> tab;
    for (size_t g0 = 0; g0 < n; g0 += kGroup) {
        const size_t gn = std::min<size_t>(kGroup, n - g0);
        tab.assign(gn, MtSource{});
        unsigned long long total = 0;
        for (size_t j = 0; j < gn; ++j) {
            const size_t k = g0 + j;
            tab[j].S = srcs[k]->view();
            load_transform(Ts + 16 * k, T_invs ? T_invs + 16 * k : nullptr, &tab[j].T, &tab[j].Ti);
            tab[j].first = (unsigned)total;
            total += ns[k];
        }
        if (!total) continue; // nothing but sources without blocks: Transform gives an empty volume, Merge returns at once
        if (total > 0x7fffffffull) return fail(OP_ERR_CAPACITY, "%s: %llu source blocks in one group of %d sources", who, total, kGroup);
        op::Scope s;
        s.bind(dst->stream);
        MtSource* d_tab = nullptr;
        OP_TRY(s.upload(tab, &d_tab));
        unsigned long long *d_mask = nullptr, *d_parts = nullptr;
        int* d_list = nullptr;
        unsigned* d_count = nullptr;
        OP_TRY(s.alloc(&d_count, 1));
        OP_TRY(s.alloc(&d_parts, (size_t)kParts * kCnt));
        unsigned nd = 0, touched = 0;
        // if the claims outgrow the pool, vol_block_count grows it (and re-hashes): mask and list are rebuilt from zero by another pass.  (A coordinate
        // outside the key range is reported by vol_block_count, as op_volume_transform reports it.)
        OP_TRY(vol_claim_until_fit(dst, [&]() -> int {
            OP_TRY(s.alloc(&d_mask, (size_t)dst->table_size));
            OP_TRY(s.alloc(&d_list, (size_t)dst->max_blocks));
            OP_HIP(hipMemsetAsync(d_mask, 0, sizeof(unsigned long long) * (size_t)dst->table_size, dst->stream));
            OP_HIP(hipMemsetAsync(d_count, 0, sizeof(unsigned), dst->stream));
            hipLaunchKernelGGL(k_merge_claim, dim3((unsigned)total), dim3(512), 0, dst->stream, (const MtSource*)d_tab, (int)gn, dst->view(), dst->state, dst->res,
                               d_mask, d_list, dst->max_blocks, d_count);
            OP_HIP(hipGetLastError());
            return OP_OK;
        }, &nd));
        OP_HIP(hipMemcpy(&touched, d_count, sizeof(touched), hipMemcpyDeviceToHost));
        if (!touched) continue;
        if (touched > dst->max_blocks) return fail(OP_ERR_HIP, "%s: %u touched blocks in a pool of %u", who, touched, dst->max_blocks); // (never: every one of them holds a pool slot)
        vol_mark_foreign(dst, nd); // merged means: general weights in the blocks that exist after this group
        if (n > (size_t)kGroup && dst->max_blocks > seen_cap) {
            unsigned char* grown = nullptr;
            OP_TRY(call.alloc(&grown, (size_t)dst->max_blocks));
            OP_HIP(hipMemsetAsync(grown, 0, (size_t)dst->max_blocks, dst->stream));
            if (seen_cap) OP_HIP(hipMemcpyAsync(grown, seen, seen_cap, hipMemcpyDeviceToDevice, dst->stream));
            seen = grown; seen_cap = dst->max_blocks;
        }
        OP_HIP(hipMemsetAsync(d_parts, 0, sizeof(unsigned long long) * kParts * kCnt, dst->stream));
        hipLaunchKernelGGL(k_merge_fill, dim3(touched), dim3(64), 0, dst->stream, (const MtSource*)d_tab, dst->view(), dst->res, (const unsigned long long*)d_mask,
                           (const int*)d_list, nd0, seen, d_parts);
        OP_HIP(hipGetLastError());
        OP_TRY(vol_check(dst));
        std::vector<unsigned long long> h((size_t)kParts * kCnt);
        OP_HIP(hipMemcpy(h.data(), d_parts, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (int p = 0; p < kParts; ++p) {
            const unsigned long long* r = &h[(size_t)p * kCnt];
            st.voxels_copied += r[0]; st.voxels_kept += r[1]; st.voxels_blended += r[2]; st.voxels_reset += r[3];
            st.pairs += r[4]; st.touched_blocks += r[5]; st.created_blocks += r[6];
        }
    }
    if (stats) *stats = st;
    return OP_OK;
}

} // namespace

extern "C" {

int op_volume_merge_transformed_many(op_volume* dst, op_volume* const* srcs, const float* Ts, const float* T_invs, size_t n, op_volume_merge_transformed_stats* stats) {
    return merge_transformed("op_volume_merge_transformed_many", dst, srcs, Ts, T_invs, n, stats);
}

int op_volume_merge_transformed(op_volume* dst, op_volume* src, const float T[16], const float* T_inv, op_volume_merge_transformed_stats* stats) {
    if (dst && !src) return fail(OP_ERR_INVALID, "op_volume_merge_transformed: null src");
    return merge_transformed("op_volume_merge_transformed", dst, &src, T, T_inv, 1, stats);
}

} // extern "C"
