// volume_coarsen.hip -- op_volume_coarsen (include/onepiece_hip.h states the definition): a NEW volume of twice the voxel size whose voxel g is the
// weighted mean of the 2 x 2 x 2 fine voxels 2g + {0,1}^3.  Voxel centres sit at (index + 0.5) * res (Integration/VoxelCube.h:49-58 of the reference),
// so a coarse voxel covers exactly eight fine ones and its centre is their centroid: nothing is resampled.  Not in the reference.
//
// Per level, on the result's stream (the source is idle: vol_block_count has synchronised it):
//   k_coarsen_alloc   one thread per source block claims the coarse id (b >> 1 per axis, arithmetic) in the result's table; up to eight claimants
//                     of one id agree on the slot (table_claim).  Idempotent: the host runs it again after vol_block_count grew the result's pool.
//   k_coarsen_fill    one workgroup per result block in pool order, one thread per result voxel.  Threads 0..7 look the eight source blocks up once
//                     (LDS).  Result voxel (x, y, z) of the block reads source block (x >> 2, y >> 2, z >> 2) of the octet, fine voxel
//                     2 (x & 3) + i, 2 (y & 3) + j, 2 (z & 3) + k: the two children along x are ONE 8-byte load per plane, and a wave (one z-slice
//                     of the result block) reads, with the loads of j = 0 and j = 1 together, two whole 256-byte fine z-slices per plane of each
//                     of its four source blocks -- whole cache lines, every source byte once.  The 20 loads of a voxel are issued before the first
//                     sum.  The sums of a voxel are formed by its own lane in the order c = i + 2j + 4k: no tree, no cross-lane step, no atomics.
//                     Per result block: at most 8 x 10 KB read, 10 KB written, 16 bytes of counts.
//   k_coarsen_stats   folds the per-block counts into 64 partial rows (plain stores); the host adds those.
#include "volume_core.hpp"
#include "voxel_interp.hpp"

namespace {

constexpr int kStatParts = 64; // partial rows of k_coarsen_stats (2 KB for the host to read)

__global__ __launch_bounds__(256) void k_coarsen_alloc(VolView S, VolView D, State* dst_state, unsigned n_src) {
    const unsigned b = blockIdx.x * 256u + threadIdx.x;
    if (b >= n_src) return;
    bool created;
    // |id| < 2^20 in the source, so the halved id is in range
    table_claim(D, dst_state, S.keys[3 * (size_t)b] >> 1, S.keys[3 * (size_t)b + 1] >> 1, S.keys[3 * (size_t)b + 2] >> 1, &created);
}

__global__ __launch_bounds__(512) void k_coarsen_fill(VolView S, VolView D, float min_weight, uint4* __restrict__ counts) {
    __shared__ int s_src[8];
    __shared__ unsigned s_part[8];
    const int b = blockIdx.x, vid = threadIdx.x;
    if (vid < 8) {
        const int kx = D.keys[3 * (size_t)b], ky = D.keys[3 * (size_t)b + 1], kz = D.keys[3 * (size_t)b + 2];
        s_src[vid] = table_find(S, 2 * kx + (vid & 1), 2 * ky + ((vid >> 1) & 1), 2 * kz + (vid >> 2));
    }
    __syncthreads();
    const int x = vid & 7, y = (vid >> 3) & 7, z = vid >> 6;
    const int idx = s_src[(x >> 2) + 2 * (y >> 2) + 4 * (z >> 2)];
    float W = 0.0f, Sd = 0.0f, C0 = 0.0f, C1 = 0.0f, C2 = 0.0f;
    unsigned n = 0, dropped = 0;
    if (idx >= 0) {
        // fine voxel (2 (x & 3), 2 (y & 3), 2 (z & 3)): an even x, so the pair along x is 8-byte aligned (a block is 10240 bytes)
        const float* t = S.pool + (size_t)idx * kBlockFloats + (2 * (x & 3) + 16 * (y & 3) + 128 * (z & 3));
        float2 v[4][5]; // [j + 2k][plane]
#pragma unroll
        for (int jk = 0; jk < 4; ++jk)
#pragma unroll
            for (int p = 0; p < 5; ++p) v[jk][p] = *reinterpret_cast<const float2*>(t + p * kVox + 8 * (jk & 1) + 64 * (jk >> 1));
#pragma unroll
        for (int jk = 0; jk < 4; ++jk) {
#pragma unroll
            for (int i = 0; i < 2; ++i) { // c = i + 2j + 4k ascending
                const float s = i ? v[jk][0].y : v[jk][0].x, w = i ? v[jk][1].y : v[jk][1].x;
                const float c0 = i ? v[jk][2].y : v[jk][2].x, c1 = i ? v[jk][3].y : v[jk][3].x, c2 = i ? v[jk][4].y : v[jk][4].x;
                // selects, not branches: the loads above stay unconditional and in flight together.  `use` is false for a NaN weight, and what
                // lies under a weight of 0 (999, NaN, inf) is computed with and thrown away: it never reaches the sums
                const bool seen = w > 0.0f, use = seen && w >= min_weight;
                W = use ? W + w : W;
                Sd = use ? Sd + w * s : Sd;
                C0 = use ? C0 + w * c0 : C0;
                C1 = use ? C1 + w * c1 : C1;
                C2 = use ? C2 + w * c2 : C2;
                n += use ? 1u : 0u;
                dropped += (seen && !use) ? 1u : 0u;
            }
        }
    }
    float* o = D.pool + (size_t)b * kBlockFloats + vid;
    if (n) {
        store_planes(o, Vox5{Sd / W, W * 0.125f, C0 / W, C1 / W, C2 / W});
    } else {
        store_planes(o, default_voxel());
    }
    // the block's counts: per wave at most 64 voxels of a kind (7 bits each) and 512 dropped children (10 bits)
    const unsigned packed = wave_sum((n == 8 ? 1u : 0u) | ((n > 0 && n < 8) ? 1u << 7 : 0u) | (n == 0 ? 1u << 14 : 0u) | (dropped << 21));
    if ((vid & 63) == 0) s_part[vid >> 6] = packed;
    __syncthreads();
    if (vid == 0) {
        uint4 c = make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int k = 0; k < 8; ++k) { const unsigned q = s_part[k]; c.x += q & 0x7fu; c.y += (q >> 7) & 0x7fu; c.z += (q >> 14) & 0x7fu; c.w += q >> 21; }
        counts[b] = c;
    }
}

__global__ __launch_bounds__(256) void k_coarsen_stats(const uint4* __restrict__ counts, unsigned n, unsigned long long* __restrict__ parts /* [kStatParts][4] */) {
    __shared__ unsigned long long s_w[4][4];
    unsigned long long a[4] = {0, 0, 0, 0};
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n; i += kStatParts * 256u) { const uint4 c = counts[i]; a[0] += c.x; a[1] += c.y; a[2] += c.z; a[3] += c.w; }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        for (int o = 32; o > 0; o >>= 1) a[k] += __shfl_xor(a[k], o, 64);
        if ((threadIdx.x & 63u) == 0) s_w[k][threadIdx.x >> 6] = a[k];
    }
    __syncthreads();
    if (threadIdx.x < 4) parts[4 * blockIdx.x + threadIdx.x] = s_w[threadIdx.x][0] + s_w[threadIdx.x][1] + s_w[threadIdx.x][2] + s_w[threadIdx.x][3];
}

// one level: *out is a new volume, st its counts
int coarsen_once(op_volume* src, float min_weight, uint64_t max_blocks, op_volume** out, op_volume_coarsen_stats* st) {
    OP_VOL(src);
    *st = op_volume_coarsen_stats{};
    unsigned ns = 0;
    OP_TRY(vol_block_count(src, &ns));
    // every result block has a source block of its own, so ns blocks always suffice; a surface shell turns ns blocks into ns / 4 .. ns / 6 (164 k -> 26 k
    // -> 4.5 k on the room volume), and the whole pool is filled with default voxels when it is created: start at a third, and let the idempotent
    // allocation pass below run again after a growth if a sparse volume needs more
    if (max_blocks == 0) max_blocks = (uint64_t)ns / 3 + 1024;
    op_volume* dst = nullptr;
    OP_TRY(op_volume_create(&src->cam, 2.0f * src->res, src->trunc, src->far_d, src->near_d, src->device, max_blocks, &dst));
    vol_mark_foreign(dst, max_blocks); // weighted means, weights that are no integers; the bound is tightened below
    st->src_blocks = ns;
    int rc = OP_OK;
    unsigned nd = 0;
    if (ns) {
        rc = vol_claim_until_fit(dst, [&]() -> int { // the (idempotent) allocation pass, again if the result outgrew a pool the caller sized
            hipLaunchKernelGGL(k_coarsen_alloc, dim3((ns + 255) / 256), dim3(256), 0, dst->stream, src->view(), dst->view(), dst->state, ns);
            return OP_OK;
        }, &nd);
        if (rc == OP_OK && nd) {
            op::Scope tmp;
            tmp.bind(dst->stream);
            uint4* counts = nullptr;
            unsigned long long* parts = nullptr;
            rc = tmp.alloc(&counts, (size_t)nd);
            if (rc == OP_OK) rc = tmp.alloc(&parts, (size_t)kStatParts * 4);
            if (rc == OP_OK) {
                hipLaunchKernelGGL(k_coarsen_fill, dim3(nd), dim3(512), 0, dst->stream, src->view(), dst->view(), min_weight, counts);
                hipLaunchKernelGGL(k_coarsen_stats, dim3(kStatParts), dim3(256), 0, dst->stream, (const uint4*)counts, nd, parts);
                unsigned long long h[kStatParts * 4] = {};
                if (hipGetLastError() != hipSuccess || hipMemcpyAsync(h, parts, sizeof(h), hipMemcpyDeviceToHost, dst->stream) != hipSuccess)
                    rc = fail(OP_ERR_HIP, "op_volume_coarsen: launch failed");
                if (rc == OP_OK) rc = vol_check(dst);
                for (int p = 0; rc == OP_OK && p < kStatParts; ++p) {
                    st->voxels_full += h[4 * p]; st->voxels_partial += h[4 * p + 1]; st->voxels_empty += h[4 * p + 2]; st->dropped_min_weight += h[4 * p + 3];
                }
            }
        }
    }
    if (rc != OP_OK) { op_volume_destroy(dst); return rc; }
    dst->plain_from = nd; // exactly the coarsened blocks
    st->dst_blocks = nd;
    *out = dst;
    return OP_OK;
}

} // namespace

extern "C" {

int op_volume_coarsen(op_volume* src, int levels, float min_weight, uint64_t max_blocks, op_volume** out, op_volume_coarsen_stats* stats) {
    // the refusals, before any device work
    if (!out) return fail(OP_ERR_INVALID, "op_volume_coarsen: null out");
    *out = nullptr;
    if (!src) return fail(OP_ERR_INVALID, "op_volume_coarsen: null volume");
    if (levels < 1 || levels > 4) return fail(OP_ERR_INVALID, "op_volume_coarsen: levels must be 1..4 (got %d)", levels);
    if (!(min_weight >= 0.0f)) return fail(OP_ERR_INVALID, "op_volume_coarsen: min_weight must be >= 0");
    op_volume_coarsen_stats st{};
    if (stats) *stats = st;
    op_volume* cur = src;
    for (int l = 0; l < levels; ++l) {
        op_volume* next = nullptr;
        const int rc = coarsen_once(cur, min_weight, max_blocks, &next, &st);
        if (cur != src) op_volume_destroy(cur); // the intermediate level
        if (rc != OP_OK) return rc;
        cur = next;
    }
    if (stats) *stats = st;
    *out = cur;
    return OP_OK;
}

} // extern "C"
