// volume_gc.hip -- op_volume_collect_garbage (include/onepiece_hip.h): drops the blocks of a volume that lie outside a box of block ids or
// hold no voxel of weight > 0 and >= min_weight, and compacts the pool in place.  The reference declares CubeHandler::CollectGarbage()
// (Integration/CubeHandler.h:357) and never defines it; the predicate on a voxel is the weight half of TSDFVoxel::IsValid (TSDFVoxel.h:75-78).
//
// Steps, all on the volume's stream (n = blocks before, m = blocks kept):
//   k_gc_classify   one wave per block over the 2 KB weight plane only (two 16-byte loads = eight weights per lane), the box test on the key,
//                   one flag byte per pool slot: kGcKept, kGcOutside, kGcUnobserved
//   k_gc_count      per chunk of kGcChunk slots: how many of each flag
//   k_gc_scan       one workgroup: the exclusive prefix of the kept counts over the chunks, the totals (m and the two removal counts), and the
//                   number of kept slots below m -- m minus that is the number of blocks that have to move
//   (the host reads those five numbers; with nothing dropped the call ends here)
//   k_gc_lists      the dropped slots below m in ascending order (holes h_0 < h_1 < ...) and the kept slots at or above m in ascending order
//                   (tails t_0 < t_1 < ...): a slot's rank is its position minus / its number of kept slots before it, from the chunk prefix
//                   and a scan inside the chunk
//   k_gc_move       one workgroup per pair: block t_j -> slot h_j, 2560 floats as 640 16-byte accesses, then the three key ints.  Sources
//                   (>= m) and destinations (< m) are disjoint sets of slots, so nothing is read after it was overwritten
//   refill [m, n) with the default voxel, n_blocks = m, clear the table and re-enter keys[0, m) (volume.hip's kernels, as after a growth)
// Every value is written with ordinary (vector) stores from plain C++; the only atomics are k_rehash's CAS on the table keys.
#include "volume_core.hpp"

namespace {

constexpr unsigned char kGcKept = 0, kGcOutside = 1, kGcUnobserved = 2, kGcBeyond = 3; // kGcBeyond: the padding of the last chunk (slots >= n)
constexpr unsigned kGcChunk = 1024;   // slots per chunk: 256 threads x one 4-byte word of flags
constexpr unsigned kGcScanThreads = 1024;
enum { kGcResKept = 0, kGcResOutside, kGcResUnobserved, kGcResMoved, kGcResKeptBelow, kGcResWords = 8 };

struct GcBox { int use, lo[3], hi[3]; };

// observed(w): the issue's one comparison pair.  NaN and negative weights fail the first compare
__device__ __forceinline__ bool gc_observed(float w, float min_weight) { return w > 0.0f && w >= min_weight; }

__global__ void __launch_bounds__(256) k_gc_classify(const float* __restrict__ pool, const int* __restrict__ keys, unsigned n, float min_weight, GcBox box,
                                                     unsigned char* __restrict__ flags) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned slot = blockIdx.x * 4u + (threadIdx.x >> 6); // wave-uniform
    if (slot >= n) return;
    const float4* wp = reinterpret_cast<const float4*>(pool + (size_t)slot * kBlockFloats + kVox); // the weight plane: 128 float4, 16-byte aligned (a block is 10240 bytes)
    const float4 a = wp[lane], b = wp[lane + 64];
    const float w8[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    bool mine = false;
#pragma unroll
    for (int k = 0; k < 8; ++k) mine = mine || gc_observed(w8[k], min_weight);
    const bool observed = __builtin_amdgcn_ballot_w64(mine) != 0ull;
    if (lane == 0) {
        bool inside = true;
        if (box.use) {
            const int x = keys[3 * (size_t)slot], y = keys[3 * (size_t)slot + 1], z = keys[3 * (size_t)slot + 2];
            inside = box.lo[0] <= x && x <= box.hi[0] && box.lo[1] <= y && y <= box.hi[1] && box.lo[2] <= z && z <= box.hi[2];
        }
        flags[slot] = !inside ? kGcOutside : (observed ? kGcKept : kGcUnobserved);
    }
}

// how many of the four flag bytes of `word` equal f
__device__ __forceinline__ unsigned gc_count4(unsigned word, unsigned f) {
    unsigned c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) c += ((word >> (8 * k)) & 0xffu) == f ? 1u : 0u;
    return c;
}

// sums of three values over a workgroup of 256 threads; the result is valid in thread 0
__device__ __forceinline__ void gc_block_sum3(unsigned& a, unsigned& b, unsigned& c) {
    __shared__ unsigned part[3][4];
    a = wave_sum(a); b = wave_sum(b); c = wave_sum(c);
    if ((threadIdx.x & 63u) == 0) { part[0][threadIdx.x >> 6] = a; part[1][threadIdx.x >> 6] = b; part[2][threadIdx.x >> 6] = c; }
    __syncthreads();
    a = part[0][0] + part[0][1] + part[0][2] + part[0][3];
    b = part[1][0] + part[1][1] + part[1][2] + part[1][3];
    c = part[2][0] + part[2][1] + part[2][2] + part[2][3];
}

__global__ void __launch_bounds__(256) k_gc_count(const unsigned* __restrict__ flag_words, unsigned* __restrict__ counts /* [chunks][4] */) {
    const unsigned word = flag_words[(size_t)blockIdx.x * (kGcChunk / 4) + threadIdx.x];
    unsigned kept = gc_count4(word, kGcKept), outside = gc_count4(word, kGcOutside), unobs = gc_count4(word, kGcUnobserved);
    gc_block_sum3(kept, outside, unobs);
    if (threadIdx.x == 0) {
        counts[4 * (size_t)blockIdx.x] = kept; counts[4 * (size_t)blockIdx.x + 1] = outside; counts[4 * (size_t)blockIdx.x + 2] = unobs;
    }
}

// One workgroup.  Thread t owns the chunks [t * per, (t + 1) * per): their kept counts are summed, the sums scanned over the workgroup, and the
// exclusive prefix of every chunk written to chunk_off.  res: the totals, and kept slots below m (the chunk prefix plus a count inside m's chunk).
__global__ void __launch_bounds__(kGcScanThreads) k_gc_scan(const unsigned* __restrict__ counts, unsigned chunks, const unsigned* __restrict__ flag_words, unsigned n,
                                                            unsigned* __restrict__ chunk_off, unsigned* __restrict__ res) {
    __shared__ unsigned s_kept[kGcScanThreads], s_tot[3], s_below;
    const unsigned t = threadIdx.x, per = (chunks + kGcScanThreads - 1) / kGcScanThreads;
    const unsigned first = t * per, last = first + per < chunks ? first + per : chunks; // (first may exceed chunks: an empty range)
    unsigned kept = 0, outside = 0, unobs = 0;
    for (unsigned c = first; c < last; ++c) { kept += counts[4 * (size_t)c]; outside += counts[4 * (size_t)c + 1]; unobs += counts[4 * (size_t)c + 2]; }
    if (t == 0) { s_tot[0] = 0; s_tot[1] = 0; s_tot[2] = 0; s_below = 0; }
    s_kept[t] = kept;
    __syncthreads();
    for (unsigned d = 1; d < kGcScanThreads; d <<= 1) { // inclusive scan (Hillis-Steele)
        const unsigned add = t >= d ? s_kept[t - d] : 0u;
        __syncthreads();
        s_kept[t] += add;
        __syncthreads();
    }
    unsigned run = s_kept[t] - kept; // exclusive prefix of this thread's first chunk
    for (unsigned c = first; c < last; ++c) { chunk_off[c] = run; run += counts[4 * (size_t)c]; }
    atomicAdd(&s_tot[1], outside); atomicAdd(&s_tot[2], unobs); // (LDS atomics)
    __syncthreads(); // chunk_off is also visible to this workgroup's own reads below
    const unsigned m = s_kept[kGcScanThreads - 1];
    if (m < n) { // kept slots below m: m's chunk prefix plus the kept flags of that chunk in front of m
        const unsigned c = m / kGcChunk;
        if (t < kGcChunk / 4) {
            const unsigned word = flag_words[(size_t)c * (kGcChunk / 4) + t];
            unsigned cnt = 0;
#pragma unroll
            for (unsigned k = 0; k < 4; ++k) cnt += (c * kGcChunk + 4 * t + k < m && ((word >> (8 * k)) & 0xffu) == kGcKept) ? 1u : 0u;
            if (cnt) atomicAdd(&s_below, cnt);
        }
        __syncthreads();
        if (t == 0) s_below += chunk_off[c];
    } else if (t == 0) {
        s_below = m; // every slot is kept
    }
    __syncthreads();
    if (t == 0) {
        res[kGcResKept] = m; res[kGcResOutside] = s_tot[1]; res[kGcResUnobserved] = s_tot[2];
        res[kGcResMoved] = m - s_below; res[kGcResKeptBelow] = s_below;
        res[5] = 0; res[6] = 0; res[7] = 0;
    }
}

// One workgroup per chunk.  kept_before(i) = chunk_off[chunk] + kept flags of the chunk in front of i.  A dropped slot i < m is hole number
// i - kept_before(i) (the dropped slots in front of it); a kept slot i >= m is tail number kept_before(i) - kept_below_m.
__global__ void __launch_bounds__(256) k_gc_lists(const unsigned* __restrict__ flag_words, const unsigned* __restrict__ chunk_off, const unsigned* __restrict__ res,
                                                   unsigned* __restrict__ holes, unsigned* __restrict__ tails) {
    __shared__ unsigned s_wave[4];
    const unsigned m = res[kGcResKept], kept_below = res[kGcResKeptBelow], moved = res[kGcResMoved];
    const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const unsigned word = flag_words[(size_t)blockIdx.x * (kGcChunk / 4) + t];
    const unsigned mine = gc_count4(word, kGcKept);
    unsigned incl = mine; // inclusive scan over the wave
    for (unsigned d = 1; d < 64; d <<= 1) { const unsigned o = __shfl_up(incl, d, 64); if (lane >= d) incl += o; }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    unsigned before = chunk_off[blockIdx.x] + incl - mine;
    for (unsigned w = 0; w < wave; ++w) before += s_wave[w];
#pragma unroll
    for (unsigned k = 0; k < 4; ++k) {
        const unsigned i = blockIdx.x * kGcChunk + 4 * t + k, f = (word >> (8 * k)) & 0xffu;
        if (f == kGcKept) {
            if (i >= m) { const unsigned j = before - kept_below; if (j < moved) tails[j] = i; }
            ++before;
        } else if (f != kGcBeyond && i < m) {
            const unsigned j = i - before;
            if (j < moved) holes[j] = i;
        }
    }
}

// One workgroup per pair: the block in slot tails[j] goes to slot holes[j] (five planes = 640 float4, then the key).
__global__ void __launch_bounds__(256) k_gc_move(float* __restrict__ pool, int* __restrict__ keys, const unsigned* __restrict__ holes, const unsigned* __restrict__ tails,
                                                  unsigned n_slots) {
    const unsigned src = tails[blockIdx.x], dst = holes[blockIdx.x];
    if (src >= n_slots || dst >= src) return; // (cannot happen: a hole lies below m, a tail at or above it)
    const float4* from = reinterpret_cast<const float4*>(pool + (size_t)src * kBlockFloats);
    float4* to = reinterpret_cast<float4*>(pool + (size_t)dst * kBlockFloats);
    for (unsigned i = threadIdx.x; i < kBlockFloats / 4; i += 256) to[i] = from[i];
    if (threadIdx.x < 3) keys[3 * (size_t)dst + threadIdx.x] = keys[3 * (size_t)src + threadIdx.x];
}

} // namespace

extern "C" {

int op_volume_collect_garbage(op_volume* v, float min_weight, const int32_t box_lo[3], const int32_t box_hi[3], op_volume_collect_stats* stats) {
    if (!v) { OP_TRY(op::use_device(0)); return fail(OP_ERR_INVALID, "null volume"); } // the device comes first, as for the other extensions
    OP_HIP(hipSetDevice(v->device));
    v->last_collect = op_volume_collect_stats{};
    if (!(min_weight >= 0.0f) || std::isinf(min_weight)) return fail(OP_ERR_INVALID, "op_volume_collect_garbage: min_weight must be finite and >= 0");
    if ((box_lo == nullptr) != (box_hi == nullptr)) return fail(OP_ERR_INVALID, "op_volume_collect_garbage: box_lo and box_hi must both be given or both be NULL");
    op_volume_collect_stats st{};
    if (stats) *stats = st;
    unsigned n = 0;
    OP_TRY(vol_block_count(v, &n)); // vol_check: every accepted frame is fused, the log is empty, the stream idle
    st.blocks_before = st.blocks_kept = n;
    v->last_collect = st;
    if (n == 0) { if (stats) *stats = st; return OP_OK; }

    GcBox box{};
    if (box_lo) { box.use = 1; for (int a = 0; a < 3; ++a) { box.lo[a] = box_lo[a]; box.hi[a] = box_hi[a]; } }
    const unsigned chunks = (n + kGcChunk - 1) / kGcChunk;
    op::Scope tmp;
    tmp.bind(v->stream);
    unsigned char* flags = nullptr;
    unsigned *counts = nullptr, *chunk_off = nullptr, *res = nullptr, *holes = nullptr, *tails = nullptr;
    OP_TRY(tmp.alloc(&flags, (size_t)chunks * kGcChunk));
    OP_TRY(tmp.alloc(&counts, (size_t)chunks * 4));
    OP_TRY(tmp.alloc(&chunk_off, (size_t)chunks));
    OP_TRY(tmp.alloc(&res, (size_t)kGcResWords));
    OP_HIP(hipMemsetAsync(flags, kGcBeyond, (size_t)chunks * kGcChunk, v->stream));
    hipLaunchKernelGGL(k_gc_classify, dim3((n + 3) / 4), dim3(256), 0, v->stream, (const float*)v->pool, (const int*)v->keys, n, min_weight, box, flags);
    hipLaunchKernelGGL(k_gc_count, dim3(chunks), dim3(256), 0, v->stream, (const unsigned*)flags, counts);
    hipLaunchKernelGGL(k_gc_scan, dim3(1), dim3(kGcScanThreads), 0, v->stream, (const unsigned*)counts, chunks, (const unsigned*)flags, n, chunk_off, res);
    OP_HIP(hipGetLastError());
    unsigned h[kGcResWords] = {};
    OP_HIP(hipMemcpyAsync(h, res, sizeof(h), hipMemcpyDeviceToHost, v->stream));
    OP_HIP(hipStreamSynchronize(v->stream));
    const unsigned m = h[kGcResKept], moved = h[kGcResMoved];
    if (m > n || (unsigned long long)m + h[kGcResOutside] + h[kGcResUnobserved] != n || moved > m || moved > n - m)
        return fail(OP_ERR_HIP, "op_volume_collect_garbage: inconsistent classification (%u kept + %u + %u of %u blocks, %u to move)", m, h[kGcResOutside], h[kGcResUnobserved], n, moved);
    st.blocks_kept = m; st.removed_outside = h[kGcResOutside]; st.removed_unobserved = h[kGcResUnobserved]; st.blocks_moved = moved;
    if (m == n) { v->last_collect = st; if (stats) *stats = st; return OP_OK; } // nothing to drop: the volume is untouched

    if (moved) {
        OP_TRY(tmp.alloc(&holes, (size_t)moved));
        OP_TRY(tmp.alloc(&tails, (size_t)moved));
        OP_HIP(hipMemsetAsync(holes, 0xff, sizeof(unsigned) * (size_t)moved, v->stream)); // an entry the lists did not fill would fail k_gc_move's guard
        OP_HIP(hipMemsetAsync(tails, 0xff, sizeof(unsigned) * (size_t)moved, v->stream));
        hipLaunchKernelGGL(k_gc_lists, dim3(chunks), dim3(256), 0, v->stream, (const unsigned*)flags, (const unsigned*)chunk_off, (const unsigned*)res, holes, tails);
        hipLaunchKernelGGL(k_gc_move, dim3(moved), dim3(256), 0, v->stream, v->pool, v->keys, (const unsigned*)holes, (const unsigned*)tails, n);
    }
    vol_launch_fill_pool(v, m, (size_t)(n - m));      // slots [m, n) are default voxels again, as op_volume_clear leaves them
    OP_HIP(hipMemsetD32Async((hipDeviceptr_t)v->n_blocks, (int)m, 1, v->stream));
    vol_launch_rehash(v, m);                           // no tombstones: the table is cleared and keys[0, m) re-enter it (bmask is zero between launches and stays so)
    OP_HIP(hipGetLastError());
    OP_HIP(hipStreamSynchronize(v->stream));
    if (v->hstat) v->hstat[1] = m;
    // Table slots moved and pool slots changed their meaning: pending op_volume_unpack_sum_begin slots and the raycaster's block summaries are
    // stale (the summaries are NOT moved along with the blocks; the next view marches what it sees and restates them).
    ++v->generation; ++v->content_gen;
    // plain / lean_ok / lean_frames are unchanged: a kept block holds the voxels it held, a freed slot the default voxel, which is what both
    // forms of k_integrate assume of a slot they did not write (integrate.hip, PLAIN / LEAN).  Foreign blocks lay below plain_from and only ever
    // move to a lower slot, below m; every slot from m on is default.
    if (m < v->plain_from) v->plain_from = m;
    v->last_collect = st;
    if (stats) *stats = st;
    return OP_OK;
}

int op_volume_collect_last_stats(op_volume* v, op_volume_collect_stats* stats) {
    if (!v) { OP_TRY(op::use_device(0)); return fail(OP_ERR_INVALID, "null volume"); }
    if (!stats) return fail(OP_ERR_INVALID, "null stats");
    *stats = v->last_collect;
    return OP_OK;
}

} // extern "C"
