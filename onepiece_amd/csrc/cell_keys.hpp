// cell_keys.hpp -- what downsample.hip and mesh_cluster.hip share: the cell of a coordinate, the coalesced load of 12-byte rows, the bounds
// of a set of cells and the packed sort key built from them.  Both restate a host loop whose cell is (int)floorf(p / grid_len).
#pragma once
#include <climits>
#include <cstddef>

#include "common.hpp"

namespace op {
namespace cells {

constexpr int kThreads = 256;
constexpr int kAxisBits = 21;   // widest extent of one axis, in cells: 3 x 21 = 63 key bits
constexpr unsigned kBadPoint = 1u;

// The 7 words the host reads back after a bounds kernel.
struct Bounds { unsigned error; int lo[3]; int hi[3]; };

struct KeyLayout { int lo[3]; int shift[3]; }; // key = sum over the axes of (cell - lo) << shift

// (int)floorf(p / grid_len): what PointCloud.cpp:94 and TriangleMesh.cpp:123 compute.  ok = the host's cast is defined (finite, inside int).
__device__ inline int cell_of(float p, float grid_len, bool& ok) {
    const float f = floorf(p / grid_len);
    ok = ok && f >= -2147483648.0f && f < 2147483648.0f; // false for NaN; an infinite p gives an infinite f
    return ok ? (int)f : 0;
}

// A workgroup's 3 * kThreads consecutive floats -> one point per thread.  The loads are consecutive dwords per lane (a 12-byte read per lane
// would touch three cache lines a wave-instruction); the LDS reads have stride 3, which is odd: no bank conflict.
__device__ inline void load_points(const float* __restrict__ xyz, size_t n, float (&tile)[3 * kThreads], float& x, float& y, float& z) {
    const size_t base = (size_t)blockIdx.x * kThreads * 3, end = n * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const size_t e = base + (size_t)k * kThreads + threadIdx.x;
        tile[k * kThreads + threadIdx.x] = e < end ? xyz[e] : 0.0f;
    }
    __syncthreads();
    x = tile[3 * threadIdx.x]; y = tile[3 * threadIdx.x + 1]; z = tile[3 * threadIdx.x + 2];
}

__device__ inline int wave_min(int v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v = min(v, __shfl_xor(v, m, op::kWave));
    return v;
}
__device__ inline int wave_max(int v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v = max(v, __shfl_xor(v, m, op::kWave));
    return v;
}

// The workgroup's share of Bounds: per-axis min / max over the threads with `mine` (wave reduction, then one integer atomic per workgroup and
// word); `error` (0 or flag bits) is ORed in.  Called by every thread of a kThreads workgroup.
__device__ inline void fold_bounds(bool mine, const int (&c)[3], unsigned error, Bounds* __restrict__ bounds) {
    __shared__ int part[kThreads / op::kWave][6];
    __shared__ unsigned bad_any;
    if (threadIdx.x == 0) bad_any = 0u;
    __syncthreads();
    if (error) atomicOr(&bad_any, error);
    const int lane = threadIdx.x & (op::kWave - 1), wave = threadIdx.x / op::kWave;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int lo = wave_min(mine ? c[k] : INT_MAX), hi = wave_max(mine ? c[k] : INT_MIN);
        if (lane == 0) { part[wave][k] = lo; part[wave][3 + k] = hi; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        int v = part[0][threadIdx.x];
        for (int w = 1; w < kThreads / op::kWave; ++w) v = threadIdx.x < 3 ? min(v, part[w][threadIdx.x]) : max(v, part[w][threadIdx.x]);
        if (threadIdx.x < 3) atomicMin(&bounds->lo[threadIdx.x], v); else atomicMax(&bounds->hi[threadIdx.x - 3], v);
    }
    if (threadIdx.x == 0 && bad_any) atomicOr(&bounds->error, bad_any);
}

// every point passed the bounds kernel: 0 <= cell - lo < 2^21, formed in 64 bits (the difference of two ints)
__device__ inline unsigned long long pack_key(const float (&p)[3], float grid_len, const KeyLayout& layout) {
    bool ok = true;
    unsigned long long key = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) key |= (unsigned long long)((long long)cell_of(p[k], grid_len, ok) - (long long)layout.lo[k]) << layout.shift[k];
    return key;
}

inline unsigned blocks_for(size_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// bits that hold 0 .. extent - 1
inline int bits_for(long long extent) {
    int b = 0;
    while ((1ll << b) < extent) ++b;
    return b;
}

// Bounds -> the key's layout (z lowest, as the library's other packed cell keys) and the bits a sort has to look at.  `what`: "cloud", "mesh".
inline int key_layout(const Bounds& bounds, float grid_len, const char* what, KeyLayout* layout, int* total_bits) {
    int bits = 0;
    for (int k = 2; k >= 0; --k) {
        const long long extent = (long long)bounds.hi[k] - (long long)bounds.lo[k] + 1;
        if (extent > (1ll << kAxisBits))
            return fail(OP_ERR_CAPACITY, "the %s spans %lld cells of %g on axis %d (cells %d .. %d): more than the 2^%d a packed key holds", what, extent,
                        (double)grid_len, k, bounds.lo[k], bounds.hi[k], kAxisBits);
        layout->lo[k] = bounds.lo[k];
        layout->shift[k] = bits;
        bits += bits_for(extent);
    }
    *total_bits = bits < 1 ? 1 : bits; // one cell: a one-bit sort of equal keys
    return OP_OK;
}

inline int check_grid_len(float grid_len) {
    return grid_len > 0.0f && std::isfinite(grid_len) ? OP_OK : fail(OP_ERR_INVALID, "grid_len must be positive and finite (got %g)", (double)grid_len);
}

} // namespace cells
} // namespace op
