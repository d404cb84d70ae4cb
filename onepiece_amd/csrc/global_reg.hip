// global_reg.hip -- global registration on the device: FPFH features (Registration/3DFeature.cpp), exhaustive feature matching
// (GlobalRegistration.cpp:28-78) and the scoring half of the rigid RANSAC (Ransac.cpp:7-40 over GRANSAC.hpp / TransformationModel.hpp).
// Every kernel restates the host path of host/one_piece/src/GlobalRegistration.cpp and RansacRigid.cpp operation by operation (float32,
// separate multiply and add -- the library is built with -ffp-contract=off -- correctly rounded sqrt and divide), so that the class surface
// can switch paths (OP_RUNTIME_OPT_GLOBAL_REGISTRATION) without changing a result.  The one exception is the atan2 of the first Darboux
// angle: it is evaluated in double on the float operands and rounded once, where the host calls its libm's atan2f (see k_spfh).
// What FPFH is pinned to, beyond the host path: exact radius neighbours (every point with float32 d2 < radius, by (d2, index)) followed by
// the arithmetic of the reference's 3DFeature.cpp, stated independently in numpy by tests/global_registration_common.py (brute force, no
// cells).  Not pinned: nanoflann's approximate radius search that the reference asks with 1024 checks, and the seeding of the RANSAC.
//
//   k_fpfh_neighbours   one wave per point: candidates of the 27 cells around the point, d2 < radius, exact top-knn by (d2, index)
//   k_spfh              one wave per point: pair descriptor + three bins per neighbour, integer histogram in LDS
//   k_fpfh              one wave per point: 1/dist-weighted neighbour histograms in list order, per-third renormalisation
//   k_feature_match     one query per lane (33 registers), targets tiled through LDS, sequential d2, lowest index on ties
//   k_ransac_count      one hypothesis per lane (12 registers), correspondences tiled through LDS, integer counts
//   k_ransac_inlier_ids the ascending inlier list of one hypothesis
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "common.hpp"

namespace {

using op::fail;

constexpr int kBins = 11, kDim = 3 * kBins;
constexpr int kNbMaxK = 256;    // largest knn (DenseSlam asks for 100)
constexpr int kNbBuf = 512;     // keys of a wave's selection buffer: the kept ones plus what arrived since the last cut
constexpr int kCellBits = 21;   // cell coordinates relative to the cloud's lowest cell, 1 .. 2^21 - 2
constexpr unsigned long long kNoKey = ~0ull;

__host__ __device__ inline unsigned long long cell_key(unsigned x, unsigned y, unsigned z) {
    return ((unsigned long long)x << (2 * kCellBits)) | ((unsigned long long)y << kCellBits) | (unsigned long long)z;
}

// first position of sorted `keys` that is not below `k`
__device__ inline unsigned lower_bound_key(const unsigned long long* keys, unsigned n, unsigned long long k) {
    unsigned lo = 0, hi = n;
    while (lo < hi) {
        const unsigned mid = (lo + hi) >> 1;
        if (keys[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ascending bitonic sort of buf[0, n2) by the 64 lanes of the block's one wave; n2 a power of two >= 64
__device__ inline void wave_sort(unsigned long long* buf, int n2, int lane) {
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < (n2 >> 1); t += op::kWave) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const unsigned long long a = buf[i], b = buf[l];
                const bool up = (i & k) == 0;
                if ((a > b) == up) { buf[i] = b; buf[l] = a; }
            }
            __syncthreads();
        }
}

// pads buf[cnt, n2) and sorts; returns the number of kept keys (at most knn)
__device__ inline int wave_cut(unsigned long long* buf, int cnt, int knn, int lane) {
    int n2 = op::kWave;
    while (n2 < cnt) n2 <<= 1;
    for (int t = cnt + lane; t < n2; t += op::kWave) buf[t] = kNoKey;
    __syncthreads();
    wave_sort(buf, n2, lane);
    return cnt < knn ? cnt : knn;
}

// RadiusNeighbours of GlobalRegistration.cpp.  The grid arrives sorted: cell_keys[nc] ascending (x, y, z packed, z lowest), cell_start[nc + 1]
// into cell_points[n].  Within a key run (x + dx, y + dy, z - 1 .. z + 1) the cells are adjacent in that order, so a point's 27 cells are 9
// ranges of cell_points.  What is kept depends on (d2, index) alone: a candidate is one 64-bit key, d2's bits above the index (d2 >= 0, so the
// bit pattern orders like the value), and the knn smallest keys are selected exactly for any number of candidates -- the buffer is cut back to
// the knn best whenever the next 64 candidates might not fit, and from then on only keys below the knn-th best are admitted.
__global__ __launch_bounds__(64) void k_fpfh_neighbours(const float* __restrict__ xyz, const int* __restrict__ pcell, unsigned n,
                                                        const unsigned long long* __restrict__ cell_keys, const unsigned* __restrict__ cell_start,
                                                        unsigned nc, const int* __restrict__ cell_points, float r2, int knn,
                                                        int* __restrict__ nb_out, int* __restrict__ count_out) {
    __shared__ unsigned long long buf[kNbBuf];
    const unsigned i = blockIdx.x;
    const int lane = threadIdx.x;
    if (i >= n) return;
    const float px = xyz[3 * i], py = xyz[3 * i + 1], pz = xyz[3 * i + 2];
    const unsigned cx = (unsigned)pcell[3 * i], cy = (unsigned)pcell[3 * i + 1], cz = (unsigned)pcell[3 * i + 2];
    unsigned lo = 0, hi = 0;
    if (lane < 9) { // relative coordinates start at 1 and end below 2^21 - 1: neither -1 nor +1 leaves the field
        const unsigned x = cx + (unsigned)(lane / 3) - 1u, y = cy + (unsigned)(lane % 3) - 1u;
        lo = cell_start[lower_bound_key(cell_keys, nc, cell_key(x, y, cz - 1u))];
        hi = cell_start[lower_bound_key(cell_keys, nc, cell_key(x, y, cz + 2u))];
    }
    int cnt = 0;
    unsigned long long limit = kNoKey;
    for (int r = 0; r < 9; ++r) {
        const unsigned s = __shfl(lo, r, op::kWave), e = __shfl(hi, r, op::kWave);
        for (unsigned base = s; base < e; base += op::kWave) {
            if (cnt + op::kWave > kNbBuf) {
                cnt = wave_cut(buf, cnt, knn, lane);
                if (cnt == knn) limit = buf[knn - 1];
                __syncthreads();
            }
            bool take = false;
            unsigned long long key = 0;
            if (base + lane < e) {
                const int j = cell_points[base + lane];
                const float dx = xyz[3 * j] - px, dy = xyz[3 * j + 1] - py, dz = xyz[3 * j + 2] - pz; // (pj - pi).squaredNorm()
                const float d2 = dx * dx + dy * dy + dz * dz;
                key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)j;
                take = d2 < r2 && key < limit;
            }
            const unsigned long long mask = __ballot(take);
            if (take) buf[cnt + __popcll(mask & ((1ull << lane) - 1ull))] = key;
            cnt += __popcll(mask);
        }
    }
    __syncthreads();
    cnt = wave_cut(buf, cnt, knn, lane);
    for (int t = lane; t < knn; t += op::kWave) nb_out[(size_t)i * knn + t] = t < cnt ? (int)(unsigned)(buf[t] & 0xffffffffull) : -1;
    if (lane == 0) count_out[i] = cnt;
}

__device__ inline int fpfh_bin(double x) { // floor(11 x) clamped to [0, 10] (3DFeature.cpp:62-71); NaN lands in bin 0 as on the host
    const int b = (int)floor((double)kBins * x);
    return b > kBins - 1 ? kBins - 1 : (b < 0 ? 0 : b);
}

// ComputePairDescriptor + the binning of ComputeFPFHFeature's first pass.  The histogram counts in integers; every increment is the same
// integer `each` = 100 / (m - 1) and the sums stay far below 2^24, so each * count is the float the host reaches by repeated addition.
// Angle 0: atan2 in double on the two float dot products, rounded to float once -- a correctly rounded atan2f for every practical purpose,
// where the host's atan2f is its libm's (within one ulp of that): the two can disagree only for pairs that sit on a bin boundary.
__global__ __launch_bounds__(64) void k_spfh(const float* __restrict__ xyz, const float* __restrict__ nrm, unsigned n, const int* __restrict__ nb,
                                             const int* __restrict__ count, int knn, float* __restrict__ spfh) {
    __shared__ int hist[kDim];
    const unsigned i = blockIdx.x;
    const int lane = threadIdx.x;
    if (i >= n) return;
    if (lane < kDim) hist[lane] = 0;
    __syncthreads();
    const int m = count[i];
    const float psx = xyz[3 * i], psy = xyz[3 * i + 1], psz = xyz[3 * i + 2];
    const float u0 = nrm[3 * i], u1 = nrm[3 * i + 1], u2 = nrm[3 * i + 2];
    for (int j = 1 + lane; j < m; j += op::kWave) {
        const int q = nb[(size_t)i * knn + j];
        const float t0 = nrm[3 * q], t1 = nrm[3 * q + 1], t2 = nrm[3 * q + 2];
        const float ex = xyz[3 * q] - psx, ey = xyz[3 * q + 1] - psy, ez = xyz[3 * q + 2] - psz; // delta = pt - ps
        const float distance = sqrtf(ex * ex + ey * ey + ez * ez);
        const float d0 = ex / distance, d1 = ey / distance, d2 = ez / distance;                  // dir
        const float v0 = u1 * d2 - u2 * d1, v1 = u2 * d0 - u0 * d2, v2 = u0 * d1 - u1 * d0;      // v = u x dir
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
        if (!(sqrtf(v0 * v0 + v1 * v1 + v2 * v2) == 0.0f)) {
            const float w0 = u1 * v2 - u2 * v1, w1 = u2 * v0 - u0 * v2, w2 = u0 * v1 - u1 * v0;  // w = u x v
            a1 = v0 * t0 + v1 * t1 + v2 * t2;
            a2 = u0 * d0 + u1 * d1 + u2 * d2;
            a0 = (float)atan2((double)(w0 * t0 + w1 * t1 + w2 * t2), (double)(u0 * t0 + u1 * t1 + u2 * t2));
        }
        atomicAdd(&hist[fpfh_bin(((double)a0 + M_PI) / (2.0 * M_PI))], 1);
        atomicAdd(&hist[kBins + fpfh_bin((double)(a1 + 1.0f) / 2.0)], 1);
        atomicAdd(&hist[2 * kBins + fpfh_bin((double)(a2 + 1.0f) / 2.0)], 1);
    }
    __syncthreads();
    const int each = m - 1 > 0 ? 100 / (m - 1) : 0; // the INTEGER quotient, as written in the reference
    if (lane < kDim) spfh[(size_t)i * kDim + lane] = (float)(each * hist[lane]);
}

// The second pass of ComputeFPFHFeature: lanes 0..32 own one bin each, lanes 33..35 the unweighted sum of one third (a float sum over its 11
// bins per neighbour, accumulated in double).  Neighbours in list order, exact duplicates (dist == 0) skipped, a third without weight stays 0.
__global__ __launch_bounds__(64) void k_fpfh(const float* __restrict__ xyz, unsigned n, const int* __restrict__ nb, const int* __restrict__ count, int knn,
                                             const float* __restrict__ spfh, float* __restrict__ fpfh) {
    const unsigned i = blockIdx.x;
    const int lane = threadIdx.x;
    if (i >= n) return;
    const int m = count[i];
    const float px = xyz[3 * i], py = xyz[3 * i + 1], pz = xyz[3 * i + 2];
    float acc = 0.0f;
    double sum = 0.0;
    for (int j = 1; j < m; ++j) {
        const int q = nb[(size_t)i * knn + j];
        const float dx = px - xyz[3 * q], dy = py - xyz[3 * q + 1], dz = pz - xyz[3 * q + 2]; // (pi - pq).norm()
        const float dist = sqrtf(dx * dx + dy * dy + dz * dz);
        if (dist == 0.0f) continue;
        const float w = 1.0f / dist;
        const float* row = spfh + (size_t)q * kDim;
        if (lane < kDim) acc += w * row[lane];
        else if (lane < kDim + 3) {
            float s = 0.0f;
            for (int b = 0; b < kBins; ++b) s += row[(lane - kDim) * kBins + b];
            sum += s;
        }
    }
    const float scale = lane >= kDim && lane < kDim + 3 && sum != 0.0 ? (float)(100.0 / sum) : 0.0f;
    const float mine = __shfl(scale, kDim + (lane < kDim ? lane / kBins : 0), op::kWave);
    if (lane < kDim) fpfh[(size_t)i * kDim + lane] = acc * mine + spfh[(size_t)i * kDim + lane];
}

// FeatureMatching3D.  Block = 256 queries x one slice of the targets; a tile of 128 target rows (padded to 36 floats: 16-byte reads, every
// lane the same address) is staged per step.  d2 is the host's sequential sum.  Within a slice the scan is the host's (ascending, strict <);
// slices meet in one 64-bit atomic minimum per query over (d2 bits, index) -- the smallest d2 and, among equals, the lowest index, which is
// what an ascending scan with a strict comparison keeps.
constexpr int kFmThreads = 256, kFmTile = 128, kFmStride = 36;
__global__ __launch_bounds__(kFmThreads) void k_feature_match(const float* __restrict__ src, unsigned ns, const float* __restrict__ tgt, unsigned nt,
                                                              unsigned slice, unsigned long long* __restrict__ best) {
    __shared__ __attribute__((aligned(16))) float tile[kFmTile * kFmStride];
    const unsigned i = blockIdx.x * kFmThreads + threadIdx.x;
    float q[kDim];
#pragma unroll
    for (int b = 0; b < kDim; ++b) q[b] = i < ns ? src[(size_t)i * kDim + b] : 0.0f;
    const unsigned t_begin = blockIdx.y * slice, t_end = min(nt, t_begin + slice);
    float best_d2 = 0.0f;
    int arg = -1;
    for (unsigned t0 = t_begin; t0 < t_end; t0 += kFmTile) {
        const unsigned rows = min((unsigned)kFmTile, t_end - t0);
        __syncthreads();
        for (unsigned e = threadIdx.x; e < rows * kDim; e += kFmThreads) tile[(e / kDim) * kFmStride + e % kDim] = tgt[(size_t)t0 * kDim + e];
        __syncthreads();
        for (unsigned j = 0; j < rows; ++j) {
            const float4* row = reinterpret_cast<const float4*>(tile + j * kFmStride);
            float d2 = 0.0f;
#pragma unroll
            for (int v = 0; v < 8; ++v) {
                const float4 t = row[v];
                float e;
                e = q[4 * v] - t.x; d2 += e * e;
                e = q[4 * v + 1] - t.y; d2 += e * e;
                e = q[4 * v + 2] - t.z; d2 += e * e;
                e = q[4 * v + 3] - t.w; d2 += e * e;
            }
            { const float e = q[32] - tile[j * kFmStride + 32]; d2 += e * e; }
            if (arg < 0 || d2 < best_d2) { best_d2 = d2; arg = (int)(t0 + j); }
        }
    }
    if (i < ns && arg >= 0) atomicMin(&best[i], ((unsigned long long)__float_as_uint(best_d2) << 32) | (unsigned)arg);
}

__global__ void k_feature_match_finish(const unsigned long long* __restrict__ best, unsigned ns, int* __restrict__ nearest) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < ns) nearest[i] = best[i] == kNoKey ? -1 : (int)(unsigned)(best[i] & 0xffffffffull);
}

// |R p + t - q| < threshold as RansacRigid.cpp::Inlier forms it (TransformationModel.hpp:37-49)
__device__ inline bool ransac_inlier(const float (&T)[12], float sx, float sy, float sz, float tx, float ty, float tz, float threshold) {
    const float d0 = (T[0] * sx + T[1] * sy + T[2] * sz) + T[3] - tx;
    const float d1 = (T[4] * sx + T[5] * sy + T[6] * sz) + T[7] - ty;
    const float d2 = (T[8] * sx + T[9] * sy + T[10] * sz) + T[11] - tz;
    return sqrtf(d0 * d0 + d1 * d1 + d2 * d2) < threshold;
}

// One hypothesis per lane, so a wave owns 64 of them and a count never leaves its register until the end; block = 256 hypotheses x one slice
// of the correspondences, staged 256 at a time as two float4 each.  Slices meet in one integer atomic add per hypothesis.
constexpr int kRcThreads = 256, kRcTile = 256;
__global__ __launch_bounds__(kRcThreads) void k_ransac_count(const float* __restrict__ src, const float* __restrict__ tgt, unsigned n, const float* __restrict__ Ts,
                                                             unsigned H, float threshold, unsigned slice, unsigned* __restrict__ counts) {
    __shared__ float4 tile[2 * kRcTile];
    const unsigned h = blockIdx.x * kRcThreads + threadIdx.x;
    float T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = h < H ? Ts[(size_t)h * 12 + k] : 0.0f;
    const unsigned c_begin = blockIdx.y * slice, c_end = min(n, c_begin + slice);
    unsigned count = 0;
    for (unsigned c0 = c_begin; c0 < c_end; c0 += kRcTile) {
        const unsigned rows = min((unsigned)kRcTile, c_end - c0);
        __syncthreads();
        if (threadIdx.x < rows) {
            const size_t c = (size_t)(c0 + threadIdx.x) * 3;
            tile[2 * threadIdx.x] = make_float4(src[c], src[c + 1], src[c + 2], 0.0f);
            tile[2 * threadIdx.x + 1] = make_float4(tgt[c], tgt[c + 1], tgt[c + 2], 0.0f);
        }
        __syncthreads();
        for (unsigned j = 0; j < rows; ++j) {
            const float4 s = tile[2 * j], t = tile[2 * j + 1];
            count += ransac_inlier(T, s.x, s.y, s.z, t.x, t.y, t.z, threshold) ? 1u : 0u;
        }
    }
    if (h < H && count) atomicAdd(&counts[h], count);
}

// The inliers of ONE hypothesis, ascending: a single block walks the correspondences 1024 at a time and compacts each step with a ballot per
// wave and a scan over the 16 wave totals.
constexpr int kRiThreads = 1024;
__global__ __launch_bounds__(kRiThreads) void k_ransac_inlier_ids(const float* __restrict__ src, const float* __restrict__ tgt, unsigned n, const float* __restrict__ T12,
                                                                  float threshold, int* __restrict__ ids, unsigned* __restrict__ n_out) {
    __shared__ unsigned wave_total[kRiThreads / op::kWave];
    float T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = T12[k];
    const int lane = threadIdx.x & (op::kWave - 1), wave = threadIdx.x / op::kWave;
    unsigned base = 0;
    for (unsigned c0 = 0; c0 < n; c0 += kRiThreads) {
        const unsigned c = c0 + threadIdx.x;
        const bool in = c < n && ransac_inlier(T, src[3 * (size_t)c], src[3 * (size_t)c + 1], src[3 * (size_t)c + 2], tgt[3 * (size_t)c], tgt[3 * (size_t)c + 1],
                                               tgt[3 * (size_t)c + 2], threshold);
        const unsigned long long mask = __ballot(in);
        __syncthreads();
        if (lane == 0) wave_total[wave] = (unsigned)__popcll(mask);
        __syncthreads();
        unsigned before = 0, total = 0;
        for (int w = 0; w < kRiThreads / op::kWave; ++w) { const unsigned t = wave_total[w]; before += w < wave ? t : 0u; total += t; }
        if (in) ids[base + before + (unsigned)__popcll(mask & ((1ull << lane) - 1ull))] = (int)c;
        base += total;
    }
    if (threadIdx.x == 0) *n_out = base;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------

using op::Scope;      // the device buffers of one call (common.hpp)
using op::check_mem;

} // namespace

extern "C" {

int op_fpfh_compute(const float* xyz, const float* normals, size_t n, int knn, float radius, int mem, int device, float* fpfh_out, int* neighbours_out,
                    float* spfh_out) {
    if (!xyz || !normals || !fpfh_out) return fail(OP_ERR_INVALID, "null argument");
    OP_TRY(check_mem(mem));
    if (knn < 1 || knn > kNbMaxK) return fail(OP_ERR_INVALID, "knn must be in [1, %d]", kNbMaxK);
    if (!(radius > 0.0f) || !std::isfinite(radius)) return fail(OP_ERR_INVALID, "radius must be positive and finite");
    if (n > 0x7fffffffu / (size_t)kNbMaxK) return fail(OP_ERR_INVALID, "too many points");
    Scope s;
    OP_TRY(s.open(device));
    if (n == 0) return OP_OK;
    // The cells are those of the host path, the CELL RULE stated and argued at RadiusNeighbours of host/one_piece/src/GlobalRegistration.cpp:
    // floor((double)p / c) per axis with c = sqrt((double)radius) * (1 + 2^-20), in double, so that two points with float32 d2 < radius are
    // never two cells apart for any index accepted below (|p / c| < 1e9).  They are formed and sorted here, on the host, in
    // O(n log n) -- the cloud of a submap is a few thousand points; the candidate distances and the selection are the device's.
    std::vector<float> host_xyz;
    const float* hx = xyz;
    if (mem == OP_MEM_DEVICE) {
        host_xyz.resize(n * 3);
        OP_HIP(hipMemcpy(host_xyz.data(), xyz, n * 12, hipMemcpyDeviceToHost));
        hx = host_xyz.data();
    }
    const double cell = std::sqrt((double)radius) * (1.0 + 1.0 / 1048576.0);
    std::vector<int> pcell(n * 3);
    long long lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    for (size_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) {
            const double f = std::floor((double)hx[3 * i + a] / cell);
            if (!(std::fabs(f) < 1.0e9)) return fail(OP_ERR_INVALID, "point %zu is not finite or too far from the origin for cells of %g", i, cell);
            const int c = static_cast<int>(f);
            pcell[3 * i + a] = c;
            if (i == 0 || c < lo[a]) lo[a] = c;
            if (i == 0 || c > hi[a]) hi[a] = c;
        }
    for (int a = 0; a < 3; ++a)
        if (hi[a] - lo[a] > (1ll << kCellBits) - 4) return fail(OP_ERR_INVALID, "the cloud spans more than 2^%d cells of %g", kCellBits, (double)cell);
    std::vector<std::pair<unsigned long long, int> > keyed(n);
    for (size_t i = 0; i < n; ++i) {
        for (int a = 0; a < 3; ++a) pcell[3 * i + a] = (int)(pcell[3 * i + a] - lo[a] + 1);
        keyed[i] = std::make_pair(cell_key((unsigned)pcell[3 * i], (unsigned)pcell[3 * i + 1], (unsigned)pcell[3 * i + 2]), (int)i);
    }
    std::sort(keyed.begin(), keyed.end());
    std::vector<unsigned long long> cell_keys;
    std::vector<unsigned> cell_start;
    std::vector<int> cell_points(n);
    for (size_t k = 0; k < n; ++k) {
        if (k == 0 || keyed[k].first != keyed[k - 1].first) { cell_keys.push_back(keyed[k].first); cell_start.push_back((unsigned)k); }
        cell_points[k] = keyed[k].second;
    }
    cell_start.push_back((unsigned)n); // also what a key beyond the last one resolves to
    const unsigned nc = (unsigned)cell_keys.size();

    const float *d_xyz = nullptr, *d_nrm = nullptr;
    OP_TRY(s.input(xyz, n * 3, mem, &d_xyz));
    OP_TRY(s.input(normals, n * 3, mem, &d_nrm));
    int *d_pcell = nullptr, *d_points = nullptr, *d_nb = nullptr, *d_count = nullptr;
    unsigned long long* d_keys = nullptr;
    unsigned* d_start = nullptr;
    float *d_spfh = nullptr, *d_fpfh = nullptr;
    OP_TRY(s.upload(pcell, &d_pcell));
    OP_TRY(s.upload(cell_points, &d_points));
    OP_TRY(s.upload(cell_keys, &d_keys));
    OP_TRY(s.upload(cell_start, &d_start));
    OP_TRY(s.alloc(&d_nb, n * (size_t)knn));
    OP_TRY(s.alloc(&d_count, n));
    OP_TRY(s.alloc(&d_spfh, n * kDim));
    OP_TRY(s.alloc(&d_fpfh, n * kDim));
    hipLaunchKernelGGL(k_fpfh_neighbours, dim3((unsigned)n), dim3(op::kWave), 0, s.stream, d_xyz, d_pcell, (unsigned)n, d_keys, d_start, nc, d_points, radius, knn,
                       d_nb, d_count);
    hipLaunchKernelGGL(k_spfh, dim3((unsigned)n), dim3(op::kWave), 0, s.stream, d_xyz, d_nrm, (unsigned)n, d_nb, d_count, knn, d_spfh);
    hipLaunchKernelGGL(k_fpfh, dim3((unsigned)n), dim3(op::kWave), 0, s.stream, d_xyz, (unsigned)n, d_nb, d_count, knn, d_spfh, d_fpfh);
    OP_HIP(hipGetLastError());
    if (neighbours_out) OP_TRY(s.output(neighbours_out, d_nb, n * (size_t)knn, mem));
    if (spfh_out) OP_TRY(s.output(spfh_out, d_spfh, n * kDim, mem));
    OP_TRY(s.output(fpfh_out, d_fpfh, n * kDim, mem));
    return OP_OK;
}

int op_feature_match(const float* src, size_t ns, const float* tgt, size_t nt, int mem, int device, int* nearest_out) {
    if ((ns && !src) || (nt && !tgt) || (ns && !nearest_out)) return fail(OP_ERR_INVALID, "null argument");
    OP_TRY(check_mem(mem));
    if (ns > 0x7fffffffu / kDim || nt > 0x7fffffffu / kDim) return fail(OP_ERR_INVALID, "too many features");
    Scope s;
    OP_TRY(s.open(device));
    if (ns == 0) return OP_OK;
    const float *d_src = nullptr, *d_tgt = nullptr;
    OP_TRY(s.input(src, ns * kDim, mem, &d_src));
    OP_TRY(s.input(tgt, nt * kDim, mem, &d_tgt));
    unsigned long long* d_best = nullptr;
    int* d_nearest = nullptr;
    OP_TRY(s.alloc(&d_best, ns));
    OP_TRY(s.alloc(&d_nearest, ns));
    OP_HIP(hipMemsetAsync(d_best, 0xff, ns * 8, s.stream));
    const unsigned qblocks = (unsigned)((ns + kFmThreads - 1) / kFmThreads);
    if (nt) { // enough slices for about 2048 workgroups, each a whole number of tiles
        const unsigned tiles = (unsigned)((nt + kFmTile - 1) / kFmTile);
        const unsigned slices = std::max(1u, std::min(tiles, 2048u / qblocks));
        const unsigned slice = (tiles + slices - 1) / slices * kFmTile;
        hipLaunchKernelGGL(k_feature_match, dim3(qblocks, (unsigned)((nt + slice - 1) / slice)), dim3(kFmThreads), 0, s.stream, d_src, (unsigned)ns, d_tgt, (unsigned)nt,
                           slice, d_best);
    }
    hipLaunchKernelGGL(k_feature_match_finish, dim3(qblocks), dim3(kFmThreads), 0, s.stream, d_best, (unsigned)ns, d_nearest);
    OP_HIP(hipGetLastError());
    return s.output(nearest_out, d_nearest, ns, mem);
}

int op_ransac_count_inliers(const float* src_xyz, const float* tgt_xyz, size_t n, const float* T, size_t H, float threshold, int mem, int device,
                            unsigned* counts_out) {
    if ((n && (!src_xyz || !tgt_xyz)) || (H && (!T || !counts_out))) return fail(OP_ERR_INVALID, "null argument");
    OP_TRY(check_mem(mem));
    if (n > 0x7fffffffu / 3 || H > 0x7fffffffu / 12) return fail(OP_ERR_INVALID, "too many correspondences or hypotheses");
    Scope s;
    OP_TRY(s.open(device));
    if (H == 0) return OP_OK;
    const float *d_src = nullptr, *d_tgt = nullptr, *d_T = nullptr;
    OP_TRY(s.input(src_xyz, n * 3, mem, &d_src));
    OP_TRY(s.input(tgt_xyz, n * 3, mem, &d_tgt));
    OP_TRY(s.input(T, H * 12, mem, &d_T));
    unsigned* d_counts = nullptr;
    OP_TRY(s.alloc(&d_counts, H));
    OP_HIP(hipMemsetAsync(d_counts, 0, H * 4, s.stream));
    if (n) {
        const unsigned hblocks = (unsigned)((H + kRcThreads - 1) / kRcThreads);
        const unsigned tiles = (unsigned)((n + kRcTile - 1) / kRcTile);
        const unsigned slices = std::max(1u, std::min(tiles, 2048u / hblocks));
        const unsigned slice = (tiles + slices - 1) / slices * kRcTile;
        hipLaunchKernelGGL(k_ransac_count, dim3(hblocks, (unsigned)((n + slice - 1) / slice)), dim3(kRcThreads), 0, s.stream, d_src, d_tgt, (unsigned)n, d_T, (unsigned)H,
                           threshold, slice, d_counts);
        OP_HIP(hipGetLastError());
    }
    return s.output(counts_out, d_counts, H, mem);
}

int op_ransac_inlier_ids(const float* src_xyz, const float* tgt_xyz, size_t n, const float* T, float threshold, int mem, int device, int* ids_out,
                         size_t* n_out) {
    if ((n && (!src_xyz || !tgt_xyz || !ids_out)) || !T || !n_out) return fail(OP_ERR_INVALID, "null argument");
    OP_TRY(check_mem(mem));
    if (n > 0x7fffffffu / 3) return fail(OP_ERR_INVALID, "too many correspondences");
    Scope s;
    OP_TRY(s.open(device));
    *n_out = 0;
    if (n == 0) return OP_OK;
    const float *d_src = nullptr, *d_tgt = nullptr, *d_T = nullptr;
    OP_TRY(s.input(src_xyz, n * 3, mem, &d_src));
    OP_TRY(s.input(tgt_xyz, n * 3, mem, &d_tgt));
    OP_TRY(s.input(T, (size_t)12, mem, &d_T));
    int* d_ids = nullptr;
    unsigned* d_n = nullptr;
    OP_TRY(s.alloc(&d_ids, n));
    OP_TRY(s.alloc(&d_n, (size_t)1));
    hipLaunchKernelGGL(k_ransac_inlier_ids, dim3(1), dim3(kRiThreads), 0, s.stream, d_src, d_tgt, (unsigned)n, d_T, threshold, d_ids, d_n);
    OP_HIP(hipGetLastError());
    unsigned count = 0;
    OP_HIP(hipMemcpyAsync(&count, d_n, 4, hipMemcpyDeviceToHost, s.stream));
    OP_HIP(hipStreamSynchronize(s.stream));
    *n_out = count;
    return s.output(ids_out, d_ids, count, mem);
}

} // extern "C"
