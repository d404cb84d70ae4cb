// volume_register.hip -- op_volume_register_* (include/onepiece_hip.h): where a cloud or a depth frame belongs in the fused model.  Point-to-plane
// against the FIELD: at the transformed point p the strict trilinear sdf s is the residual and the normalised central difference n the plane normal
// (op_volume_sample's OP_SAMPLE_TRILINEAR and its gradient: trilinear_sample.hpp), the row is icp_iter.hip's (n ; p x n).  No target cloud, no
// normals, no neighbour search.
// k_volume_register: one lane per point, grid-stride, read-only.  The seven samples go through the lane's block cache one after the other, as in
// k_volume_sample.  Nothing per point is written (the ROWS instantiation writes the row for tests and op_volume_register_system's optional output).
// The 32 slots of a point (21 + 6 + 1 sums, 4 counts as doubles) are reduced over the wave PER TRIP by op::wave_reduce_scatter32_lazy -- the terms
// are recomputed from the seven floats (j, s) inside the first halving step -- and every lane keeps ONE double, the running total of its slot: a
// lane never holds 32 accumulators (64 VGPRs on top of the sampling's 66).  A frame's 307 k points are two trips at the most (1024 workgroups),
// and a trip's reduction (32 fp64 adds and the swaps) is small next to its 56 gathered taps.  Then LDS across the four waves, one row of 32 per
// workgroup, and k_register_fold adds the rows in index order (32 row lanes, then those in order): fixed for a given n, no floating-point
// atomics.  32 doubles come back per evaluation.
// The Gauss-Newton loop runs on the host: op_ldlt_solve6, op_se3_exp, a float32 4x4 product.  The host side has ONE path behind every entry
// point: reg_family decides which instantiations a call runs and reg_grid on how many workgroups, reg_launch maps a family to its kernel and
// fold, reg_unpack turns a folded row of 32, 35 or 38 into the 31 sums and 7 counts every entry hands on; an entry of a narrower family
// (op_volume_register_system, _color_system, the plain and colour loops) copies out its prefix.
// The COLOR instantiations (op_volume_register_color_* / _rgbd) take the colour sums of the same seven samples (rc_sample_global<true>): the model
// intensity m = I(c) at p, its central difference g over the six shifted samples, the row jc = color_scale (g ; p x g) and the residual
// color_scale (m - y) join the geometric terms of slots 0..27 inside the same reduction.  The three quantities that have no slot of the 32 (the
// unscaled sum of (m - y)^2, the geometric sum of s^2, the count of coloured points) travel by a butterfly of their own: three doubles per lane,
// six xor steps per trip, every lane ends with the wave's total; lane 0 puts them behind the wave's 32 slots (35 per row) and
// k_register_fold_color adds the rows.  color_scale == 0 runs the geometric instantiation: the colour planes are never read.
// The ROBUST instantiations (op_volume_register_robust_*) choose the linearisation -- which vector a the row (a ; p x a) is built from and which
// residual r goes with it: NORMAL (n, s: the entries above), GRADIENT (d / res, s), METRIC (n, s / (|d| / res)) -- and may scale row and residual
// by the square root of a Huber weight, the colour term by one of its own.  The mode and the two thresholds are wave-uniform arguments.  The six
// quantities without a slot (the colour kernel's three, the sum of the unweighted r^2, the two down-weighted counts) travel by the same butterfly:
// rows of 38, k_register_fold_robust.  All-zero options run the instantiations above: nothing about them changes.
// The OFFSET instantiations (op_volume_register_offset_* and, over the band voxels of a second volume -- volume_band.hip --,
// op_volume_register_volume) give every point a target value o_i of its own: the residual the linearisation starts from is s - o_i, one more
// load and one subtraction per point; the USED rule, max_distance and the stored-sdf sum keep s.  They are ROBUST instantiations with one more
// template parameter: the reduction, the rows of 38 and the fold are those; offset == NULL runs the instantiations above.
// The BATCH kernel (op_volume_register_batch_*: k_volume_register_batch) is the same body -- volume_register_body.inc, included by both kernels --
// behind a prologue that finds the workgroup's cloud in the round's table (a wave-uniform binary search, scalar loads) and points A at that cloud's
// range, pose and first row; k_register_fold_batch folds every active cloud's rows with one workgroup each, in the single fold's order.  The host
// loop is RegLoopState: reg_loop drives one, the batch entries one per cloud; RegRun and RegBatch take family, grid, dispatch and unpacking from
// the same four functions.
// Not built: damping, multi-resolution, re-ordering the points by block.
#include "volume_core.hpp"
#include "trilinear_sample.hpp"

#include <cmath>
#include <cstring>

namespace opi { int device_exclusive_scan(const unsigned* d_count, size_t n, unsigned* d_start, hipStream_t stream, unsigned* total_out); } // icp_grid.hip

namespace {

constexpr int kRegWg = 256;
constexpr unsigned kRegMaxGrid = 1024; // rows k_register_fold adds: 4 workgroups per CU
constexpr int kRegSlots = 32;          // [0, 21) j_a j_b (a <= b, row by row), [21, 27) s j_a, [27] s s, [28, 32) used, invalid, no_gradient, too_far
constexpr int kFoldWg = 1024;          // k_register_fold: one workgroup, 32 row lanes of 32 slots
constexpr int kFoldRows = kFoldWg / kRegSlots;
constexpr int kRegSlotsC = 35;         // COLOR: the 32 above (0..27 with the colour terms added), [32] rc rc, [33] s s alone, [34] colored
constexpr int kFoldRowsC = kFoldWg / 64; // k_register_fold_color: 16 row lanes of 64 threads, 35 of them at work
constexpr int kRegSlotsR = 38;         // ROBUST: the 35 above, [35] r r (unweighted), [36] downweighted, [37] color_downweighted

struct RegView { float res, inv_res; }; // what trilinear_sample.hpp reads of a view

struct RegArgs {
    const float* xyz;
    size_t n;
    float T[16];
    RegView W;
    float max_distance;
    float* rows;     // n x 8 {j[6], s, used} (ROWS only); COLOR: n x 16 {j[6], s, used, jc[6], rcs, colored}; ROBUST: the same layouts, the scaled values
    double* partial; // gridDim.x x kRegSlots (COLOR: x kRegSlotsC, ROBUST: x kRegSlotsR)
};
struct RegColor { // what the COLOR instantiations read on top
    const float* intensity; // n observed intensities
    float color_scale, max_color_residual;
};
struct RegRobust { // what the ROBUST instantiations take in RegColor's place: the same three first
    const float* intensity;
    float color_scale, max_color_residual;
    int linearization;        // OP_REGISTER_LIN_*
    float huber, huber_color; // <= 0: no weights
};
struct RegOffset : RegRobust { // what the OFFSET instantiations take: and the points' target values
    const float* offset;      // n
};

// intensity of a colour triple in stored channel order
__device__ __forceinline__ float reg_intensity(const float* c) { return (0.114f * c[0] + 0.587f * c[1]) + 0.299f * c[2]; }

// one sdf sample of the gradient: invalid when its own g is out of range (no conversion to int then)
// (COLOR: and its intensity, from the colour sums of the same taps)
template <bool COLOR>
__device__ __forceinline__ bool reg_sample_sdf(const VolView& V, const RegView& W, BlockCache& bc, float x, float y, float z, float* s, float* in) {
    if (!sample_in_range(x * W.inv_res - 0.5f, y * W.inv_res - 0.5f, z * W.inv_res - 0.5f)) return false;
    if constexpr (COLOR) {
        float c[3];
        if (!rc_sample_global<true>(V, W, bc, x, y, z, s, c)) return false;
        *in = reg_intensity(c);
        return true;
    } else {
        return rc_sample_global<false>(V, W, bc, x, y, z, s, nullptr);
    }
}

template <bool ROBUST, bool OFFSET>
using RegExtra = std::conditional_t<OFFSET, RegOffset, std::conditional_t<ROBUST, RegRobust, RegColor>>;

template <bool ROWS, bool COLOR, bool ROBUST = false, bool OFFSET = false>
__global__ __launch_bounds__(kRegWg) void k_volume_register(VolView V, RegArgs A, RegExtra<ROBUST, OFFSET> K) {
#define REG_WG blockIdx.x
#define REG_N_WG gridDim.x
#include "volume_register_body.inc"
#undef REG_WG
#undef REG_N_WG
}

// the rows in index order: row lane r adds rows r, r + 32, ..., then the 32 row lanes are added in order (four loads in flight per lane: the adds keep their order)
__device__ __forceinline__ void register_fold(const double* __restrict__ partial, unsigned n_rows, double* __restrict__ out) {
    __shared__ double s_fin[kFoldRows][kRegSlots];
    const unsigned fk = threadIdx.x & 31u, fr = threadIdx.x >> 5;
    double t = 0.0;
    unsigned p = fr;
    for (; p + 3 * kFoldRows < n_rows; p += 4 * kFoldRows) {
        const double a0 = partial[(size_t)p * kRegSlots + fk], a1 = partial[(size_t)(p + kFoldRows) * kRegSlots + fk];
        const double a2 = partial[(size_t)(p + 2 * kFoldRows) * kRegSlots + fk], a3 = partial[(size_t)(p + 3 * kFoldRows) * kRegSlots + fk];
        t += a0; t += a1; t += a2; t += a3;
    }
    for (; p < n_rows; p += kFoldRows) t += partial[(size_t)p * kRegSlots + fk];
    s_fin[fr][fk] = t;
    __syncthreads();
    if (threadIdx.x < kRegSlots) {
        double u = s_fin[0][threadIdx.x];
        for (int r = 1; r < kFoldRows; ++r) u += s_fin[r][threadIdx.x];
        out[threadIdx.x] = u;
    }
}
__global__ __launch_bounds__(kFoldWg) void k_register_fold(const double* __restrict__ partial, unsigned n_rows, double* __restrict__ out) {
    register_fold(partial, n_rows, out);
}

// the same for rows of 35 (COLOR) or 38 (ROBUST): row lane r (of 16) adds rows r, r + 16, ..., then the 16 row lanes are added in order
template <int SLOTS>
__device__ __forceinline__ void register_fold_wide(const double* __restrict__ partial, unsigned n_rows, double* __restrict__ out) {
    __shared__ double s_fin[kFoldRowsC][SLOTS];
    const unsigned fk = threadIdx.x & 63u, fr = threadIdx.x >> 6;
    if (fk < (unsigned)SLOTS) {
        double t = 0.0;
        unsigned p = fr;
        for (; p + 3 * kFoldRowsC < n_rows; p += 4 * kFoldRowsC) {
            const double a0 = partial[(size_t)p * SLOTS + fk], a1 = partial[(size_t)(p + kFoldRowsC) * SLOTS + fk];
            const double a2 = partial[(size_t)(p + 2 * kFoldRowsC) * SLOTS + fk], a3 = partial[(size_t)(p + 3 * kFoldRowsC) * SLOTS + fk];
            t += a0; t += a1; t += a2; t += a3;
        }
        for (; p < n_rows; p += kFoldRowsC) t += partial[(size_t)p * SLOTS + fk];
        s_fin[fr][fk] = t;
    }
    __syncthreads();
    if (threadIdx.x < (unsigned)SLOTS) {
        double u = s_fin[0][threadIdx.x];
        for (int r = 1; r < kFoldRowsC; ++r) u += s_fin[r][threadIdx.x];
        out[threadIdx.x] = u;
    }
}
__global__ __launch_bounds__(kFoldWg) void k_register_fold_color(const double* __restrict__ partial, unsigned n_rows, double* __restrict__ out) {
    register_fold_wide<kRegSlotsC>(partial, n_rows, out);
}
__global__ __launch_bounds__(kFoldWg) void k_register_fold_robust(const double* __restrict__ partial, unsigned n_rows, double* __restrict__ out) {
    register_fold_wide<kRegSlotsR>(partial, n_rows, out);
}

// ---- the depth entry's points: op_points_from_depth's definition over every stride-th pixel in both directions, row-major, compacted
struct SubGrid { int w, h, sw, sh, stride; };
__device__ __forceinline__ float reg_depth_at(const void* depth, int is_u16, float depth_scale, size_t px) {
    return is_u16 ? (float)((const unsigned short*)depth)[px] / depth_scale : ((const float*)depth)[px];
}
// (one sub-grid pixel k of one image: the count kernel's answer and the scatter kernel's stores; the batch kernels below call the same two)
__device__ __forceinline__ unsigned reg_pixel_kept(const void* __restrict__ depth, int is_u16, float depth_scale, const SubGrid& G, size_t k) {
    const int r = (int)(k / G.sw) * G.stride, c = (int)(k % G.sw) * G.stride;
    return reg_depth_at(depth, is_u16, depth_scale, (size_t)r * G.w + c) > 0 ? 1u : 0u;
}
// (RGB: and the kept pixel's intensity from its three bytes, each b / 255.0f as the integration rounds it)
template <bool RGB>
__device__ __forceinline__ void reg_pixel_scatter(const void* __restrict__ depth, int is_u16, const op_camera& cam, const SubGrid& G, size_t k, const unsigned* __restrict__ start_of_k,
                                                  float* __restrict__ xyz, const unsigned char* __restrict__ rgb, float* __restrict__ intensity) {
    const int r = (int)(k / G.sw) * G.stride, c = (int)(k % G.sw) * G.stride;
    const float z = reg_depth_at(depth, is_u16, cam.depth_scale, (size_t)r * G.w + c);
    if (!(z > 0)) return;
    const unsigned p = *start_of_k;
    xyz[3 * p] = ((float)c - cam.cx) * z / cam.fx; // PointCloud.cpp:90-93
    xyz[3 * p + 1] = ((float)r - cam.cy) * z / cam.fy;
    xyz[3 * p + 2] = z;
    if constexpr (RGB) {
        const unsigned char* b = rgb + 3 * ((size_t)r * G.w + c);
        const float col[3] = {(float)b[0] / 255.0f, (float)b[1] / 255.0f, (float)b[2] / 255.0f};
        intensity[p] = reg_intensity(col);
    }
}
__global__ __launch_bounds__(256) void k_register_depth_count(const void* __restrict__ depth, int is_u16, float depth_scale, SubGrid G, unsigned* __restrict__ count) {
    const size_t k = blockIdx.x * (size_t)256 + threadIdx.x;
    if (k >= (size_t)G.sw * G.sh) return;
    count[k] = reg_pixel_kept(depth, is_u16, depth_scale, G, k);
}
template <bool RGB>
__global__ __launch_bounds__(256) void k_register_depth_scatter(const void* __restrict__ depth, int is_u16, op_camera cam, SubGrid G, const unsigned* __restrict__ start,
                                                                float* __restrict__ xyz, const unsigned char* __restrict__ rgb, float* __restrict__ intensity) {
    const size_t k = blockIdx.x * (size_t)256 + threadIdx.x;
    if (k >= (size_t)G.sw * G.sh) return;
    reg_pixel_scatter<RGB>(depth, is_u16, cam, G, k, start + k, xyz, rgb, intensity);
}

// ---- many clouds in one launch (op_volume_register_batch_*)
// A round's launch holds the workgroups of every cloud that needs an evaluation in that round, cloud after cloud.  Cloud c has the n_wg workgroups
// RegRun::open gives it alone, and its workgroup b runs the trips the single kernel's workgroup b runs (volume_register_body.inc), so its n_wg
// rows, and their fold in k_register_fold's order, are the single entry's bits whatever else the launch holds.  A workgroup finds its cloud by a
// binary search over the first_wg column of the round's table: blockIdx.x is wave-uniform, so are the addresses, and the table, the pose and
// the cloud's range come through scalar loads.  The table has one entry per active cloud, never one per workgroup.
struct RegBatchEntry {
    unsigned long long start, n; // the cloud's points are [start, start + n) of the call's buffers
    unsigned first_wg, n_wg;     // its workgroups [first_wg, first_wg + n_wg) of the launch; its rows are those of the partial buffer
    float T[16];
};
struct RegBatchArgs {
    const float* xyz;
    const RegBatchEntry* table;
    unsigned n_active;
    RegView W;
    float max_distance;
    double* partial; // (the launch's workgroups) x slots
};

template <bool COLOR, bool ROBUST, bool OFFSET>
__global__ __launch_bounds__(kRegWg) void k_volume_register_batch(VolView V, RegBatchArgs B, RegExtra<ROBUST, OFFSET> K) {
    constexpr bool ROWS = false;
    constexpr int kRowSlots = ROBUST ? kRegSlotsR : COLOR ? kRegSlotsC : kRegSlots;
    const RegBatchEntry* __restrict__ table = B.table;
    unsigned lo = 0, hi = B.n_active; // the last entry whose first workgroup is not after this one (entry 0 starts at 0)
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) >> 1;
        if (table[mid].first_wg <= blockIdx.x) lo = mid; else hi = mid;
    }
    const RegBatchEntry* __restrict__ E = table + lo;
    const unsigned first_wg = E->first_wg, cloud_wgs = E->n_wg;
    const size_t start = E->start;
    RegArgs A;
    A.xyz = B.xyz + 3 * start;
    A.n = E->n;
#pragma unroll
    for (int k = 0; k < 16; ++k) A.T[k] = E->T[k];
    A.W = B.W;
    A.max_distance = B.max_distance;
    A.rows = nullptr;
    A.partial = B.partial + (size_t)first_wg * kRowSlots;
    if constexpr (COLOR) K.intensity += start;
    if constexpr (OFFSET) K.offset += start;
    const unsigned cloud_wg = blockIdx.x - first_wg;
#define REG_WG cloud_wg
#define REG_N_WG cloud_wgs
#include "volume_register_body.inc"
#undef REG_WG
#undef REG_N_WG
}

// one workgroup per active cloud: k_register_fold / register_fold_wide over that cloud's rows
__global__ __launch_bounds__(kFoldWg) void k_register_fold_batch(const double* __restrict__ partial, const RegBatchEntry* __restrict__ table, double* __restrict__ out) {
    const RegBatchEntry* E = table + blockIdx.x;
    register_fold(partial + (size_t)E->first_wg * kRegSlots, E->n_wg, out + (size_t)blockIdx.x * kRegSlots);
}
template <int SLOTS>
__global__ __launch_bounds__(kFoldWg) void k_register_fold_batch_wide(const double* __restrict__ partial, const RegBatchEntry* __restrict__ table, double* __restrict__ out) {
    const RegBatchEntry* E = table + blockIdx.x;
    register_fold_wide<SLOTS>(partial + (size_t)E->first_wg * SLOTS, E->n_wg, out + (size_t)blockIdx.x * SLOTS);
}

// the frames entry's points: every frame's sub-grid in one count, one scan and one scatter; frame f's image is base + f stride bytes
struct FrameSet {
    const unsigned char* depth;
    size_t depth_stride;
    const unsigned char* rgb;
    size_t rgb_stride;
    size_t n_sub, n_all; // sub-grid pixels of one frame, of all
};
__global__ __launch_bounds__(256) void k_register_depth_count_batch(FrameSet F, int is_u16, float depth_scale, SubGrid G, unsigned* __restrict__ count) {
    const size_t k = blockIdx.x * (size_t)256 + threadIdx.x;
    if (k >= F.n_all) return;
    const size_t f = k / F.n_sub;
    count[k] = reg_pixel_kept(F.depth + f * F.depth_stride, is_u16, depth_scale, G, k - f * F.n_sub);
}
template <bool RGB>
__global__ __launch_bounds__(256) void k_register_depth_scatter_batch(FrameSet F, int is_u16, op_camera cam, SubGrid G, const unsigned* __restrict__ start,
                                                                      float* __restrict__ xyz, float* __restrict__ intensity) {
    const size_t k = blockIdx.x * (size_t)256 + threadIdx.x;
    if (k >= F.n_all) return;
    const size_t f = k / F.n_sub;
    reg_pixel_scatter<RGB>(F.depth + f * F.depth_stride, is_u16, cam, G, k - f * F.n_sub, start + k, xyz, RGB ? F.rgb + f * F.rgb_stride : nullptr, intensity);
}
// where each frame's points begin, and after the last one the total
__global__ __launch_bounds__(256) void k_register_frame_starts(const unsigned* __restrict__ count, const unsigned* __restrict__ start, size_t n_sub, size_t n_frames,
                                                               unsigned* __restrict__ out) {
    const size_t f = blockIdx.x * (size_t)256 + threadIdx.x;
    if (f < n_frames) out[f] = start[f * n_sub];
    else if (f == n_frames) out[f] = start[n_frames * n_sub - 1] + count[n_frames * n_sub - 1];
}

// ---- host side
const op_volume_register_options kRegNoOptions{OP_REGISTER_LIN_NORMAL, 0.0f, 0.0f};

// Which instantiations a call runs.  Decided here and nowhere else: RegRun and RegBatch both take theirs from reg_family and their grids from
// reg_grid, so a batch cloud's kernel, workgroups and fold are the single entry's.
struct RegFamily {
    bool color = false, robust = false, offset = false;
    int slots() const { return robust ? kRegSlotsR : color ? kRegSlotsC : kRegSlots; }
    int row_width() const { return color ? 16 : 8; } // of the rows the ROWS instantiations write
};
// (d_offset: n target values on the device, or NULL; n: the call's points)
inline RegFamily reg_family(float color_scale, const op_volume_register_options& O, const float* d_offset, size_t n) {
    RegFamily F;
    F.color = color_scale > 0.0f;
    F.offset = d_offset && n;
    F.robust = F.offset || O.linearization != OP_REGISTER_LIN_NORMAL || O.huber > 0.0f || (F.color && O.huber_color > 0.0f);
    return F;
}
inline unsigned reg_grid(size_t n) { return (unsigned)std::min<size_t>((n + kRegWg - 1) / kRegWg, kRegMaxGrid); }

// The one place a family becomes an instantiation, and its fold: plain and colour take a RegColor (plain a zeroed one: the colour planes are
// never read), robust a RegRobust, offset a RegOffset; rows of 32, 35 or 38.  ARGS is RegArgs (one cloud on `wgs` workgroups, the ROWS
// instantiation when A.rows is set, one fold workgroup) or RegBatchArgs (a round's table, `folds` clouds).
template <class ARGS>
void reg_launch(const RegFamily& F, const VolView& V, const ARGS& A, const RegOffset& K, unsigned wgs, unsigned folds, double* d_out, hipStream_t stream) {
    constexpr bool kSingle = std::is_same<ARGS, RegArgs>::value;
    const dim3 g(wgs), b(kRegWg), gf(folds), bf(kFoldWg);
    auto launch = [&](auto color, auto robust, auto offset, const auto& extra) {
        constexpr bool C = decltype(color)::value, R = decltype(robust)::value, O = decltype(offset)::value;
        if constexpr (kSingle) {
            if (A.rows) hipLaunchKernelGGL((k_volume_register<true, C, R, O>), g, b, 0, stream, V, A, extra);
            else hipLaunchKernelGGL((k_volume_register<false, C, R, O>), g, b, 0, stream, V, A, extra);
        } else {
            hipLaunchKernelGGL((k_volume_register_batch<C, R, O>), g, b, 0, stream, V, A, extra);
        }
    };
    const std::true_type yes{};
    const std::false_type no{};
    const RegRobust& KR = K;
    // (The compiler emits the instantiations in the order of these calls.  It is the order the code object has always listed them in -- the
    // batch kernels' colour before plain, the reason for the two arms below -- so that a change to the host side leaves the code, the kernel
    // descriptors and the metadata of the unit's code object the same bytes, every kernel at the address it had: DESIGN.md section 3.9.)
    if (!F.robust) {
        const RegColor KC = F.color ? RegColor{K.intensity, K.color_scale, K.max_color_residual} : RegColor{nullptr, 0.0f, 0.0f};
        if constexpr (kSingle) { if (!F.color) launch(no, no, no, KC); else launch(yes, no, no, KC); }
        else { if (F.color) launch(yes, no, no, KC); else launch(no, no, no, KC); }
    } else if (F.offset) {
        if (F.color) launch(yes, yes, yes, K); else launch(no, yes, yes, K);
    } else {
        if (F.color) launch(yes, yes, no, KR); else launch(no, yes, no, KR);
    }
    const double* partial = A.partial;
    if constexpr (kSingle) {
        if (!F.color && !F.robust) hipLaunchKernelGGL(k_register_fold, gf, bf, 0, stream, partial, wgs, d_out);
        else if (!F.robust) hipLaunchKernelGGL(k_register_fold_color, gf, bf, 0, stream, partial, wgs, d_out);
        else hipLaunchKernelGGL(k_register_fold_robust, gf, bf, 0, stream, partial, wgs, d_out);
    } else {
        if (!F.color && !F.robust) hipLaunchKernelGGL(k_register_fold_batch, gf, bf, 0, stream, partial, A.table, d_out);
        else if (!F.robust) hipLaunchKernelGGL(k_register_fold_batch_wide<kRegSlotsC>, gf, bf, 0, stream, partial, A.table, d_out);
        else hipLaunchKernelGGL(k_register_fold_batch_wide<kRegSlotsR>, gf, bf, 0, stream, partial, A.table, d_out);
    }
}

// A folded row of `slots` doubles as every entry hands it on: 31 sums ([28] rc rc, [29] s s alone, [30] r r unweighted) and 7 counts; what a
// narrower family has no slot for is what the wider one computes when the colour term or the options are off.  r == NULL: no point, zeros.
void reg_unpack(int slots, const double* r, double sums[31], uint64_t counts[7]) {
    if (!r) {
        for (int k = 0; k < 31; ++k) sums[k] = 0.0;
        for (int k = 0; k < 7; ++k) counts[k] = 0;
        return;
    }
    for (int k = 0; k < 28; ++k) sums[k] = r[k];
    for (int k = 0; k < 4; ++k) counts[k] = (uint64_t)r[28 + k]; // whole numbers below 2^53: exact in any order
    if (slots == kRegSlots) { sums[28] = 0.0; sums[29] = sums[27]; counts[4] = 0; }
    else { sums[28] = r[32]; sums[29] = r[33]; counts[4] = (uint64_t)r[34]; }
    if (slots == kRegSlotsR) { sums[30] = r[35]; counts[5] = (uint64_t)r[36]; counts[6] = (uint64_t)r[37]; }
    else { sums[30] = sums[29]; counts[5] = 0; counts[6] = 0; }
}

// one call's device state: the points are on the device, the partial rows and the folded row allocated once
struct RegRun {
    op_volume* v;
    op::Scope tmp; // (everything runs on the volume's stream)
    RegFamily F;
    RegArgs A{};
    RegOffset K{};
    unsigned grid = 0;
    double *d_out = nullptr, *h_out = nullptr;

    explicit RegRun(op_volume* vol) : v(vol) { tmp.bind(v->stream); }
    // color_scale == 0: the geometric system; all-zero options: the plain one; d_offset: the points' target values
    int open(const float* d_xyz, const float* d_intensity, const float* d_offset, size_t n, float max_distance, float color_scale, float max_color_residual,
             const op_volume_register_options& O) {
        F = reg_family(color_scale, O, d_offset, n);
        A.xyz = d_xyz; A.n = n; A.W.res = v->res; A.W.inv_res = 1.0f / v->res; A.max_distance = max_distance;
        K.intensity = d_intensity; K.color_scale = color_scale; K.max_color_residual = max_color_residual;
        K.linearization = O.linearization; K.huber = O.huber; K.huber_color = O.huber_color;
        K.offset = d_offset;
        grid = reg_grid(n);
        if (!grid) return OP_OK;
        OP_TRY(tmp.alloc(&A.partial, (size_t)grid * F.slots()));
        OP_TRY(tmp.alloc(&d_out, (size_t)F.slots()));
        OP_TRY(tmp.pinned(&h_out, (size_t)F.slots()));
        return OP_OK;
    }
    // the system at T (d_rows: n x F.row_width() on the device, or NULL); no point: zeros
    int eval(const float T[16], float* d_rows, double sums[31], uint64_t counts[7]) {
        reg_unpack(F.slots(), nullptr, sums, counts);
        if (!grid) return OP_OK;
        for (int k = 0; k < 16; ++k) A.T[k] = T[k];
        A.rows = d_rows;
        reg_launch(F, v->view(), A, K, grid, 1, d_out, v->stream);
        OP_HIP(hipGetLastError());
        OP_HIP(hipMemcpyAsync(h_out, d_out, sizeof(double) * F.slots(), hipMemcpyDeviceToHost, v->stream));
        OP_HIP(hipStreamSynchronize(v->stream));
        reg_unpack(F.slots(), h_out, sums, counts);
        return OP_OK;
    }
};

// The rows of a one-pass entry on their way to the caller: the kernel writes rows of `kernel_w` floats, the entry promises rows of `entry_w` in
// the caller's `mem`.  A device buffer of the kernel's width is written in place; anything else goes through a temporary of the kernel's width.
// The only place that widens (rows of 8 become the first halves of rows of 16, the second halves zero).
struct RegRows {
    float *out = nullptr, *d = nullptr;
    size_t n = 0;
    int mem = OP_MEM_HOST, kernel_w = 8, entry_w = 8;
    int open(op::Scope& tmp, float* rows, size_t n_rows, int rows_mem, int kernel_width, int entry_width) {
        out = n_rows ? rows : nullptr; n = n_rows; mem = rows_mem; kernel_w = kernel_width; entry_w = entry_width;
        if (!out) return OP_OK;
        if (mem == OP_MEM_DEVICE && kernel_w == entry_w) { d = out; return OP_OK; }
        return tmp.alloc(&d, (size_t)kernel_w * n);
    }
    int deliver() const {
        if (!out || d == out) return OP_OK;
        if (kernel_w == entry_w) { OP_HIP(hipMemcpy(out, d, sizeof(float) * kernel_w * n, hipMemcpyDeviceToHost)); return OP_OK; }
        if (mem == OP_MEM_HOST) std::memset(out, 0, sizeof(float) * entry_w * n);
        else OP_HIP(hipMemset(out, 0, sizeof(float) * entry_w * n));
        OP_HIP(hipMemcpy2D(out, sizeof(float) * entry_w, d, sizeof(float) * kernel_w, sizeof(float) * kernel_w, n, mem == OP_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice));
        return OP_OK;
    }
};

inline double reg_rmse(double sum_sq, uint64_t count) { return count ? std::sqrt(sum_sq / (double)count) : 0.0; }

// C = A B, float32, each element ((a0 b0 + a1 b1) + a2 b2) + a3 b3
inline void reg_mul4(const float a[16], const float b[16], float c[16]) {
    for (int r = 0; r < 4; ++r)
        for (int k = 0; k < 4; ++k)
            c[4 * r + k] = ((a[4 * r] * b[k] + a[4 * r + 1] * b[4 + k]) + a[4 * r + 2] * b[8 + k]) + a[4 * r + 3] * b[12 + k];
}

int reg_check_params(const op_volume_register_params* p, const char* who) {
    if (p && p->max_iterations < 0) return fail(OP_ERR_INVALID, "%s: max_iterations < 0", who);
    return OP_OK;
}
int reg_check_color_scale(float color_scale, const char* who) {
    if (!(color_scale >= 0.0f) || !std::isfinite(color_scale)) return fail(OP_ERR_INVALID, "%s: color_scale must be finite and >= 0", who);
    return OP_OK;
}
int reg_check_options(const op_volume_register_options* o, const char* who) {
    if (!o) return OP_OK;
    if (o->linearization < OP_REGISTER_LIN_NORMAL || o->linearization > OP_REGISTER_LIN_METRIC) return fail(OP_ERR_INVALID, "%s: linearization %d", who, o->linearization);
    if (!(o->huber >= 0.0f) || !std::isfinite(o->huber)) return fail(OP_ERR_INVALID, "%s: huber must be finite and >= 0", who);
    if (!(o->huber_color >= 0.0f) || !std::isfinite(o->huber_color)) return fail(OP_ERR_INVALID, "%s: huber_color must be finite and >= 0", who);
    return OP_OK;
}
int reg_check_mem(int mem, const char* who) {
    if (mem != OP_MEM_HOST && mem != OP_MEM_DEVICE) return fail(OP_ERR_INVALID, "%s: bad mem %d", who, mem);
    return OP_OK;
}

op_volume_register_params reg_defaults(const op_volume* v) {
    op_volume_register_params p;
    p.max_iterations = 30; // ICPParameter's
    p.max_distance = v->trunc;
    p.min_step = 1e-5f;
    p.min_points = 6;
    return p;
}

op_volume_register_color_params reg_color_defaults(const op_volume* v) {
    op_volume_register_color_params p;
    p.base = reg_defaults(v);
    p.color_scale = 1.0f;        // equal weight, as LAMBDA_HYBRID_DEPTH 0.5 gives the tracker's two terms
    p.max_color_residual = 0.0f; // no gate
    return p;
}

// The parameters a loop entry was given.  An entry of the first family has no colour part: it is geometric whatever the colour defaults say.
struct RegParamsArg {
    const op_volume_register_params* base;        // NULL: reg_defaults
    const op_volume_register_color_params* color; // NULL where the entry has a colour part: reg_color_defaults
    bool has_color;
    RegParamsArg(const op_volume_register_params* p) : base(p), color(nullptr), has_color(false) {}
    RegParamsArg(const op_volume_register_color_params* p) : base(p ? &p->base : nullptr), color(p), has_color(true) {}
    int check(const char* who) const {
        OP_TRY(reg_check_params(base, who));
        if (color) OP_TRY(reg_check_color_scale(color->color_scale, who));
        return OP_OK;
    }
    bool wants_color() const { return has_color && (!color || color->color_scale > 0.0f); } // (the default color_scale is 1)
    op_volume_register_color_params resolve(const op_volume* v) const {
        if (color) return *color;
        if (has_color) return reg_color_defaults(v);
        return op_volume_register_color_params{base ? *base : reg_defaults(v), 0.0f, 0.0f};
    }
};

// The Gauss-Newton loop of ONE cloud as a state machine: while wants_evaluation(), the caller evaluates the system at T and hands it to take().
// reg_loop drives it with one cloud's RegRun, the batch entries drive one per cloud with a launch per round: the solve, the update, the stop
// rules and the result are this one copy.  A cloud that stopped after a step gets ONE more evaluation (the system at the pose that is
// returned); one that stopped on an evaluation that is current gets none.
struct RegLoopState {
    op_volume_register_params P{};
    op_volume_register_result res{};
    float T[16];
    double sums[31], first_sums[31];
    uint64_t counts[7], first_counts[7];
    bool have_first = false, current = false; // current: sums / counts are the system at T
    bool closing = false, done = false;       // closing: the next evaluation is the last one
    int it = 0;
    uint32_t evaluations = 0;
    uint64_t min_points = 0;
    double min_step2 = 0.0;

    void start(const float init_T[16], const op_volume_register_params& params) {
        P = params;
        for (int k = 0; k < 16; ++k) T[k] = init_T[k];
        for (int k = 0; k < 31; ++k) sums[k] = first_sums[k] = 0.0;
        for (int k = 0; k < 7; ++k) counts[k] = first_counts[k] = 0;
        res.status = OP_REGISTER_MAX_ITERATIONS;
        min_points = P.min_points > 0 ? (uint64_t)P.min_points : 0;
        min_step2 = (double)P.min_step * (double)P.min_step;
        closing = !(P.max_iterations > 0);
    }
    bool wants_evaluation() const { return !done; }
    int take(const double s[31], const uint64_t c[7]) { // the system at T
        for (int k = 0; k < 31; ++k) sums[k] = s[k];
        for (int k = 0; k < 7; ++k) counts[k] = c[k];
        ++evaluations;
        if (closing) { done = true; return OP_OK; }
        current = true;
        if (!have_first) {
            have_first = true;
            for (int k = 0; k < 31; ++k) first_sums[k] = sums[k];
            for (int k = 0; k < 7; ++k) first_counts[k] = counts[k];
        }
        bool stop = true;
        do {
            if (counts[0] < min_points) { res.status = OP_REGISTER_TOO_FEW_POINTS; break; }
            double JTJ[36], JTr[6];
            int k = 0;
            for (int a = 0; a < 6; ++a)
                for (int b = a; b < 6; ++b) { JTJ[6 * a + b] = sums[k]; JTJ[6 * b + a] = sums[k]; ++k; }
            for (int a = 0; a < 6; ++a) JTr[a] = sums[21 + a];
            float x[6];
            OP_TRY(op_ldlt_solve6(JTJ, JTr, x));
            double ss = 0.0;
            bool finite = true;
            for (int a = 0; a < 6; ++a) { finite = finite && std::isfinite(x[a]); ss += (double)x[a] * (double)x[a]; }
            if (!finite) { res.status = OP_REGISTER_SINGULAR; break; }
            float E[16], N[16];
            OP_TRY(op_se3_exp(x, E));
            reg_mul4(E, T, N);
            for (int a = 0; a < 16; ++a) T[a] = N[a];
            current = false;
            ++res.iterations;
            res.last_step = std::sqrt(ss);
            if (ss < min_step2) { res.status = OP_REGISTER_CONVERGED; break; }
            stop = false;
        } while (false);
        ++it;
        if (stop || it >= P.max_iterations) { if (current) done = true; else closing = true; }
        return OP_OK;
    }
    void finish(op_volume_register_robust_result* robust) {
        op_volume_register_color_result* out = &robust->color;
        if (!have_first) { // max_iterations == 0
            for (int k = 0; k < 31; ++k) first_sums[k] = sums[k];
            for (int k = 0; k < 7; ++k) first_counts[k] = counts[k];
            if (counts[0] < min_points) res.status = OP_REGISTER_TOO_FEW_POINTS;
        }
        for (int k = 0; k < 16; ++k) res.T[k] = T[k];
        res.used = counts[0]; res.invalid = counts[1]; res.no_gradient = counts[2]; res.too_far = counts[3];
        res.first_used = first_counts[0];
        res.rmse = reg_rmse(sums[29], counts[0]); // the geometric sum of s^2 (sums[27] holds the colour term too)
        res.first_rmse = reg_rmse(first_sums[29], first_counts[0]);
        out->base = res;
        out->colored = counts[4]; out->first_colored = first_counts[4];
        out->rmse_color = reg_rmse(sums[28], counts[4]);
        out->first_rmse_color = reg_rmse(first_sums[28], first_counts[4]);
        robust->downweighted = counts[5]; robust->color_downweighted = counts[6]; robust->first_downweighted = first_counts[5];
        robust->rmse_residual = reg_rmse(sums[30], counts[0]);
        robust->first_rmse_residual = reg_rmse(first_sums[30], first_counts[0]);
    }
};

// the Gauss-Newton loop over points (and, with color_scale > 0, intensities; with d_offset, target values) that are on the device.  The entries
// of the narrower families return a prefix of the result: robust.color, robust.color.base.
int reg_loop(op_volume* v, const float* d_xyz, const float* d_intensity, const float* d_offset, size_t n, const float init_T[16],
             const op_volume_register_color_params& P, float color_scale, const op_volume_register_options& options, op_volume_register_robust_result* robust) {
    RegRun R(v);
    OP_TRY(R.open(d_xyz, d_intensity, d_offset, n, P.base.max_distance, color_scale, P.max_color_residual, options));
    RegLoopState S;
    S.start(init_T, P.base);
    double sums[31];
    uint64_t counts[7];
    while (S.wants_evaluation()) {
        OP_TRY(R.eval(S.T, nullptr, sums, counts));
        OP_TRY(S.take(sums, counts));
    }
    S.finish(robust);
    return OP_OK;
}

// the depth entries' points (and intensities) in the volume's buffers
int reg_back_project(op_volume* v, op::Scope& tmp, const op_camera& c, const void* depth, int depth_fmt, const unsigned char* rgb, int mem, int pixel_stride,
                     unsigned* total) {
    SubGrid G{c.width, c.height, (c.width + pixel_stride - 1) / pixel_stride, (c.height + pixel_stride - 1) / pixel_stride, pixel_stride};
    const size_t npix = (size_t)c.width * c.height, nsub = (size_t)G.sw * G.sh;
    const void* d_depth = depth;
    const unsigned char* d_rgb = rgb;
    if (mem == OP_MEM_HOST) {
        const unsigned char* d = nullptr;
        OP_TRY(tmp.input(static_cast<const unsigned char*>(depth), npix * (depth_fmt == OP_DEPTH_U16 ? 2 : 4), mem, &d));
        d_depth = d;
        if (rgb) OP_TRY(tmp.input(rgb, npix * 3, mem, &d_rgb));
    }
    if (nsub > v->reg_cap) {
        if (v->reg_pts) op::cached_free(v->reg_pts);
        v->reg_pts = nullptr; v->reg_cap = 0;
        OP_HIP(op::cached_malloc((void**)&v->reg_pts, nsub * 12));
        v->reg_cap = nsub;
    }
    if (rgb && nsub > v->reg_int_cap) {
        if (v->reg_int) op::cached_free(v->reg_int);
        v->reg_int = nullptr; v->reg_int_cap = 0;
        OP_HIP(op::cached_malloc((void**)&v->reg_int, nsub * 4));
        v->reg_int_cap = nsub;
    }
    unsigned *d_count = nullptr, *d_start = nullptr;
    OP_TRY(tmp.alloc(&d_count, nsub));
    OP_TRY(tmp.alloc(&d_start, nsub));
    const dim3 g((unsigned)((nsub + 255) / 256)), b(256);
    hipLaunchKernelGGL(k_register_depth_count, g, b, 0, v->stream, d_depth, depth_fmt == OP_DEPTH_U16, c.depth_scale, G, d_count);
    OP_TRY(opi::device_exclusive_scan(d_count, nsub, d_start, v->stream, total));
    if (rgb) hipLaunchKernelGGL(k_register_depth_scatter<true>, g, b, 0, v->stream, d_depth, depth_fmt == OP_DEPTH_U16, c, G, (const unsigned*)d_start, v->reg_pts, d_rgb, v->reg_int);
    else hipLaunchKernelGGL(k_register_depth_scatter<false>, g, b, 0, v->stream, d_depth, depth_fmt == OP_DEPTH_U16, c, G, (const unsigned*)d_start, v->reg_pts, (const unsigned char*)nullptr, (float*)nullptr);
    OP_HIP(hipGetLastError());
    return OP_OK;
}

// ---- what the entries share.  Every check names the entry (`who`) and comes before any device use; their order is what a caller with several
// bad arguments sees.
// a cloud-taking entry's first checks; starts: the batch entries' n_clouds + 1 offsets (n is then the last of them)
int reg_check_clouds(const char* who, const op_volume* v, int mem, const uint64_t* starts, size_t n_clouds, bool batch, const float* xyz, size_t* n,
                     const void* pose, const char* pose_name, const void* out, const char* out_name) {
    if (!v) return fail(OP_ERR_INVALID, "%s: null volume", who);
    OP_TRY(reg_check_mem(mem, who));
    if (batch) {
        if (!starts) return fail(OP_ERR_INVALID, "%s: null starts", who);
        for (size_t c = 0; c < n_clouds; ++c)
            if (starts[c + 1] < starts[c]) return fail(OP_ERR_INVALID, "%s: starts decrease at cloud %zu", who, c);
        *n = (size_t)starts[n_clouds];
    }
    if (*n > 0 && !xyz) return fail(OP_ERR_INVALID, "%s: null xyz", who);
    if (!pose) return fail(OP_ERR_INVALID, "%s: null %s", who, pose_name);
    if (!out) return fail(OP_ERR_INVALID, "%s: null %s", who, out_name);
    return OP_OK;
}
// a frame-taking entry's checks; rgb_required: a NULL colour image is refused, not taken as "geometric"; c: the camera the frames have
int reg_check_frames(const char* who, const op_volume* v, const op_camera* cam, const void* depth, int depth_fmt, const uint8_t* rgb, bool rgb_required, int mem,
                     int pixel_stride, const void* pose, const char* pose_name, const void* out, const char* out_name, const RegParamsArg& params,
                     const op_volume_register_options* options, op_camera* c) {
    if (!v) return fail(OP_ERR_INVALID, "%s: null volume", who);
    OP_TRY(reg_check_mem(mem, who));
    if (depth_fmt != OP_DEPTH_F32 && depth_fmt != OP_DEPTH_U16) return fail(OP_ERR_INVALID, "%s: bad depth format %d", who, depth_fmt);
    if (!depth) return fail(OP_ERR_INVALID, "%s: null depth", who);
    if (rgb_required && !rgb) return fail(OP_ERR_INVALID, "%s: null rgb", who);
    if (pixel_stride < 1) return fail(OP_ERR_INVALID, "%s: pixel_stride < 1", who);
    if (!pose) return fail(OP_ERR_INVALID, "%s: null %s", who, pose_name);
    if (!out) return fail(OP_ERR_INVALID, "%s: null %s", who, out_name);
    OP_TRY(params.check(who));
    OP_TRY(reg_check_options(options, who));
    *c = cam ? *cam : v->cam;
    return check_cam(c);
}
// the call's points on the device, uploaded once where they are the host's (intensity / offset: only where the call reads them)
int reg_inputs(op::Scope& tmp, const float* xyz, const float* intensity, bool with_intensity, const float* offset, bool with_offset, size_t n, int mem,
               const float** d_xyz, const float** d_int, const float** d_off) {
    OP_TRY(tmp.input(xyz, 3 * n, mem, d_xyz));
    if (with_intensity) OP_TRY(tmp.input(intensity, n, mem, d_int));
    if (with_offset) OP_TRY(tmp.input(offset, n, mem, d_off));
    return OP_OK;
}

// what a one-pass entry writes: the first `sums` of the 31 sums, the first `counts` of the 7 counts, rows of `row_w` floats
struct RegExtent { int sums, counts, row_w; };
constexpr RegExtent kRegPlainExtent{28, 4, 8}, kRegColorExtent{30, 5, 16}, kRegRobustExtent{31, 7, 16};

// the one-pass entries.  offset (n floats in `mem`, or NULL): the OFFSET instantiations; a narrower entry passes the arguments it does not have
// as 0 / NULL, which the checks for them accept
int reg_system_entry(const char* who, op_volume* v, const float* xyz, const float* offset, const float* intensity, size_t n, int mem, const float T[16],
                     float max_distance, float color_scale, float max_color_residual, const op_volume_register_options* options, const RegExtent& ext, double* sums,
                     uint64_t* counts, float* rows) {
    OP_TRY(reg_check_clouds(who, v, mem, nullptr, 1, false, xyz, &n, T, "T", sums, "sums"));
    OP_TRY(reg_check_color_scale(color_scale, who));
    if (n > 0 && color_scale > 0.0f && !intensity) return fail(OP_ERR_INVALID, "%s: null intensity", who);
    OP_TRY(reg_check_options(options, who));
    OP_VOL(v);
    OP_TRY(vol_check(v)); // every accepted frame is fused, the stream idle
    RegRun R(v);
    const float *d_xyz = nullptr, *d_int = nullptr, *d_off = nullptr;
    OP_TRY(reg_inputs(R.tmp, xyz, intensity, color_scale > 0.0f, offset, offset != nullptr, n, mem, &d_xyz, &d_int, &d_off)); // (color_scale == 0: the intensities are not read either)
    OP_TRY(R.open(d_xyz, d_int, d_off, n, max_distance, color_scale, max_color_residual, options ? *options : kRegNoOptions));
    RegRows W;
    OP_TRY(W.open(R.tmp, rows, n, mem, R.F.row_width(), ext.row_w));
    double s[31];
    uint64_t c[7];
    OP_TRY(R.eval(T, W.d, s, c));
    OP_TRY(W.deliver());
    for (int k = 0; k < ext.sums; ++k) sums[k] = s[k];
    if (counts) for (int k = 0; k < ext.counts; ++k) counts[k] = c[k];
    return OP_OK;
}

// the loop entries over a cloud; result NULL is refused: a narrower entry passes a local one and copies its prefix out
int reg_points_entry(const char* who, op_volume* v, const float* xyz, const float* offset, const float* intensity, size_t n, int mem, const float init_T[16],
                     const RegParamsArg& params, const op_volume_register_options* options, op_volume_register_robust_result* result) {
    OP_TRY(reg_check_clouds(who, v, mem, nullptr, 1, false, xyz, &n, init_T, "init_T", result, "result"));
    OP_TRY(params.check(who));
    if (n > 0 && !intensity && params.wants_color()) return fail(OP_ERR_INVALID, "%s: null intensity", who);
    OP_TRY(reg_check_options(options, who));
    OP_VOL(v);
    OP_TRY(vol_check(v));
    const op_volume_register_color_params P = params.resolve(v);
    op::Scope up;
    up.bind(v->stream);
    const float *d_xyz = nullptr, *d_int = nullptr, *d_off = nullptr;
    OP_TRY(reg_inputs(up, xyz, intensity, P.color_scale > 0.0f, offset, offset != nullptr, n, mem, &d_xyz, &d_int, &d_off)); // uploaded once
    return reg_loop(v, d_xyz, d_int, d_off, n, init_T, P, P.color_scale, options ? *options : kRegNoOptions, result);
}

// the loop entries over a depth frame back-projected on the device; no colour image: the geometric registration
int reg_frame_entry(const char* who, op_volume* v, const op_camera* cam, const void* depth, int depth_fmt, const uint8_t* rgb, bool rgb_required, int mem,
                    int pixel_stride, const float init_pose[16], const RegParamsArg& params, const op_volume_register_options* options,
                    op_volume_register_robust_result* result) {
    op_camera c;
    OP_TRY(reg_check_frames(who, v, cam, depth, depth_fmt, rgb, rgb_required, mem, pixel_stride, init_pose, "init_pose", result, "result", params, options, &c));
    OP_VOL(v);
    OP_TRY(vol_check(v));
    const op_volume_register_color_params P = params.resolve(v);
    op::Scope tmp;
    tmp.bind(v->stream);
    unsigned total = 0;
    OP_TRY(reg_back_project(v, tmp, c, depth, depth_fmt, rgb, mem, pixel_stride, &total));
    return reg_loop(v, v->reg_pts, rgb ? v->reg_int : nullptr, nullptr, (size_t)total, init_pose, P, rgb ? P.color_scale : 0.0f,
                    options ? *options : kRegNoOptions, result); // (the loop's kernels follow the scatter on the volume's stream)
}

// ---- the batch entries
// one call's device state for many clouds: the points are on the device; the partial rows of every cloud, the round table and the folded rows
// are allocated once, in the call's Scope
struct RegBatch {
    op_volume* v;
    op::Scope& tmp;
    RegFamily F;
    RegBatchArgs B{};
    RegOffset K{};
    std::vector<unsigned> n_wg; // per cloud: reg_grid of its points
    const uint64_t* starts = nullptr;
    RegBatchEntry *h_table = nullptr, *d_table = nullptr;
    double *d_out = nullptr, *h_out = nullptr;
    uint32_t launches = 0;

    RegBatch(op_volume* vol, op::Scope& scope) : v(vol), tmp(scope) {}
    int open(const float* d_xyz, const float* d_intensity, const float* d_offset, const uint64_t* cloud_starts, size_t n_clouds, float max_distance, float color_scale,
             float max_color_residual, const op_volume_register_options& O) {
        starts = cloud_starts;
        F = reg_family(color_scale, O, d_offset, (size_t)starts[n_clouds]);
        B.xyz = d_xyz; B.W.res = v->res; B.W.inv_res = 1.0f / v->res; B.max_distance = max_distance;
        K.intensity = d_intensity; K.color_scale = color_scale; K.max_color_residual = max_color_residual;
        K.linearization = O.linearization; K.huber = O.huber; K.huber_color = O.huber_color;
        K.offset = d_offset;
        n_wg.resize(n_clouds);
        size_t rows = 0, with_rows = 0;
        for (size_t c = 0; c < n_clouds; ++c) {
            n_wg[c] = reg_grid((size_t)(starts[c + 1] - starts[c]));
            rows += n_wg[c];
            with_rows += n_wg[c] ? 1 : 0;
        }
        if (rows > 0x7fffffffu) return fail(OP_ERR_INVALID, "op_volume_register_batch: %zu workgroups in one round", rows);
        if (!with_rows) return OP_OK;
        const size_t slots = (size_t)F.slots();
        OP_TRY(tmp.alloc(&B.partial, rows * slots));
        OP_TRY(tmp.alloc(&d_table, with_rows));
        OP_TRY(tmp.pinned(&h_table, with_rows));
        OP_TRY(tmp.alloc(&d_out, with_rows * slots));
        OP_TRY(tmp.pinned(&h_out, with_rows * slots));
        return OP_OK;
    }
    // one round: cloud active[k] at the pose Ts[k]; the systems go to sums + 31 k, counts + 7 k.  One launch, one fold, one copy, one synchronisation;
    // nothing is launched when no active cloud has a point.
    int round(const std::vector<size_t>& active, const std::vector<const float*>& Ts, double* sums, uint64_t* counts) {
        unsigned n_tab = 0, wgs = 0;
        for (size_t k = 0; k < active.size(); ++k) {
            const size_t c = active[k];
            if (!n_wg[c]) continue;
            RegBatchEntry& E = h_table[n_tab++];
            E.start = starts[c]; E.n = starts[c + 1] - starts[c];
            E.first_wg = wgs; E.n_wg = n_wg[c];
            for (int a = 0; a < 16; ++a) E.T[a] = Ts[k][a];
            wgs += n_wg[c];
        }
        const int slots = F.slots();
        if (n_tab) {
            OP_HIP(hipMemcpyAsync(d_table, h_table, sizeof(RegBatchEntry) * n_tab, hipMemcpyHostToDevice, v->stream));
            B.table = d_table; B.n_active = n_tab;
            reg_launch(F, v->view(), B, K, wgs, n_tab, d_out, v->stream);
            OP_HIP(hipGetLastError());
            OP_HIP(hipMemcpyAsync(h_out, d_out, sizeof(double) * n_tab * (size_t)slots, hipMemcpyDeviceToHost, v->stream));
            OP_HIP(hipStreamSynchronize(v->stream));
            launches += 2;
        }
        unsigned e = 0;
        for (size_t k = 0; k < active.size(); ++k) // (no point, no workgroup: zeros)
            reg_unpack(slots, n_wg[active[k]] ? h_out + (size_t)(e++) * slots : nullptr, sums + 31 * k, counts + 7 * k);
        return OP_OK;
    }
};

// every cloud's loop, a round at a time: the clouds that want an evaluation share one launch
int reg_batch_loop(op_volume* v, op::Scope& tmp, const float* d_xyz, const float* d_intensity, const float* d_offset, const uint64_t* starts, size_t n_clouds,
                   const float* init_T, const op_volume_register_color_params& P, float color_scale, const op_volume_register_options& O,
                   op_volume_register_robust_result* results, op_volume_register_batch_stats* stats) {
    RegBatch R(v, tmp);
    OP_TRY(R.open(d_xyz, d_intensity, d_offset, starts, n_clouds, P.base.max_distance, color_scale, P.max_color_residual, O));
    std::vector<RegLoopState> S(n_clouds);
    for (size_t c = 0; c < n_clouds; ++c) S[c].start(init_T + 16 * c, P.base);
    std::vector<size_t> active;
    std::vector<const float*> Ts;
    std::vector<double> sums;
    std::vector<uint64_t> counts;
    uint32_t rounds = 0;
    for (;;) {
        active.clear(); Ts.clear();
        for (size_t c = 0; c < n_clouds; ++c)
            if (S[c].wants_evaluation()) { active.push_back(c); Ts.push_back(S[c].T); }
        if (active.empty()) break;
        sums.resize(31 * active.size()); counts.resize(7 * active.size());
        OP_TRY(R.round(active, Ts, sums.data(), counts.data()));
        for (size_t k = 0; k < active.size(); ++k) OP_TRY(S[active[k]].take(sums.data() + 31 * k, counts.data() + 7 * k));
        ++rounds;
    }
    uint64_t evaluations = 0;
    for (size_t c = 0; c < n_clouds; ++c) { S[c].finish(results + c); evaluations += S[c].evaluations; }
    if (stats) { stats->rounds = rounds; stats->launches = R.launches; stats->evaluations = evaluations; stats->points = starts[n_clouds]; }
    return OP_OK;
}

} // namespace

extern "C" {

int op_volume_register_default_params(op_volume* v, op_volume_register_params* p) {
    if (!v) return fail(OP_ERR_INVALID, "op_volume_register_default_params: null volume");
    if (!p) return fail(OP_ERR_INVALID, "op_volume_register_default_params: null params");
    *p = reg_defaults(v);
    return OP_OK;
}

int op_volume_register_system(op_volume* v, const float* xyz, size_t n, int mem, const float T[16], float max_distance, double sums[28], uint64_t counts[4],
                              float* rows) {
    return reg_system_entry("op_volume_register_system", v, xyz, nullptr, nullptr, n, mem, T, max_distance, 0.0f, 0.0f, nullptr, kRegPlainExtent, sums, counts, rows);
}

int op_volume_register_points(op_volume* v, const float* xyz, size_t n, int mem, const float init_T[16], const op_volume_register_params* params,
                              op_volume_register_result* result) {
    op_volume_register_robust_result r{};
    OP_TRY(reg_points_entry("op_volume_register_points", v, xyz, nullptr, nullptr, n, mem, init_T, params, nullptr, result ? &r : nullptr));
    *result = r.color.base;
    return OP_OK;
}

int op_volume_register_depth(op_volume* v, const op_camera* cam, const void* depth, int depth_fmt, int mem, int pixel_stride, const float init_pose[16],
                             const op_volume_register_params* params, op_volume_register_result* result) {
    op_volume_register_robust_result r{};
    OP_TRY(reg_frame_entry("op_volume_register_depth", v, cam, depth, depth_fmt, nullptr, false, mem, pixel_stride, init_pose, params, nullptr, result ? &r : nullptr));
    *result = r.color.base;
    return OP_OK;
}

// ---- the colour term
int op_volume_register_color_default_params(op_volume* v, op_volume_register_color_params* p) {
    if (!v) return fail(OP_ERR_INVALID, "op_volume_register_color_default_params: null volume");
    if (!p) return fail(OP_ERR_INVALID, "op_volume_register_color_default_params: null params");
    *p = reg_color_defaults(v);
    return OP_OK;
}

int op_volume_register_color_system(op_volume* v, const float* xyz, const float* intensity, size_t n, int mem, const float T[16], float max_distance,
                                    float color_scale, float max_color_residual, double sums[30], uint64_t counts[5], float* rows) {
    return reg_system_entry("op_volume_register_color_system", v, xyz, nullptr, intensity, n, mem, T, max_distance, color_scale, max_color_residual, nullptr, kRegColorExtent,
                            sums, counts, rows);
}

int op_volume_register_color_points(op_volume* v, const float* xyz, const float* intensity, size_t n, int mem, const float init_T[16],
                                    const op_volume_register_color_params* params, op_volume_register_color_result* result) {
    op_volume_register_robust_result r{};
    OP_TRY(reg_points_entry("op_volume_register_color_points", v, xyz, nullptr, intensity, n, mem, init_T, params, nullptr, result ? &r : nullptr));
    *result = r.color;
    return OP_OK;
}

int op_volume_register_rgbd(op_volume* v, const op_camera* cam, const void* depth, int depth_fmt, const uint8_t* rgb, int mem, int pixel_stride,
                            const float init_pose[16], const op_volume_register_color_params* params, op_volume_register_color_result* result) {
    op_volume_register_robust_result r{};
    OP_TRY(reg_frame_entry("op_volume_register_rgbd", v, cam, depth, depth_fmt, rgb, true, mem, pixel_stride, init_pose, params, nullptr, result ? &r : nullptr));
    *result = r.color;
    return OP_OK;
}

// ---- the linearisation and the Huber weights
int op_volume_register_robust_default_options(op_volume* v, op_volume_register_options* o) {
    if (!v) return fail(OP_ERR_INVALID, "op_volume_register_robust_default_options: null volume");
    if (!o) return fail(OP_ERR_INVALID, "op_volume_register_robust_default_options: null options");
    o->linearization = OP_REGISTER_LIN_METRIC; o->huber = 0.0f; o->huber_color = 0.0f;
    return OP_OK;
}

int op_volume_register_robust_system(op_volume* v, const float* xyz, const float* intensity, size_t n, int mem, const float T[16], float max_distance,
                                     float color_scale, float max_color_residual, const op_volume_register_options* options, double sums[31],
                                     uint64_t counts[7], float* rows) {
    return reg_system_entry("op_volume_register_robust_system", v, xyz, nullptr, intensity, n, mem, T, max_distance, color_scale, max_color_residual, options, kRegRobustExtent,
                            sums, counts, rows);
}

int op_volume_register_robust_points(op_volume* v, const float* xyz, const float* intensity, size_t n, int mem, const float init_T[16],
                                     const op_volume_register_color_params* params, const op_volume_register_options* options,
                                     op_volume_register_robust_result* result) {
    return reg_points_entry("op_volume_register_robust_points", v, xyz, nullptr, intensity, n, mem, init_T, params, options, result);
}

int op_volume_register_robust_frame(op_volume* v, const op_camera* cam, const void* depth, int depth_fmt, const uint8_t* rgb, int mem, int pixel_stride,
                                    const float init_pose[16], const op_volume_register_color_params* params, const op_volume_register_options* options,
                                    op_volume_register_robust_result* result) {
    return reg_frame_entry("op_volume_register_robust_frame", v, cam, depth, depth_fmt, rgb, false, mem, pixel_stride, init_pose, params, options, result);
}

// ---- a target value per point, and one fused volume against another
int op_volume_register_offset_system(op_volume* v, const float* xyz, const float* offset, const float* intensity, size_t n, int mem, const float T[16],
                                     float max_distance, float color_scale, float max_color_residual, const op_volume_register_options* options, double sums[31],
                                     uint64_t counts[7], float* rows) {
    return reg_system_entry("op_volume_register_offset_system", v, xyz, offset, intensity, n, mem, T, max_distance, color_scale, max_color_residual, options, kRegRobustExtent,
                            sums, counts, rows);
}

int op_volume_register_offset_points(op_volume* v, const float* xyz, const float* offset, const float* intensity, size_t n, int mem, const float init_T[16],
                                     const op_volume_register_color_params* params, const op_volume_register_options* options,
                                     op_volume_register_robust_result* result) {
    return reg_points_entry("op_volume_register_offset_points", v, xyz, offset, intensity, n, mem, init_T, params, options, result);
}

int op_volume_register_volume(op_volume* target, op_volume* source, const float init_T[16], const op_volume_band_params* sel,
                              const op_volume_register_color_params* params, const op_volume_register_options* options,
                              op_volume_register_volume_result* result) {
    const char* who = "op_volume_register_volume";
    const RegParamsArg PA(params);
    if (!target) return fail(OP_ERR_INVALID, "%s: null target", who);
    if (!source) return fail(OP_ERR_INVALID, "%s: null source", who);
    if (!init_T) return fail(OP_ERR_INVALID, "%s: null init_T", who);
    if (!result) return fail(OP_ERR_INVALID, "%s: null result", who);
    OP_TRY(vol_band_check(sel, who));
    OP_TRY(PA.check(who));
    OP_TRY(reg_check_options(options, who));
    if (target->device != source->device) return fail(OP_ERR_INVALID, "%s: the volumes are on devices %d and %d", who, target->device, source->device);
    OP_VOL(target);
    OP_TRY(vol_check(source)); // both queues flushed, both streams idle
    if (source != target) OP_TRY(vol_check(target));
    const op_volume_register_color_params P = PA.resolve(target);
    const op_volume_register_options O = options ? *options : op_volume_register_options{OP_REGISTER_LIN_GRADIENT, 0.0f, 0.0f};
    op::Scope list; // the source's band voxels, selected once: the source does not change over the iterations
    list.bind(target->stream);
    float *d_xyz = nullptr, *d_sdf = nullptr, *d_int = nullptr;
    size_t n = 0;
    OP_TRY(vol_band_select(list, source, sel, SIZE_MAX, &d_xyz, &d_sdf, P.color_scale > 0.0f ? &d_int : nullptr, &n)); // (the source's stream is idle on return)
    result->selected = n;
    return reg_loop(target, d_xyz, d_int, d_sdf, n, init_T, P, P.color_scale, O, &result->robust);
}

// ---- many clouds, many frames
int op_volume_register_batch_system(op_volume* v, const float* xyz, const float* offset, const float* intensity, const uint64_t* starts, size_t n_clouds, int mem,
                                    const float* T, float max_distance, float color_scale, float max_color_residual, const op_volume_register_options* options,
                                    double* sums, uint64_t* counts) {
    const char* who = "op_volume_register_batch_system";
    size_t n = 0;
    OP_TRY(reg_check_clouds(who, v, mem, starts, n_clouds, true, xyz, &n, T, "T", sums, "sums"));
    OP_TRY(reg_check_color_scale(color_scale, who));
    if (n > 0 && color_scale > 0.0f && !intensity) return fail(OP_ERR_INVALID, "%s: null intensity", who);
    OP_TRY(reg_check_options(options, who));
    if (!n_clouds) return OP_OK;
    OP_VOL(v);
    OP_TRY(vol_check(v));
    op::Scope tmp;
    tmp.bind(v->stream);
    const float *d_xyz = nullptr, *d_int = nullptr, *d_off = nullptr;
    OP_TRY(reg_inputs(tmp, xyz, intensity, color_scale > 0.0f, offset, offset && n, n, mem, &d_xyz, &d_int, &d_off));
    RegBatch R(v, tmp);
    OP_TRY(R.open(d_xyz, d_int, d_off, starts, n_clouds, max_distance, color_scale, max_color_residual, options ? *options : kRegNoOptions));
    std::vector<size_t> active(n_clouds);
    std::vector<const float*> Ts(n_clouds);
    for (size_t c = 0; c < n_clouds; ++c) { active[c] = c; Ts[c] = T + 16 * c; }
    std::vector<uint64_t> cnt(7 * n_clouds);
    OP_TRY(R.round(active, Ts, sums, cnt.data()));
    if (counts) for (size_t k = 0; k < cnt.size(); ++k) counts[k] = cnt[k];
    return OP_OK;
}

int op_volume_register_batch_points(op_volume* v, const float* xyz, const float* offset, const float* intensity, const uint64_t* starts, size_t n_clouds, int mem,
                                    const float* init_T, const op_volume_register_color_params* params, const op_volume_register_options* options,
                                    op_volume_register_robust_result* results, op_volume_register_batch_stats* stats) {
    const char* who = "op_volume_register_batch_points";
    const RegParamsArg PA(params);
    size_t n = 0;
    OP_TRY(reg_check_clouds(who, v, mem, starts, n_clouds, true, xyz, &n, init_T, "init_T", results, "results"));
    OP_TRY(PA.check(who));
    if (n > 0 && !intensity && PA.wants_color()) return fail(OP_ERR_INVALID, "%s: null intensity", who);
    OP_TRY(reg_check_options(options, who));
    if (!n_clouds) return OP_OK;
    OP_VOL(v);
    OP_TRY(vol_check(v));
    const op_volume_register_color_params P = PA.resolve(v);
    op::Scope tmp;
    tmp.bind(v->stream);
    const float *d_xyz = nullptr, *d_int = nullptr, *d_off = nullptr;
    OP_TRY(reg_inputs(tmp, xyz, intensity, P.color_scale > 0.0f, offset, offset && n, n, mem, &d_xyz, &d_int, &d_off));
    return reg_batch_loop(v, tmp, d_xyz, d_int, d_off, starts, n_clouds, init_T, P, P.color_scale, options ? *options : kRegNoOptions, results, stats);
}

int op_volume_register_batch_frames(op_volume* v, const op_camera* cam, const void* depth, size_t depth_stride_bytes, int depth_fmt, const uint8_t* rgb,
                                    size_t rgb_stride_bytes, int mem, int pixel_stride, const float* init_poses, size_t n_frames,
                                    const op_volume_register_color_params* params, const op_volume_register_options* options,
                                    op_volume_register_robust_result* results, op_volume_register_batch_stats* stats) {
    const char* who = "op_volume_register_batch_frames";
    const RegParamsArg PA(params);
    op_camera c;
    OP_TRY(reg_check_frames(who, v, cam, depth, depth_fmt, rgb, false, mem, pixel_stride, init_poses, "init_poses", results, "results", PA, options, &c));
    const size_t npix = (size_t)c.width * c.height, depth_elem = depth_fmt == OP_DEPTH_U16 ? 2 : 4;
    if (depth_stride_bytes < npix * depth_elem) return fail(OP_ERR_INVALID, "%s: depth stride %zu is smaller than an image (%zu bytes)", who, depth_stride_bytes, npix * depth_elem);
    if (depth_stride_bytes % depth_elem) return fail(OP_ERR_INVALID, "%s: depth stride %zu is no multiple of a depth value's %zu bytes", who, depth_stride_bytes, depth_elem);
    if (rgb && rgb_stride_bytes < npix * 3) return fail(OP_ERR_INVALID, "%s: rgb stride %zu is smaller than an image (%zu bytes)", who, rgb_stride_bytes, npix * 3);
    SubGrid G{c.width, c.height, (c.width + pixel_stride - 1) / pixel_stride, (c.height + pixel_stride - 1) / pixel_stride, pixel_stride};
    const size_t nsub = (size_t)G.sw * G.sh;
    if (n_frames && nsub > (size_t)0xffffffffu / n_frames) return fail(OP_ERR_INVALID, "%s: %zu frames of %zu pixels are more than 2^32 - 1 candidates", who, n_frames, nsub);
    if (!n_frames) return OP_OK;
    OP_VOL(v);
    OP_TRY(vol_check(v));
    const op_volume_register_color_params P = PA.resolve(v);
    const float color_scale = rgb ? P.color_scale : 0.0f; // no colour images: the geometric registration

    op::Scope tmp;
    tmp.bind(v->stream);
    FrameSet F{static_cast<const unsigned char*>(depth), depth_stride_bytes, rgb, rgb ? rgb_stride_bytes : 0, nsub, nsub * n_frames};
    if (mem == OP_MEM_HOST) { // one upload per plane: the frames and whatever lies between them
        OP_TRY(tmp.input(static_cast<const unsigned char*>(depth), (n_frames - 1) * depth_stride_bytes + npix * depth_elem, mem, &F.depth));
        if (rgb) OP_TRY(tmp.input(rgb, (n_frames - 1) * rgb_stride_bytes + npix * 3, mem, &F.rgb));
    }
    unsigned *d_count = nullptr, *d_start = nullptr, *d_first = nullptr, *h_first = nullptr;
    OP_TRY(tmp.alloc(&d_count, F.n_all));
    OP_TRY(tmp.alloc(&d_start, F.n_all));
    OP_TRY(tmp.alloc(&d_first, n_frames + 1));
    OP_TRY(tmp.pinned(&h_first, n_frames + 1));
    const dim3 g((unsigned)((F.n_all + 255) / 256)), b(256);
    const int is_u16 = depth_fmt == OP_DEPTH_U16;
    hipLaunchKernelGGL(k_register_depth_count_batch, g, b, 0, v->stream, F, is_u16, c.depth_scale, G, d_count);
    OP_HIP(hipGetLastError());
    OP_TRY(opi::device_exclusive_scan(d_count, F.n_all, d_start, v->stream, nullptr));
    hipLaunchKernelGGL(k_register_frame_starts, dim3((unsigned)((n_frames + 1 + 255) / 256)), b, 0, v->stream, (const unsigned*)d_count, (const unsigned*)d_start, nsub, n_frames, d_first);
    OP_HIP(hipGetLastError());
    OP_HIP(hipMemcpyAsync(h_first, d_first, sizeof(unsigned) * (n_frames + 1), hipMemcpyDeviceToHost, v->stream));
    OP_HIP(hipStreamSynchronize(v->stream));
    std::vector<uint64_t> starts(n_frames + 1);
    for (size_t f = 0; f <= n_frames; ++f) starts[f] = h_first[f];
    const size_t total = (size_t)starts[n_frames];
    float *d_xyz = nullptr, *d_int = nullptr; // the call's own: exactly the kept pixels
    OP_TRY(tmp.alloc(&d_xyz, 3 * total));
    if (rgb) OP_TRY(tmp.alloc(&d_int, total));
    if (total) {
        if (rgb) hipLaunchKernelGGL(k_register_depth_scatter_batch<true>, g, b, 0, v->stream, F, is_u16, c, G, (const unsigned*)d_start, d_xyz, d_int);
        else hipLaunchKernelGGL(k_register_depth_scatter_batch<false>, g, b, 0, v->stream, F, is_u16, c, G, (const unsigned*)d_start, d_xyz, (float*)nullptr);
        OP_HIP(hipGetLastError());
    }
    return reg_batch_loop(v, tmp, d_xyz, rgb ? d_int : nullptr, nullptr, starts.data(), n_frames, init_poses, P, color_scale, options ? *options : kRegNoOptions, results, stats);
}

} // extern "C"
