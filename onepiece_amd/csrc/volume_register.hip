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
// The Gauss-Newton loop runs on the host: op_ldlt_solve6, op_se3_exp, a float32 4x4 product.
// Not built: robust weights, colour terms, multi-resolution, re-ordering the points by block.
#include "volume_core.hpp"
#include "trilinear_sample.hpp"

#include <cmath>

namespace opi { int device_exclusive_scan(const unsigned* d_count, size_t n, unsigned* d_start, hipStream_t stream, unsigned* total_out); } // icp_grid.hip

namespace {

constexpr int kRegWg = 256;
constexpr unsigned kRegMaxGrid = 1024; // rows k_register_fold adds: 4 workgroups per CU
constexpr int kRegSlots = 32;          // [0, 21) j_a j_b (a <= b, row by row), [21, 27) s j_a, [27] s s, [28, 32) used, invalid, no_gradient, too_far
constexpr int kFoldWg = 1024;          // k_register_fold: one workgroup, 32 row lanes of 32 slots
constexpr int kFoldRows = kFoldWg / kRegSlots;

struct RegView { float res, inv_res; }; // what trilinear_sample.hpp reads of a view

struct RegArgs {
    const float* xyz;
    size_t n;
    float T[16];
    RegView W;
    float max_distance;
    float* rows;     // n x 8 {j[6], s, used} (ROWS only)
    double* partial; // gridDim.x x kRegSlots
};

// one sdf sample of the gradient: invalid when its own g is out of range (no conversion to int then)
__device__ __forceinline__ bool reg_sample_sdf(const VolView& V, const RegView& W, BlockCache& bc, float x, float y, float z, float* s) {
    if (!sample_in_range(x * W.inv_res - 0.5f, y * W.inv_res - 0.5f, z * W.inv_res - 0.5f)) return false;
    return rc_sample_global<false>(V, W, bc, x, y, z, s, nullptr);
}

template <bool ROWS>
__global__ __launch_bounds__(kRegWg) void k_volume_register(VolView V, RegArgs A) {
    __shared__ double s_red[kRegWg / 64][kRegSlots];
    double total = 0.0; // lane L: slot (L >> 1) & 31 of this wave, over its trips
    BlockCache bc{INT_MIN, INT_MIN, INT_MIN, -1};
    const size_t step = (size_t)gridDim.x * kRegWg;
    for (size_t base = (size_t)blockIdx.x * kRegWg; base < A.n; base += step) { // (the same trips for every lane of the workgroup)
        const size_t i = base + threadIdx.x;
        float j[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, s = 0.0f;
        int reason = -1; // 0 used, 1 invalid, 2 no gradient, 3 too far; -1: no point
        if (i < A.n) {
            const float x = A.xyz[3 * i], y = A.xyz[3 * i + 1], z = A.xyz[3 * i + 2];
            const float* M = A.T; // TransformPoints' order (k_prepare_frames)
            const float q0 = ((M[0] * x + M[1] * y) + M[2] * z) + M[3] * 1.0f;
            const float q1 = ((M[4] * x + M[5] * y) + M[6] * z) + M[7] * 1.0f;
            const float q2 = ((M[8] * x + M[9] * y) + M[10] * z) + M[11] * 1.0f;
            const float q3 = ((M[12] * x + M[13] * y) + M[14] * z) + M[15] * 1.0f;
            const float p0 = q0 / q3, p1 = q1 / q3, p2 = q2 / q3;
            float sv = 0.0f;
            reason = 1;
            if (reg_sample_sdf(V, A.W, bc, p0, p1, p2, &sv)) {
                const float h = 0.5f * A.W.res; // k_rc_shade's central difference
                float d[3];
                bool all = true;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    float sp = 0.0f, sm = 0.0f;
                    all = all && reg_sample_sdf(V, A.W, bc, p0 + (a == 0 ? h : 0.0f), p1 + (a == 1 ? h : 0.0f), p2 + (a == 2 ? h : 0.0f), &sp)
                              && reg_sample_sdf(V, A.W, bc, p0 - (a == 0 ? h : 0.0f), p1 - (a == 1 ? h : 0.0f), p2 - (a == 2 ? h : 0.0f), &sm);
                    d[a] = sp - sm;
                }
                const float l2 = all ? d[0] * d[0] + (d[1] * d[1] + d[2] * d[2]) : 0.0f;
                if (!(l2 > 0.0f)) reason = 2;
                else if (A.max_distance > 0.0f && !(fabsf(sv) <= A.max_distance)) reason = 3;
                else {
                    reason = 0;
                    const float l = sqrtf(l2);
                    const float n0 = d[0] / l, n1 = d[1] / l, n2 = d[2] / l;
                    j[0] = n0; j[1] = n1; j[2] = n2;
                    j[3] = p1 * n2 - p2 * n1; j[4] = p2 * n0 - p0 * n2; j[5] = p0 * n1 - p1 * n0;
                    s = sv;
                }
            }
            if (ROWS) {
                float* o = A.rows + 8 * i;
#pragma unroll
                for (int a = 0; a < 6; ++a) o[a] = j[a];
                o[6] = s; o[7] = reason == 0 ? 1.0f : 0.0f;
            }
        }
        // slot k of the point: float products, widened (an unused point's j and s are zero)
        auto val = [&](auto kc) -> double {
            constexpr int k = decltype(kc)::value;
            if constexpr (k < 21) {
                constexpr int a = k < 6 ? 0 : k < 11 ? 1 : k < 15 ? 2 : k < 18 ? 3 : k < 20 ? 4 : 5;
                constexpr int first = a == 0 ? 0 : a == 1 ? 6 : a == 2 ? 11 : a == 3 ? 15 : a == 4 ? 18 : 20;
                return (double)(j[a] * j[a + (k - first)]);
            } else if constexpr (k < 27) {
                return (double)(s * j[k - 21]);
            } else if constexpr (k == 27) {
                return (double)s * (double)s;
            } else {
                return reason == k - 28 ? 1.0 : 0.0;
            }
        };
        total += op::wave_reduce_scatter32_lazy(val);
    }
    // one row per workgroup (every lane gets here)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((lane & 1) == 0) s_red[wave][lane >> 1] = total;
    __syncthreads();
    if (threadIdx.x < kRegSlots) {
        double t = s_red[0][threadIdx.x];
        for (int w = 1; w < kRegWg / 64; ++w) t += s_red[w][threadIdx.x];
        A.partial[(size_t)blockIdx.x * kRegSlots + threadIdx.x] = t;
    }
}

// the rows in index order: row lane r adds rows r, r + 32, ..., then the 32 row lanes are added in order (four loads in flight per lane: the adds keep their order)
__global__ __launch_bounds__(kFoldWg) void k_register_fold(const double* __restrict__ partial, unsigned n_rows, double* __restrict__ out) {
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

// ---- the depth entry's points: op_points_from_depth's definition over every stride-th pixel in both directions, row-major, compacted
struct SubGrid { int w, h, sw, sh, stride; };
__device__ __forceinline__ float reg_depth_at(const void* depth, int is_u16, float depth_scale, size_t px) {
    return is_u16 ? (float)((const unsigned short*)depth)[px] / depth_scale : ((const float*)depth)[px];
}
__global__ __launch_bounds__(256) void k_register_depth_count(const void* __restrict__ depth, int is_u16, float depth_scale, SubGrid G, unsigned* __restrict__ count) {
    const size_t k = blockIdx.x * (size_t)256 + threadIdx.x;
    if (k >= (size_t)G.sw * G.sh) return;
    const int r = (int)(k / G.sw) * G.stride, c = (int)(k % G.sw) * G.stride;
    count[k] = reg_depth_at(depth, is_u16, depth_scale, (size_t)r * G.w + c) > 0 ? 1u : 0u;
}
__global__ __launch_bounds__(256) void k_register_depth_scatter(const void* __restrict__ depth, int is_u16, op_camera cam, SubGrid G, const unsigned* __restrict__ start,
                                                                float* __restrict__ xyz) {
    const size_t k = blockIdx.x * (size_t)256 + threadIdx.x;
    if (k >= (size_t)G.sw * G.sh) return;
    const int r = (int)(k / G.sw) * G.stride, c = (int)(k % G.sw) * G.stride;
    const float z = reg_depth_at(depth, is_u16, cam.depth_scale, (size_t)r * G.w + c);
    if (!(z > 0)) return;
    const unsigned p = start[k];
    xyz[3 * p] = ((float)c - cam.cx) * z / cam.fx; // PointCloud.cpp:90-93
    xyz[3 * p + 1] = ((float)r - cam.cy) * z / cam.fy;
    xyz[3 * p + 2] = z;
}

// ---- host side
// one call's device state: the points are on the device, the partial rows and the folded row allocated once
struct RegRun {
    op_volume* v;
    op::Scope tmp; // (everything runs on the volume's stream)
    RegArgs A{};
    unsigned grid = 0;
    double *d_out = nullptr, *h_out = nullptr;

    explicit RegRun(op_volume* vol) : v(vol) { tmp.bind(v->stream); }
    int open(const float* d_xyz, size_t n, float max_distance) {
        A.xyz = d_xyz; A.n = n; A.W.res = v->res; A.W.inv_res = 1.0f / v->res; A.max_distance = max_distance;
        grid = (unsigned)std::min<size_t>((n + kRegWg - 1) / kRegWg, kRegMaxGrid);
        if (!grid) return OP_OK;
        OP_TRY(tmp.alloc(&A.partial, (size_t)grid * kRegSlots));
        OP_TRY(tmp.alloc(&d_out, (size_t)kRegSlots));
        OP_TRY(tmp.pinned(&h_out, (size_t)kRegSlots));
        return OP_OK;
    }
    // the system at T: 28 sums and 4 counts (d_rows: n x 8 on the device, or NULL)
    int eval(const float T[16], float* d_rows, double sums[28], uint64_t counts[4]) {
        for (int k = 0; k < 28; ++k) sums[k] = 0.0;
        for (int k = 0; k < 4; ++k) counts[k] = 0;
        if (!grid) return OP_OK;
        for (int k = 0; k < 16; ++k) A.T[k] = T[k];
        A.rows = d_rows;
        const VolView V = v->view();
        if (d_rows) hipLaunchKernelGGL(k_volume_register<true>, dim3(grid), dim3(kRegWg), 0, v->stream, V, A);
        else hipLaunchKernelGGL(k_volume_register<false>, dim3(grid), dim3(kRegWg), 0, v->stream, V, A);
        hipLaunchKernelGGL(k_register_fold, dim3(1), dim3(kFoldWg), 0, v->stream, (const double*)A.partial, grid, d_out);
        OP_HIP(hipGetLastError());
        OP_HIP(hipMemcpyAsync(h_out, d_out, sizeof(double) * kRegSlots, hipMemcpyDeviceToHost, v->stream));
        OP_HIP(hipStreamSynchronize(v->stream));
        const double* r = h_out;
        for (int k = 0; k < 28; ++k) sums[k] = r[k];
        for (int k = 0; k < 4; ++k) counts[k] = (uint64_t)r[28 + k]; // whole numbers below 2^53: exact in any order
        return OP_OK;
    }
};

inline double reg_rmse(const double sums[28], uint64_t used) { return used ? std::sqrt(sums[27] / (double)used) : 0.0; }

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

op_volume_register_params reg_defaults(const op_volume* v) {
    op_volume_register_params p;
    p.max_iterations = 30; // ICPParameter's
    p.max_distance = v->trunc;
    p.min_step = 1e-5f;
    p.min_points = 6;
    return p;
}

// the Gauss-Newton loop over points that are on the device
int reg_loop(op_volume* v, const float* d_xyz, size_t n, const float init_T[16], const op_volume_register_params& P, op_volume_register_result* out) {
    RegRun R(v);
    OP_TRY(R.open(d_xyz, n, P.max_distance));
    op_volume_register_result res{};
    float T[16];
    for (int k = 0; k < 16; ++k) T[k] = init_T[k];
    double sums[28], first_sums[28];
    uint64_t counts[4], first_counts[4];
    bool have_first = false, current = false; // current: sums / counts are the system at T
    res.status = OP_REGISTER_MAX_ITERATIONS;
    const uint64_t min_points = P.min_points > 0 ? (uint64_t)P.min_points : 0;
    const double min_step2 = (double)P.min_step * (double)P.min_step;
    for (int it = 0; it < P.max_iterations; ++it) {
        OP_TRY(R.eval(T, nullptr, sums, counts));
        current = true;
        if (!have_first) {
            have_first = true;
            for (int k = 0; k < 28; ++k) first_sums[k] = sums[k];
            for (int k = 0; k < 4; ++k) first_counts[k] = counts[k];
        }
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
    }
    if (!current) OP_TRY(R.eval(T, nullptr, sums, counts)); // the system at the pose that is returned
    if (!have_first) { // max_iterations == 0
        for (int k = 0; k < 28; ++k) first_sums[k] = sums[k];
        for (int k = 0; k < 4; ++k) first_counts[k] = counts[k];
        if (counts[0] < min_points) res.status = OP_REGISTER_TOO_FEW_POINTS;
    }
    for (int k = 0; k < 16; ++k) res.T[k] = T[k];
    res.used = counts[0]; res.invalid = counts[1]; res.no_gradient = counts[2]; res.too_far = counts[3];
    res.first_used = first_counts[0];
    res.rmse = reg_rmse(sums, counts[0]);
    res.first_rmse = reg_rmse(first_sums, first_counts[0]);
    *out = res;
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
    // the argument checks need no device
    if (!v) return fail(OP_ERR_INVALID, "op_volume_register_system: null volume");
    if (mem != OP_MEM_HOST && mem != OP_MEM_DEVICE) return fail(OP_ERR_INVALID, "op_volume_register_system: bad mem %d", mem);
    if (n > 0 && !xyz) return fail(OP_ERR_INVALID, "op_volume_register_system: null xyz");
    if (!T) return fail(OP_ERR_INVALID, "op_volume_register_system: null T");
    if (!sums) return fail(OP_ERR_INVALID, "op_volume_register_system: null sums");
    OP_VOL(v);
    OP_TRY(vol_check(v)); // every accepted frame is fused, the stream idle
    RegRun R(v);
    const float* d_xyz = nullptr;
    OP_TRY(R.tmp.input(xyz, 3 * n, mem, &d_xyz));
    OP_TRY(R.open(d_xyz, n, max_distance));
    float* d_rows = rows;
    if (rows && n && mem == OP_MEM_HOST) OP_TRY(R.tmp.alloc(&d_rows, 8 * n));
    uint64_t c[4];
    OP_TRY(R.eval(T, n ? d_rows : nullptr, sums, c));
    if (counts) for (int k = 0; k < 4; ++k) counts[k] = c[k];
    if (rows && n && mem == OP_MEM_HOST) OP_HIP(hipMemcpy(rows, d_rows, sizeof(float) * 8 * n, hipMemcpyDeviceToHost));
    return OP_OK;
}

int op_volume_register_points(op_volume* v, const float* xyz, size_t n, int mem, const float init_T[16], const op_volume_register_params* params,
                              op_volume_register_result* result) {
    if (!v) return fail(OP_ERR_INVALID, "op_volume_register_points: null volume");
    if (mem != OP_MEM_HOST && mem != OP_MEM_DEVICE) return fail(OP_ERR_INVALID, "op_volume_register_points: bad mem %d", mem);
    if (n > 0 && !xyz) return fail(OP_ERR_INVALID, "op_volume_register_points: null xyz");
    if (!init_T) return fail(OP_ERR_INVALID, "op_volume_register_points: null init_T");
    if (!result) return fail(OP_ERR_INVALID, "op_volume_register_points: null result");
    OP_TRY(reg_check_params(params, "op_volume_register_points"));
    OP_VOL(v);
    OP_TRY(vol_check(v));
    const op_volume_register_params P = params ? *params : reg_defaults(v);
    op::Scope up;
    up.bind(v->stream);
    const float* d_xyz = nullptr;
    OP_TRY(up.input(xyz, 3 * n, mem, &d_xyz)); // uploaded once
    return reg_loop(v, d_xyz, n, init_T, P, result);
}

int op_volume_register_depth(op_volume* v, const op_camera* cam, const void* depth, int depth_fmt, int mem, int pixel_stride, const float init_pose[16],
                             const op_volume_register_params* params, op_volume_register_result* result) {
    if (!v) return fail(OP_ERR_INVALID, "op_volume_register_depth: null volume");
    if (mem != OP_MEM_HOST && mem != OP_MEM_DEVICE) return fail(OP_ERR_INVALID, "op_volume_register_depth: bad mem %d", mem);
    if (depth_fmt != OP_DEPTH_F32 && depth_fmt != OP_DEPTH_U16) return fail(OP_ERR_INVALID, "op_volume_register_depth: bad depth format %d", depth_fmt);
    if (!depth) return fail(OP_ERR_INVALID, "op_volume_register_depth: null depth");
    if (pixel_stride < 1) return fail(OP_ERR_INVALID, "op_volume_register_depth: pixel_stride < 1");
    if (!init_pose) return fail(OP_ERR_INVALID, "op_volume_register_depth: null init_pose");
    if (!result) return fail(OP_ERR_INVALID, "op_volume_register_depth: null result");
    OP_TRY(reg_check_params(params, "op_volume_register_depth"));
    const op_camera c = cam ? *cam : v->cam;
    OP_TRY(check_cam(&c));
    OP_VOL(v);
    OP_TRY(vol_check(v));
    const op_volume_register_params P = params ? *params : reg_defaults(v);

    SubGrid G{c.width, c.height, (c.width + pixel_stride - 1) / pixel_stride, (c.height + pixel_stride - 1) / pixel_stride, pixel_stride};
    const size_t npix = (size_t)c.width * c.height, nsub = (size_t)G.sw * G.sh;
    op::Scope tmp;
    tmp.bind(v->stream);
    const void* d_depth = depth;
    if (mem == OP_MEM_HOST) {
        const unsigned char* d = nullptr;
        OP_TRY(tmp.input(static_cast<const unsigned char*>(depth), npix * (depth_fmt == OP_DEPTH_U16 ? 2 : 4), mem, &d));
        d_depth = d;
    }
    if (nsub > v->reg_cap) {
        if (v->reg_pts) op::cached_free(v->reg_pts);
        v->reg_pts = nullptr; v->reg_cap = 0;
        OP_HIP(op::cached_malloc((void**)&v->reg_pts, nsub * 12));
        v->reg_cap = nsub;
    }
    unsigned *d_count = nullptr, *d_start = nullptr, total = 0;
    OP_TRY(tmp.alloc(&d_count, nsub));
    OP_TRY(tmp.alloc(&d_start, nsub));
    const dim3 g((unsigned)((nsub + 255) / 256)), b(256);
    hipLaunchKernelGGL(k_register_depth_count, g, b, 0, v->stream, d_depth, depth_fmt == OP_DEPTH_U16, c.depth_scale, G, d_count);
    OP_TRY(opi::device_exclusive_scan(d_count, nsub, d_start, v->stream, &total));
    hipLaunchKernelGGL(k_register_depth_scatter, g, b, 0, v->stream, d_depth, depth_fmt == OP_DEPTH_U16, c, G, (const unsigned*)d_start, v->reg_pts);
    OP_HIP(hipGetLastError());
    return reg_loop(v, v->reg_pts, (size_t)total, init_pose, P, result); // (the loop's kernels follow the scatter on the volume's stream)
}

} // extern "C"
