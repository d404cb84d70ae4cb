// volume_sample.hip -- op_volume_sample (include/onepiece_hip.h): what the fused model holds at a batch of caller-given points.  The two definitions
// of "the model's value at a point" the library already evaluates, made callable:
//   OP_SAMPLE_TRILINEAR   the raycaster's strict trilinear sample, its central-difference gradient and trilinear colour (trilinear_sample.hpp:
//                         rc_cell, rc_weight and the gather through the hash, the functions raycast.hip marches and shades with)
//   OP_SAMPLE_REFERENCE   VoxelCube::ReadVoxelInterpolate as CubeHandler::Transform evaluates it (voxel_interp.hpp: the voxel fetch and the lerp
//                         stages of k_transform_fill_wave)
// k_volume_sample: one lane per query, grid-stride, read-only.  A lane keeps its last block (id -> pool slot), so the eight taps of a sample cost
// one hash lookup unless they straddle blocks; the seven samples of a gradient query are gathered one after the other through that cache (their 56
// taps are 32 distinct voxels: the repeats hit the L1).  The colour planes are read only where voxels are asked for.  Every lane accumulates the
// call's statistics in registers; a workgroup reduces them (wave shuffles, then LDS) into ONE row and the host adds the rows in index order -- no
// floating-point atomics, the sums are repeatable for a given n.
// Not built: re-ordering the queries by block on the device, a block-major LDS-tile form, a nearest-voxel mode,
// projection onto the surface.  (Registration against the field is volume_register.hip.)
#include "volume_core.hpp"
#include "trilinear_sample.hpp"
#include "voxel_interp.hpp"

namespace {

constexpr int kSampleWg = 256;
constexpr unsigned kSampleMaxGrid = 1024; // rows of statistics the host adds: 4 workgroups per CU

struct SampleRow { unsigned long long valid, gradients, out_of_range; double sum_abs, sum_sq; float max_abs; unsigned pad; };
static_assert(sizeof(SampleRow) == 48, "six 8-byte words");

struct SampleView { float res, inv_res; }; // what trilinear_sample.hpp reads of a view

struct SampleArgs {
    const float* xyz;
    size_t n;
    float T[16];
    int has_T;
    SampleView W;
    float* voxels;
    float* gradients;
    unsigned char* status;
    SampleRow* rows;
};

// the five planes of the trilinear sample of cell c (rc_sample_global with the weight plane accumulated as well): false = not all 8 voxels observed
__device__ bool sample_voxel5(const VolView& V, const RcCell& c, BlockCache& bc, Vox5* out) {
    Vox5 a{0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int px = c.i0 + (k & 1), py = c.i1 + ((k >> 1) & 1), pz = c.i2 + ((k >> 2) & 1);
        const int bx = px >> 3, by = py >> 3, bz = pz >> 3;
        if (!(bx == bc.cx && by == bc.cy && bz == bc.cz)) { bc.cx = bx; bc.cy = by; bc.cz = bz; bc.idx = table_find(V, bx, by, bz); }
        if (bc.idx < 0) return false;
        const float* t = V.pool + (size_t)bc.idx * kBlockFloats + ((px - bx * 8) + (py - by * 8) * 8 + (pz - bz * 8) * 64);
        const float tw = t[kVox];
        if (!(tw > 0)) return false;
        const float w = rc_weight(c, k);
        a.s += w * t[0]; a.w += w * tw; a.c0 += w * t[2 * kVox]; a.c1 += w * t[3 * kVox]; a.c2 += w * t[4 * kVox];
    }
    *out = a;
    return true;
}

// one sdf sample of the gradient: invalid when its own g is out of range (no conversion to int then)
__device__ __forceinline__ bool sample_sdf(const VolView& V, const SampleView& W, BlockCache& bc, float x, float y, float z, float* s) {
    if (!sample_in_range(x * W.inv_res - 0.5f, y * W.inv_res - 0.5f, z * W.inv_res - 0.5f)) return false;
    return rc_sample_global<false>(V, W, bc, x, y, z, s, nullptr);
}

// fetch_voxel through the lane's last block
__device__ __forceinline__ Vox5 fetch_voxel_cached(const VolView& V, BlockCache& bc, int px, int py, int pz) {
    const int bx = px >> 3, by = py >> 3, bz = pz >> 3;
    if (!(bx == bc.cx && by == bc.cy && bz == bc.cz)) { bc.cx = bx; bc.cy = by; bc.cz = bz; bc.idx = table_find(V, bx, by, bz); }
    if (bc.idx < 0) return default_voxel();
    return load_planes(V.pool + (size_t)bc.idx * kBlockFloats + ((px - bx * 8) + (py - by * 8) * 8 + (pz - bz * 8) * 64));
}

__device__ __forceinline__ double wave_sum_f64(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// MODE = OP_SAMPLE_TRILINEAR: VOX = the voxels are asked for (all five planes; otherwise sdf and weight only), GRAD = the gradients are.
// MODE = OP_SAMPLE_REFERENCE: one instantiation (VOX, no GRAD); A.voxels may still be NULL.
template <int MODE, bool VOX, bool GRAD>
__global__ __launch_bounds__(kSampleWg) void k_volume_sample(VolView V, SampleArgs A) {
    __shared__ SampleRow s_part[kSampleWg / 64];
    unsigned n_valid = 0, n_grad = 0, n_oor = 0;
    double sum_abs = 0, sum_sq = 0;
    float max_abs = 0;
    BlockCache bc{INT_MIN, INT_MIN, INT_MIN, -1};
    const size_t step = (size_t)gridDim.x * kSampleWg;
    for (size_t i = (size_t)blockIdx.x * kSampleWg + threadIdx.x; i < A.n; i += step) {
        float x = A.xyz[3 * i], y = A.xyz[3 * i + 1], z = A.xyz[3 * i + 2];
        if (A.has_T) { // TransformPoints' order (k_prepare_frames)
            const float* M = A.T;
            const float q0 = ((M[0] * x + M[1] * y) + M[2] * z) + M[3] * 1.0f;
            const float q1 = ((M[4] * x + M[5] * y) + M[6] * z) + M[7] * 1.0f;
            const float q2 = ((M[8] * x + M[9] * y) + M[10] * z) + M[11] * 1.0f;
            const float q3 = ((M[12] * x + M[13] * y) + M[14] * z) + M[15] * 1.0f;
            x = q0 / q3; y = q1 / q3; z = q2 / q3;
        }
        unsigned st = 0;
        Vox5 r = default_voxel();
        float d[3] = {0.0f, 0.0f, 0.0f};
        if (MODE == OP_SAMPLE_TRILINEAR) {
            if (!sample_in_range(x * A.W.inv_res - 0.5f, y * A.W.inv_res - 0.5f, z * A.W.inv_res - 0.5f)) {
                st = OP_SAMPLE_INVALID | OP_SAMPLE_OUT_OF_RANGE | (GRAD ? OP_SAMPLE_NO_GRADIENT : 0);
            } else {
                Vox5 got = default_voxel();
                const bool ok = VOX ? sample_voxel5(V, rc_cell(A.W, x, y, z), bc, &got) : rc_sample_global<false>(V, A.W, bc, x, y, z, &got.s, nullptr);
                if (ok) r = got; else st |= OP_SAMPLE_INVALID;
                if (GRAD) { // k_rc_shade's central difference, unnormalised
                    const float h = 0.5f * A.W.res;
                    bool all = true;
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        float sp = 0.0f, sm = 0.0f;
                        all = all && sample_sdf(V, A.W, bc, x + (a == 0 ? h : 0.0f), y + (a == 1 ? h : 0.0f), z + (a == 2 ? h : 0.0f), &sp)
                                  && sample_sdf(V, A.W, bc, x - (a == 0 ? h : 0.0f), y - (a == 1 ? h : 0.0f), z - (a == 2 ? h : 0.0f), &sm);
                        d[a] = sp - sm;
                    }
                    if (!all) { d[0] = d[1] = d[2] = 0.0f; st |= OP_SAMPLE_NO_GRADIENT; }
                }
            }
        } else { // ReadVoxelInterpolate as k_transform_fill_wave evaluates it
            const float half = A.W.res / 2;
            const float n0 = x - half, n1 = y - half, n2 = z - half;
            const float e0 = n0 / A.W.res, e1 = n1 / A.W.res, e2 = n2 / A.W.res;
            if (!sample_in_range(e0, e1, e2)) {
                st = OP_SAMPLE_INVALID | OP_SAMPLE_OUT_OF_RANGE;
            } else {
                const int p0 = (int)floorf(e0), p1 = (int)floorf(e1), p2 = (int)floorf(e2);
                Vox5 v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = fetch_voxel_cached(V, bc, p0 + (k & 1), p1 + ((k >> 1) & 1), p2 + ((k >> 2) & 1));
                const float xw = (n0 - (float)p0 * A.W.res) / A.W.res, yw = (n1 - (float)p1 * A.W.res) / A.W.res, zw = (n2 - (float)p2 * A.W.res) / A.W.res;
                r = interp_taps(v, xw, yw, zw);
                if (r.w == 0) st |= OP_SAMPLE_INVALID;
            }
        }
        if (A.voxels) {
            float* o = A.voxels + 5 * i;
            o[0] = r.s; o[1] = r.w; o[2] = r.c0; o[3] = r.c1; o[4] = r.c2;
        }
        if (GRAD) { float* o = A.gradients + 3 * i; o[0] = d[0]; o[1] = d[1]; o[2] = d[2]; }
        if (A.status) A.status[i] = (unsigned char)st;
        if (!(st & OP_SAMPLE_INVALID)) {
            ++n_valid;
            const float as = fabsf(r.s);
            sum_abs += (double)as;
            sum_sq += (double)r.s * (double)r.s;
            max_abs = fmaxf(max_abs, as);
        }
        if (GRAD && !(st & OP_SAMPLE_NO_GRADIENT)) ++n_grad;
        if (st & OP_SAMPLE_OUT_OF_RANGE) ++n_oor;
    }
    // one row per workgroup (every lane gets here: the loop has no early exit)
    n_valid = wave_sum(n_valid); n_grad = wave_sum(n_grad); n_oor = wave_sum(n_oor);
    sum_abs = wave_sum_f64(sum_abs); sum_sq = wave_sum_f64(sum_sq);
    max_abs = wave_max(max_abs);
    if ((threadIdx.x & 63u) == 0) s_part[threadIdx.x >> 6] = SampleRow{n_valid, n_grad, n_oor, sum_abs, sum_sq, max_abs, 0u};
    __syncthreads();
    if (threadIdx.x == 0) {
        SampleRow t = s_part[0];
        for (int w = 1; w < kSampleWg / 64; ++w) {
            t.valid += s_part[w].valid; t.gradients += s_part[w].gradients; t.out_of_range += s_part[w].out_of_range;
            t.sum_abs += s_part[w].sum_abs; t.sum_sq += s_part[w].sum_sq; t.max_abs = fmaxf(t.max_abs, s_part[w].max_abs);
        }
        A.rows[blockIdx.x] = t;
    }
}

} // namespace

extern "C" {

int op_volume_sample(op_volume* v, const float* xyz, size_t n, int mem, const float* T, int mode, float* voxels, float* gradients, uint8_t* status,
                     op_volume_sample_stats* stats) {
    // the argument checks need no device
    if (mem != OP_MEM_HOST && mem != OP_MEM_DEVICE) return fail(OP_ERR_INVALID, "op_volume_sample: bad mem %d", mem);
    if (mode != OP_SAMPLE_TRILINEAR && mode != OP_SAMPLE_REFERENCE) return fail(OP_ERR_INVALID, "op_volume_sample: bad mode %d", mode);
    if (n > 0 && !xyz) return fail(OP_ERR_INVALID, "op_volume_sample: null xyz");
    if (!voxels && !gradients && !status && !stats) return fail(OP_ERR_INVALID, "op_volume_sample: no output is asked for");
    if (gradients && mode == OP_SAMPLE_REFERENCE) return fail(OP_ERR_INVALID, "op_volume_sample: gradients are defined for OP_SAMPLE_TRILINEAR only");
    OP_VOL(v);
    if (stats) *stats = op_volume_sample_stats{};
    OP_TRY(vol_check(v)); // every accepted frame is fused, the stream idle
    if (n == 0) return OP_OK;

    op::Scope tmp;
    tmp.bind(v->stream);
    SampleArgs A{};
    A.n = n;
    A.has_T = T ? 1 : 0;
    if (T) for (int k = 0; k < 16; ++k) A.T[k] = T[k];
    A.W.res = v->res; A.W.inv_res = 1.0f / v->res;
    OP_TRY(tmp.input(xyz, 3 * n, mem, &A.xyz));
    A.voxels = voxels; A.gradients = gradients; A.status = status;
    if (mem == OP_MEM_HOST) {
        if (voxels) OP_TRY(tmp.alloc(&A.voxels, 5 * n));
        if (gradients) OP_TRY(tmp.alloc(&A.gradients, 3 * n));
        if (status) OP_TRY(tmp.alloc(&A.status, n));
    }
    const unsigned grid = (unsigned)std::min<size_t>((n + kSampleWg - 1) / kSampleWg, kSampleMaxGrid);
    OP_TRY(tmp.alloc(&A.rows, (size_t)grid));
    SampleRow* h_rows = nullptr;
    if (stats) OP_TRY(tmp.pinned(&h_rows, (size_t)grid));

    const VolView V = v->view();
    const dim3 g(grid), b(kSampleWg);
    if (mode == OP_SAMPLE_REFERENCE) hipLaunchKernelGGL((k_volume_sample<OP_SAMPLE_REFERENCE, true, false>), g, b, 0, v->stream, V, A);
    else if (voxels && gradients) hipLaunchKernelGGL((k_volume_sample<OP_SAMPLE_TRILINEAR, true, true>), g, b, 0, v->stream, V, A);
    else if (voxels) hipLaunchKernelGGL((k_volume_sample<OP_SAMPLE_TRILINEAR, true, false>), g, b, 0, v->stream, V, A);
    else if (gradients) hipLaunchKernelGGL((k_volume_sample<OP_SAMPLE_TRILINEAR, false, true>), g, b, 0, v->stream, V, A);
    else hipLaunchKernelGGL((k_volume_sample<OP_SAMPLE_TRILINEAR, false, false>), g, b, 0, v->stream, V, A);
    OP_HIP(hipGetLastError());
    if (stats) OP_HIP(hipMemcpyAsync(h_rows, A.rows, sizeof(SampleRow) * grid, hipMemcpyDeviceToHost, v->stream));
    OP_HIP(hipStreamSynchronize(v->stream));
    if (mem == OP_MEM_HOST) {
        if (voxels) OP_HIP(hipMemcpy(voxels, A.voxels, sizeof(float) * 5 * n, hipMemcpyDeviceToHost));
        if (gradients) OP_HIP(hipMemcpy(gradients, A.gradients, sizeof(float) * 3 * n, hipMemcpyDeviceToHost));
        if (status) OP_HIP(hipMemcpy(status, A.status, n, hipMemcpyDeviceToHost));
    }
    if (stats) {
        const SampleRow* rows = h_rows;
        op_volume_sample_stats s{};
        s.queries = n;
        for (unsigned k = 0; k < grid; ++k) { // in index order, in double
            s.valid += rows[k].valid; s.gradients += rows[k].gradients; s.out_of_range += rows[k].out_of_range;
            s.sum_abs_sdf += rows[k].sum_abs; s.sum_sq_sdf += rows[k].sum_sq;
            s.max_abs_sdf = std::max(s.max_abs_sdf, rows[k].max_abs);
        }
        *stats = s;
    }
    return OP_OK;
}

} // extern "C"
