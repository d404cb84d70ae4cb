// volume_band.hip -- op_volume_band_* (include/onepiece_hip.h): the band voxels of a fused volume as a list -- centre, stored sdf, intensity of the
// stored colour -- in pool order.  What op_volume_register_volume (volume_register.hip) registers against another volume: a fused volume has no
// surface points, it has a band of voxels that each carry their own sdf.
// k_band_voxels: one 512-lane workgroup per block, lane o is voxel o = x + 8y + 64z, so a wave reads 64 consecutive floats of a 2 KB plane.  The
// count pass reads the sdf and weight planes, ballots, and lane 0 of every wave leaves its popcount in LDS; thread 0 adds the eight.  The block
// offsets are opi::device_exclusive_scan's (on the device: only the total comes back).  The emit pass repeats the test, ranks a selected voxel by
// the popcount of the lower lanes plus the LDS prefix of the lower waves, and only then reads the three colour planes.
#include "volume_core.hpp"

#include <cmath>

namespace opi { int device_exclusive_scan(const unsigned* d_count, size_t n, unsigned* d_start, hipStream_t stream, unsigned* total_out); } // icp_grid.hip

namespace {

struct BandSel { float band, min_weight; unsigned stride_mask; }; // stride_mask = voxel_stride - 1 (a power of two)

// EMIT false: counts[b] = the selected voxels of block b.  EMIT true: the list (an output that is NULL is not written).
template <bool EMIT>
__global__ __launch_bounds__(512) void k_band_voxels(VolView V, float res, BandSel S, unsigned* __restrict__ counts, const unsigned* __restrict__ offsets,
                                                     float* __restrict__ xyz, float* __restrict__ sdf_out, float* __restrict__ intensity) {
    __shared__ unsigned s_w[8];
    const unsigned b = blockIdx.x, o = threadIdx.x;
    const unsigned x = o & 7u, y = (o >> 3) & 7u, z = o >> 6;
    const float* t = V.pool + (size_t)b * kBlockFloats + o;
    const float sdf = t[0], w = t[kVox];
    const bool ok = w > 0.0f && w >= S.min_weight && fabsf(sdf) <= S.band && ((x | y | z) & S.stride_mask) == 0u; // (false for a NaN sdf or weight)
    const unsigned long long m = __ballot(ok);
    const unsigned lane = o & 63u, wave = o >> 6;
    if (lane == 0) s_w[wave] = (unsigned)__popcll(m);
    __syncthreads();
    if constexpr (!EMIT) {
        if (o == 0) {
            unsigned tot = 0;
            for (int k = 0; k < 8; ++k) tot += s_w[k];
            counts[b] = tot;
        }
    } else {
        if (!ok) return;
        unsigned rank = (unsigned)__popcll(m & ((1ULL << lane) - 1ULL));
        for (unsigned k = 0; k < wave; ++k) rank += s_w[k];
        const size_t pos = (size_t)offsets[b] + rank;
        if (xyz) { // GetGlobalPoint (VoxelCube.h:75-80), as k_integrate forms it
            const float half = res / 2;
            xyz[3 * pos] = ((float)V.keys[3 * b] * 8.0f) * res + ((float)x * res + half);
            xyz[3 * pos + 1] = ((float)V.keys[3 * b + 1] * 8.0f) * res + ((float)y * res + half);
            xyz[3 * pos + 2] = ((float)V.keys[3 * b + 2] * 8.0f) * res + ((float)z * res + half);
        }
        if (sdf_out) sdf_out[pos] = sdf;
        if (intensity) intensity[pos] = (0.114f * t[2 * kVox] + 0.587f * t[3 * kVox]) + 0.299f * t[4 * kVox];
    }
}

op_volume_band_params band_defaults(const op_volume* v) {
    op_volume_band_params p;
    p.band = 2.0f * v->res;
    p.min_weight = 1.0f;
    p.voxel_stride = 1;
    return p;
}

} // namespace

int opv::vol_band_check(const op_volume_band_params* sel, const char* who) {
    if (!sel) return OP_OK;
    if (sel->voxel_stride != 1 && sel->voxel_stride != 2 && sel->voxel_stride != 4 && sel->voxel_stride != 8)
        return fail(OP_ERR_INVALID, "%s: voxel_stride %d is not 1, 2, 4 or 8", who, sel->voxel_stride);
    if (!(sel->min_weight >= 0.0f) || !std::isfinite(sel->min_weight)) return fail(OP_ERR_INVALID, "%s: min_weight must be finite and >= 0", who);
    if (sel->band != sel->band) return fail(OP_ERR_INVALID, "%s: band is not a number", who);
    return OP_OK;
}

// The list of `src` under `sel` (checked by vol_band_check; NULL: the defaults) into buffers `out` owns; the kernels run on the source's stream, which
// is idle on return.  The caller has flushed the source (vol_check).  *n is the full count; an output pointer that is NULL is not produced, and
// none is (the pointers stay NULL) when the selection is empty or holds more than `cap` voxels.
int opv::vol_band_select(op::Scope& out, op_volume* src, const op_volume_band_params* sel, size_t cap, float** d_xyz, float** d_sdf, float** d_intensity, size_t* n) {
    const op_volume_band_params P = sel ? *sel : band_defaults(src);
    const BandSel S{P.band > 0.0f ? P.band : src->trunc, P.min_weight, (unsigned)P.voxel_stride - 1u};
    *n = 0;
    unsigned nb = 0;
    OP_TRY(vol_block_count(src, &nb));
    if (!nb) return OP_OK;
    if (nb > (UINT_MAX >> 9)) return fail(OP_ERR_CAPACITY, "op_volume_band_voxels: %u blocks, the list is indexed by 32 bits", nb);
    op::Scope tmp;
    tmp.bind(src->stream);
    unsigned *d_counts = nullptr, *d_offsets = nullptr;
    OP_TRY(tmp.alloc(&d_counts, nb));
    OP_TRY(tmp.alloc(&d_offsets, nb));
    const VolView V = src->view();
    hipLaunchKernelGGL(k_band_voxels<false>, dim3(nb), dim3(512), 0, src->stream, V, src->res, S, d_counts, (const unsigned*)nullptr, (float*)nullptr, (float*)nullptr,
                       (float*)nullptr);
    OP_HIP(hipGetLastError());
    unsigned total = 0;
    OP_TRY(opi::device_exclusive_scan(d_counts, nb, d_offsets, src->stream, &total));
    *n = total;
    if ((!d_xyz && !d_sdf && !d_intensity) || !total || total > cap) return OP_OK;
    float *x = nullptr, *s = nullptr, *y = nullptr;
    if (d_xyz) OP_TRY(out.alloc(&x, (size_t)total * 3));
    if (d_sdf) OP_TRY(out.alloc(&s, (size_t)total));
    if (d_intensity) OP_TRY(out.alloc(&y, (size_t)total));
    hipLaunchKernelGGL(k_band_voxels<true>, dim3(nb), dim3(512), 0, src->stream, V, src->res, S, (unsigned*)nullptr, (const unsigned*)d_offsets, x, s, y);
    OP_HIP(hipGetLastError());
    OP_HIP(hipStreamSynchronize(src->stream));
    if (d_xyz) *d_xyz = x;
    if (d_sdf) *d_sdf = s;
    if (d_intensity) *d_intensity = y;
    return OP_OK;
}

extern "C" {

int op_volume_band_default_params(op_volume* src, op_volume_band_params* p) {
    if (!src) return fail(OP_ERR_INVALID, "op_volume_band_default_params: null volume");
    if (!p) return fail(OP_ERR_INVALID, "op_volume_band_default_params: null params");
    *p = band_defaults(src);
    return OP_OK;
}

int op_volume_band_voxels(op_volume* src, const op_volume_band_params* sel, float* xyz, float* sdf, float* intensity, int mem, size_t cap, size_t* n) {
    // the argument checks need no device
    if (!src) return fail(OP_ERR_INVALID, "op_volume_band_voxels: null volume");
    if (!n) return fail(OP_ERR_INVALID, "op_volume_band_voxels: null n");
    if (mem != OP_MEM_HOST && mem != OP_MEM_DEVICE) return fail(OP_ERR_INVALID, "op_volume_band_voxels: bad mem %d", mem);
    OP_TRY(vol_band_check(sel, "op_volume_band_voxels"));
    OP_VOL(src);
    OP_TRY(vol_check(src)); // every accepted frame is fused, the stream idle
    op::Scope s;
    s.bind(src->stream);
    size_t total = 0;
    float *d_xyz = nullptr, *d_sdf = nullptr, *d_int = nullptr;
    OP_TRY(vol_band_select(s, src, sel, cap, xyz ? &d_xyz : nullptr, sdf ? &d_sdf : nullptr, intensity ? &d_int : nullptr, &total));
    *n = total;
    if ((!xyz && !sdf && !intensity) || !total) return OP_OK;
    if (total > cap) return fail(OP_ERR_CAPACITY, "op_volume_band_voxels: %zu voxels selected, the buffers hold %zu", total, cap);
    if (xyz) OP_TRY(s.output(xyz, (const float*)d_xyz, total * 3, mem));
    if (sdf) OP_TRY(s.output(sdf, (const float*)d_sdf, total, mem));
    if (intensity) OP_TRY(s.output(intensity, (const float*)d_int, total, mem));
    return OP_OK;
}

} // extern "C"
