// downsample.hip -- voxel-grid down-sampling of a point cloud on the device: geometry::PointCloud::DownSample (Geometry/PointCloud.cpp:145-189)
// and the body of Submap::GenerateSubmapModel's loop (DenseSlam.h:24-28: LoadFromRGBD + Transform + DownSample) without leaving the device.
// The kernels restate the host loop of host/one_piece/src/PointCloud.cpp:88-115 operation by operation, so that the class surface can switch
// paths (OP_RUNTIME_OPT_POINT_CLOUD_DOWNSAMPLE) without changing a bit: the cell of a point is (int)floorf(p / grid_len) with an IEEE divide,
// output point j is the j-th distinct cell in order of first appearance, every value is the float32 sum of the cell's members IN INPUT ORDER
// (separate adds: the library is built with -ffp-contract=off) divided once by (float)count.
//
//   k_ds_bounds    one thread per point: validity (ORed into an error word), per-axis min / max cell (wave reduction, then one integer atomic
//                  per workgroup and word)
//   k_ds_keys      (cell - lowest cell) of the three axes packed into one key of just the bits the cloud's extent needs, next to the index
//   rocprim::radix_sort_pairs over those bits, STABLE: every cell becomes one segment whose members are in input order
//   k_ds_heads     segment starts: the first member of a segment is the cell's first appearance -> a flag at that INPUT index
//   rocprim::exclusive_scan of the flags over the input indices: the output slot of every cell (no second sort)
//   k_ds_segments  slot -> where its segment starts
//   k_ds_sum       one lane per (cell, channel), up to 9 a cell: walks the segment, adds in order, divides, writes slot j
//
// The worst case -- every point in one cell -- is ONE dependent chain of n adds per channel.  That is the definition's own serial floor (the
// one k_seq_sums lives with); a tree or an atomic sum would be faster and would not be this function.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "cell_keys.hpp"
#include "common.hpp"

namespace {

using op::check_mem;
using op::fail;
using op::Scope;

using op::cells::blocks_for;
using op::cells::Bounds;
using op::cells::cell_of;
using op::cells::check_grid_len;
using op::cells::kBadPoint;
using op::cells::KeyLayout;
using op::cells::kThreads;
using op::cells::load_points;
constexpr int kSumAhead = 8;   // members whose loads k_ds_sum issues before it adds them

__global__ __launch_bounds__(kThreads) void k_ds_bounds(const float* __restrict__ xyz, size_t n, float grid_len, Bounds* __restrict__ bounds) {
    __shared__ float tile[3 * kThreads];
    float p[3];
    load_points(xyz, n, tile, p[0], p[1], p[2]);
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    bool ok = true;
    int c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = cell_of(p[k], grid_len, ok);
    op::cells::fold_bounds(i < n && ok, c, i < n && !ok ? kBadPoint : 0u, bounds);
}

__global__ __launch_bounds__(kThreads) void k_ds_keys(const float* __restrict__ xyz, size_t n, float grid_len, KeyLayout layout,
                                                      unsigned long long* __restrict__ keys, unsigned* __restrict__ index) {
    __shared__ float tile[3 * kThreads];
    float p[3];
    load_points(xyz, n, tile, p[0], p[1], p[2]);
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    keys[i] = op::cells::pack_key(p, grid_len, layout);
    index[i] = (unsigned)i;
}

__global__ __launch_bounds__(kThreads) void k_ds_heads(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ index, size_t n,
                                                       unsigned* __restrict__ flag /* zeroed, by input index */) {
    const size_t s = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (s < n && (s == 0 || keys[s] != keys[s - 1])) flag[index[s]] = 1u;
}

__global__ __launch_bounds__(kThreads) void k_ds_segments(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ index, size_t n,
                                                          const unsigned* __restrict__ slot, unsigned* __restrict__ segment_start) {
    const size_t s = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (s < n && (s == 0 || keys[s] != keys[s - 1])) segment_start[slot[index[s]]] = (unsigned)s;
}

struct Channels { const float* src[3]; float* dst[3]; int arrays; }; // points, then colours and / or normals

// Lane t owns channel t % (3 * arrays) of cell t / (3 * arrays); the lanes of a cell read the same keys and indices (one request).
__global__ __launch_bounds__(kThreads) void k_ds_sum(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ index, size_t n,
                                                     const unsigned* __restrict__ segment_start, size_t cells, Channels ch) {
    const size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x;
    const unsigned per_cell = 3u * (unsigned)ch.arrays;
    const size_t j = t / per_cell;
    if (j >= cells) return;
    const unsigned c = (unsigned)(t - j * per_cell), a = c / 3u, k = c - 3u * a;
    const float* __restrict__ src = a == 0 ? ch.src[0] : (a == 1 ? ch.src[1] : ch.src[2]);
    float* __restrict__ dst = a == 0 ? ch.dst[0] : (a == 1 ? ch.dst[1] : ch.dst[2]);
    size_t s = segment_start[j];
    const unsigned long long key = keys[s];
    const unsigned first = index[s];
    float acc = src[3 * (size_t)first + k]; // out->points.push_back(p), then += per further member (PointCloud.cpp:98, 102)
    unsigned count = 1;
    // The adds are one chain in member order; only the LOADS run ahead, kSumAhead members at a time (a segment is a run of equal keys, so
    // the members of a batch are a prefix of it).
    bool more = true;
    for (++s; more; s += kSumAhead) {
        bool member[kSumAhead];
        float v[kSumAhead];
#pragma unroll
        for (int u = 0; u < kSumAhead; ++u) {
            member[u] = s + u < n && keys[s + u] == key;
            v[u] = src[3 * (size_t)(member[u] ? index[s + u] : first) + k];
        }
#pragma unroll
        for (int u = 0; u < kSumAhead; ++u) {
            more = more && member[u];
            if (more) { acc += v[u]; ++count; }
        }
    }
    dst[3 * j + k] = acc / (float)count;
}

struct Mat4 { float m[16]; };

// geometry::TransformPoint (host/one_piece/src/Geometry.cpp:19-23), in place
__global__ __launch_bounds__(kThreads) void k_ds_transform(float* __restrict__ xyz, size_t n, Mat4 T) {
    __shared__ float tile[3 * kThreads];
    float x, y, z;
    load_points(xyz, n, tile, x, y, z);
    float q[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) q[r] = ((T.m[4 * r] * x + T.m[4 * r + 1] * y) + T.m[4 * r + 2] * z) + T.m[4 * r + 3] * 1.0f;
    tile[3 * threadIdx.x] = q[0] / q[3]; tile[3 * threadIdx.x + 1] = q[1] / q[3]; tile[3 * threadIdx.x + 2] = q[2] / q[3]; // each thread its own three words
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * kThreads * 3, end = n * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const size_t e = base + (size_t)k * kThreads + threadIdx.x;
        if (e < end) xyz[e] = tile[k * kThreads + threadIdx.x];
    }
}

// The down-sampling proper, on device arrays (d_colors / d_normals may be null); the outputs follow `mem`.
int downsample_device(Scope& s, const float* d_xyz, const float* d_colors, const float* d_normals, size_t n, float grid_len, int mem, float* xyz_out,
                      float* colors_out, float* normals_out, size_t* n_out) {
    Bounds* d_bounds = nullptr;
    OP_TRY(s.alloc(&d_bounds, (size_t)1));
    Bounds bounds = {0u, {INT_MAX, INT_MAX, INT_MAX}, {INT_MIN, INT_MIN, INT_MIN}};
    OP_HIP(hipMemcpyAsync(d_bounds, &bounds, sizeof(bounds), hipMemcpyHostToDevice, s.stream));
    hipLaunchKernelGGL(k_ds_bounds, dim3(blocks_for(n)), dim3(kThreads), 0, s.stream, d_xyz, n, grid_len, d_bounds);
    OP_HIP(hipGetLastError());
    OP_HIP(hipMemcpyAsync(&bounds, d_bounds, sizeof(bounds), hipMemcpyDeviceToHost, s.stream));
    OP_HIP(hipStreamSynchronize(s.stream));
    if (bounds.error)
        return fail(OP_ERR_INVALID, "a coordinate is not finite, or its cell at grid_len %g is outside the int range", (double)grid_len);
    KeyLayout layout;
    int total_bits = 0;
    OP_TRY(op::cells::key_layout(bounds, grid_len, "cloud", &layout, &total_bits));

    unsigned long long *d_keys = nullptr, *d_keys_sorted = nullptr;
    unsigned *d_index = nullptr, *d_index_sorted = nullptr, *d_flag = nullptr, *d_slot = nullptr, *d_start = nullptr;
    OP_TRY(s.alloc(&d_keys, n));
    OP_TRY(s.alloc(&d_keys_sorted, n));
    OP_TRY(s.alloc(&d_index, n));
    OP_TRY(s.alloc(&d_index_sorted, n));
    OP_TRY(s.alloc(&d_flag, n));
    OP_TRY(s.alloc(&d_slot, n + 1));
    size_t sort_bytes = 0, scan_bytes = 0;
    OP_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, d_keys, d_keys_sorted, d_index, d_index_sorted, n, 0u, (unsigned)total_bits, s.stream));
    OP_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, d_flag, d_slot, 0u, n, rocprim::plus<unsigned>(), s.stream));
    unsigned char* d_tmp = nullptr;
    OP_TRY(s.alloc(&d_tmp, std::max(sort_bytes, scan_bytes)));

    hipLaunchKernelGGL(k_ds_keys, dim3(blocks_for(n)), dim3(kThreads), 0, s.stream, d_xyz, n, grid_len, layout, d_keys, d_index);
    OP_HIP(rocprim::radix_sort_pairs(d_tmp, sort_bytes, d_keys, d_keys_sorted, d_index, d_index_sorted, n, 0u, (unsigned)total_bits, s.stream));
    OP_HIP(hipMemsetAsync(d_flag, 0, n * sizeof(unsigned), s.stream));
    hipLaunchKernelGGL(k_ds_heads, dim3(blocks_for(n)), dim3(kThreads), 0, s.stream, d_keys_sorted, d_index_sorted, n, d_flag);
    OP_HIP(rocprim::exclusive_scan(d_tmp, scan_bytes, d_flag, d_slot, 0u, n, rocprim::plus<unsigned>(), s.stream));
    OP_HIP(hipGetLastError());
    unsigned last[2] = {0u, 0u}; // cells = slot of the last point + its flag
    OP_HIP(hipMemcpyAsync(&last[0], d_slot + (n - 1), sizeof(unsigned), hipMemcpyDeviceToHost, s.stream));
    OP_HIP(hipMemcpyAsync(&last[1], d_flag + (n - 1), sizeof(unsigned), hipMemcpyDeviceToHost, s.stream));
    OP_HIP(hipStreamSynchronize(s.stream));
    const size_t cells = (size_t)last[0] + last[1];
    if (cells < 1 || cells > n) return fail(OP_ERR_HIP, "down-sampling counted %zu cells for %zu points", cells, n);

    OP_TRY(s.alloc(&d_start, cells));
    hipLaunchKernelGGL(k_ds_segments, dim3(blocks_for(n)), dim3(kThreads), 0, s.stream, d_keys_sorted, d_index_sorted, n, d_slot, d_start);
    Channels ch = {{d_xyz, nullptr, nullptr}, {nullptr, nullptr, nullptr}, 1};
    float* host_out[3] = {xyz_out, nullptr, nullptr};
    if (d_colors) { ch.src[ch.arrays] = d_colors; host_out[ch.arrays] = colors_out; ++ch.arrays; }
    if (d_normals) { ch.src[ch.arrays] = d_normals; host_out[ch.arrays] = normals_out; ++ch.arrays; }
    for (int a = 0; a < ch.arrays; ++a) {
        if (mem == OP_MEM_DEVICE) ch.dst[a] = host_out[a];
        else OP_TRY(s.alloc(&ch.dst[a], cells * 3));
    }
    hipLaunchKernelGGL(k_ds_sum, dim3(blocks_for(cells * 3 * (size_t)ch.arrays)), dim3(kThreads), 0, s.stream, d_keys_sorted, d_index_sorted, n, d_start, cells, ch);
    OP_HIP(hipGetLastError());
    if (mem == OP_MEM_HOST)
        for (int a = 0; a < ch.arrays; ++a) OP_TRY(s.output(host_out[a], static_cast<const float*>(ch.dst[a]), cells * 3, mem));
    OP_HIP(hipStreamSynchronize(s.stream));
    *n_out = cells;
    return OP_OK;
}

} // namespace

extern "C" {

int op_point_cloud_downsample(const float* xyz, const float* colors, const float* normals, size_t n, float grid_len, int mem, int device, float* xyz_out,
                              float* colors_out, float* normals_out, size_t* n_out) {
    if (!n_out || (n && (!xyz || !xyz_out || (colors && !colors_out) || (normals && !normals_out)))) return fail(OP_ERR_INVALID, "null argument");
    OP_TRY(check_mem(mem));
    OP_TRY(check_grid_len(grid_len));
    if (n > 0x7fffffffu / 3) return fail(OP_ERR_INVALID, "too many points");
    Scope s;
    OP_TRY(s.open(device));
    *n_out = 0;
    if (n == 0) return OP_OK;
    const float *d_xyz = nullptr, *d_colors = nullptr, *d_normals = nullptr;
    OP_TRY(s.input(xyz, n * 3, mem, &d_xyz));
    if (colors) OP_TRY(s.input(colors, n * 3, mem, &d_colors));
    if (normals) OP_TRY(s.input(normals, n * 3, mem, &d_normals));
    return downsample_device(s, d_xyz, d_colors, d_normals, n, grid_len, mem, xyz_out, colors_out, normals_out, n_out);
}

int op_points_from_rgbd_downsampled(const op_camera* cam, const void* depth, int depth_fmt, const uint8_t* rgb, const float* T, float grid_len, int mem, int device,
                                    float* xyz_out, float* colors_out, size_t* n_out) {
    if (!cam || !depth || !rgb || !xyz_out || !colors_out || !n_out) return fail(OP_ERR_INVALID, "null argument");
    if (cam->width <= 0 || cam->height <= 0) return fail(OP_ERR_INVALID, "invalid camera");
    if (depth_fmt != OP_DEPTH_F32 && depth_fmt != OP_DEPTH_U16) return fail(OP_ERR_INVALID, "unknown depth format %d", depth_fmt);
    OP_TRY(check_mem(mem));
    OP_TRY(check_grid_len(grid_len));
    const size_t npix = (size_t)cam->width * cam->height;
    if (npix > 0x7fffffffu / 3) return fail(OP_ERR_INVALID, "image too large");
    Scope s;
    OP_TRY(s.open(device));
    *n_out = 0;
    const unsigned char *d_depth = nullptr, *d_rgb = nullptr;
    OP_TRY(s.input(static_cast<const unsigned char*>(depth), npix * (depth_fmt == OP_DEPTH_U16 ? 2 : 4), mem, &d_depth));
    OP_TRY(s.input(static_cast<const unsigned char*>(rgb), npix * 3, mem, &d_rgb));
    float *d_xyz = nullptr, *d_colors = nullptr;
    OP_TRY(s.alloc(&d_xyz, npix * 3));
    OP_TRY(s.alloc(&d_colors, npix * 3));
    size_t n = 0; // the library's own LoadFromRGBD, device to device, on the null stream
    OP_TRY(op_points_from_rgbd(cam, d_depth, depth_fmt, d_rgb, OP_MEM_DEVICE, device, d_xyz, d_colors, &n));
    OP_HIP(hipStreamSynchronize(nullptr)); // both arrays final before this call's own (non-blocking) stream reads them, whatever that entry waits for itself
    if (n == 0) return OP_OK;
    if (T) {
        Mat4 m;
        std::memcpy(m.m, T, sizeof(m.m));
        hipLaunchKernelGGL(k_ds_transform, dim3(blocks_for(n)), dim3(kThreads), 0, s.stream, d_xyz, n, m);
        OP_HIP(hipGetLastError());
    }
    return downsample_device(s, d_xyz, d_colors, nullptr, n, grid_len, mem, xyz_out, colors_out, nullptr, n_out);
}

} // extern "C"
