// mesh_cluster.hip -- clustering mesh simplification on the device: geometry::TriangleMesh::ClusteringSimplify (Geometry/MeshSimplification.cpp:579-657),
// alone and fused with the volume's mesh extraction so that the triangle soup never leaves the device.
// The kernels restate the host loop of host/one_piece/src/TriangleMesh.cpp (ClusteringSimplify + Compact) operation by operation, so that the
// class surface can switch paths (OP_RUNTIME_OPT_MESH_CLUSTERING) without changing a bit.  Corner c = 3 t + k of triangle t is vertex
// v = triangles[t](k) at p = points[v]:
//   * its cell is (int)floorf(p / grid_len) per axis, an IEEE divide; cells exist in order of first appearance over c = 0, 1, 2, ...
//   * a cell's representative is the vertex of its first corner; its position is (float)(sum / (double)count), sum the DOUBLE chain
//     ((0.0 + p_c0) + p_c1) + ... over all its corners in corner order (a vertex shared by m corners counts m times);
//   * triangle t becomes its three representatives and is dropped when two of them are equal -- two corners in one cell;
//   * output vertices are numbered by first appearance among the corners of the KEPT triangles; colours and normals are the representative's.
//
//   k_mc_bounds    one thread per corner: index and coordinate validity (ORed into an error word), per-axis min / max cell
//   k_mc_keys      (cell - lowest cell) of the three axes packed into one key of just the bits the extent needs, next to the corner index
//   rocprim::radix_sort_pairs over those bits, STABLE: every cell becomes one segment whose corners are in corner order
//   k_mc_heads     1 at every segment start; rocprim::exclusive_scan -> the segment number of every sorted position
//   k_mc_segments  segment -> where it starts; corner -> its segment (two corners share a representative exactly when they share a segment)
//   k_mc_keep      per triangle: its three segments differ; rocprim::exclusive_scan -> the slot of every kept triangle
//   k_mc_sum       one lane per (segment, axis): walks the segment, adds in order in double, divides; finds the first corner of a kept triangle
//                  and flags it; rocprim::exclusive_scan of those flags over the corners -> the new number of every surviving cell
//   k_mc_vertices  surviving cell -> its output row: the mean, the representative's colour and normal
//   k_mc_triangles kept triangle -> the new numbers of its three cells
//
// The worst case -- every corner in one cell -- is ONE dependent chain of 3 nt double adds per axis: the definition's own serial floor, as for
// k_ds_sum; a tree or an atomic sum would be faster and would not be this function.  (The chain waits for its gathers -- corner index, vertex index,
// coordinate, keep flag -- far longer than for an add, so the loads run kSumAhead members ahead of the adds.)
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "cell_keys.hpp"
#include "common.hpp"
#include "mesh_ops.hpp"
#include "volume_core.hpp"

namespace {

using op::check_mem;
using op::fail;
using op::Scope;
using op::mesh::cluster_device;
using op::cells::blocks_for;
using op::cells::Bounds;
using op::cells::cell_of;
using op::cells::check_grid_len;
using op::cells::kBadPoint;
using op::cells::KeyLayout;
using op::cells::kThreads;
using op::cells::load_points;

constexpr unsigned kBadIndex = 2u;
constexpr unsigned kNone = 0xffffffffu;
constexpr int kSumAhead = 8;   // members whose loads k_mc_sum issues before it adds them

// The position of corner c.  A soup (triangles == nullptr: corner c IS vertex c) is read as a workgroup's 3 * kThreads consecutive floats;
// an indexed mesh gathers.  ok = the index is inside the vertex array (a bad one loads nothing).  Called by every thread of the workgroup.
__device__ inline bool corner_point(const float* __restrict__ xyz, size_t nv, const unsigned* __restrict__ triangles, size_t n, float (&tile)[3 * kThreads],
                                    float (&p)[3]) {
    if (!triangles) { load_points(xyz, n, tile, p[0], p[1], p[2]); return true; }
    const size_t c = (size_t)blockIdx.x * kThreads + threadIdx.x;
    const size_t v = c < n ? triangles[c] : 0;
    const bool ok = v < nv;
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = ok ? xyz[3 * v + k] : 0.0f;
    return ok;
}

__global__ __launch_bounds__(kThreads) void k_mc_bounds(const float* __restrict__ xyz, size_t nv, const unsigned* __restrict__ triangles, size_t n, float grid_len,
                                                        Bounds* __restrict__ bounds) {
    __shared__ float tile[3 * kThreads];
    float p[3];
    const bool in_range = corner_point(xyz, nv, triangles, n, tile, p);
    const size_t c = (size_t)blockIdx.x * kThreads + threadIdx.x;
    bool ok = true;
    int cell[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) cell[k] = cell_of(p[k], grid_len, ok);
    const unsigned error = c >= n ? 0u : (!in_range ? kBadIndex : (!ok ? kBadPoint : 0u));
    op::cells::fold_bounds(c < n && in_range && ok, cell, error, bounds);
}

__global__ __launch_bounds__(kThreads) void k_mc_keys(const float* __restrict__ xyz, size_t nv, const unsigned* __restrict__ triangles, size_t n, float grid_len,
                                                      KeyLayout layout, unsigned long long* __restrict__ keys, unsigned* __restrict__ index) {
    __shared__ float tile[3 * kThreads];
    float p[3];
    corner_point(xyz, nv, triangles, n, tile, p); // (every index passed k_mc_bounds)
    const size_t c = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (c >= n) return;
    keys[c] = op::cells::pack_key(p, grid_len, layout);
    index[c] = (unsigned)c;
}

__global__ __launch_bounds__(kThreads) void k_mc_heads(const unsigned long long* __restrict__ keys, size_t n, unsigned* __restrict__ head) {
    const size_t s = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (s < n) head[s] = s == 0 || keys[s] != keys[s - 1] ? 1u : 0u;
}

// before[s] = segment starts before sorted position s: the segment of s is before[s] + head[s] - 1
__global__ __launch_bounds__(kThreads) void k_mc_segments(const unsigned* __restrict__ head, const unsigned* __restrict__ before, const unsigned* __restrict__ index, size_t n,
                                                          unsigned* __restrict__ segment_start, unsigned* __restrict__ segment_of_corner) {
    const size_t s = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (s >= n) return;
    const unsigned j = before[s] + head[s] - 1u;
    if (head[s]) segment_start[j] = (unsigned)s;
    segment_of_corner[index[s]] = j;
}

__global__ __launch_bounds__(kThreads) void k_mc_keep(const unsigned* __restrict__ segment_of_corner, size_t nt, unsigned* __restrict__ keep) {
    const size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= nt) return;
    const unsigned a = segment_of_corner[3 * t], b = segment_of_corner[3 * t + 1], c = segment_of_corner[3 * t + 2];
    keep[t] = a == b || a == c || b == c ? 0u : 1u; // TriangleMesh.cpp:133
}

// Lane t owns axis t % 3 of segment t / 3; the three lanes of a segment read the same indices (one request).
__global__ __launch_bounds__(kThreads) void k_mc_sum(const float* __restrict__ xyz, const unsigned* __restrict__ triangles, const unsigned* __restrict__ index, size_t n,
                                                     const unsigned* __restrict__ segment_start, size_t cells, const unsigned* __restrict__ keep,
                                                     float* __restrict__ mean, unsigned* __restrict__ representative, unsigned* __restrict__ first_kept,
                                                     unsigned* __restrict__ flag /* zeroed, by corner */) {
    const size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x;
    const size_t j = t / 3;
    if (j >= cells) return;
    const unsigned k = (unsigned)(t - 3 * j);
    const size_t start = segment_start[j], end = j + 1 < cells ? (size_t)segment_start[j + 1] : n;
    double acc = 0.0; // Cell c = {v, 0, {0, 0, 0}}, then sum[a] += p(a) per corner (TriangleMesh.cpp:126-130)
    unsigned kept = kNone;
    // The adds are one chain in corner order; only the LOADS run ahead, kSumAhead members at a time.
    for (size_t s = start; s < end; s += kSumAhead) {
        float v[kSumAhead];
        unsigned c[kSumAhead], kp[kSumAhead];
#pragma unroll
        for (int u = 0; u < kSumAhead; ++u) {
            c[u] = index[s + u < end ? s + u : start];
            const size_t vertex = triangles ? triangles[c[u]] : c[u];
            v[u] = xyz[3 * vertex + k];
            kp[u] = keep[c[u] / 3u];
        }
#pragma unroll
        for (int u = 0; u < kSumAhead; ++u)
            if (s + u < end) {
                acc += (double)v[u];
                if (kept == kNone && kp[u]) kept = c[u];
            }
    }
    mean[3 * j + k] = (float)(acc / (double)(unsigned)(end - start)); // c.sum[a] / c.count, count an unsigned (:138)
    if (k == 0) {
        const unsigned c0 = index[start];
        representative[j] = triangles ? triangles[c0] : c0;
        first_kept[j] = kept;
        if (kept != kNone) flag[kept] = 1u;
    }
}

struct Attributes { const float* src[2]; float* dst[2]; int arrays; }; // colours and / or normals

__global__ __launch_bounds__(kThreads) void k_mc_vertices(const float* __restrict__ mean, const unsigned* __restrict__ representative, const unsigned* __restrict__ first_kept,
                                                          const unsigned* __restrict__ number /* by corner */, size_t cells, float* __restrict__ xyz_out, Attributes at,
                                                          unsigned* __restrict__ number_of_segment) {
    const size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x;
    const size_t j = t / 3;
    if (j >= cells) return;
    const unsigned k = (unsigned)(t - 3 * j), kept = first_kept[j];
    if (kept == kNone) return; // a cell no kept triangle refers to vanishes (Compact)
    const size_t o = number[kept], r = representative[j];
    xyz_out[3 * o + k] = mean[3 * j + k];
#pragma unroll
    for (int a = 0; a < 2; ++a)
        if (a < at.arrays) at.dst[a][3 * o + k] = at.src[a][3 * r + k];
    if (k == 0) number_of_segment[j] = (unsigned)o;
}

__global__ __launch_bounds__(kThreads) void k_mc_triangles(const unsigned* __restrict__ segment_of_corner, const unsigned* __restrict__ number_of_segment,
                                                           const unsigned* __restrict__ keep, const unsigned* __restrict__ slot, size_t nt, unsigned* __restrict__ triangles_out) {
    const size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= nt || !keep[t]) return;
    const size_t o = slot[t];
#pragma unroll
    for (int k = 0; k < 3; ++k) triangles_out[3 * o + k] = number_of_segment[segment_of_corner[3 * t + k]];
}

} // namespace

// The simplification proper, on device arrays (d_colors / d_normals may be null; d_triangles null = a soup, triangle t = vertices 3t .. 3t + 2).
// The outputs follow `mem` and are written only when both counts fit their capacities.  (Declared in mesh_ops.hpp: mesh_post.hip runs it too.)
int op::mesh::cluster_device(Scope& s, const float* d_xyz, const float* d_colors, const float* d_normals, size_t nv, const unsigned* d_triangles, size_t nt, float grid_len, int mem,
                   float* xyz_out, float* colors_out, float* normals_out, size_t cap_vertices, unsigned* triangles_out, size_t cap_triangles, size_t* nv_out, size_t* nt_out) {
    const size_t n = 3 * nt;
    Bounds* d_bounds = nullptr;
    OP_TRY(s.alloc(&d_bounds, (size_t)1));
    Bounds bounds = {0u, {INT_MAX, INT_MAX, INT_MAX}, {INT_MIN, INT_MIN, INT_MIN}};
    OP_HIP(hipMemcpyAsync(d_bounds, &bounds, sizeof(bounds), hipMemcpyHostToDevice, s.stream));
    hipLaunchKernelGGL(k_mc_bounds, dim3(blocks_for(n)), dim3(kThreads), 0, s.stream, d_xyz, nv, d_triangles, n, grid_len, d_bounds);
    OP_HIP(hipGetLastError());
    OP_HIP(hipMemcpyAsync(&bounds, d_bounds, sizeof(bounds), hipMemcpyDeviceToHost, s.stream));
    OP_HIP(hipStreamSynchronize(s.stream));
    if (bounds.error & kBadIndex) return fail(OP_ERR_INVALID, "a triangle refers to a vertex beyond the %zu given", nv);
    if (bounds.error)
        return fail(OP_ERR_INVALID, "a coordinate of a referenced vertex is not finite, or its cell at grid_len %g is outside the int range", (double)grid_len);
    KeyLayout layout;
    int total_bits = 0;
    OP_TRY(op::cells::key_layout(bounds, grid_len, "mesh", &layout, &total_bits));

    unsigned long long *d_keys = nullptr, *d_keys_sorted = nullptr;
    unsigned *d_index = nullptr, *d_index_sorted = nullptr, *d_head = nullptr, *d_before = nullptr, *d_segment = nullptr, *d_keep = nullptr, *d_slot = nullptr;
    OP_TRY(s.alloc(&d_keys, n));
    OP_TRY(s.alloc(&d_keys_sorted, n));
    OP_TRY(s.alloc(&d_index, n));
    OP_TRY(s.alloc(&d_index_sorted, n));
    OP_TRY(s.alloc(&d_head, n));
    OP_TRY(s.alloc(&d_before, n));
    OP_TRY(s.alloc(&d_segment, n));
    OP_TRY(s.alloc(&d_keep, nt));
    OP_TRY(s.alloc(&d_slot, nt));
    size_t sort_bytes = 0, scan_bytes = 0, scan_bytes_nt = 0;
    OP_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, d_keys, d_keys_sorted, d_index, d_index_sorted, n, 0u, (unsigned)total_bits, s.stream));
    OP_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, d_head, d_before, 0u, n, rocprim::plus<unsigned>(), s.stream));
    OP_HIP(rocprim::exclusive_scan(nullptr, scan_bytes_nt, d_keep, d_slot, 0u, nt, rocprim::plus<unsigned>(), s.stream));
    unsigned char* d_tmp = nullptr;
    OP_TRY(s.alloc(&d_tmp, std::max(sort_bytes, std::max(scan_bytes, scan_bytes_nt))));

    hipLaunchKernelGGL(k_mc_keys, dim3(blocks_for(n)), dim3(kThreads), 0, s.stream, d_xyz, nv, d_triangles, n, grid_len, layout, d_keys, d_index);
    OP_HIP(rocprim::radix_sort_pairs(d_tmp, sort_bytes, d_keys, d_keys_sorted, d_index, d_index_sorted, n, 0u, (unsigned)total_bits, s.stream));
    hipLaunchKernelGGL(k_mc_heads, dim3(blocks_for(n)), dim3(kThreads), 0, s.stream, d_keys_sorted, n, d_head);
    OP_HIP(rocprim::exclusive_scan(d_tmp, scan_bytes, d_head, d_before, 0u, n, rocprim::plus<unsigned>(), s.stream));
    OP_HIP(hipGetLastError());
    unsigned last[2] = {0u, 0u}; // cells = segment starts before the last position + its own
    OP_HIP(hipMemcpyAsync(&last[0], d_before + (n - 1), sizeof(unsigned), hipMemcpyDeviceToHost, s.stream));
    OP_HIP(hipMemcpyAsync(&last[1], d_head + (n - 1), sizeof(unsigned), hipMemcpyDeviceToHost, s.stream));
    OP_HIP(hipStreamSynchronize(s.stream));
    const size_t cells = (size_t)last[0] + last[1];
    if (cells < 1 || cells > n) return fail(OP_ERR_HIP, "mesh clustering counted %zu cells for %zu corners", cells, n);

    unsigned *d_start = nullptr, *d_rep = nullptr, *d_first_kept = nullptr, *d_number_of_segment = nullptr;
    float* d_mean = nullptr;
    OP_TRY(s.alloc(&d_start, cells));
    OP_TRY(s.alloc(&d_rep, cells));
    OP_TRY(s.alloc(&d_first_kept, cells));
    OP_TRY(s.alloc(&d_number_of_segment, cells));
    OP_TRY(s.alloc(&d_mean, cells * 3));
    unsigned *d_flag = d_index, *d_number = d_head; // the unsorted corner indices and the head flags are spent by then: their arrays carry the flags of the surviving cells and their scan
    hipLaunchKernelGGL(k_mc_segments, dim3(blocks_for(n)), dim3(kThreads), 0, s.stream, d_head, d_before, d_index_sorted, n, d_start, d_segment);
    hipLaunchKernelGGL(k_mc_keep, dim3(blocks_for(nt)), dim3(kThreads), 0, s.stream, d_segment, nt, d_keep);
    OP_HIP(rocprim::exclusive_scan(d_tmp, scan_bytes_nt, d_keep, d_slot, 0u, nt, rocprim::plus<unsigned>(), s.stream));
    OP_HIP(hipMemsetAsync(d_flag, 0, n * sizeof(unsigned), s.stream));
    hipLaunchKernelGGL(k_mc_sum, dim3(blocks_for(cells * 3)), dim3(kThreads), 0, s.stream, d_xyz, d_triangles, d_index_sorted, n, d_start, cells, d_keep, d_mean, d_rep,
                       d_first_kept, d_flag);
    OP_HIP(rocprim::exclusive_scan(d_tmp, scan_bytes, d_flag, d_number, 0u, n, rocprim::plus<unsigned>(), s.stream));
    OP_HIP(hipGetLastError());
    unsigned tail[4] = {0u, 0u, 0u, 0u}; // vertices = number of the last corner + its flag; triangles = slot of the last triangle + its keep
    OP_HIP(hipMemcpyAsync(&tail[0], d_number + (n - 1), sizeof(unsigned), hipMemcpyDeviceToHost, s.stream));
    OP_HIP(hipMemcpyAsync(&tail[1], d_flag + (n - 1), sizeof(unsigned), hipMemcpyDeviceToHost, s.stream));
    OP_HIP(hipMemcpyAsync(&tail[2], d_slot + (nt - 1), sizeof(unsigned), hipMemcpyDeviceToHost, s.stream));
    OP_HIP(hipMemcpyAsync(&tail[3], d_keep + (nt - 1), sizeof(unsigned), hipMemcpyDeviceToHost, s.stream));
    OP_HIP(hipStreamSynchronize(s.stream));
    const size_t vertices = (size_t)tail[0] + tail[1], kept = (size_t)tail[2] + tail[3];
    if (vertices > cells || kept > nt) return fail(OP_ERR_HIP, "mesh clustering counted %zu vertices in %zu cells, %zu of %zu triangles", vertices, cells, kept, nt);
    *nv_out = vertices;
    *nt_out = kept;
    if (vertices > cap_vertices || kept > cap_triangles)
        return fail(OP_ERR_CAPACITY, "the simplified mesh has %zu vertices and %zu triangles, the buffers hold %zu and %zu", vertices, kept, cap_vertices, cap_triangles);
    if (kept == 0) return OP_OK; // (then vertices == 0 as well)

    Attributes at = {{nullptr, nullptr}, {nullptr, nullptr}, 0};
    float* host_at[2] = {nullptr, nullptr};
    if (d_colors) { at.src[at.arrays] = d_colors; host_at[at.arrays] = colors_out; ++at.arrays; }
    if (d_normals) { at.src[at.arrays] = d_normals; host_at[at.arrays] = normals_out; ++at.arrays; }
    float* d_xyz_out = xyz_out;
    unsigned* d_triangles_out = triangles_out;
    for (int a = 0; a < at.arrays; ++a) at.dst[a] = host_at[a];
    if (mem == OP_MEM_HOST) {
        OP_TRY(s.alloc(&d_xyz_out, vertices * 3));
        OP_TRY(s.alloc(&d_triangles_out, kept * 3));
        for (int a = 0; a < at.arrays; ++a) OP_TRY(s.alloc(&at.dst[a], vertices * 3));
    }
    hipLaunchKernelGGL(k_mc_vertices, dim3(blocks_for(cells * 3)), dim3(kThreads), 0, s.stream, d_mean, d_rep, d_first_kept, d_number, cells, d_xyz_out, at, d_number_of_segment);
    hipLaunchKernelGGL(k_mc_triangles, dim3(blocks_for(nt)), dim3(kThreads), 0, s.stream, d_segment, d_number_of_segment, d_keep, d_slot, nt, d_triangles_out);
    OP_HIP(hipGetLastError());
    if (mem == OP_MEM_HOST) {
        OP_HIP(hipMemcpyAsync(xyz_out, d_xyz_out, vertices * 3 * sizeof(float), hipMemcpyDeviceToHost, s.stream));
        OP_HIP(hipMemcpyAsync(triangles_out, d_triangles_out, kept * 3 * sizeof(unsigned), hipMemcpyDeviceToHost, s.stream));
        for (int a = 0; a < at.arrays; ++a) OP_HIP(hipMemcpyAsync(host_at[a], at.dst[a], vertices * 3 * sizeof(float), hipMemcpyDeviceToHost, s.stream));
    }
    OP_HIP(hipStreamSynchronize(s.stream));
    return OP_OK;
}

extern "C" {

int op_mesh_cluster_simplify(const float* points, const float* colors, const float* normals, size_t nv, const uint32_t* triangles, size_t nt, float grid_len, int mem, int device,
                             float* points_out, float* colors_out, float* normals_out, uint32_t* triangles_out, size_t* nv_out, size_t* nt_out) {
    if (!nv_out || !nt_out || (nt && (!points || !triangles || !points_out || !triangles_out || (colors && !colors_out) || (normals && !normals_out))))
        return fail(OP_ERR_INVALID, "null argument");
    OP_TRY(check_mem(mem));
    OP_TRY(check_grid_len(grid_len));
    if (nt > 0xffffffffull / 3) return fail(OP_ERR_CAPACITY, "%zu triangles: their corners are beyond 32-bit corner indices", nt);
    if (nt && nv == 0) return fail(OP_ERR_INVALID, "a triangle refers to a vertex beyond the 0 given");
    Scope s;
    OP_TRY(s.open(device));
    *nv_out = 0;
    *nt_out = 0;
    if (nt == 0) return OP_OK;
    const float *d_xyz = nullptr, *d_colors = nullptr, *d_normals = nullptr;
    const uint32_t* d_triangles = nullptr;
    OP_TRY(s.input(points, nv * 3, mem, &d_xyz));
    if (colors) OP_TRY(s.input(colors, nv * 3, mem, &d_colors));
    if (normals) OP_TRY(s.input(normals, nv * 3, mem, &d_normals));
    OP_TRY(s.input(triangles, nt * 3, mem, &d_triangles));
    const int rc = cluster_device(s, d_xyz, d_colors, d_normals, nv, d_triangles, nt, grid_len, mem, points_out, colors_out, normals_out, std::min(nv, 3 * nt), triangles_out, nt,
                                  nv_out, nt_out);
    if (rc != OP_OK) { *nv_out = 0; *nt_out = 0; }
    return rc;
}

int op_volume_extract_mesh_clustered(op_volume* v, const int32_t* tri_table, const int32_t* edge_pairs, const int32_t* only_block, float grid_len, float* points, float* colors,
                                     size_t cap_vertices, uint32_t* triangles, size_t cap_triangles, size_t* n_vertices, size_t* n_triangles) {
    if (!n_vertices || !n_triangles) return fail(OP_ERR_INVALID, "null argument");
    OP_TRY(check_grid_len(grid_len));
    OP_VOL(v);
    const bool fill = points && colors && triangles;
    Scope soup_bufs;
    soup_bufs.bind(v->stream);
    float *d_pts = nullptr, *d_col = nullptr;
    size_t soup = 0; // vertices of the soup: three per triangle
    *n_vertices = 0;
    *n_triangles = 0;
    OP_TRY(opv::vol_mesh_soup(soup_bufs, v, tri_table, edge_pairs, only_block, fill, (size_t)-1, &d_pts, &d_col, &soup));
    int rc = OP_OK;
    if (!fill) { // the sizing call: upper bounds (the soup's own sizes) -- the exact ones would take the whole pipeline
        *n_vertices = soup;
        *n_triangles = soup / 3;
    } else if (soup) {
        Scope s; // (declared later, so it returns its buffers before the soup's)
        rc = s.open(v->device);
        if (rc == OP_OK)
            rc = cluster_device(s, d_pts, d_col, nullptr, soup, nullptr, soup / 3, grid_len, OP_MEM_HOST, points, colors, nullptr, cap_vertices, triangles, cap_triangles,
                                n_vertices, n_triangles);
        if (rc != OP_OK && rc != OP_ERR_CAPACITY) { *n_vertices = 0; *n_triangles = 0; } // (too small: the counts say what is needed)
    }
    return rc;
}

} // extern "C"
