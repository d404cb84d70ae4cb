// mesh_post.hip -- the rest of the fusion drivers' mesh tail on the device: geometry::TriangleMesh::ComputeNormals (Geometry/TriangleMesh.cpp, called by
// example/ImageIntegration.cpp:45, MCGenerateMesh.cpp:24, MergeMultipleSubmaps.cpp:46) and geometry::TriangleMesh::Prune (PruneMesh.cpp:15), alone and
// fused with the volume's mesh extraction and the clustering of mesh_cluster.hip so that only the finished mesh leaves the device.
// The kernels restate the host loops of host/one_piece/src/TriangleMesh.cpp (ComputeNormals, Prune + Compact) operation by operation, so that the class
// surface can switch paths (OP_RUNTIME_OPT_MESH_POSTPROCESS) without changing a bit.  Corner c = 3 t + k of triangle t is vertex v = triangles[t](k).
//
// ComputeNormals -- float32 throughout, no FMA (-ffp-contract=off), IEEE sqrt and divide:
//   k_mp_check     one thread per corner: index inside the vertices, coordinates finite (ORed into an error word)
//   k_mp_face      one thread per triangle: n = (p1 - p0) x (p2 - p0), each product rounded, then subtracted; len = sqrtf((n0 n0 + n1 n1) + n2 n2);
//                  n /= len when len > 0 (TriangleMesh.cpp Cross, Normalize)
//   k_mp_pairs     (vertex, corner) per corner; rocprim::radix_sort_pairs over bits_for(nv) bits, STABLE: every vertex becomes one segment whose
//                  corners are in corner order
//   k_mp_spans     segment boundaries -> first and one-past-last sorted position of every vertex (a vertex nothing refers to keeps 0, 0)
//   k_mp_vertex    one lane per (vertex, axis): ((+0 + n_c0) + n_c1) + ... over its corners in corner order, then the same Normalize over the three
//                  sums of the vertex (exchanged through LDS).  A soup (triangles == nullptr) has one corner per vertex and needs no sort; it still
//                  takes 0 + n -- which turns a -0 component into +0 -- and the second Normalize.
// A vertex of valence m is ONE dependent chain of m float32 adds per axis: the definition's own serial floor, as for k_ds_sum and k_mc_sum; a tree or
// float atomics would be faster and would not be this function.
//
// Prune -- integers only, so the result depends on the partition and not on any order:
//   k_mp_init      parent[v] = v, size = 0, referenced = 0, first_kept = none
//   k_mp_union     one thread per triangle: unite(v0, v1), unite(v0, v2) in a lock-free union-find -- the LARGER root is hooked under the smaller
//                  one by atomicCAS on parent[root], finds halve their path; marks the three vertices referenced
//   k_mp_label     label[v] = the root of v = the smallest vertex id of its component; a referenced vertex adds 1 to size[label]
//   k_mp_keep      keep[t] = size[label[v0]] > min_points (TriangleMesh.cpp: dropped when <= min_points); atomicMin of the corner index into
//                  first_kept[v] over the kept corners
//   k_mp_pruned    the referenced vertices of dropped components, counted (wave ballot, one atomic per wave)
//   k_mp_first     flag[c] = corner c is kept and is the first kept corner of its vertex; rocprim::exclusive_scan over the corners -> the new number
//                  of every surviving vertex (Compact: by first appearance among the kept corners); exclusive_scan of keep -> the triangle slots
//   k_mp_gather    flagged corner -> its output row: point, colour, normal; kept triangle -> the new numbers of its three vertices
// Every loop of the union-find terminates on any input: parent[x] <= x always (only a root is ever hooked, under a smaller id; a halving writes an
// ancestor), so a find moves to a strictly smaller id every step, and a unite either exits or replaces its larger root by a strictly smaller id.
// Nothing waits for another lane.
#include <algorithm>
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
using op::cells::bits_for;
using op::cells::blocks_for;
using op::cells::kThreads;
using op::mesh::cluster_device;

constexpr unsigned kBadPoint = 1u, kBadIndex = 2u;
constexpr unsigned kNone = 0xffffffffu;
constexpr int kVertexThreads = 192; // k_mp_vertex: 64 vertices x 3 axes a workgroup, so that no vertex straddles two workgroups

__device__ inline size_t vertex_of(const unsigned* __restrict__ triangles, size_t c) { return triangles ? (size_t)triangles[c] : c; }

// ---- ComputeNormals -----------------------------------------------------------------------------------------------------------------------------

// finite = the referenced coordinates must be finite (normals); the index check alone otherwise (pruning reads no coordinate)
__global__ __launch_bounds__(kThreads) void k_mp_check(const float* __restrict__ xyz, size_t nv, const unsigned* __restrict__ triangles, size_t n, int finite,
                                                       unsigned* __restrict__ error) {
    const size_t c = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (c >= n) return;
    const size_t v = vertex_of(triangles, c);
    unsigned bad = 0u;
    if (v >= nv) bad = kBadIndex;
    else if (finite) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (!isfinite(xyz[3 * v + k])) bad = kBadPoint;
    }
    if (bad) atomicOr(error, bad); // (the rare path: a mesh with one bad corner pays one atomic)
}

// TriangleMesh.cpp Normalize: n = sqrt((v0 v0 + v1 v1) + v2 v2); if (n > 0) each component is divided by n
__device__ inline void normalize(float (&v)[3]) {
    const float n = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (n > 0.0f) { v[0] /= n; v[1] /= n; v[2] /= n; }
}

__global__ __launch_bounds__(kThreads) void k_mp_face(const float* __restrict__ xyz, const unsigned* __restrict__ triangles, size_t nt, float* __restrict__ face) {
    const size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= nt) return;
    float p[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const size_t v = vertex_of(triangles, 3 * t + i);
#pragma unroll
        for (int k = 0; k < 3; ++k) p[i][k] = xyz[3 * v + k];
    }
    float a[3], b[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { a[k] = p[1][k] - p[0][k]; b[k] = p[2][k] - p[0][k]; }
    float n[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]}; // Cross
    normalize(n);
#pragma unroll
    for (int k = 0; k < 3; ++k) face[3 * t + k] = n[k];
}

__global__ __launch_bounds__(kThreads) void k_mp_pairs(const unsigned* __restrict__ triangles, size_t n, unsigned* __restrict__ keys, unsigned* __restrict__ index) {
    const size_t c = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (c >= n) return;
    keys[c] = triangles[c];
    index[c] = (unsigned)c;
}

// first[v] / last[v] (zeroed): the sorted positions [first, last) hold the corners of vertex v, in corner order
__global__ __launch_bounds__(kThreads) void k_mp_spans(const unsigned* __restrict__ keys_sorted, size_t n, unsigned* __restrict__ first, unsigned* __restrict__ last) {
    const size_t s = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (s >= n) return;
    const unsigned v = keys_sorted[s];
    if (s == 0 || keys_sorted[s - 1] != v) first[v] = (unsigned)s;
    if (s + 1 == n || keys_sorted[s + 1] != v) last[v] = (unsigned)(s + 1);
}

// Thread 3 j + k of a workgroup owns axis k of the workgroup's vertex j.  index == nullptr: a soup, vertex v has the one corner v.
__global__ __launch_bounds__(kVertexThreads) void k_mp_vertex(const float* __restrict__ face, const unsigned* __restrict__ index, const unsigned* __restrict__ first,
                                                              const unsigned* __restrict__ last, size_t nv, float* __restrict__ normals) {
    __shared__ float sums[kVertexThreads];
    const size_t v = (size_t)blockIdx.x * (kVertexThreads / 3) + threadIdx.x / 3;
    const unsigned k = threadIdx.x % 3;
    float acc = 0.0f; // normals.assign(points.size(), Point3(0, 0, 0)), then normals[v] += n per corner (TriangleMesh.cpp ComputeNormals)
    if (v < nv) {
        if (!index) acc += face[3 * (v / 3) + k];
        else
            for (size_t s = first[v], e = last[v]; s < e; ++s) acc += face[3 * (size_t)(index[s] / 3u) + k]; // one chain, in corner order
    }
    sums[threadIdx.x] = acc;
    __syncthreads();
    if (v >= nv) return;
    const unsigned j = threadIdx.x - k;
    float sum[3] = {sums[j], sums[j + 1], sums[j + 2]};
    normalize(sum);
    normals[3 * v + k] = sum[k];
}

// normals_out: nv x 3 on the device.  Refuses (nothing written) an index beyond nv and a non-finite coordinate at a referenced vertex.
int normals_device(Scope& s, const float* d_xyz, size_t nv, const unsigned* d_triangles, size_t nt, float* d_normals_out) {
    const size_t n = 3 * nt;
    if (nv == 0) return OP_OK;
    if (nt == 0) {
        OP_HIP(hipMemsetAsync(d_normals_out, 0, nv * 3 * sizeof(float), s.stream));
        OP_HIP(hipStreamSynchronize(s.stream));
        return OP_OK;
    }
    unsigned* d_error = nullptr;
    OP_TRY(s.alloc(&d_error, (size_t)1));
    OP_HIP(hipMemsetAsync(d_error, 0, sizeof(unsigned), s.stream));
    hipLaunchKernelGGL(k_mp_check, dim3(blocks_for(n)), dim3(kThreads), 0, s.stream, d_xyz, nv, d_triangles, n, 1, d_error);
    OP_HIP(hipGetLastError());
    unsigned error = 0u;
    OP_HIP(hipMemcpyAsync(&error, d_error, sizeof(unsigned), hipMemcpyDeviceToHost, s.stream));
    OP_HIP(hipStreamSynchronize(s.stream));
    if (error & kBadIndex) return fail(OP_ERR_INVALID, "a triangle refers to a vertex beyond the %zu given", nv);
    if (error) return fail(OP_ERR_INVALID, "a coordinate of a referenced vertex is not finite");

    float* d_face = nullptr;
    OP_TRY(s.alloc(&d_face, n));
    hipLaunchKernelGGL(k_mp_face, dim3(blocks_for(nt)), dim3(kThreads), 0, s.stream, d_xyz, d_triangles, nt, d_face);
    unsigned *d_index_sorted = nullptr, *d_first = nullptr, *d_last = nullptr;
    if (d_triangles) {
        unsigned *d_keys = nullptr, *d_keys_sorted = nullptr, *d_index = nullptr;
        OP_TRY(s.alloc(&d_keys, n));
        OP_TRY(s.alloc(&d_keys_sorted, n));
        OP_TRY(s.alloc(&d_index, n));
        OP_TRY(s.alloc(&d_index_sorted, n));
        OP_TRY(s.alloc(&d_first, nv));
        OP_TRY(s.alloc(&d_last, nv));
        const unsigned bits = (unsigned)std::max(1, bits_for((long long)nv));
        size_t sort_bytes = 0;
        OP_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, d_keys, d_keys_sorted, d_index, d_index_sorted, n, 0u, bits, s.stream));
        unsigned char* d_tmp = nullptr;
        OP_TRY(s.alloc(&d_tmp, sort_bytes));
        hipLaunchKernelGGL(k_mp_pairs, dim3(blocks_for(n)), dim3(kThreads), 0, s.stream, d_triangles, n, d_keys, d_index);
        OP_HIP(rocprim::radix_sort_pairs(d_tmp, sort_bytes, d_keys, d_keys_sorted, d_index, d_index_sorted, n, 0u, bits, s.stream));
        OP_HIP(hipMemsetAsync(d_first, 0, nv * sizeof(unsigned), s.stream));
        OP_HIP(hipMemsetAsync(d_last, 0, nv * sizeof(unsigned), s.stream));
        hipLaunchKernelGGL(k_mp_spans, dim3(blocks_for(n)), dim3(kThreads), 0, s.stream, d_keys_sorted, n, d_first, d_last);
    }
    const size_t per_block = kVertexThreads / 3;
    hipLaunchKernelGGL(k_mp_vertex, dim3((unsigned)((nv + per_block - 1) / per_block)), dim3(kVertexThreads), 0, s.stream, d_face, d_index_sorted, d_first, d_last, nv,
                       d_normals_out);
    OP_HIP(hipGetLastError());
    OP_HIP(hipStreamSynchronize(s.stream));
    return OP_OK;
}

// ---- Prune --------------------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void k_mp_init(size_t nv, unsigned* __restrict__ parent, unsigned* __restrict__ size, unsigned* __restrict__ referenced,
                                                      unsigned* __restrict__ first_kept) {
    const size_t v = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (v >= nv) return;
    parent[v] = (unsigned)v;
    size[v] = 0u;
    referenced[v] = 0u;
    first_kept[v] = kNone;
}

__device__ inline unsigned parent_of(const unsigned* parent, unsigned v) { return __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of v, halving the path on the way.  parent[x] <= x, so v strictly decreases every step: at most v steps, whatever the others do.
__device__ inline unsigned find_root(unsigned* parent, unsigned v) {
    for (;;) {
        const unsigned p = parent_of(parent, v);
        if (p == v) return v;
        const unsigned g = parent_of(parent, p);
        if (g != p) atomicMin(parent + v, g); // an ancestor below the parent: never raises parent[v], never touches a root
        v = g; // (g <= p < v)
    }
}

// Hooks the larger of the two roots under the smaller.  Each round exits or replaces the larger id by a strictly smaller one.
__device__ inline void unite(unsigned* parent, unsigned a, unsigned b) {
    for (;;) {
        a = find_root(parent, a);
        b = find_root(parent, b);
        if (a == b) return;
        if (a < b) { const unsigned t = a; a = b; b = t; }
        const unsigned old = atomicCAS(parent + a, a, b);
        if (old == a) return;
        a = old; // a had been hooked meanwhile, under old < a
    }
}

// (every index passed k_mp_check)
__global__ __launch_bounds__(kThreads) void k_mp_union(const unsigned* __restrict__ triangles, size_t nt, unsigned* parent, unsigned* __restrict__ referenced) {
    const size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= nt) return;
    const unsigned v0 = (unsigned)vertex_of(triangles, 3 * t), v1 = (unsigned)vertex_of(triangles, 3 * t + 1), v2 = (unsigned)vertex_of(triangles, 3 * t + 2);
    unite(parent, v0, v1);
    unite(parent, v0, v2);
    referenced[v0] = 1u; referenced[v1] = 1u; referenced[v2] = 1u;
}

// The unions are complete (the previous kernel has ended): the root is read, nothing is written to parent.
__global__ __launch_bounds__(kThreads) void k_mp_label(const unsigned* __restrict__ parent, const unsigned* __restrict__ referenced, size_t nv, unsigned* __restrict__ label,
                                                       unsigned* __restrict__ size) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= nv) return;
    unsigned v = (unsigned)i;
    for (unsigned p = parent[v]; p != v; p = parent[v]) v = p; // (p < v)
    label[i] = v;
    if (referenced[i]) atomicAdd(size + v, 1u);
}

__global__ __launch_bounds__(kThreads) void k_mp_keep(const unsigned* __restrict__ triangles, size_t nt, const unsigned* __restrict__ label, const unsigned* __restrict__ size,
                                                      unsigned long long min_points, unsigned* __restrict__ keep, unsigned* __restrict__ first_kept) {
    const size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= nt) return;
    const unsigned kept = (unsigned long long)size[label[vertex_of(triangles, 3 * t)]] > min_points ? 1u : 0u; // dropped when size <= min_points
    keep[t] = kept;
    if (kept) {
#pragma unroll
        for (int k = 0; k < 3; ++k) atomicMin(first_kept + vertex_of(triangles, 3 * t + k), (unsigned)(3 * t + k));
    }
}

__global__ __launch_bounds__(kThreads) void k_mp_pruned(const unsigned* __restrict__ label, const unsigned* __restrict__ size, const unsigned* __restrict__ referenced, size_t nv,
                                                        unsigned long long min_points, unsigned long long* __restrict__ pruned) {
    const size_t v = (size_t)blockIdx.x * kThreads + threadIdx.x;
    const bool mine = v < nv && referenced[v] && (unsigned long long)size[label[v]] <= min_points;
    const unsigned long long votes = __ballot(mine);
    if ((threadIdx.x & (op::kWave - 1)) == 0 && votes) atomicAdd(pruned, (unsigned long long)__popcll(votes));
}

__global__ __launch_bounds__(kThreads) void k_mp_first(const unsigned* __restrict__ triangles, size_t n, const unsigned* __restrict__ keep, const unsigned* __restrict__ first_kept,
                                                       unsigned* __restrict__ flag) {
    const size_t c = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (c < n) flag[c] = keep[c / 3] && first_kept[vertex_of(triangles, c)] == (unsigned)c ? 1u : 0u;
}

struct Rows { const float* src[3]; float* dst[3]; int arrays; }; // points, then colours and / or normals

__global__ __launch_bounds__(kThreads) void k_mp_gather(const unsigned* __restrict__ triangles, size_t n, const unsigned* __restrict__ keep, const unsigned* __restrict__ slot,
                                                        const unsigned* __restrict__ first_kept, const unsigned* __restrict__ flag, const unsigned* __restrict__ number, Rows rows,
                                                        unsigned* __restrict__ triangles_out) {
    const size_t c = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (c >= n || !keep[c / 3]) return;
    const size_t v = vertex_of(triangles, c);
    const size_t o = number[first_kept[v]]; // remap[v] of Compact
    triangles_out[3 * (size_t)slot[c / 3] + c % 3] = (unsigned)o;
    if (!flag[c]) return;
#pragma unroll
    for (int a = 0; a < 3; ++a)
        if (a < rows.arrays) {
#pragma unroll
            for (int k = 0; k < 3; ++k) rows.dst[a][3 * o + k] = rows.src[a][3 * v + k];
        }
}

// Prune + Compact on device arrays (d_colors / d_normals may be null; d_triangles null = a soup).  The outputs are DEVICE arrays with room for
// cap_vertices / cap_triangles rows and are written only when both counts fit; *nv_out, *nt_out and *pruned_out are set whenever the counts are known.
int prune_device(Scope& s, const float* d_xyz, const float* d_colors, const float* d_normals, size_t nv, const unsigned* d_triangles, size_t nt, size_t min_points,
                 float* d_xyz_out, float* d_colors_out, float* d_normals_out, size_t cap_vertices, unsigned* d_triangles_out, size_t cap_triangles, size_t* nv_out,
                 size_t* nt_out, size_t* pruned_out) {
    const size_t n = 3 * nt;
    unsigned* d_error = nullptr;
    unsigned long long* d_pruned = nullptr;
    OP_TRY(s.alloc(&d_error, (size_t)1));
    OP_TRY(s.alloc(&d_pruned, (size_t)1));
    OP_HIP(hipMemsetAsync(d_error, 0, sizeof(unsigned), s.stream));
    OP_HIP(hipMemsetAsync(d_pruned, 0, sizeof(unsigned long long), s.stream));
    if (d_triangles) {
        hipLaunchKernelGGL(k_mp_check, dim3(blocks_for(n)), dim3(kThreads), 0, s.stream, d_xyz, nv, d_triangles, n, 0, d_error);
        OP_HIP(hipGetLastError());
        unsigned error = 0u;
        OP_HIP(hipMemcpyAsync(&error, d_error, sizeof(unsigned), hipMemcpyDeviceToHost, s.stream));
        OP_HIP(hipStreamSynchronize(s.stream));
        if (error) return fail(OP_ERR_INVALID, "a triangle refers to a vertex beyond the %zu given", nv);
    }
    unsigned *d_parent = nullptr, *d_label = nullptr, *d_size = nullptr, *d_referenced = nullptr, *d_first_kept = nullptr, *d_keep = nullptr, *d_slot = nullptr, *d_flag = nullptr,
             *d_number = nullptr;
    OP_TRY(s.alloc(&d_parent, nv));
    OP_TRY(s.alloc(&d_label, nv));
    OP_TRY(s.alloc(&d_size, nv));
    OP_TRY(s.alloc(&d_referenced, nv));
    OP_TRY(s.alloc(&d_first_kept, nv));
    OP_TRY(s.alloc(&d_keep, nt));
    OP_TRY(s.alloc(&d_slot, nt));
    OP_TRY(s.alloc(&d_flag, n));
    OP_TRY(s.alloc(&d_number, n));
    size_t scan_bytes = 0, scan_bytes_nt = 0;
    OP_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, d_flag, d_number, 0u, n, rocprim::plus<unsigned>(), s.stream));
    OP_HIP(rocprim::exclusive_scan(nullptr, scan_bytes_nt, d_keep, d_slot, 0u, nt, rocprim::plus<unsigned>(), s.stream));
    unsigned char* d_tmp = nullptr;
    OP_TRY(s.alloc(&d_tmp, std::max(scan_bytes, scan_bytes_nt)));

    hipLaunchKernelGGL(k_mp_init, dim3(blocks_for(nv)), dim3(kThreads), 0, s.stream, nv, d_parent, d_size, d_referenced, d_first_kept);
    hipLaunchKernelGGL(k_mp_union, dim3(blocks_for(nt)), dim3(kThreads), 0, s.stream, d_triangles, nt, d_parent, d_referenced);
    hipLaunchKernelGGL(k_mp_label, dim3(blocks_for(nv)), dim3(kThreads), 0, s.stream, d_parent, d_referenced, nv, d_label, d_size);
    hipLaunchKernelGGL(k_mp_keep, dim3(blocks_for(nt)), dim3(kThreads), 0, s.stream, d_triangles, nt, d_label, d_size, (unsigned long long)min_points, d_keep, d_first_kept);
    hipLaunchKernelGGL(k_mp_pruned, dim3(blocks_for(nv)), dim3(kThreads), 0, s.stream, d_label, d_size, d_referenced, nv, (unsigned long long)min_points, d_pruned);
    hipLaunchKernelGGL(k_mp_first, dim3(blocks_for(n)), dim3(kThreads), 0, s.stream, d_triangles, n, d_keep, d_first_kept, d_flag);
    OP_HIP(rocprim::exclusive_scan(d_tmp, scan_bytes, d_flag, d_number, 0u, n, rocprim::plus<unsigned>(), s.stream));
    OP_HIP(rocprim::exclusive_scan(d_tmp, scan_bytes_nt, d_keep, d_slot, 0u, nt, rocprim::plus<unsigned>(), s.stream));
    OP_HIP(hipGetLastError());
    unsigned tail[4] = {0u, 0u, 0u, 0u}; // vertices = number of the last corner + its flag; triangles = slot of the last triangle + its keep
    unsigned long long pruned = 0;
    OP_HIP(hipMemcpyAsync(&tail[0], d_number + (n - 1), sizeof(unsigned), hipMemcpyDeviceToHost, s.stream));
    OP_HIP(hipMemcpyAsync(&tail[1], d_flag + (n - 1), sizeof(unsigned), hipMemcpyDeviceToHost, s.stream));
    OP_HIP(hipMemcpyAsync(&tail[2], d_slot + (nt - 1), sizeof(unsigned), hipMemcpyDeviceToHost, s.stream));
    OP_HIP(hipMemcpyAsync(&tail[3], d_keep + (nt - 1), sizeof(unsigned), hipMemcpyDeviceToHost, s.stream));
    OP_HIP(hipMemcpyAsync(&pruned, d_pruned, sizeof(pruned), hipMemcpyDeviceToHost, s.stream));
    OP_HIP(hipStreamSynchronize(s.stream));
    const size_t vertices = (size_t)tail[0] + tail[1], kept = (size_t)tail[2] + tail[3];
    if (vertices > std::min(nv, n) || kept > nt || pruned > nv) return fail(OP_ERR_HIP, "mesh pruning counted %zu vertices, %zu of %zu triangles", vertices, kept, nt);
    *nv_out = vertices;
    *nt_out = kept;
    *pruned_out = (size_t)pruned;
    if (vertices > cap_vertices || kept > cap_triangles)
        return fail(OP_ERR_CAPACITY, "the pruned mesh has %zu vertices and %zu triangles, the buffers hold %zu and %zu", vertices, kept, cap_vertices, cap_triangles);
    if (kept == 0) return OP_OK; // (then vertices == 0 as well)
    Rows rows = {{d_xyz, nullptr, nullptr}, {d_xyz_out, nullptr, nullptr}, 1};
    if (d_colors) { rows.src[rows.arrays] = d_colors; rows.dst[rows.arrays] = d_colors_out; ++rows.arrays; }
    if (d_normals) { rows.src[rows.arrays] = d_normals; rows.dst[rows.arrays] = d_normals_out; ++rows.arrays; }
    hipLaunchKernelGGL(k_mp_gather, dim3(blocks_for(n)), dim3(kThreads), 0, s.stream, d_triangles, n, d_keep, d_slot, d_first_kept, d_flag, d_number, rows, d_triangles_out);
    OP_HIP(hipGetLastError());
    OP_HIP(hipStreamSynchronize(s.stream));
    return OP_OK;
}

__global__ __launch_bounds__(kThreads) void k_mp_iota(size_t n, unsigned* __restrict__ out) {
    const size_t c = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (c < n) out[c] = (unsigned)c;
}

// The mesh as it stands between two stages of the fused tail: device arrays (triangles null = a soup)
struct Stage { const float* xyz; const float* colors; const unsigned* triangles; size_t nv, nt; };

int processed_device(Scope& s, Stage m, float grid_len, size_t min_points, float* points, float* colors, float* normals, size_t cap_vertices, uint32_t* triangles,
                     size_t cap_triangles, size_t* n_vertices, size_t* n_triangles) {
    if (grid_len > 0.0f && m.nt) {
        float *xyz = nullptr, *col = nullptr;
        unsigned* tri = nullptr;
        OP_TRY(s.alloc(&xyz, m.nv * 3));
        OP_TRY(s.alloc(&col, m.nv * 3));
        OP_TRY(s.alloc(&tri, m.nt * 3));
        size_t nv = 0, nt = 0;
        OP_TRY(cluster_device(s, m.xyz, m.colors, nullptr, m.nv, m.triangles, m.nt, grid_len, OP_MEM_DEVICE, xyz, col, nullptr, m.nv, tri, m.nt, &nv, &nt));
        m = Stage{xyz, col, tri, nv, nt};
    }
    if (min_points > 0 && m.nt) {
        float *xyz = nullptr, *col = nullptr;
        unsigned* tri = nullptr;
        OP_TRY(s.alloc(&xyz, m.nv * 3));
        OP_TRY(s.alloc(&col, m.nv * 3));
        OP_TRY(s.alloc(&tri, m.nt * 3));
        size_t nv = 0, nt = 0, pruned = 0;
        OP_TRY(prune_device(s, m.xyz, m.colors, nullptr, m.nv, m.triangles, m.nt, min_points, xyz, col, nullptr, m.nv, tri, m.nt, &nv, &nt, &pruned));
        m = Stage{xyz, col, tri, nv, nt};
    }
    if (m.nt == 0) m.nv = 0; // (both stages leave no vertex without a triangle)
    *n_vertices = m.nv;
    *n_triangles = m.nt;
    if (m.nv > cap_vertices || m.nt > cap_triangles)
        return fail(OP_ERR_CAPACITY, "the processed mesh has %zu vertices and %zu triangles, the buffers hold %zu and %zu", m.nv, m.nt, cap_vertices, cap_triangles);
    if (m.nt == 0) return OP_OK;
    float* d_normals = nullptr;
    if (normals) {
        OP_TRY(s.alloc(&d_normals, m.nv * 3));
        OP_TRY(normals_device(s, m.xyz, m.nv, m.triangles, m.nt, d_normals));
    }
    if (!m.triangles) {
        unsigned* tri = nullptr;
        OP_TRY(s.alloc(&tri, m.nt * 3));
        hipLaunchKernelGGL(k_mp_iota, dim3(blocks_for(m.nt * 3)), dim3(kThreads), 0, s.stream, m.nt * 3, tri);
        OP_HIP(hipGetLastError());
        m.triangles = tri;
    }
    OP_HIP(hipMemcpyAsync(points, m.xyz, m.nv * 3 * sizeof(float), hipMemcpyDeviceToHost, s.stream));
    OP_HIP(hipMemcpyAsync(colors, m.colors, m.nv * 3 * sizeof(float), hipMemcpyDeviceToHost, s.stream));
    if (normals) OP_HIP(hipMemcpyAsync(normals, d_normals, m.nv * 3 * sizeof(float), hipMemcpyDeviceToHost, s.stream));
    OP_HIP(hipMemcpyAsync(triangles, m.triangles, m.nt * 3 * sizeof(unsigned), hipMemcpyDeviceToHost, s.stream));
    OP_HIP(hipStreamSynchronize(s.stream));
    return OP_OK;
}

int check_corners(size_t nv, size_t nt) {
    if (nt > 0xffffffffull / 3) return fail(OP_ERR_CAPACITY, "%zu triangles: their corners are beyond 32-bit corner indices", nt);
    if (nt && nv == 0) return fail(OP_ERR_INVALID, "a triangle refers to a vertex beyond the 0 given");
    return OP_OK;
}

} // namespace

extern "C" {

int op_mesh_compute_normals(const float* points, size_t nv, const uint32_t* triangles, size_t nt, int mem, int device, float* normals_out) {
    if ((nv && (!points || !normals_out)) || (nt && !triangles)) return fail(OP_ERR_INVALID, "null argument");
    OP_TRY(check_mem(mem));
    OP_TRY(check_corners(nv, nt));
    Scope s;
    OP_TRY(s.open(device));
    if (nv == 0) return OP_OK;
    const float* d_xyz = nullptr;
    const uint32_t* d_triangles = nullptr;
    OP_TRY(s.input(points, nv * 3, mem, &d_xyz));
    if (nt) OP_TRY(s.input(triangles, nt * 3, mem, &d_triangles));
    float* d_normals = normals_out; // (nothing is written before the checks have passed)
    if (mem == OP_MEM_HOST) OP_TRY(s.alloc(&d_normals, nv * 3));
    OP_TRY(normals_device(s, d_xyz, nv, d_triangles, nt, d_normals));
    if (mem == OP_MEM_HOST) OP_TRY(s.output(normals_out, (const float*)d_normals, nv * 3, mem));
    return OP_OK;
}

int op_mesh_prune(const float* points, const float* colors, const float* normals, size_t nv, const uint32_t* triangles, size_t nt, size_t min_points, int mem, int device,
                  float* points_out, float* colors_out, float* normals_out, uint32_t* triangles_out, size_t* nv_out, size_t* nt_out, size_t* pruned_out) {
    if (!nv_out || !nt_out || !pruned_out || (nt && (!points || !triangles || !points_out || !triangles_out || (colors && !colors_out) || (normals && !normals_out))))
        return fail(OP_ERR_INVALID, "null argument");
    OP_TRY(check_mem(mem));
    OP_TRY(check_corners(nv, nt));
    Scope s;
    OP_TRY(s.open(device));
    *nv_out = 0;
    *nt_out = 0;
    *pruned_out = 0;
    if (nt == 0) return OP_OK;
    const float *d_xyz = nullptr, *d_colors = nullptr, *d_normals = nullptr;
    const uint32_t* d_triangles = nullptr;
    OP_TRY(s.input(points, nv * 3, mem, &d_xyz));
    if (colors) OP_TRY(s.input(colors, nv * 3, mem, &d_colors));
    if (normals) OP_TRY(s.input(normals, nv * 3, mem, &d_normals));
    OP_TRY(s.input(triangles, nt * 3, mem, &d_triangles));
    const size_t cap = std::min(nv, 3 * nt);
    float *d_out[3] = {points_out, colors_out, normals_out}, *host_out[3] = {points_out, colors_out, normals_out};
    const bool given[3] = {true, colors != nullptr, normals != nullptr};
    unsigned* d_triangles_out = triangles_out;
    if (mem == OP_MEM_HOST) {
        for (int a = 0; a < 3; ++a)
            if (given[a]) OP_TRY(s.alloc(&d_out[a], cap * 3));
        OP_TRY(s.alloc(&d_triangles_out, nt * 3));
    }
    const int rc = prune_device(s, d_xyz, d_colors, d_normals, nv, d_triangles, nt, min_points, d_out[0], d_out[1], d_out[2], cap, d_triangles_out, nt, nv_out, nt_out, pruned_out);
    if (rc != OP_OK) { *nv_out = 0; *nt_out = 0; *pruned_out = 0; return rc; }
    if (mem == OP_MEM_HOST && *nt_out) {
        for (int a = 0; a < 3; ++a)
            if (given[a]) OP_HIP(hipMemcpyAsync(host_out[a], d_out[a], *nv_out * 3 * sizeof(float), hipMemcpyDeviceToHost, s.stream));
        OP_HIP(hipMemcpyAsync(triangles_out, d_triangles_out, *nt_out * 3 * sizeof(unsigned), hipMemcpyDeviceToHost, s.stream));
        OP_HIP(hipStreamSynchronize(s.stream));
    }
    return OP_OK;
}

int op_volume_extract_mesh_processed(op_volume* v, const int32_t* tri_table, const int32_t* edge_pairs, const int32_t* only_block, float grid_len, size_t min_points,
                                     float* points, float* colors, float* normals, size_t cap_vertices, uint32_t* triangles, size_t cap_triangles, size_t* n_vertices,
                                     size_t* n_triangles) {
    if (!n_vertices || !n_triangles) return fail(OP_ERR_INVALID, "null argument");
    if (!(grid_len >= 0.0f) || !std::isfinite(grid_len)) return fail(OP_ERR_INVALID, "grid_len must be 0 (no clustering) or positive and finite (got %g)", (double)grid_len);
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
            rc = processed_device(s, Stage{d_pts, d_col, nullptr, soup, soup / 3}, grid_len, min_points, points, colors, normals, cap_vertices, triangles, cap_triangles,
                                  n_vertices, n_triangles);
        if (rc != OP_OK && rc != OP_ERR_CAPACITY) { *n_vertices = 0; *n_triangles = 0; } // (too small: the counts say what is needed)
    }
    return rc;
}

} // extern "C"
