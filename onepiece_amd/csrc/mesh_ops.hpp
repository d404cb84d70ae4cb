// mesh_ops.hpp -- what mesh_cluster.hip lends mesh_post.hip: the clustering simplification on device arrays, so that the fused tail
// (extract -> cluster -> prune -> normals) can run it between two stages that never leave the device.
#pragma once
#include <cstddef>

#include "common.hpp"

namespace op {
namespace mesh {

// mesh_cluster.hip: TriangleMesh::ClusteringSimplify + Compact on device arrays (d_colors / d_normals may be null; d_triangles null = a soup,
// triangle t = vertices 3t .. 3t + 2).  The outputs follow `mem` and are written only when both counts fit their capacities.
int cluster_device(Scope& s, const float* d_xyz, const float* d_colors, const float* d_normals, size_t nv, const unsigned* d_triangles, size_t nt, float grid_len, int mem,
                   float* xyz_out, float* colors_out, float* normals_out, size_t cap_vertices, unsigned* triangles_out, size_t cap_triangles, size_t* nv_out, size_t* nt_out);

} // namespace mesh
} // namespace op
