// MeshSimplify.cpp -- the tail of the reference's fusion drivers (example/DenseFusion/DenseFusion.cpp:104-105, ImageSequenceIntegration.cpp:53-56):
// cube_handler.ExtractTriangleMesh(mesh), then mesh.ClusteringSimplify(grid) -- stage by stage, so that every stage can be timed and the result written out.
//
//   MeshSimplify --mesh points.f32 --triangles tri.u32 [--colors colors.f32] [--normals normals.f32] [--grid 0.05] [--path host|device] [--dump DIR]
//   MeshSimplify [--frames 3] [--res 0.02] [--grid L] [--path host|device|fused] [--warmup 1] [--dump DIR]
//
//   --mesh         one mesh (raw little-endian nv x 3 float32 arrays, nt x 3 uint32 indices) through TriangleMesh::ClusteringSimplify(--grid);
//                  with --path host no device is touched
//   the frames     views of the analytic room of SubmapModel.cpp (a box with two spheres) fused into a volume of --res voxels; --grid defaults to --res
//   --path host    OP_RUNTIME_OPT_MESH_CLUSTERING 0: ExtractTriangleMesh, then ClusteringSimplify as the host loop
//   --path device  the option at 1: the same two calls, ClusteringSimplify forwards to op_mesh_cluster_simplify (the soup comes down and goes up again)
//   --path fused   CubeHandler::ExtractSimplifiedTriangleMesh: one call, only the simplified mesh leaves the device
//   --warmup N     untimed extract + simplify passes before the timed one (first launches load code objects, first buffers are allocated)
//   --dump DIR     mesh_points.f32, mesh_colors.f32, mesh_normals.f32, mesh_triangles.u32 and result.json with the sizes and the time of every stage;
//                  with the frames also soup_points.f32 / soup_colors.f32, the triangle soup of this process's volume (three vertices per triangle)
// The last line printed is that JSON.  ms.extract is the whole ExtractTriangleMesh call -- count and emit kernels, the soup's download and its unpacking
// into the mesh, which the class surface does not time apart: ms.download is null on these paths and 0 on the fused one, where extract is the one call.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "Geometry/Geometry.h"
#include "Geometry/TriangleMesh.h"
#include "Integration/CubeHandler.h"
#include "onepiece_hip.h"
#include "src/Bridge.h" // the class surface's own device choice and conversions
using namespace one_piece;

namespace {

double Now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

template <class List>
bool WriteRaw(const std::string& dir, const std::string& name, const List& p) {
    std::ofstream os((dir + "/" + name).c_str(), std::ios::binary);
    if (!p.empty()) os.write(reinterpret_cast<const char*>(p[0].data()), static_cast<std::streamsize>(p.size() * 12));
    return static_cast<bool>(os);
}
template <class List, class Row>
bool ReadRaw(const std::string& file, List& out, const Row& zero) {
    std::ifstream is(file.c_str(), std::ios::binary | std::ios::ate);
    if (!is) return false;
    const std::streamsize bytes = is.tellg();
    if (bytes < 0 || bytes % 12 != 0) return false;
    out.assign(static_cast<size_t>(bytes / 12), zero);
    is.seekg(0);
    return bytes == 0 || static_cast<bool>(is.read(reinterpret_cast<char*>(out[0].data()), bytes));
}
bool DumpMesh(const std::string& dir, const geometry::TriangleMesh& m) {
    return WriteRaw(dir, "mesh_points.f32", m.points) && WriteRaw(dir, "mesh_colors.f32", m.colors) && WriteRaw(dir, "mesh_normals.f32", m.normals) &&
           WriteRaw(dir, "mesh_triangles.u32", m.triangles);
}

// camera-to-world pose on a circle of radius 0.5 m at angle th, looking outward, slightly pitched (SubmapModel.cpp)
geometry::TransformationMatrix ViewPose(float th, float pitch) {
    const float cy = std::cos(th), sy = std::sin(th), cp = std::cos(pitch), sp = std::sin(pitch);
    geometry::TransformationMatrix T = geometry::TransformationMatrix::Identity();
    const float Ry[9] = {cy, 0, sy, 0, 1, 0, -sy, 0, cy}, Rx[9] = {1, 0, 0, 0, cp, -sp, 0, sp, cp};
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) T(r, c) = Ry[3 * r] * Rx[c] + Ry[3 * r + 1] * Rx[3 + c] + Ry[3 * r + 2] * Rx[6 + c];
    T(0, 3) = 0.5f * sy; T(1, 3) = 0.05f; T(2, 3) = 0.5f * cy;
    return T;
}
// z-depth and colour of that room seen from `pose`: a 5.2 x 2.8 x 5.2 m box around the origin with two spheres in it (SubmapModel.cpp)
void RenderRoom(const geometry::TransformationMatrix& P, const camera::PinholeCamera& cam, cv::Mat& depth, cv::Mat& rgb) {
    const int W = cam.GetWidth(), H = cam.GetHeight();
    depth.create(H, W, CV_32FC1);
    rgb.create(H, W, CV_8UC3);
    const float half[3] = {2.6f, 1.4f, 2.6f}, spheres[2][4] = {{1.2f, 0.7f, 1.6f, 0.55f}, {-1.4f, 0.5f, -1.1f, 0.7f}};
    for (int v = 0; v < H; ++v)
        for (int u = 0; u < W; ++u) {
            const float c[3] = {(u - cam.GetCx()) / cam.GetFx(), (v - cam.GetCy()) / cam.GetFy(), 1.0f};
            float d[3], o[3], t = 1e9f;
            for (int r = 0; r < 3; ++r) { d[r] = P(r, 0) * c[0] + P(r, 1) * c[1] + P(r, 2) * c[2]; o[r] = P(r, 3); }
            for (int r = 0; r < 3; ++r)
                if (std::fabs(d[r]) > 1e-9f) t = std::min(t, ((d[r] > 0 ? half[r] : -half[r]) - o[r]) / d[r]);
            const float dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
            for (int s = 0; s < 2; ++s) {
                const float l[3] = {o[0] - spheres[s][0], o[1] - spheres[s][1], o[2] - spheres[s][2]};
                const float b = d[0] * l[0] + d[1] * l[1] + d[2] * l[2], cc = l[0] * l[0] + l[1] * l[1] + l[2] * l[2] - spheres[s][3] * spheres[s][3];
                const float disc = b * b - dd * cc;
                if (disc > 0) { const float ts = (-b - std::sqrt(disc)) / dd; if (ts > 0.05f && ts < t) t = ts; }
            }
            depth.at<float>(v, u) = t;
            cv::Vec3b& px = rgb.at<cv::Vec3b>(v, u);
            for (int r = 0; r < 3; ++r) px[r] = static_cast<unsigned char>(128.0f + 100.0f * std::sin(2.5f * (o[r] + t * d[r]) + 0.7f * r));
        }
}

struct Times { double extract = 0, simplify = 0; };

void Emit(const std::string& dump, const std::string& js) {
    std::cout << js << std::endl;
    if (!dump.empty()) { std::ofstream os((dump + "/result.json").c_str()); os << js << std::endl; }
}

} // namespace

int main(int argc, char** argv) {
    int n_frames = 3, warmup = 1;
    float grid = -1.0f, res = 0.02f;
    std::string dump, path = "host", mesh_file, triangles_file, colors_file, normals_file;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--frames" && i + 1 < argc) n_frames = std::atoi(argv[++i]);
        else if (a == "--warmup" && i + 1 < argc) warmup = std::atoi(argv[++i]);
        else if (a == "--path" && i + 1 < argc) path = argv[++i];
        else if (a == "--dump" && i + 1 < argc) dump = argv[++i];
        else if (a == "--mesh" && i + 1 < argc) mesh_file = argv[++i];
        else if (a == "--triangles" && i + 1 < argc) triangles_file = argv[++i];
        else if (a == "--colors" && i + 1 < argc) colors_file = argv[++i];
        else if (a == "--normals" && i + 1 < argc) normals_file = argv[++i];
        else if (a == "--grid" && i + 1 < argc) grid = static_cast<float>(std::atof(argv[++i]));
        else if (a == "--res" && i + 1 < argc) res = static_cast<float>(std::atof(argv[++i]));
        else { std::cout << "unknown argument " << a << std::endl; return 2; }
    }
    const bool fused = path == "fused";
    if (n_frames < 1 || warmup < 0 || !(res > 0) || (path != "host" && path != "device" && !fused) || (fused && !mesh_file.empty()) || (mesh_file.empty() != triangles_file.empty())) {
        std::cout << "Usage: MeshSimplify --mesh points.f32 --triangles tri.u32 [--colors colors.f32] [--normals normals.f32] [--grid L] [--path host|device] [--dump DIR]\n"
                     "       MeshSimplify [--frames N] [--res R] [--grid L] [--path host|device|fused] [--warmup N] [--dump DIR]" << std::endl;
        return 2;
    }
    if (op_runtime_set_option(OP_RUNTIME_OPT_MESH_CLUSTERING, path == "host" ? 0 : 1) != OP_OK) { std::cout << op_last_error() << std::endl; return 3; }

    if (!mesh_file.empty()) {
        if (grid < 0) grid = 0.05f;
        geometry::TriangleMesh in;
        const geometry::Point3 zero(0, 0, 0);
        if (!ReadRaw(mesh_file, in.points, zero) || !ReadRaw(triangles_file, in.triangles, geometry::Point3ui(0, 0, 0)) || (!colors_file.empty() && !ReadRaw(colors_file, in.colors, zero)) ||
            (!normals_file.empty() && !ReadRaw(normals_file, in.normals, zero))) {
            std::cout << "cannot read the mesh" << std::endl;
            return 3;
        }
        double t = Now();
        const geometry::TriangleMesh out = *in.ClusteringSimplify(grid);
        t = Now() - t;
        if (!dump.empty() && !DumpMesh(dump, out)) { std::cout << "cannot write to " << dump << std::endl; return 3; }
        std::ostringstream js;
        js << "{\"path\": \"" << path << "\", \"grid\": " << grid << ", \"points\": " << in.GetPointSize() << ", \"triangles\": " << in.GetTriangleSize() << ", \"points_out\": "
           << out.GetPointSize() << ", \"triangles_out\": " << out.GetTriangleSize() << ", \"ms\": {\"simplify\": " << t << "}}";
        Emit(dump, js.str());
        return 0;
    }

    if (grid < 0) grid = res;
    camera::PinholeCamera cam(514.817f, 515.375f, 318.771f, 238.447f, 640, 480, 1.0f); // depth scale 1: the rendered depth is metres in float
    integration::CubeHandler cube_handler(cam);
    cube_handler.SetVoxelResolution(res);
    for (int i = 0; i < n_frames; ++i) { // every third frame of a slow pan: 0.03 rad between the views that are used
        const geometry::TransformationMatrix pose = ViewPose(0.40f + 0.03f * i, -0.04f + 0.005f * i);
        cv::Mat depth, rgb;
        RenderRoom(pose, cam, depth, rgb);
        cube_handler.IntegrateImage(depth, rgb, pose);
    }
    cube_handler.Synchronize();

    geometry::TriangleMesh soup, mesh;
    Times ms;
    size_t soup_triangles = 0;
    for (int pass = 0; pass <= warmup; ++pass) {
        ms = Times();
        double t = Now();
        if (fused) {
            cube_handler.ExtractSimplifiedTriangleMesh(mesh, grid);
            ms.extract = Now() - t;
        } else {
            cube_handler.ExtractTriangleMesh(soup);                  // DenseFusion.cpp:104
            ms.extract = Now() - t; t = Now();
            mesh = *soup.ClusteringSimplify(grid);                   // :105
            ms.simplify = Now() - t;
            soup_triangles = soup.GetTriangleSize();
        }
    }
    if (!dump.empty()) {
        // the soup this process simplified goes out too: blocks are meshed in pool order, and the order in which a frame's blocks enter the pool is not
        // the same from one process to the next, so two runs agree on the soup as a set of triangles, not as a sequence -- and the simplified mesh
        // (cells and vertices by first appearance, sums in corner order) follows the sequence.  On the fused path the soup is extracted here, untimed.
        if (fused) cube_handler.ExtractTriangleMesh(soup);
        if (!DumpMesh(dump, mesh) || !WriteRaw(dump, "soup_points.f32", soup.points) || !WriteRaw(dump, "soup_colors.f32", soup.colors)) {
            std::cout << "cannot write to " << dump << std::endl;
            return 3;
        }
        if (fused) soup_triangles = soup.GetTriangleSize();
    }
    std::ostringstream js;
    js << "{\"path\": \"" << path << "\", \"frames\": " << n_frames << ", \"res\": " << res << ", \"grid\": " << grid << ", \"warmup\": " << warmup << ", \"blocks\": " << cube_handler.GetCubeCount()
       << ", \"soup_triangles\": " << soup_triangles << ", \"points_out\": " << mesh.GetPointSize() << ", \"triangles_out\": " << mesh.GetTriangleSize() << ", \"ms\": {\"extract\": " << ms.extract
       << ", \"download\": " << (fused ? "0" : "null") << ", \"simplify\": " << ms.simplify << ", \"total\": " << ms.extract + ms.simplify << "}}";
    Emit(dump, js.str());
    return 0;
}
