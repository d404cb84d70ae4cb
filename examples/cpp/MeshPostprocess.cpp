// MeshPostprocess.cpp -- the whole tail of the reference's fusion drivers (example/MergeMultipleSubmaps.cpp:45-46, ImageIntegration.cpp:45, PruneMesh.cpp:15):
// cube_handler.ExtractTriangleMesh(mesh), then mesh.ClusteringSimplify(grid), mesh.Prune(min_points), mesh.ComputeNormals() -- stage by stage, so that every
// stage can be timed and the result written out.
//
//   MeshPostprocess --mesh points.f32 --triangles tri.u32 [--colors colors.f32] [--normals normals.f32] [--op normals|prune|both] [--min-points N] [--path host|device] [--dump DIR]
//   MeshPostprocess [--frames 3] [--res 0.02] [--grid G] [--min-points N] [--normals] [--path host|device|fused] [--warmup 1] [--dump DIR]
//
//   --mesh         one mesh (raw little-endian nv x 3 float32 arrays, nt x 3 uint32 indices) through TriangleMesh::Prune(--min-points) and / or
//                  TriangleMesh::ComputeNormals (both: Prune first); with --path host no device is touched.  (Here --normals names the file of the input normals.)
//   the frames     views of the analytic room of SubmapModel.cpp fused into a volume of --res voxels; --grid 0 (the default): no clustering; --min-points 0
//                  (the default): no pruning; --normals: ComputeNormals at the end
//   --path host    OP_RUNTIME_OPT_MESH_CLUSTERING and OP_RUNTIME_OPT_MESH_POSTPROCESS 0: ExtractTriangleMesh, then the host loops
//   --path device  both options at 1: the same calls, each forwards to its device entry (the mesh comes down and goes up again between them)
//   --path fused   CubeHandler::ExtractProcessedTriangleMesh: one call, only the finished mesh leaves the device
//   --warmup N     untimed passes before the timed one
//   --dump DIR     mesh_points.f32, mesh_colors.f32, mesh_normals.f32, mesh_triangles.u32 and result.json; with the frames also soup_points.f32 /
//                  soup_colors.f32, the triangle soup of this process's volume (pool order differs between processes: DESIGN.md section 0)
// The last line printed is that JSON: ms.extract, simplify, prune, normals, total; the sizes; pruned = the referenced vertices Prune dropped (null on the
// fused path, which does not report it).  On the fused path ms.extract is the one call and the other stages are 0.
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


// the vertices some triangle refers to
size_t Referenced(const geometry::TriangleMesh& m) {
    std::vector<char> seen(m.points.size(), 0);
    size_t n = 0;
    for (size_t t = 0; t < m.triangles.size(); ++t)
        for (int k = 0; k < 3; ++k) {
            const unsigned v = m.triangles[t](k);
            if (v < seen.size() && !seen[v]) { seen[v] = 1; ++n; }
        }
    return n;
}

struct Times { double extract = 0, simplify = 0, prune = 0, normals = 0; };

void Emit(const std::string& dump, const std::string& js) {
    std::cout << js << std::endl;
    if (!dump.empty()) { std::ofstream os((dump + "/result.json").c_str()); os << js << std::endl; }
}

std::string Stages(const Times& ms) {
    std::ostringstream js;
    js << "\"ms\": {\"extract\": " << ms.extract << ", \"simplify\": " << ms.simplify << ", \"prune\": " << ms.prune << ", \"normals\": " << ms.normals << ", \"total\": "
       << ms.extract + ms.simplify + ms.prune + ms.normals << "}";
    return js.str();
}

} // namespace

int main(int argc, char** argv) {
    int n_frames = 3, warmup = 1;
    float grid = 0.0f, res = 0.02f;
    long long min_points = 0;
    bool normals_flag = false;
    std::string dump, path = "host", op = "both", mesh_file, triangles_file, colors_file, normals_file;
    for (int i = 1; i < argc; ++i) mesh_file = std::string(argv[i]) == "--mesh" && i + 1 < argc ? argv[i + 1] : mesh_file;
    const bool mesh_mode = !mesh_file.empty();
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--frames" && i + 1 < argc) n_frames = std::atoi(argv[++i]);
        else if (a == "--warmup" && i + 1 < argc) warmup = std::atoi(argv[++i]);
        else if (a == "--path" && i + 1 < argc) path = argv[++i];
        else if (a == "--op" && i + 1 < argc) op = argv[++i];
        else if (a == "--dump" && i + 1 < argc) dump = argv[++i];
        else if (a == "--mesh" && i + 1 < argc) ++i;
        else if (a == "--triangles" && i + 1 < argc) triangles_file = argv[++i];
        else if (a == "--colors" && i + 1 < argc) colors_file = argv[++i];
        else if (a == "--normals" && mesh_mode && i + 1 < argc) normals_file = argv[++i];
        else if (a == "--normals" && !mesh_mode) normals_flag = true;
        else if (a == "--min-points" && i + 1 < argc) min_points = std::atoll(argv[++i]);
        else if (a == "--grid" && i + 1 < argc) grid = static_cast<float>(std::atof(argv[++i]));
        else if (a == "--res" && i + 1 < argc) res = static_cast<float>(std::atof(argv[++i]));
        else { std::cout << "unknown argument " << a << std::endl; return 2; }
    }
    const bool fused = path == "fused";
    if (n_frames < 1 || warmup < 0 || !(res > 0) || !(grid >= 0) || min_points < 0 || (path != "host" && path != "device" && !fused) || (fused && mesh_mode) ||
        (mesh_mode && triangles_file.empty()) || (op != "normals" && op != "prune" && op != "both")) {
        std::cout << "Usage: MeshPostprocess --mesh points.f32 --triangles tri.u32 [--colors colors.f32] [--normals normals.f32] [--op normals|prune|both] [--min-points N] [--path host|device] [--dump DIR]\n"
                     "       MeshPostprocess [--frames N] [--res R] [--grid G] [--min-points N] [--normals] [--path host|device|fused] [--warmup N] [--dump DIR]" << std::endl;
        return 2;
    }
    const long long on = path == "host" ? 0 : 1;
    if (op_runtime_set_option(OP_RUNTIME_OPT_MESH_CLUSTERING, on) != OP_OK || op_runtime_set_option(OP_RUNTIME_OPT_MESH_POSTPROCESS, on) != OP_OK) {
        std::cout << op_last_error() << std::endl;
        return 3;
    }
    const size_t min_pts = static_cast<size_t>(min_points);

    if (mesh_mode) {
        geometry::TriangleMesh mesh;
        const geometry::Point3 zero(0, 0, 0);
        if (!ReadRaw(mesh_file, mesh.points, zero) || !ReadRaw(triangles_file, mesh.triangles, geometry::Point3ui(0, 0, 0)) ||
            (!colors_file.empty() && !ReadRaw(colors_file, mesh.colors, zero)) || (!normals_file.empty() && !ReadRaw(normals_file, mesh.normals, zero))) {
            std::cout << "cannot read the mesh" << std::endl;
            return 3;
        }
        const size_t points_in = mesh.GetPointSize(), triangles_in = mesh.GetTriangleSize(), referenced = Referenced(mesh);
        Times ms;
        bool pruned_known = false;
        size_t pruned = 0;
        if (op != "normals") {
            const double t = Now();
            mesh = *mesh.Prune(min_pts);
            ms.prune = Now() - t;
            pruned = referenced - mesh.GetPointSize(); // (Compact leaves the referenced vertices of the kept components)
            pruned_known = true;
        }
        if (op != "prune") {
            const double t = Now();
            mesh.ComputeNormals();
            ms.normals = Now() - t;
        }
        if (!dump.empty() && !DumpMesh(dump, mesh)) { std::cout << "cannot write to " << dump << std::endl; return 3; }
        std::ostringstream js;
        js << "{\"path\": \"" << path << "\", \"op\": \"" << op << "\", \"min_points\": " << min_points << ", \"points\": " << points_in << ", \"triangles\": " << triangles_in
           << ", \"points_out\": " << mesh.GetPointSize() << ", \"triangles_out\": " << mesh.GetTriangleSize() << ", \"pruned\": ";
        if (pruned_known) js << pruned; else js << "null";
        js << ", " << Stages(ms) << "}";
        Emit(dump, js.str());
        return 0;
    }

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
    size_t soup_triangles = 0, pruned = 0;
    bool pruned_known = false;
    for (int pass = 0; pass <= warmup; ++pass) {
        ms = Times();
        double t = Now();
        if (fused) {
            cube_handler.ExtractProcessedTriangleMesh(mesh, grid, min_pts, normals_flag);
            ms.extract = Now() - t;
        } else {
            cube_handler.ExtractTriangleMesh(soup);                            // MergeMultipleSubmaps.cpp:44
            ms.extract = Now() - t;
            soup_triangles = soup.GetTriangleSize();
            mesh = soup;
            if (grid > 0) { t = Now(); mesh = *mesh.ClusteringSimplify(grid); ms.simplify = Now() - t; } // :45
            if (min_pts > 0) {
                const size_t before = Referenced(mesh);
                t = Now(); mesh = *mesh.Prune(min_pts); ms.prune = Now() - t;  // PruneMesh.cpp:15
                pruned = before - mesh.GetPointSize();
                pruned_known = true;
            }
            if (normals_flag) { t = Now(); mesh.ComputeNormals(); ms.normals = Now() - t; } // :46
        }
    }
    if (!dump.empty()) {
        // the soup this process worked on goes out too (see MeshSimplify.cpp): on the fused path it is extracted here, untimed
        if (fused) { cube_handler.ExtractTriangleMesh(soup); soup_triangles = soup.GetTriangleSize(); }
        if (!DumpMesh(dump, mesh) || !WriteRaw(dump, "soup_points.f32", soup.points) || !WriteRaw(dump, "soup_colors.f32", soup.colors)) {
            std::cout << "cannot write to " << dump << std::endl;
            return 3;
        }
    }
    std::ostringstream js;
    js << "{\"path\": \"" << path << "\", \"frames\": " << n_frames << ", \"res\": " << res << ", \"grid\": " << grid << ", \"min_points\": " << min_points << ", \"normals\": "
       << (normals_flag ? "true" : "false") << ", \"warmup\": " << warmup << ", \"blocks\": " << cube_handler.GetCubeCount() << ", \"soup_triangles\": " << soup_triangles
       << ", \"points_out\": " << mesh.GetPointSize() << ", \"triangles_out\": " << mesh.GetTriangleSize() << ", \"pruned\": ";
    if (pruned_known) js << pruned; else js << "null";
    js << ", " << Stages(ms) << "}";
    Emit(dump, js.str());
    return 0;
}
