// ScannetIntegration.cpp -- the flow of the reference's example/GenerateModelFromScannet.cpp written against THIS repository's class surface: read a
// ScanNet-layout directory (_info.txt, frame-%06d.color.* / .depth.png / .pose.txt: two cameras), align the colour image to the depth pixels, fuse
// every 10th frame with SetFarPlane(3) and SetTruncation(0.15), then the mesh tail.  Three paths for the alignment:
//   --path host     tool::AlignColorToDepth's host loop, then IntegrateImage                       (what the class surface did before the device path)
//   --path device   the same two calls with OP_RUNTIME_OPT_COLOR_ALIGNMENT = 1 (op_align_color_to_depth: the aligned image returns to the host)
//   --path fused    the IntegrateImage overload that takes the colour camera (op_volume_integrate_unaligned: the aligned image stays on the device)
// The reference also bilateral-filters the depth it fuses (not the one it aligns with); that filter is left out here so that the three paths fuse
// the same images.  cv::imread of this repository reads PNG only: the reader returns the reference's .color.jpg names, and --color-ext png swaps
// the extension.
//
//   ScannetIntegration <dir> [--voxel 0.02] [--stride 10] [--frames N] [--path host|device|fused] [--color-ext png] [--ply out.ply] [--dump DIR]
//   ScannetIntegration --align DIR [--path host|device]      one image pair from DIR/params.txt, color.u8, depth.f32 | depth.u16 -> DIR/aligned.u8
//     params.txt: colour camera (fx fy cx cy width height), depth camera (fx fy cx cy width height depth_scale), colour rows, colour cols,
//                 1 for uint16 depth, the 16 entries of color_to_depth
//   ScannetIntegration --list DIR                             what tool::ReadImageSequenceFromScannetWithPose returns for DIR, as one JSON line (no device)
//   --dump DIR      volume_keys.i32 (n x 3, sorted), volume_voxels.f32 (n x 512 x {sdf, weight, c0, c1, c2}) and result.json
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>

#include "Geometry/Geometry.h"
#include "Integration/CubeHandler.h"
#include "Tool/IO.h"
#include "Tool/ImageProcessing.h"
#include "onepiece_hip.h"
using namespace one_piece;

namespace {

double Seconds(const std::chrono::steady_clock::time_point& t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

bool ReadAll(const std::string& file, void* dst, size_t bytes) {
    std::ifstream is(file.c_str(), std::ios::binary);
    is.read(static_cast<char*>(dst), static_cast<std::streamsize>(bytes));
    return static_cast<size_t>(is.gcount()) == bytes;
}

int AlignOne(const std::string& dir, const std::string& path) {
    std::ifstream ps((dir + "/params.txt").c_str());
    double c[6], d[7], m[16];
    int rows = 0, cols = 0, u16 = 0;
    for (double& x : c) ps >> x;
    for (double& x : d) ps >> x;
    ps >> rows >> cols >> u16;
    for (double& x : m) ps >> x;
    if (!ps) { std::cout << "cannot read " << dir << "/params.txt" << std::endl; return 1; }
    camera::PinholeCamera color_camera, depth_camera;
    color_camera.SetPara(static_cast<float>(c[0]), static_cast<float>(c[1]), static_cast<float>(c[2]), static_cast<float>(c[3]), static_cast<int>(c[4]), static_cast<int>(c[5]));
    depth_camera.SetPara(static_cast<float>(d[0]), static_cast<float>(d[1]), static_cast<float>(d[2]), static_cast<float>(d[3]), static_cast<int>(d[4]), static_cast<int>(d[5]),
                         static_cast<float>(d[6]));
    geometry::TransformationMatrix M;
    for (int r = 0; r < 4; ++r)
        for (int k = 0; k < 4; ++k) M(r, k) = static_cast<float>(m[4 * r + k]);
    int depth_rows = static_cast<int>(d[5]), depth_cols = static_cast<int>(d[4]);
    { // an optional "depth_rows depth_cols" pair: a depth IMAGE whose size is not the camera's (the refused input of the tests)
        int r2 = 0, c2 = 0;
        if (ps >> r2 >> c2) { depth_rows = r2; depth_cols = c2; }
    }
    cv::Mat color(rows, cols, CV_8UC3), depth(depth_rows, depth_cols, u16 ? CV_16UC1 : CV_32FC1);
    if (!ReadAll(dir + "/color.u8", color.data, color.total() * 3) || !ReadAll(dir + (u16 ? "/depth.u16" : "/depth.f32"), depth.data, depth.total() * (u16 ? 2 : 4))) {
        std::cout << "cannot read the images in " << dir << std::endl;
        return 1;
    }
    long long opt = -1;
    op_runtime_get_option(OP_RUNTIME_OPT_COLOR_ALIGNMENT, &opt);
    const long long opt_default = opt;
    if (path == "device" && op_runtime_set_option(OP_RUNTIME_OPT_COLOR_ALIGNMENT, 1) != OP_OK) { std::cout << op_last_error() << std::endl; return 1; }
    const cv::Mat aligned = tool::AlignColorToDepth(color, depth, color_camera, depth_camera, M);
    std::ofstream os((dir + "/aligned.u8").c_str(), std::ios::binary);
    os.write(reinterpret_cast<const char*>(aligned.data), static_cast<std::streamsize>(aligned.total() * 3));
    std::cout << "{\"path\": \"" << path << "\", \"rows\": " << aligned.rows << ", \"cols\": " << aligned.cols << ", \"option_default\": " << opt_default << "}" << std::endl;
    return os ? 0 : 1;
}

int ListDirectory(const std::string& dir) {
    std::vector<std::string> rgb_files, depth_files;
    std::vector<geometry::TransformationMatrix> poses;
    camera::PinholeCamera c, d;
    tool::ReadImageSequenceFromScannetWithPose(dir, rgb_files, depth_files, poses, c, d);
    std::ostringstream js;
    js.precision(9);
    js << "{\"rgb_files\": [";
    for (size_t i = 0; i < rgb_files.size(); ++i) js << (i ? ", " : "") << "\"" << rgb_files[i] << "\"";
    js << "], \"depth_files\": [";
    for (size_t i = 0; i < depth_files.size(); ++i) js << (i ? ", " : "") << "\"" << depth_files[i] << "\"";
    js << "], \"rgb_camera\": [" << c.GetFx() << ", " << c.GetFy() << ", " << c.GetCx() << ", " << c.GetCy() << ", " << c.GetWidth() << ", " << c.GetHeight() << ", " << c.GetDepthScale()
       << "], \"depth_camera\": [" << d.GetFx() << ", " << d.GetFy() << ", " << d.GetCx() << ", " << d.GetCy() << ", " << d.GetWidth() << ", " << d.GetHeight() << ", "
       << d.GetDepthScale() << "], \"poses\": [";
    for (size_t i = 0; i < poses.size(); ++i)
        for (int k = 0; k < 16; ++k) js << (i || k ? ", " : "") << poses[i](k / 4, k % 4);
    js << "]}";
    std::cout << js.str() << std::endl;
    return 0;
}

bool DumpVolume(const std::string& dir, integration::CubeHandler& cube_handler) {
    const integration::CubeMap map = cube_handler.GetCubeMap();
    std::vector<const integration::VoxelCube*> cubes;
    for (integration::CubeMap::const_iterator it = map.begin(); it != map.end(); ++it) cubes.push_back(&it->second);
    std::sort(cubes.begin(), cubes.end(), [](const integration::VoxelCube* a, const integration::VoxelCube* b) {
        for (int k = 0; k < 3; ++k)
            if (a->cube_id(k) != b->cube_id(k)) return a->cube_id(k) < b->cube_id(k);
        return false;
    });
    std::ofstream keys((dir + "/volume_keys.i32").c_str(), std::ios::binary), vox((dir + "/volume_voxels.f32").c_str(), std::ios::binary);
    for (const integration::VoxelCube* cube : cubes) {
        const int id[3] = {cube->cube_id(0), cube->cube_id(1), cube->cube_id(2)};
        keys.write(reinterpret_cast<const char*>(id), sizeof(id));
        for (const integration::TSDFVoxel& t : cube->voxels) {
            const float v[5] = {t.sdf, t.weight, t.color(0), t.color(1), t.color(2)};
            vox.write(reinterpret_cast<const char*>(v), sizeof(v));
        }
    }
    return keys && vox;
}

} // namespace

int main(int argc, char* argv[]) {
    std::string dir, path = "host", color_ext, ply_file, dump, align_dir, list_dir;
    float voxel = 0.02f;
    size_t stride = 10, max_frames = 0; // GenerateModelFromScannet.cpp:51
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--voxel" && i + 1 < argc) voxel = static_cast<float>(std::atof(argv[++i]));
        else if (a == "--stride" && i + 1 < argc) stride = static_cast<size_t>(std::atoi(argv[++i]));
        else if (a == "--frames" && i + 1 < argc) max_frames = static_cast<size_t>(std::atoi(argv[++i]));
        else if (a == "--path" && i + 1 < argc) path = argv[++i];
        else if (a == "--color-ext" && i + 1 < argc) color_ext = argv[++i];
        else if (a == "--ply" && i + 1 < argc) ply_file = argv[++i];
        else if (a == "--dump" && i + 1 < argc) dump = argv[++i];
        else if (a == "--align" && i + 1 < argc) align_dir = argv[++i];
        else if (a == "--list" && i + 1 < argc) list_dir = argv[++i];
        else if (dir.empty() && a[0] != '-') dir = a;
    }
    if (!list_dir.empty()) return ListDirectory(list_dir);
    const bool known = path == "host" || path == "device" || path == "fused";
    if (!align_dir.empty() && known && path != "fused") return AlignOne(align_dir, path);
    if (dir.empty() || !known || stride == 0) {
        std::cout << "Usage: ScannetIntegration <dir> [--voxel V] [--stride N] [--frames N] [--path host|device|fused] [--color-ext png] [--ply out.ply] [--dump DIR]\n"
                     "       ScannetIntegration --align DIR [--path host|device]\n"
                     "       ScannetIntegration --list DIR" << std::endl;
        return 1;
    }
    std::vector<std::string> rgb_files, depth_files;
    std::vector<geometry::TransformationMatrix> poses;
    camera::PinholeCamera color_camera, depth_camera;
    tool::ReadImageSequenceFromScannetWithPose(dir, rgb_files, depth_files, poses, color_camera, depth_camera);
    if (!color_ext.empty())
        for (std::string& f : rgb_files) f = f.substr(0, f.rfind('.') + 1) + color_ext;
    if (path == "device" && op_runtime_set_option(OP_RUNTIME_OPT_COLOR_ALIGNMENT, 1) != OP_OK) { std::cout << op_last_error() << std::endl; return 1; }
    integration::CubeHandler cube_handler(depth_camera);
    cube_handler.SetVoxelResolution(voxel);
    cube_handler.SetFarPlane(3);       // GenerateModelFromScannet.cpp:39-40
    cube_handler.SetTruncation(0.15f);
    double t_read = 0, t_align = 0, t_integrate = 0;
    size_t used = 0;
    const std::chrono::steady_clock::time_point t_all = std::chrono::steady_clock::now();
    for (size_t i = 0; i != rgb_files.size(); ++i) {
        if (i % stride != 0) continue;
        if (max_frames && used == max_frames) break;
        std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
        cv::Mat rgb = cv::imread(rgb_files[i]);
        cv::Mat depth = cv::imread(depth_files[i], -1);
        if (rgb.empty() || depth.empty()) {
            std::cout << RED << "[ERROR]::cannot read frame " << i << " (" << rgb_files[i] << ")" << RESET << std::endl;
            return 1;
        }
        cv::Mat refined_depth;
        tool::ConvertDepthTo32F(depth, refined_depth, depth_camera.GetDepthScale());
        t_read += Seconds(t0);
        t0 = std::chrono::steady_clock::now();
        if (path == "fused") {
            cube_handler.IntegrateImage(refined_depth, rgb, poses[i], color_camera);
            t_integrate += Seconds(t0);
        } else {
            cv::Mat aligned_rgb = tool::AlignColorToDepth(rgb, refined_depth, color_camera, depth_camera);
            t_align += Seconds(t0);
            t0 = std::chrono::steady_clock::now();
            cube_handler.IntegrateImage(refined_depth, aligned_rgb, poses[i]);
            t_integrate += Seconds(t0);
        }
        ++used;
    }
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    cube_handler.Synchronize();
    const double t_sync = Seconds(t0), t_frames = Seconds(t_all);
    const size_t blocks = cube_handler.GetCubeCount();
    bool ok = true;
    if (!dump.empty()) ok = DumpVolume(dump, cube_handler);
    size_t triangles = 0;
    double t_mesh = 0;
    if (!ply_file.empty()) {
        t0 = std::chrono::steady_clock::now();
        geometry::TriangleMesh mesh;
        cube_handler.ExtractSimplifiedTriangleMesh(mesh, voxel); // ExtractTriangleMesh + ClusteringSimplify(voxel_resolution), GenerateModelFromScannet.cpp:68-69
        t_mesh = Seconds(t0);
        triangles = mesh.GetTriangleSize();
        mesh.WriteToPLY(ply_file);
    }
    std::ostringstream js;
    js << "{\"path\": \"" << path << "\", \"frames\": " << used << ", \"of\": " << rgb_files.size() << ", \"blocks\": " << blocks << ", \"triangles\": " << triangles
       << ", \"read_s\": " << t_read << ", \"align_s\": " << t_align << ", \"integrate_s\": " << t_integrate << ", \"sync_s\": " << t_sync << ", \"frames_s\": " << t_frames
       << ", \"mesh_s\": " << t_mesh << "}";
    std::cout << js.str() << std::endl;
    if (!dump.empty()) { std::ofstream os((dump + "/result.json").c_str()); os << js.str() << std::endl; }
    return ok ? 0 : 1;
}
