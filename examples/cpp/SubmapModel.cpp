// SubmapModel.cpp -- the model of one submap as Submap::GenerateSubmapModel builds it (example/DenseFusion/DenseSlam.h:19-33) and
// DownSampleAndExtractFeature then thins it: per frame LoadFromRGBD, Transform(relative pose), DownSample(0.025), MergePCD, and one
// DownSample(0.05) of the merged cloud -- stage by stage, so that every intermediate cloud can be written out and every stage timed.
//
//   SubmapModel [--frames 17] [--path host|device|fused] [--warmup 1] [--dump DIR]
//   SubmapModel --cloud points.f32 [--colors colors.f32] [--normals normals.f32] [--grid 0.05] [--path host|device] [--dump DIR]
//
//   the frames     views of the analytic room of GlobalRegistration.cpp --synthetic (a box with two spheres) along its circle of camera poses,
//                  rendered to float depth and to a colour that is a function of the surface point; poses relative to the first view
//   --path host    OP_RUNTIME_OPT_POINT_CLOUD_DOWNSAMPLE 0: PointCloud::DownSample is the host loop
//   --path device  the option at 1: the same calls, DownSample forwards to op_point_cloud_downsample
//   --path fused   load + transform + down-sample of a frame in one call that leaves only the thinned cloud on the host
//                  (op_points_from_rgbd_downsampled); the final DownSample with the option at 1
//   --warmup N     whole untimed passes before the timed one (first launches load code objects, first buffers are allocated)
//   --cloud        instead of the frames: one raw little-endian n x 3 float32 cloud through DownSample(--grid); with --path host no device is touched
//   --dump DIR     frame_NN_points.f32 / frame_NN_colors.f32, merged_*.f32, final_*.f32 (--cloud: cloud_points.f32, cloud_colors.f32,
//                  cloud_normals.f32) and result.json with the sizes and the time of every stage
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
#include "Geometry/PointCloud.h"
#include "onepiece_hip.h"
#include "src/Bridge.h" // the class surface's own device choice and conversions
using namespace one_piece;

namespace {

double Now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

bool WriteRaw(const std::string& dir, const std::string& name, const geometry::Point3List& p) {
    std::ofstream os((dir + "/" + name).c_str(), std::ios::binary);
    if (!p.empty()) os.write(reinterpret_cast<const char*>(p[0].data()), static_cast<std::streamsize>(p.size() * 3 * sizeof(float)));
    return static_cast<bool>(os);
}
bool ReadRaw(const std::string& file, geometry::Point3List& out) {
    std::ifstream is(file.c_str(), std::ios::binary | std::ios::ate);
    if (!is) return false;
    const std::streamsize bytes = is.tellg();
    if (bytes < 0 || bytes % 12 != 0) return false;
    out.assign(static_cast<size_t>(bytes / 12), geometry::Point3(0, 0, 0));
    is.seekg(0);
    return bytes == 0 || static_cast<bool>(is.read(reinterpret_cast<char*>(out[0].data()), bytes));
}
bool DumpCloud(const std::string& dir, const std::string& tag, const geometry::PointCloud& pcd) {
    return WriteRaw(dir, tag + "_points.f32", pcd.points) && WriteRaw(dir, tag + "_colors.f32", pcd.colors) && (pcd.normals.empty() || WriteRaw(dir, tag + "_normals.f32", pcd.normals));
}

// camera-to-world pose on a circle of radius 0.5 m at angle th, looking outward, slightly pitched (GlobalRegistration.cpp --synthetic)
geometry::TransformationMatrix ViewPose(float th, float pitch) {
    const float cy = std::cos(th), sy = std::sin(th), cp = std::cos(pitch), sp = std::sin(pitch);
    geometry::TransformationMatrix T = geometry::TransformationMatrix::Identity();
    const float Ry[9] = {cy, 0, sy, 0, 1, 0, -sy, 0, cy}, Rx[9] = {1, 0, 0, 0, cp, -sp, 0, sp, cp};
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) T(r, c) = Ry[3 * r] * Rx[c] + Ry[3 * r + 1] * Rx[3 + c] + Ry[3 * r + 2] * Rx[6 + c];
    T(0, 3) = 0.5f * sy; T(1, 3) = 0.05f; T(2, 3) = 0.5f * cy;
    return T;
}
// z-depth and colour of that room seen from `pose`: a 5.2 x 2.8 x 5.2 m box around the origin with two spheres in it; the colour is a smooth
// function of the surface point, so that neighbouring views agree on it
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

struct Frame { cv::Mat depth, rgb; geometry::TransformationMatrix relative; };
struct Times { double load = 0, transform = 0, downsample = 0, fused = 0, merge = 0, final_downsample = 0; };

// One pass over the frames: the body of GenerateSubmapModel, then the 0.05 m DownSample of DownSampleAndExtractFeature (GlobalRegistration.cpp:133-140)
bool BuildModel(const std::vector<Frame>& frames, const camera::PinholeCamera& cam, bool fused, std::vector<geometry::PointCloud>& per_frame,
                geometry::PointCloud& merged, geometry::PointCloud& final_cloud, Times& ms) {
    const op_camera pod = cam.Pod();
    per_frame.assign(frames.size(), geometry::PointCloud());
    merged.Reset();
    ms = Times();
    for (size_t i = 0; i < frames.size(); ++i) {
        double t = Now();
        if (fused) {
            geometry::PointCloud& out = per_frame[i];
            const size_t npix = static_cast<size_t>(pod.width) * pod.height;
            out.points.resize(npix);
            out.colors.resize(npix);
            float T[16];
            bridge::RowMajor(frames[i].relative, T);
            size_t n = 0;
            if (bridge::Failed(op_points_from_rgbd_downsampled(&pod, frames[i].depth.data, bridge::DepthFormat(frames[i].depth), frames[i].rgb.data, T, 0.025f, OP_MEM_HOST,
                                                               bridge::Device(), bridge::Floats(out.points), bridge::Floats(out.colors), &n),
                               "SubmapModel"))
                return false;
            out.points.resize(n);
            out.colors.resize(n);
            ms.fused += Now() - t;
        } else {
            geometry::PointCloud tmp;
            tmp.LoadFromRGBD(frames[i].rgb, frames[i].depth, cam);          // DenseSlam.h:26
            ms.load += Now() - t; t = Now();
            tmp.Transform(frames[i].relative);                               // :27
            ms.transform += Now() - t; t = Now();
            per_frame[i] = *tmp.DownSample(0.025f);                          // :28
            ms.downsample += Now() - t;
        }
        t = Now();
        merged.MergePCD(per_frame[i]);                                       // :30
        ms.merge += Now() - t;
    }
    const double t = Now();
    final_cloud = *merged.DownSample(0.05f);
    ms.final_downsample = Now() - t;
    return true;
}

} // namespace

int main(int argc, char** argv) {
    int n_frames = 17, warmup = 1;
    float grid = 0.05f;
    std::string dump, path = "host", cloud_file, colors_file, normals_file;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--frames" && i + 1 < argc) n_frames = std::atoi(argv[++i]);
        else if (a == "--warmup" && i + 1 < argc) warmup = std::atoi(argv[++i]);
        else if (a == "--path" && i + 1 < argc) path = argv[++i];
        else if (a == "--dump" && i + 1 < argc) dump = argv[++i];
        else if (a == "--cloud" && i + 1 < argc) cloud_file = argv[++i];
        else if (a == "--colors" && i + 1 < argc) colors_file = argv[++i];
        else if (a == "--normals" && i + 1 < argc) normals_file = argv[++i];
        else if (a == "--grid" && i + 1 < argc) grid = static_cast<float>(std::atof(argv[++i]));
        else { std::cout << "unknown argument " << a << std::endl; return 2; }
    }
    const bool fused = path == "fused";
    if (n_frames < 1 || warmup < 0 || (path != "host" && path != "device" && !fused) || (fused && !cloud_file.empty())) {
        std::cout << "Usage: SubmapModel [--frames N] [--path host|device|fused] [--warmup N] [--dump DIR]\n"
                     "       SubmapModel --cloud points.f32 [--colors colors.f32] [--normals normals.f32] [--grid L] [--path host|device] [--dump DIR]" << std::endl;
        return 2;
    }
    if (op_runtime_set_option(OP_RUNTIME_OPT_POINT_CLOUD_DOWNSAMPLE, path == "host" ? 0 : 1) != OP_OK) { std::cout << op_last_error() << std::endl; return 3; }

    if (!cloud_file.empty()) {
        geometry::PointCloud in;
        if (!ReadRaw(cloud_file, in.points) || (!colors_file.empty() && !ReadRaw(colors_file, in.colors)) || (!normals_file.empty() && !ReadRaw(normals_file, in.normals))) {
            std::cout << "cannot read the cloud" << std::endl;
            return 3;
        }
        double t = Now();
        const geometry::PointCloud out = *in.DownSample(grid);
        t = Now() - t;
        if (!dump.empty() && !DumpCloud(dump, "cloud", out)) { std::cout << "cannot write to " << dump << std::endl; return 3; }
        std::ostringstream js;
        js << "{\"path\": \"" << path << "\", \"grid\": " << grid << ", \"points\": " << in.GetSize() << ", \"cells\": " << out.GetSize() << ", \"ms\": {\"downsample\": " << t << "}}";
        std::cout << js.str() << std::endl;
        if (!dump.empty()) { std::ofstream os((dump + "/result.json").c_str()); os << js.str() << std::endl; }
        return 0;
    }

    camera::PinholeCamera cam(514.817f, 515.375f, 318.771f, 238.447f, 640, 480, 1.0f); // depth scale 1: the rendered depth is metres in float
    std::vector<Frame> frames(static_cast<size_t>(n_frames));
    const geometry::TransformationMatrix first_inverse = ViewPose(0.40f, -0.04f).inverse();
    for (int i = 0; i < n_frames; ++i) { // every third frame of a slow pan: 0.03 rad between the views that are used
        const geometry::TransformationMatrix pose = ViewPose(0.40f + 0.03f * i, -0.04f + 0.005f * i);
        RenderRoom(pose, cam, frames[static_cast<size_t>(i)].depth, frames[static_cast<size_t>(i)].rgb);
        frames[static_cast<size_t>(i)].relative = first_inverse * pose;
    }
    std::vector<geometry::PointCloud> per_frame;
    geometry::PointCloud merged, final_cloud;
    Times ms;
    for (int pass = 0; pass <= warmup; ++pass)
        if (!BuildModel(frames, cam, fused, per_frame, merged, final_cloud, ms)) return 3;

    if (!dump.empty()) {
        bool ok = DumpCloud(dump, "merged", merged) && DumpCloud(dump, "final", final_cloud);
        for (size_t i = 0; ok && i < per_frame.size(); ++i) {
            char tag[32];
            std::snprintf(tag, sizeof(tag), "frame_%02d", static_cast<int>(i));
            ok = DumpCloud(dump, tag, per_frame[i]);
        }
        if (!ok) { std::cout << "cannot write to " << dump << std::endl; return 3; }
    }
    std::ostringstream js;
    js << "{\"path\": \"" << path << "\", \"frames\": " << n_frames << ", \"warmup\": " << warmup << ", \"frame_points\": [";
    for (size_t i = 0; i < per_frame.size(); ++i) js << (i ? ", " : "") << per_frame[i].GetSize();
    js << "], \"merged_points\": " << merged.GetSize() << ", \"final_points\": " << final_cloud.GetSize() << ", \"ms\": {\"load\": " << ms.load << ", \"transform\": " << ms.transform
       << ", \"downsample\": " << ms.downsample << ", \"fused\": " << ms.fused << ", \"merge\": " << ms.merge << ", \"final_downsample\": " << ms.final_downsample
       << ", \"total\": " << ms.load + ms.transform + ms.downsample + ms.fused + ms.merge + ms.final_downsample << "}}";
    std::cout << js.str() << std::endl;
    if (!dump.empty()) { std::ofstream os((dump + "/result.json").c_str()); os << js.str() << std::endl; }
    return 0;
}
