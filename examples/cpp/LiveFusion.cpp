// LiveFusion.cpp -- the live reconstruction loop on this repository's class surface: every new frame is tracked against the MODEL fused so far
// (render -> track -> compose -> integrate: the KinectFusion loop), or, for comparison, against the previous frame as the reference's
// example/DenseFusion does (DenseSlam.cpp:22-30).  Frame-to-frame chains every tracking error into the trajectory; frame-to-model is anchored to
// the volume, whose surface averages the frames fused so far, so its drift levels off (DESIGN.md "Frame-to-model tracking").
//
//   LiveFusion --synthetic N STRIDE SEED [--track frame|model] [--res 0.01] [--bilateral] [--sums ref|fp64] [--out DIR]
//   --synthetic N STRIDE SEED  N frames of an analytic room (a box with two spheres, coloured by position), rendered in this program from a camera
//                              that orbits near the room's centre looking outward: frame k is step FIRST + k * STRIDE of a 1000-step orbit, and SEED
//                              picks FIRST (seed 1: step 0).  No input files.
//   --track                    model (default): odometry::Odometry::DenseTrackingToModel against integration::CubeHandler's volume rendered at the last
//                              good pose; frame: DenseTracking(last tracked frame, new frame), poses chained
//   --res                      voxel size in metres
//   --bilateral                fuse the bilaterally filtered depth (tool::BilateralFilter), as example/DenseFusion does; tracking reads the raw frame
//   --sums                     how the tracker sums an iteration's normal equations: ref (the library's default: the reference's sequential float32
//                              order) or fp64 (the order-free device reduction)
//   --out DIR                  where trajectory.txt (one pose per line, 16 floats row-major, every frame: an untracked frame repeats the last good pose)
//                              and pose_error.txt (frame, translation error in metres, rotation error in degrees against the orbit's true pose) go;
//                              default: the working directory
// Frame 0 is fused at its given pose without tracking.  A frame whose track fails is not fused and the last good pose is kept.  Per stage the
// program prints the mean time per frame: render (the model view, on the device's clock), track, integrate (host clock, each stage waited for).
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "Geometry/Geometry.h"
#include "Geometry/RGBDFrame.h"
#include "Integration/CubeHandler.h"
#include "Odometry/Odometry.h"
#include "Tool/ImageProcessing.h"
#include "onepiece_hip.h"
using namespace one_piece;

namespace {

const double kPi = 3.14159265358979323846;
const float kRoomHalf[3] = {2.6f, 1.4f, 2.6f};
const float kSpheres[2][4] = {{1.2f, 0.7f, 1.6f, 0.55f}, {-1.4f, 0.5f, -1.1f, 0.7f}};

// camera-to-world pose of orbit step i: radius 0.4 m, looking outward, a slow pitch
geometry::TransformationMatrix RoomPose(long i) {
    const double th = 2.0 * kPi * static_cast<double>(i % 1000) / 1000.0;
    const long loop = i / 1000;
    const double radius = 0.4 + 0.05 * static_cast<double>(loop % 8), pitch = 0.12 * std::sin(2.0 * th + 0.3 * static_cast<double>(loop));
    const double cy = std::cos(th), sy = std::sin(th), cp = std::cos(pitch), sp = std::sin(pitch);
    const double Ry[3][3] = {{cy, 0, sy}, {0, 1, 0}, {-sy, 0, cy}}, Rx[3][3] = {{1, 0, 0}, {0, cp, -sp}, {0, sp, cp}};
    geometry::TransformationMatrix T = geometry::TransformationMatrix::Identity();
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) T(r, c) = static_cast<float>(Ry[r][0] * Rx[0][c] + Ry[r][1] * Rx[1][c] + Ry[r][2] * Rx[2][c]);
    T(0, 3) = static_cast<float>(radius * sy);
    T(1, 3) = static_cast<float>(0.15 * std::sin(3.0 * th));
    T(2, 3) = static_cast<float>(radius * cy);
    return T;
}

float Slab(float o, float d, float half) {
    if (!(std::fabs(d) > 1e-9f)) return 1e9f;
    return ((d > 0 ? half : -half) - o) / d;
}

// the room seen from `pose`: z-depth in metres (CV_32FC1) and a colour that depends on the surface point alone (CV_8UC3)
void RoomRender(const geometry::TransformationMatrix& pose, const camera::PinholeCamera& cam, cv::Mat& depth, cv::Mat& rgb) {
    const int w = static_cast<int>(cam.GetWidth()), h = static_cast<int>(cam.GetHeight());
    depth.create(h, w, CV_32FC1);
    rgb.create(h, w, CV_8UC3);
    const float fx = cam.GetFx(), fy = cam.GetFy(), cx = cam.GetCx(), cy = cam.GetCy();
    const float ox = pose(0, 3), oy = pose(1, 3), oz = pose(2, 3);
    for (int v = 0; v < h; ++v)
        for (int u = 0; u < w; ++u) {
            const float a = (static_cast<float>(u) - cx) / fx, b = (static_cast<float>(v) - cy) / fy;
            const float dx = pose(0, 0) * a + pose(0, 1) * b + pose(0, 2), dy = pose(1, 0) * a + pose(1, 1) * b + pose(1, 2), dz = pose(2, 0) * a + pose(2, 1) * b + pose(2, 2);
            float t = std::fmin(std::fmin(Slab(ox, dx, kRoomHalf[0]), Slab(oy, dy, kRoomHalf[1])), Slab(oz, dz, kRoomHalf[2]));
            const float dd = dx * dx + dy * dy + dz * dz;
            for (int s = 0; s < 2; ++s) {
                const float lx = ox - kSpheres[s][0], ly = oy - kSpheres[s][1], lz = oz - kSpheres[s][2];
                const float bb = dx * lx + dy * ly + dz * lz, cc = lx * lx + ly * ly + lz * lz - kSpheres[s][3] * kSpheres[s][3];
                const float disc = bb * bb - dd * cc;
                if (disc > 0) {
                    const float ts = (-bb - std::sqrt(disc)) / dd;
                    if (ts > 0.05f && ts < t) t = ts;
                }
            }
            const float hx = ox + t * dx, hy = oy + t * dy, hz = oz + t * dz;
            const float r = 128.0f + 110.0f * std::sin(3.1f * hx + 0.7f * hy), g = 128.0f + 110.0f * std::sin(2.3f * hy + 1.9f * hz), bl = 128.0f + 110.0f * std::sin(2.7f * hz - 1.3f * hx);
            depth.at<float>(v, u) = t;
            unsigned char* px = rgb.data + 3 * (static_cast<size_t>(v) * w + u); // stored order B, G, R like cv::imread
            px[0] = static_cast<unsigned char>(std::fmin(std::fmax(bl, 0.0f), 255.0f));
            px[1] = static_cast<unsigned char>(std::fmin(std::fmax(g, 0.0f), 255.0f));
            px[2] = static_cast<unsigned char>(std::fmin(std::fmax(r, 0.0f), 255.0f));
        }
}

// translation error in metres and rotation error in degrees of an estimated camera pose
void PoseError(const geometry::TransformationMatrix& est, const geometry::TransformationMatrix& truth, double* dt, double* deg) {
    double t2 = 0, trace = 0;
    for (int r = 0; r < 3; ++r) {
        const double d = static_cast<double>(est(r, 3)) - static_cast<double>(truth(r, 3));
        t2 += d * d;
        for (int c = 0; c < 3; ++c) trace += static_cast<double>(est(r, c)) * static_cast<double>(truth(r, c)); // trace(est^T truth)
    }
    double cs = (trace - 1.0) / 2.0;
    cs = cs > 1.0 ? 1.0 : (cs < -1.0 ? -1.0 : cs);
    *dt = std::sqrt(t2);
    *deg = std::acos(cs) * 180.0 / kPi;
}

double Seconds(std::chrono::steady_clock::time_point a) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - a).count(); }

} // namespace

int main(int argc, char* argv[]) {
    long synthetic[3] = {0, 1, 1};
    bool is_synthetic = false, bilateral = false;
    std::string track = "model", sums, out_dir = ".";
    float res = 0.01f;
    bool bad = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--synthetic" && i + 3 < argc) { is_synthetic = true; for (int k = 0; k < 3; ++k) synthetic[k] = std::atol(argv[++i]); }
        else if (a == "--track" && i + 1 < argc) track = argv[++i];
        else if (a == "--res" && i + 1 < argc) res = static_cast<float>(std::atof(argv[++i]));
        else if (a == "--bilateral") bilateral = true;
        else if (a == "--sums" && i + 1 < argc) sums = argv[++i];
        else if (a == "--out" && i + 1 < argc) out_dir = argv[++i];
        else bad = true;
    }
    if (bad || !is_synthetic || synthetic[0] < 1 || synthetic[1] < 1 || synthetic[2] < 0 || (track != "frame" && track != "model") || !(res > 0) ||
        (!sums.empty() && sums != "ref" && sums != "fp64")) {
        std::cout << "usage::LiveFusion --synthetic N STRIDE SEED [--track frame|model] [--res 0.01] [--bilateral] [--sums ref|fp64] [--out DIR]" << std::endl;
        return 2;
    }
    if (!sums.empty()) // before the first tracker exists: the mode new trackers start in
        op_runtime_set_option(OP_RUNTIME_OPT_TRACKER_DEFAULT_SUMS, sums == "fp64" ? OP_TRACK_SUMS_FP64 : OP_TRACK_SUMS_REFERENCE_F32);
    const bool to_model = track == "model";
    const long n = synthetic[0], stride = synthetic[1], first = ((synthetic[2] + 999) % 1000) * 97 % 1000;

    camera::PinholeCamera camera;
    camera.SetCameraType(camera::CameraType::OPEN3D_DATASET);
    odometry::Odometry rgbd_odometry(camera);
    integration::CubeHandler cube_handler(camera);
    cube_handler.SetVoxelResolution(res);

    std::vector<geometry::TransformationMatrix> trajectory;
    std::vector<double> err_t, err_r;
    geometry::TransformationMatrix last_pose = geometry::TransformationMatrix::Identity();
    geometry::RGBDFrame last_frame;
    double t_render = 0, t_track = 0, t_integrate = 0;
    long tracked = 0, lost = 0;
    size_t min_model_pixels = static_cast<size_t>(-1);
    auto integrate = [&](const geometry::RGBDFrame& frame, const geometry::TransformationMatrix& pose) {
        const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
        if (bilateral) {
            cv::Mat filtered;
            tool::BilateralFilter(frame.depth, filtered);
            cube_handler.IntegrateImage(filtered, frame.rgb, pose);
        } else {
            cube_handler.IntegrateImage(frame.depth, frame.rgb, pose);
        }
        cube_handler.Synchronize(); // the stage is waited for, so that the next frame's render time is the render's alone
        t_integrate += Seconds(t0);
    };
    for (long k = 0; k < n; ++k) {
        const geometry::TransformationMatrix truth = RoomPose(first + k * stride);
        cv::Mat depth, rgb;
        RoomRender(truth, camera, depth, rgb);
        geometry::RGBDFrame frame(rgb, depth, static_cast<int>(k));
        if (k == 0) {
            last_pose = truth;
            integrate(frame, last_pose);
            last_frame = frame;
        } else {
            const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
            bool ok = false;
            geometry::TransformationMatrix pose = last_pose;
            if (to_model) {
                std::shared_ptr<odometry::ModelTrackingResult> r = rgbd_odometry.DenseTrackingToModel(cube_handler, last_pose, frame, geometry::TransformationMatrix::Identity(), 0);
                ok = r->tracking_success;
                pose = r->pose;
                if (r->model_pixels < min_model_pixels) min_model_pixels = r->model_pixels;
                const double total = Seconds(t0);
                double render_ms = 0;
                rgbd_odometry.LastModelTimes(&render_ms, nullptr);
                t_render += render_ms / 1000.0;
                t_track += total - render_ms / 1000.0;
            } else {
                std::shared_ptr<odometry::DenseTrackingResult> r = rgbd_odometry.DenseTracking(last_frame, frame, geometry::TransformationMatrix::Identity(), 0);
                ok = r->tracking_success;
                if (ok) pose = last_pose * r->T.inverse(); // DenseSlam.cpp:30
                t_track += Seconds(t0);
            }
            if (ok) {
                ++tracked;
                last_pose = pose;
                integrate(frame, last_pose);
                last_frame = frame;
            } else {
                ++lost;
                std::cout << YELLOW << "[WARNING]::tracking lost at frame " << k << RESET << std::endl;
            }
        }
        trajectory.push_back(last_pose);
        double dt = 0, deg = 0;
        PoseError(last_pose, truth, &dt, &deg);
        err_t.push_back(dt);
        err_r.push_back(deg);
    }
    {
        std::ofstream ofs((out_dir + "/trajectory.txt").c_str());
        ofs.precision(9);
        for (size_t k = 0; k < trajectory.size(); ++k)
            for (int r = 0; r < 4; ++r)
                for (int c = 0; c < 4; ++c) ofs << trajectory[k](r, c) << (r == 3 && c == 3 ? "\n" : " ");
        std::ofstream efs((out_dir + "/pose_error.txt").c_str());
        efs.precision(9);
        for (size_t k = 0; k < err_t.size(); ++k) efs << k << " " << err_t[k] << " " << err_r[k] << "\n";
        if (!ofs || !efs) { std::cout << RED << "[ERROR]::cannot write to " << out_dir << RESET << std::endl; return 1; }
    }
    const double per = n > 1 ? 1000.0 / static_cast<double>(n - 1) : 0.0, per_fused = 1000.0 / static_cast<double>(tracked + 1);
    std::cout << "{\"frames\": " << n << ", \"stride\": " << stride << ", \"first\": " << first << ", \"track\": \"" << track << "\", \"sums\": \"" << (sums.empty() ? "ref" : sums)
              << "\", \"res\": " << res << ", \"bilateral\": " << (bilateral ? "true" : "false") << ", \"tracked\": " << tracked << ", \"lost\": " << lost
              << ", \"ms_per_frame\": {\"render\": " << t_render * per << ", \"track\": " << t_track * per << ", \"integrate\": " << t_integrate * per_fused << "}"
              << ", \"min_model_pixels\": " << (to_model && n > 1 ? static_cast<long long>(min_model_pixels) : -1LL) << ", \"blocks\": " << cube_handler.GetCubeCount()
              << ", \"final_error_m\": " << err_t.back() << ", \"final_error_deg\": " << err_r.back() << "}" << std::endl;
    return 0;
}
