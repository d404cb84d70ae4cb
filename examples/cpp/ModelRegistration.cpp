// ModelRegistration.cpp -- telling the fused model where a frame belongs.  N frames of the analytic room are fused; then every K-th frame is taken
// out of the model (DeintegrateImage), its depth image is registered against what is left from a drifted pose, and the frame is fused again at the
// pose that was found.  The registration is point-to-plane against the field itself (op_volume_register_depth states the definition): the trilinear
// sdf at a transformed point is the residual, its normalised central difference the normal.
//
//   ModelRegistration --synthetic N STRIDE SEED [--res 0.01] [--perturb K] [--iters I] [--path sample|fused] [--color off|on [--color-scale S]]
//   --batch K [--batch-stride S]   after the run: the first K frames against the whole model from their perturbed poses, all in ONE call of the batch
//                              entry (op_volume_register_batch_frames) and one call per frame, at pixel stride S (default 4); the JSON gains "batch"
//                     [--linearization normal|gradient|metric] [--huber D] [--huber-color D] [--min-step S]
//   --synthetic N STRIDE SEED  N frames of the analytic room of LiveFusion.cpp: frame k is step FIRST + k * STRIDE of a 1000-step orbit, SEED picks FIRST
//   --perturb K                every K-th frame is re-registered (default 20); its start is its true pose moved by 3-4 cm and about a degree
//   --iters I                  Gauss-Newton iterations per frame (default 10; min_step is 0, so both paths take all of them)
//   --path fused (default)     op_volume_register_depth: the back-projection, every iteration's sampling, rows and 6 x 6 reduction on the device; 32
//                              doubles come back per iteration
//   --path sample              the only route there was before it: per iteration op_volume_sample writes sdf, gradient and status of every point
//                              (33 bytes), the host reads them back and forms the same rows and sums in a loop (in point order, in double)
//   --color on                 (fused path only; default off) op_volume_register_rgbd: the colour term -- the model's intensity at the point against the
//                              frame's own -- joins the system with weight --color-scale (default 1); one line per frame (pose error, sdf rmse, colour
//                              rmse, coloured points) precedes the JSON line, which gains "color_scale", "rmse_color" and "colored_last"
//   --linearization L, --huber D, --huber-color D
//                              (fused path only) any of them: op_volume_register_robust_frame -- row and residual of the chosen linearisation
//                              (default metric), Huber weights on the residual (metres) and on the colour residual (default 0: none); with --color
//                              off the depth image alone.  One line per frame: what --color on prints, then the frame's iteration count, status,
//                              last step and down-weighted points; the JSON line gains "linearization", "huber", "huber_color", "downweighted_last"
//                              and "rmse_residual"
//   --min-step S               (with the three above; default 0) the step below which a frame stops: with it the iteration counts say something
//   --coarse L                 (plain fused path only; default 0) every frame is ALSO registered, from the same start, against the model coarsened L times
//                              (CubeHandler::Coarsen, then the same RegisterDepth): two rows after the run -- coarse 0 and coarse L, per-iteration time and
//                              final pose error -- and "coarse" in the JSON.  The frame is fused again at the pose the fine model gave, as without the flag
// Both paths solve with op_ldlt_solve6, update with op_se3_exp and the same float32 product, and gate with the same rules; their sums differ in
// the order of the additions only.  It prints one JSON line: pose errors before and after, iterations, stage times (host clock).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "Geometry/Geometry.h"
#include "Integration/CubeHandler.h"
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

double Seconds(std::chrono::steady_clock::time_point a) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - a).count(); }

void RowMajor(const geometry::TransformationMatrix& T, float out[16]) {
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) out[4 * r + c] = T(r, c);
}
geometry::TransformationMatrix FromRowMajor(const float in[16]) {
    geometry::TransformationMatrix T = geometry::TransformationMatrix::Identity();
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) T(r, c) = in[4 * r + c];
    return T;
}
// C = A B in float32, each element ((a0 b0 + a1 b1) + a2 b2) + a3 b3
void Mul4(const float a[16], const float b[16], float c[16]) {
    for (int r = 0; r < 4; ++r)
        for (int k = 0; k < 4; ++k) c[4 * r + k] = ((a[4 * r] * b[k] + a[4 * r + 1] * b[4 + k]) + a[4 * r + 2] * b[8 + k]) + a[4 * r + 3] * b[12 + k];
}

// a drifted estimate of frame k: pose * (a rotation of about a degree about y, a shift of 3-4 cm); deterministic
void Perturbed(const float pose[16], long k, float out[16]) {
    const double a = 0.015 + 0.002 * static_cast<double>(k % 3);
    float P[16] = {static_cast<float>(std::cos(a)), 0, static_cast<float>(std::sin(a)), 0.03f, 0, 1, 0, -0.02f + 0.005f * static_cast<float>(k % 2),
                   static_cast<float>(-std::sin(a)), 0, static_cast<float>(std::cos(a)), 0.025f, 0, 0, 0, 1};
    Mul4(pose, P, out);
}

// distance between two poses: of the origins in metres, of the rotations in degrees
void PoseError(const float T[16], const float truth[16], double* metres, double* degrees) {
    double d2 = 0, trace = 0;
    for (int r = 0; r < 3; ++r) {
        const double d = static_cast<double>(T[4 * r + 3]) - truth[4 * r + 3];
        d2 += d * d;
        for (int c = 0; c < 3; ++c) trace += static_cast<double>(T[4 * r + c]) * truth[4 * r + c]; // trace(R Rt^T)
    }
    *metres = std::sqrt(d2);
    *degrees = std::acos(std::fmax(-1.0, std::fmin(1.0, (trace - 1.0) / 2.0))) * 180.0 / kPi;
}

struct Outcome { float T[16]; int iterations; unsigned long long used; double rmse, first_rmse; };

// the system at T from op_volume_sample's outputs: the definition of op_volume_register_system, the sums in point order
bool SampleSystem(op_volume* vol, const std::vector<float>& xyz, const float T[16], float max_distance, std::vector<float>& voxels, std::vector<float>& grads,
                  std::vector<uint8_t>& status, double sums[28], unsigned long long* used) {
    const size_t n = xyz.size() / 3;
    for (int k = 0; k < 28; ++k) sums[k] = 0.0;
    *used = 0;
    if (!n) return true;
    if (op_volume_sample(vol, xyz.data(), n, OP_MEM_HOST, T, OP_SAMPLE_TRILINEAR, voxels.data(), grads.data(), status.data(), nullptr) != OP_OK) return false;
    for (size_t i = 0; i < n; ++i) {
        if (status[i] & (OP_SAMPLE_INVALID | OP_SAMPLE_NO_GRADIENT)) continue;
        const float d0 = grads[3 * i], d1 = grads[3 * i + 1], d2 = grads[3 * i + 2], s = voxels[5 * i];
        const float l2 = d0 * d0 + (d1 * d1 + d2 * d2);
        if (!(l2 > 0) || (max_distance > 0 && !(std::fabs(s) <= max_distance))) continue;
        const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        const float q0 = ((T[0] * x + T[1] * y) + T[2] * z) + T[3] * 1.0f, q1 = ((T[4] * x + T[5] * y) + T[6] * z) + T[7] * 1.0f;
        const float q2 = ((T[8] * x + T[9] * y) + T[10] * z) + T[11] * 1.0f, q3 = ((T[12] * x + T[13] * y) + T[14] * z) + T[15] * 1.0f;
        const float p0 = q0 / q3, p1 = q1 / q3, p2 = q2 / q3;
        const float l = std::sqrt(l2), n0 = d0 / l, n1 = d1 / l, n2 = d2 / l;
        const float j[6] = {n0, n1, n2, p1 * n2 - p2 * n1, p2 * n0 - p0 * n2, p0 * n1 - p1 * n0};
        int k = 0;
        for (int a = 0; a < 6; ++a)
            for (int b = a; b < 6; ++b) sums[k++] += static_cast<double>(j[a] * j[b]);
        for (int a = 0; a < 6; ++a) sums[21 + a] += static_cast<double>(s * j[a]);
        sums[27] += static_cast<double>(s) * static_cast<double>(s);
        ++*used;
    }
    return true;
}

// op_volume_register_points' loop around SampleSystem (min_step 0)
bool SampleRegister(op_volume* vol, const std::vector<float>& xyz, const float init[16], int iterations, float max_distance, Outcome* out) {
    const size_t n = xyz.size() / 3;
    std::vector<float> voxels(5 * n), grads(3 * n);
    std::vector<uint8_t> status(n);
    float T[16];
    for (int k = 0; k < 16; ++k) T[k] = init[k];
    double sums[28];
    unsigned long long used = 0;
    out->iterations = 0; out->first_rmse = 0;
    for (int it = 0; it <= iterations; ++it) { // the last evaluation describes the pose that is returned
        if (!SampleSystem(vol, xyz, T, max_distance, voxels, grads, status, sums, &used)) return false;
        if (it == 0) out->first_rmse = used ? std::sqrt(sums[27] / static_cast<double>(used)) : 0.0;
        if (it == iterations || used < 6) break;
        double JTJ[36], JTr[6];
        int k = 0;
        for (int a = 0; a < 6; ++a)
            for (int b = a; b < 6; ++b) { JTJ[6 * a + b] = sums[k]; JTJ[6 * b + a] = sums[k]; ++k; }
        for (int a = 0; a < 6; ++a) JTr[a] = sums[21 + a];
        float x[6], E[16], N[16];
        if (op_ldlt_solve6(JTJ, JTr, x) != OP_OK) return false;
        bool finite = true;
        for (int a = 0; a < 6; ++a) finite = finite && std::isfinite(x[a]);
        if (!finite) break;
        if (op_se3_exp(x, E) != OP_OK) return false;
        Mul4(E, T, N);
        for (int a = 0; a < 16; ++a) T[a] = N[a];
        ++out->iterations;
    }
    for (int k = 0; k < 16; ++k) out->T[k] = T[k];
    out->used = used;
    out->rmse = used ? std::sqrt(sums[27] / static_cast<double>(used)) : 0.0;
    return true;
}

double Median(std::vector<double> v) {
    if (v.empty()) return 0.0;
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

} // namespace

int main(int argc, char* argv[]) {
    long synthetic[3] = {0, 1, 1}, every = 20, iters = 10, batch = 0, batch_stride = 4, coarse = 0;
    bool is_synthetic = false, bad = false;
    std::string path = "fused", color = "off", linearization = "metric";
    float res = 0.01f, color_scale = 1.0f, huber = 0.0f, huber_color = 0.0f, min_step = 0.0f;
    bool have_scale = false, robust = false, have_min_step = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--synthetic" && i + 3 < argc) { is_synthetic = true; for (int k = 0; k < 3; ++k) synthetic[k] = std::atol(argv[++i]); }
        else if (a == "--res" && i + 1 < argc) res = static_cast<float>(std::atof(argv[++i]));
        else if (a == "--perturb" && i + 1 < argc) every = std::atol(argv[++i]);
        else if (a == "--iters" && i + 1 < argc) iters = std::atol(argv[++i]);
        else if (a == "--path" && i + 1 < argc) path = argv[++i];
        else if (a == "--color" && i + 1 < argc) color = argv[++i];
        else if (a == "--color-scale" && i + 1 < argc) { color_scale = static_cast<float>(std::atof(argv[++i])); have_scale = true; }
        else if (a == "--linearization" && i + 1 < argc) { linearization = argv[++i]; robust = true; }
        else if (a == "--huber" && i + 1 < argc) { huber = static_cast<float>(std::atof(argv[++i])); robust = true; }
        else if (a == "--huber-color" && i + 1 < argc) { huber_color = static_cast<float>(std::atof(argv[++i])); robust = true; }
        else if (a == "--min-step" && i + 1 < argc) { min_step = static_cast<float>(std::atof(argv[++i])); have_min_step = true; }
        else if (a == "--batch" && i + 1 < argc) { batch = std::atol(argv[++i]); robust = true; }
        else if (a == "--batch-stride" && i + 1 < argc) batch_stride = std::atol(argv[++i]);
        else if (a == "--coarse" && i + 1 < argc) coarse = std::atol(argv[++i]);
        else bad = true;
    }
    const int lin = linearization == "normal" ? OP_REGISTER_LIN_NORMAL : linearization == "gradient" ? OP_REGISTER_LIN_GRADIENT : linearization == "metric" ? OP_REGISTER_LIN_METRIC : -1;
    const long n = synthetic[0], stride = synthetic[1];
    if (bad || !is_synthetic || n < 1 || stride < 1 || synthetic[2] < 0 || !(res > 0) || every < 1 || iters < 0 || iters > 1000 || (path != "sample" && path != "fused") ||
        (color != "off" && color != "on") || (color == "on" && path != "fused") || (have_scale && color != "on") || !(color_scale >= 0) || lin < 0 || (robust && path != "fused") || !(huber >= 0) || !(huber_color >= 0) ||
        (have_min_step && !robust) || !(min_step >= 0) || batch < 0 || batch_stride < 1 ||
        coarse < 0 || coarse > 4 || (coarse > 0 && (path != "fused" || color == "on" || robust))) {
        std::cout << "usage::ModelRegistration --synthetic N STRIDE SEED [--res 0.01] [--perturb K] [--iters I] [--path sample|fused] [--color off|on [--color-scale S]]"
                     " [--linearization normal|gradient|metric] [--huber D] [--huber-color D] [--min-step S] [--batch K [--batch-stride S]] [--coarse L]" << std::endl;
        return bad || argc > 1 ? 2 : 0;
    }
    const long first = ((synthetic[2] + 999) % 1000) * 97 % 1000;

    camera::PinholeCamera camera;
    camera.SetCameraType(camera::CameraType::OPEN3D_DATASET);
    integration::CubeHandler volume(camera);
    volume.SetVoxelResolution(res);
    if (!volume.Handle()) return 1; // (no device: the class has said so)

    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    for (long k = 0; k < n; ++k) {
        cv::Mat depth, rgb;
        const geometry::TransformationMatrix pose = RoomPose(first + k * stride);
        RoomRender(pose, camera, depth, rgb);
        volume.IntegrateImage(depth, rgb, pose);
    }
    volume.Synchronize();
    const double t_fuse = Seconds(t0);

    op_volume_register_params params;
    if (op_volume_register_default_params(volume.Handle(), &params) != OP_OK) return 1;
    params.max_iterations = static_cast<int>(iters);
    params.min_step = 0.0f;
    const bool with_color = color == "on";
    op_volume_register_color_params color_params;
    if (op_volume_register_color_default_params(volume.Handle(), &color_params) != OP_OK) return 1;
    color_params.base = params;
    color_params.color_scale = color_scale;
    if (robust) color_params.base.min_step = min_step;
    op_volume_register_options options;
    options.linearization = lin; options.huber = huber; options.huber_color = huber_color;
    const char* const status_names[4] = {"converged", "max_iterations", "too_few_points", "singular"};
    std::vector<double> rmse_residual;
    unsigned long long downweighted = 0;
    std::vector<double> register_ms, per_iteration_ms, before_m, before_deg, after_m, after_deg, rmse, first_rmse, rmse_color;
    unsigned long long points = 0, used = 0, colored = 0;
    long frames = 0, iterations = 0;
    double t_out = 0, t_back = 0;
    std::vector<double> coarse_ms, coarse_iteration_ms, coarse_after_m, coarse_after_deg, coarse_rmse, coarsen_ms;
    unsigned long long coarse_blocks = 0;
    for (long k = 0; k < n; k += every, ++frames) {
        cv::Mat depth, rgb;
        const geometry::TransformationMatrix pose = RoomPose(first + k * stride);
        RoomRender(pose, camera, depth, rgb);
        t0 = std::chrono::steady_clock::now();
        volume.DeintegrateImage(depth, rgb, pose);
        volume.Synchronize();
        t_out += Seconds(t0);
        float truth[16], start[16];
        RowMajor(pose, truth);
        Perturbed(truth, k, start);
        Outcome got;
        t0 = std::chrono::steady_clock::now();
        if (robust) {
            op_volume_register_robust_result b;
            if (!volume.RegisterRGBDRobust(depth, with_color ? rgb : cv::Mat(), FromRowMajor(start), 1, &color_params, &options, &b)) return 1;
            const op_volume_register_color_result& c = b.color;
            const op_volume_register_result& r = c.base;
            for (int a = 0; a < 16; ++a) got.T[a] = r.T[a];
            got.iterations = r.iterations; got.used = r.used; got.rmse = r.rmse; got.first_rmse = r.first_rmse;
            points = r.used + r.invalid + r.no_gradient + r.too_far;
            colored = c.colored;
            downweighted = b.downweighted;
            rmse_color.push_back(c.rmse_color);
            rmse_residual.push_back(b.rmse_residual);
            double m = 0, deg = 0;
            PoseError(got.T, truth, &m, &deg);
            std::printf("frame %ld: pose error %.3f mm / %.5f deg, rmse %.6f (first %.6f), colour rmse %.6f (first %.6f), coloured %llu of %llu used, iterations %d, status %s, "
                        "last step %.3e, residual rmse %.6f, down-weighted %llu / %llu\n", k, m * 1000.0, deg, r.rmse, r.first_rmse, c.rmse_color, c.first_rmse_color,
                        static_cast<unsigned long long>(c.colored), static_cast<unsigned long long>(r.used), r.iterations, status_names[r.status & 3], r.last_step, b.rmse_residual,
                        static_cast<unsigned long long>(b.downweighted), static_cast<unsigned long long>(b.color_downweighted));
        } else if (with_color) {
            op_volume_register_color_result c;
            if (!volume.RegisterRGBD(depth, rgb, FromRowMajor(start), 1, &color_params, &c)) return 1;
            const op_volume_register_result& r = c.base;
            for (int a = 0; a < 16; ++a) got.T[a] = r.T[a];
            got.iterations = r.iterations; got.used = r.used; got.rmse = r.rmse; got.first_rmse = r.first_rmse;
            points = r.used + r.invalid + r.no_gradient + r.too_far;
            colored = c.colored;
            rmse_color.push_back(c.rmse_color);
            double m = 0, deg = 0;
            PoseError(got.T, truth, &m, &deg);
            std::printf("frame %ld: pose error %.3f mm / %.5f deg, rmse %.6f (first %.6f), colour rmse %.6f (first %.6f), coloured %llu of %llu used\n", k, m * 1000.0, deg,
                        r.rmse, r.first_rmse, c.rmse_color, c.first_rmse_color, static_cast<unsigned long long>(c.colored), static_cast<unsigned long long>(r.used));
        } else if (path == "fused") {
            op_volume_register_result r;
            if (!volume.RegisterDepth(depth, FromRowMajor(start), 1, &params, &r)) return 1;
            for (int a = 0; a < 16; ++a) got.T[a] = r.T[a];
            got.iterations = r.iterations; got.used = r.used; got.rmse = r.rmse; got.first_rmse = r.first_rmse;
            points = r.used + r.invalid + r.no_gradient + r.too_far;
            if (coarse > 0) { // the same frame, the same start, the model coarsened `coarse` times (timed apart from the fine registration)
                const double fine_ms = Seconds(t0) * 1000.0;
                std::chrono::steady_clock::time_point t1 = std::chrono::steady_clock::now();
                op_volume_coarsen_stats cs;
                std::shared_ptr<integration::CubeHandler> lod = volume.Coarsen(static_cast<int>(coarse), 0.0f, &cs);
                if (!lod) return 1;
                coarsen_ms.push_back(Seconds(t1) * 1000.0);
                coarse_blocks = cs.dst_blocks;
                op_volume_register_result rc;
                t1 = std::chrono::steady_clock::now();
                if (!lod->RegisterDepth(depth, FromRowMajor(start), 1, &params, &rc)) return 1;
                const double ms = Seconds(t1) * 1000.0;
                coarse_ms.push_back(ms);
                coarse_iteration_ms.push_back(ms / static_cast<double>(rc.iterations + 1));
                double m = 0, deg = 0;
                PoseError(rc.T, truth, &m, &deg);
                coarse_after_m.push_back(m); coarse_after_deg.push_back(deg);
                coarse_rmse.push_back(rc.rmse);
                t0 = std::chrono::steady_clock::now() - std::chrono::duration_cast<std::chrono::steady_clock::duration>(std::chrono::duration<double>(fine_ms / 1000.0));
            }
        } else {
            std::vector<float> xyz; // op_points_from_depth's definition, on the host
            const float fx = camera.GetFx(), fy = camera.GetFy(), cx = camera.GetCx(), cy = camera.GetCy();
            for (int v = 0; v < depth.rows; ++v)
                for (int u = 0; u < depth.cols; ++u) {
                    const float z = depth.at<float>(v, u);
                    if (!(z > 0)) continue;
                    xyz.push_back((static_cast<float>(u) - cx) * z / fx); xyz.push_back((static_cast<float>(v) - cy) * z / fy); xyz.push_back(z);
                }
            points = xyz.size() / 3;
            if (!SampleRegister(volume.Handle(), xyz, start, static_cast<int>(iters), params.max_distance, &got)) {
                std::cout << RED << "[ERROR]::the sample path failed: " << op_last_error() << RESET << std::endl;
                return 1;
            }
        }
        const double ms = Seconds(t0) * 1000.0;
        register_ms.push_back(ms);
        per_iteration_ms.push_back(ms / static_cast<double>(got.iterations + 1)); // iterations + 1 evaluations of the system
        double m = 0, deg = 0;
        PoseError(start, truth, &m, &deg);
        before_m.push_back(m); before_deg.push_back(deg);
        PoseError(got.T, truth, &m, &deg);
        after_m.push_back(m); after_deg.push_back(deg);
        rmse.push_back(got.rmse); first_rmse.push_back(got.first_rmse);
        used = got.used;
        iterations += got.iterations;
        t0 = std::chrono::steady_clock::now();
        volume.IntegrateImage(depth, rgb, FromRowMajor(got.T));
        volume.Synchronize();
        t_back += Seconds(t0);
    }
    // --batch K: the first K frames of the sequence against the whole model from their perturbed poses, K frames per call through the batch entry
    // (CubeHandler::RegisterFramesRobust) and one call per frame (RegisterRGBDRobust), both timed: the same poses, one launch per round against
    // one per frame and iteration
    double batch_ms = 0, batch_single_ms = 0;
    op_volume_register_batch_stats batch_stats = op_volume_register_batch_stats();
    bool batch_same = true;
    if (batch > 0) {
        const long K = std::min(batch, n);
        std::vector<cv::Mat> depths(K), rgbs(K);
        geometry::Mat4List starts(K);
        for (long k = 0; k < K; ++k) {
            const geometry::TransformationMatrix pose = RoomPose(first + k * stride);
            RoomRender(pose, camera, depths[k], rgbs[k]);
            float truth[16], start[16];
            RowMajor(pose, truth);
            Perturbed(truth, k, start);
            starts[k] = FromRowMajor(start);
        }
        const std::vector<cv::Mat> no_rgbs;
        std::vector<op_volume_register_robust_result> many, one(K);
        for (int pass = 0; pass < 2; ++pass) { // (the first pass is not timed)
            t0 = std::chrono::steady_clock::now();
            if (volume.RegisterFramesRobust(depths, with_color ? rgbs : no_rgbs, starts, static_cast<int>(batch_stride), &color_params, &options, &many, &batch_stats).size() != static_cast<size_t>(K)) return 1;
            batch_ms = Seconds(t0) * 1000.0;
            t0 = std::chrono::steady_clock::now();
            for (long k = 0; k < K; ++k)
                if (!volume.RegisterRGBDRobust(depths[k], with_color ? rgbs[k] : cv::Mat(), starts[k], static_cast<int>(batch_stride), &color_params, &options, &one[k])) return 1;
            batch_single_ms = Seconds(t0) * 1000.0;
        }
        for (long k = 0; k < K; ++k) batch_same = batch_same && std::memcmp(&many[k], &one[k], sizeof(one[k])) == 0;
    }
    if (coarse > 0) {
        std::printf("coarse 0: per iteration %.3f ms, final pose error %.3f mm / %.5f deg (max %.3f mm), rmse %.6f\n", Median(per_iteration_ms), Median(after_m) * 1000.0, Median(after_deg),
                    *std::max_element(after_m.begin(), after_m.end()) * 1000.0, Median(rmse));
        std::printf("coarse %ld: per iteration %.3f ms, final pose error %.3f mm / %.5f deg (max %.3f mm), rmse %.6f, %llu blocks, coarsening %.3f ms\n", coarse, Median(coarse_iteration_ms),
                    Median(coarse_after_m) * 1000.0, Median(coarse_after_deg), *std::max_element(coarse_after_m.begin(), coarse_after_m.end()) * 1000.0, Median(coarse_rmse), coarse_blocks,
                    Median(coarsen_ms));
    }
    std::cout << "{\"frames\": " << n << ", \"stride\": " << stride << ", \"first\": " << first << ", \"res\": " << res << ", \"path\": \"" << path << "\", \"registered\": " << frames
              << ", \"iters\": " << iters << ", \"iterations\": " << iterations << ", \"points\": " << points << ", \"used_last\": " << used
              << ", \"error_before\": {\"mm\": " << Median(before_m) * 1000.0 << ", \"deg\": " << Median(before_deg) << "}"
              << ", \"error_after\": {\"mm\": " << Median(after_m) * 1000.0 << ", \"deg\": " << Median(after_deg) << ", \"max_mm\": " << *std::max_element(after_m.begin(), after_m.end()) * 1000.0
              << ", \"max_deg\": " << *std::max_element(after_deg.begin(), after_deg.end()) << "}"
              << ", \"rmse\": {\"first\": " << Median(first_rmse) << ", \"final\": " << Median(rmse) << "}";
    if (with_color) std::cout << ", \"color_scale\": " << color_scale << ", \"rmse_color\": " << Median(rmse_color) << ", \"colored_last\": " << colored;
    if (robust) std::cout << ", \"linearization\": \"" << linearization << "\", \"huber\": " << huber << ", \"huber_color\": " << huber_color << ", \"downweighted_last\": " << downweighted
                          << ", \"rmse_residual\": " << Median(rmse_residual);
    if (batch > 0) std::cout << ", \"batch\": {\"frames\": " << std::min(batch, n) << ", \"pixel_stride\": " << batch_stride << ", \"ms\": " << batch_ms << ", \"single_ms\": " << batch_single_ms
                             << ", \"rounds\": " << batch_stats.rounds << ", \"launches\": " << batch_stats.launches << ", \"evaluations\": " << batch_stats.evaluations
                             << ", \"points\": " << batch_stats.points << ", \"same_bits\": " << (batch_same ? "true" : "false") << "}";
    if (coarse > 0) std::cout << ", \"coarse\": {\"levels\": " << coarse << ", \"blocks\": " << coarse_blocks << ", \"error_after\": {\"mm\": " << Median(coarse_after_m) * 1000.0 << ", \"deg\": "
                              << Median(coarse_after_deg) << ", \"max_mm\": " << *std::max_element(coarse_after_m.begin(), coarse_after_m.end()) * 1000.0 << "}, \"rmse\": " << Median(coarse_rmse)
                              << ", \"per_iteration_median\": " << Median(coarse_iteration_ms) << ", \"register_median\": " << Median(coarse_ms) << ", \"coarsen_median\": " << Median(coarsen_ms) << "}";
    std::cout
              << ", \"ms\": {\"fuse\": " << t_fuse * 1000.0 << ", \"deintegrate\": " << t_out * 1000.0 << ", \"reintegrate\": " << t_back * 1000.0
              << ", \"register_median\": " << Median(register_ms) << ", \"per_iteration_median\": " << Median(per_iteration_ms) << "}}" << std::endl;
    return 0;
}
