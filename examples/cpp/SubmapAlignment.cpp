// SubmapAlignment.cpp -- refining a submap's pose against the model it is about to be merged into.  The reference's submap flow
// (example/MergeMultipleSubmaps.cpp) reads fused submaps, Transforms each by a pose and Merges them; a submap merged a few centimetres off leaves a
// doubled surface.  Here K submaps are fused from overlapping ranges of the analytic room's frames at their true poses (so every submap's true
// transformation is the identity), the poses of submaps 1..K-1 are moved by 3-4 cm and about a degree, each is registered against the model merged
// so far, and Transform + Merge fix it at the pose that was found.
//
//   SubmapAlignment --synthetic N STRIDE SEED [--submaps K] [--overlap F] [--perturb P] [--res R] [--band B] [--voxel-stride S] [--iters I]
//                   [--linearization normal|gradient|metric] [--color on|off] [--path cloud|mesh|volume] [--merge two-step|fused]
//                   [--recompose single|batch] [--out DIR]
//   --synthetic N STRIDE SEED  N frames of the analytic room of LiveFusion.cpp: frame k is step FIRST + k * STRIDE of a 1000-step orbit, SEED picks FIRST
//   --submaps K                (default 2) submap i holds the frames [i * step, i * step + L), L = N / (K - (K - 1) F), step = L (1 - F)
//   --overlap F                (default 0.4) the share of a submap's frames that the next one holds too
//   --perturb P                (default 1) submap i starts at the drifted pose number P + i (a rotation of about a degree about y, a shift of 3-4 cm)
//   --path volume (default)    CubeHandler::RegisterVolume (op_volume_register_volume): the submap's band voxels, selected on the device, each with its
//                              own sdf as the value the model's field should have there; --band B (metres; default 0 = two voxels, negative = the
//                              truncation) and --voxel-stride S (default 1) choose them; --color on (default) adds the colour term
//   --path cloud               the route there was before: GetPointCloud() of the submap -- its whole truncation band, as if it lay on the surface --
//                              through RegisterPointCloudRobust (no colour: GetPointCloud's colours are |sdf| / truncation)
//   --path mesh                the other one: ExtractTriangleMesh of the submap, its vertices through RegisterPointCloudRobust (--color on: their colours)
//   --linearization L          (default gradient)   --iters I  Gauss-Newton iterations at the most (default 30; min_step 1e-5)
//   --merge two-step (default) Merge(part, T): Transform into an intermediate volume, then Merge, as example/MergeMultipleSubmaps.cpp places a submap
//   --merge fused              MergeTransformed(part, T) (op_volume_merge_transformed): the same voxels, resampled straight into the model's blocks
//   --recompose single|batch   after the loop a fresh, empty model receives ALL submaps at their final poses (submap 0 at the identity), as a system
//                              that re-composes its global model after a pose-graph update does: K MergeTransformed calls, or one call with K sources
//   --out DIR                  writes model_<i>.map (the model submap i was registered against), submap_<i>.map, the final model.map and, with
//                              --recompose, recomposed.map
// One line per submap (pose error before and after, points, iterations, status, times), then one JSON line with the same, the stage times and the
// doubled-surface figure: the rmse of the distance (DistanceToModel) of the merged model's mesh vertices to a model fused from all frames at their
// true poses.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "Geometry/Geometry.h"
#include "Geometry/PointCloud.h"
#include "Geometry/TriangleMesh.h"
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

// a drifted estimate number k of the identity: a rotation of about a degree about y, a shift of 3-4 cm; deterministic
geometry::TransformationMatrix Perturbed(long k) {
    const double a = 0.015 + 0.002 * static_cast<double>(k % 3);
    geometry::TransformationMatrix T = geometry::TransformationMatrix::Identity();
    T(0, 0) = static_cast<float>(std::cos(a)); T(0, 2) = static_cast<float>(std::sin(a));
    T(2, 0) = static_cast<float>(-std::sin(a)); T(2, 2) = static_cast<float>(std::cos(a));
    T(0, 3) = 0.03f; T(1, 3) = -0.02f + 0.005f * static_cast<float>(k % 2); T(2, 3) = 0.025f;
    return T;
}

// distance of T from the identity: of the origins in metres, of the rotations in degrees
void PoseError(const geometry::TransformationMatrix& T, double* metres, double* degrees) {
    double d2 = 0, trace = 0;
    for (int r = 0; r < 3; ++r) {
        d2 += static_cast<double>(T(r, 3)) * T(r, 3);
        trace += static_cast<double>(T(r, r));
    }
    *metres = std::sqrt(d2);
    *degrees = std::acos(std::fmax(-1.0, std::fmin(1.0, (trace - 1.0) / 2.0))) * 180.0 / kPi;
}

void PrintMatrix(const geometry::TransformationMatrix& T) {
    std::printf("[");
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) std::printf("%s%.9g", r + c ? ", " : "", static_cast<double>(T(r, c)));
    std::printf("]");
}

struct Row {
    geometry::TransformationMatrix start, T;
    double before_mm, before_deg, after_mm, after_deg, select_ms, register_ms, merge_ms, rmse, rmse_residual;
    unsigned long long points, used, first_used, colored;
    int iterations, status;
};

} // namespace

int main(int argc, char* argv[]) {
    long synthetic[3] = {0, 1, 1}, submaps = 2, perturb = 1, voxel_stride = 1, iters = 30;
    bool is_synthetic = false, bad = false;
    std::string path = "volume", color = "on", linearization = "gradient", out_dir, merge = "two-step", recompose;
    float res = 0.01f, band = 0.0f, overlap = 0.4f;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--synthetic" && i + 3 < argc) { is_synthetic = true; for (int k = 0; k < 3; ++k) synthetic[k] = std::atol(argv[++i]); }
        else if (a == "--submaps" && i + 1 < argc) submaps = std::atol(argv[++i]);
        else if (a == "--overlap" && i + 1 < argc) overlap = static_cast<float>(std::atof(argv[++i]));
        else if (a == "--perturb" && i + 1 < argc) perturb = std::atol(argv[++i]);
        else if (a == "--res" && i + 1 < argc) res = static_cast<float>(std::atof(argv[++i]));
        else if (a == "--band" && i + 1 < argc) band = static_cast<float>(std::atof(argv[++i]));
        else if (a == "--voxel-stride" && i + 1 < argc) voxel_stride = std::atol(argv[++i]);
        else if (a == "--iters" && i + 1 < argc) iters = std::atol(argv[++i]);
        else if (a == "--linearization" && i + 1 < argc) linearization = argv[++i];
        else if (a == "--color" && i + 1 < argc) color = argv[++i];
        else if (a == "--path" && i + 1 < argc) path = argv[++i];
        else if (a == "--merge" && i + 1 < argc) merge = argv[++i];
        else if (a == "--recompose" && i + 1 < argc) recompose = argv[++i];
        else if (a == "--out" && i + 1 < argc) out_dir = argv[++i];
        else bad = true;
    }
    const int lin = linearization == "normal" ? OP_REGISTER_LIN_NORMAL : linearization == "gradient" ? OP_REGISTER_LIN_GRADIENT : linearization == "metric" ? OP_REGISTER_LIN_METRIC : -1;
    const long n = synthetic[0], stride = synthetic[1];
    if (bad || !is_synthetic || n < 1 || stride < 1 || synthetic[2] < 0 || submaps < 2 || submaps > n || !(overlap >= 0) || !(overlap < 1) || perturb < 0 || !(res > 0) ||
        !(band == band) || (voxel_stride != 1 && voxel_stride != 2 && voxel_stride != 4 && voxel_stride != 8) || iters < 0 || iters > 1000 || lin < 0 ||
        (color != "off" && color != "on") || (path != "cloud" && path != "mesh" && path != "volume") ||
        (merge != "two-step" && merge != "fused") || (!recompose.empty() && recompose != "single" && recompose != "batch")) {
        std::cout << "usage::SubmapAlignment --synthetic N STRIDE SEED [--submaps K] [--overlap F] [--perturb P] [--res R] [--band B] [--voxel-stride S] [--iters I]"
                     " [--linearization normal|gradient|metric] [--color on|off] [--path cloud|mesh|volume] [--merge two-step|fused] [--recompose single|batch] [--out DIR]" << std::endl;
        return bad || argc > 1 ? 2 : 0;
    }
    const long first = ((synthetic[2] + 999) % 1000) * 97 % 1000;
    const bool with_color = color == "on" && path != "cloud";
    const long length = std::max(1L, std::min(n, static_cast<long>(std::ceil(static_cast<double>(n) / (static_cast<double>(submaps) - static_cast<double>(submaps - 1) * overlap)))));

    camera::PinholeCamera camera;
    camera.SetCameraType(camera::CameraType::OPEN3D_DATASET);
    // the frames once, the K submaps and the model every frame belongs to, all at the true poses
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    std::vector<cv::Mat> depths(n), rgbs(n);
    std::vector<geometry::TransformationMatrix> poses(n);
    for (long k = 0; k < n; ++k) {
        poses[k] = RoomPose(first + k * stride);
        RoomRender(poses[k], camera, depths[k], rgbs[k]);
    }
    const double t_render = Seconds(t0);
    t0 = std::chrono::steady_clock::now();
    integration::CubeHandler truth(camera);
    truth.SetVoxelResolution(res);
    if (!truth.Handle()) return 1; // (no device: the class has said so)
    for (long k = 0; k < n; ++k) truth.IntegrateImage(depths[k], rgbs[k], poses[k]);
    truth.Synchronize();
    std::vector<std::shared_ptr<integration::CubeHandler> > owned(submaps);
    std::vector<long> begin(submaps), end(submaps);
    for (long i = 0; i < submaps; ++i) {
        begin[i] = submaps > 1 ? std::min(n - length, static_cast<long>(std::floor(static_cast<double>(i) * static_cast<double>(n - length) / static_cast<double>(submaps - 1) + 0.5))) : 0;
        end[i] = begin[i] + length;
        owned[i] = std::make_shared<integration::CubeHandler>(camera);
        integration::CubeHandler& part = *owned[i];
        part.SetVoxelResolution(res);
        for (long k = begin[i]; k < end[i]; ++k) part.IntegrateImage(depths[k], rgbs[k], poses[k]);
        part.Synchronize();
    }
    const double t_fuse = Seconds(t0);

    op_volume_band_params sel;
    if (op_volume_band_default_params(owned[0]->Handle(), &sel) != OP_OK) return 1;
    if (band > 0) sel.band = band;
    else if (band < 0) sel.band = 0.0f; // the truncation
    sel.voxel_stride = static_cast<int>(voxel_stride);
    op_volume_register_color_params params;
    if (op_volume_register_color_default_params(owned[0]->Handle(), &params) != OP_OK) return 1;
    params.base.max_iterations = static_cast<int>(iters);
    params.color_scale = with_color ? 1.0f : 0.0f;
    op_volume_register_options options;
    options.linearization = lin; options.huber = 0.0f; options.huber_color = 0.0f;
    const char* const status_names[4] = {"converged", "max_iterations", "too_few_points", "singular"};

    // submap 0 becomes the model the others are merged into: the re-composition needs it as it was
    std::shared_ptr<integration::CubeHandler> first_submap;
    if (!recompose.empty()) first_submap = std::make_shared<integration::CubeHandler>(*owned[0]);
    integration::CubeHandler& model = *owned[0];
    std::vector<Row> rows;
    op_volume_merge_transformed_stats merge_stats = op_volume_merge_transformed_stats(); // --merge fused: summed over the submaps
    for (long i = 1; i < submaps; ++i) {
        Row row = Row();
        integration::CubeHandler& part = *owned[i];
        row.start = Perturbed(perturb + i);
        PoseError(row.start, &row.before_mm, &row.before_deg);
        if (!out_dir.empty()) {
            if (!model.WriteToFile(out_dir + "/model_" + std::to_string(i) + ".map") || !part.WriteToFile(out_dir + "/submap_" + std::to_string(i) + ".map")) return 1;
        }
        op_volume_register_robust_result got = op_volume_register_robust_result();
        if (path == "volume") {
            size_t count = 0; // the selection alone, to time it: the registration below selects again
            t0 = std::chrono::steady_clock::now();
            if (op_volume_band_voxels(part.Handle(), &sel, nullptr, nullptr, nullptr, OP_MEM_HOST, 0, &count) != OP_OK) return 1;
            row.select_ms = Seconds(t0) * 1000.0;
            op_volume_register_volume_result r;
            t0 = std::chrono::steady_clock::now();
            if (!model.RegisterVolume(part, row.start, &sel, &params, &options, &r)) return 1;
            row.register_ms = Seconds(t0) * 1000.0;
            got = r.robust;
            row.points = r.selected;
        } else {
            geometry::PointCloud pcd;
            t0 = std::chrono::steady_clock::now();
            if (path == "cloud") {
                pcd = *part.GetPointCloud();
                pcd.colors.clear(); // (|sdf| / truncation: no colour of the scene)
            } else {
                geometry::TriangleMesh mesh;
                part.ExtractTriangleMesh(mesh);
                pcd.points = mesh.points;
                if (with_color) pcd.colors = mesh.colors;
            }
            row.select_ms = Seconds(t0) * 1000.0;
            row.points = pcd.points.size();
            t0 = std::chrono::steady_clock::now();
            if (!model.RegisterPointCloudRobust(pcd, row.start, &params, &options, &got)) return 1;
            row.register_ms = Seconds(t0) * 1000.0;
        }
        const op_volume_register_result& b = got.color.base;
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) row.T(r, c) = b.T[4 * r + c];
        row.iterations = b.iterations; row.status = b.status; row.used = b.used; row.first_used = b.first_used; row.colored = got.color.colored;
        row.rmse = b.rmse; row.rmse_residual = got.rmse_residual;
        PoseError(row.T, &row.after_mm, &row.after_deg);
        t0 = std::chrono::steady_clock::now();
        if (merge == "fused") {
            op_volume_merge_transformed_stats ms;
            model.MergeTransformed(part, row.T, &ms);
            merge_stats.sources += ms.sources; merge_stats.src_blocks += ms.src_blocks; merge_stats.touched_blocks += ms.touched_blocks;
            merge_stats.created_blocks += ms.created_blocks; merge_stats.pairs += ms.pairs; merge_stats.voxels_copied += ms.voxels_copied;
            merge_stats.voxels_kept += ms.voxels_kept; merge_stats.voxels_blended += ms.voxels_blended; merge_stats.voxels_reset += ms.voxels_reset;
        } else {
            model.Merge(part, row.T); // Transform + Merge, as example/MergeMultipleSubmaps.cpp places a submap
        }
        model.Synchronize();
        row.merge_ms = Seconds(t0) * 1000.0;
        std::printf("submap %ld (frames %ld..%ld): pose error %.3f mm / %.5f deg -> %.3f mm / %.5f deg, %llu points, %llu used, %d iterations, status %s, rmse %.6f, residual rmse %.6f, "
                    "select %.3f ms, register %.3f ms, merge %.3f ms\n", i, begin[i], end[i] - 1, row.before_mm * 1000.0, row.before_deg, row.after_mm * 1000.0, row.after_deg, row.points,
                    row.used, row.iterations, status_names[row.status & 3], row.rmse, row.rmse_residual, row.select_ms, row.register_ms, row.merge_ms);
        rows.push_back(row);
    }
    if (!out_dir.empty() && !model.WriteToFile(out_dir + "/model.map")) return 1;
    // the global model composed again from all submaps at their final poses, into a fresh volume
    double recompose_ms = 0.0;
    op_volume_merge_transformed_stats recompose_stats = op_volume_merge_transformed_stats();
    if (!recompose.empty()) {
        std::vector<const integration::CubeHandler*> parts(1, first_submap.get());
        std::vector<geometry::TransformationMatrix> at(1, geometry::TransformationMatrix::Identity());
        for (long i = 1; i < submaps; ++i) { parts.push_back(owned[i].get()); at.push_back(rows[i - 1].T); }
        integration::CubeHandler global(camera);
        global.SetVoxelResolution(res);
        if (!global.Handle()) return 1;
        global.Synchronize();
        t0 = std::chrono::steady_clock::now();
        if (recompose == "batch") {
            global.MergeTransformed(parts, at, &recompose_stats);
        } else {
            for (size_t k = 0; k < parts.size(); ++k) {
                op_volume_merge_transformed_stats ms;
                global.MergeTransformed(*parts[k], at[k], &ms);
                recompose_stats.sources += ms.sources; recompose_stats.src_blocks += ms.src_blocks; recompose_stats.touched_blocks += ms.touched_blocks;
                recompose_stats.created_blocks += ms.created_blocks; recompose_stats.pairs += ms.pairs; recompose_stats.voxels_copied += ms.voxels_copied;
                recompose_stats.voxels_kept += ms.voxels_kept; recompose_stats.voxels_blended += ms.voxels_blended; recompose_stats.voxels_reset += ms.voxels_reset;
            }
        }
        global.Synchronize();
        recompose_ms = Seconds(t0) * 1000.0;
        std::printf("recompose %s: %zu submaps, %llu blocks touched, %.3f ms\n", recompose.c_str(), parts.size(), static_cast<unsigned long long>(recompose_stats.touched_blocks), recompose_ms);
        if (!out_dir.empty() && !global.WriteToFile(out_dir + "/recomposed.map")) return 1;
    }
    // the doubled surface: how far the merged model's mesh lies from the model every frame was fused into at its true pose
    t0 = std::chrono::steady_clock::now();
    geometry::TriangleMesh merged;
    model.ExtractTriangleMesh(merged);
    geometry::PointCloud vertices;
    vertices.points = merged.points;
    const op_volume_sample_stats st = truth.DistanceToModel(vertices);
    const double t_figure = Seconds(t0);
    const double doubled = st.valid ? std::sqrt(st.sum_sq_sdf / static_cast<double>(st.valid)) : 0.0;

    std::printf("{\"frames\": %ld, \"stride\": %ld, \"first\": %ld, \"res\": %g, \"submaps\": %ld, \"length\": %ld, \"overlap\": %g, \"path\": \"%s\", \"color\": \"%s\", "
                "\"linearization\": \"%s\", \"band\": %.9g, \"voxel_stride\": %ld, \"iters\": %ld, \"merge\": \"%s\", \"recompose\": \"%s\", \"recompose_ms\": %g, ", n, stride, first, static_cast<double>(res), submaps, length,
                static_cast<double>(overlap), path.c_str(), with_color ? "on" : "off", linearization.c_str(), static_cast<double>(sel.band), voxel_stride, iters, merge.c_str(), recompose.empty() ? "none" : recompose.c_str(), recompose_ms);
    const op_volume_merge_transformed_stats* const both[2] = {&merge_stats, &recompose_stats};
    for (int k = 0; k < 2; ++k) // (touched_blocks of --recompose single and of --merge fused: summed per call, not a union)
        std::printf("\"%s\": {\"sources\": %llu, \"src_blocks\": %llu, \"touched_blocks\": %llu, \"created_blocks\": %llu, \"pairs\": %llu, \"voxels_copied\": %llu, "
                    "\"voxels_kept\": %llu, \"voxels_blended\": %llu, \"voxels_reset\": %llu}, ", k ? "recompose_stats" : "merge_stats",
                    static_cast<unsigned long long>(both[k]->sources), static_cast<unsigned long long>(both[k]->src_blocks), static_cast<unsigned long long>(both[k]->touched_blocks),
                    static_cast<unsigned long long>(both[k]->created_blocks), static_cast<unsigned long long>(both[k]->pairs), static_cast<unsigned long long>(both[k]->voxels_copied),
                    static_cast<unsigned long long>(both[k]->voxels_kept), static_cast<unsigned long long>(both[k]->voxels_blended), static_cast<unsigned long long>(both[k]->voxels_reset));
    std::printf("\"registered\": [");
    for (size_t k = 0; k < rows.size(); ++k) {
        const Row& r = rows[k];
        std::printf("%s{\"submap\": %zu, \"points\": %llu, \"used\": %llu, \"first_used\": %llu, \"colored\": %llu, \"iterations\": %d, \"status\": %d, \"rmse\": %.17g, "
                    "\"rmse_residual\": %.17g, \"error_before\": {\"mm\": %g, \"deg\": %g}, \"error_after\": {\"mm\": %g, \"deg\": %g}, \"ms\": {\"select\": %g, \"register\": %g, "
                    "\"per_iteration\": %g, \"merge\": %g}, \"start\": ", k ? ", " : "", k + 1, r.points, r.used, r.first_used, r.colored, r.iterations, r.status, r.rmse, r.rmse_residual,
                    r.before_mm * 1000.0, r.before_deg, r.after_mm * 1000.0, r.after_deg, r.select_ms, r.register_ms, r.register_ms / static_cast<double>(r.iterations + 1), r.merge_ms);
        PrintMatrix(r.start);
        std::printf(", \"T\": ");
        PrintMatrix(r.T);
        std::printf("}");
    }
    std::printf("], \"doubled_surface\": {\"rmse_mm\": %g, \"max_mm\": %g, \"vertices\": %llu, \"valid\": %llu}, \"ms\": {\"render\": %g, \"fuse\": %g, \"figure\": %g}}\n", doubled * 1000.0,
                static_cast<double>(st.max_abs_sdf) * 1000.0, static_cast<unsigned long long>(st.queries), static_cast<unsigned long long>(st.valid), t_render * 1000.0, t_fuse * 1000.0,
                t_figure * 1000.0);
    return 0;
}
