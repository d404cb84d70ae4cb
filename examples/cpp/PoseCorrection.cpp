// PoseCorrection.cpp -- using a corrected pose of a frame that is already fused.  N frames of the analytic room are fused, K of them at a perturbed
// (drifted) pose; then the volume is repaired, either the only way there was before de-integration -- Clear() and fusing all N frames again at the
// true poses -- or by moving the K frames: CubeHandler::ReintegrateImage(depth, rgb, drifted pose, true pose), about 2 K frame updates.
//
//   PoseCorrection --synthetic N STRIDE SEED [--perturb K] [--res 0.01] [--path refuse|reintegrate|split] [--runs R]
//   --synthetic N STRIDE SEED  N frames of the analytic room of LiveFusion.cpp: frame k is step FIRST + k * STRIDE of a 1000-step orbit, SEED picks FIRST
//   --perturb K                K of the N frames (evenly spread) are first fused 3 cm and about one degree off (default N / 10, at least 1)
//   --res                      voxel size in metres
//   --path                     refuse (default): Clear() + IntegrateImage of all N frames; reintegrate: ReintegrateImage of the K frames
//                              split: DeintegrateImage of the K frames, then IntegrateImage of the K frames (the two kernels side by side under a profiler)
//   --runs R                   R > 1: one untimed pass and R timed ones in this process (the volume cleared in between); the medians are printed
//   --collect none|device|roundtrip   after the repair (--path defaults to reintegrate then) the blocks it emptied are freed: device = CubeHandler::CollectGarbage(),
//                              roundtrip = what there was before it (download, filter on the host, Clear(), upload), none = they stay.  The JSON gains
//                              "collect": block counts before and after, the collection's time (median over the runs) and the times of one ExtractTriangleMesh, one
//                              RenderFrame and one WriteToFile over the volume as it is then
//   --dump FILE                with --collect: the final volume as (key, block) records sorted by key (device and roundtrip write equal files)
//   --path refine              the K poses are not handed over but FOUND: the K frames are registered against the volume they were fused into, each
//                              from its drifted pose (op_volume_register_robust_frame's loop), and then moved to the estimates by
//                              op_volume_reintegrate_sequence.  The K frames are brought to the device once, before the clock starts.
//     --refine single|batch    single (default): one op_volume_register_robust_frame call per frame; batch: one op_volume_register_batch_frames call
//                              for all K -- the same poses bit for bit (with --dump FILE both write the same file: K x 16 numbers)
//     --stride S --iters I --linearization normal|gradient|metric --color on|off   pixel stride (4), iterations at most (10), linearisation (metric),
//                              colour term (off) of the registration
//                              The JSON gains "refine": the estimate's and the move's times, the pose errors of the K frames before and after
//                              against the synthetic truth, and for batch the rounds, launches and evaluations of the call
// It prints one JSON line: the stage times (host clock, each stage waited for) and, against a second volume fused at the true poses, the number of
// voxels whose weights differ and the largest |sdf| and |colour| differences over the others.  A re-fused volume is that volume bit for bit; a
// re-integrated one has the same weights and differs by the float32 roundings of the inverse running mean (op_volume_deintegrate).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <string>
#include <vector>

#include "Geometry/Geometry.h"
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

// a drifted estimate of `pose`: 3 cm and about a degree off, the direction depending on k
geometry::TransformationMatrix Drifted(const geometry::TransformationMatrix& pose, long k) {
    const double a = 0.015 + 0.002 * static_cast<double>(k % 3);
    geometry::TransformationMatrix D = geometry::TransformationMatrix::Identity();
    D(0, 0) = static_cast<float>(std::cos(a)); D(0, 2) = static_cast<float>(std::sin(a));
    D(2, 0) = static_cast<float>(-std::sin(a)); D(2, 2) = static_cast<float>(std::cos(a));
    D(0, 3) = 0.03f; D(1, 3) = k % 2 ? -0.015f : -0.02f; D(2, 3) = 0.025f;
    return pose * D;
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

struct Blocks {
    std::vector<int32_t> keys;
    std::vector<float> vox; // n x 512 x {sdf, weight, c0, c1, c2}
    size_t n;
};

bool Download(integration::CubeHandler& h, Blocks* out) {
    op_volume* v = h.Handle();
    size_t n = 0, got = 0;
    if (!v || op_volume_block_count(v, &n) != OP_OK) return false;
    out->keys.resize(3 * n + 3);
    out->vox.resize(n * 512 * 5 + 5);
    if (n && op_volume_download(v, out->keys.data(), out->vox.data(), n, &got) != OP_OK) return false;
    out->n = n ? got : 0;
    return true;
}

// The route there was before CubeHandler::CollectGarbage: the whole pool to the host, the blocks without a voxel of weight > 0 taken out there,
// Clear(), and the rest uploaded again.
bool CollectByRoundTrip(integration::CubeHandler& h) {
    Blocks all;
    if (!Download(h, &all)) return false;
    size_t kept = 0;
    for (size_t b = 0; b < all.n; ++b) {
        bool observed = false;
        for (int i = 0; i < 512 && !observed; ++i) observed = all.vox[b * 2560 + 5 * i + 1] > 0.0f;
        if (!observed) continue;
        if (kept != b) {
            std::copy(all.keys.begin() + 3 * b, all.keys.begin() + 3 * b + 3, all.keys.begin() + 3 * kept);
            std::copy(all.vox.begin() + b * 2560, all.vox.begin() + (b + 1) * 2560, all.vox.begin() + kept * 2560);
        }
        ++kept;
    }
    h.Clear();
    return kept == 0 || op_volume_upload(h.Handle(), all.keys.data(), all.vox.data(), kept) == OP_OK;
}

// (key, block) records sorted by key: equal files = equal volumes as sets of blocks
bool Dump(integration::CubeHandler& h, const std::string& file) {
    Blocks all;
    if (!Download(h, &all)) return false;
    std::vector<size_t> order(all.n);
    for (size_t b = 0; b < all.n; ++b) order[b] = b;
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return std::lexicographical_compare(all.keys.begin() + 3 * a, all.keys.begin() + 3 * a + 3, all.keys.begin() + 3 * b, all.keys.begin() + 3 * b + 3); });
    FILE* f = fopen(file.c_str(), "wb");
    if (!f) return false;
    for (size_t i = 0; i < all.n; ++i) {
        fwrite(&all.keys[3 * order[i]], sizeof(int32_t), 3, f);
        fwrite(&all.vox[order[i] * 2560], sizeof(float), 2560, f);
    }
    return fclose(f) == 0;
}

} // namespace

int main(int argc, char* argv[]) {
    long synthetic[3] = {0, 1, 1}, perturb = -1, runs = 1;
    bool is_synthetic = false, bad = false, path_given = false;
    std::string path = "refuse", collect, dump, refine = "single", linearization = "metric", color = "off";
    long pixel_stride = 4, iters = 10;
    float res = 0.01f;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--synthetic" && i + 3 < argc) { is_synthetic = true; for (int k = 0; k < 3; ++k) synthetic[k] = std::atol(argv[++i]); }
        else if (a == "--perturb" && i + 1 < argc) perturb = std::atol(argv[++i]);
        else if (a == "--res" && i + 1 < argc) res = static_cast<float>(std::atof(argv[++i]));
        else if (a == "--path" && i + 1 < argc) { path = argv[++i]; path_given = true; }
        else if (a == "--runs" && i + 1 < argc) runs = std::atol(argv[++i]);
        else if (a == "--collect" && i + 1 < argc) collect = argv[++i];
        else if (a == "--dump" && i + 1 < argc) dump = argv[++i];
        else if (a == "--refine" && i + 1 < argc) refine = argv[++i];
        else if (a == "--stride" && i + 1 < argc) pixel_stride = std::atol(argv[++i]);
        else if (a == "--iters" && i + 1 < argc) iters = std::atol(argv[++i]);
        else if (a == "--linearization" && i + 1 < argc) linearization = argv[++i];
        else if (a == "--color" && i + 1 < argc) color = argv[++i];
        else bad = true;
    }
    if (!collect.empty() && !path_given) path = "reintegrate"; // a re-fused volume has nothing to collect
    const long n = synthetic[0], stride = synthetic[1];
    if (perturb < 0) perturb = n / 10 > 0 ? n / 10 : 1;
    if (bad || !is_synthetic || n < 1 || stride < 1 || synthetic[2] < 0 || perturb < 1 || perturb > n || !(res > 0) || runs < 1 || (path != "refuse" && path != "reintegrate" && path != "split" && path != "refine") ||
        (refine != "single" && refine != "batch") || pixel_stride < 1 || iters < 0 || (linearization != "normal" && linearization != "gradient" && linearization != "metric") ||
        (color != "on" && color != "off") ||
        (!collect.empty() && collect != "none" && collect != "device" && collect != "roundtrip")) {
        std::cout << "usage::PoseCorrection --synthetic N STRIDE SEED [--perturb K] [--res 0.01] [--path refuse|reintegrate|split|refine] [--runs R] [--collect none|device|roundtrip] [--dump FILE] "
                     "[--refine single|batch] [--stride S] [--iters I] [--linearization normal|gradient|metric] [--color on|off]" << std::endl;
        return bad || argc > 1 ? 2 : 0;
    }
    const long first = ((synthetic[2] + 999) % 1000) * 97 % 1000;

    camera::PinholeCamera camera;
    camera.SetCameraType(camera::CameraType::OPEN3D_DATASET);
    std::vector<cv::Mat> depth(n), rgb(n);
    std::vector<geometry::TransformationMatrix> truth(n), fused_at(n);
    std::vector<char> moved(n, 0);
    for (long k = 0; k < perturb; ++k) moved[(2 * k + 1) * n / (2 * perturb)] = 1; // K frames, evenly spread
    for (long k = 0; k < n; ++k) {
        truth[k] = RoomPose(first + k * stride);
        RoomRender(truth[k], camera, depth[k], rgb[k]);
        fused_at[k] = moved[k] ? Drifted(truth[k], k) : truth[k];
    }

    integration::CubeHandler volume(camera), reference(camera);
    volume.SetVoxelResolution(res);
    reference.SetVoxelResolution(res);
    if (!volume.Handle()) return 1; // (no device: the class has said so)

    // --path refine: the K frames side by side on the device (frame j at j * bytes of an image), their drifted poses, and what the registration is told
    const size_t npix = static_cast<size_t>(camera.GetWidth()) * static_cast<size_t>(camera.GetHeight()), dbytes = npix * sizeof(float), cbytes = npix * 3;
    const char* dev_env = std::getenv("ONEPIECE_HIP_DEVICE");
    const int device = dev_env ? std::atoi(dev_env) : 0;
    void *d_depth = nullptr, *d_rgb = nullptr;
    std::vector<long> moved_index;
    std::vector<float> old_poses, new_poses;
    op_volume_register_color_params reg_params;
    op_volume_register_options reg_options;
    op_volume_register_batch_stats reg_stats = op_volume_register_batch_stats();
    std::vector<double> estimate_s, move_s;
    if (path == "refine") {
        std::vector<unsigned char> hd, hc;
        for (long k = 0; k < n; ++k) {
            if (!moved[k]) continue;
            moved_index.push_back(k);
            hd.insert(hd.end(), depth[k].data, depth[k].data + dbytes);
            hc.insert(hc.end(), rgb[k].data, rgb[k].data + cbytes);
            for (int r = 0; r < 4; ++r)
                for (int c = 0; c < 4; ++c) old_poses.push_back(fused_at[k](r, c));
        }
        new_poses = old_poses;
        if (op_device_upload(hd.data(), hd.size(), device, &d_depth) != OP_OK || op_device_upload(hc.data(), hc.size(), device, &d_rgb) != OP_OK ||
            op_volume_register_color_default_params(volume.Handle(), &reg_params) != OP_OK) {
            std::cout << RED << "[ERROR]::cannot bring the frames to the device: " << op_last_error() << RESET << std::endl;
            return 1;
        }
        reg_params.base.max_iterations = static_cast<int>(iters);
        if (color == "off") reg_params.color_scale = 0.0f;
        reg_options.linearization = linearization == "normal" ? OP_REGISTER_LIN_NORMAL : linearization == "gradient" ? OP_REGISTER_LIN_GRADIENT : OP_REGISTER_LIN_METRIC;
        reg_options.huber = 0.0f; reg_options.huber_color = 0.0f;
    }

    // with --runs R > 1: one untimed pass, then R timed ones (the volume cleared in between); the medians are reported
    std::vector<double> fuse_s, repair_s, collect_s;
    size_t blocks_drifted = 0, blocks_repaired = 0;
    std::chrono::steady_clock::time_point t0;
    for (long pass = runs > 1 ? -1 : 0; pass < runs; ++pass) {
        volume.Clear();
        t0 = std::chrono::steady_clock::now();
        for (long k = 0; k < n; ++k) volume.IntegrateImage(depth[k], rgb[k], fused_at[k]);
        volume.Synchronize();
        const double tf = Seconds(t0);
        blocks_drifted = volume.GetCubeCount();
        t0 = std::chrono::steady_clock::now();
        if (path == "refuse") {
            volume.Clear();
            for (long k = 0; k < n; ++k) volume.IntegrateImage(depth[k], rgb[k], truth[k]);
        } else if (path == "reintegrate") {
            for (long k = 0; k < n; ++k)
                if (moved[k]) volume.ReintegrateImage(depth[k], rgb[k], fused_at[k], truth[k]);
        } else if (path == "refine") { // find the K poses (the queue is flushed by the first registration call), then move the frames there
            const size_t K = moved_index.size();
            const op_camera pod = camera.Pod();
            const uint8_t* c_rgb = color == "on" ? static_cast<const uint8_t*>(d_rgb) : nullptr;
            std::vector<op_volume_register_robust_result> found(K);
            int rc = OP_OK;
            if (refine == "batch") {
                rc = op_volume_register_batch_frames(volume.Handle(), &pod, d_depth, dbytes, OP_DEPTH_F32, c_rgb, cbytes, OP_MEM_DEVICE, static_cast<int>(pixel_stride),
                                                     old_poses.data(), K, &reg_params, &reg_options, found.data(), &reg_stats);
            } else {
                for (size_t j = 0; j < K && rc == OP_OK; ++j)
                    rc = op_volume_register_robust_frame(volume.Handle(), &pod, static_cast<const unsigned char*>(d_depth) + j * dbytes, OP_DEPTH_F32, c_rgb ? c_rgb + j * cbytes : nullptr,
                                                         OP_MEM_DEVICE, static_cast<int>(pixel_stride), old_poses.data() + 16 * j, &reg_params, &reg_options, &found[j]);
            }
            if (rc != OP_OK) { std::cout << RED << "[ERROR]::registration failed: " << op_last_error() << RESET << std::endl; return 1; }
            const double te = Seconds(t0);
            for (size_t j = 0; j < K; ++j) std::copy(found[j].color.base.T, found[j].color.base.T + 16, new_poses.begin() + 16 * j);
            const std::chrono::steady_clock::time_point t1 = std::chrono::steady_clock::now();
            if (op_volume_reintegrate_sequence(volume.Handle(), d_depth, dbytes, OP_DEPTH_F32, static_cast<const uint8_t*>(d_rgb), cbytes, old_poses.data(), new_poses.data(), K) != OP_OK) {
                std::cout << RED << "[ERROR]::re-integration failed: " << op_last_error() << RESET << std::endl;
                return 1;
            }
            volume.Synchronize();
            if (pass >= 0) { estimate_s.push_back(te); move_s.push_back(Seconds(t1)); }
        } else { // split: the K de-integrations in launches of their own, then the K frames through the ordinary integration of a volume that is no longer plain
            for (long k = 0; k < n; ++k)
                if (moved[k]) volume.DeintegrateImage(depth[k], rgb[k], fused_at[k]);
            volume.Synchronize();
            for (long k = 0; k < n; ++k)
                if (moved[k]) volume.IntegrateImage(depth[k], rgb[k], truth[k]);
        }
        volume.Synchronize();
        const double tr = Seconds(t0);
        double tc = 0;
        if (!collect.empty()) { // the blocks the repair emptied: freed on the device, or by the route there was before (download, filter, Clear, upload)
            blocks_repaired = volume.GetCubeCount();
            t0 = std::chrono::steady_clock::now();
            if (collect == "device") volume.CollectGarbage();
            else if (collect == "roundtrip" && !CollectByRoundTrip(volume)) { std::cout << RED << "[ERROR]::round trip failed: " << op_last_error() << RESET << std::endl; return 1; }
            volume.Synchronize();
            tc = Seconds(t0);
        }
        if (pass >= 0) { fuse_s.push_back(tf); repair_s.push_back(tr); collect_s.push_back(tc); }
    }
    std::sort(fuse_s.begin(), fuse_s.end());
    std::sort(repair_s.begin(), repair_s.end());
    std::sort(collect_s.begin(), collect_s.end());
    const double t_fuse = fuse_s[fuse_s.size() / 2], t_repair = repair_s[repair_s.size() / 2], t_collect = collect_s[collect_s.size() / 2];

    // one pass of three consumers over the volume as the collection left it (with --collect none: over the volume with its empty blocks)
    double t_mesh = 0, t_render = 0, t_write = 0;
    size_t blocks_collected = 0, triangles = 0, rendered = 0;
    if (!collect.empty()) {
        blocks_collected = volume.GetCubeCount();
        t0 = std::chrono::steady_clock::now();
        geometry::TriangleMesh mesh;
        volume.ExtractTriangleMesh(mesh);
        t_mesh = Seconds(t0);
        triangles = mesh.GetTriangleSize();
        t0 = std::chrono::steady_clock::now();
        cv::Mat view_rgb, view_depth;
        rendered = volume.RenderFrame(truth[n / 2], view_rgb, view_depth);
        t_render = Seconds(t0);
        const char* tmp = std::getenv("TMPDIR");
        const std::string map_file = std::string(tmp ? tmp : "/tmp") + "/pose_correction_" + std::to_string(static_cast<long>(std::chrono::steady_clock::now().time_since_epoch().count())) + ".map";
        t0 = std::chrono::steady_clock::now();
        volume.WriteToFile(map_file);
        t_write = Seconds(t0);
        std::remove(map_file.c_str());
        if (!dump.empty() && !Dump(volume, dump)) { std::cout << RED << "[ERROR]::cannot write " << dump << RESET << std::endl; return 1; }
    }

    t0 = std::chrono::steady_clock::now();
    for (long k = 0; k < n; ++k) reference.IntegrateImage(depth[k], rgb[k], truth[k]);
    reference.Synchronize();
    const double t_reference = Seconds(t0);

    Blocks got, want;
    if (!Download(volume, &got) || !Download(reference, &want)) { std::cout << RED << "[ERROR]::cannot read the volumes back: " << op_last_error() << RESET << std::endl; return 1; }
    std::map<std::vector<int32_t>, size_t> at;
    for (size_t b = 0; b < got.n; ++b) at[std::vector<int32_t>(got.keys.begin() + 3 * b, got.keys.begin() + 3 * b + 3)] = b;
    unsigned long long weight_mismatch = 0, missing_blocks = 0, extra_observed = 0;
    double max_sdf = 0, max_col = 0;
    std::vector<char> seen(got.n, 0);
    for (size_t b = 0; b < want.n; ++b) {
        std::map<std::vector<int32_t>, size_t>::const_iterator it = at.find(std::vector<int32_t>(want.keys.begin() + 3 * b, want.keys.begin() + 3 * b + 3));
        if (it == at.end()) { ++missing_blocks; continue; }
        seen[it->second] = 1;
        const float* w = &want.vox[b * 2560];
        const float* g = &got.vox[it->second * 2560];
        for (int i = 0; i < 512; ++i) {
            if (w[5 * i + 1] != g[5 * i + 1]) { ++weight_mismatch; continue; }
            if (!(w[5 * i + 1] > 0)) continue;
            max_sdf = std::fmax(max_sdf, std::fabs(static_cast<double>(w[5 * i]) - static_cast<double>(g[5 * i])));
            for (int c = 2; c < 5; ++c) max_col = std::fmax(max_col, std::fabs(static_cast<double>(w[5 * i + c]) - static_cast<double>(g[5 * i + c])));
        }
    }
    for (size_t b = 0; b < got.n; ++b) // blocks only the drifted frames selected: they remain, and must hold nothing
        if (!seen[b])
            for (int i = 0; i < 512; ++i)
                if (got.vox[b * 2560 + 5 * i + 1] != 0.0f) ++extra_observed;
    // --path refine: how far the K frames were from the truth before and after (translation in mm, rotation in degrees), and the poses themselves
    double err_before[2] = {0, 0}, err_after[2] = {0, 0}, err_after_max[2] = {0, 0};
    if (path == "refine") {
        for (size_t j = 0; j < moved_index.size(); ++j) {
            const geometry::TransformationMatrix& want_pose = truth[moved_index[j]];
            for (int which = 0; which < 2; ++which) {
                const float* T = (which ? new_poses : old_poses).data() + 16 * j;
                double tt = 0, tr = 0;
                for (int r = 0; r < 3; ++r) {
                    tt += (static_cast<double>(T[4 * r + 3]) - want_pose(r, 3)) * (static_cast<double>(T[4 * r + 3]) - want_pose(r, 3));
                    for (int c = 0; c < 3; ++c) tr += static_cast<double>(T[4 * r + c]) * want_pose(r, c); // trace(R_est^T R_true)
                }
                const double mm = 1000.0 * std::sqrt(tt), deg = 180.0 / kPi * std::acos(std::fmin(1.0, std::fmax(-1.0, (tr - 1.0) / 2.0)));
                double* sum = which ? err_after : err_before;
                sum[0] += mm / moved_index.size(); sum[1] += deg / moved_index.size();
                if (which) { err_after_max[0] = std::fmax(err_after_max[0], mm); err_after_max[1] = std::fmax(err_after_max[1], deg); }
            }
        }
        if (!dump.empty()) {
            FILE* f = fopen(dump.c_str(), "w");
            if (!f) { std::cout << RED << "[ERROR]::cannot write " << dump << RESET << std::endl; return 1; }
            for (size_t j = 0; j < moved_index.size(); ++j) {
                fprintf(f, "%ld", moved_index[j]);
                for (int a = 0; a < 16; ++a) fprintf(f, " %.9g", new_poses[16 * j + a]);
                fprintf(f, "\n");
            }
            fclose(f);
        }
        op_device_release(d_depth, device);
        op_device_release(d_rgb, device);
    }
    uint64_t dei[4] = {0, 0, 0, 0};
    op_volume_deintegrate_stats(volume.Handle(), &dei[0], &dei[1], &dei[2], &dei[3]);
    std::cout << "{\"frames\": " << n << ", \"stride\": " << stride << ", \"first\": " << first << ", \"perturbed\": " << perturb << ", \"res\": " << res << ", \"path\": \"" << path
              << "\", \"runs\": " << runs << ", \"repair_ms_min_max\": [" << repair_s.front() * 1000.0 << ", " << repair_s.back() * 1000.0 << "]"
              << ", \"ms\": {\"fuse_drifted\": " << t_fuse * 1000.0 << ", \"repair\": " << t_repair * 1000.0 << ", \"reference\": " << t_reference * 1000.0 << "}"
              << ", \"blocks_drifted\": " << blocks_drifted << ", \"blocks\": " << got.n << ", \"blocks_reference\": " << want.n << ", \"missing_blocks\": " << missing_blocks
              << ", \"weight_mismatches\": " << weight_mismatch + extra_observed << ", \"max_abs_sdf_diff\": " << max_sdf << ", \"max_abs_colour_diff\": " << max_col
              << ", \"deintegrated\": {\"frames\": " << dei[0] << ", \"reverted\": " << dei[1] << ", \"reset\": " << dei[2] << ", \"skipped\": " << dei[3] << "}";
    if (path == "refine") {
        std::sort(estimate_s.begin(), estimate_s.end());
        std::sort(move_s.begin(), move_s.end());
        std::cout << ", \"refine\": {\"mode\": \"" << refine << "\", \"pixel_stride\": " << pixel_stride << ", \"iters\": " << iters << ", \"linearization\": \"" << linearization
                  << "\", \"color\": \"" << color << "\", \"estimate_ms\": " << estimate_s[estimate_s.size() / 2] * 1000.0 << ", \"estimate_ms_min_max\": [" << estimate_s.front() * 1000.0
                  << ", " << estimate_s.back() * 1000.0 << "], \"move_ms\": " << move_s[move_s.size() / 2] * 1000.0 << ", \"error_before_mm_deg\": [" << err_before[0] << ", "
                  << err_before[1] << "], \"error_after_mm_deg\": [" << err_after[0] << ", " << err_after[1] << "], \"error_after_max_mm_deg\": [" << err_after_max[0] << ", "
                  << err_after_max[1] << "], \"rounds\": " << reg_stats.rounds << ", \"launches\": " << reg_stats.launches << ", \"evaluations\": " << reg_stats.evaluations
                  << ", \"points\": " << reg_stats.points << "}";
    }
    if (!collect.empty()) {
        const op_volume_collect_stats& cs = volume.CollectStats();
        std::cout << ", \"collect\": {\"route\": \"" << collect << "\", \"blocks_before\": " << blocks_repaired << ", \"blocks_after\": " << blocks_collected << ", \"ms\": " << t_collect * 1000.0
                  << ", \"ms_min_max\": [" << collect_s.front() * 1000.0 << ", " << collect_s.back() * 1000.0 << "], \"removed_unobserved\": " << cs.removed_unobserved
                  << ", \"blocks_moved\": " << cs.blocks_moved << ", \"after_ms\": {\"extract_triangle_mesh\": " << t_mesh * 1000.0 << ", \"render_frame\": " << t_render * 1000.0
                  << ", \"write_to_file\": " << t_write * 1000.0 << "}, \"triangles\": " << triangles << ", \"rendered_pixels\": " << rendered << "}";
    }
    std::cout << "}" << std::endl;
    return 0;
}
