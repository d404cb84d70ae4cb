// GlobalRegistration.cpp -- submap-to-submap global registration as example/MergeMultipleSubmaps.cpp and DenseSlam::RegisterSubmap
// (DenseSlam.cpp:66-118) drive it, on two clouds and stage by stage so that every intermediate result can be written out: down-sampling and
// normals, FPFH (neighbour lists, simplified histograms, features), feature matching, three rounds of pruning, RANSAC.  The stages are the
// library's own public functions in the order registration::RansacRegistration calls them; parameters default to DenseSlam's (DenseSlam.h:49-68).
//
//   GlobalRegistration <source.ply> <target.ply> | --synthetic   [--path host|device] [--dump DIR] [--max-iteration 40000] [--voxel 0.05]
//                      [--as-given] [--features-only] [--load-features DIR] [--knn 100] [--search-radius 0.25]
//
//   --synthetic       two views of an analytic room (a box with two spheres) rendered to depth and back-projected (op_points_from_depth through
//                     PointCloud::LoadFromDepth); the source is the second view expressed in its own camera frame, so the transform that is
//                     looked for is known: inverse(pose_target) * pose_source, written to the JSON as "expected_T"; the estimated normals
//                     are turned towards the camera
//   --path            OP_RUNTIME_OPT_GLOBAL_REGISTRATION: host (default) or device
//   --as-given        PLY clouds that carry normals are used as they are (no down-sampling)
//   --features-only   stop after the features (no device is needed on the host path up to there)
//   --knn, --search-radius   FPFH's neighbour count and radius (the radius is compared with squared distances); DenseSlam's 100 and 0.25
//   --load-features   match with the features of an earlier --dump instead of the ones just computed
//   --dump DIR        raw little-endian arrays (float32 / int32) and result.json with the sizes, the result and the time of every stage
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "Geometry/Geometry.h"
#include "Geometry/PointCloud.h"
#include "Registration/GlobalRegistration.h"
#include "onepiece_hip.h"
using namespace one_piece;

namespace {

double Now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

template <class T>
bool WriteRaw(const std::string& dir, const char* name, const std::vector<T>& v) {
    std::ofstream os((dir + "/" + name).c_str(), std::ios::binary);
    if (!v.empty()) os.write(reinterpret_cast<const char*>(v.data()), static_cast<std::streamsize>(v.size() * sizeof(T)));
    return static_cast<bool>(os);
}
std::vector<float> Flat(const geometry::Point3List& p) {
    std::vector<float> v(p.size() * 3);
    for (size_t i = 0; i < p.size(); ++i) for (int k = 0; k < 3; ++k) v[3 * i + k] = p[i](k);
    return v;
}
std::vector<float> Flat(const registration::FeatureSet& f) {
    std::vector<float> v(f.size() * 33);
    for (size_t i = 0; i < f.size(); ++i) for (int b = 0; b < 33; ++b) v[33 * i + b] = f[i](b);
    return v;
}
std::vector<float> Flat(const std::vector<std::vector<float> >& s) {
    std::vector<float> v(s.size() * 33);
    for (size_t i = 0; i < s.size(); ++i) for (int b = 0; b < 33; ++b) v[33 * i + b] = s[i][static_cast<size_t>(b)];
    return v;
}
std::vector<int> Padded(const std::vector<std::vector<int> >& nb, int knn) { // n x knn, -1 padded
    std::vector<int> v(nb.size() * static_cast<size_t>(knn), -1);
    for (size_t i = 0; i < nb.size(); ++i) for (size_t k = 0; k < nb[i].size(); ++k) v[i * knn + k] = nb[i][k];
    return v;
}
std::vector<int> Flat(const geometry::FMatchSet& m) {
    std::vector<int> v(m.size() * 2);
    for (size_t i = 0; i < m.size(); ++i) { v[2 * i] = m[i].first; v[2 * i + 1] = m[i].second; }
    return v;
}
bool ReadFeatures(const std::string& file, size_t n, registration::FeatureSet& out) {
    std::ifstream is(file.c_str(), std::ios::binary);
    std::vector<float> v(n * 33);
    if (!is || (n && !is.read(reinterpret_cast<char*>(v.data()), static_cast<std::streamsize>(v.size() * 4)))) return false;
    registration::Feature zero; zero.resize(33); zero.setZero();
    out.assign(n, zero);
    for (size_t i = 0; i < n; ++i) for (int b = 0; b < 33; ++b) out[i](b) = v[33 * i + b];
    return true;
}

// camera-to-world pose on a circle of radius 0.5 m at angle th, looking outward, slightly pitched
geometry::TransformationMatrix ViewPose(float th, float pitch) {
    const float cy = std::cos(th), sy = std::sin(th), cp = std::cos(pitch), sp = std::sin(pitch);
    geometry::TransformationMatrix T = geometry::TransformationMatrix::Identity();
    const float Ry[9] = {cy, 0, sy, 0, 1, 0, -sy, 0, cy}, Rx[9] = {1, 0, 0, 0, cp, -sp, 0, sp, cp};
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) T(r, c) = Ry[3 * r] * Rx[c] + Ry[3 * r + 1] * Rx[3 + c] + Ry[3 * r + 2] * Rx[6 + c];
    T(0, 3) = 0.5f * sy; T(1, 3) = 0.05f; T(2, 3) = 0.5f * cy;
    return T;
}
// z-depth of the analytic room seen from `pose`: a 5.2 x 2.8 x 5.2 m box around the origin with two spheres in it
cv::Mat RenderRoom(const geometry::TransformationMatrix& P, const camera::PinholeCamera& cam) {
    const int W = cam.GetWidth(), H = cam.GetHeight();
    cv::Mat depth(H, W, CV_32FC1);
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
        }
    return depth;
}

void Matrix(std::ostream& os, const geometry::TransformationMatrix& T) {
    os << "[";
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) { char b[40]; std::snprintf(b, sizeof(b), "%s%.9g", r + c ? ", " : "", static_cast<double>(T(r, c))); os << b; }
    os << "]";
}

} // namespace

int main(int argc, char** argv) {
    registration::RANSACParameter r_para; // DenseSlam.h:49-68
    r_para.search_radius = 0.25; r_para.max_nn = 100; r_para.voxel_len = 0.05; r_para.search_radius_normal = 0.1; r_para.max_nn_normal = 30;
    r_para.max_iteration = 40000; r_para.threshold = 0.1;
    std::vector<std::string> files;
    std::string dump, load_features, path = "host";
    bool synthetic = false, as_given = false, features_only = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--synthetic") synthetic = true;
        else if (a == "--as-given") as_given = true;
        else if (a == "--features-only") features_only = true;
        else if (a == "--path" && i + 1 < argc) path = argv[++i];
        else if (a == "--dump" && i + 1 < argc) dump = argv[++i];
        else if (a == "--load-features" && i + 1 < argc) load_features = argv[++i];
        else if (a == "--max-iteration" && i + 1 < argc) r_para.max_iteration = std::atoi(argv[++i]);
        else if (a == "--voxel" && i + 1 < argc) r_para.voxel_len = static_cast<float>(std::atof(argv[++i]));
        else if (a == "--knn" && i + 1 < argc) r_para.max_nn = std::atoi(argv[++i]);
        else if (a == "--search-radius" && i + 1 < argc) r_para.search_radius = static_cast<float>(std::atof(argv[++i]));
        else if (a.compare(0, 2, "--") != 0) files.push_back(a);
        else { std::cout << "unknown argument " << a << std::endl; return 2; }
    }
    if ((!synthetic && files.size() != 2) || (path != "host" && path != "device") || r_para.max_nn < 1 || !(r_para.search_radius > 0)) {
        std::cout << "Usage: GlobalRegistration <source.ply> <target.ply> | --synthetic [--path host|device] [--dump DIR] [--max-iteration N] [--voxel L] [--as-given] "
                     "[--features-only] [--load-features DIR] [--knn K] [--search-radius R]" << std::endl;
        return 2;
    }
    if (op_runtime_set_option(OP_RUNTIME_OPT_GLOBAL_REGISTRATION, path == "device" ? 1 : 0) != OP_OK) { std::cout << op_last_error() << std::endl; return 3; }

    geometry::PointCloud clouds[2]; // source, target
    geometry::TransformationMatrix expected = geometry::TransformationMatrix::Zero();
    if (synthetic) {
        camera::PinholeCamera cam(514.817f, 515.375f, 318.771f, 238.447f, 640, 480, 1.0f); // depth scale 1: the rendered depth is metres in float
        const geometry::TransformationMatrix pose_s = ViewPose(0.65f, 0.06f), pose_t = ViewPose(0.40f, -0.04f);
        clouds[0].LoadFromDepth(RenderRoom(pose_s, cam), cam);
        clouds[1].LoadFromDepth(RenderRoom(pose_t, cam), cam);
        expected = pose_t.inverse() * pose_s;
    } else {
        for (int k = 0; k < 2; ++k)
            if (!clouds[k].LoadFromPLY(files[static_cast<size_t>(k)])) return 3;
    }
    if (clouds[0].GetSize() == 0 || clouds[1].GetSize() == 0) { std::cout << "empty cloud" << std::endl; return 3; }

    double t_prepare = Now();
    geometry::PointCloud down[2];
    for (int k = 0; k < 2; ++k) {
        if (!synthetic && as_given && clouds[k].HasNormals()) { down[k] = clouds[k]; continue; }
        down[k] = *clouds[k].DownSample(r_para.voxel_len);                                         // GlobalRegistration.cpp:133-140
        if (!down[k].HasNormals()) down[k].EstimateNormals(r_para.search_radius_normal, r_para.max_nn_normal);
        if (synthetic) // EstimateNormals leaves the sign open (as the reference does); a view knows where its camera is: normals face the origin
            for (size_t i = 0; i < down[k].normals.size(); ++i)
                if (down[k].normals[i].dot(down[k].points[i]) > 0) down[k].normals[i] = -down[k].normals[i];
    }
    t_prepare = Now() - t_prepare;

    registration::FeatureSet features[2];
    std::vector<std::vector<int> > neighbours[2];
    std::vector<std::vector<float> > spfh[2];
    double t_features = Now();
    for (int k = 0; k < 2; ++k) registration::ComputeFPFHFeatureDebug(down[k], features[k], r_para.max_nn, r_para.search_radius, &neighbours[k], &spfh[k]);
    t_features = Now() - t_features;
    const char* tag[2] = {"source", "target"};
    if (!dump.empty())
        for (int k = 0; k < 2; ++k) {
            const std::string t = tag[k];
            if (!WriteRaw(dump, (t + "_points.f32").c_str(), Flat(down[k].points)) || !WriteRaw(dump, (t + "_normals.f32").c_str(), Flat(down[k].normals)) ||
                !WriteRaw(dump, (t + "_neighbours.i32").c_str(), Padded(neighbours[k], r_para.max_nn)) || !WriteRaw(dump, (t + "_spfh.f32").c_str(), Flat(spfh[k])) ||
                !WriteRaw(dump, (t + "_fpfh.f32").c_str(), Flat(features[k]))) {
                std::cout << "cannot write to " << dump << std::endl;
                return 3;
            }
        }
    if (!load_features.empty())
        for (int k = 0; k < 2; ++k)
            if (!ReadFeatures(load_features + "/" + tag[k] + "_fpfh.f32", down[k].GetSize(), features[k])) { std::cout << "cannot read features from " << load_features << std::endl; return 3; }

    double t_match = 0, t_reject = 0, t_ransac = 0;
    geometry::FMatchSet matches, kept;
    std::vector<int> inlier_ids;
    geometry::PointCorrespondenceSet inliers;
    geometry::TransformationMatrix T = geometry::TransformationMatrix::Zero();
    float rmse = 0;
    if (!features_only) {
        t_match = Now();
        registration::FeatureMatching3D(features[0], features[1], matches);                         // GlobalRegistration.cpp:165
        t_match = Now() - t_match;
        t_reject = Now();
        kept = matches;
        std::default_random_engine engine;                                                         // :166
        for (int round = 0; round < 3; ++round) registration::RejectMatchesRanSaPC(down[0].points, down[1].points, engine, kept); // :167-169
        t_reject = Now() - t_reject;
        geometry::PointCorrespondenceSet correspondence_set;
        for (size_t i = 0; i != kept.size(); ++i)
            correspondence_set.push_back(std::make_pair(down[0].points[static_cast<size_t>(kept[i].first)], down[1].points[static_cast<size_t>(kept[i].second)]));
        t_ransac = Now();
        T = geometry::EstimateRigidTransformationRANSAC(correspondence_set, inliers, inlier_ids, r_para.max_iteration, static_cast<float>(r_para.threshold)); // :196
        t_ransac = Now() - t_ransac;
        float sum_error = 0.0;                                                                     // ComputeRMSE, GlobalRegistration.cpp:8-16
        for (size_t i = 0; i != inliers.size(); ++i) {
            const geometry::Point3& p = inliers[i].first;
            float d[3];
            for (int r = 0; r < 3; ++r) d[r] = (T(r, 0) * p(0) + T(r, 1) * p(1) + T(r, 2) * p(2)) + T(r, 3) - inliers[i].second(r);
            sum_error += d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        }
        rmse = std::sqrt(sum_error / inliers.size());
        if (!dump.empty()) {
            geometry::FMatchSet index;
            for (size_t i = 0; i < inlier_ids.size(); ++i) index.push_back(kept[static_cast<size_t>(inlier_ids[i])]);
            std::vector<float> t16(16);
            for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) t16[static_cast<size_t>(4 * r + c)] = T(r, c);
            if (!WriteRaw(dump, "matches.i32", Flat(matches)) || !WriteRaw(dump, "matches_kept.i32", Flat(kept)) || !WriteRaw(dump, "inlier_ids.i32", inlier_ids) ||
                !WriteRaw(dump, "correspondence_set_index.i32", Flat(index)) || !WriteRaw(dump, "T.f32", t16) || !WriteRaw(dump, "rmse.f32", std::vector<float>(1, rmse))) {
                std::cout << "cannot write to " << dump << std::endl;
                return 3;
            }
        }
    }
    std::ostringstream js;
    js << "{\"path\": \"" << path << "\", \"source_points\": " << down[0].GetSize() << ", \"target_points\": " << down[1].GetSize() << ", \"knn\": " << r_para.max_nn
       << ", \"max_iteration\": " << r_para.max_iteration << ", \"matches\": " << matches.size() << ", \"matches_kept\": " << kept.size() << ", \"inliers\": " << inlier_ids.size()
       << ", \"rmse\": " << (std::isfinite(rmse) ? rmse : -1.0f) << ", \"T\": ";
    Matrix(js, T);
    js << ", \"expected_T\": ";
    Matrix(js, expected);
    js << ", \"ms\": {\"prepare\": " << t_prepare << ", \"features\": " << t_features << ", \"matching\": " << t_match << ", \"rejection\": " << t_reject
       << ", \"ransac\": " << t_ransac << ", \"total\": " << t_features + t_match + t_reject + t_ransac << "}}";
    std::cout << js.str() << std::endl;
    if (!dump.empty()) { std::ofstream os((dump + "/result.json").c_str()); os << js.str() << std::endl; }
    return 0;
}
