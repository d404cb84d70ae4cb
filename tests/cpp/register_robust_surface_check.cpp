// register_robust_surface_check.cpp -- CubeHandler::RobustRegistrationSystem / RegisterPointCloudRobust / RegisterRGBDRobust (host/one_piece) over a
// volume read from a .map file, points and colours read from float32 files, a depth image from a float32 file and a colour image from a byte
// file; prints what they return for tests/test_volume_register_robust_gpu.py to compare with the C-ABI's answers.
//   register_robust_surface_check MAP RES POINTS COLORS DEPTH RGB FX FY CX CY WIDTH HEIGHT POSE(16 floats, row-major, text file)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "Geometry/PointCloud.h"
#include "Integration/CubeHandler.h"
using namespace one_piece;

template <class T>
static std::vector<T> ReadAll(const char* file) {
    std::vector<T> raw;
    FILE* f = fopen(file, "rb");
    if (!f) return raw;
    T buf[256];
    size_t got;
    while ((got = fread(buf, sizeof(T), 256, f)) > 0) raw.insert(raw.end(), buf, buf + got);
    fclose(f);
    return raw;
}

static void Print(const char* what, const registration::RegistrationResult& r, const op_volume_register_robust_result& b) {
    const op_volume_register_color_result& c = b.color;
    const op_volume_register_result& d = c.base;
    printf("%s %d %d %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %.17g %.17g %.17g %.17g %.17g %.17g %.17g", what, d.iterations, d.status, (unsigned long long)d.used,
           (unsigned long long)d.invalid, (unsigned long long)d.no_gradient, (unsigned long long)d.too_far, (unsigned long long)d.first_used,
           (unsigned long long)c.colored, (unsigned long long)c.first_colored, (unsigned long long)b.downweighted, (unsigned long long)b.color_downweighted,
           (unsigned long long)b.first_downweighted, d.rmse, d.first_rmse, c.rmse_color, c.first_rmse_color, b.rmse_residual, b.first_rmse_residual, r.rmse);
    for (int i = 0; i < 4; ++i)
        for (int k = 0; k < 4; ++k) printf(" %.9g", r.T(i, k));
    printf("\n");
}

int main(int argc, char* argv[]) {
    if (argc != 14) return 2;
    camera::PinholeCamera camera;
    const int width = std::atoi(argv[11]), height = std::atoi(argv[12]);
    camera.SetPara(static_cast<float>(std::atof(argv[7])), static_cast<float>(std::atof(argv[8])), static_cast<float>(std::atof(argv[9])),
                   static_cast<float>(std::atof(argv[10])), width, height, 1000.0f);
    integration::CubeHandler volume(camera);
    volume.SetVoxelResolution(static_cast<float>(std::atof(argv[2])));
    if (!volume.ReadFromFile(argv[1])) return 3;
    const std::vector<float> raw = ReadAll<float>(argv[3]), col = ReadAll<float>(argv[4]);
    std::vector<float> depth = ReadAll<float>(argv[5]);
    std::vector<unsigned char> rgb = ReadAll<unsigned char>(argv[6]);
    const size_t npix = static_cast<size_t>(width) * height;
    if (raw.empty() || col.size() != raw.size() || depth.size() != npix || rgb.size() != 3 * npix) return 4;
    geometry::PointCloud pcd;
    pcd.points.resize(raw.size() / 3);
    pcd.colors.resize(raw.size() / 3);
    std::vector<float> intensity(raw.size() / 3);
    for (size_t i = 0; i < pcd.points.size(); ++i) {
        pcd.points[i] = geometry::Point3(raw[3 * i], raw[3 * i + 1], raw[3 * i + 2]);
        pcd.colors[i] = geometry::Point3(col[3 * i], col[3 * i + 1], col[3 * i + 2]);
        const float a = 0.114f * col[3 * i], b = 0.587f * col[3 * i + 1], c = 0.299f * col[3 * i + 2];
        const float ab = a + b;
        intensity[i] = ab + c;
    }
    geometry::TransformationMatrix init = geometry::TransformationMatrix::Identity(), pose;
    init(0, 3) = 0.01f; init(1, 3) = -0.02f; init(2, 3) = 0.005f;
    FILE* f = fopen(argv[13], "r");
    if (!f) return 4;
    for (int i = 0; i < 4; ++i)
        for (int k = 0; k < 4; ++k) {
            float x = 0;
            if (fscanf(f, "%f", &x) != 1) return 4;
            pose(i, k) = x;
        }
    fclose(f);

    op_volume_register_options options;
    options.linearization = OP_REGISTER_LIN_GRADIENT; options.huber = 0.005f; options.huber_color = 0.01f;
    double sums[31];
    uint64_t counts[7];
    if (!volume.RobustRegistrationSystem(pcd.points, intensity, init, 0.1f, 0.5f, 0.25f, &options, sums, counts)) return 5;
    printf("system");
    for (int k = 0; k < 7; ++k) printf(" %llu", (unsigned long long)counts[k]);
    for (int k = 0; k < 31; ++k) printf(" %.17g", sums[k]);
    printf("\n");

    op_volume_register_color_params params;
    params.base.max_iterations = 4; params.base.max_distance = 0.1f; params.base.min_step = 0.0f; params.base.min_points = 6;
    params.color_scale = 0.5f; params.max_color_residual = 0.25f;
    options.linearization = OP_REGISTER_LIN_METRIC;
    op_volume_register_robust_result details;
    std::shared_ptr<registration::RegistrationResult> r = volume.RegisterPointCloudRobust(pcd, init, &params, &options, &details);
    if (!r || !r->correspondence_set.empty() || !r->correspondence_set_index.empty()) return 6;
    Print("points", *r, details);
    r = volume.RegisterPointCloudRobust(pcd, geometry::TransformationMatrix::Identity(), nullptr, nullptr, &details); // identity, the defaults: METRIC, no weights
    if (!r) return 6;
    Print("defaults", *r, details);
    geometry::PointCloud bare;
    bare.points = pcd.points;
    r = volume.RegisterPointCloudRobust(bare, init, &params, &options, &details); // no colours: the geometric registration
    if (!r) return 6;
    Print("bare", *r, details);
    cv::Mat image(height, width, CV_32FC1, depth.data()), color(height, width, CV_8UC3, rgb.data());
    r = volume.RegisterRGBDRobust(image, color, pose, 2, &params, &options, &details);
    if (!r) return 6;
    Print("rgbd", *r, details);
    r = volume.RegisterRGBDRobust(image, cv::Mat(), pose, 2, &params, &options, &details); // no colour image: the depth alone
    if (!r) return 6;
    Print("depth", *r, details);
    return 0;
}
