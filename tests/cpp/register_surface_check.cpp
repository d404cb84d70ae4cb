// register_surface_check.cpp -- CubeHandler::RegistrationSystem / RegisterPointCloud / RegisterDepth (host/one_piece) over a volume read from a .map
// file, points read from a float32 file and a depth image read from a float32 file; prints what they return for
// tests/test_volume_register_gpu.py to compare with the C-ABI's answers.
//   register_surface_check MAP RES POINTS DEPTH FX FY CX CY WIDTH HEIGHT POSE(16 floats, row-major, text file)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "Geometry/PointCloud.h"
#include "Integration/CubeHandler.h"
using namespace one_piece;

static std::vector<float> ReadFloats(const char* file) {
    std::vector<float> raw;
    FILE* f = fopen(file, "rb");
    if (!f) return raw;
    float buf[256];
    size_t got;
    while ((got = fread(buf, sizeof(float), 256, f)) > 0) raw.insert(raw.end(), buf, buf + got);
    fclose(f);
    return raw;
}

static void Print(const char* what, const registration::RegistrationResult& r, const op_volume_register_result& d) {
    printf("%s %d %d %llu %llu %llu %llu %llu %.17g %.17g %.17g", what, d.iterations, d.status, (unsigned long long)d.used, (unsigned long long)d.invalid,
           (unsigned long long)d.no_gradient, (unsigned long long)d.too_far, (unsigned long long)d.first_used, d.rmse, d.first_rmse, r.rmse);
    for (int i = 0; i < 4; ++i)
        for (int k = 0; k < 4; ++k) printf(" %.9g", r.T(i, k));
    printf("\n");
}

int main(int argc, char* argv[]) {
    if (argc != 12) return 2;
    camera::PinholeCamera camera;
    const int width = std::atoi(argv[9]), height = std::atoi(argv[10]);
    camera.SetPara(static_cast<float>(std::atof(argv[5])), static_cast<float>(std::atof(argv[6])), static_cast<float>(std::atof(argv[7])),
                   static_cast<float>(std::atof(argv[8])), width, height, 1000.0f);
    integration::CubeHandler volume(camera);
    volume.SetVoxelResolution(static_cast<float>(std::atof(argv[2])));
    if (!volume.ReadFromFile(argv[1])) return 3;
    const std::vector<float> raw = ReadFloats(argv[3]);
    std::vector<float> depth = ReadFloats(argv[4]);
    if (raw.empty() || depth.size() != static_cast<size_t>(width) * height) return 4;
    geometry::PointCloud pcd;
    pcd.points.resize(raw.size() / 3);
    for (size_t i = 0; i < pcd.points.size(); ++i) pcd.points[i] = geometry::Point3(raw[3 * i], raw[3 * i + 1], raw[3 * i + 2]);
    geometry::TransformationMatrix init = geometry::TransformationMatrix::Identity(), pose;
    init(0, 3) = 0.01f; init(1, 3) = -0.02f; init(2, 3) = 0.005f;
    FILE* f = fopen(argv[11], "r");
    if (!f) return 4;
    for (int i = 0; i < 4; ++i)
        for (int k = 0; k < 4; ++k) {
            float x = 0;
            if (fscanf(f, "%f", &x) != 1) return 4;
            pose(i, k) = x;
        }
    fclose(f);

    double sums[28];
    uint64_t counts[4];
    if (!volume.RegistrationSystem(pcd.points, init, 0.1f, sums, counts)) return 5;
    printf("system %llu %llu %llu %llu", (unsigned long long)counts[0], (unsigned long long)counts[1], (unsigned long long)counts[2], (unsigned long long)counts[3]);
    for (int k = 0; k < 28; ++k) printf(" %.17g", sums[k]);
    printf("\n");

    op_volume_register_params params;
    params.max_iterations = 4; params.max_distance = 0.1f; params.min_step = 0.0f; params.min_points = 6;
    op_volume_register_result details;
    std::shared_ptr<registration::RegistrationResult> r = volume.RegisterPointCloud(pcd, init, &params, &details);
    if (!r || !r->correspondence_set.empty() || !r->correspondence_set_index.empty()) return 6;
    Print("points", *r, details);
    r = volume.RegisterPointCloud(pcd); // identity, the defaults
    if (!r) return 6;
    details = op_volume_register_result();
    Print("defaults", *r, details);
    cv::Mat image(height, width, CV_32FC1, depth.data());
    r = volume.RegisterDepth(image, pose, 2, &params, &details);
    if (!r) return 6;
    Print("depth", *r, details);
    return 0;
}
