// register_volume_surface_check.cpp -- CubeHandler::RegisterVolume / GetBandVoxels (host/one_piece) over two volumes read from .map files.  Inside
// one process the source's pool order is fixed, so the program itself holds RegisterVolume to op_volume_register_offset_points on GetBandVoxels'
// list bit for bit (exit code 7 otherwise), then prints what it got for tests/test_register_volume_gpu.py to compare with the Python entry's answer.
//   register_volume_surface_check TARGET_MAP SOURCE_MAP RES START(16 floats, row-major, text file)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "Integration/CubeHandler.h"
using namespace one_piece;

static void Print(const char* what, const registration::RegistrationResult& r, const op_volume_register_volume_result& v) {
    const op_volume_register_robust_result& b = v.robust;
    const op_volume_register_color_result& c = b.color;
    const op_volume_register_result& d = c.base;
    printf("%s %llu %d %d %llu %llu %llu %llu %llu %llu %llu %.17g %.17g %.17g %.17g %.17g", what, (unsigned long long)v.selected, d.iterations, d.status, (unsigned long long)d.used,
           (unsigned long long)d.invalid, (unsigned long long)d.no_gradient, (unsigned long long)d.too_far, (unsigned long long)d.first_used, (unsigned long long)c.colored,
           (unsigned long long)c.first_colored, d.rmse, d.first_rmse, c.first_rmse_color, b.first_rmse_residual, r.rmse);
    for (int i = 0; i < 4; ++i)
        for (int k = 0; k < 4; ++k) printf(" %.9g", r.T(i, k));
    printf("\n");
}

int main(int argc, char* argv[]) {
    if (argc != 5) return 2;
    camera::PinholeCamera camera;
    camera.SetCameraType(camera::CameraType::OPEN3D_DATASET);
    integration::CubeHandler target(camera), source(camera);
    const float res = static_cast<float>(std::atof(argv[3]));
    target.SetVoxelResolution(res);
    source.SetVoxelResolution(res);
    if (!target.ReadFromFile(argv[1]) || !source.ReadFromFile(argv[2])) return 3;
    geometry::TransformationMatrix start;
    float t[16];
    FILE* f = fopen(argv[4], "r");
    if (!f) return 4;
    for (int i = 0; i < 4; ++i)
        for (int k = 0; k < 4; ++k) {
            float x = 0;
            if (fscanf(f, "%f", &x) != 1) return 4;
            start(i, k) = x;
            t[4 * i + k] = x;
        }
    fclose(f);

    op_volume_band_params sel;
    sel.band = 0.0f; sel.min_weight = 2.0f; sel.voxel_stride = 2; // the truncation, two frames at least, every second voxel
    geometry::Point3List points;
    std::vector<float> sdf, intensity;
    if (!source.GetBandVoxels(points, sdf, intensity, &sel) || points.empty() || sdf.size() != points.size() || intensity.size() != points.size()) return 5;
    op_volume_register_color_params params;
    params.base.max_iterations = 5; params.base.max_distance = 0.1f; params.base.min_step = 0.0f; params.base.min_points = 6;
    params.color_scale = 0.5f; params.max_color_residual = 0.25f;
    op_volume_register_options options;
    options.linearization = OP_REGISTER_LIN_METRIC; options.huber = 0.01f; options.huber_color = 0.02f;
    op_volume_register_volume_result details;
    std::shared_ptr<registration::RegistrationResult> r = target.RegisterVolume(source, start, &sel, &params, &options, &details);
    if (!r || !r->correspondence_set.empty() || details.selected != points.size()) return 6;
    op_volume_register_robust_result want;
    if (op_volume_register_offset_points(target.Handle(), points[0].data(), sdf.data(), intensity.data(), points.size(), OP_MEM_HOST, t, &params, &options, &want) != OP_OK) return 6;
    if (std::memcmp(&want, &details.robust, sizeof(want)) != 0) return 7;
    Print("given", *r, details);
    r = target.RegisterVolume(source, start, nullptr, nullptr, nullptr, &details); // the defaults: two voxels, GRADIENT, the colour term with weight 1
    if (!r) return 6;
    Print("defaults", *r, details);
    return 0;
}
