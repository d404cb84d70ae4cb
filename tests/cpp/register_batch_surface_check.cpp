// register_batch_surface_check.cpp -- CubeHandler::RegisterFramesRobust / RegisterPointCloudsRobust (host/one_piece) over a volume read from a .map
// file and N frames read from a float32 depth file and a byte colour file: every element of the batch calls' answers must be, byte for byte, what
// RegisterRGBDRobust / RegisterPointCloudRobust return for that frame alone; prints one line per frame for
// tests/test_volume_register_batch_gpu.py to compare with the C-ABI's answers.  Exit 0 only when everything agreed.
//   register_batch_surface_check MAP RES DEPTHS RGBS FX FY CX CY WIDTH HEIGHT POSES(N x 16 floats, row-major, text file) N
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

static void Print(const char* what, size_t f, const registration::RegistrationResult& r, const op_volume_register_robust_result& b) {
    const op_volume_register_result& d = b.color.base;
    printf("%s %zu %d %d %llu %llu %.17g %.17g %.17g", what, f, d.iterations, d.status, (unsigned long long)d.used, (unsigned long long)b.downweighted, d.rmse,
           b.rmse_residual, r.rmse);
    for (int i = 0; i < 4; ++i)
        for (int k = 0; k < 4; ++k) printf(" %.9g", r.T(i, k));
    printf("\n");
}

static bool Same(const op_volume_register_robust_result& a, const op_volume_register_robust_result& b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

int main(int argc, char* argv[]) {
    if (argc != 13) return 2;
    camera::PinholeCamera camera;
    const int width = std::atoi(argv[9]), height = std::atoi(argv[10]);
    const float fx = static_cast<float>(std::atof(argv[5])), fy = static_cast<float>(std::atof(argv[6])), cx = static_cast<float>(std::atof(argv[7])),
                cy = static_cast<float>(std::atof(argv[8]));
    camera.SetPara(fx, fy, cx, cy, width, height, 1000.0f);
    integration::CubeHandler volume(camera);
    volume.SetVoxelResolution(static_cast<float>(std::atof(argv[2])));
    if (!volume.ReadFromFile(argv[1])) return 3;
    const size_t n = static_cast<size_t>(std::atoi(argv[12])), npix = static_cast<size_t>(width) * height;
    std::vector<float> depth = ReadAll<float>(argv[3]);
    std::vector<unsigned char> rgb = ReadAll<unsigned char>(argv[4]);
    if (!n || depth.size() != n * npix || rgb.size() != 3 * n * npix) return 4;
    geometry::Mat4List poses(n);
    FILE* pf = fopen(argv[11], "r");
    if (!pf) return 4;
    for (size_t f = 0; f < n; ++f)
        for (int i = 0; i < 4; ++i)
            for (int k = 0; k < 4; ++k) {
                float x = 0;
                if (fscanf(pf, "%f", &x) != 1) return 4;
                poses[f](i, k) = x;
            }
    fclose(pf);
    std::vector<cv::Mat> depths, rgbs;
    std::vector<geometry::PointCloud> clouds(n);
    for (size_t f = 0; f < n; ++f) {
        depths.push_back(cv::Mat(height, width, CV_32FC1, depth.data() + f * npix));
        rgbs.push_back(cv::Mat(height, width, CV_8UC3, rgb.data() + 3 * f * npix));
        for (int r = 0; r < height; r += 2)                            // a cloud per frame: every second pixel, camera coordinates, colours byte / 255
            for (int c = 0; c < width; c += 2) {
                const float z = depth[f * npix + static_cast<size_t>(r) * width + c];
                if (!(z > 0)) continue;
                clouds[f].points.push_back(geometry::Point3((c - cx) * z / fx, (r - cy) * z / fy, z));
                const unsigned char* b = rgb.data() + 3 * (f * npix + static_cast<size_t>(r) * width + c);
                clouds[f].colors.push_back(geometry::Point3(b[0] / 255.0f, b[1] / 255.0f, b[2] / 255.0f));
            }
    }

    op_volume_register_color_params params;
    params.base.max_iterations = 3; params.base.max_distance = 0.1f; params.base.min_step = 1e-3f; params.base.min_points = 6;
    params.color_scale = 0.5f; params.max_color_residual = 0.25f;
    op_volume_register_options options;
    options.linearization = OP_REGISTER_LIN_METRIC; options.huber = 0.01f; options.huber_color = 0.01f;
    std::vector<op_volume_register_robust_result> details;
    op_volume_register_batch_stats stats;
    int bad = 0;

    for (int color = 1; color >= 0; --color) {
        const std::vector<std::shared_ptr<registration::RegistrationResult>> got =
            volume.RegisterFramesRobust(depths, color ? rgbs : std::vector<cv::Mat>(), poses, 2, &params, &options, &details, &stats);
        if (got.size() != n || details.size() != n) return 5;
        uint64_t evaluations = 0;
        for (size_t f = 0; f < n; ++f) {
            op_volume_register_robust_result one;
            std::shared_ptr<registration::RegistrationResult> r = volume.RegisterRGBDRobust(depths[f], color ? rgbs[f] : cv::Mat(), poses[f], 2, &params, &options, &one);
            if (!r || !got[f]) return 6;
            if (!Same(one, details[f]) || r->rmse != got[f]->rmse) { fprintf(stderr, "frame %zu (colour %d) differs from the single call\n", f, color); ++bad; }
            evaluations += static_cast<uint64_t>(one.color.base.iterations) + 1;
            Print(color ? "rgbd" : "depth", f, *got[f], details[f]);
        }
        if (stats.evaluations != evaluations) { fprintf(stderr, "%llu evaluations, the single calls made %llu\n", (unsigned long long)stats.evaluations, (unsigned long long)evaluations); ++bad; }
        printf("stats %d %u %u %llu %llu\n", color, stats.rounds, stats.launches, (unsigned long long)stats.evaluations, (unsigned long long)stats.points);
    }
    // defaults (nullptr params and options) and the clouds
    const std::vector<std::shared_ptr<registration::RegistrationResult>> def = volume.RegisterFramesRobust(depths, rgbs, poses, 3, nullptr, nullptr, &details);
    if (def.size() != n) return 5;
    for (size_t f = 0; f < n; ++f) {
        op_volume_register_robust_result one;
        if (!volume.RegisterRGBDRobust(depths[f], rgbs[f], poses[f], 3, nullptr, nullptr, &one)) return 6;
        if (!Same(one, details[f])) { fprintf(stderr, "frame %zu differs from the single call under the defaults\n", f); ++bad; }
    }
    const std::vector<std::shared_ptr<registration::RegistrationResult>> pts = volume.RegisterPointCloudsRobust(clouds, poses, &params, &options, &details, &stats);
    if (pts.size() != n) return 5;
    for (size_t f = 0; f < n; ++f) {
        op_volume_register_robust_result one;
        if (!volume.RegisterPointCloudRobust(clouds[f], poses[f], &params, &options, &one)) return 6;
        if (!Same(one, details[f])) { fprintf(stderr, "cloud %zu differs from the single call\n", f); ++bad; }
        Print("cloud", f, *pts[f], details[f]);
    }
    // mismatched lists are refused with an empty answer
    geometry::Mat4List fewer(poses.begin(), poses.begin() + (n - 1));
    if (!volume.RegisterFramesRobust(depths, rgbs, fewer).empty() || !volume.RegisterPointCloudsRobust(clouds, fewer).empty()) ++bad;
    return bad ? 7 : 0;
}
