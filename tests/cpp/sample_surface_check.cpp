// sample_surface_check.cpp -- CubeHandler::SampleVoxels / SampleGradients / DistanceToModel (host/one_piece) over a volume read from a .map file and
// points read from a float32 file; writes what they return for tests/test_volume_sample_gpu.py to compare with the C-ABI's answers.
//   sample_surface_check MAP RES POINTS OUT_PREFIX
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "Geometry/PointCloud.h"
#include "Integration/CubeHandler.h"
using namespace one_piece;

static bool Write(const std::string& file, const void* p, size_t bytes) {
    FILE* f = fopen(file.c_str(), "wb");
    if (!f) return false;
    const bool ok = bytes == 0 || fwrite(p, 1, bytes, f) == bytes;
    return fclose(f) == 0 && ok;
}

int main(int argc, char* argv[]) {
    if (argc != 5) return 2;
    const std::string out = argv[4];
    camera::PinholeCamera camera;
    integration::CubeHandler volume(camera);
    volume.SetVoxelResolution(static_cast<float>(std::atof(argv[2])));
    if (!volume.ReadFromFile(argv[1])) return 3;
    FILE* f = fopen(argv[3], "rb");
    if (!f) return 4;
    std::vector<float> raw;
    float buf[3];
    while (fread(buf, sizeof(float), 3, f) == 3) raw.insert(raw.end(), buf, buf + 3);
    fclose(f);
    const size_t n = raw.size() / 3;
    geometry::Point3List pts(n);
    for (size_t i = 0; i < n; ++i) pts[i] = geometry::Point3(raw[3 * i], raw[3 * i + 1], raw[3 * i + 2]);
    geometry::TransformationMatrix T = geometry::TransformationMatrix::Identity();
    T(0, 3) = 0.01f; T(1, 3) = -0.02f; T(2, 3) = 0.005f;

    std::vector<integration::TSDFVoxel> vox;
    std::vector<uint8_t> status;
    std::vector<float> flat(5 * n);
    const char* names[3] = {"_tri", "_ref", "_tri_T"};
    for (int c = 0; c < 3; ++c) {
        if (c == 2) volume.SampleVoxels(pts, vox, status, false, T); else volume.SampleVoxels(pts, vox, status, c == 1);
        if (vox.size() != n || status.size() != n) return 5;
        for (size_t i = 0; i < n; ++i) {
            flat[5 * i] = vox[i].sdf; flat[5 * i + 1] = vox[i].weight;
            for (int k = 0; k < 3; ++k) flat[5 * i + 2 + k] = vox[i].color(k);
        }
        if (!Write(out + names[c] + "_voxels.bin", flat.data(), flat.size() * sizeof(float)) || !Write(out + names[c] + "_status.bin", status.data(), n)) return 6;
    }
    geometry::Point3List grad;
    volume.SampleGradients(pts, grad, status);
    if (grad.size() != n || status.size() != n) return 5;
    std::vector<float> g(3 * n);
    for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) g[3 * i + k] = grad[i](k);
    if (!Write(out + "_gradients.bin", g.data(), g.size() * sizeof(float)) || !Write(out + "_gradient_status.bin", status.data(), n)) return 6;
    geometry::PointCloud pcd;
    pcd.points = pts;
    const op_volume_sample_stats a = volume.DistanceToModel(pcd), b = volume.DistanceToModel(pcd, T);
    printf("%llu %llu %.17g %.17g %.9g\n%llu %llu %.17g %.17g %.9g\n", (unsigned long long)a.queries, (unsigned long long)a.valid, a.sum_abs_sdf, a.sum_sq_sdf, a.max_abs_sdf,
           (unsigned long long)b.queries, (unsigned long long)b.valid, b.sum_abs_sdf, b.sum_sq_sdf, b.max_abs_sdf);
    return 0;
}
