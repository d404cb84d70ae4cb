// Calls the two members CubeHandler gained with de-integration; tests/test_deintegrate_cpu.py compiles and links it as C++11 against the class
// surface (no GPU needed to build; with one it moves a frame and prints the counters).
#include <cstdint>
#include <iostream>

#include "Geometry/Geometry.h"
#include "Integration/CubeHandler.h"
#include "onepiece_hip.h"
using namespace one_piece;

int main(int argc, char**) {
    if (argc < 2) { std::cout << "usage::deintegrate_surface run" << std::endl; return 0; }
    camera::PinholeCamera camera;
    camera.SetCameraType(camera::CameraType::OPEN3D_DATASET);
    cv::Mat depth, rgb;
    depth.create(static_cast<int>(camera.GetHeight()), static_cast<int>(camera.GetWidth()), CV_32FC1);
    rgb.create(static_cast<int>(camera.GetHeight()), static_cast<int>(camera.GetWidth()), CV_8UC3);
    for (int v = 0; v < depth.rows; ++v)
        for (int u = 0; u < depth.cols; ++u) {
            depth.at<float>(v, u) = 1.5f;
            for (int c = 0; c < 3; ++c) rgb.data[3 * (static_cast<size_t>(v) * depth.cols + u) + c] = static_cast<unsigned char>(u + v + c);
        }
    geometry::TransformationMatrix a = geometry::TransformationMatrix::Identity(), b = a;
    b(0, 3) = 0.02f;
    integration::CubeHandler handler(camera);
    handler.IntegrateImage(depth, rgb, a);
    handler.ReintegrateImage(depth, rgb, a, b);
    handler.DeintegrateImage(depth, rgb, b);
    if (!handler.Handle()) return 1;
    uint64_t n[4] = {0, 0, 0, 0};
    if (op_volume_deintegrate_stats(handler.Handle(), &n[0], &n[1], &n[2], &n[3]) != OP_OK) return 1;
    std::cout << "deintegrated " << n[0] << " frames: reverted " << n[1] << ", reset " << n[2] << ", skipped " << n[3] << std::endl;
    return n[0] == 2 && n[1] == 0 && n[3] == 0 ? 0 : 1;
}
