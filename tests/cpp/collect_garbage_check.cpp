// Runs a pose-correction scenario through the class surface -- CubeHandler::IntegrateImage, ReintegrateImage, then CollectGarbage() (or
// CollectGarbage(2.f) / CropToCubes) and GetCubeMap() -- and dumps keys and voxels; tests/test_collect_garbage_gpu.py compares the dump with
// the model, tests/test_collect_garbage_cpu.py compiles and links it as C++11 (no GPU needed to build or to print the usage line).
//   collect_garbage_check gc|weight2|crop IN OUT
//   IN : int32 {frames, width, height, moves}, float32 {fx, fy, cx, cy, depth_scale, resolution, truncation}, per frame depth [h,w] float32,
//        rgb [h,w,3] uint8, pose [16] float32 (row-major), per move int32 frame, old pose [16], new pose [16]
//   OUT: uint64 {blocks, blocks_before, blocks_kept, removed_outside, removed_unobserved, blocks_moved}, keys [n,3] int32, voxels [n,512,5] float32
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "Geometry/Geometry.h"
#include "Integration/CubeHandler.h"
#include "onepiece_hip.h"
using namespace one_piece;

namespace {
bool ReadPose(FILE* f, geometry::TransformationMatrix* T) {
    float p[16];
    if (fread(p, sizeof(float), 16, f) != 16) return false;
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) (*T)(r, c) = p[4 * r + c];
    return true;
}
} // namespace

int main(int argc, char* argv[]) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (argc != 4 || (mode != "gc" && mode != "weight2" && mode != "crop")) { std::cout << "usage::collect_garbage_check gc|weight2|crop IN OUT" << std::endl; return argc > 1 ? 2 : 0; }
    FILE* in = fopen(argv[2], "rb");
    if (!in) return 2;
    int32_t head[4];
    float par[7];
    if (fread(head, sizeof(int32_t), 4, in) != 4 || fread(par, sizeof(float), 7, in) != 7) return 2;
    const int n = head[0], w = head[1], h = head[2], moves = head[3];
    camera::PinholeCamera camera(par[0], par[1], par[2], par[3], w, h, par[4]);
    std::vector<cv::Mat> depth(n), rgb(n);
    std::vector<geometry::TransformationMatrix> pose(n);
    for (int k = 0; k < n; ++k) {
        depth[k].create(h, w, CV_32FC1);
        rgb[k].create(h, w, CV_8UC3);
        const size_t px = static_cast<size_t>(w) * h;
        if (fread(depth[k].data, sizeof(float), px, in) != px || fread(rgb[k].data, 1, 3 * px, in) != 3 * px || !ReadPose(in, &pose[k])) return 2;
    }
    integration::CubeHandler handler(camera);
    handler.SetVoxelResolution(par[5]);
    handler.SetTruncation(par[6]);
    for (int k = 0; k < n; ++k) handler.IntegrateImage(depth[k], rgb[k], pose[k]);
    for (int k = 0; k < moves; ++k) {
        int32_t at = 0;
        geometry::TransformationMatrix from, to;
        if (fread(&at, sizeof(at), 1, in) != 1 || at < 0 || at >= n || !ReadPose(in, &from) || !ReadPose(in, &to)) return 2;
        handler.ReintegrateImage(depth[at], rgb[at], from, to);
    }
    fclose(in);
    if (!handler.Handle()) return 1; // (no device: the class has said so)
    if (mode == "gc") handler.CollectGarbage();
    else if (mode == "weight2") handler.CollectGarbage(2.f);
    else handler.CropToCubes(integration::CubeID(-2, -1, -2), integration::CubeID(1, 0, 1));
    const op_volume_collect_stats st = handler.CollectStats();
    const integration::CubeMap map = handler.GetCubeMap();
    FILE* out = fopen(argv[3], "wb");
    if (!out) return 2;
    const uint64_t top[6] = {static_cast<uint64_t>(map.size()), st.blocks_before, st.blocks_kept, st.removed_outside, st.removed_unobserved, st.blocks_moved};
    fwrite(top, sizeof(uint64_t), 6, out);
    for (integration::CubeMap::const_iterator it = map.begin(); it != map.end(); ++it) {
        const int32_t key[3] = {it->first(0), it->first(1), it->first(2)};
        fwrite(key, sizeof(int32_t), 3, out);
    }
    std::vector<float> vox(512 * 5);
    for (integration::CubeMap::const_iterator it = map.begin(); it != map.end(); ++it) {
        for (int i = 0; i < 512; ++i) {
            const integration::TSDFVoxel& t = it->second.voxels[i];
            vox[5 * i] = t.sdf; vox[5 * i + 1] = t.weight;
            for (int c = 0; c < 3; ++c) vox[5 * i + 2 + c] = t.color(c);
        }
        fwrite(vox.data(), sizeof(float), vox.size(), out);
    }
    fclose(out);
    std::cout << "collect_garbage_check " << mode << ": " << st.blocks_before << " -> " << st.blocks_kept << " blocks, " << st.blocks_moved << " moved" << std::endl;
    return 0;
}
