// coarsen_surface_check.cpp -- CubeHandler::Coarsen (host/one_piece) over a volume read from a .map file; prints the result's voxel size, the block id of (1, 1, 1), the block
// count and the last level's counts for tests/test_volume_coarsen_gpu.py to compare with the C-ABI's answers.
//   coarsen_surface_check MAP RES LEVELS MIN_WEIGHT
#include <cstdio>
#include <cstdlib>

#include "Integration/CubeHandler.h"
using namespace one_piece;

int main(int argc, char* argv[]) {
    if (argc != 5) return 2;
    camera::PinholeCamera camera;
    camera.SetPara(50.0f, 50.0f, 32.0f, 24.0f, 64, 48, 1000.0f);
    integration::CubeHandler volume(camera);
    volume.SetVoxelResolution(static_cast<float>(std::atof(argv[2])));
    if (!volume.ReadFromFile(argv[1])) return 3;
    op_volume_coarsen_stats st;
    std::shared_ptr<integration::CubeHandler> coarse = volume.Coarsen(std::atoi(argv[3]), static_cast<float>(std::atof(argv[4])), &st);
    if (!coarse) return 4;
    std::shared_ptr<integration::CubeHandler> once = volume.Coarsen(); // one level, every observed voxel
    if (!once) return 4;
    float res = 0, res_once = 0, res_source = 0;
    if (op_volume_resolution(coarse->Handle(), &res) != OP_OK || op_volume_resolution(once->Handle(), &res_once) != OP_OK ||
        op_volume_resolution(volume.Handle(), &res_source) != OP_OK)
        return 5;
    const geometry::Point3 one(1.0f, 1.0f, 1.0f); // its block id tells the handler's own c_para.VoxelResolution
    printf("coarse %.9g %d %zu %llu %llu %llu %llu %llu %llu\n", res, coarse->GetCubeID(one)(0), coarse->GetCubeCount(), (unsigned long long)st.src_blocks,
           (unsigned long long)st.dst_blocks, (unsigned long long)st.voxels_full, (unsigned long long)st.voxels_partial, (unsigned long long)st.voxels_empty,
           (unsigned long long)st.dropped_min_weight);
    printf("once %.9g %d %zu source %.9g %d %zu\n", res_once, once->GetCubeID(one)(0), once->GetCubeCount(), res_source, volume.GetCubeID(one)(0), volume.GetCubeCount());
    return 0;
}
