// main.cpp of the golden generator (oracle/tools/gen_volume_golden.py): runs the REFERENCE's own integration::CubeHandler -- its
// Integration/*.cpp and Geometry/{TriangleMesh,Geometry,PointCloud}.cpp compiled where they lie against the cv::Mat stand-in of
// tests/tools/align_color_golden/opencv2 -- on one case per call:  volume_golden IN OUT.  IN and OUT are streams of named arrays
// (u32 name length, name, u32 type {0 f32, 1 i32, 2 u8, 3 u16, 4 u64}, u32 rank, u64 extents, data); which arrays IN holds decides
// what is run (see run_fusion / run_volume).  Every block set leaves in sorted key order.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <string>
#include <vector>

#include "Integration/CubeHandler.h"
#include "Integration/MarchingCubePredefined.h"

namespace cv { // never reached by the integration path
void pyrDown(const Mat&, Mat&, const Size&) { std::abort(); }
void cvtColor(const Mat&, Mat&, int) { std::abort(); }
void Sobel(const Mat&, Mat&, int, int, int) { std::abort(); }
void GaussianBlur(const Mat&, Mat&, const Size&, double) { std::abort(); }
void bilateralFilter(const Mat&, Mat&, int, double, double) { std::abort(); }
} // namespace cv

using namespace one_piece;
using integration::CubeHandler;
using integration::CubeID;
using integration::CubeMap;
using integration::VoxelCube;

struct Arr {
    uint32_t type = 0;
    std::vector<uint64_t> dims;
    std::vector<unsigned char> bytes;
    size_t count() const { size_t n = 1; for (uint64_t d : dims) n *= (size_t)d; return n; }
    const float* f() const { return reinterpret_cast<const float*>(bytes.data()); }
    const int32_t* i() const { return reinterpret_cast<const int32_t*>(bytes.data()); }
};
static const size_t kTypeSize[5] = {4, 4, 1, 2, 8};
typedef std::map<std::string, Arr> Bag;

static Bag read_bag(const char* path) {
    Bag bag;
    std::ifstream is(path, std::ios::binary);
    uint32_t len;
    while (is.read((char*)&len, 4)) {
        std::string name(len, ' ');
        is.read(&name[0], len);
        Arr a;
        uint32_t rank;
        is.read((char*)&a.type, 4);
        is.read((char*)&rank, 4);
        a.dims.resize(rank);
        is.read((char*)a.dims.data(), 8 * rank);
        a.bytes.resize(a.count() * kTypeSize[a.type]);
        is.read((char*)a.bytes.data(), (std::streamsize)a.bytes.size());
        if (!is) { std::cerr << "truncated input at " << name << std::endl; std::exit(1); }
        bag[name] = a;
    }
    return bag;
}

static std::ofstream g_out;
static void put(const std::string& name, uint32_t type, std::vector<uint64_t> dims, const void* data) {
    uint32_t len = (uint32_t)name.size(), rank = (uint32_t)dims.size();
    size_t n = kTypeSize[type];
    for (uint64_t d : dims) n *= (size_t)d;
    g_out.write((const char*)&len, 4);
    g_out.write(name.data(), len);
    g_out.write((const char*)&type, 4);
    g_out.write((const char*)&rank, 4);
    g_out.write((const char*)dims.data(), 8 * rank);
    g_out.write((const char*)data, (std::streamsize)n);
}

static geometry::TransformationMatrix matrix_of(const float* m) {
    geometry::TransformationMatrix M;
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) M(r, c) = m[4 * r + c];
    return M;
}

static std::vector<CubeID> sorted_ids(const CubeMap& map) {
    std::vector<CubeID> ids;
    for (const auto& kv : map) ids.push_back(kv.first);
    std::sort(ids.begin(), ids.end(), [](const CubeID& a, const CubeID& b) {
        return a(0) != b(0) ? a(0) < b(0) : a(1) != b(1) ? a(1) < b(1) : a(2) < b(2);
    });
    return ids;
}

// keys [n,3] i32 and voxels [n,512,5] f32 {sdf, weight, r, g, b}, sorted by key
static void put_volume(const std::string& name, CubeHandler& h) {
    const CubeMap map = h.GetCubeMap();
    const std::vector<CubeID> ids = sorted_ids(map);
    std::vector<int32_t> keys;
    std::vector<float> vox;
    for (const CubeID& id : ids) {
        for (int c = 0; c < 3; ++c) keys.push_back(id(c));
        const VoxelCube& cube = map.at(id);
        for (const auto& v : cube.voxels) {
            vox.push_back(v.sdf); vox.push_back(v.weight);
            vox.push_back(v.color(0)); vox.push_back(v.color(1)); vox.push_back(v.color(2));
        }
    }
    put(name + "/keys", 1, {ids.size(), 3}, keys.data());
    put(name + "/voxels", 0, {ids.size(), 512, 5}, vox.data());
}

static CubeMap map_of(const Arr& keys, const Arr& vox) {
    CubeMap map;
    const size_t n = (size_t)keys.dims[0];
    for (size_t b = 0; b < n; ++b) {
        const CubeID id(keys.i()[3 * b], keys.i()[3 * b + 1], keys.i()[3 * b + 2]);
        VoxelCube cube(id);
        for (size_t v = 0; v < 512; ++v) {
            const float* t = vox.f() + (b * 512 + v) * 5;
            cube.voxels[v].sdf = t[0];
            cube.voxels[v].weight = t[1];
            cube.voxels[v].color = geometry::Point3(t[2], t[3], t[4]);
        }
        map[id] = cube;
    }
    return map;
}

static void put_mesh(const std::string& name, const geometry::TriangleMesh& mesh) {
    std::vector<float> p, c;
    for (const auto& x : mesh.points) for (int k = 0; k < 3; ++k) p.push_back(x(k));
    for (const auto& x : mesh.colors) for (int k = 0; k < 3; ++k) c.push_back(x(k));
    put(name + "/points", 0, {mesh.points.size(), 3}, p.data());
    put(name + "/colors", 0, {mesh.colors.size(), 3}, c.data());
}

// params: fx fy cx cy width height depth_scale resolution truncation far near
static void configure(CubeHandler& h, const float* p) {
    camera::PinholeCamera cam;
    cam.SetPara(p[0], p[1], p[2], p[3], (int)p[4], (int)p[5], p[6]);
    h.SetCamera(cam);
    h.SetVoxelResolution(p[7]);
    h.SetTruncation(p[8]);
    h.SetFarPlane(p[9]);
    h.SetNearPlane(p[10]);
}

// fusion: params, depth [n,h,w] u16 | f32, rgb [n,h,w,3] u8, poses [n,16] -> per frame the cube_id_list of PrepareCubes and the volume
static void run_fusion(const Bag& in) {
    CubeHandler h;
    configure(h, in.at("params").f());
    const Arr& depth = in.at("depth");
    const Arr& rgb = in.at("rgb");
    const size_t n = (size_t)depth.dims[0];
    const int rows = (int)depth.dims[1], cols = (int)depth.dims[2];
    const bool u16 = depth.type == 3;
    for (size_t f = 0; f < n; ++f) {
        cv::Mat d(rows, cols, u16 ? CV_16UC1 : CV_32FC1), c(rows, cols, CV_8UC3);
        std::memcpy(d.data, depth.bytes.data() + f * (size_t)rows * cols * (u16 ? 2 : 4), (size_t)rows * cols * (u16 ? 2 : 4));
        std::memcpy(c.data, rgb.bytes.data() + f * (size_t)rows * cols * 3, (size_t)rows * cols * 3);
        const geometry::TransformationMatrix pose = matrix_of(in.at("poses").f() + 16 * f);
        std::vector<CubeID> list;
        h.PrepareCubes(d, pose, list); // allocates what IntegrateImage's own PrepareCubes would
        std::vector<int32_t> ids;
        for (const CubeID& id : list) for (int k = 0; k < 3; ++k) ids.push_back(id(k));
        put("frame" + std::to_string(f) + "/cube_id_list", 1, {list.size(), 3}, ids.data());
        h.IntegrateImage(d, c, pose);
        put_volume("frame" + std::to_string(f), h);
    }
}

// a volume A (params, keys, voxels) and what the other arrays ask for
static void run_volume(const Bag& in, const std::string& dir) {
    CubeHandler a;
    configure(a, in.at("params").f());
    a.SetCubeMap(map_of(in.at("keys"), in.at("voxels")));
    if (in.count("transforms")) {
        const Arr& T = in.at("transforms");
        for (size_t k = 0; k < (size_t)T.dims[0]; ++k) {
            const geometry::TransformationMatrix M = matrix_of(T.f() + 16 * k);
            auto t = a.Transform(M);
            put_volume("transform" + std::to_string(k), *t);
            auto n = a.TransformNearest(M);
            put_volume("nearest" + std::to_string(k), *n);
        }
    }
    if (in.count("other_keys")) { // Merge(another) [, trans]; other_params[7] may differ: the refused merge
        CubeHandler b, dst;
        configure(b, in.at("other_params").f());
        b.SetCubeMap(map_of(in.at("other_keys"), in.at("other_voxels")));
        configure(dst, in.at("params").f());
        dst.SetCubeMap(a.GetCubeMap());
        if (in.count("merge_transform")) dst.Merge(b, matrix_of(in.at("merge_transform").f()));
        else dst.Merge(b);
        put_volume("merged", dst);
    }
    if (in.count("point_cloud")) {
        auto pcd = a.GetPointCloud();
        std::vector<float> p, c;
        for (const auto& x : pcd->points) for (int k = 0; k < 3; ++k) p.push_back(x(k));
        for (const auto& x : pcd->colors) for (int k = 0; k < 3; ++k) c.push_back(x(k));
        put("point_cloud/points", 0, {pcd->points.size(), 3}, p.data());
        put("point_cloud/colors", 0, {pcd->colors.size(), 3}, c.data());
    }
    if (in.count("mesh")) {
        const std::vector<CubeID> ids = sorted_ids(a.GetCubeMap());
        for (size_t k = 0; k < ids.size(); ++k) {
            geometry::TriangleMesh mesh;
            a.GenerateMeshByCube(ids[k], mesh);
            put_mesh("block_mesh" + std::to_string(k), mesh);
        }
        geometry::TriangleMesh whole;
        a.ExtractTriangleMesh(whole);
        put_mesh("mesh", whole);
    }
    if (in.count("map_file")) {
        const std::string path = dir + "/volume.map";
        a.WriteToFile(path);
        std::ifstream is(path.c_str(), std::ios::binary);
        std::vector<char> bytes((std::istreambuf_iterator<char>(is)), std::istreambuf_iterator<char>());
        put("map_file/bytes", 2, {bytes.size()}, bytes.data());
        CubeHandler r;
        configure(r, in.at("params").f());
        r.ReadFromFile(path);
        put_volume("map_file", r);
    }
    if (in.count("add_cubes")) {
        const Arr& ids = in.at("add_cubes");
        std::vector<int32_t> counts;
        for (size_t k = 0; k < (size_t)ids.dims[0]; ++k) {
            a.AddCube(CubeID(ids.i()[3 * k], ids.i()[3 * k + 1], ids.i()[3 * k + 2]));
            counts.push_back((int32_t)a.GetCubeMap().size());
        }
        put("add_cubes/counts", 1, {counts.size()}, counts.data());
        put_volume("add_cubes", a);
    }
    if (in.count("legacy_stream")) {
        const std::string path = dir + "/legacy.map";
        { std::ofstream os(path.c_str(), std::ios::binary); os.write((const char*)in.at("legacy_stream").bytes.data(), (std::streamsize)in.at("legacy_stream").bytes.size()); }
        CubeHandler r;
        r.ReadFromFileFloat(path);
        put_volume("legacy", r);
    }
}

int main(int argc, char** argv) {
    if (argc != 4) { std::cerr << "usage: volume_golden IN OUT SCRATCH_DIR" << std::endl; return 2; }
    std::cout.setstate(std::ios::failbit); // the reference prints a line per call
    const Bag in = read_bag(argv[1]);
    g_out.open(argv[2], std::ios::binary);
    if (in.count("tables")) {
        std::vector<int32_t> tri, pairs;
        for (int r = 0; r < 256; ++r) for (int c = 0; c < 16; ++c) tri.push_back(integration::MCLookTable[r][c]);
        for (int r = 0; r < 12; ++r) for (int c = 0; c < 2; ++c) pairs.push_back(integration::EdgeIndexPairs[r][c]);
        put("tables/tri_table", 1, {256, 16}, tri.data());
        put("tables/edge_pairs", 1, {12, 2}, pairs.data());
    }
    if (in.count("depth")) run_fusion(in);
    if (in.count("keys")) run_volume(in, argv[3]);
    g_out.close();
    return g_out ? 0 : 1;
}
