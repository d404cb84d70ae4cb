// ModelLod.cpp -- a fused model at half and quarter resolution.  N frames of the analytic room are fused; then the model is coarsened level by level
// (CubeHandler::Coarsen; op_volume_coarsen states the definition: a voxel of twice the size is the weighted mean of the 2 x 2 x 2 fine voxels it
// covers exactly) and every level is meshed, rendered and compared with the fine model.
//
//   ModelLod --synthetic N STRIDE SEED [--res 0.01] [--levels 1] [--min-weight 0] [--path device|host] [--out DIR] [--warmup 0] [--repeat 1]
//   --synthetic N STRIDE SEED  N frames of the analytic room of LiveFusion.cpp: frame k is step FIRST + k * STRIDE of a 1000-step orbit, SEED picks FIRST
//   --levels L                 1..4 levels, each coarsened from the one before
//   --min-weight W             fine voxels below this weight do not contribute
//   --path device (default)    CubeHandler::Coarsen: one claim per source block, one workgroup per result block, on the device
//   --path host                what there was before it: GetCubeMap(), a loop over the hash map that states the definition in plain C++, SetCubeMap
//                              into a fresh handler of twice the voxel size
//   --out DIR                  the last level's blocks sorted by id, DIR/lod_PATH.blocks: per block three int32 and 512 x {sdf, weight, colour} float32;
//                              the two paths write the same bytes
//   --warmup A --repeat B      the coarsening of every level is run A + B times, the last B are timed (median, minimum, maximum)
// It prints one JSON line per level (0 = the fused model): blocks, pool bytes, the counts, the time of the coarsening, time and triangles of
// ExtractTriangleMesh, the time of one RenderFrame at the first frame's pose, and the fidelity: CubeHandler::DistanceToModel of the FINE model's mesh
// vertices against the level -- rmse and 95th percentile of |sdf| over the valid ones, and the share that is invalid.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "Geometry/Geometry.h"
#include "Geometry/PointCloud.h"
#include "Geometry/TriangleMesh.h"
#include "Integration/CubeHandler.h"
#include "onepiece_hip.h"
using namespace one_piece;

namespace {

const double kPi = 3.14159265358979323846;
const float kRoomHalf[3] = {2.6f, 1.4f, 2.6f};
const float kSpheres[2][4] = {{1.2f, 0.7f, 1.6f, 0.55f}, {-1.4f, 0.5f, -1.1f, 0.7f}};

// camera-to-world pose of orbit step i: radius 0.4 m, looking outward, a slow pitch
geometry::TransformationMatrix RoomPose(long i) {
    const double th = 2.0 * kPi * static_cast<double>(i % 1000) / 1000.0;
    const long loop = i / 1000;
    const double radius = 0.4 + 0.05 * static_cast<double>(loop % 8), pitch = 0.12 * std::sin(2.0 * th + 0.3 * static_cast<double>(loop));
    const double cy = std::cos(th), sy = std::sin(th), cp = std::cos(pitch), sp = std::sin(pitch);
    const double Ry[3][3] = {{cy, 0, sy}, {0, 1, 0}, {-sy, 0, cy}}, Rx[3][3] = {{1, 0, 0}, {0, cp, -sp}, {0, sp, cp}};
    geometry::TransformationMatrix T = geometry::TransformationMatrix::Identity();
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) T(r, c) = static_cast<float>(Ry[r][0] * Rx[0][c] + Ry[r][1] * Rx[1][c] + Ry[r][2] * Rx[2][c]);
    T(0, 3) = static_cast<float>(radius * sy);
    T(1, 3) = static_cast<float>(0.15 * std::sin(3.0 * th));
    T(2, 3) = static_cast<float>(radius * cy);
    return T;
}

float Slab(float o, float d, float half) {
    if (!(std::fabs(d) > 1e-9f)) return 1e9f;
    return ((d > 0 ? half : -half) - o) / d;
}

// the room seen from `pose`: z-depth in metres (CV_32FC1) and a colour that depends on the surface point alone (CV_8UC3)
void RoomRender(const geometry::TransformationMatrix& pose, const camera::PinholeCamera& cam, cv::Mat& depth, cv::Mat& rgb) {
    const int w = static_cast<int>(cam.GetWidth()), h = static_cast<int>(cam.GetHeight());
    depth.create(h, w, CV_32FC1);
    rgb.create(h, w, CV_8UC3);
    const float fx = cam.GetFx(), fy = cam.GetFy(), cx = cam.GetCx(), cy = cam.GetCy();
    const float ox = pose(0, 3), oy = pose(1, 3), oz = pose(2, 3);
    for (int v = 0; v < h; ++v)
        for (int u = 0; u < w; ++u) {
            const float a = (static_cast<float>(u) - cx) / fx, b = (static_cast<float>(v) - cy) / fy;
            const float dx = pose(0, 0) * a + pose(0, 1) * b + pose(0, 2), dy = pose(1, 0) * a + pose(1, 1) * b + pose(1, 2), dz = pose(2, 0) * a + pose(2, 1) * b + pose(2, 2);
            float t = std::fmin(std::fmin(Slab(ox, dx, kRoomHalf[0]), Slab(oy, dy, kRoomHalf[1])), Slab(oz, dz, kRoomHalf[2]));
            const float dd = dx * dx + dy * dy + dz * dz;
            for (int s = 0; s < 2; ++s) {
                const float lx = ox - kSpheres[s][0], ly = oy - kSpheres[s][1], lz = oz - kSpheres[s][2];
                const float bb = dx * lx + dy * ly + dz * lz, cc = lx * lx + ly * ly + lz * lz - kSpheres[s][3] * kSpheres[s][3];
                const float disc = bb * bb - dd * cc;
                if (disc > 0) {
                    const float ts = (-bb - std::sqrt(disc)) / dd;
                    if (ts > 0.05f && ts < t) t = ts;
                }
            }
            const float hx = ox + t * dx, hy = oy + t * dy, hz = oz + t * dz;
            const float r = 128.0f + 110.0f * std::sin(3.1f * hx + 0.7f * hy), g = 128.0f + 110.0f * std::sin(2.3f * hy + 1.9f * hz), bl = 128.0f + 110.0f * std::sin(2.7f * hz - 1.3f * hx);
            depth.at<float>(v, u) = t;
            unsigned char* px = rgb.data + 3 * (static_cast<size_t>(v) * w + u); // stored order B, G, R like cv::imread
            px[0] = static_cast<unsigned char>(std::fmin(std::fmax(bl, 0.0f), 255.0f));
            px[1] = static_cast<unsigned char>(std::fmin(std::fmax(g, 0.0f), 255.0f));
            px[2] = static_cast<unsigned char>(std::fmin(std::fmax(r, 0.0f), 255.0f));
        }
}

double Seconds(std::chrono::steady_clock::time_point a) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - a).count(); }

int Half(int b) { return b >= 0 ? b / 2 : -((-b + 1) / 2); } // the arithmetic shift b >> 1: -1, -2, -3 -> -1, -1, -2

// One level of op_volume_coarsen's definition over the host map, in plain C++: the children of a coarse voxel in the order c = i + 2j + 4k, a
// child contributes iff w > 0 && w >= min_weight, every product and every sum a float operation of its own, starting from 0.
integration::CubeMap HostCoarsen(const integration::CubeMap& fine, float min_weight, op_volume_coarsen_stats* st) {
    integration::CubeMap coarse;
    for (integration::CubeMap::const_iterator it = fine.begin(); it != fine.end(); ++it) {
        const integration::CubeID id(Half(it->first(0)), Half(it->first(1)), Half(it->first(2)));
        if (coarse.find(id) == coarse.end()) coarse.insert(std::make_pair(id, integration::VoxelCube(id)));
    }
    *st = op_volume_coarsen_stats();
    st->src_blocks = fine.size();
    st->dst_blocks = coarse.size();
    for (integration::CubeMap::iterator it = coarse.begin(); it != coarse.end(); ++it) {
        const integration::VoxelCube* src[8];
        for (int b = 0; b < 8; ++b) {
            const integration::CubeID id(2 * it->first(0) + (b & 1), 2 * it->first(1) + ((b >> 1) & 1), 2 * it->first(2) + (b >> 2));
            integration::CubeMap::const_iterator f = fine.find(id);
            src[b] = f == fine.end() ? nullptr : &f->second;
        }
        for (int v = 0; v < 512; ++v) {
            const int x = v & 7, y = (v >> 3) & 7, z = v >> 6;
            const integration::VoxelCube* from = src[(x >> 2) + 2 * (y >> 2) + 4 * (z >> 2)];
            volatile float W = 0.0f, S = 0.0f, C0 = 0.0f, C1 = 0.0f, C2 = 0.0f; // (volatile: every sum is stored as a float before the next one)
            int n = 0;
            for (int c = 0; from && c < 8; ++c) {
                const int fx = 2 * (x & 3) + (c & 1), fy = 2 * (y & 3) + ((c >> 1) & 1), fz = 2 * (z & 3) + (c >> 2);
                const integration::TSDFVoxel& t = from->voxels[fx + 8 * fy + 64 * fz];
                const float w = t.weight;
                if (w > 0.0f && w >= min_weight) {
                    volatile float p;
                    W = W + w;
                    p = w * t.sdf; S = S + p;
                    p = w * t.color(0); C0 = C0 + p;
                    p = w * t.color(1); C1 = C1 + p;
                    p = w * t.color(2); C2 = C2 + p;
                    ++n;
                } else if (w > 0.0f) {
                    ++st->dropped_min_weight;
                }
            }
            integration::TSDFVoxel& o = it->second.voxels[v];
            if (n) {
                const float Wf = W;
                o.sdf = S / Wf; o.weight = Wf * 0.125f; o.color = geometry::Point3(C0 / Wf, C1 / Wf, C2 / Wf);
            } else {
                o = integration::TSDFVoxel();
            }
            if (n == 8) ++st->voxels_full; else if (n) ++st->voxels_partial; else ++st->voxels_empty;
        }
    }
    return coarse;
}

struct ById {
    bool operator()(const integration::VoxelCube* a, const integration::VoxelCube* b) const {
        for (int k = 0; k < 3; ++k)
            if (a->cube_id(k) != b->cube_id(k)) return a->cube_id(k) < b->cube_id(k);
        return false;
    }
};

bool Dump(integration::CubeHandler& volume, const std::string& file) {
    const integration::CubeMap map = volume.GetCubeMap();
    std::vector<const integration::VoxelCube*> blocks;
    for (integration::CubeMap::const_iterator it = map.begin(); it != map.end(); ++it) blocks.push_back(&it->second);
    std::sort(blocks.begin(), blocks.end(), ById());
    FILE* f = std::fopen(file.c_str(), "wb");
    if (!f) return false;
    for (size_t b = 0; b < blocks.size(); ++b) {
        const int32_t id[3] = {blocks[b]->cube_id(0), blocks[b]->cube_id(1), blocks[b]->cube_id(2)};
        std::fwrite(id, sizeof(int32_t), 3, f);
        for (int v = 0; v < 512; ++v) {
            const integration::TSDFVoxel& t = blocks[b]->voxels[v];
            const float rec[5] = {t.sdf, t.weight, t.color(0), t.color(1), t.color(2)};
            std::fwrite(rec, sizeof(float), 5, f);
        }
    }
    return std::fclose(f) == 0;
}

double Median(std::vector<double> v) {
    if (v.empty()) return 0.0;
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

} // namespace

int main(int argc, char* argv[]) {
    long synthetic[3] = {0, 1, 1}, levels = 1, warmup = 0, repeat = 1;
    bool is_synthetic = false, bad = false;
    std::string path = "device", out_dir;
    float res = 0.01f, min_weight = 0.0f;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--synthetic" && i + 3 < argc) { is_synthetic = true; for (int k = 0; k < 3; ++k) synthetic[k] = std::atol(argv[++i]); }
        else if (a == "--res" && i + 1 < argc) res = static_cast<float>(std::atof(argv[++i]));
        else if (a == "--levels" && i + 1 < argc) levels = std::atol(argv[++i]);
        else if (a == "--min-weight" && i + 1 < argc) min_weight = static_cast<float>(std::atof(argv[++i]));
        else if (a == "--path" && i + 1 < argc) path = argv[++i];
        else if (a == "--out" && i + 1 < argc) out_dir = argv[++i];
        else if (a == "--warmup" && i + 1 < argc) warmup = std::atol(argv[++i]);
        else if (a == "--repeat" && i + 1 < argc) repeat = std::atol(argv[++i]);
        else bad = true;
    }
    const long n = synthetic[0], stride = synthetic[1];
    if (bad || !is_synthetic || n < 1 || stride < 1 || synthetic[2] < 0 || !(res > 0) || levels < 1 || levels > 4 || !(min_weight >= 0) || (path != "device" && path != "host") ||
        warmup < 0 || repeat < 1) {
        std::cout << "usage::ModelLod --synthetic N STRIDE SEED [--res 0.01] [--levels 1] [--min-weight 0] [--path device|host] [--out DIR] [--warmup 0] [--repeat 1]" << std::endl;
        return bad || argc > 1 ? 2 : 0;
    }
    const long first = ((synthetic[2] + 999) % 1000) * 97 % 1000;

    camera::PinholeCamera camera;
    camera.SetCameraType(camera::CameraType::OPEN3D_DATASET);
    std::shared_ptr<integration::CubeHandler> fine = std::make_shared<integration::CubeHandler>(camera);
    fine->SetVoxelResolution(res);
    if (!fine->Handle()) return 1; // (no device: the class has said so)
    for (long k = 0; k < n; ++k) {
        cv::Mat depth, rgb;
        const geometry::TransformationMatrix pose = RoomPose(first + k * stride);
        RoomRender(pose, camera, depth, rgb);
        fine->IntegrateImage(depth, rgb, pose);
    }
    fine->Synchronize();
    const geometry::TransformationMatrix view = RoomPose(first);

    geometry::PointCloud fine_vertices; // the fine model's mesh vertices: what every level is measured against
    std::shared_ptr<integration::CubeHandler> cur = fine;
    float cur_res = res;
    for (long level = 0; level <= levels; ++level) {
        op_volume_coarsen_stats st = op_volume_coarsen_stats();
        std::vector<double> coarsen_ms;
        if (level > 0) {
            std::shared_ptr<integration::CubeHandler> next;
            for (long pass = -warmup; pass < repeat; ++pass) {
                next.reset();
                const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
                if (path == "device") {
                    next = cur->Coarsen(1, min_weight, &st);
                    if (!next) return 1;
                } else {
                    const integration::CubeMap coarse = HostCoarsen(cur->GetCubeMap(), min_weight, &st);
                    next = std::make_shared<integration::CubeHandler>(camera);
                    next->SetVoxelResolution(2.0f * cur_res);
                    next->SetCubeMap(coarse);
                    next->Synchronize();
                }
                if (pass >= 0) coarsen_ms.push_back(Seconds(t0) * 1000.0);
            }
            cur = next;
            cur_res = 2.0f * cur_res;
        }
        uint64_t max_blocks = 0;
        if (op_volume_growth_stats(cur->Handle(), &max_blocks, nullptr, nullptr) != OP_OK) return 1;
        float device_res = 0;
        if (op_volume_resolution(cur->Handle(), &device_res) != OP_OK) return 1;

        geometry::TriangleMesh mesh;
        std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
        cur->ExtractTriangleMesh(mesh);
        const double mesh_ms = Seconds(t0) * 1000.0;
        if (level == 0) fine_vertices.points = mesh.points;
        cv::Mat rgb, depth;
        cur->RenderFrame(view, rgb, depth); // (the first view also sizes the raycaster's buffers)
        t0 = std::chrono::steady_clock::now();
        const size_t seen = cur->RenderFrame(view, rgb, depth);
        const double render_ms = Seconds(t0) * 1000.0;

        // fidelity: |sdf| of the level at the fine model's vertices
        const op_volume_sample_stats d = cur->DistanceToModel(fine_vertices);
        std::vector<integration::TSDFVoxel> voxels;
        std::vector<uint8_t> status;
        cur->SampleVoxels(fine_vertices.points, voxels, status);
        std::vector<float> dist;
        for (size_t i = 0; i < voxels.size(); ++i)
            if (!(status[i] & OP_SAMPLE_INVALID)) dist.push_back(std::fabs(voxels[i].sdf));
        std::sort(dist.begin(), dist.end());
        const double p95 = dist.empty() ? 0.0 : dist[std::min(dist.size() - 1, static_cast<size_t>(0.95 * static_cast<double>(dist.size())))];
        const double rmse = d.valid ? std::sqrt(d.sum_sq_sdf / static_cast<double>(d.valid)) : 0.0;
        const double invalid = d.queries ? 1.0 - static_cast<double>(d.valid) / static_cast<double>(d.queries) : 0.0;

        std::vector<double> sorted = coarsen_ms;
        std::sort(sorted.begin(), sorted.end());
        std::printf("{\"level\": %ld, \"path\": \"%s\", \"res\": %.9g, \"blocks\": %zu, \"pool_bytes\": %llu, \"stats\": {\"src_blocks\": %llu, \"dst_blocks\": %llu, \"voxels_full\": %llu, "
                    "\"voxels_partial\": %llu, \"voxels_empty\": %llu, \"dropped_min_weight\": %llu}, \"coarsen_ms\": {\"median\": %.4f, \"min\": %.4f, \"max\": %.4f}, "
                    "\"mesh_ms\": %.3f, \"triangles\": %zu, \"render_ms\": %.3f, \"pixels_seen\": %zu, \"fidelity_vertices\": %llu, \"fidelity_rmse\": %.6g, \"fidelity_p95\": %.6g, "
                    "\"fidelity_invalid\": %.6g}\n",
                    level, path.c_str(), device_res, cur->GetCubeCount(), static_cast<unsigned long long>(max_blocks) * 10240ull, static_cast<unsigned long long>(st.src_blocks),
                    static_cast<unsigned long long>(st.dst_blocks), static_cast<unsigned long long>(st.voxels_full), static_cast<unsigned long long>(st.voxels_partial),
                    static_cast<unsigned long long>(st.voxels_empty), static_cast<unsigned long long>(st.dropped_min_weight), Median(coarsen_ms), sorted.empty() ? 0.0 : sorted.front(),
                    sorted.empty() ? 0.0 : sorted.back(), mesh_ms, mesh.triangles.size(), render_ms, seen, static_cast<unsigned long long>(d.queries), rmse, p95, invalid);
        std::fflush(stdout);
    }
    if (!out_dir.empty() && !Dump(*cur, out_dir + "/lod_" + path + ".blocks")) {
        std::cout << RED << "[ERROR]::cannot write to " << out_dir << RESET << std::endl;
        return 1;
    }
    return 0;
}
