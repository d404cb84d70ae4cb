// ModelQuery.cpp -- asking the fused model what it holds at given points.  N frames of the analytic room are fused; then a batch of points is
// sampled, either on the device (op_volume_sample: one call, the volume never leaves HBM) or the only way there was before it: GetCubeMap() -- the
// whole pool to the host -- and a host loop of the same definition over a hash map.  Both paths produce the same bytes.
//
//   ModelQuery --synthetic N STRIDE SEED [--res 0.01] [--queries mesh|mesh-shuffled|frame] [--mode trilinear|reference] [--gradients]
//              [--path host|device] [--warmup W] [--repeat K] [--dump DIR]
//   --synthetic N STRIDE SEED  N frames of the analytic room of LiveFusion.cpp: frame k is step FIRST + k * STRIDE of a 1000-step orbit, SEED picks FIRST
//   --queries                  mesh (default): the vertices of the model's own extracted mesh, block by block (sorted by block, then by coordinates: the
//                              same batch in every run); mesh-shuffled: the same vertices in a fixed pseudo-random order; frame: the camera-frame points of the middle
//                              frame's depth image, with its pose passed as T
//   --mode                     trilinear (default): the raycaster's strict trilinear sample; reference: VoxelCube::ReadVoxelInterpolate
//   --gradients                also the central-difference gradient of the trilinear sdf (trilinear only)
//   --path                     device (default) or host
//   --warmup W --repeat K      W untimed and K timed repetitions of the query (defaults 0 and 1); the median, minimum and maximum are printed
//   --dump DIR                 writes DIR/voxels.bin (n x 5 float32), DIR/status.bin (n bytes) and, with --gradients, DIR/gradients.bin (n x 3 float32)
// It prints one JSON line: the stage times (host clock, each stage waited for), the statistics of the batch, and the bytes the algorithm has to move
// per query (12 in; 64 of sdf and weight taps, 96 of colour taps, 192 more for a gradient's 24 extra taps; 20, 12 and 1 out).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <unordered_map>
#include <vector>

#include "Geometry/Geometry.h"
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

// ---- the host path: the definition of op_volume_sample (include/onepiece_hip.h) over a CubeMap, every operation one float32 operation --------------
struct Vox { float s, w, c0, c1, c2; };
const Vox kDefault = {999.0f, 0.0f, -1.0f, -1.0f, -1.0f};
const float kLimit = 8388600.0f;

struct HostModel {
    integration::CubeMap map;
    const integration::VoxelCube* last;
    int lx, ly, lz;
    float res;
    explicit HostModel(float r) : last(nullptr), lx(0), ly(0), lz(0), res(r) {}
    // the voxel at integer voxel coordinates p; false: its block is not held
    bool Fetch(int px, int py, int pz, Vox* out) {
        const int bx = px >> 3, by = py >> 3, bz = pz >> 3;
        if (!last || bx != lx || by != ly || bz != lz) {
            lx = bx; ly = by; lz = bz;
            integration::CubeMap::const_iterator it = map.find(integration::CubeID(bx, by, bz));
            last = it == map.end() ? nullptr : &it->second;
            if (!last) { lx = ly = lz = 0; }
        }
        if (!last) { *out = kDefault; return false; }
        const integration::TSDFVoxel& t = last->voxels[(px - bx * 8) + (py - by * 8) * 8 + (pz - bz * 8) * 64];
        out->s = t.sdf; out->w = t.weight; out->c0 = t.color(0); out->c1 = t.color(1); out->c2 = t.color(2);
        return true;
    }
};

bool InRange(float a, float b, float c) { return std::fabs(a) < kLimit && std::fabs(b) < kLimit && std::fabs(c) < kLimit; }

// the strict trilinear sample; `in_range` (may be null) tells an out-of-range g from an unobserved tap
bool Trilinear(HostModel& m, float x, float y, float z, Vox* out, bool* in_range) {
    const float inv = 1.0f / m.res;
    const float g0 = x * inv - 0.5f, g1 = y * inv - 0.5f, g2 = z * inv - 0.5f;
    const bool ok = InRange(g0, g1, g2);
    if (in_range) *in_range = ok;
    if (!ok) return false;
    const float b0 = std::floor(g0), b1 = std::floor(g1), b2 = std::floor(g2);
    const int i0 = static_cast<int>(b0), i1 = static_cast<int>(b1), i2 = static_cast<int>(b2);
    const float f0 = g0 - b0, f1 = g1 - b1, f2 = g2 - b2;
    Vox a = {0, 0, 0, 0, 0};
    for (int k = 0; k < 8; ++k) {
        Vox t;
        if (!m.Fetch(i0 + (k & 1), i1 + ((k >> 1) & 1), i2 + ((k >> 2) & 1), &t) || !(t.w > 0)) return false;
        const float wx = (k & 1) ? f0 : 1.0f - f0, wy = (k & 2) ? f1 : 1.0f - f1, wz = (k & 4) ? f2 : 1.0f - f2;
        const float w = (wx * wy) * wz;
        a.s += w * t.s; a.w += w * t.w; a.c0 += w * t.c0; a.c1 += w * t.c1; a.c2 += w * t.c2;
    }
    *out = a;
    return true;
}

Vox Scale(const Vox& a, float wgt) {
    if (wgt == 0 || a.w == 0) return kDefault;
    const Vox r = {a.s * wgt, a.w * wgt, a.c0 * wgt, a.c1 * wgt, a.c2 * wgt};
    return r;
}
Vox Add(const Vox& a, const Vox& b) {
    if (a.w == 0) return b;
    if (b.w == 0) return a;
    const Vox r = {a.s + b.s, a.w + b.w, a.c0 + b.c0, a.c1 + b.c1, a.c2 + b.c2};
    return r;
}
Vox Stage(const Vox& a, const Vox& b, float t) {
    if (!(a.w != 0 || b.w != 0)) return kDefault;
    const Vox sum = Add(Scale(a, 1 - t), Scale(b, t));
    const float d = (1 - t) * static_cast<float>(a.w != 0) + t * static_cast<float>(b.w != 0);
    return Scale(sum, 1 / d);
}

// VoxelCube::ReadVoxelInterpolate as CubeHandler::Transform evaluates it; false: out of range
bool Reference(HostModel& m, float x, float y, float z, Vox* out) {
    const float res = m.res, half = res / 2;
    const float n0 = x - half, n1 = y - half, n2 = z - half;
    const float e0 = n0 / res, e1 = n1 / res, e2 = n2 / res;
    if (!InRange(e0, e1, e2)) return false;
    const int p0 = static_cast<int>(std::floor(e0)), p1 = static_cast<int>(std::floor(e1)), p2 = static_cast<int>(std::floor(e2));
    Vox v[8];
    for (int k = 0; k < 8; ++k) m.Fetch(p0 + (k & 1), p1 + ((k >> 1) & 1), p2 + ((k >> 2) & 1), &v[k]);
    const float xw = (n0 - static_cast<float>(p0) * res) / res, yw = (n1 - static_cast<float>(p1) * res) / res, zw = (n2 - static_cast<float>(p2) * res) / res;
    const Vox z1 = Stage(Stage(v[0], v[1], xw), Stage(v[2], v[3], xw), yw);
    const Vox z2 = Stage(Stage(v[4], v[5], xw), Stage(v[6], v[7], xw), yw);
    *out = Stage(z1, z2, zw);
    return true;
}

void HostSample(HostModel& m, const std::vector<float>& xyz, const float* T, bool reference, bool gradients, std::vector<float>& voxels, std::vector<float>& grads,
                std::vector<uint8_t>& status, op_volume_sample_stats* st) {
    const size_t n = xyz.size() / 3;
    op_volume_sample_stats s = {n, 0, 0, 0, 0.0, 0.0, 0.0f};
    for (size_t i = 0; i < n; ++i) {
        float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        if (T) {
            const float q0 = ((T[0] * x + T[1] * y) + T[2] * z) + T[3] * 1.0f, q1 = ((T[4] * x + T[5] * y) + T[6] * z) + T[7] * 1.0f;
            const float q2 = ((T[8] * x + T[9] * y) + T[10] * z) + T[11] * 1.0f, q3 = ((T[12] * x + T[13] * y) + T[14] * z) + T[15] * 1.0f;
            x = q0 / q3; y = q1 / q3; z = q2 / q3;
        }
        unsigned stt = 0;
        Vox r = kDefault;
        float d[3] = {0.0f, 0.0f, 0.0f};
        if (!reference) {
            bool in_range = true;
            Vox got;
            if (Trilinear(m, x, y, z, &got, &in_range)) r = got; else stt |= OP_SAMPLE_INVALID;
            if (!in_range) stt |= OP_SAMPLE_OUT_OF_RANGE | (gradients ? OP_SAMPLE_NO_GRADIENT : 0);
            else if (gradients) {
                const float h = 0.5f * m.res;
                bool all = true;
                for (int a = 0; a < 3 && all; ++a) {
                    Vox sp, sm;
                    all = Trilinear(m, x + (a == 0 ? h : 0.0f), y + (a == 1 ? h : 0.0f), z + (a == 2 ? h : 0.0f), &sp, nullptr) &&
                          Trilinear(m, x - (a == 0 ? h : 0.0f), y - (a == 1 ? h : 0.0f), z - (a == 2 ? h : 0.0f), &sm, nullptr);
                    if (all) d[a] = sp.s - sm.s;
                }
                if (!all) { d[0] = d[1] = d[2] = 0.0f; stt |= OP_SAMPLE_NO_GRADIENT; }
            }
        } else {
            if (!Reference(m, x, y, z, &r)) { r = kDefault; stt |= OP_SAMPLE_INVALID | OP_SAMPLE_OUT_OF_RANGE; }
            else if (r.w == 0) stt |= OP_SAMPLE_INVALID;
        }
        voxels[5 * i] = r.s; voxels[5 * i + 1] = r.w; voxels[5 * i + 2] = r.c0; voxels[5 * i + 3] = r.c1; voxels[5 * i + 4] = r.c2;
        if (gradients) { grads[3 * i] = d[0]; grads[3 * i + 1] = d[1]; grads[3 * i + 2] = d[2]; }
        status[i] = static_cast<uint8_t>(stt);
        if (!(stt & OP_SAMPLE_INVALID)) {
            ++s.valid;
            s.sum_abs_sdf += static_cast<double>(std::fabs(r.s));
            s.sum_sq_sdf += static_cast<double>(r.s) * static_cast<double>(r.s);
            s.max_abs_sdf = std::fmax(s.max_abs_sdf, std::fabs(r.s));
        }
        if (gradients && !(stt & OP_SAMPLE_NO_GRADIENT)) ++s.gradients;
        if (stt & OP_SAMPLE_OUT_OF_RANGE) ++s.out_of_range;
    }
    *st = s;
}

bool WriteFile(const std::string& file, const void* data, size_t bytes) {
    FILE* f = fopen(file.c_str(), "wb");
    if (!f) return false;
    const bool ok = bytes == 0 || fwrite(data, 1, bytes, f) == bytes;
    return fclose(f) == 0 && ok;
}

} // namespace

int main(int argc, char* argv[]) {
    long synthetic[3] = {0, 1, 1}, warmup = 0, repeat = 1;
    bool is_synthetic = false, bad = false, gradients = false;
    std::string queries = "mesh", mode = "trilinear", path = "device", dump;
    float res = 0.01f;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--synthetic" && i + 3 < argc) { is_synthetic = true; for (int k = 0; k < 3; ++k) synthetic[k] = std::atol(argv[++i]); }
        else if (a == "--res" && i + 1 < argc) res = static_cast<float>(std::atof(argv[++i]));
        else if (a == "--queries" && i + 1 < argc) queries = argv[++i];
        else if (a == "--mode" && i + 1 < argc) mode = argv[++i];
        else if (a == "--gradients") gradients = true;
        else if (a == "--path" && i + 1 < argc) path = argv[++i];
        else if (a == "--warmup" && i + 1 < argc) warmup = std::atol(argv[++i]);
        else if (a == "--repeat" && i + 1 < argc) repeat = std::atol(argv[++i]);
        else if (a == "--dump" && i + 1 < argc) dump = argv[++i];
        else bad = true;
    }
    const long n = synthetic[0], stride = synthetic[1];
    if (bad || !is_synthetic || n < 1 || stride < 1 || synthetic[2] < 0 || !(res > 0) || warmup < 0 || repeat < 1 ||
        (queries != "mesh" && queries != "mesh-shuffled" && queries != "frame") || (mode != "trilinear" && mode != "reference") || (path != "host" && path != "device") ||
        (gradients && mode == "reference")) {
        std::cout << "usage::ModelQuery --synthetic N STRIDE SEED [--res 0.01] [--queries mesh|mesh-shuffled|frame] [--mode trilinear|reference] [--gradients] [--path host|device] "
                     "[--warmup W] [--repeat K] [--dump DIR]" << std::endl;
        return bad || argc > 1 ? 2 : 0;
    }
    const long first = ((synthetic[2] + 999) % 1000) * 97 % 1000;
    const bool reference = mode == "reference";

    camera::PinholeCamera camera;
    camera.SetCameraType(camera::CameraType::OPEN3D_DATASET);
    integration::CubeHandler volume(camera);
    volume.SetVoxelResolution(res);
    if (!volume.Handle()) return 1; // (no device: the class has said so)

    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    cv::Mat mid_depth;
    geometry::TransformationMatrix mid_pose = geometry::TransformationMatrix::Identity();
    for (long k = 0; k < n; ++k) {
        cv::Mat depth, rgb;
        const geometry::TransformationMatrix pose = RoomPose(first + k * stride);
        RoomRender(pose, camera, depth, rgb);
        volume.IntegrateImage(depth, rgb, pose);
        if (k == n / 2) { mid_depth = depth.clone(); mid_pose = pose; }
    }
    volume.Synchronize();
    const double t_fuse = Seconds(t0);

    // the batch
    t0 = std::chrono::steady_clock::now();
    std::vector<float> xyz;
    float T[16];
    const float* Tp = nullptr;
    if (queries == "frame") {
        const int w = mid_depth.cols, h = mid_depth.rows;
        const float fx = camera.GetFx(), fy = camera.GetFy(), cx = camera.GetCx(), cy = camera.GetCy();
        for (int v = 0; v < h; ++v)
            for (int u = 0; u < w; ++u) {
                const float z = mid_depth.at<float>(v, u);
                if (!(z > 0)) continue;
                xyz.push_back((static_cast<float>(u) - cx) * z / fx); xyz.push_back((static_cast<float>(v) - cy) * z / fy); xyz.push_back(z);
            }
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) T[4 * r + c] = mid_pose(r, c);
        Tp = T;
    } else {
        geometry::TriangleMesh mesh;
        volume.ExtractTriangleMesh(mesh);
        const size_t nv = mesh.points.size();
        // The mesh comes block by block in pool order, which differs from run to run (blocks are claimed concurrently); its vertices as a set do not.
        // Sorted by the block a vertex lies in, then by its coordinates, the batch is the same in every run and still block-major.
        std::vector<size_t> order(nv);
        for (size_t i = 0; i < nv; ++i) order[i] = i;
        const float block_len = 8.0f * res;
        std::vector<float> key(6 * nv);
        for (size_t i = 0; i < nv; ++i)
            for (int c = 0; c < 3; ++c) { key[6 * i + c] = std::floor(mesh.points[i](c) / block_len); key[6 * i + 3 + c] = mesh.points[i](c); }
        std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return std::lexicographical_compare(key.begin() + 6 * a, key.begin() + 6 * a + 6, key.begin() + 6 * b, key.begin() + 6 * b + 6); });
        if (queries == "mesh-shuffled") { // Fisher-Yates with a fixed 64-bit LCG
            unsigned long long s = 0x9E3779B97F4A7C15ULL;
            for (size_t i = nv; i > 1; --i) {
                s = s * 6364136223846793005ULL + 1442695040888963407ULL;
                std::swap(order[i - 1], order[static_cast<size_t>((s >> 33) % i)]);
            }
        }
        xyz.resize(3 * nv);
        for (size_t i = 0; i < nv; ++i)
            for (int c = 0; c < 3; ++c) xyz[3 * i + c] = mesh.points[order[i]](c);
    }
    const double t_batch = Seconds(t0);
    const size_t nq = xyz.size() / 3;

    std::vector<float> voxels(5 * nq), grads(gradients ? 3 * nq : 0);
    std::vector<uint8_t> status(nq);
    op_volume_sample_stats st = {0, 0, 0, 0, 0.0, 0.0, 0.0f};
    std::vector<double> sample_s, download_s;
    size_t blocks = volume.GetCubeCount();
    for (long pass = -warmup; pass < repeat; ++pass) {
        double t_down = 0;
        t0 = std::chrono::steady_clock::now();
        if (path == "device") {
            if (nq && op_volume_sample(volume.Handle(), xyz.data(), nq, OP_MEM_HOST, Tp, reference ? OP_SAMPLE_REFERENCE : OP_SAMPLE_TRILINEAR, voxels.data(),
                                       gradients ? grads.data() : nullptr, status.data(), &st) != OP_OK) {
                std::cout << RED << "[ERROR]::op_volume_sample failed: " << op_last_error() << RESET << std::endl;
                return 1;
            }
        } else {
            HostModel model(res);
            model.map = volume.GetCubeMap();
            t_down = Seconds(t0);
            HostSample(model, xyz, Tp, reference, gradients, voxels, grads, status, &st);
        }
        if (pass >= 0) { sample_s.push_back(Seconds(t0)); download_s.push_back(t_down); }
    }
    std::sort(sample_s.begin(), sample_s.end());
    std::sort(download_s.begin(), download_s.end());

    if (!dump.empty()) {
        bool ok = WriteFile(dump + "/voxels.bin", voxels.data(), voxels.size() * sizeof(float)) && WriteFile(dump + "/status.bin", status.data(), status.size());
        if (gradients) ok = ok && WriteFile(dump + "/gradients.bin", grads.data(), grads.size() * sizeof(float));
        if (!ok) { std::cout << RED << "[ERROR]::cannot write the dumps under " << dump << RESET << std::endl; return 1; }
    }
    const unsigned long long bytes_per_query = 12 + 64 + 96 + (gradients ? 192 + 12 : 0) + 20 + 1;
    std::cout << "{\"frames\": " << n << ", \"stride\": " << stride << ", \"first\": " << first << ", \"res\": " << res << ", \"queries\": \"" << queries << "\", \"mode\": \"" << mode
              << "\", \"gradients\": " << (gradients ? "true" : "false") << ", \"path\": \"" << path << "\", \"blocks\": " << blocks << ", \"n\": " << nq
              << ", \"warmup\": " << warmup << ", \"repeat\": " << repeat << ", \"ms\": {\"fuse\": " << t_fuse * 1000.0 << ", \"batch\": " << t_batch * 1000.0
              << ", \"sample\": " << sample_s[sample_s.size() / 2] * 1000.0 << ", \"sample_min_max\": [" << sample_s.front() * 1000.0 << ", " << sample_s.back() * 1000.0
              << "], \"get_cube_map\": " << download_s[download_s.size() / 2] * 1000.0 << "}"
              << ", \"stats\": {\"queries\": " << st.queries << ", \"valid\": " << st.valid << ", \"gradients\": " << st.gradients << ", \"out_of_range\": " << st.out_of_range
              << ", \"sum_abs_sdf\": " << st.sum_abs_sdf << ", \"sum_sq_sdf\": " << st.sum_sq_sdf << ", \"max_abs_sdf\": " << st.max_abs_sdf << "}"
              << ", \"algorithm_bytes_per_query\": " << bytes_per_query << ", \"algorithm_bytes\": " << bytes_per_query * nq << "}" << std::endl;
    return 0;
}
