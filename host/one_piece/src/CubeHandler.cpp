// CubeHandler.cpp -- integration::CubeHandler over the C-ABI (include/onepiece_hip.h).  See the header for the contract.
#include "Integration/CubeHandler.h"

#include <cmath>
#include <unordered_set>

#include "Bridge.h"
#include "DeviceFrame.h"

namespace one_piece {
namespace integration {

using bridge::Failed;

void CubeHandler::Report(const char* where) { std::cout << RED << "[ERROR]::[CubeHandler::" << where << "]::" << op_last_error() << RESET << std::endl; }

bool CubeHandler::Ensure() const {
    if (vol) return true;
    const int rc = op_volume_create(&camera.Pod(), c_para.VoxelResolution, integrator.truncation, far, near, bridge::Device(), 0, &vol);
    if (rc != OP_OK) { Report("create"); vol = nullptr; return false; }
    return true;
}

CubeHandler::CubeHandler() : cube_map(this) { c_para.InitializeVoxelCube(); }
CubeHandler::CubeHandler(const camera::PinholeCamera& _camera) : camera(_camera), cube_map(this) { c_para.InitializeVoxelCube(); }

// ---- the protected cube_map mirror -----------------------------------------------------------------------------------
const CubeMap& CubeMapMirror::get() const {
    if (!edited && seen != owner->changes) { // stale: the volume changed on the device since the last look
        host = owner->GetCubeMap();          // (commits nothing: `edited` is false here)
        seen = owner->changes;
    }
    return host;
}
CubeMap& CubeMapMirror::edit() {
    get();
    edited = true;
    return host;
}
void CubeHandler::Pending() const {
    if (cube_map.edited) const_cast<CubeHandler*>(this)->CommitCubeMap();
}
void CubeHandler::CommitCubeMap() {
    if (!cube_map.edited) return;
    cube_map.edited = false; // first: the upload below goes through members that call Pending()
    if (!Ensure()) return;
    if (op_volume_clear(vol) != OP_OK) { Report("CommitCubeMap"); return; }
    std::vector<int32_t> keys;
    std::vector<float> vox;
    keys.reserve(3 * cube_map.host.size());
    vox.reserve(cube_map.host.size() * 512 * 5);
    for (CubeMap::const_iterator it = cube_map.host.begin(); it != cube_map.host.end(); ++it) {
        for (int k = 0; k < 3; ++k) keys.push_back(it->first(k));
        for (int v = 0; v < 512; ++v) {
            const TSDFVoxel& t = it->second.voxels[v];
            const float rec[5] = {t.sdf, t.weight, t.color(0), t.color(1), t.color(2)};
            vox.insert(vox.end(), rec, rec + 5);
        }
    }
    if (!keys.empty() && op_volume_upload(vol, keys.data(), vox.data(), keys.size() / 3) != OP_OK) Report("CommitCubeMap");
    Touch();
    cube_map.seen = changes; // the mirror IS the volume's content
}

CubeHandler::CubeHandler(op_volume* adopted, const CubeHandler& like, float resolution)
    : camera(like.camera), integrator(like.integrator), far(like.far), near(like.near), cube_map(this), vol(adopted) {
    c_para.VoxelResolution = resolution;
    c_para.InitializeVoxelCube();
}

// value semantics: the copy owns its own device volume with the same content (Merge into an empty volume copies
// every block verbatim)
CubeHandler::CubeHandler(const CubeHandler& other)
    : camera(other.camera), integrator(other.integrator), c_para(other.c_para), far(other.far), near(other.near), cube_map(this) {
    other.Pending();
    if (other.vol && Ensure() && op_volume_merge(vol, other.vol) != OP_OK) Report("copy");
}
CubeHandler& CubeHandler::operator=(const CubeHandler& other) {
    if (this == &other) return *this;
    other.Pending();
    cube_map.edited = false; // whatever was pending here is overwritten
    Touch();
    if (vol) { op_volume_destroy(vol); vol = nullptr; borrowed_.clear(); } // (the destroy synchronised: nothing reads the borrowed device frames any more)
    camera = other.camera; integrator = other.integrator; c_para = other.c_para; far = other.far; near = other.near;
    if (other.vol && Ensure() && op_volume_merge(vol, other.vol) != OP_OK) Report("assign");
    return *this;
}
CubeHandler::~CubeHandler() {
    if (vol) op_volume_destroy(vol);
}

op_volume* CubeHandler::Handle() const { Pending(); Touch(); return Ensure() ? vol : nullptr; } // (the caller may change the volume through the handle)

void CubeHandler::SetVoxelResolution(float resolution) {
    Pending();
    c_para.SetVoxelResolution(resolution);
    if (vol && op_volume_set_resolution(vol, resolution) != OP_OK) Report("SetVoxelResolution");
}
void CubeHandler::SetTruncation(float trunc) {
    integrator.SetTruncation(trunc);
    if (vol && op_volume_set_truncation(vol, trunc) != OP_OK) Report("SetTruncation");
}
void CubeHandler::SetCamera(const camera::PinholeCamera& _camera) {
    camera = _camera;
    if (vol && op_volume_set_camera(vol, &camera.Pod()) != OP_OK) Report("SetCamera");
}
void CubeHandler::SetFarPlane(float _far) {
    far = _far;
    if (vol && op_volume_set_near_far(vol, near, far) != OP_OK) Report("SetFarPlane");
}
void CubeHandler::SetNearPlane(float _near) {
    near = _near;
    if (vol && op_volume_set_near_far(vol, near, far) != OP_OK) Report("SetNearPlane");
}

void CubeHandler::Clear() {
    cube_map.edited = false; // pending edits would be wiped with the volume
    Touch();
    if (vol && op_volume_clear(vol) != OP_OK) Report("Clear");
}
void CubeHandler::Collect(float min_weight, const int32_t* lo, const int32_t* hi, const char* where) {
    Pending();
    if (!vol) return; // no device volume yet: nothing is allocated
    Touch();
    if (op_volume_collect_garbage(vol, min_weight, lo, hi, nullptr) != OP_OK) Report(where);
    else ReleaseBorrowed(); // op_volume_collect_garbage synchronises
}
op_volume_collect_stats CubeHandler::CollectStats() const {
    op_volume_collect_stats st = {0, 0, 0, 0, 0};
    if (vol && op_volume_collect_last_stats(vol, &st) != OP_OK) Report("CollectStats");
    return st;
}
void CubeHandler::CollectGarbage() { Collect(0.0f, nullptr, nullptr, "CollectGarbage"); }
void CubeHandler::CollectGarbage(float min_weight) { Collect(min_weight, nullptr, nullptr, "CollectGarbage"); }
void CubeHandler::CropToCubes(const CubeID& lo, const CubeID& hi) {
    const int32_t l[3] = {lo(0), lo(1), lo(2)}, h[3] = {hi(0), hi(1), hi(2)};
    Collect(0.0f, l, h, "CropToCubes");
}
bool CubeHandler::HasCube(const CubeID& cube_id) const {
    Pending();
    if (!vol) return false;
    int present = 0;
    if (op_volume_has_cube(vol, cube_id(0), cube_id(1), cube_id(2), &present) != OP_OK) Report("HasCube");
    return present != 0;
}
size_t CubeHandler::GetCubeCount() const {
    Pending();
    size_t n = 0;
    if (vol && op_volume_block_count(vol, &n) != OP_OK) Report("GetCubeCount");
    else ReleaseBorrowed(); // op_volume_block_count synchronises
    return n;
}
void CubeHandler::Synchronize() const {
    Pending();
    if (vol && op_volume_sync(vol) != OP_OK) Report("Synchronize");
    else ReleaseBorrowed();
}

void CubeHandler::AddCube(const CubeID& cube_id) {
    Pending();
    if (!Ensure() || HasCube(cube_id)) return;
    Touch();
    const int32_t key[3] = {cube_id(0), cube_id(1), cube_id(2)};
    std::vector<float> fresh(512 * 5);
    for (int v = 0; v < 512; ++v) { fresh[5 * v] = 999; fresh[5 * v + 1] = 0; fresh[5 * v + 2] = fresh[5 * v + 3] = fresh[5 * v + 4] = -1; }
    if (op_volume_upload(vol, key, fresh.data(), 1) != OP_OK) Report("AddCube");
}

// CubeHandler.h:199-241 of the reference: ALLOCATE (AddCube) the blocks that the voxel centres of `v_cube` land in after
// `trans` -- the eight trilinear neighbours of the moved centre, or the one voxel that contains it.  The arithmetic is the
// reference's (4x4 * (p,1) accumulated column by column, division by w, float division by the resolution, floor).
void CubeHandler::AddTransformedCubes(const VoxelCube& v_cube, const geometry::TransformationMatrix& trans, bool nearest) {
    if (!Ensure()) return;
    const float res = c_para.VoxelResolution, half = res / 2;
    std::unordered_set<CubeID, CubeHasher> wanted;
    for (size_t voxel_id = 0; voxel_id != v_cube.voxels.size(); ++voxel_id) {
        geometry::Point3 p = geometry::TransformPoint(trans, c_para.GetGlobalPoint(v_cube.cube_id, static_cast<int>(voxel_id)));
        if (!nearest) p = p - geometry::Point3(half, half, half);
        const geometry::Point3i base(static_cast<int>(std::floor(p(0) / res)), static_cast<int>(std::floor(p(1) / res)), static_cast<int>(std::floor(p(2) / res)));
        for (int n = 0; n < (nearest ? 1 : 8); ++n)
            wanted.insert(c_para.GetCubeID(geometry::Point3i(base(0) + (n & 1), base(1) + ((n >> 1) & 1), base(2) + (n >> 2))));
    }
    for (std::unordered_set<CubeID, CubeHasher>::const_iterator it = wanted.begin(); it != wanted.end(); ++it) AddCube(*it);
}
void CubeHandler::AddTransformedCube(const VoxelCube& v_cube, const geometry::TransformationMatrix& trans) { AddTransformedCubes(v_cube, trans, false); }
void CubeHandler::AddTransformedCubeNearest(const VoxelCube& v_cube, const geometry::TransformationMatrix& trans) { AddTransformedCubes(v_cube, trans, true); }

void CubeHandler::ComputeBounding(const cv::Mat& depth, const geometry::TransformationMatrix& pose, geometry::Point3& max_pos, geometry::Point3& min_pos) {
    Pending();
    if (!Ensure()) return;
    float p[16], mx[3], mn[3];
    bridge::RowMajor(pose, p);
    size_t inside = 0;
    if (op_volume_compute_bounding(vol, depth.data, bridge::DepthFormat(depth), OP_MEM_HOST, p, mx, mn, &inside) != OP_OK) { Report("ComputeBounding"); return; }
    max_pos = geometry::Point3(mx[0], mx[1], mx[2]);
    min_pos = geometry::Point3(mn[0], mn[1], mn[2]);
}

void CubeHandler::PrepareCubes(const cv::Mat& depth, const geometry::TransformationMatrix& pose, std::vector<CubeID>& cube_id_list) {
    cube_id_list.clear();
    Pending();
    if (!Ensure()) return;
    Touch(); // PrepareCubes allocates the blocks it selects (CubeHandler.cpp:181-190)
    float p[16], pi[16];
    bridge::RowMajor(pose, p);
    bridge::RowMajor(pose.inverse(), pi); // the caller's own Eigen inverse when built with Eigen (Integrator.cpp:18)
    std::vector<int32_t> ids(3 * 65536);
    size_t n = 0;
    int rc = op_volume_prepare_cubes(vol, depth.data, bridge::DepthFormat(depth), OP_MEM_HOST, p, pi, ids.data(), ids.size() / 3, &n, nullptr);
    if (rc == OP_OK && n > ids.size() / 3) { // the blocks are allocated already: the second call only lists them
        ids.resize(3 * n);
        rc = op_volume_prepare_cubes(vol, depth.data, bridge::DepthFormat(depth), OP_MEM_HOST, p, pi, ids.data(), n, &n, nullptr);
    }
    if (rc != OP_OK) { Report("PrepareCubes"); return; }
    cube_id_list.reserve(n);
    for (size_t i = 0; i < n; ++i) cube_id_list.push_back(CubeID(ids[3 * i], ids[3 * i + 1], ids[3 * i + 2]));
}

void CubeHandler::IntegrateImage(const cv::Mat& depth, const cv::Mat& rgb, const geometry::TransformationMatrix& pose) {
    Pending();
    if (!Ensure()) return;
    Touch();
    float p[16], pi[16];
    bridge::RowMajor(pose, p);
    bridge::RowMajor(pose.inverse(), pi);
    // the images are only borrowed for the call: the library copies them into its pinned staging ring before returning
    if (op_volume_integrate(vol, depth.data, bridge::DepthFormat(depth), rgb.data, OP_MEM_HOST, p, pi) != OP_OK) { Report("IntegrateImage"); return; }
    // the reference prints two lines per frame here (CubeHandler.cpp:202-209); at > 10 k frames/s that would be the
    // bottleneck, so the line is opt-in (ONEPIECE_HIP_VERBOSE=1) and says what is true: the frame is queued
    static const bool verbose = std::getenv("ONEPIECE_HIP_VERBOSE") != nullptr;
    if (verbose) std::cout << GREEN << "[IntegrateImage]::[Info]::Image queued for integration." << RESET << std::endl;
}
void CubeHandler::DeintegrateImage(const cv::Mat& depth, const cv::Mat& rgb, const geometry::TransformationMatrix& pose) {
    Pending();
    if (!Ensure()) return;
    Touch();
    float p[16], pi[16];
    bridge::RowMajor(pose, p);
    bridge::RowMajor(pose.inverse(), pi); // as IntegrateImage forms it: the voxels project to the pixels the fused frame used
    if (op_volume_deintegrate(vol, depth.data, bridge::DepthFormat(depth), rgb.data, OP_MEM_HOST, p, pi) != OP_OK) Report("DeintegrateImage");
}
void CubeHandler::ReintegrateImage(const cv::Mat& depth, const cv::Mat& rgb, const geometry::TransformationMatrix& old_pose, const geometry::TransformationMatrix& new_pose) {
    Pending();
    if (!Ensure()) return;
    Touch();
    float po[16], pn[16];
    bridge::RowMajor(old_pose, po);
    bridge::RowMajor(new_pose, pn);
    if (op_volume_reintegrate(vol, depth.data, bridge::DepthFormat(depth), rgb.data, OP_MEM_HOST, po, pn) != OP_OK) Report("ReintegrateImage");
}
void CubeHandler::IntegrateImage(const cv::Mat& depth, const cv::Mat& rgb, const geometry::TransformationMatrix& pose, const camera::PinholeCamera& rgb_camera,
                                 const geometry::TransformationMatrix& color_to_depth) {
    Pending();
    if (!Ensure()) return;
    Touch();
    if (depth.rows != camera.Pod().height || depth.cols != camera.Pod().width || rgb.type() != CV_8UC3) {
        std::cout << RED << "[ERROR]::[IntegrateImage]::the depth image must have the volume camera's size, the colour image three byte channels." << RESET << std::endl;
        return;
    }
    float p[16], pi[16], m[16];
    bridge::RowMajor(pose, p);
    bridge::RowMajor(pose.inverse(), pi);
    bridge::RowMajor(color_to_depth, m);
    // both images are only borrowed for the call
    if (op_volume_integrate_unaligned(vol, depth.data, bridge::DepthFormat(depth), rgb.data, rgb.rows, rgb.cols, &rgb_camera.Pod(), m, OP_MEM_HOST, p, pi) != OP_OK)
        Report("IntegrateImage");
}
void CubeHandler::IntegrateImage(const geometry::RGBDFrame& rgbd, const geometry::TransformationMatrix& pose) {
    if (!rgbd.on_device) { IntegrateImage(rgbd.depth, rgbd.rgb, pose); return; }
    // the frame's images are on the device already (the tracker put them there): fused in place, nothing crosses PCIe again
    Pending();
    if (!Ensure()) return;
    Touch();
    std::shared_ptr<bridge::DeviceImages> d = std::static_pointer_cast<bridge::DeviceImages>(rgbd.on_device);
    // the device copy was made for the tracker's camera: it is fused in place only if it is what THIS volume reads -- its camera's size, its device
    if (d->width != camera.GetWidth() || d->height != camera.GetHeight() || d->device != bridge::Device()) {
        if (rgbd.depth.empty() || rgbd.rgb.empty()) {
            std::cout << RED << "[ERROR]::[IntegrateImage]::the frame's device copy (" << d->width << " x " << d->height << ", device " << d->device
                      << ") does not match the volume's camera (" << camera.GetWidth() << " x " << camera.GetHeight() << ") and the frame has no host images" << RESET << std::endl;
            return;
        }
        IntegrateImage(rgbd.depth, rgbd.rgb, pose);
        return;
    }
    float p[16], pi[16];
    bridge::RowMajor(pose, p);
    bridge::RowMajor(pose.inverse(), pi);
    // the volume reads the device images when their batch is launched (and again if it is replayed after a pool growth): they are held here
    // until the volume reports their batch complete (op_volume_progress: no waiting) -- about three batches' worth of frames in steady state
    uint64_t accepted = 0, done = 0;
    if (op_volume_progress(vol, &accepted, &done) != OP_OK) { Report("IntegrateImage"); return; }
    while (!borrowed_.empty() && borrowed_.front().first < done) borrowed_.pop_front();
    if (op_volume_integrate(vol, d->depth, d->depth_fmt, static_cast<const uint8_t*>(d->rgb), OP_MEM_DEVICE, p, pi) != OP_OK) { Report("IntegrateImage"); return; }
    borrowed_.push_back(std::make_pair(static_cast<unsigned long long>(accepted), rgbd.on_device)); // this frame is number `accepted` (0-based)
}

void CubeHandler::Merge(const CubeHandler& another) {
    if (c_para.VoxelResolution != another.c_para.VoxelResolution) {
        std::cout << YELLOW << "[Warning]::[MergeVoxelHash]::Voxel resolution is not identical." << RESET << std::endl;
        return;
    }
    Pending();
    another.Pending();
    if (!another.vol || !Ensure()) return;
    Touch();
    if (op_volume_merge(vol, another.vol) != OP_OK) Report("Merge");
}
void CubeHandler::Merge(const CubeHandler& another, const geometry::TransformationMatrix& trans) {
    if (c_para.VoxelResolution != another.c_para.VoxelResolution) {
        std::cout << YELLOW << "[Warning]::[MergeVoxelHash]::Voxel resolution is not identical." << RESET << std::endl;
        return;
    }
    std::shared_ptr<CubeHandler> moved = another.Transform(trans);
    if (moved) Merge(*moved);
}

void CubeHandler::MergeTransformed(const CubeHandler& another, const geometry::TransformationMatrix& trans, op_volume_merge_transformed_stats* stats) {
    MergeTransformed(std::vector<const CubeHandler*>(1, &another), std::vector<geometry::TransformationMatrix>(1, trans), stats);
}
void CubeHandler::MergeTransformed(const std::vector<const CubeHandler*>& others, const std::vector<geometry::TransformationMatrix>& trans,
                                   op_volume_merge_transformed_stats* stats) {
    if (stats) *stats = op_volume_merge_transformed_stats();
    if (others.size() != trans.size()) {
        std::cout << YELLOW << "[Warning]::[MergeTransformed]::" << others.size() << " volumes, " << trans.size() << " transformations." << RESET << std::endl;
        return;
    }
    for (size_t k = 0; k < others.size(); ++k)
        if (!others[k] || c_para.VoxelResolution != others[k]->c_para.VoxelResolution) {
            std::cout << YELLOW << "[Warning]::[MergeVoxelHash]::Voxel resolution is not identical." << RESET << std::endl;
            return;
        }
    Pending();
    std::vector<op_volume*> vols;
    std::vector<float> T, Ti;
    for (size_t k = 0; k < others.size(); ++k) {
        others[k]->Pending();
        if (!others[k]->vol) continue; // never used: no blocks (Transform of it is empty, Merge of that changes nothing)
        float m[16], mi[16];
        bridge::RowMajor(trans[k], m);
        bridge::RowMajor(trans[k].inverse(), mi);
        vols.push_back(others[k]->vol);
        T.insert(T.end(), m, m + 16);
        Ti.insert(Ti.end(), mi, mi + 16);
    }
    if (vols.empty() || !Ensure()) return;
    Touch();
    if (op_volume_merge_transformed_many(vol, vols.data(), T.data(), Ti.data(), vols.size(), stats) != OP_OK) Report("MergeTransformed");
}

std::shared_ptr<CubeHandler> CubeHandler::Transform(const geometry::TransformationMatrix& trans) const {
    Pending();
    if (!Ensure()) return std::shared_ptr<CubeHandler>();
    float T[16], Ti[16];
    bridge::RowMajor(trans, T);
    bridge::RowMajor(trans.inverse(), Ti);
    op_volume* out = nullptr;
    if (op_volume_transform(vol, T, Ti, 0, 0, &out) != OP_OK) { Report("Transform"); return std::shared_ptr<CubeHandler>(); }
    return std::shared_ptr<CubeHandler>(new CubeHandler(out, *this, c_para.VoxelResolution));
}
std::shared_ptr<CubeHandler> CubeHandler::TransformNearest(const geometry::TransformationMatrix& trans) {
    Pending();
    if (!Ensure()) return std::shared_ptr<CubeHandler>();
    float T[16], Ti[16];
    bridge::RowMajor(trans, T);
    bridge::RowMajor(trans.inverse(), Ti);
    op_volume* out = nullptr;
    if (op_volume_transform(vol, T, Ti, 1, 0, &out) != OP_OK) { Report("TransformNearest"); return std::shared_ptr<CubeHandler>(); }
    // the reference does not hand its c_para to the result (CubeHandler.h:299-305): it keeps the default resolution
    return std::shared_ptr<CubeHandler>(new CubeHandler(out, *this, CubePara().VoxelResolution));
}

std::shared_ptr<CubeHandler> CubeHandler::Coarsen(int levels, float min_weight, op_volume_coarsen_stats* stats) const {
    Pending();
    if (!Ensure()) return std::shared_ptr<CubeHandler>();
    op_volume* out = nullptr;
    if (op_volume_coarsen(vol, levels, min_weight, 0, &out, stats) != OP_OK) { Report("Coarsen"); return std::shared_ptr<CubeHandler>(); }
    float res = c_para.VoxelResolution;
    if (op_volume_resolution(out, &res) != OP_OK) { Report("Coarsen"); op_volume_destroy(out); return std::shared_ptr<CubeHandler>(); }
    return std::shared_ptr<CubeHandler>(new CubeHandler(out, *this, res)); // 2^levels * VoxelResolution, as the device doubled it
}

std::shared_ptr<geometry::PointCloud> CubeHandler::GetPointCloud() const {
    std::shared_ptr<geometry::PointCloud> pcd = std::make_shared<geometry::PointCloud>();
    Pending();
    if (!vol) return pcd;
    size_t n = 0;
    if (op_volume_point_cloud(vol, nullptr, nullptr, 0, &n) != OP_OK) { Report("GetPointCloud"); return pcd; }
    pcd->points.resize(n);
    pcd->colors.resize(n);
    if (n && op_volume_point_cloud(vol, bridge::Floats(pcd->points), bridge::Floats(pcd->colors), n, &n) != OP_OK) { Report("GetPointCloud"); pcd->Reset(); }
    return pcd;
}

namespace {
void AppendMesh(op_volume* vol, const int32_t* only_block, geometry::TriangleMesh& mesh, const char* where) {
    const int *tri = nullptr, *edges = nullptr;
    GetMarchingCubeTables(&tri, &edges);
    size_t n = 0;
    if (Failed(op_volume_extract_mesh(vol, tri, edges, only_block, nullptr, nullptr, 0, &n), where) || n == 0) return;
    std::vector<float> p(3 * n), c(3 * n);
    if (Failed(op_volume_extract_mesh(vol, tri, edges, only_block, p.data(), c.data(), n, &n), where)) return;
    unsigned index = static_cast<unsigned>(mesh.points.size()); // triangles index the running vertex list (MarchingCube.cpp:39)
    for (size_t k = 0; k < n; ++k) {
        mesh.points.push_back(geometry::Point3(p[3 * k], p[3 * k + 1], p[3 * k + 2]));
        mesh.colors.push_back(geometry::Point3(c[3 * k], c[3 * k + 1], c[3 * k + 2]));
        if (k % 3 == 2) { mesh.triangles.push_back(geometry::Point3ui(index, index + 1, index + 2)); index += 3; }
    }
}
} // namespace

void CubeHandler::ExtractTriangleMesh(geometry::TriangleMesh& mesh) {
    mesh.Reset(); // CubeHandler.cpp:11
    Pending();
    if (!vol) return;
    AppendMesh(vol, nullptr, mesh, "ExtractTriangleMesh");
    std::cout << BLUE << "[ExtractTriangleMesh]::[INFO]::Finish Extracting Mesh, " << mesh.triangles.size() << " triangles." << RESET << std::endl;
}
void CubeHandler::ExtractSimplifiedTriangleMesh(geometry::TriangleMesh& mesh, float grid_len) {
    mesh.Reset();
    Pending();
    if (!vol) return;
    const int *tri = nullptr, *edges = nullptr;
    GetMarchingCubeTables(&tri, &edges);
    size_t nv = 0, nt = 0; // the sizing call returns upper bounds (the soup's sizes), the filling call the true sizes
    int rc = op_volume_extract_mesh_clustered(vol, tri, edges, nullptr, grid_len, nullptr, nullptr, 0, nullptr, 0, &nv, &nt);
    if (rc == OP_OK && nt > 0) {
        mesh.points.resize(nv);
        mesh.colors.resize(nv);
        mesh.triangles.resize(nt);
        rc = op_volume_extract_mesh_clustered(vol, tri, edges, nullptr, grid_len, bridge::Floats(mesh.points), bridge::Floats(mesh.colors), nv, bridge::Indices(mesh.triangles), nt,
                                              &nv, &nt);
        if (rc != OP_OK) nv = nt = 0;
        mesh.points.resize(nv);
        mesh.colors.resize(nv);
        mesh.triangles.resize(nt);
    }
    if (rc == OP_ERR_INVALID || rc == OP_ERR_CAPACITY) {
        // Refused: the two calls this one stands for (ExtractTriangleMesh prints its own line).  A grid_len that is not positive is refused before any
        // kernel runs; a mesh too wide to key has by then cost the count pass of the sizing call and the count + emit passes and the clustering's
        // bounds kernel of the filling call, and the volume is extracted once more here -- the price of a rare refusal, not of the usual call.
        ExtractTriangleMesh(mesh);
        mesh = *mesh.ClusteringSimplify(grid_len);
        return;
    }
    if (Failed(rc, "ExtractSimplifiedTriangleMesh")) return;
    std::cout << BLUE << "[ExtractTriangleMesh]::[INFO]::Finish Extracting Mesh, " << mesh.triangles.size() << " triangles after simplification." << RESET << std::endl;
}
void CubeHandler::ExtractProcessedTriangleMesh(geometry::TriangleMesh& mesh, float grid_len, size_t min_points, bool compute_normals) {
    mesh.Reset();
    Pending();
    if (!vol) return;
    const int *tri = nullptr, *edges = nullptr;
    GetMarchingCubeTables(&tri, &edges);
    size_t nv = 0, nt = 0; // the sizing call returns upper bounds (the soup's sizes), the filling call the true sizes
    int rc = op_volume_extract_mesh_processed(vol, tri, edges, nullptr, grid_len, min_points, nullptr, nullptr, nullptr, 0, nullptr, 0, &nv, &nt);
    if (rc == OP_OK && nt > 0) {
        mesh.points.resize(nv);
        mesh.colors.resize(nv);
        if (compute_normals) mesh.normals.resize(nv);
        mesh.triangles.resize(nt);
        rc = op_volume_extract_mesh_processed(vol, tri, edges, nullptr, grid_len, min_points, bridge::Floats(mesh.points), bridge::Floats(mesh.colors),
                                              compute_normals ? bridge::Floats(mesh.normals) : nullptr, nv, bridge::Indices(mesh.triangles), nt, &nv, &nt);
        if (rc != OP_OK) nv = nt = 0;
        mesh.points.resize(nv);
        mesh.colors.resize(nv);
        if (compute_normals) mesh.normals.resize(nv);
        mesh.triangles.resize(nt);
    }
    if (rc == OP_ERR_INVALID || rc == OP_ERR_CAPACITY) { // refused: the calls this one stands for (see ExtractSimplifiedTriangleMesh for what that costs)
        ExtractTriangleMesh(mesh);
        if (grid_len > 0 || grid_len < 0) mesh = *mesh.ClusteringSimplify(grid_len);
        if (min_points > 0) mesh = *mesh.Prune(min_points);
        if (compute_normals) mesh.ComputeNormals();
        return;
    }
    if (Failed(rc, "ExtractProcessedTriangleMesh")) return;
    std::cout << BLUE << "[ExtractTriangleMesh]::[INFO]::Finish Extracting Mesh, " << mesh.triangles.size() << " triangles after post-processing." << RESET << std::endl;
}
size_t CubeHandler::RenderFrame(const geometry::TransformationMatrix& pose, cv::Mat& rgb, cv::Mat& depth) {
    Pending();
    if (!Ensure()) return 0;
    const op_camera pod = camera.Pod();
    rgb.create(pod.height, pod.width, CV_8UC3);
    depth.create(pod.height, pod.width, CV_32FC1);
    float p[16];
    bridge::RowMajor(pose, p);
    uint64_t n = 0;
    if (op_volume_render_frame(vol, &pod, p, rgb.data, reinterpret_cast<float*>(depth.data), OP_MEM_HOST, &n) != OP_OK) { Report("RenderFrame"); return 0; }
    ReleaseBorrowed(); // (the call synchronised the volume)
    return static_cast<size_t>(n);
}
namespace {
// the row-major T op_volume_sample takes, or nullptr for an exact identity (which is not applied: the points are sampled as they are given)
const float* SampleTransform(const geometry::TransformationMatrix& T, float out[16]) {
    bridge::RowMajor(T, out);
    bool identity = true;
    for (int k = 0; k < 16; ++k) identity = identity && out[k] == ((k % 5 == 0) ? 1.0f : 0.0f);
    return identity ? nullptr : out;
}
} // namespace
void CubeHandler::SampleVoxels(const geometry::Point3List& points, std::vector<TSDFVoxel>& voxels, std::vector<uint8_t>& status, bool reference_interpolation,
                               const geometry::TransformationMatrix& T) {
    Pending();
    const size_t n = points.size();
    voxels.assign(n, TSDFVoxel());
    status.assign(n, static_cast<uint8_t>(OP_SAMPLE_INVALID));
    if (n == 0 || !Ensure()) return;
    float t[16];
    const float* tp = SampleTransform(T, t);
    std::vector<float> flat(5 * n);
    if (op_volume_sample(vol, bridge::Floats(points), n, OP_MEM_HOST, tp, reference_interpolation ? OP_SAMPLE_REFERENCE : OP_SAMPLE_TRILINEAR, flat.data(), nullptr,
                         status.data(), nullptr) != OP_OK) { Report("SampleVoxels"); return; }
    ReleaseBorrowed(); // (the call synchronised the volume)
    for (size_t i = 0; i < n; ++i) {
        voxels[i].sdf = flat[5 * i]; voxels[i].weight = flat[5 * i + 1];
        voxels[i].color = geometry::Point3(flat[5 * i + 2], flat[5 * i + 3], flat[5 * i + 4]);
    }
}
void CubeHandler::SampleGradients(const geometry::Point3List& points, geometry::Point3List& gradients, std::vector<uint8_t>& status, const geometry::TransformationMatrix& T) {
    Pending();
    const size_t n = points.size();
    gradients.assign(n, geometry::Point3(0, 0, 0));
    status.assign(n, static_cast<uint8_t>(OP_SAMPLE_INVALID | OP_SAMPLE_NO_GRADIENT));
    if (n == 0 || !Ensure()) return;
    float t[16];
    const float* tp = SampleTransform(T, t);
    if (op_volume_sample(vol, bridge::Floats(points), n, OP_MEM_HOST, tp, OP_SAMPLE_TRILINEAR, nullptr, bridge::Floats(gradients), status.data(), nullptr) != OP_OK) {
        Report("SampleGradients");
        return;
    }
    ReleaseBorrowed();
}
namespace {
std::shared_ptr<registration::RegistrationResult> RegistrationOutcome(const op_volume_register_result& r) {
    registration::RegistrationResult result;
    for (int i = 0; i < 4; ++i)
        for (int k = 0; k < 4; ++k) result.T(i, k) = r.T[4 * i + k];
    result.rmse = r.rmse;
    return std::make_shared<registration::RegistrationResult>(std::move(result));
}
op_volume_register_result RegistrationNotRun(const geometry::TransformationMatrix& init) {
    op_volume_register_result r = op_volume_register_result();
    bridge::RowMajor(init, r.T);
    r.status = OP_REGISTER_TOO_FEW_POINTS;
    return r;
}
} // namespace
std::shared_ptr<registration::RegistrationResult> CubeHandler::RegisterPointCloud(const geometry::PointCloud& pcd, const geometry::TransformationMatrix& init,
                                                                                  const op_volume_register_params* params, op_volume_register_result* details) {
    Pending();
    op_volume_register_result r = RegistrationNotRun(init);
    if (Ensure()) {
        float t[16];
        bridge::RowMajor(init, t);
        if (op_volume_register_points(vol, bridge::Floats(pcd.points), pcd.points.size(), OP_MEM_HOST, t, params, &r) != OP_OK) {
            Report("RegisterPointCloud");
            r = RegistrationNotRun(init);
        } else {
            ReleaseBorrowed(); // (the call synchronised the volume)
        }
    }
    if (details) *details = r;
    return RegistrationOutcome(r);
}
std::shared_ptr<registration::RegistrationResult> CubeHandler::RegisterDepth(const cv::Mat& depth, const geometry::TransformationMatrix& init_pose, int pixel_stride,
                                                                             const op_volume_register_params* params, op_volume_register_result* details) {
    Pending();
    op_volume_register_result r = RegistrationNotRun(init_pose);
    if (Ensure()) {
        float t[16];
        bridge::RowMajor(init_pose, t);
        const op_camera pod = camera.Pod();
        if (op_volume_register_depth(vol, &pod, depth.data, bridge::DepthFormat(depth), OP_MEM_HOST, pixel_stride, t, params, &r) != OP_OK) {
            Report("RegisterDepth");
            r = RegistrationNotRun(init_pose);
        } else {
            ReleaseBorrowed();
        }
    }
    if (details) *details = r;
    return RegistrationOutcome(r);
}
bool CubeHandler::RegistrationSystem(const geometry::Point3List& points, const geometry::TransformationMatrix& T, float max_distance, double sums[28], uint64_t counts[4]) {
    Pending();
    for (int k = 0; k < 28; ++k) sums[k] = 0.0;
    for (int k = 0; k < 4; ++k) counts[k] = 0;
    if (!Ensure()) return false;
    float t[16];
    bridge::RowMajor(T, t);
    if (op_volume_register_system(vol, bridge::Floats(points), points.size(), OP_MEM_HOST, t, max_distance, sums, counts, nullptr) != OP_OK) {
        Report("RegistrationSystem");
        return false;
    }
    ReleaseBorrowed();
    return true;
}
namespace {
op_volume_register_color_result ColorRegistrationNotRun(const geometry::TransformationMatrix& init) {
    op_volume_register_color_result r = op_volume_register_color_result();
    r.base = RegistrationNotRun(init);
    return r;
}
op_volume_register_robust_result RobustRegistrationNotRun(const geometry::TransformationMatrix& init) {
    op_volume_register_robust_result r = op_volume_register_robust_result();
    r.color = ColorRegistrationNotRun(init);
    return r;
}
// I(c) of a cloud's colours (stored channel order, byte / 255: LoadFromRGBD); false for a cloud without colours
bool CloudIntensity(const geometry::PointCloud& pcd, std::vector<float>& intensity) {
    const size_t n = pcd.points.size();
    if (pcd.colors.size() != n) return false;
    intensity.resize(n);
    for (size_t i = 0; i < n; ++i) {
        const float c0 = pcd.colors[i](0), c1 = pcd.colors[i](1), c2 = pcd.colors[i](2);
        const float a = 0.114f * c0, b = 0.587f * c1, c = 0.299f * c2; // every product and sum rounded separately
        const float ab = a + b;
        intensity[i] = ab + c;
    }
    return true;
}
} // namespace
std::shared_ptr<registration::RegistrationResult> CubeHandler::RegisterColoredPointCloud(const geometry::PointCloud& pcd, const geometry::TransformationMatrix& init,
                                                                                         const op_volume_register_color_params* params,
                                                                                         op_volume_register_color_result* details) {
    Pending();
    op_volume_register_color_result r = ColorRegistrationNotRun(init);
    if (Ensure()) {
        float t[16];
        bridge::RowMajor(init, t);
        const size_t n = pcd.points.size();
        op_volume_register_color_params p;
        bool ok = true;
        if (params) p = *params;
        else ok = op_volume_register_color_default_params(vol, &p) == OP_OK;
        std::vector<float> intensity;
        if (!CloudIntensity(pcd, intensity)) p.color_scale = 0.0f;
        if (!ok || op_volume_register_color_points(vol, bridge::Floats(pcd.points), intensity.empty() ? nullptr : intensity.data(), n, OP_MEM_HOST, t, &p, &r) != OP_OK) {
            Report("RegisterColoredPointCloud");
            r = ColorRegistrationNotRun(init);
        } else {
            ReleaseBorrowed(); // (the call synchronised the volume)
        }
    }
    if (details) *details = r;
    return RegistrationOutcome(r.base);
}
std::shared_ptr<registration::RegistrationResult> CubeHandler::RegisterRGBD(const cv::Mat& depth, const cv::Mat& rgb, const geometry::TransformationMatrix& init_pose,
                                                                            int pixel_stride, const op_volume_register_color_params* params,
                                                                            op_volume_register_color_result* details) {
    Pending();
    op_volume_register_color_result r = ColorRegistrationNotRun(init_pose);
    if (Ensure()) {
        float t[16];
        bridge::RowMajor(init_pose, t);
        const op_camera pod = camera.Pod();
        if (op_volume_register_rgbd(vol, &pod, depth.data, bridge::DepthFormat(depth), rgb.data, OP_MEM_HOST, pixel_stride, t, params, &r) != OP_OK) {
            Report("RegisterRGBD");
            r = ColorRegistrationNotRun(init_pose);
        } else {
            ReleaseBorrowed();
        }
    }
    if (details) *details = r;
    return RegistrationOutcome(r.base);
}
bool CubeHandler::ColorRegistrationSystem(const geometry::Point3List& points, const std::vector<float>& intensity, const geometry::TransformationMatrix& T,
                                          float max_distance, float color_scale, float max_color_residual, double sums[30], uint64_t counts[5]) {
    Pending();
    for (int k = 0; k < 30; ++k) sums[k] = 0.0;
    for (int k = 0; k < 5; ++k) counts[k] = 0;
    if (!Ensure()) return false;
    float t[16];
    bridge::RowMajor(T, t);
    const float* y = intensity.size() == points.size() && !intensity.empty() ? intensity.data() : nullptr; // (a missing intensity is the library's refusal)
    if (op_volume_register_color_system(vol, bridge::Floats(points), y, points.size(), OP_MEM_HOST, t, max_distance, color_scale, max_color_residual, sums, counts,
                                        nullptr) != OP_OK) {
        Report("ColorRegistrationSystem");
        return false;
    }
    ReleaseBorrowed();
    return true;
}
std::shared_ptr<registration::RegistrationResult> CubeHandler::RegisterPointCloudRobust(const geometry::PointCloud& pcd, const geometry::TransformationMatrix& init,
                                                                                        const op_volume_register_color_params* params,
                                                                                        const op_volume_register_options* options,
                                                                                        op_volume_register_robust_result* details) {
    Pending();
    op_volume_register_robust_result r = RobustRegistrationNotRun(init);
    if (Ensure()) {
        float t[16];
        bridge::RowMajor(init, t);
        op_volume_register_color_params p;
        op_volume_register_options o;
        bool ok = true;
        if (params) p = *params;
        else ok = op_volume_register_color_default_params(vol, &p) == OP_OK;
        if (options) o = *options;
        else ok = ok && op_volume_register_robust_default_options(vol, &o) == OP_OK;
        std::vector<float> intensity;
        if (!CloudIntensity(pcd, intensity)) p.color_scale = 0.0f;
        if (!ok || op_volume_register_robust_points(vol, bridge::Floats(pcd.points), intensity.empty() ? nullptr : intensity.data(), pcd.points.size(), OP_MEM_HOST, t, &p,
                                                    &o, &r) != OP_OK) {
            Report("RegisterPointCloudRobust");
            r = RobustRegistrationNotRun(init);
        } else {
            ReleaseBorrowed(); // (the call synchronised the volume)
        }
    }
    if (details) *details = r;
    return RegistrationOutcome(r.color.base);
}
std::shared_ptr<registration::RegistrationResult> CubeHandler::RegisterRGBDRobust(const cv::Mat& depth, const cv::Mat& rgb, const geometry::TransformationMatrix& init_pose,
                                                                                  int pixel_stride, const op_volume_register_color_params* params,
                                                                                  const op_volume_register_options* options, op_volume_register_robust_result* details) {
    Pending();
    op_volume_register_robust_result r = RobustRegistrationNotRun(init_pose);
    if (Ensure()) {
        float t[16];
        bridge::RowMajor(init_pose, t);
        const op_camera pod = camera.Pod();
        op_volume_register_options o;
        bool ok = true;
        if (options) o = *options;
        else ok = op_volume_register_robust_default_options(vol, &o) == OP_OK;
        if (!ok || op_volume_register_robust_frame(vol, &pod, depth.data, bridge::DepthFormat(depth), rgb.data, OP_MEM_HOST, pixel_stride, t, params, &o, &r) != OP_OK) {
            Report("RegisterRGBDRobust");
            r = RobustRegistrationNotRun(init_pose);
        } else {
            ReleaseBorrowed();
        }
    }
    if (details) *details = r;
    return RegistrationOutcome(r.color.base);
}
bool CubeHandler::RobustRegistrationSystem(const geometry::Point3List& points, const std::vector<float>& intensity, const geometry::TransformationMatrix& T,
                                           float max_distance, float color_scale, float max_color_residual, const op_volume_register_options* options, double sums[31],
                                           uint64_t counts[7]) {
    Pending();
    for (int k = 0; k < 31; ++k) sums[k] = 0.0;
    for (int k = 0; k < 7; ++k) counts[k] = 0;
    if (!Ensure()) return false;
    float t[16];
    bridge::RowMajor(T, t);
    op_volume_register_options o;
    if (options) o = *options;
    else if (op_volume_register_robust_default_options(vol, &o) != OP_OK) { Report("RobustRegistrationSystem"); return false; }
    const float* y = intensity.size() == points.size() && !intensity.empty() ? intensity.data() : nullptr; // (a missing intensity is the library's refusal)
    if (op_volume_register_robust_system(vol, bridge::Floats(points), y, points.size(), OP_MEM_HOST, t, max_distance, color_scale, max_color_residual, &o, sums, counts,
                                         nullptr) != OP_OK) {
        Report("RobustRegistrationSystem");
        return false;
    }
    ReleaseBorrowed();
    return true;
}
std::vector<std::shared_ptr<registration::RegistrationResult>> CubeHandler::RegisterFramesRobust(const std::vector<cv::Mat>& depths, const std::vector<cv::Mat>& rgbs,
                                                                                                 const geometry::Mat4List& init_poses, int pixel_stride,
                                                                                                 const op_volume_register_color_params* params,
                                                                                                 const op_volume_register_options* options,
                                                                                                 std::vector<op_volume_register_robust_result>* details,
                                                                                                 op_volume_register_batch_stats* stats) {
    Pending();
    std::vector<std::shared_ptr<registration::RegistrationResult>> out;
    if (details) details->clear();
    if (stats) *stats = op_volume_register_batch_stats();
    const size_t n = depths.size();
    if (init_poses.size() != n || (!rgbs.empty() && rgbs.size() != n)) { std::fprintf(stderr, "RegisterFramesRobust: one pose (and one colour image) per depth image\n"); return out; }
    if (!n || !Ensure()) return out;
    // the frames side by side in one buffer per plane: frame f at f * (bytes of an image)
    const size_t dbytes = depths[0].total() * depths[0].elemSize(), cbytes = rgbs.empty() ? 0 : rgbs[0].total() * rgbs[0].elemSize();
    std::vector<unsigned char> d(n * dbytes), c(n * cbytes);
    std::vector<float> poses(16 * n);
    for (size_t f = 0; f < n; ++f) {
        const bool same = depths[f].rows == depths[0].rows && depths[f].cols == depths[0].cols && depths[f].type() == depths[0].type() && depths[f].data &&
                          (rgbs.empty() || (rgbs[f].rows == depths[0].rows && rgbs[f].cols == depths[0].cols && rgbs[f].type() == CV_8UC3 && rgbs[f].data));
        if (!same) { std::fprintf(stderr, "RegisterFramesRobust: frame %zu differs from frame 0 in size or type\n", f); return out; }
        std::memcpy(d.data() + f * dbytes, depths[f].data, dbytes);
        if (cbytes) std::memcpy(c.data() + f * cbytes, rgbs[f].data, cbytes);
        bridge::RowMajor(init_poses[f], poses.data() + 16 * f);
    }
    const op_camera pod = camera.Pod();
    op_volume_register_options o;
    bool ok = true;
    if (options) o = *options;
    else ok = op_volume_register_robust_default_options(vol, &o) == OP_OK;
    std::vector<op_volume_register_robust_result> r(n);
    op_volume_register_batch_stats st = op_volume_register_batch_stats();
    if (!ok || op_volume_register_batch_frames(vol, &pod, d.data(), dbytes, bridge::DepthFormat(depths[0]), cbytes ? c.data() : nullptr, cbytes, OP_MEM_HOST, pixel_stride,
                                               poses.data(), n, params, &o, r.data(), &st) != OP_OK) {
        Report("RegisterFramesRobust");
        return out;
    }
    ReleaseBorrowed(); // (the call synchronised the volume)
    for (size_t f = 0; f < n; ++f) out.push_back(RegistrationOutcome(r[f].color.base));
    if (details) *details = r;
    if (stats) *stats = st;
    return out;
}
std::vector<std::shared_ptr<registration::RegistrationResult>> CubeHandler::RegisterPointCloudsRobust(const std::vector<geometry::PointCloud>& pcds,
                                                                                                      const geometry::Mat4List& inits,
                                                                                                      const op_volume_register_color_params* params,
                                                                                                      const op_volume_register_options* options,
                                                                                                      std::vector<op_volume_register_robust_result>* details,
                                                                                                      op_volume_register_batch_stats* stats) {
    Pending();
    std::vector<std::shared_ptr<registration::RegistrationResult>> out;
    if (details) details->clear();
    if (stats) *stats = op_volume_register_batch_stats();
    const size_t n = pcds.size();
    if (inits.size() != n) { std::fprintf(stderr, "RegisterPointCloudsRobust: one initial transformation per cloud\n"); return out; }
    if (!n || !Ensure()) return out;
    op_volume_register_color_params p;
    op_volume_register_options o;
    bool ok = true;
    if (params) p = *params;
    else ok = op_volume_register_color_default_params(vol, &p) == OP_OK;
    if (options) o = *options;
    else ok = ok && op_volume_register_robust_default_options(vol, &o) == OP_OK;
    std::vector<uint64_t> starts(n + 1, 0);
    for (size_t c = 0; c < n; ++c) starts[c + 1] = starts[c] + pcds[c].points.size();
    std::vector<float> xyz(3 * starts[n]), intensity, one, Ts(16 * n);
    bool colored = true;
    for (size_t c = 0; c < n; ++c) {
        if (!pcds[c].points.empty()) std::memcpy(xyz.data() + 3 * starts[c], bridge::Floats(pcds[c].points), sizeof(float) * 3 * pcds[c].points.size());
        colored = colored && CloudIntensity(pcds[c], one);
        if (colored) intensity.insert(intensity.end(), one.begin(), one.end());
        bridge::RowMajor(inits[c], Ts.data() + 16 * c);
    }
    if (!colored) p.color_scale = 0.0f;
    std::vector<op_volume_register_robust_result> r(n);
    op_volume_register_batch_stats st = op_volume_register_batch_stats();
    if (!ok || op_volume_register_batch_points(vol, xyz.data(), nullptr, colored && !intensity.empty() ? intensity.data() : nullptr, starts.data(), n, OP_MEM_HOST, Ts.data(),
                                               &p, &o, r.data(), &st) != OP_OK) {
        Report("RegisterPointCloudsRobust");
        return out;
    }
    ReleaseBorrowed();
    for (size_t c = 0; c < n; ++c) out.push_back(RegistrationOutcome(r[c].color.base));
    if (details) *details = r;
    if (stats) *stats = st;
    return out;
}
std::shared_ptr<registration::RegistrationResult> CubeHandler::RegisterVolume(const CubeHandler& source, const geometry::TransformationMatrix& init,
                                                                              const op_volume_band_params* sel, const op_volume_register_color_params* params,
                                                                              const op_volume_register_options* options, op_volume_register_volume_result* details) {
    Pending();
    source.Pending();
    op_volume_register_volume_result r = op_volume_register_volume_result();
    r.robust = RobustRegistrationNotRun(init);
    if (Ensure() && source.Ensure()) {
        float t[16];
        bridge::RowMajor(init, t);
        if (op_volume_register_volume(vol, source.vol, t, sel, params, options, &r) != OP_OK) {
            Report("RegisterVolume");
            r = op_volume_register_volume_result();
            r.robust = RobustRegistrationNotRun(init);
        } else {
            ReleaseBorrowed(); // (the call synchronised both volumes)
            source.ReleaseBorrowed();
        }
    }
    if (details) *details = r;
    return RegistrationOutcome(r.robust.color.base);
}
bool CubeHandler::GetBandVoxels(geometry::Point3List& points, std::vector<float>& sdf, std::vector<float>& intensity, const op_volume_band_params* sel) const {
    Pending();
    points.clear(); sdf.clear(); intensity.clear();
    if (!Ensure()) return false;
    size_t n = 0;
    if (op_volume_band_voxels(vol, sel, nullptr, nullptr, nullptr, OP_MEM_HOST, 0, &n) != OP_OK) { Report("GetBandVoxels"); return false; }
    ReleaseBorrowed(); // (the call synchronised the volume)
    points.resize(n); sdf.resize(n); intensity.resize(n);
    if (n == 0) return true;
    if (op_volume_band_voxels(vol, sel, bridge::Floats(points), sdf.data(), intensity.data(), OP_MEM_HOST, n, &n) != OP_OK) { Report("GetBandVoxels"); return false; }
    return true;
}
op_volume_sample_stats CubeHandler::DistanceToModel(const geometry::PointCloud& pcd, const geometry::TransformationMatrix& pose) {
    Pending();
    op_volume_sample_stats st = {0, 0, 0, 0, 0.0, 0.0, 0.0f};
    const size_t n = pcd.points.size();
    st.queries = n;
    if (n == 0 || !Ensure()) return st;
    float t[16];
    const float* tp = SampleTransform(pose, t);
    if (op_volume_sample(vol, bridge::Floats(pcd.points), n, OP_MEM_HOST, tp, OP_SAMPLE_TRILINEAR, nullptr, nullptr, nullptr, &st) != OP_OK) { Report("DistanceToModel"); return st; }
    ReleaseBorrowed();
    return st;
}
void CubeHandler::GenerateMeshByCube(const CubeID& cube_id, geometry::TriangleMesh& mesh) {
    Pending();
    if (!vol) return;
    const int32_t only[3] = {cube_id(0), cube_id(1), cube_id(2)};
    AppendMesh(vol, only, mesh, "GenerateMeshByCube");
}

CubeMap CubeHandler::GetCubeMap() {
    Pending();
    CubeMap cube_map; // (a fresh copy BY VALUE, as the reference returns one; not the mirror member)
    if (!vol) return cube_map;
    size_t n = 0;
    if (op_volume_block_count(vol, &n) != OP_OK) { Report("GetCubeMap"); return cube_map; }
    std::vector<int32_t> keys(3 * n);
    std::vector<float> vox(n * 512 * 5);
    if (n && op_volume_download(vol, keys.data(), vox.data(), n, &n) != OP_OK) { Report("GetCubeMap"); return cube_map; }
    cube_map.reserve(n);
    for (size_t b = 0; b < n; ++b) {
        const CubeID id(keys[3 * b], keys[3 * b + 1], keys[3 * b + 2]);
        VoxelCube& cube = (cube_map[id] = VoxelCube(id));
        const float* src = &vox[b * 512 * 5];
        for (int v = 0; v < 512; ++v, src += 5) cube.voxels[v] = TSDFVoxel(src[0], src[1], geometry::Point3(src[2], src[3], src[4]));
    }
    return cube_map;
}

void CubeHandler::SetCubeMap(const CubeMap& _cube_map) {
    std::cout << YELLOW << "[WARNING]::[SetCubeMap]::Note that you are changing the hashing map directly." << RESET << std::endl;
    this->cube_map.edited = false; // replaced wholesale
    Touch();
    if (!Ensure()) return;
    if (op_volume_clear(vol) != OP_OK) { Report("SetCubeMap"); return; }
    std::vector<int32_t> keys;
    std::vector<float> vox;
    keys.reserve(3 * _cube_map.size());
    vox.reserve(_cube_map.size() * 512 * 5);
    for (CubeMap::const_iterator it = _cube_map.begin(); it != _cube_map.end(); ++it) {
        for (int k = 0; k < 3; ++k) keys.push_back(it->first(k));
        for (int v = 0; v < 512; ++v) {
            const TSDFVoxel& t = it->second.voxels[v];
            const float rec[5] = {t.sdf, t.weight, t.color(0), t.color(1), t.color(2)};
            vox.insert(vox.end(), rec, rec + 5);
        }
    }
    if (!keys.empty() && op_volume_upload(vol, keys.data(), vox.data(), keys.size() / 3) != OP_OK) Report("SetCubeMap");
}

bool CubeHandler::WriteToFile(const std::string& filename) const {
    Pending();
    if (Ensure() && op_volume_write_file(vol, filename.c_str()) != OP_OK) Report("WriteToFile");
    else std::cout << GREEN << "[CubeHandler]::[INFO]::Write TSDF field done!(To BinaryFile) " << RESET << std::endl;
    return true; // the reference's file calls always return true (SURVEY 8b "Errors")
}
bool CubeHandler::ReadFromFile(const std::string& filename) {
    cube_map.edited = false;
    Touch();
    if (Ensure() && op_volume_read_file(vol, filename.c_str(), 0) != OP_OK) Report("ReadFromFile");
    return true;
}
bool CubeHandler::ReadFromFileFloat(const std::string& filename) {
    cube_map.edited = false;
    Touch();
    if (Ensure() && op_volume_read_file(vol, filename.c_str(), 1) != OP_OK) Report("ReadFromFileFloat");
    return true;
}

bool CubeHandler::MergeAcrossRanks(void* nccl_comm, int root) {
    Pending();
    Touch();
    if (!Ensure()) return false;
    if (op_volume_merge_rccl(vol, nccl_comm, root, nullptr) != OP_OK) { Report("MergeAcrossRanks"); return false; }
    return true;
}

} // namespace integration
} // namespace one_piece
