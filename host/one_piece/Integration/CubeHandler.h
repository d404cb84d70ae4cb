// Integration/CubeHandler.h -- one_piece::integration::CubeHandler on an MI355X.
//
// Same class name, namespace, public signatures, default arguments and value semantics as the reference's
// src/Integration/CubeHandler.h:24-366, so that code written against it (example/ImageSequenceIntegration.cpp,
// example/DenseFusion) compiles and links against this library instead.  What differs is where the block hash lives:
// the reference holds a std::unordered_map<CubeID, VoxelCube> on the host; here the object owns a device-resident
// volume (op_volume, include/onepiece_hip.h) and every member forwards to the C-ABI:
//
//   IntegrateImage      -> op_volume_integrate   (enqueues; frames are fused in batches of up to 32 per launch)
//   every reader        -> flushes + synchronises first (GetCubeMap, HasCube, ExtractTriangleMesh, WriteToFile, ...),
//                          so the deferral cannot be observed (SURVEY 8b "Threading")
//   GetCubeMap()        -> downloads into a fresh CubeMap and returns it BY VALUE, as the reference does
//   copy construction / assignment -> deep copy on the device (a CubeHandler owns its volume; no sharing)
//   Transform* / GetPointCloud     -> std::shared_ptr to freshly made objects
//   errors              -> a coloured line on std::cout and an early return; nothing throws (reference behaviour)
//
// The reference's protected `CubeMap cube_map` member (CubeHandler.h:359) is a MIRROR here (CubeMapMirror below): a derived class
// that reads it gets a host copy refreshed from the device when the volume has changed since its last look, and what it writes
// through it is uploaded before the next member call touches the volume.  Device selection: environment variable
// ONEPIECE_HIP_DEVICE (default 0).
#pragma once
#include <deque>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "Camera/Camera.h"
#include "Geometry/Geometry.h"
#include "Geometry/RGBDFrame.h"
#include "Geometry/TriangleMesh.h"
#include "Integration/Frustum.h" // the reference's CubeHandler.h brings it in (CubeHandler.h:5; example/ImageIntegration.cpp:30)
#include "Integration/Integrator.h"
#include "Integration/MarchingCube.h"
#include "Integration/VoxelCube.h"
#include "Registration/RegistrationResult.h"

#define TRUNCATED_DISTANCES 1.0

struct op_volume;

namespace one_piece {
namespace integration {

typedef std::unordered_map<CubeID, VoxelCube, CubeHasher> CubeMap;

class CubeHandler;

// The protected `cube_map` of the reference's CubeHandler (CubeHandler.h:359), for classes derived from it.  The volume itself lives in HBM; this
// object hands out a host-side CubeMap that is downloaded lazily -- on the first access after the device volume changed -- and uploaded
// lazily: access through a non-const member marks it edited, and the handler pushes it to the device before its next member call looks at
// or changes the volume (or at CommitCubeMap()).  The container members derived classes use are forwarded; anything else is reachable
// through get() / edit().  A full download / upload per change of ownership: meant for inspection and small edits, not for per-frame use.
class CubeMapMirror {
  public:
    typedef CubeMap::iterator iterator;
    typedef CubeMap::const_iterator const_iterator;
    typedef CubeMap::key_type key_type;
    typedef CubeMap::mapped_type mapped_type;
    typedef CubeMap::value_type value_type;
    typedef CubeMap::size_type size_type;

    const CubeMap& get() const; // refreshed from the device if stale
    CubeMap& edit();            // refreshed, and marked edited
    operator const CubeMap&() const { return get(); }

    size_type size() const { return get().size(); }
    bool empty() const { return get().empty(); }
    size_type count(const key_type& k) const { return get().count(k); }
    const_iterator find(const key_type& k) const { return get().find(k); }
    const_iterator begin() const { return get().begin(); }
    const_iterator end() const { return get().end(); }
    const_iterator cbegin() const { return get().begin(); }
    const_iterator cend() const { return get().end(); }
    const mapped_type& at(const key_type& k) const { return get().at(k); }
    iterator find(const key_type& k) { return edit().find(k); }
    iterator begin() { return edit().begin(); }
    iterator end() { return edit().end(); }
    mapped_type& at(const key_type& k) { return edit().at(k); }
    mapped_type& operator[](const key_type& k) { return edit()[k]; }
    std::pair<iterator, bool> insert(const value_type& v) { return edit().insert(v); }
    size_type erase(const key_type& k) { return edit().erase(k); }
    void clear() { edit().clear(); }
    void reserve(size_type n) { edit().reserve(n); }
    CubeMapMirror& operator=(const CubeMap& m) { edit() = m; return *this; }

  private:
    friend class CubeHandler;
    explicit CubeMapMirror(CubeHandler* o) : owner(o) {}
    CubeMapMirror(const CubeMapMirror&);            // a mirror belongs to one handler: not copyable
    CubeMapMirror& operator=(const CubeMapMirror&);
    CubeHandler* owner;
    mutable CubeMap host;
    mutable unsigned long long seen = 0; // the handler's change counter at the last download / upload (0 = never)
    mutable bool edited = false;
};

class CubeHandler {
  public:
    CubeHandler();
    CubeHandler(const camera::PinholeCamera& _camera);
    CubeHandler(const CubeHandler& other);
    CubeHandler& operator=(const CubeHandler& other);
    ~CubeHandler();

    void SetVoxelResolution(float resolution);
    bool ReadFromFile(const std::string& filename);
    bool ReadFromFileFloat(const std::string& filename);
    bool WriteToFile(const std::string& filename) const;
    bool HasCube(const CubeID& cube_id) const;
    void Clear();
    void SetCamera(const camera::PinholeCamera& _camera);
    void SetTruncation(float trunc);
    void Merge(const CubeHandler& another);
    void Merge(const CubeHandler& another, const geometry::TransformationMatrix& trans);
    // EXTENSION (not in the reference): what Merge(another, trans) -- for the list form, one such call per entry, in order -- leaves in this
    // volume, bit for bit, in ONE device call and without the intermediate volume of Transform: every source is resampled straight into this
    // volume's blocks (op_volume_merge_transformed_many states the definition).  A resolution that is not identical (or lists of different
    // lengths): the reference's warning line (a message), nothing changes.  stats: the call's counts.
    void MergeTransformed(const CubeHandler& another, const geometry::TransformationMatrix& trans, op_volume_merge_transformed_stats* stats = nullptr);
    void MergeTransformed(const std::vector<const CubeHandler*>& others, const std::vector<geometry::TransformationMatrix>& trans,
                          op_volume_merge_transformed_stats* stats = nullptr);
    void ComputeBounding(const cv::Mat& depth, const geometry::TransformationMatrix& pose, geometry::Point3& max_pos, geometry::Point3& min_pos);
    void PrepareCubes(const cv::Mat& depth, const geometry::TransformationMatrix& pose, std::vector<CubeID>& cube_id_list);
    void IntegrateImage(const cv::Mat& depth, const cv::Mat& rgb, const geometry::TransformationMatrix& pose);
    void IntegrateImage(const geometry::RGBDFrame& rgbd, const geometry::TransformationMatrix& pose);
    // EXTENSION (not in the reference): IntegrateImage(depth, tool::AlignColorToDepth(rgb, depth, rgb_camera, this camera, color_to_depth), pose) for a
    // colour image from a second camera (the ScanNet flow, example/GenerateModelFromScannet.cpp) -> op_volume_integrate_unaligned: the alignment runs
    // on the volume's stream and the aligned image never leaves the device
    void IntegrateImage(const cv::Mat& depth, const cv::Mat& rgb, const geometry::TransformationMatrix& pose, const camera::PinholeCamera& rgb_camera,
                        const geometry::TransformationMatrix& color_to_depth = geometry::TransformationMatrix::Identity());
    // EXTENSION (not in the reference): takes a frame that was fused at `pose` out of the volume again -- the steps of IntegrateImage (same selection,
    // same pixel, same predicate) with TSDFVoxel::operator+ given an observation of weight -1; a voxel whose weight returns to 0 is the default voxel
    // again (op_volume_deintegrate states the definition).  Queued like IntegrateImage, in call order with the integrations around it.
    void DeintegrateImage(const cv::Mat& depth, const cv::Mat& rgb, const geometry::TransformationMatrix& pose);
    // EXTENSION: DeintegrateImage(depth, rgb, old_pose) then IntegrateImage(depth, rgb, new_pose) on one uploaded copy of the images and in one launch
    // (op_volume_reintegrate): what a corrected pose of an already fused frame is used for.
    void ReintegrateImage(const cv::Mat& depth, const cv::Mat& rgb, const geometry::TransformationMatrix& old_pose, const geometry::TransformationMatrix& new_pose);
    // CollectGarbage(): declared by the reference (CubeHandler.h:357) and defined nowhere in it.  Here it frees every block that holds no voxel of
    // weight > 0 -- what a de-integration leaves behind, what PrepareCubes selected and nothing updated -- on the device, compacting the pool in
    // place (op_volume_collect_garbage states the definition).  EXTENSIONS: CollectGarbage(min_weight) also drops the blocks whose largest weight is
    // below min_weight (depth-edge noise fewer than min_weight frames supported); CropToCubes(lo, hi) drops the blocks whose id lies outside
    // [lo, hi] (inclusive, per axis) or that hold no observed voxel.  CollectStats(): what the last of these calls did.
    void CollectGarbage();
    void CollectGarbage(float min_weight);
    void CropToCubes(const CubeID& lo, const CubeID& hi);
    op_volume_collect_stats CollectStats() const; // (kept by the device volume: the class gains no data member, its layout is the one earlier builds were compiled against)
    CubeID GetCubeID(const geometry::Point3& point) const { return c_para.GetCubeID(point); }
    void AddCube(const CubeID& cube_id);
    // allocate the blocks the voxel centres of v_cube land in after trans: their eight trilinear neighbours / the voxel
    // that contains them (the allocation passes of Transform / TransformNearest, CubeHandler.h:199-241)
    void AddTransformedCube(const VoxelCube& v_cube, const geometry::TransformationMatrix& trans);
    void AddTransformedCubeNearest(const VoxelCube& v_cube, const geometry::TransformationMatrix& trans);
    void ExtractTriangleMesh(geometry::TriangleMesh& mesh);
    // equals ExtractTriangleMesh(mesh) followed by mesh = *mesh.ClusteringSimplify(grid_len), bit for bit -- the tail of the reference's fusion
    // drivers (example/DenseFusion/DenseFusion.cpp:104-105) in one device call (op_volume_extract_mesh_clustered): the triangle soup never reaches
    // the host.  Not in the reference.  What the device entry refuses (a grid_len that is not positive, a mesh too wide to key) takes the two calls.
    void ExtractSimplifiedTriangleMesh(geometry::TriangleMesh& mesh, float grid_len);
    // equals ExtractTriangleMesh(mesh), then mesh = *mesh.ClusteringSimplify(grid_len) if grid_len > 0, then mesh = *mesh.Prune(min_points) if
    // min_points > 0, then mesh.ComputeNormals() if compute_normals, bit for bit -- the whole tail of the reference's fusion drivers
    // (example/MergeMultipleSubmaps.cpp:45-46, ImageIntegration.cpp:45) in one device call (op_volume_extract_mesh_processed): only the finished mesh
    // reaches the host.  Not in the reference.  What the device entry refuses takes the separate calls.
    void ExtractProcessedTriangleMesh(geometry::TriangleMesh& mesh, float grid_len, size_t min_points, bool compute_normals);
    // the model seen from `pose` as an RGB-D frame in the format IntegrateImage and odometry::Odometry::DenseTracking take: rgb CV_8UC3, depth CV_32FC1 in
    // metres (0 = no surface), both of the handler's camera's size (op_volume_render_frame: the raycast with colours, packed on the device).  Returns the
    // number of pixels that see the model.  Not in the reference, which has no raycaster; the frame-to-model tracker that uses the same view without
    // bringing it to the host is odometry::Odometry::DenseTrackingToModel.
    size_t RenderFrame(const geometry::TransformationMatrix& pose, cv::Mat& rgb, cv::Mat& depth);
    // EXTENSIONS (not in the reference, which can only be read whole): what the model holds at the caller's points, one batch per device call
    // (op_volume_sample states the definitions).  The points are taken through T first (an exact identity is not applied).  status[i] holds the
    // OP_SAMPLE_* bits of point i.
    //   SampleVoxels     the raycaster's strict trilinear sample (valid iff all eight voxels around the point are observed; otherwise the default
    //                    voxel), or with reference_interpolation VoxelCube::ReadVoxelInterpolate as Transform evaluates it
    //   SampleGradients  the central difference of the trilinear sdf at +-res/2 per axis, unnormalised (divided by the voxel resolution it
    //                    approximates the gradient of the field; normalised it is the raycaster's normal); zero where a sample is missing
    //   DistanceToModel  the statistics of |sdf| over the points of a cloud placed at `pose`: how far the cloud lies from the model
    void SampleVoxels(const geometry::Point3List& points, std::vector<TSDFVoxel>& voxels, std::vector<uint8_t>& status, bool reference_interpolation = false,
                      const geometry::TransformationMatrix& T = geometry::TransformationMatrix::Identity());
    void SampleGradients(const geometry::Point3List& points, geometry::Point3List& gradients, std::vector<uint8_t>& status,
                         const geometry::TransformationMatrix& T = geometry::TransformationMatrix::Identity());
    op_volume_sample_stats DistanceToModel(const geometry::PointCloud& pcd, const geometry::TransformationMatrix& pose = geometry::TransformationMatrix::Identity());
    // EXTENSIONS (not in the reference, which registers clouds against clouds by a kd-tree ICP): where a cloud or a depth frame belongs in the
    // model, by point-to-plane Gauss-Newton against the field itself -- the trilinear sdf is the residual, its normalised gradient the normal
    // (op_volume_register_points states the definition).  Returned like registration::PointToPlane's result: T (cloud to model / the refined
    // camera-to-world pose) and rmse at T; the correspondence sets stay empty (there are no pairs).  params == nullptr: the defaults (30 iterations,
    // max_distance = the truncation, min_step 1e-5, min_points 6); details (status, counts, iterations) go to *details when it is given.
    //   RegistrationSystem  one evaluation at T: sums[28] = the upper triangle of JtJ row by row, Jtr, the sum of s^2; counts[4] = used, invalid,
    //                       no_gradient, too_far.  false when the call failed.
    std::shared_ptr<registration::RegistrationResult> RegisterPointCloud(const geometry::PointCloud& pcd,
                                                                         const geometry::TransformationMatrix& init = geometry::TransformationMatrix::Identity(),
                                                                         const op_volume_register_params* params = nullptr, op_volume_register_result* details = nullptr);
    std::shared_ptr<registration::RegistrationResult> RegisterDepth(const cv::Mat& depth, const geometry::TransformationMatrix& init_pose, int pixel_stride = 1,
                                                                    const op_volume_register_params* params = nullptr, op_volume_register_result* details = nullptr);
    bool RegistrationSystem(const geometry::Point3List& points, const geometry::TransformationMatrix& T, float max_distance, double sums[28], uint64_t counts[4]);
    // The same with the colour term (op_volume_register_color_points states the definition): the model's intensity at the point against the
    // observed one is a second residual, which holds a view that the sdf alone lets slide along a wall.  The result's rmse stays the sdf rmse;
    // the colour rmse and the count of coloured points go to *details.  params == nullptr: the defaults above, color_scale 1, no colour gate.
    //   RegisterColoredPointCloud  the observed intensity of point i is I(pcd.colors[i]) = (0.114f c0 + 0.587f c1) + 0.299f c2.  LoadFromRGBD leaves
    //                       the pixel's three bytes / 255.0f there in STORED channel order (PointCloud.cpp:40-42), the order the volume's colour
    //                       planes have: a cloud loaded from a frame gets the intensities RegisterRGBD gives that frame.  A cloud without colours
    //                       (colors.size() != points.size()) is registered with color_scale 0: RegisterPointCloud's result.
    //   RegisterRGBD        depth as RegisterDepth, rgb CV_8UC3 of the same size.
    //   ColorRegistrationSystem  one evaluation at T: sums[30] = the 28 above with the colour terms added, the sum of rc^2, the geometric sum of
    //                       s^2; counts[5] = used, invalid, no_gradient, too_far, colored.  false when the call failed.
    std::shared_ptr<registration::RegistrationResult> RegisterColoredPointCloud(const geometry::PointCloud& pcd,
                                                                                const geometry::TransformationMatrix& init = geometry::TransformationMatrix::Identity(),
                                                                                const op_volume_register_color_params* params = nullptr,
                                                                                op_volume_register_color_result* details = nullptr);
    std::shared_ptr<registration::RegistrationResult> RegisterRGBD(const cv::Mat& depth, const cv::Mat& rgb, const geometry::TransformationMatrix& init_pose,
                                                                   int pixel_stride = 1, const op_volume_register_color_params* params = nullptr,
                                                                   op_volume_register_color_result* details = nullptr);
    bool ColorRegistrationSystem(const geometry::Point3List& points, const std::vector<float>& intensity, const geometry::TransformationMatrix& T,
                                 float max_distance, float color_scale, float max_color_residual, double sums[30], uint64_t counts[5]);
    // The same under a linearisation in which row and residual agree and with Huber weights (op_volume_register_robust_points states the
    // definition and why: the stored sdf is projective, its gradient is not of length 1, and the entries above overshoot by that length).
    // options == nullptr: OP_REGISTER_LIN_METRIC without weights (op_volume_register_robust_default_options); all-zero options give the entries
    // above bit for bit.  The residual rmse in metres and the down-weighted counts go to *details.
    //   RegisterPointCloudRobust  intensities as RegisterColoredPointCloud takes them; a cloud without colours is registered with color_scale 0.
    //   RegisterRGBDRobust  an empty rgb (rgb.data == nullptr): the geometric registration of the depth image.
    //   RobustRegistrationSystem  one evaluation at T: sums[31] = the 30 above from the scaled rows and the sum of the unweighted r^2;
    //                       counts[7] = the five above, downweighted, color_downweighted.  false when the call failed.
    std::shared_ptr<registration::RegistrationResult> RegisterPointCloudRobust(const geometry::PointCloud& pcd,
                                                                               const geometry::TransformationMatrix& init = geometry::TransformationMatrix::Identity(),
                                                                               const op_volume_register_color_params* params = nullptr,
                                                                               const op_volume_register_options* options = nullptr,
                                                                               op_volume_register_robust_result* details = nullptr);
    std::shared_ptr<registration::RegistrationResult> RegisterRGBDRobust(const cv::Mat& depth, const cv::Mat& rgb, const geometry::TransformationMatrix& init_pose,
                                                                         int pixel_stride = 1, const op_volume_register_color_params* params = nullptr,
                                                                         const op_volume_register_options* options = nullptr,
                                                                         op_volume_register_robust_result* details = nullptr);
    bool RobustRegistrationSystem(const geometry::Point3List& points, const std::vector<float>& intensity, const geometry::TransformationMatrix& T,
                                  float max_distance, float color_scale, float max_color_residual, const op_volume_register_options* options, double sums[31],
                                  uint64_t counts[7]);
    // Many frames, or many clouds, in one call (op_volume_register_batch_frames / _points state the definition): every frame follows
    // RegisterRGBDRobust's loop on its own -- its own pose, its own stop rule -- and the frames that still iterate share one launch per round, so
    // a stopped frame costs nothing more.  Element f of the returned list, and of *details, is what RegisterRGBDRobust /
    // RegisterPointCloudRobust return for frame f alone, bit for bit.  One params and one options serve the whole batch (nullptr as there).
    // Not in the reference.
    //   RegisterFramesRobust       depths of one size and type, init_poses one per depth; rgbs empty: the geometric registration, else one CV_8UC3
    //                              image per depth.  The images are packed into one upload.
    //   RegisterPointCloudsRobust  inits one per cloud; the colour term needs colours on EVERY cloud, otherwise color_scale 0.
    // A size mismatch or a failed call: an empty list.  *stats (when given): rounds, launches, evaluations, points.
    std::vector<std::shared_ptr<registration::RegistrationResult>> RegisterFramesRobust(const std::vector<cv::Mat>& depths, const std::vector<cv::Mat>& rgbs,
                                                                                        const geometry::Mat4List& init_poses, int pixel_stride = 1,
                                                                                        const op_volume_register_color_params* params = nullptr,
                                                                                        const op_volume_register_options* options = nullptr,
                                                                                        std::vector<op_volume_register_robust_result>* details = nullptr,
                                                                                        op_volume_register_batch_stats* stats = nullptr);
    std::vector<std::shared_ptr<registration::RegistrationResult>> RegisterPointCloudsRobust(const std::vector<geometry::PointCloud>& pcds,
                                                                                             const geometry::Mat4List& inits,
                                                                                             const op_volume_register_color_params* params = nullptr,
                                                                                             const op_volume_register_options* options = nullptr,
                                                                                             std::vector<op_volume_register_robust_result>* details = nullptr,
                                                                                             op_volume_register_batch_stats* stats = nullptr);
    // One fused volume against another (op_volume_register_volume states the definition): where the submap `source` belongs in this model, before
    // Transform + Merge (example/MergeMultipleSubmaps.cpp) fix its place for good.  A fused volume has no surface points, it has a band of voxels
    // that each carry their own sdf: the residual is this model's sdf at the transformed voxel centre MINUS the source voxel's own sdf, over the
    // source's band voxels, selected once on the device; its stored colour gives the colour term.  Not in the reference.
    //   RegisterVolume  init: source to this model.  sel == nullptr: the source's defaults (|sdf| <= 2 voxels, weight >= 1, every voxel);
    //                   params == nullptr: this model's colour defaults; options == nullptr: OP_REGISTER_LIN_GRADIENT without weights (NOT the
    //                   point entries' default).  The result's rmse stays this model's sdf rmse at the voxels; everything else goes to *details.
    //   GetBandVoxels   the list itself (op_volume_band_voxels): centres, stored sdf and I(stored colour) of the selected voxels, blocks in pool
    //                   order, voxels x + 8y + 64z ascending.  false when the call failed.
    std::shared_ptr<registration::RegistrationResult> RegisterVolume(const CubeHandler& source,
                                                                     const geometry::TransformationMatrix& init = geometry::TransformationMatrix::Identity(),
                                                                     const op_volume_band_params* sel = nullptr, const op_volume_register_color_params* params = nullptr,
                                                                     const op_volume_register_options* options = nullptr,
                                                                     op_volume_register_volume_result* details = nullptr);
    bool GetBandVoxels(geometry::Point3List& points, std::vector<float>& sdf, std::vector<float>& intensity, const op_volume_band_params* sel = nullptr) const;
    void GenerateMeshByCube(const CubeID& cube_id, geometry::TriangleMesh& mesh);
    std::shared_ptr<geometry::PointCloud> GetPointCloud() const;
    std::shared_ptr<CubeHandler> Transform(const geometry::TransformationMatrix& trans) const;
    std::shared_ptr<CubeHandler> TransformNearest(const geometry::TransformationMatrix& trans);
    // EXTENSION (not in the reference, whose only way to a cheaper model is to fuse every frame again at a larger voxel): a NEW handler of
    // 2^levels times the voxel size, on the device (op_volume_coarsen states the definition).  A voxel centre is (index + 0.5) * res, so a voxel
    // of twice the size covers exactly 2 x 2 x 2 fine voxels: its sdf and colour are their weighted means over the children of weight > 0 and
    // >= min_weight, summed in a fixed order, and its weight is their sum / 8.  This handler is not changed; the result's
    // c_para.VoxelResolution is the doubled one, and it is an ordinary handler (meshing, rendering, sampling, registration, Merge, fusion).
    // An empty pointer (after a message) when the call failed.  stats: the last level's counts.
    std::shared_ptr<CubeHandler> Coarsen(int levels = 1, float min_weight = 0, op_volume_coarsen_stats* stats = nullptr) const;
    CubeMap GetCubeMap();
    void SetCubeMap(const CubeMap& _cube_map);
    void SetFarPlane(float _far);
    void SetNearPlane(float _near);

    // ---- beyond the reference's surface -------------------------------------------------------------------
    // blocks currently allocated (cube_map.size() in the reference); flushes
    size_t GetCubeCount() const;
    // waits until every queued frame has been fused
    void Synchronize() const;
    // frame-sharded fusion: merges the volumes of all ranks of an RCCL communicator into `root`'s with one
    // reduce; see op_volume_merge_rccl.  comm is an ncclComm_t.
    bool MergeAcrossRanks(void* nccl_comm, int root);
    // the C-ABI handle (created on first use), for callers that mix in direct op_volume_* calls
    op_volume* Handle() const;

    // pushes what a derived class wrote through `cube_map` to the device now (it happens by itself before the next member call)
    void CommitCubeMap();

  protected:
    camera::PinholeCamera camera;
    Integrator integrator;
    CubePara c_para;
    float far = 5.0;
    float near = 0.5;
    CubeMapMirror cube_map; // CubeHandler.h:359: see CubeMapMirror

  private:
    friend class CubeMapMirror;
    void Pending() const;                // uploads an edited mirror; first statement of every member that looks at or changes the volume
    void Touch() const { ++changes; }    // the device volume has (possibly) changed: the mirror is stale
    mutable unsigned long long changes = 1;
    bool Ensure() const;                 // creates the device volume on first use; false (after a message) without a GPU
    static void Report(const char* where);
    void AddTransformedCubes(const VoxelCube& v_cube, const geometry::TransformationMatrix& trans, bool nearest);
    mutable op_volume* vol = nullptr;
    void Collect(float min_weight, const int32_t* lo, const int32_t* hi, const char* where);
    // device images of frames that were fused in place (RGBDFrame::on_device): held until the volume is known to be done with them
    mutable std::deque<std::pair<unsigned long long, std::shared_ptr<void> > > borrowed_; // (position among the volume's accepted frames, images)
    void ReleaseBorrowed() const { borrowed_.clear(); } // call only right after a synchronising C-ABI call
    explicit CubeHandler(op_volume* adopted, const CubeHandler& like, float resolution);
};

} // namespace integration
} // namespace one_piece
