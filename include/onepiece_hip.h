/*
 * onepiece_hip.h -- C-ABI of the MI355X (gfx950) implementation of OnePiece's TSDF-fusion + ICP
 * hot path.  This is the drop-in boundary: the reference has no FFI layer (its boundary is the C++
 * header surface one_piece::integration::CubeHandler / one_piece::registration::PointToPlane), so
 * every entry point below names the reference declaration (file:line under /root/reference/src)
 * whose work it replaces; INTEGRATION.md shows the forwarding calls a maintainer adds inside the
 * reference's CubeHandler / ICP to bind them.
 *
 * Conventions
 *   - extern "C", POD only, caller-allocated outputs, int return: 0 = OP_OK, otherwise an
 *     op_status; op_last_error() returns a thread-local description of the last failure.
 *   - All 4x4 matrices are ROW-MAJOR float[16] (the shim transposes Eigen's column-major storage).
 *   - Images: depth is float32 metres (OP_DEPTH_F32, cv CV_32FC1) or uint16 / depth_scale
 *     (OP_DEPTH_U16, cv CV_16UC1), row-major width x height; colour is 3 bytes / pixel in stored
 *     channel order (cv CV_8UC3).  `mem` says where image/point buffers live: OP_MEM_HOST buffers
 *     are copied to the device by the call, OP_MEM_DEVICE buffers are used in place and must stay
 *     valid until op_volume_sync()/the next synchronising call.
 *   - A volume owns one HIP stream.  op_volume_integrate() only enqueues work; every accessor that
 *     returns data synchronises first (SURVEY.md 8b "Threading").
 *   - There is NO CPU fallback: every compute entry point fails with OP_ERR_NO_DEVICE when no
 *     gfx950 device is usable.
 */
#ifndef ONEPIECE_HIP_H
#define ONEPIECE_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OP_ABI_VERSION 1

typedef enum {
    OP_OK = 0,
    OP_ERR_INVALID = 1,      /* bad argument */
    OP_ERR_NO_DEVICE = 2,    /* no usable HIP device / HIP runtime error */
    OP_ERR_CAPACITY = 3,     /* block pool or hash table exhausted (create with more max_blocks) */
    OP_ERR_MISMATCH = 4,     /* e.g. Merge of volumes with different voxel resolution */
    OP_ERR_NO_NORMALS = 5,   /* PointToPlane without target normals (ICP.cpp:159-163) */
    OP_ERR_HIP = 6
} op_status;

enum { OP_DEPTH_F32 = 0, OP_DEPTH_U16 = 1 };
enum { OP_MEM_HOST = 0, OP_MEM_DEVICE = 1 };
enum { OP_ICP_POINT_TO_POINT = 0, OP_ICP_POINT_TO_PLANE = 1 };
enum { OP_TRACK_HYBRID = 0, OP_TRACK_PHOTO = 1, OP_TRACK_DEPTH = 2 }; /* DenseTracking term_type (Odometry.cpp:546-553) */

/* camera::PinholeCamera (Camera/Camera.h:13-131) as a POD. */
typedef struct {
    float fx, fy, cx, cy;
    int32_t width, height;
    float depth_scale;
} op_camera;

typedef struct op_volume op_volume; /* device-resident integration::CubeHandler state */
typedef struct op_icp op_icp;       /* device-resident target cloud + search grid */
typedef struct op_tracker op_tracker; /* dense RGB-D tracker workspace (stream, device state) */
typedef struct op_nn_index op_nn_index; /* a target cloud and its search grid for batches of exact 1-NN queries */

/* ---- library ----------------------------------------------------------------------------- */
int op_abi_version(void);
const char *op_last_error(void);
/* ---- process-wide settings.  The library reads nothing from the environment and changes nothing in it on its own (rounds 1-4 set
 * GPU_MAX_HW_QUEUES from a load-time constructor and took test hooks from ONEPIECE_* variables): a host opts in through these calls.
 *
 * op_runtime_configure(hw_queues): every volume and every tracker owns a HIP stream, and streams that share a hardware queue serialise;
 *   the runtime maps streams onto 4 queues unless GPU_MAX_HW_QUEUES says otherwise, and reads that variable ONCE, at its first API call.
 *   This call sets it (never overwriting a value the caller has set) -- to be made before the process touches HIP; the C++ class surface
 *   (host/one_piece) makes it when its first device object is constructed, the Python package before it loads the library -- both ask for 16:
 *   K one-workgroup kernels on K streams take ceil(K / queues) kernel times (tools/queue_probe.hip), and the tracking + fusion pipeline's rate with
 *   16 pairs in flight goes from 349 to 489 frames/s between 8 and 16 queues (with 32 the rates of a process that also runs torch collapse).
 * op_runtime_hw_queues: what is in the variable now (4 = the runtime's default when unset); whether the runtime had already read it cannot be known. */
int op_runtime_configure(int hw_queues);
int op_runtime_hw_queues(int *requested);
/* op_runtime_set_option:
 *   OP_RUNTIME_OPT_MERGE_ALGORITHM        OP_MERGE_OWNER_EXCHANGE (default) / OP_MERGE_DENSE_REDUCE -- see op_volume_merge_rccl
 *   OP_RUNTIME_OPT_MERGE_SLICE_BLOCKS     union blocks per reduce slice of the dense merge (0 = the built-in 32 768; tests force several slices)
 *   OP_RUNTIME_OPT_MERGE_FORCE_SINGLE_RANK  1: run the whole exchange with a one-rank communicator too (how a one-GPU box exercises the RCCL path)
 *   OP_RUNTIME_OPT_TRACKER_GRAPH          0: trackers created afterwards issue plain launches instead of replaying a captured hipGraph
 *   OP_RUNTIME_OPT_COPY_THREADS           0 .. 8 helper threads of the pageable -> pinned staging copies (before the first host image)
 *   OP_RUNTIME_OPT_CACHE_DEVICE_BYTES     bytes of RELEASED device buffers (block pools, cell tables, images) the library keeps per device for the next
 *                                         request of a similar size instead of returning them to the driver (default 32 GB; 0 = keep none; buffers
 *                                         already kept stay until op_release_cached_memory)
 *   OP_RUNTIME_OPT_MERGE_FAULT            TEST HOOK: stage * 1024 + rank + 1 makes that rank's allocation of that stage of the owner-exchange merge fail
 *                                         (stage 1: the partition's sums after the exchange; stage 2: the root's gather buffers) -- every rank must then
 *                                         return an error, nobody may wait inside RCCL (tests/test_config5_gpu.py); 0 = off (default)
 *   OP_RUNTIME_OPT_ICP_DEFAULT_SUMS       the OP_ICP_OPT_SUMS mode of ICP contexts created afterwards (op_icp_create, op_icp_register, hence
 *                                         registration::PointToPlane / PointToPoint of the class surface).  Default OP_ICP_SUMS_REFERENCE_F32: the reference's own
 *                                         sequential float32 sums, the mode whose pose is within 1e-4 of the CPU path's on EVERY pair (~0.6 k iterations/s at
 *                                         307 200 points); OP_ICP_SUMS_FP64 opts into the order-free fp64 reduction (~24 k iterations/s; equal to the CPU path
 *                                         with double sums, but up to 1e-2 from its float32 answer where J^T J is rank-deficient -- DESIGN.md section 5)
 *   OP_RUNTIME_OPT_TRACKER_DEFAULT_SUMS   likewise the OP_TRACK_OPT_SUMS mode of trackers created afterwards (Odometry::DenseTracking of the class surface): default
 *                                         OP_TRACK_SUMS_REFERENCE_F32 (every pair within 1e-4 of the CPU path: ~75 tracks/s alone, ~230 frames/s with four pairs in flight);
 *                                         OP_TRACK_SUMS_FP64 opts into the fp64 reduction (~2.2 k tracks/s; 20 of 23 pairs of the bench's chain within 1e-4, worst 4.4e-4)
 *   OP_RUNTIME_OPT_TRACKER_BATCH_SUMS     0 (default): every tracker launches its own one-workgroup sum kernel.  1: twelve or more trackers in the reference-order mode that
 *                                         run at the same time (pairs in flight of a pipeline) meet once per iteration and take their sequential sums in ONE launch, a
 *                                         workgroup per tracker (what op_icp_run_many does for nine or more reference-order ICP contexts).  Measured WITHOUT gain for the
 *                                         tracker (profiles/r06_track_depth_probe.txt): what its pipeline needs is a hardware queue per tracker stream
 *                                         (op_runtime_configure(16)).  Results do not depend on it.
 *   OP_RUNTIME_OPT_ICP_MANY_IN_FLIGHT     iterations op_icp_run_many keeps enqueued at a time, in turn over its fp64-mode contexts (default 4, 1 .. 1024)
 *   OP_RUNTIME_OPT_GLOBAL_REGISTRATION    0 (default): the class surface's global registration (registration::ComputeFPFHFeature, FeatureMatching3D, DownSampleAndExtractFeature,
 *                                         RansacRegistration, geometry::EstimateRigidTransformationRANSAC) runs its host loops, exactly as before the option existed.  1: the
 *                                         same functions forward to op_fpfh_compute / op_feature_match / op_ransac_count_inliers / op_ransac_inlier_ids.  The C-ABI entries
 *                                         themselves do not look at it; op_runtime_get_option lets the class surface read it.
 *   OP_RUNTIME_OPT_POINT_CLOUD_DOWNSAMPLE 0 (default): geometry::PointCloud::DownSample of the class surface runs its host loop, exactly as before the option existed.
 *                                         1: it forwards to op_point_cloud_downsample (bit-identical), and falls back to the host loop for a cloud the device entry
 *                                         refuses (OP_ERR_INVALID, OP_ERR_CAPACITY).  Read through op_runtime_get_option like the option above.
 *   OP_RUNTIME_OPT_MESH_CLUSTERING        0 (default): geometry::TriangleMesh::ClusteringSimplify of the class surface runs its host loop, exactly as before the option existed.
 *                                         1: it forwards to op_mesh_cluster_simplify (bit-identical), and falls back to the host loop for a mesh the device entry
 *                                         refuses (OP_ERR_INVALID, OP_ERR_CAPACITY).  Read through op_runtime_get_option like the two options above.
 *   OP_RUNTIME_OPT_MESH_POSTPROCESS       0 (default): geometry::TriangleMesh::ComputeNormals and Prune of the class surface run their host loops, exactly as before the option
 *                                         existed.  1: they forward to op_mesh_compute_normals / op_mesh_prune (bit-identical), and fall back to the host loop for a mesh the
 *                                         device entry refuses (OP_ERR_INVALID, OP_ERR_CAPACITY).  Read through op_runtime_get_option like the three options above.
 *   OP_RUNTIME_OPT_COLOR_ALIGNMENT        0 (default): tool::AlignColorToDepth of the class surface runs its host loop.  1: it forwards to op_align_color_to_depth
 *                                         (bit-identical), and falls back to the host loop for images the device entry refuses (OP_ERR_INVALID, OP_ERR_CAPACITY).
 *                                         Read through op_runtime_get_option like the four options above.
 *   OP_RUNTIME_OPT_NEAREST_BATCH          0 (default): geometry::KDTree<3>::NearestBatch and tool::TransferLabels of the class surface run the loop of KnnSearch(q, ..., 1)
 *                                         that example/GetLabelUsingKDTree.cpp writes.  1: they forward to op_nn_index_query / op_nn_index_transfer_labels (the same
 *                                         indices and distance bits), and fall back to the host loop for input the device entry refuses (OP_ERR_INVALID, OP_ERR_CAPACITY).
 *                                         Read through op_runtime_get_option like the five options above.
 *   OP_RUNTIME_OPT_ALLOC_FAULT            TEST HOOK: k > 0 makes the k-th request to the library's buffer cache from now (device or pinned, process-wide) fail as if the
 *                                         device were out of memory -- a host-side error return, before HIP or the cache is touched; once it has fired the option is 0
 *                                         again (default; op_runtime_get_option reads it).  tests/test_scoped_buffers_gpu.py: every entry returns OP_ERR_HIP and leaves
 *                                         nothing behind in the cache's live set (op_debug_cache_live)
 * op_runtime_set_rccl_library(path): the RCCL to bind at the first merge instead of "librccl.so.1" (a site build; the test suite names a
 *   host-memory double that runs several ranks on one device); NULL = the system's.  Fails once RCCL has been bound. */
#define OP_RUNTIME_OPT_MERGE_ALGORITHM 0
#define OP_RUNTIME_OPT_MERGE_SLICE_BLOCKS 1
#define OP_RUNTIME_OPT_MERGE_FORCE_SINGLE_RANK 2
#define OP_RUNTIME_OPT_TRACKER_GRAPH 3
#define OP_RUNTIME_OPT_COPY_THREADS 4
#define OP_RUNTIME_OPT_CACHE_DEVICE_BYTES 5
#define OP_RUNTIME_OPT_MERGE_FAULT 6
#define OP_RUNTIME_OPT_ICP_DEFAULT_SUMS 7
#define OP_RUNTIME_OPT_TRACKER_DEFAULT_SUMS 8
#define OP_RUNTIME_OPT_TRACKER_BATCH_SUMS 9
#define OP_RUNTIME_OPT_ICP_MANY_IN_FLIGHT 10
#define OP_RUNTIME_OPT_GLOBAL_REGISTRATION 11
#define OP_RUNTIME_OPT_POINT_CLOUD_DOWNSAMPLE 12
#define OP_RUNTIME_OPT_MESH_CLUSTERING 13
#define OP_RUNTIME_OPT_MESH_POSTPROCESS 14
#define OP_RUNTIME_OPT_COLOR_ALIGNMENT 15
#define OP_RUNTIME_OPT_NEAREST_BATCH 16
#define OP_RUNTIME_OPT_ALLOC_FAULT 17
#define OP_MERGE_OWNER_EXCHANGE 0
#define OP_MERGE_DENSE_REDUCE 1
int op_runtime_set_option(int option, long long value);
int op_runtime_get_option(int option, long long *value); /* OP_RUNTIME_OPT_GLOBAL_REGISTRATION, OP_RUNTIME_OPT_POINT_CLOUD_DOWNSAMPLE, OP_RUNTIME_OPT_MESH_CLUSTERING, OP_RUNTIME_OPT_MESH_POSTPROCESS, OP_RUNTIME_OPT_COLOR_ALIGNMENT, OP_RUNTIME_OPT_NEAREST_BATCH and OP_RUNTIME_OPT_ALLOC_FAULT: the others are read inside the library */
int op_runtime_set_rccl_library(const char *path);
/* Images that are used more than once -- a frame is tracked against twice and fused once (example/DenseFusion/DenseSlam.cpp:24-33,
 * DenseFusion.cpp:86-96) -- can be brought to the device ONCE and then handed to op_tracker_dense_tracking(_enqueue) /
 * op_volume_integrate with OP_MEM_DEVICE.
 *   op_device_alloc    a buffer from the library's buffer cache (hipMalloc synchronises the whole device: allocate slabs, not frames)
 *   op_device_write    one or two host arrays -> the buffer at the given byte offsets: staged through pinned memory by the caller's thread
 *                      and the library's copy helpers, one DMA; blocking (complete and visible to every stream on return)
 *   op_device_upload   alloc + write of one array
 *   op_device_release  returns a buffer of op_device_alloc / op_device_upload
 * The caller keeps a buffer alive until its last consumer has finished (op_tracker_wait; for a volume: op_volume_progress). */
int op_device_alloc(size_t bytes, int device, void **device_ptr);
int op_device_write(void *device_ptr, size_t n_parts, const void *const *parts, const size_t *bytes, const size_t *offsets, int device);
int op_device_upload(const void *host, size_t bytes, int device, void **device_ptr);
int op_device_release(void *device_ptr, int device);
/* Registration objects (op_icp, the contexts behind op_icp_register / op_estimate_normals / op_points_from_depth) are
 * created and dropped per call, as registration::PointToPlane builds and drops its kd-tree (Registration/ICP.cpp:
 * 166-170); their device and pinned buffers, streams and events are kept in a per-process cache when released and
 * handed out again, so that a steady stream of calls does not allocate.  This empties the cache (at most 8 GB of
 * device memory per GPU and 1 GB of pinned memory are ever held). */
int op_release_cached_memory(void);
int op_device_count(int *count);
/* OPEN3D_DATASET / TUM_DATASET presets, Camera/Camera.h:76-104.  type: 0 = TUM, 1 = OPEN3D. */
int op_camera_preset(int type, op_camera *out);

/* ---- host-side geometry used on the path (bit-faithful to the reference's Eigen build) ---- */
/* geometry::TransformationMatrix::inverse() as Eigen 3.3.7 evaluates it with -msse4.2
 * (Integrator.cpp:18,48; 3rdparty/Eigen/Eigen/src/LU/arch/Inverse_SSE.h:35-165). */
int op_mat4_inverse(const float m[16], float out[16]);
/* geometry::VoxelGridHasher::operator() (Geometry/Geometry.h:101-112). */
uint64_t op_hash_key(int32_t x, int32_t y, int32_t z);
/* Frustum::ComputeFromCamera (Integration/Frustum.cpp:7-46): planes top,left,right,bottom,near,far. */
int op_frustum_planes(const op_camera *cam, const float pose[16], float far_dist, float near_dist,
                      float planes[24]);
/* The whole integration::Frustum object (Integration/Frustum.h:10-105): the six planes as above plus, when
 * corners != NULL, the eight corner points in the order of the reference's public `corners` member
 * (Frustum.cpp:49-56: far top-left, far top-right, far bottom-left, far bottom-right, near bottom-right,
 * near top-left, near top-right, near bottom-left).  op_frustum_from_camera = Frustum::ComputeFromCamera
 * (Frustum.cpp:7-24), op_frustum_from_vectors = Frustum::ComputeFromVectors (:25-94).  Host arithmetic in
 * the reference's float order; no device needed. */
int op_frustum_from_camera(const op_camera *cam, const float pose[16], float far_dist, float near_dist,
                           float planes[24], float corners[24]);
int op_frustum_from_vectors(const float forward[3], const float position[3], const float right[3],
                            const float up[3], float far_dist, float near_dist, float fov, float aspect,
                            float planes[24], float corners[24]);
/* Integrator::GetSDF (Integrator.cpp:8-35) for one world point against a HOST depth image: 999 when the point projects
 * off the image or onto a pixel without depth, else depth - z.  pose_inv may be NULL (computed as op_mat4_inverse).
 * A host scalar in the reference's float / double order; the kernels evaluate the same expression for every probe. */
int op_get_sdf(const op_camera *cam, const float point[3], const float pose[16], const float *pose_inv,
               const void *depth, int depth_fmt, float *sdf);
/* Test hook: the pixel rounding of Integrator.cpp:20-21 applied to a = fx*X/Z and c = cx.
 * fast = 0: the reference's double formula; fast = 1: the fp32/integer evaluation the kernels use
 * (valid when |c| >= 1 or c == 0).  Both return INT_MIN for values no int can hold. */
int op_debug_project_px(float a, float c, int fast);
/* Test hook (device): the kernels' projection of n operand triples -- u = (fx*X)/Z + 0.5 + cx, v likewise, the two
 * quotients sharing one refined reciprocal (csrc/volume_core.hpp: project_pixel) -- next to the same formula with the plain
 * IEEE division.  out: n x {u, v, u_plain, v_plain}; INT_MIN stands for "no int can hold it". */
int op_debug_project_uv(float fx, float fy, float cx, float cy, const float *X, const float *Y, const float *Z,
                        size_t n, int device, int32_t *out);
/* ... the same for an image of width x height pixels (op_debug_project_uv's is 640 x 480); {u, v} = {INT_MIN, INT_MIN} for a pixel outside it. */
int op_debug_project_uv_image(float fx, float fy, float cx, float cy, int width, int height, const float *X, const float *Y,
                              const float *Z, size_t n, int device, int32_t *out);
/* Test hook (device): TSDFVoxel::operator+ with other = (new_sdf, 1, rgb / 255) (Integration/TSDFVoxel.h:24-39; Integrator.cpp:74-87)
 * for n stored voxels {s, w, c0, c1, c2} and observations {new_sdf, rgba}, lanes packed 64 to a wave in input order.
 * out_fast: the fusion kernel's update of a volume it alone has written (csrc/integrate.hip voxel_update<true>: one hardware
 * reciprocal of the integer weight sum, three operations per quotient); out_ref: the two-branch form with four IEEE divisions
 * (voxel_update<false>).  Both n x {s, w, c0, c1, c2}.  Runs on device 0. */
int op_debug_voxel_update(const float *s, const float *w, const float *c0, const float *c1, const float *c2,
                          const float *new_sdf, const unsigned *rgba, long long n, float *out_fast, float *out_ref);
/* Test hook (device): out[i] = v_rcp_f32(x[i]), the unrefined hardware reciprocal (csrc/integrate.hip voxel_update<true>:
 * y = __builtin_amdgcn_rcpf(wsum)).  Runs on device 0. */
int op_debug_rcp(const float *x, long long n, float *out);
/* Test hook (host): the bound on |1 - Z * v_rcp_f32(Z)| that the certified pixel projection's error bound assumes of the unrefined
 * hardware reciprocal (csrc/px_round.hpp kPxRcpErr); tests/test_kc_diet_gpu.py holds op_debug_rcp to it over every significand. */
double op_debug_px_rcp_err(void);
/* Test hook (host): out[0..2] = the k_integrate launches this volume has enqueued since it was created (replays included), by the form of the
 * projection and the gather: exact projection; certified projection without the window test on Z (csrc/zwin_cert.hpp proves its upper side per
 * frame on the host) with the raw gather; the same with the structured gather.  A batch with a frame the host cannot certify counts under [0]. */
int op_debug_volume_gather_kinds(op_volume *v, unsigned long long *out);
/* Test hook (host): what k_prepare_frames is told about a frame of this camera at this pose (csrc/ka_cert.hpp): rect = {j_lo, j_hi, i_lo,
 * i_hi} and z = {z_lo, z_hi}, the pixels and depths certified to lie inside the frame's own frustum (j_lo > j_hi: no certificate), and
 * quot = whether the three-operation quotients by fx, fy and (for 16-bit depth) depth_scale are in use. */
int op_debug_ka_certificate(const op_camera *cam, const float pose[16], float far_dist, float near_dist, int32_t rect[4], float z[2], int32_t quot[3]);
/* Test hook (device): the fusion kernel's structured gather (csrc/volume_core.hpp gather2d: a buffer descriptor with stride = one image
 * row and num_records = the rows does the row test and the address arithmetic) of n pixels uv = n x {u, v}, each in [-2^23, 2^23), from
 * frame `frame` of a stack of n_frames packed images (images: n_frames x height x width records {depth bits, rgba}; width <= 2047).
 * out: n x {depth bits, rgba}, {0, 0} for a pixel outside the image.  column_test = 1: gather2d as the kernel uses it; 0: the descriptor
 * alone (vindex = v, voffset = u * 8) -- what the hardware's range check makes of the pair; every address base + v * stride + u * 8
 * must then lie inside the stack.  Runs on device 0. */
int op_debug_gather2d(const unsigned *images, int width, int height, int n_frames, int frame, int column_test, const int *uv,
                      long long n, unsigned *out);
/* Test hook (host): the rows of one tile of the sequential-sum kernels (csrc/seq_sums.hip kSeqRows); the tests derive their sizes from it. */
int op_debug_seq_tile_rows(void);
/* TEST HOOK: how many buffers of `device` the buffer cache has handed out and not got back (device memory, pinned host memory; either pointer may be NULL) */
int op_debug_cache_live(int device, uint64_t *device_buffers, uint64_t *pinned_buffers);
/* Test hook (device): the in-order float32 sums of the reference-order modes (csrc/seq_sums.hip k_seq_sums) over rows the caller makes up.
 * layout 0 / 1 / 2 = one row {J[6], r} per item / two such rows per item / two values per item, summed as they are (7, 14, 2 floats per
 * item; 42, 42, 2 sums).  All n_uploaded items of the host array `rows` go to the device, the first n_items <= n_uploaded <= 2^24 of them
 * are summed through the production object (SeqSums::run, one workgroup on a stream of its own); rows may be NULL only when both counts
 * are 0.  out: the sums, then n_items as an unsigned word.  OP_ERR_NO_DEVICE where the device cannot run the kernel.  Runs on device 0. */
int op_debug_seq_sums(int layout, const float *rows, unsigned n_uploaded, unsigned n_items, float *out);
/* Test hook (device): k problems of that layout, 1 <= k <= 32, in ONE launch of k_seq_sums_many, a workgroup each (what a meeting of
 * reference-order contexts launches).  rows[i]: host array of n_items[i] <= 2^24 items, may be NULL when n_items[i] is 0.
 * out: k x {the sums, n_items[i]}.  Runs on device 0. */
int op_debug_seq_sums_many(int layout, const float *const *rows, const unsigned *n_items, int k, float *out);
/* geometry::Se3ToSE3 (Geometry/Geometry.cpp:9-13). */
int op_se3_exp(const float x[6], float T[16]);

/* ---- integration::CubeHandler (Integration/CubeHandler.h:24-366) ------------------------- */
/* CubeHandler(const PinholeCamera&) + SetVoxelResolution + SetTruncation + SetFar/NearPlane.
 * max_blocks sizes the device block pool (10 KiB per 8^3 block) and hash table; 0 = default. */
int op_volume_create(const op_camera *cam, float voxel_res, float truncation, float far_dist,
                     float near_dist, int device, uint64_t max_blocks, op_volume **out);
int op_volume_destroy(op_volume *v);
int op_volume_set_resolution(op_volume *v, float voxel_res);  /* CubeHandler.h:36-39 */
int op_volume_set_truncation(op_volume *v, float truncation); /* CubeHandler.h:141-144 */
int op_volume_set_camera(op_volume *v, const op_camera *cam); /* CubeHandler.h:137-140 */
int op_volume_set_near_far(op_volume *v, float near_dist, float far_dist); /* CubeHandler.h:339-346 */
/* OP_VOLUME_OPT_UPDATE: how the frames of a batch reach a voxel (TSDFVoxel::operator+, Integration/TSDFVoxel.h:24-39; Integrator.cpp:74-87).
 *   OP_VOLUME_UPDATE_EXACT (default): frame by frame in frame order, every product, sum and quotient rounded as the reference rounds it --
 *     voxels bit-identical to the reference's CPU path.
 *   OP_VOLUME_UPDATE_SUM_FORM: the observations a batch of frames (<= 32) makes of a voxel are summed and the weighted mean with the stored
 *     voxel is formed once per batch.  Same blocks, same pixels, same weights; sdf and colour agree with the reference to float rounding
 *     (<= 1e-6 of the truncation distance / of 1 in practice; the path's bar is 1e-4 relative).  The integrate kernel executes a third
 *     fewer instructions per voxel and frame.  Precondition: truncation < 1 -- the reference re-tests IsValid (sdf < 1) before every frame,
 *     the sum form once per batch (on the stored voxel), and the two only agree while no observation can itself be "invalid"; with
 *     truncation >= 1 the exact update runs whatever this option says.
 * Changing the option waits for the frames accepted so far (they are fused under the old setting). */
#define OP_VOLUME_OPT_UPDATE 0
#define OP_VOLUME_UPDATE_EXACT 0
#define OP_VOLUME_UPDATE_SUM_FORM 1
/* OP_VOLUME_OPT_SELECT: which form of the selection step (CubeHandler::PrepareCubes, CubeHandler.cpp:147-196) a batch takes.  The
 * selected set is the same either way (tests/test_integration_gpu.py); a tuning and test knob, not part of the reference's surface.
 *   OP_VOLUME_SELECT_AUTO (default): in batches of >= 20 frames the frames record their selections per super-block (4 x 4 x 4 blocks) and one pass
 *                                    claims every block once (faster from ~16 frames on); a frame whose candidate range exceeds 2^18 super-blocks,
 *                                    and every frame of a shorter batch, claims its blocks directly;
 *   OP_VOLUME_SELECT_DIRECT: every frame claims directly (the only form of rounds 1-3);
 *   n >= 1: every batch of >= 2 frames takes the recording form, with n super-blocks as the limit (forces every mix of the two on small scenes). */
#define OP_VOLUME_OPT_SELECT 1
#define OP_VOLUME_SELECT_AUTO 0
#define OP_VOLUME_SELECT_DIRECT -1
/* OP_VOLUME_OPT_RAYCAST_PRUNE (default 1): op_volume_raycast remembers, per block it loaded, whether the block holds an observed sdf <= 0 / > 0,
 * and later views use that to drop blocks in which no zero crossing can end before loading them.  Fusion with the default (exact) update keeps
 * the knowledge current -- the kernel that changes a block restates its summary -- so a view that follows a fused frame still prunes; every other
 * writer (sum-form fusion, upload, merge, resampling, clear, pool growth) invalidates what was remembered.  0: every view loads every visible block,
 * as the first view after such a change does.
 * The images are identical either way (tests/test_volume_ops_gpu.py); a measurement and test knob. */
#define OP_VOLUME_OPT_RAYCAST_PRUNE 2
int op_volume_set_option(op_volume *v, int option, int value);
/* How far the volume has got with the frames handed to op_volume_integrate / _sequence, WITHOUT waiting: frames accepted so far, and how many
 * of them belong to batches the device has reported complete (frames are queued up to 32 per launch and a launched batch may still be
 * replayed after a pool growth).  Device images of the first `frames_done` frames (OP_MEM_DEVICE, in call order) are
 * no longer read and may be released or overwritten; host images are only borrowed for the call anyway.  Every queue entry counts: a
 * de-integration is one, a re-integration two. */
int op_volume_progress(op_volume *v, uint64_t *frames_accepted, uint64_t *frames_done);
int op_volume_clear(op_volume *v);                            /* CubeHandler.h:133-136 */
int op_volume_sync(op_volume *v);
/* Launches the frames op_volume_integrate / op_volume_integrate_sequence have queued (a batch smaller than 32), without
 * waiting for them: for callers that want the GPU to start now although more frames will follow.  No reference counterpart
 * (the reference fuses inside the call). */
int op_volume_flush(op_volume *v);
int op_volume_block_count(op_volume *v, size_t *n);
int op_volume_has_cube(op_volume *v, int32_t x, int32_t y, int32_t z, int *present); /* :129-132 */
/* Raw HIP stream handle of the volume (hipStream_t), for callers that time with HIP events. */
int op_volume_stream(op_volume *v, void **stream);

/* CubeHandler::ComputeBounding (CubeHandler.cpp:116-145). */
int op_volume_compute_bounding(op_volume *v, const void *depth, int depth_fmt, int mem,
                               const float pose[16], float max_pos[3], float min_pos[3],
                               size_t *n_inside);
/* CubeHandler::PrepareCubes (CubeHandler.cpp:147-196): selects + allocates blocks; ids_xyz gets the
 * cube_id_list in the reference's i,j,k loop order (n x 3).  *n is the full list length even when
 * it exceeds cap.  pose_inv may be NULL (then op_mat4_inverse(pose) is used). */
int op_volume_prepare_cubes(op_volume *v, const void *depth, int depth_fmt, int mem,
                            const float pose[16], const float *pose_inv, int32_t *ids_xyz,
                            size_t cap, size_t *n, size_t *n_candidates);
/* CubeHandler::IntegrateImage(depth, rgb, pose) (CubeHandler.cpp:197-210 -> Integrator.cpp:36-94).
 * Asynchronous: frames are queued and fused up to 32 at a time (results identical to frame-by-frame
 * fusion); every accessor / setter / op_volume_sync flushes the queue first.  OP_MEM_HOST images are
 * copied before the call returns; OP_MEM_DEVICE images must stay valid until the next
 * synchronising call. */
int op_volume_integrate(op_volume *v, const void *depth, int depth_fmt, const uint8_t *rgb,
                        int mem, const float pose[16], const float *pose_inv);
/* Integrator::IntegrateImage(depth, rgb, pose, camera, voxel_cube, c_para) (Integrator.cpp:36-94), the reference's
 * public per-cube member, for a caller-chosen list of n cube ids: the frame is fused into exactly those cubes
 * (allocated when absent; a cube listed twice is fused once), without PrepareCubes' selection.  Synchronous. */
int op_volume_integrate_cubes(op_volume *v, const void *depth, int depth_fmt, const uint8_t *rgb, int mem,
                              const float pose[16], const float *pose_inv, const int32_t *keys_xyz, size_t n);
/* Multi-frame form of the same call for frames already resident on the device: frame f uses
 * depth + f*depth_stride_bytes, rgb + f*rgb_stride_bytes, poses + 16*f.  Results are bit-identical
 * to n_frames sequential op_volume_integrate calls -- the frames join the same queue: they are fused in batches of
 * up to 32 per kernel launch (inside a batch every voxel applies its frames in order in registers), a remainder
 * waits for the next frames or the next flushing call, and the images must stay valid until then. */
int op_volume_integrate_sequence(op_volume *v, const void *depth, size_t depth_stride_bytes,
                                 int depth_fmt, const uint8_t *rgb, size_t rgb_stride_bytes,
                                 const float *poses, size_t n_frames);
/* tool::AlignColorToDepth (Tool/IO.cpp:9-58): the colour image of a second camera re-sampled onto the depth pixels.  aligned_out is
 * depth_cam->height x depth_cam->width x 3 bytes.  Per depth pixel (v, u) with z = depth(v, u) (uint16: (float)d / depth_cam->depth_scale): nothing is
 * sampled (0, 0, 0) unless z > 0; x = ((float)u - cx_d) * z / fx_d, y likewise; q = color_to_depth (x, y, z, 1), p = q.xyz / q.w; a = p0 / p2, b = p1 / p2,
 * c = p2 / p2; uf = fx_c * a + cx_c * c, vf = fy_c * b + cy_c * c (float32, no contraction); cu = (int)((double)uf + 0.5), cv likewise (truncation);
 * the pixel copies color(cv, cu) when 0 <= cu < color_cam->width and 0 <= cv < DEPTH_cam->height -- the reference's own bound (IO.cpp:33).  Only z of the
 * depth-camera point is tested; a point behind the colour camera is sampled like any other.  Defined here where the reference is not: a NaN or a value
 * whose truncation does not fit an int is rejected, and so is a (cv, cu) outside the color_rows x color_cols image that was passed (the reference reads
 * past its image there).  The depth image has the depth camera's size; color_to_depth is row-major, NULL = identity.  Host or device buffers (mem), like
 * op_points_from_rgbd; synchronous. */
int op_align_color_to_depth(const op_camera *color_cam, const op_camera *depth_cam, const uint8_t *color, int color_rows, int color_cols,
                            const void *depth, int depth_fmt, const float *color_to_depth /* NULL = identity */, int mem, int device,
                            uint8_t *aligned_out);
/* IntegrateImage(depth, AlignColorToDepth(color, depth, color_cam, volume camera, color_to_depth), pose) (Tool/IO.cpp:9-58, then CubeHandler.cpp:197-210):
 * the aligned image is made on the volume's stream into a ring of 64 images the volume owns, and the frame joins the queue of op_volume_integrate as a
 * device-resident frame.  A ring slot is rewritten only after the batch that reads it is confirmed complete (a replay after pool growth reads it again);
 * if the device is that far behind, the call waits.  OP_MEM_HOST images are copied before the call returns; OP_MEM_DEVICE: the colour image is read by
 * work enqueued here, the depth image is used in place -- both must stay valid until the next synchronising call. */
int op_volume_integrate_unaligned(op_volume *v, const void *depth, int depth_fmt, const uint8_t *color, int color_rows, int color_cols,
                                  const op_camera *color_cam, const float *color_to_depth, int mem, const float pose[16],
                                  const float *pose_inv);
/* Multi-frame form for frames resident on the device (Tool/IO.cpp:9-58 per frame), mirroring op_volume_integrate_sequence: frame f uses
 * depth + f*depth_stride_bytes, color + f*color_stride_bytes, poses + 16*f; one colour camera, one color_to_depth.  Bit-identical to n_frames
 * op_volume_integrate_unaligned calls. */
int op_volume_integrate_unaligned_sequence(op_volume *v, const void *depth, size_t depth_stride_bytes, int depth_fmt, const uint8_t *color,
                                           size_t color_stride_bytes, int color_rows, int color_cols, const op_camera *color_cam,
                                           const float *color_to_depth, const float *poses, size_t n_frames);
/* DE-INTEGRATION: take a fused frame out of the volume again (NO reference member; the arithmetic is the reference's own).  D(depth, rgb, pose)
 * takes the steps of IntegrateImage(depth, rgb, pose) (Integrator.cpp:52-92): the frame is prepared and its blocks are selected as for a fused frame --
 * neither depends on what the volume stores -- and a selected block the volume does not hold is ALLOCATED, all-default, exactly as integration would.
 * Every voxel of a selected block is projected to the same pixel and tested by the same predicate (pixel inside, d > 0, |new_sdf| < truncation).  A voxel
 * that passes holds (s, w, c); with the observation o = new_sdf and oc = byte / 255 per channel it receives TSDFVoxel::operator+ (TSDFVoxel.h:24-39)
 * with an observation of weight -1, the inverse of the running mean:
 *   1. applied iff TSDFVoxel::IsValid (!(s >= 1 || w <= 0)) and w >= 1; otherwise the voxel is left as it is and counted `skipped` (never observed,
 *      invalid, or a fractional weight < 1 from an upload or a merge; the reference's `weight == 0 -> return other` would store weight -1: not reproduced);
 *   2. rw = w + (-1) in float32;
 *   3. rw == 0: the voxel becomes the default voxel {999, 0, -1, -1, -1}, the reference's default-constructed result (`reset`);
 *   4. otherwise s' = (RN(w s) + RN(-1 o)) / rw, the same per colour channel, w' = rw (`reverted`): every product, sum and quotient rounded to float32.
 * So a frame fused and de-integrated at the SAME pose leaves the weights exactly as they were, a voxel only that frame had seen default again, and sdf /
 * colour within a few float32 roundings per operation of never having fused it (tests/test_deintegrate_cpu.py derives the bound).
 * Queue entries -- integrations and de-integrations alike -- are applied to a voxel in call order; they share the queue and its batches of up to 32
 * per launch, and a batch that holds a de-integration runs one kernel (k_integrate's SIGNED form) for all its entries.  After such a launch the volume keeps the
 * general (reference-literal) update for the blocks that existed then, and the shorter exact forms of k_integrate's first frames are not used again
 * until op_volume_clear; OP_VOLUME_UPDATE_SUM_FORM does not apply to such a launch (its entries take the exact forms); the raycaster's block summaries
 * are invalidated.  Images: as for op_volume_integrate (OP_MEM_HOST copied before the call returns, OP_MEM_DEVICE valid until the next synchronising
 * call).  Frames of a second colour camera are aligned first (op_align_color_to_depth). */
int op_volume_deintegrate(op_volume *v, const void *depth, int depth_fmt, const uint8_t *rgb, int mem, const float pose[16],
                          const float *pose_inv);
/* Multi-frame form for device-resident frames, mirroring op_volume_integrate_sequence (TSDFVoxel.h:24-39 with weight -1 under the predicate of
 * Integrator.cpp:52-92, as above): bit-identical to n_frames op_volume_deintegrate calls in order. */
int op_volume_deintegrate_sequence(op_volume *v, const void *depth, size_t depth_stride_bytes, int depth_fmt, const uint8_t *rgb,
                                   size_t rgb_stride_bytes, const float *poses, size_t n_frames);
/* R(depth, rgb, old_pose, new_pose) = D(old_pose) then I(new_pose) (TSDFVoxel.h:24-39 with weights -1 and +1 under the predicate of
 * Integrator.cpp:52-92, as above) as two entries of the queue on ONE uploaded copy of the images: a frame that was fused at old_pose moves to
 * new_pose.  Both entries stay in one launch.  With old_pose == new_pose every weight is exactly unchanged. */
int op_volume_reintegrate(op_volume *v, const void *depth, int depth_fmt, const uint8_t *rgb, int mem, const float old_pose[16],
                          const float new_pose[16]);
/* Multi-frame form for device-resident frames: D(old_poses + 16 f), I(new_poses + 16 f) for f = 0 .. n_frames - 1 in that order (definition above:
 * TSDFVoxel.h:24-39, Integrator.cpp:52-92), 16 frames per launch. */
int op_volume_reintegrate_sequence(op_volume *v, const void *depth, size_t depth_stride_bytes, int depth_fmt, const uint8_t *rgb,
                                   size_t rgb_stride_bytes, const float *old_poses, const float *new_poses, size_t n_frames);
/* Counters of the de-integrations since create/clear (synchronises): frames de-integrated, and of their voxels that passed the predicate of
 * Integrator.cpp:52-92 those that were reverted (step 4 above), reset to the default voxel (step 3) and skipped (step 1; TSDFVoxel.h:24-39). */
int op_volume_deintegrate_stats(op_volume *v, uint64_t *frames, uint64_t *reverted, uint64_t *reset, uint64_t *skipped);

/* CubeHandler::CollectGarbage (declared at Integration/CubeHandler.h:357, never defined by the reference; no reference counterpart for the box and
 * the weight bound): frees the blocks no frame supports any more -- what a de-integration leaves behind, what PrepareCubes selected and nothing
 * ever updated -- and, on request, the blocks outside a box of block ids or below a weight.  THE DEFINITION:
 *   - Like every accessor the call first sees all frames accepted before it (flush, synchronise, grow + replay); n = the blocks then.
 *   - inside(b): true when box_lo and box_hi are both NULL; otherwise box_lo[a] <= CubeID(b)[a] <= box_hi[a] on every axis a, inclusive, in block
 *     ids.  Exactly one of them NULL -> OP_ERR_INVALID.  box_lo[a] > box_hi[a] on an axis is legal and empties the volume.
 *   - observed(b): some voxel of b has w > 0 && w >= min_weight (one float comparison pair per voxel; a NaN or negative weight, which only
 *     foreign data can hold, counts as unobserved -- what TSDFVoxel::IsValid, TSDFVoxel.h:75-78, makes of it).  min_weight must be finite and
 *     >= 0, otherwise OP_ERR_INVALID; 0 is pure garbage collection.
 *   - b is kept iff inside(b) && observed(b).  A dropped block counts in removed_outside if it is not inside, otherwise in removed_unobserved.
 *   - Pool order afterwards (what op_volume_download returns), m = blocks kept: a kept block in a slot < m stays where it is.  The dropped slots
 *     below m, h_0 < h_1 < ..., are exactly as many as the kept slots at or above m, t_0 < t_1 < ...; block t_j (its five planes and its key)
 *     moves to slot h_j, in place -- sources and destinations are disjoint.  blocks_moved is that count.
 *   - Slots [m, n) hold default voxels again, as op_volume_clear leaves them, and are handed out as fresh; the block count is m; the hash table
 *     is cleared and re-entered from the m keys (no tombstones).
 *   - Pending op_volume_unpack_sum_begin slots and the raycaster's block summaries are invalidated.  Whether the volume takes the plain or the
 *     lean update is unchanged (a kept block holds what it held, a freed slot the default voxel); foreign data only ever moves to a lower slot.
 *   - The cumulative counters (op_volume_stats, op_volume_deintegrate_stats) count events and do not change.
 *   - An empty volume, or nothing to drop: OP_OK, stats {n, n, 0, 0, 0}, and nothing runs beyond the classification and its count.
 * Runs on the volume's stream and returns when it is done.  Without a device: OP_ERR_NO_DEVICE. */
typedef struct { uint64_t blocks_before, blocks_kept, removed_outside, removed_unobserved, blocks_moved; } op_volume_collect_stats;
int op_volume_collect_garbage(op_volume *v, float min_weight, const int32_t box_lo[3], const int32_t box_hi[3],
                              op_volume_collect_stats *stats /* may be NULL */);
/* What the last op_volume_collect_garbage of this volume did (CubeHandler::CollectStats; no reference counterpart): zeros before the first
 * one and after a refused one.  Does not synchronise. */
int op_volume_collect_last_stats(op_volume *v, op_volume_collect_stats *stats);
/* Counters since create/clear (synchronises): frames integrated, sum over frames of
 * len(cube_id_list), of voxels visited (512 x len) and of voxels that passed the update predicate
 * (Integrator.cpp:63,70,74).  frames, blocks_selected and voxels_visited also count DE-INTEGRATED frames (they are prepared and selected like fused
 * ones); voxels_updated counts integration updates only -- op_volume_deintegrate_stats has the rest. */
int op_volume_stats(op_volume *v, uint64_t *frames, uint64_t *blocks_selected, uint64_t *voxels_visited,
                    uint64_t *voxels_updated);
/* Launch-level counters since create/clear (synchronises; measurement hook, no reference counterpart):
 * Integrator::IntegrateImage runs as ONE kernel launch per batch of up to 32 frames that reads every
 * selected block once and writes every voxel that changed once, so the HBM traffic of a launch is
 * bounded below by 20 B x 512 x blocks_read + 20 B x voxels_written (+ the packed images), whatever
 * the number of frames in the batch.  launches = k_integrate launches that fused something; shader_cycles = their summed
 * durations in SHADER clock cycles (the longest s_memtime span of one of the launch's resident workgroups) --
 * the denominator of the kernel's instruction-issue utilisation, whatever the clock did while it ran. */
int op_volume_stats_launches(op_volume *v, uint64_t *launches, uint64_t *blocks_read, uint64_t *voxels_written,
                             uint64_t *shader_cycles);

/* The volume grows like the reference's std::unordered_map (CubeHandler.h:22): current capacity in blocks, how often the
 * pool has been enlarged since create, and how many batches were launched a second time because a batch had exhausted the
 * pool before the host noticed (results are unaffected; the replays cost time).  Does not synchronise. */
int op_volume_growth_stats(op_volume *v, uint64_t *max_blocks, uint64_t *grows, uint64_t *replayed_batches);
/* Measurement hook (no reference counterpart): with sample_every = k > 0, every k-th launch group
 * (one group = one op_volume_integrate call, or one batch of up to 32 frames of
 * op_volume_integrate_sequence) is bracketed by HIP events on the volume's stream.  profile_read
 * synchronises and returns the summed durations in ms of the three kernels -- [0] frame
 * preparation + ComputeBounding (KA), [1] PrepareCubes (KB), [2] Integrator::IntegrateImage (KC) --
 * over n_launches sampled groups covering n_frames frames. */
int op_volume_profile_enable(op_volume *v, int sample_every);
int op_volume_profile_read(op_volume *v, double ms_sum[3], uint64_t *n_launches, uint64_t *n_frames);

/* CubeHandler::GetCubeMap (CubeHandler.h:347-350): keys n x 3 int32; voxels n x 512 x 5 float in
 * the reference's TSDFVoxel member order {sdf, weight, color[0..2]}, voxel index x + 8y + 64z. */
int op_volume_download(op_volume *v, int32_t *keys_xyz, float *voxels_aos, size_t cap, size_t *n);
/* CubeHandler::SetCubeMap / AddCube + assignment (CubeHandler.h:185-198,351-356). */
int op_volume_upload(op_volume *v, const int32_t *keys_xyz, const float *voxels_aos, size_t n);
/* CubeHandler::Merge(const CubeHandler&) (CubeHandler.h:145-167), both volumes on one device. */
int op_volume_merge(op_volume *dst, op_volume *src);

/* CubeHandler::Transform (nearest = 0, trilinear ReadVoxelInterpolate, CubeHandler.h:242-298,
 * VoxelCube.cpp:6-50) / CubeHandler::TransformNearest (nearest = 1, CubeHandler.h:299-338) on the
 * device: returns a NEW volume on the same device (destroy it with op_volume_destroy).  T_inv may
 * be NULL.  The reference's quirk is kept: TransformNearest's result has the default voxel
 * resolution 0.01 and allocates its blocks with it.  max_blocks = 0 sizes the result automatically. */
int op_volume_transform(op_volume *src, const float T[16], const float *T_inv, int nearest,
                        uint64_t max_blocks, op_volume **out);
int op_volume_resolution(op_volume *v, float *voxel_res);
/* CubeHandler::Coarsen (no reference counterpart): a half-resolution copy of a fused model, on the device.  Voxel centres sit at
 * (index + 0.5) * res (Integration/VoxelCube.h:49-58), so a voxel of twice the size covers exactly a 2 x 2 x 2 group of fine voxels and its centre is
 * their centroid: nothing is resampled or interpolated.  THE DEFINITION of one level:
 *   - The result is a NEW volume on the source's device (destroy it with op_volume_destroy) with the source's camera, truncation, near and far and
 *     voxel_res = 2 * the source's (exact in float32).  It is marked foreign over all of its blocks, as op_volume_transform's result is: its
 *     weights are no integers, and fusion into it takes the general update.  The source is not changed.
 *   - Result block B exists iff at least one of the eight source blocks 2B + {0,1}^3 exists: the id on each axis is the arithmetic shift b >> 1
 *     (source blocks -1, -2, -3 go to -1, -1, -2).  A block whose voxels all come out unobserved is kept (op_volume_collect_garbage drops it).
 *   - Coarse global voxel g has the children f = 2g + (i, j, k), i, j, k in {0, 1}, visited in the order c = i + 2j + 4k ascending.  A child in a
 *     missing block is the default voxel.  A child CONTRIBUTES iff w_c > 0 && w_c >= min_weight -- false for NaN, so whatever sdf lies under a
 *     weight of 0 (999, NaN, inf) never reaches the sums.
 *   - Over the contributing children, in that order, in float32, every product and every sum rounded on its own, starting from 0.0f:
 *       W = W + w_c;  S = S + w_c * s_c;  C_m = C_m + w_c * col_c[m]  (m = 0, 1, 2)
 *   - No child contributes: the default voxel {999, 0, -1, -1, -1}.  Otherwise sdf = S / W, colour[m] = C_m / W (IEEE divisions) and
 *     weight = W * 0.125f -- the mean over all EIGHT cells, exact: a fully observed region keeps its weight, a half-observed coarse cell carries
 *     half of it, and later fusion or op_volume_merge into the result weighs it as what it is.
 * levels in 1..4: that many applications, one after the other, the intermediates released.  max_blocks = 0 sizes the result automatically (it
 * never needs more than the source's block count); a max_blocks that is too small grows and the allocation pass runs again, as
 * op_volume_transform's does.  stats (may be NULL), for the LAST level: source and result blocks, result voxels with 8, with 1..7 and with 0
 * contributing children, and fine voxels of weight > 0 that min_weight kept out.  Refused with OP_ERR_INVALID before any device work: NULL src or
 * out, levels outside 1..4, min_weight negative or NaN. */
typedef struct { uint64_t src_blocks, dst_blocks, voxels_full, voxels_partial, voxels_empty, dropped_min_weight; } op_volume_coarsen_stats;
int op_volume_coarsen(op_volume *src, int levels, float min_weight, uint64_t max_blocks, op_volume **out,
                      op_volume_coarsen_stats *stats /* may be NULL */);
/* CubeHandler::Merge(another, trans) (CubeHandler.h:168-177; example/MergeMultipleSubmaps.cpp:34-42 places its submaps with it) for one source or
 * for n of them, WITHOUT the intermediate volume: the sources are resampled straight into dst's blocks.  op_volume_merge_transformed is
 * op_volume_merge_transformed_many with n = 1.  THE DEFINITION: after the call dst holds, as a map from block id to block, bit for bit what
 *     for k = 0 .. n-1 in order:  op_volume_transform(srcs[k], Ts + 16 k, T_invs ? T_invs + 16 k : NULL, 0, 0, &tmp);  op_volume_merge(dst, tmp);  op_volume_destroy(tmp);
 * leaves (the order of the pool is unspecified, as everywhere).  Spelled out:
 *   - The claim set C_k is AddTransformedCube's (CubeHandler.h:199-225): each of the 512 voxel centres of EVERY block of source k, observed or not,
 *     goes through T_k and the division by w; res / 2 is subtracted and the result floored by res; C_k is the blocks (>> 3) of that voxel and of
 *     its + {0,1}^3 neighbours.  Every block of C_k that dst lacks is created with default voxels (AddCube).
 *   - For every voxel of every block of C_k, and only those, r = ReadVoxelInterpolate (VoxelCube.cpp:6-50) of source k at T_k^-1 * centre, a
 *     missing block reading as default voxels (T_invs NULL: the inverse is formed as op_volume_transform forms it).
 *   - With t the destination voxel as sources 0 .. k-1 left it, TSDFVoxel::operator+= as op_volume_merge has it: t.w == 0 -> t = r (all five
 *     values); else r.w == 0 -> unchanged; else w = t.w + r.w and, if w != 0, sdf and colour = (t.w * t_x + r.w * r_x) / w, every product, sum and
 *     division rounded on its own, otherwise sdf = 999, colour = -1; the weight is w.
 *   - Membership matters: a block that source j brought into the union and that is not in C_k receives nothing from source k, even where source
 *     k's taps would reach observed voxels.
 * stats (may be NULL): sources = n; src_blocks = the sum of the sources' block counts; pairs = sum |C_k|; touched_blocks = |union of the C_k|;
 * created_blocks = how many of those dst lacked; the four voxel counts classify every (block of C_k, voxel) visit by the comparisons above, in
 * that order: copied (t.w == 0), kept (r.w == 0), blended (w != 0; a NaN weight lands here), reset (otherwise) -- they sum to 512 * pairs.
 * Integer counters: exact and repeatable.
 * Refused before any device work, dst untouched: OP_ERR_INVALID for a NULL dst, NULL srcs or Ts with n > 0, a NULL srcs[k], srcs[k] == dst, a
 * source on another device; OP_ERR_MISMATCH for a source whose resolution differs from dst's (op_last_error is the reference's warning line, as
 * op_volume_merge gives it).  Not refused: n == 0 and sources without blocks (OP_OK); the same source twice at two poses.  A block coordinate
 * outside the key range or a table that cannot grow is reported as op_volume_transform reports it; dst may then have gained default blocks and
 * the merges of the groups that had completed (sources are taken in consecutive groups of 64).
 * Like every accessor the call first flushes what is queued on dst and on every source; the kernels run on dst's stream after the sources' work
 * is complete, and dst is final on return.  dst is marked as op_volume_merge marks it (general weights in every block that exists afterwards).
 * Not built: a nearest-neighbour form, un-merging, per-source weights, sources on other devices. */
typedef struct { uint64_t sources, src_blocks, touched_blocks, created_blocks, pairs,
                 voxels_copied, voxels_kept, voxels_blended, voxels_reset; } op_volume_merge_transformed_stats;
int op_volume_merge_transformed(op_volume *dst, op_volume *src, const float T[16], const float *T_inv /* or NULL */,
                                op_volume_merge_transformed_stats *stats /* or NULL */);
int op_volume_merge_transformed_many(op_volume *dst, op_volume *const *srcs, const float *Ts /* n x 16 */,
                                     const float *T_invs /* NULL or n x 16 */, size_t n,
                                     op_volume_merge_transformed_stats *stats /* or NULL */);
/* CubeHandler::GetPointCloud (CubeHandler.cpp:45-69): points and grey colours |sdf|/truncation
 * (n x 3 floats each, host).  *n is the full count; xyz/colors may be NULL to query it. */
int op_volume_point_cloud(op_volume *v, float *xyz, float *colors, size_t cap, size_t *n);
/* CubeHandler::ExtractTriangleMesh (Integration/CubeHandler.cpp:9-44) = GenerateMeshByCube (:70-114) over
 * every block + MarchingCube (MarchingCube.cpp:8-74), on the device.  tri_table (256 x 16 int32, rows of edge
 * ids terminated by -1) and edge_pairs (12 x 2 corner ids) are the CALLER'S tables -- in the reference they are
 * `MCLookTable` / `EdgeIndexPairs` of MarchingCubePredefined.h, which its shim passes straight through (the
 * library neither contains nor assumes a particular table).  Output: three unshared vertices per triangle
 * (triangle k = vertices 3k..3k+2), points and colours as n x 3 floats, exactly as MarchingCube() pushes them;
 * blocks in pool order (the reference's order is its unordered_map's), voxels in the x, y, z loop order.
 * only_block: NULL, or the one CubeID to mesh (= GenerateMeshByCube).  points/colors may be NULL to query
 * *n_vertices. */
int op_volume_extract_mesh(op_volume *v, const int32_t *tri_table, const int32_t *edge_pairs,
                           const int32_t *only_block, float *points, float *colors,
                           size_t cap_vertices, size_t *n_vertices);
/* CubeHandler::WriteToFile / ReadFromFile / ReadFromFileFloat (CubeHandler.h:40-128): the .map
 * float-stream format (VoxelCube.h:128-193).  Blocks are written in pool order. */
int op_volume_write_file(op_volume *v, const char *path);
int op_volume_read_file(op_volume *v, const char *path, int legacy_float_format);

/* TSDF ray casting (north_star "integrate/raycast").  NO reference counterpart: OnePiece has no
 * raycast (its closest relative is the trilinear gather of VoxelCube::ReadVoxelInterpolate,
 * Integration/VoxelCube.cpp:6-50), so the definition is this library's own, restated on the CPU in
 * the test suite's CPU checker and validated against the analytic synthetic scene.  For every pixel (u, v) of
 * `cam` (NULL = the volume's camera) at camera-to-world `pose`:
 *   ray      origin = the pose's translation, direction d = R ((u - cx) / fx, (v - cy) / fy, 1): the parameter t is the z-depth;
 *   lattice  t_k = near + k * res for k = 0, 1, ... while t_k <= far;  p_k = origin + t_k d;
 *   sample   s_k = trilinear sdf over the 8 voxel centres around p_k (g = p * (1 / res) - 0.5, base voxel floor(g)),
 *            valid when all 8 voxels are observed (weight > 0);
 *   hit      the smallest k >= 1 with s_(k-1) valid and > 0 and s_k valid and <= 0:
 *            depth = t_(k-1) + (t_k - t_(k-1)) * s_(k-1) / (s_(k-1) - s_k), in metres (0 = no hit).
 * Optional outputs (W*H*3 floats each, zero where there is no hit): world-frame normals = the normalised central difference
 * of the trilinear sdf at +-res/2 around the hit point, and the trilinear colour there -- each zero unless all its samples are valid.
 * The crossing test is local to a lattice pair, so the result does not depend on the order the volume is traversed in: the kernels
 * march block by block from an LDS tile per block (csrc/raycast.hip) and agree with the CPU restatement bit for bit (depth). */
int op_volume_raycast(op_volume *v, const op_camera *cam, const float pose[16], float *depth_out,
                      float *normals_out, float *colors_out, int mem);
/* Measurement hook: what the LAST op_volume_raycast call on this volume did -- blocks whose sample domain met the view frustum, how many
 * of those earlier views' summaries dropped before loading (OP_VOLUME_OPT_RAYCAST_PRUNE), how many were loaded into LDS and how many of
 * the loaded ones were marched (the others held no zero crossing). */
int op_volume_raycast_stats(op_volume *v, uint64_t *visible_blocks, uint64_t *dropped_unloaded, uint64_t *loaded_blocks, uint64_t *marched_blocks);
/* The same view as an RGB-D FRAME, in the format op_volume_integrate and op_tracker_dense_tracking consume (NO reference counterpart either):
 * op_volume_raycast with colours, then per pixel p
 *   depth_out[p]     = the raycast depth in metres (0 = no hit), W*H floats;
 *   rgb_out[3p + k]  = (uint8_t)min(max(c_k * 255.0f + 0.5f, 0.0f), 255.0f), c_k the raycast colour in stored channel order (product and sum
 *                      rounded separately) -- 0 where there is no hit or the colour is not valid; W*H*3 bytes;
 *   *n_valid         = the number of pixels with depth > 0 (may be NULL).
 * cam == NULL: the volume's camera.  Like every accessor the call sees all frames integrated before it (the queue is flushed first); the kernels run on
 * the volume's stream and the call returns when they are done.  The float colours never leave the device: a packing kernel (four pixels per lane, three
 * dword stores) follows the raycaster's.  An empty volume or a view that sees nothing gives an all-zero frame and OP_OK. */
int op_volume_render_frame(op_volume *v, const op_camera *cam, const float pose[16], uint8_t *rgb_out, float *depth_out, int mem, uint64_t *n_valid);

/* What the model holds at the caller's points: a batch of n queries, one lane each (csrc/volume_sample.hip; NO reference counterpart for the entry --
 * the two definitions are the ones this library already evaluates, made callable).  Every operation below is float32 and rounded separately;
 * nothing is contracted.
 *   query point  with T (16 floats, row-major, host memory): q_r = ((m_r0 x + m_r1 y) + m_r2 z) + m_r3 * 1 per row r, p = q.xyz / q.w -- the order
 *                TransformPoints takes (k_prepare_frames); without T (NULL): p is the given point.
 *   OP_SAMPLE_TRILINEAR (the raycaster's rule, op_volume_raycast above): inv = 1.0f / res, g_a = p_a * inv - 0.5f, base voxel i = floor(g),
 *                f = g - floor(g); taps i + (k & 1, (k >> 1) & 1, (k >> 2) & 1), k = 0..7, of weight (wx * wy) * wz with w_a = f_a where the tap's
 *                bit is set and 1.0f - f_a where it is not; each of the five planes accumulates acc += w * t in tap order from 0.  The sample is
 *                VALID iff all eight taps lie in held blocks and have weight > 0 (a NaN or negative weight is unobserved).  Valid: voxels gets the
 *                five sums {sdf, weight, c0, c1, c2}.  Invalid: the default voxel {999, 0, -1, -1, -1} and OP_SAMPLE_INVALID in the status.
 *   gradient     (OP_SAMPLE_TRILINEAR only) h = 0.5f * res, d_a = s(p + h e_a) - s(p - h e_a): six more trilinear sdf samples, k_rc_shade's
 *                difference, unnormalised (d / res approximates the gradient of the sdf; the raycaster's normal is d divided by
 *                sqrt(d0 d0 + (d1 d1 + d2 d2))).  If any of the six samples is invalid -- a sample whose g is out of range, below, is -- the
 *                gradient is (0, 0, 0) and the status carries OP_SAMPLE_NO_GRADIENT.  The bit is only ever set when gradients are asked for.
 *   OP_SAMPLE_REFERENCE (VoxelCube::ReadVoxelInterpolate, VoxelCube.cpp:6-50, as CubeHandler::Transform evaluates it): half = res / 2,
 *                n = p - half, p0 = floor(n / res), weights (n - (float)p0 * res) / res; the eight taps p0 + (k & 1, (k >> 1) & 1, (k >> 2) & 1)
 *                are fetched (a block that is not held gives the default voxel) and go through the seven lerp stages in the reference's order;
 *                the resulting voxel is written as it comes, and the status carries OP_SAMPLE_INVALID iff its weight is 0.
 *   OP_SAMPLE_OUT_OF_RANGE  a coordinate of g (of n / res in the reference mode) is NaN or of magnitude >= 8388600: decided by an explicit
 *                test before any conversion to int (inside the bound every tap's block id is a legal one).  Implies OP_SAMPLE_INVALID, and
 *                OP_SAMPLE_NO_GRADIENT where gradients are asked for: the default voxel and a zero gradient.
 *   stats        queries = n; valid, gradients, out_of_range = the queries without OP_SAMPLE_INVALID, those with a gradient (0 unless gradients
 *                are asked for), those out of range; sum_abs_sdf / sum_sq_sdf = the sums over valid samples of (double)|s| and (double)s * (double)s,
 *                max_abs_sdf the largest |s| among them (0 without one).  Every workgroup reduces its lanes and writes one row; the host adds the
 *                rows in index order in double: repeatable for a given n, no floating-point atomics.
 * mem says where xyz (n x 3), voxels (n x 5), gradients (n x 3) and status (n bytes) live; T and stats are host memory.  The device buffers need
 * the alignment of their element type only.  Like every accessor the call sees all frames accepted before it (the queue is flushed first); the kernel
 * runs on the volume's stream and the call returns when it is done.  The volume is only read.  n == 0: OP_OK and zero stats.  OP_ERR_INVALID: a
 * NULL volume, a NULL xyz with n > 0, every output (voxels, gradients, status, stats) NULL, a bad mem or mode, gradients with OP_SAMPLE_REFERENCE. */
enum { OP_SAMPLE_TRILINEAR = 0, OP_SAMPLE_REFERENCE = 1 };
enum { OP_SAMPLE_INVALID = 1, OP_SAMPLE_NO_GRADIENT = 2, OP_SAMPLE_OUT_OF_RANGE = 4 }; /* status bits */
typedef struct { uint64_t queries, valid, gradients, out_of_range; double sum_abs_sdf, sum_sq_sdf; float max_abs_sdf; } op_volume_sample_stats;
int op_volume_sample(op_volume *v, const float *xyz, size_t n, int mem, const float *T /* NULL or 16, row-major */, int mode,
                     float *voxels /* n x 5 {sdf, weight, c0, c1, c2} or NULL */, float *gradients /* n x 3 or NULL */,
                     uint8_t *status /* n or NULL */, op_volume_sample_stats *stats /* host, or NULL */);

/* Where a cloud or a depth frame belongs in the model: point-to-plane registration against the FIELD (csrc/volume_register.hip; NO reference
 * counterpart -- the reference registers clouds against clouds by a kd-tree ICP).  At a point the trilinear sdf is the residual and the normalised
 * central difference the plane normal; no target cloud, no normals, no neighbour search.  Every per-point operation below is float32 and rounded
 * separately; nothing is contracted.  For point x_i and a row-major T (16 floats, host memory):
 *   1. p = T x in TransformPoints' order with the divide by q.w: exactly op_volume_sample's "query point".
 *   2. s and the status bits are OP_SAMPLE_TRILINEAR's at p (sdf only); d is its gradient (six more samples at +-h, h = 0.5f * res, unnormalised;
 *      NO_GRADIENT if any of the six is invalid).  OUT_OF_RANGE is decided by the same explicit compare and implies INVALID.
 *   3. l2 = d0 d0 + (d1 d1 + d2 d2) (the raycaster's normal rule).
 *   4. The point is USED iff INVALID is not set, NO_GRADIENT is not set, l2 > 0, and fabsf(s) <= max_distance (false for NaN; max_distance <= 0:
 *      no gate; metres, as the volume stores sdf).
 *   5. n_a = d_a / sqrtf(l2).
 *   6. The row is j = (n0, n1, n2, p1 n2 - p2 n1, p2 n0 - p0 n2, p0 n1 - p1 n0): registration::PointToPlane's row (ICP.cpp:121-136) with the
 *      transformed point in place of the transformed source point and the field's normal in place of the target's.
 *   7. A used point contributes 28 terms, an unused one nothing: sums[0..20] += (double)(j_a j_b) for a <= b, row by row (the product is float32,
 *      then widened, as ICP does); sums[21..26] += (double)(s j_a); sums[27] += (double)s * (double)s.
 *   8. counts = {used, invalid, no_gradient, too_far}: every rejected point is counted once, under the first reason in this order -- invalid:
 *      INVALID is set; no_gradient: NO_GRADIENT is set or l2 > 0 does not hold, on an otherwise valid sample; too_far: gated by max_distance alone.
 *   9. The sums are taken in double.  Every wave reduces its 64 points' 32 slots (the 28 sums, the 4 counts as doubles) per trip of the grid-stride
 *      loop and adds the trips in order; a workgroup adds its four waves in order and writes one row; a second kernel adds the rows (at most 1024)
 *      in index order -- row r, r + 32, ... per row lane, then the 32 row lanes in order.  The order is fixed for a given n: two calls give the
 *      same bits.  No floating-point atomics.
 * op_volume_register_system evaluates this once: sums[28], counts[4] (host; counts may be NULL) and optionally rows: n x 8 floats in `mem`,
 * {j[6], s, 1.0f} for a used point and eight zeros for an unused one.  The sums are the same bits with and without rows.
 * op_volume_register_points runs Gauss-Newton on the host around it:
 *   T = init_T; for each of at most max_iterations iterations: evaluate the system at T; used < min_points -> stop, OP_REGISTER_TOO_FEW_POINTS;
 *   x = op_ldlt_solve6(JTJ, JTr) (JTJ.ldlt().solve(-JTr), JTJ the symmetric 6 x 6 of sums[0..20], JTr = sums[21..26]); a non-finite component of
 *   x -> stop, OP_REGISTER_SINGULAR; T <- op_se3_exp(x) T, the 4 x 4 product in float32, each element ((a0 b0 + a1 b1) + a2 b2) + a3 b3;
 *   iterations counts the updates; last_step = sqrt(sum (double)x_a^2); sum (double)x_a^2 < (double)min_step * (double)min_step -> stop,
 *   OP_REGISTER_CONVERGED; after max_iterations updates: OP_REGISTER_MAX_ITERATIONS.
 *   After the loop the system is evaluated at the returned T: used, invalid, no_gradient, too_far and rmse = sqrt(sums[27] / used) (0 when used
 *   is 0) describe the pose that is returned; first_used / first_rmse are the same at init_T.  max_iterations == 0: T = init_T, one evaluation,
 *   OP_REGISTER_TOO_FEW_POINTS if used < min_points and OP_REGISTER_MAX_ITERATIONS otherwise.
 *   Defaults (params == NULL, op_volume_register_default_params): max_iterations 30 (ICPParameter's), max_distance = the volume's truncation,
 *   min_step 1e-5, min_points 6.  A host cloud is uploaded once; every iteration runs on the volume's stream and brings back one folded row.
 * op_volume_register_depth back-projects the depth image once on the device by op_points_from_depth's definition (PointCloud::LoadFromDepth), keeping
 * every pixel_stride-th pixel in both directions (rows 0, stride, ...; columns likewise) in row-major order and skipping pixels without depth, into
 * a buffer the volume owns, then runs the same loop with init_pose (camera to world) as init_T: its result is, bit for bit, op_volume_register_points
 * on those points.  cam == NULL: the volume's camera.
 * Like every accessor the calls see all frames accepted before them (the queue is flushed first) and only read the volume.  The argument checks
 * run before any device use; OP_ERR_INVALID: a NULL volume, result, sums, T / init_T / init_pose or depth, a NULL xyz with n > 0, a bad mem or
 * depth format, pixel_stride < 1, max_iterations < 0.  n == 0 or an empty volume is no error: zero sums, used = 0, OP_REGISTER_TOO_FEW_POINTS
 * (with min_points > 0), T = init_T. */
typedef struct { int max_iterations; float max_distance, min_step; int min_points; } op_volume_register_params;
typedef struct { float T[16]; int iterations, status; uint64_t used, invalid, no_gradient, too_far, first_used;
                 double rmse, first_rmse, last_step; } op_volume_register_result;
enum { OP_REGISTER_CONVERGED = 0, OP_REGISTER_MAX_ITERATIONS = 1, OP_REGISTER_TOO_FEW_POINTS = 2, OP_REGISTER_SINGULAR = 3 };
int op_volume_register_default_params(op_volume *v, op_volume_register_params *p);
int op_volume_register_system(op_volume *v, const float *xyz, size_t n, int mem, const float T[16], float max_distance,
                              double sums[28], uint64_t counts[4], float *rows /* n x 8 in `mem`, or NULL */);
int op_volume_register_points(op_volume *v, const float *xyz, size_t n, int mem, const float init_T[16],
                              const op_volume_register_params *params /* NULL: defaults */, op_volume_register_result *result);
int op_volume_register_depth(op_volume *v, const op_camera *cam /* NULL: the volume's */, const void *depth, int depth_fmt, int mem,
                             int pixel_stride, const float init_pose[16], const op_volume_register_params *params,
                             op_volume_register_result *result);

/* The colour term of the registration against the field (csrc/volume_register.hip, the COLOR instantiations of k_volume_register; NO reference
 * counterpart).  The sdf says nothing about motion in a surface's own plane; the fused colour does.  Every point carries an observed intensity
 * y_i (a float in the volume's colour units, byte / 255), and the model's intensity at the transformed point, with its central difference as
 * gradient, gives a second residual and a second row.  Every per-point operation below is float32 and rounded separately; nothing is contracted.
 *   1. p, s, d, l2, the USED rule, n, the row j and the counts used / invalid / no_gradient / too_far are exactly op_volume_register_system's.
 *   2. The intensity of a colour triple in stored channel order is I(c) = (0.114f c0 + 0.587f c1) + 0.299f c2.
 *   3. The model intensity is m = I(c), c the three colour sums of the same OP_SAMPLE_TRILINEAR sample at p that gives s: the same taps and
 *      weights, each plane accumulated in tap order from 0.
 *   4. g_a = (I(c(p + h e_a)) - I(c(p - h e_a))) / res, h = 0.5f * res: the colour sums of the six samples already taken for d, one float32
 *      subtraction and one float32 divide.  A tap is valid for colour exactly when it is valid for sdf (weight > 0): a used point always has g.
 *   5. rc = m - y_i.
 *   6. The point is COLOURED iff it is used, y_i is finite and (max_color_residual <= 0 or fabsf(rc) <= max_color_residual).  A point that is
 *      used but not coloured keeps its geometric contribution.
 *   7. jc = color_scale * (g0, g1, g2, p1 g2 - p2 g1, p2 g0 - p0 g2, p0 g1 - p1 g0) and rcs = color_scale * rc: each product one float32
 *      operation, the scaling applied after the cross products.
 *   8. Slot k of sums[0..27] receives per used point the geometric term as in op_volume_register_system and, for a coloured point, the
 *      colour term (double)(jc_a jc_b), (double)(rcs jc_a), (double)rcs * (double)rcs: geometric + colour, added in that order into one double
 *      before the reduction.
 *   9. sums[28] += (double)rc * (double)rc over coloured points (unscaled); sums[29] += (double)s * (double)s over used points (the geometric
 *      part of sums[27] alone).
 *  10. counts = {used, invalid, no_gradient, too_far, colored}.
 *  11. Slots 0..27 and the first four counts are reduced exactly as point 9 of op_volume_register_system states.  The three other quantities
 *      (sums[28], sums[29], colored) are reduced over the wave per trip by a butterfly -- partner lanes 32, 16, 8, 4, 2, 1 apart, in that order --
 *      and the trips added in order; then, like the rest, the four waves in order, one row of 35 per workgroup, and a second kernel adds the rows
 *      (at most 1024) in index order -- row r, r + 16, ... per row lane, then the 16 row lanes in order.  Fixed for a given n: two calls give the
 *      same bits, with and without rows.  No floating-point atomics.
 * color_scale == 0: the colour planes and the intensities are not read (intensity may be NULL), colored and sums[28] are 0, sums[29] is
 * sums[27], and sums[0..27], the first four counts, T and every field of result->base are bit for bit those of the geometric entries above (the
 * geometric kernel runs).  color_scale < 0 or not finite: OP_ERR_INVALID.
 * op_volume_register_color_system evaluates this once: sums[30], counts[5] (host; counts may be NULL) and optionally rows: n x 16 floats in `mem`,
 * {j[6], s, used, jc[6], rcs, colored}: sixteen zeros for an unused point, zeros in the second half for an uncoloured one.
 * op_volume_register_color_points is op_volume_register_points' host loop (op_ldlt_solve6, op_se3_exp, the float32 product, the same stop rules
 * and statuses) around this system.  result->base describes the geometry as before -- base.rmse = sqrt(sums[29] / used) stays the sdf rmse --;
 * colored and rmse_color = sqrt(sums[28] / colored) (0 without a coloured point) describe the returned pose, first_colored / first_rmse_color
 * init_T.  Defaults (params == NULL, op_volume_register_color_default_params): the base as above, color_scale 1 (equal weight, as the dense
 * tracker's LAMBDA_HYBRID_DEPTH 0.5 gives its two terms), max_color_residual 0 (no gate).
 * op_volume_register_rgbd back-projects exactly as op_volume_register_depth does (same pixels, same order) and gives each kept pixel
 * y = I(b0 / 255.0f, b1 / 255.0f, b2 / 255.0f) from its three bytes (W*H*3, stored channel order; an IEEE divide, as the integration rounds
 * them) into a second buffer the volume owns: its result is, bit for bit, op_volume_register_color_points on those points and intensities.
 * `mem` says where depth and rgb live.
 * Refusals as above, decided before any device use; in addition OP_ERR_INVALID for a NULL intensity with n > 0 and color_scale > 0 and for a
 * NULL rgb. */
typedef struct { op_volume_register_params base; float color_scale, max_color_residual; } op_volume_register_color_params;
typedef struct { op_volume_register_result base; uint64_t colored, first_colored; double rmse_color, first_rmse_color; } op_volume_register_color_result;
int op_volume_register_color_default_params(op_volume *v, op_volume_register_color_params *p);
int op_volume_register_color_system(op_volume *v, const float *xyz, const float *intensity /* n, in `mem` */, size_t n, int mem, const float T[16],
                                    float max_distance, float color_scale, float max_color_residual, double sums[30], uint64_t counts[5],
                                    float *rows /* n x 16 in `mem`, or NULL */);
int op_volume_register_color_points(op_volume *v, const float *xyz, const float *intensity, size_t n, int mem, const float init_T[16],
                                    const op_volume_register_color_params *params /* NULL: defaults */, op_volume_register_color_result *result);
int op_volume_register_rgbd(op_volume *v, const op_camera *cam /* NULL: the volume's */, const void *depth, int depth_fmt, const uint8_t *rgb,
                            int mem, int pixel_stride, const float init_pose[16], const op_volume_register_color_params *params,
                            op_volume_register_color_result *result);

/* Consistent linearisations and Huber weights for the registration against the field (csrc/volume_register.hip, the ROBUST instantiations of
 * k_volume_register; NO reference counterpart).  The stored sdf is projective -- measured along the fusing cameras' rays -- so across a surface
 * seen at angle theta it changes by about 1 / cos theta per metre: |grad s| = sqrtf(l2) / res is not 1.  The entries above pair the residual s
 * with the NORMALISED difference n, which understates the Jacobian by |grad s|: every Gauss-Newton step overshoots by that factor (a zig-zag
 * below 2, an alternation between two poses at 2).  Here row and residual agree.  Every per-point operation below is float32 and rounded
 * separately; nothing is contracted.
 *   1. p, s, d, l2, the USED rule (max_distance gates fabsf(s), the stored sdf, in every mode), n = d / sqrtf(l2) and the counts used / invalid /
 *      no_gradient / too_far are exactly op_volume_register_system's steps 1-5 and 8: the USED set does not depend on the options.
 *   2. The linearisation sets the geometric row vector a and the residual r:
 *        OP_REGISTER_LIN_NORMAL   (0)  a = n,                r = s                      (the entries above)
 *        OP_REGISTER_LIN_GRADIENT (1)  a_k = d_k / res,      r = s                      (the Gauss-Newton of sum s^2)
 *        OP_REGISTER_LIN_METRIC   (2)  a = n,                r = s / m, m = sqrtf(l2) / res   (the first-order distance in metres)
 *      and the row is j = (a0, a1, a2, p1 a2 - p2 a1, p2 a0 - p0 a2, p0 a1 - p1 a0).
 *   3. huber > 0: w = 1 when fabsf(r) <= huber, else w = huber / fabsf(r); q = sqrtf(w); j_a <- q j_a, r <- q r, one product each.  The point
 *      counts as downweighted iff w < 1.  huber == 0: no weights (no product).
 *   4. The colour term is op_volume_register_color_system's steps 2-7 (rc, the COLOURED rule, jc, rcs).  huber_color > 0: wc = 1 when
 *      fabsf(rc) <= huber_color (rc unscaled), else huber_color / fabsf(rc); qc = sqrtf(wc); jc_a <- qc jc_a, rcs <- qc rcs.  A coloured point
 *      with wc < 1 counts as color_downweighted.
 *   5. sums[0..27] are formed from the scaled j, r (in s's place), jc, rcs exactly as steps 7 / 8 of the two definitions above form them.
 *   6. sums[28] += (double)rc * (double)rc over coloured points (unscaled, unweighted); sums[29] += (double)s * (double)s over used points (the
 *      stored sdf, unweighted); sums[30] += (double)r * (double)r over used points, r of step 2 (unweighted).
 *   7. counts = {used, invalid, no_gradient, too_far, colored, downweighted, color_downweighted}.
 *   8. Slots 0..27 and the first four counts are reduced exactly as point 9 of op_volume_register_system states.  The six other quantities are
 *      reduced over the wave per trip by the colour entry's butterfly (partner lanes 32, 16, 8, 4, 2, 1 apart, in that order), the trips added
 *      in order, then the four waves in order, one row of 38 per workgroup, and a second kernel adds the rows (at most 1024) in index order --
 *      row r, r + 16, ... per row lane, then the 16 row lanes in order.  Fixed for a given n: two calls give the same bits, with and without
 *      rows.  No floating-point atomics.
 * options == NULL or {0, 0, 0}: sums[0..29], counts[0..4], rows, T and result->color are bit for bit what op_volume_register_color_* give for
 * the same arguments (those kernels run; with color_scale == 0 that is the geometric entries); sums[30] = sums[29], the two new counts 0.
 * huber_color is not looked at when color_scale == 0.
 * op_volume_register_robust_system evaluates this once: sums[31], counts[7] (host; counts may be NULL) and optionally rows: n x 16 floats in
 * `mem` in op_volume_register_color_system's layout {j[6], r, used, jc[6], rcs, colored}, holding what enters the sums (the scaled values).
 * op_volume_register_robust_points is the same host loop (op_ldlt_solve6, op_se3_exp, the float32 product, the same stop rules and statuses)
 * around this system; result->color is filled as op_volume_register_color_points fills it (base.rmse stays sqrt(sums[29] / used), the stored
 * sdf), downweighted / color_downweighted describe the returned pose, first_downweighted init_T, rmse_residual = sqrt(sums[30] / used) and
 * first_rmse_residual likewise (0 when used is 0).
 * op_volume_register_robust_frame back-projects exactly as op_volume_register_rgbd does; rgb == NULL: no intensities, the geometric
 * registration whatever params->color_scale says.  Its result is, bit for bit, op_volume_register_robust_points on those points and
 * intensities.  op_volume_register_robust_default_options gives {OP_REGISTER_LIN_METRIC, 0, 0}.
 * Refusals, decided before any device use: everything the colour entries refuse (a NULL rgb excepted) and OP_ERR_INVALID for a linearisation
 * outside 0..2 and for a negative or non-finite huber or huber_color. */
enum { OP_REGISTER_LIN_NORMAL = 0, OP_REGISTER_LIN_GRADIENT = 1, OP_REGISTER_LIN_METRIC = 2 };
typedef struct { int linearization; float huber, huber_color; } op_volume_register_options;
typedef struct { op_volume_register_color_result color; uint64_t downweighted, color_downweighted, first_downweighted;
                 double rmse_residual, first_rmse_residual; } op_volume_register_robust_result;
int op_volume_register_robust_default_options(op_volume *v, op_volume_register_options *options);
int op_volume_register_robust_system(op_volume *v, const float *xyz, const float *intensity /* n in `mem`, or NULL */, size_t n, int mem,
                                     const float T[16], float max_distance, float color_scale, float max_color_residual,
                                     const op_volume_register_options *options /* NULL: zeros */, double sums[31], uint64_t counts[7],
                                     float *rows /* n x 16 in `mem`, or NULL */);
int op_volume_register_robust_points(op_volume *v, const float *xyz, const float *intensity, size_t n, int mem, const float init_T[16],
                                     const op_volume_register_color_params *params /* NULL: defaults */,
                                     const op_volume_register_options *options /* NULL: zeros */, op_volume_register_robust_result *result);
int op_volume_register_robust_frame(op_volume *v, const op_camera *cam /* NULL: the volume's */, const void *depth, int depth_fmt,
                                    const uint8_t *rgb /* NULL: geometric */, int mem, int pixel_stride, const float init_pose[16],
                                    const op_volume_register_color_params *params, const op_volume_register_options *options,
                                    op_volume_register_robust_result *result);

/* The band voxels of a fused volume as a list (csrc/volume_band.hip; NO reference counterpart -- CubeHandler::GetPointCloud returns the whole
 * truncation band as if it were the surface and drops the sdf).  A fused volume has no surface points: it has a band of voxels, each carrying
 * its own sdf.  Every operation below is float32 and rounded separately; nothing is contracted.
 *   1. A voxel of a held block, with stored sdf s, weight w and local coordinates (x, y, z) in 0..7, is SELECTED iff w > 0, w >= min_weight,
 *      fabsf(s) <= band (false for a NaN s) and x, y and z are all multiples of voxel_stride.
 *   2. band <= 0 means the volume's truncation.  voxel_stride is 1, 2, 4 or 8 (512, 64, 8 or 1 candidates per block).
 *   3. Per selected voxel of block id, per axis with local coordinate l: the centre ((float)id * 8.0f) * res + ((float)l * res + res / 2)
 *      (VoxelCube::GetGlobalPoint, as the integration forms it); the stored sdf; the intensity I(c) = (0.114f c0 + 0.587f c1) + 0.299f c2 of the
 *      stored colour (op_volume_register_color_system's step 2).
 *   4. Order: pool slot ascending (op_volume_download's block order), inside a block voxel index x + 8y + 64z ascending.
 * *n is always the full count.  xyz (n x 3), sdf (n) and intensity (n) live in `mem`, hold `cap` voxels each, and each may be NULL: an output that
 * is NULL is not written, all three NULL query the count.  More than cap selected voxels with an output asked for: OP_ERR_CAPACITY, as
 * op_volume_point_cloud returns it, *n set and nothing written.  Like every accessor the call sees all frames accepted before it (the queue is
 * flushed first) and only reads the volume.  Two passes of one kernel, one workgroup per block: the counts are scanned on the device and only the
 * total comes back.  Defaults (sel == NULL, op_volume_band_default_params): band = 2 * res, min_weight 1, voxel_stride 1.
 * Refusals, decided before any device use: OP_ERR_INVALID for a NULL volume or n, a bad mem, a voxel_stride other than 1, 2, 4, 8, a negative or
 * non-finite min_weight, a NaN band. */
typedef struct { float band, min_weight; int voxel_stride; } op_volume_band_params;
int op_volume_band_default_params(op_volume *src, op_volume_band_params *p);
int op_volume_band_voxels(op_volume *src, const op_volume_band_params *sel /* NULL: defaults */, float *xyz /* n x 3 */, float *sdf /* n */,
                          float *intensity /* n, or NULL */, int mem, size_t cap, size_t *n);

/* A target value per point, and one fused volume against another (csrc/volume_register.hip, the OFFSET instantiations of k_volume_register; NO
 * reference counterpart).  The entries above register points that are assumed to lie on the surface: their residual is the target's sdf alone.
 * Here point i carries the value o_i the field should have at it -- for a band voxel of a second volume its own stored sdf -- and the residual is
 * s_target(T x_i) - o_i.
 * The definition is op_volume_register_robust_system's with ONE change, in its step 2: the residual the linearisation starts from is
 * e = s - o_i, one float32 subtraction, wherever that step says s -- NORMAL r = e, GRADIENT r = e, METRIC r = e / m.  Three things stay on the
 * target's STORED sdf s: the USED rule and its max_distance gate (fabsf(s) <= max_distance), and sums[29] (hence base.rmse).  sums[30],
 * rmse_residual and the huber weight see the new r; the Huber scaling is unchanged (row and residual by the same q).  A non-finite o_i (NaN or
 * +-inf) makes the point unused: it is counted under `invalid`, before any sample is taken.  Reduction, row layout, fold, the host loop, its
 * stop rules and statuses are the robust entries'.
 * offset == NULL IS the robust entry: the existing kernels run and sums, counts, rows and every result field are bit for bit
 * op_volume_register_robust_system's / _points' for the same arguments, all-zero or NULL options included.  With an offset the ROBUST instantiation
 * runs whatever the options are (all-zero options: NORMAL, no weights).  offset is n floats in `mem`.
 * op_volume_register_volume registers the band voxels of `source` against `target`: it selects once (op_volume_band_voxels' rule under `sel`) into
 * buffers of the call -- the source does not change over the iterations -- and runs op_volume_register_offset_points on that list with init_T
 * (source to target): result->robust is, bit for bit, that entry on op_volume_band_voxels' output (xyz, sdf as offset, intensity; the intensity is
 * neither formed nor read with color_scale == 0), result->selected the length of the list.
 *   options == NULL here means {OP_REGISTER_LIN_GRADIENT, 0, 0} -- this default DIFFERS from the point entries' (NULL: zeros): on overlapping
 *   submaps GRADIENT ends at 3-4 mm where METRIC ends at 6-10 mm.  params == NULL: the target's colour defaults
 *   (op_volume_register_color_default_params).  sel == NULL: the source's band defaults.
 *   The volumes may differ in resolution and truncation: the centres use the source's resolution, the samples the target's.  Both must be on one
 *   device (OP_ERR_INVALID otherwise); source == target is allowed.  Both queues are flushed first; the source's stream is synchronised before the
 *   target's stream reads the list.  Both volumes are only read.  An empty selection: zero sums, OP_REGISTER_TOO_FEW_POINTS (min_points > 0),
 *   T = init_T.
 * Refusals, decided before any device use: everything the robust entries refuse; for op_volume_register_volume OP_ERR_INVALID for a NULL target,
 * source, init_T or result, what op_volume_band_voxels refuses of `sel`, and volumes on different devices. */
typedef struct { op_volume_register_robust_result robust; uint64_t selected; } op_volume_register_volume_result;
int op_volume_register_offset_system(op_volume *v, const float *xyz, const float *offset /* n in `mem`, or NULL */,
                                     const float *intensity /* n in `mem`, or NULL */, size_t n, int mem, const float T[16], float max_distance,
                                     float color_scale, float max_color_residual, const op_volume_register_options *options /* NULL: zeros */,
                                     double sums[31], uint64_t counts[7], float *rows /* n x 16 in `mem`, or NULL */);
int op_volume_register_offset_points(op_volume *v, const float *xyz, const float *offset, const float *intensity, size_t n, int mem,
                                     const float init_T[16], const op_volume_register_color_params *params /* NULL: defaults */,
                                     const op_volume_register_options *options /* NULL: zeros */, op_volume_register_robust_result *result);
int op_volume_register_volume(op_volume *target, op_volume *source, const float init_T[16] /* source -> target */,
                              const op_volume_band_params *sel /* NULL: defaults */, const op_volume_register_color_params *params,
                              const op_volume_register_options *options /* NULL: GRADIENT */, op_volume_register_volume_result *result);

/* Many clouds, or many frames, against the fused field in one call (csrc/volume_register.hip, k_volume_register_batch; NO reference counterpart).
 * The entries above place one cloud per call and pay a launch, a fold, a copy and a stream synchronisation per Gauss-Newton iteration; at
 * pixel_stride 4 that latency is most of an iteration.  Here every cloud follows the single entries' loop ON ITS OWN -- its own pose, its own
 * stop rule -- and the clouds that want an evaluation in a round share ONE launch, one fold, one copy and one synchronisation.
 * The definition is the single entries': cloud c is points [starts[c], starts[c + 1]) of xyz (and of offset and intensity), and
 *   results[c], and sums + 31 c / counts + 7 c, are BIT FOR BIT what op_volume_register_offset_points / _offset_system return for cloud c alone
 *   with the same arguments (offset == NULL: the robust entries; all-zero or NULL options: the colour entries; color_scale == 0: the geometric
 *   ones); results[f] of the frames entry is op_volume_register_robust_frame on frame f alone.
 * This holds for every argument combination those entries accept, and does not depend on the order of the clouds, on what else is in the batch
 * or on the rounds in which the other clouds stop: a cloud's workgroups, their trips, its rows and their fold are the single entry's
 * (min(ceil(n_c / 256), 1024) workgroups, rows of 32 / 35 / 38, 32 or 16 row lanes), and the host loop is the same code.  One set of params and
 * options serves the whole batch.
 * A cloud that has stopped, and has had the evaluation at its returned T (skipped when its last evaluation is already current), is never
 * evaluated again.  stats (or NULL): evaluations is the sum over the clouds of the evaluations each one's loop made -- what the single entries would
 * make --, rounds the largest such count of one cloud, launches the kernels of the rounds (a round with no cloud that has a point launches
 * nothing), points starts[n_clouds], for the frames entry the kept pixels.
 * An empty cloud, an all-zero depth image or an empty volume is no error: zero sums, OP_REGISTER_TOO_FEW_POINTS (min_points > 0), T = init_T.
 * n_clouds == 0 (n_frames == 0) returns OP_OK and writes nothing.
 * Frames use op_volume_integrate_sequence's addressing: frame f's depth image is depth + f * depth_stride_bytes, its colour image
 * rgb + f * rgb_stride_bytes, both in `mem`; rgb == NULL registers geometrically.  Every frame's sub-grid is counted by one kernel, scanned once
 * and scattered once; inside a frame the kept pixels are in op_volume_register_depth's row-major order with its arithmetic.  Host images are
 * uploaded once.  The point, intensity, row and output buffers belong to the call (the volume's own registration buffers are not touched).
 * starts, T / init_T / init_poses, sums, counts, results and stats are HOST memory whatever `mem` says.  Like every accessor the call sees all
 * frames accepted before it (the queue is flushed first) and only reads the volume.
 * Refusals, decided before any device use (OP_ERR_INVALID): everything the single entries refuse; a NULL starts, T / init_T / init_poses, results
 * or sums; starts that decrease; a depth or colour stride smaller than an image, a depth stride that is no multiple of a depth value's size; more
 * than 2^32 - 1 sub-grid pixels in all.
 * Not built: params per cloud, the solve on the device, damping, a batch form of op_volume_register_volume. */
typedef struct { uint32_t rounds, launches; uint64_t evaluations, points; } op_volume_register_batch_stats;
/* one evaluation of every cloud at its own T */
int op_volume_register_batch_system(op_volume *v, const float *xyz, const float *offset /* or NULL */, const float *intensity /* or NULL */,
                                    const uint64_t *starts /* n_clouds + 1, host, non-decreasing */, size_t n_clouds, int mem,
                                    const float *T /* n_clouds x 16, host */, float max_distance, float color_scale, float max_color_residual,
                                    const op_volume_register_options *options /* NULL: zeros */, double *sums /* n_clouds x 31 */,
                                    uint64_t *counts /* n_clouds x 7, or NULL */);
/* the loops */
int op_volume_register_batch_points(op_volume *v, const float *xyz, const float *offset, const float *intensity, const uint64_t *starts,
                                    size_t n_clouds, int mem, const float *init_T /* n_clouds x 16 */,
                                    const op_volume_register_color_params *params /* NULL: defaults */,
                                    const op_volume_register_options *options /* NULL: zeros */,
                                    op_volume_register_robust_result *results /* n_clouds */, op_volume_register_batch_stats *stats /* or NULL */);
int op_volume_register_batch_frames(op_volume *v, const op_camera *cam /* NULL: the volume's */, const void *depth, size_t depth_stride_bytes,
                                    int depth_fmt, const uint8_t *rgb /* or NULL: geometric */, size_t rgb_stride_bytes, int mem, int pixel_stride,
                                    const float *init_poses /* n_frames x 16 */, size_t n_frames,
                                    const op_volume_register_color_params *params, const op_volume_register_options *options,
                                    op_volume_register_robust_result *results /* n_frames */, op_volume_register_batch_stats *stats /* or NULL */);

/* Frame-sharded multi-GPU merge (the distributed form of CubeHandler::Merge; DESIGN.md "Multi-GPU").
 * All pointers are DEVICE pointers on the volume's device.
 *   keys_device : copy this volume's block keys (n x 3 int32) into d_keys.
 *   pack_sum    : for the n_union keys (any order) write sum-form voxels
 *                 [w*sdf, w, w*c0, w*c1, w*c2] x 512 per block, SoA planes per block
 *                 (5 x 512 floats), zeros where this volume has no block / w == 0.
 *   unpack_sum  : replace the volume's content by the normalised reduction result. */
int op_volume_keys_device(op_volume *v, int32_t *d_keys, size_t cap, size_t *n);
int op_volume_pack_sum(op_volume *v, const int32_t *d_union_keys, size_t n_union, float *d_out);
int op_volume_unpack_sum(op_volume *v, const int32_t *d_union_keys, size_t n_union,
                         const float *d_sum);
/* The same in slices, so that the reduce of later slices overlaps the normalisation of earlier ones: _begin enters the
 * union keys (growing the pool if needed; the volume's own content is dropped only after validation), _chunk writes
 * union blocks [first, first + count) from a buffer holding just those (count x 5 x 512 floats). */
int op_volume_unpack_sum_begin(op_volume *v, const int32_t *d_union_keys, size_t n_union);
int op_volume_unpack_sum_chunk(op_volume *v, size_t first, size_t count, const float *d_sum_chunk);
/* The whole merge as ONE call for a C/C++ host: CubeHandler::Merge (CubeHandler.h:145-167) across the ranks of a
 * communicator.  nccl_comm is an ncclComm_t whose rank owns the volume's device; call from one host thread (or process) per rank.
 * *n_union (may be NULL) = number of blocks in the merged map.  RCCL is bound at run time (dlopen), so the library does not need it
 * until this entry point is used.  Two algorithms (OP_RUNTIME_OPT_MERGE_ALGORITHM):
 *   OP_MERGE_OWNER_EXCHANGE (default): every block key has an owner rank (a hash of the key); each rank sends the blocks it HOLDS, in sum
 *     form, to their owners (one group of ncclSend / ncclRecv over all pairs), the owners add them up in rank order; then
 *       root >= 0: the owners send their partitions to the root, which normalises the whole map into its volume (the others' volumes
 *                  are left untouched) -- the reference's Merge semantics;
 *       root == -1: no gather -- every rank's volume is REPLACED by its owned, merged partition (a distributed map).
 *   OP_MERGE_DENSE_REDUCE: all-gather of the keys, the same sorted union on every rank, every rank packs the whole union (zeros where it
 *     holds nothing), ONE sliced ncclReduce(float32, sum) to `root` (>= 0), normalisation on the root. */
int op_volume_merge_rccl(op_volume *v, void *nccl_comm, int root, size_t *n_union);
/* The same call, reporting what was moved and how the time was spent (for the N > 1 bench line): ranks / rank of the communicator, blocks
 * in the union, the number of reduce slices (dense) and the bytes this rank put into the reduce / the exchange, host wall time of the
 * preparation, of the transfer pipeline, and of the whole call in milliseconds; the algorithm that ran; the blocks this rank HELD, the blocks
 * it OWNS after the exchange (dense: the union on the root, 0 elsewhere) and the payload bytes it sent / received over the wire (keys included;
 * the few-word agreements excluded).  Owner exchange: sent = (blocks held of OTHER ranks' partitions) x 10 248 B (+ its summed partition
 * when a root gathers) -- on average held x 10 248 x (world - 1) / world. */
typedef struct op_merge_stats {
    int32_t ranks, rank;
    uint64_t union_blocks, reduce_bytes, slices;
    double prepare_ms, transfer_ms, total_ms;
    int32_t algorithm, pad_;
    uint64_t held_blocks, owned_blocks, wire_bytes_sent, wire_bytes_received;
} op_merge_stats;
int op_volume_merge_rccl_stats(op_volume *v, void *nccl_comm, int root, size_t *n_union, op_merge_stats *stats);

/* ---- registration (Registration/ICP.h:13-26, RegistrationResult.h:9-16) ------------------- */
typedef struct {
    float T[16];        /* RegistrationResult::T: Kabsch over the final inlier set (ICP.cpp:221) */
    float last_T[16];   /* accumulated start_T after the last iteration (ICP.cpp:198) */
    double rmse;        /* RegistrationResult::rmse (ICP.cpp:206) */
    uint64_t n_inliers; /* correspondence_set_index.size() */
    int32_t iterations;
} op_icp_result;

/* Builds the device search structure over the target cloud (replaces KDTree::BuildTree,
 * ICP.cpp:172-173).  threshold = ICPParameter::threshold (max correspondence distance). */
int op_icp_create(const float *tgt_xyz, const float *tgt_normals, size_t m, double threshold,
                  int mem, int device, op_icp **out);
int op_icp_destroy(op_icp *icp);
/* How the two sequential float32 accumulations of the reference are reproduced.
 *   OP_ICP_OPT_FINISH: the Kabsch fit that becomes RegistrationResult::T (ICP.cpp:215-221 -> Geometry.cpp:117-133).
 *     OP_ICP_FINISH_REFERENCE (default): the final inlier pairs are compacted on the device in ascending source
 *       index and summed by one host thread in float32, pair by pair, exactly like the reference's two loops --
 *       over 3e5 near-planar pairs their rounding is ~1e-3 of T, i.e. it is part of the reference's result.
 *     OP_ICP_FINISH_FP64: order-free fp64 reduction on the device (closer to the exact Kabsch of the pairs).
 *   OP_ICP_OPT_SUMS: the per-iteration sums (JTJ/JTr, ICP.cpp:121-136; the point-to-point Kabsch, :76-79).
 *     (a new context starts in the process-wide OP_RUNTIME_OPT_ICP_DEFAULT_SUMS mode: OP_ICP_SUMS_REFERENCE_F32 unless the host opted into the fp64 reduction)
 *     OP_ICP_SUMS_FP64: fp64 reduction on the device, no host round trip in the point-to-point loop: ~24 000 iterations/s at 307 200 points.  Equal to the
 *       CPU path WITH DOUBLE SUMS to 1e-7; within 1e-4 of the reference's float32 answer only where that answer is stable (2 of the bench's 4 pairs).
 *     OP_ICP_SUMS_REFERENCE_F32 (default): every iteration's inlier rows are put in inlier order on the device and summed
 *       sequentially in float32 as the reference does -- point-to-plane by one wave on the device (36 + 6 accumulators,
 *       one lane each; 42 numbers come back), point-to-point on one host thread after a transfer of the rows.  The
 *       per-iteration inlier counts and the poses then equal the CPU path's at any size and on every frame pair: where
 *       J^T J sits at JacobiSVD's rank threshold the reference's own float32 rounding decides which way its step goes
 *       (its pose moves by up to 5e-2 when the same sums are taken in double), and only this mode follows it there.
 *       ~600 iterations/s at 307 200 points against ~24 000 with the fp64 reduction.  No middle way exists: tests/tools/icp_sigma_probe.py
 *       (profiles/r06_icp_sigma_probe.txt) shows the smallest eigenvalue of the float32 J^T J is summation noise in EVERY iteration, so no test on the fp64
 *       sums can tell which iterations need the reference's order.
 *   OP_ICP_OPT_TIES: which target a source point is paired with when its nearest candidates are EXACTLY equidistant (duplicated
 *     target points, clouds on a lattice, quantised coordinates; on depth-derived clouds a chance event of ~1e-7 per query).
 *     OP_ICP_TIES_REFERENCE (default): the target the reference's kd-tree (nanoflann 1.3.2 as Geometry/KDTree.h:62-98,171-190 drives it)
 *       returns: the candidate its depth-first traversal meets first.  The search marks the tied queries (one compare and one select per
 *       candidate: +2-4 % on the iteration kernel); their number comes back with the sums and their records through host-mapped memory.
 *       Only for them does the host repeat the search, in the tree nanoflann would build (onepiece_nanotree.hpp; built on the first tie,
 *       ~1 us per query afterwards), and where the partner changes it exchanges the pair's contribution to the sums (same float
 *       expressions as the kernel's) and patches the stored correspondence; floods of ties (lattices) and the reference-order summation
 *       mode take the sums again on the device instead.  Measured at 307 200 points: a depth-derived pair has 0-3 tied queries per
 *       pass (two float32 squared distances equal in every bit); 60 iterations 2.32 ms against 2.25 ms.  op_icp_tie_stats counts them.
 *     OP_ICP_TIES_LOWEST_INDEX: the smallest target index among the equidistant ones -- what the grid search yields without the marking. */
#define OP_ICP_OPT_FINISH 0
#define OP_ICP_OPT_SUMS 1
#define OP_ICP_OPT_TIES 2
#define OP_ICP_FINISH_REFERENCE 0
#define OP_ICP_FINISH_FP64 1
#define OP_ICP_SUMS_FP64 0
#define OP_ICP_SUMS_REFERENCE_F32 1
#define OP_ICP_TIES_LOWEST_INDEX 0
#define OP_ICP_TIES_REFERENCE 1
int op_icp_set_option(op_icp *icp, int option, int value);
int op_icp_set_source(op_icp *icp, const float *src_xyz, size_t n, int mem);
/* OP_ICP_TIES_REFERENCE: queries with exactly equidistant nearest candidates seen since op_icp_create (summed over passes), and how many of
 * them the reference pairs with another target than the smallest index. */
int op_icp_tie_stats(op_icp *icp, uint64_t *tied_queries, uint64_t *changed);
/* The final CountInliers of a registration (ICP.cpp:206) measures the LAST search's correspondences with the pose the last solve produced.  The
 * grid search vouches for a correspondence only within one cell edge (a little over the threshold) of its query -- all that matters while search
 * and count share a pose -- so op_icp_run's final pass singles out the source points whose stored partner lies beyond that under the search's pose
 * AND that the last step moved far enough to bridge the gap, and re-decides exactly those in the tree the reference would search (none in a
 * converged registration; many when the loop is stopped after one or two large steps).  redecided: how many since op_icp_create. */
int op_icp_final_stats(op_icp *icp, uint64_t *redecided);
/* One loop body of ICP.cpp:177-199 without the solve: transform by T, 1-NN, CountInliers and the
 * normal-equation sums.  mode PLANE: sums[0..35] = JTJ (row-major 6x6), sums[36..41] = JTr.
 * mode POINT: sums[0..2] = sum s', [3..5] = sum t, [6..14] = sum s' t^T (row-major), s' = T*s. */
int op_icp_iterate(op_icp *icp, const float T[16], int mode, double sums[42], uint64_t *n_inliers,
                   double *sum_sq_err);
/* registration::PointToPlane / PointToPoint end to end (ICP.cpp:146-224 / :31-107).
 * pairs (cap x 2 int32: source id, target id, ascending source id), per_iter_inliers (max_iter)
 * and per_iter_T (max_iter x 16) may be NULL. */
int op_icp_run(op_icp *icp, int mode, const float init_T[16], int max_iteration,
               op_icp_result *result, int32_t *pairs, size_t pairs_cap, int32_t *per_iter_inliers,
               float *per_iter_T);
/* The same run split in two, so that several contexts work on independent frame pairs at once -- ICP shards only as REPLICAS,
 * and one 307 200-point problem cannot fill the chip (28 k iterations/s = 4 % of the HBM rate its 11 MB would allow).  The loop needs
 * the host after every iteration (the 6x6 solve), so an enqueued run proceeds on a host thread of the context's own; `result` and `pairs`
 * (may be NULL) must stay valid until op_icp_wait, which returns the run's status.  One run may be outstanding per context; results are
 * those of op_icp_run (each context is independent of the others). */
int op_icp_run_enqueue(op_icp *icp, int mode, const float init_T[16], int max_iteration, op_icp_result *result, int32_t *pairs, size_t pairs_cap);
int op_icp_wait(op_icp *icp);
/* K registrations on K contexts from ONE host thread (ICP does not shard -- replicas only).  Contexts in the fp64-reduction mode are pipelined by the
 * caller's thread: every context has one iteration in flight, the thread goes round waiting for a context's sums (host-mapped memory), solving, enqueueing its next
 * iteration; the finishes run side by side on helper threads.  Contexts in the reference-order mode get a submitter thread each (they synchronise every iteration).
 * init_T: K x 16 floats, or NULL for the identity everywhere; results: K entries; every context's result equals what op_icp_run gives it alone. */
int op_icp_run_many(op_icp *const *icps, int k, int mode, const float *init_T, int max_iteration, op_icp_result *results);

/* Convenience: create + set_source + run + destroy with host buffers. */
int op_icp_register(int mode, const float *src_xyz, size_t n, const float *tgt_xyz,
                    const float *tgt_normals, size_t m, const float init_T[16], int max_iteration,
                    double threshold, int device, op_icp_result *result, int32_t *pairs,
                    size_t pairs_cap);
/* registration::EstimateRigidTransformationPointToPlane (ICP.h:24-26, ICP.cpp:108-144): one Gauss-Newton
 * step over caller-supplied inliers (n x 2 int32: source id, target id); source = the ALREADY transformed
 * points, as the reference's loop passes them.  Sums on the device (fp64), JacobiSVD-semantics solve +
 * SE3 exp on the host. */
int op_estimate_rigid_point_to_plane(const float *source_xyz, size_t n_source, const float *target_xyz,
                                     const float *target_normals, size_t n_target,
                                     const int32_t *inliers, size_t n_inliers, int mem, int device,
                                     float T[16]);
/* The same with the accumulation chosen: sums = OP_ICP_SUMS_FP64 (what the plain entry does) or
 * OP_ICP_SUMS_REFERENCE_F32 (JTJ/JTr summed sequentially in float32 on one host thread, ICP.cpp:121-136). */
int op_estimate_rigid_point_to_plane_ex(const float *source_xyz, size_t n_source, const float *target_xyz,
                                        const float *target_normals, size_t n_target,
                                        const int32_t *inliers, size_t n_inliers, int mem, int device,
                                        int sums, float T[16]);
/* geometry::EstimateRigidTransformation (Geometry/Geometry.cpp:107-151): Kabsch fit of a correspondence set
 * given as n x 6 floats (source xyz, target xyz).  The plain entry sums as the reference does (sequential
 * float32 in pair order, OP_ICP_FINISH_REFERENCE); _ex selects OP_ICP_FINISH_FP64 (order-free device reduction). */
int op_estimate_rigid_transformation(const float *pairs_xyz6, size_t n_pairs, int mem, int device,
                                     float T[16]);
int op_estimate_rigid_transformation_ex(const float *pairs_xyz6, size_t n_pairs, int mem, int device,
                                        int finish, float T[16]);
/* tool::ConvertDepthTo32F + tool::BilateralFilter (Tool/ImageProcessing.cpp:68-91, 64-67; header default
 * range = 7, Tool/ImageProcessing.h:19), the depth preprocessing every fusion driver runs right before
 * IntegrateImage (example/ImageSequenceIntegration.cpp:36-38, DenseFusion/DenseFusion.cpp:92-94,
 * ImageIntegration.cpp:24-27): cv::bilateralFilter(src, dst, d, sigma_color = 0.03, sigma_space = 4.5) on
 * n_images row-major width x height depth images (OP_DEPTH_U16 input is first divided by depth_scale).
 * PARITY NOTE: OpenCV is not vendored by the reference; this is cv::bilateralFilter's documented CV_32FC1
 * definition, unpinned:  radius = d / 2 (d <= 0: round(1.5 sigma_space); at least 1), sigma <= 0 -> 1,
 *     out(p) = sum_q w(q) src(q) / sum_q w(q),  q = p + (i, j) with i*i + j*j <= radius^2, BORDER_REFLECT_101,
 *     w(q) = exp(-(i*i + j*j) / (2 sigma_space^2)) * exp(-(src(q) - src(p))^2 / (2 sigma_color^2)),
 * in float32, taps summed row by row.  (OpenCV evaluates the second factor through a 4096-bin linearly
 * interpolated table over the image's value range; this evaluates it directly.)
 * stream: NULL -> the call runs on the library's stream and returns when `out` is final; a hipStream_t
 * (OP_MEM_DEVICE only) -> only enqueued on that stream, e.g. op_volume_stream() so that the filtered depth
 * feeds op_volume_integrate without a host synchronisation. */
int op_bilateral_filter_depth(const void *depth, int depth_format, float depth_scale, int width, int height,
                              int n_images, int d, float sigma_color, float sigma_space, int mem, int device,
                              void *stream, float *out);

/* PointCloud::LoadFromDepth (Geometry/PointCloud.cpp:72-100) on the device: xyz_out (mem) gets the
 * compacted row-major-ordered points; *n the count. */
int op_points_from_depth(const op_camera *cam, const void *depth, int depth_fmt, int mem, int device,
                         float *xyz_out, size_t *n);

/* PointCloud::LoadFromRGBD (Geometry/PointCloud.cpp:17-48): the same compaction plus colours =
 * (b0,b1,b2)/255 in stored channel order (n x 3 floats). */
int op_points_from_rgbd(const op_camera *cam, const void *depth, int depth_fmt, const uint8_t *rgb,
                        int mem, int device, float *xyz_out, float *colors_out, size_t *n);

/* PointCloud::EstimateNormals(radius, knn) (Geometry/PointCloud.cpp:102-144) on the device: exact
 * knn nearest neighbours (knn <= 32), the prefix whose SQUARED distance is <= radius (the
 * reference's KnnRadiusSearch, KDTree.h:230-255), PCA plane fit (geometry::FitPlane,
 * Geometry.cpp:172-218).  normals_out: n x 3 floats in `mem`; the sign of each normal is
 * undetermined (as in the reference, whose disambiguation is #if 0'd out); < 3 neighbours -> 0. */
int op_estimate_normals(const float *xyz, size_t n, float radius, int knn, int mem, int device,
                        float *normals_out);

/* ---- batched exact nearest-neighbour queries and label transfer (example/GetLabelUsingKDTree.cpp) ----
 * What example/GetLabelUsingKDTree.cpp does per vertex -- KDTree<>::KnnSearch(q, indices, dists, 1) (Geometry/KDTree.h:147-196), then
 * `dists[0] < max_distance`, then labels[i] = reference_labels[indices[0]] -- for a whole batch of queries against one target cloud.  Every
 * index is the one nanoflann 1.3.2 reports (queries whose runner-up is as near as the best, or within 2^-15 of it relatively -- the reach of
 * the rounding in the tree's pruning bound -- are re-decided on the host in the tree that library would build), every distance is its
 * L2_Simple_Adaptor in float32 (d = 0; d += dx*dx; d += dy*dy; d += dz*dz).  max_sq_dist is compared with the SQUARED distance, strictly,
 * as the example does; INFINITY = no cutoff.  A query with no target below the cutoff gets index -1, distance +infinity and the default label.
 * OP_ERR_INVALID for a non-finite coordinate (target or query), a target whose grid cannot be sized, and 2^28 or more targets or queries
 * (the packed (distance, index) key, 32-bit record offsets).  n = 0 succeeds and writes nothing; m = 0 answers -1 / default_label
 * everywhere.  Host or device buffers (mem); synchronous; an index is used by one thread at a time. */
/* replaces kdtree.BuildTree(reference_mesh.points) of example/GetLabelUsingKDTree.cpp:45-46 (Geometry/KDTree.h:147-196 searches it): built once, queried many times */
int op_nn_index_create(const float *tgt_xyz, size_t m, int mem, int device, op_nn_index **index);
/* the end of that kdtree's life (example/GetLabelUsingKDTree.cpp:45, rebuilt at :96 and :119; Geometry/KDTree.h:147-196): releases the index; NULL is accepted */
int op_nn_index_destroy(op_nn_index *index);
/* replaces the loop of KnnSearch(q, indices, dists, 1) + cutoff of example/GetLabelUsingKDTree.cpp:49-56 (Geometry/KDTree.h:147-196): out_idx n x int32, out_sq_dist n floats */
int op_nn_index_query(op_nn_index *index, const float *query_xyz, size_t n, int mem, float max_sq_dist, int32_t *out_idx, float *out_sq_dist /* may be NULL */);
/* replaces the whole loop of example/GetLabelUsingKDTree.cpp:49-60 / 98-108 / 121-132 (Geometry/KDTree.h:147-196 per query): out_labels[i] = out_idx[i] >= 0 ?
 * tgt_labels[out_idx[i]] : default_label; labels are int32 (the example's unsigned short semantic labels are widened by the caller) */
int op_nn_index_transfer_labels(op_nn_index *index, const int32_t *tgt_labels /* m x int32 */, const float *query_xyz, size_t n, int mem, float max_sq_dist,
                                int32_t default_label, int32_t *out_labels, int32_t *out_idx /* may be NULL */);
/* since the index was created: queries answered, and how many of them the host re-decided in the tree because their runner-up was exactly as
 * near as the best (tied) or within the bound chain's rounding of it (doubtful) -- what example/GetLabelUsingKDTree.cpp's KnnSearch (Geometry/KDTree.h:147-196) decides by traversal */
int op_nn_index_stats(op_nn_index *index, uint64_t *queries, uint64_t *tied, uint64_t *doubtful);
/* one pass of example/GetLabelUsingKDTree.cpp (BuildTree + the loop, Geometry/KDTree.h:147-196) in one call: create, transfer, destroy */
int op_transfer_labels(const float *tgt_xyz, const int32_t *tgt_labels, size_t m, const float *query_xyz, size_t n, int mem, int device, float max_sq_dist,
                       int32_t default_label, int32_t *out_labels, int32_t *out_idx /* may be NULL */);

/* ---- voxel-grid down-sampling (Geometry/PointCloud.h, example/DenseFusion/DenseSlam.h) ----
 * op_point_cloud_downsample == geometry::PointCloud::DownSample (Geometry/PointCloud.cpp:145-189), bit-identical to the host loop of
 *   host/one_piece/src/PointCloud.cpp: the cell of a point is (int)floorf(p / grid_len) per axis (IEEE float divide); output point j belongs to
 *   the j-th distinct cell in order of first appearance in the input; each of its values is ((v_i0 + v_i1) + v_i2) + ... in float32 over the
 *   cell's members i0 < i1 < ... in input order, divided once by (float)count.  colors / normals are carried (same rule) when given.  Every
 *   array follows `mem`; the outputs need room for n points; *n_out (always host memory) is the number of cells.
 *   Refused, with nothing written: grid_len not positive and finite, a non-finite coordinate or a cell outside the int range (the host's cast
 *   is undefined there) -> OP_ERR_INVALID; a cloud more than 2^21 cells wide on an axis (the three axes share one 63-bit sort key) ->
 *   OP_ERR_CAPACITY.  n == 0 is OP_OK with *n_out = 0.
 *   The sum of a cell is one chain of adds in member order, by definition: a cloud that falls into ONE cell takes n dependent adds.
 * op_points_from_rgbd_downsampled == the body of Submap::GenerateSubmapModel's loop (DenseSlam.h:24-28) for one frame without leaving the device:
 *   points and colours exactly as op_points_from_rgbd produces them (compacted, row-major), then geometry::TransformPoint of the class surface
 *   (host/one_piece/src/Geometry.cpp:19-23: ((T(r,0) x + T(r,1) y) + T(r,2) z) + T(r,3) 1.0f per row, the first three divided by the fourth), then the down-sampling above.  Colours are
 *   not transformed.  depth, rgb and the outputs (room for width * height points each) follow `mem`; T and *n_out are always host memory. */
int op_point_cloud_downsample(const float *xyz, const float *colors /* NULL or n x 3 */, const float *normals /* NULL or n x 3 */,
                              size_t n, float grid_len, int mem, int device,
                              float *xyz_out, float *colors_out, float *normals_out /* each n x 3 capacity, same mem */,
                              size_t *n_out /* always host */);
int op_points_from_rgbd_downsampled(const op_camera *cam, const void *depth, int depth_fmt, const uint8_t *rgb,
                                    const float *T /* 16 row-major, NULL = no transform */, float grid_len,
                                    int mem, int device, float *xyz_out, float *colors_out /* width*height x 3 capacity */, size_t *n_out);

/* ---- clustering mesh simplification (Geometry/TriangleMesh.h, the tail of the fusion drivers) ----
 * op_mesh_cluster_simplify == geometry::TriangleMesh::ClusteringSimplify (Geometry/MeshSimplification.cpp:579-657), bit-identical to the host loop of
 *   host/one_piece/src/TriangleMesh.cpp (ClusteringSimplify + Compact).  Corner c = 3 t + k of triangle t is vertex v = triangles[3 t + k] at points[v]; its
 *   cell is (int)floorf(p / grid_len) per axis (IEEE float divide); cells exist in order of first appearance over the corners.  A cell's representative is the
 *   vertex of its first corner (also when that corner's triangle is dropped); its position is (float)(sum / (double)count) per axis, sum the double chain
 *   ((0.0 + p_c0) + p_c1) + ... over ALL its corners in corner order (a vertex shared by m corners counts m times, corners of dropped triangles count).
 *   Triangle t becomes its three representatives and is dropped when two are equal.  Output vertices are numbered by first appearance among the corners of
 *   the kept triangles, in order; cells no kept triangle refers to and vertices nothing refers to vanish; colours and normals of an output vertex are its
 *   representative's own (copied, not averaged).
 *   Every array follows `mem`; points_out / colors_out / normals_out need room for min(nv, 3 nt) rows, triangles_out for nt; *nv_out and *nt_out are
 *   always host memory.  nt == 0 is OP_OK with both 0.
 *   Refused, with nothing written: grid_len not positive and finite, a triangle index >= nv, a non-finite coordinate at a referenced vertex or a cell
 *   outside the int range -> OP_ERR_INVALID; a mesh more than 2^21 cells wide on an axis (the three axes share one 63-bit sort key), or 3 nt beyond
 *   32-bit corner indices -> OP_ERR_CAPACITY.
 *   The sum of a cell is one chain of double adds in corner order, by definition: a mesh that falls into ONE cell takes 3 nt dependent adds.
 * op_volume_extract_mesh_clustered == CubeHandler::ExtractTriangleMesh (Integration/CubeHandler.cpp:9-44) followed by ClusteringSimplify(grid_len)
 *   (MeshSimplification.cpp:579-657) without the triangle soup leaving the device: the count and emit passes of op_volume_extract_mesh into device
 *   buffers, the simplification above on that soup (triangles[c] = c, colours carried), only the simplified mesh copied out (host memory).
 *   Sizes: a call with points, colors or triangles NULL returns UPPER BOUNDS in *n_vertices / *n_triangles -- the soup's own vertex and triangle counts
 *   (the exact sizes would take the whole pipeline) -- and writes nothing; the filling call returns the TRUE sizes.  Buffers smaller than the true
 *   sizes -> OP_ERR_CAPACITY with nothing written and the true sizes in the counts.  Other refusals as above (counts 0). */
int op_mesh_cluster_simplify(const float *points, const float *colors /* NULL or nv x 3 */, const float *normals /* NULL or nv x 3 */, size_t nv,
                             const uint32_t *triangles /* nt x 3 */, size_t nt, float grid_len, int mem, int device,
                             float *points_out, float *colors_out, float *normals_out /* each min(nv, 3 nt) x 3 capacity, same mem */,
                             uint32_t *triangles_out /* nt x 3 capacity, same mem */, size_t *nv_out, size_t *nt_out /* always host */);
int op_volume_extract_mesh_clustered(op_volume *v, const int32_t *tri_table, const int32_t *edge_pairs, const int32_t *only_block, float grid_len,
                                     float *points, float *colors, size_t cap_vertices, uint32_t *triangles, size_t cap_triangles,
                                     size_t *n_vertices, size_t *n_triangles);

/* ---- vertex normals and small-component pruning of a mesh (Geometry/TriangleMesh.h, the rest of the fusion drivers' tail) ----
 * op_mesh_compute_normals == geometry::TriangleMesh::ComputeNormals (Geometry/TriangleMesh.cpp; example/ImageIntegration.cpp:45, MCGenerateMesh.cpp:24,
 *   MergeMultipleSubmaps.cpp:46), bit-identical to the host loop of host/one_piece/src/TriangleMesh.cpp.  All in float32 without FMA: the face normal of
 *   triangle t is (p1 - p0) x (p2 - p0), every product rounded before the subtraction, divided by len = sqrtf((n0 n0 + n1 n1) + n2 n2) when len > 0
 *   (IEEE sqrt and divide).  normals[v] is ((+0 + n_c0) + n_c1) + ... over the corners c = 3 t + k that refer to v, in corner order (a vertex used
 *   twice by one triangle receives its normal twice), then normalised the same way.  A vertex nothing refers to keeps (0, 0, 0); a -0 component of
 *   a face normal becomes +0 in the vertex.  Every array follows `mem`; normals_out holds nv rows and is overwritten.  nt == 0 is OP_OK: nv rows of zeros.
 *   Refused, with nothing written: a triangle index >= nv, a non-finite coordinate at a referenced vertex (elsewhere it is not read) -> OP_ERR_INVALID;
 *   3 nt beyond 32-bit corner indices -> OP_ERR_CAPACITY.
 *   The sum of a vertex is one chain of float32 adds in corner order, by definition: a vertex of valence m takes m dependent adds.
 * op_mesh_prune == geometry::TriangleMesh::Prune (Geometry/TriangleMesh.cpp; example/PruneMesh.cpp:15), the result of the host loop of
 *   host/one_piece/src/TriangleMesh.cpp (Prune + Compact).  Two vertices are connected when a triangle contains both; the size of a component is its
 *   number of referenced vertices; a triangle is kept exactly when its component's size is > min_points.  Output vertices are numbered by first appearance
 *   among the corners of the kept triangles; points, colours and normals are carried; vertices nothing kept refers to vanish.  *pruned_out is the
 *   number of referenced vertices in dropped components (what Prune prints).  Every array follows `mem`; points_out / colors_out / normals_out need room
 *   for min(nv, 3 nt) rows, triangles_out for nt; the three counts are always host memory.  nt == 0 is OP_OK with all three 0.
 *   Refused, with nothing written: a triangle index >= nv -> OP_ERR_INVALID; 3 nt beyond 32-bit corner indices -> OP_ERR_CAPACITY.
 * op_volume_extract_mesh_processed == CubeHandler::ExtractTriangleMesh (Integration/CubeHandler.cpp:9-44), then ClusteringSimplify(grid_len)
 *   (MeshSimplification.cpp:579-657) if grid_len > 0, then Prune(min_points) if min_points > 0, then ComputeNormals if `normals` is given -- the tail of
 *   example/MergeMultipleSubmaps.cpp:45-46 and ImageIntegration.cpp:45 -- all in device buffers; only the finished mesh is copied out (host memory).
 *   With grid_len == 0 the mesh is the soup, triangles[c] = c.  Sizes as for op_volume_extract_mesh_clustered: a call with points, colors or triangles
 *   NULL returns UPPER BOUNDS (the soup's sizes) and writes nothing; the filling call returns the TRUE sizes; buffers smaller than those ->
 *   OP_ERR_CAPACITY with nothing written and the true sizes in the counts.  grid_len negative or not finite -> OP_ERR_INVALID; the refusals of the
 *   stages pass through (counts 0). */
int op_mesh_compute_normals(const float *points, size_t nv, const uint32_t *triangles /* nt x 3 */, size_t nt, int mem, int device,
                            float *normals_out /* nv x 3, same mem */);
int op_mesh_prune(const float *points, const float *colors /* NULL or nv x 3 */, const float *normals /* NULL or nv x 3 */, size_t nv,
                  const uint32_t *triangles /* nt x 3 */, size_t nt, size_t min_points, int mem, int device,
                  float *points_out, float *colors_out, float *normals_out /* each min(nv, 3 nt) x 3 capacity, same mem */,
                  uint32_t *triangles_out /* nt x 3 capacity, same mem */, size_t *nv_out, size_t *nt_out, size_t *pruned_out /* always host */);
int op_volume_extract_mesh_processed(op_volume *v, const int32_t *tri_table, const int32_t *edge_pairs, const int32_t *only_block,
                                     float grid_len /* 0: no clustering */, size_t min_points /* 0: no pruning */,
                                     float *points, float *colors, float *normals /* NULL: no normals */, size_t cap_vertices,
                                     uint32_t *triangles, size_t cap_triangles, size_t *n_vertices, size_t *n_triangles);

/* ---- global registration (Registration/3DFeature.h, GlobalRegistration.h, Geometry/Ransac.h) ----
 * The device counterparts of the three dense loops of submap registration; each restates the host loop of host/one_piece/src operation by
 * operation in float32 (GlobalRegistration.cpp, RansacRigid.cpp there; the reference symbols are named per entry).  The random parts -- the
 * match pruning and RANSAC's draws -- and the 8-point fits stay on the host.
 *
 * op_fpfh_compute == registration::ComputeFPFHFeature (3DFeature.cpp:86-130, with ComputePairDescriptor :9-27 and ComputeSPFH :30-84).
 *   Neighbours: the points of the 27 cells of edge sqrtf(radius) around a point whose SQUARED distance is below `radius` (the reference hands
 *   the radius to nanoflann's L2 adaptor unsquared), ordered by (squared distance, index), the first knn (1 .. 256) of them; the point itself
 *   comes first (an exact duplicate with a lower index precedes it, as on the host).  neighbours_out rows are padded with -1.  SPFH and FPFH
 *   are bit-identical to the host path except the first angle's bins: its atan2 is evaluated in double and rounded to float once, where the
 *   host calls its libm's atan2f, so a pair within an ulp of a bin boundary may fall into the adjacent bin.  A third whose neighbour sum is 0
 *   stays 0.  The cells are formed and sorted on the host (O(n log n)); with OP_MEM_DEVICE the points are read back once for that.
 * op_feature_match == registration::FeatureMatching3D (GlobalRegistration.cpp:28-78), exhaustive: nearest_out[i] = the target row with the
 *   smallest squared distance (summed over the 33 bins in order), the lowest index on ties; -1 when nt == 0.
 * op_ransac_count_inliers == the scoring loop of GRANSAC::Estimate (GRANSAC.hpp:96-118) with TransformationModel::ComputeDistanceMeasure
 *   (TransformationModel.hpp:37-49): counts_out[h] = the correspondences i with |R_h src_i + t_h - tgt_i| < threshold (float, strictly below).
 * op_ransac_inlier_ids == the inlier gathering of geometry::EstimateRigidTransformationRANSAC (Ransac.cpp:32-39) for one transform: the
 *   indices counted above, ascending; ids_out holds up to n, *n_out (always host memory) the count.
 * `mem` covers every array argument; counts and ids follow it too. */
int op_fpfh_compute(const float *xyz, const float *normals, size_t n, int knn, float radius, int mem, int device,
                    float *fpfh_out /* n x 33 */, int *neighbours_out /* NULL or n x knn, -1 padded, self first */,
                    float *spfh_out /* NULL or n x 33 */);
int op_feature_match(const float *src /* ns x 33 */, size_t ns, const float *tgt /* nt x 33 */, size_t nt,
                     int mem, int device, int *nearest_out /* ns; -1 when nt == 0 */);
int op_ransac_count_inliers(const float *src_xyz, const float *tgt_xyz, size_t n, const float *T /* H x 12, row-major 3x4 */,
                            size_t H, float threshold, int mem, int device, unsigned *counts_out /* H */);
int op_ransac_inlier_ids(const float *src_xyz, const float *tgt_xyz, size_t n, const float *T /* 12 */, float threshold,
                         int mem, int device, int *ids_out, size_t *n_out);

/* ---- dense RGB-D tracker (Odometry/Odometry.h:38-175) ------------------------
 * Boundary = the inputs of Odometry::MultiScaleComputing (Odometry.cpp:621-636): image pyramids
 * already built (cv::pyrDown / cv::Sobel / cv::GaussianBlur stay where they are in the reference,
 * Odometry.cpp:436-449,609-620).  All images are dense row-major float32 of width x height
 * (CV_32FC1); invalid depth is NaN (ConvertDepthTo32FNaN, DenseOdometryFunction.cpp:28-56); the
 * *_dx/_dy images are the raw cv::Sobel outputs (SOBEL_SCALE is applied inside).  The image-XYZ
 * pyramids of the reference are recomputed from the depth pyramids with TransformToMatXYZ's own
 * arithmetic (Geometry.cpp:72-106).  levels[0] is full resolution (camera_pyramid[0]). */
typedef struct {
    int32_t width, height;          /* camera_pyramid[l].GetWidth()/GetHeight() */
    float fx, fy, cx, cy;           /* Camera.h:38-42: halved per level */
    const float *source_color, *source_depth, *target_color, *target_depth;
    const float *target_color_dx, *target_color_dy, *target_depth_dx, *target_depth_dy;
} op_track_level;

typedef struct {
    float T[16];                 /* DenseTrackingResult::T (Odometry.h:32) */
    double rmse;                 /* ComputeReprojectionError3D(correspondence_set, T), Odometry.cpp:606 */
    uint64_t n_correspondences;  /* pixel_correspondence_set.size(): pairs of the LAST executed iteration */
    int32_t tracking_success;    /* ratio >= MIN_INLIER_RATIO_DENSE over the FULL-resolution pixel count */
    int32_t iterations;          /* iterations executed (early-out at ratio > MAX_INLIER_RATIO_DENSE) */
} op_track_result;

int op_tracker_create(int device, op_tracker **out);
int op_tracker_destroy(op_tracker *t);
/* OP_TRACK_OPT_SUMS: how an iteration's normal equations are summed (DenseOdometryFunction.cpp:297-381).
 *   (a new tracker starts in the process-wide OP_RUNTIME_OPT_TRACKER_DEFAULT_SUMS mode: OP_TRACK_SUMS_REFERENCE_F32 unless the host opted into the fp64 reduction)
 *   OP_TRACK_SUMS_FP64: fp64 reduction on the device, the whole coarse-to-fine loop without a host round trip.
 *   OP_TRACK_SUMS_REFERENCE_F32: the reference's own sums -- association, acceptance and Jacobian rows come from the same kernels, and every
 *     iteration's rows are summed in raster order in float32 exactly like the reference's loop: on the device, by one wave that owns the
 *     36 + 6 accumulators and walks the compacted rows (k_seq_sums; the other waves of its workgroup prepare the products), then the 42
 *     sums go to the host for the LDL^T solve / exp / pose update the reference-order mode shares with the CPU path.  A run follows the
 *     CPU path step for step: identical correspondence counts at every iteration, poses to 1e-6 (north_star's bar is 1e-4), at ~9 ms
 *     per 640x480 track.  NormalizeIntensity's two means likewise.
 *   OP_TRACK_SUMS_REFERENCE_F32_HOST: the same sums taken on ONE host thread after a transfer of all rows (17 MB per full-resolution
 *     iteration; ~30 tracks/s) -- the cross-check of the device sums: both give the same floats. */
#define OP_TRACK_OPT_SUMS 0
#define OP_TRACK_SUMS_FP64 0
#define OP_TRACK_SUMS_REFERENCE_F32 1
#define OP_TRACK_SUMS_REFERENCE_F32_HOST 2
int op_tracker_set_option(op_tracker *t, int option, int value);
/* Odometry::MultiScaleComputing + the result assembly of DenseTracking (Odometry.cpp:621-687,
 * :600-607).  iters_per_level[l] = iter_count_per_level[l] (Odometry.h:170, default {4,8,16});
 * levels are visited n_levels-1 .. 0.  full_width/full_height = camera.GetWidth()/GetHeight(), the
 * denominator of both inlier ratios at EVERY level (Odometry.cpp:635,669,686).
 * Optional outputs (may be NULL): pixel_corr (corr_cap x 4 int32 {v_s,u_s,v_t,u_t}, raster order of
 * the source pixel = the reference's push_back order), point_corr (corr_cap x 6 float: source xyz,
 * target xyz, both read at the SOURCE pixel of level 0 as Odometry.cpp:676-683 does),
 * per_iter_count (sum(iters) int32) and per_iter_T (sum(iters) x 16): the correspondence count used
 * by, and the pose after, each executed iteration. */
int op_tracker_track(op_tracker *t, const op_track_level *levels, int n_levels,
                     const int32_t *iters_per_level, int full_width, int full_height, int term_type,
                     const float init_T[16], int mem, op_track_result *result, int32_t *pixel_corr,
                     float *point_corr, size_t corr_cap, int32_t *per_iter_count, float *per_iter_T);
/* ComputeCorrespondencePixelWise (DenseOdometryFunction.cpp:72-128) alone, incl. its source-indexed
 * "z-buffer" (:9-27): what DenseTracking runs with the identity pose before NormalizeIntensity
 * (Odometry.cpp:543-544). */
int op_tracker_correspondences(op_tracker *t, const op_track_level *level, const float T[16], int mem,
                               int32_t *pixel_corr, size_t corr_cap, size_t *n);
/* Odometry::DenseTracking, cv::Mat overload (Odometry.cpp:463-524), end to end on the device:
 * InitializeRGBDDenseTracking (:609-620) for both frames, ComputeCorrespondencePixelWise at the
 * identity + NormalizeIntensity (:543-544, DenseOdometryFunction.cpp:129-145), CreatePyramidCameras,
 * CreateImagePyramid (:436-449), MultiScaleComputing.  rgb: 3 bytes / pixel in stored order; depth:
 * OP_DEPTH_F32 metres or OP_DEPTH_U16 raw (divided by cam->depth_scale).  n_levels = multi_scale_level.
 * PARITY NOTE: the reference's cvtColor / GaussianBlur / pyrDown / Sobel are OpenCV calls (not vendored);
 * this entry point implements their published definitions (BORDER_REFLECT_101, float) and is checked
 * against a restatement of those definitions, not against OpenCV.  A caller who needs the reference's
 * exact OpenCV pyramids builds them on the host and calls op_tracker_track. */
int op_tracker_dense_tracking(op_tracker *t, const op_camera *cam, int n_levels,
                              const int32_t *iters_per_level, const uint8_t *source_rgb,
                              const uint8_t *target_rgb, const void *source_depth,
                              const void *target_depth, int depth_fmt, const float init_T[16],
                              int term_type, int mem, op_track_result *result, int32_t *pixel_corr,
                              float *point_corr, size_t corr_cap);
/* The same call split in two so that several trackers (each owns a HIP stream) can work on independent
 * frame pairs concurrently -- a single 640x480 track is 28 strictly sequential small problems that leave
 * most of the 256 CUs idle.  _enqueue returns as soon as everything is on the tracker's stream (device
 * frames are used in place and must stay valid until the wait); op_tracker_wait synchronises that stream
 * and fills the result.  One enqueue may be outstanding per tracker.  With the reference-order sums
 * (OP_TRACK_SUMS_REFERENCE_F32*), which need the host after every iteration, the run proceeds on a host thread of
 * the tracker's own, so _enqueue still returns at once and trackers still overlap; HOST frames must then stay
 * valid until the wait as well. */
int op_tracker_dense_tracking_enqueue(op_tracker *t, const op_camera *cam, int n_levels,
                                      const int32_t *iters_per_level, const uint8_t *source_rgb,
                                      const uint8_t *target_rgb, const void *source_depth,
                                      const void *target_depth, int depth_fmt, const float init_T[16],
                                      int term_type, int mem, int want_point_corr);
int op_tracker_wait(op_tracker *t, op_track_result *result, int32_t *pixel_corr, float *point_corr,
                    size_t corr_cap);
/* Frame-to-MODEL tracking (the KinectFusion loop: render, track, fuse; NO reference counterpart -- the reference's DenseSlam tracks frame to frame).
 * The SOURCE frame is volume `v` rendered at camera-to-world `model_pose` with `cam` (op_volume_render_frame's definition), into a frame buffer the
 * tracker owns: it never reaches the host.  The TARGET frame is the caller's (rgb, depth, depth_fmt, mem as in op_tracker_dense_tracking; the model
 * view's depth is float metres whatever depth_fmt says).  `result` is exactly what op_tracker_dense_tracking returns for that source / target pair,
 * in the tracker's current OP_TRACK_OPT_SUMS mode.  pose_out (may be NULL) = model_pose * T^-1 (DenseSlam.cpp:30's composition: op_mat4_inverse's
 * arithmetic, float32 products) when result->tracking_success is set, else a copy of model_pose.  model_pixels (may be NULL) = the model view's
 * pixels with depth > 0.  The frames queued on the volume are fused before the view is rendered; the volume's stream renders, the tracker's stream
 * waits for it through an event.  An empty volume or a view that sees nothing is no error: the source frame is all zero, model_pixels = 0 and the
 * result is the one op_tracker_dense_tracking gives for such a frame.  Volume and tracker must live on the same device. */
int op_tracker_track_model(op_tracker *t, op_volume *v, const op_camera *cam, int n_levels,
                           const int32_t *iters_per_level, const float model_pose[16], const uint8_t *rgb,
                           const void *depth, int depth_fmt, const float init_T[16], int term_type, int mem,
                           op_track_result *result, float pose_out[16], uint64_t *model_pixels);
/* Measurement hook: the LAST op_tracker_track_model call of this tracker -- the time its model view took on the volume's stream (HIP events around the
 * render; it includes fusion work the volume still had queued only in so far as the render had to flush it) and the whole call on the host's clock, in ms. */
int op_tracker_model_times(op_tracker *t, double *render_ms, double *total_ms);
/* Reads back an image prepared by the last op_tracker_dense_tracking call: frame 0 source / 1 target;
 * kind 0 colour, 1 depth, 2 colour_dx, 3 colour_dy, 4 depth_dx, 5 depth_dy (derivatives: target only). */
int op_tracker_read_pyramid(op_tracker *t, int frame, int kind, int level, float *out, size_t cap);
/* Convenience: create + track + destroy. */
int op_dense_track(const op_track_level *levels, int n_levels, const int32_t *iters_per_level,
                   int full_width, int full_height, int term_type, const float init_T[16], int mem,
                   int device, op_track_result *result, int32_t *pixel_corr, float *point_corr,
                   size_t corr_cap);
/* Host-side arithmetic of that path, exported so it can be checked without a GPU:
 * K*R*K.inverse() and K*t as Eigen 3.3.7 evaluates them (DenseOdometryFunction.cpp:82-87; cam4 =
 * {fx,fy,cx,cy}, row-major 3x3 out) and JTJ.ldlt().solve(-JTr) (:404; JTJ row-major 6x6). */
int op_track_projection(const float cam4[4], const float T[16], float KRK_inv[9], float Kt[3]);
int op_ldlt_solve6(const double JTJ[36], const double JTr[6], float x[6]);

#ifdef __cplusplus
}
#endif
#endif /* ONEPIECE_HIP_H */
