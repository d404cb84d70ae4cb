/*
 * onepiece_oracle.h -- CPU restatement (plain C) of the OnePiece TSDF-fusion + ICP hot path.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing in the product path (onepiece_amd/, include/) may link,
 * import or call this.  Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg do,
 * and only as the checker / the timed CPU baseline.
 *
 * PARITY STATUS: partially pinned against the compiled reference.  The reference hot-path
 * translation units all include <opencv2/...> (src/Geometry/Geometry.h:4-8) and OpenCV is neither
 * vendored nor installed; the reference ships no tests/golden vectors.
 * What this restatement IS pinned against:
 *   - the reference's own integration::CubeHandler (fusion, Transform / TransformNearest, Merge, GetPointCloud, the mesh calls, AddCube,
 *     the .map formats), the sources of its Integration/ directory compiled in place against a cv::Mat stand-in by oracle/tools/gen_volume_golden.py:
 *     tests/golden/volume_ops_reference.npz, reproduced bit for bit (tests/test_volume_golden_cpu.py);
 *   - the reference's vendored third-party arithmetic (Eigen 3.3.7 4x4 SSE inverse, fixed-size
 *     product / dot evaluation order, JacobiSVD solve, Sophus SE3::exp), through golden vectors
 *     generated in the build container by oracle/tools/gen_eigen_golden.cpp and committed under
 *     tests/golden/;
 *   - the reference's vendored nanoflann 1.3.2, driven as geometry::KDTree drives it (KDTree.h:62-98,171-190): the 1-NN and k-NN
 *     searches return its indices and squared distances bit for bit on tie-free clouds (tests/golden/nanoflann_golden.json from
 *     oracle/tools/gen_nanoflann_golden.cpp); among exactly equidistant candidates nanoflann keeps the first its traversal met,
 *     this file the smallest index -- the fixture's lattice cases record that difference;
 *   - the VoxelGridHasher known answers in SURVEY.md A.8;
 *   - the reference-run statistics recorded in SURVEY.md Appendix B / section 6 (block count,
 *     observed-voxel count, weight sum, XOR of key hashes for the 5-frame "wall" scene).
 *
 * All matrices cross this API as ROW-MAJOR float[16].  Every function cites the reference
 * file:line (relative to /root/reference/src) that it follows.
 */
#ifndef ONEPIECE_ORACLE_H
#define ONEPIECE_ORACLE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    float fx, fy, cx, cy;
    int width, height;
    float depth_scale;
} orc_camera; /* Camera/Camera.h:13-131 */

typedef struct orc_volume orc_volume;

/* Eigen 3.3.7 LU/arch/Inverse_SSE.h:35-165 (what pose.inverse() runs, Integrator.cpp:18,48). */
void orc_mat4_inverse(const float m[16], float out[16]);
/* Geometry/Geometry.h:101-112 */
uint64_t orc_hash(int x, int y, int z);
/* Integration/Frustum.cpp:7-46, Geometry.cpp:165-171. planes: top,left,right,bottom,near,far. */
void orc_frustum_planes(const orc_camera *cam, const float pose[16], float far_d, float near_d,
                        float planes[24]);
/* Threads used by orc_compute_bounding / orc_volume_prepare_cubes / orc_volume_integrate (default 1 = the
 * reference's serial path, which is what cpu_baseline times); results do not depend on it. */
void orc_set_fusion_threads(int n);
/* Integration/CubeHandler.cpp:116-145; returns number of points inside the frustum. */
size_t orc_compute_bounding(const orc_camera *cam, const void *depth, int is_u16,
                            const float pose[16], float far_d, float near_d, float max_pos[3],
                            float min_pos[3]);
/* Integration/Integrator.cpp:8-35 (pose_inv supplied). */
float orc_get_sdf(const orc_camera *cam, const float p[3], const float pose_inv[16],
                  const void *depth, int is_u16);
/* Integration/VoxelCube.h:63-74 */
void orc_cube_id(float res, const float p[3], int id[3]);

orc_volume *orc_volume_create(const orc_camera *cam, float voxel_res, float trunc, float far_d,
                              float near_d);
void orc_volume_destroy(orc_volume *v);
void orc_volume_clear(orc_volume *v);
size_t orc_volume_block_count(const orc_volume *v);
/* Integration/CubeHandler.cpp:147-196: fills ids (n x 3, loop order), allocates blocks.
 * Returns the list length (may exceed cap; only cap entries written).  n_candidates = bbox size. */
size_t orc_volume_prepare_cubes(orc_volume *v, const void *depth, int is_u16, const float pose[16],
                                int32_t *ids, size_t cap, size_t *n_candidates);
/* Integration/CubeHandler.cpp:197-210 + Integrator.cpp:36-94.  rgb = 3 bytes / pixel in stored
 * channel order.  Returns list length; *n_visited = 512*len, *n_updated = voxels passing the
 * update predicate. */
size_t orc_volume_integrate(orc_volume *v, const void *depth, int is_u16, const uint8_t *rgb,
                            const float pose[16], uint64_t *n_visited, uint64_t *n_updated);
/* Export in insertion order: keys n x 3 int32, voxels n x 512 x 5 float {sdf,w,c0,c1,c2}. */
size_t orc_volume_export(const orc_volume *v, int32_t *keys, float *voxels, size_t cap);
/* AddCube + overwrite (used to build volumes from arrays). */
void orc_volume_import(orc_volume *v, const int32_t *keys, const float *voxels, size_t n);
/* Integration/CubeHandler.h:145-167 */
int orc_volume_merge(orc_volume *dst, const orc_volume *src);

/* Integration/CubeHandler.h:242-338 (nearest != 0: TransformNearest incl. its default-resolution
 * quirk, else Transform with trilinear ReadVoxelInterpolate, VoxelCube.cpp:6-50).  New volume. */
orc_volume *orc_volume_transform(const orc_volume *src, const float T[16], int nearest);
float orc_volume_resolution(const orc_volume *v);
/* Integration/CubeHandler.cpp:45-69: points + colours (n x 3 each); returns the full count. */
size_t orc_volume_point_cloud(const orc_volume *v, float *xyz, float *colors, size_t cap);
/* Integration/CubeHandler.h:40-128 (.map stream format; legacy_float = ReadFromFileFloat). */
int orc_volume_write_file(const orc_volume *v, const char *path);
int orc_volume_read_file(orc_volume *v, const char *path, int legacy_float);

/* CubeHandler::ExtractTriangleMesh / GenerateMeshByCube (CubeHandler.cpp:9-114) + MarchingCube
 * (MarchingCube.cpp:8-74).  tri_table (256 x 16, -1 terminated rows) and edge_pairs (12 x 2) are the
 * CALLER'S data (the reference keeps them in MarchingCubePredefined.h).  3 unshared vertices per triangle;
 * returns the vertex count (may exceed cap_vertices; only cap written).  only_block: NULL or one CubeID. */
size_t orc_volume_extract_mesh(const orc_volume *v, const int32_t *tri_table, const int32_t *edge_pairs,
                               const int32_t *only_block, float *points, float *colors, size_t cap_vertices);

/* Ray casting -- NO reference counterpart; restates the definition of op_volume_raycast. */
void orc_volume_raycast(const orc_volume *v, const orc_camera *cam, const float pose[16], float *depth_out,
                        float *normals_out, float *colors_out);

/* ---- Registration ---- */
/* Geometry/PointCloud.cpp:72-100.  Returns count; xyz has room for w*h*3 floats. */
size_t orc_load_from_depth(const orc_camera *cam, const void *depth, int is_u16, float *xyz);
/* Geometry/Geometry.cpp:9-13 via Sophus SE3::exp (3rdparty/Sophus/sophus/se3.hpp). */
void orc_se3_exp(const float x[6], float T[16]);
/* Geometry/Geometry.cpp:107-151.  pairs: n x 6 floats (source xyz, target xyz). */
void orc_kabsch(const float *pairs, size_t n, float T[16]);
/* JacobiSVD(JTJ).solve(-JTr), ICP.cpp:137-138 (restated as symmetric Jacobi in double). */
void orc_solve6(const float JTJ[36], const float JTr[6], float x[6]);
/* Registration/ICP.cpp:108-144. inliers: n x 2 int32 (source id, target id). */
void orc_p2plane_step(const float *src, const float *tgt, const float *tgt_n,
                      const int32_t *inliers, size_t n, float T[16], float JTJ[36], float JTr[6]);

/* Geometry/PointCloud.cpp:102-144 (normals up to sign; < 3 neighbours -> (0,0,0)). */
void orc_estimate_normals(const float *pts, size_t n, float radius, int knn, float *normals);
/* the kd-tree searches behind orc_icp (k = 1) and orc_estimate_normals (k > 1); checked against nanoflann's answers in tests/golden */
void orc_knn_search(const float *tgt, size_t n_tgt, const float *queries, size_t n_q, int k, int32_t *idx, float *d2, int32_t *found);

/* Diagnostic only: 1 = accumulate the normal equations in double (the reference uses float). */
void orc_set_accumulate_double(int on);

typedef struct {
    float T[16];          /* RegistrationResult::T (Kabsch over final inliers) */
    float last_T[16];     /* accumulated start_T after the loop (not returned by the reference) */
    double rmse;
    size_t n_inliers;     /* size of correspondence_set_index */
    int iterations;
} orc_icp_result;

/* Registration/ICP.cpp:146-224 (mode 1) and :31-107 (mode 0 = PointToPoint).
 * inlier_pairs: room for n_src x 2 int32; per_iter_inliers: room for max_iter entries;
 * per_iter_T: room for max_iter x 16 floats (start_T after each iteration); any may be NULL. */
int orc_icp(int point_to_plane, const float *src, size_t n_src, const float *tgt, size_t n_tgt,
            const float *tgt_normals, const float init_T[16], int max_iter, double threshold,
            orc_icp_result *res, int32_t *inlier_pairs, int32_t *per_iter_inliers,
            float *per_iter_T);

/* ---- Dense RGB-D tracker (Odometry/) ----
 * Boundary = the inputs of Odometry::MultiScaleComputing (Odometry.cpp:621-636): the image pyramids
 * are GIVEN (they come out of cv::pyrDown / cv::Sobel / cv::GaussianBlur, un-vendored OpenCV, so
 * nothing below that boundary can be pinned here).  Image-XYZ pyramids are recomputed from the
 * depth pyramids with TransformToMatXYZ's own arithmetic (Geometry.cpp:72-106). */
typedef struct {
    int width, height;              /* camera_pyramid[l].GetWidth()/GetHeight() == image size */
    float fx, fy, cx, cy;           /* Camera.h:38-42 (GenerateNextPyramid halves all four) */
    const float *source_color, *source_depth; /* CV_32FC1, depth NaN = invalid (DenseOdometryFunction.cpp:28-56) */
    const float *target_color, *target_depth;
    const float *target_color_dx, *target_color_dy, *target_depth_dx, *target_depth_dy; /* raw Sobel (x SOBEL_SCALE inside) */
} orc_track_level;

typedef struct {
    float T[16];
    double rmse;                    /* ComputeReprojectionError3D over correspondence_set */
    size_t n_correspondences;       /* of the last executed iteration */
    int tracking_success;
    int iterations;                 /* iterations actually executed */
} orc_track_result;

/* Eigen 3.3.7 LU/InverseImpl.h:126-170 (Matrix3f::inverse()), row-major. */
void orc_mat3_inverse(const float m[9], float out[9]);
/* DenseOdometryFunction.cpp:82-87; cam = {fx,fy,cx,cy}. */
void orc_track_projection(const float cam[4], const float T[16], float K_inv[9], float KRK_inv[9], float Kt[3]);
/* DenseOdometryFunction.cpp:95-101; ut = {u_t, v_t}. */
void orc_track_project_pixel(const float KRK_inv[9], const float Kt[3], float d_s, int j, int i, float uv[3], int ut[2]);
/* DenseOdometryFunction.cpp:72-128 (+ :9-27).  corr: 4 int32 each {v_s,u_s,v_t,u_t}; may be NULL. */
size_t orc_pixel_correspondences(const orc_track_level *L, const float T[16], int32_t *corr);
/* DenseOdometryFunction.cpp:146-381; term 0 hybrid, 1 photo, 2 depth. */
void orc_track_normal_equations(const orc_track_level *L, const float T[16], const int32_t *corr, size_t n, int term,
                                float JTJ[36], float JTr[6], float *r2);
/* The accumulation statement of :297-381 alone, over given rows J (n x 6) and residuals r (n). */
void orc_track_accumulate_rows(const float *J, const float *r, size_t n, float JTJ[36], float JTr[6], float *r2);
/* JTJ.ldlt().solve(-JTr), DenseOdometryFunction.cpp:404 (restated in double). */
void orc_ldlt_solve6(const float JTJ[36], const float JTr[6], float x[6]);
/* DenseOdometryFunction.cpp:382-475 */
size_t orc_track_iteration(const orc_track_level *L, int term, float T[16], int32_t *corr);
/* Odometry.cpp:621-687 + :606. */
int orc_dense_track(const orc_track_level *levels, int n_levels, const int *iters, int full_w, int full_h, int term,
                    const float init_T[16], orc_track_result *res, int32_t *pixel_corr, int32_t *per_iter_count,
                    float *per_iter_T);

/* ---- tracker image preparation.  NOT pinned to OpenCV (un-vendored): restates the definitions the
 * product uses for cvtColor / GaussianBlur 3x3 / pyrDown / Sobel 3x3 (BORDER_REFLECT_101, float,
 * horizontal then vertical, taps accumulated in order).  Reference code here: ConvertDepthTo32FNaN,
 * the /255 scaling and NormalizeIntensity (DenseOdometryFunction.cpp:28-71,129-145). */
void orc_prep_intensity(const uint8_t *rgb, int w, int h, float *out);
void orc_prep_depth_nan(const void *depth, int is_u16, float depth_scale, int w, int h, float *out);
void orc_prep_blur3(const float *in, int w, int h, float *out);
void orc_prep_pyrdown(const float *in, int w, int h, float *out);   /* out: (w/2) x (h/2) */
void orc_prep_sobel(const float *in, int w, int h, int axis, float *out);
void orc_bilateral_filter(const void *depth, int is_u16, float depth_scale, int w, int h, int d, float sigma_color,
                          float sigma_space, float *out);
void orc_normalize_intensity(float *source, float *target, int w, int h, const int32_t *corr, size_t n);
/* Odometry::DenseTracking, cv::Mat overload (Odometry.cpp:463-524).  pyr_out: optional array of
 * 2*6*n_levels image pointers [(frame*6+kind)*n_levels+level], each released with orc_free. */
int orc_dense_tracking(const orc_camera *cam, int n_levels, const int *iters, const uint8_t *src_rgb, const uint8_t *tgt_rgb,
                       const void *src_depth, const void *tgt_depth, int is_u16, int term, const float init_T[16],
                       orc_track_result *res, int32_t *pixel_corr, float **pyr_out);
void orc_free(void *p);

#ifdef __cplusplus
}
#endif
#endif
