// Registration/3DFeature.h -- FPFH point features (reference: src/Registration/3DFeature.h:16-23, 3DFeature.cpp:9-130), for
// example/DenseFusion's submap registration.  Pinned (tests/global_registration_common.py, a numpy statement that uses none of this code) to
// EXACT radius neighbours followed by the arithmetic of 3DFeature.cpp; not pinned: nanoflann's approximate radius search that the reference asks
// instead (1024 checks), and the RNG-driven RANSAC the features feed.
// Two paths, chosen by op_runtime_set_option(OP_RUNTIME_OPT_GLOBAL_REGISTRATION): 0 (default) the host loops of src/GlobalRegistration.cpp;
// 1 the device (op_fpfh_compute: k_fpfh_neighbours, k_spfh, k_fpfh), which restates those loops operation by operation.  Identical on both:
// the neighbour lists (order and count), the second and third angle's histograms and every feature bin built from them, bit for bit.  The
// ONE-BIN RULE for the first angle: the host rounds it with its libm's atan2f, the device rounds a double atan2 once; the two differ by at most
// one ulp, so a pair whose angle lies within an ulp of a bin boundary (boundaries are k * 2 pi / 11 - pi, and the +-pi wrap) may count in the
// adjacent bin, and the features that include that histogram move by that one increment.  No pair of the tested room clouds does.
//
// A feature is a 33-bin histogram (3 angles x 11 bins) held in a geometry::VectorX.  ComputeFPFHFeature follows the reference's arithmetic as
// written (src/Feature3D.cpp): neighbours = the points whose SQUARED distance is below `radius` (the reference hands the radius to nanoflann's
// L2 adaptor unsquared, KDTree.h:133), ascending by (squared distance, index), at most `knn` of them including the point itself; the FIRST of them
// is skipped as "the point itself" (3DFeature.cpp:54) -- which it is unless an exact duplicate of the point has a lower index: then the duplicate
// is skipped and the point meets itself as a neighbour at distance 0.  Every other neighbour adds the INTEGER quotient
// 100 / (n - 1) to one bin per angle (3DFeature.cpp:50: both operands are ints); the final feature is the point's own histogram plus the
// 1/distance-weighted histograms of its neighbours, each third rescaled to 100 by the UNWEIGHTED sum (3DFeature.cpp:104-124).  One deviation:
// a third whose neighbour sum is zero stays zero here (the reference multiplies by 100/0 and stores NaN).  Two roundings are also placed
// differently from a literal reading of 3DFeature.cpp, on both paths and in the tests' statement alike: the third feature is u . ((pt - ps) /
// distance) here where :21 parses as (u . (pt - ps)) / distance, and the bins of the second and third feature are floor(11.0 * x) in double
// where :64-65 multiply the float by the int 11 first; either moves a pair only when it lies within a float ulp of a bin boundary (one pair in
// 1.3 million of the tests' clouds for the first, none for the second).  The reference's ComputeSPFH takes
// its KDTree wrapper as an argument and is therefore not part of this surface.
#pragma once
#include <vector>

#include "Geometry/Geometry.h"
#include "Geometry/PointCloud.h"

namespace one_piece {
namespace registration {

typedef geometry::Vector4 PairDescriptor;
typedef geometry::VectorX Feature;        // 33 bins
typedef geometry::PointXList FeatureSet;

// the three Darboux-frame angles and the distance of an oriented point pair (3DFeature.cpp:9-27): (atan2(w.nt, u.nt), v.nt, u.d, |pt - ps|)
PairDescriptor ComputePairDescriptor(const geometry::Point3& ps, const geometry::Point3& ns, const geometry::Point3& pt, const geometry::Point3& nt);
void ComputeFPFHFeature(const geometry::PointCloud& pcd, FeatureSet& fpfh_features, int knn = 100, float radius = 0.1);
// (not in the reference) the same call, also handing out what it is built from: the neighbour list of every point (the point itself first, unless an exact duplicate
// has a lower index: ties in distance go to the lower index) and
// the simplified histograms of the first pass; either pointer may be null.  What examples/cpp/GlobalRegistration.cpp dumps and the tests compare.
void ComputeFPFHFeatureDebug(const geometry::PointCloud& pcd, FeatureSet& fpfh_features, int knn, float radius, std::vector<std::vector<int> >* neighbours_out,
                             std::vector<std::vector<float> >* spfh_out);

} // namespace registration
} // namespace one_piece
