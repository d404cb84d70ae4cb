// zwin_cert.hpp -- what lets k_integrate's certified projection (project_pixel_uv<true, false>, volume_core.hpp) run without the window test
// 2^-60 <= |Z| < 2^60 on the depth coordinate Z: the upper side is proved here, on the host, once per frame; the lower side needs no test
// at all (px_round.hpp, px_cert_bound_folded: hypotheses).  Host-compilable without HIP (tests/test_kc_zwin_cpu.py), like px_round.hpp,
// kc_lanes.hpp and ka_cert.hpp.
//
// In k_integrate Z is row 2 of a frame's inverse pose applied to the centre of a voxel of a block that is IN THE HASH TABLE:
//     Z = fl(((M8 px + M9 py) + M10 pz) + M11)          (float32, Integrator.cpp:55-58 in Eigen's association; integrate.hip `project`)
//     p = fl(fl(fl(k * 8) * res) + fl(fl(l * res) + res / 2)),  block coordinate |k| <= kCoordLimit = 2^20 (pack_key has 21 bits per axis and
//     every call of table_claim stands behind key_in_range: select.hip k_mark_cubes -- the caller-listed cubes of op_volume_integrate_cubes --
//     and the three selection kernels, volume_ops.hip k_insert_keys -- uploads, merges, files -- and k_transform_alloc; k_rehash, the garbage
//     collector and the RCCL merge only move keys that were in a table), voxel 0 <= l <= 7, res the volume's voxel resolution.
// Bound on |p|: k * 8 is exact (|k * 8| <= 2^23), the product with res rounds once, l * res + res / 2 <= 7.5 res rounds twice, the last sum once:
//     |p| <= (2^23 res (1 + u) + 7.5 res (1 + u)^2)(1 + u) < (2^23 + 8) res (1 + 2^-22) =: P,   u = 2^-24
// The large term is rounded twice, in the product with res and again in the last sum, each time by up to 2^23 res u = res / 2; every other rounding
// is below 2^-20 res.  So |p| < (2^23 + 7.5 + 1.0 + 2^-19) res: the 8 of `kCoordLimit * 8 + 8` alone does NOT cover it (8.5 is needed); the factor
// (1 + 2^-22) does, which adds 2^23 res 2^-22 = 2 res: P > (2^23 + 10) res.
// Bound on |Z|: every term passes one product and at most three sums, M11 one sum; a product or sum that lands among the denormals is off by at
// most 2^-150 instead of a relative u, seven operations in all:
//     |Z| <= ((|M8| + |M9| + |M10|) P + |M11|)(1 + u)^4 + 7 * 2^-150 < ((|M8| + |M9| + |M10|) P + |M11|)(1 + 2^-21) + 2^-140 =: zwin_bound,
// evaluated in double, whose own roundings (five operations on non-negative terms, 2^-53 each) the step from (1 + u)^4 < 1 + 2^-22 + 2^-45
// to 1 + 2^-21 covers a million times over.  No intermediate of the float chain exceeds the bound either (they are partial sums of the same
// non-negative majorants), so a certified frame's Z is finite.
//
// The threshold is kZwinLimit = 2^59: half the 2^60 of the window test this certificate replaces -- which the exact fallback keeps as its own
// exponent test -- so a certified frame's |Z| would have passed that test's upper side with a factor 2 to spare, 2^21 times the slack in the
// bound above; and 2^67 below 2^126, above which v_rcp_f32 returns 0 (a reciprocal that would be denormal is flushed), the only thing the certified path itself needs from the upper
// side.  An ordinary pose is nowhere near: row 2 of a rigid motion has |M8| + |M9| + |M10| <= sqrt(3), and with res = 1 m and a translation of
// 10^6 m the bound is 1.6e7 = 2^24.
// Rows 0 and 1 (X and Y) need nothing: an overflowing numerator f * X makes t'' +-inf or NaN, which the certificate's fract test refuses.
#pragma once
#include <cmath>

constexpr double kZwinLimit = 0x1p59;
constexpr int kZwinCoordLimit = 1 << 20; // = kCoordLimit (volume_core.hpp asserts it)

// P above: the largest |coordinate| of a voxel centre of any block the table can hold; NaN for a resolution that is not a positive finite number
inline double zwin_coord_bound(float res) {
    if (!(res > 0.0f) || !std::isfinite(res)) return NAN;
    return ((double)kZwinCoordLimit * 8.0 + 8.0) * (double)res * (1.0 + 0x1p-22);
}
// The bound on |Z| for one frame, m = the 12 floats of its PoseInv (rows 0..2 of pose^-1); NaN / inf when an entry of row 2 is not finite
inline double zwin_bound(const float* m, float res) {
    const double P = zwin_coord_bound(res);
    return ((fabs((double)m[8]) + fabs((double)m[9]) + fabs((double)m[10])) * P + fabs((double)m[11])) * (1.0 + 0x1p-21) + 0x1p-140;
}
// true: every Z k_integrate can form for this frame is finite with |Z| < kZwinLimit.  (NaN fails the compare; an infinite entry gives inf or NaN.)
inline bool zwin_certified(const float* m, float res) {
    for (int k = 8; k < 12; ++k)
        if (!std::isfinite(m[k])) return false;
    return zwin_bound(m, res) < kZwinLimit;
}
// ... and for the n frames of a batch (inv = n consecutive PoseInv): what launch_integrate asks before it picks a certified gather kind
inline bool zwin_certified_batch(const float* inv, int n, float res) {
    for (int f = 0; f < n; ++f)
        if (!zwin_certified(inv + 12 * f, res)) return false;
    return true;
}
