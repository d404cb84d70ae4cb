// px_round.hpp -- the reference's pixel rounding  int u = fx*X/Z + 0.5 + cx  (Integrator.cpp:20-21,
// 61-62) for host and device.
//
// Reference semantics: a = (fx*X)/Z is a float; the literal 0.5 promotes the sum to double;
// t = (double)a + 0.5 + (double)c is exact for any pixel-scale a; the result is t truncated toward
// zero.  Non-finite or out-of-int-range t is UB in C++ (INT_MIN from cvttsd2si on x86) and is
// reported as INT_MIN here, which every caller rejects through its `u < 0` test.
//
// px_round_dp() evaluates exactly that in double.  px_round_sp() produces the SAME integer for every
// a whenever the caller's bounds test (0 <= u < width) can pass, using only fp32 compares and
// integer adds: a = trunc(a) + af and c = floor(c) + cf are exact splits, and the position of
// af + cf + 0.5 relative to 0, 1, 2 is decided by comparing af with the exactly representable
// thresholds -0.5-cf, 0.5-cf, 1.5-cf (exact when |c| >= 1 or c == 0; px_split() checks this and
// also excludes cf == 0.5, the one case where the reference's double sum is itself inexact in a
// way that matters -- callers then fall back to px_round_dp).
// fp64 adds/converts run at a fraction of the fp32 rate on CDNA4; the integrate kernel is
// ALU-bound once frames are batched, so this matters.  Equivalence is tested exhaustively-ish in
// tests/test_abi_cpu.py::test_pixel_rounding_fast_path_equals_double_formula (4e7 cases incl.
// values within a few ulp of every rounding boundary).
#pragma once
#include <climits>
#include <cmath>

#if defined(__HIPCC__)
#define OP_HD __host__ __device__ __forceinline__
#else
#define OP_HD inline
#endif

struct PxSplit {
    int ci;          // floor(c)
    float hm, h0, h1; // -0.5 - cf, 0.5 - cf, 1.5 - cf
    int exact;       // thresholds exactly representable -> fast path allowed
};

OP_HD PxSplit px_split(float c) {
    PxSplit s;
    const float fl = floorf(c);
    const float cf = c - fl;
    s.ci = (int)fl;
    s.hm = -0.5f - cf; s.h0 = 0.5f - cf; s.h1 = 1.5f - cf;
    // cf == 0.5 is excluded: there cf + 0.5 is an integer, and for |a| < ~1e-13 the reference's
    // double additions round a away (t lands exactly on the integer) while this path stays exact.
    s.exact = (fabsf(c) >= 1.0f || c == 0.0f) && fabsf(c) < 1.0e6f && cf != 0.5f;
    return s;
}

OP_HD int px_round_dp(float a, float c) {
    const double t = (double)a + 0.5 + (double)c;
    if (!(t > -2147483649.0 && t < 2147483648.0)) return INT_MIN;
    return (int)t;
}

OP_HD int px_round_sp(float a, const PxSplit& s) {
    if (!(fabsf(a) < 1.0e9f)) return INT_MIN; // NaN, inf and values no image can contain
    const float ai = truncf(a);
    const float af = a - ai; // exact, same sign as a, |af| < 1
    const int fl = (int)ai + s.ci - 1 + (af >= s.hm) + (af >= s.h0) + (af >= s.h1); // floor(t)
    if (fl >= 0) return fl;
    // t < 0: truncation toward zero = ceil(t); t is an integer only when af sits on a threshold
    const bool integral = af == s.hm || af == s.h0 || af == s.h1;
    return integral ? fl : fl + 1;
}

// ---- in-image pixel of one axis (what the kernels use) ----------------------------------------------------------
// The kernels only ever need the pixel when it lies INSIDE the image (Integrator.cpp:63 rejects everything else), and
// inside the image the truncation above is a floor except on t in (-1, 0), which truncates to 0:
//     0 <= trunc(t) <= extent - 1   <=>   -1 < t < extent   <=>   t_lo < a < t_hi,   t_lo = -(c + 1.5), t_hi = extent - c - 0.5
//     trunc(t) = max(floor(t), 0) there,   floor(t) = trunc(a) + floor(K) - 1 + [af >= h0] + [af >= h1],
// with K = c + 0.5, kf = K - floor(K), af = a - trunc(a) (exact), h0 = -kf, h1 = 1 - kf.  Two range compares on `a`, two
// threshold compares on `af`, no integer range tests, no special handling of NaN / inf / huge values (they fail the range
// compares).  Exact whenever t_lo, t_hi, h0, h1 are representable in fp32 and kf != 0 (then a tiny |a| cannot move the
// reference's double sum across an integer); px_axis() checks that and callers fall back to the double formula otherwise.
struct PxAxis {
    float t_lo, t_hi, h0, h1;
    int base;  // floor(c + 0.5) - 1
    int exact;
    float k;   // c + 0.5 rounded to fp32
    float hc;  // certificate of the fast path (px_certified): 0.5 - B, or -1 where the certificate may not be used
    float kb;  // folded certificate (px_certified_folded): c + 0.5 + B2, the first fp32 at or above c + 0.5 + B
    float h2;  // ... and its threshold B2 + B rounded up, or 2 where the certificate may not be used
};

// ---- certified fast path (project_pixel<true>, -DOP_PX_CERTIFIED=0 builds without it) --------------------------------------
// px_pixel_sp needs the correctly rounded quotient a = RN(nx / z) (nx = f * X, z = Z; a dozen instructions on the device).  Its result
// is trunc(t) of the REAL sum t = a + K, K = c + 0.5, inside the image, i.e. for -1 < t < extent.  The fast path instead forms
//     t' = RN(nx * y + K')   (one fma; K' = K rounded to fp32, |K' - K| is added to B),   y = the once-refined reciprocal of z,
// and takes u = trunc(t') (v_cvt_i32_f32) with "inside" = (unsigned)u < extent.  That is the same pixel whenever t and t' lie in the same
// open unit interval (n, n + 1): trunc is constant there and -1, extent are integers.  The certificate px_certified() accepts a lane only
// when t' is farther than B from every integer, with B >= |t' - t| derived as follows, for 2^-60 <= |z| < 2^60 (the caller's window)
// and |t'| <= T = extent + 1:
//  * y0 = v_rcp(z) with |1 - z y0| = d <= 2^-20 (the hardware gives ~2^-23); e = RN(1 - z y0), y = RN(y0 + e y0) (two fmas):
//    z y = (1 + d r1 - d^2 (1 + r1)) (1 + r2), |r1|, |r2| <= 2^-24, so |z y - 1| <= dy = 2^-24 + 2^-39.
//  * q = nx / z (real); a = RN(q) = q (1 + ra), |ra| <= 2^-24; nx y = q (1 + dq), |dq| <= dy.
//  * s = nx y + K' (exact inside the fma), t' = RN(s): |t' - s| <= 2^-24 |s|, |s| <= S = T / (1 - 2^-24).
//  * |s - t| = |q dq - q ra + K' - K| <= |q| (dy + 2^-24) + |K' - K|, |q| <= Q = (S + |K|) / (1 - dy) (|K'| <= |K|(1 + 2^-24): absorbed below).
//  So |t' - t| <= 2^-24 S + Q (dy + 2^-24) + |K' - K|, plus 2^-22 for the fract and the subtraction in px_certified (t' - floor(t') is exact
//  except on (-1, 0), where it rounds and is clamped below 1 by at most 2^-24; f - 0.5 rounds by at most 2^-26) and for denormals.
// Lanes with T < |t'| < 2^23 that pass are outside the image on both paths: there |t' - t| < 2^-22 (|t'| + |K|) + 2^-22 < |t'| - extent
// (t' > T) resp. < |t'| - 1 (t' < -T) because extent < 2^20 and |K| < 2^20 -- so u = trunc(t') answers "outside" correctly.  |t'| >= 2^23
// has fract 0 and NaN / inf have fract NaN: both fail the certificate, as do all lanes when hc = -1.
OP_HD double px_cert_bound(double T, double absK) {
    const double u = 0x1p-24, dy = u + 0x1p-39;
    const double S = T / (1.0 - u), Q = (S + absK) / (1.0 - dy);
    return (u * S + Q * (dy + u) + 0x1p-22) * (1.0 + 0x1p-40); // (the last factor covers the rounding of this double evaluation)
}
// ---- folded certificate (what project_pixel<true> uses; px_certified above stays as the two-sided statement of the same thing) ----------
// The two-sided test costs v_fract, v_add -0.5 and a compare of the magnitude.  Shifting t' UP by a margin B2 >= B turns it into a
// one-sided test, and the shift costs nothing when it is part of the FMA's constant:
//     t'' = RN(nx * y + kb),   kb = an fp32 with B2 = kb - K >= B (exact in double: K = c + 0.5 and kb are close floats / half-integers),
//     y = v_rcp_f32(z) as the hardware delivers it, NOT refined (one step: the two FMAs of the Newton step are gone from the fast path),
//     certified  <=>  fract(t'') > h2,   h2 >= B2 + B,   pixel u = trunc(t''), inside = (unsigned)u < extent.
// Error, for -2 <= t'' <= T = extent + 1 (the sums whose pixel matters).  With s'' = nx y + kb (real, formed exactly inside the fma) the chain of
// px_cert_bound applies with kb in K's place and NO |K' - K| term -- kb's rounding is not an error here, B2 is DEFINED as kb - K, whatever px_axis
// had to round to get a float: s'' - B2 = nx y + K, t = a + K, so
//     (t'' - B2) - t = (t'' - s'') + q (dq - ra),   |t'' - s''| <= 2^-24 P,  |dq| <= dy,  |ra| <= 2^-24,
// with P = the largest power of two <= T: t'' = RN(s'') is off by at most half an ulp of t'', and every float with |t''| <= T < 2 P has an ulp of at
// most 2^-23 P (P >= 2 because T >= 2, so the sums in [-2, 0] are covered as well).  The relative form 2^-24 |s''| <= 2^-24 S of px_cert_bound charges
// the top binade's half ulp at its upper end, a quarter more than any rounding there can be (3.8e-5 instead of 3.05e-5 at T = 641); with it the bound
// was so slack that a reciprocal twice as far off as d_rcp still produced no wrong pixel, i.e. tests/test_px_unrefined_cpu.py could not see the
// hypothesis the bound rests on.  The reciprocal:
// the chain for the unrefined reciprocal is one step long: z y = 1 + d with |d| <= d_rcp = kPxRcpErr, so nx y = (nx / z)(z y) = q (1 + dq) with
// dq = d: dy = d_rcp (the refined form had dy = 2^-24 + 2^-39; px_cert_bound above still states that one).  d_rcp is not taken on faith: over all 2^23
// significands of [1, 2) and of [-2, -1), and 2^16 random ones in each of the binades 2^-60, 2^-1, 2^59, the device shows max |1 - z y| =
// 9.1483642e-8 = 0.76742 * 2^-23 (at z = +-1.8744549; tests/test_kc_diet_gpu.py repeats the sweep against the constant), rounded up to the short
// binary constant 2^-23 = 1.1920929e-7 -- which is also what an error of one ulp of y gives at most (|y - 1/z| <= ulp(y) <= 2^-24 for y in [1/2, 1),
// times |z| < 2), the accuracy div_int_rcp (volume_core.hpp) relies on for integer divisors.
// What the chain asks of z -- stated without a caller's window, because k_integrate calls the projection without one (project_pixel_uv<true, false>):
//  * z normal with a normal reciprocal, 2^-126 <= |z| <= 2^126 (the device returns 2^-126 for 2^126 and 0 for everything larger).  v_rcp_f32 works on the
//    significand and negates the exponent, so the sweep over all 2^23 significands covers every such binade, the ones below 2^-60 included: samples
//    of each binade from 2^-126 to 2^-60 show at most 0.763 * 2^-23 (tests/test_kc_zwin_gpu.py).  Nothing else in the chain depends on |z|: q = nx / z is
//    a real number, nx y is formed exactly inside the FMA (the code objects keep fp32 denormals, float_denorm_mode_32 = 3, so a denormal nx enters
//    it as it is), and |q| is bounded through t'', not through z.  The upper end is the caller's: |z| < 2^60 by the window test, or |z| < 2^59 by
//    the host's bound for every frame of a k_integrate launch (zwin_cert.hpp).
//  * z zero or denormal: v_rcp_f32 returns +-inf (measured for +-0 and for denormals across the range, same file), so t'' = fma(nx, +-inf, kb) is
//    +-inf, or NaN when nx is 0: fract(t'') is NaN and the lane is refused by the certificate itself.  It takes the exact sequence, whose own
//    exponent test rescales such a z.
//  * a denormal nx = fl(f X): the same float on both paths (and in the reference), so its rounding is no difference between them; charged as one all
//    the same it is 2^-150 |y| <= 2^-24.  A denormal quotient a = RN(q) is off by 2^-150 at most instead of a relative 2^-24.  Both fit the 2^-22 in
//    reserve below: B is unchanged, and so is the share of wave-projections on the exact fallback.
//  * NaN z gives NaN, a product nx y beyond the floats +-inf: refused.  (z = +-inf, which no caller lets through, gives y = 0 and t'' = kb, the sum of
//    the quotient 0 the reference forms.)
// Here |s''| <= |t''| / (1 - 2^-24), so s'' lies in [-L, S] with L = 2 / (1 - 2^-24), S = T / (1 - 2^-24) >= L, and q (1 + dq) = s'' - kb lies in
// [-L - kb, S - kb]: |q| <= Qf = (max(|S - K|, |L + K|) + 1/4) / (1 - dy) for every kb in [K, K + 1/4] (px_axis refuses an axis whose B2 would exceed
// 1/4).  px_cert_bound took |q| <= S + |K| over the whole window |t'| <= T instead; for a principal point near the middle of the image that is three
// times what a sum in [-2, T] can have, and the far negative part of the window needs no such bound (last paragraph).  So
//     |(t'' - B2) - t| < B := px_cert_bound_folded(T, K) = 2^-24 P + Qf (dy + 2^-24) + 2^-22,
// the last term in reserve for denormal quotients (their RN is off by 2^-150 at most, not by a relative 2^-24).  For a certified t'' in [-2, T],
// n = floor(t''), f = fract(t''):
//  * n >= 0: f = t'' - n exactly.  t > t'' - B2 - B > n + h2 - B2 - B >= n, and t < t'' - B2 + B < n + 1 because B2 >= B: t lies in
//    (n, n + 1), trunc(t) = n = trunc(t'').
//  * -1 < t'' < 0 (v_cvt_i32_f32 gives 0; the reference's pixel 0 covers the reals (-1, 1)): v_fract returns RN(t'' + 1) clamped below 1, and
//    RN(x) > h2 needs x > h2 (h2 is a float, RN is monotone): t'' + 1 > h2, t > t'' - B2 - B > -1 + h2 - B2 - B >= -1; and t < t'' - B2 + B
//    <= t'' < 0: trunc(t) = 0.  (The downward shift, certified <=> fract < h2, fails exactly here: it would certify t'' = -1, fract 0,
//    whose t lies in (-1, 0) -- pixel 0 -- while trunc(-1) = -1 says outside.  Upward, t'' = -1 and t'' = +-0 have fract 0: refused.)
//  * -2 < t'' < -1 (t'' = -2 and -1 have fract 0 and are refused): f = t'' + 2 exactly, t lies in (-2, -1) as in the first case: trunc(t) = -1 =
//    trunc(t''), outside on both paths.
// Off the image, 2^23 > t'' > T or -2^23 < t'' < -2: with |q| <= (|s''| + |kb|) / (1 - dy) and extent, |K| < 2^20 the error is
// |(t'' - B2) - t| <= 2^-24 |s''| + 3 * 2^-24 |q| < 2^-22 (|t''| + |K| + 1/4) + 2^-22 < 0.26 + 2^-22 |t''|.  t'' > extent + 1: t > t'' - 1/4 - 0.26 - 2^-22 t'' > extent (the left side
// grows with t''): outside, and u = trunc(t'') >= extent + 1 says so.  t'' < -2: t < t'' + 0.26 + 2^-22 |t''| < -1: trunc(t) <= -1, and u <= -2.
// |t''| >= 2^23 has fract 0, NaN has fract NaN (so has +-inf, whose v_cvt_i32_f32 saturates outside the image anyway), h2 = 2 exceeds every fract:
// all refused.
// Width of the accepted set per unit interval: 1 - h2 = 1 - 2B - (B2 - B) with 0 <= B2 - B < ulp(kb) (+ one ulp of h2's own rounding).  With the
// bound of the two-sided form the fold would cost up to one ulp(K) of width (3e-5 at K ~ 320, a tenth of its 2B: 3.42 % -> 3.76 % of wave-
// projections took the exact fallback on the bench frames); with B halved by the argument above the rate falls instead (profiles/kc_trim_ab.txt).
// The unrefined reciprocal widens B again, by Qf (d_rcp - 2^-24), and the half-ulp rounding term takes 2^-24 (S - P) back: for 640 pixels and a
// principal point near the middle (Qf ~ 322, P = 512) B goes from 7.7e-5 to 8.8e-5 (9.6e-5 with the relative rounding term); the fallback share on
// the bench frames is in profiles/kc_diet_ab.txt.
constexpr double kPxRcpErr = 0x1p-23; // d_rcp: >= |1 - z * v_rcp_f32(z)| for every normal z whose reciprocal is normal (measured maximum 0.76742 * 2^-23, see above)
OP_HD double px_cert_bound_folded(double T, double K) {
    const double u = 0x1p-24, dy = kPxRcpErr;
    const double S = T / (1.0 - u), L = 2.0 / (1.0 - u);
    const double Qf = (fmax(fabs(S - K), fabs(L + K)) + 0.25) / (1.0 - dy);
    int e2;
    frexp(T, &e2);
    const double P = ldexp(1.0, e2 - 1);                       // the largest power of two <= T
    return (u * P + Qf * (dy + u) + 0x1p-22) * (1.0 + 0x1p-40); // (the last factor covers the rounding of this double evaluation)
}

OP_HD PxAxis px_axis(float c, int extent) {
    PxAxis s;
    const double K = (double)c + 0.5, ki = floor(K), kf = K - ki;
    const double t_lo = -((double)c + 1.5), t_hi = (double)extent - (double)c - 0.5, h0 = -kf, h1 = 1.0 - kf;
    s.t_lo = (float)t_lo; s.t_hi = (float)t_hi; s.h0 = (float)h0; s.h1 = (float)h1;
    s.base = (int)ki - 1;
    s.exact = (double)s.t_lo == t_lo && (double)s.t_hi == t_hi && (double)s.h0 == h0 && (double)s.h1 == h1 && kf != 0.0 &&
              fabs((double)c) < 1.0e6 && extent > 0 && extent < (1 << 20);
    s.k = (float)K;
    s.hc = -1.0f;
    if (s.exact) {
        const double B = px_cert_bound((double)extent + 1.0, fabs(K)) + fabs((double)s.k - K); // (s.k is K rounded to fp32: exact, or off by <= 2^-24 |K|)
        float hc = (float)(0.5 - B);
        if ((double)hc > 0.5 - B) hc = nextafterf(hc, 0.0f); // rounded down: never wider than derived
        s.hc = hc;
    }
    s.kb = s.k;
    s.h2 = 2.0f;
    if (s.exact) {
        const double B2min = px_cert_bound_folded((double)extent + 1.0, K);
        float kb = (float)(K + B2min);
        if ((double)kb < K + B2min) kb = nextafterf(kb, INFINITY);  // rounded up: B2 = kb - K >= B
        const double B2 = (double)kb - K;                           // exact
        float h2 = (float)(B2 + B2min);
        if ((double)h2 < B2 + B2min) h2 = nextafterf(h2, INFINITY); // rounded up: never wider than derived
        if (B2 <= 0.25) { s.kb = kb; s.h2 = h2; }
    }
    return s;
}

// true + the pixel when it is inside [0, extent), false otherwise
OP_HD bool px_pixel_sp(float a, const PxAxis& s, int& u) {
    const float ai = truncf(a);
    const float af = a - ai; // exact
    const int fl = (int)ai + s.base + (af >= s.h0) + (af >= s.h1);
    u = fl < 0 ? 0 : fl;
    return a > s.t_lo && a < s.t_hi;
}
// The fast path's certificate on t' (see px_cert_bound): true when trunc(t') is the pixel px_pixel_sp gives, inside or outside.
OP_HD float px_fract(float t) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_fractf(t); // v_fract_f32: t - floor(t) clamped below 1; NaN for NaN and +-inf
#else
    const float f = t - floorf(t); // (inf - inf = NaN, as on the device)
    return f >= 1.0f ? 0x1.fffffep-1f : f;
#endif
}
OP_HD bool px_certified(float t, const PxAxis& s) {
    return fabsf(px_fract(t) - 0.5f) < s.hc; // distance of t to the nearest integer > 0.5 - hc >= B; false for NaN
}
// The folded certificate on t'' = fma(f*X, y, kb) (see above): true when trunc(t'') is the pixel px_pixel_sp gives, inside or outside.
OP_HD bool px_certified_folded(float t2, const PxAxis& s) {
    return px_fract(t2) > s.h2; // false for NaN
}
OP_HD bool px_pixel_dp(float a, float c, int extent, int& u) {
    u = px_round_dp(a, c);
    return u >= 0 && u < extent;
}
