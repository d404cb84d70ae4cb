// ka_cert.hpp -- what lets k_prepare_frames (select.hip) skip work whose outcome the host can prove per frame and per camera.  Host-compilable
// without HIP (tests/test_ka_cert_cpu.py), like px_round.hpp and kc_lanes.hpp.  Compile with -ffp-contract=off.
//
// The kernel back-projects every valid pixel (j, i, z) of a camera's own image, transforms it by the pose and asks Frustum::ContainPoint whether
// the point lies in that same camera's frustum (CubeHandler.cpp:116-145).  Two things are decided here, on the host:
//
//  1. ka_quot(b): the quotient RN(n / b) by a camera constant b (fx, fy, depth_scale) in three operations with the stored reciprocal
//     y = RN(1 / b):   q0 = RN(n y),  r = fma(-b, q0, n),  q = fma(r, y, q0)   (ka_div_const; div_int_rcp in volume_core.hpp is the same sequence
//     for integer b).  Markstein's division theorem covers the case of a q0 within one ulp of n / b; q0 = RN(n RN(1/b)) can be 1.3 ulp off for an
//     unlucky b, so the flag is not taken from the theorem alone but from an exact enumeration of the only numerators that can go wrong:
//       Scale b and n to [1, 2): b = B 2^-23, n = N 2^-23, 2^23 <= B, N < 2^24, Q = N / B in (1/2, 2), delta = y - 1/b with |delta| <= 2^-25 (y is the
//       NEAREST float to 1/b in [1/2, 1]: checked exactly below, b y - 1 is exact in double).  |Q - q0| <= n |delta| + 2^-24 < 2^-23, so
//       r' = n - b q0 has |r'| < 2^-22; the FMA delivers r = RN(r') with |r - r'| <= 2^-47 (r' is a multiple of 2^-48 below 2^-22: at most two bits
//       too long).  The last FMA rounds V = q0 + r y ONCE, and V = Q + r' delta + (r - r') y: |V - Q| < 2^-47 + 2^-47 = 2^-46.
//       RN(V) differs from RN(Q) only if a rounding midpoint m lies between them (or on V): |Q - m| < 2^-46.  Midpoints are odd multiples K 2^-25
//       (Q below 1) or K 2^-24 (Q in [1, 2)), K in (2^24, 2^25) both times: |Q - m| = |N 2^25 - B K| / (B 2^25) > |D| 2^-49 with the integer
//       D = N 2^25 - B K (never 0: a quotient of two floats is no midpoint), resp. > |D| 2^-48 with D = N 2^24 - B K.  So only |D| < 8 (resp. < 4) can
//       fail.  For each such D the congruence B K = -D (mod 2^25, resp. 2^24) has at most 8 (resp. 16) solutions K in that range, none unless the
//       power of two in B divides D; each gives one N = (B K + D) / 2^25 (resp. 2^24).  ka_quot runs the float sequence on exactly those
//       numerators (ka_detail::risky_numerators: a few dozen) and compares with the IEEE quotient.  The significands decide: inside the window
//       below no operation leaves the normal range, and scaling n by a power of two scales q0, r and q exactly.
//       (For Q in [1, 2) the enumeration is a second line: there n |delta| < 2^-24 is half an ulp, q0 is within one ulp of Q, and Markstein's
//       theorem applies as it stands.  The 1.3 ulp case is Q in (1/2, 1), n close below b.)
//       The flag is a safety net: none of the divisors the tests draw is refused by the enumeration; what it buys is that an arbitrary camera
//       constant needs no argument beyond the one above.
//     The window, as binary exponents lo <= exponent(n) <= hi, is where q0, r and q are 0 or normal: r is a multiple of ulp(b) ulp(q0) >=
//     2^(e_n - 47 + tz), tz = trailing zero bits of B, which is normal from e_n = -79 - tz on; q0 >= 2^(e_n - e_b - 1) is normal from e_n = e_b - 125 on;
//     q0 stays finite up to e_n = 127 (b >= 1) or 127 + e_b (b < 1).  n = +0 gives q = +0, the IEEE quotient.  (n = -0 would give +0 where IEEE gives -0:
//     the kernel's numerators (j - cx) z, z > 0, are never -0: a float difference that vanishes is +0.)
//
//  2. ka_certificate(pose, planes, cam, near, far): a pixel rectangle and a depth interval such that every pixel inside with a depth inside is
//     in the frustum, by a margin that beats every rounding of the kernel's float chain.  Then ContainPoint's six planes, the fourth row of the pose
//     product and the division by it need not run: the answer is "inside" and w is exactly 1.
//     Plane images.  With M = pose (rows 0..2: R | t), a plane (n, d) and a camera-space point P:  n . (R P + t) + d = (R^T n) . P + (n . t + d)
//     -- an identity for ANY R, orthogonal or not.  P = z (a, b, 1), a = (j - cx) / fx, b = (i - cy) / fy, so the real distance of the real
//     back-projection is  dist_k = z g_k(j, i) + dc_k,  g_k = nc_k0 a + nc_k1 b + nc_k2,  nc_k = R^T n_k,  dc_k = n_k . t + d_k:  linear in (j, i),
//     and for a fixed pixel linear in z.  Its minimum over a pixel rectangle times a depth interval is at a corner.
//     Error bound.  u = 2^-24, gamma_k = k u / (1 - k u).  The kernel forms x = RN(RN(RN(j - cx) z) / fx): three roundings (the short quotient is
//     the same float), |x - X| <= gamma_3 |X|; likewise y.  q_r = ((M_r0 x + M_r1 y) + M_r2 z) + M_r3 * 1: the x and y terms pass a product and
//     three sums, the z term a product and two, t_r one sum:  |q_r - Q_r| <= e_r = gamma_7 S_r z + gamma_1 |t_r|,  S_r = |M_r0| A + |M_r1| Bm + |M_r2|,
//     A, Bm = the largest |a|, |b| of the image.  p = q (w = 1, below).  dist = fl((n_0 p_0 + (n_1 p_1 + n_2 p_2)) + d): every term at most a
//     product and three sums, d one sum:  |dist_fl - dist| <= sum_r |n_r| (gamma_4 (|P_r| + e_r) + e_r) + gamma_1 |d|,  |P_r| <= S_r z + |t_r|.  So
//       E(z) = E0 + E1 z,   E1 = (gamma_4 + (1 + gamma_4) gamma_7) sum_r |n_r| S_r,   E0 = (gamma_4 + (1 + gamma_4) gamma_1) sum_r |n_r| |t_r| + gamma_1 |d|,
//     plus 2^-44 of the same magnitudes for the double arithmetic here and 2^-120 for products that underflow (|M|, |n| <= 2 is checked).
//     The certificate asks  z (g_k - E1_k) + dc_k - E0_k > 0  at the four corners of the rectangle and both ends of the depth interval, for all
//     six planes: there dist_fl >= dist - E > 0, which is ContainPoint's "inside" without its "== 0" exit.  The depth interval comes from the near
//     and far planes over the whole image, the rectangle from the four side planes at z_lo (a side plane's margin grows with z; what does not is
//     dc_k - E0_k, the rounding of t in the plane's own d), and the final test is run on the result as it stands, so a slip in choosing the
//     intervals costs a certificate, never a wrong one.
//     w = 1.  q_3 = ((M_30 x + M_31 y) + M_32 z) + M_33 * 1 with the bottom row exactly (0, 0, 0, 1) and finite x, y, z is (0 + 0) + 0 + 1 = 1.
//     No certificate (the empty rectangle j_lo > j_hi): a bottom row that is not (0, 0, 0, 1), a non-finite entry, |R^T R - I| > kKaOrthoTol in some
//     entry (a pose that is no rigid motion is not what this path is for; the bound itself does not need orthogonality), margins that cannot be
//     met, or numerators (j - cx) z, (i - cy) z of the rectangle that are not all +0 or inside the quotient windows.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "px_round.hpp" // OP_HD

struct KaQuot {
    float y;    // RN(1 / b)
    int ok;     // the three-operation quotient is RN(n / b) for every n of the window
    int lo, hi; // the window: lo <= binary exponent of n <= hi (n = +0 also allowed)
};
struct KaCert { int j_lo, j_hi, i_lo, i_hi; float z_lo, z_hi; }; // columns, rows, depths (all inclusive); j_lo > j_hi: no certificate
struct KaCam { KaQuot qx, qy, qd; };                             // fx, fy, depth_scale

constexpr double kKaOrthoTol = 1.0e-4;

OP_HD float ka_div_const(float n, float b, float y) {
    const float q0 = n * y;
    const float r = __builtin_fmaf(-b, q0, n);
    return __builtin_fmaf(r, y, q0);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
namespace ka_detail {
inline uint32_t bits_of(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
inline int exponent_of(float f) { return (int)((bits_of(f) >> 23) & 0xffu) - 127; }
// inverse of an odd a modulo 2^32 (Newton: five steps double 3 correct bits to 48)
inline uint32_t inv_odd(uint32_t a) { uint32_t x = a; for (int k = 0; k < 5; ++k) x *= 2u - a * x; return x; }
constexpr int kKaMaxD = 8; // |D| <= 8 is enumerated: a superset of the |D| < 8 (quotients below 1) and |D| < 4 (above) that can fail
// Calls f(N) for every significand 2^23 <= N < 2^24 of a numerator whose quotient N / B (2^23 <= B < 2^24) lies within |D| <= kKaMaxD of a rounding
// midpoint: kind 0, quotients in (1/2, 1): midpoints K 2^-25, D = N 2^25 - B K; kind 1, quotients in [1, 2): midpoints K 2^-24, D = N 2^24 - B K; K odd in
// (2^24, 2^25) both times.  B K = -D modulo 2^sh fixes K modulo 2^(sh - tz) when 2^tz (the power of two in B) divides D, and has no solution otherwise.
// tests/test_ka_cert_cpu.py compares the set with a brute force over all 2^23 numerators.
template <class F>
inline void risky_numerators(uint32_t B, F&& f) {
    const int tz = __builtin_ctz(B);
    if (tz > 3) return; // no 0 < |D| <= 8 is a multiple of 16
    const uint32_t Bo = B >> tz; // odd
    for (int kind = 0; kind < 2; ++kind) {
        const int sh = kind == 0 ? 25 : 24;
        const uint64_t m2 = (1ull << sh) >> tz; // K is determined modulo 2^(sh - tz)
        for (int D = -kKaMaxD; D <= kKaMaxD; ++D) {
            if (D == 0 || (D & ((1 << tz) - 1)) != 0) continue;
            const int64_t rhs = -(int64_t)(D / (1 << tz));
            const uint64_t K0 = ((uint64_t)(uint32_t)((uint32_t)rhs * inv_odd(Bo))) & (m2 - 1);
            for (uint64_t K = K0; K < (1ull << 25); K += m2) {
                if (K < (1ull << 24) || (K & 1ull) == 0) continue;
                const int64_t num = (int64_t)((uint64_t)B * K) + D; // = N 2^sh
                if ((num & (int64_t)((1ull << sh) - 1)) != 0) continue;
                const int64_t N = num >> sh;
                if (N >= (1 << 23) && N < (1 << 24)) f((uint32_t)N);
            }
        }
    }
}
} // namespace ka_detail

inline KaQuot ka_quot(float b) {
    using namespace ka_detail;
    KaQuot q{0.0f, 0, 0, -1};
    if (!(b > 0.0f) || !std::isfinite(b) || (bits_of(b) >> 23) == 0u) return q; // positive normal divisors only
    const float y = 1.0f / b; // IEEE division; that it IS the nearest float is checked exactly, not assumed
    q.y = y;
    if (!std::isfinite(y) || (bits_of(y) >> 23) == 0u) return q;
    const double by = std::fma((double)b, (double)y, -1.0); // exact: a multiple of 2^-47 (scaled) below 2^-23
    const double bl = std::fma((double)b, (double)std::nextafterf(y, 0.0f), -1.0), bh = std::fma((double)b, (double)std::nextafterf(y, INFINITY), -1.0);
    if (!(std::fabs(by) < std::fabs(bl) && std::fabs(by) < std::fabs(bh))) return q;
    const uint32_t frac = bits_of(b) & 0x7fffffu;
    if (frac == 0x7fffffu) return q; // the all-ones significand: 1 / b sits next to a midpoint (|delta| at its maximum)
    const int eb = exponent_of(b);
    const uint32_t B = frac | 0x800000u;
    const int tz = __builtin_ctz(B);
    // the numerators that can round differently (see the head of the file), tried at the scale of b itself
    const float bs = std::ldexp(1.0f, eb - 23); // N bs = the numerator with significand N and b's exponent
    bool same = true;
    risky_numerators(B, [&](uint32_t N) {
        const float n = (float)N * bs;
        same = same && bits_of(ka_div_const(n, b, y)) == bits_of(n / b) && bits_of(ka_div_const(-n, b, y)) == bits_of(-n / b);
    });
    if (!same) return q;
    q.lo = eb - 125 > -79 - tz ? eb - 125 : -79 - tz;
    q.hi = eb >= 0 ? 127 : 127 + eb; // n < 2^(128 + e_b), y <= 2^-e_b (and below it by a factor 1 - 2^-24 unless b is a power of two): n y stays finite
    q.ok = q.lo <= q.hi;
    return q;
}

inline KaCam ka_cam(float fx, float fy, float depth_scale) { return KaCam{ka_quot(fx), ka_quot(fy), ka_quot(depth_scale)}; }

// One axis of the rectangle's numerators (j - c) z, j in [lo, hi], z in [z_lo, z_hi]: all +0 or inside the window of Q?
inline bool ka_axis_in_window(float c, int lo, int hi, float z_lo, float z_hi, const KaQuot& Q) {
    double amin = INFINITY, amax = 0.0;
    const double fl = std::floor((double)c);
    const double cand[5] = {(double)lo, (double)hi, fl - 1.0, fl, fl + 1.0};
    for (double j : cand) {
        if (j < lo || j > hi) continue;
        const float a = (float)j - c; // the kernel's own difference
        const double m = std::fabs((double)a);
        if (m != 0.0 && m < amin) amin = m;
        if (m > amax) amax = m;
    }
    if (amax == 0.0) return true; // every numerator is +0
    // one ulp of slack on each side for the product's rounding
    return amin * (double)z_lo >= std::ldexp(1.0, Q.lo + 1) && amax * (double)z_hi < std::ldexp(1.0, Q.hi);
}

// planes: the 24 floats of frustum_planes (top, left, right, bottom, near, far), pose: the 16 floats they were made from.
// e_scale scales the error bound E (1 in the product; the host test sets 0 to show that its sweep can fail), whole_image skips the rectangle.
inline KaCert ka_certificate(const float pose[16], const float planes[24], float fx, float fy, float cx, float cy, int width, int height, const KaCam& Q,
                             double e_scale = 1.0, bool whole_image = false) {
    const KaCert none{0, -1, 0, -1, 1.0f, 0.0f};
    if (!Q.qx.ok || !Q.qy.ok || width <= 0 || height <= 0) return none;
    if (!(pose[12] == 0.0f && pose[13] == 0.0f && pose[14] == 0.0f && pose[15] == 1.0f)) return none;
    double mag = 0.0;
    for (int k = 0; k < 12; ++k) mag += std::fabs((double)pose[k]);
    for (int k = 0; k < 24; ++k) mag += std::fabs((double)planes[k]);
    if (!std::isfinite(mag) || !(fx > 0.0f) || !(fy > 0.0f) || !std::isfinite(cx) || !std::isfinite(cy)) return none;
    double M[3][4];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) M[r][c] = (double)pose[4 * r + c];
    for (int a = 0; a < 3; ++a)
        for (int b = a; b < 3; ++b) {
            const double s = M[0][a] * M[0][b] + M[1][a] * M[1][b] + M[2][a] * M[2][b] - (a == b ? 1.0 : 0.0);
            if (!(std::fabs(s) <= kKaOrthoTol)) return none;
        }
    const double u = 0x1p-24;
    const double g1 = u / (1 - u), g4 = 4 * u / (1 - 4 * u), g7 = 7 * u / (1 - 7 * u);
    const double A = std::fmax(std::fabs(0.0 - (double)cx), std::fabs((double)(width - 1) - (double)cx)) / (double)fx;
    const double Bm = std::fmax(std::fabs(0.0 - (double)cy), std::fabs((double)(height - 1) - (double)cy)) / (double)fy;
    double c0[6], c1[6], c2[6], dc[6], E0[6], E1[6]; // g_k = c0 (j - cx) + c1 (i - cy) + c2
    for (int k = 0; k < 6; ++k) {
        const double n[3] = {(double)planes[4 * k], (double)planes[4 * k + 1], (double)planes[4 * k + 2]}, d = (double)planes[4 * k + 3];
        if (std::fabs(n[0]) > 2.0 || std::fabs(n[1]) > 2.0 || std::fabs(n[2]) > 2.0) return none;
        double nc[3], sS = 0.0, sT = 0.0;
        for (int c = 0; c < 3; ++c) nc[c] = M[0][c] * n[0] + M[1][c] * n[1] + M[2][c] * n[2];
        for (int r = 0; r < 3; ++r) {
            sS += std::fabs(n[r]) * (std::fabs(M[r][0]) * A + std::fabs(M[r][1]) * Bm + std::fabs(M[r][2]));
            sT += std::fabs(n[r]) * std::fabs(M[r][3]);
        }
        c0[k] = nc[0] / (double)fx; c1[k] = nc[1] / (double)fy; c2[k] = nc[2];
        dc[k] = (n[0] * M[0][3] + n[1] * M[1][3] + n[2] * M[2][3]) + d;
        E1[k] = e_scale * ((g4 + (1 + g4) * g7) * sS + 0x1p-44 * sS);
        E0[k] = e_scale * ((g4 + (1 + g4) * g1) * sT + g1 * std::fabs(d) + 0x1p-44 * (sT + std::fabs(d)) + 0x1p-120);
    }
    const auto g = [&](int k, double j, double i) { return c0[k] * (j - (double)cx) + c1[k] * (i - (double)cy) + c2[k]; };
    const auto gmin = [&](int k, int jl, int jh, int il, int ih) {
        return std::fmin(std::fmin(g(k, jl, il), g(k, jh, il)), std::fmin(g(k, jl, ih), g(k, jh, ih)));
    };
    // depth interval: every plane whose slope over the whole image has a definite sign bounds z from one side (near: below, far: above)
    double zl = 0x1p-60, zh = 0x1p60;
    for (int k = 4; k < 6; ++k) {
        const double s = gmin(k, 0, width - 1, 0, height - 1) - E1[k], off = dc[k] - E0[k];
        if (s > 0) { if (off < 0) zl = std::fmax(zl, -off / s); }
        else if (s < 0) { if (!(off > 0)) return none; zh = std::fmin(zh, off / -s); }
        else if (!(off > 0)) return none;
    }
    float z_lo = (float)zl, z_hi = (float)zh;
    if ((double)z_lo < zl) z_lo = std::nextafterf(z_lo, INFINITY);
    if ((double)z_hi > zh) z_hi = std::nextafterf(z_hi, 0.0f);
    z_lo = std::nextafterf(z_lo, INFINITY); z_hi = std::nextafterf(z_hi, 0.0f); // strict inequalities, with room for the divisions above
    if (!(z_lo > 0.0f) || !(z_lo <= z_hi)) return none;
    if (whole_image) return KaCert{0, width - 1, 0, height - 1, z_lo, z_hi}; // (the host test's control: no rectangle, no final test)
    // rectangle: a side plane leans on one image axis; the other axis is charged at its worst over the whole image
    int jl = 0, jh = width - 1, il = 0, ih = height - 1;
    for (int k = 0; k < 4; ++k) {
        const double need = E1[k] + std::fmax((E0[k] - dc[k]) / (double)z_lo, 0.0) + 0x1p-40;
        if (std::fabs(c0[k]) * width >= std::fabs(c1[k]) * height) {
            if (c0[k] == 0.0) return none;
            const double w = std::fmin(c1[k] * (0.0 - (double)cy), c1[k] * ((double)(height - 1) - (double)cy));
            const double lim = (double)cx + (need - c2[k] - w) / c0[k];
            if (!std::isfinite(lim) || std::fabs(lim) > 1.0e9) return none;
            if (c0[k] > 0) jl = std::max(jl, (int)std::ceil(lim)); else jh = std::min(jh, (int)std::floor(lim));
        } else {
            const double w = std::fmin(c0[k] * (0.0 - (double)cx), c0[k] * ((double)(width - 1) - (double)cx));
            const double lim = (double)cy + (need - c2[k] - w) / c1[k];
            if (!std::isfinite(lim) || std::fabs(lim) > 1.0e9) return none;
            if (c1[k] > 0) il = std::max(il, (int)std::ceil(lim)); else ih = std::min(ih, (int)std::floor(lim));
        }
    }
    // the certificate's statement, checked on the intervals as they stand (one retry a pixel further in)
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (jl > jh || il > ih) return none;
        bool ok = true;
        for (int k = 0; k < 6 && ok; ++k) {
            const double s = gmin(k, jl, jh, il, ih) - E1[k], off = dc[k] - E0[k];
            ok = s * (double)z_lo + off > 0 && s * (double)z_hi + off > 0;
        }
        if (ok) {
            if (!ka_axis_in_window(cx, jl, jh, z_lo, z_hi, Q.qx) || !ka_axis_in_window(cy, il, ih, z_lo, z_hi, Q.qy)) return none;
            return KaCert{jl, jh, il, ih, z_lo, z_hi};
        }
        ++jl; --jh; ++il; --ih;
    }
    return none;
}
