"""csrc/px_round.hpp px_certified_folded with the UNREFINED reciprocal -- what project_pixel_uv<true> evaluates, restated on the host.

The device forms t'' = fma(f*X, y0, kb) with y0 = v_rcp_f32(Z) as the hardware delivers it (no Newton step) and kb = c + 0.5 + B2, takes
trunc(t'') as the pixel and certifies the lane with fract(t'') > h2.  px_cert_bound_folded's only hypothesis about y0 is |1 - Z y0| <= kPxRcpErr
(d_rcp; tests/test_kc_diet_gpu.py holds the device to it over every significand).  Same cameras and quotient families as
tests/test_px_folded_cpu.py:
  * abstract: t'' = RN(a (1 + e) + kb) with |e| up to 2^-24 + d_rcp (a = RN(q) is off by 2^-24, q y0 Z by d_rcp), extremes included;
  * the device's own sequence in fp32 (fmaf, IEEE division for the reference quotient), with y0 = the correctly rounded reciprocal perturbed
    by anything that keeps |1 - Z y0| <= d_rcp (the extremes of that interval among them), and no refinement.
Quotients: dense over the image and its surroundings, within 64 ulp of every integer and image border of the sum (and of the points a margin B
away from them, where the certificate flips), any bit pattern, specials.  A certified lane must give exactly what the reference's double
formula (px_round_dp + the bounds test) gives; lanes whose real sum lies in (-1, 0) (pixel 0) and in (-2, -1) (outside) must be among the
certified ones.

That the test can see an error: with the threshold h2 halved the same run must report mismatches; and with the margin as shipped but a
reciprocal off by 2 d_rcp it must report mismatches too -- the bound is not so slack that the hypothesis it rests on goes unseen."""
import os
import subprocess
import tempfile
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = textwrap.dedent(r'''
    #include <cstdio>
    #include <cstdint>
    #include <cstring>
    #include <cmath>
    #include "px_round.hpp"
    static uint32_t st = 2463534242u;
    static uint32_t rnd() { st ^= st << 13; st ^= st >> 17; st ^= st << 5; return st; }
    static double unif() { return (rnd() >> 8) * (1.0 / 16777216.0); }
    static float bump(float x, int k) { int32_t b; memcpy(&b, &x, 4); b += k; memcpy(&x, &b, 4); return x; }
    // [0]: the certificate as px_axis gives it, [1]: its threshold halved, [2], [3]: as given, on sums formed with a reciprocal off by 2 d_rcp, by 3 d_rcp
    long n = 0, ncert[4] = {0, 0, 0, 0}, bad[4] = {0, 0, 0, 0}, cert_m10 = 0, cert_m21 = 0;
    static void check(float a, float t2, float c, int extent, const PxAxis& s, const char* what, int h) {
        if (h == 0) ++n;
        PxAxis q = s;
        if (h == 1) q.h2 = s.h2 * 0.5f;
        if (!px_certified_folded(t2, q)) return;
        ++ncert[h];
        const int r = px_round_dp(a, c);
        const bool in_ref = r >= 0 && r < extent;
        const int u = (int)t2; // |t''| < 2^23 on a certified lane
        const bool in_fast = (unsigned)u < (unsigned)extent;
        const bool ok = in_ref == in_fast && (!in_ref || u == r);
        if (!ok) {
            if (h == 0 && bad[0] < 8) printf("%s: c=%.9g extent=%d a=%.9g t''=%.9g ref=%d fast=%d\n", what, c, extent, a, t2, r, u);
            ++bad[h];
        }
        if (h == 0 && ok) {
            const double t = (double)a + 0.5 + (double)c;
            if (t > -1.0 && t < 0.0) ++cert_m10;
            if (t > -2.0 && t < -1.0) ++cert_m21;
        }
    }
    // the float nearest to (1 + d) / z: |1 - z y0| is d up to y0's own rounding; pulled back inside the interval when that rounding left it
    static float rcp_off(float z, double d, double lim) {
        float y0 = (float)((1.0 + d) / (double)z);
        for (int k = 0; k < 2 && fabs(1.0 - (double)z * (double)y0) > lim; ++k) y0 = bump(y0, (fabs((double)z * (double)y0) > 1.0) ? -1 : 1);
        return y0;
    }
    int main() {
        const float cs[6] = {318.771f, 238.447f, 318.6f, 255.3f, 262144.3f, 1.25f};
        const float fs[6] = {514.817f, 515.375f, 517.3f, 516.5f, 300000.0f, 2.0f};
        const int ext[6] = {640, 480, 640, 480, 1 << 19, 3};
        const double D = kPxRcpErr;
        const double E = 0x1p-24 + D; // |t'' - RN(q) - kb| / |q| before t'' is rounded
        if (!(D >= 0x1p-24 && D <= 0x1p-20)) { printf("d_rcp=%.9g\n", D); return 2; }
        int certifiable = 0;
        long inside = 0;
        for (int k = 0; k < 6; ++k) {
            const float c = cs[k], f = fs[k]; const int extent = ext[k];
            const PxAxis s = px_axis(c, extent);
            if (!s.exact) { if (s.h2 != 2.0f) { printf("h2=%.9g on an inexact axis\n", s.h2); return 2; } continue; } // (the kernels take the double formula)
            const double K = (double)c + 0.5, B2 = (double)s.kb - K, B = px_cert_bound_folded((double)extent + 1.0, K);
            if (!(B2 >= B && B2 <= 0.25 && (double)s.h2 >= B2 + B && (double)s.h2 < (B2 + B) * (1.0 + 0x1p-22) && B2 - B < (double)(nextafterf(s.kb, INFINITY) - s.kb) &&
                  s.h2 < (extent <= 4096 ? 0.001f : 1.0f))) { printf("kb=%.9g h2=%.9g for c=%.9g extent=%d (B=%.9g)\n", s.kb, s.h2, c, extent, B); return 2; }
            if (k == 0) printf("B(640 px, c=%.9g) = %.6g, h2 = %.6g\n", c, B, s.h2);
            ++certifiable;
            for (long it = 0; it < 1500000; ++it) {
                float a; const int mode = it % 6;
                if (mode == 0) { uint32_t b = rnd(); memcpy(&a, &b, 4); }                               // any bit pattern
                else if (mode < 3) a = (float)((unif() * 1.2 - 0.1) * (extent + 2) - 2.5 * (mode - 1) * unif() - K);  // pixel scale (and, every other time, down to t = -2.5 also on the tiny image)
                else {                                                                                  // +-64 ulp of an integer / border of the sum, or of the point +-B away
                    const int kk = mode == 3 ? (int)(rnd() % (unsigned)(extent + 41)) - 20 : ((rnd() & 1) ? ((rnd() & 1) ? -1 : 0) : extent);
                    const double off = (it / 6) % 3 == 0 ? 0.0 : ((it / 6) % 3 == 1 ? B : -B);
                    a = bump((float)((double)kk + off - K), (int)(rnd() % 129u) - 64);
                }
                // abstract model: the extremes and a random point of the relative error interval; and the same with 2 d_rcp in d_rcp's place
                const double e3[3] = {-E, E, (2.0 * unif() - 1.0) * E};
                for (double e : e3) {
                    check(a, (float)((double)a * (1.0 + e) + (double)s.kb), c, extent, s, "abstract", 0);
                    check(a, (float)((double)a * (1.0 + e) + (double)s.kb), c, extent, s, "abstract", 1);
                }
                const double e2[2] = {-(0x1p-24 + 2.0 * D), 0x1p-24 + 2.0 * D};
                for (double e : e2) check(a, (float)((double)a * (1.0 + e) + (double)s.kb), c, extent, s, "abstract 2d", 2);
                const double e3d[2] = {-(0x1p-24 + 3.0 * D), 0x1p-24 + 3.0 * D};
                for (double e : e3d) check(a, (float)((double)a * (1.0 + e) + (double)s.kb), c, extent, s, "abstract 3d", 3);
                // the device sequence: Z, and X such that f*X/Z is near a; the raw reciprocal anywhere within d_rcp, extremes every other time; no refinement
                const float z = (float)((0.2 + 8.0 * unif()) * ((rnd() & 7) ? 1.0 : -1.0));
                const float X = (float)((double)a * z / f);
                const float nx = f * X, A = nx / z;
                const int pick = (int)(rnd() % 4u);
                const double d = pick == 0 ? D : (pick == 1 ? -D : (2.0 * unif() - 1.0) * D);
                const float y0 = rcp_off(z, d, D);
                if (fabs(1.0 - (double)z * (double)y0) <= D) { ++inside; check(A, fmaf(nx, y0, s.kb), c, extent, s, "device", 0); check(A, fmaf(nx, y0, s.kb), c, extent, s, "device", 1); }
                const float y2 = rcp_off(z, pick & 1 ? -2.0 * D : 2.0 * D, 2.0 * D);
                check(A, fmaf(nx, y2, s.kb), c, extent, s, "device 2d", 2);
                const float y3 = rcp_off(z, pick & 1 ? -3.0 * D : 3.0 * D, 3.0 * D);
                check(A, fmaf(nx, y3, s.kb), c, extent, s, "device 3d", 3);
            }
            // sums no lane may be certified on, whatever the quotient
            const float never[12] = {0.0f, -0.0f, -1.0f, 1.0f, (float)extent, INFINITY, -INFINITY, NAN, 8388608.0f, -8388609.0f, 1e9f, -3e38f};
            for (float t2 : never) if (px_certified_folded(t2, s)) { printf("t''=%.9g certified\n", t2); return 2; }
            // special quotients through the abstract model
            const float sp[10] = {0.0f, -0.0f, INFINITY, -INFINITY, NAN, 1e-45f, -1e-45f, 3e38f, -3e38f, 1e9f};
            for (float a : sp) check(a, (float)((double)a + (double)s.kb), c, extent, s, "specials", 0);
        }
        // principal points whose fast path may not be certified
        if (px_axis(318.5f, 640).h2 != 2.0f || px_axis(319.5f, 640).h2 != 2.0f || px_axis(3.0e6f, 640).h2 != 2.0f) { printf("refusal\n"); return 2; }
        printf("%d %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld\n", certifiable, n, ncert[0], bad[0], cert_m10, cert_m21, ncert[1], bad[1], ncert[2], bad[2], inside, ncert[3], bad[3]);
        return bad[0] != 0;
    }
''')


_run = {}


def _figures():
    """The program's figures, computed once."""
    if not _run:
        with tempfile.TemporaryDirectory() as td:
            cpp, exe = os.path.join(td, "t.cpp"), os.path.join(td, "t")
            open(cpp, "w").write(SRC)
            subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "onepiece_amd", "csrc"), cpp, "-o", exe])
            out = subprocess.run([exe], capture_output=True, text=True)
        print(out.stdout)
        assert out.returncode == 0, out.stdout
        keys = ("certifiable", "n", "ncert", "bad", "m10", "m21", "ncert_half", "bad_half", "ncert_2d", "bad_2d", "inside", "ncert_3d", "bad_3d")
        _run.update(zip(keys, map(int, out.stdout.split()[-len(keys):])))
    return _run


def test_unrefined_reciprocal_certificate_equals_double_formula_and_a_halved_margin_does_not():
    r = _figures()
    assert r["certifiable"] == 5 and r["bad"] == 0   # the TUM camera's y axis (cy = 255.3) has inexact thresholds: double formula
    assert r["n"] > 2.9e7 and r["ncert"] > 0.5 * r["n"]   # the certificate accepts most lanes, specials and near-threshold ones aside
    assert r["inside"] == 5 * 1500000                # every perturbed reciprocal of the device sequence lies within d_rcp
    assert r["m10"] > 1000 and r["m21"] > 1000       # certified lanes left of pixel 0: sums in (-1, 0) are pixel 0, sums in (-2, -1) are outside
    assert r["ncert_half"] > r["ncert"] and r["bad_half"] > 100  # with half the margin lanes are certified whose pixel is wrong, and the test sees them


def test_a_reciprocal_off_by_twice_d_rcp_breaks_the_shipped_margin():
    """The margin as shipped, sums formed with a reciprocal off by 2 d_rcp (abstract extremes and device sequence): lanes are certified whose pixel
    is wrong, so the bound is not so slack that its hypothesis goes unseen.  (With the rounding of t'' charged as 2^-24 S instead of half an ulp,
    2^-24 P, this count was 0 of 19 118 382 and the first wrong pixels appeared at 2.25 d_rcp: px_round.hpp, px_cert_bound_folded.)"""
    r = _figures()
    assert r["ncert_2d"] > 0 and r["bad_3d"] > r["bad_2d"]
    assert r["bad_2d"] > 0
