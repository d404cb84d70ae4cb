"""csrc/px_round.hpp px_certified_folded -- the one-compare certificate project_pixel<true> uses, restated on the host.

The device forms t'' = fma(f*X, y, kb) with y the once-refined v_rcp of Z and kb = c + 0.5 + B2 (the certificate's margin folded into the
FMA's constant), takes trunc(t'') as the pixel and certifies the lane with fract(t'') > h2.  Same cameras and error models as
tests/test_px_certified_cpu.py:
  * abstract: t'' = RN(a (1 + e) + kb) with |e| up to the derived relative bound 2^-24 + (2^-24 + 2^-39), extremes included;
  * the device's own sequence in fp32 (fmaf, IEEE division for the reference quotient) with the reciprocal v_rcp perturbed by up to 4 ulp.
Quotients: dense over the image and its surroundings, within 64 ulp of every integer and image border of the sum (and of the points a margin
away from them, where the certificate flips), and any bit pattern.  A certified lane must give exactly what the reference's double formula
(px_round_dp + the bounds test) gives; lanes whose real sum lies in (-1, 0) (pixel 0 by truncation toward zero) and in (-2, -1) (pixel -1:
outside) must be among the certified ones.

That the test can see an error: the same run with the compare's margin halved (kb as px_axis gives it, the threshold h2 / 2) must report
mismatches."""
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
    // [0]: the certificate as px_axis gives it, [1]: its threshold halved
    long n = 0, ncert[2] = {0, 0}, bad[2] = {0, 0}, cert_m10 = 0, cert_m21 = 0;
    // reference pixel (in-image or not) vs the fast path's trunc(t'') on a certified lane
    static void check(float a, float t2, float c, int extent, const PxAxis& s, const char* what) {
        ++n;
        for (int h = 0; h < 2; ++h) {
            PxAxis q = s;
            if (h) q.h2 = s.h2 * 0.5f;
            if (!px_certified_folded(t2, q)) continue;
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
    }
    int main() {
        const float cs[6] = {318.771f, 238.447f, 318.6f, 255.3f, 262144.3f, 1.25f};
        const float fs[6] = {514.817f, 515.375f, 517.3f, 516.5f, 300000.0f, 2.0f};
        const int ext[6] = {640, 480, 640, 480, 1 << 19, 3};
        const double E = 0x1p-24 + (0x1p-24 + 0x1p-39); // |t'' - RN(q) - kb| / |q| before t'' is rounded
        int certifiable = 0;
        for (int k = 0; k < 6; ++k) {
            const float c = cs[k], f = fs[k]; const int extent = ext[k];
            const PxAxis s = px_axis(c, extent);
            if (!s.exact) { if (s.h2 != 2.0f) { printf("h2=%.9g on an inexact axis\n", s.h2); return 2; } continue; } // (the kernels take the double formula)
            const double K = (double)c + 0.5, B2 = (double)s.kb - K, B = px_cert_bound_folded((double)extent + 1.0, K);
            // kb - K >= B, h2 >= B2 + B, and no wider than one ulp of kb (and of h2) more than that; the accepted share of a unit interval
            if (!(B2 >= B && B2 <= 0.25 && (double)s.h2 >= B2 + B && (double)s.h2 < (B2 + B) * (1.0 + 0x1p-22) && B2 - B < (double)(nextafterf(s.kb, INFINITY) - s.kb) &&
                  s.h2 < (extent <= 4096 ? 0.001f : 1.0f))) { printf("kb=%.9g h2=%.9g for c=%.9g extent=%d (B=%.9g)\n", s.kb, s.h2, c, extent, B); return 2; }
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
                // abstract model: the extremes and a random point of the relative error interval
                const double e3[3] = {-E, E, (2.0 * unif() - 1.0) * E};
                for (double e : e3) check(a, (float)((double)a * (1.0 + e) + (double)s.kb), c, extent, s, "abstract");
                // the device sequence: Z, and X such that f*X/Z is near a; v_rcp perturbed by up to 4 ulp
                const float z = (float)((0.2 + 8.0 * unif()) * ((rnd() & 7) ? 1.0 : -1.0));
                const float X = (float)((double)a * z / f);
                const float nx = f * X, A = nx / z;
                const float y0 = bump(1.0f / z, (int)(rnd() % 9u) - 4);  // |1 - z y0| < 2^-20, what px_cert_bound assumes
                const float e = fmaf(-z, y0, 1.0f), y = fmaf(e, y0, y0);
                check(A, fmaf(nx, y, s.kb), c, extent, s, "device");
            }
            // sums no lane may be certified on, whatever the quotient: fract 0 (integers, among them -1, whose truncation is not pixel 0's; +-0; everything
            // from 2^23 on) and fract NaN
            const float never[12] = {0.0f, -0.0f, -1.0f, 1.0f, (float)extent, INFINITY, -INFINITY, NAN, 8388608.0f, -8388609.0f, 1e9f, -3e38f};
            for (float t2 : never) if (px_certified_folded(t2, s)) { printf("t''=%.9g certified\n", t2); return 2; }
            // special quotients through the abstract model
            const float sp[10] = {0.0f, -0.0f, INFINITY, -INFINITY, NAN, 1e-45f, -1e-45f, 3e38f, -3e38f, 1e9f};
            for (float a : sp) check(a, (float)((double)a + (double)s.kb), c, extent, s, "specials");
        }
        // principal points whose fast path may not be certified
        if (px_axis(318.5f, 640).h2 != 2.0f || px_axis(319.5f, 640).h2 != 2.0f || px_axis(3.0e6f, 640).h2 != 2.0f) { printf("refusal\n"); return 2; }
        printf("%d %ld %ld %ld %ld %ld %ld %ld\n", certifiable, n, ncert[0], bad[0], cert_m10, cert_m21, ncert[1], bad[1]);
        return bad[0] != 0;
    }
''')


def test_folded_certificate_equals_double_formula_and_a_halved_margin_does_not():
    with tempfile.TemporaryDirectory() as td:
        cpp, exe = os.path.join(td, "t.cpp"), os.path.join(td, "t")
        open(cpp, "w").write(SRC)
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "onepiece_amd", "csrc"), cpp, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout
        certifiable, n, ncert, bad, m10, m21, ncert_half, bad_half = map(int, out.stdout.split()[-8:])
        print(out.stdout)
        assert certifiable == 5 and bad == 0   # the TUM camera's y axis (cy = 255.3) has inexact thresholds: double formula
        assert n > 2.9e7 and ncert > 0.5 * n   # the certificate accepts most lanes, specials and near-threshold ones aside
        assert m10 > 1000 and m21 > 1000       # certified lanes left of pixel 0: sums in (-1, 0) are pixel 0, sums in (-2, -1) are outside
        assert ncert_half > ncert and bad_half > 100  # with half the margin lanes are certified whose pixel is wrong, and the test sees them
