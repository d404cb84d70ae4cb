"""csrc/px_round.hpp px_certified / px_cert_bound -- the certificate of project_pixel<true>'s fast path, restated on the host.

The device forms t' = fma(f*X, y, c + 0.5) with y the once-refined v_rcp of Z and takes trunc(t') as the pixel whenever
px_certified(t') holds.  Two error models, each over dense random quotients, quotients within 64 ulp of every rounding
threshold and image border, and specials:
  * abstract: t' = RN(a (1 + e) + K') (K' = c + 0.5 in fp32, as the device has it) with |e| up to the derived relative bound 2^-24 + (2^-24 + 2^-39), extremes included;
  * the device's own sequence in fp32 (fmaf, IEEE division for the reference quotient) with the reciprocal v_rcp perturbed by
    up to 4 ulp (the hardware's is within 1).
A certified lane must give exactly what the reference's double formula (px_round_dp + the bounds test) gives.  Run for the
bench camera, the TUM camera and a 2^19-pixel-wide image."""
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
    long n = 0, ncert = 0, bad = 0;
    // reference pixel (in-image or not) vs the fast path's trunc(t') on a certified lane
    static void check(float a, float t, float c, int extent, const PxAxis& s, const char* what) {
        ++n;
        if (!px_certified(t, s)) return;
        ++ncert;
        const int r = px_round_dp(a, c);
        const bool in_ref = r >= 0 && r < extent;
        const int u = (int)t; // |t| < 2^23 on a certified lane
        const bool in_fast = (unsigned)u < (unsigned)extent;
        if (in_ref != in_fast || (in_ref && u != r)) {
            if (bad < 8) printf("%s: c=%.9g extent=%d a=%.9g t'=%.9g ref=%d fast=%d\n", what, c, extent, a, t, r, u);
            ++bad;
        }
    }
    int main() {
        const float cs[6] = {318.771f, 238.447f, 318.6f, 255.3f, 262144.3f, 1.25f};
        const float fs[6] = {514.817f, 515.375f, 517.3f, 516.5f, 300000.0f, 2.0f};
        const int ext[6] = {640, 480, 640, 480, 1 << 19, 3};
        const double E = 0x1p-24 + (0x1p-24 + 0x1p-39); // |t' - RN(q) - K| / |q| before t' is rounded
        int certifiable = 0;
        for (int k = 0; k < 6; ++k) {
            const float c = cs[k], f = fs[k]; const int extent = ext[k];
            const PxAxis s = px_axis(c, extent);
            if (!s.exact) { if (s.hc != -1.0f) { printf("hc=%.9g on an inexact axis\n", s.hc); return 2; } continue; } // (the kernels take the double formula)
            if (!(s.hc > (extent <= 4096 ? 0.499f : 0.0f) && s.hc < 0.5f)) { printf("hc=%.9g for c=%.9g extent=%d\n", s.hc, c, extent); return 2; }
            ++certifiable;
            const double K = (double)c + 0.5;
            for (long it = 0; it < 1500000; ++it) {
                float a; const int mode = it % 6;
                if (mode == 0) { uint32_t b = rnd(); memcpy(&a, &b, 4); }                               // any bit pattern
                else if (mode < 3) a = (float)((unif() * 1.2 - 0.1) * (extent + 2) - K);                 // pixel scale
                else {                                                                                  // +-64 ulp of a threshold / border
                    const int kk = mode == 3 ? (int)(rnd() % (unsigned)(extent + 41)) - 20 : ((rnd() & 1) ? -1 : extent);
                    a = bump((float)((double)kk - K), (int)(rnd() % 129u) - 64);
                }
                // abstract model: the extremes and a random point of the relative error interval
                const double e3[3] = {-E, E, (2.0 * unif() - 1.0) * E};
                for (double e : e3) check(a, (float)((double)a * (1.0 + e) + (double)s.k), c, extent, s, "abstract");
                // the device sequence: Z, and X such that f*X/Z is near a; v_rcp perturbed by up to 4 ulp
                const float z = (float)((0.2 + 8.0 * unif()) * ((rnd() & 7) ? 1.0 : -1.0));
                const float X = (float)((double)a * z / f);
                const float nx = f * X, A = nx / z;
                const float y0 = bump(1.0f / z, (int)(rnd() % 9u) - 4);  // |1 - z y0| < 2^-20, what px_cert_bound assumes
                const float e = fmaf(-z, y0, 1.0f), y = fmaf(e, y0, y0);
                check(A, fmaf(nx, y, s.k), c, extent, s, "device");
            }
            const float sp[12] = {0.0f, -0.0f, INFINITY, -INFINITY, NAN, 1e-45f, -1e-45f, 3e38f, -3e38f, 8388608.0f, -8388609.0f, 1e9f};
            for (float a : sp) for (float t : sp) check(a, t, c, extent, s, "specials");
        }
        // principal points whose fast path may not be certified
        if (px_axis(318.5f, 640).hc != -1.0f || px_axis(319.5f, 640).hc != -1.0f || px_axis(3.0e6f, 640).hc != -1.0f) { printf("refusal\n"); return 2; }
        printf("%d %ld %ld %ld\n", certifiable, n, ncert, bad);
        return bad != 0;
    }
''')


def test_certified_pixel_equals_double_formula():
    with tempfile.TemporaryDirectory() as td:
        cpp, exe = os.path.join(td, "t.cpp"), os.path.join(td, "t")
        open(cpp, "w").write(SRC)
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "onepiece_amd", "csrc"), cpp, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout
        certifiable, n, ncert, bad = map(int, out.stdout.split()[-4:])
        assert certifiable == 5 and bad == 0   # the TUM camera's y axis (cy = 255.3) has inexact thresholds: double formula
        assert n > 2.9e7 and ncert > 0.5 * n   # the certificate accepts most lanes, specials and near-threshold ones aside
