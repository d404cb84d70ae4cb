// ka_cert_check.cpp -- the host program of tests/test_ka_cert_cpu.py: ka_cert.hpp against a replay of k_prepare_frames' float sequence.
//   ka_cert_check quot   the three-operation quotient by a constant: exhaustive significand sweeps, the window's edges, the flag
//   ka_cert_check cert   the in-frustum certificate: cameras x poses x near / far, every certified (pixel, depth) replayed
// Built with -ffp-contract=off (the kernel's own rule); prints one line per fact, the test reads them.  Exit status 0 unless a line says FAIL.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "host_math.hpp"
#include "ka_cert.hpp"

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static bool subnormal_or_nonfinite(float f) { const uint32_t e = (bits(f) >> 23) & 0xffu; return e == 0xffu || (e == 0u && (bits(f) & 0x7fffffu) != 0u); }
static int g_fail = 0;

// ---------------------------------------------------------------------------------------------------------------- quotients
// all 2^23 significands of the binade 2^e, both signs: numerators whose short quotient is not the IEEE one
static long sweep_binade(float b, float y, int e) {
    long bad = 0;
    const uint32_t hi = (uint32_t)(e + 127) << 23;
    for (uint32_t s = 0; s < (1u << 23); ++s) {
        const float n = from_bits(hi | s);
        bad += bits(ka_div_const(n, b, y)) != bits(n / b);
        bad += bits(ka_div_const(-n, b, y)) != bits(-n / b);
    }
    return bad;
}
// a numerator of the binade 2^e for which the short form differs, or one of q0, r, q is subnormal / not finite, or r is not exact
static bool binade_breaks(float b, float y, int e) {
    if (e > 127) { // beyond the largest binade: the numerator is infinite, q0 with it
        const float n = INFINITY;
        return !std::isfinite(n * y);
    }
    if (e < -126) return true; // the numerator itself is subnormal
    const uint32_t hi = (uint32_t)(e + 127) << 23;
    for (uint32_t s = 0; s < (1u << 23); ++s) {
        const float n = from_bits(hi | s);
        const float q0 = n * y, r = __builtin_fmaf(-b, q0, n), q = __builtin_fmaf(r, y, q0);
        if (bits(q) != bits(n / b) || subnormal_or_nonfinite(q0) || subnormal_or_nonfinite(r) || subnormal_or_nonfinite(q)) return true;
    }
    return false;
}

// every significand N whose quotient N / B lies within |D| <= kKaMaxD of a rounding midpoint, by integer arithmetic over all 2^23 of them
static std::set<uint32_t> brute_risky(uint32_t B) {
    std::set<uint32_t> out;
    for (uint32_t N = 1u << 23; N < (1u << 24); ++N) {
        const int sh = N < B ? 25 : 24; // quotient in (1/2, 1): midpoints K 2^-25; in [1, 2): K 2^-24
        const uint64_t t = ((uint64_t)N << sh) / B;
        for (uint64_t K = t - 1; K <= t + 2; ++K) {
            if ((K & 1ull) == 0) continue;
            const int64_t D = (int64_t)((uint64_t)N << sh) - (int64_t)((uint64_t)B * K);
            if (D != 0 && D >= -ka_detail::kKaMaxD && D <= ka_detail::kKaMaxD) out.insert(N);
        }
    }
    return out;
}

static int run_quot() {
    {   // the enumeration ka_quot's flag rests on against the brute force
        std::mt19937 rng(99u);
        std::vector<float> bs = {517.3f, 1.3333334f, 1000.0f, 3.0f, 1.9999996f, 1.0000001f};
        for (int t = 0; t < 6; ++t) bs.push_back(from_bits((127u << 23) | (rng() & 0x7fffffu) | 1u)); // odd significands: every D has solutions
        bs.push_back(from_bits((127u << 23) | ((rng() & 0x7fffffu) & ~3u) | 2u)); // one and two trailing zero bits
        bs.push_back(from_bits((127u << 23) | ((rng() & 0x7fffffu) & ~7u) | 4u));
        for (float b : bs) {
            const uint32_t B = (bits(b) & 0x7fffffu) | 0x800000u;
            std::set<uint32_t> got;
            ka_detail::risky_numerators(B, [&](uint32_t N) { got.insert(N); });
            const std::set<uint32_t> want = brute_risky(B);
            size_t above = 0;
            for (uint32_t N : want) above += N >= B;
            std::printf("QUOTENUM b %.9g enumerated %zu brute %zu above_one %zu equal %d\n", (double)b, got.size(), want.size(), above, (int)(got == want));
        }
    }
    const float fxs[4] = {525.0f, 517.3f, 585.0f, 1050.25f}, dss[2] = {1000.0f, 5000.0f};
    for (int k = 0; k < 6; ++k) {
        const float b = k < 4 ? fxs[k] : dss[k - 4];
        const KaQuot q = ka_quot(b);
        long bad = 0;
        const int binades[5] = {-1, 0, 10, q.lo, q.hi};
        for (int e : binades) bad += sweep_binade(b, q.y, e);
        std::printf("QUOT b %.9g flag %d lo %d hi %d mismatches %ld\n", (double)b, q.ok, q.lo, q.hi, bad);
        if (k >= 4) {
            long badi = 0;
            for (int n = 0; n < 65536; ++n) badi += bits(ka_div_const((float)n, b, q.y)) != bits((float)n / b);
            std::printf("QUOT16 b %.9g mismatches %ld window_holds_u16 %d\n", (double)b, badi, q.lo <= 0 && q.hi >= 15);
        }
        // below: 1 = a numerator of the first binade under the window breaks, 2 = only one of the second, 0 = neither
        const int below = binade_breaks(b, q.y, q.lo - 1) ? 1 : binade_breaks(b, q.y, q.lo - 2) ? 2 : 0;
        std::printf("QUOTEDGE b %.9g below %d above %d\n", (double)b, below, (int)binade_breaks(b, q.y, q.hi + 1));
    }
    // divisors below 1: the only ones whose window ends under the largest binade, so that its upper edge can be probed with finite numerators
    // (for b >= 1, hi = 127 and "above the window" is the infinite numerator alone)
    for (float b : {0.75f, 0.001337f}) {
        const KaQuot q = ka_quot(b);
        const long bad = sweep_binade(b, q.y, q.lo) + sweep_binade(b, q.y, q.hi);
        const int below = binade_breaks(b, q.y, q.lo - 1) ? 1 : binade_breaks(b, q.y, q.lo - 2) ? 2 : 0;
        const int above = binade_breaks(b, q.y, q.hi + 1) ? 1 : binade_breaks(b, q.y, q.hi + 2) ? 2 : 0;
        std::printf("QUOTSMALL b %.9g flag %d lo %d hi %d mismatches %ld below %d above %d\n", (double)b, q.ok, q.lo, q.hi, bad, below, above);
    }
    // the excluded significand
    const float ones = std::nextafterf(1024.0f, 0.0f);
    std::printf("QUOTONES b %.9g flag %d\n", (double)ones, ka_quot(ones).ok);
    // the flag is a statement about every numerator: divisors drawn at random, each swept over a whole binade when its flag is set
    std::mt19937 rng(20261020u);
    int flagged = 0, refused = 0;
    long bad = 0;
    for (int t = 0; t < 24; ++t) {
        const float b = from_bits(((uint32_t)(127 + (int)(rng() % 12)) << 23) | (rng() & 0x7fffffu));
        const KaQuot q = ka_quot(b);
        if (!q.ok) { ++refused; continue; }
        ++flagged;
        bad += sweep_binade(b, q.y, (int)(rng() % 3) - 1);
    }
    std::printf("QUOTRANDOM flagged %d refused %d mismatches %ld\n", flagged, refused, bad);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- certificate
struct Cam { const char* name; float fx, fy, cx, cy; int w, h; };
struct Replay { bool in, all_pos; float q3; };

// k_prepare_frames' sequence for one pixel, IEEE divisions, ContainPoint with its early exits (in) and all six distances (all_pos)
static Replay replay(const Cam& c, const float* M, const float* P, int j, int i, float z) {
    const float x = ((float)j - c.cx) * z / c.fx;
    const float y = ((float)i - c.cy) * z / c.fy;
    const float q0 = ((M[0] * x + M[1] * y) + M[2] * z) + M[3] * 1.0f;
    const float q1 = ((M[4] * x + M[5] * y) + M[6] * z) + M[7] * 1.0f;
    const float q2 = ((M[8] * x + M[9] * y) + M[10] * z) + M[11] * 1.0f;
    const float q3 = ((M[12] * x + M[13] * y) + M[14] * z) + M[15] * 1.0f;
    float p0 = q0, p1 = q1, p2 = q2;
    if (q3 != 1.0f) { p0 = q0 / q3; p1 = q1 / q3; p2 = q2 / q3; }
    Replay r{true, true, q3};
    bool decided = false;
    for (int k = 0; k < 6; ++k) {
        const float dist = (P[4 * k] * p0 + (P[4 * k + 1] * p1 + P[4 * k + 2] * p2)) + P[4 * k + 3];
        if (!(dist > 0)) r.all_pos = false;
        if (!decided) {
            if (dist < 0) { r.in = false; decided = true; }
            else if (dist == 0) decided = true;
        }
    }
    return r;
}

static void random_pose(std::mt19937& rng, float t_max, float M[16]) {
    std::normal_distribution<double> g(0.0, 1.0);
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    double q[4], n = 0;
    for (double& v : q) { v = g(rng); n += v * v; }
    n = std::sqrt(n);
    const double w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
    const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                         2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) M[4 * r + c] = (float)R[3 * r + c];
        M[4 * r + 3] = (float)(t_max * u(rng));
    }
    M[12] = M[13] = M[14] = 0.0f; M[15] = 1.0f;
}

static std::vector<std::pair<int, int>> pixels_of(const Cam& c, std::mt19937& rng) {
    std::vector<std::pair<int, int>> px;
    if ((long)c.w * c.h <= 20000) {
        for (int i = 0; i < c.h; ++i)
            for (int j = 0; j < c.w; ++j) px.push_back({j, i});
        return px;
    }
    for (int j = 0; j < c.w; ++j) { px.push_back({j, 0}); px.push_back({j, c.h - 1}); px.push_back({j, 1}); px.push_back({j, c.h - 2}); }
    for (int i = 0; i < c.h; ++i) { px.push_back({0, i}); px.push_back({c.w - 1, i}); px.push_back({1, i}); px.push_back({c.w - 2, i}); }
    for (int k = 0; k < 100000; ++k) px.push_back({(int)(rng() % (unsigned)c.w), (int)(rng() % (unsigned)c.h)});
    return px;
}

static float step(float z, int ulps) {
    for (int k = 0; k < std::abs(ulps); ++k) z = std::nextafterf(z, ulps > 0 ? INFINITY : 0.0f);
    return z;
}

struct Sweep { long checked = 0, certified = 0, violations = 0, pixels_certified = 0, pixels = 0; };

// every pixel of the set with the depths of the issue; a certified (pixel, depth) must have six positive distances and q3 == 1
static Sweep sweep(const Cam& c, const float* M, const float* P, const KaCert& T, const KaCam& Q, float nearD, float farD, std::mt19937& rng, bool verbose) {
    Sweep s;
    const auto px = pixels_of(c, rng);
    std::uniform_real_distribution<float> uz(0.5f * nearD, 1.2f * farD);
    for (const auto& p : px) {
        const int j = p.first, i = p.second;
        float zs[20];
        int nz = 0;
        for (int d = -3; d <= 3; ++d) { zs[nz++] = step(T.z_lo, d); zs[nz++] = step(T.z_hi, d); }
        zs[nz++] = nearD; zs[nz++] = farD;
        for (int k = 0; k < 4; ++k) zs[nz++] = uz(rng);
        const bool in_rect = j >= T.j_lo && j <= T.j_hi && i >= T.i_lo && i <= T.i_hi;
        ++s.pixels; s.pixels_certified += in_rect;
        for (int k = 0; k < nz; ++k) {
            const float z = zs[k];
            ++s.checked;
            if (!(z > 0) || !in_rect || !(z >= T.z_lo && z <= T.z_hi)) continue;
            ++s.certified;
            const Replay r = replay(c, M, P, j, i, z);
            const float nx = ((float)j - c.cx) * z, ny = ((float)i - c.cy) * z;
            const bool quot = bits(ka_div_const(nx, c.fx, Q.qx.y)) == bits(nx / c.fx) && bits(ka_div_const(ny, c.fy, Q.qy.y)) == bits(ny / c.fy);
            if (!r.all_pos || !r.in || r.q3 != 1.0f || !quot) {
                if (verbose && s.violations < 3) std::printf("FAIL %s pixel (%d, %d) z %.9g: all_pos %d in %d q3 %.9g quotients %d\n", c.name, j, i, (double)z, r.all_pos, r.in, (double)r.q3, quot);
                ++s.violations;
            }
        }
    }
    return s;
}

static int run_cert() {
    const Cam cams[6] = {{"bench", 514.817f, 515.375f, 318.771f, 238.447f, 640, 480}, {"integer_c", 525.0f, 525.0f, 320.0f, 240.0f, 640, 480},
                         {"off_centre", 525.0f, 525.0f, 160.0f, 239.5f, 640, 480}, {"fx_ne_fy", 585.0f, 517.3f, 319.5f, 239.5f, 640, 480},
                         {"small_37x29", 30.0f, 30.0f, 18.0f, 14.5f, 37, 29}, {"wide_2047x2", 1050.25f, 1050.25f, 1023.0f, 0.5f, 2047, 2}};
    const float nf[2][2] = {{0.5f, 5.0f}, {1.0f, 1.5f}}; // near, far: the volume's defaults and a narrow pair
    std::mt19937 rng(7u);
    long control_violations = 0;
    for (const Cam& c : cams) {
        const KaCam Q = ka_cam(c.fx, c.fy, 1000.0f);
        op_host::CameraPOD pod{c.fx, c.fy, c.cx, c.cy, c.w, c.h, 1000.0f};
        std::vector<std::vector<float>> poses;
        std::vector<std::string> names;
        const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        poses.emplace_back(I, I + 16); names.push_back("identity");
        for (int k = 0; k < 3; ++k) { float M[16]; random_pose(rng, 50.0f, M); poses.emplace_back(M, M + 16); names.push_back("random" + std::to_string(k)); }
        for (int n = 0; n < 2; ++n)
            for (size_t p = 0; p < poses.size(); ++p) {
                float P[24];
                op_host::frustum_planes(pod, poses[p].data(), nf[n][1], nf[n][0], P);
                const KaCert T = ka_certificate(poses[p].data(), P, c.fx, c.fy, c.cx, c.cy, c.w, c.h, Q);
                const Sweep s = sweep(c, poses[p].data(), P, T, Q, nf[n][0], nf[n][1], rng, true);
                if (s.violations) g_fail = 1;
                std::printf("CERT %s %s near %.3g far %.3g rect [%d, %d] x [%d, %d] z [%.9g, %.9g] pixels %ld in_rect %ld checked %ld certified %ld violations %ld\n", c.name, names[p].c_str(),
                            (double)nf[n][0], (double)nf[n][1], T.j_lo, T.j_hi, T.i_lo, T.i_hi, (double)T.z_lo, (double)T.z_hi, s.pixels, s.pixels_certified, s.checked, s.certified, s.violations);
                if (std::string(c.name) == "integer_c") { // the control: no error bound, no rectangle -- the same sweep has to object
                    const KaCert T0 = ka_certificate(poses[p].data(), P, c.fx, c.fy, c.cx, c.cy, c.w, c.h, Q, 0.0, true);
                    control_violations += sweep(c, poses[p].data(), P, T0, Q, nf[n][0], nf[n][1], rng, false).violations;
                }
            }
        // refused poses: a rotation perturbed by 1e-3 and a projective bottom row
        float P[24], Mp[16], Mb[16];
        const double a = 0.3;
        const float Rz[16] = {(float)std::cos(a), (float)-std::sin(a), 0, 0.1f, (float)std::sin(a), (float)std::cos(a), 0, -0.2f, 0, 0, 1, 0.3f, 0, 0, 0, 1};
        std::memcpy(Mp, Rz, sizeof(Rz)); Mp[0] += 1.0e-3f;
        std::memcpy(Mb, Rz, sizeof(Rz)); Mb[14] = 1.0e-3f;
        op_host::frustum_planes(pod, Rz, 5.0f, 0.5f, P);
        const KaCert Tr = ka_certificate(Rz, P, c.fx, c.fy, c.cx, c.cy, c.w, c.h, Q);
        op_host::frustum_planes(pod, Mp, 5.0f, 0.5f, P);
        const KaCert Tp = ka_certificate(Mp, P, c.fx, c.fy, c.cx, c.cy, c.w, c.h, Q);
        op_host::frustum_planes(pod, Mb, 5.0f, 0.5f, P);
        const KaCert Tb = ka_certificate(Mb, P, c.fx, c.fy, c.cx, c.cy, c.w, c.h, Q);
        std::printf("REFUSED %s rigid_certified %d perturbed_refused %d projective_refused %d\n", c.name, Tr.j_lo <= Tr.j_hi, Tp.j_lo > Tp.j_hi, Tb.j_lo > Tb.j_hi);
    }
    std::printf("CONTROL integer_c violations %ld\n", control_violations);
    {   // the share of (pixel, depth) pairs certified on the bench camera: identity pose, default near / far, depths uniform in [0.5, 5] m
        const Cam& c = cams[0];
        const KaCam Q = ka_cam(c.fx, c.fy, 1000.0f);
        op_host::CameraPOD pod{c.fx, c.fy, c.cx, c.cy, c.w, c.h, 1000.0f};
        const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        float P[24];
        op_host::frustum_planes(pod, I, 5.0f, 0.5f, P);
        const KaCert T = ka_certificate(I, P, c.fx, c.fy, c.cx, c.cy, c.w, c.h, Q);
        std::uniform_real_distribution<float> uz(0.5f, 5.0f);
        long cert = 0, in_frustum = 0, all = 0;
        for (int i = 0; i < c.h; ++i)
            for (int j = 0; j < c.w; ++j) {
                const float z = uz(rng);
                ++all;
                cert += j >= T.j_lo && j <= T.j_hi && i >= T.i_lo && i <= T.i_hi && z >= T.z_lo && z <= T.z_hi;
                in_frustum += replay(c, I, P, j, i, z).in;
            }
        std::printf("SHARE bench identity certified %.6f in_frustum %.6f\n", (double)cert / (double)all, (double)in_frustum / (double)all);
    }
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "quot") run_quot();
    else if (mode == "cert") run_cert();
    else { std::fprintf(stderr, "usage: ka_cert_check quot|cert\n"); return 2; }
    return g_fail;
}
