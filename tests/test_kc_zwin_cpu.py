"""k_integrate's projection without the window test on Z (csrc/zwin_cert.hpp, px_round.hpp, volume_core.hpp project_pixel_uv<true, false>), on the host.

The certified projection used to send every lane with |Z| outside [2^-60, 2^60) to the exact sequence.  k_integrate now calls it without that test:
  * the upper side is a bound the host proves per frame (zwin_certified): |Z| < 2^59 for every voxel centre of every block the hash table can hold;
  * the lower side needs no test: a normal Z with a normal reciprocal satisfies the hypotheses of px_cert_bound_folded in every binade, and a zero or
    denormal Z has the reciprocal +-inf on the device (tests/test_kc_zwin_gpu.py measures it), which makes t'' +-inf or NaN -- refused by fract(t'') > h2.

Certificate: the header is compiled into a small shared object and asked about rows M[8..11] of an inverse pose; the float32 Z of the 64 corner voxel
centres of the key range (block ids -2^20 and 2^20 - 1, voxels 0 and 7 per axis), evaluated with numpy float32 in the reference's association
((M8 px + M9 py) + M10 pz) + M11, never exceeds the bound; rows with inf / NaN, rows and resolutions that push the bound past 2^59 are refused; of two
adjacent floats the one just under the threshold is accepted and the one just over it refused.

Emulation: the device sequence in fp32 (fmaf, the reciprocal anywhere within kPxRcpErr of exact, unrefined, no window test), as
tests/test_px_unrefined_cpu.py does, over Z in every binade from 2^-126 to 2^58 and both signs, sums in and around the image and within 64 ulp of the
pixel boundaries: a certified lane gives exactly the pixel of the reference's double formula.  Zero and denormal Z with the device's reciprocal
(+-inf) are never certified.  The control: the same lanes with a reciprocal that is finite and inexact (2^126, the largest power of two a
saturating reciprocal could return) ARE certified with wrong pixels -- the test sees the hypothesis it rests on."""
import ctypes as C
import os
import subprocess
import textwrap

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "onepiece_amd", "csrc")
LIMIT = 2.0 ** 59
COORD = 1 << 20

SHIM = r"""
#include "zwin_cert.hpp"
extern "C" double zw_bound(const float* m, float res) { return zwin_bound(m, res); }
extern "C" int zw_ok(const float* m, float res) { return zwin_certified(m, res) ? 1 : 0; }
extern "C" int zw_ok_batch(const float* inv, int n, float res) { return zwin_certified_batch(inv, n, res) ? 1 : 0; }
extern "C" double zw_limit() { return kZwinLimit; }
extern "C" int zw_coord() { return kZwinCoordLimit; }
"""


@pytest.fixture(scope="module")
def zw(tmp_path_factory):
    d = tmp_path_factory.mktemp("kc_zwin")
    src, so = d / "shim.cpp", d / "libzw.so"
    src.write_text(SHIM)
    subprocess.check_call(["g++", "-O1", "-Wall", "-ffp-contract=off", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    fp = C.POINTER(C.c_float)
    lib.zw_bound.restype = C.c_double
    lib.zw_bound.argtypes = [fp, C.c_float]
    lib.zw_ok.argtypes = [fp, C.c_float]
    lib.zw_ok_batch.argtypes = [fp, C.c_int, C.c_float]
    lib.zw_limit.restype = C.c_double
    assert lib.zw_limit() == LIMIT and lib.zw_coord() == COORD

    def row(m8, m9, m10, m11):
        m = np.zeros(12, np.float32)
        m[:8] = 1e30                                           # rows 0 and 1 must not matter
        m[8:] = (m8, m9, m10, m11)
        return m

    class Z:
        @staticmethod
        def bound(r, res):
            m = row(*r)
            return lib.zw_bound(m.ctypes.data_as(fp), np.float32(res))

        @staticmethod
        def ok(r, res):
            m = row(*r)
            return bool(lib.zw_ok(m.ctypes.data_as(fp), np.float32(res)))

        @staticmethod
        def ok_batch(rows, res):
            inv = np.ascontiguousarray(np.stack([row(*r) for r in rows]), np.float32)
            return bool(lib.zw_ok_batch(inv.ctypes.data_as(fp), len(rows), np.float32(res)))
    return Z


def _corner_coords(res):
    """The float32 coordinate of a voxel centre as the kernel and the reference form it (VoxelCube.h:48-61, 75-80), at the ends of the key range."""
    res = np.float32(res)
    half = res / np.float32(2)
    out = []
    for k in (-COORD, COORD - 1):
        for l in (0, 7):
            out.append((np.float32(k) * np.float32(8.0)) * res + (np.float32(l) * res + half))
    return np.array(out, np.float32)


def _z_of_corners(r, res):
    """|Z| (float32, the reference's association) over the 64 corners; all operations in numpy float32."""
    p = _corner_coords(res)
    px, py, pz = (a.ravel() for a in np.meshgrid(p, p, p, indexing="ij"))
    m8, m9, m10, m11 = (np.float32(v) for v in r)
    with np.errstate(all="ignore"):
        z = ((m8 * px + m9 * py) + m10 * pz) + m11 * np.float32(1.0)
    assert z.dtype == np.float32
    return z


def test_bound_dominates_the_float32_depth_of_every_corner_of_the_key_range(zw):
    rng = np.random.default_rng(2031)
    n_rows = n_checked = n_ok = 0
    tight = 0.0
    for res in (0.005, 0.04, 1.0, 2.0 ** -20, 100.0, 3.3e7):
        for k in range(700):
            kind = k % 7
            if kind == 0:                                       # a rotation's row and a translation
                v = rng.normal(size=3); v /= np.linalg.norm(v)
                r = (*v, rng.uniform(-50, 50))
            elif kind == 1:                                     # magnitudes 2^-40 .. 2^40, mixed signs
                r = tuple(rng.choice([-1.0, 1.0], 4) * 2.0 ** rng.uniform(-40, 40, 4))
            elif kind == 2:                                     # exactly 2^+-40
                r = tuple(rng.choice([-1.0, 1.0], 4) * 2.0 ** rng.choice([-40.0, 40.0], 4))
            elif kind == 3:                                     # exact zeros among ordinary entries
                r = tuple(np.where(rng.random(4) < 0.5, 0.0, rng.normal(size=4)))
            elif kind == 4:                                     # cancellation: the corner sums nearly vanish
                a = rng.uniform(0.5, 2.0)
                r = (a, -a, rng.choice([0.0, 2.0 ** -40]), rng.choice([0.0, 2.0 ** -30, -1.0]))
            elif kind == 5:                                     # tiny rows: denormal products and sums
                r = tuple(rng.choice([-1.0, 1.0], 4) * 2.0 ** rng.uniform(-149, -100, 4))
            else:                                               # near the threshold from both sides
                r = tuple(rng.choice([-1.0, 1.0], 4) * 2.0 ** rng.uniform(20, 62, 4))
            r = tuple(float(np.float32(v)) for v in r)
            b = zw.bound(r, res)
            n_rows += 1
            if not np.isfinite(b):
                assert not zw.ok(r, res)
                continue
            z = np.abs(_z_of_corners(r, res).astype(np.float64))
            assert np.all(z <= b), (r, res, float(z.max()), b)
            n_checked += 1
            tight = max(tight, float(z.max()) / b)
            assert zw.ok(r, res) == (b < LIMIT)
            n_ok += zw.ok(r, res)
    print("%d rows, %d with a finite bound checked on 64 corners, %d certified; largest |Z| / bound %.9f" % (n_rows, n_checked, n_ok, tight))
    assert n_rows == 4200 and n_checked > 4000 and 0.5 * n_rows < n_ok < n_rows
    assert tight > 0.999                                        # the bound is not slack where all terms have one sign at a far corner


def test_ordinary_poses_are_certified_and_absurd_ones_refused(zw):
    for res in (0.005, 0.02, 0.04, 1.0):
        assert zw.ok((0.0, 0.0, 1.0, 0.0), res) and zw.ok((0.6, -0.64, 0.48, -1.0e6), res)
        assert zw.ok((0.0, 0.0, 0.0, 0.0), res) and zw.ok((2.0 ** -70, 0.0, 0.0, 0.0), res) and zw.ok((2.0 ** -130, 0.0, 0.0, 0.0), res)
        assert zw.bound((0.6, -0.64, 0.48, -1.0e6), res) < 2.0 ** 25
    for bad in (np.inf, -np.inf, np.nan):
        for pos in range(4):
            r = [0.1, 0.2, 0.3, 0.4]
            r[pos] = bad
            assert not zw.ok(tuple(r), 0.04)
    assert not zw.ok((2.0 ** 70, 2.0 ** 70, 2.0 ** 70, 2.0 ** 70), 0.04)       # the finite pose of the GPU test's refused case
    assert not zw.ok((0.0, 0.0, 0.0, 2.0 ** 59), 0.04) and zw.ok((0.0, 0.0, 0.0, 2.0 ** 58), 0.04)
    assert not zw.ok((3.0e38, 3.0e38, 3.0e38, 3.0e38), 0.04)                    # the double bound does not overflow where the float sum would
    # a resolution large enough to break the bound, and resolutions that are no resolutions
    assert zw.ok((0.0, 0.0, 1.0, 0.0), 2.0 ** 35) and not zw.ok((0.0, 0.0, 1.0, 0.0), 2.0 ** 36)
    for res in (0.0, -0.04, np.inf, np.nan):
        assert not zw.ok((0.0, 0.0, 1.0, 0.0), res)
    # a batch is certified when every frame is
    good, absurd = (0.0, 0.0, 1.0, 0.5), (2.0 ** 70, 0.0, 0.0, 0.0)
    assert zw.ok_batch([good] * 32, 0.04) and not zw.ok_batch([good] * 31 + [absurd], 0.04) and not zw.ok_batch([absurd] + [good] * 31, 0.04)


@pytest.mark.parametrize("res", [0.005, 0.04, 1.0])
@pytest.mark.parametrize("pos", [0, 1, 2, 3])
def test_adjacent_floats_around_the_threshold(zw, res, pos):
    """The largest float32 entry (alone in its row) that is accepted, found by bisection on the bit pattern: it is accepted with a bound just under 2^59,
    its successor is refused, and at the far corner of the key range its float32 Z is indeed within a factor 1 + 2^-18 of the bound (the bound's
    own slack: 8.5 voxels of 2^23 on the coordinate, 2^-22 and 2^-21 in its two safety factors, together below 2^-19 + 2^-21)."""
    def r_of(bits):
        r = [0.0] * 4
        r[pos] = float(np.uint32(bits).view(np.float32))
        return tuple(r)
    lo, hi = np.float32(1.0).view(np.uint32).item(), np.float32(2.0 ** 100).view(np.uint32).item()
    assert zw.ok(r_of(lo), res) and not zw.ok(r_of(hi), res)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if zw.ok(r_of(mid), res):
            lo = mid
        else:
            hi = mid
    b_lo, b_hi = zw.bound(r_of(lo), res), zw.bound(r_of(hi), res)
    assert zw.ok(r_of(lo), res) and not zw.ok(r_of(hi), res)
    assert LIMIT * (1 - 2.0 ** -22) < b_lo < LIMIT <= b_hi < LIMIT * (1 + 2.0 ** -22)
    z = np.abs(_z_of_corners(r_of(lo), res).astype(np.float64)).max()
    assert b_lo / (1 + 2.0 ** -18) < z <= b_lo
    assert not zw.ok(tuple(-v for v in r_of(hi)), res) and zw.ok(tuple(-v for v in r_of(lo)), res)


EMU = textwrap.dedent(r'''
    #include <cstdio>
    #include <cstdint>
    #include <cstring>
    #include <cmath>
    #include "px_round.hpp"
    #include "zwin_cert.hpp"
    static uint32_t st = 2463534242u;
    static uint32_t rnd() { st ^= st << 13; st ^= st >> 17; st ^= st << 5; return st; }
    static double unif() { return (rnd() >> 8) * (1.0 / 16777216.0); }
    static float bump(float x, int k) { int32_t b; memcpy(&b, &x, 4); b += k; memcpy(&x, &b, 4); return x; }
    static float bits(uint32_t b) { float x; memcpy(&x, &b, 4); return x; }
    // [0]: normal Z, the device's reciprocal within d_rcp; [1]: zero / denormal Z, the device's reciprocal (+-inf); [2]: zero / denormal Z with a finite, inexact one
    long n[3] = {0, 0, 0}, ncert[3] = {0, 0, 0}, bad[3] = {0, 0, 0}, in_img[3] = {0, 0, 0};
    long n_low = 0, cert_low = 0, n_dnx = 0, cert_dnx = 0;   // Z below 2^-60; of the normal-Z lanes those whose numerator f X is denormal
    static bool check(float a, float t2, float c, int extent, const PxAxis& s, int h) {
        ++n[h];
        if (!px_certified_folded(t2, s)) return false;
        ++ncert[h];
        const int r = px_round_dp(a, c);
        const bool in_ref = r >= 0 && r < extent;
        const int u = (int)t2; // |t''| < 2^23 on a certified lane
        const bool in_fast = (unsigned)u < (unsigned)extent;
        const bool ok = in_ref == in_fast && (!in_ref || u == r);
        if (!ok) {
            if (h == 0 && bad[0] < 8) printf("c=%.9g extent=%d a=%.9g t''=%.9g ref=%d fast=%d\n", c, extent, a, t2, r, u);
            ++bad[h];
        }
        in_img[h] += in_ref;
        return true;
    }
    // the float nearest to (1 + d) / z, pulled back inside |1 - z y0| <= lim when its own rounding left it
    static float rcp_off(float z, double d, double lim) {
        float y0 = (float)((1.0 + d) / (double)z);
        for (int k = 0; k < 2 && fabs(1.0 - (double)z * (double)y0) > lim; ++k) y0 = bump(y0, (fabs((double)z * (double)y0) > 1.0) ? -1 : 1);
        return y0;
    }
    static float quotient_target(int mode, long it, int extent, double K, double B) {
        if (mode < 2) return (float)((unif() * 1.2 - 0.1) * (extent + 2) - 2.5 * mode * unif() - K);   // pixel scale, and down to t = -2.5
        const int kk = mode == 2 ? (int)(rnd() % (unsigned)(extent + 41)) - 20 : ((rnd() & 1) ? ((rnd() & 1) ? -1 : 0) : extent);
        const double off = (it / 4) % 3 == 0 ? 0.0 : ((it / 4) % 3 == 1 ? B : -B);
        return bump((float)((double)kk + off - K), (int)(rnd() % 129u) - 64);                          // +-64 ulp of an integer / border, or of the point +-B away
    }
    int main() {
        const float cs[3] = {318.771f, 238.447f, 18.25f};
        const float fs[3] = {514.817f, 515.375f, 30.0f};
        const int ext[3] = {640, 480, 37};
        const double D = kPxRcpErr;
        int top = 0;
        frexp(kZwinLimit, &top);           // kZwinLimit = 2^(top - 1): binades up to top - 2
        long outside = 0;
        for (int k = 0; k < 3; ++k) {
            const float c = cs[k], f = fs[k]; const int extent = ext[k];
            const PxAxis s = px_axis(c, extent);
            if (!s.exact || s.h2 >= 1.0f) { printf("axis %d not certifiable\n", k); return 2; }
            const double K = (double)c + 0.5, B = px_cert_bound_folded((double)extent + 1.0, K);
            for (int e = -126; e <= top - 2; ++e)
                for (long it = 0; it < 12000; ++it) {
                    float a = quotient_target((int)(it % 4), it, extent, K, B);
                    if (e <= -125 && (it & 1)) { // quotients below 1 in magnitude: with |Z| < 2^-124 the numerator f X is denormal.  The two pixel boundaries next to K, and anything between
                        const double off = (it / 2) % 3 == 0 ? 0.0 : ((it / 2) % 3 == 1 ? B : -B);
                        a = (it & 2) ? bump((float)(floor(K) + (double)((it >> 2) & 1) + off - K), (int)(rnd() % 129u) - 64) : (float)(2.0 * unif() - 1.0);
                    }
                    const uint32_t sig = (it % 16 == 0) ? 0u : (it % 16 == 1) ? 0x7fffffu : (rnd() & 0x7fffffu);
                    const float z = bits(((rnd() & 7) ? 0u : 0x80000000u) | ((uint32_t)(127 + e) << 23) | sig);
                    const float X = (float)((double)a * (double)z / (double)f);
                    const float nx = f * X, A = nx / z;      // the numerator as both paths form it; the reference's quotient
                    const int pick = (int)(rnd() % 4u);
                    const double d = pick == 0 ? D : (pick == 1 ? -D : (2.0 * unif() - 1.0) * D);
                    const float y0 = rcp_off(z, d, D);
                    if (!(fabs(1.0 - (double)z * (double)y0) <= D) || !std::isnormal(y0)) { ++outside; continue; }
                    const bool cert = check(A, fmaf(nx, y0, s.kb), c, extent, s, 0);
                    if (e < -60) { ++n_low; cert_low += cert; }
                    if (nx != 0.0f && !std::isnormal(nx)) { ++n_dnx; cert_dnx += cert; }
                }
            // zero and denormal Z
            for (long it = 0; it < 200000; ++it) {
                const float a = quotient_target((int)(it % 4), it, extent, K, B);
                const uint32_t m = it < 64 ? (uint32_t)(it / 2) : (it % 3 == 0 ? (0x400000u | (rnd() & 0x3fffffu)) : (rnd() & 0x7fffffu) >> (rnd() % 23u));
                const float z = bits(((it & 1) ? 0x80000000u : 0u) | m);
                const float X = (float)((double)a * (double)z / (double)f);
                const float nx = f * X, A = nx / z;
                const float y_dev = copysignf(INFINITY, z);  // what v_rcp_f32 returns for a zero or a denormal
                check(A, fmaf(nx, y_dev, s.kb), c, extent, s, 1);
                if (z != 0.0f) check(A, fmaf(nx, copysignf(0x1p126f, z), s.kb), c, extent, s, 2);
            }
        }
        printf("%ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %d\n", n[0], ncert[0], bad[0], in_img[0], n_low, cert_low, n_dnx, cert_dnx, outside, n[1], ncert[1],
               n[2], ncert[2], bad[2], in_img[2], top - 2);
        return bad[0] != 0;
    }
''')

_run = {}


def _figures(tmp_path_factory):
    if not _run:
        d = tmp_path_factory.mktemp("kc_zwin_emu")
        cpp, exe = d / "emu.cpp", d / "emu"
        cpp.write_text(EMU)
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-I", CSRC, str(cpp), "-o", str(exe)])
        out = subprocess.run([str(exe)], capture_output=True, text=True)
        print(out.stdout)
        assert out.returncode == 0, out.stdout
        keys = ("n", "ncert", "bad", "in_img", "n_low", "cert_low", "n_dnx", "cert_dnx", "outside", "n_den", "cert_den", "n_fin", "cert_fin", "bad_fin", "in_fin", "top")
        _run.update(zip(keys, map(int, out.stdout.split()[-len(keys):])))
    return _run


def test_certified_lanes_give_the_exact_pixel_in_every_binade_without_the_window(tmp_path_factory):
    r = _figures(tmp_path_factory)
    assert r["top"] == 58                                       # binades 2^-126 .. 2^58: everything below the host's threshold 2^59
    assert r["bad"] == 0
    assert r["n"] > 3 * 185 * 12000 * 0.999 and r["outside"] < 1e-3 * r["n"]   # (a perturbed reciprocal that left the normal floats at |Z| = 2^-126 is not the device's)
    assert r["ncert"] > 0.5 * r["n"] and r["in_img"] > 0.3 * r["n"]
    # the binades the window test used to send to the exact sequence are certified like the others, denormal numerators included
    assert r["n_low"] > 3 * 66 * 12000 * 0.999 and r["cert_low"] > 0.5 * r["n_low"]
    assert r["n_dnx"] > 10000 and r["cert_dnx"] > 0.3 * r["n_dnx"]             # (half of them sit within 64 ulp of a pixel boundary or of its margin)


def test_zero_and_denormal_depths_are_refused_by_the_certificate_itself(tmp_path_factory):
    r = _figures(tmp_path_factory)
    assert r["n_den"] == 3 * 200000 and r["cert_den"] == 0


def test_a_finite_inexact_reciprocal_of_a_denormal_is_caught(tmp_path_factory):
    """The control: were the hardware to return a finite, inexact reciprocal for a denormal Z, lanes would be certified with wrong pixels inside the
    image, and this test's comparison sees them."""
    r = _figures(tmp_path_factory)
    assert r["cert_fin"] > 1000 and r["bad_fin"] > 1000
