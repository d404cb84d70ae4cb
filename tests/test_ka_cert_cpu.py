"""k_prepare_frames' host side (onepiece_amd/csrc/ka_cert.hpp): the per-frame in-frustum certificate and the three-operation quotient by a camera constant.

A stand-alone host program (tests/tools/ka_cert_check.cpp) is compiled against the header and host_math.hpp with -ffp-contract=off, the kernel's rule,
and replays the kernel's float sequence: back-projection with IEEE divisions, the pose product, the six planes.

Certificate: for the bench camera, a camera whose principal point lies on integers (column 0 and row 0 sit on the frustum's planes), an off-centre
principal point, fx != fy and the 37 x 29 and 2047 x 2 images; the identity and three random rigid poses with translations up to 50 m; the default
near / far pair and a narrow one.  Every pixel of the small images, every border pixel (two deep) and 10^5 sampled pixels of the large ones, each at
z_lo, z_hi, their neighbours up to three ulps inside and outside, the near and far distances and random depths: a certified (pixel, depth) must
have all six distances > 0, q3 == 1.0f and both short quotients equal to the IEEE ones.  A rotation perturbed by 1e-3 and a projective bottom row
get no certificate.  The same sweep with the error bound set to 0 and no rectangle must object on the integer camera, or it could not fail.

Quotients: for fx in {525, 517.3, 585, 1050.25} and depth_scale in {1000, 5000} all 2^23 significands of the numerator, both signs, in the binades
2^-1, 2^0, 2^10 and the window's two edge binades are bit-equal to n / b; for the depth scales so are all 65536 integer numerators; a divisor with
an all-ones significand is refused; 24 random divisors whose flag is set pass a whole binade each.  The numerators ka_quot tries
(ka_detail::risky_numerators) are, for 14 divisors with odd and even significands, exactly those an integer brute force over all 2^23
significands finds within |D| <= 8 of a rounding midpoint, below and above a quotient of 1.
The window's edges.  Below the window a numerator must exist for which the short form differs or one of q0, r, q is subnormal or not finite.  The
issue asks for it just outside; this test accepts it in the first binade below or in the second: the lower edge is the analytic guarantee
(r is a multiple of a granule that is normal from there on), and for a divisor whose first binade below happens to hold no residual of exactly
one granule (517.3) it is one binade conservative.  That is weaker than the issue's wording and is said here, not hidden.  Above the window: for
b >= 1 the window ends with the largest binade and the only numerator above it is infinite, so the upper edge cannot be probed there (the check
is kept, it can only see q0 = inf); two divisors below 1 (0.75, 0.001337) probe it with finite numerators: the first binade above must break."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ka_cert") / "ka_cert_check"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I", os.path.join(ROOT, "onepiece_amd", "csrc"),
                           os.path.join(ROOT, "tests", "tools", "ka_cert_check.cpp"), "-o", str(exe)])
    return str(exe)


def _run(program, mode):
    run = subprocess.run([program, mode], capture_output=True, text=True, timeout=600)
    print(run.stdout)
    assert run.returncode == 0 and "FAIL" not in run.stdout, run.stdout[-4000:] + run.stderr
    return run.stdout.splitlines()


def _fields(line):
    return dict(re.findall(r"(\w+) (-?[\d.e+-]+)(?= |$)", line))


def test_certified_pixels_are_inside_by_the_replayed_float_sequence(program):
    lines = _run(program, "cert")
    certs = [l for l in lines if l.startswith("CERT ")]
    assert len(certs) == 6 * 4 * 2
    for l in certs:
        f = _fields(l)
        assert int(f["violations"]) == 0, l
        assert int(f["certified"]) > 0 and int(f["in_rect"]) > 0, "a rigid pose of these cameras gets a certificate: " + l
    # the integer principal point: column 0 and row 0 lie on the planes and stay outside the rectangle; the centred camera keeps every pixel
    assert all("rect [1, 639] x [1, 479]" in l for l in certs if l.startswith("CERT integer_c "))
    assert all("rect [0, 639] x [0, 479]" in l for l in certs if l.startswith("CERT fx_ne_fy "))
    refused = [l for l in lines if l.startswith("REFUSED ")]
    assert len(refused) == 6
    for l in refused:
        assert l.endswith("rigid_certified 1 perturbed_refused 1 projective_refused 1"), l
    control = [l for l in lines if l.startswith("CONTROL ")]
    assert len(control) == 1 and int(control[0].split()[-1]) > 0, "without the error bound and the rectangle the sweep must find a violation"
    share = [l for l in lines if l.startswith("SHARE ")]
    m = re.search(r"certified ([\d.]+) in_frustum ([\d.]+)", share[0])
    print("certified share on the bench camera, identity pose, depths in [0.5, 5] m: %s (in the frustum at all: %s)" % m.groups())
    assert float(m.group(1)) >= 0.95


def test_short_quotients_equal_the_ieee_division(program):
    lines = _run(program, "quot")
    # the enumeration the flag rests on is the set an integer brute force over all 2^23 numerators finds, quotients above 1 included
    enum = [_fields(l) for l in lines if l.startswith("QUOTENUM ")]
    assert len(enum) == 14 and all(int(f["equal"]) == 1 and f["enumerated"] == f["brute"] for f in enum), enum
    assert sum(int(f["brute"]) for f in enum) >= 40 and sum(int(f["above_one"]) for f in enum) >= 10 and any(int(f["brute"]) == 0 for f in enum)
    small = [_fields(l) for l in lines if l.startswith("QUOTSMALL ")]   # divisors below 1: the window's upper edge lies under the largest binade
    assert len(small) == 2
    for f in small:
        assert int(f["flag"]) == 1 and int(f["mismatches"]) == 0 and int(f["hi"]) < 127 and int(f["above"]) == 1 and int(f["below"]) in (1, 2), f
    quot = [l for l in lines if l.startswith("QUOT ")]
    assert len(quot) == 6
    for l in quot:
        f = _fields(l)
        assert int(f["flag"]) == 1 and int(f["mismatches"]) == 0 and int(f["lo"]) <= -60 and int(f["hi"]) == 127, l
    q16 = [l for l in lines if l.startswith("QUOT16 ")]
    assert len(q16) == 2 and all(l.endswith("mismatches 0 window_holds_u16 1") for l in q16), q16
    edges = [l for l in lines if l.startswith("QUOTEDGE ")]
    assert len(edges) == 6
    for l in edges:
        f = _fields(l)
        assert int(f["above"]) == 1, l
        assert int(f["below"]) in (1, 2), "no numerator breaks in the two binades below the window: it is narrower than it need be: " + l
    assert [l for l in lines if l.startswith("QUOTONES ")][0].endswith("flag 0")
    rnd = _fields([l for l in lines if l.startswith("QUOTRANDOM ")][0])
    assert int(rnd["mismatches"]) == 0 and int(rnd["flagged"]) >= 12, rnd
