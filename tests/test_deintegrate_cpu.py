"""De-integration without a GPU: the numpy restatement of the definition (tests/deintegrate_common.py) against exact rational arithmetic,
what the restatement makes of the oracle's volumes (alone-then-de-integrate, the round trip and its error bound), and the new entries'
surface (OP_ERR_NO_DEVICE without a device; a C++ translation unit that calls the new CubeHandler members compiles and links)."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import deintegrate_common as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U = 2.0 ** -24


def rn32(x):
    """The float32 nearest to the rational x, ties to even (exact: integer arithmetic only); overflow -> +-inf."""
    if x == 0:
        return F32(0.0)
    sign, a = (-1 if x < 0 else 1), abs(Fraction(x))
    e = a.numerator.bit_length() - a.denominator.bit_length()         # 2^(e-1) < a < 2^(e+1)
    if Fraction(2) ** e > a:
        e -= 1                                                        # now 2^e <= a < 2^(e+1)
    q = max(e - 23, -149)                                             # the spacing of float32 at a (denormals: 2^-149)
    scaled = a / Fraction(2) ** q
    n, rem = divmod(scaled.numerator, scaled.denominator)
    twice = 2 * rem
    if twice > scaled.denominator or (twice == scaled.denominator and (n & 1)):
        n += 1
    val = Fraction(n) * Fraction(2) ** q
    if val >= Fraction(2) ** 128:
        return F32(sign * np.inf)
    return F32(sign * float(val))                                     # exact: n < 2^25 and q >= -149 fit a double, then a float32


def exact_deintegrate(s, w, c, o, oc):
    """Steps 1-4 of the definition for ONE voxel, every operation rounded once from its exact rational value."""
    fs, fw = Fraction(float(s)), Fraction(float(w))
    if (s >= 1 or w <= 0) or not (w >= 1):
        return (F32(s), F32(w)) + tuple(F32(x) for x in c), "skipped"
    rw = rn32(fw + Fraction(-1))
    if rw == 0:
        return (F32(999.0), F32(0.0), F32(-1.0), F32(-1.0), F32(-1.0)), "reset"
    out = []
    for stored, obs in [(s, o)] + list(zip(c, oc)):
        p = rn32(fw * Fraction(float(stored)))
        m = rn32(Fraction(-1) * Fraction(float(obs)))
        t = rn32(Fraction(float(p)) + Fraction(float(m)))
        if not np.isfinite(t):
            return None, "overflow"
        out.append(rn32(Fraction(float(t)) / Fraction(float(rw))))
    return (out[0], rw, out[1], out[2], out[3]), "reverted"


def _adversarial_operands():
    rng = np.random.default_rng(20261019)
    up = lambda x: np.nextafter(F32(x), F32(np.inf))
    down = lambda x: np.nextafter(F32(x), F32(-np.inf))
    weights = [1, up(1), 1.5, 2, up(2), down(2), 3, 7, 33, 2 ** 19, 2 ** 24, 2 ** 24 + 2, 1e9, 0.5, down(1), 0, -1, 1e-30]
    sdfs = [0, 0.1, -0.1, down(0.1), up(-0.6), 0.59999, down(1), 1, 1.25, 999, 1e-40, -1e-40, 2 ** -126, 1 / 3, -2 / 3]
    obs = [0.05, -0.05, down(0.1), 0.59, -1.4999, 1e-38, 2 ** -149, 1 / 3]
    cases = [(s, w, o) for s in sdfs for w in weights for o in obs]
    for _ in range(1500):                                             # means of in-band observations at random weights, integer and not
        w = F32(rng.integers(1, 70)) if rng.random() < 0.7 else F32(1 + 40 * rng.random())
        cases.append((F32(rng.uniform(-0.6, 0.6)), w, F32(rng.uniform(-0.6, 0.6))))
    col = rng.integers(0, 256, (len(cases), 3)).astype(F32) / F32(255.0)
    stored_col = rng.random((len(cases), 3)).astype(F32)
    stored_col[::7] = -1.0                                            # the default voxel's colour
    a = np.array(cases, F32)
    return a[:, 0], a[:, 1], stored_col, a[:, 2], col


def test_restatement_matches_exact_rational_arithmetic_per_operation():
    s, w, c, o, oc = _adversarial_operands()
    s2, w2, c2, applied, reset = D.deintegrate_voxels(s, w, c, o, oc)
    kinds = {"skipped": 0, "reset": 0, "reverted": 0}
    for i in range(len(s)):
        want, kind = exact_deintegrate(s[i], w[i], c[i], o[i], oc[i])
        if kind == "overflow":
            continue
        kinds[kind] += 1
        assert bool(applied[i]) == (kind != "skipped") and bool(reset[i]) == (kind == "reset"), (i, kind)
        got = np.array([s2[i], w2[i], c2[i, 0], c2[i, 1], c2[i, 2]], F32)
        assert np.array_equal(got.view(np.uint32), np.array(want, F32).view(np.uint32)), (i, kind, s[i], w[i], o[i], got, want)
    assert min(kinds.values()) > 50, kinds


def test_rn32_is_the_ieee_rounding():
    rng = np.random.default_rng(3)
    for _ in range(2000):
        a, b = F32(rng.normal() * 10.0 ** rng.integers(-42, 30)), F32(rng.normal() * 10.0 ** rng.integers(-10, 10))
        with np.errstate(all="ignore"):
            for got, want in ((rn32(Fraction(float(a)) * Fraction(float(b))), a * b), (rn32(Fraction(float(a)) + Fraction(float(b))), a + b)):
                assert np.array_equal(np.array(got, F32).view(np.uint32), np.array(want, F32).view(np.uint32)) or (got == 0 and want == 0), (a, b, got, want)
    assert rn32(Fraction(2) ** 128) == np.inf and rn32(Fraction(2) ** -150) == 0 and rn32(Fraction(3, 2) * Fraction(2) ** -149) == F32(2.0 ** -148)


@pytest.fixture(scope="module")
def frames37():
    return D.frames(D.CAM_37, 33)


def test_a_frame_fused_alone_and_deintegrated_leaves_an_all_default_volume(oracle, frames37):
    for trunc in (0.1, 0.6, 1.5):
        m = D.Model(oracle, D.CAM_37, trunc)
        m.integrate(frames37[12])
        k0, v0 = m.export()
        hits = int((v0[..., 1] == 1).sum())
        assert hits > 1000 and hits == m.updated
        m.deintegrate(frames37[12])
        k1, v1 = m.export()
        assert np.array_equal(k0, k1)
        # an observation with sdf >= 1 (possible from truncation 1 on) is stored as an INVALID voxel (TSDFVoxel::IsValid), which step 1 leaves alone
        invalid = (v0[..., 1] == 1) & (v0[..., 0] >= 1)
        assert (invalid.sum() > 0) == (trunc > 1)
        assert D.is_default(v1[~invalid]).all() and np.array_equal(v1[invalid].view(np.uint32), v0[invalid].view(np.uint32))
        assert m.last == {"hits": hits, "reverted": 0, "reset": hits - int(invalid.sum()), "skipped": int(invalid.sum())}
        m.deintegrate(frames37[12])                                   # again: nothing is there to take out
        assert m.last == {"hits": hits, "reverted": 0, "reset": 0, "skipped": hits} and np.array_equal(m.export()[1].view(np.uint32), v1.view(np.uint32))


@pytest.mark.parametrize("trunc", [0.1, 0.6])
def test_round_trip_stays_inside_the_rounding_bound(oracle, frames37, trunc):
    """Fusing 33 frames and de-integrating frames 10..20 against fusing the other 22 frames only.

    The bound.  One applied operation maps (s, w) to s' = RN(RN(RN(w s) -+ o) / w') with w' = w +- 1 (the products with +-1 are exact).  With
    u = 2^-24 and M >= |s|, |o|, |s'|, to first order: the product is off by <= w M u, the sum by <= (w + 1) M u, and both are divided by w';
    the quotient's own rounding adds <= M u.  So one operation injects an error of at most
        ((2 w + 1) / w' + 1) M u   <=   3 M u for an integration (w' = w + 1),   <=   6 M u for a de-integration (w' = w - 1 >= 1; worst at w = 2),
    i.e. at most 6 * 2^-24 * M per applied operation.  An error e already in s passes through a later operation as e * w / w': the factors of
    consecutive operations telescope, so an error injected at weight w_k arrives at the end as e * w_k / w_end <= e * W / w_end, W the largest
    weight the voxel had.  A voxel that has seen N operations therefore ends within N * 6 M u * W / w_end of the exact mean of the observations
    that remain -- linear in N -- and the comparison volume, w_end integrations at weights <= w_end, within w_end * 3 M u of the same exact mean.
    Per voxel, with W its weight before the de-integrations: N = W + (W - w_end), and
        |delta| <= (1 + 1e-3) * M u * (6 (2 W - w_end) W / w_end + 3 w_end),
    M = truncation for the sdf (|o| < truncation; a mean of such observations and its rounded forms exceed it by less than the factor
    1e-3 that also covers the second-order terms, O(N^2 u^2)), M = 1 for the colours.
    Figures of this restatement on the oracle's volumes (37 x 29 camera, 4 cm voxels), printed below: truncation 0.1: largest |delta sdf| =
    12.5 * 2^-24 * T, colour 22 * 2^-24; truncation 0.6: 46.7 * 2^-24 * T, colour 35 * 2^-24; no weight differs in either."""
    full, part = D.Model(oracle, D.CAM_37, trunc), D.Model(oracle, D.CAM_37, trunc)
    for k, f in enumerate(frames37):
        full.integrate(f)
        if not 10 <= k <= 20:
            part.integrate(f)
    kb, vb = full.export()                                            # before the de-integrations: W
    for k in range(10, 21):
        full.deintegrate(frames37[k])
    ka, va = full.export()
    kp, vp = part.export()
    assert np.array_equal(ka, kb)                                     # every selection was there already
    at = {tuple(k): i for i, k in enumerate(ka.tolist())}
    assert all(tuple(k) in at for k in kp.tolist()), "the keys are a superset of the comparison volume's"
    rows = np.array([at[tuple(k)] for k in kp.tolist()])
    only = np.setdiff1d(np.arange(len(ka)), rows)
    assert D.is_default(va[only]).all(), "blocks only the removed frames selected hold default voxels"
    got, before = va[rows], vb[rows]
    assert np.array_equal(got[..., 1], vp[..., 1]), "weights are exact"
    assert D.is_default(va[va[..., 1] == 0]).all(), "a voxel that ends at weight 0 is the default voxel bit for bit"
    seen = vp[..., 1] > 0
    W, w_end = before[..., 1][seen].astype(np.float64), vp[..., 1][seen].astype(np.float64)
    factor = (1 + 1e-3) * U * (6 * (2 * W - w_end) * W / w_end + 3 * w_end)
    d_sdf = np.abs(got[..., 0][seen].astype(np.float64) - vp[..., 0][seen].astype(np.float64))
    d_col = np.abs(got[..., 2:][seen].astype(np.float64) - vp[..., 2:][seen].astype(np.float64)).max(axis=-1)
    print("truncation %g: %d blocks, last de-integration %s, largest |dsdf| = %.1f * 2^-24 * T, largest |dcolour| = %.1f * 2^-24, tightest bound used %.1f * 2^-24"
          % (trunc, len(ka), full.last, d_sdf.max() / (U * trunc), d_col.max() / U, factor.min() / U))
    assert (d_sdf <= factor * trunc).all() and (d_col <= factor).all()
    # the issue's sketch, 6 * 2^-24 * M per applied operation growing linearly with the operations (at most 33 + 11), covers the measured figures
    assert d_sdf.max() <= 44 * 6 * U * trunc * W.max() and d_col.max() <= 44 * 6 * U * W.max()


def test_new_entries_fail_loudly_without_a_device(hip):
    import torch
    lib = hip.load()
    n = [C.c_uint64(0) for _ in range(4)]
    if torch.cuda.is_available():                                     # with a device the same calls get as far as their null volume
        assert lib.op_volume_deintegrate_stats(None, *[C.byref(x) for x in n]) == hip.OP_ERR_INVALID
        return
    for rc in (lib.op_volume_deintegrate(None, None, 0, None, hip.OP_MEM_HOST, None, None),
               lib.op_volume_deintegrate_sequence(None, None, 0, 0, None, 0, None, 0),
               lib.op_volume_reintegrate(None, None, 0, None, hip.OP_MEM_HOST, None, None),
               lib.op_volume_reintegrate_sequence(None, None, 0, 0, None, 0, None, None, 0),
               lib.op_volume_deintegrate_stats(None, *[C.byref(x) for x in n])):
        assert rc == hip.OP_ERR_NO_DEVICE and b"no CPU fallback" in lib.op_last_error()
    from onepiece_amd import integration as I
    for name in ("DeintegrateImage", "DeintegrateSequence", "ReintegrateImage", "ReintegrateSequence", "DeintegrateStats"):
        assert callable(getattr(I.CubeHandler, name))


def test_a_translation_unit_that_calls_the_new_members_compiles_and_links(hip, tmp_path):
    host = os.path.join(ROOT, "host", "one_piece")
    lib = os.path.join(ROOT, "onepiece_amd")
    subprocess.check_call(["make", "-s"], cwd=host)
    exe = str(tmp_path / "deintegrate_surface.bin")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-I", host, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "deintegrate_surface.cpp"),
                           "-L", host, "-lone_piece_hip_host", "-L", lib, "-lonepiece_hip", "-Wl,-rpath," + host, "-Wl,-rpath," + lib, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)      # the usage line: the binary starts (no GPU needed)
    assert out.returncode == 0 and "usage" in out.stdout
