"""project_pixel<true>'s certified fast path (csrc/volume_core.hpp, px_round.hpp px_certified) on the device.

Operands are concentrated inside and just outside the certification band around every rounding threshold and image border,
so that waves take the fast path, the exact fallback, and both at once; the pixel must equal the reference formula with the
plain IEEE division (op_debug_project_uv) for several intrinsics."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 640, 480   # op_debug_project_uv's image


def _run(lib, L, fx, fy, cx, cy, X, Y, Z):
    X, Y, Z = (np.ascontiguousarray(a, np.float32) for a in (X, Y, Z))
    out = np.empty((len(X), 4), np.int32)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    L.check(lib.op_debug_project_uv(float(fx), float(fy), float(cx), float(cy), vp(X), vp(Y), vp(Z), len(X), 0, vp(out)))
    return out


def _agree(out):
    r_in = (out[:, 2] >= 0) & (out[:, 2] < W) & (out[:, 3] >= 0) & (out[:, 3] < H)
    f_in = out[:, 0] != np.iinfo(np.int32).min
    bad = (r_in != f_in) | (r_in & ((out[:, 0] != out[:, 2]) | (out[:, 1] != out[:, 3])))
    assert not bad.any(), (np.flatnonzero(bad)[:5], out[bad][:5])
    return r_in.mean()


def _band_operands(rng, n, f, c, extent, width):
    """X and Z with (f*X)/Z + c + 0.5 within +-width of an integer in [-3, extent + 3]."""
    k = rng.integers(-3, extent + 4, n).astype(np.float64)
    t = k + rng.uniform(-width, width, n)
    Z = rng.uniform(0.2, 8.0, n) * np.where(rng.random(n) < 0.05, -1.0, 1.0)
    a = t - (np.float64(np.float32(c)) + 0.5)
    X = (a * Z / np.float64(np.float32(f))).astype(np.float32)
    return X, Z.astype(np.float32)


@pytest.mark.parametrize("fx,fy,cx,cy", [
    (514.817, 515.375, 318.771, 238.447),   # the bench / Open3D camera
    (517.3, 516.5, 318.6, 240.3),           # TUM's fx, fy, cx (its cy has inexact thresholds: the double formula)
    (600.0, 600.0, 321.37, 233.9),
    (1200.25, 1190.5, 300.01, 250.99),
])
def test_certified_projection_equals_plain_division(fx, fy, cx, cy):
    from onepiece_amd import _lib as L
    lib = L.load()
    rng = np.random.default_rng(11)
    n = 1 << 20
    fx, fy, cx, cy = (np.float32(v) for v in (fx, fy, cx, cy))
    other = lambda m: rng.uniform(-0.3, 0.3, m).astype(np.float32)
    # the certification band of these cameras is ~1e-4 wide: 1e-3 straddles it (both paths, mixed in one wave), 2e-5 sits
    # inside it (the fallback in nearly every wave), 5e-3 mostly outside it (the fast path)
    for width in (2e-5, 1e-3, 5e-3):
        X, Z = _band_operands(rng, n, fx, cx, W, width)
        _agree(_run(lib, L, fx, fy, cx, cy, X, other(n) * Z, Z))
        Y, Z = _band_operands(rng, n, fy, cy, H, width)
        _agree(_run(lib, L, fx, fy, cx, cy, other(n) * Z, Y, Z))
    # both axes near a boundary at once: x within the band, y a few ulp around exact boundary quotients
    X, Z = _band_operands(rng, n, fx, cx, W, 1e-4)
    Y = ((rng.integers(-2, H + 3, n) - (np.float64(cy) + 0.5)) * Z.astype(np.float64) / np.float64(fy)).astype(np.float32)
    Y = (Y.view(np.int32) + rng.integers(-8, 9, n).astype(np.int32)).view(np.float32)
    _agree(_run(lib, L, fx, fy, cx, cy, X, Y, Z))
    # camera-like operands: mostly the fast path
    Z = rng.uniform(0.05, 20.0, n).astype(np.float32)
    assert _agree(_run(lib, L, fx, fy, cx, cy, rng.uniform(-1, 1, n) * Z * (0.7 * W / fx), rng.uniform(-1, 1, n) * Z * (0.7 * H / fy), Z)) > 0.3
    # specials mixed into waves of ordinary lanes: NaN, inf, overflowing f*X, |Z| outside the window, huge quotients
    sp = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38, 0.0, -0.0, 1e-45, 2.0 ** -61, 2.0 ** 61, 1e7, -1e7], np.float32)
    m = 1 << 16
    X, Y, Z = (rng.uniform(lo, hi, m).astype(np.float32) for lo, hi in ((-1, 1), (-1, 1), (0.5, 4)))
    for arr in (X, Y, Z):
        idx = rng.integers(0, m, m // 64)
        arr[idx] = rng.choice(sp, len(idx))
    with np.errstate(all="ignore"):
        out = _run(lib, L, fx, fy, cx, cy, X, Y, Z)
    fin = ~np.isinf(Z)   # Z = +-inf: the plain quotient is 0, the shared reciprocal NaN (no pixel) -- as in test_integration_gpu
    _agree(out[fin])
    assert np.all(out[~fin][:, :2] == np.iinfo(np.int32).min)
