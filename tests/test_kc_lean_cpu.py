"""The two statements k_integrate's lean form rests on (csrc/integrate.hip: voxel_update<true, true> and the band test in `apply`), in numpy
float32 with every operation kept separate (one rounding each, nothing fused), no GPU:

* the bound: a running mean s' = RN(RN(RN(w * s) + o) / (w + 1)) of observations |o| < T = 0.5, taken from the first observation to weight
  2^19, never reaches 1 -- so TSDFVoxel::IsValid holds for every stored voxel of weight >= 1 and the select the lean form drops would have
  passed the weight through.  (The kernel forms the quotient with a hardware reciprocal and one correction; tests/test_voxel_quotient_cpu.py
  and tests/test_voxel_update_gpu.py show that to be the IEEE division bit for bit, which is what runs here.)  The colour means obey the same
  recurrence with observations byte / 255 and must stay in [0, 1];
* the band predicate: (d > 0) & (|d - zc| < trunc) equals the form it replaces, band = d > 0 ? |d - zc| : trunc; band < trunc, for every
  input, the special ones included."""
import numpy as np

T = np.float32(0.5)
W_MAX = 1 << 19
# csrc/integrate.hip, the LEAN comment: B_W = T g / (1 - W d) with g = (1 + 2^-24)^3 = 1 + d
_D = (1.0 + 2.0 ** -24) ** 3 - 1.0
BOUND_RATIO = (1.0 + _D) / (1.0 - W_MAX * _D)


def _run(obs):
    """obs [steps, lanes] float32 -> (largest |x| any lane held after any step, smallest x, final x).  All lanes advance together: the weight
    is the step number."""
    x = obs[0].copy()                                      # the first observation: (0 * s + o) / 1 = o
    hi, lo = np.abs(x), x.copy()
    t = np.empty_like(x)
    for k in range(1, len(obs)):
        w = np.float32(k)
        np.multiply(x, w, out=t)                           # RN(w * s)
        np.add(t, obs[k], out=t)                           # RN(. + 1 * o)
        np.divide(t, w + np.float32(1), out=x)             # RN(. / (w + 1))
        np.maximum(hi, np.abs(x), out=hi)
        np.minimum(lo, x, out=lo)
    return hi, lo, x


_shared = {}


def _streams():
    """Both tests' streams advance in ONE pass over the weights 1 .. 2^19 (half a million numpy steps), computed once."""
    if not _shared:
        sdf, col = _sdf_streams(), _colour_streams()
        obs = np.concatenate([np.stack(list(sdf.values()), axis=1), np.stack(list(col.values()), axis=1)], axis=1)
        assert obs.dtype == np.float32 and obs.shape == (W_MAX, len(sdf) + len(col))
        hi, lo, last = _run(obs)
        k = len(sdf)
        _shared["sdf"] = (sdf, obs[:, :k], hi[:k], lo[:k], last[:k])
        _shared["colour"] = (col, obs[:, k:], hi[k:], lo[k:], last[k:])
    return _shared


def _sdf_streams():
    top = np.nextafter(T, np.float32(0))                   # the largest float below T
    rng = np.random.default_rng(20241)
    n = W_MAX
    sign = np.where(np.arange(n) % 2 == 0, np.float32(1), np.float32(-1)).astype(np.float32)
    lanes = {
        "all top": np.full(n, top, np.float32),
        "all -top": np.full(n, -top, np.float32),
        "alternating +-top": top * sign,
        "alternating -+top": -top * sign,
        "random in (-T, T)": rng.uniform(-1, 1, n).astype(np.float32) * top,
        "random in [T/2, T)": (rng.uniform(0.5, 1, n).astype(np.float32) * top),
        "random in (-T, -T/2]": -(rng.uniform(0.5, 1, n).astype(np.float32) * top),
        "top, then odd mantissas just below": np.where(np.arange(n) % 3 == 0, top, np.float32(0.49999994)).astype(np.float32),
        "one -top, then top": np.concatenate([[-top], np.full(n - 1, top, np.float32)]).astype(np.float32),
    }
    return lanes


def test_running_mean_of_in_band_observations_stays_valid_up_to_weight_2_19():
    assert T.dtype == np.float32 and BOUND_RATIO < 1.1035
    top = np.nextafter(T, np.float32(0))
    lanes, obs, hi, _lo, last = _streams()["sdf"]
    assert (np.abs(obs) < T).all()
    worst = float(hi.max()) / float(T)
    for name, h, x in zip(lanes, hi, last):
        print("%-36s worst |s| / T = %.9f   final s / T = %+.9f" % (name, float(h) / float(T), float(x) / float(T)))
    print("worst |s| / T over all streams and all weights 1 .. 2^19: %.9f (the argument's bound: %.6f; at T = 0.5 that is |s| < %.4f)"
          % (worst, BOUND_RATIO, BOUND_RATIO * 0.5))
    assert (hi < 1).all()                                  # at every step: IsValid's `sdf < 1` holds
    assert worst <= BOUND_RATIO                            # ... and the argument's own bound does
    # the limit on T is needed: the same worst ratio at T = 1 would leave no room below 1 (observations there can be >= 1 - 2^-24 themselves)
    assert worst >= float(top) / float(T)


def _colour_streams():
    rng = np.random.default_rng(20242)
    n = W_MAX
    c255 = (np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float32)   # (float)b / 255.0f, as the kernel's table
    assert c255[255] == 1 and c255[0] == 0
    alt = np.where(np.arange(n) % 2 == 0, 255, 0)
    lanes = {
        "all 255": np.full(n, 255), "all 254": np.full(n, 254), "all 1": np.full(n, 1), "all 0": np.zeros(n, np.int64),
        "alternating 255 / 0": alt, "alternating 0 / 255": 255 - alt,
        "random bytes": rng.integers(0, 256, n), "random bright": rng.integers(250, 256, n), "random dark": rng.integers(0, 3, n),
        "one 0, then 255": np.concatenate([[0], np.full(n - 1, 255)]),
    }
    return {name: c255[v] for name, v in lanes.items()}


def test_colour_means_stay_in_the_unit_interval():
    _lanes, obs, hi, lo, _last = _streams()["colour"]
    assert obs.dtype == np.float32 and (obs >= 0).all() and (obs <= 1).all()
    print("colour means over weights 1 .. 2^19: min %.9g, max %.9g" % (float(lo.min()), float(hi.max())))
    assert (lo >= 0).all() and (hi <= 1).all()


def _old_hit(d, zc, trunc):
    with np.errstate(invalid="ignore", over="ignore"):
        sdf = d - zc
        band = np.where(d > 0, np.abs(sdf), trunc)
        return band < trunc


def _new_hit(d, zc, trunc):
    with np.errstate(invalid="ignore", over="ignore"):
        sdf = d - zc
        return (d > 0) & (np.abs(sdf) < trunc)


def test_band_predicate_in_two_compares_equals_the_select_form():
    f = np.float32
    nan, inf, den = f(np.nan), f(np.inf), f(1e-42)
    tiny = np.finfo(np.float32).tiny
    truncs = np.array([0.1, 0.5, np.nextafter(f(0.5), f(1)), 1.5, 0.04, 0.0, -0.0, -1.0, den, tiny, inf, -inf, nan, 3.0e38], np.float32)
    ds = np.array([-1.0, -0.0, 0.0, den, -den, tiny, nan, inf, -inf, 0.5, 1.0, 1.5, 2.0, 4.999, 0.1, 3.0e38, 65.535], np.float32)
    rng = np.random.default_rng(20243)
    ds = np.concatenate([ds, rng.uniform(0.2, 6.0, 64).astype(np.float32)])
    with np.errstate(invalid="ignore", over="ignore"):
        # zc: specials, and for every (d, trunc) the values that put sdf on, just inside and just outside +-trunc
        base = np.array([nan, inf, -inf, 0.0, -0.0, den, -1.0, 1.0, 2.5, -3.0e38, 3.0e38], np.float32)
        D, TR = np.meshgrid(ds, truncs, indexing="ij")
        edge = []
        for sgn in (f(1), f(-1)):
            z = (D - sgn * TR).astype(np.float32)
            edge += [z, np.nextafter(z, f(np.inf)), np.nextafter(z, f(-np.inf))]
        Z = np.concatenate([np.broadcast_to(base, D.shape + base.shape), np.stack(edge, axis=-1)], axis=-1).astype(np.float32)
        Dg, Tg = np.broadcast_to(D[..., None], Z.shape), np.broadcast_to(TR[..., None], Z.shape)     # (broadcast, not + 0: keeps -0.0)
        sdf = Dg - Z
    assert Dg.dtype == Tg.dtype == Z.dtype == np.float32
    finite_t = np.isfinite(Tg) & (Tg > 0)
    assert (sdf[finite_t] == Tg[finite_t]).any() and (sdf[finite_t] == -Tg[finite_t]).any()     # sdf exactly +-trunc is in the grid
    assert np.isnan(Z).any() and np.isnan(Dg).any() and np.isnan(Tg).any() and (Dg == 0).any() and np.signbit(Dg[Dg == 0]).any()
    old, new = _old_hit(Dg, Z, Tg), _new_hit(Dg, Z, Tg)
    print("band predicate: %d cases, %d hits" % (old.size, int(old.sum())))
    assert old.any() and not old.all()
    assert np.array_equal(old, new)
    # what the kernel relies on beyond equality: nothing non-finite and no d <= 0 is a hit
    assert not new[~(Dg > 0)].any() and not new[np.isnan(sdf) | np.isinf(sdf)].any()
