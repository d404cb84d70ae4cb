"""div_int_rcp (csrc/volume_core.hpp), the three-operation quotient of the plain voxel update, in exact integer arithmetic.

    q0 = RN(a * y),  r = fma(-b, q0, a),  q = fma(r, y, q0)

must equal RN(a / b), the IEEE float32 quotient, for every integer divisor 1 <= b <= 2^19, every y within one ulp of 1/b
(RN(1/b) and both of its float neighbours: v_rcp_f32 promises no more) and every numerator the kernel admits: 0 or at
least 2^-60 in magnitude.  No GPU, no native build: floats are pairs (m, e) = m * 2^e of Python integers, every product and
sum is formed exactly and rounded once, to nearest even, as the hardware's multiply and FMA round.  The rounding refuses
(asserts) any non-zero result below 2^-126, so the run also shows that q0, r and the quotient stay normal down to the guard
threshold, which is what lets the kernel's comment not rest on the denormal mode."""
import random

P = 24            # significand bits of a float32
EMIN = -149       # exponent of the last place of the smallest normal binade (2^-126 = 2^23 * 2^-149)
GUARD_EXP = -60   # voxel_update<true>: a non-zero sdf numerator below 2^-60 takes the plain division
B_MAX = 1 << 19   # ... and so does a weight sum above 2^19


def rn(n, d, e):
    """(n / d) * 2^e rounded to the nearest float32, ties to even -> (m, e') with 2^23 <= |m| < 2^24, or (0, 0).  d > 0."""
    if n == 0:
        return (0, 0)
    sign = -1 if n < 0 else 1
    n = abs(n)
    k = n.bit_length() - d.bit_length() - P      # n / d / 2^k in [2^22, 2^25)
    while True:
        nn, dd = (n, d << k) if k >= 0 else (n << -k, d)
        q, rem = divmod(nn, dd)
        if q >= 1 << P:
            k += 1
        elif q < 1 << (P - 1):
            k -= 1
        else:
            break
    if 2 * rem > dd or (2 * rem == dd and (q & 1)):
        q += 1
        if q == 1 << P:
            q >>= 1
            k += 1
    assert e + k >= EMIN, "a non-zero result below 2^-126: outside what the guard admits"
    assert e + k + P <= 128
    return (sign * q, e + k)


def fmul(x, y):
    return rn(x[0] * y[0], 1, x[1] + y[1])


def fma(x, y, z):
    """RN(x * y + z), one rounding."""
    pm, pe = x[0] * y[0], x[1] + y[1]
    if z[0] == 0:
        return rn(pm, 1, pe)
    e = min(pe, z[1])
    return rn((pm << (pe - e)) + (z[0] << (z[1] - e)), 1, e)


def fadd(x, y):
    return fma(x, (1 << (P - 1), -(P - 1)), y)


def fl(m, e=0):
    """The float32 nearest to the integer m times 2^e."""
    return rn(m, 1, e)


def neighbour(x, step):
    """The float next to x != 0: step = +1 / -1 in units of its last place, across binades."""
    m, e = x
    if abs(m + step) == 1 << P:
        return ((m + step) // 2, e + 1)
    if abs(m + step) < 1 << (P - 1):
        return (2 * m + step, e - 1)
    return (m + step, e)


def div_int_rcp(a, b, y):
    fb = fl(b)
    assert fb[0] << fb[1] == b if fb[1] >= 0 else fb[0] == b << -fb[1]   # b <= 2^24 is a float
    q0 = fmul(a, y)
    r = fma((-fb[0], fb[1]), q0, a)
    return fma(r, y, q0), q0, r


def recips(b):
    y = rn(1, b, 0)
    return (y, neighbour(y, -1), neighbour(y, +1))


def check(a, b, ys, stats):
    want = rn(a[0], b, a[1])
    for y in ys:
        got, q0, r = div_int_rcp(a, b, y)
        assert got == want, "a = %d * 2^%d, b = %d, y = %d * 2^%d: got %r, RN(a/b) = %r" % (a + (b,) + y + (got, want))
        stats["cases"] += 1
        # step 1 of the proof, where its hypothesis |y - 1/b| <= 2^-23 / b holds (the farther neighbour of RN(1/b) can be
        # 1.5 ulp off: beyond it, and the quotient above is right all the same): 2 |b q0 - a| <= 5 b ulp(q0)
        if abs(y[0] * b - (1 << -y[1])) << 23 <= 1 << -y[1]:
            e = min(q0[1], a[1]) if a[0] else q0[1]
            assert 2 * abs(((b * q0[0]) << (q0[1] - e)) - (a[0] << (a[1] - e))) <= (5 * b) << (q0[1] - e)
            stats["in_hypothesis"] += 1
        stats["r_nonzero"] += r[0] != 0


def adversarial(b, rng):
    """Numerators whose quotient lies as close to a rounding midpoint as a float numerator can bring it: with b = b' * 2^j,
    b' odd, and X = 2Q + 1 the midpoint's 25-bit odd significand, b' * X = A * 2^k +- 1 for the k low bits a float drops."""
    bo = b
    while bo % 2 == 0:
        bo //= 2
    out = []
    for sgn in (1, -1):
        k = bo.bit_length() + 1
        x0 = (sgn * pow(bo, -1, 1 << k)) % (1 << k)      # b' * x0 = +-1 (mod 2^k); odd
        lo, hi = -(-((1 << 24) + 1 - x0) >> k), ((1 << 25) - 1 - x0) >> k
        if lo > hi:
            continue
        x = x0 + (rng.randint(lo, hi) << k)
        e = rng.randrange(-40, 8)
        a = rn(bo * x, 1, e)                             # the float nearest to b * midpoint (up to a power of two)
        out += [a, neighbour(a, 1), neighbour(a, -1), (-a[0], a[1])]
    return out


def numerators(b, rng, n_random):
    wv = fl(b - 1) if b > 1 else (0, 0)
    out = []
    for _ in range(n_random):
        # wv * c + n as the kernel forms it: a stored mean and an observation, sdf-like (either sign) or colour-like (>= 0)
        if rng.random() < 0.5:
            c, n = fl(rng.randrange(-(1 << 24), 1 << 24), -28), fl(rng.randrange(-(1 << 24), 1 << 24), -28)
        else:
            c, n = rn(rng.randrange(0, 255 * 64), 255 * 64, 0), rn(rng.randrange(256), 255, 0)
        out.append(fadd(fmul(wv, c), n))
    # an sdf numerator that cancelled: any significand, magnitudes from the guard threshold upwards; the threshold itself
    m = rng.randrange(1 << 23, 1 << 24) * rng.choice((1, -1))
    out.append((m, GUARD_EXP - 23 + rng.choice((0, 0, 1, 5, 20))))
    out.append((1 << 23, GUARD_EXP - 23))
    out.append(neighbour((1 << 23, GUARD_EXP - 23), 1))
    out.append((0, 0))
    return out + adversarial(b, rng)


def divisors(rng):
    bs = list(range(1, 4097))
    for p in range(13, 20):
        c = 1 << p
        bs += [c - 3, c - 2, c - 1, c, c + 1, c + 2, c + 3] if p < 19 else [c - 3, c - 2, c - 1, c]
        bs += [rng.randrange(c >> 1, c) for _ in range(8)]
    return bs


def test_helpers_round_like_float32():
    import struct
    rng = random.Random(1)
    f32 = lambda v: struct.unpack("f", struct.pack("f", v))[0]
    val = lambda x: float(x[0]) * 2.0 ** x[1]
    for _ in range(2000):
        a, b = rng.randrange(1, 1 << 30), rng.randrange(1, 1 << 30)
        assert val(rn(a, b, -7)) == f32(a / b / 128.0) or abs(a / b) == 0   # double division is exact enough: 53 > 2 * 24 + 2
        x, y = fl(rng.randrange(-(1 << 24), 1 << 24), -20), fl(rng.randrange(1, 1 << 24), -3)
        assert val(fmul(x, y)) == f32(val(x) * val(y))
    one = (1 << 23, -23)
    assert neighbour(one, -1) == ((1 << 24) - 1, -24) and neighbour(one, 1) == ((1 << 23) + 1, -23)
    assert neighbour(((1 << 24) - 1, -24), 1) == one


def test_three_operation_quotient_is_the_ieee_quotient():
    rng = random.Random(20260)
    stats = {"cases": 0, "r_nonzero": 0, "in_hypothesis": 0}
    for b in divisors(rng):
        ys = recips(b)
        for a in numerators(b, rng, 2 if b <= 4096 else 6):
            check(a, b, ys, stats)
    assert stats["cases"] > 150000 and stats["r_nonzero"] > stats["cases"] // 4 and stats["in_hypothesis"] > stats["cases"] // 2, stats


def test_weight_sum_one_returns_the_numerator():
    """A first observation or an invalid voxel: wsum = 1, y = v_rcp_f32(1) = 1, so q0 = a and r = 0 exactly."""
    rng = random.Random(3)
    one = (1 << 23, -23)
    for _ in range(2000):
        a = (rng.randrange(1 << 23, 1 << 24) * rng.choice((1, -1)), rng.randrange(GUARD_EXP - 23, 10))
        q, q0, r = div_int_rcp(a, 1, one)
        assert q == a and q0 == a and r == (0, 0)


def test_the_bound_on_b_is_not_decorative():
    """Beyond the proof's range the short sequence does fail (so the kernel's wsum guard is needed, and this test can tell):
    some divisor between 2^22 and 2^24 with a one-ulp-off reciprocal and an adversarial numerator gives another float."""
    rng = random.Random(5)
    bad = 0
    for _ in range(400):
        b = rng.randrange(1 << 22, 1 << 24) | 1
        for a in adversarial(b, rng):
            want = rn(a[0], b, a[1])
            bad += any(div_int_rcp(a, b, y)[0] != want for y in recips(b))
    assert bad > 0
