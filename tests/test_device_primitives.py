"""The device's numeric and lane primitives on their own (tests/prim_probe.hip, built by
tests/prim_lib.py with libgm's compiler, flags and include directories).

Every stage above these primitives has a crafted-case test against an independent model; this
file checks the layer underneath, where a wrong refinement step, DPP control or comparison shows
up in a stage test only as "physics differs from the oracle somewhere".

References.  numpy float64 sqrt, / and 1.0 / x are IEEE-754 correctly rounded operations, so the
"correctly rounded" family (sqrt_n, rcp_n, div_n, and rsq_n / rcp_piv in the -DGM_CAL_TU build) is
compared with them bit for bit, as .view(np.int64) equality.  Bounds in ulps are taken against
np.longdouble (64-bit significand) or mpmath values.  No operand lies outside the ranges
gm_real.h documents (x >= 2^-767 or +-0 for sqrt_n; |a|, |b|, |a / b| in [2^-899, 2^899] for
rcp_n / div_n; no negative sqrt argument, NaN, inf or zero divisor): the functions promise
nothing there.

The probe compiles the functions in its own translation unit: it shows what the source means
under libgm's flags and pragmas, not the instruction stream inlined into gm_step_kernel (the
stage-level parity tests remain the check of that).
"""
import math

import mpmath
import numpy as np
import pytest

import prim_lib
from conftest import gpu_available
from gmx.policy import _mix
from test_policy import Q_ATOL

LD = np.longdouble
RNG_SEED = 20240611

# ---------------------------------------------------------------- measured figures
# (b) rsq_n, rcp_refined and rcp_piv of the default build: maximum distance, in ulps, from the
# correctly rounded value over the tables below, measured on an MI355X; the bound is that + 1.
RSQ_N_MEASURED_ULPS = 1          # measured maximum: 1 ulp
RCP_REFINED_MEASURED_ULPS = 1    # measured maximum: 1 ulp
RCP_PIV_MEASURED_ULPS = 1        # measured maximum: 1 ulp (rcp_piv is rcp_refined in this build)
RSQ_N_BOUND = RSQ_N_MEASURED_ULPS + 1
RCP_REFINED_BOUND = RCP_REFINED_MEASURED_ULPS + 1
RCP_PIV_BOUND = RCP_PIV_MEASURED_ULPS + 1
# (c) gm_sincos' host build against mpmath on sincos_table(), measured on the CPU (the device is
# tied to the host build bit for bit).  Where |reference| >= 2^-10 the measured maximum error is
# 1.3075 ulps: B is the next quarter ulp.  The measured maximum absolute error over every point is
# 1.3300e-16: A is twice that.  Where |reference| < 2^-10 the measured maximum relative error is
# 2.8612e-05, at the multiple of pi / 2 that lies closest to a double in proportion to its k (the
# two-term Cody-Waite reduction is off by k * 3.52e-27 there, plus the rounding of k * pio2_1t):
# the bound is twice that.  The reduction's error is deterministic and the table holds those k.
SINCOS_B_ULPS = 1.5
SINCOS_A_ABS = 2.66e-16
SINCOS_SMALL_REL = 5.7224e-05


def i64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def assert_bits_equal(got, ref, operands, what):
    g, r = i64(got), i64(ref)
    bad = np.flatnonzero(g != r)
    if bad.size:
        k = bad[0]
        ops = ", ".join(float(o[k]).hex() for o in operands)
        raise AssertionError(f"{what}: {bad.size} of {g.size} results differ in bits; first at [{k}]: "
                             f"operands {ops}: got {float(got[k]).hex()}, expected {float(ref[k]).hex()}")


def ulps_apart(got, ref):
    """Integer distance in units of the last place between finite doubles of one sign."""
    g, r = i64(got), i64(ref)
    assert np.all((g < 0) == (r < 0)), "sign differs"
    return np.abs(g - r)


def round_int_to_double(N: int, exp2: int) -> float:
    """The double nearest N * 2^exp2 (ties to even) for a positive Python integer N."""
    sh = N.bit_length() - 53
    if sh <= 0:
        return math.ldexp(float(N), exp2)
    M, rem, half = N >> sh, N & ((1 << sh) - 1), 1 << (sh - 1)
    if rem > half or (rem == half and (M & 1)):
        M += 1
    return math.ldexp(float(M), sh + exp2)


def with_neighbours(x):
    x = np.asarray(x, dtype=np.float64)
    return np.concatenate([x, np.nextafter(x, 0.0), np.nextafter(x, np.copysign(np.inf, x))])


# ---------------------------------------------------------------- operand tables (a, b)
SQRT_LO, SQRT_HI = -767, 1023   # sqrt_n: x >= 2^-767 (or +-0)
DIV_E = 899                     # rcp_n / div_n: |a|, |b|, |a / b| inside [2^-899, 2^899]


def sqrt_hard_cases(rng, n=4096):
    """Doubles next to the square of a rounding midpoint: for a mantissa m in [2^52, 2^53) the
    double nearest (m + 1/2)^2 (Python integers) and both of its neighbours.  (2 m + 1)^2 has 107
    bits for m < 2^52 sqrt(2) and 108 above, so the operands have even and odd exponents; 2^(2 j)
    scales them over the range.  Rounding (m + 1/2)^2 to a double moves the root by up to 0.36 ulp,
    so for a random m the root lies within that of the midpoint; for m = 2^52 + i and
    m = 2^53 - 1 - i with small i, m (m + 1) = i (i + 1) modulo the operand's ulp, the rounding
    moves the operand by i (i + 1) + 1/4 only and the root lies within 2^-30 ulp of the midpoint.
    Returns n random m first, then n of the near kind (n / 2 from each end), then the neighbours."""
    i = np.arange(n // 2, dtype=np.int64)
    ms = np.concatenate([rng.integers(1 << 52, 1 << 53, n - 2), [6369051672525773, 6369051672525772],
                         (1 << 52) + i, (1 << 53) - 1 - i])
    js = rng.integers(-430, 456, ms.size)
    xs = [round_int_to_double((2 * int(m) + 1) ** 2, 2 * int(j) - 2) for m, j in zip(ms, js)]
    return with_neighbours(xs)


def sqrt_table():
    rng = np.random.default_rng(RNG_SEED)
    e = rng.integers(SQRT_LO, SQRT_HI + 1, 1 << 15)
    rand = np.ldexp(rng.uniform(1.0, 2.0, e.size), e)
    p2 = np.ldexp(1.0, np.arange(SQRT_LO, SQRT_HI + 1))
    pw = np.concatenate([p2, np.nextafter(p2, np.inf), np.nextafter(p2[1:], 0.0)])   # (none below 2^-767)
    return np.concatenate([rand, [0.0, -0.0, 2.0 ** SQRT_LO], pw, sqrt_hard_cases(rng)])


def rcp_table():
    rng = np.random.default_rng(RNG_SEED + 1)
    e = rng.integers(-DIV_E, DIV_E, 1 << 15)
    rand = np.ldexp(rng.uniform(1.0, 2.0, e.size), e) * rng.choice([-1.0, 1.0], e.size)
    p2 = np.ldexp(1.0, np.arange(-DIV_E + 1, DIV_E))
    pw = with_neighbours(p2)
    edges = np.array([2.0 ** -DIV_E, 2.0 ** DIV_E, -2.0 ** -DIV_E, -2.0 ** DIV_E])
    # next to powers of two: 1 + k ulp and 2 - k ulp, k = 1..64
    k = np.arange(1, 65, dtype=np.int64)
    near = np.concatenate([(np.int64(0x3FF0000000000000) + k).view(np.float64),
                           (np.int64(0x4000000000000000) - k).view(np.float64)])
    # a run of r leading ones in the mantissa, random bits below it
    runs = []
    for r in range(20, 53):
        low = rng.integers(0, 1 << (52 - r), 16) if r < 52 else np.zeros(16, dtype=np.int64)
        mant = (((1 << r) - 1) << (52 - r)) | low.astype(np.int64)
        runs.append((np.int64(0x3FF0000000000000) | mant).view(np.float64))
    hard = np.concatenate([near] + runs)
    hard = np.concatenate([hard, -hard, np.ldexp(hard, rng.integers(-890, 890, hard.size))])
    return np.concatenate([rand, pw, -pw[::7], edges, hard])


def div_hard_cases(rng, n=4096):
    """Quotients next to a rounding midpoint: a random b = mb 2^eb and a midpoint q + ulp / 2 =
    (2 mq + 1) 2^s; a is the double nearest b (q + ulp / 2) (Python integers), and its neighbours.
    Rounding a moves the quotient by up to half an ulp, so in the first half of the cases the
    quotient lies anywhere about the midpoint; in the second half mq is chosen for mb (odd) so that
    mb (2 mq + 1) = r modulo 2^54 with a small odd r: rounding a then removes r alone and the
    quotient lies within |r| 2^-53 ulp of the midpoint."""
    a, b = [], []
    while len(a) < n:
        Eb, Eq = (int(v) for v in rng.integers(-890, 891, 2))
        if abs(Eb + Eq) > 890:
            continue
        mb, mq = (int(v) for v in rng.integers(1 << 52, 1 << 53, 2))
        t = 2 * mq + 1
        if len(a) >= n // 2:
            mb |= 1
            r = (2 * int(rng.integers(0, 1 << int(rng.integers(1, 20)))) + 1) * int(rng.choice([-1, 1]))
            t = (r * pow(mb, -1, 1 << 54)) % (1 << 54)
            if t < (1 << 53):
                continue
        a.append(round_int_to_double(mb * t, (Eb - 52) + (Eq - 53)))
        b.append(math.ldexp(float(mb), Eb - 52))
    a, b = np.array(a), np.array(b)
    sgn = rng.choice([-1.0, 1.0], 3 * n)
    return with_neighbours(a) * sgn, np.concatenate([b, b, b])


def div_table():
    rng = np.random.default_rng(RNG_SEED + 2)
    n = 1 << 15
    eb, eq = rng.integers(-DIV_E + 1, DIV_E - 1, 3 * n), rng.integers(-DIV_E + 1, DIV_E - 1, 3 * n)
    keep = np.flatnonzero(np.abs(eb + eq) < DIV_E - 1)[:n]
    assert keep.size == n
    eb, ea = eb[keep], (eb + eq)[keep]
    b = np.ldexp(rng.uniform(1.0, 2.0, n), eb) * rng.choice([-1.0, 1.0], n)
    a = np.ldexp(rng.uniform(1.0, 2.0, n), ea) * rng.choice([-1.0, 1.0], n)
    # powers of two and their neighbours as dividend and as divisor, against random mantissas
    p2 = with_neighbours(np.ldexp(1.0, np.arange(-440, 441)))
    other = np.ldexp(rng.uniform(1.0, 2.0, p2.size), rng.integers(-440, 441, p2.size))
    # the range edges: |a|, |b| and |a / b| at 2^+-899
    big, small = 2.0 ** DIV_E, 2.0 ** -DIV_E
    ea_, eb_ = zip((big, 1.0), (small, 1.0), (1.0, big), (1.0, small), (big, big), (small, small),
                   (2.0 ** 450, 2.0 ** -449), (2.0 ** -450, 2.0 ** 449), (-big, 3.0), (small * 3, -3.0),
                   (1.5 * 2.0 ** 898, 1.25), (1.25, 1.5 * 2.0 ** 898), (big, 2.0 ** 898), (small, 2.0 ** -898))
    ha, hb = div_hard_cases(rng)
    return (np.concatenate([a, p2, other, ea_, ha]), np.concatenate([b, other, p2, eb_, hb]))


def in_div_range(v):
    v = np.abs(v)
    return np.all((v >= 2.0 ** -DIV_E) & (v <= 2.0 ** DIV_E))


def rsq_correctly_rounded(x):
    """The double nearest 1 / sqrt(x): np.longdouble's value (two 64-bit roundings, relative error
    below 2^-62) rounded to double, and mpmath wherever that lies too close to a rounding midpoint
    of the doubles (within 2^-8 ulp) for the longdouble value to decide."""
    ld = LD(1) / np.sqrt(x.astype(LD))
    cr = ld.astype(np.float64)
    frac = np.abs((ld - cr.astype(LD)) / np.spacing(cr).astype(LD))
    near = np.flatnonzero(np.abs(frac - LD(0.5)) < 2.0 ** -8)
    with mpmath.workprec(200):
        for k in near:
            cr[k] = float(1 / mpmath.sqrt(mpmath.mpf(float(x[k]))))
    return cr


# ---------------------------------------------------------------- sine / cosine table (c)
def pio2_multiples_near_doubles():
    """For every k < 2^20 / (pi / 2): the distance of k pi / 2 from its nearest double, in
    np.longdouble.  pi / 2 is split into three 40-bit pieces, so every k * piece is exact in the
    64-bit significand and (k p1 - d) is an exact difference of near-equal values."""
    with mpmath.workprec(200):
        rest, parts = mpmath.pi / 2, []
        for i in range(3):
            piece = mpmath.floor(mpmath.ldexp(rest, 39 + 40 * i)) / mpmath.mpf(2) ** (39 + 40 * i)
            parts.append(piece)
            rest -= piece
        # (exact conversions: each piece has 40 bits)
        p1, p2, p3 = (LD(int(mpmath.ldexp(p, 39 + 40 * i))) / LD(2) ** (39 + 40 * i) for i, p in enumerate(parts))
    k = np.arange(1, int(2.0 ** 20 / (math.pi / 2)) + 1).astype(LD)
    d = (k * p1 + k * p2).astype(np.float64)
    dist = ((k * p1 - d.astype(LD)) + k * p2) + k * p3
    return d, dist


def sincos_table():
    rng = np.random.default_rng(RNG_SEED + 3)
    n = 4096
    uni = np.concatenate([rng.uniform(-np.pi, np.pi, n), rng.uniform(-8, 8, n), rng.uniform(-100, 100, n),
                          rng.uniform(-2.0 ** 20, 2.0 ** 20, n)])
    offs = np.concatenate([[0.0], 10.0 ** np.arange(-15, -5), -(10.0 ** np.arange(-15, -5))])
    d, dist = pio2_multiples_near_doubles()
    # the multiples closest to a double (k = worst + 1), absolutely and in proportion to k (the
    # reduction's error grows with k: these have the largest relative error)
    worst = np.concatenate([np.argsort(np.abs(dist))[:8], np.argsort(np.abs(dist) / np.arange(1, d.size + 1))[:8]])
    ks = np.concatenate([np.arange(-8, 9), [1 << 10, 1 << 15, 1 << 19, 651000, d.size - 1, d.size,
                                            -(1 << 19), -d.size], worst + 1, -(worst + 1)])
    base = np.where(ks >= 0, d[np.abs(ks) - 1], -d[np.abs(ks) - 1])
    base[ks == 0] = 0.0
    near = (base[:, None] + offs[None, :]).ravel()
    special = np.array([0.0, -0.0, 5e-324, 1e-300, 1e-9, -1e-9])
    x = np.concatenate([uni, near, special])
    assert np.all(np.abs(x) < 2.0 ** 20)
    return x, int(worst[0]) + 1


def mp_sincos(x):
    """(sin, cos) of every double as mpmath values at 200 bits."""
    with mpmath.workprec(200):
        xs = [mpmath.mpf(float(v)) for v in x]
        return [mpmath.sin(v) for v in xs], [mpmath.cos(v) for v in xs]


def errors_vs_mp(got, ref):
    """(error in ulps of the double nearest the reference, absolute error) per point."""
    ulps, absol = np.zeros(len(ref)), np.zeros(len(ref))
    with mpmath.workprec(200):
        for i, (g, r) in enumerate(zip(got, ref)):
            e = abs(mpmath.mpf(float(g)) - r)
            absol[i] = float(e)
            rd = float(r)
            ulps[i] = float(e / mpmath.mpf(float(np.spacing(abs(rd))))) if rd != 0.0 else (0.0 if e == 0 else np.inf)
    return ulps, absol


# ---------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def host():
    """The default probe library; only its host entry point is used (no GPU needed)."""
    return prim_lib.load()


@pytest.fixture(scope="module")
def probe():
    if not gpu_available():
        pytest.skip("no GPU")
    return prim_lib.load()


@pytest.fixture(scope="module")
def probe_cal():
    if not gpu_available():
        pytest.skip("no GPU")
    return prim_lib.load(cal=True)


@pytest.fixture(scope="module")
def sqrt_x():
    return sqrt_table()


@pytest.fixture(scope="module")
def rcp_b():
    return rcp_table()


@pytest.fixture(scope="module")
def div_ab():
    return div_table()


@pytest.fixture(scope="module")
def sincos_x():
    return sincos_table()


# ---------------------------------------------------------------- table conditions (CPU)
def test_tables_stay_inside_the_documented_ranges(sqrt_x, rcp_b, div_ab):
    assert sqrt_x.size <= 1 << 16 and rcp_b.size <= 1 << 16 and div_ab[0].size <= 1 << 16
    assert np.all((sqrt_x >= 2.0 ** SQRT_LO) | (sqrt_x == 0)) and np.all(np.isfinite(sqrt_x))
    assert np.signbit(sqrt_x[sqrt_x == 0]).tolist() == [False, True]
    assert (sqrt_x == 2.0 ** SQRT_LO).any()
    assert in_div_range(rcp_b) and in_div_range(1.0 / rcp_b)
    for edge in (2.0 ** -DIV_E, 2.0 ** DIV_E):
        assert (np.abs(rcp_b) == edge).any()
    a, b = div_ab
    assert a.size == b.size and in_div_range(a) and in_div_range(b) and in_div_range(a / b)
    for edge in (2.0 ** -DIV_E, 2.0 ** DIV_E):
        assert (np.abs(a) == edge).any() and (np.abs(b) == edge).any() and (np.abs(a / b) == edge).any()


def test_hard_cases_lie_next_to_rounding_midpoints():
    """Exact integer arithmetic on the constructed central operands: how far the true root,
    respectively quotient, lies from a midpoint between two doubles (in ulps of the result)."""
    from fractions import Fraction

    def from_midpoint(v: Fraction, fb=80) -> Fraction:
        """|fraction of v's 53-bit significand - 1/2|, from v's floor at fb further bits"""
        k = int(v * (1 << 2000))
        cut = k.bit_length() - 53 - fb
        return abs(Fraction((k >> cut) & ((1 << fb) - 1), 1 << fb) - Fraction(1, 2))

    def root_from_midpoint(x: float) -> Fraction:
        r = math.isqrt(int(Fraction(x) * (1 << 4000)))        # sqrt(x) 2^2000, floor
        return from_midpoint(Fraction(r, 1 << 2000))

    rng = np.random.default_rng(RNG_SEED)
    n = 64
    xs = sqrt_hard_cases(rng, n)[:2 * n]
    assert {math.frexp(float(x))[1] & 1 for x in xs} == {0, 1}, "operands of even and of odd exponent"
    assert max(root_from_midpoint(float(x)) for x in xs[:n]) <= Fraction(36, 100)
    assert max(root_from_midpoint(float(x)) for x in xs[n:]) < Fraction(1, 1 << 30)
    a, b = div_hard_cases(rng, n)
    d = [from_midpoint(abs(Fraction(float(x)) / Fraction(float(y)))) for x, y in zip(a[:n], b[:n])]
    assert max(d[n // 2:]) < Fraction(1, 1 << 32)
    assert max(d[:n // 2]) <= Fraction(1, 2)


# ---------------------------------------------------------------- a. correctly rounded family
@pytest.mark.gpu
def test_sqrt_n_is_correctly_rounded(probe, sqrt_x):
    got = probe.unary("sqrt_n", sqrt_x)
    assert_bits_equal(got, np.sqrt(sqrt_x), [sqrt_x], "sqrt_n vs np.sqrt")   # (+-0 returns x: np.sqrt does too)


@pytest.mark.gpu
def test_rcp_n_is_correctly_rounded(probe, rcp_b):
    assert_bits_equal(probe.unary("rcp_n", rcp_b), 1.0 / rcp_b, [rcp_b], "rcp_n vs 1.0 / b")


@pytest.mark.gpu
def test_div_n_is_correctly_rounded(probe, div_ab):
    a, b = div_ab
    assert_bits_equal(probe.binary(a, b), a / b, [a, b], "div_n vs a / b")


@pytest.mark.gpu
def test_calibration_build_rsq_n_and_rcp_piv_are_the_rounded_forms(probe_cal, sqrt_x, rcp_b):
    """-DGM_CAL_TU: rsq_n is rcp_n(sqrt_n(x)), two correctly rounded operations, and rcp_piv is
    rcp_n; the family itself is the same code in both builds and is checked in both."""
    assert probe_cal.is_cal
    x = sqrt_x[sqrt_x > 0]
    assert_bits_equal(probe_cal.unary("rsq_n", x), 1.0 / np.sqrt(x), [x], "cal rsq_n vs 1.0 / np.sqrt")
    assert_bits_equal(probe_cal.unary("rcp_piv", rcp_b), 1.0 / rcp_b, [rcp_b], "cal rcp_piv vs 1.0 / b")
    assert_bits_equal(probe_cal.unary("sqrt_n", sqrt_x), np.sqrt(sqrt_x), [sqrt_x], "cal sqrt_n")
    assert_bits_equal(probe_cal.unary("rcp_n", rcp_b), 1.0 / rcp_b, [rcp_b], "cal rcp_n")


# ---------------------------------------------------------------- b. the refined, unrounded forms
@pytest.mark.gpu
def test_default_build_rsq_n_rcp_refined_rcp_piv_ulps(probe, sqrt_x, rcp_b):
    """Not correctly rounded by design (two Newton steps, no final correction).  The distance from
    the correctly rounded value (1.0 / b in float64 for the reciprocals; the longdouble / mpmath
    value rounded to double for rsq_n) stays within the measured maximum plus one ulp."""
    assert not probe.is_cal
    x = sqrt_x[sqrt_x > 0]
    d_rsq = ulps_apart(probe.unary("rsq_n", x), rsq_correctly_rounded(x))
    d_ref = ulps_apart(probe.unary("rcp_refined", rcp_b), 1.0 / rcp_b)
    d_piv = ulps_apart(probe.unary("rcp_piv", rcp_b), 1.0 / rcp_b)
    for name, d in (("rsq_n", d_rsq), ("rcp_refined", d_ref), ("rcp_piv", d_piv)):
        print(f"MEASURED {name}: max {int(d.max())} ulps; off by >= 1 ulp on {int((d > 0).sum())} of {d.size}")
    assert d_rsq.max() <= RSQ_N_BOUND
    assert d_ref.max() <= RCP_REFINED_BOUND
    assert d_piv.max() <= RCP_PIV_BOUND


# ---------------------------------------------------------------- c. sine and cosine
@pytest.mark.gpu
def test_device_sincos_equals_the_host_build_bit_for_bit(probe, sincos_x):
    x, _ = sincos_x
    hs, hc = probe.host_sincos(x)
    assert_bits_equal(probe.unary("gm_sin", x), hs, [x], "device gm_sin vs host gm_sincos")
    assert_bits_equal(probe.unary("gm_cos", x), hc, [x], "device gm_cos vs host gm_sincos")


def test_host_sincos_against_mpmath(host, sincos_x):
    """gm_sincos' host build against mpmath (200 bits) on the whole table; the device is tied to
    it by the bit-identity test above.  Next to non-zero multiples of pi / 2 the relative error
    is large (the two-term Cody-Waite reduction keeps about 86 bits of pi / 2), which is why the
    ulp bound holds only where |reference| >= 2^-10 and an absolute bound covers every point."""
    x, worst_k = sincos_x
    assert 1 <= worst_k <= int(2.0 ** 20 / (math.pi / 2))
    s, c = host.host_sincos(x)
    rs, rc = mp_sincos(x)
    worst_u, worst_a, worst_r = 0.0, 0.0, 0.0
    for got, ref in ((s, rs), (c, rc)):
        ulps, absol = errors_vs_mp(got, ref)
        mag = np.array([abs(float(r)) for r in ref])
        big = mag >= 2.0 ** -10
        small = ~big & (mag > 0)
        worst_u, worst_a = max(worst_u, ulps[big].max()), max(worst_a, absol.max())
        worst_r = max(worst_r, (absol[small] / mag[small]).max())
    print(f"MEASURED gm_sincos: max {worst_u:.4f} ulps where |ref| >= 2^-10, max abs error {worst_a:.4e}, "
          f"max relative error where |ref| < 2^-10 {worst_r:.4e}")
    assert worst_u <= SINCOS_B_ULPS
    assert worst_a <= SINCOS_A_ABS
    assert worst_r <= SINCOS_SMALL_REL


def test_host_sincos_reduction_at_power_of_two_multiples(host):
    """The reduction holds pi / 2 as 33 + 53 bits, the tail pio2_1t rounded to nearest: off by at
    most half an ulp of the tail, 2^-87.  A power of two k multiplies both parts exactly, so at
    the double nearest k pi / 2 the function that crosses zero there errs by at most k 2^-87,
    plus the last subtraction's and the polynomial's roundings (2 ulps of the tiny result allowed).
    A bound derived from the constants' description, not measured: a tail that is one ulp off in
    either direction exceeds it (the residual of the constants as they are is 3.52e-27 = 0.55 of
    2^-87)."""
    d, _ = pio2_multiples_near_doubles()
    ks = 2 ** np.arange(20)
    ks = ks[ks <= d.size]
    x = np.concatenate([d[ks - 1], -d[ks - 1]])
    s, c = host.host_sincos(x)
    rs, rc = mp_sincos(x)
    for i, k in enumerate(np.concatenate([ks, ks])):
        got, ref = (c[i], rc[i]) if k % 2 else (s[i], rs[i])
        assert abs(float(ref)) < 1e-9
        err = float(abs(mpmath.mpf(float(got)) - ref))
        assert err <= float(k) * 2.0 ** -87 + 2 * np.spacing(abs(float(ref))), (int(k), err / float(k))


def test_host_sincos_known_answers(host):
    s, c = host.host_sincos([0.0, -0.0])
    assert i64(c).tolist() == i64([1.0, 1.0]).tolist()
    assert i64(s[:1]).tolist() == [0]            # sin(+0.0) = +0.0
    # pinned as it is: the sign of zero is lost, gm_sin(-0.0) is +0.0 (libm gives -0.0)
    assert i64(s[1:]).tolist() == [0]


# ---------------------------------------------------------------- d. lane helpers
LANES = np.arange(64)
ROW, POS = LANES >> 4, LANES & 15


def lane_vectors():
    """Two wave inputs as bit patterns: doubles whose high and low words differ and both encode the
    lane, and a vector of NaN payloads (quiet and signalling), +-0 and subnormals."""
    l = LANES.astype(np.int64)
    v1 = (np.int64(0x3FF) << 52) | (l << 44) | (np.int64(0xABCD0000) + l)
    v2 = np.empty(64, dtype=np.int64)
    kinds = [lambda k: np.int64(0x7FF8000000000000) | (k << 32) | (0xDEAD0000 + k),      # quiet NaN payloads
             lambda k: np.int64(0x7FF0000000000000) | ((k + 1) << 20) | (0x100 + k),      # signalling NaNs
             lambda k: np.int64(-0x8000000000000000),                                     # -0.0
             lambda k: (k + 1) << 33 | (k + 7),                                           # subnormals, both words
             lambda k: np.int64(-0x8000000000000000) | (k + 1),                           # negative subnormals
             lambda k: np.int64(0)]                                                       # +0.0
    for k in range(64):
        v2[k] = kinds[k % 6 if k % 16 not in (0, 15) else k % 2](np.int64(k))            # (row edges: never 0 bits)
    return v1, v2


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1])
def test_row_moves_copy_bits(probe, which):
    """row_shr(off) at lane l is lane l - off of the same 16-lane row or +0.0 bits when that leaves
    the row, row_shl the mirror, row_bcast(k) lane 16 (l >> 4) + k, readlane_real(l') lane l'."""
    bits = lane_vectors()[which]
    out = i64(probe.lanes(bits.view(np.float64))).reshape(probe.n_slots, 64)
    for i, off in enumerate((1, 2, 4, 8)):
        shr = np.where(POS - off >= 0, bits[np.clip(LANES - off, 0, 63)], 0)
        shl = np.where(POS + off <= 15, bits[np.clip(LANES + off, 0, 63)], 0)
        np.testing.assert_array_equal(out[prim_lib.SLOT_SHR + i], shr, err_msg=f"row_shr({off})")
        np.testing.assert_array_equal(out[prim_lib.SLOT_SHL + i], shl, err_msg=f"row_shl({off})")
    for k in range(16):
        np.testing.assert_array_equal(out[prim_lib.SLOT_BCAST + k], bits[16 * ROW + k], err_msg=f"row_bcast({k})")
    for l in range(64):
        np.testing.assert_array_equal(out[prim_lib.SLOT_READLANE + l], np.full(64, bits[l]),
                                      err_msg=f"readlane_real({l})")


def row_totals_model(s):
    """gmf::row_totals in numpy float64, in its documented order: per 16-lane row the
    Hillis-Steele inclusive scan (every lane adds the lane `off` below it, 0 at the row edge,
    off = 1, 2, 4, 8), then ((row 0 + row 1) + row 2) + lane 56, all read after the scan."""
    s = np.array(s, dtype=np.float64)
    for off in (1, 2, 4, 8):
        t = np.where(POS - off >= 0, s[np.clip(LANES - off, 0, 63)], 0.0)
        s = s + t
    return ((s[15] + s[31]) + s[47]) + s[56]


@pytest.mark.gpu
@pytest.mark.parametrize("CL", [7, 8, 9, 10, 11, 12])
def test_row_totals(probe, CL):
    rng = np.random.default_rng(RNG_SEED + CL)
    on = ((ROW < 3) & (POS >= 1) & (POS <= CL)) | (LANES == 56)
    s = np.where(on, rng.standard_normal(64) * 10.0 ** rng.integers(-6, 7, 64), 0.0)
    got = probe.lanes(s)[prim_lib.SLOT_TOTALS]
    ref = row_totals_model(s)
    assert i64(got).tolist() == [int(i64([ref])[0])] * 64, "row_totals: wave-uniform, f64 sum in the documented order"
    n = int(on.sum())
    exact = s.astype(LD).sum()
    assert abs(LD(ref) - exact) <= n * 2.0 ** -53 * np.abs(s).sum()
    assert abs(LD(got[0]) - exact) <= n * 2.0 ** -53 * np.abs(s).sum()


def chain_system(L, CL, forward):
    """The dense CL x CL unit triangular systems of one row from the layout gm_arrow.h documents
    (index i = position i + 1): forward, x_p + sum_{k > p} L_p[k] x_k = y_p (leaf first: position
    CL is solved first); backward, x_p + sum_{j < p} L_p[j] x_j = y_p (root to leaf)."""
    A = np.eye(CL, dtype=LD)
    for p in range(1, CL + 1):
        for k in range(1, CL + 1):
            if (forward and k > p) or (not forward and k < p):
                A[p - 1, k - 1] = L[p, k]
    return A


def solve_triangular(A, Y, forward):
    """Substitution in np.longdouble on the dense matrix; Y may hold several right-hand sides."""
    n = A.shape[0]
    X = np.zeros(Y.shape, dtype=LD)
    order = range(n - 1, -1, -1) if forward else range(n)
    for i in order:
        X[i] = Y[i] - A[i] @ X          # (unknowns not yet solved are still 0 and A[i, i] X[i] = 0)
    return X


def chain_case(CL, forward):
    rng = np.random.default_rng(RNG_SEED + 100 * CL + forward)
    y = rng.standard_normal(64)
    L = rng.uniform(-1.0, 1.0, (64, 16))
    if not forward:
        # chain_backward masks j < p only: lanes above the chain would be rewritten with their own
        # multipliers, which the solves leave at zero and whose results they discard
        L[(POS < 1) | (POS > CL)] = 0.0
    return y, L


@pytest.mark.gpu
@pytest.mark.parametrize("forward", [True, False], ids=["forward", "backward"])
@pytest.mark.parametrize("CL", [7, 8, 9, 10, 11, 12])
def test_chain_substitutions(probe, probe_cal, CL, forward):
    """gmf::chain_forward<CL> / chain_backward<CL> on rows 0..2 against the np.longdouble solution
    x of the dense system A x = y.

    Bound.  Substitution in floating point gives x^ with (A + dA) x^ = y, |dA| <= gamma_CL |A|
    componentwise (Higham, Accuracy and Stability of Numerical Algorithms, theorem 8.5: each
    component takes at most CL - 1 multiply-subtract steps, in any order, and a fused step only
    drops a rounding).  Hence x - x^ = A^-1 dA x^ and |x - x^| <= gamma_CL |A^-1| |A| |x^|
    exactly, with gamma_CL = CL u / (1 - CL u) <= CL 2^-52 (u = 2^-53).  |A^-1| |A| |x^| is the
    growth of this L and y, computed from the case in longdouble (whose own error, 2^-11 of the
    bound, doubles nothing).  Lanes outside positions 1..CL and row 3 come back unchanged.  The
    unfused -DGM_CAL_TU build must also give the float64 recurrence in its written order bit for
    bit."""
    assert CL in probe.chain_lengths
    slot = prim_lib.SLOT_CHAINS + probe.chain_lengths.index(CL) + (0 if forward else len(probe.chain_lengths))
    y, L = chain_case(CL, forward)
    got = probe.lanes(y, L)[slot]
    got_cal = probe_cal.lanes(y, L)[slot]
    chain = (ROW < 3) & (POS >= 1) & (POS <= CL)
    np.testing.assert_array_equal(i64(got[~chain]), i64(y[~chain]), err_msg="lanes outside the chains changed")
    np.testing.assert_array_equal(i64(got_cal[~chain]), i64(y[~chain]))
    for f in range(3):
        lanes = 16 * f + np.arange(1, CL + 1)
        Lrow = np.zeros((CL + 1, CL + 1))
        Lrow[1:, :] = L[lanes, :CL + 1]
        A = chain_system(Lrow, CL, forward)
        x = solve_triangular(A, y[lanes].astype(LD), forward)
        Ainv = solve_triangular(A, np.eye(CL, dtype=LD), forward)
        bound = CL * 2.0 ** -52 * (np.abs(Ainv) @ (np.abs(A) @ np.abs(got[lanes]).astype(LD)))
        err = np.abs(got[lanes].astype(LD) - x)
        assert np.all(err <= bound), f"row {f}: error / bound {float((err / bound).max()):.3g}"
        # the written recurrence, unfused, in float64
        z = y[lanes].copy()
        pos = np.arange(1, CL + 1)
        for k in (range(CL, 0, -1) if forward else range(1, CL)):
            mult = np.where(pos < k if forward else k < pos, Lrow[1:, k], 0.0)
            z = z - mult * z[k - 1]
        np.testing.assert_array_equal(i64(got_cal[lanes]), i64(z), err_msg=f"row {f}: unfused recurrence")


# ---------------------------------------------------------------- e. gm_fphelpers.inc, both copies
N_HELPER_RANDOM = 256


def helper_cases():
    """[n][45] rows a[3] b[3] M[9] qa[4] qb[4] ci[10] v[6] w[6]: 256 random cases, then edges."""
    rng = np.random.default_rng(RNG_SEED + 5)
    edge_q = [[1, 0, 0, 0],
              [math.sqrt(0.5), math.sqrt(0.5), 0, 0], [math.sqrt(0.5), 0, 0, math.sqrt(0.5)],   # 90 degrees
              [0, 1, 0, 0], [0, 0, 0, 1], [0, math.sqrt(0.5), math.sqrt(0.5), 0],               # 180 degrees
              [0.5e-8, -0.5e-8, 0.5e-8, 0.5e-8], [0.5e8, 0.5e8, -0.5e8, 0.5e8],                 # norms 1e-8, 1e8
              [3e-17, -4e-17, 0, 0], [0, 0, 0, 0], [1e-16, 1e-16, 1e-16, 1e-16]]                # below the 1e-15 guard
    a0 = np.array([0.3, -1.7, 2.9])
    perp = np.array([1.7, 0.3, 0.0])
    edge_ab = [(a0, perp), (a0, 2.5 * a0), (a0, -a0), (a0, a0 * (1 + 1e-12) + 1e-13 * perp),
               (a0, a0 + np.array([0, 0, np.spacing(2.9)])), ([1.0, 0, 0], [0, 1.0, 0]), ([0, 0, 0], a0)]
    n = N_HELPER_RANDOM + max(len(edge_q), len(edge_ab))
    c = rng.standard_normal((n, 45)) * 10.0 ** rng.integers(-3, 4, (n, 1))
    for i, q in enumerate(edge_q):
        c[N_HELPER_RANDOM + i, 15:19] = q
    for i, (a, b) in enumerate(edge_ab):
        c[N_HELPER_RANDOM + i, 0:3], c[N_HELPER_RANDOM + i, 3:6] = a, b
    return c


def helpers_model(c, m=-1):
    """The helpers of gm_fphelpers.inc in their written operation order, in c's dtype: float64
    gives the unfused copy's bits (separately rounded IEEE operations), np.longdouble the
    high-precision value.  Every subtraction a - b is written a + m * b (m = -1: the same bits);
    m = +1 on |inputs| gives the sum of the terms' magnitudes.  Returns the 42 values dot3(a, b)
    cross3(a, b) mulmv3(M, a) mulmtv3(M, a) quat2mat(qa) quatmul(qa, qb) (23), inert_mul(ci, v)
    cross_motion(v, w) cross_force(v, w) dot6(v, w) (19); quatnorm is quatnorm_model's."""
    c = np.asarray(c)
    col = lambda lo, hi: [c[:, k] for k in range(lo, hi)]
    a, b, M, qa, qb, ci, v, w = col(0, 3), col(3, 6), col(6, 15), col(15, 19), col(19, 23), col(23, 33), col(33, 39), col(39, 45)

    def cross3(a, b):
        return [a[1] * b[2] + m * (a[2] * b[1]), a[2] * b[0] + m * (a[0] * b[2]), a[0] * b[1] + m * (a[1] * b[0])]

    dot3 = [a[0] * b[0] + a[1] * b[1] + a[2] * b[2]]
    mulmv3 = [M[3 * i] * a[0] + M[3 * i + 1] * a[1] + M[3 * i + 2] * a[2] for i in range(3)]
    mulmtv3 = [M[i] * a[0] + M[3 + i] * a[1] + M[6 + i] * a[2] for i in range(3)]
    qw, x, y, z = qa
    quat2mat = [1 + m * (2 * (y * y + z * z)), 2 * (x * y + m * (qw * z)), 2 * (x * z + qw * y),
                2 * (x * y + qw * z), 1 + m * (2 * (x * x + z * z)), 2 * (y * z + m * (qw * x)),
                2 * (x * z + m * (qw * y)), 2 * (y * z + qw * x), 1 + m * (2 * (x * x + y * y))]
    p, q = qa, qb
    quatmul = [p[0] * q[0] + m * (p[1] * q[1]) + m * (p[2] * q[2]) + m * (p[3] * q[3]),
               p[0] * q[1] + p[1] * q[0] + p[2] * q[3] + m * (p[3] * q[2]),
               p[0] * q[2] + m * (p[1] * q[3]) + p[2] * q[0] + p[3] * q[1],
               p[0] * q[3] + p[1] * q[2] + m * (p[2] * q[1]) + p[3] * q[0]]
    wv, u = v[:3], v[3:]
    Iw = [ci[0] * wv[0] + ci[3] * wv[1] + ci[4] * wv[2], ci[3] * wv[0] + ci[1] * wv[1] + ci[5] * wv[2],
          ci[4] * wv[0] + ci[5] * wv[1] + ci[2] * wv[2]]
    hxu, hxw = cross3(ci[6:9], u), cross3(ci[6:9], wv)
    inert_mul = [Iw[i] + hxu[i] for i in range(3)] + [ci[9] * u[i] + m * hxw[i] for i in range(3)]
    ca, cb, cc = cross3(v[:3], w[:3]), cross3(v[:3], w[3:]), cross3(v[3:], w[:3])
    cross_motion = ca + [cb[i] + cc[i] for i in range(3)]
    fa, fb, fc = cross3(v[:3], w[:3]), cross3(v[3:], w[3:]), cross3(v[:3], w[3:])
    cross_force = [fa[i] + fb[i] for i in range(3)] + fc
    dot6 = [v[0] * w[0] + v[1] * w[1] + v[2] * w[2] + v[3] * w[3] + v[4] * w[4] + v[5] * w[5]]
    cols = dot3 + cross3(a, b) + mulmv3 + mulmtv3 + quat2mat + quatmul + inert_mul + cross_motion + cross_force + dot6
    return np.stack([np.broadcast_to(k, c.shape[:1]) for k in cols], axis=1)


# terms per output value (a product counts once, the constant 1 of quat2mat's diagonal too), in
# helpers_model's order: the n of gamma_n
HELPER_TERMS = np.array([3] + [2] * 3 + [3] * 3 + [3] * 3 + [3, 2, 2, 2, 3, 2, 2, 2, 3] + [4] * 4 +
                        [5] * 3 + [3] * 3 + [2] * 3 + [4] * 3 + [4] * 3 + [2] * 3 + [6])


def quatnorm_model(q, dtype=np.float64):
    """quatnorm's file-scope copy in its written order (dtype float64: its bits)."""
    q = q.astype(dtype)
    n2 = q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3]
    n = np.sqrt(n2)
    small = n < 1e-15
    with np.errstate(divide="ignore", invalid="ignore"):
        out = q * (dtype(1.0) / n)[:, None]
    out[small] = [1, 0, 0, 0]
    return out, small


@pytest.fixture(scope="module")
def helper_c():
    return helper_cases()


def split_helpers(out):
    """(file-scope copy [n][23], its quatnorm [n][4], gmf copy [n][23 + 19], its quatnorm [n][4])"""
    return out[:, 0:23], out[:, 23:27], np.concatenate([out[:, 27:50], out[:, 54:73]], axis=1), out[:, 50:54]


@pytest.mark.gpu
def test_helpers_file_scope_copy_is_the_written_float64_expression(probe, helper_c):
    fs, fs_qn, _, _ = split_helpers(probe.helpers(helper_c))
    ref = helpers_model(helper_c)[:, :23]
    np.testing.assert_array_equal(i64(fs), i64(ref))
    qn, small = quatnorm_model(helper_c[:, 15:19])
    assert small.sum() >= 3
    np.testing.assert_array_equal(i64(fs_qn), i64(qn))


@pytest.mark.gpu
def test_helpers_physics_copy_within_the_dot_product_bound(probe, helper_c):
    """namespace gmf is compiled with FMA contraction, so its values are not the float64
    expression's bits; each is a sum of n products evaluated with at most n roundings per term,
    fused or not, hence within gamma_n sum|terms| of the exact value, gamma_n = n u / (1 - n u),
    u = 2^-53 (the standard dot-product bound; the longdouble reference's own error, n 2^-64
    sum|terms|, is added).  gmf::quatnorm calls rsq_n where the file-scope copy calls
    rcp_n(sqrt_n): each component within rsq_n's bound plus 2 ulps of q / |q| in longdouble."""
    _, _, ph, ph_qn = split_helpers(probe.helpers(helper_c))
    ref = helpers_model(helper_c.astype(LD))
    mags = helpers_model(np.abs(helper_c).astype(LD), m=+1)
    nu = HELPER_TERMS * LD(2.0) ** -53
    bound = (nu / (1 - nu) + HELPER_TERMS * LD(2.0) ** -64) * mags
    err = np.abs(ph.astype(LD) - ref)
    bad = np.argwhere(err > bound)
    assert bad.size == 0, f"first at case {bad[0][0]} value {bad[0][1]}: {float(err[tuple(bad[0])])} > {float(bound[tuple(bad[0])])}"
    qn, small = quatnorm_model(helper_c[:, 15:19], LD)
    np.testing.assert_array_equal(ph_qn[small], np.tile([1.0, 0, 0, 0], (int(small.sum()), 1)))
    big = ~small
    cr = qn[big].astype(np.float64)
    ulps = np.abs(ph_qn[big].astype(LD) - qn[big]) / np.spacing(np.abs(cr)).astype(LD)
    nz = cr != 0
    assert np.all(ph_qn[big][~nz] == 0)
    print(f"MEASURED gmf::quatnorm: max {float(ulps[nz].max()):.3f} ulps")
    assert ulps[nz].max() <= RSQ_N_BOUND + 2


@pytest.mark.gpu
def test_helpers_calibration_build_copies_agree(probe_cal, helper_c):
    """-DGM_CAL_TU: namespace gmf is unfused and its rsq_n is rcp_n(sqrt_n), so its copy equals
    the file-scope copy bit for bit, and the gmf-only helpers the written float64 expression."""
    fs, fs_qn, ph, ph_qn = split_helpers(probe_cal.helpers(helper_c))
    np.testing.assert_array_equal(i64(ph[:, :23]), i64(fs))
    np.testing.assert_array_equal(i64(ph_qn), i64(fs_qn))
    np.testing.assert_array_equal(i64(ph), i64(helpers_model(helper_c)))


# ---------------------------------------------------------------- f. the discrete chooser
M64 = (1 << 64) - 1


def mix_int(z: int) -> int:
    """gp_mix on a Python integer (splitmix64's finaliser), independent of numpy's wrap-around."""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def mix_words():
    rng = np.random.default_rng(RNG_SEED + 6)
    wrap = M64 + 1 - 0x9E3779B97F4A7C15          # z + golden wraps to exactly 0
    crafted = [0, M64, wrap, wrap - 1, wrap + 1, 1 << 63, (1 << 63) - 1, 1, 0x9E3779B97F4A7C15, M64 - 1]
    return np.concatenate([np.array(crafted, dtype=np.uint64), rng.integers(0, M64, 4096, dtype=np.uint64, endpoint=True)])


def softmax64(logits):
    x = np.asarray(logits, dtype=np.float32).astype(np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def choose_mirror(logits, eps, seed, decision, gid0):
    """gp_choose from the header's comment: h1 = mix(seed ^ mix(gid 0x100000001B3 + decision)),
    h2 = mix(h1), u = (h1 >> 40) / 2^24; a random action h2 % n_out when u < eps (eps as f32), else
    the first maximum of the f64 softmax.  Returns (actions, random mask, greedy actions, u)."""
    n, n_out = logits.shape
    gid = [(gid0 + i) & M64 for i in range(n)]
    h1 = [mix_int(seed ^ mix_int((g * 0x100000001B3 + decision) & M64)) for g in gid]
    h2 = np.array([mix_int(h) % n_out for h in h1])
    u = np.array([(h >> 40) / 16777216.0 for h in h1])
    rand = u < float(np.float32(eps))
    greedy = np.argmax(softmax64(logits), axis=1)
    return np.where(rand, h2, greedy), rand, greedy, u


CHOOSE_SEED, CHOOSE_DECISION = 0xC0FFEE1234567, 41
CHOOSE_GID0 = (1 << 32) - 512          # 1024 rows: global env ids on both sides of 2^32
N_OUTS = (1, 2, 8, 37)


def clear_logits(n_out, n=1024):
    """n logit rows whose f64 top-two softmax gap exceeds 4 Q_ATOL: the greedy action is then
    unambiguous for an f32 softmax within Q_ATOL of it."""
    rng = np.random.default_rng(RNG_SEED + 7 + n_out)
    x = (2.0 * rng.standard_normal((2 * n, n_out))).astype(np.float32)
    if n_out > 1:
        top2 = np.sort(softmax64(x), axis=1)[:, -2:]
        x = x[(top2[:, 1] - top2[:, 0]) > 4 * Q_ATOL]
    assert x.shape[0] >= n
    return np.ascontiguousarray(x[:n])


def test_mix_mirrors_agree():
    """gmx.policy._mix (numpy uint64) against the Python-integer form on the crafted words."""
    z = mix_words()
    assert _mix(z).tolist() == [mix_int(int(v)) for v in z]
    assert mix_int(0) == 0xE220A8397B1DCDAF      # splitmix64's first output for seed 0 (known answer)


@pytest.mark.parametrize("n_out", N_OUTS)
def test_chooser_inputs_draw_about_eps_random_rows(n_out):
    """A condition on the inputs, not on the kernel: with eps = 0.3 the mirror draws a random
    action on 25 % to 35 % of the 1024 rows, and ids on both sides of 2^32 are among them."""
    x = clear_logits(n_out)
    _, rand, _, u = choose_mirror(x, 0.3, CHOOSE_SEED, CHOOSE_DECISION, CHOOSE_GID0)
    assert 0.25 <= rand.mean() <= 0.35
    assert rand[:512].any() and rand[512:].any() and not rand[:512].all() and not rand[512:].all()
    assert np.all((u >= 0) & (u < 1))


@pytest.mark.gpu
def test_mix(probe):
    z = mix_words()
    assert probe.mix(z).tolist() == _mix(z).tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("eps", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("n_out", N_OUTS)
def test_choose_equals_the_mirror(probe, n_out, eps):
    x = clear_logits(n_out)
    ref, rand, greedy, _ = choose_mirror(x, eps, CHOOSE_SEED, CHOOSE_DECISION, CHOOSE_GID0)
    assert rand.all() if eps == 1.0 else (not rand.any() if eps == 0.0 else True)
    act, q, qbest = probe.choose(x, eps, CHOOSE_SEED, CHOOSE_DECISION, CHOOSE_GID0)
    np.testing.assert_array_equal(act, ref)
    np.testing.assert_allclose(q, softmax64(x), rtol=0, atol=Q_ATOL)
    np.testing.assert_array_equal(qbest.view(np.int32), q[np.arange(len(x)), greedy].view(np.int32))


@pytest.mark.gpu
def test_choose_u_below_eps_is_strict_and_ids_are_64_bit(probe):
    """eps set to one row's own u (a 24-bit fraction, exact in f32): that row stays greedy (u < eps
    is strict) while rows with a smaller u draw; a second call far above 2^32 checks that the id
    enters the hash with all 64 bits."""
    x = clear_logits(8)
    for gid0 in (CHOOSE_GID0, (1 << 63) + 12345):
        _, _, _, u = choose_mirror(x, 0.0, CHOOSE_SEED, 7, gid0)
        k = int(np.argsort(u)[len(u) // 3])
        eps = float(u[k])
        assert float(np.float32(eps)) == eps
        ref, rand, greedy, _ = choose_mirror(x, eps, CHOOSE_SEED, 7, gid0)
        assert not rand[k] and rand.sum() >= 300
        act, _, _ = probe.choose(x, eps, CHOOSE_SEED, 7, gid0)
        np.testing.assert_array_equal(act, ref)
        assert act[k] == greedy[k]
    # (the two id ranges give different draws: the id is not truncated to 32 bits)
    a = choose_mirror(x, 1.0, CHOOSE_SEED, 7, 5)[0]
    b = choose_mirror(x, 1.0, CHOOSE_SEED, 7, (1 << 32) + 5)[0]
    assert (a != b).any()
    np.testing.assert_array_equal(probe.choose(x, 1.0, CHOOSE_SEED, 7, (1 << 32) + 5)[0], b)


@pytest.mark.gpu
def test_choose_crafted_rows(probe):
    """eps = 0 on crafted rows: the first maximum wins, ties after rounding pick one of the tied
    actions, extreme logits give exact 0 and 1 and never a NaN."""
    ninf = -np.inf
    rows = np.array([[0.25] * 8,                                      # 0: all equal -> action 0
                     [0, 1, -1, 2.5, 0, 2.5, 1, -3],                  # 1: equal maxima at 3 and 5 -> 3
                     [-5, -5, -1e-9, -5, -5, 0, -5, -5],              # 2: equal only after rounding -> 2 or 5
                     [1, -2, 0.5, 3, 203, 2, -1, 0],                  # 3: one logit 200 above the rest
                     [1e30, -1e30, 1e30, -1e30, -1e30, 1e30, 1e30, -1e30],   # 4
                     [-1e30, 3, 1e30, -1e30, 0, -1e30, 5, -1e30],     # 5
                     [0.5, ninf, 1.5, 0, -0.5, 1, 0.25, -1]],         # 6: one -inf entry
                    dtype=np.float32)
    act, q, qbest = probe.choose(rows, 0.0, CHOOSE_SEED, CHOOSE_DECISION, 0)
    assert not np.isnan(q).any() and not np.isnan(qbest).any()
    np.testing.assert_allclose(q, softmax64(rows), rtol=0, atol=Q_ATOL)
    np.testing.assert_array_equal(qbest.view(np.int32), q[np.arange(len(rows)), act].view(np.int32))
    np.testing.assert_array_equal(qbest, q.max(axis=1))
    assert act[0] == 0 and np.all(q[0] == np.float32(0.125))
    assert act[1] == 3 and q[1, 3] == q[1, 5]
    assert act[2] in (2, 5)
    assert act[3] == 4 and q[3, 4] == 1.0 and np.all(np.delete(q[3], 4) == 0.0)
    assert act[4] == 0 and np.all(q[4, [0, 2, 5, 6]] == np.float32(0.25)) and np.all(q[4, [1, 3, 4, 7]] == 0.0)
    assert act[5] == 2 and q[5, 2] == 1.0 and np.all(np.delete(q[5], 2) == 0.0)
    assert act[6] == 2 and q[6, 1] == 0.0 and np.all(np.delete(q[6], 1) > 0.0)
