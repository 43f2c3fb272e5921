"""CPU checks of tests/exact_filters.py -- the exact reference the GPU filter tests (tests/test_gpu_filters.py) classify pairs by -- and
of the oracle's sphere_disc export."""
from fractions import Fraction

import mpmath
import numpy as np
import pytest

import exact_filters as X


def _mp_D(o, c, r, d):
    with mpmath.workprec(300):
        oc = [mpmath.mpf(float(o[k])) - mpmath.mpf(float(c[k])) for k in range(3)]
        hb = sum(oc[k] * mpmath.mpf(float(d[k])) for k in range(3))
        return hb * hb - sum(x * x for x in oc) + mpmath.mpf(float(r)) ** 2


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_exact_D_agrees_with_mpmath_at_300_bits(T):
    """300 bits hold every D of binary32 / binary64 inputs of exponent within +-100 exactly: the two must be equal, not close"""
    rng = np.random.default_rng(5)
    for k in (-100, -40, -12, 0, 7, 40, 100):
        for _ in range(40):
            o = (rng.normal(size=3) * 2.0 ** k).astype(T)
            c = (rng.normal(size=3) * 2.0 ** k).astype(T)
            d = rng.normal(size=3)
            d = (d / np.linalg.norm(d)).astype(T)
            r = T(abs(rng.normal()) * 2.0 ** k)
            e = X.exact_D(o, c, r, d)
            m = _mp_D(o, c, r, d)
            with mpmath.workprec(300):
                assert mpmath.mpf(e.numerator) / mpmath.mpf(e.denominator) == m


def test_D_cmp_decides_exactly_near_the_threshold():
    """the binary64 prefilter hands every pair within its error bound to Fractions: random pairs and thresholds AT the exact D"""
    rng = np.random.default_rng(6)
    n = 300
    o = rng.normal(size=(n, 3)).astype(np.float32).astype(np.float64)
    c = rng.normal(size=(n, 3)).astype(np.float32).astype(np.float64)
    d = rng.normal(size=(n, 3)).astype(np.float32).astype(np.float64)
    r = np.abs(rng.normal(size=n)).astype(np.float32).astype(np.float64)
    t = np.array([float(X.exact_D(o[i], c[i], r[i], d[i])) for i in range(n)])
    got = X.D_cmp(o, c, r, d, t)
    want = np.array([np.sign(X.exact_D(o[i], c[i], r[i], d[i]) - Fraction(t[i])) for i in range(n)])
    assert np.array_equal(got, want)
    assert (got == 0).sum() + (got != 0).sum() == n


@pytest.mark.parametrize("k", [-60, -30, -8, 0, 1, 13, 30, 60])
def test_constructed_tangent_rays_have_D_zero(k):
    """integer tangency scaled by powers of two: c = 0, r = 1, o = (1, 0, -5), d = (0, 0, 1); r = 5, o = (3, 4, -7); offset centres"""
    s = 2.0 ** k
    cases = [((1, 0, -5), (0, 0, 0), 1, (0, 0, 1)), ((3, 4, -7), (0, 0, 0), 5, (0, 0, 1)), ((-4, 11, 3), (-1, 7, 0), 5, (0, 0, -1)),
             ((-13, 0, 5), (0, 0, 0), 5, (1, 0, 0))]
    for o, c, r, d in cases:
        for T in (np.float32, np.float64):
            o_ = np.array(o, np.float64) * s
            c_ = np.array(c, np.float64) * s
            if T is np.float32 and not (np.float32(s * 13) > 0 and np.isfinite(np.float32(s * 13))):
                continue
            assert X.exact_D(o_.astype(T), c_.astype(T), T(r * s), np.array(d, T)) == 0


def test_bands_positive_over_the_accepted_range():
    """M - E (matrix pipe) and the binary32 filter's band are positive for every sphere and ray the filters accept: scales 2^-40 .. 2^40,
    |c| s up to 2^8, |o|_inf up to mf_o_max, r from 0 to the scene extent; the Float64 band for |c|, r up to 1e15 and |o|^2 < 1e30"""
    rng = np.random.default_rng(7)
    for ex in range(-40, 41, 4):
        s = 2.0 ** (8 - ex)
        _, _, omax = X.mfma_ray_constants(s)
        n = 4000
        c = rng.uniform(-1, 1, (n, 3)) * 2.0 ** ex
        c[:8] = 0.0
        r = rng.uniform(0, 1, n) * 2.0 ** ex
        r[8:16] = 0.0
        o = rng.uniform(-1, 1, (n, 3)) * omax
        o[16:24] = 0.0
        o[24:32] = omax
        b = X.mfma_band(o, c, r, s)
        assert (b > 0).all(), (ex, b.min())
        assert X.mfma_scale(np.concatenate([c, [[2.0 ** ex * 0.75, 0, 0]]]), np.concatenate([r, [0.0]])) == s
    for k in range(-100, 51, 5):
        n = 2000
        c = rng.uniform(-1, 1, (n, 3)) * 2.0 ** k
        r = rng.uniform(0, 1, n) * 2.0 ** k
        r[:10] = 0.0
        o = rng.uniform(-1, 1, (n, 3)) * min(2.0 ** (k + 6), 5e14)
        b = X.f64_filter_band(o, c, r)
        assert (b > 0).all(), (k, b.min())


def test_mfma_scale_limits():
    assert X.mfma_scale(np.array([[1.0, 0, 0]]), np.array([0.5])) == 2.0 ** 7
    assert X.mfma_scale(np.array([[2.0 ** 39 * 1.5, 0, 0]]), np.array([1.0])) == 2.0 ** -32     # emax <= 2^40 (frexp)
    assert X.mfma_scale(np.array([[2.0 ** 40, 0, 0]]), np.array([1.0])) is None                 # 2^41: the VALU scan
    assert X.mfma_scale(np.array([[2.0 ** -41, 0, 0]]), np.array([0.0])) == 2.0 ** 48
    assert X.mfma_scale(np.array([[2.0 ** -42, 0, 0]]), np.array([0.0])) is None
    assert X.mfma_scale(np.array([[0.0, 0, 0]]), np.array([0.0])) is None


@pytest.mark.usefixtures("numerics")
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_oracle_sphere_disc_is_the_deciding_value(oracle, T):
    """rtwo_sphere_disc returns the value hit_sphere tests: disc >= 0 (a -0 included) exactly where hit_sphere with an infinite
    interval finds a root (one is always >= -inf); and the sign of a zero is kept"""
    rng = np.random.default_rng(8)
    n = 400
    c = rng.normal(size=(n, 3)).astype(T)
    r = np.abs(rng.normal(size=n)).astype(T)
    o = rng.normal(size=(n, 3)).astype(T) * T(2)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(T)
    disc, hb = oracle.sphere_disc(c, r, o, d, T, half_b=True)
    assert disc.dtype == T and hb.dtype == T
    for i in range(n):
        hit = oracle.hit_sphere(c[i], r[i], o[i], d[i], -np.inf, np.inf, T) is not None
        assert hit == (not disc[i] < 0), i
    # the exact tangent: D == 0 in every mode for small integers
    z = oracle.sphere_disc([0, 0, 0], [1], [1, 0, -5], [0, 0, 1], T)
    assert z[0] == 0 and not np.signbit(z[0])
