"""Exact reference for the pass-1 filters of the closest-hit scans, and the guarantees their comments document.

Pass 1 of every scan only has to flag a SUPERSET of the spheres whose deciding discriminant is >= 0; three of the filters rest on a
hand-written error budget (raytracingweekend.jl_amd/csrc):
  * the matrix-pipe filter of hit_world_mfma (rtw_scan_mfma.hpp:27-62; margin constants set in rtw_scene.hip build_mfma_operands),
  * the binary32 filter of hit_world<double> (rtw_scan.hpp, the comment in front of `lane_ok`; G set in rtw_scene.hip upload_scene),
  * the margin form of reference_fma2 in hit_world<float> (no slack: covered by the superset test only).
This module is the checker's side: the exact discriminant of the actual inputs, and the band below zero inside which each filter
guarantees a candidate.  A helper module, not a conftest.py."""
from fractions import Fraction
import math

import numpy as np

U24 = 2.0 ** -24            # binary32 unit roundoff
MF_S2_MAX = 1.0009          # hit_world_mfma: rays with fma(dz, dz, fma(dy, dy, dx * dx)) <= 1.0009f use the filter (binary32 literal)
F64_S2_MAX = 1.001          # hit_world<double>: dot(d, d) <= 1.001 ...
F64_O2_MAX = 1e30           # ... and dot(o, o) < 1e30


def _fr(x):
    return Fraction(float(x))


def exact_D(o, c, r, d):
    """D = (d.(o - c))^2 - |o - c|^2 + r^2 of the actual input values (binary32 or binary64 scalars / 3-sequences), exactly: a Fraction."""
    oc = [_fr(o[k]) - _fr(c[k]) for k in range(3)]
    dd = [_fr(d[k]) for k in range(3)]
    hb = oc[0] * dd[0] + oc[1] * dd[1] + oc[2] * dd[2]
    rr = _fr(r)
    return hb * hb - (oc[0] * oc[0] + oc[1] * oc[1] + oc[2] * oc[2]) + rr * rr


def D_approx(o, c, r, d):
    """D in binary64 for [n, 3] / [n] arrays (numpy broadcasting), with a rigorous bound on its error: (D64, err).
    The inputs are binary32 or binary64 values; every binary64 operation adds at most 2^-53 of its result, ten of them of
    terms bounded by |d|^2 |o - c|^2 + |o - c|^2 + r^2: err = 2^-46 x that sum (a factor 8 to spare)."""
    o, c, d = (np.asarray(a, np.float64) for a in (o, c, d))
    r = np.asarray(r, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        oc = o - c
        hb = (oc * d).sum(-1)
        ococ = (oc * oc).sum(-1)
        D = hb * hb - ococ + r * r
        err = 2.0 ** -46 * ((d * d).sum(-1) * ococ + ococ + r * r)
    return D, err


def D_cmp(o, c, r, d, t):
    """sign(D - t) for every pair, EXACT (int8 array: -1, 0, +1): binary64 where it is decisive, Fractions where D lies within the
    binary64 error of the threshold t (a binary64 array or scalar)."""
    D, err = D_approx(o, c, r, d)
    shape = np.broadcast(D, np.asarray(t, np.float64)).shape
    t = np.broadcast_to(np.asarray(t, np.float64), shape)
    D = np.broadcast_to(D, shape)
    err = np.broadcast_to(err, shape)
    with np.errstate(invalid="ignore"):
        diff = D - t
        bound = err + 2.0 ** -52 * np.abs(t) + 2.0 ** -52 * np.abs(D)
        out = np.where(diff > bound, 1, np.where(diff < -bound, -1, 0)).astype(np.int8)
        out = np.where(np.isinf(t), np.where(t < 0, 1, -1), out).astype(np.int8)       # (an infinite band: every finite D is inside)
        near = ~((diff > bound) | (diff < -bound)) & np.isfinite(t)
    if near.any():
        ob, cb, db = (np.broadcast_to(np.asarray(a, np.float64), shape + (3,)) for a in (o, c, d))
        rb = np.broadcast_to(np.asarray(r, np.float64), shape)
        for ix in zip(*np.nonzero(near)):
            e = exact_D(ob[ix], cb[ix], rb[ix], db[ix]) - _fr(t[ix])
            out[ix] = (e > 0) - (e < 0)
    return out


# ---- the matrix-pipe filter (hit_world_mfma) ---------------------------------------------------------------------------------
A_S = 2.0 ** -17            # rtw_scene.hip build_mfma_operands: A_S = 32 x 2^-22
A_R = 12.0 * 2.0 ** -22     # ... A_r = 12 x 2^-22


def mfma_scale(c, r):
    """mf_sc of a scene (rtw_scene.hip build_mfma_operands): 2^(8 - ex), emax <= 2^ex the largest |c_k| (rounded to binary32) or |r|;
    None where the scene gets no matrix-pipe operands (|ex| > 40)."""
    c = np.asarray(c, np.float64).astype(np.float32).astype(np.float64)
    r2 = np.asarray(r, np.float64) ** 2
    emax = max(float(np.abs(c).max()), float(np.sqrt(np.abs(r2)).max()))
    if not emax > 0 or not math.isfinite(emax):
        return None
    ex = math.frexp(emax)[1]
    if ex > 40 or ex < -40:
        return None
    return 2.0 ** (8 - ex)


def mfma_ray_constants(s):
    """(mf_oo_keep, mf_o1_coef, mf_o_max) as uploaded (binary32, rounded in the safe direction), for scale s"""
    phi_c = 2.0 ** -25 / s
    keep = np.float32(1.0 - 1.02 * 2 * A_S)
    if float(keep) > 1.0 - 1.02 * 2 * A_S:
        keep = np.nextafter(keep, np.float32(0))
    coef = np.float32(1.02 * 9 * phi_c)
    if float(coef) < 1.02 * 9 * phi_c:
        coef = np.nextafter(coef, np.float32(np.inf))
    return float(keep), float(coef), float(np.float32(2.0 ** 13 / s))


def mfma_band(o, c, r, s):
    """M - E for pairs of ray origins o [n, 3] and spheres (c [n, 3], r [n]) at scale s (broadcasting): every pair with
    D >= -(M - E) is flagged for a ray that uses the filter (ok).
      M: the sphere's margin Gs as uploaded (rtw_scan_mfma.hpp:59 / rtw_scene.hip build_mfma_operands, the remainder of k' s^2 rounded
         up only widens it) plus the ray's share |o|^2 - oo' = (1 - mf_oo_keep) |o|^2 + mf_o1_coef |o|_1 (rtw_scan_mfma.hpp:61-62; the
         rounding of oo' itself is a term of E);
      E: rtw_scan_mfma.hpp:56-58, 2^-22 (35.9 |c|^2 + 28.7 |o|^2 + 5 r^2) + floors, floors = phi_c (5.5 |o|_1 + |c|_1) + 1.4 phi_k, plus
         the 4 Gs of the MFMA accumulation term (rtw_scan_mfma.hpp:48) that line 56 leaves out; c and r in binary32 as the operands hold them."""
    o = np.asarray(o, np.float64)
    c = np.asarray(c, np.float64).astype(np.float32).astype(np.float64)
    r2 = np.asarray(r, np.float64) ** 2
    phi_c, phi_k = 2.0 ** -25 / s, 2.0 ** -20 / (s * s)
    c2, c1 = (c * c).sum(-1), np.abs(c).sum(-1)
    o2, o1 = (o * o).sum(-1), np.abs(o).sum(-1)
    Gs = 1.02 * ((2 * A_S + A_R) * c2 + A_R * r2 + 9 * phi_c * c1 + 1.5 * phi_k)
    keep, coef, _ = mfma_ray_constants(s)
    M = Gs + (1.0 - keep) * o2 + coef * o1
    E = 2.0 ** -22 * (35.9 * c2 + 28.7 * o2 + 5 * r2 + 4 * Gs) + phi_c * (5.5 * o1 + c1) + 1.4 * phi_k
    return M - E


# ---- the binary32 filter of hit_world<double> -----------------------------------------------------------------------------------
def f64_G(c, r):
    """G as uploaded (rtw_scene.hip upload_scene): 1.01 (2^-18 r^2 + 2^-20 |c|^2 + 2^-20 r^2) + 1e-30, rounded up to binary32; inf for
    astronomically large spheres"""
    c = np.asarray(c, np.float64)
    r2 = np.asarray(r, np.float64) ** 2
    c2 = (c * c).sum(-1)
    G = 1.01 * (2.0 ** -18 * r2 + 2.0 ** -20 * c2 + 2.0 ** -20 * r2) + 1e-30
    with np.errstate(over="ignore"):
        g = G.astype(np.float32)
    g = np.where(g.astype(np.float64) < G, np.nextafter(g, np.float32(np.inf)), g).astype(np.float64)
    return np.where((c2 < 1e30) & (r2 < 1e30), g, np.inf)


def f64_filter_band(o, c, r):
    """2^-18 |o - c|^2 + G - 2^-18 r^2 - Err (rtw_scan.hpp, the comment of hit_world's binary32 filter):
    Err = u [28.5 |o - c|^2 + 12.2 |c|^2 + 6.1 r^2 + 2 G], u = 2^-24.  Every pair with D >= -band is flagged for an ok ray."""
    o, c = np.asarray(o, np.float64), np.asarray(c, np.float64)
    r2 = np.asarray(r, np.float64) ** 2
    oc = o - c
    ococ, c2 = (oc * oc).sum(-1), (c * c).sum(-1)
    G = f64_G(c, np.asarray(r, np.float64))
    with np.errstate(invalid="ignore"):
        err = U24 * (28.5 * ococ + 12.2 * c2 + 6.1 * r2 + 2 * G)
        return np.where(np.isinf(G), np.inf, 2.0 ** -18 * ococ + G - 2.0 ** -18 * r2 - err)     # (G = inf: always a candidate)


def f32_mf_ok(o, d, s):
    """which rays use the matrix-pipe filter (hit_world_mfma `ok`), evaluated as the kernel does in binary32"""
    o = np.asarray(o, np.float64).astype(np.float32)
    d = np.asarray(d, np.float64).astype(np.float32)
    _, _, omax = mfma_ray_constants(s)
    with np.errstate(invalid="ignore", over="ignore"):
        s2 = np.array([_fma32(d[i, 2], d[i, 2], _fma32(d[i, 1], d[i, 1], d[i, 0] * d[i, 0])) for i in range(len(d))], np.float32)
        oinf = np.abs(o).max(-1)
        return (s2 <= np.float32(MF_S2_MAX)) & (oinf <= np.float32(omax)) & np.isfinite(oinf) & np.isfinite(s2)


def _fma32(a, b, c):
    """binary32 fma(a, b, c), correctly rounded (exact product and sum in Fractions)"""
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return np.float32(a * b + c)
    x = Fraction(a) * Fraction(b) + Fraction(c)
    return round_f32(x)


def round_f32(x):
    """a Fraction rounded to the nearest binary32 (ties to even, subnormals, overflow to inf)"""
    if x == 0:
        return np.float32(0.0)
    f = float(x)                                       # binary64 first: correct except for a double rounding ...
    g = np.float32(f)
    if not np.isfinite(g):
        return g
    # ... which can only matter when x lies exactly halfway between two binary32 values after the first rounding: check the neighbours
    best = g
    for cand in (np.nextafter(g, np.float32(-np.inf)), np.nextafter(g, np.float32(np.inf))):
        if abs(Fraction(float(cand)) - x) < abs(Fraction(float(best)) - x):
            best = cand
    return best


def f64_ok(o, d):
    """which rays use hit_world<double>'s binary32 filter (lane_ok)"""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        o2 = (o[:, 0] * o[:, 0] + o[:, 1] * o[:, 1]) + o[:, 2] * o[:, 2]
        return (s2 <= F64_S2_MAX) & (o2 < F64_O2_MAX)
