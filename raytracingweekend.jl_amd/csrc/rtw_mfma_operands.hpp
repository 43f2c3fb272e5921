// rtw_mfma_operands.hpp -- host side of the matrix-pipe filter's K = 32 contraction (rtw_scan_mfma.hpp holds the slot table, the error
// budget and the coarse margin): the scale constants of a scene, the sphere-side operand words of one row, and a host MIRROR of the ray-side
// words that the scan's prologue builds on the device.  Plain C++ (no HIP, no _Float16: binary16 is rounded in software), so that
// tests/two_stage_check.cpp can evaluate both MFMAs of a (ray, sphere) pair in exact arithmetic.  build_mfma_operands (rtw_scene.hip) is the
// only product user; the mirror is not in the library.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

namespace rtwh {

// ---- binary16 in software: values are carried as doubles that binary16 holds exactly ----
// x rounded to the nearest binary16 (ties to even, subnormals honoured); |x| < 65520, finite
inline double f16_rn(double x) {
    if (x == 0.0) return x;
    int e;
    (void)std::frexp(std::fabs(x), &e);                 // |x| = m 2^e, m in [0.5, 1): the ulp of its binade is 2^(e - 11)
    int q = e - 11;
    if (q < -24) q = -24;
    return std::ldexp(std::nearbyint(std::ldexp(x, -q)), q);      // (default rounding mode: to nearest, ties to even)
}
// the smallest binary16 >= x
inline double f16_up(double x) {
    double h = f16_rn(x);
    if (h < x) {
        int e;
        (void)std::frexp(std::fabs(h), &e);
        int q = (h == 0.0 ? -24 : e - 11);
        if (h < 0.0 && std::ldexp(1.0, e - 1) == -h) q -= 1;     // leaving a negative power of two towards zero: the finer binade's step
        if (q < -24) q = -24;
        h += std::ldexp(1.0, q);
    }
    return h;
}
inline unsigned f16_bits(double h) {                   // the encoding of a value binary16 holds exactly
    if (h == 0.0) return std::signbit(h) ? 0x8000u : 0u;
    const unsigned sign = h < 0.0 ? 0x8000u : 0u;
    int e;
    const double m = std::frexp(std::fabs(h), &e);     // m in [0.5, 1)
    if (e - 1 < -14) return sign | (unsigned)std::ldexp(std::fabs(h), 24);                 // subnormal: multiples of 2^-24
    return sign | ((unsigned)(e - 1 + 15) << 10) | ((unsigned)std::ldexp(m, 11) & 0x3ffu);
}
inline double f16_value(unsigned b) {
    const double sign = (b & 0x8000u) ? -1.0 : 1.0;
    const int ex = (int)((b >> 10) & 31u), fr = (int)(b & 0x3ffu);
    if (ex == 0) return sign * std::ldexp((double)fr, -24);
    return sign * std::ldexp((double)(fr + 1024), ex - 25);
}
// the two binary16 pieces of the binary32 value x: p1 = RN16(x), p2 = RN16(x - p1)  (split_f16 on the device; x - p1 is exact in binary32)
inline void f16_split(float x, double &p1, double &p2) {
    p1 = f16_rn((double)x);
    p2 = f16_rn((double)x - p1);
}

// ---- a scene's constants ----
// The coarse margin Mc = Ms(sphere) + Mr(ray) of the two-stage evaluation, derived in rtw_scan_mfma.hpp ("Two stages"):
//   Ms s^2 = 1.01 [(1.506 x 2^-10 + 3.1 x 2^-20) |c|^2 + 1.1 x 2^-20 r^2] s^2 + 2^-19       folded into k1 (rounded UP)
//   Mr s^2 = 1.01 (0.502 x 2^-10 + 1.003 x 2^-11 + 2.1 x 2^-20) |o|^2 s^2 + 2^-9            added to (q^2 - oo') s^2 before t1 is rounded
#define RTW_MF_MS_C2 (1.01 * (1.506 * 0x1p-10 + 3.1 * 0x1p-20))
#define RTW_MF_MS_R2 (1.01 * 1.1 * 0x1p-20)
#define RTW_MF_MS_FLOOR 0x1p-19
#define RTW_MF_MR_O2 (1.01 * (0.502 * 0x1p-10 + 1.003 * 0x1p-11 + 2.1 * 0x1p-20))
#define RTW_MF_MR_FLOOR 0x1p-9f
struct MfmaScales {
    double sc, sig2, phi_c, phi_k;
    float keep, coef, o_max, mr;      // mf_oo_keep, mf_o1_coef, mf_o_max, mf_mr as uploaded
};
// emax: the largest |c_k| (binary32) or radius of the scene.  false: outside what the scaled f16 pieces cover (the VALU scan is used)
inline bool mfma_scales(double emax, MfmaScales *S) {
    if (!(emax > 0) || !std::isfinite(emax)) return false;
    int ex = 0;
    (void)std::frexp(emax, &ex);                         // emax <= 2^ex
    if (ex > 40 || ex < -40) return false;
    // lengths x s: sphere coordinates and radii use 2^8 of the f16 range (their products, halved: 2^15), ray origins may use
    // 2^13 -- rays up to 32 x the scene's extent away still take the filter (2 |p_k| s <= 2 x 2.74 x 2^13 < 65504).
    // phi_c: a coordinate's second f16 piece is a subnormal below 2^-3 (absolute error 2^-25 scaled); phi_k: the same floor for
    // the 2^4-scaled pieces of k' and of the ray's constant and for the second pieces of the quadratic features.
    S->sc = std::ldexp(1.0, 8 - ex); S->sig2 = S->sc * S->sc;
    S->phi_c = std::ldexp(1.0, -25) / S->sc; S->phi_k = std::ldexp(1.0, -20) / S->sig2;
    const double A_S = std::ldexp(1.0, -17);
    float keep = (float)(1.0 - 1.02 * 2 * A_S);
    if ((double)keep > 1.0 - 1.02 * 2 * A_S) keep = std::nextafter(keep, 0.0f);
    S->keep = keep;
    float coef = (float)(1.02 * 9 * S->phi_c);
    if ((double)coef < 1.02 * 9 * S->phi_c) coef = std::nextafter(coef, INFINITY);
    S->coef = coef;
    S->o_max = (float)(std::ldexp(1.0, 13) / S->sc);
    float mr = (float)(RTW_MF_MR_O2 * S->sig2);
    if ((double)mr < RTW_MF_MR_O2 * S->sig2) mr = std::nextafter(mr, INFINITY);
    S->mr = mr;
    return true;
}

// ---- the sphere side: one row of a block's two A operands ----
// pieces of a row, as values: the quadratic features c_i c_j s^2 / 2 (xx yy zz xy xz yz), the linear ones c_k s, and the constant
// k' s^2 = 2^15 k1 + 2^4 k2 with the sphere's share Ms of the coarse margin folded in: k1 is the smallest binary16 with
// 2^15 k1 >= k' s^2 + Ms s^2, k2 the remainder (negative: it takes the margin back in the second MFMA) rounded UP -- a larger k' only
// widens the filter.  A row outside the filter (padding, or a sphere every lane tests by itself): k' s^2 = -2^30, all features 0.
struct MfmaSphereRow { double q1[6], q2[6], l1[3], l2[3], k1, k2, kx; };      // kx: k' s^2 itself (what 2^15 k1 + 2^4 k2 stands for)
inline void mfma_sphere_row(bool in_filter, double cx, double cy, double cz, double r2, const MfmaScales &S, MfmaSphereRow *R) {
    double fq[6] = {0, 0, 0, 0, 0, 0}, fl[3] = {0, 0, 0};
    double kx = -1073741824.0, fold = 0.0;               // padding sphere: k' s^2 = -2^30: W = -2^30 + (q^2 - oo') s^2 < 0, coarse value included
    if (in_filter) {
        const double c2 = cx * cx + cy * cy + cz * cz;
        const double A_S = std::ldexp(1.0, -17), A_r = std::ldexp(12.0, -22);
        const double Gs = 1.02 * ((2 * A_S + A_r) * c2 + A_r * r2 + 9 * S.phi_c * (std::fabs(cx) + std::fabs(cy) + std::fabs(cz)) + 1.5 * S.phi_k);
        kx = (r2 - c2 + Gs) * S.sig2;
        fold = (RTW_MF_MS_C2 * c2 + RTW_MF_MS_R2 * r2) * S.sig2 + RTW_MF_MS_FLOOR;
        const double hs = 0.5 * S.sig2;
        fq[0] = cx * cx * hs; fq[1] = cy * cy * hs; fq[2] = cz * cz * hs; fq[3] = cx * cy * hs; fq[4] = cx * cz * hs; fq[5] = cy * cz * hs;
        fl[0] = cx * S.sc; fl[1] = cy * S.sc; fl[2] = cz * S.sc;
    }
    for (int k = 0; k < 6; ++k) f16_split((float)fq[k], R->q1[k], R->q2[k]);
    for (int k = 0; k < 3; ++k) f16_split((float)fl[k], R->l1[k], R->l2[k]);
    R->kx = kx;
    R->k1 = f16_up((kx + fold) / 32768.0);
    R->k2 = f16_up((kx - 32768.0 * R->k1) / 16.0);
}
// the row's operand words: m1 / m2 = the A operand of MFMA 1 / MFMA 2, H = the lane group (slots 8 H .. 8 H + 7 of each); slot table in rtw_scan_mfma.hpp
inline void mfma_sphere_words(const MfmaSphereRow &R, int H, uint32_t m1[4], uint32_t m2[4]) {
    auto pk = [](double lo, double hi) { return (uint32_t)(f16_bits(lo) | (f16_bits(hi) << 16)); };
    if (H == 0) {
        m1[0] = pk(R.q1[0], R.q1[1]); m1[1] = pk(R.q1[2], R.q1[3]); m1[2] = pk(R.q1[4], R.q1[5]); m1[3] = pk(R.l1[1], R.l2[1]);      // xx yy | zz xy | xz yz | py py
        m2[0] = pk(R.q2[0], R.q1[0]); m2[1] = pk(R.q2[1], R.q1[1]); m2[2] = pk(R.q2[2], R.q1[2]); m2[3] = pk(R.q2[3], R.q1[3]);      // xx xx | yy yy | zz zz | xy xy
    } else {
        m1[0] = pk(R.l2[0], R.l1[0]); m1[1] = pk(R.l2[2], R.l1[2]); m1[2] = pk(R.l1[0], R.l1[2]); m1[3] = pk(R.k1, 32768.0);         // px px | pz pz | px pz | k T
        m2[0] = pk(R.q2[4], R.q1[4]); m2[1] = pk(R.q2[5], R.q1[5]); m2[2] = pk(R.l1[1], R.k2); m2[3] = pk(16.0, 16.0);               // xz xz | yz yz | py k | T T
    }
}

// ---- the ray side: a host mirror of the prologue of hit_world_mfma (same operations in the same order, binary32; binary16 roundings as
//      v_cvt_f16_f32 / v_fma_mixhi_f16 make them) -- g0 / g1: the eight words of lane groups 0 / 1, words 0-3 MFMA 1, words 4-7 MFMA 2 ----
struct MfmaRayWords { uint32_t g0[8], g1[8]; bool ok; float tx; };      // tx: (q^2 - oo') s^2 itself (what 2^15 t1 + 2^4 (t2 + t3) stands for)
inline void mfma_ray_words(const float o[3], const float d[3], bool has_ray, const MfmaScales &S, MfmaRayWords *Wd) {
    const float ox = o[0], oy = o[1], oz = o[2], dx = d[0], dy = d[1], dz = d[2];
    const float sc = (float)S.sc, sig2 = (float)S.sig2;
    const float s2 = std::fmaf(dz, dz, std::fmaf(dy, dy, dx * dx));
    const float oinf = std::fmax(std::fmax(std::fabs(ox), std::fabs(oy)), std::fabs(oz));
    const bool ok = has_ray && s2 <= 1.0009f && oinf <= S.o_max;
    const float q = std::fmaf(oz, dz, std::fmaf(oy, dy, ox * dx));
    const float oo = std::fmaf(oz, oz, std::fmaf(oy, oy, ox * ox));
    const float o1 = (std::fabs(ox) + std::fabs(oy)) + std::fabs(oz);
    const float oop = std::fmaf(oo, S.keep, -(S.coef * o1));
    const float tq = sig2 * std::fmaf(q, q, -oop);
    const float z = ok ? 1.0f : 0.0f, z2 = z + z, zs2 = z2 * sc;
    const float fp[3] = {std::fmaf(-q, dx, ox) * zs2, std::fmaf(-q, dy, oy) * zs2, std::fmaf(-q, dz, oz) * zs2};
    const float dx2 = dx * z2, dy2 = dy * z2, dz2 = dz * z2;
    const float fq[6] = {dx2 * dx, dy2 * dy, dz2 * dz, (dx2 + dx2) * dy, (dx2 + dx2) * dz, (dy2 + dy2) * dz};
    const float tx = ok ? tq : (has_ray ? 60000.0f * 32768.0f : -60000.0f * 32768.0f);
    const float um = std::fmaf(oo, S.mr, RTW_MF_MR_FLOOR);
    const float txm = tx + (ok ? um : 0.0f);
    double q1[6], q2[6], p1[3], p2[3], t2, t3;
    for (int k = 0; k < 6; ++k) f16_split(fq[k], q1[k], q2[k]);
    for (int k = 0; k < 3; ++k) f16_split(fp[k], p1[k], p2[k]);
    const double t1 = f16_rn((double)(txm * (1.0f / 32768.0f)));
    const float trem = std::fmaf(-32768.0f, (float)t1, tx);
    f16_split(trem * (1.0f / 16.0f), t2, t3);
    const double big = ok ? 32768.0 : 0.0, small = ok ? 16.0 : 0.0;
    auto pk = [](double lo, double hi) { return (uint32_t)(f16_bits(lo) | (f16_bits(hi) << 16)); };
    const uint32_t a0[8] = {pk(q1[0], q1[1]), pk(q1[2], q1[3]), pk(q1[4], q1[5]), pk(p1[1], p1[1]),
                            pk(q1[0], q2[0]), pk(q1[1], q2[1]), pk(q1[2], q2[2]), pk(q1[3], q2[3])};
    const uint32_t a1[8] = {pk(p1[0], p2[0]), pk(p1[2], p2[2]), pk(p1[0], p1[2]), pk(big, t1),
                            pk(q1[4], q2[4]), pk(q1[5], q2[5]), pk(p2[1], small), pk(t2, t3)};
    std::memcpy(Wd->g0, a0, sizeof a0); std::memcpy(Wd->g1, a1, sizeof a1);
    Wd->ok = ok; Wd->tx = tx;
}

}  // namespace rtwh
