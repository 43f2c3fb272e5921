// two_stage_check.cpp -- CPU check of the two-stage evaluation of the matrix-pipe filter (raytracingweekend.jl_amd/csrc/rtw_scan_mfma.hpp,
// "Two stages"): the host's sphere operands and a host mirror of the scan prologue's ray operands (csrc/rtw_mfma_operands.hpp, plain C++)
// are multiplied slot by slot in EXACT arithmetic -- every binary16 piece is an integer multiple of 2^-24, so a product is an integer
// multiple of 2^-48 and the 16-term sums of both MFMAs fit a 128-bit integer -- for random and adversarial (ray, sphere) pairs:
//   (a) P1' + P2' equals the 32-product sum of the un-folded pieces (k1 = RN16, t1 = RN16 of the constants themselves) up to the fold's
//       documented rounding: the k pieces stand for k' s^2 from above by at most 2^-10 of the remainder + 2^-20, the t pieces for
//       (q^2 - oo') s^2 within 2^-21.5 of the remainder + 2^-21;
//   (b) P1' - (P1' + P2') >= E1 = 2^-20 x sum |terms of MFMA 1| (the bound the budget reserves for MFMA 1's accumulation error) for every
//       ray that uses the filter and every sphere in it: the coarse value never rejects what the fine value accepts, with the hardware's
//       error to spare; and where the exact discriminant of the pair is >= 0, P1' - E1 > 0 and W - E1 - E2 > 0;
//   (c) every piece is a finite binary16 inside the documented ranges (|k2| < 2^11, |t2| < 2^15; no piece is +-inf or NaN);
//   and the special rows and rays keep their meaning in the coarse value: a ray that is not ok has P1' = W = +2^15 x 60000 for every row,
//   a lane without a ray -2^15 x 60000, a padding row P1' < 0 and W < 0 for every ray that uses the filter.
//   two_stage_check                the self-check: prints one summary line; exit code 1 on the first violation
//   two_stage_check --pairs FILE   the exact coarse and fine values of given (ray, sphere) pairs (tests/test_gpu_two_stage.py builds its cases on them)
// Compiled and run by tests/test_two_stage_layout.py (no GPU, no HIP);
// host-only, so it may also be built with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "../raytracingweekend.jl_amd/csrc/rtw_mfma_operands.hpp"

typedef __int128 i128;
static const double U48 = 281474976710656.0;      // 2^48

static i128 piece(unsigned half) { return (i128)std::llround(std::ldexp(rtwh::f16_value(half), 24)); }      // in units of 2^-24, exact
static double to_double(i128 v) { return (double)v / U48; }

struct Sphere { double c[3], r; };
struct Ray { float o[3], d[3]; bool has_ray; };
struct Stats { long long pairs = 0, ok_pairs = 0, coarse_neg = 0, exact_neg = 0, tangent = 0; double min_slack = 1e300; };

static bool bad_half(unsigned h) { return ((h >> 10) & 31u) == 31u; }

// one (ray, sphere row) pair.  in_filter = false: a padding row.
static int check_pair(const char *what, const rtwh::MfmaScales &S, const Ray &ray, const rtwh::MfmaRayWords &rw, bool in_filter, const Sphere &sp, Stats *st) {
    using namespace rtwh;
    MfmaSphereRow row;
    const double cx = (double)(float)sp.c[0], cy = (double)(float)sp.c[1], cz = (double)(float)sp.c[2], r2 = sp.r * sp.r;
    mfma_sphere_row(in_filter, cx, cy, cz, r2, S, &row);
    uint32_t a[2][8];      // [lane group][word]: words 0-3 MFMA 1, 4-7 MFMA 2
    mfma_sphere_words(row, 0, a[0], a[0] + 4);
    mfma_sphere_words(row, 1, a[1], a[1] + 4);
    i128 P[2] = {0, 0}, absP[2] = {0, 0};
    for (int H = 0; H < 2; ++H)
        for (int wd = 0; wd < 8; ++wd) {
            const uint32_t bw = H ? rw.g1[wd] : rw.g0[wd];
            for (int half = 0; half < 2; ++half) {
                const unsigned ah = (a[H][wd] >> (16 * half)) & 0xffffu, bh = (bw >> (16 * half)) & 0xffffu;
                if (bad_half(ah) || bad_half(bh)) { printf("%s: a piece is not finite (group %d word %d half %d: %04x x %04x)\n", what, H, wd, half, ah, bh); return 1; }
                const i128 t = piece(ah) * piece(bh);
                P[wd >> 2] += t; absP[wd >> 2] += t < 0 ? -t : t;
            }
        }
    const double P1 = to_double(P[0]), W = to_double(P[0] + P[1]), P2 = to_double(P[1]);
    const double E1 = std::ldexp(to_double(absP[0]), -20), E2 = std::ldexp(to_double(absP[1]) + std::fabs(P1) + E1, -20);
    ++st->pairs;
    const double big = 60000.0 * 32768.0;
    if (!rw.ok) {
        const double want = ray.has_ray ? big : -big;
        if (P1 != want || W != want) { printf("%s: a ray off the filter gives P1' = %.17g, W = %.17g, expected %.17g\n", what, P1, W, want); return 1; }
        return 0;
    }
    if (!in_filter) {
        if (!(P1 + E1 < 0) || !(W + E1 + E2 < 0)) { printf("%s: a padding row gives P1' = %.17g, W = %.17g\n", what, P1, W); return 1; }
        return 0;
    }
    ++st->ok_pairs;
    // (c) ranges
    if (!(std::fabs(row.k2) < 2048.0)) { printf("%s: k2 = %g\n", what, row.k2); return 1; }
    const double t1 = f16_value(rw.g1[3] >> 16), t2 = f16_value(rw.g1[7] & 0xffffu), t3 = f16_value(rw.g1[7] >> 16);
    if (!(std::fabs(t2) < 32768.0)) { printf("%s: t2 = %g\n", what, t2); return 1; }
    // (a) the folded constants against what they stand for, and against the un-folded pieces
    const double kx = row.kx, tx = (double)rw.tx;
    const double Kf = 32768.0 * row.k1 + 16.0 * row.k2, Tf = 32768.0 * t1 + 16.0 * (t2 + t3);
    const double krem = 32768.0 * row.k1 - kx, trem = std::fabs(32768.0 * t1 - tx);
    const double tol = 1e-9 * (std::fabs(kx) * 0x1p-40 + 1e-30);          // (the builder's own binary64 arithmetic)
    if (!(Kf - kx >= -tol) || !(Kf - kx <= std::ldexp(krem, -10) + 0x1p-20 + tol)) { printf("%s: 2^15 k1 + 2^4 k2 - k' s^2 = %.17g, remainder %.17g\n", what, Kf - kx, krem); return 1; }
    if (!(std::fabs(Tf - tx) <= trem * 0x1.6ap-22 + 0x1p-21)) { printf("%s: 2^15 t1 + 2^4 (t2 + t3) - tx = %.17g, remainder %.17g\n", what, Tf - tx, trem); return 1; }
    {
        // the un-folded pieces: k1 = RN16(k' s^2 / 2^15), k2 the remainder rounded up; t1 = RN16(tx / 2^15), (t2, t3) the split remainder
        const double k1o = f16_rn(kx / 32768.0), k2o = f16_up((kx - 32768.0 * k1o) / 16.0);
        const double t1o = f16_rn((double)(rw.tx * (1.0f / 32768.0f)));
        double t2o, t3o;
        f16_split(std::fmaf(-32768.0f, (float)t1o, rw.tx) * (1.0f / 16.0f), t2o, t3o);
        const double Ko = 32768.0 * k1o + 16.0 * k2o, To = 32768.0 * t1o + 16.0 * (t2o + t3o);
        const double W0 = W - (Kf - Ko) - (Tf - To);                      // the same 27 feature products + the un-folded constants
        const double fold_tol = std::ldexp(krem, -10) + std::ldexp(std::fabs(32768.0 * k1o - kx), -10) + 0x1p-19 + (trem + std::fabs(32768.0 * t1o - tx)) * 0x1.6ap-22 + 0x1p-20;
        if (!(std::fabs(W - W0) <= fold_tol)) { printf("%s: folded W = %.17g, un-folded %.17g, tolerance %.17g\n", what, W, W0, fold_tol); return 1; }
    }
    // (b) the coarse value dominates the fine one by MFMA 1's error bound
    if (!(-P2 >= E1)) { printf("%s: P1' - W = %.17g < E1 = %.17g (P1' %.17g, W %.17g; o %g %g %g, c %g %g %g r %g, s %g)\n", what, -P2, E1, P1, W, ray.o[0], ray.o[1], ray.o[2], cx, cy, cz, sp.r, S.sc); return 1; }
    if (-P2 - E1 < st->min_slack) st->min_slack = -P2 - E1;
    // the property itself, where the exact discriminant of the pair says so (binary32 inputs, long double: 64 bits -- decisive away from |D| ~ 2^-60 S)
    {
        const long double ex = (long double)ray.o[0] - cx, ey = (long double)ray.o[1] - cy, ez = (long double)ray.o[2] - cz;
        const long double hb = ex * ray.d[0] + ey * ray.d[1] + ez * ray.d[2];
        const long double D = hb * hb - (ex * ex + ey * ey + ez * ez) + (long double)r2;
        if (D >= 0) {
            if (!(P1 - E1 > 0) || !(W - E1 - E2 > 0)) { printf("%s: D = %Lg >= 0 but P1' = %.17g (E1 %.17g), W = %.17g\n", what, D, P1, E1, W); return 1; }
        } else {
            ++st->exact_neg;
            if (P1 + E1 < 0) ++st->coarse_neg;
        }
    }
    return 0;
}

// --pairs FILE: FILE holds n and n spheres "cx cy cz r", then m and m rays "ox oy oz dx dy dz has_ray" (decimal or hexadecimal floating point).
// Prints, per ray, a line "ray <ok>" and per sphere of the scene a line "P1' E1 W E2" (hexadecimal floating point): the exact coarse and
// fine values of the pair in scaled units and the error bounds of the two MFMAs -- P1' - E1 > 0: the coarse test leaves the pair open on
// any hardware within the budget, P1' + E1 < 0: it settles it; W likewise with E1 + E2.  Every sphere has a row (none is treated as huge).
static int pairs_mode(const char *path) {
    FILE *f = fopen(path, "r");
    int n = 0, m = 0;
    if (!f || fscanf(f, "%d", &n) != 1 || n <= 0) { printf("cannot read %s\n", path); return 2; }
    std::vector<Sphere> sph((size_t)n);
    double emax = 0;
    for (Sphere &s : sph) {
        if (fscanf(f, "%la %la %la %la", &s.c[0], &s.c[1], &s.c[2], &s.r) != 4) { printf("short file\n"); return 2; }
        for (int k = 0; k < 3; ++k) emax = std::fmax(emax, std::fabs((double)(float)s.c[k]));
        emax = std::fmax(emax, std::fabs(s.r));
    }
    rtwh::MfmaScales S;
    if (!rtwh::mfma_scales(emax, &S)) { printf("no scales\n"); return 2; }
    if (fscanf(f, "%d", &m) != 1 || m < 0) { printf("short file\n"); return 2; }
    for (int i = 0; i < m; ++i) {
        double v[6]; int has = 0;
        if (fscanf(f, "%la %la %la %la %la %la %d", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &has) != 7) { printf("short file\n"); return 2; }
        Ray r; r.has_ray = has != 0;
        for (int k = 0; k < 3; ++k) { r.o[k] = (float)v[k]; r.d[k] = (float)v[3 + k]; }
        rtwh::MfmaRayWords rw;
        rtwh::mfma_ray_words(r.o, r.d, r.has_ray, S, &rw);
        printf("ray %d\n", rw.ok ? 1 : 0);
        for (const Sphere &s : sph) {
            rtwh::MfmaSphereRow row;
            rtwh::mfma_sphere_row(true, (double)(float)s.c[0], (double)(float)s.c[1], (double)(float)s.c[2], s.r * s.r, S, &row);
            uint32_t a[2][8];
            rtwh::mfma_sphere_words(row, 0, a[0], a[0] + 4);
            rtwh::mfma_sphere_words(row, 1, a[1], a[1] + 4);
            i128 P[2] = {0, 0}, absP[2] = {0, 0};
            for (int H = 0; H < 2; ++H)
                for (int wd = 0; wd < 8; ++wd)
                    for (int half = 0; half < 2; ++half) {
                        const i128 t = piece((a[H][wd] >> (16 * half)) & 0xffffu) * piece(((H ? rw.g1[wd] : rw.g0[wd]) >> (16 * half)) & 0xffffu);
                        P[wd >> 2] += t; absP[wd >> 2] += t < 0 ? -t : t;
                    }
            const double P1 = to_double(P[0]), E1 = std::ldexp(to_double(absP[0]), -20);
            printf("%a %a %a %a\n", P1, E1, to_double(P[0] + P[1]), std::ldexp(to_double(absP[1]) + std::fabs(P1) + E1, -20));
        }
    }
    fclose(f);
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 2 && strcmp(argv[1], "--pairs") == 0) return pairs_mode(argv[2]);
    std::mt19937_64 gen(77);
    auto uni = [&](double a, double b) { return a + (b - a) * (double)(gen() >> 11) * (1.0 / 9007199254740992.0); };
    auto unit = [&](float d[3], double len) {
        double v[3], n;
        do { v[0] = uni(-1, 1); v[1] = uni(-1, 1); v[2] = uni(-1, 1); n = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); } while (n < 0.1 || n > 1);
        for (int k = 0; k < 3; ++k) d[k] = (float)(v[k] / n * len);
    };
    Stats st;
    // the software binary16 against a few known encodings
    {
        using namespace rtwh;
        const double v[] = {1.0, -2.5, 65504.0, 0x1p-14, 0x1p-24, 1023.0 * 0x1p-24, 0.0, 60000.0, -32768.0, 16.0};
        const unsigned b[] = {0x3c00u, 0xc100u, 0x7bffu, 0x0400u, 0x0001u, 0x03ffu, 0u, 0x7b53u, 0xf800u, 0x4c00u};
        for (int i = 0; i < 10; ++i) if (f16_bits(v[i]) != b[i] || f16_value(b[i]) != v[i]) { printf("f16_bits(%g) = %04x, expected %04x\n", v[i], f16_bits(v[i]), b[i]); return 1; }
        if (f16_rn(1.0 + 0x1p-11) != 1.0 || f16_rn(1.0 + 3 * 0x1p-11) != 1.0 + 0x1p-9 || f16_up(1.0 + 0x1p-30) != 1.0 + 0x1p-10 || f16_up(-1.0 - 0x1p-30) != -1.0 ||
            f16_up(-1.0 + 0x1p-30) != -1.0 + 0x1p-11 || f16_up(0x1p-30) != 0x1p-24 || f16_rn(0x1p-25) != 0.0 || f16_up(-0x1p-30) != 0.0) { printf("f16 rounding\n"); return 1; }
    }
    // scenes of every scale: the largest coordinate fixes s; spheres from the centre out to the scene-scale limit |c_k| s = 2^8, radii 1e-3 .. 1e3
    const int exps[] = {-5, 0, 4, 10, 20};
    for (int ex : exps) {
        const double ext = std::ldexp(1.0, ex);
        rtwh::MfmaScales S;
        if (!rtwh::mfma_scales(ext * 0.99999, &S)) { printf("no scales for 2^%d\n", ex); return 1; }
        std::vector<Sphere> sph;
        for (int i = 0; i < 96; ++i) {
            Sphere s;
            const double reach = i % 4 == 0 ? 0.99999 : (i % 4 == 1 ? 0.05 : 0.6);
            for (int k = 0; k < 3; ++k) s.c[k] = (i % 4 == 0 ? (uni(0, 1) < 0.5 ? -1.0 : 1.0) * reach * ext : uni(-reach, reach) * ext);
            if (i % 7 == 3) s.c[1] = 0.0;                                  // a flat coordinate: zero pieces
            if (i % 11 == 5) s.c[2] = uni(-1, 1) * 0x1p-22 * ext;          // a coordinate whose pieces are binary16 subnormals
            s.r = std::fmin(ext * 0.99999, std::pow(10.0, uni(-3, 3)) * std::fmin(1.0, ext));
            if (i % 13 == 6) s.r = std::sqrt(s.c[0] * s.c[0] + s.c[1] * s.c[1] + s.c[2] * s.c[2]);       // k' ~ 0: the leading piece of k nearly cancels
            if (s.r > ext * 0.99999) s.r = ext * 0.99999;
            sph.push_back(s);
        }
        std::vector<Ray> rays;
        const double omax = (double)S.o_max;
        for (int i = 0; i < 160; ++i) {
            Ray r; r.has_ray = true;
            const double reach = (i % 5 == 0 ? 1.0 : i % 5 == 1 ? 0.9 : i % 5 == 2 ? 1e-3 : i % 5 == 3 ? 1.0 / 32 : 0.3) * omax;
            for (int k = 0; k < 3; ++k) r.o[k] = (float)(i % 5 == 0 ? (uni(0, 1) < 0.5 ? -reach : reach) : uni(-reach, reach));
            unit(r.d, i % 9 == 4 ? 1.0004 : 1.0);                          // |d|^2 up to 1.0008: still on the filter
            if (i % 17 == 8) { r.d[0] = 0.0f; r.d[1] = 0.0f; r.d[2] = 1.0f; }
            if (i % 19 == 9) { r.o[0] = r.o[1] = r.o[2] = 0.0f; }
            rays.push_back(r);
        }
        // tangent rays (D = 0 up to the rounding of the inputs, and a little to either side), as tests/exact_filters.py's callers build them:
        // through the point c + r n, n perpendicular to d, from near the origin and from 0.9 x the filter's |o| limit
        for (int i = 0; i < 96; ++i) {
            const Sphere &s = sph[(size_t)i];
            Ray r; r.has_ray = true;
            unit(r.d, 1.0);
            float nf[3]; unit(nf, 1.0);
            double n[3] = {nf[0], nf[1], nf[2]}, dn = n[0] * r.d[0] + n[1] * r.d[1] + n[2] * r.d[2], nn = 0;
            for (int k = 0; k < 3; ++k) { n[k] -= dn * r.d[k]; nn += n[k] * n[k]; }
            if (nn < 1e-3) continue;
            const double rr = s.r * (1.0 + (i % 3 - 1) * 1e-6);
            const double back = (i % 2 ? 0.9 * omax : 0.01 * ext);
            bool inside = true;
            for (int k = 0; k < 3; ++k) { r.o[k] = (float)(s.c[k] + rr * n[k] / std::sqrt(nn) - back * r.d[k]); inside = inside && std::fabs(r.o[k]) <= omax; }
            if (!inside) continue;
            rays.push_back(r); ++st.tangent;
        }
        // rays off the filter (not unit, too far out) and a lane without a ray.  (Rays that are not FINITE are not modelled here: their features are
        // NaN, so both stages give NaN for every row -- the same operands, hence the same value, before and after the second MFMA.)
        { Ray r; r.has_ray = true; r.o[0] = 1; r.o[1] = 2; r.o[2] = 3; r.d[0] = 0; r.d[1] = 0; r.d[2] = 1.01f; rays.push_back(r); }
        { Ray r; r.has_ray = true; r.o[0] = (float)(1.5 * omax); r.o[1] = 0; r.o[2] = 0; unit(r.d, 1.0); rays.push_back(r); }
        { Ray r; r.has_ray = false; r.o[0] = 1; r.o[1] = 2; r.o[2] = 3; unit(r.d, 1.0); rays.push_back(r); }
        for (const Ray &r : rays) {
            rtwh::MfmaRayWords rw;
            rtwh::mfma_ray_words(r.o, r.d, r.has_ray, S, &rw);
            char what[64];
            snprintf(what, sizeof what, "scale 2^%d", ex);
            for (const Sphere &s : sph) if (check_pair(what, S, r, rw, true, s, &st)) return 1;
            if (check_pair(what, S, r, rw, false, sph[0], &st)) return 1;
        }
    }
    // (the share of the pairs with a negative exact discriminant that the coarse value settles by itself is reported, not asserted)
    printf("two stage: %lld pairs (%lld on the filter, %lld tangent rays): P1' - W >= E1 everywhere (least slack %.3g), sums and special rows as documented; "
           "coarse value negative for %.1f %% of the pairs with D < 0\n", st.pairs, st.ok_pairs, st.tangent, st.min_slack, 100.0 * (double)st.coarse_neg / (double)(st.exact_neg ? st.exact_neg : 1));
    return 0;
}
