// plain_layout_check.cpp -- CPU check of the plain matrix-pipe scan's block layout (raytracingweekend.jl_amd/csrc/rtw_plain_layout.hpp, plain
// C++): random and degenerate sets of centres -- all equal, all on one line, lattices with exact ties, the sizes around the block edges --
// must come out as a permutation into exactly ceil(n / 32) blocks whose fill differs by at most one, the caller's order when there is at
// most one block, and the same permutation when asked twice.  Prints one summary line; exit code 1 on the first violation.
//   plain_layout_check                 the self-check
//   plain_layout_check --blocks FILE   FILE holds n and then n centres "x y z": prints the block of every sphere, in input order
// Compiled and run by tests/test_plain_layout.py (no GPU, no HIP); host-only, so it may also be built with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include "../raytracingweekend.jl_amd/csrc/rtw_plain_layout.hpp"

static int check(const char *what, const std::vector<double> &x, const std::vector<double> &y, const std::vector<double> &z, long long *cases) {
    const int n = (int)x.size();
    rtwh::PlainLayout L, L2;
    rtwh::build_plain_layout(x.data(), y.data(), z.data(), n, &L);
    rtwh::build_plain_layout(x.data(), y.data(), z.data(), n, &L2);
    ++*cases;
    const int want = (n + 31) / 32;
    if (L.blocks != want) { printf("%s n=%d: %d blocks, expected %d\n", what, n, L.blocks, want); return 1; }
    if ((int)L.slot.size() != 32 * want) { printf("%s n=%d: %zu slots\n", what, n, L.slot.size()); return 1; }
    if (L.slot != L2.slot || L.blocks != L2.blocks) { printf("%s n=%d: the second call gave another permutation\n", what, n); return 1; }
    std::vector<int> seen(n, 0);
    int lo = 1 << 30, hi = 0;
    for (int b = 0; b < want; ++b) {
        int fill = 0;
        bool gap = false;
        for (int k = 0; k < 32; ++k) {
            const int i = L.slot[(size_t)b * 32 + k];
            if (i < 0) { gap = true; continue; }
            if (i >= n) { printf("%s n=%d: slot holds %d\n", what, n, i); return 1; }
            if (gap) { printf("%s n=%d: block %d has a hole in front of row %d\n", what, n, b, k); return 1; }
            ++seen[i]; ++fill;
        }
        lo = fill < lo ? fill : lo; hi = fill > hi ? fill : hi;
    }
    for (int i = 0; i < n; ++i) if (seen[i] != 1) { printf("%s n=%d: sphere %d appears %d times\n", what, n, i, seen[i]); return 1; }
    if (want > 0 && hi - lo > 1) { printf("%s n=%d: leaves of %d and %d spheres\n", what, n, lo, hi); return 1; }
    if (want <= 1) for (int i = 0; i < n; ++i) if (L.slot[i] != i) { printf("%s n=%d: one block, but row %d holds %d\n", what, n, i, L.slot[i]); return 1; }
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 2 && strcmp(argv[1], "--blocks") == 0) {
        FILE *f = fopen(argv[2], "r");
        int n = 0;
        if (!f || fscanf(f, "%d", &n) != 1 || n < 0) { printf("cannot read %s\n", argv[2]); return 2; }
        std::vector<double> x(n), y(n), z(n);
        for (int i = 0; i < n; ++i) if (fscanf(f, "%lf %lf %lf", &x[i], &y[i], &z[i]) != 3) { printf("short file\n"); return 2; }
        fclose(f);
        rtwh::PlainLayout L;
        rtwh::build_plain_layout(x.data(), y.data(), z.data(), n, &L);
        std::vector<int> blk(n, -1);
        for (size_t k = 0; k < L.slot.size(); ++k) if (L.slot[k] >= 0) blk[L.slot[k]] = (int)(k / 32);
        printf("blocks %d\n", L.blocks);
        for (int i = 0; i < n; ++i) printf("%d\n", blk[i]);
        return 0;
    }
    std::mt19937_64 gen(2024);
    auto uni = [&](double a, double b) { return a + (b - a) * (double)(gen() >> 11) * (1.0 / 9007199254740992.0); };
    const int sizes[] = {0, 1, 31, 32, 33, 64, 65, 96, 97, 484, 1000, 2047};
    long long cases = 0;
    for (int n : sizes) {
        std::vector<double> x(n), y(n), z(n);
        // all centres equal
        for (int i = 0; i < n; ++i) { x[i] = 1.5; y[i] = -2.0; z[i] = 0.25; }
        if (check("equal", x, y, z, &cases)) return 1;
        // all on one line (each axis in turn, and a diagonal), with repeated points
        for (int ax = 0; ax < 4; ++ax) {
            for (int i = 0; i < n; ++i) {
                const double t = (double)((i * 7) % 13);
                x[i] = ax == 0 || ax == 3 ? t : 0.0; y[i] = ax == 1 || ax == 3 ? t : 0.0; z[i] = ax == 2 || ax == 3 ? -t : 0.0;
            }
            if (check("line", x, y, z, &cases)) return 1;
        }
        // a lattice: exact ties on every axis, equally wide axes
        for (int i = 0; i < n; ++i) { x[i] = (double)(i % 5); y[i] = (double)((i / 5) % 5); z[i] = (double)((i / 25) % 5); }
        if (check("lattice", x, y, z, &cases)) return 1;
        // random: a flat layer like the reference's scene, a cube, clusters far from the origin
        for (int rep = 0; rep < 20; ++rep) {
            const double far = rep % 3 == 0 ? 1e6 : 0.0, flat = rep % 2 ? 0.0 : 1.0;
            for (int i = 0; i < n; ++i) { x[i] = far + uni(-11, 11); y[i] = 0.2 + flat * uni(-11, 11); z[i] = uni(-11, 11) - far; }
            if (rep % 5 == 4) for (int i = 0; i + 1 < n; i += 2) { x[i + 1] = x[i]; y[i + 1] = y[i]; z[i + 1] = z[i]; }      // pairs of identical centres
            if (check("random", x, y, z, &cases)) return 1;
        }
    }
    // the headline scene's shape: 484 spheres on a jittered 22 x 22 lattice -> 16 leaves of 30 or 31, each a compact patch
    {
        const int n = 484;
        std::vector<double> x(n), y(n, 0.2), z(n);
        for (int i = 0; i < n; ++i) { x[i] = (double)(i / 22 - 11) + uni(0, 0.9); z[i] = (double)(i % 22 - 11) + uni(0, 0.9); }
        if (check("headline", x, y, z, &cases)) return 1;
        rtwh::PlainLayout L;
        rtwh::build_plain_layout(x.data(), y.data(), z.data(), n, &L);
        double worst = 0;
        for (int b = 0; b < L.blocks; ++b) {
            double mn[2] = {1e300, 1e300}, mx[2] = {-1e300, -1e300};
            for (int k = 0; k < 32; ++k) {
                const int i = L.slot[(size_t)b * 32 + k];
                if (i < 0) continue;
                mn[0] = std::fmin(mn[0], x[i]); mx[0] = std::fmax(mx[0], x[i]); mn[1] = std::fmin(mn[1], z[i]); mx[1] = std::fmax(mx[1], z[i]);
            }
            worst = std::fmax(worst, std::fmax(mx[0] - mn[0], mx[1] - mn[1]));
        }
        // (a strip of 32 consecutive spheres of the list is 22 units long; a patch of 30 of a 22 x 22 lattice is about 5 x 6)
        if (!(worst < 9.0)) { printf("headline: a leaf is %.2f units long\n", worst); return 1; }
    }
    printf("plain layout: %lld sets checked, every sphere once, ceil(n / 32) evenly filled blocks, deterministic\n", cases);
    return 0;
}
