// The byte arithmetic of the host paths (csrc/rtw_layout.hpp, plain C++) on the CPU: the regions of a context's device buffer and the alias
// check.  Built with the host compiler and its address / undefined-behaviour sanitizers and run by tests/test_host_layout.py.  No GPU, no HIP.
#include "../raytracingweekend.jl_amd/csrc/rtw_layout.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace rtwh;

static int failures = 0;
#define CHECK(cond, ...)                                                       \
    do {                                                                       \
        if (!(cond)) { ++failures; printf("FAILED %s:%d %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

struct Region { size_t off, bytes; };

// every region on a 16-byte boundary, behind the one before it; `total` reaches the end of the last
static void check_regions(const char *what, const std::vector<Region> &r, size_t total) {
    for (size_t k = 0; k < r.size(); ++k) {
        CHECK(r[k].off % 16 == 0, "%s: region %zu starts at %zu", what, k, r[k].off);
        if (k) CHECK(r[k].off >= r[k - 1].off + r[k - 1].bytes, "%s: region %zu at %zu starts inside region %zu (%zu + %zu)", what, k, r[k].off, k - 1, r[k - 1].off, r[k - 1].bytes);
        if (k) CHECK(r[k].off < r[k - 1].off + r[k - 1].bytes + 16, "%s: a gap of 16 bytes or more before region %zu", what, k);
    }
    CHECK(total >= r.back().off + r.back().bytes, "%s: total %zu ends before the last region (%zu + %zu)", what, total, r.back().off, r.back().bytes);
}

static void check_layouts() {
    DevLayout L;
    CHECK(L.add(5) == 0 && L.total == 5 && L.add(0) == 16 && L.total == 16 && L.add(16) == 16 && L.add(1) == 32 && L.total == 33, "DevLayout");
    DevLayout M{33};
    CHECK(M.add(7) == 48 && M.total == 55, "DevLayout behind 33 bytes");
    const int frames_wh[4][2] = {{1, 1}, {5, 3}, {17, 33}, {96, 54}};
    for (const auto &wh : frames_wh)
        for (size_t elem : {(size_t)4, (size_t)8})
            for (int n_views : {0, 1, 3}) {
                const int w = wh[0], h = wh[1];
                const size_t n = (size_t)w * h, frames = n_views ? n_views : 1;
                // sizes that are no multiple of 16: what the library reports is, but the layouts may not rely on it
                const size_t work_b = n * 4 * elem + 4, state_b = n * 8 * elem + elem, moment_b = n * 4 * elem + 4;
                char what[128];
                snprintf(what, sizeof what, "%dx%d elem %zu n_views %d", w, h, elem, n_views);

                const DenoiseLayout D(elem, w, h, n_views, work_b);
                CHECK(D.img_b == n * frames * 3 * elem && D.feat_b == n * frames * 8 * elem, "%s", what);
                check_regions(what, {{0, D.img_b}, {D.off_feat, D.feat_b}, {D.off_out, D.img_b}, {D.off_work, work_b * frames}}, D.total);

                const int lw = (w + 1) / 2, lh = (h + 1) / 2;
                const UpsampleLayout U(elem, lw, lh, w, h, n_views, work_b);
                CHECK(U.img_b == (size_t)lw * lh * frames * 3 * elem && U.out_b == n * frames * 3 * elem, "%s", what);
                check_regions(what, {{0, U.img_b}, {U.off_flo, U.flo_b}, {U.off_fhi, U.fhi_b}, {U.off_out, U.out_b}, {U.off_work, work_b * frames}}, U.total);

                for (bool filter : {false, true})
                    for (size_t paths : {(size_t)1, frames}) {
                        const TemporalLayout T(elem, w, h, frames, filter, paths, state_b, work_b);
                        CHECK(T.st_b == state_b * paths && T.img_b == T.frame_b * frames, "%s", what);
                        check_regions(what, {{0, T.img_b}, {T.off_feat, T.feat_b}, {T.off_acc, T.img_b}, {T.off_flt, filter ? T.img_b : 0}, {T.off_st[0], T.st_b}, {T.off_st[1], T.st_b},
                                             {T.off_work, filter ? work_b * frames : 0}}, T.total);
                        for (bool moments : {false, true}) {
                            const MomentLayout R(elem, w, h, frames, filter, paths, moments, state_b, work_b, moment_b);
                            CHECK(R.total == T.total && R.off_st[1] == T.off_st[1] && R.off_work == T.off_work, "%s: the moments moved the temporal regions", what);
                            check_regions(what, {{R.off_work, filter ? work_b * frames : 0}, {R.off_mo[0], R.mo_b}, {R.off_mo[1], R.mo_b}, {R.off_noise, R.noise_b * frames}}, R.total_m);
                            CHECK(R.total_m % 16 == 0 && R.mo_b == moment_b * paths && R.tab_b == frames * 32 * elem, "%s", what);
                            CHECK(R.off_tab % 16 == 0 && R.off_tab >= (moments ? R.total_m : R.total) && R.total_p >= R.off_tab + R.tab_b, "%s: the table", what);
                        }
                    }
            }
}

// what ranges_overlap has to say, byte by byte
static bool share_a_byte(const char *a, size_t na, const char *b, size_t nb) {
    for (size_t i = 0; i < na; ++i)
        for (size_t j = 0; j < nb; ++j)
            if (a + i == b + j) return true;
    return false;
}

static void check_alias_pairs() {
    static char buf[64];
    struct { size_t off, bytes; } r[] = {{0, 8}, {16, 8}, {8, 8}, {8, 1}, {7, 1}, {0, 9}, {0, 32}, {8, 4}, {31, 1}, {32, 8}, {24, 16}};
    const int n = sizeof r / sizeof r[0];
    int hits = 0;
    for (int a = 0; a < n; ++a)
        for (int b = 0; b < n; ++b) {
            const bool want = share_a_byte(buf + r[a].off, r[a].bytes, buf + r[b].off, r[b].bytes);
            hits += want;
            CHECK(ranges_overlap(buf + r[a].off, r[a].bytes, buf + r[b].off, r[b].bytes) == want, "[%zu, +%zu) against [%zu, +%zu)", r[a].off, r[a].bytes, r[b].off, r[b].bytes);
            const ByteRange out = {"out", buf + r[a].off, r[a].bytes}, in = {"in", buf + r[b].off, r[b].bytes};
            const AliasPair hit = first_alias(&out, 1, &in, 1);
            CHECK(want ? (hit.out == 0 && hit.other == 0 && hit.input) : hit.out < 0, "first_alias of [%zu, +%zu) against [%zu, +%zu)", r[a].off, r[a].bytes, r[b].off, r[b].bytes);
            const ByteRange two[2] = {out, in};                                  // ... and as two outputs
            const AliasPair hit2 = first_alias(two, 2, nullptr, 0);
            CHECK(want ? (hit2.out == 0 && hit2.other == 1 && !hit2.input) : hit2.out < 0, "first_alias of two outputs");
        }
    CHECK(hits > n && hits < n * n, "the hand-made ranges hold both kinds of pair");
    // the named cases: disjoint, touching at one end, one byte shared, nested (either way round)
    CHECK(!ranges_overlap(buf, 8, buf + 16, 8) && !ranges_overlap(buf, 8, buf + 8, 8) && !ranges_overlap(buf + 8, 8, buf, 8), "disjoint / touching");
    CHECK(ranges_overlap(buf, 9, buf + 8, 8) && ranges_overlap(buf + 8, 8, buf, 9), "one byte shared");
    CHECK(ranges_overlap(buf, 32, buf + 8, 4) && ranges_overlap(buf + 8, 4, buf, 32), "nested");
    // an absent (null) range is skipped, whatever its size
    const ByteRange outs[3] = {{"a", nullptr, ~(size_t)0 >> 1}, {"b", buf, 8}, {"c", nullptr, 64}};
    const ByteRange ins[2] = {{"x", nullptr, ~(size_t)0 >> 1}, {"y", buf + 8, 8}};
    CHECK(first_alias(outs, 3, ins, 2).out < 0, "null ranges take part");
}

static void check_precedence() {
    static char buf[64];
    auto is = [](AliasPair h, int out, int other, bool input) { return h.out == out && h.other == other && h.input == input; };
    const ByteRange ins[2] = {{"x", buf + 4, 4}, {"y", buf + 6, 4}};
    {   // the first output against a later output comes before the first output against an input
        const ByteRange outs[3] = {{"a", buf, 8}, {"b", buf + 32, 8}, {"c", buf + 7, 8}};
        CHECK(is(first_alias(outs, 3, ins, 2), 0, 2, false), "a and c before a and x");
    }
    {   // the first output against an input comes before the later outputs against each other; the inputs in their order
        const ByteRange outs[3] = {{"a", buf, 8}, {"b", buf + 32, 8}, {"c", buf + 36, 8}};
        CHECK(is(first_alias(outs, 3, ins, 2), 0, 0, true), "a and x before b and c, x before y");
        const ByteRange only_y[2] = {{"x", nullptr, 4}, ins[1]};
        CHECK(is(first_alias(outs, 3, only_y, 2), 0, 1, true), "a and y when x is absent");
    }
    {   // a clean first output: the second against the third, then the second against the inputs
        const ByteRange outs[3] = {{"a", buf + 48, 8}, {"b", buf + 2, 4}, {"c", buf + 5, 2}};
        CHECK(is(first_alias(outs, 3, ins, 2), 1, 2, false), "b and c");
        const ByteRange outs2[3] = {{"a", buf + 48, 8}, {"b", buf + 2, 4}, {"c", buf + 40, 2}};
        CHECK(is(first_alias(outs2, 3, ins, 2), 1, 0, true), "b and x");
        const ByteRange outs3[3] = {{"a", buf + 48, 8}, {"b", buf + 20, 4}, {"c", buf + 9, 2}};
        CHECK(is(first_alias(outs3, 3, ins, 2), 2, 1, true), "c and y");
    }
}

int main() {
    check_layouts();
    check_alias_pairs();
    check_precedence();
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("host layout ok\n");
    return 0;
}
