// The byte arithmetic of the ray queries (csrc/rtw_layout.hpp, plain C++) on the CPU: the regions of the host form's device buffer, the alias
// ranges of its three host buffers and the persistent grid.  Built with the host compiler and its address / undefined-behaviour sanitizers
// and run by tests/test_rays_layout.py.  No GPU, no HIP.
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

static void check_layout() {
    const int64_t counts[] = {0, 1, 3, 63, 64, 65, 255, 256, 257, 1000, 1920 * 1080, ((int64_t)1 << 31) - 1};
    for (int64_t n : counts)
        for (size_t elem : {(size_t)4, (size_t)8})
            for (bool records : {false, true}) {
                const RaysLayout R(elem, n, records);
                const size_t un = (size_t)n;
                CHECK(R.rays_b == un * 8 * elem && R.idx_b == un * 4 && R.rec_b == (records ? un * 8 * elem : 0), "n %lld elem %zu", (long long)n, elem);
                CHECK(R.off_rec % 16 == 0 && R.off_rays % 16 == 0, "n %lld: offsets %zu %zu", (long long)n, R.off_rec, R.off_rays);
                CHECK(R.off_rec >= R.idx_b && R.off_rec < R.idx_b + 16, "n %lld: records at %zu behind %zu bytes of indices", (long long)n, R.off_rec, R.idx_b);
                CHECK(R.off_rays >= R.off_rec + R.rec_b && R.off_rays < R.off_rec + R.rec_b + 16, "n %lld: rays at %zu", (long long)n, R.off_rays);
                CHECK(R.total == R.off_rays + R.rays_b, "n %lld: total %zu", (long long)n, R.total);
            }
    const RaysLayout neg(4, -5, true);
    CHECK(neg.total == 0 && neg.rays_b == 0, "a negative count holds nothing");
    // the regions really hold what the kernel writes: walk a small buffer the way the host form does
    for (int64_t n : {1, 63, 65, 257}) {
        const RaysLayout R(4, n, true);
        std::vector<unsigned char> buf(R.total, 0);
        for (int64_t i = 0; i < n; ++i) {
            for (int b = 0; b < 4; ++b) buf[(size_t)i * 4 + b] += 1;
            for (int b = 0; b < 32; ++b) { buf[R.off_rec + (size_t)i * 32 + b] += 1; buf[R.off_rays + (size_t)i * 32 + b] += 1; }
        }
        size_t twice = 0;
        for (unsigned char c : buf) twice += c > 1;
        CHECK(twice == 0, "n %lld: %zu bytes belong to two regions", (long long)n, twice);
    }
}

static void check_alias_ranges() {
    // the host form's call: outputs idx, rec against each other, then against the rays; a null rec is skipped
    std::vector<unsigned char> mem(4096);
    unsigned char *base = mem.data();
    const RaysLayout R(4, 10, true);
    auto first = [&](const void *idx, const void *rec, const void *rays) {
        const ByteRange outs[2] = {{"idx", idx, R.idx_b}, {"rec", rec, R.rec_b}}, ins[1] = {{"rays", rays, R.rays_b}};
        return first_alias(outs, 2, ins, 1);
    };
    AliasPair p = first(base, base + 64, base + 1024);
    CHECK(p.out < 0, "disjoint buffers");
    p = first(base, base + R.idx_b, base + R.idx_b + R.rec_b);
    CHECK(p.out < 0, "touching buffers share no byte");
    p = first(base, base + R.idx_b - 1, base + 1024);
    CHECK(p.out == 0 && p.other == 1 && !p.input, "idx and rec share one byte");
    p = first(base + 1024 + 16, base, base + 1024);
    CHECK(p.out == 0 && p.other == 0 && p.input, "idx inside the rays");
    p = first(base, base + 1024 + R.rays_b - 1, base + 1024);
    CHECK(p.out == 1 && p.other == 0 && p.input, "rec on the last byte of the rays");
    p = first(base + 1024, nullptr, base + 1024);
    CHECK(p.out == 0 && p.input, "a null rec is skipped, idx on the rays is found");
    p = first(base, nullptr, base + 1024);
    CHECK(p.out < 0, "a null rec is skipped");
    const RaysLayout Z(8, 0, true);
    const ByteRange outs[2] = {{"idx", base, Z.idx_b}, {"rec", base, Z.rec_b}}, ins[1] = {{"rays", base, Z.rays_b}};
    CHECK(first_alias(outs, 2, ins, 1).out < 0, "empty ranges share nothing");
}

static void check_grid() {
    CHECK(rays_grid(1, 256, 8, 0) == 1 && rays_grid(256, 256, 8, 0) == 1 && rays_grid(257, 256, 8, 0) == 2, "one workgroup per 256 rays");
    CHECK(rays_grid(1000, 256, 8, 0) == 4 && rays_grid(1000, 256, 8, 1) == 1 && rays_grid(1000, 256, 8, 3) == 3 && rays_grid(1000, 256, 8, 9) == 4, "max_workgroups caps");
    CHECK(rays_grid(1920 * 1080, 256, 8, 0) == 2048 && rays_grid(1920 * 1080, 256, 3, 0) == 768 && rays_grid(1920 * 1080, 256, 8, 100000) == 2048, "the resident grid");
    CHECK(rays_grid(((int64_t)1 << 31) - 1, 256, 8, 0) == 2048 && rays_grid(((int64_t)1 << 31) - 1, 1 << 20, 1 << 10, 0) == (1 << 23), "n < 2^31 fits");
    CHECK(rays_grid(5, 0, 0, 0) == 1 && rays_grid(100000, 0, -3, 0) == 1 && rays_grid(0, 256, 8, 0) == 1, "never below 1");
    for (int64_t n : {1, 64, 65, 1000, 100000})
        for (int cap : {0, 1, 3, 7}) {
            const int g = rays_grid(n, 256, 4, cap);
            // every batch of 64 rays belongs to exactly one (workgroup, wave, trip)
            const int64_t batches = (n + 63) / 64;
            std::vector<int> seen((size_t)batches, 0);
            for (int64_t wg = 0; wg < g; ++wg)
                for (int wave = 0; wave < 4; ++wave)
                    for (int64_t b = wg * 4 + wave; b < batches; b += 4 * (int64_t)g) seen[(size_t)b] += 1;
            size_t bad = 0;
            for (int s : seen) bad += s != 1;
            CHECK(bad == 0, "n %lld cap %d grid %d: %zu batches not walked exactly once", (long long)n, cap, g, bad);
        }
}

int main() {
    check_layout();
    check_alias_ranges();
    check_grid();
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("rays layout ok\n");
    return 0;
}
