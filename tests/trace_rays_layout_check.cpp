// The byte arithmetic of the radiance queries (csrc/rtw_layout.hpp, plain C++) on the CPU: the regions of the host form's device buffer, the
// alias ranges of its two host buffers, the two 64-bit range checks, the batch count and the grid.  Built with the host compiler and its
// address / undefined-behaviour sanitizers and run by tests/test_trace_rays_layout.py.  No GPU, no HIP.
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
    const int64_t counts[] = {0, 1, 3, 63, 64, 65, 129, 257, 1000, 1920 * 1080, ((int64_t)1 << 31) - 1};
    for (int64_t n : counts)
        for (size_t elem : {(size_t)4, (size_t)8}) {
            const TraceRaysLayout R(elem, n);
            const size_t un = (size_t)n;
            CHECK(R.rays_b == un * 8 * elem && R.out_b == un * 24, "n %lld elem %zu", (long long)n, elem);
            CHECK(R.off_rays % 16 == 0, "n %lld: offset %zu", (long long)n, R.off_rays);
            CHECK(R.off_rays >= R.out_b && R.off_rays < R.out_b + 16, "n %lld: rays at %zu behind %zu bytes of results", (long long)n, R.off_rays, R.out_b);
            CHECK(R.total == R.off_rays + R.rays_b, "n %lld: total %zu", (long long)n, R.total);
        }
    const TraceRaysLayout neg(4, -5);
    CHECK(neg.total == 0 && neg.rays_b == 0 && neg.out_b == 0, "a negative count holds nothing");
    // the regions really hold what the kernel reads and writes: walk a small buffer the way the host form does
    for (int64_t n : {1, 63, 65, 257})
        for (size_t elem : {(size_t)4, (size_t)8}) {
            const TraceRaysLayout R(elem, n);
            std::vector<unsigned char> buf(R.total, 0);
            for (int64_t i = 0; i < n; ++i) {
                for (size_t b = 0; b < 24; ++b) buf[(size_t)i * 24 + b] += 1;
                for (size_t b = 0; b < 8 * elem; ++b) buf[R.off_rays + (size_t)i * 8 * elem + b] += 1;
            }
            size_t twice = 0;
            for (unsigned char c : buf) twice += c > 1;
            CHECK(twice == 0, "n %lld: %zu bytes belong to two regions", (long long)n, twice);
        }
}

static void check_alias_ranges() {
    // the host form's call: the results against the rays
    std::vector<unsigned char> mem(4096);
    unsigned char *base = mem.data();
    const TraceRaysLayout R(4, 10);
    auto first = [&](const void *out, const void *rays) {
        const ByteRange outs[1] = {{"out", out, R.out_b}}, ins[1] = {{"rays", rays, R.rays_b}};
        return first_alias(outs, 1, ins, 1);
    };
    CHECK(first(base, base + 1024).out < 0, "disjoint buffers");
    CHECK(first(base, base + R.out_b).out < 0 && first(base + R.rays_b, base).out < 0, "touching buffers share no byte");
    AliasPair p = first(base + 1024, base + 1024);
    CHECK(p.out == 0 && p.other == 0 && p.input, "out on the rays");
    p = first(base + 1024 + R.rays_b - 1, base + 1024);
    CHECK(p.out == 0 && p.input, "out on the last byte of the rays");
    p = first(base + 1024 - R.out_b + 1, base + 1024);
    CHECK(p.out == 0 && p.input, "the last byte of out on the rays");
    const TraceRaysLayout Z(8, 0);
    const ByteRange outs[1] = {{"out", base, Z.out_b}}, ins[1] = {{"rays", base, Z.rays_b}};
    CHECK(first_alias(outs, 1, ins, 1).out < 0, "empty ranges share nothing");
}

static void check_ranges() {
    const uint64_t top = UINT64_MAX;
    CHECK(!u64_range_wraps(0, 0) && !u64_range_wraps(0, top) && !u64_range_wraps(top, 0) && !u64_range_wraps(top - 10, 10), "sums up to 2^64 - 1 stay");
    CHECK(u64_range_wraps(top, 1) && u64_range_wraps(top - 9, 10) && u64_range_wraps(1, top) && u64_range_wraps(top, top), "sums of 2^64 and more wrap");
    CHECK(!u64_range_wraps((uint64_t)1 << 63, ((uint64_t)1 << 63) - 1) && u64_range_wraps((uint64_t)1 << 63, (uint64_t)1 << 63), "the middle");
    // the largest call: n = 2^31 - 1 rays, spp = 2^31 - 1
    const uint64_t big = ((uint64_t)1 << 31) - 1;
    CHECK(!u64_range_wraps(top - big, big) && u64_range_wraps(top - big + 1, big), "the largest n and spp");
}

static void check_batches_and_grid() {
    CHECK(trace_rays_batches(0) == 0 && trace_rays_batches(-3) == 0 && trace_rays_batches(1) == 1 && trace_rays_batches(64) == 1 && trace_rays_batches(65) == 2, "ceil(n / 64)");
    CHECK(trace_rays_batches(((int64_t)1 << 31) - 1) == (1u << 25), "n < 2^31 fits");
    CHECK(trace_rays_grid(1, 256, 8, 0) == 1 && trace_rays_grid(257, 256, 8, 0) == 2 && trace_rays_grid(1000, 256, 8, 3) == 3 && trace_rays_grid(1000, 256, 8, 9) == 4, "the ray kernel's grid");
    CHECK(trace_rays_grid(1920 * 1080, 256, 3, 0) == 768 && trace_rays_grid(5, 0, 0, 0) == 1 && trace_rays_grid(0, 256, 8, 0) == 1, "resident, never below 1");
    // the waves claim batches from a counter: whatever the grid and whoever claims, a counter that hands out 0, 1, 2, ... gives every batch
    // of 64 rays to exactly one wave, every ray to exactly one (batch, lane), and a claim past the last batch ends a wave
    for (int64_t n : {1, 63, 64, 65, 129, 257, 1000})
        for (int cap : {0, 1, 3}) {
            const int waves = 4 * trace_rays_grid(n, 256, 4, cap);
            const unsigned batches = trace_rays_batches(n);
            std::vector<int> seen((size_t)n, 0);
            unsigned counter = 0, ended = 0;
            for (int turn = 0; ended < (unsigned)waves; ++turn) {            // the waves claim in turn (any order gives the same sets)
                const unsigned b = counter++;
                if (b >= batches) { ++ended; continue; }
                const uint64_t first = (uint64_t)b * 64, end = first + 64 < (uint64_t)n ? first + 64 : (uint64_t)n;
                for (uint64_t i = first; i < end; ++i) seen[(size_t)i] += 1;
            }
            size_t bad = 0;
            for (int s : seen) bad += s != 1;
            CHECK(bad == 0 && counter == batches + (unsigned)waves, "n %lld cap %d: %zu rays not taken exactly once", (long long)n, cap, bad);
        }
}

int main() {
    check_layout();
    check_alias_ranges();
    check_ranges();
    check_batches_and_grid();
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("trace rays layout ok\n");
    return 0;
}
