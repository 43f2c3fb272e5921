// The byte arithmetic of the batched lens stage (csrc/rtw_layout.hpp LensBatchLayout) on the CPU, a program of its own: tests/test_lens_batch_layout.py
// builds it with the host compiler's address and undefined-behaviour sanitizers and runs it.  The strides, extents and regions are restated
// here from the header's words (include/rtw_hip.h rtw_lens_batch_*) and every view's bytes are WRITTEN into a buffer of exactly `total`
// bytes: a view that left its region, or two regions that shared a byte, would be reported by the sanitizer or by the checks below.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../raytracingweekend.jl_amd/csrc/rtw_layout.hpp"

using namespace rtwh;

static int failures = 0;
#define CHECK(cond)                                                                       \
    do {                                                                                  \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static size_t r4(size_t n) { return (n + 3) / 4 * 4; }
static size_t tiles(size_t w, size_t h) { return ((h + 15) / 16) * ((w + 15) / 16); }

// the single stage's workspace in elements, from the header's table of regions
static size_t work_elems(size_t W, size_t H, int max_radius) {
    const size_t narrow = 4 * W * H + r4(tiles(W, H));
    if (max_radius <= 8) return narrow;
    const size_t s = max_radius <= 16 ? 2 : 4, w = (W + s - 1) / s, h = (H + s - 1) / s;
    return narrow + 4 * W * H + r4(tiles(W, H)) + r4(3 * W * H) + r4(3 * w * h) + 4 * w * h + r4(tiles(w, h)) + r4(3 * w * h);
}

int main() {
    const int sizes[][2] = {{1, 1}, {5, 3}, {17, 33}, {33, 17}, {130, 5}, {96, 54}};
    const int radii[] = {1, 8, 9, 16, 17, 32};
    const int views[] = {1, 2, 3, 7};
    for (const auto &sz : sizes)
        for (size_t elem : {(size_t)4, (size_t)8})
            for (int mr : radii)
                for (int nv : views)
                    for (int nf : {nv, 1}) {
                        const size_t W = (size_t)sz[0], H = (size_t)sz[1];
                        const LensBatchLayout L(elem, sz[0], sz[1], mr, nv, nf);
                        const size_t frame = W * H * 3 * elem, feat = W * H * 8 * elem, work = work_elems(W, H, mr) * elem;
                        CHECK(work == WideApertureLayout(sz[0], sz[1], mr).total * elem);
                        CHECK(L.frame_b == frame && L.out_stride == frame && L.work_stride == work && work % 16 == 0);
                        CHECK(L.img_stride == (nf > 1 ? frame : 0) && L.feat_stride == (nf > 1 ? feat : 0));
                        CHECK(L.img_b == frame * (size_t)nf && L.feat_b == feat * (size_t)nf && L.out_b == frame * (size_t)nv && L.work_b == work * (size_t)nv);
                        CHECK(L.tab_b == (size_t)nv * 32 * elem);
                        // the regions: each on a 16-byte boundary behind the one before it, `total` the end of the last
                        const size_t off[5] = {0, L.off_feat, L.off_out, L.off_work, L.off_tab}, len[5] = {L.img_b, L.feat_b, L.out_b, L.work_b, L.tab_b};
                        for (int k = 0; k < 5; ++k) {
                            CHECK(off[k] % 16 == 0);
                            if (k) CHECK(off[k] >= off[k - 1] + len[k - 1] && off[k] < off[k - 1] + len[k - 1] + 16);
                        }
                        CHECK(L.total == L.off_tab + L.tab_b);
                        // every view writes its own bytes: the count of bytes written once is the sum of the regions
                        std::vector<unsigned char> buf(L.total, 0);
                        for (int v = 0; v < nv; ++v) {
                            unsigned char *img = buf.data() + (size_t)v * L.img_stride, *ft = buf.data() + L.off_feat + (size_t)v * L.feat_stride;
                            unsigned char *out = buf.data() + L.off_out + (size_t)v * L.out_stride, *wk = buf.data() + L.off_work + (size_t)v * L.work_stride;
                            unsigned char *tab = buf.data() + L.off_tab + (size_t)v * 32 * elem;
                            if (nf > 1 || v == 0) { for (size_t k = 0; k < frame; ++k) ++img[k]; for (size_t k = 0; k < feat; ++k) ++ft[k]; }
                            for (size_t k = 0; k < frame; ++k) ++out[k];
                            for (size_t k = 0; k < work; ++k) ++wk[k];
                            for (size_t k = 0; k < 32 * elem; ++k) ++tab[k];
                            CHECK(((size_t)(wk - buf.data())) % 16 == 0);
                        }
                        size_t once = 0, more = 0;
                        for (unsigned char c : buf) { once += c == 1; more += c > 1; }
                        CHECK(more == 0 && once == L.img_b + L.feat_b + L.out_b + L.work_b + L.tab_b);
                    }
    // n_views == 0, the SINGLE call: one frame in, one out, one workspace and NO table -- the regions are the denoiser's of one frame with
    // this stage's workspace (what the single host forms used before they shared this layout), whatever n_frames says; a batch of one
    // view has the same strides, extents and offsets and the table behind them
    for (const auto &sz : sizes)
        for (size_t elem : {(size_t)4, (size_t)8})
            for (int mr : radii)
                for (int nf : {0, 1, 5}) {
                    const size_t W = (size_t)sz[0], H = (size_t)sz[1];
                    const LensBatchLayout L(elem, sz[0], sz[1], mr, 0, nf), B(elem, sz[0], sz[1], mr, 1, 1);
                    const size_t frame = W * H * 3 * elem, feat = W * H * 8 * elem, work = work_elems(W, H, mr) * elem;
                    const DenoiseLayout D(elem, sz[0], sz[1], 0, work);
                    CHECK(L.frame_b == frame && L.img_b == frame && L.out_b == frame && L.feat_b == feat && L.work_b == work && L.work_stride == work && L.out_stride == frame);
                    CHECK(L.img_stride == 0 && L.feat_stride == 0);
                    CHECK(L.tab_b == 0 && L.total == L.off_work + L.work_b && L.off_tab == L.total);
                    CHECK(L.off_feat == D.off_feat && L.off_out == D.off_out && L.off_work == D.off_work && L.total == D.total && L.img_b == D.img_b && L.feat_b == D.feat_b);
                    CHECK(L.off_feat == B.off_feat && L.off_out == B.off_out && L.off_work == B.off_work && L.off_tab == B.off_tab && B.total == L.total + 32 * elem);
                    CHECK(L.img_b == B.img_b && L.feat_b == B.feat_b && L.out_b == B.out_b && L.work_b == B.work_b && L.img_stride == B.img_stride && L.feat_stride == B.feat_stride);
                    std::vector<unsigned char> buf(L.total, 0);
                    for (size_t k = 0; k < L.img_b; ++k) ++buf[k];
                    for (size_t k = 0; k < L.feat_b; ++k) ++buf[L.off_feat + k];
                    for (size_t k = 0; k < L.out_b; ++k) ++buf[L.off_out + k];
                    for (size_t k = 0; k < L.work_b; ++k) ++buf[L.off_work + k];
                    size_t once = 0, more = 0;
                    for (unsigned char c : buf) { once += c == 1; more += c > 1; }
                    CHECK(more == 0 && once == L.img_b + L.feat_b + L.out_b + L.work_b);
                }
    // the defocus stage's workspace is the narrow part of the wide-aperture stage's, and all of it up to max_radius 8
    for (const auto &sz : sizes) {
        const size_t W = (size_t)sz[0], H = (size_t)sz[1];
        CHECK(WideApertureLayout(sz[0], sz[1], 8).narrow == 4 * W * H + r4(tiles(W, H)) && WideApertureLayout(sz[0], sz[1], 8).total == WideApertureLayout(sz[0], sz[1], 32).narrow);
        CHECK(WideApertureLayout::tiles(W, H) == tiles(W, H));
    }
    // the extents the alias check sees: with n_frames == 1 an output one frame behind the images' start is free, with n_frames == n_views it is not
    {
        const LensBatchLayout one(4, 10, 6, 16, 3, 1), all(4, 10, 6, 16, 3, 3);
        unsigned char *base = (unsigned char *)0x100000;
        CHECK(!ranges_overlap(base + one.frame_b, one.out_b, base, one.img_b));
        CHECK(ranges_overlap(base + all.frame_b, all.out_b, base, all.img_b));
        CHECK(ranges_overlap(base + one.frame_b - 1, one.out_b, base, one.img_b));
    }
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("lens batch layout ok\n");
    return 0;
}
