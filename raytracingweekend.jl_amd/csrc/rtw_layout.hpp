// rtw_layout.hpp -- byte arithmetic of the host paths, plain C++ (no HIP: a host compiler builds it alone, tests/test_host_layout.py does):
// the regions of a context's device buffer (DevLayout and the layouts built with it), the strides and extents of the batched lens stage
// and the one alias check over named byte ranges.
#pragma once
#include <cstddef>
#include <cstdint>

namespace rtwh {

// do the byte ranges [a, a + na) and [b, b + nb) share a byte?
inline bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb) { return (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na; }

// Regions of one buffer, one behind the other, each on a 16-byte boundary: add() rounds `total` up to 16, returns that offset and advances
// `total` past the region.  add(0): the rounded end.  (DevLayout{n}: regions behind the first n bytes.)
struct DevLayout {
    size_t total = 0;
    size_t add(size_t bytes) {
        const size_t off = (total + 15) & ~(size_t)15;
        total = off + bytes;
        return off;
    }
};

// ---- the alias check ---------------------------------------------------------------------------------------------
struct ByteRange { const char *name; const void *ptr; size_t bytes; };      // ptr null: absent, skipped
// The first offending pair, in this precedence: the outputs in order, each against the outputs behind it, then against the inputs in
// order.  out < 0: none.  `input`: `other` indexes `ins` (else `outs`).
struct AliasPair { int out = -1, other = -1; bool input = false; };
inline AliasPair first_alias(const ByteRange *outs, int n_out, const ByteRange *ins, int n_in) {
    for (int a = 0; a < n_out; ++a) {
        if (!outs[a].ptr) continue;
        for (int b = a + 1; b < n_out; ++b)
            if (outs[b].ptr && ranges_overlap(outs[a].ptr, outs[a].bytes, outs[b].ptr, outs[b].bytes)) return {a, b, false};
        for (int b = 0; b < n_in; ++b)
            if (ins[b].ptr && ranges_overlap(outs[a].ptr, outs[a].bytes, ins[b].ptr, ins[b].bytes)) return {a, b, true};
    }
    return {};
}

// ---- the regions of the stages (`elem`: bytes of an element; the workspace, state and moment sizes are the callers': rtw_*_bytes) ------
constexpr size_t LAYOUT_FEATURE_CHANNELS = 8;         // RTW_FEATURE_CHANNELS (rtw_host_ctx.hpp asserts it)

// The denoiser's regions: image, features, output, workspace (work_b per frame) -- each holds the frames of a batch one behind the other.
struct DenoiseLayout {
    size_t img_b, feat_b, off_feat, off_out, off_work, total;
    DenoiseLayout(size_t elem, int32_t width, int32_t height, int32_t n_views, size_t work_b) {
        const size_t frames = n_views ? (size_t)n_views : 1, n = (size_t)width * (size_t)height * frames;
        img_b = n * 3 * elem; feat_b = n * LAYOUT_FEATURE_CHANNELS * elem;
        DevLayout L;
        L.add(img_b); off_feat = L.add(feat_b); off_out = L.add(img_b); off_work = L.add(work_b * frames);
        total = L.total;
    }
};

// The upsampler's regions: small image, small features, full features, output, workspace (work_b per frame) -- frames as above.
struct UpsampleLayout {
    size_t img_b, flo_b, fhi_b, out_b, off_flo, off_fhi, off_out, off_work, total;
    UpsampleLayout(size_t elem, int32_t lo_width, int32_t lo_height, int32_t width, int32_t height, int32_t n_views, size_t work_b) {
        const size_t frames = n_views ? (size_t)n_views : 1, n_lo = (size_t)lo_width * (size_t)lo_height * frames, n_hi = (size_t)width * (size_t)height * frames;
        img_b = n_lo * 3 * elem; flo_b = n_lo * LAYOUT_FEATURE_CHANNELS * elem; fhi_b = n_hi * LAYOUT_FEATURE_CHANNELS * elem; out_b = n_hi * 3 * elem;
        DevLayout L;
        L.add(img_b); off_flo = L.add(flo_b); off_fhi = L.add(fhi_b); off_out = L.add(out_b); off_work = L.add(work_b * frames);
        total = L.total;
    }
};

// The regions of the temporal paths: the linear images and the features of `frames` views, the accumulated images, (filter: the filtered
// images,) two states, (filter: the denoiser's workspace, work_b per frame).  `paths` >= 1 (rtw_render_paths_*): each of the two states
// (state_b bytes per path) is a SET of that many, one behind the other.  Without `filter` off_flt and off_work are where those regions would start.
struct TemporalLayout {
    size_t frame_b, img_b, feat_b, st_b, off_feat, off_acc, off_flt, off_st[2], off_work, total;
    TemporalLayout(size_t elem, int32_t width, int32_t height, size_t frames, bool filter, size_t paths, size_t state_b, size_t work_b) {
        const size_t n = (size_t)width * (size_t)height;
        frame_b = n * 3 * elem; img_b = frame_b * frames; feat_b = n * LAYOUT_FEATURE_CHANNELS * elem * frames;
        st_b = state_b * paths;
        DevLayout L;
        L.add(img_b); off_feat = L.add(feat_b); off_acc = L.add(img_b); off_flt = L.add(filter ? img_b : 0);
        off_st[0] = L.add(st_b); off_st[1] = L.add(st_b); off_work = L.add(filter ? work_b * frames : 0);
        total = L.total;
    }
};

// The regions of the temporal paths with moments: TemporalLayout, then two moment planes (moment_b bytes per path; sets of `paths`) and the
// noise maps of `frames` views: total_m bytes.  The table of the `frames` steps' camera constants (rtw_reproject_table_*) lies behind
// everything else: total_p bytes, with `moments`' regions or without them.
struct MomentLayout : TemporalLayout {
    size_t mo_b, noise_b, off_mo[2], off_noise, total_m, tab_b, off_tab, total_p;
    MomentLayout(size_t elem, int32_t width, int32_t height, size_t frames, bool filter, size_t paths, bool moments, size_t state_b, size_t work_b, size_t moment_b)
        : TemporalLayout(elem, width, height, frames, filter, paths, state_b, work_b) {
        mo_b = moment_b * paths;
        noise_b = (size_t)width * (size_t)height * elem;
        DevLayout L{total};
        off_mo[0] = L.add(mo_b); off_mo[1] = L.add(mo_b); off_noise = L.add(noise_b * frames);
        total_m = L.add(0);
        tab_b = frames * 32 * elem;
        DevLayout P{moments ? total_m : total};
        off_tab = P.add(tab_b);
        total_p = P.total;
    }
};

// The workspace of the wide-aperture stage (include/rtw_hip.h rtw_wide_aperture_*), in ELEMENTS: every region begins on a multiple of four.
// scale 1 (max_radius <= 8): the defocus stage's workspace alone -- the CoC plane and the tile plane; everything else is empty.
struct WideApertureLayout {
    int scale, lo_width, lo_height, lo_mmax;
    size_t narrow, off_coc, off_tile, off_n, off_lo_img, off_lo_coc, off_lo_tile, off_lo_out, total;
    static size_t r4(size_t n) { return (n + 3) & ~(size_t)3; }
    static size_t tiles(size_t width, size_t height) { return ((height + 15) / 16) * ((width + 15) / 16); }
    WideApertureLayout(int32_t width, int32_t height, int32_t max_radius) {
        scale = max_radius <= 8 ? 1 : (max_radius <= 16 ? 2 : 4);
        lo_width = (width + scale - 1) / scale; lo_height = (height + scale - 1) / scale;
        lo_mmax = (max_radius + scale - 1) / scale;
        const size_t n = (size_t)width * (size_t)height, n_lo = (size_t)lo_width * (size_t)lo_height;
        narrow = n * 4 + r4(tiles(width, height));
        off_coc = narrow; off_tile = off_coc + n * 4; off_n = off_tile + r4(tiles(width, height));
        off_lo_img = off_n + r4(n * 3); off_lo_coc = off_lo_img + r4(n_lo * 3); off_lo_tile = off_lo_coc + n_lo * 4;
        off_lo_out = off_lo_tile + r4(tiles(lo_width, lo_height));
        total = scale == 1 ? narrow : off_lo_out + r4(n_lo * 3);
    }
};

// The lens stages (include/rtw_hip.h rtw_defocus_*, rtw_wide_aperture_*, rtw_lens_batch_*), in BYTES.  n_views >= 1: a batch of that many
// views of one size, each with its own output frame and its own workspace (the single stage's layout above, work_stride bytes: a multiple
// of 16); n_frames == n_views: view v reads frame v of the images and the features; n_frames == 1: every view reads frame 0, the input
// strides are 0 and the inputs' extents one frame's.  n_views == 0: the SINGLE call -- one frame in, one out, one workspace, NO table
// (tab_b == 0: its region is empty and `total` ends behind the workspace); n_frames is not read.
// *_stride: from one view to the next; *_b: the extent of the whole call; off_*, total: the regions of a context's device buffer for the
// host-buffer form -- images at 0, features, outputs, workspaces, the lens table (32 elements per view).
struct LensBatchLayout {
    size_t frame_b, img_stride, feat_stride, out_stride, work_stride, img_b, feat_b, out_b, work_b, tab_b, off_feat, off_out, off_work, off_tab, total;
    LensBatchLayout(size_t elem, int32_t width, int32_t height, int32_t max_radius, int32_t n_views, int32_t n_frames) {
        const size_t n = (size_t)width * (size_t)height, views = n_views ? (size_t)n_views : 1, frames = n_views ? (size_t)n_frames : 1;
        frame_b = n * 3 * elem;
        img_stride = frames > 1 ? frame_b : 0; feat_stride = frames > 1 ? n * LAYOUT_FEATURE_CHANNELS * elem : 0;
        out_stride = frame_b; work_stride = WideApertureLayout(width, height, max_radius).total * elem;
        img_b = frame_b * frames; feat_b = n * LAYOUT_FEATURE_CHANNELS * elem * frames;
        out_b = out_stride * views; work_b = work_stride * views; tab_b = n_views ? views * 32 * elem : 0;
        DevLayout L;
        L.add(img_b); off_feat = L.add(feat_b); off_out = L.add(out_b); off_work = L.add(work_b); off_tab = L.add(tab_b);
        total = L.total;
    }
};

// Ray queries (include/rtw_hip.h rtw_cast_rays_*), in BYTES: n rays of 8 elements, n indices of 4 bytes, n records of 8 elements (records
// false: none -- the region is empty).  off_*, total: the regions of a context's device buffer for the host-buffer form -- the indices at
// 0 (what the one-device path copies out last), the records, the rays.
struct RaysLayout {
    size_t rays_b, idx_b, rec_b, off_rec, off_rays, total;
    RaysLayout(size_t elem, int64_t n, bool records) {
        const size_t rays = n > 0 ? (size_t)n : 0;
        rays_b = rays * 8 * elem; idx_b = rays * sizeof(int32_t); rec_b = records ? rays * 8 * elem : 0;
        DevLayout L;
        L.add(idx_b); off_rec = L.add(rec_b); off_rays = L.add(rays_b);
        total = L.total;
    }
};
// The persistent grid of the ray kernel: workgroups of 256 lanes, min(ceil(n / 256), CUs x resident workgroups per CU), capped by
// max_workgroups when that is not 0; at least 1.  (n < 2^31, so the result fits an int whatever the device reports.)
inline int rays_grid(int64_t n, int num_cus, int blocks_per_cu, int32_t max_workgroups) {
    int64_t g = (n + 255) / 256;
    const int64_t resident = (int64_t)(num_cus > 0 ? num_cus : 1) * (blocks_per_cu > 0 ? blocks_per_cu : 1);
    if (g > resident) g = resident;
    if (max_workgroups > 0 && g > max_workgroups) g = max_workgroups;
    return g < 1 ? 1 : (int)g;
}

// Radiance queries (include/rtw_hip.h rtw_trace_rays_*), in BYTES: n rays of 8 elements, n results of 3 binary64 whatever the element is.
// off_rays, total: the regions of a context's device buffer for the host-buffer form -- the results at 0 (what the one-device path copies
// out), the rays behind them.
struct TraceRaysLayout {
    size_t rays_b, out_b, off_rays, total;
    TraceRaysLayout(size_t elem, int64_t n) {
        const size_t rays = n > 0 ? (size_t)n : 0;
        rays_b = rays * 8 * elem; out_b = rays * 3 * sizeof(double);
        DevLayout L;
        L.add(out_b); off_rays = L.add(rays_b);
        total = L.total;
    }
};
// does first + count leave the unsigned 64-bit range?  (the streams first_stream + i of n rays, the samples first_sample + s of spp)
inline bool u64_range_wraps(uint64_t first, uint64_t count) { return first > UINT64_MAX - count; }
// The grid of the radiance kernel: the ray kernel's -- ceil(n / 256) workgroups, capped by the resident ones and by max_workgroups, at
// least 1.  Its waves CLAIM batches of 64 rays from a counter, so every grid >= 1 walks every batch exactly once.
inline int trace_rays_grid(int64_t n, int num_cus, int blocks_per_cu, int32_t max_workgroups) { return rays_grid(n, num_cus, blocks_per_cu, max_workgroups); }
// batches of 64 rays in a list of n (n < 2^31)
inline unsigned trace_rays_batches(int64_t n) { return n > 0 ? (unsigned)((n + 63) / 64) : 0u; }

}  // namespace rtwh
