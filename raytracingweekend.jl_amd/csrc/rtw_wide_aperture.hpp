// rtw_wide_aperture.hpp -- the two kernels the wide-aperture stage adds to the defocus stage's (include/rtw_hip.h rtw_wide_aperture_*: the
// definition is there).  The stage gathers a copy of the frame reduced by S = 2 or 4 with df_gather as it is, so that a circle of confusion of up to
// 32 px costs a window of at most 8 small pixels, and blends the result back by the radius.
//   wa_reduce<T, S>   one workgroup per 16 x 16 SMALL tile, lane t at small row t % 16, small column t / 16 (df_prepare's mapping).  A lane reads its
//                     S x S block column by column: its S rows of one column are consecutive slots of the column-major planes, the 16 lanes of a
//                     small column read 16*S consecutive slots.  The CoC slots are loaded whole (16 / 32 bytes).  Two divisions per channel or
//                     radius: by the count (colour, radius) and 1 / Rh^2.  The tile's greatest R_s: six cross-lane exchanges per wave, one pass
//                     over the four waves' maxima in LDS, as in df_prepare.
//   wa_compose<T, S>  one full-size pixel per lane, the 16 x 16 tile mapping.  The four bilinear taps are read from global memory: the S x S
//                     pixels of a block share them, so a wave's 64 pixels touch at most (16/S + 1) * (4/S + 1) small pixels, and the small
//                     planes (1/4 or 1/16 of the frame) stay in L2.  No LDS, no barrier.
//   VIEWS             true (rtw_lens_batch_device_*): n_views views in one launch, rtw_defocus.hpp DfViews with one stride per pointer;
//                     false: the instance is the single form's, instruction for instruction.
// Every operation is rounded once (the Makefile's -ffp-contract=off -fno-fast-math); divisions and sqrt are the compiler's IEEE ones; what does not
// take part is dropped by selects.  A block's pixels outside the frame are not loaded.
#pragma once
#include "rtw_defocus.hpp"

namespace rtw {

constexpr int WA_MAX_RADIUS = 32;       // RTW_WIDE_APERTURE_MAX_RADIUS

template <typename T, int S, bool VIEWS = false>
__global__ __launch_bounds__(256) void wa_reduce(int W_, int H_, const T *__restrict__ image, const typename DnVec<T>::type *__restrict__ coc, T *__restrict__ lo_image,
                                                 typename DnVec<T>::type *__restrict__ lo_coc, T *__restrict__ lo_tile, [[maybe_unused]] DfViews<T, VIEWS, 5> B) {
    using V = typename DnVec<T>::type;
    __shared__ T s_r[4];
    if constexpr (VIEWS) {
        const long long v = df_view();
        if (v >= B.n_views) return;
        image = tp_adv(image, v * B.stride[0]); coc = tp_adv(coc, v * B.stride[1]); lo_image = tp_adv(lo_image, v * B.stride[2]);
        lo_coc = tp_adv(lo_coc, v * B.stride[3]); lo_tile = tp_adv(lo_tile, v * B.stride[4]);
    }
    const int H = H_, W = W_;
    const int h = (H + S - 1) / S, w = (W + S - 1) / S;
    const int th = (h + DF_TILE - 1) / DF_TILE;
    const int tb = (int)(blockIdx.x / (unsigned)th), ta = (int)blockIdx.x - tb * th;
    const int t = (int)threadIdx.x;
    const int a = ta * DF_TILE + (t & 15), b = tb * DF_TILE + (t >> 4);
    T R = T(-1);                                    // (a lane outside the small frame, a block with no valid pixel: never above a valid block's R_s >= 0)
    if (a < h && b < w) {
        T c0 = T(0), c1 = T(0), c2 = T(0), rs = T(0), zm = df_inf<T>();
        int n = 0;
#pragma unroll
        for (int dc = 0; dc < S; ++dc) {
            const int j = b * S + dc;
            if (j < W) {
#pragma unroll
                for (int dr = 0; dr < S; ++dr) {
                    const int i = a * S + dr;
                    if (i < H) {
                        const long long P = (long long)j * H + i;
                        const V s = coc[P];
                        const T q0 = image[P * 3 + 0], q1 = image[P * 3 + 1], q2 = image[P * 3 + 2];
                        const bool ok = s.y == s.y;
                        const T e0 = c0 + q0, e1 = c1 + q1, e2 = c2 + q2, er = rs + s.x;
                        c0 = ok ? e0 : c0; c1 = ok ? e1 : c1; c2 = ok ? e2 : c2; rs = ok ? er : rs;
                        zm = (ok && s.y < zm) ? s.y : zm;
                        n += ok ? 1 : 0;
                    }
                }
            }
        }
        const bool any = n > 0;
        const T cnt = (T)(any ? n : 1);
        const T Rs = (rs / cnt) * T(1.0 / S);
        const T Rh = df_max<T>(Rs, T(0.5));
        const T wq = T(1) / (Rh * Rh);
        const long long p = (long long)b * h + a;
        lo_image[p * 3 + 0] = any ? c0 / cnt : T(0);
        lo_image[p * 3 + 1] = any ? c1 / cnt : T(0);
        lo_image[p * 3 + 2] = any ? c2 / cnt : T(0);
        R = any ? Rs : T(-1);
        V s;
        s.x = R; s.y = any ? zm : dn_nan<T>(); s.z = any ? wq : T(0); s.w = T(0);
        lo_coc[p] = s;
    }
    // ---- the small tile's maximum: the wave's, then the four waves'
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) R = df_max<T>(__shfl_xor(R, m), R);
    if ((t & 63) == 0) s_r[t >> 6] = R;
    __syncthreads();
    if (t == 0) lo_tile[blockIdx.x] = df_max<T>(df_max<T>(s_r[1], s_r[0]), df_max<T>(s_r[3], s_r[2]));
}

// coc: the WIDE CoC plane; narrow: N, the defocus stage's output with max_radius 8, linear; lo_coc, lo_out: the small CoC plane and the small gather's image O
template <typename T, int S, bool VIEWS = false>
__global__ __launch_bounds__(256) void wa_compose(int W_, int H_, int gamma, const typename DnVec<T>::type *__restrict__ coc, const T *__restrict__ narrow,
                                                  const typename DnVec<T>::type *__restrict__ lo_coc, const T *__restrict__ lo_out, T *__restrict__ out,
                                                  [[maybe_unused]] DfViews<T, VIEWS, 5> B) {
    using V = typename DnVec<T>::type;
    if constexpr (VIEWS) {
        const long long v = df_view();
        if (v >= B.n_views) return;
        coc = tp_adv(coc, v * B.stride[0]); narrow = tp_adv(narrow, v * B.stride[1]); lo_coc = tp_adv(lo_coc, v * B.stride[2]);
        lo_out = tp_adv(lo_out, v * B.stride[3]); out = tp_adv(out, v * B.stride[4]);
    }
    constexpr int LOG2 = S == 2 ? 2 : 3;            // 2S = 1 << LOG2
    const int H = H_, W = W_;
    const int h = (H + S - 1) / S, w = (W + S - 1) / S;
    const int TH = (H + DF_TILE - 1) / DF_TILE;
    const int tb = (int)(blockIdx.x / (unsigned)TH), ta = (int)blockIdx.x - tb * TH;
    const int t = (int)threadIdx.x;
    const int i = ta * DF_TILE + (t & 15), j = tb * DF_TILE + (t >> 4);
    if (i >= H || j >= W) return;
    const long long P = (long long)j * H + i;
    const V sx = coc[P];
    const bool valid = sx.y == sx.y;
    const T n0 = narrow[P * 3 + 0], n1 = narrow[P * 3 + 1], n2 = narrow[P * 3 + 2];
    // ---- the bilinear taps: floor division and remainder by 2S as a shift and a mask (u may be negative: the shift is arithmetic); the
    // quotient by T(2S), a power of two, as the product with its reciprocal -- the same bits
    const int u = 2 * i + 1 - S, v = 2 * j + 1 - S;
    const int a0 = u >> LOG2, b0 = v >> LOG2;
    const T fy = (T)(u & (2 * S - 1)) * T(0.5 / S), fx = (T)(v & (2 * S - 1)) * T(0.5 / S);
    const T wy[2] = {T(1) - fy, fy}, wx[2] = {T(1) - fx, fx};
    const int ra[2] = {a0 < 0 ? 0 : a0, a0 + 1 > h - 1 ? h - 1 : a0 + 1}, cb[2] = {b0 < 0 ? 0 : b0, b0 + 1 > w - 1 ? w - 1 : b0 + 1};
    T ws = T(0), s0 = T(0), s1 = T(0), s2 = T(0);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const long long q = (long long)cb[c] * h + ra[r];
            const V sq = lo_coc[q];
            const T q0 = lo_out[q * 3 + 0], q1 = lo_out[q * 3 + 1], q2 = lo_out[q * 3 + 2];
            const bool ok = sq.y == sq.y;
            const T wt = wy[r] * wx[c];
            const T e = ws + wt, e0 = s0 + wt * q0, e1 = s1 + wt * q1, e2 = s2 + wt * q2;
            ws = ok ? e : ws; s0 = ok ? e0 : s0; s1 = ok ? e1 : s1; s2 = ok ? e2 : s2;
        }
    }
    const T u0 = s0 / ws, u1 = s1 / ws, u2 = s2 / ws;
    const T tt = df_clamp01<T>((sx.x - T(4)) * T(0.25));
    T o0 = tt <= T(0) ? n0 : (tt >= T(1) ? u0 : n0 + tt * (u0 - n0));
    T o1 = tt <= T(0) ? n1 : (tt >= T(1) ? u1 : n1 + tt * (u1 - n1));
    T o2 = tt <= T(0) ? n2 : (tt >= T(1) ? u2 : n2 + tt * (u2 - n2));
    if (gamma) { o0 = dn_sqrt(o0); o1 = dn_sqrt(o1); o2 = dn_sqrt(o2); }
    out[P * 3 + 0] = valid ? o0 : dn_nan<T>();
    out[P * 3 + 1] = valid ? o1 : dn_nan<T>();
    out[P * 3 + 2] = valid ? o2 : dn_nan<T>();
}

}  // namespace rtw
