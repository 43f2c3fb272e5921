// rtw_upsample.hpp -- the kernel of the feature-guided upsampler (include/rtw_hip.h rtw_upsample_*: the definition is there): a full-size image
// from a small frame's filtered colour plane and a full-size feature buffer.
//   up_sample      one FULL-SIZE pixel per lane, lanes along i.  The pixel's own guides (cov, n, z, a) are computed inline from its two feature
//                  vectors; its 4 x 4 taps come from the small frame's planes as the denoiser's prepare and level kernels leave them
//                  (rtw_denoise.hpp: E = (e0, e1, e2, z), G = (n.x, n.y, n.z, cov; cov = NaN: not valid), A = (a0, a1, a2, .)), read from
//                  global memory (L1 / L2): a wave's taps in one column are about 35 consecutive slots of each plane.
// No atomics, no cross-lane operation; the trip count over the 16 taps is uniform, skipped taps are dropped by selects, as in dn_tap.
// Every operation is rounded once (the Makefile's -ffp-contract=off -fno-fast-math); divisions and sqrt are the compiler's IEEE ones.
//   BATCH          N views in one launch (rtw_upsample_batch_*): the small planes hold N*w*h slots, view v at slot offset v*w*h; the features
//                  and the result hold the full frames one behind the other.  The lane splits its flat pixel into (view, j, i) and bounds
//                  every tap by its view's own small frame; the arithmetic of a pixel is up_pixel as in the single form.
#pragma once
#include "rtw_denoise.hpp"

namespace rtw {

template <typename T> struct UpParams {
    T inv_sa, inv_sz;       // 1 / sigma_albedo^2 and 1 / sigma_depth^2, computed in binary64 and rounded to T by the host
    int m, mode;            // normal_power_log2; RTW_DN_DEMOD | RTW_DN_GAMMA
    int w, h, W, H;         // the small and the full frame
};
// the batched kernel's first argument: UpParams of ONE view with the batch's full-size pixel count behind it
template <typename T> struct UpParamsBatch { UpParams<T> U; long long n_all; };     // n_all = N * W * H

// One axis of the position in the small frame: pixel centres coincide, so full-size index `c` of `full` lies at (2c + 3) * small - 3 * full
// in units of 1 / (2 * full) behind the small index -2 (exact integers).  -> first tap index - (-1), i.e. x0; `f` = the fraction in [0, 1).
// `narrow`: (2 * full + 2) * full fits 32 bits, so the one division is a 32-bit one.
template <typename T>
__device__ __forceinline__ long long up_axis(long long c, long long small, long long full, bool narrow, T &f) {
    const long long num = (2 * c + 3) * small + full;           // num_x + 4 * full >= 0: the quotient below is floor(num_x / (2 * full)) + 2
    long long k, r;
    if (narrow) {
        const unsigned d = (unsigned)(2 * full), kk = (unsigned)num / d;
        k = kk; r = (unsigned)num - kk * d;
        f = (T)(unsigned)r / (T)d;
    } else {
        k = num / (2 * full); r = num - k * (2 * full);
        f = (T)r / (T)(2 * full);
    }
    return k - 2;
}

// the tent of one axis at tap offset `o` (-1 .. 2): 1 - |o - f| / 2, never negative
template <typename T> __device__ __forceinline__ T up_tent(int o, T f) { return T(1) - dn_abs(T(o) - f) * T(0.5); }

template <typename T> struct UpSum { T w, e0, e1, e2, s, s0, s1, s2; };

// one tap; `ok`: inside the small frame and valid.  The data of a tap that is not ok may be anything: selects, not weights, drop it.
// (aP, nP, zP, covP: the full-size pixel's guides; hasP: it is covered)
template <typename T, typename V>
__device__ __forceinline__ void up_tap(UpSum<T> &a, const V &aP, const V &nP, T zP, T covP, bool hasP, const V &eq, const V &gq, const V &aq, T s, bool ok,
                                       const UpParams<T> &U) {
    const T d0 = aP.x - aq.x, d1 = aP.y - aq.y, d2 = aP.z - aq.z;
    const T dA = (d0 * d0 + d1 * d1) + d2 * d2;
    const T wa = T(1) / (T(1) + dA * U.inv_sa);
    const T tv = T(1) - dn_abs(covP - gq.w);
    const T wv = tv > T(0) ? tv : T(0);
    T w = (s * wa) * wv;
    const T dot = (nP.x * gq.x + nP.y * gq.y) + nP.z * gq.z;
    T t = dot > T(0) ? dot : T(0);
    for (int r = 0; r < U.m; ++r) t = t * t;
    const T zs = zP + eq.w;
    const T rz = (zP - eq.w) / (zs > T(0) ? zs : T(1));
    const T wz = T(1) / (T(1) + (rz * rz) * U.inv_sz);
    const T wg = (w * t) * wz;
    w = (hasP && gq.w > T(0)) ? wg : w;                 // has(P) && has(q)  (cov_q = NaN: not valid, so not has)
    a.w = a.w + (ok ? w : T(0));
    a.e0 = a.e0 + (ok ? w * eq.x : T(0));
    a.e1 = a.e1 + (ok ? w * eq.y : T(0));
    a.e2 = a.e2 + (ok ? w * eq.z : T(0));
    a.s = a.s + (ok ? s : T(0));
    a.s0 = a.s0 + (ok ? s * eq.x : T(0));
    a.s1 = a.s1 + (ok ? s * eq.y : T(0));
    a.s2 = a.s2 + (ok ? s * eq.z : T(0));
}

// Full-size pixel (i, j), slot P of the features and of the result; `lo`: the first slot of its view's small frame in the planes.
template <typename T, typename V>
__device__ __forceinline__ void up_pixel(const UpParams<T> &U, long long i, long long j, long long P, long long lo, bool narrow, const V *__restrict__ E,
                                         const V *__restrict__ G, const V *__restrict__ A, const V *__restrict__ feat, T *__restrict__ out) {
    const long long h = U.h, w = U.w;
    const V f0 = feat[P * 2 + 0], f1 = feat[P * 2 + 1];        // albedo, n.x | n.y, n.z, depth, coverage
    const bool validP = dn_finite(f0.x) && dn_finite(f0.y) && dn_finite(f0.z) && dn_finite(f0.w) && dn_finite(f1.x) && dn_finite(f1.y) && dn_finite(f1.z) &&
                        dn_finite(f1.w);
    const T covP = f1.w;
    const bool hasP = validP && covP > T(0);
    const T dv = hasP ? covP : T(1);
    V nP, aP;
    nP.x = hasP ? f0.w / dv : T(0); nP.y = hasP ? f1.x / dv : T(0); nP.z = hasP ? f1.y / dv : T(0); nP.w = T(0);
    const T zP = hasP ? f1.z / dv : T(0);
    aP.x = aP.y = aP.z = T(1); aP.w = T(0);
    if (U.mode & RTW_DN_DEMOD) {
        const T floor_ = T(0.015625);               // 2^-6
        aP.x = f0.x > floor_ ? f0.x : floor_; aP.y = f0.y > floor_ ? f0.y : floor_; aP.z = f0.z > floor_ ? f0.z : floor_;
    }
    T fx, fy;
    const long long x0 = up_axis<T>(j, w, U.W, narrow, fx), y0 = up_axis<T>(i, h, U.H, narrow, fy);
    UpSum<T> a = {T(0), T(0), T(0), T(0), T(0), T(0), T(0), T(0)};
    // one column of taps -- 12 loads -- in flight per trip: unrolling the columns too keeps all 48 loads' registers live (Float32: 168
    // VGPRs instead of 80, 3 waves per SIMD instead of 6; Float64: 256 + 68 instead of 148, 1 wave instead of 3)
#ifdef RTW_UP_UNROLL_COLUMNS         // (A/B builds only: make EXTRA=-DRTW_UP_UNROLL_COLUMNS)
#pragma unroll
#else
#pragma unroll 1
#endif
    for (int b = -1; b <= 2; ++b) {
        const T kx = up_tent<T>(b, fx);
#pragma unroll
        for (int c = -1; c <= 2; ++c) {
            const T ky = up_tent<T>(c, fy);
            const long long qi = y0 + c, qj = x0 + b;
            const bool in = qi >= 0 && qi < h && qj >= 0 && qj < w;
            const long long q = lo + (in ? qj * h + qi : 0);
            const V eq = E[q], gq = G[q], aq = A[q];
            up_tap<T>(a, aP, nP, zP, covP, hasP, eq, gq, aq, ky * kx, in && gq.w == gq.w, U);
        }
    }
    // guided sums if any guide let a tap through, else the purely spatial ones, else the pixel is not valid
    const bool guided = a.w > T(0);
    const T den = guided ? a.w : a.s;
    T e0 = (guided ? a.e0 : a.s0) / den, e1 = (guided ? a.e1 : a.s1) / den, e2 = (guided ? a.e2 : a.s2) / den;
    if (U.mode & RTW_DN_DEMOD) { e0 = e0 * aP.x; e1 = e1 * aP.y; e2 = e2 * aP.z; }
    if (U.mode & RTW_DN_GAMMA) { e0 = dn_sqrt(e0); e1 = dn_sqrt(e1); e2 = dn_sqrt(e2); }
    const bool valid = validP && den > T(0);
    out[P * 3 + 0] = valid ? e0 : dn_nan<T>();
    out[P * 3 + 1] = valid ? e1 : dn_nan<T>();
    out[P * 3 + 2] = valid ? e2 : dn_nan<T>();
}

// the divisions of up_axis are 32-bit ones when (2 * full + 2) * full < 2^32 on both axes
__device__ __forceinline__ bool up_narrow(long long W, long long H) { return W <= 32768 && H <= 32768; }

// lane = flat full-size pixel P = (view * W + j) * H + i; BATCH = false: one view
template <typename T, bool BATCH>
__global__ __launch_bounds__(256) void up_sample(UpParamsBatch<T> B, const typename DnVec<T>::type *__restrict__ E, const typename DnVec<T>::type *__restrict__ G,
                                                 const typename DnVec<T>::type *__restrict__ A, const typename DnVec<T>::type *__restrict__ feat, T *__restrict__ out) {
    const UpParams<T> &U = B.U;
    const long long H = U.H, W = U.W, WH = W * H;
    const long long P = (long long)blockIdx.x * 256 + threadIdx.x;
    if (P >= B.n_all) return;
    // (32-bit divisions whenever the launch allows it)
    long long lo = 0, j, i;
    if (B.n_all < (1ll << 31)) {
        unsigned r = (unsigned)P;
        if constexpr (BATCH) { const unsigned v = r / (unsigned)WH; r -= v * (unsigned)WH; lo = (long long)v * U.w * U.h; }
        const unsigned jj = r / (unsigned)H;
        j = jj; i = r - jj * (unsigned)H;
    } else {
        long long r = P;
        if constexpr (BATCH) { const long long v = r / WH; r -= v * WH; lo = v * U.w * U.h; }
        j = r / H; i = r - j * H;
    }
    up_pixel<T>(U, i, j, P, lo, up_narrow(W, H), E, G, A, feat, out);
}

}  // namespace rtw
