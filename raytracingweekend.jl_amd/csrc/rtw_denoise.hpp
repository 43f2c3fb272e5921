// rtw_denoise.hpp -- the kernels of the feature-guided denoiser (include/rtw_hip.h rtw_denoise_*: an edge-avoiding a-trous filter, the
// definition is there): prepare, and the level kernel.
//   prepare        one pixel per lane: validity, the guides n = f[3..5] / cov, z = f[6] / cov, the (de)modulated colour e = c / a.  Three planes of
//                  4-element slots (16 bytes in Float32, 32 in Float64), pixel p at slot p:  E = (e0, e1, e2, z)   G = (n.x, n.y, n.z, cov)
//                  A = (a0, a1, a2, 0).  A pixel that is not valid has cov = NaN in G (a valid pixel's cov is finite): never a neighbour.
//   level          one pixel per lane, lanes along i, the 24 neighbours read from global memory (L1 / L2)
// The colour plane ping-pongs between two E planes; the last level multiplies the albedo back, applies gamma and the NaN rule and writes the
// image.  No atomics, no cross-lane operation; the trip count over the taps is uniform, skipped taps are predicated by selects.
// Every operation is rounded once (the Makefile's -ffp-contract=off -fno-fast-math); divisions and sqrt are the compiler's IEEE ones.
//   GUIDED         the noise-guided form (include/rtw_hip.h rtw_guided_filter_device_*): prepare also reads the caller's noise map, treats a
//                  pixel whose entry is not finite as not valid and stores the pixel's colour variance v in A.w (the slot the plain form
//                  leaves 0); the level kernel divides a tap's colour distance by the CENTRE pixel's v.  Nothing else differs, and the
//                  instances with GUIDED = false are the plain form's code.
//   BATCH          N frames of one size in each launch (include/rtw_hip.h rtw_filter_batch_*, rtw_guided_filter_batch_device_*): every plane holds N*W*H slots,
//                  view v at slot offset v*W*H; the image and the result at v*W*H*3 elements, the features at v*W*H*2 vectors.  Prepare
//                  looks at its own pixel only, so the batch runs the plain prepare over N*W*H pixels; the level kernel's batched twin, dn_level_batch,
//                  splits its flat pixel into (view, j, i) and bounds every tap by the view's own frame -- the arithmetic of a pixel is
//                  dn_tap / dn_centre / dn_store as everywhere.  GUIDED: the noise map holds N*W*H elements, view v at v*W*H; the centre pixel's
//                  variance is A[p].w as in dn_level<T, true>; the instance with GUIDED = false is the plain batched form's code.
#pragma once
#include <hip/hip_runtime.h>

namespace rtw {

template <typename T> struct DnVec;
template <> struct DnVec<float> { using type = float4; };
// (not double4: its natural alignment is 32 bytes, and the contract of the buffers and of the workspace is 16)
struct alignas(16) DnDouble4 { double x, y, z, w; };
template <> struct DnVec<double> { using type = DnDouble4; };

#define RTW_DN_FINAL 1      // DnLevel::mode: the last level (writes the image)
#define RTW_DN_DEMOD 2      //   ... multiplies the albedo back
#define RTW_DN_GAMMA 4      //   ... sqrt per channel

template <typename T> struct DnLevel {
    T inv_sc, inv_sz;       // 1 / (sigma_color 2^-k)^2 and 1 / sigma_depth^2, computed in binary64 and rounded to T by the host
    int step, m, mode;      // 2^k; normal_power_log2; RTW_DN_*
    int W, H;
};

__device__ __forceinline__ float dn_abs(float x) { return __builtin_fabsf(x); }
__device__ __forceinline__ double dn_abs(double x) { return __builtin_fabs(x); }
__device__ __forceinline__ float dn_sqrt(float x) { return __builtin_sqrtf(x); }
__device__ __forceinline__ double dn_sqrt(double x) { return __builtin_sqrt(x); }
template <typename T> __device__ __forceinline__ T dn_nan() { return (T)__builtin_nanf(""); }
template <typename T> __device__ __forceinline__ bool dn_finite(T x) { return dn_abs(x) < (T)__builtin_inff(); }   // (false for NaN)

template <typename T> struct DnSum { T w, e0, e1, e2; };

// the bounds of the guided form's variance: powers of two (the clamps and a division by them are exact), normal numbers in binary32
#define RTW_DN_V_MIN 0x1p-40
#define RTW_DN_V_MAX 0x1p40

// one tap that is not the centre; `ok`: inside the frame and valid.  The data of a tap that is not ok may be anything: selects, not weights, drop it.
// GUIDED: `vp` is the centre pixel's variance (RTW_DN_V_MIN <= vp <= RTW_DN_V_MAX), the colour distance is measured in units of it.
template <typename T, bool GUIDED, typename V>
__device__ __forceinline__ void dn_tap(DnSum<T> &a, const V &ep, const V &gp, const V &eq, const V &gq, T h, bool ok, const DnLevel<T> &L, [[maybe_unused]] T vp) {
    const T d0 = ep.x - eq.x, d1 = ep.y - eq.y, d2 = ep.z - eq.z;
    T dc = (d0 * d0 + d1 * d1) + d2 * d2;
    if constexpr (GUIDED) dc = dc / vp;
    const T wc = T(1) / (T(1) + dc * L.inv_sc);
    const T tv = T(1) - dn_abs(gp.w - gq.w);
    const T wv = tv > T(0) ? tv : T(0);
    T w = (h * wc) * wv;
    const T dot = (gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z;
    T t = dot > T(0) ? dot : T(0);
    for (int r = 0; r < L.m; ++r) t = t * t;
    const T zs = ep.w + eq.w;
    const T rz = (ep.w - eq.w) / (zs > T(0) ? zs : T(1));
    const T wz = T(1) / (T(1) + (rz * rz) * L.inv_sz);
    const T wg = (w * t) * wz;
    w = (gp.w > T(0) && gq.w > T(0)) ? wg : w;         // has(p) && has(q)  (cov = NaN: not valid, so not has)
    a.w = a.w + (ok ? w : T(0));
    a.e0 = a.e0 + (ok ? w * eq.x : T(0));
    a.e1 = a.e1 + (ok ? w * eq.y : T(0));
    a.e2 = a.e2 + (ok ? w * eq.z : T(0));
}
template <typename T, typename V>
__device__ __forceinline__ void dn_centre(DnSum<T> &a, const V &ep) {
    const T h = T(9) / T(64);
    a.w = a.w + h;
    a.e0 = a.e0 + h * ep.x; a.e1 = a.e1 + h * ep.y; a.e2 = a.e2 + h * ep.z;
}
__device__ constexpr double dn_k(int d) { return d == 0 ? 0.375 : (d == 1 || d == -1) ? 0.25 : 0.0625; }

// after the 25 taps: the quotients, and either the next level's colour slot or the image's pixel
template <typename T, typename V>
__device__ __forceinline__ void dn_store(const DnSum<T> &a, const V &ep, const V &gp, long long p, const DnLevel<T> &L, const V *__restrict__ A, V *__restrict__ Eout, T *__restrict__ out) {
    T e0 = a.e0 / a.w, e1 = a.e1 / a.w, e2 = a.e2 / a.w;
    if (!(L.mode & RTW_DN_FINAL)) {
        V o; o.x = e0; o.y = e1; o.z = e2; o.w = ep.w;
        Eout[p] = o;
        return;
    }
    if (L.mode & RTW_DN_DEMOD) { const V al = A[p]; e0 = e0 * al.x; e1 = e1 * al.y; e2 = e2 * al.z; }
    if (L.mode & RTW_DN_GAMMA) { e0 = dn_sqrt(e0); e1 = dn_sqrt(e1); e2 = dn_sqrt(e2); }
    const bool valid = gp.w == gp.w;
    out[p * 3 + 0] = valid ? e0 : dn_nan<T>();
    out[p * 3 + 1] = valid ? e1 : dn_nan<T>();
    out[p * 3 + 2] = valid ? e2 : dn_nan<T>();
}

template <typename T, bool GUIDED = false>
__global__ __launch_bounds__(256) void dn_prepare(const T *__restrict__ image, const typename DnVec<T>::type *__restrict__ feat, typename DnVec<T>::type *__restrict__ E,
                                                  typename DnVec<T>::type *__restrict__ G, typename DnVec<T>::type *__restrict__ A, long long n_pix, int demod,
                                                  [[maybe_unused]] const T *__restrict__ noise) {
    using V = typename DnVec<T>::type;
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pix) return;
    const T c0 = image[p * 3 + 0], c1 = image[p * 3 + 1], c2 = image[p * 3 + 2];
    const V f0 = feat[p * 2 + 0], f1 = feat[p * 2 + 1];        // albedo, n.x | n.y, n.z, depth, coverage
    bool valid = dn_finite(c0) && dn_finite(c1) && dn_finite(c2) && dn_finite(f0.x) && dn_finite(f0.y) && dn_finite(f0.z) && dn_finite(f0.w) &&
                 dn_finite(f1.x) && dn_finite(f1.y) && dn_finite(f1.z) && dn_finite(f1.w);
    [[maybe_unused]] T rho = T(0);
    if constexpr (GUIDED) { rho = noise[p]; valid = valid && dn_finite(rho); }
    const T cov = f1.w;
    const bool has = valid && cov > T(0);
    const T dv = has ? cov : T(1);
    const T nx = f0.w / dv, ny = f1.x / dv, nz = f1.y / dv, z = f1.z / dv;
    V e, g, a;
    a.x = a.y = a.z = T(1); a.w = T(0);
    if (demod) {
        const T floor_ = T(0.015625);               // 2^-6
        a.x = f0.x > floor_ ? f0.x : floor_; a.y = f0.y > floor_ ? f0.y : floor_; a.z = f0.z > floor_ ? f0.z : floor_;
        e.x = c0 / a.x; e.y = c1 / a.y; e.z = c2 / a.z;
    } else {
        e.x = c0; e.y = c1; e.z = c2;
    }
    e.w = has ? z : T(0);
    g.x = has ? nx : T(0); g.y = has ? ny : T(0); g.z = has ? nz : T(0);
    g.w = valid ? cov : dn_nan<T>();
    if constexpr (GUIDED) {
        // the pixel's own standard deviation estimate: the relative noise times its (demodulated) brightness, floored like the albedo
        const T floor_ = T(0.015625);
        const T L = (e.x + e.y) + e.z;
        const T s = rho * (L > floor_ ? L : floor_);
        T v = s * s;
        v = v > T(RTW_DN_V_MIN) ? v : T(RTW_DN_V_MIN);
        v = v < T(RTW_DN_V_MAX) ? v : T(RTW_DN_V_MAX);
        a.w = valid ? v : T(1);
    }
    if (!valid) { e.x = e.y = e.z = T(0); a.x = a.y = a.z = T(1); }
    E[p] = e; G[p] = g; A[p] = a;
}

// the batched level kernel's first argument: DnLevel of ONE frame with the batch's pixel count behind it
template <typename T> struct DnLevelBatch { DnLevel<T> L; long long n_all; };       // n_all = N * W * H

template <typename T, bool GUIDED = false>
__global__ __launch_bounds__(256) void dn_level(DnLevel<T> L, const typename DnVec<T>::type *__restrict__ Ein, const typename DnVec<T>::type *__restrict__ G,
                                                       const typename DnVec<T>::type *__restrict__ A, typename DnVec<T>::type *__restrict__ Eout, T *__restrict__ out) {
    using V = typename DnVec<T>::type;
    const long long H = L.H, W = L.W, s = L.step;
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= W * H) return;
    // (a 32-bit division whenever the frame allows it)
    const long long j = W * H < (1ll << 31) ? (long long)((unsigned)p / (unsigned)H) : p / H, i = p - j * H;
    const V ep = Ein[p], gp = G[p];
    [[maybe_unused]] T vp = T(1);
    if constexpr (GUIDED) vp = A[p].w;
    DnSum<T> a = {T(0), T(0), T(0), T(0)};
#pragma unroll
    for (int dj = -2; dj <= 2; ++dj) {
#pragma unroll
        for (int di = -2; di <= 2; ++di) {
            if (di == 0 && dj == 0) { dn_centre<T>(a, ep); continue; }
            const long long qi = i + s * di, qj = j + s * dj;
            const bool in = qi >= 0 && qi < H && qj >= 0 && qj < W;
            const long long q = in ? qj * H + qi : p;
            const V eq = Ein[q], gq = G[q];
            dn_tap<T, GUIDED>(a, ep, gp, eq, gq, (T)(dn_k(di) * dn_k(dj)), in && gq.w == gq.w, L, vp);
        }
    }
    dn_store<T>(a, ep, gp, p, L, A, Eout, out);
}

// BATCH: lane = flat pixel p of the batch = view * W*H + j*H + i; `base` is the view's first slot, every tap stays in [base, base + W*H)
template <typename T, bool GUIDED = false>
__global__ __launch_bounds__(256) void dn_level_batch(DnLevelBatch<T> B, const typename DnVec<T>::type *__restrict__ Ein, const typename DnVec<T>::type *__restrict__ G,
                                                             const typename DnVec<T>::type *__restrict__ A, typename DnVec<T>::type *__restrict__ Eout, T *__restrict__ out) {
    using V = typename DnVec<T>::type;
    const DnLevel<T> &L = B.L;
    const long long H = L.H, W = L.W, s = L.step, WH = W * H;
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= B.n_all) return;
    // (32-bit divisions whenever the batch allows it)
    long long base, j, i;
    if (B.n_all < (1ll << 31)) {
        const unsigned v = (unsigned)p / (unsigned)WH, r = (unsigned)p - v * (unsigned)WH, jj = r / (unsigned)H;
        base = (long long)v * WH; j = jj; i = r - jj * (unsigned)H;
    } else {
        const long long v = p / WH, r = p - v * WH;
        base = v * WH; j = r / H; i = r - j * H;
    }
    const V ep = Ein[p], gp = G[p];
    [[maybe_unused]] T vp = T(1);
    if constexpr (GUIDED) vp = A[p].w;
    DnSum<T> a = {T(0), T(0), T(0), T(0)};
#pragma unroll
    for (int dj = -2; dj <= 2; ++dj) {
#pragma unroll
        for (int di = -2; di <= 2; ++di) {
            if (di == 0 && dj == 0) { dn_centre<T>(a, ep); continue; }
            const long long qi = i + s * di, qj = j + s * dj;
            const bool in = qi >= 0 && qi < H && qj >= 0 && qj < W;
            const long long q = in ? base + qj * H + qi : p;
            const V eq = Ein[q], gq = G[q];
            dn_tap<T, GUIDED>(a, ep, gp, eq, gq, (T)(dn_k(di) * dn_k(dj)), in && gq.w == gq.w, L, vp);
        }
    }
    dn_store<T>(a, ep, gp, p, L, A, Eout, out);
}

}  // namespace rtw
