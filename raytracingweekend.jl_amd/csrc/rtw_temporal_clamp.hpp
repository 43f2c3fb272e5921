// rtw_temporal_clamp.hpp -- the kernel of the clamped temporal step (include/rtw_hip.h rtw_clamped_step_*: the definition is there): tp_step's
// step with the reprojected history clamped to mean +- ks*sd of the CURRENT frame's (2r+1)^2 window before the blend.
//   tp_step_clamped  a workgroup of 256 lanes owns a tile of TP_TI = 32 rows x TP_TJ = 8 columns of the frame, lanes along i (lane = tj*32 + ti: a
//                    wave is two columns of 32 rows).  It stages the PREPARED pixels of the tile and its halo of r -- (32+2r) x (8+2r) of them,
//                    column after column like the frame itself -- into LDS once: two planes of V slots, E = (e0, e1, e2, z) and G = (n, cov;
//                    cov = NaN: not valid), the very slots tp_step stores into the next state.  Every staged pixel pays dn_prepare's arithmetic
//                    once (up to 7 IEEE quotients); a halo pixel outside the frame is marked not valid without a global load.  After the one
//                    barrier a lane takes its own pixel and the window's taps from LDS (lanes along i read consecutive 16- or 32-byte slots),
//                    forms the bounds, and goes on as tp_step does: its ray, the projection, the 2 x 2 taps of the previous state from global
//                    memory through tp_tap, the clamp, the blend, the stores.
//   MOMENTS          as in tp_step: the moment plane is gathered, blended with the alpha that results, and stored; it is not clamped.
//   GUIDES           RTW_CLAMP_GUIDES: the window's taps carry tp_tap's weight (sb = 1, zexp = z_p) on the current frame's guides; without it
//                    every tap weighs 1 and no product by w is formed.  (G is staged in both instances: a lane's own guides come from it.)
// There is no HAS_PREV = false form: the first frame is tp_step<T, false, MOMENTS>.  Lanes of a tail tile whose own pixel lies outside the frame
// stage and reach the barrier like any other lane and leave behind it.  The window's trip count is the radius', uniform; a tap that takes no
// part is dropped by selects.  LDS: 2 * 38 * 14 slots, 17024 bytes (Float32) / 34048 bytes (Float64), sized for r = 3 whatever r is.
#pragma once
#include "rtw_temporal.hpp"

namespace rtw {

constexpr int TP_TI = 32, TP_TJ = 8, TP_RMAX = 3;
constexpr int TP_SLOTS = (TP_TI + 2 * TP_RMAX) * (TP_TJ + 2 * TP_RMAX);

// what the host derives from rtw_temporal_clamp_t, by value, next to the step's own TpParams
template <typename T> struct TpClampParams {
    T ks, ls;                           // sigma, len_scale (binary64, rounded to T)
    int r;                              // radius
    unsigned tiles_i;                   // tiles along i: ceil(H / TP_TI)
};

// block = tile (tile column tJ, tile row tI) = blockIdx.x / tiles_i, blockIdx.x % tiles_i; lane = (tj, ti) = threadIdx.x / 32, threadIdx.x % 32
// PATHS (rtw_temporal.hpp TpPaths): blockIdx.x numbers the tiles of ONE path; the path comes from blockIdx.y / .z, so a whole workgroup leaves
// together before the barrier when its path index is past the last one.
// MOTION (rtw_temporal.hpp TpTail; never with PATHS): the pixel's slot of the motion plane is subtracted from its world point, as in tp_step.
template <typename T, bool MOMENTS, bool GUIDES, bool PATHS = false, bool MOTION = false>
__global__ __launch_bounds__(256) void tp_step_clamped(TpParams<T> U, TpClampParams<T> C, const T *__restrict__ image, const typename DnVec<T>::type *__restrict__ feat,
                                                       const typename DnVec<T>::type *__restrict__ Ep, const typename DnVec<T>::type *__restrict__ Gp, const T *__restrict__ Lp,
                                                       typename DnVec<T>::type *__restrict__ En, typename DnVec<T>::type *__restrict__ Gn, T *__restrict__ Ln, T *__restrict__ out,
                                                       const T *__restrict__ Mp, T *__restrict__ Mn, [[maybe_unused]] TpTail<T, PATHS, MOTION> B) {
    using V = typename DnVec<T>::type;
    static_assert(!(MOTION && PATHS), "the motion plane belongs to a single path's step");
    __shared__ V sE[TP_SLOTS], sG[TP_SLOTS];
    if constexpr (PATHS) {
        const long long s = (long long)blockIdx.z * gridDim.y + blockIdx.y;
        if (s >= B.n_paths) return;
        const long long fr = (long long)U.W * U.H * (long long)sizeof(T);         // bytes of one plane of one element per pixel
        image = tp_adv(image, s * fr * 3); out = tp_adv(out, s * fr * 3); feat = tp_adv(feat, s * fr * 8);
        Ep = tp_adv(Ep, s * B.st_stride); Gp = tp_adv(Gp, s * B.st_stride); Lp = tp_adv(Lp, s * B.st_stride);
        En = tp_adv(En, s * B.st_stride); Gn = tp_adv(Gn, s * B.st_stride); Ln = tp_adv(Ln, s * B.st_stride);
        if constexpr (MOMENTS) { Mp = tp_adv(Mp, s * B.mo_stride); Mn = tp_adv(Mn, s * B.mo_stride); }
        tp_load_cameras(U, B.table + s * 32);
    }
    const long long H = U.H, W = U.W;
    const int r = C.r, SI = TP_TI + 2 * r, n_stage = SI * (TP_TJ + 2 * r);
    const unsigned tJ = blockIdx.x / C.tiles_i, tI = blockIdx.x - tJ * C.tiles_i;
    const long long i0 = (long long)tI * TP_TI, j0 = (long long)tJ * TP_TJ;
    const bool demod = (U.mode & RTW_DN_DEMOD) != 0;
    const T floor_ = T(0.015625);                       // 2^-6
    // ---- stage: dn_prepare's arithmetic on every pixel of the tile and its halo, once
    for (int s = threadIdx.x; s < n_stage; s += 256) {
        const int sj = s / SI, si = s - sj * SI;
        const long long qi = i0 - r + si, qj = j0 - r + sj;
        V e, g;
        e.x = T(0); e.y = T(0); e.z = T(0); e.w = T(0);
        g.x = T(0); g.y = T(0); g.z = T(0); g.w = dn_nan<T>();
        if (qi >= 0 && qi < H && qj >= 0 && qj < W) {
            const long long q = qj * H + qi;
            const T c0 = image[q * 3 + 0], c1 = image[q * 3 + 1], c2 = image[q * 3 + 2];
            const V f0 = feat[q * 2 + 0], f1 = feat[q * 2 + 1];        // albedo, n.x | n.y, n.z, depth, coverage
            const bool valid = dn_finite(c0) && dn_finite(c1) && dn_finite(c2) && dn_finite(f0.x) && dn_finite(f0.y) && dn_finite(f0.z) && dn_finite(f0.w) &&
                               dn_finite(f1.x) && dn_finite(f1.y) && dn_finite(f1.z) && dn_finite(f1.w);
            const T cov = f1.w;
            const bool has = valid && cov > T(0);
            const T dv = has ? cov : T(1);
            const T nx = f0.w / dv, ny = f1.x / dv, nz = f1.y / dv, zq = f1.z / dv;
            g.x = has ? nx : T(0); g.y = has ? ny : T(0); g.z = has ? nz : T(0); g.w = valid ? cov : dn_nan<T>();
            T e0 = c0, e1 = c1, e2 = c2;
            if (demod) {
                const T a0 = f0.x > floor_ ? f0.x : floor_, a1 = f0.y > floor_ ? f0.y : floor_, a2 = f0.z > floor_ ? f0.z : floor_;
                e0 = c0 / a0; e1 = c1 / a1; e2 = c2 / a2;
            }
            e.x = e0; e.y = e1; e.z = e2; e.w = has ? zq : T(0);
        }
        sE[s] = e; sG[s] = g;
    }
    __syncthreads();
    const int tj = threadIdx.x >> 5, ti = threadIdx.x & 31;
    const long long i = i0 + ti, j = j0 + tj;
    if (i >= H || j >= W) return;                       // (a tail tile's lanes outside the frame: behind the only barrier)
    const long long P = j * H + i;
    const int sc = (tj + r) * SI + (ti + r);            // the pixel's own slot
    const V ec = sE[sc];
    V g = sG[sc];
    const bool valid = g.w == g.w;
    const T cov = g.w;
    const bool has = valid && cov > T(0);
    const T z = ec.w;
    const T e0 = ec.x, e1 = ec.y, e2 = ec.z;
    T a0 = T(1), a1 = T(1), a2 = T(1);
    if (demod) {
        const V f0 = feat[P * 2 + 0];                   // (the albedo again: the end multiplies it back)
        a0 = f0.x > floor_ ? f0.x : floor_; a1 = f0.y > floor_ ? f0.y : floor_; a2 = f0.z > floor_ ? f0.z : floor_;
    }
    [[maybe_unused]] T y2 = T(0), mom = T(0);
    if constexpr (MOMENTS) {
        const T y = (e0 + e1) + e2;
        y2 = y * y; mom = y2;
    }
    // ---- the window of the current frame, from LDS: dj outer, di inner
    TpSum<T> S = {T(0), T(0), T(0), T(0), T(0)};        // (S.w = S0; S.e0..2 = S1)
    T q0 = T(0), q1 = T(0), q2 = T(0);                  // S2
    for (int dj = -r; dj <= r; ++dj) {
        for (int di = -r; di <= r; ++di) {
            const int sq = sc + dj * SI + di;
            const V eq = sE[sq], gq = sG[sq];
            const bool ok = gq.w == gq.w;               // (outside the frame: staged as not valid)
            if constexpr (GUIDES) {
                const T w = tp_tap<T>(S, g, has, z, eq, gq, T(0), T(1), ok, U);
                q0 = q0 + (ok ? w * (eq.x * eq.x) : T(0));
                q1 = q1 + (ok ? w * (eq.y * eq.y) : T(0));
                q2 = q2 + (ok ? w * (eq.z * eq.z) : T(0));
            } else {
                S.w = S.w + (ok ? T(1) : T(0));
                S.e0 = S.e0 + (ok ? eq.x : T(0)); S.e1 = S.e1 + (ok ? eq.y : T(0)); S.e2 = S.e2 + (ok ? eq.z : T(0));
                q0 = q0 + (ok ? eq.x * eq.x : T(0)); q1 = q1 + (ok ? eq.y * eq.y : T(0)); q2 = q2 + (ok ? eq.z * eq.z : T(0));
            }
        }
    }
    const T mu0 = S.e0 / S.w, mu1 = S.e1 / S.w, mu2 = S.e2 / S.w;
    const T vt0 = q0 / S.w - mu0 * mu0, vt1 = q1 / S.w - mu1 * mu1, vt2 = q2 / S.w - mu2 * mu2;
    const T sd0 = dn_sqrt(vt0 > T(0) ? vt0 : T(0)), sd1 = dn_sqrt(vt1 > T(0) ? vt1 : T(0)), sd2 = dn_sqrt(vt2 > T(0) ? vt2 : T(0));
    const T d0_ = C.ks * sd0, d1_ = C.ks * sd1, d2_ = C.ks * sd2;
    const T lo0 = mu0 - d0_, lo1 = mu1 - d1_, lo2 = mu2 - d2_;
    const T hi0 = mu0 + d0_, hi1 = mu1 + d1_, hi2 = mu2 + d2_;
    // ---- the pixel's own ray in the current camera, the point to reproject, the projection: tp_step's
#include "rtw_temporal_project.inc"
    const bool inr = x > T(-1) && x < T((int)W) && y > T(-1) && y < T((int)H);       // (a NaN fails)
    const T xs = inr ? x : T(0), ys = inr ? y : T(0);
    const T xf = tp_floor(xs), yf = tp_floor(ys);
    const long long x0 = (int)xf, y0 = (int)yf;             // -1 .. W-1, -1 .. H-1
    const T fx = xs - xf, fy = ys - yf;
    const T zexp = dn_sqrt((d0 * d0 + d1 * d1) + d2 * d2);
    // ---- the taps of the previous state, from global memory
    TpSum<T> a = {T(0), T(0), T(0), T(0), T(0)};
    [[maybe_unused]] T sum_m = T(0);
#pragma unroll
    for (int b = 0; b <= 1; ++b) {
        const T kx = b ? fx : T(1) - fx;
#pragma unroll
        for (int c = 0; c <= 1; ++c) {
            const T ky = c ? fy : T(1) - fy;
            const long long qi = y0 + c, qj = x0 + b;
            const bool in = qi >= 0 && qi < H && qj >= 0 && qj < W;
            const long long q = in ? qj * H + qi : P;
            const V eq = Ep[q], gq = Gp[q];
            const T lq = Lp[q];
            const bool ok = in && gq.w == gq.w;
            const T w = tp_tap<T>(a, g, has, zexp, eq, gq, lq, ky * kx, ok, U);
            if constexpr (MOMENTS) {
                const T mq = Mp[q];
                sum_m = sum_m + (ok ? w * mq : T(0));
            }
        }
    }
    // ---- clamp (a NaN bound fails both comparisons), then tp_step's blend with hc and lh' in place of eh and lh
    const bool accept = front && inr && a.w >= U.w_min;      // (a NaN sum fails)
    const T h0 = a.e0 / a.w, h1 = a.e1 / a.w, h2 = a.e2 / a.w, lh = a.l / a.w;
    const T c0 = h0 < lo0 ? lo0 : (h0 > hi0 ? hi0 : h0);
    const T c1 = h1 < lo1 ? lo1 : (h1 > hi1 ? hi1 : h1);
    const T c2 = h2 < lo2 ? lo2 : (h2 > hi2 ? hi2 : h2);
    const bool moved = c0 != h0 || c1 != h1 || c2 != h2;
    const T lc = moved ? lh * C.ls : lh;
    const T l1 = lc + T(1);
    const T nn = l1 < U.n_max ? l1 : U.n_max;
    const T alpha = T(1) / nn;
    const T b0 = c0 + alpha * (e0 - c0), b1 = c1 + alpha * (e1 - c1), b2 = c2 + alpha * (e2 - c2);
    const T r0 = accept ? b0 : e0, r1 = accept ? b1 : e1, r2 = accept ? b2 : e2;
    const T len = accept ? nn : T(1);
    if constexpr (MOMENTS) {
        const T mh = sum_m / a.w;
        const T mb = mh + alpha * (y2 - mh);
        mom = accept ? mb : y2;
    }
    // ---- end: the image and the next state
    T o0 = r0, o1 = r1, o2 = r2;
    if (demod) { o0 = r0 * a0; o1 = r1 * a1; o2 = r2 * a2; }
    if (U.mode & RTW_DN_GAMMA) { o0 = dn_sqrt(o0); o1 = dn_sqrt(o1); o2 = dn_sqrt(o2); }
    out[P * 3 + 0] = valid ? o0 : dn_nan<T>();
    out[P * 3 + 1] = valid ? o1 : dn_nan<T>();
    out[P * 3 + 2] = valid ? o2 : dn_nan<T>();
    V en;
    en.x = valid ? r0 : T(0); en.y = valid ? r1 : T(0); en.z = valid ? r2 : T(0); en.w = z;
    En[P] = en; Gn[P] = g;
    Ln[P] = valid ? len : T(0);
    if constexpr (MOMENTS) Mn[P] = valid ? mom : T(0);
}

}  // namespace rtw
