// rtw_temporal.hpp -- the kernel of the temporal reprojection (include/rtw_hip.h rtw_temporal_*: the definition is there): one step of history
// reuse along a camera path.
//   tp_step        one pixel per lane, lanes along i.  The pixel is prepared inline exactly as dn_prepare prepares it (validity, n, z, cov, the
//                  (de)modulated colour e); its own ray in the current camera gives the world point (or, for a sky pixel, the direction) that is
//                  projected into the PREVIOUS camera; the 2 x 2 taps around that position gather one E slot, one G slot and one L element each
//                  from the previous state in global memory (L1 / L2); the blend and the next state follow.  State planes, pixel p at slot p:
//                  E = (e0, e1, e2, z)   G = (n.x, n.y, n.z, cov; cov = NaN: not valid)   L = len.
//   HAS_PREV       false: the first frame -- no camera, no state, every pixel resets; the instance reads neither.
//   MOMENTS        true (rtw_history_moments_*): the step also carries the moment plane M, one element per pixel at slot p -- the running second
//                  moment of the pixel's (de)modulated luminance: one more element gathered per tap, one more stored.  The image and the three
//                  state planes are those of the MOMENTS = false instance on the bits; that instance never looks at the two moment pointers.
//   tp_noise       the per-pixel relative-noise map (rtw_history_noise_device_*) from a state and its moment plane: one pixel per lane, lanes along
//                  i.  A pixel whose history is at least min_len long divides its temporal variance M - Lm^2 by len; any other pixel estimates
//                  the variance over its (2r+1)^2 window under tp_tap's weights (sb = 1, zexp = z_p), taps from global memory: the E and the G
//                  slot, one element of M (Lm_q comes from the E slot) -- two 16-byte slots and one element per tap; len is the centre's alone.
//   PATHS          true (rtw_reproject_*_batch_device_*): n_paths paths in one launch, TpPaths below; false: the instance is the single form's,
//                  instruction for instruction (the flag only adds code under `if constexpr`).
//   MOTION         true (rtw_animated_step_device_*, HAS_PREV instances only, never with PATHS): the scene moved between the two frames -- the
//                  pixel's slot of the motion plane (rtw_first_hit_motion_device_*: (m.x, m.y, m.z, id), one 16- or 32-byte load) is
//                  subtracted from its world point before the previous origin is; false: the instance is the static step's, instruction
//                  for instruction.
// (The pixel's own ray, the point to reproject and its projection are the text of rtw_temporal_project.inc, which tp_step_clamped and the motion
// blur's velocity kernel include too: one copy of that arithmetic, and the instances keep their instructions.)
// No LDS, no atomics, no cross-lane operation; the trip count over the 4 taps is uniform, skipped taps are dropped by selects, as in dn_tap.
// (tp_noise: lanes with a long history skip the window by a branch of their own; the window's trip count is the radius', uniform.)
// Every operation is rounded once (the Makefile's -ffp-contract=off -fno-fast-math); divisions and sqrt are the compiler's IEEE ones.
#pragma once
#include "rtw_denoise.hpp"

namespace rtw {

// the two cameras and what the host derives from them and from rtw_temporal_t, by value
template <typename T> struct TpParams {
    T o[3], llc[3], hor[3], ver[3];     // the current camera: origin, lower_left_corner, horizontal, vertical
    T po[3], pw[3], ph[3], pv[3];       // the previous camera: origin, w, horizontal, vertical  (HAS_PREV = false: unused)
    T Kw, Qh, Qv, ih, iv;               // q = llc - origin of the previous camera: q.w, q.hor, q.ver, 1 / hor.hor, 1 / ver.ver (binary64, rounded to T)
    T inv_sz, w_min, n_max;             // 1 / sigma_depth^2, min_weight, history_max (binary64, rounded to T)
    int m, mode;                        // normal_power_log2; RTW_DN_DEMOD | RTW_DN_GAMMA
    int W, H;
};

__device__ __forceinline__ float tp_floor(float x) { return __builtin_floorf(x); }
__device__ __forceinline__ double tp_floor(double x) { return __builtin_floor(x); }
template <typename T> __device__ __forceinline__ T tp_dot(T ax, T ay, T az, const T *b) { return (ax * b[0] + ay * b[1]) + az * b[2]; }

// the camera constants of a path from its table entry (include/rtw_hip.h rtw_reproject_table_*: TpParams' head o .. iv, element for element)
template <typename T> __device__ __forceinline__ void tp_load_cameras(TpParams<T> &U, const T *__restrict__ e) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        U.o[k] = e[k]; U.llc[k] = e[3 + k]; U.hor[k] = e[6 + k]; U.ver[k] = e[9 + k];
        U.po[k] = e[12 + k]; U.pw[k] = e[15 + k]; U.ph[k] = e[18 + k]; U.pv[k] = e[21 + k];
    }
    U.Kw = e[24]; U.Qh = e[25]; U.Qv = e[26]; U.ih = e[27]; U.iv = e[28];
}

template <typename T> struct TpSum { T w, e0, e1, e2, l; };

// one tap of the previous state; `ok`: inside the frame and valid.  The data of a tap that is not ok may be anything: selects, not weights, drop it.
// (g: the pixel's own guides (n, cov); hasP: it is covered; zexp: the depth its point has in the previous view)
// -> the tap's weight w (meaningful only where ok).  U: anything with m and inv_sz (TpParams, TpNoiseParams)
template <typename T, typename V, typename P>
__device__ __forceinline__ T tp_tap(TpSum<T> &a, const V &g, bool hasP, T zexp, const V &eq, const V &gq, T lq, T sb, bool ok, const P &U) {
    const T tv = T(1) - dn_abs(g.w - gq.w);
    const T wv = tv > T(0) ? tv : T(0);
    T w = sb * wv;
    const T dot = (g.x * gq.x + g.y * gq.y) + g.z * gq.z;
    T t = dot > T(0) ? dot : T(0);
    for (int r = 0; r < U.m; ++r) t = t * t;
    const T zs = zexp + eq.w;
    const T rz = (zexp - eq.w) / (zs > T(0) ? zs : T(1));
    const T wz = T(1) / (T(1) + (rz * rz) * U.inv_sz);
    const T wg = (w * t) * wz;
    w = (hasP && gq.w > T(0)) ? wg : w;                 // has(p) && has(q)  (cov_q = NaN: not valid, so not has)
    a.w = a.w + (ok ? w : T(0));
    a.e0 = a.e0 + (ok ? w * eq.x : T(0));
    a.e1 = a.e1 + (ok ? w * eq.y : T(0));
    a.e2 = a.e2 + (ok ? w * eq.z : T(0));
    a.l = a.l + (ok ? w * lq : T(0));
    return w;
}

// The trailing argument of the three kernels.  PATHS = false (one path): empty.  PATHS = true (rtw_reproject_batch_device_*,
// rtw_reproject_noise_batch_device_*): n_paths independent paths in one launch, the path index s = blockIdx.z * gridDim.y + blockIdx.y uniform over
// a workgroup; blockIdx.x numbers the blocks (tiles) of ONE path as in the single form.  Path s reads its camera constants from elements
// [32 s, 32 s + 29) of `table` -- the head of TpParams, o .. iv, in this order (uniform addresses: scalar loads) -- and finds its image, features,
// states and moment planes s strides behind the base pointers; then the body runs unchanged: it indexes relative to its base pointers and
// bounds every tap by W and H, which keeps a tap inside its own path.
constexpr unsigned TP_PATHS_Y = 65535;     // paths per grid row: what one 16-bit grid dimension holds
template <typename T, bool PATHS> struct TpPaths {};
template <typename T> struct TpPaths<T, true> {
    const T *table;                     // 32 elements per path (tp_noise: unused)
    long long st_stride, mo_stride;     // BYTES from one path's state / moment plane to the next (rtw_temporal_state_bytes, rtw_history_moment_bytes)
    unsigned n_paths;
};
// The trailing argument of the two step kernels: TpPaths and, MOTION = true (one path only), the motion plane behind it, pixel P at slot P.
// MOTION = false adds nothing: the argument has TpPaths' own bytes, so the kernel arguments of those instances lie where they always did.
template <typename T, bool PATHS, bool MOTION> struct TpTail : TpPaths<T, PATHS> {};
template <typename T> struct TpTail<T, false, true> : TpPaths<T, false> { const typename DnVec<T>::type *plane; };
template <typename T> __device__ __forceinline__ const T *tp_adv(const T *p, long long bytes) { return (const T *)((const char *)p + bytes); }
template <typename T> __device__ __forceinline__ T *tp_adv(T *p, long long bytes) { return (T *)((char *)p + bytes); }

// lane = flat pixel P = j*H + i
template <typename T, bool HAS_PREV, bool MOMENTS = false, bool PATHS = false, bool MOTION = false>
__global__ __launch_bounds__(256) void tp_step(TpParams<T> U, const T *__restrict__ image, const typename DnVec<T>::type *__restrict__ feat,
                                               const typename DnVec<T>::type *__restrict__ Ep, const typename DnVec<T>::type *__restrict__ Gp, const T *__restrict__ Lp,
                                               typename DnVec<T>::type *__restrict__ En, typename DnVec<T>::type *__restrict__ Gn, T *__restrict__ Ln, T *__restrict__ out,
                                               const T *__restrict__ Mp, T *__restrict__ Mn, [[maybe_unused]] TpTail<T, PATHS, MOTION> B) {
    using V = typename DnVec<T>::type;
    static_assert(!MOTION || (HAS_PREV && !PATHS), "the motion plane belongs to a single path's step behind the first frame");
    if constexpr (PATHS) {
        const long long s = (long long)blockIdx.z * gridDim.y + blockIdx.y;
        if (s >= B.n_paths) return;
        const long long fr = (long long)U.W * U.H * (long long)sizeof(T);         // bytes of one plane of one element per pixel
        image = tp_adv(image, s * fr * 3); out = tp_adv(out, s * fr * 3); feat = tp_adv(feat, s * fr * 8);
        En = tp_adv(En, s * B.st_stride); Gn = tp_adv(Gn, s * B.st_stride); Ln = tp_adv(Ln, s * B.st_stride);
        if constexpr (MOMENTS) Mn = tp_adv(Mn, s * B.mo_stride);
        if constexpr (HAS_PREV) {
            Ep = tp_adv(Ep, s * B.st_stride); Gp = tp_adv(Gp, s * B.st_stride); Lp = tp_adv(Lp, s * B.st_stride);
            if constexpr (MOMENTS) Mp = tp_adv(Mp, s * B.mo_stride);
            tp_load_cameras(U, B.table + s * 32);
        }
    }
    const long long H = U.H, W = U.W, n_pix = W * H;
    const long long P = (long long)blockIdx.x * 256 + threadIdx.x;
    if (P >= n_pix) return;
    // (a 32-bit division whenever the frame allows it)
    long long j, i;
    if (n_pix < (1ll << 31)) {
        const unsigned jj = (unsigned)P / (unsigned)H;
        j = jj; i = (unsigned)P - jj * (unsigned)H;
    } else {
        j = P / H; i = P - j * H;
    }
    // ---- prepare: dn_prepare's arithmetic on this pixel
    const T c0 = image[P * 3 + 0], c1 = image[P * 3 + 1], c2 = image[P * 3 + 2];
    const V f0 = feat[P * 2 + 0], f1 = feat[P * 2 + 1];        // albedo, n.x | n.y, n.z, depth, coverage
    const bool valid = dn_finite(c0) && dn_finite(c1) && dn_finite(c2) && dn_finite(f0.x) && dn_finite(f0.y) && dn_finite(f0.z) && dn_finite(f0.w) &&
                       dn_finite(f1.x) && dn_finite(f1.y) && dn_finite(f1.z) && dn_finite(f1.w);
    const T cov = f1.w;
    const bool has = valid && cov > T(0);
    const T dv = has ? cov : T(1);
    const T nx = f0.w / dv, ny = f1.x / dv, nz = f1.y / dv, zq = f1.z / dv;
    V g;
    g.x = has ? nx : T(0); g.y = has ? ny : T(0); g.z = has ? nz : T(0); g.w = cov;
    const T z = has ? zq : T(0);
    T a0 = T(1), a1 = T(1), a2 = T(1), e0 = c0, e1 = c1, e2 = c2;
    if (U.mode & RTW_DN_DEMOD) {
        const T floor_ = T(0.015625);               // 2^-6
        a0 = f0.x > floor_ ? f0.x : floor_; a1 = f0.y > floor_ ? f0.y : floor_; a2 = f0.z > floor_ ? f0.z : floor_;
        e0 = c0 / a0; e1 = c1 / a1; e2 = c2 / a2;
    }
    T r0 = e0, r1 = e1, r2 = e2, len = T(1);        // a reset
    [[maybe_unused]] T y2 = T(0), mom = T(0);       // (MOMENTS) the luminance's square; a reset stores it
    if constexpr (MOMENTS) {
        const T y = (e0 + e1) + e2;
        y2 = y * y; mom = y2;
    }
    if constexpr (HAS_PREV) {
#include "rtw_temporal_project.inc"
        const bool inr = x > T(-1) && x < T((int)W) && y > T(-1) && y < T((int)H);       // (a NaN fails)
        // (a position that is not in range decides nothing: its taps are gathered around (0, 0) and thrown away)
        const T xs = inr ? x : T(0), ys = inr ? y : T(0);
        const T xf = tp_floor(xs), yf = tp_floor(ys);
        const long long x0 = (int)xf, y0 = (int)yf;             // -1 .. W-1, -1 .. H-1
        const T fx = xs - xf, fy = ys - yf;
        const T zexp = dn_sqrt((d0 * d0 + d1 * d1) + d2 * d2);
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
        // ---- blend
        const bool accept = front && inr && a.w >= U.w_min;      // (a NaN sum fails)
        const T h0 = a.e0 / a.w, h1 = a.e1 / a.w, h2 = a.e2 / a.w, lh = a.l / a.w;
        const T l1 = lh + T(1);
        const T nn = l1 < U.n_max ? l1 : U.n_max;
        const T alpha = T(1) / nn;
        const T b0 = h0 + alpha * (e0 - h0), b1 = h1 + alpha * (e1 - h1), b2 = h2 + alpha * (e2 - h2);
        r0 = accept ? b0 : e0; r1 = accept ? b1 : e1; r2 = accept ? b2 : e2;
        len = accept ? nn : T(1);
        if constexpr (MOMENTS) {
            const T mh = sum_m / a.w;
            const T mb = mh + alpha * (y2 - mh);
            mom = accept ? mb : y2;
        }
    }
    // ---- end: the image and the next state
    T o0 = r0, o1 = r1, o2 = r2;
    if (U.mode & RTW_DN_DEMOD) { o0 = r0 * a0; o1 = r1 * a1; o2 = r2 * a2; }
    if (U.mode & RTW_DN_GAMMA) { o0 = dn_sqrt(o0); o1 = dn_sqrt(o1); o2 = dn_sqrt(o2); }
    out[P * 3 + 0] = valid ? o0 : dn_nan<T>();
    out[P * 3 + 1] = valid ? o1 : dn_nan<T>();
    out[P * 3 + 2] = valid ? o2 : dn_nan<T>();
    V en;
    en.x = valid ? r0 : T(0); en.y = valid ? r1 : T(0); en.z = valid ? r2 : T(0); en.w = z;
    g.w = valid ? cov : dn_nan<T>();
    En[P] = en; Gn[P] = g;
    Ln[P] = valid ? len : T(0);
    if constexpr (MOMENTS) Mn[P] = valid ? mom : T(0);
}

// what the host derives from rtw_temporal_noise_t, by value
template <typename T> struct TpNoiseParams {
    T inv_sz, min_len;                  // 1 / sigma_depth^2, min_len (binary64, rounded to T)
    int m, r;                           // normal_power_log2, radius
    int W, H;
};

// lane = flat pixel P = j*H + i of the state (E, G, L) and the moment plane M -> noise[P]
template <typename T, bool PATHS = false>
__global__ __launch_bounds__(256) void tp_noise(TpNoiseParams<T> U, const typename DnVec<T>::type *__restrict__ E, const typename DnVec<T>::type *__restrict__ G, const T *__restrict__ L,
                                                const T *__restrict__ M, T *__restrict__ noise, [[maybe_unused]] TpPaths<T, PATHS> B) {
    using V = typename DnVec<T>::type;
    if constexpr (PATHS) {
        const long long s = (long long)blockIdx.z * gridDim.y + blockIdx.y;
        if (s >= B.n_paths) return;
        E = tp_adv(E, s * B.st_stride); G = tp_adv(G, s * B.st_stride); L = tp_adv(L, s * B.st_stride);
        M = tp_adv(M, s * B.mo_stride);
        noise = tp_adv(noise, s * ((long long)U.W * U.H * (long long)sizeof(T)));
    }
    const long long H = U.H, W = U.W, n_pix = W * H;
    const long long P = (long long)blockIdx.x * 256 + threadIdx.x;
    if (P >= n_pix) return;
    long long j, i;
    if (n_pix < (1ll << 31)) {
        const unsigned jj = (unsigned)P / (unsigned)H;
        j = jj; i = (unsigned)P - jj * (unsigned)H;
    } else {
        j = P / H; i = P - j * H;
    }
    const V e = E[P], g = G[P];
    const T len = L[P], mp = M[P];
    const bool valid = g.w == g.w;
    const T lm = (e.x + e.y) + e.z;
    const T vt = mp - lm * lm;
    T var = vt > T(0) ? vt : T(0);
    if (valid && !(len >= U.min_len)) {
        // ---- a short history: the variance over the window, tp_tap's weights with sb = 1 and zexp = z_p (the centre tap is one of them)
        const bool has = g.w > T(0);
        TpSum<T> a = {T(0), T(0), T(0), T(0), T(0)};       // (a.w = S0; a.l = S1, fed Lm_q in len's place)
        T s2 = T(0);
        for (int dj = -U.r; dj <= U.r; ++dj) {
            for (int di = -U.r; di <= U.r; ++di) {
                const long long qi = i + di, qj = j + dj;
                const bool in = qi >= 0 && qi < H && qj >= 0 && qj < W;
                const long long q = in ? qj * H + qi : P;
                const V eq = E[q], gq = G[q];
                const T mq = M[q];
                const bool ok = in && gq.w == gq.w;
                const T lq = (eq.x + eq.y) + eq.z;
                const T w = tp_tap<T>(a, g, has, e.w, eq, gq, lq, T(1), ok, U);
                s2 = s2 + (ok ? w * mq : T(0));
            }
        }
        const T mu = a.l / a.w;
        const T vs = s2 / a.w - mu * mu;
        var = vs > T(0) ? vs : T(0);
    }
    const T v = var / len;
    const T floor_ = T(0.015625);                          // 2^-6
    const T rho = dn_sqrt(v) / (lm > floor_ ? lm : floor_);
    noise[P] = valid ? rho : dn_nan<T>();
}

}  // namespace rtw
