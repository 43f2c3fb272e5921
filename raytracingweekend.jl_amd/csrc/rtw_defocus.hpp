// rtw_defocus.hpp -- the kernels of the defocus stage (include/rtw_hip.h rtw_defocus_*: the definition is there): depth of field as a gather on a
// finished pinhole frame, driven by the depth plane of the feature buffer.
//   df_prepare     one workgroup per 16 x 16 tile, lane t at row t % 16, column t / 16 of the tile (consecutive lanes: consecutive slots of the
//                  column-major planes), the motion blur's mb_velocity mapping.  The pixel is prepared as tp_step prepares it (validity, cov, z),
//                  its own ray is the step's (rtw_temporal_project.inc; the projection behind it is dead code here), and its circle of confusion
//                  (R, zc, w, 0) goes to the CoC plane in one 16- / 32-byte store.  The tile's greatest R is reduced by six cross-lane exchanges per
//                  wave and one pass over the four waves' maxima in LDS; lane 0 writes the tile plane's element.
//   df_gather      one workgroup per tile with the same lane mapping.  RN (the greatest R of the up to nine tiles around) and m are uniform
//                  over the workgroup: the tile slots' addresses depend on blockIdx alone (scalar loads), the early-out is a uniform branch.
//                  The workgroup stages its (16 + 2m)^2 window ONCE in LDS -- colour, max(R, 1/2), zc, w, structure of arrays per window
//                  column -- and the tap loop reads only LDS.  A window pixel outside the frame or not valid is staged as (Rh = -1, zc = NaN):
//                  its cover is 0, so a tap needs no bounds test.  dist comes from the host-built table DfDist (uniform index: scalar loads);
//                  there is no division in the tap loop (w = 1 / Rh^2 was divided in df_prepare), one per channel behind it.
//   LDS layout     window pixel (wi, wj) (row, column), array k of (c0, c1, c2, Rh, zc, w), lies at element (wj*6 + k)*32 + (wi ^ ((wj & 1) << 4)):
//                  a window column is 32 elements, the six arrays of a column follow each other (one address register per tap, the arrays at
//                  immediate offsets), and the rows of odd columns are rotated by 16.  A 32-lane half of a wave is 16 rows of two neighbouring
//                  columns, one even and one odd: the 16 rows a .. a+15 of the even column and the rows (a .. a+15) ^ 16 of the odd one fall on
//                  32 different elements modulo 32, so ds_read_b32 (bank = dword mod 32) and ds_read_b64 (bank = dword mod 64, two per lane)
//                  are conflict-free at every tap offset; a plain pitch of 32 would be 2-way for both.  The staging writes go a column of 32
//                  rows per half wave: 32 consecutive elements, conflict-free.  
//   VIEWS          true (rtw_lens_batch_device_*): n_views views in one launch, DfViews below; false: the instance is the single
//                  form's, instruction for instruction (the flag only adds code under `if constexpr`).
// Every operation is rounded once (the Makefile's -ffp-contract=off -fno-fast-math); divisions and sqrt are the compiler's IEEE ones; taps that
// do not take part are dropped by selects.
#pragma once
#include "rtw_temporal.hpp"

namespace rtw {

constexpr int DF_TILE = 16;             // RTW_DEFOCUS_TILE
constexpr int DF_MAX_RADIUS = 8;        // RTW_DEFOCUS_MAX_RADIUS
constexpr int DF_COL = 6 * 32;          // elements of one window column in LDS: six arrays of 32 rows

// dist = sqrt(T(di*di + dj*dj)) for |di|, |dj| <= 8, built by the host in T: d[|dj|*9 + |di|]
template <typename T> struct DfDist { T d[(DF_MAX_RADIUS + 1) * (DF_MAX_RADIUS + 1)]; };

__device__ __forceinline__ float df_ceil(float x) { return __builtin_ceilf(x); }
__device__ __forceinline__ double df_ceil(double x) { return __builtin_ceil(x); }
__device__ __forceinline__ float df_abs(float x) { return __builtin_fabsf(x); }
__device__ __forceinline__ double df_abs(double x) { return __builtin_fabs(x); }
template <typename T> __device__ __forceinline__ T df_inf() { return T(__builtin_huge_valf()); }
template <typename T> __device__ __forceinline__ T df_min(T a, T b) { return a < b ? a : b; }
template <typename T> __device__ __forceinline__ T df_max(T a, T b) { return a > b ? a : b; }
template <typename T> __device__ __forceinline__ T df_clamp01(T x) { return x > T(0) ? (x < T(1) ? x : T(1)) : T(0); }

// the direction nD of pixel (i, j)'s own ray, by the step's own text (rtw_temporal_project.inc; what it projects is not used here)
template <typename T>
__device__ __forceinline__ void df_ray(const TpParams<T> &U, long long i, long long j, long long W, long long H, bool has, T z, T &n0_, T &n1_, T &n2_) {
    using V = typename DnVec<T>::type;
    constexpr bool MOTION = false;
    [[maybe_unused]] const long long P = 0;
    [[maybe_unused]] const struct { const V *plane; } B = {nullptr};
#include "rtw_temporal_project.inc"
    (void)front; (void)x; (void)y;
    n0_ = n0; n1_ = n1; n2_ = n2;
}

// The trailing argument of the lens kernels (df_prepare, df_gather; wa_reduce, wa_compose of rtw_wide_aperture.hpp).  VIEWS = false (one
// view): empty, so the kernel arguments of those instances lie where they always did.  VIEWS = true: n_views independent views in one launch,
// the view index v = blockIdx.z * gridDim.y + blockIdx.y uniform over a workgroup (df_view); blockIdx.x numbers the tiles of ONE view as in the
// single form.  View v finds pointer k of the kernel's N pointers, in the order of its arguments, v * stride[k] BYTES behind the base (a stride
// of 0: every view reads the same frame); then the body runs unchanged: it indexes relative to its base pointers and bounds every tap by W
// and H, which keeps a tap inside its own view.  A workgroup with v >= n_views (the last grid row) leaves before its first barrier.
constexpr unsigned DF_VIEWS_Y = 65535;      // views per grid row: what one 16-bit grid dimension holds
template <typename T, bool VIEWS, int N> struct DfViews {};
template <typename T, int N> struct DfViews<T, true, N> {
    long long stride[N];
    unsigned n_views;
};
// df_prepare's: the strides and the lens table -- 32 elements per view: [0, 29) the head of TpParams, o .. iv (rtw_reproject_table_* of the
// view's camera as its own previous one), 29: F, 30: K, 31: 0 -- read at uniform addresses (scalar loads, like tp_load_cameras)
template <typename T, bool VIEWS> struct DfLens : DfViews<T, VIEWS, 4> {};
template <typename T> struct DfLens<T, true> : DfViews<T, true, 4> { const T *table; };
__device__ __forceinline__ long long df_view() { return (long long)blockIdx.z * gridDim.y + blockIdx.y; }

// U: the camera's fields and W, H (the head of a step's TpParams built with cam_prev = cam, so that U.pw is the camera's w; nothing else of the
// previous camera is read); F, K, Rm: the host constants of the definition
template <typename T, bool VIEWS = false>
__global__ __launch_bounds__(256) void df_prepare(TpParams<T> U, T F, T K, T Rm, const T *__restrict__ image, const typename DnVec<T>::type *__restrict__ feat,
                                                  typename DnVec<T>::type *__restrict__ coc, T *__restrict__ tile, [[maybe_unused]] DfLens<T, VIEWS> B) {
    using V = typename DnVec<T>::type;
    __shared__ T s_r[4];
    if constexpr (VIEWS) {
        const long long v = df_view();
        if (v >= B.n_views) return;
        image = tp_adv(image, v * B.stride[0]); feat = tp_adv(feat, v * B.stride[1]); coc = tp_adv(coc, v * B.stride[2]); tile = tp_adv(tile, v * B.stride[3]);
        const T *__restrict__ e = B.table + v * 32;
        tp_load_cameras(U, e);
        F = e[29]; K = e[30];
    }
    const long long H = U.H, W = U.W;
    const unsigned TH = (unsigned)((H + DF_TILE - 1) / DF_TILE);
    const unsigned tb = blockIdx.x / TH, ta = blockIdx.x - tb * TH;
    const int t = (int)threadIdx.x;
    const long long i = (long long)ta * DF_TILE + (t & 15), j = (long long)tb * DF_TILE + (t >> 4);
    T R = T(-1);                                    // (a lane outside the frame, a pixel that is not valid: never above a valid pixel's R >= 0)
    if (i < H && j < W) {
        const long long P = j * H + i;
        // ---- prepare: tp_step's arithmetic on this pixel (validity, cov, z)
        const T c0 = image[P * 3 + 0], c1 = image[P * 3 + 1], c2 = image[P * 3 + 2];
        const V f0 = feat[P * 2 + 0], f1 = feat[P * 2 + 1];
        const bool valid = dn_finite(c0) && dn_finite(c1) && dn_finite(c2) && dn_finite(f0.x) && dn_finite(f0.y) && dn_finite(f0.z) && dn_finite(f0.w) &&
                           dn_finite(f1.x) && dn_finite(f1.y) && dn_finite(f1.z) && dn_finite(f1.w);
        const T cov = f1.w;
        const bool has = valid && cov > T(0);
        const T zq = f1.z / (has ? cov : T(1));
        const T z = has ? zq : T(0);
        // ---- the depth along the optical axis and the circle of confusion
        T n0, n1, n2;
        df_ray<T>(U, i, j, W, H, has, z, n0, n1, n2);
        const T ca = -tp_dot<T>(n0, n1, n2, U.pw);
        const T zax = z * ca;
        const T dz = zax - F;
        const T Rl = df_min<T>(K * (df_abs(dz) / zax), Rm), Rs = df_min<T>(K, Rm);
        const T Rv = (has && zax > T(0)) ? Rl : Rs;
        const T Rh = df_max<T>(Rv, T(0.5));
        const T w = T(1) / (Rh * Rh);
        R = valid ? Rv : T(-1);
        V s;
        s.x = R; s.y = valid ? (has ? z : df_inf<T>()) : dn_nan<T>(); s.z = valid ? w : T(0); s.w = T(0);
        coc[P] = s;
    }
    // ---- the tile's maximum: the wave's, then the four waves'
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) R = df_max<T>(__shfl_xor(R, m), R);
    if ((t & 63) == 0) s_r[t >> 6] = R;
    __syncthreads();
    if (t == 0) tile[blockIdx.x] = df_max<T>(df_max<T>(s_r[1], s_r[0]), df_max<T>(s_r[3], s_r[2]));
}

// mmax: max_radius, what the launch's dynamic LDS holds -- (16 + 2*mmax) window columns of DF_COL elements
template <typename T, bool VIEWS = false>
__global__ __launch_bounds__(256) void df_gather(int W_, int H_, int mmax, int gamma, DfDist<T> tab, const T *__restrict__ image, const typename DnVec<T>::type *__restrict__ coc,
                                                 const T *__restrict__ tile, T *__restrict__ out, [[maybe_unused]] DfViews<T, VIEWS, 4> B) {
    using V = typename DnVec<T>::type;
    extern __shared__ __align__(16) unsigned char df_lds[];
    T *win = reinterpret_cast<T *>(df_lds);
    if constexpr (VIEWS) {
        const long long v = df_view();
        if (v >= B.n_views) return;
        image = tp_adv(image, v * B.stride[0]); coc = tp_adv(coc, v * B.stride[1]); tile = tp_adv(tile, v * B.stride[2]); out = tp_adv(out, v * B.stride[3]);
    }
    const int H = H_, W = W_;
    const int TH = (H + DF_TILE - 1) / DF_TILE, TW = (W + DF_TILE - 1) / DF_TILE;
    const int tb = (int)(blockIdx.x / (unsigned)TH), ta = (int)blockIdx.x - tb * TH;
    const int t = (int)threadIdx.x;
    // ---- the neighbourhood's greatest radius (uniform: scalar loads of up to nine tile slots)
    T RN = T(-1);
    for (int db = -1; db <= 1; ++db) {
        for (int da = -1; da <= 1; ++da) {
            const int qa = ta + da, qb = tb + db;
            if (qa >= 0 && qa < TH && qb >= 0 && qb < TW) RN = df_max<T>(tile[qb * TH + qa], RN);
        }
    }
    const bool filt = RN >= T(0.5);
    int m = 0;
    if (filt) {
        m = (int)df_ceil(RN + T(0.5)) - 1;
        m = m < mmax ? m : mmax;                    // (R <= Rm = mmax by df_prepare's min: never taken; the bound of the LDS window)
        m = __builtin_amdgcn_readfirstlane(m);
        // ---- stage the (16 + 2m)^2 window: a half wave per window column, 8 columns per pass
        const int S = DF_TILE + 2 * m;
        const int wi = t & 31;
        const int gi = ta * DF_TILE - m + wi;
        for (int wj = t >> 5; wj < S; wj += 8) {
            const int gj = tb * DF_TILE - m + wj;
            if (wi < S) {
                const bool inq = gi >= 0 && gi < H && gj >= 0 && gj < W;
                const long long q = inq ? (long long)gj * H + gi : 0;
                const V s = coc[q];
                const T q0 = image[q * 3 + 0], q1 = image[q * 3 + 1], q2 = image[q * 3 + 2];
                const bool ok = inq && s.y == s.y;
                T *p = win + wj * DF_COL + (wi ^ ((wj & 1) << 4));
                p[0] = ok ? q0 : T(0); p[32] = ok ? q1 : T(0); p[64] = ok ? q2 : T(0);
                p[96] = ok ? df_max<T>(s.x, T(0.5)) : T(-1); p[128] = ok ? s.y : dn_nan<T>(); p[160] = ok ? s.z : T(0);
            }
        }
    }
    __syncthreads();
    const int i = ta * DF_TILE + (t & 15), j = tb * DF_TILE + (t >> 4);
    if (i >= H || j >= W) return;
    const long long P = (long long)j * H + i;
    const T c0 = image[P * 3 + 0], c1 = image[P * 3 + 1], c2 = image[P * 3 + 2];
    const V sx = coc[P];
    const bool valid = sx.y == sx.y;
    T o0 = c0, o1 = c1, o2 = c2;
    if (filt) {
        const T zX = sx.y, wX = sx.z, RhX = df_max<T>(sx.x, T(0.5));
        const int ci = (t & 15) + m, cj = (t >> 4) + m;
        T wsum = T(0), s0 = T(0), s1 = T(0), s2 = T(0);
        for (int dj = -m; dj <= m; ++dj) {
            const int wj = cj + dj, sw = (wj & 1) << 4;
            const T *col = win + wj * DF_COL;
            const T *drow = tab.d + (dj < 0 ? -dj : dj) * (DF_MAX_RADIUS + 1);
            for (int di = -m; di <= m; ++di) {
                const T dist = drow[di < 0 ? -di : di];
                const T *p = col + ((ci + di) ^ sw);
                const T q0 = p[0], q1 = p[32], q2 = p[64], Rhq = p[96], zq = p[128], wq = p[160];
                const bool lim = zq > zX && RhX < Rhq;
                const T Re = lim ? RhX : Rhq, we = lim ? wX : wq;
                const T cover = df_clamp01<T>((Re + T(0.5)) - dist);
                const bool ok = cover > T(0);
                const T a = cover * we;
                const T ws = wsum + a, t0 = s0 + a * q0, t1 = s1 + a * q1, t2 = s2 + a * q2;
                wsum = ok ? ws : wsum; s0 = ok ? t0 : s0; s1 = ok ? t1 : s1; s2 = ok ? t2 : s2;
            }
        }
        o0 = s0 / wsum; o1 = s1 / wsum; o2 = s2 / wsum;
    }
    if (gamma) { o0 = dn_sqrt(o0); o1 = dn_sqrt(o1); o2 = dn_sqrt(o2); }
    out[P * 3 + 0] = valid ? o0 : dn_nan<T>();
    out[P * 3 + 1] = valid ? o1 : dn_nan<T>();
    out[P * 3 + 2] = valid ? o2 : dn_nan<T>();
}

}  // namespace rtw
