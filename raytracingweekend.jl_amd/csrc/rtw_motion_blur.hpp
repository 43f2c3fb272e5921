// rtw_motion_blur.hpp -- the kernels of the motion-blur stage (include/rtw_hip.h rtw_velocity_blur_*: the definition is there): a deterministic
// form of McGuire et al. 2012 on the motion plane -- tile max, neighbour max, a gather along the neighbourhood's dominant velocity.
//   mb_velocity    one workgroup per 16 x 16 tile, lane t at row t % 16, column t / 16 of the tile (consecutive lanes: consecutive slots of the
//                  column-major planes).  The pixel is prepared as tp_step prepares it (validity, cov, z), projected into the previous camera
//                  by the step's own code (rtw_temporal_project.inc), with the motion plane, and its half-extent (h.x, h.y, zc, l) goes to the blur plane.
//                  The tile's greatest l (ties: the lowest slot, which inside a tile is the lowest lane) is reduced by six cross-lane
//                  exchanges per wave and one pass over the four waves' winners in LDS; lane 0 writes the tile plane's slot (h.x, h.y, l, 0).
//   mb_neighbour   one lane per tile: the greatest l over the up to nine tiles around it, ties to the lowest tile index -> (vN.x, vN.y, lN, 0).
//   mb_gather      one workgroup per tile with mb_velocity's lane mapping, so a wave is a 16-row x 4-column patch inside ONE tile: vN, lN and
//                  the tap parameter are uniform over the workgroup, the early-out on lN is a uniform branch, and at every tap consecutive
//                  lanes read consecutive slots.  Taps come from global memory (L1 / L2): one slot of the blur plane and three colour elements
//                  each, as dn_level's do.  No LDS.  PASS = true (the first frame of rtw_render_blurred_*: no previous camera):
//                  the pixel passes through -- validity from the image and the features, the gamma, nothing else is read.
// Every operation is rounded once (the Makefile's -ffp-contract=off -fno-fast-math); divisions and sqrt are the compiler's IEEE ones; taps that
// do not take part are dropped by selects.
#pragma once
#include "rtw_temporal.hpp"

namespace rtw {

constexpr int MB_TILE = 16;             // RTW_VELOCITY_BLUR_TILE

__device__ __forceinline__ float mb_rint(float x) { return __builtin_rintf(x); }
__device__ __forceinline__ double mb_rint(double x) { return __builtin_rint(x); }
template <typename T> __device__ __forceinline__ T mb_inf() { return T(__builtin_huge_valf()); }
template <typename T> __device__ __forceinline__ T mb_clamp01(T x) { return x > T(0) ? (x < T(1) ? x : T(1)) : T(0); }
template <typename T> __device__ __forceinline__ T mb_cone(T dist, T l) { return mb_clamp01<T>(T(1) - dist / l); }
template <typename T> __device__ __forceinline__ T mb_cyl(T dist, T l) {
    const T x = mb_clamp01<T>((dist - T(0.95) * l) / (T(0.1) * l));
    return T(1) - (x * x) * (T(3) - T(2) * x);
}
// (l, lane) against (l2, lane2): the greater l wins, among equals the lower lane
template <typename T> __device__ __forceinline__ bool mb_beats(T l2, int t2, T l, int t) { return l2 > l || (l2 == l && t2 < t); }

// where pixel (i, j) at slot P lay in the previous view, by the step's own projection (rtw_temporal_project.inc) with the motion plane
template <typename T, typename V>
__device__ __forceinline__ void mb_previous(const TpParams<T> &U, long long i, long long j, long long W, long long H, long long P, bool has, T z, const V *plane, bool &front_, T &x_, T &y_) {
    constexpr bool MOTION = true;
    const struct { const V *plane; } B = {plane};
#include "rtw_temporal_project.inc"
    front_ = front; x_ = x; y_ = y;
}

// U: the two cameras and W, H (the head of a step's TpParams; inv_sz .. mode are not read); hs = T(shutter / 2)
template <typename T>
__global__ __launch_bounds__(256) void mb_velocity(TpParams<T> U, T hs, const T *__restrict__ image, const typename DnVec<T>::type *__restrict__ feat,
                                                   const typename DnVec<T>::type *__restrict__ motion, typename DnVec<T>::type *__restrict__ blur,
                                                   typename DnVec<T>::type *__restrict__ tile) {
    using V = typename DnVec<T>::type;
    __shared__ T s_l[4], s_x[4], s_y[4];
    __shared__ int s_t[4];
    const long long H = U.H, W = U.W;
    const unsigned TH = (unsigned)((H + MB_TILE - 1) / MB_TILE);
    const unsigned tb = blockIdx.x / TH, ta = blockIdx.x - tb * TH;
    const int t = (int)threadIdx.x;
    const long long i = (long long)ta * MB_TILE + (t & 15), j = (long long)tb * MB_TILE + (t >> 4);
    const bool in = i < H && j < W;
    T hx = T(0), hy = T(0), l = T(-1);             // (a lane outside the frame never wins: every tile holds a pixel, and l >= 0 there)
    if (in) {
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
        // ---- where the pixel's surface was in the previous view: the motion step's projection
        bool front;
        T x, y;
        mb_previous<T>(U, i, j, W, H, P, has, z, motion, front, x, y);
        const bool moved = valid && front && dn_finite(x) && dn_finite(y);
        const T ux = moved ? T((int)j) - x : T(0), uy = moved ? T((int)i) - y : T(0);
        // ---- the half-extent, at most MB_TILE pixels long
        hx = ux * hs; hy = uy * hs;
        T l2 = hx * hx + hy * hy;
        const bool big = l2 > T(MB_TILE * MB_TILE);
        const T sc = T(MB_TILE) / dn_sqrt(l2);
        const T kx = hx * sc, ky = hy * sc;
        hx = big ? kx : hx; hy = big ? ky : hy;
        const T k2 = hx * hx + hy * hy;
        l2 = big ? k2 : l2;
        l = dn_sqrt(l2);
        V s;
        s.x = hx; s.y = hy; s.z = valid ? (has ? z : mb_inf<T>()) : dn_nan<T>(); s.w = l;
        blur[P] = s;
    }
    // ---- the tile's maximum: the wave's, then the four waves'
    int wt = t;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const T l2 = __shfl_xor(l, m), x2 = __shfl_xor(hx, m), y2 = __shfl_xor(hy, m);
        const int t2 = __shfl_xor(wt, m);
        const bool b = mb_beats<T>(l2, t2, l, wt);
        l = b ? l2 : l; hx = b ? x2 : hx; hy = b ? y2 : hy; wt = b ? t2 : wt;
    }
    if ((t & 63) == 0) { s_l[t >> 6] = l; s_x[t >> 6] = hx; s_y[t >> 6] = hy; s_t[t >> 6] = wt; }
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const bool b = mb_beats<T>(s_l[w], s_t[w], l, wt);
            l = b ? s_l[w] : l; hx = b ? s_x[w] : hx; hy = b ? s_y[w] : hy; wt = b ? s_t[w] : wt;
        }
        V o;
        o.x = hx; o.y = hy; o.z = l; o.w = T(0);
        tile[blockIdx.x] = o;
    }
}

// lane = tile index b*TH + a
template <typename T>
__global__ __launch_bounds__(256) void mb_neighbour(int TH, int TW, const typename DnVec<T>::type *__restrict__ tile, typename DnVec<T>::type *__restrict__ nb) {
    using V = typename DnVec<T>::type;
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= (long long)TH * TW) return;
    const int b = (int)(k / TH), a = (int)(k - (long long)b * TH);
    T bx = T(0), by = T(0), bl = T(-1);
    // (in the order of the tile index, a strictly greater l replaces: ties stay with the lowest index)
    for (int db = -1; db <= 1; ++db) {
        for (int da = -1; da <= 1; ++da) {
            const int qa = a + da, qb = b + db;
            const bool in = qa >= 0 && qa < TH && qb >= 0 && qb < TW;
            const V v = tile[in ? (long long)qb * TH + qa : k];
            const bool up = in && v.z > bl;
            bx = up ? v.x : bx; by = up ? v.y : by; bl = up ? v.z : bl;
        }
    }
    V o;
    o.x = bx; o.y = by; o.z = bl; o.w = T(0);
    nb[k] = o;
}

template <typename T, bool PASS>
__global__ __launch_bounds__(256) void mb_gather(int W_, int H_, int taps, int gamma, T ext, const T *__restrict__ image, [[maybe_unused]] const typename DnVec<T>::type *__restrict__ feat,
                                                 [[maybe_unused]] const typename DnVec<T>::type *__restrict__ blur, [[maybe_unused]] const typename DnVec<T>::type *__restrict__ nb,
                                                 T *__restrict__ out) {
    using V = typename DnVec<T>::type;
    const long long H = H_, W = W_;
    const unsigned TH = (unsigned)((H + MB_TILE - 1) / MB_TILE);
    const unsigned tb = blockIdx.x / TH, ta = blockIdx.x - tb * TH;
    const int t = (int)threadIdx.x;
    const long long i = (long long)ta * MB_TILE + (t & 15), j = (long long)tb * MB_TILE + (t >> 4);
    if (i >= H || j >= W) return;
    const long long P = j * H + i;
    const T c0 = image[P * 3 + 0], c1 = image[P * 3 + 1], c2 = image[P * 3 + 2];
    T o0 = c0, o1 = c1, o2 = c2;
    bool valid;
    if constexpr (PASS) {
        const V f0 = feat[P * 2 + 0], f1 = feat[P * 2 + 1];
        valid = dn_finite(c0) && dn_finite(c1) && dn_finite(c2) && dn_finite(f0.x) && dn_finite(f0.y) && dn_finite(f0.z) && dn_finite(f0.w) &&
                dn_finite(f1.x) && dn_finite(f1.y) && dn_finite(f1.z) && dn_finite(f1.w);
    } else {
        const V sx = blur[P];
        const V vn = nb[blockIdx.x];                           // (uniform)
        valid = sx.z == sx.z;
        if (vn.z >= T(0.5)) {
            const T zx = sx.z;
            const bool finx = zx < mb_inf<T>();
            const T lX = sx.w > T(0.5) ? sx.w : T(0.5);
            const T w0 = T(1) / lX;
            T wsum = w0, s0 = c0 * w0, s1 = c1 * w0, s2 = c2 * w0;
            const int mid = (taps - 1) >> 1;
            const T fj = T((int)j), fi = T((int)i), den = T(taps + 1);
            for (int n = 0; n < taps; ++n) {
                if (n == mid) continue;
                const T tt = T(2 * (n + 1) - (taps + 1)) / den;
                const long long qj = (int)mb_rint(fj + vn.x * tt), qi = (int)mb_rint(fi + vn.y * tt);
                const bool inq = qi >= 0 && qi < H && qj >= 0 && qj < W;
                const long long q = inq ? qj * H + qi : P;
                const V sq = blur[q];
                const T q0 = image[q * 3 + 0], q1 = image[q * 3 + 1], q2 = image[q * 3 + 2];
                const bool ok = inq && sq.z == sq.z;
                const T dx = T((int)(qj - j)), dy = T((int)(qi - i));
                const T dist = dn_sqrt(dx * dx + dy * dy);
                const T lY = sq.w > T(0.5) ? sq.w : T(0.5);
                // ---- the soft depth compare: arithmetic only between two finite depths that differ
                const T zy = sq.z;
                const bool finy = zy < mb_inf<T>(), same = zy == zx, both = finx && finy;
                const T fa = mb_clamp01<T>(T(1) - (zy - zx) / ext), ba = mb_clamp01<T>(T(1) - (zx - zy) / ext);
                const T f = same ? T(1) : both ? fa : finy ? T(1) : T(0);
                const T b = same ? T(1) : both ? ba : finx ? T(1) : T(0);
                const T a = (f * mb_cone<T>(dist, lY) + b * mb_cone<T>(dist, lX)) + (mb_cyl<T>(dist, lY) * mb_cyl<T>(dist, lX)) * T(2);
                const T ws = wsum + a, t0 = s0 + a * q0, t1 = s1 + a * q1, t2 = s2 + a * q2;
                wsum = ok ? ws : wsum; s0 = ok ? t0 : s0; s1 = ok ? t1 : s1; s2 = ok ? t2 : s2;
            }
            o0 = s0 / wsum; o1 = s1 / wsum; o2 = s2 / wsum;
        }
    }
    if (gamma) { o0 = dn_sqrt(o0); o1 = dn_sqrt(o1); o2 = dn_sqrt(o2); }
    out[P * 3 + 0] = valid ? o0 : dn_nan<T>();
    out[P * 3 + 1] = valid ? o1 : dn_nan<T>();
    out[P * 3 + 2] = valid ? o2 : dn_nan<T>();
}

}  // namespace rtw
