// rtw_present.hpp -- the kernel of the present stage (include/rtw_hip.h rtw_present_*: the definition is there): a frame of T elements in the
// render entry points' column-major layout -> display-ready bytes, row-major, 3 or 4 per pixel.  A transpose of small elements fused with
// the quantisation; memory-bound (12 or 24 bytes in, 3 or 4 out per pixel), so what matters is that both global sides run along their fast axis.
//   pr_present     one workgroup of 256 per tile of 64 x 64 pixels (the view folded into the tile index: a batch is one launch).
//     in             lanes along i: wave w takes the tile's columns w, w + 4, ...; lane l reads the three elements of pixel (i0 + l, j), so a
//                    wave reads 192 consecutive elements of its column.  Each channel is quantised in binary64 (pr_byte) and the pixel
//                    becomes ONE packed dword (byte 0..2 in output order, byte 3 = 255) at tile[l * 65 + c].
//     LDS            64 rows of 65 dwords (16 640 bytes).  ds_write_b32 and ds_read_b32 bank on (a/4) % 32 per 32-lane half: the column-order
//                    write of a half hits banks (l + c) % 32, l = 32 consecutive rows -- conflict-free; the row-order read of C = 4 hits
//                    (r + c) % 32, c = 32 consecutive columns -- conflict-free; the C = 3 reads take columns 4g + m of dword d = 3g + m, 32
//                    consecutive d span 42 columns -- 2-way (7 or 8 of the 32 banks hold two addresses), counted in DESIGN.md 6.
//     out            lanes along j, whole dwords.  C = 4: the packed dword as it is.  C = 3: dword at byte o of a row holds bytes o .. o + 3 =
//                    the last 3 - m bytes of pixel q = o / 3 (m = o % 3) and the first m + 1 of pixel q + 1: two neighbouring LDS dwords,
//                    ((lo & 0xffffff) >> 8m) | (hi << (24 - 8m)).
//   ALIGNED        C = 3 only.  true (W % 4 == 0: every row of every view starts on a dword): the tile's th * (3 tw / 4) dwords are dealt
//                    to the 256 lanes in one flat loop.  false: a row starts at any byte -- per row 0..3 head bytes up to the next dword
//                    boundary (lanes 48..50, byte stores), the dword body (lanes 0..47) and 0..3 tail bytes (lanes 52..54).  A head / tail byte's
//                    dword is shared with the neighbouring tile or row, which writes its own bytes of it: no byte is written twice.
// No atomics, no cross-lane operation but the LDS tile; scratch 0.  Every operation is rounded once (the Makefile's -ffp-contract=off
// -fno-fast-math: y + t is never fused into v * 255); the sqrt is the compiler's IEEE one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rtw {

#define RTW_PR_TILE 64
#define RTW_PR_STRIDE 65     // dwords per LDS row (odd: a column of the tile walks all 32 banks)
#define RTW_PR_DITHER 1      // the flags of rtw_present_t (include/rtw_hip.h RTW_PRESENT_*)
#define RTW_PR_BGR 2
#define RTW_PR_SQRT 4

struct PrParams {
    double exposure;
    int W, H;
    int tiles_y, tiles_per_view;    // tiles down a column of tiles; tiles of one view (tile index = (view * tiles_x + tj) * tiles_y + ti)
    int flags;
    unsigned nan_rgb;               // nan_rgb[k] in bits 8k .. 8k + 7 (R, G, B order: the swap happens with the other bytes)
};

// 64 * t of the ordered dither, t = (B(i mod 8, j mod 8) + 0.5) / 64: the 8 x 8 Bayer index, bits of r ^ c and r interleaved from the top
__device__ __forceinline__ double pr_threshold(int i, int j) {
    const unsigned r = (unsigned)i & 7u, x = ((unsigned)i ^ (unsigned)j) & 7u;
    unsigned B = 0;
    for (int b = 0; b < 3; ++b) B |= (((x >> b) & 1u) << (5 - 2 * b)) | (((r >> b) & 1u) << (4 - 2 * b));
    return (double)(2 * B + 1) * (1.0 / 128.0);            // exact
}

// one channel: steps 1 - 7 of the definition, binary64 throughout (binary32 would round x * 255 where binary64 does not)
template <typename T>
__device__ __forceinline__ unsigned pr_byte(T x, unsigned nan_byte, double t, const PrParams &U) {
    double v = (double)x;
    if (v != v) return nan_byte;
    v = v * U.exposure;
    v = v > 0.0 ? v : 0.0;                                 // (-0.0 and -inf: 0)
    v = v < 1.0 ? v : 1.0;
    if (U.flags & RTW_PR_SQRT) v = __builtin_sqrt(v);
    const double y = v * 255.0;
    double q;
    if (U.flags & RTW_PR_DITHER) { q = __builtin_floor(y + t); q = q < 255.0 ? q : 255.0; }
    else q = __builtin_rint(y);                            // ties to even
    return (unsigned)(int)q;
}

// bytes o .. o + 3 of a row of packed R, G, B triples, from the tile row `row` of packed dwords
__device__ __forceinline__ unsigned pr_dword3(const unsigned *row, int o) {
    const int q = o / 3, m = o - 3 * q;
    const unsigned lo = row[q], hi = row[q + 1];
    return ((lo & 0xffffffu) >> (8 * m)) | (hi << (24 - 8 * m));
}
__device__ __forceinline__ unsigned char pr_byte3(const unsigned *row, int o) {
    const int q = o / 3, m = o - 3 * q;
    return (unsigned char)(row[q] >> (8 * m));
}

template <typename T, int C, bool ALIGNED>
__global__ __launch_bounds__(256) void pr_present(const PrParams U, const T *__restrict__ in, unsigned char *__restrict__ out) {
    static_assert(C == 3 || (C == 4 && ALIGNED), "C = 4 has one path");
    __shared__ unsigned tile[RTW_PR_TILE * RTW_PR_STRIDE];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const unsigned b = blockIdx.x;
    const unsigned view = b / (unsigned)U.tiles_per_view, r = b - view * (unsigned)U.tiles_per_view;
    const int tj = (int)(r / (unsigned)U.tiles_y), ti = (int)(r - (unsigned)tj * (unsigned)U.tiles_y);
    const int i0 = ti * RTW_PR_TILE, j0 = tj * RTW_PR_TILE;
    const int th = min(RTW_PR_TILE, U.H - i0), tw = min(RTW_PR_TILE, U.W - j0);
    const long long n_pix = (long long)U.W * U.H, pix0 = (long long)view * n_pix;     // pix0: the view's first pixel in either buffer

    // ---- in: columns of the tile, quantised and packed ----
    if (lane < th) {
        const int i = i0 + lane;
        const bool bgr = (U.flags & RTW_PR_BGR) != 0;
        const int s0 = bgr ? 16 : 0, s2 = bgr ? 0 : 16;
        const T *src = in + (pix0 + i) * 3;
#pragma unroll 4
        for (int c = wave; c < tw; c += 4) {
            const int j = j0 + c;
            const T *p = src + (long long)j * U.H * 3;
            const T x0 = p[0], x1 = p[1], x2 = p[2];
            const double td = (U.flags & RTW_PR_DITHER) ? pr_threshold(i, j) : 0.0;
            const unsigned q0 = pr_byte(x0, U.nan_rgb & 0xffu, td, U), q1 = pr_byte(x1, (U.nan_rgb >> 8) & 0xffu, td, U),
                           q2 = pr_byte(x2, (U.nan_rgb >> 16) & 0xffu, td, U);
            tile[lane * RTW_PR_STRIDE + c] = (q0 << s0) | (q1 << 8) | (q2 << s2) | 0xff000000u;
        }
    }
    __syncthreads();

    // ---- out: rows of the tile ----
    if (C == 4) {
        uint32_t *o = reinterpret_cast<uint32_t *>(out) + pix0;
        if (lane < tw)
            for (int rr = wave; rr < th; rr += 4) o[(long long)(i0 + rr) * U.W + j0 + lane] = tile[rr * RTW_PR_STRIDE + lane];
    } else if (ALIGNED) {
        // W % 4 == 0: (pix0 + i * W + j0) * 3 is a multiple of 4 for every row, and so is 3 * tw
        uint32_t *o = reinterpret_cast<uint32_t *>(out);
        const int nd = tw * 3 / 4, total = th * nd;
        for (int idx = t; idx < total; idx += 256) {
            const int rr = idx / nd, d = idx - rr * nd;
            o[(pix0 + (long long)(i0 + rr) * U.W + j0) * 3 / 4 + d] = pr_dword3(tile + rr * RTW_PR_STRIDE, 4 * d);
        }
    } else {
        const int nb = tw * 3;                                           // bytes of a tile row (<= 192)
        for (int rr = wave; rr < th; rr += 4) {
            const unsigned *row = tile + rr * RTW_PR_STRIDE;
            const long long rowb = (pix0 + (long long)(i0 + rr) * U.W + j0) * 3;           // the row's first byte (`out` is dword aligned)
            const int head = min((int)((4 - (rowb & 3)) & 3), nb), body = (nb - head) >> 2, tail = nb - head - 4 * body;
            if (lane < body) {
                const int o = head + 4 * lane;
                *reinterpret_cast<uint32_t *>(out + rowb + o) = pr_dword3(row, o);
            } else if (lane >= 48 && lane < 48 + head) {
                const int o = lane - 48;
                out[rowb + o] = pr_byte3(row, o);
            } else if (lane >= 52 && lane < 52 + tail) {
                const int o = head + 4 * body + (lane - 52);
                out[rowb + o] = pr_byte3(row, o);
            }
        }
    }
}

}  // namespace rtw
