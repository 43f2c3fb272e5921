// rtw_accum_kernels.hip -- everything of the accumulator that runs on the device, and what exists to test it: the merge and resolve
// kernels, the tile kernels that evaluate the adaptive render's stopping rule from the accumulator words, the noise map, the batched forms of
// all of them, their launches (rtw_accum.hpp) and the unit ops 21-23, 25, 30, 31 on hand-made words (accum_unit).  Nothing here looks into an
// accumulator object: words, C_t arrays and view tables come in as device pointers.  (rtw_accum.hip: the object and the host paths.)
//
// "View v of a batch is bit for bit the single call" holds because an element's arithmetic is written once -- resolve_value, noise_value,
// tile_not_converged -- and the single and the batched kernel differ in how they find the element's view and nothing else.
// (-ffp-contract=off: no FMA anywhere in this library unless the source writes one.)
#include "rtw_accum.hpp"
#include "rtw_path.hpp"         // fx_to_double

#include <optional>

namespace rtwh {

namespace {

// dst += src: lane = one 16-byte pair of one pixel -- a channel's (lo, hi) (128-bit add with carry) or (poison, 0) (plain add)
__global__ __launch_bounds__(256) void accum_merge_kernel(ulonglong2 *__restrict__ dst, const ulonglong2 *__restrict__ src, size_t n_pairs) {
    const size_t k = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= n_pairs) return;
    const ulonglong2 a = dst[k], b = src[k];
    ulonglong2 r;
    r.x = a.x + b.x;
    r.y = a.y + b.y + (((k & 3u) != 3u && r.x < a.x) ? 1ull : 0ull);
    dst[k] = r;
}

// ---- one element of a frame: store_job's formula (rtw_kernels.hpp) on the pixel's 8 words `a`, channel `ch`, with the divisor `samples` ----
template <typename T>
__device__ __forceinline__ T resolve_value(const unsigned long long *__restrict__ a, unsigned ch, int samples, int gamma) {
    double v = rtw::fx_to_double(a[2 * ch], a[2 * ch + 1]);
    if (a[6] != 0ull) v = __builtin_nan("");
    v = v / (double)samples;
    if (gamma) v = __builtin_sqrt(v);
    return (T)v;
}
// the samples the tile of pixel (i, j) of an adaptive accumulator holds: min(spp, C_t * chunk_spp)
__device__ __forceinline__ int tile_samples(const int *__restrict__ chunks, size_t i, size_t j, int tiles_i, int spp, int chunk_spp) {
    const long long held = (long long)chunks[(j >> 3) * (size_t)tiles_i + (i >> 3)] * chunk_spp;
    return held < spp ? (int)held : spp;
}

// accumulator -> RGB{T} frame; lane = (pixel, channel)
template <typename T>
__global__ __launch_bounds__(256) void accum_resolve_kernel(const unsigned long long *__restrict__ words, T *__restrict__ out, size_t n_elems, int samples, int gamma) {
    const size_t k = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= n_elems) return;
    const size_t pix = k / 3u;
    const unsigned ch = (unsigned)(k - pix * 3u);
    out[k] = resolve_value<T>(words + pix * 8u, ch, samples, gamma);
}
// ... for an adaptive accumulator: a pixel is divided by the samples ITS TILE holds
template <typename T>
__global__ __launch_bounds__(256) void accum_resolve_tiles_kernel(const unsigned long long *__restrict__ words, T *__restrict__ out, size_t n_elems, const int *__restrict__ chunks,
                                                                  int height, int tiles_i, int spp, int chunk_spp, int gamma) {
    const size_t k = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= n_elems) return;
    const size_t pix = k / 3u;
    const unsigned ch = (unsigned)(k - pix * 3u);
    const size_t j = pix / (size_t)height, i = pix - j * (size_t)height;
    const int samples = tile_samples(chunks, i, j, tiles_i, spp, chunk_spp);
    out[k] = resolve_value<T>(words + pix * 8u, ch, samples, gamma);
}

// ---- adaptive render: the tile kernels (plain vector loads, stores and shuffles; tiles are numbered t = tj * tiles_i + ti) ----
// The stopping rule of include/rtw_hip.h at checkpoint `c`, one wave per tile, lane = the pixel (i mod 8) + 8 (j mod 8): flags[t] = 1 for
// a tile that holds exactly c chunks and is NOT converged (it stays active), 0 for every other tile.  D and Y are summed sequentially in
// lane order by every lane (64 shuffles each): the written rule's own order, so the result does not depend on how a reduction would
// associate.  n = (double)(c * chunk_spp).
// (tile_not_converged: the rule itself for tile t of one frame, whole wave, the same value in every lane -- shared with the batched check)
__device__ __forceinline__ int tile_not_converged(const unsigned long long *__restrict__ words, int t, unsigned lane, int tiles_i, int width, int height, double n, double tol, double floor) {
    const int tj = t / tiles_i, ti = t - tj * tiles_i;
    const int i = ti * 8 + (int)(lane & 7u), j = tj * 8 + (int)(lane >> 3);
    const bool valid = i < height && j < width;
    double d = 0.0, y = 0.0;
    if (valid) {
        const unsigned long long *a = words + ((size_t)j * (size_t)height + (size_t)i) * 8u;
        if (a[6] == 0ull) {
            const long long h = (long long)a[7];
            const unsigned long long m = h < 0 ? 0ull - (unsigned long long)h : (unsigned long long)h;
            d = (double)m * 0x1p-24;                  // (exact scaling)
            y = (rtw::fx_to_double(a[0], a[1]) + rtw::fx_to_double(a[2], a[3])) + rtw::fx_to_double(a[4], a[5]);
            y = y > 0.0 ? y : 0.0;
        }
    }
    const double npix = (double)__popcll(__ballot(valid));
    double D = 0.0, Y = 0.0;
    for (int k = 0; k < 64; ++k) { D = D + __shfl(d, k); Y = Y + __shfl(y, k); }
    const double dark = (floor * n) * npix;
    const double M = Y > dark ? Y : dark;
    return D <= tol * M ? 0 : 1;
}
__global__ __launch_bounds__(256) void accum_tile_check_kernel(const unsigned long long *__restrict__ words, const int *__restrict__ chunks, int *__restrict__ flags,
                                                               int n_tiles, int tiles_i, int width, int height, int c, double n, double tol, double floor) {
    const unsigned lane = threadIdx.x & 63u;
    const int t = (int)(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (t >= n_tiles) return;                         // (whole waves: no barrier below)
    if (chunks[t] != c) { if (lane == 0) flags[t] = 0; return; }
    const int f = tile_not_converged(words, t, lane, tiles_i, width, height, n, tol, floor);
    if (lane == 0) flags[t] = f;
}

// ---- the same for a batch of N views (rtw_render_adaptive_batch_*): batch-global tile g = v * n_tiles + t, view v's words and C_t ----
// one wave per (view, tile): tile_not_converged on view v's words
__global__ __launch_bounds__(256) void accum_tile_check_batch_kernel(const TileView *__restrict__ views, int *__restrict__ flags, int n_views, int n_tiles, int tiles_i,
                                                                     int width, int height, int c, double n, double tol, double floor) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned g = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (g >= (unsigned)n_views * (unsigned)n_tiles) return;      // (whole waves: no barrier below)
    const unsigned v = g / (unsigned)n_tiles;
    const int t = (int)(g - v * (unsigned)n_tiles);
    const TileView V = views[v];
    if (V.chunks[t] != c) { if (lane == 0) flags[g] = 0; return; }
    const int f = tile_not_converged(V.words, t, lane, tiles_i, width, height, n, tol, floor);
    if (lane == 0) flags[g] = f;
}
// The batch's list in three small launches instead of one workgroup's loop over N * n_tiles flags (accum_tile_compact_kernel: a chain of
// n / 1024 dependent steps): blocks of 256 flags are counted, ONE workgroup turns the counts into offsets (and the total into *count), the
// blocks write their tiles behind their offsets.  The order is the flags' order, so the list is the one the loop makes: sorted.
__global__ __launch_bounds__(256) void accum_tile_count_kernel(const int *__restrict__ flags, int *__restrict__ block_n, int n) {
    __shared__ int wave_n[4];
    const int t = (int)(blockIdx.x * 256u + threadIdx.x);
    const bool f = t < n && flags[t] != 0;
    const unsigned long long m = __ballot(f);
    if ((threadIdx.x & 63u) == 0u) wave_n[threadIdx.x >> 6] = (int)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) block_n[blockIdx.x] = (wave_n[0] + wave_n[1]) + (wave_n[2] + wave_n[3]);
}
// counts -> exclusive prefix sums, in place; one workgroup, 1024 counts per step
__global__ __launch_bounds__(1024) void accum_tile_scan_kernel(int *__restrict__ block_n, int *__restrict__ count, int nb) {
    __shared__ int wave_s[16];
    __shared__ int base;
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nb; b0 += 1024) {
        const int b = b0 + (int)threadIdx.x;
        const int v = b < nb ? block_n[b] : 0;
        int x = v;                                    // inclusive sums within the wave
        for (unsigned d = 1; d < 64u; d <<= 1) { const int y = __shfl_up(x, d); if (lane >= d) x += y; }
        if (lane == 63u) wave_s[wave] = x;
        __syncthreads();
        int off = base;
        for (unsigned k = 0; k < wave; ++k) off += wave_s[k];
        if (b < nb) block_n[b] = off + x - v;
        __syncthreads();
        if (threadIdx.x == 0) { int s = 0; for (int k = 0; k < 16; ++k) s += wave_s[k]; base += s; }
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = base;
}
__global__ __launch_bounds__(256) void accum_tile_scatter_kernel(const int *__restrict__ flags, const int *__restrict__ block_off, int *__restrict__ list, int n) {
    __shared__ int wave_n[4];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const int t = (int)(blockIdx.x * 256u + threadIdx.x);
    const bool f = t < n && flags[t] != 0;
    const unsigned long long m = __ballot(f);
    if (lane == 0u) wave_n[wave] = (int)__popcll(m);
    __syncthreads();
    if (f) {
        int off = block_off[blockIdx.x];
        for (unsigned k = 0; k < wave; ++k) off += wave_n[k];
        list[off + (int)__popcll(m & ((1ull << lane) - 1ull))] = t;
    }
}
// after a pass of `add` chunks: C_t += add in each listed tile's OWN view (list == null: for all n = N * n_tiles tiles)
__global__ __launch_bounds__(256) void accum_tile_advance_batch_kernel(const int *__restrict__ list, int n, const TileView *__restrict__ views, int n_tiles, int add) {
    const int k = (int)(blockIdx.x * 256u + threadIdx.x);
    if (k >= n) return;
    const unsigned g = (unsigned)(list ? list[k] : k), v = g / (unsigned)n_tiles;
    views[v].chunks[g - v * (unsigned)n_tiles] += add;
}

// flags -> the SORTED list of the active tiles + its length, one workgroup: ascending tile numbers keep what the sharded path's queues
// give a shard -- consecutive list entries are neighbours in the frame, local tile k goes to die k mod 8, and a die works through its
// part of the list in frame order -- and make the list, like everything else here, the same from run to run (an atomic append would
// finish a few microseconds sooner and order the list by arrival).
__global__ __launch_bounds__(1024) void accum_tile_compact_kernel(const int *__restrict__ flags, int *__restrict__ list, int *__restrict__ count, int n_tiles) {
    __shared__ int wave_n[16];
    __shared__ int base;
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    for (int t0 = 0; t0 < n_tiles; t0 += 1024) {
        const int t = t0 + (int)threadIdx.x;
        const bool f = t < n_tiles && flags[t] != 0;
        const unsigned long long m = __ballot(f);
        if (lane == 0) wave_n[wave] = (int)__popcll(m);
        __syncthreads();
        int off = base;
        for (unsigned k = 0; k < wave; ++k) off += wave_n[k];
        if (f) list[off + (int)__popcll(m & ((1ull << lane) - 1ull))] = t;
        __syncthreads();
        if (threadIdx.x == 0) { int n = 0; for (int k = 0; k < 16; ++k) n += wave_n[k]; base += n; }
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = base;
}

// after a pass of `add` chunks: C_t += add for the tiles of the list (list == null: for all n tiles)
__global__ __launch_bounds__(256) void accum_tile_advance_kernel(const int *__restrict__ list, int n, int *__restrict__ chunks, int add) {
    const int k = (int)(blockIdx.x * 256u + threadIdx.x);
    if (k >= n) return;
    chunks[list ? list[k] : k] += add;
}

// ---- the noise map of an adaptive accumulator (include/rtw_hip.h rtw_accum_noise_*) ----
// rho of one pixel: the stopping rule's D / M for the pixel alone, n = the samples ITS tile holds.  false: the pixel is poisoned.
__device__ __forceinline__ bool pixel_rho(const unsigned long long *__restrict__ words, const int *__restrict__ chunks, size_t i, size_t j, int height, int tiles_i, int spp,
                                          int chunk_spp, double floor, double *rho) {
    const unsigned long long *a = words + (j * (size_t)height + i) * 8u;
    if (a[6] != 0ull) return false;
    const double n = (double)tile_samples(chunks, i, j, tiles_i, spp, chunk_spp);
    const long long h = (long long)a[7];
    const unsigned long long m = h < 0 ? 0ull - (unsigned long long)h : (unsigned long long)h;
    const double D = (double)m * 0x1p-24;                  // (exact scaling)
    double y = (rtw::fx_to_double(a[0], a[1]) + rtw::fx_to_double(a[2], a[3])) + rtw::fx_to_double(a[4], a[5]);
    y = y > 0.0 ? y : 0.0;
    const double dark = floor * n;
    const double M = y > dark ? y : dark;
    *rho = M > 0.0 ? D / M : 0.0;
    return true;
}
// the map's value at pixel (i, j): the 3 x 3 binomial mean of rho over the neighbours inside the frame that are not poisoned, dj outer, di
// inner, both sums sequential; a poisoned centre is a quiet NaN.  Reads only; no LDS, no atomics, no cross-lane operation.
__device__ __forceinline__ double noise_value(const unsigned long long *__restrict__ words, const int *__restrict__ chunks, size_t i, size_t j, int width, int height, int tiles_i,
                                              int spp, int chunk_spp, double floor) {
    double rho;
    if (!pixel_rho(words, chunks, i, j, height, tiles_i, spp, chunk_spp, floor, &rho)) return __builtin_nan("");
    double num = 0.0, den = 0.0;
    for (int dj = -1; dj <= 1; ++dj)
        for (int di = -1; di <= 1; ++di) {
            const long long qi = (long long)i + di, qj = (long long)j + dj;
            if (qi < 0 || qi >= height || qj < 0 || qj >= width) continue;
            double r;
            if (!pixel_rho(words, chunks, (size_t)qi, (size_t)qj, height, tiles_i, spp, chunk_spp, floor, &r)) continue;
            const double b = (double)((di == 0 ? 2 : 1) * (dj == 0 ? 2 : 1));
            num = num + b * r;
            den = den + b;
        }
    return num / den;
}
// one pixel per lane, lanes along i
template <typename T>
__global__ __launch_bounds__(256) void accum_noise_kernel(const unsigned long long *__restrict__ words, const int *__restrict__ chunks, T *__restrict__ out, int width, int height,
                                                          int tiles_i, int spp, int chunk_spp, double floor) {
    const size_t p = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (p >= (size_t)width * (size_t)height) return;
    const size_t j = p / (size_t)height, i = p - j * (size_t)height;
    out[p] = (T)noise_value(words, chunks, i, j, width, height, tiles_i, spp, chunk_spp, floor);
}

// ---- the read-only passes over a batch of N accumulators of one size (rtw_accum_resolve_batch_*, rtw_accum_noise_batch_*): ONE launch over
// the views' elements, flat element g = v * (elements of a view) + k; view v is read through a device table (ReadView) and written at
// out + v * (elements of a view) ----
// element k of view v = accum_resolve_tiles_kernel's (adaptive) or accum_resolve_kernel's (uniform) of that view
template <typename T>
__global__ __launch_bounds__(256) void accum_resolve_batch_kernel(const ReadView *__restrict__ views, T *__restrict__ out, size_t view_elems, size_t n_elems, int height, int tiles_i, int gamma) {
    const size_t g = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (g >= n_elems) return;
    const size_t view = g / view_elems, k = g - view * view_elems;
    const ReadView V = views[view];
    const size_t pix = k / 3u;
    const unsigned ch = (unsigned)(k - pix * 3u);
    int samples = V.samples;
    if (V.chunks) {
        const size_t j = pix / (size_t)height, i = pix - j * (size_t)height;
        samples = tile_samples(V.chunks, i, j, tiles_i, V.spp, V.chunk_spp);
    }
    out[g] = resolve_value<T>(V.words + pix * 8u, ch, samples, gamma);
}
// pixel p of view v = accum_noise_kernel's of that view, every neighbour bounded by the view's own frame
template <typename T>
__global__ __launch_bounds__(256) void accum_noise_batch_kernel(const ReadView *__restrict__ views, T *__restrict__ out, size_t n_pix, int width, int height, int tiles_i, int spp,
                                                                int chunk_spp, double floor) {
    const size_t g = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (g >= n_pix) return;
    const size_t view_pix = (size_t)width * (size_t)height, view = g / view_pix, p = g - view * view_pix;
    const size_t j = p / (size_t)height, i = p - j * (size_t)height;
    out[g] = (T)noise_value(views[view].words, views[view].chunks, i, j, width, height, tiles_i, spp, chunk_spp, floor);
}

}  // namespace

// ---- the launches (rtw_accum.hpp) ----
int tiles_down(int height) { return (height + 7) / 8; }
int tiles_of(int width, int height) { return tiles_down(height) * ((width + 7) / 8); }
void launch_merge(hipStream_t stream, unsigned long long *dst, const unsigned long long *src, size_t n_pixels) {
    const size_t n = n_pixels * 4u;
    hipLaunchKernelGGL(accum_merge_kernel, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, stream, reinterpret_cast<ulonglong2 *>(dst), reinterpret_cast<const ulonglong2 *>(src), n);
}
void launch_tile_check(hipStream_t stream, const unsigned long long *words, const int *chunks, int *flags, int width, int height, int c, int cs, double tol, double floor) {
    const int n_tiles = tiles_of(width, height);
    hipLaunchKernelGGL(accum_tile_check_kernel, dim3((unsigned)((n_tiles + 3) / 4)), dim3(256), 0, stream, words, chunks, flags, n_tiles, tiles_down(height),
                       width, height, c, (double)((long long)c * cs), tol, floor);
}
void launch_tile_check_batch(hipStream_t stream, const TileView *d_views, int *flags, int n_views, int width, int height, int c, int cs, double tol, double floor) {
    const int n_tiles = tiles_of(width, height);
    const long long n_all = (long long)n_views * n_tiles;
    hipLaunchKernelGGL(accum_tile_check_batch_kernel, dim3((unsigned)((n_all + 3) / 4)), dim3(256), 0, stream, d_views, flags, n_views, n_tiles, tiles_down(height),
                       width, height, c, (double)((long long)c * cs), tol, floor);
}
void launch_compact_loop(hipStream_t stream, const int *flags, int *list, int *count, int n) {
    hipLaunchKernelGGL(accum_tile_compact_kernel, dim3(1), dim3(1024), 0, stream, flags, list, count, n);
}
int compact_blocks(long long n) { return (int)((n + 255) / 256); }
void launch_compact_blocks(hipStream_t stream, const int *flags, int *blocks, int *list, int *count, int n) {
    const int n_blocks = compact_blocks(n);
    hipLaunchKernelGGL(accum_tile_count_kernel, dim3((unsigned)n_blocks), dim3(256), 0, stream, flags, blocks, n);
    hipLaunchKernelGGL(accum_tile_scan_kernel, dim3(1), dim3(1024), 0, stream, blocks, count, n_blocks);
    hipLaunchKernelGGL(accum_tile_scatter_kernel, dim3((unsigned)n_blocks), dim3(256), 0, stream, flags, blocks, list, n);
}
void launch_tile_advance(hipStream_t stream, const int *list, int n, int *chunks, int add) {
    hipLaunchKernelGGL(accum_tile_advance_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, list, n, chunks, add);
}
void launch_tile_advance_batch(hipStream_t stream, const int *list, int n, const TileView *d_views, int n_tiles, int add) {
    hipLaunchKernelGGL(accum_tile_advance_batch_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, list, n, d_views, n_tiles, add);
}
template <typename T>
void launch_resolve(hipStream_t stream, const unsigned long long *words, T *d_out, int width, int height, int samples, int gamma) {
    const size_t n = (size_t)width * (size_t)height * 3u;
    hipLaunchKernelGGL(accum_resolve_kernel<T>, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, stream, words, d_out, n, samples, gamma);
}
template <typename T>
void launch_resolve_tiles(hipStream_t stream, const unsigned long long *words, T *d_out, const int *chunks, int width, int height, int spp, int chunk_spp, int gamma) {
    const size_t n = (size_t)width * (size_t)height * 3u;
    hipLaunchKernelGGL(accum_resolve_tiles_kernel<T>, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, stream, words, d_out, n, chunks, height, tiles_down(height),
                       spp, chunk_spp, gamma);
}
template <typename T>
void launch_noise(hipStream_t stream, const unsigned long long *words, T *d_out, const int *chunks, int width, int height, int spp, int chunk_spp, double floor) {
    const size_t n = (size_t)width * (size_t)height;
    hipLaunchKernelGGL(accum_noise_kernel<T>, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, stream, words, chunks, d_out, width, height, tiles_down(height), spp, chunk_spp, floor);
}
template <typename T>
void launch_resolve_batch(hipStream_t stream, const ReadView *d_views, T *d_out, int n_views, int width, int height, int gamma) {
    const size_t view_elems = (size_t)width * (size_t)height * 3u, n = view_elems * (size_t)n_views;
    hipLaunchKernelGGL(accum_resolve_batch_kernel<T>, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, stream, d_views, d_out, view_elems, n, height, tiles_down(height), gamma);
}
template <typename T>
void launch_noise_batch(hipStream_t stream, const ReadView *d_views, T *d_out, int n_views, int width, int height, int spp, int chunk_spp, double floor) {
    const size_t n = (size_t)width * (size_t)height * (size_t)n_views;
    hipLaunchKernelGGL(accum_noise_batch_kernel<T>, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, stream, d_views, d_out, n, width, height, tiles_down(height), spp, chunk_spp, floor);
}
RTW_ACCUM_LAUNCH_INSTANCES(template, float)
RTW_ACCUM_LAUNCH_INSTANCES(template, double)

namespace {

// ---- the unit ops 21-23, 25, 30, 31 (include/rtw_hip.h rtw_unit_f32 / _f64; tests/test_gpu_accum_kernels.py, test_gpu_accum_denoise.py,
// test_gpu_accum_filter_batch.py): the kernels above on the caller's words ----
// A test seam like the other rtw_unit ops: host slots in, host slots out, the null stream, blocking copies, one device allocation that is
// freed on return.  Everything is validated before the first HIP call: nulls -1; a size or a value the layout does not hold, or a call
// of more than RTW_ACCUM_UNIT_SLOTS input slots, -2.  The kernels run through the launches of the host paths.
#define RTW_ACCUM_UNIT_SLOTS (1ll << 24)         // 128 MiB of 8-byte slots
#define RTW_ACCUM_UNIT_PIXELS (1ll << 20)        // ... and frames of at most this many pixels, 16384 on a side
struct DevBuf { void *p = nullptr; ~DevBuf() { if (p) HIP_IGNORE(hipFree(p)); } };
size_t up16(size_t b) { return (b + 15u) / 16u * 16u; }
// a slot that holds an integer of [lo, hi] as a binary64 value
bool slot_int(double d, long long lo, long long hi, int *out) {
    if (!(d >= (double)lo && d <= (double)hi) || d != std::floor(d)) return false;
    *out = (int)d;
    return true;
}
bool slot_floor(double d) { return std::isfinite(d) && d >= 0.0; }
int unit_device() {
    int dev;
    if (int rc = resolve_device(-1, &dev)) return rc;
    HIP_TRY(hipSetDevice(dev));
    return 0;
}

// The one layout of the ops that take frames: in = width, height, c (op 21) or spp, chunk_spp, slot 4 [, slot 5], zeros up to slot 7 | per view:
// n_tiles x C_t, W * H * 8 raw words.  Slot 4: tolerance (op 21, with dark_floor in slot 5), gamma (23, 30) or dark_floor (25, 31).  count = the
// number of views; 23 and 25 take exactly one.  unit_stage parses and refuses, then -- the first HIP calls -- makes the call's one allocation:
// words | table | out | C_t, with the words and C_t of every view in place.  The table (n_views entries of `tab_entry` bytes) and the output
// (`outs` results of n_views x `per` elements of `elem` bytes) are the op's to fill.
struct UnitStage {
    int W, H, n, cs, gamma = 0;            // n: slot 2
    double tol = 0.0, floor = 0.0;
    long long n_tiles, n_words, n_all;     // of a view, of a view, tiles of all views
    size_t per, n_out;                     // output elements of one view in one result; of the call
    std::optional<DeviceGuard> guard;
    DevBuf buf;
    unsigned long long *d_words;           // view v: + v * n_words
    int32_t *d_chunks;                     //         + v * n_tiles
    void *d_tab, *d_out;
};
int unit_stage(int op, int n_views, const double *in, size_t tab_entry, size_t elem, UnitStage *u) {
    const bool check = op == 21, noise = op == 25 || op == 31, one_view = op == 23 || op == 25;
    if (one_view ? n_views != 1 : n_views < 1) return fail(-2, "unit op %d: count is %s (got %d)", op, one_view ? "1" : "the number of views", n_views);
    if (!slot_int(in[0], 1, 1 << 14, &u->W) || !slot_int(in[1], 1, 1 << 14, &u->H) || (long long)u->W * u->H > RTW_ACCUM_UNIT_PIXELS)
        return fail(-2, "accumulator unit op: a frame of %g x %g (at most 16384 on a side, %lld pixels)", in[0], in[1], RTW_ACCUM_UNIT_PIXELS);
    if (!slot_int(in[2], check ? 0 : 1, 0x7fffffff, &u->n) || !slot_int(in[3], 1, 0x7fffffff, &u->cs))
        return fail(-2, "unit op %d: %s %g, chunk_spp %g", op, check ? "checkpoint" : "spp", in[2], in[3]);
    if (check) { u->tol = in[4]; u->floor = in[5]; }
    else if (noise) u->floor = in[4];
    if (check ? !std::isfinite(u->tol) || !(u->tol > 0.0) || !slot_floor(u->floor) : noise ? !slot_floor(u->floor) : !slot_int(in[4], 0, 1, &u->gamma))
        return fail(-2, "unit op %d: %s %g", op, check ? "tolerance and dark_floor: slot 4" : noise ? "dark_floor" : "gamma", in[4]);
    for (int k = check ? 6 : 5; k < 8; ++k) if (in[k] != 0.0) return fail(-2, "unit op %d: header slot %d must be 0", op, k);
    const int W = u->W, H = u->H;
    u->n_tiles = tiles_of(W, H); u->n_words = (long long)W * H * 8; u->n_all = (long long)n_views * u->n_tiles;
    const long long stride = u->n_tiles + u->n_words;
    if (8 + (long long)n_views * stride > RTW_ACCUM_UNIT_SLOTS) return fail(-2, "unit op %d: %d views of %d x %d exceed %lld slots", op, n_views, W, H, RTW_ACCUM_UNIT_SLOTS);
    std::vector<int32_t> chunks((size_t)u->n_all);
    for (int v = 0; v < n_views; ++v)
        for (long long k = 0; k < u->n_tiles; ++k) {
            const double c = in[8 + (size_t)v * (size_t)stride + (size_t)k];
            if (!slot_int(c, check ? 0 : 1, 0x7fffffff, &chunks[(size_t)v * (size_t)u->n_tiles + (size_t)k])) return fail(-2, "accumulator unit op: tile chunk count %g (view %d, slot %lld)", c, v, k);
        }
    u->per = check ? (size_t)u->n_tiles : (size_t)W * (size_t)H * (noise ? 1u : 3u);
    u->n_out = (one_view ? 1u : 2u) * (size_t)n_views * u->per;
    u->guard.emplace();
    if (int rc = unit_device()) return rc;
    const size_t words_b = (size_t)n_views * (size_t)u->n_words * 8u, tab_b = up16((size_t)n_views * tab_entry), out_b = up16(u->n_out * elem);
    HIP_TRY(hipMalloc(&u->buf.p, words_b + tab_b + out_b + (size_t)u->n_all * sizeof(int32_t)));
    char *base = static_cast<char *>(u->buf.p);
    u->d_words = reinterpret_cast<unsigned long long *>(base);
    u->d_tab = base + words_b;
    u->d_out = base + words_b + tab_b;
    u->d_chunks = reinterpret_cast<int32_t *>(base + words_b + tab_b + out_b);
    for (int v = 0; v < n_views; ++v)
        HIP_TRY(hipMemcpy(u->d_words + (size_t)v * (size_t)u->n_words, in + 8 + (size_t)v * (size_t)stride + (size_t)u->n_tiles, (size_t)u->n_words * 8u, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(u->d_chunks, chunks.data(), chunks.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    return 0;
}

// op 21: slot 2 = the checkpoint c; out (raw int64) = per view the n_tiles flags of accum_tile_check_kernel, launched view by view | the
// n_views * n_tiles flags of ONE accum_tile_check_batch_kernel launch.  A flag nobody wrote reads -1.
int unit_tile_check(int n_views, const double *in, long long *out) {
    UnitStage u;
    if (int rc = unit_stage(21, n_views, in, sizeof(TileView), sizeof(int32_t), &u)) return rc;
    TileView *d_views = static_cast<TileView *>(u.d_tab);
    int32_t *d_flags = static_cast<int32_t *>(u.d_out);
    std::vector<TileView> h_views((size_t)n_views);
    for (int v = 0; v < n_views; ++v) h_views[(size_t)v] = TileView{u.d_words + (size_t)v * (size_t)u.n_words, u.d_chunks + (size_t)v * (size_t)u.n_tiles};
    HIP_TRY(hipMemcpy(d_views, h_views.data(), (size_t)n_views * sizeof(TileView), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d_flags, 0xff, u.n_out * sizeof(int32_t)));
    (void)hipGetLastError();
    for (int v = 0; v < n_views; ++v) launch_tile_check(nullptr, h_views[(size_t)v].words, h_views[(size_t)v].chunks, d_flags + (size_t)v * u.per, u.W, u.H, u.n, u.cs, u.tol, u.floor);
    launch_tile_check_batch(nullptr, d_views, d_flags + u.n_all, n_views, u.W, u.H, u.n, u.cs, u.tol, u.floor);
    HIP_TRY(hipGetLastError());
    std::vector<int32_t> h(u.n_out);
    HIP_TRY(hipMemcpy(h.data(), d_flags, u.n_out * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < h.size(); ++k) out[k] = h[k];
    return 0;
}

// op 22: in = n slots whose low 32 bits are the flags; out (raw int64) = count, list[n] of accum_tile_compact_kernel | the same of count /
// scan / scatter.  Both lists are prefilled with -1: the slots behind the count read -1.
int unit_compact(int n, const unsigned long long *in, long long *out) {
    if (n < 1 || n > RTW_ACCUM_UNIT_SLOTS) return fail(-2, "unit op 22: count is the number of flags, 1 .. %lld (got %d)", RTW_ACCUM_UNIT_SLOTS, n);
    std::vector<int32_t> flags((size_t)n);
    for (int k = 0; k < n; ++k) flags[(size_t)k] = (int32_t)(uint32_t)in[k];
    DeviceGuard guard;
    if (int rc = unit_device()) return rc;
    const int n_blocks = compact_blocks(n);
    const size_t res = (size_t)n + 4u;                               // one result: list | count (+ 3 unused)
    DevBuf buf;
    HIP_TRY(hipMalloc(&buf.p, ((size_t)n + 2u * res + (size_t)n_blocks) * sizeof(int32_t)));
    int32_t *d_flags = static_cast<int32_t *>(buf.p), *d_res = d_flags + n, *d_blocks = d_res + 2u * res;
    HIP_TRY(hipMemcpy(d_flags, flags.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d_res, 0xff, 2u * res * sizeof(int32_t)));
    (void)hipGetLastError();
    launch_compact_loop(nullptr, d_flags, d_res, d_res + n, n);
    launch_compact_blocks(nullptr, d_flags, d_blocks, d_res + res, d_res + res + n, n);
    HIP_TRY(hipGetLastError());
    std::vector<int32_t> h(2u * res);
    HIP_TRY(hipMemcpy(h.data(), d_res, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int r = 0; r < 2; ++r) {
        long long *o = out + (size_t)r * ((size_t)n + 1u);
        const int32_t *s = h.data() + (size_t)r * res;
        o[0] = s[n];
        for (int k = 0; k < n; ++k) o[1 + k] = s[k];
    }
    return 0;
}

// ops 23 / 25 and 30 / 31: the per-tile resolve / the noise map, slot 2 = spp, every C_t >= 1.  With E = W * H * 3 (resolve) or W * H (noise): out =
// per view the E values of the single kernel (accum_resolve_tiles_kernel / accum_noise_kernel), launched view by view [ | ops 30 / 31: the
// n_views * E values of ONE launch of the batch kernel]; each of type T, widened to binary64.  An element nobody wrote reads -7.
template <typename T>
int unit_read(int op, int n_views, const double *in, double *out) {
    const bool noise = op == 25 || op == 31, batch = op >= 30;
    UnitStage u;
    if (int rc = unit_stage(op, n_views, in, sizeof(ReadView), sizeof(T), &u)) return rc;
    ReadView *d_views = static_cast<ReadView *>(u.d_tab);
    T *d_out = static_cast<T *>(u.d_out);
    std::vector<ReadView> h_views((size_t)n_views);
    for (int v = 0; v < n_views; ++v) h_views[(size_t)v] = ReadView{u.d_words + (size_t)v * (size_t)u.n_words, u.d_chunks + (size_t)v * (size_t)u.n_tiles, 0, u.n, u.cs, 0};
    std::vector<T> h(u.n_out, (T)-7);
    HIP_TRY(hipMemcpy(d_views, h_views.data(), (size_t)n_views * sizeof(ReadView), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_out, h.data(), u.n_out * sizeof(T), hipMemcpyHostToDevice));
    (void)hipGetLastError();
    for (int v = 0; v < n_views; ++v) {
        const ReadView &V = h_views[(size_t)v];
        if (noise) launch_noise<T>(nullptr, V.words, d_out + (size_t)v * u.per, V.chunks, u.W, u.H, u.n, u.cs, u.floor);
        else launch_resolve_tiles<T>(nullptr, V.words, d_out + (size_t)v * u.per, V.chunks, u.W, u.H, u.n, u.cs, u.gamma);
    }
    if (batch && noise) launch_noise_batch<T>(nullptr, d_views, d_out + (size_t)n_views * u.per, n_views, u.W, u.H, u.n, u.cs, u.floor);
    else if (batch) launch_resolve_batch<T>(nullptr, d_views, d_out + (size_t)n_views * u.per, n_views, u.W, u.H, u.gamma);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(h.data(), d_out, u.n_out * sizeof(T), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < u.n_out; ++k) out[k] = (double)h[k];
    return 0;
}

}  // namespace

int accum_unit(int op, bool f64, int count, const void *in, void *out) {
    if (!in || !out) return fail(-1, "null argument");
    if (op != 23 && op != 25 && op != 30 && op != 31 && !f64) return fail(-2, "unit op %d is an op of rtw_unit_f64", op);
    switch (op) {
        case 21: return unit_tile_check(count, static_cast<const double *>(in), static_cast<long long *>(out));
        case 22: return unit_compact(count, static_cast<const unsigned long long *>(in), static_cast<long long *>(out));
        case 23: case 25: case 30: case 31: return f64 ? unit_read<double>(op, count, static_cast<const double *>(in), static_cast<double *>(out))
                                                       : unit_read<float>(op, count, static_cast<const double *>(in), static_cast<double *>(out));
    }
    return fail(-2, "unknown unit op %d", op);
}

}  // namespace rtwh
