// rtw_accum.hpp -- what the two accumulator units share (internal, like rtw_host.hpp): the accumulator object (rtw_accum.hip owns it) and the
// launches of the accumulator's kernels (rtw_accum_kernels.hip defines them and the kernels; it never looks into the object).
#pragma once
#include "rtw_host.hpp"

#pragma GCC visibility push(hidden)

// what an accumulator is bound to by its first pass: everything that decides the value of a sample
struct AccumBind {
    int32_t is_f64, spp, chunk_spp, n_chunks, max_depth, numerics;
    uint64_t seed, scene_hash;
    unsigned char cam[sizeof(rtw_camera_f64)];     // the camera's bytes (Float32: the first half, the rest 0)
};

struct rtw_accum {
    int device = -1;
    int32_t width = 0, height = 0;
    unsigned long long *words = nullptr;           // device memory: width * height * 8
    hipEvent_t ev = nullptr;                       // behind the last operation enqueued on `words`
    bool bound = false;
    AccumBind bind;
    std::vector<std::pair<int32_t, int32_t>> ranges;    // chunk ranges [begin, end) already added: sorted, disjoint, coalesced
                                                        // (adaptive: the one prefix [0, min C_t) -- what the least sampled tile holds)
    // ---- adaptive accumulators (rtw_render_adaptive_*): tile t holds the chunks [0, C_t) ----
    bool adaptive = false;
    bool ad_complete = false;                      // no tile is active under ad.tolerance (false only after a call that failed half way)
    rtw_adaptive_t ad;                             // the last call's, min_chunks / check_chunks as their effective values
    int32_t ad_rounds = 0;                         // passes of the last call that held one of its tiles
    int32_t *d_tiles = nullptr;                    // device memory, 3 n_tiles + 4 int32: C_t | active flags | active list | count (made by the first adaptive call)
    std::vector<int32_t> tile_chunks;              // host copy of C_t, read back at the end of every call
    // ---- the view table of a batched read-only pass (rtw_accum_resolve_batch_* / rtw_accum_noise_batch_*) whose FIRST accumulator this is ----
    void *d_tab = nullptr, *h_tab = nullptr;       // device table; pinned staging of its H2D
    size_t tab_cap = 0, tab_bytes = 0;             // tab_bytes: how much of h_tab the device table is known to hold (0: nothing -- stage it)
    hipEvent_t tab_ev = nullptr;                   // behind the last H2D out of h_tab
};

namespace rtwh {

// one view of a batch, as the batched kernels read it from a device-resident table
struct TileView { const unsigned long long *words; int *chunks; };      // the tile kernels: view v's words and C_t
// the read-only passes.  chunks null: a uniform accumulator, `samples` is its divisor; else an adaptive one, its C_t array and its render's spp / chunk size
struct ReadView { const unsigned long long *words; const int *chunks; int samples, spp, chunk_spp, pad; };

// ---- the launches of the accumulator's kernels (rtw_accum_kernels.hip): the host paths of rtw_accum.hip and the unit ops (accum_unit) all go
// through these, so the test seam runs the product's kernels with the product's grids.  (enqueue only: the caller clears and reads
// hipGetLastError around them.)  Tiles are 8 x 8 pixels, numbered t = tj * tiles_i + ti. ----
int tiles_down(int height);
int tiles_of(int width, int height);
// dst += src, both of n_pixels pixels
void launch_merge(hipStream_t stream, unsigned long long *dst, const unsigned long long *src, size_t n_pixels);
// the check at checkpoint `c` of ONE frame: flags[t] for its tiles (n handed to the rule: the samples of c chunks of `cs`)
void launch_tile_check(hipStream_t stream, const unsigned long long *words, const int *chunks, int *flags, int width, int height, int c, int cs, double tol, double floor);
// ... of the n_views frames of a device-resident view table: flags[v * n_tiles + t]
void launch_tile_check_batch(hipStream_t stream, const TileView *d_views, int *flags, int n_views, int width, int height, int c, int cs, double tol, double floor);
// n flags -> the sorted list + its length: one workgroup's loop, or count / scan / scatter over compact_blocks(n) ints of scratch
void launch_compact_loop(hipStream_t stream, const int *flags, int *list, int *count, int n);
int compact_blocks(long long n);
void launch_compact_blocks(hipStream_t stream, const int *flags, int *blocks, int *list, int *count, int n);
// after a pass of `add` chunks: C_t += add for the n tiles of the list (list == null: for the first n tiles), batch-global tiles in their own views
void launch_tile_advance(hipStream_t stream, const int *list, int n, int *chunks, int add);
void launch_tile_advance_batch(hipStream_t stream, const int *list, int n, const TileView *d_views, int n_tiles, int add);

// launch_resolve: the frame of a uniform accumulator, every pixel over `samples`; launch_resolve_tiles: of an adaptive one, every pixel over the
// samples its tile holds; launch_noise: the noise map of a frame whose tile t holds C_t = chunks[t] >= 1 chunks; the _batch forms: of the n_views
// frames of a device-resident view table, view v at d_out + v * W * H * 3 (resolve) / v * W * H (noise).  T: the element type of d_out.
template <typename T> void launch_resolve(hipStream_t stream, const unsigned long long *words, T *d_out, int width, int height, int samples, int gamma);
template <typename T> void launch_resolve_tiles(hipStream_t stream, const unsigned long long *words, T *d_out, const int *chunks, int width, int height, int spp, int chunk_spp, int gamma);
template <typename T> void launch_noise(hipStream_t stream, const unsigned long long *words, T *d_out, const int *chunks, int width, int height, int spp, int chunk_spp, double floor);
template <typename T> void launch_resolve_batch(hipStream_t stream, const ReadView *d_views, T *d_out, int n_views, int width, int height, int gamma);
template <typename T> void launch_noise_batch(hipStream_t stream, const ReadView *d_views, T *d_out, int n_views, int width, int height, int spp, int chunk_spp, double floor);
// (instantiated for float and double in rtw_accum_kernels.hip: X = `extern template` here, `template` there)
#define RTW_ACCUM_LAUNCH_INSTANCES(X, T)                                                                                                  \
    X void launch_resolve<T>(hipStream_t, const unsigned long long *, T *, int, int, int, int);                                            \
    X void launch_resolve_tiles<T>(hipStream_t, const unsigned long long *, T *, const int *, int, int, int, int, int);                    \
    X void launch_noise<T>(hipStream_t, const unsigned long long *, T *, const int *, int, int, int, int, double);                         \
    X void launch_resolve_batch<T>(hipStream_t, const ReadView *, T *, int, int, int, int);                                                \
    X void launch_noise_batch<T>(hipStream_t, const ReadView *, T *, int, int, int, int, int, double);
RTW_ACCUM_LAUNCH_INSTANCES(extern template, float)
RTW_ACCUM_LAUNCH_INSTANCES(extern template, double)

}  // namespace rtwh

#pragma GCC visibility pop
