// rtw_launch.hip -- one render = ONE launch of the trace kernel (rtw_kernels.hpp; opt-in: the ray-pool kernel of rtw_pool.hpp).  launch_render
// reads top to bottom: validate, parameters, scene view (rtw_scene_view.hpp), instance (rtw_instances.hpp), occupancy, job shape, record
// (rtw_host.hpp begin_record / run_record), views, launch; its own steps are the static functions in front of it.  Behind it: resolve_rec.
#include "rtw_scene_view.hpp"
#include "rtw_kernels.hpp"
#include "rtw_instances.hpp"
#ifdef RTW_WITH_POOL          // `make POOL=1`: the ray-pool kernel (a measured 16 - 19 % LOSS on this chip, DESIGN_LOG R4) is not in the default library
#include "rtw_pool.hpp"
template <typename T> using pool_kern_t = void (*)(rtw::KParams, rtw::Camera<T>, rtw::DevScene<T>, T *, rtw::DevCounters *);
#endif

namespace rtwh {

// magic number for exact unsigned 32-bit division by an invariant d >= 1 (Granlund-Montgomery / Hacker's
// Delight "add" form): n / d == (umulhi(n, m) + ((n - umulhi(n, m)) >> 1)) >> s for all 32-bit n
void make_udiv(unsigned d, unsigned *m, unsigned *s) {
    if (d <= 1) { *m = 0; *s = 0x80000000u; return; }   // flag: identity
    unsigned l = 0;
    while ((1ull << l) < d) ++l;                        // l = ceil(log2 d) >= 1
    *m = (unsigned)((((1ull << l) - d) << 32) / d + 1);
    *s = l - 1;
}

// The ray-pool kernel (rtw_pool.hpp; opt-in: RTW_FLAG_RAY_POOL, or RTW_POOL=1 in the environment for A/B runs) exists in `make POOL=1`
// builds only: `eligible` launches (Float32 plain scans on the matrix pipe, no batch, no pass), when the pool, the rings and the scene copy fit the
// 160 KB of LDS of a CU (one workgroup of RTW_POOL_W waves per CU); everything else runs the lane-loop kernel.  The default library refuses the flag.
struct PoolChoice { bool use = false; const void *kern = nullptr; size_t lds = 0; int block_threads = 256, blocks_per_cu = 0; };
template <typename T>
static int choose_pool(const DeviceCtx *ctx, const rtw_scene_dev *scene, const rtw_params *p, int cs, bool eligible, bool phase_profile, PoolChoice *pool) {
#ifdef RTW_WITH_POOL
    static const bool env_pool = aid_flag("RTW_POOL");
    if constexpr (sizeof(T) == 4) {
        pool->lds = rtw::pool_fixed_lds_bytes<T, RTW_POOL_W, RTW_POOL_R>() + rtw::pool_scene_lds_bytes<T>(scene->n, scene->n_pad);
        pool->use = eligible && (env_pool || (p->flags & RTW_FLAG_RAY_POOL)) && pool->lds <= ctx->lds_per_cu && cs <= RTW_POOL_MAX_CHUNK_SPP;
        pool->kern = phase_profile ? (const void *)rtw::trace_pool_kernel<T, RTW_POOL_W, RTW_POOL_R, true> : (const void *)rtw::trace_pool_kernel<T, RTW_POOL_W, RTW_POOL_R, false>;
    }
    if (pool->use) {
        pool->block_threads = RTW_POOL_W * 64;
        // "everything else runs the lane-loop kernel": also a device (or a runtime) that refuses this much dynamic LDS
        hipError_t e = hipFuncSetAttribute(pool->kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pool->lds);
        if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&pool->blocks_per_cu, pool->kern, pool->block_threads, pool->lds);
        if (e != hipSuccess || pool->blocks_per_cu < 1) { (void)hipGetLastError(); pool->use = false; pool->block_threads = 256; pool->blocks_per_cu = 0; }
    }
#else
    if (p->flags & RTW_FLAG_RAY_POOL)
        return fail(-7, "RTW_FLAG_RAY_POOL: this build of librtw_hip has no ray-pool kernel (a measured loss on MI355X; `make POOL=1` builds it in)");
#endif
    return 0;
}

// The job shape of a launch over `n_local` tiles and `nch` chunks with `grid` workgroups at full occupancy (tiles_i x tiles_j, shard_count: as
// the kernel sees them -- a batch's columns side by side, 0 shards for a tile list): a pure function of its arguments.  (ShapeAids: the aids of A/B
// runs, tools/gpu_ab.sh -- RTW_JOB_PIXELS = 1, 4, 8 or 16, else ignored; RTW_ROWS_SHIFT; RTW_GRID_BLOCKS caps the persistent grid: fewer waves per SIMD)
struct ShapeAids { int job_pixels, rows_shift; long long grid_blocks; };
struct JobShape { int job_shift, rows_shift; unsigned slot_stride, n_slots; long long total_jobs, bpj, grid; };
static int job_shape(int nch, long long n_local, int tiles_i, int tiles_j, int shard_count, long long grid, int job_pixels, bool pool, const ShapeAids &aids, JobShape *out) {
    // Job size.  A job is owned by one workgroup, so its size sets the end-of-queue drain; smaller jobs also store the
    // image in smaller pieces (more partial-line writes).  2x2 pixels (a batch = 4 pixels x 16 chunks) when the chunks
    // fill such batches, else 4x4 (x 4 chunks); ONE pixel (x 64 chunks) when a workgroup would otherwise see fewer than
    // 150 jobs (small frames, shards of a multi-GPU render).  Measured at 1080p x 1000 spp / 250 chunks
    // (tools/gpu_drain.py): drain 4.4 / 9.7 / 30 ms of idle wave slots for 1 / 4 / 16-pixel jobs; full frame 859 / 859 /
    // 871 ms; a 1/8 shard 115.6 / 119.8 / 137.7 ms; HBM writes 148 / 72 / 45 MB per frame.
    // (Slots per workgroup: 24 / 12 / 4 -- one-pixel jobs need many slots in flight; with 6 they ran 33 % slower.)
    // Round 6, with out-of-order job slots and static first claims (tools/gpu_small_sweep.sh, kernel us for 1 / 4 / 8 / 16 pixels):
    //   1/8 shard of 1080p x 1000 spp (250 chunks)   51.1 / 53.0 / -- / 73.8 ms      one-pixel jobs: the shortest drain
    //   1/8 shard of 1080p x 64 spp (64 chunks)      4.28 / 4.08 / -- / 5.22 ms      (1 pixel x 64 chunks = ONE batch per job: every batch opens a job)
    //   320 x 180 x 64 spp (64 chunks; 11 jobs of 4 pixels per workgroup)            1008 / 838 / 1002 / 997 us
    //   200 x 112 x 32 spp Float64 (32 chunks; 5 per workgroup)                      572 / 377 / 419 / 334 us
    //   96 x 54 x 16 spp (16 chunks; 1 per workgroup)                                527 / 155 / 91 / 58 us
    // -> one pixel only when its batches are many (>= 2 per job); the LARGEST jobs when a workgroup sees only a handful (a frame of
    //    a few hundred microseconds is a latency chain per wave: the fewest job openings win).
    int job_shift = nch >= 16 ? 2 : 4;
    if (nch >= 128 && n_local * 16 < 150 * grid) job_shift = 0;
    else if (n_local * 16 < 8 * grid) job_shift = 4;
    if (!job_pixels) job_pixels = aids.job_pixels;
    if (job_pixels == 16 || job_pixels == 8 || job_pixels == 4 || job_pixels == 1) {
        job_shift = job_pixels == 16 ? 4 : job_pixels == 8 ? 3 : job_pixels == 4 ? 2 : 0;
    } else if (job_pixels != 0) {
        return fail(-2, "job_pixels must be 0 (automatic), 1, 4, 8 or 16");
    }
    const long long total_jobs = n_local * (64 >> job_shift);
    const long long cpb = 64 >> job_shift;
    const long long bpj = (nch + cpb - 1) / cpb;
    // (claim_job packs a queue position into 28 bits; queue 0 is the longest: every 8th tile column, or every 8th tile of a shard)
    const long long queue0_jobs = (shard_count == 1 ? (long long)((tiles_j + 7) / 8) * tiles_i : (n_local + 7) / 8) * (64 >> job_shift);
    if (total_jobs >= (1ll << 30) || queue0_jobs >= (1ll << 28) || total_jobs * bpj >= (1ll << 40))
        return fail(-5, "render too large for one call: %lld pixel-block jobs", total_jobs);
    out->total_jobs = total_jobs; out->bpj = bpj; out->job_shift = job_shift;
    out->rows_shift = std::min(job_shift, 3);       // 4 x 1, 8 x 1, 8 x 2 pixels: whole column strips
    if (aids.rows_shift >= 0 && aids.rows_shift <= job_shift && aids.rows_shift <= 3 && job_shift - aids.rows_shift <= 2) out->rows_shift = aids.rows_shift;
    out->slot_stride = (unsigned)(sizeof(rtw::JobSlot) + 64u * (1u << job_shift));
    out->n_slots = std::min(24u, (unsigned)RTW_SLOT_BYTES / out->slot_stride);             // 24 / 12 / 7 / 4 slots of 1 / 4 / 8 / 16 pixels
    long long max_useful = (total_jobs * bpj + 3) / 4;                                             // one batch per wave, 4 waves per block
#ifdef RTW_WITH_POOL
    if (pool) max_useful = (total_jobs * bpj * 64 + RTW_POOL_R - 1) / RTW_POOL_R;                  // one item per slot of the pool
#endif
    if (grid > max_useful) grid = max_useful;
    if (aids.grid_blocks > 0 && grid > aids.grid_blocks) grid = aids.grid_blocks;
    out->grid = grid < 1 ? 1 : grid;
    return 0;
}

// A batch's views: the cameras and seeds go into the record's pinned buffer, then ONE asynchronous H2D on the render's stream (the record
// is handed out again only after ev2, behind this copy, so the pinned buffer is free whenever a render holds the record).
// (a batched pass: behind them the views' accumulators and divisors, rtw::AccumView; the batched feature pass over adaptive accumulators:
//  behind them `tiles`, the n_views device pointers of the accumulators' tile-chunk arrays -- *d_tiles receives the table's device address)
template <typename T, typename CamT>
static int upload_batch(RenderRec *rec, const CamT *cam, int n_views, const uint64_t *seeds, uint64_t seed, const AccumPass *pass, hipStream_t stream, rtw::BatchArgs<T> *B, rtw::AccumArgs *A,
                        const int *const *tiles = nullptr, const int *const **d_tiles = nullptr) {
    const size_t cam_bytes = (size_t)n_views * sizeof(rtw::Camera<T>), seed_bytes = (size_t)n_views * sizeof(unsigned long long);
    static_assert(sizeof(rtw::Camera<T>) % 8 == 0, "the seeds and the view table behind the cameras are 8-byte aligned");
    const size_t tiles_off = cam_bytes + seed_bytes + (pass ? (size_t)n_views * sizeof(rtw::AccumView) : 0);
    const size_t bytes = tiles_off + (tiles ? (size_t)n_views * sizeof(const int *) : 0);
    if (rec->views_cap < bytes) {
        if (rec->d_views) { HIP_IGNORE(hipFree(rec->d_views)); rec->d_views = nullptr; }
        if (rec->h_views) { HIP_IGNORE(hipHostFree(rec->h_views)); rec->h_views = nullptr; }
        rec->views_cap = 0;
        HIP_TRY(hipMalloc(&rec->d_views, bytes));
        HIP_TRY(hipHostMalloc(&rec->h_views, bytes, hipHostMallocDefault));
        rec->views_cap = bytes;
    }
    rtw::Camera<T> *hc = reinterpret_cast<rtw::Camera<T> *>(rec->h_views);
    unsigned long long *hs = reinterpret_cast<unsigned long long *>(static_cast<char *>(rec->h_views) + cam_bytes);
    for (int v = 0; v < n_views; ++v) { hc[v] = device_camera<T>(cam[v]); hs[v] = seeds ? seeds[v] : seed; }
    if (pass) {
        rtw::AccumView *hv = reinterpret_cast<rtw::AccumView *>(static_cast<char *>(rec->h_views) + cam_bytes + seed_bytes);
        for (int v = 0; v < n_views; ++v) { hv[v].words = pass->views[v].words; hv[v].samples = pass->views[v].samples; hv[v].pad = 0; }
        A->views = reinterpret_cast<const rtw::AccumView *>(static_cast<const char *>(rec->d_views) + cam_bytes + seed_bytes);
    }
    if (tiles) {
        memcpy(static_cast<char *>(rec->h_views) + tiles_off, tiles, (size_t)n_views * sizeof(const int *));
        *d_tiles = reinterpret_cast<const int *const *>(static_cast<const char *>(rec->d_views) + tiles_off);
    }
    HIP_TRY(hipMemcpyAsync(rec->d_views, rec->h_views, bytes, hipMemcpyHostToDevice, stream));
    B->cams = reinterpret_cast<const rtw::Camera<T> *>(rec->d_views);
    B->seeds = reinterpret_cast<const unsigned long long *>(static_cast<const char *>(rec->d_views) + cam_bytes);
    return 0;
}

// the same upload for a launch that is not the trace kernel's (the batched feature pass, rtw_features.hip): the device arrays of the
// cameras and of the seeds in the record's buffer
template <typename T, typename CamT>
int upload_views(RenderRec *rec, const CamT *cams, int n_views, const uint64_t *seeds, uint64_t seed, hipStream_t stream, const void **d_cams, const unsigned long long **d_seeds,
                 const int *const *tiles, const int *const **d_tiles) {
    rtw::BatchArgs<T> B;
    memset(&B, 0, sizeof B);
    if (int rc = upload_batch<T>(rec, cams, n_views, seeds, seed, nullptr, stream, &B, nullptr, tiles, d_tiles)) return rc;
    *d_cams = B.cams; *d_seeds = B.seeds;
    return 0;
}

// Enqueue one render (this shard's tiles) on `stream`; `rec` receives the counters and the kernel's events.
// n_views >= 1: a batch (validate_batch has accepted it): `cam` points to n_views cameras, `seeds` to n_views seeds (null: p->seed for
// every view), `d_out` to n_views frames.  The views' tile columns are laid side by side (rtw::BatchArgs), so the job shape, the grid and
// the queues see the batch's total tile count.  n_views == 0: one render of `cam`.
// `pass` non-null (n_views == 0; validate_accum has accepted it): one pass of a progressive render -- the chunks [chunk_begin, chunk_begin +
// chunk_count) of the render `p` describes, added to pass->words (rtw::AccumArgs); the job shape, the grid and the batches are those of a
// render of chunk_count chunks; `d_out` may be null.  pass->adapt: a pass of an adaptive render (the ADAPT instances: the half difference
// in word 7); with pass->tile_list also a pass over the pass->list_tiles tiles of that device-resident list only -- scheduled like a shard
// of that many tiles (K.shard_count = 0 marks it).
// n_views >= 1 AND `pass`: one pass of n_views progressive (adaptive) renders (the BATCH && ACCUM instances, rtw_batch_accum_f32.hip / _f64.hip):
// pass->views holds every view's accumulator and divisor, a tile list numbers the tiles batch-globally (v * n_tiles + t).
template <typename T, typename CamT>
int launch_render(rtw_scene_handle scene, const CamT *cam, int n_views, const uint64_t *seeds, const rtw_params *p, void *d_out, hipStream_t stream,
                  RenderRec **rec_out, CtxPtr *ctx_out, const AccumPass *pass) {
    if (!scene || !cam || (!d_out && !pass)) return fail(-1, "null argument");
    if (scene->is_f64 != (sizeof(T) == 8)) return fail(-4, "scene handle precision does not match the call");
    int nch, cs;
    if (int rc = validate_params(p, &nch, &cs)) return rc;
    if (pass) nch = pass->chunk_count;          // (what the scheduling sees; K.spp and K.chunk_spp stay the whole render's)
    const bool batch = n_views > 0;
    if (p->device >= 0 && p->device != scene->device)
        return fail(-4, "params.device %d != scene device %d", p->device, scene->device);
    CtxPtr ctx;
    if (int rc = get_ctx(scene->device, &ctx)) return rc;
    *ctx_out = ctx;
    HIP_TRY(hipSetDevice(scene->device));

    rtw::KParams K;
    memset(&K, 0, sizeof K);
    K.width = p->width; K.height = p->height; K.spp = p->spp; K.max_depth = p->max_depth;
    K.seed = p->seed; K.n_chunks = nch; K.chunk_spp = cs;
    K.shard_index = p->shard_index; K.shard_count = p->shard_count;
    const bool listed = pass && pass->adapt && pass->tile_list;
    if (listed) { K.shard_index = 0; K.shard_count = 0; }
    K.tiles_i = (p->height + 7) / 8; K.tiles_j = (p->width + 7) / 8;
    rtw::BatchArgs<T> B;
    memset(&B, 0, sizeof B);
    if (batch) {
        B.tiles_jv = (unsigned)K.tiles_j;
        make_udiv(B.tiles_jv, &B.div_tjv_m, &B.div_tjv_s);
        B.view_elems = (unsigned long long)p->width * (unsigned long long)p->height * 3ull;
        K.tiles_j *= n_views;                   // (validate_batch: N x tiles_j fits the queue positions)
    }
    rtw::AccumArgs A;
    memset(&A, 0, sizeof A);
    if (pass) { A.words = pass->words; A.chunk_begin = pass->chunk_begin; A.samples = pass->samples; A.tile_list = pass->adapt ? pass->tile_list : nullptr; }
    if (batch && pass && !pass->views) return fail(-1, "null argument");
    if (listed && (pass->list_tiles < 0 || pass->list_tiles > (long long)K.tiles_i * K.tiles_j)) return fail(-2, "tile list of %d entries", pass->list_tiles);
    const long long n_local = listed ? (long long)pass->list_tiles : batch ? (long long)K.tiles_i * K.tiles_j : local_tiles(p);
    K.gamma = p->gamma;
    K.out_layout = (p->flags & RTW_FLAG_COMPACT_TILES) ? 1 : 0;
    make_udiv((unsigned)K.tiles_i, &K.div_tiles_m, &K.div_tiles_s);
    const rtw::Camera<T> C = device_camera<T>(*cam);
    // ---- scene view: group cull reads the caller's order beside the cull layout, whose exact rows and index are what is staged in LDS ----
    using V4 = typename rtw::Vec4<T>::type;
    const int numerics = numerics_of(p->flags);
    static const bool phase_profile = aid_env("RTW_PHASE_PROFILE") != nullptr;   // debugging aid, not for timed runs
    const size_t list_bytes = (size_t)RTW_LIST_CAP * 256 * sizeof(unsigned short);
    const size_t shared_bytes = (sizeof(rtw::WgShared<T>) + 15) / 16 * 16;
    const bool cull = (p->flags & RTW_FLAG_GROUP_CULL) != 0;
    rtw::CullScene<T> CS = cull_scene_of<T>(scene);
    CS.numerics = numerics;
    // the plain scan runs pass 1 on the matrix pipe (RTW_SCAN=valu: the all-VALU scan, for A/B measurements)
    static const bool force_valu = aid_env("RTW_SCAN") != nullptr && strcmp(aid_env("RTW_SCAN"), "valu") == 0;
    // (group cull: on the matrix pipe too when the scene has the operands; RTW_FLAG_SCAN_VALU selects the all-VALU cull scan)
    const bool mfma = (cull ? scene->c_mf_ops != nullptr : scene->mf_ops != nullptr) && !force_valu && !(p->flags & RTW_FLAG_SCAN_VALU);
    PlainView<T> V;
    if (cull) {
        const size_t n_cull = (size_t)rtw::cull_exact_count(CS);
        V.scene = dev_scene_of<T>(scene);
        V.scene.numerics = numerics;
        // (on the matrix pipe the tables of the block vote travel with the scene copy)
        V.scene_bytes = n_cull * sizeof(V4) + ((n_cull * sizeof(unsigned short) + 15) / 16) * 16 + (mfma ? (size_t)rtw::cull_tab_words(scene->c_mf_blocks) * sizeof(unsigned) : 0);
        V.lds_scene = V.scene_bytes <= RTW_LDS_SCENE_MAX_BYTES;
    } else if (int rc = plain_scene_view<T>(scene, mfma, numerics, &V)) return rc;
    const bool lds_scene = V.lds_scene;
    const size_t lds_bytes = list_bytes + shared_bytes + (mfma ? rtw::mfma_cell_bytes<T>() : 0) + (lds_scene ? V.scene_bytes : 0);
    // ---- instance (rtw_instances.hpp; a pass of a batch of renders: the BATCH && ACCUM instances, a translation unit per precision) ----
    const bool fixed = numerics == rtw::NUM_REFERENCE;
    TraceInstance inst;
    if (!batch && !pass) inst = trace_instance_of<T, false, false, false>(cull, mfma, lds_scene, fixed, phase_profile);
    else if (batch && pass) inst = sizeof(T) == 8 ? batch_accum_kernel_f64(cull, mfma, lds_scene, fixed, pass->adapt) : batch_accum_kernel_f32(cull, mfma, lds_scene, fixed, pass->adapt);
    else if (batch) inst = trace_instance_of<T, true, false, false>(cull, mfma, lds_scene, fixed, phase_profile);
    else if (!pass->adapt) inst = trace_instance_of<T, false, true, false>(cull, mfma, lds_scene, fixed, phase_profile);
    else inst = trace_instance_of<T, false, true, true>(cull, mfma, lds_scene, fixed, phase_profile);
    const trace_kern_t<T> kern = (trace_kern_t<T>)inst.kern;
    // ---- occupancy: the persistent grid is enough 256-thread blocks to fill every CU at the kernel's occupancy ----
    PoolChoice pool;
    if (int rc = choose_pool<T>(ctx.get(), scene, p, cs, !batch && !pass && mfma && !cull, phase_profile, &pool)) return rc;
    int blocks_per_cu = pool.blocks_per_cu;
    if (!pool.use) {
        // (the runtime's answer for a (kernel, LDS size) pair does not change: asked once per device context -- 4 us per render otherwise)
        std::lock_guard<std::mutex> lk(ctx->mu);
        for (auto &o : ctx->occupancy) if (o.first.first == inst.kern && o.first.second == lds_bytes) blocks_per_cu = o.second;
        if (blocks_per_cu < 1) {
            HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks_per_cu, kern, 256, lds_bytes));
            ctx->occupancy.push_back({{inst.kern, lds_bytes}, blocks_per_cu});
        }
    }
    if (blocks_per_cu < 1) blocks_per_cu = 1;
    // (test aid: which instance the table picked -- `fixed`: the one with the default numerics mode compiled in)
    static const bool debug = aid_env("RTW_DEBUG") != nullptr;
    if (debug && !pool.use)
        fprintf(stderr, "[rtw debug] trace instance: %s lds_scene=%d cull=%d mfma=%d fixed=%d batch=%d accum=%d adapt=%d lds_bytes=%zu blocks_per_cu=%d\n", sizeof(T) == 8 ? "f64" : "f32",
                (int)lds_scene, (int)cull, (int)mfma, (int)inst.fixed, (int)batch, (int)(pass != nullptr), (int)(pass && pass->adapt), lds_bytes, blocks_per_cu);
    // ---- job shape ----
    static const ShapeAids aids = {[] { const char *e = aid_env("RTW_JOB_PIXELS"); const int v = e ? atoi(e) : 0; return (v == 1 || v == 4 || v == 8 || v == 16) ? v : 0; }(),
                                   aid_env("RTW_ROWS_SHIFT") ? atoi(aid_env("RTW_ROWS_SHIFT")) : -1, aid_env("RTW_GRID_BLOCKS") ? atoll(aid_env("RTW_GRID_BLOCKS")) : 0};
    JobShape J;
    if (int rc = job_shape(nch, n_local, K.tiles_i, K.tiles_j, K.shard_count, (long long)ctx->num_cus * blocks_per_cu, p->job_pixels, pool.use, aids, &J)) return rc;
    K.total_jobs = (unsigned)J.total_jobs; K.local_tiles = (unsigned)n_local; K.bpj = (unsigned)J.bpj; K.job_shift = (unsigned)J.job_shift;
    K.rows_shift = (unsigned)J.rows_shift; K.slot_stride = J.slot_stride; K.n_slots = J.n_slots;
    make_udiv((unsigned)J.bpj, &K.div_bpj_m, &K.div_bpj_s);
    // ---- record.  The counters: queue heads + segment / sample counts (+ the phase cells) are cleared per render; the drain clocks and
    // their 16 KB histogram only when the drain is profiled (the kernel touches them only then) ----
    static const bool drain_profile = aid_env("RTW_DRAIN_PROFILE") != nullptr;
    K.drain_profile = drain_profile ? 1 : 0;
    const size_t ctr_bytes = (drain_profile || phase_profile || pool.use) ? sizeof(rtw::DevCounters) : offsetof(rtw::DevCounters, t_first);    // (the ray-pool kernel keeps its stage profile / watchdog state in the histogram cells)
    if (int rc = begin_record(ctx.get(), scene, nch, (int)J.grid, pool.block_threads, ctr_bytes, stream, rec_out)) return rc;
    RenderRec *rec = *rec_out;
    if (drain_profile) HIP_TRY(hipMemsetAsync(&rec->ctr->t_first, 0xff, sizeof(unsigned long long), stream));
    // ---- views ----
    if (batch) if (int rc = upload_batch<T>(rec, cam, n_views, seeds, p->seed, pass, stream, &B, &A)) return rc;
    // pixels of other shards read 0 in the full-frame layout (the sum over the shards is the image)
    if (K.out_layout == 0 && p->shard_count > 1 && d_out)
        HIP_TRY(hipMemsetAsync(d_out, 0, (size_t)p->width * p->height * 3 * sizeof(T), stream));
    // ---- launch ----
    return run_record(rec, stream, [&] {
        if (J.total_jobs <= 0) return;
#ifdef RTW_WITH_POOL
        if (pool.use) {
            rtw::DevScene<T> S_caller = dev_scene_of<T>(scene);      // (the caller's order)
            S_caller.numerics = numerics;
            hipLaunchKernelGGL((pool_kern_t<T>)pool.kern, dim3((unsigned)J.grid), dim3((unsigned)pool.block_threads), pool.lds, stream, K, C, S_caller, (T *)d_out, rec->ctr);
            return;
        }
#endif
        hipLaunchKernelGGL(kern, dim3((unsigned)J.grid), dim3(256), lds_bytes, stream, K, C, V.scene, CS, (T *)d_out, rec->ctr, B, A);
    });
}

// wait for a record's kernel and add its counters to `agg`
int resolve_rec(RenderRec *r, rtw_stats_t *agg) {
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipEventSynchronize(r->ev2));
    r->done = true;
    float k_ms = 0;
    HIP_TRY(hipEventElapsedTime(&k_ms, r->ev0, r->ev1));
    const rtw::DevCounters &c = *r->h_ctr;         // (the copy that followed the kernel on its stream; the drain part only with RTW_DRAIN_PROFILE)
    if (aid_env("RTW_DEBUG")) {
        rtw::DevCounters chk;
        HIP_TRY(hipMemcpy(&chk, r->ctr, offsetof(rtw::DevCounters, t_first), hipMemcpyDeviceToHost));
        fprintf(stderr, "[rtw debug] resolve rec %p dev %d grid %d: pinned copy samples %llu segments %llu | device now samples %llu segments %llu%s\n", (void *)r, r->device, r->grid,
                (unsigned long long)c.samples, (unsigned long long)c.segments, (unsigned long long)chk.samples, (unsigned long long)chk.segments, c.samples != chk.samples ? "  <-- STALE" : "");
    }
    if (aid_env("RTW_PHASE_PROFILE") && r->block != 256) {
        const unsigned long long *pp = reinterpret_cast<const unsigned long long *>(c.end_hist + 256);
        static const char *names[6] = {"SCAN", "LM", "END", "DIEL", "REJ", "WAIT"};
        const double tot = (double)pp[26];
        fprintf(stderr, "[rtw pool profile] wave-cycles %.4g; idle %.1f%%; lost pops %llu; blocks without a candidate %.1f%% of %llu\n", tot, 100.0 * (double)pp[24] / tot, (unsigned long long)pp[25],
                pp[28] ? 100.0 * (double)pp[27] / (double)pp[28] : 0.0, (unsigned long long)pp[28]);
        for (int k = 0; k < 6; ++k)
            fprintf(stderr, "[rtw pool profile]   %-5s batches %10llu  mean fill %5.1f  %5.1f%% of wave-cycles  %7.0f cycles/batch\n", names[k], (unsigned long long)pp[4 * k],
                    pp[4 * k] ? (double)pp[4 * k + 1] / (double)pp[4 * k] : 0.0, 100.0 * (double)pp[4 * k + 2] / tot, pp[4 * k] ? (double)pp[4 * k + 2] / (double)pp[4 * k] : 0.0);
    } else if (aid_env("RTW_PHASE_PROFILE")) {
        double tot = 0;
        for (int k = 0; k < 6; ++k) tot += (double)c.phase[k];
        fprintf(stderr, "[rtw phase profile] wave-cycles: pull %.1f%%  sample+scatter finish %.1f%%  scan-pass1/level1 %.1f%%  extract/level2 %.1f%%  resolve %.1f%%  shade %.1f%%  (total %.3g)\n",
                100 * c.phase[0] / tot, 100 * c.phase[1] / tot, 100 * c.phase[2] / tot, 100 * c.phase[4] / tot,
                100 * c.phase[5] / tot, 100 * c.phase[3] / tot, tot);
        if (c.phase[8])
            fprintf(stderr, "[rtw phase profile] lane loop: %llu wave-iterations, lane utilisation at the scan %.2f %% (%llu lanes with a ray), %.2f %% of the iterations without any ray; "
                            "lane-iterations lost at batch boundaries %.2f %% (pool short) + %.2f %% (no usable batch)\n", (unsigned long long)c.phase[8],
                    100.0 * (double)c.phase[9] / (64.0 * (double)c.phase[8]), (unsigned long long)c.phase[9], 100.0 * (double)c.phase[10] / (double)c.phase[8],
                    100.0 * (double)c.phase[11] / (64.0 * (double)c.phase[8]), 100.0 * (double)c.phase[12] / (64.0 * (double)c.phase[8]));
        if (c.phase[8]) {
            fprintf(stderr, "[rtw phase counts] per wave-iteration:");
            static const char *nm[32] = {0, 0, 0, 0, 0, 0, "blocks_without_candidate", "blocks", "iterations", "lanes_with_ray", "iterations_without_ray", "takers_pool_short", "takers_unserved",
                                         "list_entries", "exact_test_rounds", "exact_tests", "reject_trials", "R_executed", "H1_executed", "H1_rounds", "A_executed", "jobs_stored", "batches_set_up",
                                         "H2_executed", "B_executed", "F_normalize_executed", "sign_collections", "blocks_recording", "explode_iterations", "reject_trials_3_draws", "half_blocks", "half_blocks_settled_coarse"};
            for (int k = 6; k < 32; ++k) if (nm[k]) fprintf(stderr, " %s=%.4f", nm[k], (double)c.phase[k] / (double)c.phase[8]);
            fprintf(stderr, "\n");
        }
        if (c.phase[8] && c.phase[13])
            fprintf(stderr, "[rtw phase profile] pass 2: %.1f list entries, %.2f exact-test rounds and %.1f exact tests per wave-iteration (lanes busy in a round: %.1f %%)\n",
                    (double)c.phase[13] / (double)c.phase[8], (double)c.phase[14] / (double)c.phase[8], (double)c.phase[15] / (double)c.phase[8], 100.0 * (double)c.phase[15] / (64.0 * (double)c.phase[14]));
        if (c.phase[7])
            fprintf(stderr, "[rtw phase profile] matrix-pipe scan: %.1f%% of the (wave, block of 32 spheres) evaluations found no candidate in any lane (%llu of %llu)\n",
                    100.0 * (double)c.phase[6] / (double)c.phase[7], (unsigned long long)c.phase[6], (unsigned long long)c.phase[7]);
    }
    if (r->ctr_bytes == sizeof(rtw::DevCounters) && c.end_hist[0] == 0xdeadbeefu) {        // (RTW_POOL_WATCHDOG builds: the pool kernel gave up; its state)
        fprintf(stderr, "[rtw pool watchdog]");
        for (int k = 1; k <= 113; ++k) fprintf(stderr, " %u", c.end_hist[k]);
        fprintf(stderr, "\n");
    }
    if (aid_env("RTW_DRAIN_PROFILE") && c.n_waves) {
        const double span = (double)(c.t_last - c.t_first) * 1e-5, mean_end = ((double)c.t_end_sum / (double)c.n_waves - (double)c.t_first) * 1e-5;
        fprintf(stderr, "[rtw drain profile] %llu waves: kernel span %.2f ms, mean wave end at %.2f ms -> %.2f ms (%.1f %%) of idle wave slots at the end of the queue\n",
                (unsigned long long)c.n_waves, span, mean_end, span - mean_end, 100.0 * (span - mean_end) / span);
        int last = 4095;
        while (last > 0 && !c.end_hist[last]) --last;
        fprintf(stderr, "[rtw drain profile] waves ending per 0.25 ms bin, last 64 bins (ending at %.2f ms):", (last + 1) * 0.25);
        for (int b = std::max(0, last - 63); b <= last; ++b) fprintf(stderr, " %u", c.end_hist[b]);
        fprintf(stderr, "\n");
    }
    agg->samples += c.samples;
    agg->segments += c.segments;
    agg->sphere_tests += c.segments * (uint64_t)r->n_spheres;
    agg->kernel_ms = std::max(agg->kernel_ms, (double)k_ms);
    agg->total_ms = std::max(agg->total_ms, (double)k_ms);
    agg->n_chunks = r->n_chunks;
    agg->grid_blocks = std::max(agg->grid_blocks, r->grid);
    agg->block_threads = std::max(agg->block_threads, r->block);
    return 0;
}

template int upload_views<float>(RenderRec *, const rtw_camera_f32 *, int, const uint64_t *, uint64_t, hipStream_t, const void **, const unsigned long long **, const int *const *, const int *const **);
template int upload_views<double>(RenderRec *, const rtw_camera_f64 *, int, const uint64_t *, uint64_t, hipStream_t, const void **, const unsigned long long **, const int *const *, const int *const **);
template int launch_render<float>(rtw_scene_handle, const rtw_camera_f32 *, int, const uint64_t *, const rtw_params *, void *, hipStream_t, RenderRec **, CtxPtr *, const AccumPass *);
template int launch_render<double>(rtw_scene_handle, const rtw_camera_f64 *, int, const uint64_t *, const rtw_params *, void *, hipStream_t, RenderRec **, CtxPtr *, const AccumPass *);

}  // namespace rtwh
