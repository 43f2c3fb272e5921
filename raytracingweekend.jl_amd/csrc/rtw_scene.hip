// rtw_scene.hip -- scene upload (rtw_scene_upload_f32/_f64 and the cached uploads of the host-buffer entry points): the SoA rows the
// kernels read, the kd split and boxes of the opt-in group-cull layout, and the sphere-side operands of the matrix-pipe filter
// (hit_world_mfma, rtw_device.hpp) with their error-margin constants.  Host code only; -ffp-contract=off like the kernels.
#include "rtw_scene_view.hpp"
#include "rtw_cull_tables.hpp"
#include "rtw_plain_layout.hpp"
#include "rtw_mfma_operands.hpp"

namespace rtwh {

// kd median split of the small class into clusters of <= RTW_CULL_GS spheres (ids = indices into the caller's list)
template <typename SceneT>
void kd_split(const SceneT *s, std::vector<int> &ids, int lo, int hi, std::vector<std::vector<int>> &groups) {
    const int cnt = hi - lo;
    if (cnt <= RTW_CULL_GS) {
        if (cnt > 0) groups.emplace_back(ids.begin() + lo, ids.begin() + hi);
        return;
    }
    double mn[3] = {1e300, 1e300, 1e300}, mx[3] = {-1e300, -1e300, -1e300};
    for (int k = lo; k < hi; ++k) {
        const double c[3] = {(double)s->cx[ids[k]], (double)s->cy[ids[k]], (double)s->cz[ids[k]]};
        for (int a = 0; a < 3; ++a) { mn[a] = std::min(mn[a], c[a]); mx[a] = std::max(mx[a], c[a]); }
    }
    int ax = 0;
    for (int a = 1; a < 3; ++a) if (mx[a] - mn[a] > mx[ax] - mn[ax]) ax = a;
    // left part: whole clusters -- and whole PAIRS of clusters while more than one pair is left, so that the blocks of 32 of
    // the matrix-pipe cull (two consecutive clusters) are always siblings of this tree
    const int unit = cnt > 2 * RTW_CULL_GS ? 2 * RTW_CULL_GS : RTW_CULL_GS;
    int half = ((cnt / 2 + unit - 1) / unit) * unit;
    if (half >= cnt) half = cnt - 1;
    auto key = [&](int i) { return ax == 0 ? (double)s->cx[i] : ax == 1 ? (double)s->cy[i] : (double)s->cz[i]; };
    std::nth_element(ids.begin() + lo, ids.begin() + lo + half, ids.begin() + hi, [&](int a, int b) { return key(a) < key(b); });
    kd_split(s, ids, lo, lo + half, groups);
    kd_split(s, ids, lo + half, hi, groups);
}

// the cold per-sphere rows (rtw_device.hpp "device scene"): mat0 = (r, param, kind, 1 / ir), mat1 = albedo -- or, for a Dielectric,
// Schlick's r0 for a front and a back face (dielectric_constants: the reference's own expressions evaluated once, in T)
template <typename T, typename V4, typename SceneT>
void material_rows(const SceneT *s, int i, V4 &m0, V4 &m1) {
    m0 = V4{s->r[i], s->param[i], (T)s->kind[i], (T)0};
    m1 = V4{s->ar[i], s->ag[i], s->ab[i], (T)0};
    if (s->kind[i] == rtw::DIELECTRIC) {
        const rtw::DielConst<T> c = rtw::dielectric_constants<T>(s->param[i]);
        m0.w = c.inv_ir;
        m1 = V4{c.r0_front, c.r0_back, (T)0, (T)0};
    }
}

// cluster-major arrays for the opt-in group-cull scan (rtw_device.hpp, "opt-in accelerated scan")
template <typename T, typename V4>
int build_mfma_operands(const std::vector<V4> &geom, int n, rtw_scene_dev *h, void **ops_out, int *blocks_out, int n_skip = 0, const int *skip = nullptr, int n_rows = -1);

template <typename T, typename SceneT>
int build_cull(const SceneT *s, rtw_scene_dev *h) {
    using V4 = typename rtw::Vec4<T>::type;
    const int n = s->n;
    constexpr int pair = 2 * RTW_CULL_BG, GS = RTW_CULL_GS;
    // BIG class: |r| > 4 x lower-median |r| (the ground sphere, the unit spheres of scene_random_spheres)
    std::vector<int> small_ids, big_ids;
    if (n > 0) {
        std::vector<double> rr(n);
        for (int i = 0; i < n; ++i) rr[i] = std::fabs((double)s->r[i]);
        std::vector<double> tmp(rr);
        std::nth_element(tmp.begin(), tmp.begin() + (n - 1) / 2, tmp.end());
        const double thr = 4.0 * tmp[(n - 1) / 2];
        for (int i = 0; i < n; ++i) (rr[i] > thr ? big_ids : small_ids).push_back(i);
    }
    std::vector<std::vector<int>> groups;
    kd_split(s, small_ids, 0, (int)small_ids.size(), groups);
    const int ng = (int)groups.size();
    const int ng_pad = ((ng + pair - 1) / pair) * pair;
    const int n_big = (int)big_ids.size();
    const int n_exact = ng_pad * GS + ((n_big + 31) / 32) * 32;          // whole blocks of 32 (the matrix-pipe scan may list any slot of a block)
    if (n_exact >= 65536) return fail(-5, "too many spheres (%d) for the group-cull layout", n);
    std::vector<T> box((size_t)(ng_pad + RTW_CULL_BG) * 8);            // + one prefetch group
    std::vector<V4> exact(std::max(n_exact, 1)), mat0(std::max(n_exact, 1)), mat1(std::max(n_exact, 1));
    std::vector<unsigned short> orig(std::max(n_exact, 1), 0);
    // dead cluster: far away and empty; dead sphere: r^2 = -1e30 (never a candidate)
    for (auto &b : box) b = (T)1e15;                                    // dead cluster: a point far away
    for (int k = 0; k < n_exact; ++k) { exact[k] = V4{(T)0, (T)0, (T)0, (T)-1e30}; mat0[k] = V4{(T)1, (T)0, (T)0, (T)0}; mat1[k] = V4{(T)0, (T)0, (T)0, (T)0}; }
    auto put = [&](int k, int i) {
        exact[k] = V4{s->cx[i], s->cy[i], s->cz[i], s->r[i] * s->r[i]};
        material_rows<T, V4>(s, i, mat0[k], mat1[k]);
        orig[k] = (unsigned short)i;
    };
    double cs[3] = {0, 0, 0}, rs = 0;
    long nsm = 0;
    for (auto &g : groups) for (int i : g) { cs[0] += s->cx[i]; cs[1] += s->cy[i]; cs[2] += s->cz[i]; ++nsm; }
    if (nsm) { cs[0] /= nsm; cs[1] /= nsm; cs[2] /= nsm; }
    for (int gi = 0; gi < ng; ++gi) {
        const auto &g = groups[gi];
        double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
        for (int j = 0; j < (int)g.size(); ++j) {
            const int i = g[j];
            const double c[3] = {(double)s->cx[i], (double)s->cy[i], (double)s->cz[i]}, ar = std::fabs((double)s->r[i]);
            for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], c[a] - ar); hi[a] = std::max(hi[a], c[a] + ar); }
            put(gi * GS + j, i);
            const double ex = c[0] - cs[0], ey = c[1] - cs[1], ez = c[2] - cs[2];
            rs = std::max(rs, std::sqrt(ex * ex + ey * ey + ez * ez) + ar);
        }
        for (int a = 0; a < 3; ++a) {                                    // round outwards
            T l = (T)lo[a], u2 = (T)hi[a];
            if ((double)l > lo[a]) l = std::nextafter(l, (T)-INFINITY);
            if ((double)u2 < hi[a]) u2 = std::nextafter(u2, (T)INFINITY);
            box[(size_t)gi * 8 + a] = l; box[(size_t)gi * 8 + 4 + a] = u2;
        }
        box[(size_t)gi * 8 + 3] = box[(size_t)gi * 8 + 7] = (T)0;
    }
    for (int k = 0; k < n_big; ++k) put(ng_pad * GS + k, big_ids[k]);
    h->c_groups_pad = ng_pad; h->c_big = n_big;
    h->c_cs[0] = (double)(T)cs[0]; h->c_cs[1] = (double)(T)cs[1]; h->c_cs[2] = (double)(T)cs[2];
    h->c_rs = rs * (1.0 + 1e-5) + 1e-3 * (std::fabs(cs[0]) + std::fabs(cs[1]) + std::fabs(cs[2])) * (sizeof(T) == 4 ? 1e-4 : 1e-12);
    const size_t bb = sizeof(T) * box.size(), eb = sizeof(V4) * exact.size(), ob = sizeof(unsigned short) * orig.size();
    HIP_TRY(hipMalloc(&h->c_bound, bb));
    HIP_TRY(hipMalloc(&h->c_exact, eb));
    HIP_TRY(hipMalloc(&h->c_mat0, eb));
    HIP_TRY(hipMalloc(&h->c_mat1, eb));
    HIP_TRY(hipMalloc((void **)&h->c_orig, ob));
    HIP_TRY(hipMemcpy(h->c_bound, box.data(), bb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->c_exact, exact.data(), eb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->c_mat0, mat0.data(), eb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->c_mat1, mat1.data(), eb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->c_orig, orig.data(), ob, hipMemcpyHostToDevice));
    // Group cull on the matrix pipe (hit_world_mfma<.., CULLED>): the operands in this cluster-major order and one
    // box per block of 32 = two clusters (dead clusters left out; the BIG class: everything).  Boxes are binary32,
    // rounded outwards, for both precisions -- the slab test runs in binary32 with the Float32 margin.
    if (h->mf_ops && n_exact > 0) {
        h->c_n_inlane = 0;
        for (int k = 0; k < RTW_CULL_INLANE_MAX; ++k) h->c_inlane[k] = -1;
        for (int k = 0; k < h->n_huge; ++k) {                     // the huge spheres (tested in-lane) in this order
            int at = -1;
            for (int dI = 0; dI < n_exact; ++dI)
                if ((double)exact[dI].w > -1e29 && (int)orig[dI] == h->huge[k]) { at = dI; break; }
            if (at < 0) return fail(-9, "internal: huge sphere %d not found in the cull layout", h->huge[k]);
            h->c_inlane[h->c_n_inlane++] = at;
        }
        // The BIG class is a block of its own that every half wave visits.  When all of it fits the in-lane list (the reference's scenes: the
        // ground and three spheres of radius 1), every lane tests those spheres by itself -- the exact test, the same keys -- and the block
        // is dead: 4 MFMAs, their sign collection and a pass-2 batch per scan less.  Scheduling only.
        {
            std::vector<int> rest;
            for (int k = 0; k < n_big; ++k) {
                const int dI = ng_pad * GS + k;
                if (!((double)exact[dI].w > -1e29)) continue;
                bool have = false;
                for (int j = 0; j < h->c_n_inlane; ++j) have = have || h->c_inlane[j] == dI;
                if (!have) rest.push_back(dI);
            }
            // (Float32 only -- measured 293.1 -> 288.9 ms at configs[2]; the binary64 tests cost more than the block: 93.3 -> 93.9 ms at the published configuration)
            static const bool inlane_f64 = aid_flag("RTW_INLANE_F64");      // (A/B aid: the in-lane class for Float64 too -- with the discriminant-only form of round 6)
            if ((sizeof(T) == 4 || inlane_f64) && h->c_n_inlane + (int)rest.size() <= RTW_CULL_INLANE_MAX)
                for (int dI : rest) h->c_inlane[h->c_n_inlane++] = dI;
        }
        auto in_lane = [&](int dI) { for (int j = 0; j < h->c_n_inlane; ++j) if (h->c_inlane[j] == dI) return true; return false; };
        if (int rc = build_mfma_operands<T>(exact, n_exact, h, &h->c_mf_ops, &h->c_mf_blocks, h->c_n_inlane, h->c_inlane)) return rc;
        const int nb = h->c_mf_blocks;
        std::vector<float> bx((size_t)(nb + 1) * 8, 0.0f);
        for (int b = 0; b <= nb; ++b) {
            double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
            bool all = false, any = false;
            for (int c = 2 * b; c < 2 * b + 2; ++c) {
                if (c >= ng_pad) {                                                            // BIG class (device indices >= ng_pad * GS): any row left for the filter?
                    if (b < nb) for (int dI = c * GS; dI < std::min((c + 1) * GS, n_exact); ++dI) if ((double)exact[dI].w > -1e29 && !in_lane(dI)) all = true;
                    continue;
                }
                if (c >= ng) continue;                                                        // dead cluster
                any = true;
                for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], (double)box[(size_t)c * 8 + a]); hi[a] = std::max(hi[a], (double)box[(size_t)c * 8 + 4 + a]); }
            }
            float *q = &bx[(size_t)b * 8];
            for (int a = 0; a < 3; ++a) {
                if (all) { q[a] = -INFINITY; q[4 + a] = INFINITY; }                          // never skipped (the vote of hit_world_mfma)
                else if (!any) { q[a] = 1e15f; q[4 + a] = 1e15f; }                            // nothing alive: a point far away
                else {
                    float l = (float)lo[a], u2 = (float)hi[a];
                    if ((double)l > lo[a]) l = std::nextafter(l, -INFINITY);
                    if ((double)u2 < hi[a]) u2 = std::nextafter(u2, INFINITY);
                    q[a] = l; q[4 + a] = u2;
                }
            }
        }
        // the box of the whole small class: the union of the live, finite block boxes (none: lo > hi, every ray misses it)
        for (int a = 0; a < 3; ++a) { h->c_glo[a] = INFINITY; h->c_ghi[a] = -INFINITY; }
        for (int b = 0; b < nb; ++b) {
            const float *q = &bx[(size_t)b * 8];
            if (!std::isfinite(q[0]) || q[0] >= 1e15f) continue;                                   // BIG class / nothing alive
            for (int a = 0; a < 3; ++a) { h->c_glo[a] = std::min(h->c_glo[a], q[a]); h->c_ghi[a] = std::max(h->c_ghi[a], q[4 + a]); }
        }
        // The tables of the block vote (rtw::CullGrid): rtw_cull_tables.hpp builds them (plain C++, checked on the CPU by tests/cull_tables_check.cpp)
        CullTables ct;
        build_cull_tables(bx.data(), nb, h->c_glo, h->c_ghi, h->c_n_inlane, h->c_inlane, &ct);
        for (int k = 0; k < 3; ++k) { h->c_grid[k] = ct.inv[k]; h->c_grid[3 + k] = ct.off[k]; }
        std::vector<float> cells(ct.words.size(), 0.0f);
        memcpy(cells.data(), ct.words.data(), ct.words.size() * sizeof(unsigned));
        bx.insert(bx.end(), cells.begin(), cells.end());
        HIP_TRY(hipMalloc(&h->c_mf_box, bx.size() * sizeof(float)));
        HIP_TRY(hipMemcpy(h->c_mf_box, bx.data(), bx.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    return 0;
}

// Operands of pass 1 on the matrix pipe (rtw_device.hpp, hit_world_mfma): per block of 32 spheres the two A operands of the
// chained v_mfma_f32_32x32x16_f16 pair -- the sphere side of the K = 32 contraction
//     [cx^2 cy^2 cz^2 cxcy cxcz cycz] s^2 / 2 | [cx cy cz] s | k' s^2 (k' = r^2 - |c|^2 + the sphere's share Gs of the error margin) | 1
// every feature split into two f16 pieces, in the slot order documented there.  Row i of the instruction holds sphere
// 16 ((i >> 2) & 1) + (((i >> 3) << 2) | (i & 3)) of the block, so that result register r of lane (H, j) is sphere 16 H + r.
// `geom`: n entries; entries with r^2 < -1e29 are padding (never a candidate).  *ops_out / *blocks_out receive the device
// array; the scale constants in `h` depend on the set of spheres only, so every order of a scene gets the same ones.
// n_rows >= 0: only the first n_rows entries get rows (the plain scan's order keeps its huge spheres behind the blocks: they count for the
// scales like everything else).
template <typename T, typename V4>
int build_mfma_operands(const std::vector<V4> &geom, int n, rtw_scene_dev *h, void **ops_out, int *blocks_out, int n_skip, const int *skip, int n_rows) {
    *ops_out = nullptr; *blocks_out = 0;
    if (n <= 0) return 0;
    auto live = [&](int i) { return i < n && (double)geom[i].w > -1e29; };
    // `skip`: spheres whose filter ROW is disabled (written like a padding row: never flagged for a ray that uses the filter) because
    // every lane tests them exactly by itself (DevScene::huge).  They still count for the scales: both orders of a scene share those.
    if (n_rows < 0) n_rows = n;
    auto in_filter = [&](int i) { if (!live(i) || i >= n_rows) return false; for (int k = 0; k < n_skip; ++k) if (skip[k] == i) return false; return true; };
    double emax = 0;
    for (int i = 0; i < n; ++i) {
        if (!live(i)) continue;
        const double r = std::sqrt(std::fabs((double)geom[i].w));
        emax = std::max(emax, std::max(std::max(std::fabs((double)(float)geom[i].x), std::fabs((double)(float)geom[i].y)),
                                       std::max(std::fabs((double)(float)geom[i].z), r)));
    }
    // the scales, the margin constants and the rows' words: rtw_mfma_operands.hpp (plain C++, checked on the CPU by tests/two_stage_check.cpp)
    MfmaScales S;
    if (!mfma_scales(emax, &S)) return 0;                // outside what the scaled f16 pieces cover: VALU scan
    const int nb = (n_rows + 31) / 32;
    std::vector<uint4> ops((size_t)(nb + 1) * 128);
    for (int blk = 0; blk <= nb; ++blk)
        for (int lane = 0; lane < 64; ++lane) {
            const int i = lane & 31, H = lane >> 5;
            const int sph = blk * 32 + 16 * ((i >> 2) & 1) + (((i >> 3) << 2) | (i & 3));
            MfmaSphereRow row;
            if (in_filter(sph)) mfma_sphere_row(true, (double)(float)geom[sph].x, (double)(float)geom[sph].y, (double)(float)geom[sph].z, (double)geom[sph].w, S, &row);
            else mfma_sphere_row(false, 0, 0, 0, 0, S, &row);
            uint32_t w1[4], w2[4];
            mfma_sphere_words(row, H, w1, w2);
            const uint4 m1 = {w1[0], w1[1], w1[2], w1[3]}, m2 = {w2[0], w2[1], w2[2], w2[3]};
            ops[(size_t)blk * 128 + lane] = m1;
            ops[(size_t)blk * 128 + 64 + lane] = m2;
        }
    HIP_TRY(hipMalloc(ops_out, ops.size() * sizeof(uint4)));
    HIP_TRY(hipMemcpy(*ops_out, ops.data(), ops.size() * sizeof(uint4), hipMemcpyHostToDevice));
    *blocks_out = nb;
    h->mf_sc = (float)S.sc; h->mf_sigma2 = (float)S.sig2;
    h->mf_oo_keep = S.keep; h->mf_o1_coef = S.coef; h->mf_o_max = S.o_max; h->mf_mr = S.mr;
    return 0;
}

// The plain matrix-pipe scan's own order (rtw_plain_layout.hpp): the spheres that go through the filter in spatially sorted, evenly filled
// blocks of 32, unused rows dead, the huge spheres (tested in-lane, no row) behind the blocks; operands, geom / mat0 / mat1 in that order
// and the caller's index of every entry -- what "the later sphere wins a tie" is decided by (hit_world_mfma).  Uploaded once with the scene.
// At most one block, or more entries than a 16-bit index holds: the caller's arrays themselves, with the identity for the index array.
template <typename T, typename V4>
int build_plain(const std::vector<V4> &geom, const std::vector<V4> &mat0, const std::vector<V4> &mat1, int n, rtw_scene_dev *h) {
    if (!h->mf_ops) return 0;
    static const bool keep_env = aid_env("RTW_PLAIN_ORDER") != nullptr && strcmp(aid_env("RTW_PLAIN_ORDER"), "caller") == 0;      // A/B aid: the caller's order in the new code path
    auto is_huge = [&](int i) { for (int k = 0; k < h->n_huge; ++k) if (h->huge[k] == i) return true; return false; };
    std::vector<int> filt;
    std::vector<double> cx, cy, cz;
    for (int i = 0; i < n; ++i) {
        if (is_huge(i)) continue;
        filt.push_back(i);
        cx.push_back((double)geom[i].x); cy.push_back((double)geom[i].y); cz.push_back((double)geom[i].z);
    }
    PlainLayout L;
    build_plain_layout(cx.data(), cy.data(), cz.data(), (int)filt.size(), &L);
    constexpr int grp = rtw::ScanGroup<T>::N;
    const int n_rows = L.blocks * RTW_PLAIN_BLOCK, np = n_rows + h->n_huge, np_pad = ((np + grp - 1) / grp) * grp;
    const int np_alloc = rtw::scene_geom_alloc(np, np_pad);
    std::vector<unsigned short> orig;
    if (keep_env || L.blocks <= 1 || np_alloc >= 65536) {
        h->p_alias = 1;
        h->p_mf_ops = h->mf_ops; h->p_geom = h->geom; h->p_mat0 = h->mat0; h->p_mat1 = h->mat1;
        h->p_n = n; h->p_n_pad = h->n_pad; h->p_mf_blocks = h->mf_blocks; h->p_huge[0] = h->huge[0]; h->p_huge[1] = h->huge[1];
        orig.resize((size_t)rtw::scene_geom_alloc(n, h->n_pad));
        for (size_t i = 0; i < orig.size(); ++i) orig[i] = (unsigned short)i;
    } else {
        std::vector<V4> g(np_alloc, V4{(T)0, (T)0, (T)0, (T)-1e30}), m0(np_alloc, V4{(T)1, (T)0, (T)0, (T)0}), m1(np_alloc, V4{(T)0, (T)0, (T)0, (T)0});
        orig.assign((size_t)np_alloc, 0);
        auto put = [&](int k, int i) { g[k] = geom[i]; m0[k] = mat0[i]; m1[k] = mat1[i]; orig[k] = (unsigned short)i; };
        for (int k = 0; k < n_rows; ++k) if (L.slot[k] >= 0) put(k, filt[L.slot[k]]);
        for (int k = 0; k < h->n_huge; ++k) { put(n_rows + k, h->huge[k]); h->p_huge[k] = n_rows + k; }
        h->p_n = np; h->p_n_pad = np_pad;
        const size_t bytes = sizeof(V4) * (size_t)np_alloc;
        HIP_TRY(hipMalloc(&h->p_geom, bytes));
        HIP_TRY(hipMalloc(&h->p_mat0, bytes));
        HIP_TRY(hipMalloc(&h->p_mat1, bytes));
        HIP_TRY(hipMemcpy(h->p_geom, g.data(), bytes, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(h->p_mat0, m0.data(), bytes, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(h->p_mat1, m1.data(), bytes, hipMemcpyHostToDevice));
        if (int rc = build_mfma_operands<T>(g, np, h, &h->p_mf_ops, &h->p_mf_blocks, h->n_huge, h->p_huge, n_rows)) return rc;
        if (!h->p_mf_ops) return fail(-9, "internal: no matrix-pipe operands for the plain scan's order");
    }
    if (aid_env("RTW_DEBUG"))
        fprintf(stderr, "[rtw debug] plain scan layout: %d spheres through the filter, %d blocks, %s\n", (int)filt.size(), h->p_mf_blocks,
                h->p_alias ? "the caller's order" : "its own order");
    HIP_TRY(hipMalloc((void **)&h->p_orig, orig.size() * sizeof(unsigned short)));
    HIP_TRY(hipMemcpy(h->p_orig, orig.data(), orig.size() * sizeof(unsigned short), hipMemcpyHostToDevice));
    return 0;
}

template <typename T, typename SceneT>
int upload_scene(const SceneT *s, int device, rtw_scene_handle *out) {
    if (!s || !out) return fail(-1, "null argument");
    if (s->n < 0) return fail(-2, "scene.n < 0");
    if (s->n > 0 && (!s->cx || !s->cy || !s->cz || !s->r || !s->kind || !s->ar || !s->ag || !s->ab || !s->param))
        return fail(-1, "null scene array");
    for (int i = 0; i < s->n; ++i) {
        if (s->kind[i] < 0 || s->kind[i] > 2) return fail(-3, "sphere %d: unknown material kind %d", i, s->kind[i]);
        if (!std::isfinite((double)s->cx[i]) || !std::isfinite((double)s->cy[i]) || !std::isfinite((double)s->cz[i]) ||
            !std::isfinite((double)s->r[i]))
            return fail(-3, "sphere %d: centre / radius is not finite", i);
    }
    DeviceGuard guard;
    int dev;
    if (int rc = resolve_device(device, &dev)) return rc;
    CtxPtr ctx;
    if (int rc = get_ctx(dev, &ctx)) return rc;
    HIP_TRY(hipSetDevice(dev));
    using V4 = typename rtw::Vec4<T>::type;
    const int n = s->n;
    constexpr int grp = rtw::ScanGroup<T>::N;                                            // 8 (f32) / 4 (f64)
    const int n_pad = ((n + grp - 1) / grp) * grp;                                       // 0 spheres: no scan at all
    const int n_alloc = rtw::scene_geom_alloc(n, n_pad);                                  // prefetch tail group / whole blocks of 32
    if (n_pad >= 65536) return fail(-5, "too many spheres (%d): candidate lists hold 16-bit indices", n);
    std::vector<V4> geom(n_alloc), mat0(n_alloc), mat1(n_alloc);
    for (int i = 0; i < n_alloc; ++i) {
        if (i < n) {
            geom[i] = V4{s->cx[i], s->cy[i], s->cz[i], s->r[i] * s->r[i]};  // r^2: src/hit.jl:17
            material_rows<T, V4>(s, i, mat0[i], mat1[i]);
        } else {
            // padding sphere that can never be hit: r^2 hugely negative => disc < 0 always
            geom[i] = V4{(T)0, (T)0, (T)0, (T)-1e30};
            mat0[i] = V4{(T)1, (T)0, (T)0, (T)0};
            mat1[i] = V4{(T)0, (T)0, (T)0, (T)0};
        }
    }
    ScenePtr h(new rtw_scene_dev());                      // freed on every error path below
    memset(h.get(), 0, sizeof(rtw_scene_dev));
    h->device = dev; h->is_f64 = sizeof(T) == 8; h->n = n; h->n_pad = n_pad;
    {
        uint64_t hsh = 0xcbf29ce484222325ull;
        auto mix = [&hsh](const void *q, size_t nb) { const unsigned char *b = static_cast<const unsigned char *>(q); for (size_t k = 0; k < nb; ++k) { hsh ^= b[k]; hsh *= 0x100000001b3ull; } };
        const int32_t tag[2] = {(int32_t)sizeof(T), (int32_t)n};
        mix(tag, sizeof tag);
        for (const T *arr : {s->cx, s->cy, s->cz, s->r, s->ar, s->ag, s->ab, s->param}) mix(arr, sizeof(T) * (size_t)n);
        mix(s->kind, sizeof(int32_t) * (size_t)n);
        h->content_hash = hsh;
    }
    const size_t bytes = sizeof(V4) * (size_t)n_alloc;
    HIP_TRY(hipMalloc(&h->geom, bytes));
    HIP_TRY(hipMalloc(&h->mat0, bytes));
    HIP_TRY(hipMalloc(&h->mat1, bytes));
    HIP_TRY(hipMemcpy(h->geom, geom.data(), bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->mat0, mat0.data(), bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->mat1, mat1.data(), bytes, hipMemcpyHostToDevice));
    if (sizeof(T) == 8) {
        // pass-1 filter data of hit_world<double>: centre and r^2 rounded to binary32 (to nearest) and the sphere's
        // share G of the error margin, rounded up (derivation in rtw_device.hpp)
        std::vector<float> f((size_t)n_alloc * 8, 0.0f);
        for (int i = 0; i < n_alloc; ++i) {
            float *q = &f[(size_t)i * 8];
            q[0] = (float)geom[i].x; q[1] = (float)geom[i].y; q[2] = (float)geom[i].z; q[3] = (float)geom[i].w;
            if (i < n) {
                const double r2 = (double)geom[i].w, c2 = (double)geom[i].x * geom[i].x + (double)geom[i].y * geom[i].y + (double)geom[i].z * geom[i].z;
                const double G = 1.01 * (std::ldexp(r2, -18) + std::ldexp(c2, -20) + std::ldexp(r2, -20)) + 1e-30;
                float g = (float)G;
                if ((double)g < G) g = std::nextafter(g, INFINITY);
                if (!(c2 < 1e30) || !(r2 < 1e30)) g = INFINITY;                  // astronomically large: always a candidate
                q[4] = g;
            }                                                                     // padding spheres: r^2 = -1e30, G = 0
        }
        HIP_TRY(hipMalloc(&h->scan, f.size() * sizeof(float)));
        HIP_TRY(hipMemcpy(h->scan, f.data(), f.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    // "Huge" spheres: a ground sphere of radius 1000 under spheres of radius 0.2 has a non-negative discriminant for nearly every ray, so
    // it costs every scan two non-skipped half blocks, an extraction trip and a full 64-entry batch of pass 2.  At most two spheres whose
    // radius is >= 16 x the median radius are instead tested exactly by every lane for its own ray (hit_world_mfma; same contract test,
    // same tie rule), and their rows of the filter are disabled.  Scheduling only: the image cannot change.
    h->n_huge = 0;
    if (n >= 8) {
        std::vector<double> ra(n);
        for (int i = 0; i < n; ++i) ra[i] = std::fabs((double)s->r[i]);
        std::vector<double> sorted(ra);
        std::nth_element(sorted.begin(), sorted.begin() + n / 2, sorted.end());
        const double med = sorted[n / 2];
        for (int pick = 0; pick < 2; ++pick) {
            int best = -1;
            for (int i = 0; i < n; ++i) {
                if (!(ra[i] >= 16.0 * med) || !std::isfinite(ra[i])) continue;
                if (h->n_huge > 0 && h->huge[0] == i) continue;
                if (best < 0 || ra[i] > ra[best]) best = i;
            }
            if (best < 0) break;
            h->huge[h->n_huge++] = best;
        }
    }
    static const bool env_no_huge = aid_flag("RTW_NO_HUGE");      // A/B aid
    if (env_no_huge) h->n_huge = 0;
    if (int rc = build_mfma_operands<T>(geom, n, h.get(), &h->mf_ops, &h->mf_blocks, h->n_huge, h->huge)) return rc;
    if (int rc = build_plain<T>(geom, mat0, mat1, n, h.get())) return rc;
    if (int rc = build_cull<T>(s, h.get())) return rc;
    *out = h.release();
    return 0;
}

template int upload_scene<float>(const rtw_scene_f32 *, int, rtw_scene_handle *);
template int upload_scene<double>(const rtw_scene_f64 *, int, rtw_scene_handle *);

}  // namespace rtwh
