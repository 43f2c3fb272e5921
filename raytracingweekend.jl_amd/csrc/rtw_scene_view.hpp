// rtw_scene_view.hpp -- the device-side views (rtw_device.hpp DevScene / CullScene) of an uploaded scene handle; the numerics mode and the camera of a launch
#pragma once
#include "rtw_host.hpp"
#include "rtw_device.hpp"

namespace rtwh {

template <typename T>
rtw::CullScene<T> cull_scene_of(const rtw_scene_dev *h) {
    using V4 = typename rtw::Vec4<T>::type;
    rtw::CullScene<T> C;
    C.box = (const T *)h->c_bound; C.exact = (const V4 *)h->c_exact; C.orig = h->c_orig;
    C.mat0 = (const V4 *)h->c_mat0; C.mat1 = (const V4 *)h->c_mat1;
    C.n_groups_pad = h->c_groups_pad; C.n_big = h->c_big;
    C.cs[0] = (T)h->c_cs[0]; C.cs[1] = (T)h->c_cs[1]; C.cs[2] = (T)h->c_cs[2]; C.rs = (T)h->c_rs;
    C.kappa = sizeof(T) == 4 ? (T)0.00390625 : (T)2.384185791015625e-07;     // 2^-8 / 2^-22
    C.mf_ops = (const uint4 *)h->c_mf_ops; C.mf_box = (const float *)h->c_mf_box; C.mf_blocks = h->c_mf_blocks;
    for (int k = 0; k < 3; ++k) { C.mf_glo[k] = h->c_glo[k]; C.mf_ghi[k] = h->c_ghi[k]; }
    static_assert(RTW_CULL_INLANE_MAX == 8, "rtw_scene_dev::c_inlane");
    C.n_huge = h->c_mf_ops ? h->c_n_inlane : 0;
    C.n_huge_exact = h->c_mf_ops ? std::min(h->n_huge, h->c_n_inlane) : 0;      // (the huge spheres come first in c_inlane)
    for (int k = 0; k < 3; ++k) { C.grid.inv[k] = h->c_grid[k]; C.grid.off[k] = h->c_grid[3 + k]; }
    C.numerics = rtw::NUM_REFERENCE;
    return C;
}

template <typename T>
rtw::DevScene<T> dev_scene_of(const rtw_scene_dev *h) {
    using V4 = typename rtw::Vec4<T>::type;
    rtw::DevScene<T> S;
    memset(&S, 0, sizeof S);
    S.geom = (const V4 *)h->geom; S.mat0 = (const V4 *)h->mat0; S.mat1 = (const V4 *)h->mat1;
    S.scan = (const float *)(h->scan ? h->scan : h->geom);
    S.n = h->n; S.n_pad = h->n_pad;
    S.mf_ops = (const uint4 *)h->mf_ops; S.mf_blocks = h->mf_blocks;
    S.mf_sc = h->mf_sc; S.mf_sigma2 = h->mf_sigma2; S.mf_oo_keep = h->mf_oo_keep; S.mf_o1_coef = h->mf_o1_coef; S.mf_o_max = h->mf_o_max; S.mf_mr = h->mf_mr;
    S.n_huge = h->mf_ops ? h->n_huge : 0; S.huge[0] = h->huge[0]; S.huge[1] = h->huge[1];
    return S;
}

// the scene as the trace kernel's plain matrix-pipe scan reads it: its own sphere order (rtw_scene.hip build_plain) and the index array
template <typename T>
rtw::DevScene<T> dev_scene_plain_of(const rtw_scene_dev *h) {
    using V4 = typename rtw::Vec4<T>::type;
    rtw::DevScene<T> S = dev_scene_of<T>(h);
    S.geom = (const V4 *)h->p_geom; S.mat0 = (const V4 *)h->p_mat0; S.mat1 = (const V4 *)h->p_mat1;
    S.n = h->p_n; S.n_pad = h->p_n_pad;
    S.mf_ops = (const uint4 *)h->p_mf_ops; S.mf_blocks = h->p_mf_blocks;
    S.huge[0] = h->p_huge[0]; S.huge[1] = h->p_huge[1];
    S.orig = h->p_orig;
    return S;
}

// the deciding arithmetic of the ray-sphere test (include/rtw_hip.h RTW_FLAG_NUMERICS_*): a property of the render, not of the upload
inline int numerics_of(int flags) { return (flags & RTW_FLAG_NUMERICS_CONTRACT) ? rtw::NUM_CONTRACT : (flags & RTW_FLAG_NUMERICS_REFERENCE_FMA2) ? rtw::NUM_REFERENCE_FMA2 : rtw::NUM_REFERENCE; }

// a camera of the C ABI (rtw_camera_f32 / _f64) as the kernels take it
template <typename T, typename CamT>
rtw::Camera<T> device_camera(const CamT &cam) {
    rtw::Camera<T> C;
    for (int k = 0; k < 3; ++k) {
        C.origin[k] = cam.origin[k]; C.llc[k] = cam.lower_left_corner[k];
        C.horizontal[k] = cam.horizontal[k]; C.vertical[k] = cam.vertical[k];
        C.u[k] = cam.u[k]; C.v[k] = cam.v[k]; C.w[k] = cam.w[k];
    }
    C.lens_radius = cam.lens_radius;
    return C;
}

// What a launch without group cull (the trace kernel's plain render, the feature kernel) passes and asks for: the scene with `numerics` set,
// whether the instance that stages it in LDS runs, and the dynamic LDS the scene then needs.  Pass 1 on the matrix pipe (`mfma`) reads the
// plain scan's own order (rtw_scene.hip build_plain), whose index array travels with the scene copy; the all-VALU scan the caller's order.
// (lds_scene is decided by the caller-order bytes, so a scene takes the same instance whatever the layout; what is then asked for is scene_bytes: in the plain
//  order up to 31 dead rows + the huge spheres more, and 2 B per entry for the index -- at most 24 KB x 18 / 16 + 1.2 KB.  A trace launch's grid follows the
//  runtime's occupancy answer for the bytes really requested.)
template <typename T> struct PlainView { rtw::DevScene<T> scene; bool lds_scene; size_t scene_bytes; };
template <typename T>
int plain_scene_view(const rtw_scene_dev *h, bool mfma, int numerics, PlainView<T> *out) {
    using V4 = typename rtw::Vec4<T>::type;
    out->scene = dev_scene_of<T>(h);
    out->scene_bytes = (size_t)rtw::scene_geom_alloc(h->n, h->n_pad) * sizeof(V4);
    out->lds_scene = out->scene_bytes <= RTW_LDS_SCENE_MAX_BYTES;
    if (mfma) {
        if (!h->p_mf_ops || !h->p_orig) return fail(-9, "internal: the scene has no arrays in the plain scan's order");
        out->scene = dev_scene_plain_of<T>(h);
        const size_t na = (size_t)rtw::scene_geom_alloc(out->scene.n, out->scene.n_pad);
        out->scene_bytes = na * sizeof(V4) + ((na * sizeof(unsigned short) + 15) / 16) * 16;
    }
    out->scene.numerics = numerics;
    return 0;
}

}  // namespace rtwh
