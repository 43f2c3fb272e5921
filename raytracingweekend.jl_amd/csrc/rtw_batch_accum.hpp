// rtw_batch_accum.hpp -- the BATCH && ACCUM and BATCH && ACCUM && ADAPT instances of the trace kernel (rtw_kernels.hpp): one pass of N views'
// progressive or adaptive renders in one launch (rtw_render_accum_batch_*, rtw_render_adaptive_batch_*).  They live in translation units of
// their own, one per precision (rtw_batch_accum_f32.hip / _f64.hip), so that rtw_launch.hip builds as fast as before and the units
// compile in parallel; launch_render (rtw_launch.hip) asks for the instance of a scan variant by the same rules it applies to the others.
#pragma once
#include "rtw_scene_view.hpp"
#include "rtw_kernels.hpp"

namespace rtwh {

template <typename T, bool ADAPT>
const void *batch_accum_kernel_of(bool cull, bool mfma, bool lds_scene, bool fixed) {
    typedef void (*kern_t)(rtw::KParams, rtw::Camera<T>, rtw::DevScene<T>, rtw::CullScene<T>, T *, rtw::DevCounters *, rtw::BatchArgs<T>, rtw::AccumArgs);
    kern_t kern;
    if (cull && mfma) kern = lds_scene ? (kern_t)rtw::trace_kernel<T, false, true, true, true, -1, true, true, ADAPT> : (kern_t)rtw::trace_kernel<T, false, false, true, true, -1, true, true, ADAPT>;
    else if (cull) kern = lds_scene ? (kern_t)rtw::trace_kernel<T, false, true, true, false, -1, true, true, ADAPT> : (kern_t)rtw::trace_kernel<T, false, false, true, false, -1, true, true, ADAPT>;
    else if (mfma) kern = lds_scene ? (kern_t)rtw::trace_kernel<T, false, true, false, true, -1, true, true, ADAPT> : (kern_t)rtw::trace_kernel<T, false, false, false, true, -1, true, true, ADAPT>;
    else kern = lds_scene ? (kern_t)rtw::trace_kernel<T, false, true, false, false, -1, true, true, ADAPT> : (kern_t)rtw::trace_kernel<T, false, false, false, false, -1, true, true, ADAPT>;
    if (fixed && lds_scene && mfma)
        kern = cull ? (kern_t)rtw::trace_kernel<T, false, true, true, true, rtw::NUM_REFERENCE, true, true, ADAPT> : (kern_t)rtw::trace_kernel<T, false, true, false, true, rtw::NUM_REFERENCE, true, true, ADAPT>;
    return (const void *)kern;
}

}  // namespace rtwh
