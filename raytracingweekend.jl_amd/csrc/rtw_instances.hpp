// rtw_instances.hpp -- the kernel-instance table: which instance of the trace kernel (rtw_kernels.hpp) runs a scan variant -- group cull,
// pass 1 on the matrix pipe, the scene in LDS, the default numerics mode compiled in -- for one combination of BATCH, ACCUM and ADAPT.
// launch_render (rtw_launch.hip) asks it for the BATCH, the ACCUM and the ACCUM && ADAPT instances (the plain ones, which alone have
// phase-profile variants, it lists itself); the BATCH && ACCUM (&& ADAPT) instances -- one pass of N views' progressive or adaptive
// renders in one launch -- are asked for in translation units of their own, one per precision (rtw_batch_accum_f32.hip / _f64.hip), so
// that rtw_launch.hip builds as fast as before and the units compile in parallel.
#pragma once
#include "rtw_scene_view.hpp"
#include "rtw_kernels.hpp"

namespace rtwh {

// (`fixed`: the numerics mode is the default one, NUM_REFERENCE)
template <typename T, bool BATCH, bool ACCUM, bool ADAPT>
const void *trace_instance_of(bool cull, bool mfma, bool lds_scene, bool fixed) {
    typedef void (*kern_t)(rtw::KParams, rtw::Camera<T>, rtw::DevScene<T>, rtw::CullScene<T>, T *, rtw::DevCounters *, rtw::BatchArgs<T>, rtw::AccumArgs);
    kern_t kern;
    if (cull && mfma) kern = lds_scene ? (kern_t)rtw::trace_kernel<T, false, true, true, true, -1, BATCH, ACCUM, ADAPT> : (kern_t)rtw::trace_kernel<T, false, false, true, true, -1, BATCH, ACCUM, ADAPT>;
    else if (cull) kern = lds_scene ? (kern_t)rtw::trace_kernel<T, false, true, true, false, -1, BATCH, ACCUM, ADAPT> : (kern_t)rtw::trace_kernel<T, false, false, true, false, -1, BATCH, ACCUM, ADAPT>;
    else if (mfma) kern = lds_scene ? (kern_t)rtw::trace_kernel<T, false, true, false, true, -1, BATCH, ACCUM, ADAPT> : (kern_t)rtw::trace_kernel<T, false, false, false, true, -1, BATCH, ACCUM, ADAPT>;
    else kern = lds_scene ? (kern_t)rtw::trace_kernel<T, false, true, false, false, -1, BATCH, ACCUM, ADAPT> : (kern_t)rtw::trace_kernel<T, false, false, false, false, -1, BATCH, ACCUM, ADAPT>;
    // the default numerics mode of the headline variants (scene in LDS, matrix pipe): an instance with the mode fixed at compile time
    if (fixed && lds_scene && mfma)
        kern = cull ? (kern_t)rtw::trace_kernel<T, false, true, true, true, rtw::NUM_REFERENCE, BATCH, ACCUM, ADAPT> : (kern_t)rtw::trace_kernel<T, false, true, false, true, rtw::NUM_REFERENCE, BATCH, ACCUM, ADAPT>;
    return (const void *)kern;
}

}  // namespace rtwh
