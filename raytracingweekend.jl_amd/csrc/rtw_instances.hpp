// rtw_instances.hpp -- the kernel-instance table: the only place that names instances of the trace kernel (rtw_kernels.hpp).  Which one
// runs a scan variant -- group cull, pass 1 on the matrix pipe, the scene in LDS, the default numerics mode compiled in, the phase
// profile -- for one combination of BATCH, ACCUM and ADAPT.  launch_render (rtw_launch.hip) asks it for the plain, the BATCH, the ACCUM
// and the ACCUM && ADAPT instances; the BATCH && ACCUM (&& ADAPT) instances -- one pass of N views' progressive or adaptive renders in
// one launch -- are asked for in translation units of their own, one per precision (rtw_batch_accum_f32.hip / _f64.hip, which pass
// profile = false), so that rtw_launch.hip builds as fast as before and the units compile in parallel.
#pragma once
#include "rtw_scene_view.hpp"
#include "rtw_kernels.hpp"

namespace rtwh {

template <typename T>
using trace_kern_t = void (*)(rtw::KParams, rtw::Camera<T>, rtw::DevScene<T>, rtw::CullScene<T>, T *, rtw::DevCounters *, rtw::BatchArgs<T>, rtw::AccumArgs);

// `fixed`: the numerics mode is the default one, NUM_REFERENCE; `profile`: the phase profile is on (RTW_PHASE_PROFILE).  -> the kernel and
// whether it is the instance with the numerics mode compiled in.  A row per scan variant: the phase-profile pair (scene in LDS, in global
// memory), then the pair without.  The irregularities:
//   - only the plain instances (no BATCH, ACCUM or ADAPT) have phase-profile variants: every other launch ignores `profile` (P is false there);
//   - group cull with the scene in global memory has no PROFILE instance: a phase-profile launch falls back to the non-profile one;
//   - a phase-profile launch never takes the NUM_REFERENCE instance (there is none with the profile).
template <typename T, bool BATCH, bool ACCUM, bool ADAPT>
TraceInstance trace_instance_of(bool cull, bool mfma, bool lds_scene, bool fixed, bool profile) {
    constexpr bool P = !BATCH && !ACCUM && !ADAPT;
    const bool prof = P && profile;
    trace_kern_t<T> kern;
    if (cull && mfma) kern = prof ? (lds_scene ? rtw::trace_kernel<T, P, true, true, true, -1, BATCH, ACCUM, ADAPT> : rtw::trace_kernel<T, false, false, true, true, -1, BATCH, ACCUM, ADAPT>)
                                  : (lds_scene ? rtw::trace_kernel<T, false, true, true, true, -1, BATCH, ACCUM, ADAPT> : rtw::trace_kernel<T, false, false, true, true, -1, BATCH, ACCUM, ADAPT>);
    else if (cull) kern = prof ? (lds_scene ? rtw::trace_kernel<T, P, true, true, false, -1, BATCH, ACCUM, ADAPT> : rtw::trace_kernel<T, false, false, true, false, -1, BATCH, ACCUM, ADAPT>)
                               : (lds_scene ? rtw::trace_kernel<T, false, true, true, false, -1, BATCH, ACCUM, ADAPT> : rtw::trace_kernel<T, false, false, true, false, -1, BATCH, ACCUM, ADAPT>);
    else if (mfma) kern = prof ? (lds_scene ? rtw::trace_kernel<T, P, true, false, true, -1, BATCH, ACCUM, ADAPT> : rtw::trace_kernel<T, P, false, false, true, -1, BATCH, ACCUM, ADAPT>)
                               : (lds_scene ? rtw::trace_kernel<T, false, true, false, true, -1, BATCH, ACCUM, ADAPT> : rtw::trace_kernel<T, false, false, false, true, -1, BATCH, ACCUM, ADAPT>);
    else kern = prof ? (lds_scene ? rtw::trace_kernel<T, P, true, false, false, -1, BATCH, ACCUM, ADAPT> : rtw::trace_kernel<T, P, false, false, false, -1, BATCH, ACCUM, ADAPT>)
                     : (lds_scene ? rtw::trace_kernel<T, false, true, false, false, -1, BATCH, ACCUM, ADAPT> : rtw::trace_kernel<T, false, false, false, false, -1, BATCH, ACCUM, ADAPT>);
    // the default numerics mode of the headline variants (scene in LDS, matrix pipe): an instance with the mode fixed at compile time
    const bool take_fixed = fixed && lds_scene && mfma && !prof;
    if (take_fixed)
        kern = cull ? rtw::trace_kernel<T, false, true, true, true, rtw::NUM_REFERENCE, BATCH, ACCUM, ADAPT> : rtw::trace_kernel<T, false, true, false, true, rtw::NUM_REFERENCE, BATCH, ACCUM, ADAPT>;
    return {(const void *)kern, take_fixed};
}

}  // namespace rtwh
