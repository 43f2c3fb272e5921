// rtw_batch_accum_f64.hip -- the double BATCH && ACCUM (&& ADAPT) instances of the trace kernel (rtw_instances.hpp)
#include "rtw_instances.hpp"

namespace rtwh {

TraceInstance batch_accum_kernel_f64(bool cull, bool mfma, bool lds_scene, bool fixed, bool adapt) {
    return adapt ? trace_instance_of<double, true, true, true>(cull, mfma, lds_scene, fixed, false) : trace_instance_of<double, true, true, false>(cull, mfma, lds_scene, fixed, false);
}

}  // namespace rtwh
