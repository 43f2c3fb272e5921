// rtw_batch_accum_f64.hip -- the double BATCH && ACCUM (&& ADAPT) instances of the trace kernel (rtw_batch_accum.hpp)
#include "rtw_batch_accum.hpp"

namespace rtwh {

const void *batch_accum_kernel_f64(bool cull, bool mfma, bool lds_scene, bool fixed, bool adapt) {
    return adapt ? batch_accum_kernel_of<double, true>(cull, mfma, lds_scene, fixed) : batch_accum_kernel_of<double, false>(cull, mfma, lds_scene, fixed);
}

}  // namespace rtwh
