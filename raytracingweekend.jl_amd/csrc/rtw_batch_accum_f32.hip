// rtw_batch_accum_f32.hip -- the float BATCH && ACCUM (&& ADAPT) instances of the trace kernel (rtw_batch_accum.hpp)
#include "rtw_batch_accum.hpp"

namespace rtwh {

const void *batch_accum_kernel_f32(bool cull, bool mfma, bool lds_scene, bool fixed, bool adapt) {
    return adapt ? batch_accum_kernel_of<float, true>(cull, mfma, lds_scene, fixed) : batch_accum_kernel_of<float, false>(cull, mfma, lds_scene, fixed);
}

}  // namespace rtwh
