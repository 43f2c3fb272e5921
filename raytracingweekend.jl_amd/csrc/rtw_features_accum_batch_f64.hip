// rtw_features_accum_batch_f64.hip -- the double TILED && BATCH instances of the feature kernel (rtw_features.hpp): the pass over what N adaptive
// accumulators hold in one launch (include/rtw_hip.h rtw_accum_features_batch_*); the table launch_features (rtw_features.hip) selects from
#include "rtw_host.hpp"
#include "rtw_features.hpp"

namespace rtwh {

const void *features_tiled_batch_kernel_f64(bool mfma, bool lds_scene, bool fixed) {
    if (fixed) return (const void *)rtw::features_kernel<double, true, true, rtw::NUM_REFERENCE, true, true>;
    if (mfma) return lds_scene ? (const void *)rtw::features_kernel<double, true, true, -1, true, true> : (const void *)rtw::features_kernel<double, true, false, -1, true, true>;
    return lds_scene ? (const void *)rtw::features_kernel<double, false, true, -1, true, true> : (const void *)rtw::features_kernel<double, false, false, -1, true, true>;
}

}  // namespace rtwh
