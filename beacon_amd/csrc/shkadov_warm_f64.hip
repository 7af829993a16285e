// double instantiations of shkadov_warm_k, the device-side random-start reset (env1d_impl.inc: shkadov_action.inc with WARM = true); built with
// -ffp-contract=off like env1d_f64.hip (beacon_amd/build.py): the same operations in the same order as shkadov_step_k<double, ..>
#define BCN_ENV1D_DOUBLE 1
#define BCN_ENV1D_WARM 1
#include "env1d_impl.inc"
