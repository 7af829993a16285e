// float instantiations of shkadov_warm_k, the device-side random-start reset (env1d_impl.inc: shkadov_action.inc with WARM = true) -- a unit of
// their own: env1d_f32.hip keeps exactly the kernels it had
#define BCN_ENV1D_FLOAT 1
#define BCN_ENV1D_WARM 1
#include "env1d_impl.inc"
