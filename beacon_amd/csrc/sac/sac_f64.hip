// sac_f64.hip -- the float64 instantiation of the kernels of sac_impl.h (include/beacon_sac.h).  Built with -ffp-contract=off: one
// rounding per written operation, as td3_f64.hip; the layers' sums are explicit fma chains either way.
#include "sac_impl.h"

SAC_DEFINE_LAUNCH(double)
