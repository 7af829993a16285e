// td3_f64.hip -- the float64 instantiation of the kernels of td3_impl.h (include/beacon_td3.h).  Built with -ffp-contract=off: one
// rounding per written operation, as actor_f64.hip and learner_f64.hip; the layers' sums are explicit fma chains either way.
#include "td3_impl.h"

TD3_DEFINE_LAUNCH(double)
