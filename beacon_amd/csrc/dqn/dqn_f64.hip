// dqn_f64.hip -- the float64 instantiation of the kernels of dqn_impl.h (include/beacon_dqn.h).  Built with -ffp-contract=off: one
// rounding per written operation, as td3_f64.hip; the layers' sums are explicit fma chains either way.
#include "dqn_impl.h"

DQN_DEFINE_LAUNCH(double)
