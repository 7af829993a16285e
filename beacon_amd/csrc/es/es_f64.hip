// es_f64.hip -- the float64 instantiation of the kernels of es_impl.h (include/beacon_es.h).  Built with -ffp-contract=off: one
// rounding per written operation, as td3_f64.hip; the layers' sums are explicit fma chains either way.
#include "es_impl.h"

ES_DEFINE_LAUNCH(double)
