// float32 instantiation of the ODE env kernels (ode_env.h); contraction to FMA allowed
#define BCN_ODE_IMPL 1
#include "ode_env.h"
BCN_ODE_INSTANTIATE(float)
