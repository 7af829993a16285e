// float64 instantiation of the ODE env kernels (ode_env.h); built with -ffp-contract=off (beacon_amd/build.py): the host ports'
// operation order without FMA contraction -> bit-identical trajectories
#define BCN_ODE_IMPL 1
#include "ode_env.h"
BCN_ODE_INSTANTIATE(double)
