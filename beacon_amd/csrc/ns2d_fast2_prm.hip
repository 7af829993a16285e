// ns2d_fast2_prm.hip -- the built-in grid of ns2d_fast2.hip once more, as kernels that read the per-replica parameter table
// (ns2d_prm.h; bcn_set_option "params_kernel"): ns2d_launch_fast2_prm, ns2d_fast2_supported_prm (params.h).
#define BCN_PRM_KERNELS 1
#include "params.h"
#include "ns2d_fast2.hip"
