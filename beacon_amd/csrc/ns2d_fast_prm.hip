// ns2d_fast_prm.hip -- the built-in grids of ns2d_fast.hip once more, as kernels that read the per-replica parameter table
// (ns2d_prm.h; bcn_set_option "params_kernel"): ns2d_launch_fast_prm, ns2d_fast_supported_prm (params.h).  float32; the float64
// instantiations are ns2d_fast_prm_f64.hip (own compiler flags, like ns2d_fast.hip / ns2d_fast_f64.hip: beacon_amd/build.py).
#define BCN_PRM_KERNELS 1
#define BCN_JACOBI_RUNS 1   // (these kernels are not pinned: the Jacobi cells in runs, as in ns2d_fast_runs.hip)
#include "params.h"
#include "ns2d_fast.hip"
