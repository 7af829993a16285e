// ns2d_prm.h -- the per-replica parameter variant of the register-resident kernels (bcn_set_option "params_kernel").
//
// ns2d_fast_impl.h, ns2d_fast2_impl.h and ns2d_fast4_impl.h are compiled twice.  A translation unit that defines BCN_PRM_KERNELS
// before it includes them (ns2d_fast_prm.hip, ns2d_fast_prm_f64.hip, ns2d_fast2_prm.hip; jit/ns2d_jit.hip with -DBCN_JIT_PRM=1) gets
// kernels that take the table of bcn_set_params as an argument of their own -- [2][B] (rayleigh: kmom, ksc) / [3][B] (mixing:
// kmom, ksc, u_max) in the handle's dtype, what ns2d_generic_step reads -- and launchers with the table as their last argument.
// Every other unit sees the macros below expand to nothing and preprocesses to the tokens it had before: same kernel names, same
// code (tests/test_params_fast_host.py compares their resources with the commit before).  NS2DArgs is the same in both.
//
// The table is read at the top of a unit of work (fast_unit, fast2_unit, fast4_unit), behind the mask test and in front of every
// field load: the unit overwrites kmom, ksc and (mixing) u_max of a LOCAL copy of the argument block, and every use site stays
// as it is.  A persistent workgroup of the ticket scheduler reloads them for every (chunk, replica) unit it draws.  The replica
// index is made wave-uniform first (in the scheduler it comes out of LDS) and the table is read through the constant address
// space -- it is written by a host copy in front of the launch and only ever read by these kernels --, so the loads are scalar
// loads and the constants stay in scalar registers, like the argument block's.
#pragma once
#include "ns2d.h"

#ifdef BCN_PRM_KERNELS
#define BCN_PRM_NAME(f) f##_prm
#define BCN_PRM_PARAM , const real* prm                              /* host launchers: the device table */
#define BCN_PRM_ARG , prm
#define BCN_PRM_LAUNCH , prm, batch                                  /* kernel launch: the table and the length B of its rows */
#define BCN_PRM_KPARAM , const real* __restrict__ prm, const int prm_b   /* kernels and units */
#define BCN_PRM_KARG , prm, prm_b
#define BCN_PRM_A A_in
#define BCN_PRM_LOCAL(KIND) NS2DArgs<real> A = A_in; bcn_prm_load<real, KIND>(A, prm, prm_b, b);

template <typename real, int KIND>
__device__ __forceinline__ void bcn_prm_load(NS2DArgs<real>& A, const real* prm, const int B, const int b) {
  typedef const __attribute__((address_space(4))) real creal;
  creal* const t = (creal*)prm;
  const int bu = __builtin_amdgcn_readfirstlane(b);
  A.kmom = t[bu];
  A.ksc = t[(size_t)B + bu];
  if (KIND == 1) A.u_max = t[2 * (size_t)B + bu];
}
#else
#define BCN_PRM_NAME(f) f
#define BCN_PRM_PARAM
#define BCN_PRM_ARG
#define BCN_PRM_LAUNCH
#define BCN_PRM_KPARAM
#define BCN_PRM_KARG
#define BCN_PRM_A A
#define BCN_PRM_LOCAL(KIND)
#endif
