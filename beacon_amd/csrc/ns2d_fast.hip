// ns2d_fast.hip -- the register-resident kernels (ns2d_fast_impl.h) instantiated for the grids built into the library:
// the metric grid 128x64 (float32 / float64), the reference's default 50x50 and its other natural aspect ratios.
// Every other grid gets its own instantiation at run time (ns2d_jit.hip, beacon_amd/jit.py).
// ns2d_fast_prm.hip compiles this file a second time with BCN_PRM_KERNELS (ns2d_prm.h): the same grids, kernels that read the
// per-replica table, entry points named *_prm.  Here the BCN_PRM_* macros expand to nothing.
#include "ns2d_builtin.h"
#include "ns2d_fast_impl.h"

namespace {

// what the one-row family asks of a handle beyond its grid: rayleigh, and the actions of at most one wave
template <typename real>
bool fast_pre(const NS2DArgs<real>& a) { return a.kind == 0 && a.n_sgts <= 64; }

}  // namespace

template <typename real>
bool BCN_PRM_NAME(ns2d_fast_supported)(const NS2DArgs<real>& a) {
  if (BCN_PRM_NAME(ns2d_fast2_supported)<real>(a)) return true;
#define BCN_ROW(REAL, NX, NY, R, KIND, GF) \
  if (BCN_BUILTIN_IS(real, a, REAL, NX, NY, KIND)) return fast_pre<real>(a);
  BCN_BUILTIN_FAST(BCN_ROW)
#undef BCN_ROW
  return false;
}

template <typename real>
int BCN_PRM_NAME(ns2d_launch_fast)(const NS2DArgs<real>& a, int batch, hipStream_t s BCN_PRM_PARAM) {
  if (BCN_PRM_NAME(ns2d_fast2_supported)<real>(a)) return BCN_PRM_NAME(ns2d_launch_fast2)<real>(a, batch, s BCN_PRM_ARG);
#define BCN_ROW(REAL, NX, NY, R, KIND, GF)                                                         \
  if constexpr (std::is_same<real, REAL>::value) {                                                 \
    if (BCN_BUILTIN_IS(real, a, REAL, NX, NY, KIND) && fast_pre<real>(a)) return launch_fast<REAL, NX, NY, R, KIND, GF>(a, batch, s BCN_PRM_ARG); \
  }
  BCN_BUILTIN_FAST(BCN_ROW)
#undef BCN_ROW
  bcn_set_error("no register-resident kernel for this grid");
  return BCN_ERR_UNSUPPORTED;
}

#ifndef BCN_PRM_KERNELS   // (the scratch is the handle's: one size for both variants)
template <typename real>
size_t ns2d_fast_scratch_elems(const NS2DArgs<real>& a) {
  if (ns2d_fast2_supported<real>(a)) return ns2d_fast2_scratch_elems<real>(a);
#define BCN_ROW(REAL, NX, NY, R, KIND, GF) \
  if (BCN_BUILTIN_IS(real, a, REAL, NX, NY, KIND) && fast_pre<real>(a)) return FastGeom<NX, NY, R, GF>::scratch_elems();
  BCN_BUILTIN_FAST(BCN_ROW)
#undef BCN_ROW
  return 0;
}
#endif
// One translation unit per precision (ns2d_fast_f64.hip includes this file with BCN_FAST_TU_F64): the two are built with different
// optimisation levels -- the float32 kernels gain 1 % from -O2, the float64 ones lose 0.7 % (beacon_amd/build.py, round 6)
#ifdef BCN_PRM_KERNELS
#ifndef BCN_FAST_TU_F64
template bool ns2d_fast_supported_prm<float>(const NS2DArgs<float>&);
template int ns2d_launch_fast_prm<float>(const NS2DArgs<float>&, int, hipStream_t, const float*);
#else
template bool ns2d_fast_supported_prm<double>(const NS2DArgs<double>&);
template int ns2d_launch_fast_prm<double>(const NS2DArgs<double>&, int, hipStream_t, const double*);
#endif
#elif !defined(BCN_FAST_TU_F64)
template size_t ns2d_fast_scratch_elems<float>(const NS2DArgs<float>&);
template bool ns2d_fast_supported<float>(const NS2DArgs<float>&);
template int ns2d_launch_fast<float>(const NS2DArgs<float>&, int, hipStream_t);
#else
template size_t ns2d_fast_scratch_elems<double>(const NS2DArgs<double>&);
template bool ns2d_fast_supported<double>(const NS2DArgs<double>&);
template int ns2d_launch_fast<double>(const NS2DArgs<double>&, int, hipStream_t);
#endif
