// ns2d_fast2.hip -- the two-rows-per-lane kernels (ns2d_fast2_impl.h) instantiated for the grid built into the library.
// ns2d_fast2_prm.hip compiles this file a second time with BCN_PRM_KERNELS (ns2d_prm.h): the same grid, kernels that read the
// per-replica table, entry points named *_prm.  Here the BCN_PRM_* macros expand to nothing.
#include "ns2d_builtin.h"
#include "ns2d_fast2_impl.h"

namespace {

// what the two-row family asks of a handle beyond its grid: rayleigh's actions are those of at most one wave
template <typename real>
bool fast2_pre(const NS2DArgs<real>& a) { return a.kind == 1 || a.n_sgts <= 64; }

}  // namespace

template <typename real>
bool BCN_PRM_NAME(ns2d_fast2_supported)(const NS2DArgs<real>& a) {
#define BCN_ROW(REAL, NX, NY, R, KIND, GF) \
  if (BCN_BUILTIN_IS(real, a, REAL, NX, NY, KIND)) return fast2_pre<real>(a);
  BCN_BUILTIN_FAST2(BCN_ROW)
#undef BCN_ROW
  return false;
}

template <typename real>
int BCN_PRM_NAME(ns2d_launch_fast2)(const NS2DArgs<real>& a, int batch, hipStream_t s BCN_PRM_PARAM) {
#define BCN_ROW(REAL, NX, NY, R, KIND, GF)                                                         \
  if constexpr (std::is_same<real, REAL>::value) {                                                 \
    if (BCN_BUILTIN_IS(real, a, REAL, NX, NY, KIND)) return launch_fast2<REAL, NX, NY, R, KIND, GF>(a, batch, s BCN_PRM_ARG); \
  }
  BCN_BUILTIN_FAST2(BCN_ROW)
#undef BCN_ROW
  bcn_set_error("no two-rows-per-lane kernel for this grid");
  return BCN_ERR_UNSUPPORTED;
}

#ifdef BCN_PRM_KERNELS
template bool ns2d_fast2_supported_prm<float>(const NS2DArgs<float>&);
template bool ns2d_fast2_supported_prm<double>(const NS2DArgs<double>&);
template int ns2d_launch_fast2_prm<float>(const NS2DArgs<float>&, int, hipStream_t, const float*);
template int ns2d_launch_fast2_prm<double>(const NS2DArgs<double>&, int, hipStream_t, const double*);
#else
template <typename real>
size_t ns2d_fast2_scratch_elems(const NS2DArgs<real>& a) {
#define BCN_ROW(REAL, NX, NY, R, KIND, GF) \
  if (BCN_BUILTIN_IS(real, a, REAL, NX, NY, KIND)) return Fast2Geom<NX, NY, R, GF>::scratch_elems();
  BCN_BUILTIN_FAST2(BCN_ROW)
#undef BCN_ROW
  return 0;
}
template size_t ns2d_fast2_scratch_elems<float>(const NS2DArgs<float>&);
template size_t ns2d_fast2_scratch_elems<double>(const NS2DArgs<double>&);
template bool ns2d_fast2_supported<float>(const NS2DArgs<float>&);
template bool ns2d_fast2_supported<double>(const NS2DArgs<double>&);
template int ns2d_launch_fast2<float>(const NS2DArgs<float>&, int, hipStream_t);
template int ns2d_launch_fast2<double>(const NS2DArgs<double>&, int, hipStream_t);
#endif
