// ns2d_fast_runs.hip -- the float32 one-row-per-lane grids of ns2d_builtin.h once more, with the Jacobi cells stated in RUNS
// (BCN_JACOBI_RUNS: several cells per asm statement, bcn_jacobi_cells.h; the same bits, DESIGN.md 6 "slot by slot").  These are the
// kernels a float32 handle on a built-in grid runs: capi.hip asks this unit first.  ns2d_fast.hip keeps its cell-by-cell
// instantiations -- its kernels, those of the on-demand plugins and the table-reading ones are pinned instruction for instruction by
// tests/golden/params_fast_parent_kernels.json -- and stays the path of every handle this unit does not take (float32: 100x50).
// Built with the flags of ns2d_fast.hip (beacon_amd/build.py).
#define BCN_JACOBI_RUNS 1
#include "ns2d_builtin.h"
#include "ns2d_fast_impl.h"

namespace {

bool runs_pre(const NS2DArgs<float>& a) { return a.kind == 0 && a.n_sgts <= 64; }   // as ns2d_fast.hip's fast_pre

// The rows of this unit: float32 with a strip width that takes the runs (jacobi_runs_fit: all but 100x50, R = 10, which
// ns2d_fast.hip keeps).  B = 512, ms per env step, cell by cell -> runs: 128x64 17.40 -> 17.21, 50x50 8.16 -> 8.12,
// 150x50 29.6 -> 28.6, 200x50 40.5 -> 36.7.
template <typename REAL, int R> constexpr bool runs_row() { return std::is_same<REAL, float>::value && jacobi_runs_fit(R); }

}  // namespace

bool ns2d_fast_runs_supported(const NS2DArgs<float>& a) {
#define BCN_ROW(REAL, NX, NY, R, KIND, GF) \
  if (runs_row<REAL, R>() && BCN_BUILTIN_IS(float, a, REAL, NX, NY, KIND)) return runs_pre(a);
  BCN_BUILTIN_FAST(BCN_ROW)
#undef BCN_ROW
  return false;
}

namespace {
template <typename real>
int launch_runs(const NS2DArgs<real>& a, int batch, hipStream_t s) {
#define BCN_ROW(REAL, NX, NY, R, KIND, GF)                                                         \
  if constexpr (std::is_same<real, REAL>::value && runs_row<REAL, R>()) {                     \
    if (BCN_BUILTIN_IS(real, a, REAL, NX, NY, KIND) && runs_pre(a)) return launch_fast<REAL, NX, NY, R, KIND, GF>(a, batch, s); \
  }
  BCN_BUILTIN_FAST(BCN_ROW)
#undef BCN_ROW
  bcn_set_error("no register-resident kernel with cell runs for this grid");
  return BCN_ERR_UNSUPPORTED;
}
}  // namespace

int ns2d_launch_fast_runs(const NS2DArgs<float>& a, int batch, hipStream_t s) { return launch_runs<float>(a, batch, s); }

// 1 where a float32 rayleigh handle on this grid steps through this unit's kernels (for the tests: the kernels of both units carry
// the same names).  Default visibility like bcn_jit_builtin: no part of the ABI of include/beacon_hip.h.
extern "C" __attribute__((visibility("default"))) int bcn_builtin_cell_runs(int nx, int ny) {
  NS2DArgs<float> a{};
  a.nx = nx; a.ny = ny; a.kind = 0; a.n_sgts = 1;
  return ns2d_fast_runs_supported(a) ? 1 : 0;
}
