// ns2d_jit.hip -- ONE instantiation of the register-resident 2D kernels for a grid that is not built into
// libbeacon_hip.so, compiled on demand by beacon_amd/jit.py into its own small shared object:
//   hipcc ... -DBCN_JIT_ROWS=1|2|4 -DBCN_JIT_REAL=float|double -DBCN_JIT_NX=.. -DBCN_JIT_NY=.. -DBCN_JIT_R=.. -DBCN_JIT_KIND=0|1
//            [-DBCN_JIT_GF=0|1|2] [-DBCN_JIT_RPL=2|3|4] [-DBCN_JIT_PRM=1]
// (ROWS: 1 = ns2d_fast_impl.h, one row per lane, ny <= 64; 2 = ns2d_fast2_impl.h, two rows per lane, 64 < ny <= 128;
//  4 = ns2d_fast4_impl.h, Poisson solve in registers with BCN_JIT_RPL rows per lane, 128 < ny <= 256.)
// The reference takes any L, H (rayleigh.py:20-27: nx = 50 L, ny = 50 H; mixing.py:20-28: 100 L, 100 H); the library
// hands the argument block of a step to bcn_jit_launch through bcn_set_fast_plugin (include/beacon_hip.h).
// -DBCN_JIT_PRM=1: a shared object of its own with the kernels that read the per-replica parameter table (../ns2d_prm.h) and
// bcn_jit_launch_prm (bcn_set_fast_plugin_params); its bcn_jit_launch declines (it holds no kernel that runs without a table).
// Without the flag this file compiles to what it always did.
#if defined(BCN_JIT_PRM) && BCN_JIT_PRM
#define BCN_PRM_KERNELS 1
#endif
#if BCN_JIT_ROWS == 1 && BCN_JIT_KIND != 0
#error "ns2d_fast_impl.h (one row per lane, ny <= 64) implements the rayleigh boundary conditions only: mixing needs BCN_JIT_ROWS=2"
#endif
#if BCN_JIT_ROWS == 1
#ifndef BCN_JACOBI_RUNS     // -DBCN_JACOBI_RUNS=0: the cell-by-cell twin of this grid's kernels (tests/test_gpu_jacobi_cells.py: the same bits)
#define BCN_JACOBI_RUNS 1   // float32, dx == dy: the Jacobi cells in runs where the strip width takes them (../bcn_jacobi_cells.h)
#endif
#include "../ns2d_fast_impl.h"
#elif BCN_JIT_ROWS == 2
#include "../ns2d_fast2_impl.h"
#else
#include "../ns2d_fast4_impl.h"
#endif

#ifndef BCN_JIT_GF
#define BCN_JIT_GF 0
#endif

extern "C" {

#ifdef BCN_PRM_KERNELS
#define BCN_JIT_TABLE , static_cast<const BCN_JIT_REAL*>(table)
__attribute__((visibility("default"))) int bcn_jit_launch(const void*, int, void*) {
  bcn_set_error("kernel plugin built with BCN_JIT_PRM: it holds the table-reading kernels only (bcn_jit_launch_prm)");
  return BCN_ERR_UNSUPPORTED;   // (the library's answer to it: the generic kernel takes the step)
}
__attribute__((visibility("default"))) int bcn_jit_launch_prm(const void* args, int batch, void* stream, const void* table) {
#else
#define BCN_JIT_TABLE
__attribute__((visibility("default"))) int bcn_jit_launch(const void* args, int batch, void* stream) {
#endif
#ifdef BCN_JIT_BREAK   // TEST HOOK (tests/test_gpu_parity.py): a deliberately wrong kernel -- the first-use self-check of beacon_amd/jit.py must refuse it
  // 1: dt x 1.5 (grossly wrong); 2: dt x (1 + BCN_JIT_BREAK_EPS), subtly wrong -- below the self-check's old float32 bound (2e-4)
  // but above its per-field bounds
#ifndef BCN_JIT_BREAK_EPS
#define BCN_JIT_BREAK_EPS 3e-4
#endif
  NS2DArgs<BCN_JIT_REAL> a = *static_cast<const NS2DArgs<BCN_JIT_REAL>*>(args);
#if BCN_JIT_BREAK == 2
  a.dt *= BCN_JIT_REAL(1.0 + BCN_JIT_BREAK_EPS);
#else
  a.dt *= BCN_JIT_REAL(1.5);
#endif
#else
  const NS2DArgs<BCN_JIT_REAL>& a = *static_cast<const NS2DArgs<BCN_JIT_REAL>*>(args);
#endif
  if (a.nx != BCN_JIT_NX || a.ny != BCN_JIT_NY || a.kind != BCN_JIT_KIND) {
    bcn_set_error("kernel plugin built for %dx%d kind %d, handle is %dx%d kind %d", BCN_JIT_NX, BCN_JIT_NY, BCN_JIT_KIND,
                  a.nx, a.ny, a.kind);
    return BCN_ERR_ARG;
  }
#if BCN_JIT_ROWS == 1
  return launch_fast<BCN_JIT_REAL, BCN_JIT_NX, BCN_JIT_NY, BCN_JIT_R, BCN_JIT_KIND, BCN_JIT_GF>(a, batch, static_cast<hipStream_t>(stream) BCN_JIT_TABLE);
#elif BCN_JIT_ROWS == 2
  return launch_fast2<BCN_JIT_REAL, BCN_JIT_NX, BCN_JIT_NY, BCN_JIT_R, BCN_JIT_KIND, BCN_JIT_GF>(a, batch, static_cast<hipStream_t>(stream) BCN_JIT_TABLE);
#else
  return launch_fast4<BCN_JIT_REAL, BCN_JIT_NX, BCN_JIT_NY, BCN_JIT_R, BCN_JIT_RPL, BCN_JIT_KIND>(a, batch, static_cast<hipStream_t>(stream) BCN_JIT_TABLE);
#endif
}

// elements of per-workgroup field scratch the kernel needs (0: its fields live in LDS)
__attribute__((visibility("default"))) size_t bcn_jit_scratch_elems(void) {
#if BCN_JIT_ROWS == 1
  return FastGeom<BCN_JIT_NX, BCN_JIT_NY, BCN_JIT_R, BCN_JIT_GF>::scratch_elems();
#elif BCN_JIT_ROWS == 2
  return Fast2Geom<BCN_JIT_NX, BCN_JIT_NY, BCN_JIT_R, BCN_JIT_GF>::scratch_elems();
#else
  return 0;   // the fields stay where the generic kernel keeps them
#endif
}

__attribute__((visibility("default"))) size_t bcn_jit_lds_bytes(void) {
#if BCN_JIT_ROWS == 1
  return FastGeom<BCN_JIT_NX, BCN_JIT_NY, BCN_JIT_R, BCN_JIT_GF>::lds_bytes<BCN_JIT_REAL>();
#elif BCN_JIT_ROWS == 2
  return Fast2Geom<BCN_JIT_NX, BCN_JIT_NY, BCN_JIT_R, BCN_JIT_GF>::lds_elems() * sizeof(BCN_JIT_REAL);
#else
  return (size_t)Fast4Geom<BCN_JIT_NX, BCN_JIT_NY, BCN_JIT_R, BCN_JIT_RPL>::lds_elems(sizeof(BCN_JIT_REAL)) * sizeof(BCN_JIT_REAL);
#endif
}

// 1 where this plugin's float32 kernels state their Jacobi cells in runs (dx == dy launches)
__attribute__((visibility("default"))) int bcn_jit_cell_runs(void) {
#if BCN_JIT_ROWS == 1
  return BCN_JACOBI_RUNS && std::is_same<BCN_JIT_REAL, float>::value && bcn_dpp::jacobi_runs_fit(BCN_JIT_R) ? 1 : 0;
#else
  return 0;
#endif
}

}  // extern "C"
