// bcn_common.h -- shared host/device helpers for libbeacon_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/beacon_hip.h"

#define BCN_WAVE 64

// Guard of the extrapolating residual plan (bcn_set_option "conv_plan" 3; ns2d_fast_impl.h).  The reference's norm
// err_k = d_k' (I + G) d_k of the Jacobi increments can GROW from one sweep to a later one -- by at most
// C = max_m || W^(1/2) J^m W^(-1/2) ||^2 = 1.0300 over every grid, cell aspect ratio and boundary type computed by
// scripts/weighted_norm_bound.py (1.0166 in one sweep, the maximum after 4..6 sweeps).  So an evaluation that directly
// follows skipped sweeps proves that none of them passed the test (err_j <= tol) exactly when it finds err > C tol.
#define BCN_CONV_GUARD 1.035
// 1.25 log2(BCN_CONV_GUARD * 1.003): the zone in front of a solve's stop that its speculative opening stays clear of, in bits of err
#define BCN_OPEN_ZONE_L2 0.0674f

__attribute__((visibility("default"))) void bcn_set_error(const char* fmt, ...);

#define BCN_HIP(call)                                                                      \
  do {                                                                                     \
    hipError_t e__ = (call);                                                               \
    if (e__ != hipSuccess) {                                                               \
      bcn_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e__)); \
      return BCN_ERR_HIP;                                                                  \
    }                                                                                      \
  } while (0)

// ---- wave / workgroup reductions (wave = 64 lanes) ---------------------------------------
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, BCN_WAVE);
  return v;
}

// Sum over the workgroup; every thread gets the same value (same summation order, so a
// branch on it is uniform).  `red` is LDS scratch of >= NT/64 elements; callers alternate
// between two scratch rows so that ONE barrier per call is enough.
template <typename T, int NT>
__device__ __forceinline__ T block_sum(T v, T* red) {
  constexpr int NW = NT / BCN_WAVE;
  v = wave_sum(v);
  if ((threadIdx.x & (BCN_WAVE - 1)) == 0) red[threadIdx.x / BCN_WAVE] = v;
  __syncthreads();
  T s = red[0];
#pragma unroll
  for (int w = 1; w < NW; w++) s += red[w];
  return s;
}

// |x| as the instruction's source modifier (free); the compare + select form costs two instructions of two issue slots each
__device__ __forceinline__ float bcn_abs(float x) { return __builtin_fabsf(x); }
__device__ __forceinline__ double bcn_abs(double x) { return __builtin_fabs(x); }

// ---- handle ------------------------------------------------------------------------------
struct bcn_env_s {
  int kind = -1;
  int batch = 0;
  int dtype = BCN_F32;
  int device = 0;
  int n_obs = 0;
  int n_act = 0;
  int variant = 0;
  size_t esz = 4;
  virtual ~bcn_env_s() { delete[] prm_host; }
  virtual size_t state_elems() const = 0;
  virtual int get_state(void* buf, int is_device, hipStream_t s) = 0;
  virtual int set_state(const void* buf, int is_device, hipStream_t s) = 0;
  virtual int set_variant(int v) { variant = 0; (void)v; return 0; }
  virtual void set_mask(const uint8_t* m) = 0;
  virtual int set_sched(int, int, int, int) { return BCN_OK; }
  virtual int set_fast_plugin(void*, size_t) { bcn_set_error("this env takes no kernel plugin"); return BCN_ERR_ARG; }
  virtual int set_fast_plugin_params(void*) { bcn_set_error("this env takes no kernel plugin"); return BCN_ERR_ARG; }
  virtual int set_noise(double, uint64_t, int64_t) { bcn_set_error("this env has no inlet noise"); return BCN_ERR_ARG; }
  virtual int set_option(const char* name, int) { bcn_set_error("unknown option '%s' for this env", name); return BCN_ERR_ARG; }
  virtual int set_slow_mode_bound(int, const double*, const double*) { bcn_set_error("this env has no Jacobi solve"); return BCN_ERR_ARG; }
  virtual int get_slow_mode_bound(double*, double*) const { return 0; }
  virtual int get_counters(uint64_t* host, hipStream_t) { memset(host, 0, (size_t)batch * 4 * sizeof(uint64_t)); return BCN_OK; }   // only the 2D register-resident kernels schedule
  virtual const char* kernel_name() const = 0;
  virtual void kernel_shape(int* k, int* nt) const { *k = 0; *nt = 0; }   // (0, 0): the env has no such notion
  virtual int cell_runs_active() const { return 0; }   // 2D envs: the next variant-1 step runs the kernels with Jacobi cell runs
  // per-replica physical parameters (bcn_set_params; params.h)
  virtual void use_params(const void* table) = 0;   // the kernels read `table` from the next launch on (nullptr: the argument block's values)
  void* prm_dev = nullptr;      // [n_derived][B] in the handle's dtype: allocated by the first bcn_set_params, never moved (freed by bcn_destroy)
  double* prm_host = nullptr;   // [n_params][B], the values in force; nullptr: none set (every replica has the cfg's)
  double prm_cfg[3] = {0, 0, 0};   // the cfg's values of the parameters, in the order of bcn_param_name
  double prm_aux[2] = {0, 0};      // what else of the cfg the derived constants need (params.h: bcn_derive_params)
  int32_t* stp = nullptr;  // device int32[B]
  int ndt_act = 0;         // timesteps per action step (rows of the callers' sweeps / noise buffers: bcn_ndt_act)
  uint64_t cfg_hash = 0;   // of the constructor's cfg (bcn_snapshot_signature)
};

// device allocation tracked per handle
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  int alloc(size_t n) {
    bytes = n;
    hipError_t e = hipMalloc(&p, n ? n : 4);
    if (e != hipSuccess) { bcn_set_error("hipMalloc(%zu): %s", n, hipGetErrorString(e)); return BCN_ERR_HIP; }
    return BCN_OK;
  }
  // n elements of T, zeroed; *out = the typed pointer
  template <typename T> int zalloc(size_t n, T** out) {
    const int rc = alloc(n * sizeof(T));
    if (rc) return rc;
    BCN_HIP(hipMemset(p, 0, bytes));
    *out = static_cast<T*>(p);
    return BCN_OK;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; }
};
