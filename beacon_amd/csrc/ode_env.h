// ode_env.h -- the two ODE envs (lorenz: lorenz/lorenz.py, vortex: vortex/vortex.py): one lane per replica, the whole state in
// registers for the ndt_act timesteps x 5 stages of the low-storage RK4 of an action step.  Persistent state is structure-of-arrays
// [field][B] (coalesced loads and stores); the observation rows [B][n_obs] of the packed output buffer are staged through LDS so
// that every store instruction of a workgroup writes contiguous bytes (obs_stage 1, the float64 default) or written one row per lane
// (obs_stage 0, the float32 default): whichever measured faster (capi.hip).
// The evaluation order is that of the host ports beacon_amd/lorenz.py:56-66 / beacon_amd/vortex.py:68-84, which are bit-exact
// against the reference's episodes: the float64 instantiations are built with -ffp-contract=off (beacon_amd/build.py).
#pragma once
#include "bcn_common.h"

#define BCN_ODE_NT 256

// state columns (include/beacon_hip.h: bcn_state_elems / bcn_get_state); lorenz keeps its action index u as int32 apart (iu)
enum { LZ_X = 0, LZ_FX = 3, LZ_T = 6, LZ_NREAL = 7, LZ_NSTATE = 8 };
enum { VX_X = 0, VX_FX = 4, VX_T = 8, VX_Y = 9, VX_KMOD = 10, VX_KPHASE = 11, VX_U = 12, VX_NREAL = 14, VX_NSTATE = 14 };

template <typename real>
struct OdeArgs {
  int kind;                 // BCN_LORENZ / BCN_VORTEX
  int batch, ndt_act, n_act, n_obs;
  int obs_stage;            // 1: observation rows through LDS, 0: direct strided stores (bcn_set_option "obs_stage")
  real dt;
  // lorenz (lorenz.py:22-40)
  real sigma, rho, beta;
  // vortex (vortex.py:26-48); derived constants computed in double on the host as the reference does, narrowed once
  real lmbda_re, lmbda_cx, mu_re, mu_cx, alpha_re, alpha_cx, ire;
  real omega_f, m_omega_f_gamma /* -omega_f * gamma */, domega, beta_m;
  real mod_min, dmod /* mod_max - mod_min */, phase_min, dphase /* phase_max - phase_min */;
  real rwd_k /* 2 omega_s gamma */, weight;
  real* st;                 // [n_real][B]
  int32_t* iu;              // lorenz: [B] last action index
  int32_t* stp;
  const uint8_t* mask;
  // per-replica physical parameters (bcn_set_params): [3][B] sigma, rho, beta (lorenz) / [2][B] ire, weight (vortex), one more
  // coalesced column each; NULL: the values above for every replica
  const real* prm;
  // per call
  const void* actions;      // lorenz int32 [B], vortex real [B][2]; NULL = repeat the stored action
  real* obs_out;            // [B][n_obs], may be NULL on reset
  real* rwd_out;
  uint8_t* done;
  uint8_t* trunc;
  int32_t* status;
};

template <typename real> int ode_launch_step(const OdeArgs<real>& a, hipStream_t s);
template <typename real> int ode_launch_reset(const OdeArgs<real>& a, hipStream_t s);
// state copies between the device's [field][B] columns and a caller's [B][n_state] rows (device pointer `ext`)
template <typename real> int ode_launch_pack(const OdeArgs<real>& a, real* ext, hipStream_t s);
template <typename real> int ode_launch_unpack(const OdeArgs<real>& a, const real* ext, hipStream_t s);

// ---------------------------------------------------------------------------------------------------------------------------------
// kernels: compiled by ode_f32.hip / ode_f64.hip only (each with its own flags), never instantiated elsewhere
#ifdef BCN_ODE_IMPL
#include <type_traits>

// Carpenter-Kennedy 5-stage low-storage RK4 (lorenz.py:272-280); A[0] = 0 stays a multiply, as in lsrk4.update
__device__ __forceinline__ double ode_rk_a(int j) {
  return j == 0 ? 0.000000000000000 : j == 1 ? -0.417890474499852 : j == 2 ? -1.192151694642677 : j == 3 ? -1.697784692471528
                                                                                                       : -1.514183444257156;
}
__device__ __forceinline__ double ode_rk_b(int j) {
  return j == 0 ? 0.149659021999229 : j == 1 ? 0.379210312999627 : j == 2 ? 0.822955029386982 : j == 3 ? 0.699450455949122
                                                                                                      : 0.153057247968152;
}

__device__ __forceinline__ float ode_cos(float x) { return cosf(x); }
__device__ __forceinline__ double ode_cos(double x) { return cos(x); }
__device__ __forceinline__ float ode_sin(float x) { return sinf(x); }
__device__ __forceinline__ double ode_sin(double x) { return sin(x); }

// One workgroup's observation rows: obs_out[b0 .. b0 + nb)[NOBS].  STAGE: every lane parks its row in LDS, then the workgroup
// writes the contiguous span element by element (lane i of store k writes element k * NT + i), skipping the rows of masked-off
// replicas.  Otherwise each lane writes its own row (NOBS elements NOBS * esz bytes apart across the lanes of a store).
template <typename real, int NOBS, bool STAGE>
__device__ __forceinline__ void ode_store_obs(real* obs_out, const real (&o)[NOBS], bool live, int b0, int nb) {
  if (!obs_out) return;
  if constexpr (STAGE) {
    __shared__ real sh[BCN_ODE_NT * NOBS];
    __shared__ uint8_t act[BCN_ODE_NT];
#pragma unroll
    for (int i = 0; i < NOBS; i++) sh[threadIdx.x * NOBS + i] = o[i];
    act[threadIdx.x] = live ? 1 : 0;
    __syncthreads();
    real* dst = obs_out + (size_t)b0 * NOBS;
    const int n = nb * NOBS;
#pragma unroll
    for (int k = 0; k < NOBS; k++) {
      const int e = k * BCN_ODE_NT + (int)threadIdx.x;
      if (e < n && act[e / NOBS]) dst[e] = sh[e];
    }
  } else {
    if (!live) return;
    real* dst = obs_out + (size_t)(b0 + (int)threadIdx.x) * NOBS;
#pragma unroll
    for (int i = 0; i < NOBS; i++) dst[i] = o[i];
  }
}

// ---- lorenz: lorenz.py:120-172 (beacon_amd/lorenz.py:52-73) ----------------------------------------------------------------------
template <typename real, bool STAGE>
__global__ __launch_bounds__(BCN_ODE_NT) void lorenz_step_k(OdeArgs<real> A) {
  const int b0 = blockIdx.x * BCN_ODE_NT, b = b0 + (int)threadIdx.x, nb = min(BCN_ODE_NT, A.batch - b0);
  const bool live = b < A.batch && (!A.mask || A.mask[b]);
  real o[6] = {};
  if (live) {
    const size_t B = (size_t)A.batch;
    real* st = A.st;
    real x0 = st[LZ_X * B + b], x1 = st[(LZ_X + 1) * B + b], x2 = st[(LZ_X + 2) * B + b], t = st[LZ_T * B + b];
    int u;
    if (A.actions) {
      u = static_cast<const int32_t*>(A.actions)[b];
      A.iu[b] = u;
    } else {
      u = A.iu[b];
    }
    // self.actions[u] of (-1, 0, 1); an index outside 0..2 applies no force
    const real force = u == 0 ? real(-1) : u == 2 ? real(1) : real(0);
    const real* prm = A.prm;
    const real sigma = prm ? prm[b] : A.sigma, rho = prm ? prm[B + b] : A.rho, beta = prm ? prm[2 * B + b] : A.beta, dt = A.dt;
    real f0 = 0, f1 = 0, f2 = 0;
    for (int n = 0; n < A.ndt_act; n++) {
      real k0 = x0, k1 = x1, k2 = x2;
#pragma unroll
      for (int j = 0; j < 5; j++) {
        const real a = (real)ode_rk_a(j), bb = (real)ode_rk_b(j);
        f0 = sigma * (k1 - k0);
        f1 = k0 * (rho - k2) - k1;
        f2 = k0 * k1 - beta * k2;
        f1 += force;
        x0 = a * x0 + dt * f0; k0 += bb * x0;
        x1 = a * x1 + dt * f1; k1 += bb * x1;
        x2 = a * x2 + dt * f2; k2 += bb * x2;
      }
      x0 = k0; x1 = k1; x2 = k2;
      t += dt;
    }
    st[LZ_X * B + b] = x0; st[(LZ_X + 1) * B + b] = x1; st[(LZ_X + 2) * B + b] = x2;
    st[LZ_FX * B + b] = f0; st[(LZ_FX + 1) * B + b] = f1; st[(LZ_FX + 2) * B + b] = f2;
    st[LZ_T * B + b] = t;
    o[0] = x0; o[1] = x1; o[2] = x2; o[3] = f0; o[4] = f1; o[5] = f2;
    const int s = A.stp[b];
    if (A.rwd_out) A.rwd_out[b] = x0 < real(0) ? real(1) : real(0);
    const uint8_t d = s == A.n_act - 1 ? 1 : 0;
    if (A.done) A.done[b] = d;
    if (A.trunc) A.trunc[b] = d;
    if (A.status) A.status[b] = BCN_ST_OK;
    A.stp[b] = s + 1;
  }
  ode_store_obs<real, 6, STAGE>(A.obs_out, o, live, b0, nb);
}

// lorenz.py:60-95: x = 10, fx = 0, t = 0, u = 1 (no force), stp = 0
template <typename real, bool STAGE>
__global__ __launch_bounds__(BCN_ODE_NT) void lorenz_reset_k(OdeArgs<real> A) {
  const int b0 = blockIdx.x * BCN_ODE_NT, b = b0 + (int)threadIdx.x, nb = min(BCN_ODE_NT, A.batch - b0);
  const bool live = b < A.batch && (!A.mask || A.mask[b]);
  real o[6] = {real(10), real(10), real(10), real(0), real(0), real(0)};
  if (live) {
    const size_t B = (size_t)A.batch;
#pragma unroll
    for (int i = 0; i < 3; i++) { A.st[(LZ_X + i) * B + b] = real(10); A.st[(LZ_FX + i) * B + b] = real(0); }
    A.st[LZ_T * B + b] = real(0);
    A.iu[b] = 1;
    A.stp[b] = 0;
  }
  ode_store_obs<real, 6, STAGE>(A.obs_out, o, live, b0, nb);
}

// ---- vortex: vortex.py:149-209 (beacon_amd/vortex.py:64-100) -----------------------------------------------------------------------
template <typename real, bool STAGE>
__global__ __launch_bounds__(BCN_ODE_NT) void vortex_step_k(OdeArgs<real> A) {
  const int b0 = blockIdx.x * BCN_ODE_NT, b = b0 + (int)threadIdx.x, nb = min(BCN_ODE_NT, A.batch - b0);
  const bool live = b < A.batch && (!A.mask || A.mask[b]);
  real o[8] = {};
  if (live) {
    const size_t B = (size_t)A.batch;
    real* st = A.st;
    real x0 = st[VX_X * B + b], x1 = st[(VX_X + 1) * B + b], x2 = st[(VX_X + 2) * B + b], x3 = st[(VX_X + 3) * B + b];
    real t = st[VX_T * B + b];
    const real yp = st[VX_Y * B + b];
    real u0, u1;
    if (A.actions) {
      const real* ac = static_cast<const real*>(A.actions) + 2 * (size_t)b;
      u0 = ac[0]; u1 = ac[1];
      st[VX_U * B + b] = u0; st[(VX_U + 1) * B + b] = u1;
    } else {
      u0 = st[VX_U * B + b]; u1 = st[(VX_U + 1) * B + b];
    }
    const real kmod = A.mod_min + real(0.5) * (u0 + real(1)) * A.dmod;
    const real kphase = A.phase_min + real(0.5) * (u1 + real(1)) * A.dphase;
    // cos / sin of the phase: the reference evaluates them in every stage; they are the same values
    const real ck = ode_cos(kphase), sk = ode_sin(kphase);
    const real* prm = A.prm;
    const real ire = prm ? prm[b] : A.ire, weight = prm ? prm[B + b] : A.weight;
    const real lre = A.lmbda_re, lcx = A.lmbda_cx, mre = A.mu_re, mcx = A.mu_cx, are = A.alpha_re, acx = A.alpha_cx;
    const real mwg = A.m_omega_f_gamma, dw = A.domega, bm = A.beta_m, dt = A.dt;
    real f0 = 0, f1 = 0, f2 = 0, f3 = 0;
    for (int n = 0; n < A.ndt_act; n++) {
      real k0 = x0, k1 = x1, k2 = x2, k3 = x3;
#pragma unroll
      for (int j = 0; j < 5; j++) {
        const real a = (real)ode_rk_a(j), bb = (real)ode_rk_b(j);
        const real m2 = k0 * k0 + k1 * k1;
        f0 = ire * (lre * k0 - lcx * k1) - (mre * k0 - mcx * k1) * m2 + (are * k2 - acx * k3) + k0 * kmod * ck - k1 * kmod * sk;
        f1 = ire * (lre * k1 + lcx * k0) - (mre * k1 + mcx * k0) * m2 + (are * k3 + acx * k2) + k0 * kmod * sk + k1 * kmod * ck;
        f2 = mwg * k2 - dw * k3 + bm * k0;
        f3 = mwg * k3 + dw * k2 + bm * k1;
        x0 = a * x0 + dt * f0; k0 += bb * x0;
        x1 = a * x1 + dt * f1; k1 += bb * x1;
        x2 = a * x2 + dt * f2; k2 += bb * x2;
        x3 = a * x3 + dt * f3; k3 += bb * x3;
      }
      x0 = k0; x1 = k1; x2 = k2; x3 = k3;
      t += dt;
    }
    // get_rwd (vortex.py:197-208): y of the new time against the previous one
    const real wt = A.omega_f * t;
    const real c = ode_cos(wt), s = ode_sin(wt);
    const real y = real(2) * (x2 * c - x3 * s);
    real cost = real(2) * kmod * ck * (x0 * c - x1 * s) - real(2) * kmod * sk * (x1 * c + x0 * s);
    cost = real(0.5) * (cost * cost);
    const real dy = (y - yp) / dt;
    const real r = A.rwd_k * (dy * dy) - weight * cost;
    st[VX_X * B + b] = x0; st[(VX_X + 1) * B + b] = x1; st[(VX_X + 2) * B + b] = x2; st[(VX_X + 3) * B + b] = x3;
    st[VX_FX * B + b] = f0; st[(VX_FX + 1) * B + b] = f1; st[(VX_FX + 2) * B + b] = f2; st[(VX_FX + 3) * B + b] = f3;
    st[VX_T * B + b] = t; st[VX_Y * B + b] = y;
    st[VX_KMOD * B + b] = kmod; st[VX_KPHASE * B + b] = kphase;
    o[0] = x0; o[1] = x1; o[2] = x2; o[3] = x3; o[4] = f0; o[5] = f1; o[6] = f2; o[7] = f3;
    const int sp = A.stp[b];
    if (A.rwd_out) A.rwd_out[b] = r;
    const uint8_t d = sp == A.n_act - 1 ? 1 : 0;
    if (A.done) A.done[b] = d;
    if (A.trunc) A.trunc[b] = d;
    if (A.status) A.status[b] = BCN_ST_OK;
    A.stp[b] = sp + 1;
  }
  ode_store_obs<real, 8, STAGE>(A.obs_out, o, live, b0, nb);
}

// vortex.py:91-125: the fixed start point, y = _y() at t = 0, u = (0, 0), kmod = kphase = 0
template <typename real, bool STAGE>
__global__ __launch_bounds__(BCN_ODE_NT) void vortex_reset_k(OdeArgs<real> A) {
  const int b0 = blockIdx.x * BCN_ODE_NT, b = b0 + (int)threadIdx.x, nb = min(BCN_ODE_NT, A.batch - b0);
  const bool live = b < A.batch && (!A.mask || A.mask[b]);
  const real x[4] = {real(-0.00385), real(-0.00378), real(0.00118), real(-0.00131)};
  real o[8] = {x[0], x[1], x[2], x[3], real(0), real(0), real(0), real(0)};
  if (live) {
    const size_t B = (size_t)A.batch;
#pragma unroll
    for (int i = 0; i < 4; i++) { A.st[(VX_X + i) * B + b] = x[i]; A.st[(VX_FX + i) * B + b] = real(0); }
    const real c = ode_cos(real(0)), s = ode_sin(real(0));
    A.st[VX_T * B + b] = real(0);
    A.st[VX_Y * B + b] = real(2) * (x[2] * c - x[3] * s);
    A.st[VX_KMOD * B + b] = real(0); A.st[VX_KPHASE * B + b] = real(0);
    A.st[VX_U * B + b] = real(0); A.st[(VX_U + 1) * B + b] = real(0);
    A.stp[b] = 0;
  }
  ode_store_obs<real, 8, STAGE>(A.obs_out, o, live, b0, nb);
}

// state rows <-> columns; lorenz's column LZ_NREAL is the int32 action index
template <typename real>
__global__ __launch_bounds__(BCN_ODE_NT) void ode_pack_k(OdeArgs<real> A, real* ext, const real* in, int out) {
  const int b = blockIdx.x * BCN_ODE_NT + (int)threadIdx.x;
  if (b >= A.batch) return;
  const size_t B = (size_t)A.batch;
  const bool lz = A.kind == BCN_LORENZ;
  const int nreal = lz ? LZ_NREAL : VX_NREAL, nst = lz ? LZ_NSTATE : VX_NSTATE;
  for (int k = 0; k < nreal; k++) {
    if (out) ext[(size_t)b * nst + k] = A.st[k * B + b];
    else A.st[k * B + b] = in[(size_t)b * nst + k];
  }
  if (lz) {
    if (out) ext[(size_t)b * nst + LZ_NREAL] = (real)A.iu[b];
    else A.iu[b] = (int32_t)in[(size_t)b * nst + LZ_NREAL];
  }
}

static inline int ode_grid(int batch) { return (batch + BCN_ODE_NT - 1) / BCN_ODE_NT; }

template <typename real>
int ode_launch_step(const OdeArgs<real>& a, hipStream_t s) {
  const dim3 g(ode_grid(a.batch)), t(BCN_ODE_NT);
  if (a.kind == BCN_LORENZ) {
    if (a.obs_stage) hipLaunchKernelGGL((lorenz_step_k<real, true>), g, t, 0, s, a);
    else hipLaunchKernelGGL((lorenz_step_k<real, false>), g, t, 0, s, a);
  } else {
    if (a.obs_stage) hipLaunchKernelGGL((vortex_step_k<real, true>), g, t, 0, s, a);
    else hipLaunchKernelGGL((vortex_step_k<real, false>), g, t, 0, s, a);
  }
  BCN_HIP(hipGetLastError());
  return BCN_OK;
}

template <typename real>
int ode_launch_reset(const OdeArgs<real>& a, hipStream_t s) {
  const dim3 g(ode_grid(a.batch)), t(BCN_ODE_NT);
  if (a.kind == BCN_LORENZ) hipLaunchKernelGGL((lorenz_reset_k<real, true>), g, t, 0, s, a);   // once per episode: one variant
  else hipLaunchKernelGGL((vortex_reset_k<real, true>), g, t, 0, s, a);
  BCN_HIP(hipGetLastError());
  return BCN_OK;
}

template <typename real>
int ode_launch_pack(const OdeArgs<real>& a, real* ext, hipStream_t s) {
  hipLaunchKernelGGL((ode_pack_k<real>), dim3(ode_grid(a.batch)), dim3(BCN_ODE_NT), 0, s, a, ext, (const real*)nullptr, 1);
  BCN_HIP(hipGetLastError());
  return BCN_OK;
}

template <typename real>
int ode_launch_unpack(const OdeArgs<real>& a, const real* ext, hipStream_t s) {
  hipLaunchKernelGGL((ode_pack_k<real>), dim3(ode_grid(a.batch)), dim3(BCN_ODE_NT), 0, s, a, (real*)nullptr, ext, 0);
  BCN_HIP(hipGetLastError());
  return BCN_OK;
}

#define BCN_ODE_INSTANTIATE(real)                                                   \
  template int ode_launch_step<real>(const OdeArgs<real>&, hipStream_t);            \
  template int ode_launch_reset<real>(const OdeArgs<real>&, hipStream_t);           \
  template int ode_launch_pack<real>(const OdeArgs<real>&, real*, hipStream_t);     \
  template int ode_launch_unpack<real>(const OdeArgs<real>&, const real*, hipStream_t);
#endif  // BCN_ODE_IMPL
