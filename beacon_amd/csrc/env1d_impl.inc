// env1d_impl.inc -- burgers / shkadov / sloshing action steps, one workgroup per replica.  Compiled twice:
// env1d_f32.hip (float instantiations) and env1d_f64.hip (double instantiations, built with -ffp-contract=off:
// with the reference's operation order and no fused multiply-adds the float64 fields and observations are
// BIT-IDENTICAL to the reference's, see scripts/bit1d.py) -- and twice more with BCN_ENV1D_WARM, for shkadov's random-start reset
// alone (shkadov_warm_f32.hip, shkadov_warm_f64.hip: shkadov_warm_k and its launcher, none of the other kernels and launchers).
//
// Each thread owns K consecutive cells of every state array in registers for the whole
// action step (ndt_act timesteps); per timestep the only traffic is one LDS halo exchange
// (double-buffered: ONE barrier per timestep) -- HBM is touched once on entry and once on
// exit.  Inlet noise is an explicit input (the reference draws it from numpy's global
// stream: burgers.py:127, shkadov.py:204).  Citations: file:line into
// /root/reference/beacon/.
#include <stdlib.h>

#include <type_traits>

#include "bcn_dpp.h"
#include "env1d.h"

namespace {

typedef float bcn_f2 __attribute__((ext_vector_type(2)));   // two cells per v_pk_{add,mul,fma}_f32 (float32 kernels)

template <typename real>
__device__ __forceinline__ real np_clip01(real r) {
  // np.maximum(0, np.minimum(r, 1)): NaN propagates (shkadov.py:500)
  real t = (r > real(1)) ? real(1) : r;
  return (t < real(0)) ? real(0) : t;
}

// float32: one v_med3_f32 (2 issue slots) instead of two compare + select pairs (2 slots per instruction, 8 in all:
// profiles/r02_ubench_pk_issue_costs.log); a NaN argument gives 0 instead of NaN -- its operands are NaN already then
template <>
__device__ __forceinline__ float np_clip01<float>(float r) { return __builtin_amdgcn_fmed3f(r, 0.0f, 1.0f); }

template <typename real>
__device__ __forceinline__ real np_max(real a, real b) {
  return (a > b || a != a) ? a : b;
}

// float32: one v_max_f32 (a NaN operand is dropped instead of propagated: the float32 kernels flag blow-up by magnitude)
template <>
__device__ __forceinline__ float np_max<float>(float a, float b) { return __builtin_fmaxf(a, b); }

// float32 kernels: divisions use a * v_rcp_f32(b) (~1.5 ulp, operands are O(1): no denormal scaling
// needed) and 1/dx is a multiplication; IEEE division costs ~10 VALU instructions and made up 20-40 % of
// the step time.  Burgers' BDF2 update divides by 3 exactly (div3 below: a bare reciprocal constant is a systematic
// bias there).  float64 keeps the reference's divisions.
template <typename real> __device__ __forceinline__ real fdiv(real a, real b) { return a / b; }
template <> __device__ __forceinline__ float fdiv<float>(float a, float b) { return a * __builtin_amdgcn_rcpf(b); }
template <typename real> __device__ __forceinline__ real divc(real a, real c, real rc) { (void)rc; return a / c; }
template <> __device__ __forceinline__ float divc<float>(float a, float c, float rc) { (void)c; return a * rc; }
// x / 3, correctly rounded, in three instructions (float32): q = x * RN(1/3), then one FMA refinement of the remainder
// (10 000 000 random floats: every quotient equal to IEEE division; the bare product differs in 1/3 of them, with a
// bias that compounds to 2e-4 over 12 400 burgers timesteps); IEEE division is ~10 instructions
template <typename real> __device__ __forceinline__ real div3(real x) { return x / real(3); }
template <> __device__ __forceinline__ float div3<float>(float x) {
  const float c = 0x1.555556p-2f;
  const float q = x * c;
  const float r = __builtin_fmaf(-3.0f, q, x);
  return __builtin_fmaf(r, c, q);
}
// van Leer limiter of r = a / b (burgers.py:232-236): (r + |r|) / (1 + r).  float32: multiplied through by b it is
// (a + |a| sgn(b)) / (a + b) -- one reciprocal instead of two (v_rcp_f32 costs four plain instructions), exactly 0 for r < 0
// as the original, 0/0 at r = -1 as the original; float64 keeps the reference's two divisions
template <typename real> __device__ __forceinline__ real vanleer(real a, real b) {
  const real r = a / b;
  return (r + bcn_abs(r)) / (real(1) + r);
}
template <> __device__ __forceinline__ float vanleer<float>(float a, float b) {
  return (a + __builtin_copysignf(a, b)) * __builtin_amdgcn_rcpf(a + b);
}
template <typename real> __device__ __forceinline__ real fsqrt(real a) { return sqrt(a); }
template <> __device__ __forceinline__ float fsqrt<float>(float a) { return __builtin_amdgcn_sqrtf(a); }

// Per-replica physical parameters (bcn_set_params).  One workgroup is one replica (blockIdx.x of gridDim.x), so its parameters are
// wave-uniform: at entry, before any store, a kernel overwrites the fields of ITS OWN by-value copy of the argument block from the
// table [k][B] -- scalar loads into the scalar registers the kernel arguments would have occupied -- and every use site below reads
// A.u_target, A.amp, A.delta_p, A.g, A.alpha as before.
template <typename real>
__device__ __forceinline__ void burgers_params(Env1DArgs<real>& A) {
  if (A.prm) { const size_t B = gridDim.x; const real* __restrict__ p = A.prm + blockIdx.x; A.u_target = p[0]; A.amp = p[B]; }
}
template <typename real>
__device__ __forceinline__ void shkadov_params(Env1DArgs<real>& A) {
  if (A.prm) A.delta_p = A.prm[blockIdx.x];
}
template <typename real>
__device__ __forceinline__ void sloshing_params(Env1DArgs<real>& A) {
  if (A.prm) { const size_t B = gridDim.x; const real* __restrict__ p = A.prm + blockIdx.x; A.amp = p[0]; A.alpha = p[B]; A.g = p[2 * B]; }
}

template <typename real, int NT>
__device__ __forceinline__ void finish(const Env1DArgs<real>& A, int b, real rwd, bool blow, real blow_rwd,
                                       bool blow_overrides_rwd) {
  if (threadIdx.x == 0) {
    const int stp = A.stp[b];
    uint8_t dn = (stp == A.n_act - 1) ? 1 : 0, tr = dn;
    if (blow) { dn = 1; tr = 0; if (blow_overrides_rwd) rwd = blow_rwd; }
    if (A.rwd_out) A.rwd_out[b] = rwd;
    if (A.done) A.done[b] = dn;
    if (A.trunc) A.trunc[b] = tr;
    if (A.status) A.status[b] = blow ? BCN_ST_BLOWUP : BCN_ST_OK;
    A.stp[b] = stp + 1;
  }
}

// =========================================================================================
// burgers (burgers.py:119-166, kernels :230-255)
// =========================================================================================
template <typename real, int NT>
__device__ real burgers_obs_rwd(const Env1DArgs<real>& A, int b, real* red) {
  const real* gu = A.f0 + (size_t)b * A.n;
  if (A.obs_out && threadIdx.x < A.n_obs_pts)
    A.obs_out[(size_t)b * A.n_obs + threadIdx.x] = gu[A.ctrl_pos - A.n_obs_pts + threadIdx.x];
  real loc = 0;
  for (int i = A.ctrl_pos + threadIdx.x; i < A.n; i += NT) loc += bcn_abs(gu[i] - A.u_target);
  return -block_sum<real, NT>(loc, red) * A.dx;
}

// FIT: the grid fills the wave exactly (n == 64 K, one wave: BASELINE configs[1], N = 512 = 64 x 8).  Which cells are the
// inlet, the outflow copy, an end of the limiter is then a property of (lane, k) known at compile time for every k but the
// first and the last: the per-cell masks of the general kernel -- a third of its instructions were v_cndmask -- shrink to
// five selects on "lane 0" / "lane 63", and the limiter of the cell below the lane's first one (ph[0]) is the lane below's
// ph[K], fetched by DPP instead of recomputed (the same operation on the same values: bit-identical; one v_rcp_f32 -- four
// issue slots of a lone wave -- and eight other instructions less per timestep).
template <typename real, int K, int NT, bool FIT = false>
__global__ __launch_bounds__(NT) void burgers_step_k(Env1DArgs<real> A) {
  if (A.mask && !A.mask[blockIdx.x]) return;
  burgers_params(A);
  static_assert(!FIT || NT == 64, "FIT: one wave");
  // NT == 64: the replica is ONE wave -- its halo cells come from the neighbouring lanes by DPP wave shifts, and a
  // timestep needs neither LDS nor a barrier (B = 1024 replicas of 512 cells: 57 -> ~25 us per action step)
  constexpr bool ONEWAVE = (NT == 64);
  constexpr int NB = (2 * NT * K * sizeof(real) <= 65536) ? 2 : 1;
  __shared__ real lds[NB][ONEWAVE ? 1 : NT * K + 1];   // + 1: a slot holding 0 for reads outside the array
  __shared__ real red[NT / BCN_WAVE];
  const int b = blockIdx.x, tid = threadIdx.x, i0 = tid * K, n = A.n;
  real* gu = A.f0 + (size_t)b * n;
  real* gup = A.f1 + (size_t)b * n;
  real* gupp = A.f2 + (size_t)b * n;
  real u[K], up[K], upp[K];
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int c = i0 + k;
    u[k] = c < n ? gu[c] : real(0);
    up[k] = c < n ? gup[c] : real(0);
    upp[k] = c < n ? gupp[c] : real(0);
  }
  const real act = A.actions ? A.actions[b] : A.a_last[b];
  // inlet noise of this action step (burgers.py:127): the caller's, or drawn here (bcn_set_noise)
  const bool dev_noise = !A.noise && A.nsigma > real(0);
  const uint32_t nctr = dev_noise ? A.nctr[b] : 0u;
  const real noise = A.noise ? A.noise[b] : (dev_noise ? bcn_device_noise<real>(A, b, nctr, 0) : real(0));
  if (tid == 0) { A.a_last[b] = act; if (dev_noise) A.nctr[b] = nctr + 1u; }
  const real force = act * A.amp;
  // static per thread: halo indices with the outflow copy u[nx-1] = u[nx-2] (:138) resolved on read
  // (cells outside the array read a slot holding 0: they only feed limiter entries that are masked)
  constexpr int ZERO = NT * K;
  auto hidx = [&](int c) -> int { return (c < 0 || c >= n) ? ZERO : (c == n - 1 ? n - 2 : c); };
  const int xm2 = hidx(i0 - 2), xm1 = hidx(i0 - 1), xp0 = hidx(i0 + K);
  const bool has_last = (i0 <= n - 1) && (n - 1 < i0 + K);
  if constexpr (!ONEWAVE) { if (tid == 0) { lds[0][ZERO] = 0; lds[NB - 1][ZERO] = 0; } }
  // static per thread: which of its cells the update writes (:249 writes 1 .. nx-2), where the limiter is zero
  // (:232-236), the forcing of its cells (:143: only cell ctrl_pos) -- selects instead of branches in the timestep
  bool m_int[K], m_ph[K + 1];
  real fk[K];
#pragma unroll
  for (int k = 0; k < K; k++) { const int c = i0 + k; m_int[k] = (c >= 1 && c <= n - 2); fk[k] = (c == A.ctrl_pos) ? force : real(0); }
#pragma unroll
  for (int k = 0; k <= K; k++) { const int c = i0 - 1 + k; m_ph[k] = !(c <= 0 || c >= n - 1); }
  const bool is0 = (tid == 0);
  const bool is63 = (tid == 63);
  const real inlet = A.u_target + noise;              // burgers.py:137

  // One timestep: X = u, Y = up on entry; the new u goes to Z (the old upp, dead by then), so that the reference's
  // "upp = up; up = u" (:133-134) is a renaming (X becomes up, Y becomes upp), not 2K register copies.
  auto step = [&](real (&X)[K], real (&Y)[K], real (&Z)[K], const int it) {
    real cur[K];   // this thread's cells with the inlet value (:137) and the outflow copy (:138) in place
#pragma unroll
    for (int k = 0; k < K; k++) cur[k] = X[k];
    cur[0] = is0 ? inlet : cur[0];
    real e[K + 3];  // cells i0-2 .. i0+K
    if constexpr (FIT) {
      // cell n-1 = (lane 63, k = K-1) takes the outflow copy u[nx-1] = u[nx-2] (:138); lane 0 reads zeros below itself
      cur[K - 1] = is63 ? cur[K > 1 ? K - 2 : 0] : cur[K - 1];
      e[0] = real(0);                                  // (cell i0-2 only feeds ph[0], which comes from the lane below here)
      e[1] = bcn_dpp::from_below(real(0), cur[K - 1]);
      e[K + 2] = bcn_dpp::from_above(real(0), cur[0]);
    } else if constexpr (ONEWAVE) {
      // lanes outside the array hold zeros, lane 0 reads zeros
      const real lb = bcn_dpp::from_below(real(0), cur[K - 1]);
#pragma unroll
      for (int k = 0; k < K; k++) {
        const bool last = has_last && (i0 + k == n - 1);
        cur[k] = last ? ((k > 0) ? cur[k > 0 ? k - 1 : 0] : lb) : cur[k];
      }
      e[0] = bcn_dpp::from_below(real(0), K > 1 ? cur[K > 1 ? K - 2 : 0] : bcn_dpp::from_below(real(0), cur[0]));
      e[1] = bcn_dpp::from_below(real(0), cur[K - 1]);
      e[K + 2] = bcn_dpp::from_above(real(0), cur[0]);
    } else {
      real* L = lds[it & (NB - 1)];
#pragma unroll
      for (int k = 0; k < K; k++) L[i0 + k] = cur[k];
      __syncthreads();
      e[0] = L[xm2];
      e[1] = L[xm1];
      const real um = L[has_last ? n - 2 : 0];
#pragma unroll
      for (int k = 0; k < K; k++) cur[k] = (has_last && i0 + k == n - 1) ? um : cur[k];
      e[K + 2] = L[xp0];
    }
#pragma unroll
    for (int k = 0; k < K; k++) e[k + 2] = cur[k];
    real ph[K + 1];  // limiter at cells i0-1 .. i0+K-1 (zero at both ends, :232-236)
    if constexpr (FIT) {
#pragma unroll
      for (int k = 1; k <= K; k++) ph[k] = vanleer<real>(e[k + 1] - e[k], e[k + 2] - e[k + 1] + real(1.0e-8));
      ph[1] = is0 ? real(0) : ph[1];                   // cell 0
      ph[K] = is63 ? real(0) : ph[K];                  // cell n-1
      ph[0] = bcn_dpp::from_below(real(0), ph[K]);     // cell i0-1: the lane below's ph[K]; lane 0 (cell -1): 0
    } else {
#pragma unroll
      for (int k = 0; k <= K; k++) {
        real f = vanleer<real>(e[k + 1] - e[k], e[k + 2] - e[k + 1] + real(1.0e-8));
        ph[k] = m_ph[k] ? f : real(0);
      }
    }
#pragma unroll
    for (int k = 0; k < K; k++) {
      real fp = e[k + 2] + real(0.5) * ph[k + 1] * (e[k + 3] - e[k + 2]);
      real fm = e[k + 1] + real(0.5) * ph[k] * (e[k + 2] - e[k + 1]);
      real du = divc<real>(fp - fm, A.dx, A.rdx);
      real rhs = e[k + 2] * du + fk[k];               // :143 (+ 0 elsewhere)
      real un = div3<real>(real(4) * X[k] - Y[k] - real(2) * A.dt * rhs);   // :246-249
      if constexpr (FIT) Z[k] = (k == 0 ? is0 : (k == K - 1 ? is63 : false)) ? cur[k] : un;   // cells 0 and n-1 are not updated (:249)
      else Z[k] = m_int[k] ? un : cur[k];
    }
    if (!ONEWAVE && NB == 1) __syncthreads();
  };
  int it = 0;
  for (; it + 3 <= A.ndt_act; it += 3) {
    step(u, up, upp, it);
    step(upp, u, up, it + 1);
    step(up, upp, u, it + 2);
  }
  const int rem = A.ndt_act - it;
  if (rem >= 1) step(u, up, upp, it);
  if (rem >= 2) step(upp, u, up, it + 1);
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int c = i0 + k;
    // (u, up, upp) after 0 / 1 / 2 remaining steps: (u, up, upp) / (upp, u, up) / (up, upp, u)
    const real fu = rem == 0 ? u[k] : (rem == 1 ? upp[k] : up[k]);
    const real fup = rem == 0 ? up[k] : (rem == 1 ? u[k] : upp[k]);
    const real fupp = rem == 0 ? upp[k] : (rem == 1 ? up[k] : u[k]);
    if (c < n) { gu[c] = fu; gup[c] = fup; gupp[c] = fupp; }
  }
  __syncthreads();
  real rwd = burgers_obs_rwd<real, NT>(A, b, red);
  finish<real, NT>(A, b, rwd, false, real(0), false);
}

#ifdef BCN_ENV1D_FLOAT
// float32, n == 64 K (K = 8: BASELINE configs[1], N = 512; K = 4: N = 256), ONE wave, PACKED: a lone wave issues one vector
// instruction per 4 cycles whatever its width (MI355X_MICROARCH.md, "vector-instruction ISSUE cost"), and B = 1024 replicas are
// one wave per SIMD -- so what counts is the number of instructions, and v_pk_{add,mul,fma}_f32 do two cells in one.  Lane l
// holds its K cells as H = K/2 register PAIRS (cell k, cell k + H), k = 0 .. H-1: every stencil neighbour of a pair -- cells
// k-1, k+1 and k+H-1, k+H+1 -- is then again an aligned pair, and only the two halo pairs (cells -1 | H-1 and H | K) are
// assembled from a DPP wave shift and a half of an existing pair.  The flux at the lower face of a cell is the upper-face flux
// of the cell below (burgers.py:238-244: the same expression on the same values), so one flux pair per cell pair plus one DPP
// serves both faces, and the limiter is evaluated K times per lane, not K + 1.  Per cell the operations are those of
// burgers_step_k<float, K, 64, true> (hipcc contracts a few multiply-adds differently: last-bit differences, the same distance
// from the float64 oracle: tests/test_gpu_parity.py); per timestep 137 -> 94 instructions, none of them a wait state.  Prologue and epilogue: two 128-bit loads / stores per array and lane, observations and reward taken from the
// registers (the general kernel stores the fields and reads them back through L2 behind a barrier).
// FIT: n == 64 K.  Otherwise (the reference's own nx = 500: 64 K - 12) the last cell sits somewhere inside a lane: the outflow copy,
// the limiter's zero and "not updated" at cell n-1 become per-lane masks (17 instructions per timestep more), lanes past the
// array hold zeros that nothing updates.
template <int K, bool FIT>
__global__ __launch_bounds__(64) void burgers_step_pk_k(Env1DArgs<float> A) {
  if (A.mask && !A.mask[blockIdx.x]) return;
  burgers_params(A);
  static_assert(K == 8 || K == 4, "pairs (k, k + K/2), vector loads of K/2 cells");
  constexpr int H = K / 2;
  typedef float fH __attribute__((ext_vector_type(H)));
  const int b = blockIdx.x, lane = threadIdx.x, n = A.n, i0 = lane * K;
  float* const gu = A.f0 + (size_t)b * n + i0;
  float* const gup = A.f1 + (size_t)b * n + i0;
  float* const gupp = A.f2 + (size_t)b * n + i0;
  bcn_f2 u[H], up[H], upp[H];
  if constexpr (FIT) {
    const fH a0 = *(const fH*)gu, a1 = *(const fH*)(gu + H), b0 = *(const fH*)gup, b1 = *(const fH*)(gup + H);
    const fH c0 = *(const fH*)gupp, c1 = *(const fH*)(gupp + H);
#pragma unroll
    for (int j = 0; j < H; j++) { u[j] = (bcn_f2){a0[j], a1[j]}; up[j] = (bcn_f2){b0[j], b1[j]}; upp[j] = (bcn_f2){c0[j], c1[j]}; }
  } else {
#pragma unroll
    for (int j = 0; j < H; j++) {
      const bool in0 = i0 + j < n, in1 = i0 + j + H < n;
      u[j] = (bcn_f2){in0 ? gu[j] : 0.f, in1 ? gu[j + H] : 0.f};
      up[j] = (bcn_f2){in0 ? gup[j] : 0.f, in1 ? gup[j + H] : 0.f};
      upp[j] = (bcn_f2){in0 ? gupp[j] : 0.f, in1 ? gupp[j + H] : 0.f};
    }
  }
  // !FIT: per-lane masks of the last cell / of the cells the update writes (1 .. n-2, :249) / where the limiter is not zero
  bool mlast[K], mupd[K];
#pragma unroll
  for (int k = 0; k < K; k++) { const int c = i0 + k; mlast[k] = (c == n - 1); mupd[k] = (c >= 1 && c <= n - 2); }
  const float act = A.actions ? A.actions[b] : A.a_last[b];
  const bool dev_noise = !A.noise && A.nsigma > 0.f;
  const uint32_t nctr = dev_noise ? A.nctr[b] : 0u;
  const float noise = A.noise ? A.noise[b] : (dev_noise ? bcn_device_noise<float>(A, b, nctr, 0) : 0.f);
  if (lane == 0) { A.a_last[b] = act; if (dev_noise) A.nctr[b] = nctr + 1u; }
  const float force = act * A.amp;
  bcn_f2 fk[H];   // the forcing acts on cell ctrl_pos only (burgers.py:143)
#pragma unroll
  for (int j = 0; j < H; j++) fk[j] = (bcn_f2){i0 + j == A.ctrl_pos ? force : 0.f, i0 + j + H == A.ctrl_pos ? force : 0.f};
  const bool is0 = (lane == 0), is63 = (lane == 63);
  const float inlet = A.u_target + noise;              // burgers.py:137
  const bcn_f2 eps2 = 1.0e-8f, half2 = 0.5f, rdx2 = A.rdx, four2 = 4.f, m2dt2 = -2.f * A.dt, c3 = 0x1.555556p-2f, m3 = -3.f;

  // One timestep: X = u, Y = up on entry, the new u goes to Z (see burgers_step_k)
  auto step = [&](bcn_f2 (&X)[H], bcn_f2 (&Y)[H], bcn_f2 (&Z)[H]) {
    bcn_f2 C[H + 2];   // C[j + 1] = cells (j, j + H), j = -1 .. H, with the inlet value (:137) and the outflow copy (:138) in place
#pragma unroll
    for (int j = 0; j < H; j++) C[j + 1] = X[j];
    C[1].x = is0 ? inlet : C[1].x;                                   // cell 0
    if constexpr (FIT) {
      C[H].y = is63 ? C[H - 1].y : C[H].y;                           // cell n-1 = u[nx-2]
    } else {
      // the one cell that is n-1 takes the cell below it (which is not n-1: any order of these selects reads unmodified values)
      const float below0 = bcn_dpp::from_below(0.f, C[H].y);
#pragma unroll
      for (int j = H - 1; j >= 1; j--) { C[j + 1].y = mlast[j + H] ? C[j].y : C[j + 1].y; C[j + 1].x = mlast[j] ? C[j].x : C[j + 1].x; }
      C[1].y = mlast[H] ? C[H].x : C[1].y;
      C[1].x = mlast[0] ? below0 : C[1].x;
    }
    C[H + 1] = (bcn_f2){C[1].y, bcn_dpp::from_above(0.f, C[1].x)};   // cells H | K (the lane above's first; lane 63: 0, unused)
    C[0] = (bcn_f2){bcn_dpp::from_below(0.f, C[H].y), C[H].x};       // cells -1 (the lane below's last; lane 0: 0) | H-1
    bcn_f2 D[H + 1];   // D[j] = upper-face difference of cells (j-1, j+H-1)
#pragma unroll
    for (int j = 0; j <= H; j++) D[j] = C[j + 1] - C[j];
    // Stage by stage over the H pairs, not pair by pair: a packed instruction that reads the result of the one before it costs a
    // wait state (s_nop, 4 cycles of a lone wave); the H independent chains side by side need none.
    bcn_f2 F[H], sm[H], num[H], ph[H], t[H], q[H];   // F: upper-face flux of cells (j, j + H)
    // van Leer limiter of r = a / bb (burgers.py:232-236) as in vanleer<float>: (a + |a| sgn(bb)) / (a + bb), a = D[j], bb = D[j+1] + eps
#pragma unroll
    for (int j = 0; j < H; j++) { ph[j] = D[j + 1] + eps2; t[j] = __builtin_elementwise_fma(four2, X[j], -Y[j]); }   // (t: :246-249)
#pragma unroll
    for (int j = 0; j < H; j++) sm[j] = D[j] + ph[j];
#pragma unroll
    for (int j = 0; j < H; j++) num[j] = D[j] + (bcn_f2){__builtin_copysignf(D[j].x, ph[j].x), __builtin_copysignf(D[j].y, ph[j].y)};
#pragma unroll
    for (int j = 0; j < H; j++) sm[j] = (bcn_f2){__builtin_amdgcn_rcpf(sm[j].x), __builtin_amdgcn_rcpf(sm[j].y)};
#pragma unroll
    for (int j = 0; j < H; j++) ph[j] = num[j] * sm[j];
    if constexpr (FIT) {
      ph[0].x = is0 ? 0.f : ph[0].x;                                  // cell 0 (:232-236: zero at both ends)
      ph[H - 1].y = is63 ? 0.f : ph[H - 1].y;                         // cell n-1
#pragma unroll
      for (int j = 0; j < H; j++) ph[j] = half2 * ph[j];
    } else {
#pragma unroll
      for (int j = 0; j < H; j++) { ph[j].x = mupd[j] ? ph[j].x : 0.f; ph[j].y = mupd[j + H] ? ph[j].y : 0.f; }   // (selects: a 0/0 there must not spread)
#pragma unroll
      for (int j = 0; j < H; j++) ph[j] = half2 * ph[j];
    }
#pragma unroll
    for (int j = 0; j < H; j++) F[j] = __builtin_elementwise_fma(ph[j], D[j + 1], C[j + 1]);
    const bcn_f2 Fm = (bcn_f2){bcn_dpp::from_below(0.f, F[H - 1].y), F[H - 1].x};   // faces below cells 0 | H
#pragma unroll
    for (int j = 0; j < H; j++) q[j] = F[j] - (j == 0 ? Fm : F[j > 0 ? j - 1 : 0]);
#pragma unroll
    for (int j = 0; j < H; j++) q[j] = q[j] * rdx2;                                                  // du
#pragma unroll
    for (int j = 0; j < H; j++) q[j] = __builtin_elementwise_fma(C[j + 1], q[j], fk[j]);             // rhs (:143)
#pragma unroll
    for (int j = 0; j < H; j++) t[j] = __builtin_elementwise_fma(m2dt2, q[j], t[j]);                 // 4 u - up - 2 dt rhs
#pragma unroll
    for (int j = 0; j < H; j++) q[j] = t[j] * c3;                                                    // t / 3: div3<float>
#pragma unroll
    for (int j = 0; j < H; j++) t[j] = __builtin_elementwise_fma(m3, q[j], t[j]);
#pragma unroll
    for (int j = 0; j < H; j++) Z[j] = __builtin_elementwise_fma(t[j], c3, q[j]);
    if constexpr (FIT) {
      Z[0].x = is0 ? C[1].x : Z[0].x;                                // cells 0 and n-1 are not updated (:249)
      Z[H - 1].y = is63 ? C[H].y : Z[H - 1].y;
    } else {
#pragma unroll
      for (int j = 0; j < H; j++) { Z[j].x = mupd[j] ? Z[j].x : C[j + 1].x; Z[j].y = mupd[j + H] ? Z[j].y : C[j + 1].y; }
    }
  };
  int it = 0;
  for (; it + 3 <= A.ndt_act; it += 3) {
    step(u, up, upp);
    step(upp, u, up);
    step(up, upp, u);
  }
  const int rem = A.ndt_act - it;
  if (rem >= 1) step(u, up, upp);
  if (rem >= 2) step(upp, u, up);
  fH o[6];
  float loc = 0.f;
  const int obs0 = A.ctrl_pos - A.n_obs_pts;
  float* const obs = A.obs_out ? A.obs_out + (size_t)b * A.n_obs : nullptr;
#pragma unroll
  for (int j = 0; j < H; j++) {
    // (u, up, upp) after 0 / 1 / 2 remaining steps: (u, up, upp) / (upp, u, up) / (up, upp, u)
    const bcn_f2 fu = rem == 0 ? u[j] : (rem == 1 ? upp[j] : up[j]);
    const bcn_f2 fup = rem == 0 ? up[j] : (rem == 1 ? u[j] : upp[j]);
    const bcn_f2 fupp = rem == 0 ? upp[j] : (rem == 1 ? up[j] : u[j]);
    o[0][j] = fu.x; o[1][j] = fu.y; o[2][j] = fup.x; o[3][j] = fup.y; o[4][j] = fupp.x; o[5][j] = fupp.y;
    // observations: the n_obs_pts cells upstream of the control (:150-153); reward: -dx sum |u - u_target| downstream (:155-158)
    const int c0 = i0 + j, c1 = i0 + j + H;
    if (obs && c0 >= obs0 && c0 < A.ctrl_pos) obs[c0 - obs0] = fu.x;
    if (obs && c1 >= obs0 && c1 < A.ctrl_pos) obs[c1 - obs0] = fu.y;
    loc += ((c0 >= A.ctrl_pos && c0 < n) ? bcn_abs(fu.x - A.u_target) : 0.f) + ((c1 >= A.ctrl_pos && c1 < n) ? bcn_abs(fu.y - A.u_target) : 0.f);
    if constexpr (!FIT) {
      if (c0 < n) { gu[j] = fu.x; gup[j] = fup.x; gupp[j] = fupp.x; }
      if (c1 < n) { gu[j + H] = fu.y; gup[j + H] = fup.y; gupp[j + H] = fupp.y; }
    }
  }
  if constexpr (FIT) {
    *(fH*)gu = o[0]; *(fH*)(gu + H) = o[1];
    *(fH*)gup = o[2]; *(fH*)(gup + H) = o[3];
    *(fH*)gupp = o[4]; *(fH*)(gupp + H) = o[5];
  }
  const float rwd = -bcn_dpp::read_lane(bcn_dpp::wave_sum_lane63<float>(loc), 63) * A.dx;
  finish<float, 64>(A, b, rwd, false, 0.f, false);
}
#endif

template <typename real, int NT>
__global__ __launch_bounds__(NT) void burgers_reset_k(Env1DArgs<real> A) {
  if (A.mask && !A.mask[blockIdx.x]) return;
  burgers_params(A);
  __shared__ real red[NT / BCN_WAVE];
  const int b = blockIdx.x, n = A.n;
  for (int c = threadIdx.x; c < n; c += NT) {
    A.f0[(size_t)b * n + c] = A.u_target;
    A.f1[(size_t)b * n + c] = A.u_target;
    A.f2[(size_t)b * n + c] = A.u_target;
  }
  if (threadIdx.x == 0) { A.a_last[b] = 0; A.stp[b] = 0; }
  __syncthreads();
  (void)burgers_obs_rwd<real, NT>(A, b, red);
}

// =========================================================================================
// shkadov (shkadov.py:188-264, kernels :484-518)
// =========================================================================================
template <typename real, int NT>
__device__ real shkadov_obs_rwd(const Env1DArgs<real>& A, int b, real* red, bool* blow) {
  const real* gh = A.f0 + (size_t)b * A.n;
  const real* gq = A.f1 + (size_t)b * A.n;
  if (A.obs_out)
    for (int k = threadIdx.x; k < A.n_obs; k += NT) {
      const int j = k / A.n_obs_jet, m = k - j * A.n_obs_jet;
      const int s = A.jet_pos + j * A.jet_space - A.l_obs;
      A.obs_out[(size_t)b * A.n_obs + k] = gq[s + m * A.obs_stride];
    }
  real loc = 0;
  for (int k = threadIdx.x; k < A.n_jets * A.l_rwd; k += NT) {
    const int j = k / A.l_rwd, m = k - j * A.l_rwd;
    const real d = gh[A.jet_pos + j * A.jet_space + m] - real(1);
    loc += d * d;
  }
  real bl = 0;
  for (int c = threadIdx.x; c < A.n; c += NT) {
    const real hv = gh[c];
    // shkadov.py:176: h outside +-5 h_max; a NaN film (which the reference's comparisons let pass, and which the float32
    // limiter's v_med3 / v_max no longer propagate into every cell) counts as blown up as well
    if (!(hv >= -A.h_blow && hv <= A.h_blow)) bl = 1;
  }
  real tot = block_sum<real, NT>(loc, red);
  __syncthreads();
  *blow = block_sum<real, NT>(bl, red) > real(0);
  return -(tot * A.dx) / (real)(A.n_jets * A.l_rwd);
}

// shkadov_step_k and shkadov_warm_k (the device-side random-start reset, shkadov.py:119-123) share ONE body, shkadov_action.inc,
// included into both with the compile-time flag WARM, so that the two cannot drift apart.  It is an included text and not an
// inlined function on purpose: with WARM = false the compiler sees the statements the step kernel always had, and the gfx950 code
// of env1d_f32.hip / env1d_f64.hip is the code of before, instruction for instruction (an always-inlined function and a plain
// `for` around the timesteps each changed register allocation and scheduling of every shkadov_step_k).
// WARM = false: one action step of the replica -- load, ndt_act timesteps, store, observation, reward, flags.
// WARM = true: the replica is reset in registers (shkadov_reset_k's values), takes n_warm action steps of the zero action under
// device noise without leaving the chip, and is stored once: fields, stp = 0, the observation row, n_out -- and no rwd / done /
// trunc / status (in step_autoreset those rows hold the terminal step's values).  n_warm comes from n_steps (clamped to [0,
// rand_steps]) or from the env's Philox stream: counter (replica, nctr, 0, 1) -- word 3 is 0 in every noise draw -- mapped by
// umulhi(word, rand_steps + 1); the count costs one tick of nctr whatever its source.  Between two action steps the state is
// rounded as the store and reload of 1 + h' round it (float32), the cells past the array take their reload values again, the next
// noise row is staged, and a barrier on each side of that staging separates the last read of an exchange buffer from its next
// write (an odd ndt_act ends and starts on the same buffer).  A blow-up is not evaluated during the warm-up (the reference prints
// and carries on); the first real step reports it.
template <typename real, int K, int NT>
__global__ __launch_bounds__(NT) void shkadov_step_k(Env1DArgs<real> A) {
  if (A.mask && !A.mask[blockIdx.x]) return;
  shkadov_params(A);
  constexpr bool WARM = false;
  const int32_t* const n_steps = nullptr;
  int32_t* const n_out = nullptr;
  const int rand_steps = 0;
#include "shkadov_action.inc"
}

#ifdef BCN_ENV1D_WARM
// shkadov.reset with rand_init (shkadov.py:113-146), one launch (see above).  Instantiated in shkadov_warm_f32.hip /
// shkadov_warm_f64.hip only.
template <typename real, int K, int NT>
__global__ __launch_bounds__(NT) void shkadov_warm_k(Env1DArgs<real> A, const int32_t* __restrict__ n_steps, const int rand_steps,
                                                     int32_t* __restrict__ n_out) {
  if (A.mask && !A.mask[blockIdx.x]) return;
  shkadov_params(A);
  constexpr bool WARM = true;
#include "shkadov_action.inc"
}
#endif

template <typename real, int NT>
__global__ __launch_bounds__(NT) void shkadov_reset_k(Env1DArgs<real> A) {
  if (A.mask && !A.mask[blockIdx.x]) return;
  shkadov_params(A);
  __shared__ real red[NT / BCN_WAVE];
  const int b = blockIdx.x, n = A.n;
  for (int c = threadIdx.x; c < n; c += NT) {
    A.f0[(size_t)b * n + c] = A.init_fields ? A.init_fields[c] : real(1);
    A.f1[(size_t)b * n + c] = A.init_fields ? A.init_fields[n + c] : real(1);
    A.f2[(size_t)b * n + c] = 0;
    A.f3[(size_t)b * n + c] = 0;
  }
  if (threadIdx.x < A.n_jets) {
    A.a_last[(size_t)b * A.n_jets + threadIdx.x] = 0;
    A.a_prev[(size_t)b * A.n_jets + threadIdx.x] = 0;
  }
  if (threadIdx.x == 0) A.stp[b] = 0;
  __syncthreads();
  bool blow;
  (void)shkadov_obs_rwd<real, NT>(A, b, red, &blow);
}

// =========================================================================================
// sloshing (sloshing.py:168-244, kernels :322-331); arrays have n = nx+2 entries
// =========================================================================================
template <typename real, int NT>
__device__ real sloshing_obs_rwd(const Env1DArgs<real>& A, int b, real ua, real* red, bool* blow) {
  const real* gh = A.f0 + (size_t)b * A.n;
  const real* gq = A.f1 + (size_t)b * A.n;
  if (A.obs_out)
    for (int k = threadIdx.x; k < A.n_obs; k += NT) A.obs_out[(size_t)b * A.n_obs + k] = gq[1 + 2 * k];
  real loc = 0, bl = 0;
  for (int c = threadIdx.x; c < A.n; c += NT) {
    const real hv = gh[c];
    if (c >= 1 && c <= A.nx) { const real d = hv - real(1); loc += d * d; }
    if (!(hv >= real(-5) && hv <= real(2))) bl = 1;     // sloshing.py:156 (and NaN: see shkadov)
  }
  real tot = block_sum<real, NT>(loc, red);
  __syncthreads();
  *blow = block_sum<real, NT>(bl, red) > real(0);
  return -(sqrt(tot) * A.dx) - A.alpha * bcn_abs(A.amp * ua);
}

template <typename real, int K, int NT>
__global__ __launch_bounds__(NT) void sloshing_step_k(Env1DArgs<real> A) {
  if (A.mask && !A.mask[blockIdx.x]) return;
  sloshing_params(A);
  constexpr bool ONEWAVE = (NT == 64);   // one wave per replica: halos by DPP wave shifts, no LDS, no barrier (see burgers)
  constexpr int NB = (4 * NT * K * sizeof(real) <= 65536) ? 2 : 1;
  __shared__ real lh[NB][ONEWAVE ? 1 : NT * K + 1];   // + 1: a slot holding 1 (h) / 0 (q) for reads outside the array
  __shared__ real lq[NB][ONEWAVE ? 1 : NT * K + 1];
  __shared__ real red[NT / BCN_WAVE];
  const int b = blockIdx.x, tid = threadIdx.x, i0 = tid * K, n = A.n, nx = A.nx;
  real* gh = A.f0 + (size_t)b * n;
  real* gq = A.f1 + (size_t)b * n;
  real* grh = A.f2 + (size_t)b * n;
  real* grq = A.f3 + (size_t)b * n;
  real h[K], q[K], rh[K], rq[K];
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int c = i0 + k;
    h[k] = c < n ? gh[c] : real(1);
    q[k] = c < n ? gq[c] : real(0);
    rh[k] = c < n ? grh[c] : real(0);
    rq[k] = c < n ? grq[c] : real(0);
  }
  const real uo = A.a_last[b];
  const real un = A.actions ? A.actions[b] : uo;
  __syncthreads();
  if (tid == 0) { A.a_last[b] = un; A.a_prev[b] = uo; }
  const real g = A.g;
  // static per thread: halo indices with the wall BCs h[0]=h[1], q[0]=0, h[nx+1]=h[nx], q[nx+1]=0 (:184-187)
  // resolved on read
  constexpr int SLOT = NT * K;
  auto hh = [&](int c) -> int { return (c < 0 || c >= n) ? SLOT : (c == 0 ? 1 : (c == n - 1 ? n - 2 : c)); };
  auto hq = [&](int c) -> int { return (c <= 0 || c >= n - 1) ? SLOT : c; };
  const int xhm = hh(i0 - 1), xhp = hh(i0 + K), xqm = hq(i0 - 1), xqp = hq(i0 + K);
  const bool has_wall = (i0 == 0) || ((i0 <= n - 1) && (n - 1 < i0 + K));
  if constexpr (!ONEWAVE) { if (tid == 0) { lh[0][SLOT] = 1; lh[NB - 1][SLOT] = 1; lq[0][SLOT] = 0; lq[NB - 1][SLOT] = 0; } }
  // static per thread: which of its cells are the two wall cells / are updated (:213-218 writes 1 .. nx) -- selects instead
  // of branches in the timestep (a divergent branch is an exec save, a skip branch and a restore: three issue slots of a lone wave)
  bool m_w0[K], m_wn[K], m_upd[K];
#pragma unroll
  for (int k = 0; k < K; k++) { const int c = i0 + k; m_w0[k] = (c == 0); m_wn[k] = (c == n - 1); m_upd[k] = (c >= 1 && c <= nx); }

  for (int it = 0; it < A.ndt_act; it++) {
    real eh[K + 2], eq[K + 2];  // cells i0-1 .. i0+K
    if constexpr (ONEWAVE) {
      // wall cells first (h[0] = h[1], h[nx+1] = h[nx], q = 0: :184-187), then the halos; lanes outside the array
      // hold h = 1, q = 0, and the missing neighbours of lanes 0 / 63 read the same
      const real hb = bcn_dpp::from_below(real(1), h[K - 1]), ha = bcn_dpp::from_above(real(1), h[0]);
      {
        real hn[K];
#pragma unroll
        for (int k = 0; k < K; k++) {
          const real up1 = (k < K - 1) ? h[k < K - 1 ? k + 1 : 0] : ha, dn1 = (k > 0) ? h[k > 0 ? k - 1 : 0] : hb;
          hn[k] = m_w0[k] ? up1 : (m_wn[k] ? dn1 : h[k]);
        }
#pragma unroll
        for (int k = 0; k < K; k++) { h[k] = hn[k]; q[k] = (m_w0[k] || m_wn[k]) ? real(0) : q[k]; }
      }
      eh[0] = bcn_dpp::from_below(real(1), h[K - 1]); eq[0] = bcn_dpp::from_below(real(0), q[K - 1]);
      eh[K + 1] = bcn_dpp::from_above(real(1), h[0]); eq[K + 1] = bcn_dpp::from_above(real(0), q[0]);
    } else {
      real* Lh = lh[it & (NB - 1)];
      real* Lq = lq[it & (NB - 1)];
#pragma unroll
      for (int k = 0; k < K; k++) { Lh[i0 + k] = h[k]; Lq[i0 + k] = q[k]; }
      __syncthreads();
      eh[0] = Lh[xhm]; eq[0] = Lq[xqm];
      if (has_wall) {
#pragma unroll
        for (int k = 0; k < K; k++) {
          const int c = i0 + k;
          if (c == 0 || c == n - 1) { h[k] = Lh[c == 0 ? 1 : n - 2]; q[k] = real(0); }
        }
      }
      eh[K + 1] = Lh[xhp]; eq[K + 1] = Lq[xqp];
    }
#pragma unroll
    for (int k = 0; k < K; k++) {
      eh[k + 1] = h[k];
      eq[k + 1] = q[k];
    }
    real ev[K + 2], eg[K + 2], es[K + 2];  // v, q^2/h + g h^2/2, |v| + sqrt(g h) (:193-199)
#pragma unroll
    for (int k = 0; k < K + 2; k++) {
      ev[k] = fdiv<real>(eq[k], eh[k]);
      eg[k] = fdiv<real>(eq[k] * eq[k], eh[k]) + real(0.5) * g * (eh[k] * eh[k]);
      es[k] = bcn_abs(ev[k]) + fsqrt<real>(g * eh[k]);
    }
    const real alpha = fmin((real)it / (real)A.n_interp, real(1));
    const real uu = (real(1) - alpha) * uo + alpha * un;
#pragma unroll
    for (int k = 0; k < K; k++) {
      const int c = i0 + k;
      const real cl = np_max(es[k], es[k + 1]);        // c[c-1]
      const real cr = np_max(es[k + 1], es[k + 2]);    // c[c]
      // rusanov (:322-325)
      real fhg = real(0.5) * (eq[k] + eq[k + 1]) - real(0.5) * cl * (eh[k + 1] - eh[k]);
      real fhd = real(0.5) * (eq[k + 1] + eq[k + 2]) - real(0.5) * cr * (eh[k + 2] - eh[k + 1]);
      real fqg = real(0.5) * (eg[k] + eg[k + 1]) - real(0.5) * cl * (eq[k + 1] - eq[k]);
      real fqd = real(0.5) * (eg[k + 1] + eg[k + 2]) - real(0.5) * cr * (eq[k + 2] - eq[k + 1]);
      real rhn = divc<real>(fhd - fhg, A.dx, A.rdx);
      real rqn = divc<real>(fqd - fqg, A.dx, A.rdx) + uu * A.amp;      // :213-218
      {
        const real rhp = rh[k], rqp = rq[k];
        const real hu = h[k] + real(0.5) * A.dt * (real(-3) * rhn + rhp);  // adams (:328-331)
        const real qu = q[k] + real(0.5) * A.dt * (real(-3) * rqn + rqp);
        rh[k] = m_upd[k] ? rhn : rhp;
        rq[k] = m_upd[k] ? rqn : rqp;
        h[k] = m_upd[k] ? hu : h[k];
        q[k] = m_upd[k] ? qu : q[k];
      }
    }
    if (!ONEWAVE && NB == 1) __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int c = i0 + k;
    if (c < n) { gh[c] = h[k]; gq[c] = q[k]; grh[c] = rh[k]; grq[c] = rq[k]; }
  }
  __syncthreads();
  bool blow;
  real rwd = sloshing_obs_rwd<real, NT>(A, b, un, red, &blow);
  finish<real, NT>(A, b, rwd, blow, real(0), false);  // the -10 blow-up reward is dead code (:156-160)
}

#ifdef BCN_ENV1D_FLOAT
// float32, one wave with four cells per lane (n <= 256: the reference's nx = 200), PACKED -- as burgers_step_pk_k: a lone wave
// pays 4 cycles per instruction whatever its width, so a lane's cells are the pairs (c0, c2), (c1, c3), whose stencil neighbours
// are pairs again.  Three more changes carry as much: (1) the Rusanov flux (:322-325) is evaluated per FACE, once -- the upper face
// of a cell is the lower face of the next (the same expression on the same values), the face above the lane's last cell comes
// from the lane above by DPP; (2) v, q^2/h + g h^2/2 and |v| + sqrt(g h) (:193-199) are computed for the lane's own cells only and
// the one halo cell's come from the lane below by DPP (the kernel it replaces evaluates them for six cells per lane: 6 v_rcp, 6
// v_sqrt, 8 cycles each); (3) "not updated" (walls, lanes past the array) is a 0 in the increment's factor instead of a select per
// field and cell, and the wall conditions (:184-187) are two selects on the two lanes concerned.  195 -> ~95 instructions per
// timestep.  Observations, reward and the blow-up flag from the registers.
template <int K>
__global__ __launch_bounds__(64) void sloshing_step_pk_k(Env1DArgs<float> A) {
  if (A.mask && !A.mask[blockIdx.x]) return;
  sloshing_params(A);
  static_assert(K == 4, "pairs (c0, c2), (c1, c3)");
  typedef bcn_f2 f2;
  const int b = blockIdx.x, lane = threadIdx.x, n = A.n, nx = A.nx, i0 = lane * K;
  float* const gh = A.f0 + (size_t)b * n;
  float* const gq = A.f1 + (size_t)b * n;
  float* const grh = A.f2 + (size_t)b * n;
  float* const grq = A.f3 + (size_t)b * n;
  float hs[K], qs[K], rhs_[K], rqs[K];
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int c = i0 + k;
    hs[k] = c < n ? gh[c] : 1.f;
    qs[k] = c < n ? gq[c] : 0.f;
    rhs_[k] = c < n ? grh[c] : 0.f;
    rqs[k] = c < n ? grq[c] : 0.f;
  }
  f2 hP[2] = {{hs[0], hs[2]}, {hs[1], hs[3]}}, qP[2] = {{qs[0], qs[2]}, {qs[1], qs[3]}};
  f2 rhP[2] = {{rhs_[0], rhs_[2]}, {rhs_[1], rhs_[3]}}, rqP[2] = {{rqs[0], rqs[2]}, {rqs[1], rqs[3]}};
  const float uo = A.a_last[b];
  const float un = A.actions ? A.actions[b] : uo;
  // the forcing of every timestep (:213-218: (1 - alpha) u_old + alpha u_new, alpha = min(it / n_interp, 1)), times amp: once
  __shared__ float s_ua[64];
  if (lane < A.ndt_act) {
    const float alpha = fminf((float)lane / (float)A.n_interp, 1.f);
    s_ua[lane] = ((1.f - alpha) * uo + alpha * un) * A.amp;
  }
  __syncthreads();
  if (lane == 0) { A.a_last[b] = un; A.a_prev[b] = uo; }
  // the walls: cell 0 (lane 0) and cell n-1 = (lane lw, cell kw of the lane), kw >= 1: its lower neighbour is the lane's own
  const int lw = (n - 1) / K, kw = (n - 1) - lw * K;
  const bool isL = (lane == 0), w1 = (lane == lw && kw == 1), w2 = (lane == lw && kw == 2), w3 = (lane == lw && kw == 3);
  // factors: 0 where q is a wall value / where a cell is not updated (:213-218 write 1 .. nx), else 1 (times dt / 2 for the update)
  f2 keepq[2], upd[2], updt[2], crh[2], crq[2];
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const int c0 = i0 + j, c1 = i0 + j + 2;
    keepq[j] = (f2){(c0 == 0 || c0 == n - 1) ? 0.f : 1.f, (c1 == 0 || c1 == n - 1) ? 0.f : 1.f};
    upd[j] = (f2){(c0 >= 1 && c0 <= nx) ? 1.f : 0.f, (c1 >= 1 && c1 <= nx) ? 1.f : 0.f};
    updt[j] = upd[j] * (0.5f * A.dt);
    crh[j] = ((f2)1.f - upd[j]) * rhP[j];      // the rhs arrays of cells that are never updated keep what they hold
    crq[j] = ((f2)1.f - upd[j]) * rqP[j];
  }
  const f2 hg2 = 0.5f * A.g, g2 = A.g, half2 = 0.5f, mhalf2 = -0.5f, rdx2 = A.rdx, cm3 = -3.f;
  auto FMA = [](const f2 a, const f2 b, const f2 c) -> f2 { return __builtin_elementwise_fma(a, b, c); };
  auto below = [](const float v) -> float { return bcn_dpp::from_below(0.f, v); };
  for (int it = 0; it < A.ndt_act; it++) {
    // wall cells (:184-187): h[0] = h[1], h[nx+1] = h[nx], q = 0
    hP[0].x = isL ? hP[1].x : hP[0].x;
    hP[1].x = w1 ? hP[0].x : hP[1].x;
    hP[0].y = w2 ? hP[1].x : hP[0].y;
    hP[1].y = w3 ? hP[0].y : hP[1].y;
    qP[0] = qP[0] * keepq[0]; qP[1] = qP[1] * keepq[1];
    // v = q / h, G = q^2 / h + g h^2 / 2, S = |v| + sqrt(g h) of the lane's cells (:193-199)
    f2 r[2], G[2], S[2];
#pragma unroll
    for (int j = 0; j < 2; j++) r[j] = (f2){__builtin_amdgcn_rcpf(hP[j].x), __builtin_amdgcn_rcpf(hP[j].y)};
#pragma unroll
    for (int j = 0; j < 2; j++) { S[j] = g2 * hP[j]; G[j] = (qP[j] * qP[j]) * r[j]; r[j] = qP[j] * r[j]; }
#pragma unroll
    for (int j = 0; j < 2; j++) { S[j] = (f2){__builtin_amdgcn_sqrtf(S[j].x), __builtin_amdgcn_sqrtf(S[j].y)}; G[j] = FMA(hg2 * hP[j], hP[j], G[j]); }
#pragma unroll
    for (int j = 0; j < 2; j++) S[j] = (f2){__builtin_fabsf(r[j].x) + S[j].x, __builtin_fabsf(r[j].y) + S[j].y};
    // the cells below the pairs: (c-1, c1) and (c0, c2)
    const f2 hL[2] = {{below(hP[1].y), hP[1].x}, hP[0]}, qL[2] = {{below(qP[1].y), qP[1].x}, qP[0]};
    const f2 GL[2] = {{below(G[1].y), G[1].x}, G[0]}, SL[2] = {{below(S[1].y), S[1].x}, S[0]};
    // rusanov (:322-325) at the faces below cells (0, 2) and (1, 3)
    f2 Fh[2], Fq[2];
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const f2 cc = (f2){__builtin_fmaxf(SL[j].x, S[j].x), __builtin_fmaxf(SL[j].y, S[j].y)} * half2;
      Fh[j] = FMA(-cc, hP[j] - hL[j], half2 * (qL[j] + qP[j]));
      Fq[j] = FMA(-cc, qP[j] - qL[j], half2 * (GL[j] + G[j]));
    }
    // ... and above them: faces (1, 3) are the pair above, faces (2, 4) = (face 2, the lane above's face 0)
    const f2 FhU = (f2){Fh[0].y, bcn_dpp::from_above(0.f, Fh[0].x)}, FqU = (f2){Fq[0].y, bcn_dpp::from_above(0.f, Fq[0].x)};
    const f2 ua2 = s_ua[it];
    f2 rhn[2], rqn[2];
    rhn[0] = (Fh[1] - Fh[0]) * rdx2; rhn[1] = (FhU - Fh[1]) * rdx2;                     // :213-218
    rqn[0] = FMA(Fq[1] - Fq[0], rdx2, ua2); rqn[1] = FMA(FqU - Fq[1], rdx2, ua2);
#pragma unroll
    for (int j = 0; j < 2; j++) {   // adams (:328-331); cells that are not updated keep h, q and their rhs
      hP[j] = FMA(updt[j], FMA(cm3, rhn[j], rhP[j]), hP[j]);
      qP[j] = FMA(updt[j], FMA(cm3, rqn[j], rqP[j]), qP[j]);
      rhP[j] = FMA(upd[j], rhn[j], crh[j]);
      rqP[j] = FMA(upd[j], rqn[j], crq[j]);
    }
  }
  (void)mhalf2;
  // store; observations q[1 + 2 k] (:150), reward -(sqrt(sum (h - 1)^2 over 1 .. nx) dx) - alpha |amp u| (:152-155), blow-up (:156)
  float loc = 0.f;
  bool bl = false;
  float* const obs = A.obs_out ? A.obs_out + (size_t)b * A.n_obs : nullptr;
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int c = i0 + k;
    const float hv = (k & 1) ? (k == 1 ? hP[1].x : hP[1].y) : (k == 0 ? hP[0].x : hP[0].y);
    const float qv = (k & 1) ? (k == 1 ? qP[1].x : qP[1].y) : (k == 0 ? qP[0].x : qP[0].y);
    const float rhv = (k & 1) ? (k == 1 ? rhP[1].x : rhP[1].y) : (k == 0 ? rhP[0].x : rhP[0].y);
    const float rqv = (k & 1) ? (k == 1 ? rqP[1].x : rqP[1].y) : (k == 0 ? rqP[0].x : rqP[0].y);
    if (c < n) {
      gh[c] = hv; gq[c] = qv; grh[c] = rhv; grq[c] = rqv;
      if (c >= 1 && c <= nx) { const float d = hv - 1.f; loc += d * d; }
      if (!(hv >= -5.f && hv <= 2.f)) bl = true;
      if (obs && (c & 1) && (c >> 1) < A.n_obs) obs[c >> 1] = qv;
    }
  }
  const float tot = bcn_dpp::read_lane(bcn_dpp::wave_sum_lane63<float>(loc), 63);
  const bool blow = __builtin_amdgcn_ballot_w64(bl) != 0;
  const float rwd = -(sqrtf(tot) * A.dx) - A.alpha * bcn_abs(A.amp * un);
  finish<float, 64>(A, b, rwd, blow, 0.f, false);
}
#endif

template <typename real, int NT>
__global__ __launch_bounds__(NT) void sloshing_reset_k(Env1DArgs<real> A) {
  if (A.mask && !A.mask[blockIdx.x]) return;
  sloshing_params(A);
  __shared__ real red[NT / BCN_WAVE];
  const int b = blockIdx.x, n = A.n;
  for (int c = threadIdx.x; c < n; c += NT) {
    A.f0[(size_t)b * n + c] = A.init_fields ? A.init_fields[c] : real(1);
    A.f1[(size_t)b * n + c] = A.init_fields ? A.init_fields[n + c] : real(0);
    A.f2[(size_t)b * n + c] = 0;
    A.f3[(size_t)b * n + c] = 0;
  }
  if (threadIdx.x == 0) { A.a_last[b] = 0; A.a_prev[b] = 0; A.stp[b] = 0; }
  __syncthreads();
  bool blow;
  (void)sloshing_obs_rwd<real, NT>(A, b, real(0), red, &blow);
}

// ---- (K, NT) selection: NT*K >= n ------------------------------------------------------------
// K cells per thread, NT threads per replica.  Fewer cells per thread = more waves per replica: the
// per-timestep work of a thread is a dependent chain (halo exchange -> stencil -> update), so small
// batches of short grids want K small (more waves per SIMD to hide it), long grids want K = 8 (less
// halo traffic per cell).  pick_k(): 4 cells per thread up to 4096 cells (8 beyond), 2 when that leaves
// the chip with fewer than ~8 waves per CU; bcn_set_option "cells_per_thread" overrides (tests / tuning).
inline int pick_k(int n, int batch, int force) {
  static int ncu = 0;
  if (ncu <= 0) {
    int dev = 0;
    ncu = 256;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
  }
  if (force == 1 || force == 2 || force == 4 || force == 8) return (n <= force * 1024) ? force : 8;
  // measured (scripts/exp_1dk.sh, B=1024): burgers N=512 K=8/4/2/1 -> 0.121/0.099/0.096/0.103 ms,
  // sloshing N=202 0.148/0.081/0.079/0.090 ms, shkadov N=4096 K=8/4 -> 1.146/0.937 ms
  int k = (n > 4096) ? 8 : 4;
  if (k == 4 && n <= 2048 && (long)batch * ((n + 255) / 256) < 8L * ncu) k = 2;
  return k;
}
// burgers / sloshing up to 512 cells: ONE wave per replica (K = 1, 2, 4 or 8 cells per lane), halos by DPP
inline int pick_k_onewave(int n, int one_wave) {
  if (!one_wave || n > 512) return 0;
  return n <= 64 ? 1 : (n <= 128 ? 2 : (n <= 256 ? 4 : 8));
}

// (K, NT) of the instantiation that is launched goes to the caller's Env1DLaunch (env1d.h): bcn_kernel_shape reports it
// (... : further kernel arguments behind the argument block)
#define BCN_LAUNCH_NT_(KERNEL, K_, NT_, A, BATCH, STREAM, NOTE, ...)                                            \
  do {                                                                                                          \
    hipLaunchKernelGGL((KERNEL<real, K_, NT_>), dim3(BATCH), dim3(NT_), 0, STREAM, A, ##__VA_ARGS__);           \
    (NOTE)->k = K_; (NOTE)->nt = NT_;                                                                           \
  } while (0)
#define BCN_LAUNCH_NT(KERNEL, K_, A, BATCH, STREAM, NOTE, ...)                                                  \
  do {                                                                                                          \
    const int n__ = (A).n;                                                                                      \
    if (n__ <= K_ * 64) BCN_LAUNCH_NT_(KERNEL, K_, 64, A, BATCH, STREAM, NOTE, ##__VA_ARGS__);                                 \
    else if (n__ <= K_ * 128) BCN_LAUNCH_NT_(KERNEL, K_, 128, A, BATCH, STREAM, NOTE, ##__VA_ARGS__);                          \
    else if (n__ <= K_ * 256) BCN_LAUNCH_NT_(KERNEL, K_, 256, A, BATCH, STREAM, NOTE, ##__VA_ARGS__);                          \
    else if (n__ <= K_ * 512) BCN_LAUNCH_NT_(KERNEL, K_, 512, A, BATCH, STREAM, NOTE, ##__VA_ARGS__);                          \
    else BCN_LAUNCH_NT_(KERNEL, K_, 1024, A, BATCH, STREAM, NOTE, ##__VA_ARGS__);                                              \
  } while (0)

#define BCN_DISPATCH_1D(KERNEL, A, BATCH, STREAM, ONEWAVE_OK, NOTE, ...)                       \
  do {                                                                                         \
    if ((A).n > 8 * 1024) {                                                                    \
      bcn_set_error("1D grid of %d cells exceeds the 8192-cell kernel limit", (A).n);          \
      return BCN_ERR_UNSUPPORTED;                                                              \
    }                                                                                          \
    int k__ = (ONEWAVE_OK) ? pick_k_onewave((A).n, (A).one_wave) : 0;                          \
    if (k__ == 0) k__ = pick_k((A).n, BATCH, (A).force_k);                                     \
    while ((A).n > k__ * 1024) k__ *= 2;                                                       \
    switch (k__) {                                                                             \
      case 1: BCN_LAUNCH_NT(KERNEL, 1, A, BATCH, STREAM, NOTE, ##__VA_ARGS__); break;                         \
      case 2: BCN_LAUNCH_NT(KERNEL, 2, A, BATCH, STREAM, NOTE, ##__VA_ARGS__); break;                         \
      case 4: BCN_LAUNCH_NT(KERNEL, 4, A, BATCH, STREAM, NOTE, ##__VA_ARGS__); break;                         \
      default: BCN_LAUNCH_NT(KERNEL, 8, A, BATCH, STREAM, NOTE, ##__VA_ARGS__); break;                        \
    }                                                                                          \
    BCN_HIP(hipGetLastError());                                                                \
  } while (0)

}  // namespace

#ifdef BCN_ENV1D_WARM
// The same (K, NT) as shkadov_launch_step picks for this handle (cells_per_thread, one_wave; float32: the packed timestep under
// the same conditions), so that the result is what reset + n[b] masked steps compute
template <typename real> int shkadov_launch_warm(const Env1DArgs<real>& a, int batch, const int32_t* n_steps, int rand_steps, int32_t* n_out,
                                                 hipStream_t s, Env1DLaunch* note) {
  if (a.n_jets > 64) { bcn_set_error("n_jets > 64 unsupported"); return BCN_ERR_UNSUPPORTED; }
  BCN_DISPATCH_1D(shkadov_warm_k, a, batch, s, false, note, n_steps, rand_steps, n_out);
  note->name = "shkadov_warm_k";
  return BCN_OK;
}
#ifdef BCN_ENV1D_FLOAT
template int shkadov_launch_warm<float>(const Env1DArgs<float>&, int, const int32_t*, int, int32_t*, hipStream_t, Env1DLaunch*);
#endif
#ifdef BCN_ENV1D_DOUBLE
template int shkadov_launch_warm<double>(const Env1DArgs<double>&, int, const int32_t*, int, int32_t*, hipStream_t, Env1DLaunch*);
#endif
#else   // the step and reset launchers: env1d_f32.hip / env1d_f64.hip

template <typename real> int burgers_launch_step(const Env1DArgs<real>& a, int batch, hipStream_t s, Env1DLaunch* note) {
#ifdef BCN_ENV1D_FLOAT
  if constexpr (std::is_same<real, float>::value) {   // float32, 129 .. 511 cells that do not fill the wave (the reference's nx = 500): packed, with masks
    if (a.one_wave == 1 && a.force_k == 0 && a.n > 128 && a.n < 512 && a.n != 256 && a.ctrl_pos >= a.n_obs_pts && a.ctrl_pos <= a.n) {
      if (a.n > 256) hipLaunchKernelGGL((burgers_step_pk_k<8, false>), dim3(batch), dim3(64), 0, s, a);
      else hipLaunchKernelGGL((burgers_step_pk_k<4, false>), dim3(batch), dim3(64), 0, s, a);
      *note = {"burgers_step_pk_k", a.n > 256 ? 8 : 4, 64};
      BCN_HIP(hipGetLastError());
      return BCN_OK;
    }
  }
#endif
  // a grid that fills one wave exactly (n = 64 K: BASELINE configs[1], N = 512): the kernel without per-cell masks (FIT)
  if (a.one_wave && a.force_k == 0 && (a.n == 512 || a.n == 256 || a.n == 128)) {
#ifdef BCN_ENV1D_FLOAT
    if constexpr (std::is_same<real, float>::value) {   // float32: the packed kernel (two cells per instruction)
      if (a.one_wave == 1 && (a.n == 512 || a.n == 256) && a.ctrl_pos >= a.n_obs_pts && a.ctrl_pos <= a.n) {
        if (a.n == 512) hipLaunchKernelGGL((burgers_step_pk_k<8, true>), dim3(batch), dim3(64), 0, s, a);
        else hipLaunchKernelGGL((burgers_step_pk_k<4, true>), dim3(batch), dim3(64), 0, s, a);
        *note = {"burgers_step_pk_k", a.n / 64, 64};
        BCN_HIP(hipGetLastError());
        return BCN_OK;
      }
    }
#endif
    if (a.n == 512) hipLaunchKernelGGL((burgers_step_k<real, 8, 64, true>), dim3(batch), dim3(64), 0, s, a);
    else if (a.n == 256) hipLaunchKernelGGL((burgers_step_k<real, 4, 64, true>), dim3(batch), dim3(64), 0, s, a);
    else hipLaunchKernelGGL((burgers_step_k<real, 2, 64, true>), dim3(batch), dim3(64), 0, s, a);
    *note = {nullptr, a.n / 64, 64};   // FIT: n == 64 K
    BCN_HIP(hipGetLastError());
    return BCN_OK;
  }
  BCN_DISPATCH_1D(burgers_step_k, a, batch, s, true, note);
  return BCN_OK;
}
template <typename real> int burgers_launch_reset(const Env1DArgs<real>& a, int batch, hipStream_t s) {
  hipLaunchKernelGGL((burgers_reset_k<real, 64>), dim3(batch), dim3(64), 0, s, a);
  BCN_HIP(hipGetLastError());
  return BCN_OK;
}
template <typename real> int shkadov_launch_step(const Env1DArgs<real>& a, int batch, hipStream_t s, Env1DLaunch* note) {
  if (a.n_jets > 64) { bcn_set_error("n_jets > 64 unsupported"); return BCN_ERR_UNSUPPORTED; }
  BCN_DISPATCH_1D(shkadov_step_k, a, batch, s, false, note);
  return BCN_OK;
}
template <typename real> int shkadov_launch_reset(const Env1DArgs<real>& a, int batch, hipStream_t s) {
  hipLaunchKernelGGL((shkadov_reset_k<real, 256>), dim3(batch), dim3(256), 0, s, a);
  BCN_HIP(hipGetLastError());
  return BCN_OK;
}
template <typename real> int sloshing_launch_step(const Env1DArgs<real>& a, int batch, hipStream_t s, Env1DLaunch* note) {
#ifdef BCN_ENV1D_FLOAT
  if constexpr (std::is_same<real, float>::value) {   // float32, up to 256 cells, the far wall not a lane's first cell: the packed kernel
    if (a.one_wave == 1 && a.force_k == 0 && a.n > 128 && a.n <= 256 && ((a.n - 1) & 3) != 0 && a.ndt_act <= 64 && a.nx == a.n - 2) {
      hipLaunchKernelGGL((sloshing_step_pk_k<4>), dim3(batch), dim3(64), 0, s, a);
      *note = {"sloshing_step_pk_k", 4, 64};
      BCN_HIP(hipGetLastError());
      return BCN_OK;
    }
  }
#endif
  BCN_DISPATCH_1D(sloshing_step_k, a, batch, s, true, note);
  return BCN_OK;
}
template <typename real> int sloshing_launch_reset(const Env1DArgs<real>& a, int batch, hipStream_t s) {
  hipLaunchKernelGGL((sloshing_reset_k<real, 64>), dim3(batch), dim3(64), 0, s, a);
  BCN_HIP(hipGetLastError());
  return BCN_OK;
}

#define BCN_INST(T)                                                                   \
  template int burgers_launch_step<T>(const Env1DArgs<T>&, int, hipStream_t, Env1DLaunch*);   \
  template int burgers_launch_reset<T>(const Env1DArgs<T>&, int, hipStream_t);        \
  template int shkadov_launch_step<T>(const Env1DArgs<T>&, int, hipStream_t, Env1DLaunch*);   \
  template int shkadov_launch_reset<T>(const Env1DArgs<T>&, int, hipStream_t);        \
  template int sloshing_launch_step<T>(const Env1DArgs<T>&, int, hipStream_t, Env1DLaunch*);  \
  template int sloshing_launch_reset<T>(const Env1DArgs<T>&, int, hipStream_t);
#ifdef BCN_ENV1D_FLOAT
BCN_INST(float)
#endif
#ifdef BCN_ENV1D_DOUBLE
BCN_INST(double)
#endif
#endif   // BCN_ENV1D_WARM
