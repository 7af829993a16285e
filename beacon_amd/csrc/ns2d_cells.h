// ns2d_cells.h -- the arithmetic of ONE cell of the rayleigh / mixing time step, stated once for the four kernels that run it:
// ns2d_generic.hip (fields in HBM/L2), ns2d_fast_impl.h (one row per lane), ns2d_fast2_impl.h (two rows per lane) and
// ns2d_fast4_impl.h (the hybrid).  The kernels differ in where the fields live and how cells map to lanes; what a cell computes
// from its neighbours is this file.  Memory is reached only through arguments.
//
// The register-resident kernels sit at 256 VGPRs plus scratch, and their register allocation reacts to source changes that look
// neutral.  A site uses a routine of this file only if the device code of EVERY kernel stays what it was with the text written
// out in place (scripts/params_fast_kernels.py --compare; DESIGN.md 20 has the table of piece x kernel and what was tried where a
// site keeps its own text).  What kept it so:
//   * a routine keeps each statement's expression tree and the statement boundaries of the text it replaces: the fast units
//     build with -ffp-contract=on, which fuses a multiply into an add within ONE statement only.  More than that: the operands of
//     a `cond ? a + dt * (x - y - z) : 0` are evaluated inside the arm, so a routine that returns x - y - z leaves other code
//     than one that returns x, y and z (NS2DRhs) to the caller's statement;
//   * loads, and the address arithmetic in front of them, stay where they were in program order: a caller that read a neighbour
//     between two statements of the cell still does, and an index another load of the caller shares is computed by the caller;
//   * values are passed, not references: the address of a local of a large kernel body keeps it in memory until the routine is
//     inlined, behind the compiler's first clean-up of that body;
//   * a routine is not built from another routine of this file (the statements two routines share are a macro);
//   * template instantiations keep their order.
#pragma once
#include "bcn_common.h"

// ---- predictor (rayleigh.py:370-407 / mixing.py:381-416) -----------------------------------------------------------------
// u* = u + dt (diff - conv - pres) at the face between cells (i-1, j) and (i, j); v* = v + dt (diff - conv - pres + T) at the
// face between (i, j-1) and (i, j), T the buoyancy term of rayleigh.
// Arguments: the centre value and its E, W, N, S neighbours (trailing underscore: cell values, not face averages); vNW_ =
// v(i-1, j+1) and uSE_ = u(i+1, j-1), the one diagonal neighbour each face needs; pW = p(i-1, j), pS = p(i, j-1).
// The statements of the two faces, written once.  They leave conv, diff and pres in scope; the statement that combines them
// follows in the routine that uses the block.
#define NS2D_PRED_U_TERMS                                                                     \
  real uE = real(0.5) * (uE_ + uc), uW = real(0.5) * (uc + uW_);                              \
  real uN2 = real(0.5) * (uN_ + uc), uS2 = real(0.5) * (uc + uS_);                            \
  real vN2 = real(0.5) * (vN_ + vNW_), vS2 = real(0.5) * (vc + vW_);                          \
  real conv = (uE * uE - uW * uW) * rdx + (uN2 * vN2 - uS2 * vS2) * rdy;                      \
  real diff = ((uE_ - 2 * uc + uW_) * rdx2 + (uN_ - 2 * uc + uS_) * rdy2) * kmom;             \
  real pres = (pc - pW) * rdx;
#define NS2D_PRED_V_TERMS                                                                     \
  real vE = real(0.5) * (vE_ + vc), vW = real(0.5) * (vc + vW_);                              \
  real uE = real(0.5) * (uE_ + uSE_), uW = real(0.5) * (uc + uS_);                            \
  real vN2 = real(0.5) * (vN_ + vc), vS2 = real(0.5) * (vc + vS_);                            \
  real conv = (uE * vE - uW * vW) * rdx + (vN2 * vN2 - vS2 * vS2) * rdy;                      \
  real diff = ((vE_ - 2 * vc + vW_) * rdx2 + (vN_ - 2 * vc + vS_) * rdy2) * kmom;             \
  real pres = (pc - pS) * rdy;

// ns2d_pred_u, ns2d_pred_v: the three terms of one face.  The caller writes the statement that combines them -- u + dt * (r.diff -
// r.conv - r.pres) -- under its own guard (i >= 2, j >= 2, lanes and columns that exist) and with its own buoyancy handling.
template <typename real>
struct NS2DRhs {
  real diff, conv, pres;
};

template <typename real>
__device__ __forceinline__ NS2DRhs<real> ns2d_pred_u(real uc, real uE_, real uW_, real uN_, real uS_, real vc, real vW_, real vN_, real vNW_,
                                                     real pc, real pW, real rdx, real rdy, real rdx2, real rdy2, real kmom) {
  NS2D_PRED_U_TERMS
  return NS2DRhs<real>{diff, conv, pres};
}

template <typename real>
__device__ __forceinline__ NS2DRhs<real> ns2d_pred_v(real uc, real uE_, real uS_, real uSE_, real vc, real vE_, real vW_, real vN_, real vS_,
                                                     real pc, real pS, real rdx, real rdy, real rdx2, real rdy2, real kmom) {
  NS2D_PRED_V_TERMS
  return NS2DRhs<real>{diff, conv, pres};
}

// ns2d_pred_cell: u* and v* of cell (i, j) in one routine, with the guards i >= 2, j >= 2 and the buoyancy term of rayleigh (KIND == 0)
// read between the terms of v* and their sum -- for ns2d_fast2_impl.h, whose code keeps only with this form.  The buoyancy value is
// T[i * sy + c]: a caller whose own loads share the index i * SY + j passes (sy, c) = (0, i * SY + j), one whose loads do not (fields
// in the global scratch, 64-bit addresses) passes (SY, j); either way the address arithmetic stays where the written-out text had it.
template <typename real, int KIND>
__device__ __forceinline__ void ns2d_pred_cell(real uc, real uE_, real uW_, real uN_, real uS_, real uSE_, real vc, real vE_, real vW_, real vN_,
                                               real vS_, real vNW_, real pc, real pW, real pS, int i, int j, real dt, real rdx, real rdy, real rdx2,
                                               real rdy2, const real& kmom, const real* T, int sy, int c, real& us_out, real& vs_out) {
  {
    NS2D_PRED_U_TERMS
    us_out = (i >= 2) ? uc + dt * (diff - conv - pres) : real(0);
  }
  {
    NS2D_PRED_V_TERMS
    const real buoy = (KIND == 0) ? T[i * sy + c] : real(0);
    vs_out = (j >= 2) ? vc + dt * (diff - conv - pres + buoy) : real(0);
  }
}
#undef NS2D_PRED_U_TERMS
#undef NS2D_PRED_V_TERMS

// ---- scalar transport (rayleigh.py:468-487 / mixing.py:478-497) ------------------------------------------------------------
// The reference's in-place sweep is S' = A + aW S'(i-1, j) + aS S'(i, j-1) with A = T0 + dt expl.  expl: the part of dS/dt that reads
// OLD values only -- diffusion without the west / south terms, advection through the east and north faces, and the centre value's
// share of the west and south faces.  uE, uW = u(i+1, j), u(i, j); vN, vS = v(i, j+1), v(i, j); T0, TE, TN = S(i, j), S(i+1, j), S(i, j+1).
template <typename real>
__device__ __forceinline__ real ns2d_transport_expl(real uE, real uW, real vN, real vS, real T0, real TE, real TN, real ksc, real rdx2,
                                                    real rdy2, real rdx, real rdy) {
  return ksc * ((TE - 2 * T0) * rdx2 + (TN - 2 * T0) * rdy2) -
         (uE * real(0.5) * (TE + T0) - uW * real(0.5) * T0) * rdx -
         (vN * real(0.5) * (TN + T0) - vS * real(0.5) * T0) * rdy;
}

// aW (vel = uW, the x constants) or aS (vel = vS, the y constants): the coefficient of the NEW west / south value
template <typename real>
__device__ __forceinline__ real ns2d_transport_coef(real dt, real ksc, real rd2, real vel, real rd) {
  return dt * (ksc * rd2 + real(0.5) * vel * rd);
}

// ---- stop rule of the Jacobi solve: how many sweeps to run before the residual is evaluated again (conv_plan) ------
// room = log2 of the norm over its threshold, rho = log2 of its decay per sweep (negative where it decays): the sweeps until the norm
// reaches the threshold at that rate, at most jmax; 0 where the norm is already there
__device__ __forceinline__ int ns2d_plan_steps(float room, float rho, int jmax) {
  int j = 0;
  if (room > 0.f) j = (rho < 0.f) ? (int)fminf(room / -rho, (float)jmax) : jmax;
  return j;
}

// the extrapolating plans land one sweep and a sixteenth short of the estimate, plus the option plan_overshoot
__device__ __forceinline__ int ns2d_plan_trim(int jw, int overshoot) {
  int j = jw - 1 - (jw >> 4) + overshoot;
  j = j > 0 ? j : 0;
  return j;
}

// conv_plan 3, the slow-mode guard of the landing a skip ends in: the factor over tol that the landing evaluation must exceed, from
// slow_k (ns2d_fast_impl.h: [0] log2 sqrt(3 |d_1|^2 / tol), [1], [3] log2 of the two mode cutoffs, [2], [4] their growth bounds) and
// itp, the last evaluated sweep
template <typename real>
__device__ __forceinline__ float ns2d_slow_guard(const real* slow_k, int itp) {
  const float e0 = (float)slow_k[0], fi = (float)itp;
  const float t0 = 1.f + 2.f * exp2f(e0 + fi * (float)slow_k[1]), t1 = 1.f + 2.f * exp2f(e0 + fi * (float)slow_k[3]);
  const float g = fminf(fminf((float)slow_k[2] * t0 * t0, (float)slow_k[4] * t1 * t1) * 1.001f, (float)BCN_CONV_GUARD);
  return g;
}
