// params.h -- per-replica physical parameters (include/beacon_hip.h: bcn_set_params).  The names are the reference's constructor
// arguments; what the kernels read are the constants derived from them, computed here in double by the SAME inline functions that
// the *_create entry points call (capi.hip), so that a replica whose parameters equal a uniform handle's cfg receives the constants
// of that handle bit for bit.  The device table is [n_derived][B] in the handle's dtype.
#pragma once
#include <math.h>

#include "ns2d.h"

// ---- the derived constants, one expression each -------------------------------------------------------------------------------
inline double bcn_rayleigh_kmom(double pr, double ra) { return sqrt(pr / ra); }
inline double bcn_rayleigh_ksc(double pr, double ra) { return 1.0 / sqrt(pr * ra); }
inline double bcn_mixing_kmom(double re) { return 1.0 / re; }
inline double bcn_mixing_ksc(double pe) { return 1.0 / pe; }
// mixing.py:34: u_max = re nu / L.  The cfg carries u_max and re, not nu and L: nu / L is recovered as cfg_u_max / cfg_re (exact for
// the reference's nu = 0.01 with L = 1: 1.0 / 100 is the double 0.01), and the handle's own re returns the cfg's u_max itself.
inline double bcn_mixing_u_max(double re, double cfg_re, double cfg_u_max) {
  return re == cfg_re ? cfg_u_max : re * (cfg_u_max / cfg_re);
}
inline double bcn_shkadov_delta_p(double delta) { return 1.0 / (5.0 * delta); }
// vortex.py:26-42, in the reference's order
inline double bcn_vortex_ire(double re_crit, double re) { return 1.0 / re_crit - 1.0 / re; }

#define BCN_MAX_PARAMS 3

// What one env kind takes: names in the order of the value rows of bcn_set_params, which of them must be > 0 (divisors and arguments
// of roots), and how many constants a replica's row of the device table holds.
struct BcnParamDesc {
  int n;
  const char* name[BCN_MAX_PARAMS];
  bool positive[BCN_MAX_PARAMS];
  int n_derived;
};

inline const BcnParamDesc* bcn_param_desc(int kind) {
  static const BcnParamDesc rayleigh = {1, {"ra"}, {true}, 2};                               // kmom, ksc
  static const BcnParamDesc mixing = {2, {"re", "pe"}, {true, true}, 3};                     // kmom, ksc, u_max
  static const BcnParamDesc burgers = {2, {"u_target", "amp"}, {false, false}, 2};           // the same two
  static const BcnParamDesc shkadov = {1, {"delta"}, {true}, 1};                             // delta_p
  static const BcnParamDesc sloshing = {3, {"amp", "alpha", "g"}, {false, false, true}, 3};  // the same three
  static const BcnParamDesc lorenz = {3, {"sigma", "rho", "beta"}, {false, false, false}, 3};
  static const BcnParamDesc vortex = {2, {"re", "weight"}, {true, false}, 2};                // ire, weight
  switch (kind) {
    case BCN_RAYLEIGH: return &rayleigh;
    case BCN_MIXING: return &mixing;
    case BCN_BURGERS: return &burgers;
    case BCN_SHKADOV: return &shkadov;
    case BCN_SLOSHING: return &sloshing;
    case BCN_LORENZ: return &lorenz;
    case BCN_VORTEX: return &vortex;
  }
  return nullptr;
}

// p: one replica's parameters (n of them); aux: the cfg values the expressions need besides (rayleigh: pr; mixing: the cfg's re and
// u_max; vortex: re_crit); d: its n_derived constants, in double
inline void bcn_derive_params(int kind, const double* p, const double* aux, double* d) {
  switch (kind) {
    case BCN_RAYLEIGH: d[0] = bcn_rayleigh_kmom(aux[0], p[0]); d[1] = bcn_rayleigh_ksc(aux[0], p[0]); break;
    case BCN_MIXING: d[0] = bcn_mixing_kmom(p[0]); d[1] = bcn_mixing_ksc(p[1]); d[2] = bcn_mixing_u_max(p[0], aux[0], aux[1]); break;
    case BCN_BURGERS: d[0] = p[0]; d[1] = p[1]; break;
    case BCN_SHKADOV: d[0] = bcn_shkadov_delta_p(p[0]); break;
    case BCN_SLOSHING: d[0] = p[0]; d[1] = p[1]; d[2] = p[2]; break;
    case BCN_LORENZ: d[0] = p[0]; d[1] = p[1]; d[2] = p[2]; break;
    case BCN_VORTEX: d[0] = bcn_vortex_ire(aux[0], p[0]); d[1] = p[1]; break;
  }
}

// the generic 2D kernel with the table as a kernel argument of its own (ns2d_generic.hip): NS2DArgs keeps its layout, and with it
// the register-resident kernels keep their code.  prm: [2][B] (rayleigh: kmom, ksc) / [3][B] (mixing: kmom, ksc, u_max)
template <typename real> int ns2d_launch_generic_prm(const NS2DArgs<real>& a, int batch, hipStream_t s, const real* prm);

// the register-resident kernels with the table as a kernel argument of their own (ns2d_prm.h; ns2d_fast_prm.hip, ns2d_fast_prm_f64.hip,
// ns2d_fast2_prm.hip), selected per handle by bcn_set_option "params_kernel".  ns2d_launch_fast_prm reaches the two-rows-per-lane
// built-ins the way ns2d_launch_fast does; ns2d_fast_supported_prm: the library has a table-reading kernel for this handle's grid.
template <typename real> bool ns2d_fast_supported_prm(const NS2DArgs<real>& a);
template <typename real> int ns2d_launch_fast_prm(const NS2DArgs<real>& a, int batch, hipStream_t s, const real* prm);
template <typename real> bool ns2d_fast2_supported_prm(const NS2DArgs<real>& a);
template <typename real> int ns2d_launch_fast2_prm(const NS2DArgs<real>& a, int batch, hipStream_t s, const real* prm);
