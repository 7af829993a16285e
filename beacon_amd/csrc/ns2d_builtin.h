// ns2d_builtin.h -- the register-resident instantiations built into libbeacon_hip.so, stated once: one X-macro list per
// translation unit, a row per instantiation: X(real, NX, NY, R, KIND, GF).  ns2d_fast.hip and ns2d_fast2.hip generate their
// *_supported, ns2d_launch_* and *_scratch_elems from their list; capi.hip's bcn_jit_builtin (ns2d_geom.h) enumerates both, and
// from it beacon_amd/jit.py knows which grids need no plugin.  Every other grid gets its own instantiation at run time
// (jit/ns2d_jit.hip), with the strip width jit.choose() picks -- these rows are the measured ones and need not be that pick.
// Plain C++: no HIP, no other header.
//
// The order of a list is the order in which its templates are instantiated: leave it (rule 5).  A strip width
// overridden with -D for an experiment has to reach every unit that includes this file.
#pragma once

#ifndef BCN_R128
#define BCN_R128 16
#endif
#ifndef BCN_R50
#define BCN_R50 5     // columns per lane of the 50x50 kernels
#endif
#ifndef BCN_GFD
#define BCN_GFD 2   // float64 128x64: 1 = u, v, T in global scratch, 2 = u, v in LDS and T in global scratch
#endif
#ifndef BCN_R128D
#define BCN_R128D 16   // columns per lane of the float64 128x64 kernel
#endif

// ns2d_fast.hip, one row per lane (rayleigh only): the metric grid 128x64 in both precisions (float64: fields in global scratch),
// the reference's default 50x50, and its other natural aspect ratios (nx = 50 L, ny = 50 H with H = 1) in float32.  The file is
// compiled once per precision; a unit takes the rows of its precision.
#define BCN_BUILTIN_FAST(X)            \
  X(float, 128, 64, BCN_R128, 0, 0)    \
  X(float, 50, 50, BCN_R50, 0, 0)      \
  X(double, 50, 50, BCN_R50, 0, 0)     \
  X(double, 128, 64, BCN_R128D, 0, BCN_GFD) \
  X(float, 100, 50, 10, 0, 0)          \
  X(float, 150, 50, 15, 0, 0)          \
  X(float, 200, 50, 25, 0, 0)

// ns2d_fast2.hip, two rows per lane: 100x100, mixing's default grid and rayleigh at L = H = 2.  float64 (the reference's
// arithmetic: fields in global scratch, GF = 1): mixing only -- rayleigh 100x100 float64 keeps the generic kernel.
#define BCN_BUILTIN_FAST2(X)           \
  X(float, 100, 100, 13, 1, 0)         \
  X(float, 100, 100, 13, 0, 0)         \
  X(double, 100, 100, 13, 1, 1)

// the row an argument block of precision `real` asks for
#define BCN_BUILTIN_IS(real, a, REAL, NX, NY, KIND) \
  (sizeof(real) == sizeof(REAL) && (a).nx == (NX) && (a).ny == (NY) && (a).kind == (KIND))
