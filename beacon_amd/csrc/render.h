// render.h -- argument block of the frame kernels (render.hip; include/beacon_hip.h: bcn_render_shape / bcn_render).
//
// A frame is [H + strip][W][3] uint8 (HWC): a panel of H pixel rows -- the field panel of rayleigh / mixing or the line panel of the
// 1D envs -- over `strip` rows of control bars.  The kernels read the handle's persistent state (one plane of `fields`, the stored
// action) and write frames; the pixel rules are the header's.  A workgroup stages whole pixel rows as bytes in LDS and then stores
// them as dwords (row bytes a multiple of 4 and a 4-byte aligned buffer) or byte by byte (any other width).
#pragma once
#include "bcn_common.h"

#define BCN_RENDER_NT 256             // threads per workgroup
#define BCN_RENDER_MAX_W 4096         // pixels per frame row: a staged row is at most 12 KB
#define BCN_RENDER_MAX_H 16384        // pixel rows of a line panel (a column's row range is packed into 14 + 14 bits)
#define BCN_RENDER_ROWS_LDS 16384u    // bytes of staged pixel rows per workgroup
#define BCN_RENDER_MAX_CTRL 64        // controls of a strip (rayleigh's n_sgts and shkadov's n_jets are at most 64)

struct RenderArgs {
  const void* field;        // replica 0 of the plane shown (field panel: [ny + 2][nx + 2], x fastest) / of the samples (line panel: sample 0)
  size_t rep_stride;        // elements between two replicas of it
  const void* ctrl;         // the stored action: real [B][n_ctrl], or -- ctrl_int -- mixing's int32 [B] action index
  const uint8_t* lut;       // field panel: [256][3], 4-byte aligned
  const int32_t* replicas;  // [n] or NULL: frame f shows replica f
  uint8_t* rgb;             // [n][H + strip][W][3]
  int batch, n;             // replicas of the handle, frames
  int f64, line, ctrl_int, n_ctrl;
  int nx, ny, scale;        // field panel
  int ns;                   // line panel: samples per replica
  int W, H, strip;          // pixels
  double lo, hi, ref;       // vmin, vmax / ymin, ymax, yref; narrowed once to the env's type by the kernel
  // how the workgroups split the frame (render_launch)
  unsigned row_bytes;       // 3 W
  unsigned lds_row;         // row_bytes rounded up to 4: distance of two staged rows
  int rows_lds;             // pixel rows (field panel: cell rows) staged at a time
  int nbands;               // workgroups per replica that paint the panel; ceil(strip / rows_lds) more paint the strip
  int band_rows;            // line panel: pixel rows per band, a multiple of rows_lds; field panel: rows_lds
  int dwords;               // 1: dword stores
  int lg_cell, lg_px, lg_unit;   // log2 of the threads that share a row of cells / of pixels / of store units
};

// fills the plan and enqueues ONE launch
int render_launch(RenderArgs& a, hipStream_t s);
