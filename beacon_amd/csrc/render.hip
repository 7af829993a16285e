// render.hip -- the two frame kernels behind bcn_render (render.h, include/beacon_hip.h): uint8 RGB frames of the field panel
// (rayleigh, mixing) and of the line panel (burgers, shkadov, sloshing), each over a strip of control bars, for float and double.
//
// The pixel rules are the header's and use only operations that round alike on host and device -- a subtraction, a correctly
// rounded division, a product with a power of two or with H, truncation, integers -- so tests/render_ref.py equals these kernels
// byte for byte.  The unit is built with -ffp-contract=off and without fast-math; the float division is __fdiv_rn.
//
// Store-bound (rayleigh 128x64 at scale 4, B = 512: 201 MB per call), so the shape follows the stores:
//  * a workgroup stages whole pixel rows as bytes in LDS and then stores each staged row as dwords, every wave instruction a run of
//    256 contiguous bytes; a cell row of the field panel is staged once and stored `scale` times (the rows below each other are one
//    contiguous range of the frame);
//  * frames whose row is no multiple of 4 bytes take the same staging and byte stores, still contiguous across the lanes;
//  * field panel: one workgroup per (replica, band of cell rows); a field value is loaded once, coloured once (the table sits in
//    LDS) and written to its scale pixels of the staged row;
//  * line panel: one workgroup per (replica, band of pixel rows), at most four bands: a lane per column scans its samples, the row
//    range lands in LDS and the rows are painted from it, a staged group at a time;
//  * the strip: one workgroup per (replica, staged group of strip rows);
//  * threads are laid out [rows][2^k columns] with k chosen by the host, so no pixel costs an integer division by a run-time value;
//    the divisions left are two per control and two per column of a line panel.
// No atomics, no scratch, vector stores only.
#include "render.h"

namespace {

__device__ __forceinline__ float render_div(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ double render_div(double a, double b) { return a / b; }

// bin of t among n: 0 for t <= 0, n - 1 for t >= 1, else min(int(t n), n - 1); -1 for a NaN
template <typename real>
__device__ __forceinline__ int render_bin(real t, int n) {
  if (t != t) return -1;
  if (t <= real(0)) return 0;
  if (t >= real(1)) return n - 1;
  const int k = (int)(t * (real)n);
  return k < n - 1 ? k : n - 1;
}

__device__ __forceinline__ void put_px(uint8_t* p, unsigned r, unsigned g, unsigned b) {
  p[0] = (uint8_t)r; p[1] = (uint8_t)g; p[2] = (uint8_t)b;
}

struct RenderLds {
  uint8_t* rows;      // [rows_lds][lds_row]
  uint8_t* lut;       // [768]
  int8_t* colbar;     // [W]: the control whose bar covers the column, -1: none
  int* ctop;          // [64] strip rows [ctop, cbot) of control k's bar
  int* cbot;
  int* ccol;          // 1: red, 2: blue
  uint32_t* colinfo;  // line panel [W]: first row | last row << 14 | non-finite << 28
};

__device__ __forceinline__ RenderLds render_lds(const RenderArgs& A, uint32_t* smem) {
  RenderLds L;
  uint8_t* p = reinterpret_cast<uint8_t*>(smem);
  L.rows = p; p += (size_t)A.rows_lds * A.lds_row;
  L.lut = p; p += 768;
  L.ctop = reinterpret_cast<int*>(p); p += BCN_RENDER_MAX_CTRL * 4;
  L.cbot = reinterpret_cast<int*>(p); p += BCN_RENDER_MAX_CTRL * 4;
  L.ccol = reinterpret_cast<int*>(p); p += BCN_RENDER_MAX_CTRL * 4;
  L.colinfo = reinterpret_cast<uint32_t*>(p); p += A.line ? (size_t)A.W * 4 : 0;
  L.colbar = reinterpret_cast<int8_t*>(p);
  return L;
}

// staged rows -> frame: staged row jj goes to the `rep` pixel rows from out + jj rep row_bytes on
template <bool DW>
__device__ __forceinline__ void emit_rows(const RenderArgs& A, const uint8_t* rows, uint8_t* out, int nrows, int rep) {
  const unsigned tpr = 1u << A.lg_unit, tx = threadIdx.x & (tpr - 1), ty = threadIdx.x >> A.lg_unit, step = BCN_RENDER_NT >> A.lg_unit;
  for (unsigned jj = ty; jj < (unsigned)nrows; jj += step) {
    if (DW) {
      const unsigned nd = A.row_bytes >> 2;
      const uint32_t* src = reinterpret_cast<const uint32_t*>(rows + (size_t)jj * A.lds_row);
      uint32_t* dst = reinterpret_cast<uint32_t*>(out + (size_t)jj * rep * A.row_bytes);
      for (unsigned d = tx; d < nd; d += tpr) {
        const uint32_t v = src[d];
        for (int k = 0; k < rep; k++) dst[(size_t)k * nd + d] = v;
      }
    } else {
      const uint8_t* src = rows + (size_t)jj * A.lds_row;
      uint8_t* dst = out + (size_t)jj * rep * A.row_bytes;
      for (unsigned d = tx; d < A.row_bytes; d += tpr) {
        const uint8_t v = src[d];
        for (int k = 0; k < rep; k++) dst[(size_t)k * A.row_bytes + d] = v;
      }
    }
  }
}

// the bars of replica `rep`: which control covers a column, which strip rows its bar takes, and its colour
template <typename real>
__device__ void strip_prepare(const RenderArgs& A, int rep, const RenderLds& L) {
  const int tid = threadIdx.x, W = A.W, nc = A.n_ctrl;
  for (int c = tid; c < W; c += BCN_RENDER_NT) L.colbar[c] = -1;
  if (tid < nc) {
    real c;
    if (A.ctrl_int) {   // mixing.py:212-234: u_t, u_b, v_l, v_r over u_max
      const int a = static_cast<const int32_t*>(A.ctrl)[rep];
      const int pair = tid >> 1, sgn = (tid & 1) ? 1 : -1;   // action 0: (u_t, u_b) = (-1, 1); action 2: (v_l, v_r) = (-1, 1)
      c = (a == 0 && pair == 0) || (a == 2 && pair == 1) ? (real)sgn : (a == 1 && pair == 0) || (a == 3 && pair == 1) ? (real)-sgn : real(0);
    } else {
      c = static_cast<const real*>(A.ctrl)[(size_t)rep * nc + tid];
    }
    if (c != c) c = 0;
    c = c > real(1) ? real(1) : c < real(-1) ? real(-1) : c;
    const int hb = A.strip >> 1;
    const int nrow = ((int)(bcn_abs(c) * (real)(2 * hb)) + 1) >> 1;   // round_half_up(|c| hb)
    L.ctop[tid] = c > real(0) ? hb - nrow : hb;
    L.cbot[tid] = c > real(0) ? hb : c < real(0) ? hb + nrow : hb;
    L.ccol[tid] = c > real(0) ? 1 : 2;
  }
  __syncthreads();
  for (int k = 0; k < nc; k++) {
    const int c0 = (k * W) / nc, c1 = ((k + 1) * W) / nc, q = (c1 - c0) >> 2;
    for (int c = c0 + q + tid; c < c1 - q; c += BCN_RENDER_NT) L.colbar[c] = (int8_t)k;
  }
  __syncthreads();
}

// rows [sb rows_lds, (sb + 1) rows_lds) of the strip of one frame
template <typename real, bool DW>
__device__ void strip_paint(const RenderArgs& A, int rep, const RenderLds& L, uint8_t* out, int sb) {
  strip_prepare<real>(A, rep, L);
  const unsigned tpr = 1u << A.lg_px, tx = threadIdx.x & (tpr - 1), ty = threadIdx.x >> A.lg_px, step = BCN_RENDER_NT >> A.lg_px;
  const int r0 = sb * A.rows_lds, nr = min(A.rows_lds, A.strip - r0);
  for (unsigned jj = ty; jj < (unsigned)nr; jj += step) {
    const int rr = r0 + (int)jj;
    uint8_t* dst = L.rows + (size_t)jj * A.lds_row;
    for (unsigned c = tx; c < (unsigned)A.W; c += tpr) {
      const int k = L.colbar[c];
      unsigned r = 255, g = 255, b = 255;
      if (k >= 0 && rr >= L.ctop[k] && rr < L.cbot[k]) { g = 0; if (L.ccol[k] == 1) b = 0; else r = 0; }
      put_px(dst + 3 * c, r, g, b);
    }
  }
  __syncthreads();
  emit_rows<DW>(A, L.rows, out + (size_t)r0 * A.row_bytes, nr, 1);
}

// frame f shows replica replicas[f]; an index outside the batch forms no address and leaves its frame alone
__device__ __forceinline__ int render_replica(const RenderArgs& A, int f) {
  const int rep = A.replicas ? A.replicas[f] : f;
  return (unsigned)rep < (unsigned)A.batch ? rep : -1;
}

template <typename real, bool DW>
__global__ __launch_bounds__(BCN_RENDER_NT) void render_field_k(RenderArgs A) {
  extern __shared__ uint32_t smem[];
  const RenderLds L = render_lds(A, smem);
  const int f = blockIdx.x, rep = render_replica(A, f);
  if (rep < 0) return;
  uint8_t* frame = A.rgb + (size_t)f * (size_t)(A.H + A.strip) * A.row_bytes;
  const int band = blockIdx.y;
  if (band >= A.nbands) {
    strip_paint<real, DW>(A, rep, L, frame + (size_t)A.H * A.row_bytes, band - A.nbands);
    return;
  }
  for (int i = threadIdx.x; i < 192; i += BCN_RENDER_NT) reinterpret_cast<uint32_t*>(L.lut)[i] = reinterpret_cast<const uint32_t*>(A.lut)[i];
  __syncthreads();
  const int j0 = band * A.rows_lds, nr = min(A.rows_lds, A.ny - j0), s = A.scale, sx = A.nx + 2;
  const real* plane = static_cast<const real*>(A.field) + (size_t)rep * A.rep_stride;
  const real lo = (real)A.lo, den = (real)A.hi - lo;
  const unsigned tpr = 1u << A.lg_cell, tx = threadIdx.x & (tpr - 1), ty = threadIdx.x >> A.lg_cell, step = BCN_RENDER_NT >> A.lg_cell;
  for (unsigned jj = ty; jj < (unsigned)nr; jj += step) {
    const real* src = plane + (size_t)(A.ny - (j0 + (int)jj)) * sx + 1;   // the top pixel row is the top of the domain
    uint8_t* dst = L.rows + (size_t)jj * A.lds_row;
    for (unsigned i = tx; i < (unsigned)A.nx; i += tpr) {
      const int k = render_bin(render_div(src[i] - lo, den), 256);
      unsigned r = 0, g = 0, b = 0;
      if (k >= 0) { r = L.lut[3 * k]; g = L.lut[3 * k + 1]; b = L.lut[3 * k + 2]; }
      uint8_t* p = dst + (size_t)i * s * 3;
      for (int q = 0; q < s; q++) put_px(p + 3 * q, r, g, b);
    }
  }
  __syncthreads();
  emit_rows<DW>(A, L.rows, frame + (size_t)j0 * s * A.row_bytes, nr, s);
}

template <typename real, bool DW>
__global__ __launch_bounds__(BCN_RENDER_NT) void render_line_k(RenderArgs A) {
  extern __shared__ uint32_t smem[];
  const RenderLds L = render_lds(A, smem);
  const int f = blockIdx.x, rep = render_replica(A, f);
  if (rep < 0) return;
  uint8_t* frame = A.rgb + (size_t)f * (size_t)(A.H + A.strip) * A.row_bytes;
  const int band = blockIdx.y;
  if (band >= A.nbands) {
    strip_paint<real, DW>(A, rep, L, frame + (size_t)A.H * A.row_bytes, band - A.nbands);
    return;
  }
  const real* y = static_cast<const real*>(A.field) + (size_t)rep * A.rep_stride;
  const real hi = (real)A.hi, den = hi - (real)A.lo;
  const int W = A.W, H = A.H, ns = A.ns;
  const int rref = render_bin(render_div(hi - (real)A.ref, den), H);
  // column c covers samples (c ns) // W .. min(((c + 1) ns) // W, ns - 1): the first sample of the next column joins the curve
  for (int c = threadIdx.x; c < W; c += BCN_RENDER_NT) {
    const int i0 = (c * ns) / W, i1 = min(((c + 1) * ns) / W, ns - 1);
    int rmin = H - 1, rmax = 0;
    bool bad = false;
    for (int i = i0; i <= i1; i++) {
      const real v = y[i];
      if (!(bcn_abs(v) < (real)INFINITY)) { bad = true; continue; }
      const int r = render_bin(render_div(hi - v, den), H);
      rmin = min(rmin, r); rmax = max(rmax, r);
    }
    L.colinfo[c] = bad ? (1u << 28) : ((unsigned)rmin | ((unsigned)rmax << 14));
  }
  __syncthreads();
  const unsigned tpr = 1u << A.lg_px, tx = threadIdx.x & (tpr - 1), ty = threadIdx.x >> A.lg_px, step = BCN_RENDER_NT >> A.lg_px;
  const int rend = min(H, (band + 1) * A.band_rows);
  for (int r0 = band * A.band_rows; r0 < rend; r0 += A.rows_lds) {
    const int nr = min(A.rows_lds, rend - r0);
    for (unsigned jj = ty; jj < (unsigned)nr; jj += step) {
      const int rr = r0 + (int)jj;
      uint8_t* dst = L.rows + (size_t)jj * A.lds_row;
      for (unsigned c = tx; c < (unsigned)W; c += tpr) {
        const unsigned ci = L.colinfo[c];
        const int rmin = (int)(ci & 0x3fffu), rmax = (int)((ci >> 14) & 0x3fffu);
        unsigned r = 255, g = 255, b = 255;
        if (ci >> 28) { g = 0; b = 0; }
        else if (rr >= rmin && rr <= rmax) { r = 31; g = 119; b = 180; }
        else if (rr == rref) { r = 160; g = 160; b = 160; }
        put_px(dst + 3 * c, r, g, b);
      }
    }
    __syncthreads();
    emit_rows<DW>(A, L.rows, frame + (size_t)r0 * A.row_bytes, nr, 1);
    __syncthreads();
  }
}

inline int lg_pow2_ceil(unsigned n, int lg_max) {
  int k = 0;
  while (k < lg_max && (1u << k) < n) k++;
  return k;
}

template <typename real, bool DW>
int render_launch_t(const RenderArgs& a, size_t lds, hipStream_t s) {
  const dim3 grid(a.n, a.nbands + (a.strip + a.rows_lds - 1) / a.rows_lds);
  if (a.line) hipLaunchKernelGGL((render_line_k<real, DW>), grid, dim3(BCN_RENDER_NT), lds, s, a);
  else hipLaunchKernelGGL((render_field_k<real, DW>), grid, dim3(BCN_RENDER_NT), lds, s, a);
  BCN_HIP(hipGetLastError());
  return BCN_OK;
}

}  // namespace

int render_launch(RenderArgs& a, hipStream_t s) {
  if (a.n == 0) return BCN_OK;
  a.row_bytes = 3u * (unsigned)a.W;
  a.lds_row = (a.row_bytes + 3u) & ~3u;
  const int fit = (int)(BCN_RENDER_ROWS_LDS / a.lds_row);   // >= 1: W <= BCN_RENDER_MAX_W
  if (a.line) {
    // every workgroup of a replica scans the samples again (n reals against band_rows W 3 bytes written): at most 4 bands, and only
    // while the replicas alone do not fill the device
    a.rows_lds = fit < a.H ? fit : a.H;
    const int rounds = (a.H + a.rows_lds - 1) / a.rows_lds, want = (2048 + a.n - 1) / a.n;
    const int nb = want < 1 ? 1 : want > 4 ? 4 : want;
    a.band_rows = (rounds + nb - 1) / nb * a.rows_lds;
    a.nbands = (a.H + a.band_rows - 1) / a.band_rows;
  } else {
    a.nbands = (a.ny + fit - 1) / fit;
    a.rows_lds = (a.ny + a.nbands - 1) / a.nbands;          // bands of equal height
    a.nbands = (a.ny + a.rows_lds - 1) / a.rows_lds;
    a.band_rows = a.rows_lds;
  }
  if (a.nbands + (a.strip + a.rows_lds - 1) / a.rows_lds > 65535) { bcn_set_error("bcn_render: %d bands of rows exceed one launch", a.nbands); return BCN_ERR_ARG; }
  a.dwords = a.row_bytes % 4 == 0 && (reinterpret_cast<uintptr_t>(a.rgb) & 3) == 0;
  a.lg_cell = lg_pow2_ceil((unsigned)(a.line ? 1 : a.nx), 8);
  a.lg_px = lg_pow2_ceil((unsigned)a.W, 8);
  a.lg_unit = lg_pow2_ceil(a.dwords ? a.row_bytes / 4 : a.row_bytes, 8);
  const size_t lds = (size_t)a.rows_lds * a.lds_row + 768 + 3 * BCN_RENDER_MAX_CTRL * 4 + (a.line ? (size_t)a.W * 4 : 0) + (((size_t)a.W + 3) & ~(size_t)3);
  if (a.f64) return a.dwords ? render_launch_t<double, true>(a, lds, s) : render_launch_t<double, false>(a, lds, s);
  return a.dwords ? render_launch_t<float, true>(a, lds, s) : render_launch_t<float, false>(a, lds, s);
}
