// bcn_jacobi_cells.h -- several Jacobi cells of the one-row-per-lane float32 kernels (dx == dy) as ONE asm statement.
// (included by bcn_dpp.h; a header of its own so that bcn_dpp.h keeps its three hand-written DPP pairs and this text stands alone)
//
// Every cell is bcn_dpp::jacobi_cell_eq's six instructions on the same operands in the same order, so results are bit for bit
// those of single-cell statements.  What changes is what hipcc may put BETWEEN the cells: it does not model the inside of an asm
// string and pads one wait state (`s_nop 0`) behind a statement wherever the next one follows directly -- 21 to 24 of them in a
// double sweep of the 128x64 kernel.  Inside one statement there is nothing to pad.  Measured (DESIGN.md 9.1,
// profiles/jacobi_runs_ab.log): those fillers were FREE -- 17 of them more or less move the double sweep by one cycle -- and what a
// statement of several cells does change is where hipcc can put the barrier, which ns2d_fast_impl.h therefore places itself.
//
// Hazards, on paper (tests/isa_hazards.py checks them in the disassembly of everything that is built):
//   * the only DPP reads are of the centre value %[a..] / %[c..]: an INPUT of the statement.  Every output and temporary is
//     early-clobber, so no instruction of the statement writes a register that a DPP instruction of it reads;
//   * a centre value written by the instruction directly in front of the statement (X[0] = cell(Y[0], ..) follows the statement that
//     ends by writing Y[0]) is read by DPP behind the leading v_add_f32 and the s_nop 1 of the first cell: 3 wait states, 2 needed;
//   * %[t] is written by the second DPP add and read by the final v_fma_f32 with the q-fma in between (DPP result -> VALU read), as
//     in jacobi_cell_eq; the next cell's leading v_add_f32 overwrites %[t] behind that read.
// cx is wave-uniform (a kernel argument) and goes to the final v_fma_f32 as a SCALAR operand -- VOP3 takes one SGPR and the cell
// has no other -- so it holds no VGPR and needs no v_mov in the loop.
// One set of three temporaries per statement.  An inline asm statement takes 30 operands at the most: a run of m consecutive
// cells takes m outputs, m + 2 inputs of the source row, m values of nb, 3 temporaries, cx and cBy = 3 m + 7, so m <= 7; m
// unrelated cells take 5 m + 5.  cx as a scalar operand is worth 26 cycles per sweep (795 -> 769), far more than its one v_mov.
// The cell texts are plain string macros, one line each, so that the allow-list scan of tests/test_isa_hazards_host.py reads them.
#pragma once

// cell i of a run: centre a{i+1}, east a{i+2}, west a{i}
#define BCN_RUN_CELL0 "v_add_f32 %[t], %[a2], %[a0]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[u], %[a1], %[t] wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" "v_add_f32_dpp %[t], %[a1], %[u] wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" "v_fma_f32 %[q], %[cBy], %[a1], %[n0]\n\t" "v_fma_f32 %[d0], %[cx], %[t], %[q]\n\t"
#define BCN_RUN_CELL1 "v_add_f32 %[t], %[a3], %[a1]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[u], %[a2], %[t] wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" "v_add_f32_dpp %[t], %[a2], %[u] wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" "v_fma_f32 %[q], %[cBy], %[a2], %[n1]\n\t" "v_fma_f32 %[d1], %[cx], %[t], %[q]\n\t"
#define BCN_RUN_CELL2 "v_add_f32 %[t], %[a4], %[a2]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[u], %[a3], %[t] wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" "v_add_f32_dpp %[t], %[a3], %[u] wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" "v_fma_f32 %[q], %[cBy], %[a3], %[n2]\n\t" "v_fma_f32 %[d2], %[cx], %[t], %[q]\n\t"
#define BCN_RUN_CELL3 "v_add_f32 %[t], %[a5], %[a3]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[u], %[a4], %[t] wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" "v_add_f32_dpp %[t], %[a4], %[u] wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" "v_fma_f32 %[q], %[cBy], %[a4], %[n3]\n\t" "v_fma_f32 %[d3], %[cx], %[t], %[q]\n\t"
#define BCN_RUN_CELL4 "v_add_f32 %[t], %[a6], %[a4]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[u], %[a5], %[t] wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" "v_add_f32_dpp %[t], %[a5], %[u] wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" "v_fma_f32 %[q], %[cBy], %[a5], %[n4]\n\t" "v_fma_f32 %[d4], %[cx], %[t], %[q]\n\t"
#define BCN_RUN_CELL5 "v_add_f32 %[t], %[a7], %[a5]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[u], %[a6], %[t] wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" "v_add_f32_dpp %[t], %[a6], %[u] wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" "v_fma_f32 %[q], %[cBy], %[a6], %[n5]\n\t" "v_fma_f32 %[d5], %[cx], %[t], %[q]\n\t"
#define BCN_RUN_CELL6 "v_add_f32 %[t], %[a8], %[a6]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[u], %[a7], %[t] wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" "v_add_f32_dpp %[t], %[a7], %[u] wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" "v_fma_f32 %[q], %[cBy], %[a7], %[n6]\n\t" "v_fma_f32 %[d6], %[cx], %[t], %[q]\n\t"
// cell i of unrelated cells: centre c{i}, east e{i}, west w{i}
#define BCN_ANY_CELL0 "v_add_f32 %[t], %[e0], %[w0]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[u], %[c0], %[t] wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" "v_add_f32_dpp %[t], %[c0], %[u] wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" "v_fma_f32 %[q], %[cBy], %[c0], %[n0]\n\t" "v_fma_f32 %[d0], %[cx], %[t], %[q]\n\t"
#define BCN_ANY_CELL1 "v_add_f32 %[t], %[e1], %[w1]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[u], %[c1], %[t] wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" "v_add_f32_dpp %[t], %[c1], %[u] wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" "v_fma_f32 %[q], %[cBy], %[c1], %[n1]\n\t" "v_fma_f32 %[d1], %[cx], %[t], %[q]\n\t"
#define BCN_ANY_CELL2 "v_add_f32 %[t], %[e2], %[w2]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[u], %[c2], %[t] wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" "v_add_f32_dpp %[t], %[c2], %[u] wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" "v_fma_f32 %[q], %[cBy], %[c2], %[n2]\n\t" "v_fma_f32 %[d2], %[cx], %[t], %[q]\n\t"
#define BCN_ANY_CELL3 "v_add_f32 %[t], %[e3], %[w3]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[u], %[c3], %[t] wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" "v_add_f32_dpp %[t], %[c3], %[u] wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" "v_fma_f32 %[q], %[cBy], %[c3], %[n3]\n\t" "v_fma_f32 %[d3], %[cx], %[t], %[q]\n\t"

namespace bcn_dpp {

#define BCN_CELLS_TMP [t] "=&v"(t), [u] "=&v"(u), [q] "=&v"(q)
#define BCN_RUN_O1 BCN_CELLS_TMP, [d0] "=&v"(d[0])
#define BCN_RUN_O2 BCN_RUN_O1, [d1] "=&v"(d[1])
#define BCN_RUN_O3 BCN_RUN_O2, [d2] "=&v"(d[2])
#define BCN_RUN_O4 BCN_RUN_O3, [d3] "=&v"(d[3])
#define BCN_RUN_O5 BCN_RUN_O4, [d4] "=&v"(d[4])
#define BCN_RUN_O6 BCN_RUN_O5, [d5] "=&v"(d[5])
#define BCN_RUN_O7 BCN_RUN_O6, [d6] "=&v"(d[6])
#define BCN_RUN_I1 [cx] "s"(cx), [cBy] "v"(cBy), [a0] "v"(a[0]), [a1] "v"(a[1]), [a2] "v"(a[2]), [n0] "v"(n[0])
#define BCN_RUN_I2 BCN_RUN_I1, [a3] "v"(a[3]), [n1] "v"(n[1])
#define BCN_RUN_I3 BCN_RUN_I2, [a4] "v"(a[4]), [n2] "v"(n[2])
#define BCN_RUN_I4 BCN_RUN_I3, [a5] "v"(a[5]), [n3] "v"(n[3])
#define BCN_RUN_I5 BCN_RUN_I4, [a6] "v"(a[6]), [n4] "v"(n[4])
#define BCN_RUN_I6 BCN_RUN_I5, [a7] "v"(a[7]), [n5] "v"(n[5])
#define BCN_RUN_I7 BCN_RUN_I6, [a8] "v"(a[8]), [n6] "v"(n[6])

// d[i] = cell(a[i + 1], a[i + 2], a[i], n[i]) for i < M: M consecutive cells of a row, a = &SRC[k0 - 1], d = &DST[k0], n = &nb[k0].
// d must not overlap a or n.
template <int M>
__device__ __forceinline__ void jacobi_run_eq(float* __restrict__ d, const float* __restrict__ a, const float* __restrict__ n, float cx, float cBy) {
  static_assert(M >= 1 && M <= 7, "3 M + 7 operands, 30 at the most");
  float t, u, q;
  if constexpr (M == 1) asm(BCN_RUN_CELL0 : BCN_RUN_O1 : BCN_RUN_I1);
  if constexpr (M == 2) asm(BCN_RUN_CELL0 BCN_RUN_CELL1 : BCN_RUN_O2 : BCN_RUN_I2);
  if constexpr (M == 3) asm(BCN_RUN_CELL0 BCN_RUN_CELL1 BCN_RUN_CELL2 : BCN_RUN_O3 : BCN_RUN_I3);
  if constexpr (M == 4) asm(BCN_RUN_CELL0 BCN_RUN_CELL1 BCN_RUN_CELL2 BCN_RUN_CELL3 : BCN_RUN_O4 : BCN_RUN_I4);
  if constexpr (M == 5) asm(BCN_RUN_CELL0 BCN_RUN_CELL1 BCN_RUN_CELL2 BCN_RUN_CELL3 BCN_RUN_CELL4 : BCN_RUN_O5 : BCN_RUN_I5);
  if constexpr (M == 6) asm(BCN_RUN_CELL0 BCN_RUN_CELL1 BCN_RUN_CELL2 BCN_RUN_CELL3 BCN_RUN_CELL4 BCN_RUN_CELL5 : BCN_RUN_O6 : BCN_RUN_I6);
  if constexpr (M == 7) asm(BCN_RUN_CELL0 BCN_RUN_CELL1 BCN_RUN_CELL2 BCN_RUN_CELL3 BCN_RUN_CELL4 BCN_RUN_CELL5 BCN_RUN_CELL6 : BCN_RUN_O7 : BCN_RUN_I7);
}
// Which strip widths take the runs.  A statement of several cells is something hipcc cannot put the barrier into, so the second
// sweep's R - 4 inner cells are either few enough for the barrier behind them to stand where it stood (<= 3), or enough for two runs
// with the barrier in between (>= 8, ns2d_fast_impl.h: BCN_TAIL2).  In between -- R = 8 .. 11 -- they would be ONE run with the barrier
// behind it, where the 128x64 kernel measured worst; measured at R = 10 (100x50, B = 512): 16.12 -> 16.55 ms per env step.  Those
// strip widths stay cell by cell.  (Splitting such a short run around the barrier has not been measured.)
constexpr bool jacobi_runs_fit(int r) { return r - 4 <= 3 || r - 4 >= 8; }
// run length for n cells still to do: as few statements as 7 cells each allow, of equal length where n divides (14 -> 7 + 7,
// 12 -> 6 + 6, 8 -> 4 + 4, 3 -> 3), the remainder in the last one
constexpr int jacobi_run_len(int n) { return (n + (n + 6) / 7 - 1) / ((n + 6) / 7); }
// DST[k] = cell(SRC[k], SRC[k + 1], SRC[k - 1], nb[k]) for K0 <= k < K1, in runs
template <int K0, int K1>
__device__ __forceinline__ void jacobi_range_eq(float* __restrict__ dst, const float* __restrict__ src, const float* __restrict__ nb, float cx, float cBy) {
  if constexpr (K1 > K0) {
    constexpr int M = jacobi_run_len(K1 - K0);
    jacobi_run_eq<M>(dst + K0, src + K0 - 1, nb + K0, cx, cBy);
    jacobi_range_eq<K0 + M, K1>(dst, src, nb, cx, cBy);
  }
}

#define BCN_ANY_O(i) , [d##i] "=&v"(d##i)
#define BCN_ANY_I(i) , [c##i] "v"(c##i), [e##i] "v"(e##i), [w##i] "v"(w##i), [n##i] "v"(n##i)
// unrelated cells d_i = cell(c_i, e_i, w_i, n_i) as one statement: the two strip-edge cells of a single sweep ...
__device__ __forceinline__ void jacobi_cells_eq(float& d0, float& d1, float c0, float e0, float w0, float n0, float c1, float e1, float w1, float n1,
                                                float cx, float cBy) {
  float t, u, q;
  asm(BCN_ANY_CELL0 BCN_ANY_CELL1 : BCN_CELLS_TMP BCN_ANY_O(0) BCN_ANY_O(1) : [cx] "s"(cx), [cBy] "v"(cBy) BCN_ANY_I(0) BCN_ANY_I(1));
}
// ... and the four halo-dependent / the four exchanged cells of a double sweep (the results must be four different variables)
__device__ __forceinline__ void jacobi_cells_eq(float& d0, float& d1, float& d2, float& d3, float c0, float e0, float w0, float n0, float c1, float e1,
                                                float w1, float n1, float c2, float e2, float w2, float n2, float c3, float e3, float w3, float n3,
                                                float cx, float cBy) {
  float t, u, q;
  asm(BCN_ANY_CELL0 BCN_ANY_CELL1 BCN_ANY_CELL2 BCN_ANY_CELL3
      : BCN_CELLS_TMP BCN_ANY_O(0) BCN_ANY_O(1) BCN_ANY_O(2) BCN_ANY_O(3)
      : [cx] "s"(cx), [cBy] "v"(cBy) BCN_ANY_I(0) BCN_ANY_I(1) BCN_ANY_I(2) BCN_ANY_I(3));
}

}  // namespace bcn_dpp
