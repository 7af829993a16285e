// ns2d_geom.h -- the workgroup geometry of the three register-resident 2D kernel families, stated once: strips, threads, the LDS
// map, the global field scratch, and which mappings a family can hold at all.  Plain C++17 (no HIP, no other header of the
// project): the kernel templates take their constants from here (FastGeom, Fast2Geom, Fast4Geom), and so does the host query
// bcn_jit_geometry, which is how beacon_amd/jit.py learns whether a grid fits a family -- Python restates none of it.
//
// A mapping is (nx, ny, r, gf | rpl): strips of r columns, one wave each; gf says where the fields live (one and two rows per
// lane), rpl is the hybrid's rows per lane.  Each family below gives nw(), rl(), threads(), lds_elems / lds_bytes(esz),
// scratch_elems() and two predicates: shape_ok() -- what the kernel templates assert -- and admissible(esz), which adds that
// the launch's LDS fits a workgroup.  Everything but the predicates is meaningful for a mapping with shape_ok() only.
#pragma once
#include <stddef.h>

#ifndef BCN_PDG
#define BCN_PDG 8    // global fields, diagonals ahead.  Round 3 (T through flat pointers): 4 / 8 / 12 -> 52.9 / 52.1 / 51.3 ms per step
                     // (rayleigh 128x64 float64); round 4 (global pointers): 4 / 8 / 10 / 12 / 16 / 20 -> 53.0 / 51.2 / 51.9 / 52.0 / 51.9 / 61.0.
                     // (measured depths only: an intermediate round-4 build with generic pointers stopped converging at a depth of 6)
#endif
static_assert(BCN_PDG == 4 || BCN_PDG == 8 || BCN_PDG == 10 || BCN_PDG == 12 || BCN_PDG == 16 || BCN_PDG == 20,
              "BCN_PDG: only the prefetch depths that were measured AND verified against the oracle (4, 8, 10, 12, 16, 20)");
#ifndef BCN_PDF
#define BCN_PDF 8    // fields in LDS: diagonals per block of the transport wave (two register sets: it runs PDF..2 PDF diagonals ahead;
                     // measured 4 / 6 / 8 / 12 / 16: 26.2 / 25.7 / 24.8 / 25.3 / 26.3 k cycles per timestep outside the solve)
#endif

namespace bcn_geom {

constexpr int WAVE = 64;
constexpr int LDS_BYTES = 160 * 1024;   // of one workgroup (CDNA4)
constexpr int MAX_WAVES = 16;

constexpr int strips(int nx, int r) { return (nx + r - 1) / r; }
constexpr int last_strip(int nx, int r) { return nx - (strips(nx, r) - 1) * r; }
constexpr int up16(int x) { return (x + 15) / 16 * 16; }

// ---- one row per lane (ns2d_fast_impl.h): ny <= 64 ------------------------------------------------------------------------------
// GF ("global fields", float64 at 128x64: 3 x 68.6 KB do not fit LDS): 1 = u, v, T (with the same pads) live in
// a per-workgroup global scratch and LDS holds only the exchange buffers; 2 = u, v in LDS without pads (the
// transport wave clamps its skewed reads instead) and only T, with its pads, in the global scratch.
struct Rows1 {
  int nx, ny, r, gf;
  constexpr int nw() const { return strips(nx, r); }
  constexpr int rl() const { return last_strip(nx, r); }   // columns of the last wave (a second instantiation of the body when < r)
  constexpr int threads() const { return nw() * WAVE; }
  constexpr int sy() const { return ny + 2; }
  constexpr int sx() const { return nx + 2; }
  constexpr int pd() const { return gf ? BCN_PDG : BCN_PDF; }   // transport prefetch depth (diagonals); deeper for global fields
  // GF == 2 with a narrow last strip: ONE body serves every strip (fast_body: DEADC), the last one r columns wide like the
  // others with rl of them live; its dead columns read (never write) up to r - rl + 1 columns past the east ghost column
  constexpr int deadpad() const { return (gf == 2 && rl() != r) ? (r - rl() + 2) * sy() : 0; }
  // +16: lanes >= ny read (never write) past the array; a multiple of 64 elements, so that the transport wave fetches
  // u and v of a cell (the same index in two consecutive arrays) with ONE ds_read2st64_b32
  constexpr int sz() const { return (sx() * sy() + 16 + deadpad() + 63) / 64 * 64; }
  // LDS map (elements): [ exchange 2*NW*XC*64 | errp 128 | sact 64 | red 32 | sched 16 | .. FRONT ) U V T [ BACK )
  // The transport wave reads cell (t-lane+1, lane+1) for every lane without range checks: columns
  // -62..nx+ny+PD fall into FRONT / the neighbouring arrays / BACK, always inside this allocation.
  // columns per strip in the exchange buffer: 0, 1, r-2, r-1 (depth-2 halos: two sweeps per barrier), or the two edge
  // columns only where LDS is short (GF == 2: two float64 fields in LDS)
  constexpr int xc() const { return gf == 2 ? 2 : 4; }
  constexpr int exch() const { return 2 * nw() * xc() * WAVE; }   // [2 buffers][NW][XC][64]
  constexpr int sched_words() const { return exch() + 224; }      // the scheduler's two words, behind errp / sact / red
  constexpr int misc() const { return sched_words() + 16; }
  constexpr int front() const { return up16(misc() > 63 * sy() + 1 ? misc() : 63 * sy() + 1); }
  constexpr int back() const { return (ny + 3 * pd() + 2) * sy(); }   // the transport wave prefetches two blocks of PD diagonals ahead
  constexpr int frontg() const { return up16(63 * sy() + 1); }        // front pad of the global variant
  constexpr int misca() const { return up16(misc()); }
  constexpr size_t base_elems() const {
    return gf == 1 ? (size_t)misca() : gf == 2 ? (size_t)misca() + 2 * (size_t)sz() : (size_t)front() + 3 * (size_t)sz() + back();
  }
  // While wave 0 walks the ordered part of the transport step, the other waves compute the next timestep's predictor -- and,
  // where LDS has room for it, wave 0's strip as well: p of strip 0 in, u*, and the v* increment without buoyancy out,
  // [3][r][64] elements behind everything else (fast_body)
  constexpr size_t scr() const { return 3 * (size_t)r * WAVE; }
  constexpr bool offload(size_t esz) const {
    return nw() >= 3 && (r + 3) / 4 <= nw() - 1 && (base_elems() + scr()) * esz <= (size_t)LDS_BYTES;
  }
  constexpr size_t lds_elems(size_t esz) const { return base_elems() + (offload(esz) ? scr() : 0); }
  constexpr size_t lds_bytes(size_t esz) const { return lds_elems(esz) * esz; }
  constexpr size_t scratch_elems() const {
    return gf == 1 ? (size_t)frontg() + 3 * (size_t)sz() + back() : gf == 2 ? (size_t)frontg() + sz() + back() : 0;
  }
  // lanes run along y; at most 16 waves, at least 3 columns each
  constexpr bool shape_ok() const {
    return nx >= 1 && ny >= 1 && r >= 1 && gf >= 0 && gf <= 2 && ny <= WAVE && nw() <= MAX_WAVES && rl() >= 3 && rl() <= r;
  }
  constexpr bool admissible(size_t esz) const { return shape_ok() && lds_bytes(esz) <= (size_t)LDS_BYTES; }
};

// ---- two rows per lane (ns2d_fast2_impl.h): ny <= 128 ---------------------------------------------------------------------------
// GF = 1 (float64: three float64 fields exceed LDS): u, v, S live in a per-workgroup global scratch (L2-resident), the
// Poisson rhs in LDS ([cell of the thread][thread]: conflict-free), p and the phi ping-pong in registers.
struct Rows2 {
  int nx, ny, r, gf;
  constexpr int nw() const { return strips(nx, r); }
  constexpr int rl() const { return last_strip(nx, r); }
  constexpr int threads() const { return nw() * WAVE; }
  constexpr int lh() const { return (ny + 1) / 2; }   // active lanes (odd ny: the last lane's upper row is the ghost row)
  constexpr int sy() const { return ny + 2; }
  constexpr int sx() const { return nx + 2; }
  constexpr int sz() const { return sx() * sy(); }
  // LDS map (elements): exchange [2][NW][2 sides][2 rows][64] | errp 64 | sact 64 | red 32 | U V S
  constexpr int exch() const { return 2 * nw() * 4 * WAVE; }
  // the scheduler's two words: the end of the `red` row (block_sum uses red[0..NW), the transport sink red[16..17])
  constexpr int sched_words() const { return exch() + 128 + 24; }
  constexpr int fixed() const { return exch() + 64 + 64 + 32; }
  constexpr size_t lds_elems() const { return gf ? (size_t)fixed() + 2 * (size_t)r * threads() : (size_t)fixed() + 3 * (size_t)sz(); }
  constexpr size_t lds_bytes(size_t esz) const { return lds_elems() * esz; }
  constexpr size_t scratch_elems() const { return gf ? 3 * (size_t)sz() + 16 : 0; }   // + 16: the transport wave's sink
  constexpr bool shape_ok() const {
    return nx >= 1 && ny >= 1 && r >= 1 && gf >= 0 && gf <= 1 && ny <= 2 * WAVE && nw() <= MAX_WAVES && rl() >= 3 && rl() <= r;
  }
  constexpr bool admissible(size_t esz) const { return shape_ok() && lds_bytes(esz) <= (size_t)LDS_BYTES; }
};

// ---- the hybrid (ns2d_fast4_impl.h): the Poisson solve in registers with rpl rows per lane, the fields in HBM/L2 ----------------
struct Rows4 {
  int nx, ny, r, rpl;
  constexpr int sx() const { return nx + 2; }
  constexpr int ncell() const { return sx() * (ny + 2); }
  constexpr int nw() const { return strips(nx, r); }       // waves = column strips
  constexpr int rl() const { return last_strip(nx, r); }   // columns of the last strip (1..r)
  constexpr int threads() const { return nw() * WAVE; }
  constexpr int nl() const { return (ny + rpl - 1) / rpl; }   // lanes that hold rows (the last one rt() + 1 <= rpl of them)
  constexpr int rt() const { return (ny - 1) % rpl; }         // the top row is row rt() of lane nl() - 1
  constexpr int p() const { return sx() | 1; }                // LDS pitch of a natural-layout array (odd)
  constexpr int cpl() const { return (nx + WAVE - 1) / WAVE; }   // columns per lane of the transport walk
  constexpr int hrows() const { return WAVE * rpl; }             // one edge column in the exchange buffer (lane-major)
  constexpr int sched_words() const { return 2 * 32 + 64; }   // the scheduler's two words, behind the reduction scratch [2][2][16] and the conditioned actions
  constexpr int fixed() const { return sched_words() + 16; }
  constexpr int hal() const { return 2 * nw() * 2 * hrows(); }   // [parity][wave][west|east][HROWS]
  constexpr int warr() const { return p() * (ny + 2); }
  static constexpr int lds_elems_max(int esz) { return LDS_BYTES / esz; }
  // transport: rows per block and number of blocks
  constexpr int br_cap(int esz) const { return (lds_elems_max(esz) - fixed() - 2) / (3 * p()); }
  constexpr int nblk(int esz) const { return (ny + br_cap(esz) - 1) / br_cap(esz); }
  constexpr int br(int esz) const { return (ny + nblk(esz) - 1) / nblk(esz); }
  constexpr int lds_elems(int esz) const {
    const int jac = fixed() + hal() + warr(), tr = fixed() + 3 * p() * br(esz) + 2;
    return jac > tr ? jac : tr;
  }
  constexpr size_t lds_bytes(size_t esz) const { return (size_t)lds_elems((int)esz) * esz; }
  constexpr size_t scratch_elems() const { return 0; }   // the fields stay where the generic kernel keeps them
  // at most 64 lanes of rows; 2..16 column strips
  constexpr bool shape_ok() const {
    return nx >= 1 && ny >= 1 && r >= 1 && rpl >= 1 && nl() <= WAVE && nw() >= 2 && nw() <= MAX_WAVES && rl() >= 1;
  }
  // (a transport block holds at least one row)
  constexpr bool admissible(size_t esz) const { return shape_ok() && br_cap((int)esz) >= 1 && lds_bytes(esz) <= (size_t)LDS_BYTES; }
};

}  // namespace bcn_geom

// Internal queries of libbeacon_hip.so's host side (capi.hip), for beacon_amd/jit.py alone -- like bcn_set_error and the plugins'
// bcn_jit_* symbols they are no part of the public ABI (include/beacon_hip.h), and jit.py declares their argument types itself.
extern "C" {
// rows: 1, 2 or 4 (the family); g: gf, or rpl for the hybrid.  Returns 1 where the family can hold the mapping -- then out = { nw,
// rl, threads, LDS bytes of a launch, elements of global field scratch per workgroup }, with the library's compiled prefetch
// depths -- and 0 where it cannot (out untouched).
int bcn_jit_geometry(int rows, int nx, int ny, int r, int g, int f64, long long out[5]);
// Row i of the register-resident instantiations built into the library (ns2d_builtin.h): out = { f64, nx, ny, kind, rows, r, gf };
// returns 1, or 0 past the last row.
int bcn_jit_builtin(int i, int out[7]);
}
