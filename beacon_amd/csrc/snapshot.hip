// snapshot.hip -- the two copy kernels behind bcn_snapshot_save / bcn_snapshot_load (snapshot.h, include/beacon_hip.h).
//
// No arithmetic: bytes move between the handle's arrays and one snapshot buffer, every segment in ONE launch.  A workgroup finds
// its table entry from blockIdx (the table is a kernel argument, so the search runs on scalar registers) and then copies
//  * a tile of BCN_SNAP_TILE bytes of one replica's row (fields: tens of KB per row), as 16-byte loads and stores -- four in flight per
//    lane -- where source and destination rows share their alignment modulo 16, with single bytes in front of the first and behind the
//    last 16-byte boundary (burgers nx = 497: 1988 B rows, odd 2D grids); rows whose two sides are aligned differently (a gather
//    between such rows) go dword by dword;
//  * or, for short rows (observation history, actions, counters, outputs, the ODE envs' [field][B] columns), BCN_SNAP_NT * 4 units of
//    the flattened [replica][unit] index space, a lane per unit: consecutive lanes touch consecutive addresses whenever consecutive
//    replicas take consecutive sources (identity always does).
// load reads the source index and the mask of the destination replica and forms an address only from an index inside [0, n_src);
// source and destination are different buffers, so any index vector -- permutations, duplicates -- is safe.
#include "snapshot.h"

namespace {

// workgroup-wide copy of n bytes
__device__ __forceinline__ void snap_copy_span(const char* __restrict__ from, char* __restrict__ to, unsigned n) {
  const unsigned tid = threadIdx.x;
  const uintptr_t fa = reinterpret_cast<uintptr_t>(from), ta = reinterpret_cast<uintptr_t>(to);
  if (((fa ^ ta) & 15) == 0) {
    unsigned head = (unsigned)(0 - ta) & 15u;
    if (head > n) head = n;
    if (tid < head) to[tid] = from[tid];
    const unsigned nv = (n - head) >> 4;
    const uint4* __restrict__ f4 = reinterpret_cast<const uint4*>(from + head);
    uint4* __restrict__ t4 = reinterpret_cast<uint4*>(to + head);
    unsigned i = tid;
    for (; i + 3 * BCN_SNAP_NT < nv; i += 4 * BCN_SNAP_NT) {
      const uint4 a = f4[i], b = f4[i + BCN_SNAP_NT], c = f4[i + 2 * BCN_SNAP_NT], d = f4[i + 3 * BCN_SNAP_NT];
      t4[i] = a; t4[i + BCN_SNAP_NT] = b; t4[i + 2 * BCN_SNAP_NT] = c; t4[i + 3 * BCN_SNAP_NT] = d;
    }
    for (; i < nv; i += BCN_SNAP_NT) t4[i] = f4[i];
    const unsigned done = head + (nv << 4);   // n - done < 16
    if (tid < n - done) to[done + tid] = from[done + tid];
  } else if (((fa | ta | n) & 3) == 0) {
    const uint32_t* __restrict__ f1 = reinterpret_cast<const uint32_t*>(from);
    uint32_t* __restrict__ t1 = reinterpret_cast<uint32_t*>(to);
    for (unsigned i = tid; i < (n >> 2); i += BCN_SNAP_NT) t1[i] = f1[i];
  } else {
    for (unsigned i = tid; i < n; i += BCN_SNAP_NT) to[i] = from[i];
  }
}

template <typename U>
__device__ __forceinline__ void snap_copy_unit(const char* from, char* to) {
  *reinterpret_cast<U*>(to) = *reinterpret_cast<const U*>(from);
}

template <bool LOAD>
__global__ __launch_bounds__(BCN_SNAP_NT) void snapshot_copy_k(SnapTable T, char* __restrict__ snap, const int32_t* __restrict__ src,
                                                               const uint8_t* __restrict__ mask) {
  const unsigned blk = blockIdx.x;
  int s = 0;
  while (s + 1 < T.nseg && blk >= T.seg[s + 1].blk0) s++;
  const SnapSeg g = T.seg[s];
  const unsigned lb = blk - g.blk0;
  const size_t row = g.row_bytes;
  if (g.bpr) {
    const unsigned b = lb / g.bpr, c = lb - b * g.bpr;
    if (b >= (unsigned)T.batch) return;
    unsigned sb = b;
    if (LOAD) {
      if (mask && !mask[b]) return;
      if (src) sb = (unsigned)src[b];
      if (sb >= (unsigned)T.n_src) return;   // negative indices wrap to large values: no address is formed from them
    }
    const unsigned lo = c * BCN_SNAP_TILE;
    if (lo >= g.row_bytes) return;
    const unsigned n = min(BCN_SNAP_TILE, g.row_bytes - lo);
    char* hrow = g.dev + (size_t)b * row + lo;
    char* srow = snap + g.snap_off + (size_t)sb * row + lo;
    if (LOAD) snap_copy_span(srow, hrow, n);
    else snap_copy_span(hrow, srow, n);
  } else {
    const unsigned upr = g.row_bytes / g.unit;
    const size_t total = (size_t)T.batch * upr;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const size_t e = ((size_t)lb * 4 + k) * BCN_SNAP_NT + threadIdx.x;
      if (e >= total) continue;
      const unsigned b = (unsigned)(e / upr), j = (unsigned)(e - (size_t)b * upr);
      unsigned sb = b;
      if (LOAD) {
        if (mask && !mask[b]) continue;
        if (src) sb = (unsigned)src[b];
        if (sb >= (unsigned)T.n_src) continue;
      }
      char* hp = g.dev + (size_t)b * row + (size_t)j * g.unit;
      char* sp = snap + g.snap_off + (size_t)sb * row + (size_t)j * g.unit;
      const char* from = LOAD ? sp : hp;
      char* to = LOAD ? hp : sp;
      if (g.unit == 16) snap_copy_unit<uint4>(from, to);
      else if (g.unit == 8) snap_copy_unit<uint2>(from, to);
      else if (g.unit == 4) snap_copy_unit<uint32_t>(from, to);
      else snap_copy_unit<uint8_t>(from, to);
    }
  }
}

}  // namespace

int snapshot_launch(const SnapTable& t, bool load, char* snap, const int32_t* src, const uint8_t* mask, hipStream_t s) {
  if (t.nblk == 0) return BCN_OK;
  if (load) hipLaunchKernelGGL(snapshot_copy_k<true>, dim3(t.nblk), dim3(BCN_SNAP_NT), 0, s, t, snap, src, mask);
  else hipLaunchKernelGGL(snapshot_copy_k<false>, dim3(t.nblk), dim3(BCN_SNAP_NT), 0, s, t, snap, src, mask);
  BCN_HIP(hipGetLastError());
  return BCN_OK;
}
