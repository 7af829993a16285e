// episode.hip -- the kernel behind bcn_episode_track (episode.h, include/beacon_hip.h): episode return / length bookkeeping and the
// rescue of terminal observations, ONE launch behind a step kernel, in front of the masked reset that overwrites the rows.
//
// Two roles selected from blockIdx, as in snapshot.hip:
//  * the first ceil(B / 256) workgroups keep the books, a lane per replica: every array is a [B] column, so consecutive lanes touch
//    consecutive addresses;
//  * the others copy obs rows of finished replicas into final_obs over the flattened [replica][unit] index space, a lane per unit of
//    16 / 8 / 4 bytes (the largest that divides a row), four units per lane: rayleigh's 384-real rows go as 16-byte units, lorenz's
//    24-byte float32 rows as 8-byte ones, and consecutive lanes touch consecutive addresses either way.
// The copy workgroups read done / trunc / mask themselves and never `finished`: nothing passes between workgroups of the launch.
// No atomics, no LDS, no scratch.  Batch totals are not reduced here: they are sums of the per-replica columns, taken at read time.
#include "episode.h"

namespace {

template <typename real>
__device__ __forceinline__ void episode_books(const EpisodeArgs& A, unsigned b, bool fin) {
  real* __restrict__ ret = static_cast<real*>(A.ret);
  real r = ret[b] + static_cast<const real*>(A.rwd)[b];
  int32_t l = A.len[b] + 1;
  if (fin) {
    static_cast<real*>(A.last_ret)[b] = r;
    A.last_len[b] = l;
    A.count[b] += 1;
    A.sum_ret[b] += (double)r;
    A.sum_len[b] += (long long)l;
    r = (real)0;
    l = 0;
  }
  ret[b] = r;
  A.len[b] = l;
}

template <typename U>
__device__ __forceinline__ void episode_copy_unit(const char* from, char* to) {
  *reinterpret_cast<U*>(to) = *reinterpret_cast<const U*>(from);
}

__global__ __launch_bounds__(BCN_EP_NT) void episode_track_k(EpisodeArgs A) {
  const unsigned blk = blockIdx.x;
  if (blk < A.nbk) {
    const unsigned b = blk * BCN_EP_NT + threadIdx.x;
    if (b >= A.batch) return;
    if (A.mask && !A.mask[b]) { A.finished[b] = 0; return; }   // a stale done byte of a replica that was not stepped starts no reset
    const bool fin = (A.done[b] | A.trunc[b]) != 0;
    if (A.f64) episode_books<double>(A, b, fin);
    else episode_books<float>(A, b, fin);
    A.finished[b] = fin ? 1 : 0;
    return;
  }
  const unsigned lb = blk - A.nbk;
#pragma unroll
  for (int k = 0; k < BCN_EP_UPL; k++) {
    const unsigned e = (lb * BCN_EP_UPL + k) * BCN_EP_NT + threadIdx.x;   // < total + BCN_EP_UPL * BCN_EP_NT <= 2^32 (checked by the caller)
    if (e >= A.total) continue;
    const unsigned b = e / A.upr;
    if (A.mask && !A.mask[b]) continue;
    if (!(A.done[b] | A.trunc[b])) continue;
    const size_t at = (size_t)e * A.unit;          // rows are contiguous: unit e of the flattened space sits at e * unit in both
    if (A.unit == 16) episode_copy_unit<uint4>(A.obs + at, A.final_obs + at);
    else if (A.unit == 8) episode_copy_unit<uint2>(A.obs + at, A.final_obs + at);
    else episode_copy_unit<uint32_t>(A.obs + at, A.final_obs + at);
  }
}

}  // namespace

int episode_launch(const EpisodeArgs& a, hipStream_t s) {
  const unsigned ncp = (a.total + BCN_EP_NT * BCN_EP_UPL - 1) / (BCN_EP_NT * BCN_EP_UPL);
  hipLaunchKernelGGL(episode_track_k, dim3(a.nbk + ncp), dim3(BCN_EP_NT), 0, s, a);
  BCN_HIP(hipGetLastError());
  return BCN_OK;
}
