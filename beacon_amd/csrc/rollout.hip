// rollout.hip -- the kernels behind bcn_rollout_begin / bcn_rollout_record / bcn_rollout_gae (rollout.h, include/beacon_hip.h):
// the transitions of T steps kept on the device, and generalised advantage estimation over them.
//
//  * rollout_record_k, ONE launch behind a step (behind the masked reset and the normalisation, when those run).  Two roles
//    selected from blockIdx, as in episode.hip: the first ceil(B / 256) workgroups write the [B] columns of slot t (rwd, status,
//    done, trunc, valid), a lane per replica; the others copy rows -- obs -> obs[t + 1], final_obs -> final_obs[t] where the replica
//    finished, the actions -> act[t], rwd_jets -> rwd_jets[t] -- over the flattened [replica][unit] space of each, a lane per unit of
//    16 / 8 / 4 bytes, four units per lane.  Every workgroup reads the slot t = cursor[0] itself and no lane of this launch writes
//    the cursor: a workgroup that starts late still finds the slot the early ones found.  t >= T: nothing is written.
//  * rollout_advance_k, one lane, enqueued behind it by the same entry point: cursor[0] = t + 1, or the overflow flag.
//  * rollout_begin_k: cursor = 0, overflow = 0, obs[0] <- the current observations.
//  * rollout_gae_k: a lane per column of [T][B cols], the serial backward recurrence over t in float64 whatever the env's dtype,
//    rounded once on store.  Consecutive lanes touch consecutive addresses of every plane.  The chain gae -> delta -> gae is four
//    dependent float64 operations per step; the loads do not depend on it, so those of BCN_RO_GAE_AHEAD steps are issued
//    before the first of them is used and the wave pays one memory latency per group, not per step.
// Nothing passes between workgroups of a launch.  No atomics, no LDS, no scratch: two runs agree bit for bit.
#include "rollout.h"

namespace {

template <typename U>
__device__ __forceinline__ void rollout_copy_unit(const char* from, char* to) {
  *reinterpret_cast<U*>(to) = from ? *reinterpret_cast<const U*>(from) : U{};
}

// units [lb * UPL * NT, (lb + 1) * UPL * NT) of job J into slot `slot` of its segment
__device__ __forceinline__ void rollout_copy(const RolloutJob& J, unsigned lb, unsigned long long slot, const uint8_t* mask,
                                             const uint8_t* finished) {
  char* dst = J.dst + slot * J.slot_bytes;       // 64-bit: a segment of 2^20 replicas x 128 steps passes 2^31 bytes
#pragma unroll
  for (int k = 0; k < BCN_RO_UPL; k++) {
    const unsigned e = (lb * BCN_RO_UPL + k) * BCN_RO_NT + threadIdx.x;   // < total + BCN_RO_UPL * BCN_RO_NT <= 2^32 (checked by the caller)
    if (e >= J.total) continue;
    const unsigned b = e / J.upr;
    if (J.when == RO_COPY_FINISHED && !finished[b]) continue;
    if (J.when == RO_COPY_STEPPED && mask && !mask[b]) continue;
    const size_t at = (size_t)e * J.unit;        // rows are contiguous: unit e of the flattened space sits at e * unit in both
    const char* from = J.src ? J.src + at : nullptr;
    if (J.unit == 16) rollout_copy_unit<uint4>(from, dst + at);
    else if (J.unit == 8) rollout_copy_unit<uint2>(from, dst + at);
    else rollout_copy_unit<uint32_t>(from, dst + at);
  }
}

__global__ __launch_bounds__(BCN_RO_NT) void rollout_record_k(RolloutRecordArgs A) {
  const int t = A.cursor[0];
  if (t < 0 || t >= A.T) return;                 // full: rollout_advance_k raises the flag
  const unsigned blk = blockIdx.x;
  if (blk < A.nbk) {
    const unsigned b = blk * BCN_RO_NT + threadIdx.x;
    if (b >= A.batch) return;
    const size_t at = (size_t)t * A.batch + b;
    const bool on = !A.mask || A.mask[b] != 0;
    if (A.f64) static_cast<double*>(A.d_rwd)[at] = on ? static_cast<const double*>(A.rwd)[b] : 0.0;
    else static_cast<float*>(A.d_rwd)[at] = on ? static_cast<const float*>(A.rwd)[b] : 0.0f;
    A.d_status[at] = A.status[b];
    A.d_done[at] = on ? A.done[b] : (uint8_t)0;
    A.d_trunc[at] = on ? A.trunc[b] : (uint8_t)0;
    A.d_valid[at] = on ? 1 : 0;
    return;
  }
  const unsigned lb = blk - A.nbk;
  // the last job that starts at or in front of this workgroup (uniform; the jobs that run have ascending blk0, and one that is off
  // carries blk0 = ncp, which no workgroup reaches)
  int j = 0;
#pragma unroll
  for (int k = 1; k < BCN_RO_NJOB; k++)
    if (lb >= A.job[k].blk0) j = k;
  if (j == 0) rollout_copy(A.job[0], lb - A.job[0].blk0, (unsigned long long)t + A.job[0].slot_off, A.mask, A.finished);
  else if (j == 1) rollout_copy(A.job[1], lb - A.job[1].blk0, (unsigned long long)t + A.job[1].slot_off, A.mask, A.finished);
  else if (j == 2) rollout_copy(A.job[2], lb - A.job[2].blk0, (unsigned long long)t + A.job[2].slot_off, A.mask, A.finished);
  else rollout_copy(A.job[3], lb - A.job[3].blk0, (unsigned long long)t + A.job[3].slot_off, A.mask, A.finished);
}

__global__ __launch_bounds__(64) void rollout_advance_k(int32_t* cursor, int T) {
  if (threadIdx.x != 0) return;
  const int t = cursor[0];
  if (t >= 0 && t < T) cursor[0] = t + 1;
  else cursor[1] = 1;
}

__global__ __launch_bounds__(BCN_RO_NT) void rollout_begin_k(int32_t* cursor, RolloutJob J) {
  if (blockIdx.x == 0 && threadIdx.x < 4) cursor[threadIdx.x] = 0;
  rollout_copy(J, blockIdx.x, 0ull, nullptr, nullptr);
}

// what one step of the recurrence reads
struct GaeIn { double rwd, val, boot; bool fin, valid; };

template <typename real, bool FV>
__device__ __forceinline__ GaeIn gae_load(const RolloutGaeArgs& A, int t, unsigned c, unsigned b) {
  const size_t at = (size_t)t * A.ncols + c, fl = (size_t)t * A.batch + b;
  GaeIn in;
  const uint8_t done = A.done[fl], trunc = A.trunc[fl];
  in.valid = A.valid[fl] != 0;
  in.fin = (done | trunc) != 0;
  in.rwd = (double)static_cast<const real*>(A.rwd)[at];
  in.val = (double)static_cast<const real*>(A.values)[at];
  // only rows where trunc is set are used: the others may hold anything, and a select drops them.  The load itself is conditional
  // on nothing (FV: final_values are given, decided at the launch): behind a branch it would be waited for on the spot, and
  // behind the flag it would cost one more memory latency per step
  in.boot = 0.0;
  if (FV) {
    const double fv = (double)static_cast<const real*>(A.final_values)[at];
    in.boot = trunc ? fv : 0.0;
  }
  return in;
}

template <typename real>
__device__ __forceinline__ void gae_step(const RolloutGaeArgs& A, const GaeIn& in, int t, unsigned c, double& nv, double& gae) {
  const size_t at = (size_t)t * A.ncols + c;
  real* __restrict__ adv = static_cast<real*>(A.adv);
  real* __restrict__ ret = static_cast<real*>(A.ret);
  if (!in.valid) {                               // a skipped step is transparent: nv and gae pass through
    adv[at] = (real)0;
    ret[at] = (real)in.val;
    return;
  }
  const double delta = in.rwd + A.gamma * (in.fin ? in.boot : nv) - in.val;
  gae = delta + (in.fin ? 0.0 : A.gamma * A.lam * gae);
  adv[at] = (real)gae;
  ret[at] = (real)(gae + in.val);
  nv = in.val;
}

template <typename real, bool FV>
__global__ __launch_bounds__(BCN_RO_NT) void rollout_gae_k(RolloutGaeArgs A) {
  const unsigned c = blockIdx.x * BCN_RO_NT + threadIdx.x;
  if (c >= A.ncols) return;
  const unsigned b = c / A.cols;
  int n = A.cursor[0];
  n = n < 0 ? 0 : (n > A.T ? A.T : n);
  double nv = (double)static_cast<const real*>(A.last_value)[c], gae = 0.0;
  int t = n - 1;
  for (; t >= BCN_RO_GAE_AHEAD - 1; t -= BCN_RO_GAE_AHEAD) {
    GaeIn in[BCN_RO_GAE_AHEAD];
#pragma unroll
    for (int k = 0; k < BCN_RO_GAE_AHEAD; k++) in[k] = gae_load<real, FV>(A, t - k, c, b);
#pragma unroll
    for (int k = 0; k < BCN_RO_GAE_AHEAD; k++) gae_step<real>(A, in[k], t - k, c, nv, gae);
  }
  for (; t >= 0; t--) gae_step<real>(A, gae_load<real, FV>(A, t, c, b), t, c, nv, gae);
}

}  // namespace

int rollout_begin_launch(int32_t* cursor, const RolloutJob& obs, hipStream_t s) {
  const unsigned ncp = (obs.total + BCN_RO_NT * BCN_RO_UPL - 1) / (BCN_RO_NT * BCN_RO_UPL);
  hipLaunchKernelGGL(rollout_begin_k, dim3(ncp), dim3(BCN_RO_NT), 0, s, cursor, obs);
  BCN_HIP(hipGetLastError());
  return BCN_OK;
}

int rollout_record_launch(const RolloutRecordArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(rollout_record_k, dim3(a.nbk + a.ncp), dim3(BCN_RO_NT), 0, s, a);
  BCN_HIP(hipGetLastError());
  hipLaunchKernelGGL(rollout_advance_k, dim3(1), dim3(64), 0, s, a.cursor, a.T);
  BCN_HIP(hipGetLastError());
  return BCN_OK;
}

int rollout_gae_launch(const RolloutGaeArgs& a, hipStream_t s) {
  const dim3 grid((a.ncols + BCN_RO_NT - 1) / BCN_RO_NT);
  const dim3 nt(BCN_RO_NT);
  if (a.f64 && a.final_values) hipLaunchKernelGGL((rollout_gae_k<double, true>), grid, nt, 0, s, a);
  else if (a.f64) hipLaunchKernelGGL((rollout_gae_k<double, false>), grid, nt, 0, s, a);
  else if (a.final_values) hipLaunchKernelGGL((rollout_gae_k<float, true>), grid, nt, 0, s, a);
  else hipLaunchKernelGGL((rollout_gae_k<float, false>), grid, nt, 0, s, a);
  BCN_HIP(hipGetLastError());
  return BCN_OK;
}
