// shkadov_jets.hip -- the kernel behind bcn_shkadov_jet_rewards (shkadov_jets.h, include/beacon_hip.h): the reward of every jet
// of every replica (shkadov_separable.get_rwd, shkadov.py:469-481, with the blow-up rule of :441-445) and, optionally, per-jet
// episode returns, ONE launch behind shkadov_step_k and in front of episode_track_k and the masked reset that overwrites the film.
//
// One wavefront per (replica, jet) pair, four pairs per 256-thread workgroup; a trailing wavefront without a pair returns.  The
// lanes read the l_rwd cells downstream of the jet lane-strided (consecutive lanes, consecutive addresses; one loop trip at the
// reference's l_rwd = 50), the wavefront reduces with wave_sum and lane 0 writes the result and keeps the books.  Nothing passes
// between wavefronts: no LDS, no barrier, no atomics, so the summation order is fixed and two runs agree bit for bit.  The blow-up
// bit, done and trunc are the step's own (its packed outputs): the film is not scanned again.
#include "shkadov_jets.h"

namespace {

template <typename real>
__global__ __launch_bounds__(BCN_JETS_NT) void shkadov_jets_k(ShkadovJetsArgs<real> A) {
  const unsigned pair = blockIdx.x * BCN_JETS_PAIRS + threadIdx.x / BCN_WAVE;
  const int lane = threadIdx.x & (BCN_WAVE - 1);
  if (pair >= A.npairs) return;
  const unsigned b = pair / (unsigned)A.n_jets;
  const int j = (int)(pair - b * (unsigned)A.n_jets);
  if (A.mask && !A.mask[b]) return;              // a replica that was not stepped keeps its rows
  real r;
  if (A.status[b] & BCN_ST_BLOWUP) {             // (uniform over the wavefront: one replica)
    r = A.blowup_rwd;                            // shkadov.py:441-445: whichever jet asks
  } else {
    const int s = A.jet_pos + j * A.jet_space;   // shkadov.py:475
    const real* __restrict__ gh = A.h + (size_t)b * A.n + s;
    real loc = 0;
    for (int m = lane; m < A.l_rwd; m += BCN_WAVE) {
      if (s + m >= A.nx) continue;
      const real d = gh[m] - real(1);
      loc += d * d;
    }
    r = -(wave_sum(loc) * A.dx) / (real)(A.n_jets * A.l_rwd);   // :478-479
  }
  if (lane != 0) return;
  A.rwd_jets[pair] = r;
  if (!A.ret) return;
  // the semantics of episode.hip, per jet: one add in the env's dtype, and the finished return moves on where done | trunc
  real acc = A.ret[pair] + r;
  if ((A.done[b] | A.trunc[b]) != 0) {
    A.last_ret[pair] = acc;
    A.sum_ret[pair] += (double)acc;
    acc = (real)0;
  }
  A.ret[pair] = acc;
}

}  // namespace

template <typename real>
int shkadov_jets_launch(const ShkadovJetsArgs<real>& a, hipStream_t s) {
  const unsigned nblk = (a.npairs + BCN_JETS_PAIRS - 1) / BCN_JETS_PAIRS;
  hipLaunchKernelGGL(shkadov_jets_k<real>, dim3(nblk), dim3(BCN_JETS_NT), 0, s, a);
  BCN_HIP(hipGetLastError());
  return BCN_OK;
}

template int shkadov_jets_launch<float>(const ShkadovJetsArgs<float>&, hipStream_t);
template int shkadov_jets_launch<double>(const ShkadovJetsArgs<double>&, hipStream_t);
