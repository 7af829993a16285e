// shkadov_jets.h -- argument block of the per-jet reward kernel of shkadov (shkadov_jets.hip; include/beacon_hip.h:
// bcn_shkadov_jet_rewards), the batched form of shkadov_separable.get_rwd (shkadov.py:469-481).
//
// One packed per-jet buffer of the caller holds, for the handle's B replicas of n_jets jets, four segments (every start a multiple
// of 16 bytes), each [B][n_jets]:
//   rwd_jets real      the reward of every jet after the step just taken
//   ret real           the running return of every jet in the episode in progress
//   last_ret real      that of the replica's last finished episode
//   sum_ret float64    the sum of the finished returns
// The kernel reads the film h of the handle and status / done / trunc of the step's packed outputs [obs | rwd | status | done | trunc].
#pragma once
#include "bcn_common.h"
#include "snapshot.h"

#define BCN_JETS_NT 256                          // threads per workgroup
#define BCN_JETS_PAIRS (BCN_JETS_NT / BCN_WAVE)  // (replica, jet) pairs per workgroup: one wavefront each
#define BCN_JETS_NSEG 4

// The segments in buffer order: the host addresses them by these names, never by number.
enum { JETS_RWD_JETS, JETS_RET, JETS_LAST_RET, JETS_SUM_RET, JETS_NSEG_ };
static_assert(JETS_NSEG_ == BCN_JETS_NSEG, "shkadov_jets.h: the enum and BCN_JETS_NSEG disagree");
inline void jets_segs(size_t n_jets, SegDesc* d) {
  d[JETS_RWD_JETS] = {"rwd_jets", BCN_SNAP_REAL, 1, n_jets}; d[JETS_RET] = {"ret", BCN_SNAP_REAL, 1, n_jets};
  d[JETS_LAST_RET] = {"last_ret", BCN_SNAP_REAL, 1, n_jets}; d[JETS_SUM_RET] = {"sum_ret", BCN_SNAP_F64, 1, n_jets};
}

template <typename real>
struct ShkadovJetsArgs {
  const real* h;                  // the film, [B][n]
  // the step's outputs
  const int32_t* status;
  const uint8_t* done;
  const uint8_t* trunc;
  const uint8_t* mask;            // the handle's replica mask (bcn_set_mask); NULL: every replica
  // the per-jet buffer
  real* rwd_jets;
  real* ret;                      // NULL: no statistics (last_ret and sum_ret are then not touched either)
  real* last_ret;
  double* sum_ret;
  unsigned npairs;                // batch * n_jets
  int n, nx;                      // row length of h; cells of the film
  int n_jets, jet_pos, jet_space, l_rwd;
  real dx, blowup_rwd;
};

template <typename real>
int shkadov_jets_launch(const ShkadovJetsArgs<real>& a, hipStream_t s);
